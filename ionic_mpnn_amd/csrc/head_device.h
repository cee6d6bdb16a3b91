// Device arithmetic of the model head after GlobalSumPool (f1), shared by the kernels of model_head.hip (one launch
// per pair list: the inference forward, the training forward and the backward) and the grid kernels (head_grid.hip:
// per-ion mixing rows, then every cation x anion pair; transfer_grid.hip).  One definition of every rounding step, so a
// pair gives the same bits whichever kernel evaluates it.
#pragma once

#include <hip/hip_runtime.h>

namespace impnn {

// Two softplus forms that round differently, so neither may stand in for the other.  _exact: the inference head
// (impnn_model_head) and the grid (impnn_head_grid), bit-equal to each other.  _stable: the tensor-table forward
// (impnn_model_head_tensors, _loss) and the backward (impnn_model_head_bwd, _loss_bwd), which recomputes that forward.
__device__ __forceinline__ float softplus_exact(float x) { return x > 20.f ? x + log1pf(expf(-x)) : log1pf(expf(x)); }
__device__ __forceinline__ float softplus_stable(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// A Dense output: the bias first, then the inputs in ascending order, one fmaf each.  w[i * stride] is the kernel
// entry of input i for this output.
__device__ __forceinline__ float head_chain(const float* x, const float* w, int stride, int n, float bias) {
  float acc = bias;
  for (int i = 0; i < n; ++i) acc = fmaf(x[i], w[i * stride], acc);
  return acc;
}

// relu as keras computes it: a NaN stays a NaN (fmaxf(NaN, 0) is 0), -0 and every negative value give +0.  Equal to
// 0.f + fmaxf(x, 0.f) for every x that is not a NaN.
__device__ __forceinline__ float head_relu(float x) { return !(x <= 0.f) ? x : 0.f; }

// The viscosity tail of one pair (train_viscosity.py:204-214, models/layers.py:10-49): vp = Dense(3)(mixed).
struct VftParams {
  float A, Bc, Cc;
};

__device__ __forceinline__ VftParams head_vft_params(float vp0, float vp1, float vp2) {
  return VftParams{vp0, fminf(fmaxf(softplus_exact(vp1), 0.f), 20.f), fminf(fmaxf(softplus_exact(vp2), 0.1f), 50.f)};
}

__device__ __forceinline__ float head_scaled_t(float T) { return T / 100.0f; }  // ScaleTemperature

__device__ __forceinline__ float head_vft_eval(const VftParams& p, float t100) {
  return p.A + p.Bc / (t100 + p.Cc + 1e-6f);  // ComputeLogEta
}

}  // namespace impnn
