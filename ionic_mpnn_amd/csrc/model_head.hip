// f1  The model head: everything after GlobalSumPool, one launch (train_viscosity.py:189,197-214 +
// models/layers.py:10-49; train_melting_point.py:173,191-198), behind impnn_model_head, _tensors, _bwd, _loss, _loss_bwd
// and impnn_weighted_model_head_loss[_bwd] (the loss with per-sample weights).
//   fp_g  = relu(pooled_g @ Wfp_g + bfp_g)         (D -> F)     g in {cat, an}
//   mixed = relu(fp_cat @ Wp_cat + bp_cat) + relu(fp_an @ Wp_an + bp_an)      (F -> Mx)
//   kind 0: vp = mixed @ Wv + bv (Mx -> 3); A = vp0; Bc = clip(softplus(vp1), 0, 20);
//           Cc = clip(softplus(vp2), 0.1, 50); out = A + Bc / (T/100 + Cc + 1e-6)
//   kind 1: out = relu(mixed @ Wh + bh) @ Wo + bo   (Mx -> F -> 1)
// Three kernels: the inference forward from the packed weights, the training forward from the individual weight tensors
// (with the loss) and the backward; kHeadMaxX / kHeadMaxDim (common.h) are their LDS row strides as well as their
// limits.  api.hip checks a ModelHeadCall's arguments (model_head_checked); the launchers below judge the widths, the
// pointer tables and the LDS fit, in that order.  The grid forms are in head_grid.hip, the rounding steps they share
// with the inference forward in head_device.h.
#include "common.h"
#include "head_device.h"

namespace impnn {
namespace {

// 8 samples per 256-thread workgroup, 32 threads per sample: thread (s, jj) owns outputs jj, jj+32 of
// every layer; the sample's vectors and all weights sit in LDS (13.6 KB of weights at the defaults).
constexpr int kHeadSPB = 8;

__global__ __launch_bounds__(256) void model_head_kernel(int kind, const float* __restrict__ pc,
                                                         const float* __restrict__ pa, const float* __restrict__ T,
                                                         const float* __restrict__ w, float* __restrict__ out, int B, int D,
                                                         int F, int Mx, int wfloats) {
  extern __shared__ __align__(16) float hsm[];
  float* ws = hsm;                                   // all head weights
  float* xs = ws + ((wfloats + 3) & ~3);             // [kHeadSPB][2][kHeadMaxX] pooled rows
  float* fp = xs + kHeadSPB * 2 * kHeadMaxX;         // [kHeadSPB][2][kHeadMaxDim]
  float* mix = fp + kHeadSPB * 2 * kHeadMaxDim;      // [kHeadSPB][kHeadMaxDim]
  float* hid = mix + kHeadSPB * kHeadMaxDim;         // [kHeadSPB][kHeadMaxDim]
  const int tid = threadIdx.x, sl = tid >> 5, jj = tid & 31;
  const int b = blockIdx.x * kHeadSPB + sl;
  const bool live = b < B;
  for (int t = tid; t < wfloats; t += blockDim.x) ws[t] = w[t];
  for (int g = 0; g < 2; ++g)
    for (int i = jj; i < D; i += 32) xs[(sl * 2 + g) * kHeadMaxX + i] = live ? (g == 0 ? pc : pa)[(int64_t)b * D + i] : 0.f;
  __syncthreads();
  const float* Wfp[2] = {ws, ws + D * F + F};
  const float* wp = ws + 2 * (D * F + F);
  const float* Wp[2] = {wp, wp + F * Mx + Mx};
  const float* wt = wp + 2 * (F * Mx + Mx);
  for (int g = 0; g < 2; ++g)
    for (int j = jj; j < F; j += 32) {
      float acc = Wfp[g][D * F + j];
      const float* x = xs + (sl * 2 + g) * kHeadMaxX;
      for (int i = 0; i < D; ++i) acc = fmaf(x[i], Wfp[g][i * F + j], acc);
      fp[(sl * 2 + g) * kHeadMaxDim + j] = fmaxf(acc, 0.f);
    }
  __syncthreads();
  for (int j = jj; j < Mx; j += 32) {
    float m = 0.f;
    for (int g = 0; g < 2; ++g) {
      float acc = Wp[g][F * Mx + j];
      const float* x = fp + (sl * 2 + g) * kHeadMaxDim;
      for (int i = 0; i < F; ++i) acc = fmaf(x[i], Wp[g][i * Mx + j], acc);
      m += fmaxf(acc, 0.f);  // AddTwoTensors / keras Add
    }
    mix[sl * kHeadMaxDim + j] = m;
  }
  __syncthreads();
  const float* mx = mix + sl * kHeadMaxDim;
  if (kind == 0) {
    if (jj < 3) {
      float acc = wt[Mx * 3 + jj];
      for (int i = 0; i < Mx; ++i) acc = fmaf(mx[i], wt[i * 3 + jj], acc);
      hid[sl * kHeadMaxDim + jj] = acc;
    }
    __syncthreads();
    if (jj == 0 && live) {
      const float* vp = hid + sl * kHeadMaxDim;
      out[b] = head_vft_eval(head_vft_params(vp[0], vp[1], vp[2]), head_scaled_t(T[b]));  // head_device.h
    }
  } else {
    const float* Wh = wt;
    const float* bh = Wh + Mx * F;
    const float* Wo = bh + F;
    for (int j = jj; j < F; j += 32) {
      float acc = bh[j];
      for (int i = 0; i < Mx; ++i) acc = fmaf(mx[i], Wh[i * F + j], acc);
      hid[sl * kHeadMaxDim + j] = fmaxf(acc, 0.f);
    }
    __syncthreads();
    if (jj == 0 && live) {
      float acc = Wo[F];
      for (int j = 0; j < F; ++j) acc = fmaf(hid[sl * kHeadMaxDim + j], Wo[j], acc);
      out[b] = acc;
    }
  }
}

// ---- f1 for training: the forward from the individual weight tensors (no packing) and its backward, one launch each.
// Tensor order = the packed order of impnn_model_head:
//   Wfp_cat | bfp_cat | Wfp_an | bfp_an | Wp_cat | bp_cat | Wp_an | bp_an | kind 0: Wv | bv ; kind 1: Wh | bh | Wo | bo
// Backward: 8 samples per workgroup, 32 threads per sample; the forward is recomputed; parameter gradients are
// summed in LDS per workgroup and ADDED to the individual gradient buffers with float atomics.
constexpr int kHeadTensors = 12;
struct HeadTensors {
  const float* w[kHeadTensors];
  float* g[kHeadTensors];
  int off[kHeadTensors + 1];
  int n;
  float l2[kHeadTensors];  // keras l2(lambda) per tensor (0: none); used by the loss entries only
};
// loss = mean_b (pred_b - y_b)^2 + sum_t l2_t * sum(W_t^2)   (keras "mse" + kernel_regularizer, train_viscosity.py:189,229)
struct HeadLoss {
  const float* y;        // (B); null: the kernels behave as the plain head entries
  const float* dloss;    // backward: device scalar, the gradient of the loss value
  float* loss_out;       // forward: device scalar
  float* partial;        // forward: one squared-error sum per workgroup
  unsigned int* counter; // forward: arrival ticket, zero before the first call, left at zero by every call
  float inv_B;
};
// With sample weights (keras sum_over_batch_size): (1/B) sum_b w_b (pred_b - y_b)^2 + the same penalties; B counts the
// samples of weight 0 too.  The weights are an argument of the weighted kernel instances alone: a call without them
// launches the instances whose argument block is the unweighted loss's, with no weight instruction and no multiply by 1.
template <bool kWeighted>
struct HeadLossArg : HeadLoss {};
template <>
struct HeadLossArg<true> : HeadLoss {
  const float* w;  // (B) sample weights, read for live samples only
};
__device__ __forceinline__ float head_l2(const HeadTensors& ht, int sgm) {
  float v = ht.l2[0];
#pragma unroll
  for (int q = 1; q < kHeadTensors; ++q) v = sgm == q ? ht.l2[q] : v;
  return v;
}
// deterministic workgroup sum of one value per thread (256 threads); result valid in every thread
__device__ __forceinline__ float head_block_sum(float v, float* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ int head_total(const HeadTensors& ht) {
  int tot = ht.off[1];
#pragma unroll
  for (int q = 2; q <= kHeadTensors; ++q) tot = ht.n == q ? ht.off[q] : tot;
  return tot;
}
// segment of packed index t.  Constant indices only: the table is a kernel argument, a dynamic index into it would
// be a dependent load from the kernarg segment per probe.
__device__ __forceinline__ int head_segment(const HeadTensors& ht, int t, int* base) {
  int sgm = 0, b = 0;
#pragma unroll
  for (int q = 1; q < kHeadTensors; ++q)
    if (q < ht.n && t >= ht.off[q]) sgm = q, b = ht.off[q];
  *base = b;
  return sgm;
}
__device__ __forceinline__ const float* head_wptr(const HeadTensors& ht, int sgm) {
  const float* p = ht.w[0];
#pragma unroll
  for (int q = 1; q < kHeadTensors; ++q) p = sgm == q ? ht.w[q] : p;
  return p;
}
__device__ __forceinline__ float* head_gptr(const HeadTensors& ht, int sgm) {
  float* p = ht.g[0];
#pragma unroll
  for (int q = 1; q < kHeadTensors; ++q) p = sgm == q ? ht.g[q] : p;
  return p;
}

__device__ __forceinline__ void head_load_weights(const HeadTensors& ht, float* ws) {
  const int total = head_total(ht);
  constexpr int kU = 8;  // independent loads in flight per thread
  for (int t0 = threadIdx.x; t0 < total; t0 += blockDim.x * kU) {
    float v[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int t = t0 + u * blockDim.x;
      int base;
      const int sgm = head_segment(ht, t, &base);
      v[u] = t < total ? head_wptr(ht, sgm)[t - base] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int t = t0 + u * blockDim.x;
      if (t < total) ws[t] = v[u];
    }
  }
}

// forward up to the mixed vector; returns through LDS: fpre (pre-activation of the fingerprint Dense), fp, ppre, mix
__device__ __forceinline__ void head_forward_mix(const float* ws, const float* xs, float* fpre, float* ppre, float* mix,
                                                 int sl, int jj, int D, int F, int Mx) {
  const float* Wfp[2] = {ws, ws + D * F + F};
  const float* wp = ws + 2 * (D * F + F);
  const float* Wp[2] = {wp, wp + F * Mx + Mx};
  for (int g = 0; g < 2; ++g)
    for (int j = jj; j < F; j += 32) {
      float acc = Wfp[g][D * F + j];
      const float* x = xs + (sl * 2 + g) * kHeadMaxX;
      for (int i = 0; i < D; ++i) acc = fmaf(x[i], Wfp[g][i * F + j], acc);
      fpre[(sl * 2 + g) * kHeadMaxDim + j] = acc;
    }
  __syncthreads();
  for (int j = jj; j < Mx; j += 32) {
    float m = 0.f;
    for (int g = 0; g < 2; ++g) {
      float acc = Wp[g][F * Mx + j];
      const float* x = fpre + (sl * 2 + g) * kHeadMaxDim;
      for (int i = 0; i < F; ++i) acc = fmaf(fmaxf(x[i], 0.f), Wp[g][i * Mx + j], acc);
      ppre[(sl * 2 + g) * kHeadMaxDim + j] = acc;
      m += fmaxf(acc, 0.f);
    }
    mix[sl * kHeadMaxDim + j] = m;
  }
  __syncthreads();
}

// kWeighted: a loss call with sample weights (hl.y and hl.w set); the other instance has no trace of them
template <bool kWeighted>
__global__ __launch_bounds__(256) void model_head_tensors_kernel(int kind, const float* __restrict__ pc,
                                                                 const float* __restrict__ pa,
                                                                 const float* __restrict__ T, HeadTensors ht,
                                                                 float* __restrict__ out, int B, int D, int F, int Mx,
                                                                 HeadLossArg<kWeighted> hl) {
  extern __shared__ __align__(16) float hsm[];
  __shared__ float red[256];
  __shared__ float sq[kHeadSPB];
  __shared__ int is_last;
  const int total = head_total(ht);
  float* ws = hsm;
  float* xs = ws + ((total + 3) & ~3);
  float* fpre = xs + kHeadSPB * 2 * kHeadMaxX;
  float* ppre = fpre + kHeadSPB * 2 * kHeadMaxDim;
  float* mix = ppre + kHeadSPB * 2 * kHeadMaxDim;
  float* hid = mix + kHeadSPB * kHeadMaxDim;
  const int tid = threadIdx.x, sl = tid >> 5, jj = tid & 31;
  const int b = blockIdx.x * kHeadSPB + sl;
  const bool live = b < B;
  head_load_weights(ht, ws);
  for (int g = 0; g < 2; ++g)
    for (int i = jj; i < D; i += 32) xs[(sl * 2 + g) * kHeadMaxX + i] = live ? (g == 0 ? pc : pa)[(int64_t)b * D + i] : 0.f;
  __syncthreads();
  head_forward_mix(ws, xs, fpre, ppre, mix, sl, jj, D, F, Mx);
  const float* wt = ws + 2 * (D * F + F) + 2 * (F * Mx + Mx);
  const float* mx = mix + sl * kHeadMaxDim;
  if (kind == 0) {
    if (jj < 3) {
      float acc = wt[Mx * 3 + jj];
      for (int i = 0; i < Mx; ++i) acc = fmaf(mx[i], wt[i * 3 + jj], acc);
      hid[sl * kHeadMaxDim + jj] = acc;
    }
    __syncthreads();
    if (jj == 0) {
      float pred = 0.f;
      if (live) {
        const float* vp = hid + sl * kHeadMaxDim;
        const float Bc = fminf(fmaxf(softplus_stable(vp[1]), 0.f), 20.f);
        const float Cc = fminf(fmaxf(softplus_stable(vp[2]), 0.1f), 50.f);
        pred = vp[0] + Bc / (T[b] / 100.0f + Cc + 1e-6f);
        if (out) out[b] = pred;
      }
      if constexpr (kWeighted)
        sq[sl] = live ? hl.w[b] * ((pred - hl.y[b]) * (pred - hl.y[b])) : 0.f;
      else if (hl.y)
        sq[sl] = live ? (pred - hl.y[b]) * (pred - hl.y[b]) : 0.f;
    }
  } else {
    const float* Wh = wt;
    const float* bh = Wh + Mx * F;
    const float* Wo = bh + F;
    for (int j = jj; j < F; j += 32) {
      float acc = bh[j];
      for (int i = 0; i < Mx; ++i) acc = fmaf(mx[i], Wh[i * F + j], acc);
      hid[sl * kHeadMaxDim + j] = fmaxf(acc, 0.f);
    }
    __syncthreads();
    if (jj == 0) {
      float acc = Wo[F];
      for (int j = 0; j < F; ++j) acc = fmaf(hid[sl * kHeadMaxDim + j], Wo[j], acc);
      if (live && out) out[b] = acc;
      if constexpr (kWeighted)
        sq[sl] = live ? hl.w[b] * ((acc - hl.y[b]) * (acc - hl.y[b])) : 0.f;
      else if (hl.y)
        sq[sl] = live ? (acc - hl.y[b]) * (acc - hl.y[b]) : 0.f;
    }
  }
  if (!hl.y) return;
  // ---- loss: workgroup sums in sample order, then the LAST workgroup to arrive adds them in workgroup order
  __syncthreads();
  if (tid == 0) {
    float sum = 0.f;
    for (int q = 0; q < kHeadSPB; ++q) sum += sq[q];
    __hip_atomic_store(&hl.partial[blockIdx.x], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    const unsigned int ticket = atomicAdd(hl.counter, 1u);
    is_last = ticket == gridDim.x - 1;
  }
  __syncthreads();
  if (!is_last) return;
  __threadfence();
  float v = 0.f;
  for (int i = tid; i < (int)gridDim.x; i += 256)
    v += __hip_atomic_load(&hl.partial[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const float se = head_block_sum(v, red);
  float reg = 0.f;
  for (int t = tid; t < total; t += 256) {
    int base;
    const float lam = head_l2(ht, head_segment(ht, t, &base));
    reg = fmaf(lam * ws[t], ws[t], reg);
  }
  reg = head_block_sum(reg, red);
  if (tid == 0) {
    hl.loss_out[0] = se * hl.inv_B + reg;
    *hl.counter = 0u;
  }
}

// per-sample vectors of the backward, kHeadMaxDim floats each, in LDS: the parameter gradients are outer products of these
enum { kVX0, kVX1, kVFp0, kVFp1, kVDfp0, kVDfp1, kVDpr0, kVDpr1, kVMix, kVTop, kVHid, kVOne, kHdVecs };
constexpr int kHdVecStride = 2 * kHeadMaxX + (kHdVecs - 2) * kHeadMaxDim;
__device__ __forceinline__ int head_vec_off(int which) {
  return which < 2 ? which * kHeadMaxX : 2 * kHeadMaxX + (which - 2) * kHeadMaxDim;
}

// 1024 threads: the first 256 walk the samples (8 samples x 32 lanes, as the forward kernel), all of them stage the
// weights, form the parameter gradients' outer products and flush them - the three phases that scale with the packed
// weight count (25 K floats at atom_dim 128) and made the kernel ~96 us at every batch below 2048, alone on the stream
// between the two halves of a training step.
template <bool kWeighted>
__global__ __launch_bounds__(1024) void model_head_bwd_kernel(int kind, const float* __restrict__ pc,
                                                             const float* __restrict__ pa, const float* __restrict__ T,
                                                             HeadTensors ht, const float* __restrict__ dout,
                                                             float* __restrict__ dpc, float* __restrict__ dpa, int B,
                                                             int D, int F, int Mx, HeadLossArg<kWeighted> hl) {
  extern __shared__ __align__(16) float hsm[];
  const int total = head_total(ht);
  const int tpad = (total + 3) & ~3;
  float* ws = hsm;
  float* dws = ws + tpad;  // parameter-gradient sums of this workgroup; element t is owned by thread t % 256
  float* vec = dws + tpad;  // [kHeadSPB][kHdVecStride]: the two pooled states (kHeadMaxX each), then 10 vectors of kHeadMaxDim
  float* fpre = vec + kHeadSPB * kHdVecStride;
  float* ppre = fpre + kHeadSPB * 2 * kHeadMaxDim;
  const int tid = threadIdx.x;
  const bool worker = tid < 32 * kHeadSPB;                     // a lane of a sample; the others skip the per-sample loops
  const int sl = worker ? tid >> 5 : 0, jj = worker ? (tid & 31) : (1 << 30);
  float* my = vec + sl * kHdVecStride;
  auto V = [&](int which) { return my + head_vec_off(which); };
  head_load_weights(ht, ws);
  for (int t = tid; t < tpad; t += blockDim.x) dws[t] = 0.f;
  const int o_fp[2] = {0, D * F + F};
  const int o_p0 = 2 * (D * F + F);
  const int o_p[2] = {o_p0, o_p0 + F * Mx + Mx};
  const int o_t = o_p0 + 2 * (F * Mx + Mx);

  for (int b0 = blockIdx.x * kHeadSPB; b0 < B; b0 += gridDim.x * kHeadSPB) {
    const int b = b0 + sl;
    const bool live = worker && b < B;
    __syncthreads();  // the previous group's outer products are done with vec
    // xs of head_forward_mix = vectors kVX0,kVX1 (contiguous)
    for (int g = 0; g < 2; ++g)
      for (int i = jj; i < D; i += 32) V(kVX0 + g)[i] = live ? (g == 0 ? pc : pa)[(int64_t)b * D + i] : 0.f;
    __syncthreads();
    {  // forward (same arithmetic as head_forward_mix, on this kernel's vector layout)
      for (int g = 0; g < 2; ++g)
        for (int j = jj; j < F; j += 32) {
          float acc = ws[o_fp[g] + D * F + j];
          const float* x = V(kVX0 + g);
          for (int i = 0; i < D; ++i) acc = fmaf(x[i], ws[o_fp[g] + i * F + j], acc);
          fpre[(sl * 2 + g) * kHeadMaxDim + j] = acc;
          V(kVFp0 + g)[j] = fmaxf(acc, 0.f);
        }
      __syncthreads();
      for (int j = jj; j < Mx; j += 32) {
        float m = 0.f;
        for (int g = 0; g < 2; ++g) {
          float acc = ws[o_p[g] + F * Mx + j];
          const float* x = V(kVFp0 + g);
          for (int i = 0; i < F; ++i) acc = fmaf(x[i], ws[o_p[g] + i * Mx + j], acc);
          ppre[(sl * 2 + g) * kHeadMaxDim + j] = acc;
          m += fmaxf(acc, 0.f);
        }
        V(kVMix)[j] = m;
      }
      __syncthreads();
    }
    const float* mx = V(kVMix);
    // gradient of the prediction: given (plain head), or 2 (pred - y) / B * dloss once pred is known (loss entries),
    // times the sample's weight where the call has weights
    float gscale = hl.y ? 2.0f * hl.inv_B * hl.dloss[0] : 0.f;
    if constexpr (kWeighted) gscale = live ? gscale * hl.w[b] : 0.f;
    float d = (live && !hl.y) ? dout[b] : 0.f;
    float* top = V(kVTop);
    // ---- top of the head: kVTop = gradient of [A,b,c] (kind 0) / of the hidden pre-activation (kind 1)
    if (kind == 0) {
      if (jj < 3) {
        float acc = ws[o_t + Mx * 3 + jj];
        for (int i = 0; i < Mx; ++i) acc = fmaf(mx[i], ws[o_t + i * 3 + jj], acc);
        V(kVHid)[jj] = acc;
      }
      __syncthreads();
      const float* vp = V(kVHid);
      const float sp1 = softplus_stable(vp[1]), sp2 = softplus_stable(vp[2]);
      const float Bc = fminf(fmaxf(sp1, 0.f), 20.f), Cc = fminf(fmaxf(sp2, 0.1f), 50.f);
      const float den = (live ? T[b] : 300.f) / 100.0f + Cc + 1e-6f;
      if (hl.y && live) d = gscale * (vp[0] + Bc / den - hl.y[b]);
      if (jj == 0) V(kVOne)[0] = d;
      float dvp[3];
      dvp[0] = d;
      dvp[1] = (sp1 >= 0.f && sp1 <= 20.f) ? d / den / (1.0f + expf(-vp[1])) : 0.f;  // clamp passes inside [min,max]
      dvp[2] = (sp2 >= 0.1f && sp2 <= 50.f) ? -d * Bc / (den * den) / (1.0f + expf(-vp[2])) : 0.f;
      if (jj < 3) top[jj] = jj == 0 ? dvp[0] : (jj == 1 ? dvp[1] : dvp[2]);
      for (int i = jj; i < Mx; i += 32) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc = fmaf(ws[o_t + i * 3 + c], dvp[c], acc);
        V(kVDpr0)[i] = ppre[(sl * 2 + 0) * kHeadMaxDim + i] > 0.f ? acc : 0.f;
        V(kVDpr1)[i] = ppre[(sl * 2 + 1) * kHeadMaxDim + i] > 0.f ? acc : 0.f;
      }
    } else {
      const int o_bh = o_t + Mx * F, o_wo = o_bh + F;
      for (int j = jj; j < F; j += 32) {
        float acc = ws[o_bh + j];
        for (int i = 0; i < Mx; ++i) acc = fmaf(mx[i], ws[o_t + i * F + j], acc);
        V(kVHid)[j] = fmaxf(acc, 0.f);
      }
      __syncthreads();
      if (hl.y && live) {
        float pred = ws[o_wo + F];
        for (int j = 0; j < F; ++j) pred = fmaf(V(kVHid)[j], ws[o_wo + j], pred);  // as the forward kernel
        d = gscale * (pred - hl.y[b]);
      }
      if (jj == 0) V(kVOne)[0] = d;
      for (int j = jj; j < F; j += 32) top[j] = V(kVHid)[j] > 0.f ? ws[o_wo + j] * d : 0.f;
      __syncthreads();
      for (int i = jj; i < Mx; i += 32) {
        float acc = 0.f;
        for (int j = 0; j < F; ++j) acc = fmaf(ws[o_t + i * F + j], top[j], acc);
        V(kVDpr0)[i] = ppre[(sl * 2 + 0) * kHeadMaxDim + i] > 0.f ? acc : 0.f;
        V(kVDpr1)[i] = ppre[(sl * 2 + 1) * kHeadMaxDim + i] > 0.f ? acc : 0.f;
      }
    }
    __syncthreads();
    // ---- projections (relu) -> fingerprints (relu) -> pooled
    for (int g = 0; g < 2; ++g) {
      const float* dpr = V(kVDpr0 + g);
      for (int i = jj; i < F; i += 32) {
        float acc = 0.f;
        for (int j = 0; j < Mx; ++j) acc = fmaf(ws[o_p[g] + i * Mx + j], dpr[j], acc);
        V(kVDfp0 + g)[i] = fpre[(sl * 2 + g) * kHeadMaxDim + i] > 0.f ? acc : 0.f;
      }
    }
    __syncthreads();
    for (int g = 0; g < 2; ++g) {
      const float* dfg = V(kVDfp0 + g);
      float* dx = g == 0 ? dpc : dpa;
      for (int i = jj; i < D; i += 32) {
        float acc = 0.f;
        for (int j = 0; j < F; ++j) acc = fmaf(ws[o_fp[g] + i * F + j], dfg[j], acc);
        if (live) dx[(int64_t)b * D + i] = acc;
      }
    }
    // ---- parameter gradients: element t of the packed layout = sum over the samples of a[i] * b[j]
    for (int t = tid; t < total; t += blockDim.x) {
      int base;
      const int sgm = head_segment(ht, t, &base);
      const int loc = t - base;
      int va, vb, ncols;  // va < 0: a bias (sum of b[j])
      switch (sgm) {
        case 0: va = kVX0, vb = kVDfp0, ncols = F; break;
        case 1: va = -1, vb = kVDfp0, ncols = F; break;
        case 2: va = kVX1, vb = kVDfp1, ncols = F; break;
        case 3: va = -1, vb = kVDfp1, ncols = F; break;
        case 4: va = kVFp0, vb = kVDpr0, ncols = Mx; break;
        case 5: va = -1, vb = kVDpr0, ncols = Mx; break;
        case 6: va = kVFp1, vb = kVDpr1, ncols = Mx; break;
        case 7: va = -1, vb = kVDpr1, ncols = Mx; break;
        case 8: va = kVMix, vb = kVTop, ncols = kind == 0 ? 3 : F; break;
        case 9: va = -1, vb = kVTop, ncols = kind == 0 ? 3 : F; break;
        case 10: va = kVHid, vb = kVOne, ncols = 1; break;  // Wo (F,1): hidden * dout
        default: va = -1, vb = kVOne, ncols = 1; break;     // bo
      }
      const int i = loc / ncols, j = loc - i * ncols;
      float acc = 0.f;
      if (va < 0) {
#pragma unroll
        for (int q = 0; q < kHeadSPB; ++q) acc += vec[q * kHdVecStride + head_vec_off(vb) + j];
      } else {
#pragma unroll
        for (int q = 0; q < kHeadSPB; ++q)
          acc = fmaf(vec[q * kHdVecStride + head_vec_off(va) + i], vec[q * kHdVecStride + head_vec_off(vb) + j], acc);
      }
      dws[t] += acc;
    }
  }
  __syncthreads();
  const float reg_scale = (hl.y && blockIdx.x == 0) ? 2.0f * hl.dloss[0] : 0.f;  // d/dW of l2 * sum(W^2), added once
  for (int t = tid; t < total; t += blockDim.x) {
    int base;
    const int sgm = head_segment(ht, t, &base);
    const float v = dws[t] + reg_scale * head_l2(ht, sgm) * ws[t];
    if (v != 0.f) atomicAdd(head_gptr(ht, sgm) + (t - base), v);
  }
}

}  // namespace

// ---- the launchers' part of the family's rules, after api.hip's: widths, null weight / gradient tensor i, LDS fit
namespace {
// The most dynamic LDS a launch may ask for: all 160 KB of a CU for the packed forward, which has no static LDS; 4 KB
// less for the table forward (it has 1 KB of static LDS) and the backward.  Which shapes are refused follows from these.
constexpr size_t kHeadPackedLdsCap = 160 * 1024, kHeadTableLdsCap = 156 * 1024;

size_t align4(size_t n) { return (n + 3) / 4 * 4; }

// the kernels' view of c.weights (and, with_grads, c.dweights): weight i, then gradient i, tensor by tensor
int head_tensor_table(const ModelHeadCall& c, bool with_grads, HeadTensors* ht) {
  const int D = c.D, F = c.F, Mx = c.Mx;
  const int top = c.kind == 0 ? 3 : F;  // vp (Mx -> 3), or the hidden layer (Mx -> F) and Wo | bo behind it
  const int sizes[kHeadTensors] = {D * F, F, D * F, F, F * Mx, Mx, F * Mx, Mx, Mx * top, top, F, 1};
  ht->n = c.kind == 0 ? 10 : 12;
  int off = 0;
  for (int i = 0; i < ht->n; ++i) {
    if (!c.weights[i]) return fail(IMPNN_E_BADARG, "model_head: null weight tensor %d", i);
    ht->w[i] = c.weights[i];
    ht->g[i] = with_grads ? c.dweights[i] : nullptr;
    if (with_grads && !c.dweights[i]) return fail(IMPNN_E_BADARG, "model_head_bwd: null gradient tensor %d", i);
    ht->off[i] = off;
    ht->l2[i] = c.l2 ? c.l2[i] : 0.f;
    off += sizes[i];
  }
  ht->off[ht->n] = off;
  return IMPNN_OK;
}

}  // namespace

int64_t model_head_loss_workspace_floats(int B) { return (B + kHeadSPB - 1) / kHeadSPB + 4; }

// The most weight floats (padded to 4) the backward holds: it keeps the weights and their gradient sums in LDS next to
// the sample vectors.  model.py asks for it before a training pass takes the fused head nodes (ops.HEAD_BWD_MAX_FLOATS).
int64_t model_head_bwd_max_floats() {
  const size_t vectors = (size_t)kHeadSPB * (kHdVecStride + 4 * kHeadMaxDim);
  return (int64_t)((kHeadTableLdsCap / sizeof(float) - vectors) / 2 / 4 * 4);
}

int launch_model_head(const ModelHeadCall& c) {
  if (int rc = head_widths_covered("model_head", c.D, c.F, c.Mx)) return rc;
  const int wfloats = (int)impnn_model_head_floats(c.kind, c.D, c.F, c.Mx);
  const size_t lds = sizeof(float) * (align4(wfloats) + (size_t)kHeadSPB * (2 * kHeadMaxX + 4 * kHeadMaxDim));
  // every (D <= 128, F <= 64, Mx <= 64) fits the 160 KB of a gfx950 CU: 29 057 weight floats + 16 KB of sample scratch
  if (lds > kHeadPackedLdsCap) return fail(IMPNN_E_UNSUPPORTED, "model_head: weights do not fit LDS");
  if (lds > 64 * 1024)
    if (int rc = ensure_lds_limit((const void*)model_head_kernel, 8)) return rc;
  model_head_kernel<<<(c.B + kHeadSPB - 1) / kHeadSPB, 256, lds, c.stream>>>(c.kind, c.pc, c.pa, c.T, c.w, c.out, c.B,
                                                                           c.D, c.F, c.Mx, wfloats);
  return check_launch("model_head");
}

// c.y (the loss entries) makes it the loss forward: c.out is then optional
int launch_model_head_tensors(const ModelHeadCall& c) {
  if (int rc = head_widths_covered("model_head", c.D, c.F, c.Mx)) return rc;
  HeadTensors ht{};
  if (int rc = head_tensor_table(c, false, &ht)) return rc;
  HeadLoss hl{};
  if (c.y) {  // workspace: [0] arrival counter (zero between calls) | [4...] one partial per workgroup
    hl.y = c.y;
    hl.loss_out = c.loss;
    hl.counter = reinterpret_cast<unsigned int*>(c.workspace);
    hl.partial = c.workspace + 4;
    hl.inv_B = 1.0f / (float)c.B;
  }
  const size_t lds = sizeof(float) * (align4(ht.off[ht.n]) + (size_t)kHeadSPB * (2 * kHeadMaxX + 6 * kHeadMaxDim));
  if (lds > kHeadTableLdsCap) return fail(IMPNN_E_UNSUPPORTED, "model_head: weights do not fit LDS");
  auto launch = [&](auto kernel, auto arg) {
    static_cast<HeadLoss&>(arg) = hl;
    if (lds > 48 * 1024)
      (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    kernel<<<(c.B + kHeadSPB - 1) / kHeadSPB, 256, lds, c.stream>>>(c.kind, c.pc, c.pa, c.T, ht, c.out, c.B, c.D, c.F,
                                                                  c.Mx, arg);
  };
  if (c.y && c.sample_weight) {
    HeadLossArg<true> arg{};
    arg.w = c.sample_weight;
    launch(model_head_tensors_kernel<true>, arg);
  } else {
    launch(model_head_tensors_kernel<false>, HeadLossArg<false>{});
  }
  return check_launch("model_head_tensors");
}

// c.y (the loss entries): the prediction's gradient comes from y and c.dloss, and c.dout is not read
int launch_model_head_bwd(const ModelHeadCall& c) {
  if (int rc = head_widths_covered("model_head_bwd", c.D, c.F, c.Mx)) return rc;
  HeadTensors ht{};
  if (int rc = head_tensor_table(c, true, &ht)) return rc;
  HeadLoss hl{};
  if (c.y) {
    hl.y = c.y;
    hl.dloss = c.dloss;
    hl.inv_B = 1.0f / (float)c.B;
  }
  const size_t lds = sizeof(float) * (2 * align4(ht.off[ht.n]) + (size_t)kHeadSPB * (kHdVecStride + 4 * kHeadMaxDim));
  if ((int64_t)align4(ht.off[ht.n]) > model_head_bwd_max_floats())
    return fail(IMPNN_E_UNSUPPORTED, "model_head_bwd: weights do not fit LDS");
  const int groups = (c.B + kHeadSPB - 1) / kHeadSPB;  // bounded grid: every workgroup flushes ~|weights| atomics once
  auto launch = [&](auto kernel, auto arg) {
    static_cast<HeadLoss&>(arg) = hl;
    if (lds > 48 * 1024)
      (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    kernel<<<groups < 512 ? groups : 512, 1024, lds, c.stream>>>(c.kind, c.pc, c.pa, c.T, ht, c.dout, c.dpc, c.dpa, c.B,
                                                               c.D, c.F, c.Mx, arg);
  };
  if (c.y && c.sample_weight) {
    HeadLossArg<true> arg{};
    arg.w = c.sample_weight;
    launch(model_head_bwd_kernel<true>, arg);
  } else {
    launch(model_head_bwd_kernel<false>, HeadLossArg<false>{});
  }
  return check_launch("model_head_bwd");
}

}  // namespace impnn
