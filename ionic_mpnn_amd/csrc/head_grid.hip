// f1 over a Cartesian product (include/impnn.h: impnn_head_ion_mix, impnn_head_grid).
//
// An ion's branch of the head never sees its partner until AddTwoTensors / Add (train_viscosity.py:189,197-201;
// train_melting_point.py:173,191), so a screen of C cations x A anions needs C + A mixing rows, not C * A:
//   head_ion_mix_kernel   mix_g[m] = relu(relu(pooled_g[m] Wfp_g + bfp_g) Wp_g + bp_g)      one row per ion species
//   head_grid_kernel      per pair (i, j): mixed = mix_cat[i] + mix_an[j], then the tail of model_head_kernel
// Every rounding step is the one of model_head_kernel (head_device.h; the same fmaf chains, bias first, inputs
// ascending), so element (i, j, t) carries the bits impnn_model_head gives for the sample (pooled_cat[i],
// pooled_an[j], T[t]).  No atomics, every sum in a fixed order.
#include "grid_device.h"

namespace impnn {

namespace {

constexpr int kMixRows = 8;   // ion rows per 256-thread workgroup, 32 threads per row (as model_head_kernel)

__global__ __launch_bounds__(256) void head_ion_mix_kernel(const float* __restrict__ pooled,
                                                           const float* __restrict__ wfp_g,
                                                           const float* __restrict__ wp_g, float* __restrict__ mix,
                                                           int M, int D, int F, int Mx) {
  extern __shared__ __align__(16) float sm[];
  const int nfp = D * F + F, np = F * Mx + Mx;
  float* Wfp = sm;                          // Wfp_g D*F | bfp_g F
  float* Wp = Wfp + ((nfp + 3) & ~3);       // Wp_g F*Mx | bp_g Mx
  float* xs = Wp + ((np + 3) & ~3);         // [kMixRows][kHeadMaxX]
  float* fp = xs + kMixRows * kHeadMaxX;        // [kMixRows][kHeadMaxDim]
  const int tid = threadIdx.x, sl = tid >> 5, jj = tid & 31;
  const int64_t m = (int64_t)blockIdx.x * kMixRows + sl;
  const bool live = m < M;
  for (int t = tid; t < nfp; t += blockDim.x) Wfp[t] = wfp_g[t];
  for (int t = tid; t < np; t += blockDim.x) Wp[t] = wp_g[t];
  for (int i = jj; i < D; i += 32) xs[sl * kHeadMaxX + i] = live ? pooled[m * D + i] : 0.f;
  __syncthreads();
  for (int j = jj; j < F; j += 32)
    fp[sl * kHeadMaxDim + j] = head_relu(head_chain(xs + sl * kHeadMaxX, Wfp + j, F, D, Wfp[D * F + j]));
  __syncthreads();
  if (live)
    for (int j = jj; j < Mx; j += 32)
      mix[m * Mx + j] = head_relu(head_chain(fp + sl * kHeadMaxDim, Wp + j, Mx, F, Wp[F * Mx + j]));
}

// ---- the grid: head_grid_kernel, its tile and its stores are in grid_device.h, where the selecting form of
// grid_select.hip shares them.
constexpr int kGridMaxT = 4096;  // temperatures per launch: T / 100 sits in LDS (16 KB)

}  // namespace

int launch_head_ion_mix(int kind, int ion, const float* pooled, const float* w, float* mix, int M, int D, int F, int Mx,
                        hipStream_t s) {
  (void)kind;  // both kinds share the per-ion layout
  const int nfp = D * F + F, np = F * Mx + Mx;
  const size_t lds = sizeof(float) * (align4(nfp) + align4(np) + (size_t)kMixRows * (kHeadMaxX + kHeadMaxDim));  // <= 54.3 KiB
  head_ion_mix_kernel<<<(int)(((int64_t)M + kMixRows - 1) / kMixRows), 256, lds, s>>>(pooled, w + (size_t)ion * nfp,
                                                                      w + 2 * (size_t)nfp + (size_t)ion * np, mix, M, D, F, Mx);
  return check_launch("head_ion_mix");
}

int head_grid_max_temperatures() { return kGridMaxT; }

int launch_head_grid(const GridOperands& g, float* out, float* params) {
  const GridTiles tiles = grid_tiles(0, g.C, g.A);
  if (int rc = grid_tiles_fit("head_grid", tiles)) return rc;
  launch_grid_family<0>(g, (unsigned)tiles.count(), 0, GridOut{out, params});  // <= 50.0 KiB of LDS (kind 0), 41.8 KiB (kind 1)
  return check_launch("head_grid");
}

}  // namespace impnn
