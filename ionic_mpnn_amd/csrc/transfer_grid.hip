// The transfer head over a Cartesian product (include/impnn.h: impnn_transfer_grid_prepare, impnn_transfer_ion_half,
// impnn_transfer_head_grid).  Inference semantics: moving statistics, no Dropout, as impnn_transfer_head.
//
// mix = relu(proj_cat) + relu(proj_an) is a sum and mp_dense_1 is linear in it before its relu, so
//   a1[i, j] = relu(Uc[i] + Ua[j]),   Uc = mix_cat W1 (C,256),   Ua = mix_an W1 + b1 (A,256)
// and a screen of C cations x A anions needs C + A rows of the first three Dense layers, not C * A:
//   transfer_ion_half_kernel   u_g[m] = relu(relu(pooled_g[m] Wfp_g + bfp_g) Wp_g + bp_g) W1 (+ b1 for the anion)
//   transfer_grid_kernel       per pair (i, j): bn(relu(u_cat[i] + u_an[j])) -> Dense 128 relu -> Dense 64 relu -> Dense 1
// The grid kernel runs the two GEMM layers on v_mfma_f32_32x32x2_f32 (exact f32 products, a k-ordered fmaf chain per
// output) with the PAIRS on the MFMA's column (lane) dimension and the layer's output features on its rows:
//   a2^T (128 x pairs) = W2^T (128 x 256) bn^T (256 x pairs),   a3^T (64 x pairs) = W3^T (64 x 128) a2^T
// A 32x32 result has its column on the lane and its rows in the 16 registers of the lane, which is the B operand of the
// next product up to the order of k inside a block of 32: register r of lane half h is row 8 (r / 4) + 4 h + r % 4.
// The weight image (transfer_grid_prepare_kernel) stores W2 and W3 in that k order, so a pair's activations go from
// u rows to the prediction in registers: a1, bn, a2 and a3 never exist in memory.  A pair is one column; its value
// depends on its two u rows and the image only, not on the lane, wave, tile or launch that computes it.  No atomics.
#include "grid_device.h"

namespace impnn {

namespace {

constexpr int kHalfRows = 8;  // ion rows per 256-thread workgroup, 32 threads per row (as head_ion_mix_kernel)

// (the prepared image's layout, kImg*: grid_device.h)
struct PrepTensors {
  const float *gamma, *beta, *w2, *b2, *w3, *b3, *wo, *bo, *mean, *var;
};

__global__ __launch_bounds__(256) void transfer_grid_prepare_kernel(PrepTensors t, float eps, float* __restrict__ img) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= kImgFloats) return;
  float v = 0.f;
  if (e < kImgW3) {
    const int b = e & 3, l = (e >> 2) & 63, mb = (e >> 8) & 3, g = e >> 10;
    v = t.w2[(8 * g + 4 * (l >> 5) + b) * kH2 + 32 * mb + (l & 31)];
  } else if (e < kImgScale) {
    const int r = e - kImgW3;
    const int b = r & 3, l = (r >> 2) & 63, mb = (r >> 8) & 1, g = (r >> 9) & 3, kb = r >> 11;
    v = t.w3[(32 * kb + 8 * g + 4 * (l >> 5) + b) * kH3 + 32 * mb + (l & 31)];
  } else if (e < kImgB2) {
    const int f = (e - kImgScale) & (kH1 - 1);
    const float scale = t.gamma[f] / sqrtf(t.var[f] + eps);
    v = e < kImgShift ? scale : t.beta[f] - t.mean[f] * scale;
  } else if (e < kImgB3) {
    v = t.b2[e - kImgB2];
  } else if (e < kImgWo) {
    v = t.b3[e - kImgB3];
  } else if (e < kImgBo) {
    v = t.wo[e - kImgWo];
  } else if (e == kImgBo) {
    v = t.bo[0];
  }
  img[e] = v;
}

// ---- the per-ion half: head_ion_mix_kernel's two Dense layers, then the row times W1.  O(C + A) work on the VALU.
__global__ __launch_bounds__(256) void transfer_ion_half_kernel(const float* __restrict__ pooled,
                                                                const float* __restrict__ wfp_g,
                                                                const float* __restrict__ bfp_g,
                                                                const float* __restrict__ wp_g,
                                                                const float* __restrict__ bp_g,
                                                                const float* __restrict__ w1,
                                                                const float* __restrict__ b1, float* __restrict__ u,
                                                                int M, int D, int F, int Mx) {
  extern __shared__ __align__(16) float sm[];
  const int nfp = D * F, np = F * Mx;
  float* Wfp = sm;                                 // Wfp_g D*F
  float* bfp = Wfp + ((nfp + 3) & ~3);             // bfp_g F
  float* Wp = bfp + kHeadMaxDim;                       // Wp_g F*Mx
  float* bp = Wp + ((np + 3) & ~3);                // bp_g Mx
  float* xs = bp + kHeadMaxDim;                        // [kHalfRows][kHeadMaxX]
  float* fp = xs + kHalfRows * kHeadMaxX;              // [kHalfRows][kHeadMaxDim]
  float* mix = fp + kHalfRows * kHeadMaxDim;           // [kHalfRows][kHeadMaxDim]
  const int tid = threadIdx.x, sl = tid >> 5, jj = tid & 31;
  const int64_t m = (int64_t)blockIdx.x * kHalfRows + sl;
  const bool live = m < M;
  for (int t = tid; t < nfp; t += blockDim.x) Wfp[t] = wfp_g[t];
  for (int t = tid; t < np; t += blockDim.x) Wp[t] = wp_g[t];
  for (int t = tid; t < F; t += blockDim.x) bfp[t] = bfp_g[t];
  for (int t = tid; t < Mx; t += blockDim.x) bp[t] = bp_g[t];
  for (int i = jj; i < D; i += 32) xs[sl * kHeadMaxX + i] = live ? pooled[m * D + i] : 0.f;
  __syncthreads();
  for (int j = jj; j < F; j += 32) fp[sl * kHeadMaxDim + j] = head_relu(head_chain(xs + sl * kHeadMaxX, Wfp + j, F, D, bfp[j]));
  __syncthreads();
  for (int j = jj; j < Mx; j += 32) mix[sl * kHeadMaxDim + j] = head_relu(head_chain(fp + sl * kHeadMaxDim, Wp + j, Mx, F, bp[j]));
  __syncthreads();
  if (live)
    for (int j = jj; j < kH1; j += 32)  // W1 from L2: 32 consecutive columns per row of threads
      u[m * kH1 + j] = head_chain(mix + sl * kHeadMaxDim, w1 + j, kH1, Mx, b1 ? b1[j] : 0.f);
}

// ---- the grid: transfer_grid_kernel and its tile are in grid_device.h, where grid_select.hip shares them.

}  // namespace

int64_t transfer_grid_image_floats() { return kImgFloats; }

int launch_transfer_grid_prepare(const float* const* weights, const float* moving_mean, const float* moving_var,
                                 float bn_eps, float* image, hipStream_t s) {
  const PrepTensors t{weights[10], weights[11], weights[12], weights[13], weights[14],
                      weights[15], weights[16], weights[17], moving_mean, moving_var};
  transfer_grid_prepare_kernel<<<(kImgFloats + 255) / 256, 256, 0, s>>>(t, bn_eps, image);
  return check_launch("transfer_grid_prepare");
}

int launch_transfer_ion_half(int ion, const float* pooled, const float* const* weights, float* u, int M, int D, int F,
                             int Mx, hipStream_t s) {
  const size_t lds = sizeof(float) * (align4((size_t)D * F) + align4((size_t)F * Mx) + 2 * kHeadMaxDim +
                                      (size_t)kHalfRows * (kHeadMaxX + 2 * kHeadMaxDim));  // <= 56.5 KiB
  transfer_ion_half_kernel<<<(int)(((int64_t)M + kHalfRows - 1) / kHalfRows), 256, lds, s>>>(
      pooled, weights[2 * ion], weights[2 * ion + 1], weights[4 + 2 * ion], weights[5 + 2 * ion], weights[8],
      ion == 1 ? weights[9] : nullptr, u, M, D, F, Mx);
  return check_launch("transfer_ion_half");
}

int launch_transfer_head_grid(const GridOperands& g, float* out) {
  const GridTiles tiles = grid_tiles(1, g.C, g.A);
  if (int rc = grid_tiles_fit("transfer_head_grid", tiles)) return rc;
  launch_grid_family<1>(g, (unsigned)tiles.count(), 0, GridOut{out});
  return check_launch("transfer_head_grid");
}

}  // namespace impnn
