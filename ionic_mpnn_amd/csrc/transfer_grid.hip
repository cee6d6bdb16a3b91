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
#include "common.h"
#include "head_device.h"

namespace impnn {

namespace {

constexpr int kH1 = 256, kH2 = 128, kH3 = 64;
constexpr int kHalfRows = 8;  // ion rows per 256-thread workgroup, 32 threads per row (as head_ion_mix_kernel)

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
__device__ __forceinline__ f32x4_t ld4(const float* p) { return *reinterpret_cast<const f32x4_t*>(p); }

inline size_t align4(size_t n) { return (n + 3) & ~(size_t)3; }

// ---- the prepared image, in floats.  W2 / W3 blocks are 64 lanes x 4 floats in A-operand order: lane l (row a = l & 31,
// half h = l >> 5), element b of block (g, mb) holds the kernel entry [input 8 g + 4 h + b][output 32 mb + a], so a
// lane's A operands of four consecutive k steps are one 16-byte load and a wave's load is 1 KB, contiguous.
constexpr int kImgW2 = 0;                          // [g 0..31][mb 0..3][64][4]
constexpr int kImgW3 = kImgW2 + kH1 * kH2;         // [kb 0..3][g 0..3][mb 0..1][64][4], input 32 kb + 8 g + 4 h + b
constexpr int kImgScale = kImgW3 + kH2 * kH3;      // gamma / sqrt(moving_var + eps)          [256]
constexpr int kImgShift = kImgScale + kH1;         // beta - moving_mean * scale              [256]
constexpr int kImgB2 = kImgShift + kH1;            // [128]
constexpr int kImgB3 = kImgB2 + kH2;               // [64]
constexpr int kImgWo = kImgB3 + kH3;               // [64]
constexpr int kImgBo = kImgWo + kH3;               // [1] + 3 pad
constexpr int kImgFloats = kImgBo + 4;             // 41 732 floats, 163.0 KiB

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

// ---- the grid.  One workgroup owns kTgTileC cations x kTgTileA anions; a wave owns two cations of the tile, i.e. two
// MFMA column blocks of 32 pairs (lane & 31 = anion), and fetches every weight once for its 64 pairs.
constexpr int kTgTileC = 8, kTgTileA = 32;
// Row stride (floats) of the anion u rows in LDS.  A lane reads its anion's row 16 bytes at a time (ds_read_b128: 16
// lanes per LDS cycle, 64 banks), so the 16 lanes of a group must start 4 banks apart: stride = 4 * odd.  256 unpadded
// would put every lane on one bank quad; 260 = 4 * 65.  The cation rows, scale and shift are read at one address per
// lane half (a broadcast), so they stay unpadded.
constexpr int kTgAnStride = kH1 + 4;
constexpr int kTgLdsFloats = kTgTileA * kTgAnStride + kTgTileC * kH1 + 2 * kH1 + kTgTileC * kTgTileA;  // 43.5 KiB

__device__ __forceinline__ f32x16_t mfma32(float a, float b, f32x16_t c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// Writes `rows` spans of `span` floats (row r starts at out + first + r * pitch, its values at res + r * rs) with
// 16-byte stores on every naturally aligned quad inside the span and 4-byte stores on the ragged ends (the scheme of
// head_grid.hip's store_rows, one value per pair).
__device__ __forceinline__ void store_spans(float* __restrict__ out, int64_t first, int64_t pitch, int rows, int span,
                                            const float* res, int rs) {
  const int64_t po = (int64_t)((reinterpret_cast<uintptr_t>(out) >> 2) & 3);
  const int quads = (span + 3) / 4 + 1;  // quads a span can touch at any alignment
  for (int item = threadIdx.x; item < rows * quads; item += blockDim.x) {
    const int r = item / quads, q = item - r * quads;
    const int64_t g0 = first + (int64_t)r * pitch;
    const int e0 = 4 * q - (int)((g0 + po) & 3);  // out + g0 + e0 is 16-byte aligned
    if (e0 >= span) continue;
    const float* v = res + r * rs + e0;
    if (e0 >= 0 && e0 + 3 < span) {
      // written once and not read again by the launch: a streaming (nontemporal) global_store_dwordx4
      __builtin_nontemporal_store(f32x4_t{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4_t*>(out + g0 + e0));
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e0 + k >= 0 && e0 + k < span) out[g0 + e0 + k] = v[k];
    }
  }
}

// One k group (8 input features: 4 per lane half) of Dense 128 for a wave's two column blocks: the operand
// bn(relu(u_cat + u_an)) is formed in registers, then 4 k steps x 4 row blocks x 2 column blocks of MFMA.
__device__ __forceinline__ void dense128_group(f32x16_t (&acc)[4][2], const f32x4_t (&w)[4], const float* ua_row,
                                               const float* uc_row, const float* bn_half, int g) {
  const f32x4_t ua = ld4(ua_row + 8 * g), sc = ld4(bn_half + 8 * g), sh = ld4(bn_half + kH1 + 8 * g);
  const f32x4_t uc0 = ld4(uc_row + 8 * g), uc1 = ld4(uc_row + kH1 + 8 * g);
  float x[2][4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {  // relu(mp_dense_1), then BatchNormalization's affine, per feature
    x[0][b] = fmaf(head_relu(uc0[b] + ua[b]), sc[b], sh[b]);
    x[1][b] = fmaf(head_relu(uc1[b] + ua[b]), sc[b], sh[b]);
  }
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = mfma32(w[mb][b], x[nb][b], acc[mb][nb]);
}

// One k group of Dense 64: registers 4 g .. 4 g + 3 of the input block's accumulators, relu applied on the way.
__device__ __forceinline__ void dense64_group(f32x16_t (&acc)[2][2], const f32x16_t (&in)[2], const f32x4_t (&w)[2],
                                              int g) {
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const float a2 = head_relu(in[nb][4 * g + b]);
      acc[0][nb] = mfma32(w[0][b], a2, acc[0][nb]);
      acc[1][nb] = mfma32(w[1][b], a2, acc[1][nb]);
    }
}

__global__ __launch_bounds__(256) void transfer_grid_kernel(const float* __restrict__ u_cat,
                                                            const float* __restrict__ u_an,
                                                            const float* __restrict__ img, float* __restrict__ out,
                                                            int C, int A, int tiles_a) {
  extern __shared__ __align__(16) float sm[];
  float* uan = sm;                            // [kTgTileA][kTgAnStride]
  float* ucat = uan + kTgTileA * kTgAnStride; // [kTgTileC][kH1]
  float* bnv = ucat + kTgTileC * kH1;         // scale kH1 | shift kH1
  float* res = bnv + 2 * kH1;                 // [kTgTileC][kTgTileA]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, p = lane & 31, h = lane >> 5;
  const int c0 = (blockIdx.x / tiles_a) * kTgTileC, a0 = (blockIdx.x % tiles_a) * kTgTileA;
  const int nc = min(kTgTileC, C - c0), na = min(kTgTileA, A - a0);

  // the tile's u rows; the rows of a ragged tile's padding pairs are zero (computed, not stored)
  const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
  for (int idx = tid; idx < kTgTileA * (kH1 / 4); idx += blockDim.x) {
    const int r = idx >> 6, q = idx & 63;
    *reinterpret_cast<f32x4_t*>(uan + r * kTgAnStride + 4 * q) = r < na ? ld4(u_an + (int64_t)(a0 + r) * kH1 + 4 * q) : zero4;
  }
  for (int idx = tid; idx < kTgTileC * (kH1 / 4); idx += blockDim.x) {
    const int r = idx >> 6, q = idx & 63;
    *reinterpret_cast<f32x4_t*>(ucat + r * kH1 + 4 * q) = r < nc ? ld4(u_cat + (int64_t)(c0 + r) * kH1 + 4 * q) : zero4;
  }
  for (int idx = tid; idx < 2 * kH1 / 4; idx += blockDim.x)
    *reinterpret_cast<f32x4_t*>(bnv + 4 * idx) = ld4(img + kImgScale + 4 * idx);
  __syncthreads();

  if (2 * wave < nc) {  // (wave-uniform; no barrier inside)
    const float* ua_row = uan + p * kTgAnStride + 4 * h;
    const float* uc_row = ucat + (2 * wave) * kH1 + 4 * h;
    const f32x4_t* w2 = reinterpret_cast<const f32x4_t*>(img + kImgW2) + lane;
    const f32x4_t* w3 = reinterpret_cast<const f32x4_t*>(img + kImgW3) + lane;

    // Dense 128: the accumulators start at the bias (bias first, as every Dense of this project)
    f32x16_t acc2[4][2];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4_t bb = ld4(img + kImgB2 + 32 * mb + 8 * q + 4 * h);
#pragma unroll
        for (int b = 0; b < 4; ++b) acc2[mb][0][4 * q + b] = acc2[mb][1][4 * q + b] = bb[b];
      }
    // The A operands of k group g + 1 travel while the 32 MFMAs of group g run: two register sets in turn, and
    // scheduling fences, without which the compiler sinks the loads to just before their use (one L2 latency exposed
    // per group).
    f32x4_t wa[4], wb[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) wa[mb] = w2[mb * 64];
#pragma unroll 1
    for (int g = 0; g < kH1 / 8; g += 2) {
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) wb[mb] = w2[((g + 1) * 4 + mb) * 64];
      __builtin_amdgcn_sched_barrier(0);
      dense128_group(acc2, wa, ua_row, uc_row, bnv + 4 * h, g);
      __builtin_amdgcn_sched_barrier(0);
      const int gn = min(g + 2, kH1 / 8 - 1);  // (the last turn reloads group 31: in bounds, unused)
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) wa[mb] = w2[(gn * 4 + mb) * 64];
      __builtin_amdgcn_sched_barrier(0);
      dense128_group(acc2, wb, ua_row, uc_row, bnv + 4 * h, g + 1);
      __builtin_amdgcn_sched_barrier(0);
    }

    // Dense 64: the B operand of k step 4 g + b of input block kb is register 4 g + b of acc2[kb]
    f32x16_t acc3[2][2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4_t bb = ld4(img + kImgB3 + 32 * mb + 8 * q + 4 * h);
#pragma unroll
        for (int b = 0; b < 4; ++b) acc3[mb][0][4 * q + b] = acc3[mb][1][4 * q + b] = bb[b];
      }
    f32x4_t va[2], vb[2];
    va[0] = w3[0], va[1] = w3[64];
#pragma unroll
    for (int s = 0; s < 16; s += 2) {  // s = 4 kb + g
      vb[0] = w3[((s + 1) * 2 + 0) * 64], vb[1] = w3[((s + 1) * 2 + 1) * 64];
      __builtin_amdgcn_sched_barrier(0);
      dense64_group(acc3, acc2[s >> 2], va, s & 3);
      __builtin_amdgcn_sched_barrier(0);
      const int sn = s + 2 < 16 ? s + 2 : 15;
      va[0] = w3[(sn * 2 + 0) * 64], va[1] = w3[(sn * 2 + 1) * 64];
      __builtin_amdgcn_sched_barrier(0);
      dense64_group(acc3, acc2[(s + 1) >> 2], vb, (s + 1) & 3);
      __builtin_amdgcn_sched_barrier(0);
    }

    // Dense 1: a lane sums its 32 features in ascending order, the two lane halves meet (half 0 first), then the bias
    float part[2] = {0.f, 0.f};
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4_t wo = ld4(img + kImgWo + 32 * mb + 8 * q + 4 * h);
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) part[nb] = fmaf(head_relu(acc3[mb][nb][4 * q + b]), wo[b], part[nb]);
      }
    const float bo = img[kImgBo];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const float other = __shfl_xor(part[nb], 32);
      if (h == 0) res[(2 * wave + nb) * kTgTileA + p] = (part[nb] + other) + bo;
    }
  }
  __syncthreads();
  store_spans(out, (int64_t)c0 * A + a0, (int64_t)A, nc, na, res, kTgTileA);
}

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

int launch_transfer_head_grid(const float* u_cat, const float* u_an, const float* image, float* out, int C, int A,
                              hipStream_t s) {
  const int tiles_a = (A + kTgTileA - 1) / kTgTileA;
  const int64_t tiles = (int64_t)((C + kTgTileC - 1) / kTgTileC) * tiles_a;
  if (tiles > 0x7fffffff)
    return fail(IMPNN_E_UNSUPPORTED, "transfer_head_grid: %lld tiles of %d x %d pairs exceed one launch; split the cation axis",
                (long long)tiles, kTgTileC, kTgTileA);
  transfer_grid_kernel<<<(int)tiles, 256, sizeof(float) * kTgLdsFloats, s>>>(u_cat, u_an, image, out, C, A, tiles_a);
  return check_launch("transfer_head_grid");
}

}  // namespace impnn
