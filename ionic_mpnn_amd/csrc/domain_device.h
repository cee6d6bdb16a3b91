// Device code the applicability-domain kernels (grid_domain.hip) and the diverse selection (grid_diverse.hip) share:
// the one definition of the distance's inner loop, its result and the staging of rows with zero pads.  An element has
// the same bits whichever kernel produced it.
//
// The pads of a row (k >= Mx, up to the next multiple of 4) are staged as zeros on both sides: diff = 0 - 0 and
// fmaf(0, 0, d2) = d2 exactly, so a padded quad needs no per-element test and the sum is the definition's, k ascending
// over Mx terms.  No |z|^2 - 2 z.r + |r|^2 expansion, no matrix-core product: a training pair's distance is exactly 0.
#pragma once

#include "grid_device.h"

namespace impnn {

constexpr int kDomainChunk = 64;     // reference rows per LDS chunk: 16 KiB at Mx = 64
constexpr int kDomainRegs = 128;     // latent floats a thread of the grid kernels holds

// Rows p0 .. p0 + n of the reference, in LDS as chunk[n][S2] with zero pads, against the P latent vectors of a thread:
// d2 = 0; diff = z[k] - ref[p][k]; d2 = fmaf(diff, diff, d2), k ascending; the running best (start: +inf, -1) is
// replaced on d2 < best, so the lowest p wins among equal d2 and a NaN never wins.  EXCL: row self[q] is no candidate.
template <int MXR, int P, bool EXCL>
__device__ __forceinline__ void domain_scan(const float (&z)[P][MXR], const float* chunk, int n, int p0, int Mx, int S2,
                                            const int (&self)[P], float (&best)[P], int (&nearest)[P]) {
  for (int p = 0; p < n; ++p) {
    const float* r = chunk + p * S2;
    float d2[P];
#pragma unroll
    for (int q = 0; q < P; ++q) d2[q] = 0.f;
#pragma unroll
    for (int k4 = 0; k4 < MXR; k4 += 4)
      if (k4 < Mx) {
        const f32x4_t rr = ld4(r + k4);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int q = 0; q < P; ++q) {
            const float diff = z[q][k4 + u] - rr[u];
            d2[q] = fmaf(diff, diff, d2[q]);
          }
      }
#pragma unroll
    for (int q = 0; q < P; ++q)
      if ((!EXCL || p0 + p != self[q]) && d2[q] < best[q]) best[q] = d2[q], nearest[q] = p0 + p;
  }
}

// distance = sqrt(best), correctly rounded; the initial state never replaced: NaN (and nearest -1)
__device__ __forceinline__ float domain_result(float best, int nearest) {
  return nearest < 0 ? __uint_as_float(0x7FC00000u) : sqrtf(best);
}

// `rows` rows of Mx floats from `src` (contiguous) into LDS rows of `stride` floats, zero up to S2 = align4(Mx).
// Every thread of the workgroup calls it.
__device__ __forceinline__ void domain_stage(float* dst, const float* __restrict__ src, int rows, int Mx, int S2, int stride) {
  for (int idx = threadIdx.x; idx < rows * S2; idx += blockDim.x) {
    const int r = idx / S2, k = idx - r * S2;
    dst[r * stride + k] = k < Mx ? src[(int64_t)r * Mx + k] : 0.f;
  }
}

// the LDS of a grid kernel: the tile's mixing rows and one chunk of the reference
__host__ __device__ inline size_t domain_grid_lds_floats(int Mx) {
  return (size_t)(kTileA + kTileC) * mix_row_stride(Mx) + (size_t)kDomainChunk * align4(Mx);
}

// The latent vectors of a thread's P tile rows first, first + 4, ... (lane = anion): z = cation row + anion row,
// AddTwoTensors, the cation term first; the registers past Mx are zero.  A row past the tile's edge reads the last one.
template <int MXR, int P>
__device__ __forceinline__ void domain_latent(float (&z)[P][MXR], const float* mcat, const float* pa, int first, int nc,
                                              int Mx, int S) {
#pragma unroll
  for (int q = 0; q < P; ++q) {
    const float* pc = mcat + min(first + 4 * q, nc - 1) * S;
#pragma unroll
    for (int k4 = 0; k4 < MXR; k4 += 4) {
      f32x4_t m = {0.f, 0.f, 0.f, 0.f};
      if (k4 < Mx) m = ld4(pc + k4) + ld4(pa + k4);
      z[q][k4] = m[0], z[q][k4 + 1] = m[1], z[q][k4 + 2] = m[2], z[q][k4 + 3] = m[3];
    }
  }
}

}  // namespace impnn
