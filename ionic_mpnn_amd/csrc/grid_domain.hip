// The applicability domain of a screen (include/impnn.h: impnn_domain_grid, impnn_domain_grid_mask, impnn_domain_rows):
// how far a pair's latent vector z(i, j) = mix_cat[i] + mix_an[j] - the head kernels' `mixed` - lies from the nearest
// row of a reference set, as a (C, A) plane, as a packed pair mask, or for explicit query rows.
//
// The grid kernels keep the head grid's tile (16 cations x 64 anions, 256 threads, lane = anion, a wave walks the
// tile's cations), so a mask word still has one owning workgroup and mask_store_ballot / mix_row_stride serve as they
// do there.  A thread holds the latent vectors of kDomainRegs / MXR of its wave's tile rows in registers (4 at Mx <= 32,
// 2 above) and the reference streams through LDS in chunks of kDomainChunk rows: a row's address is wave-uniform, so
// every ds_read_b128 is a broadcast, and one row read serves all of the thread's pairs.  domain_scan is the one
// definition of the inner loop: an element has the same bits whichever entry produced it.
//
// domain_device.h holds that loop, the staging of rows with zero pads and the result, shared with grid_diverse.hip.
#include "domain_device.h"

namespace impnn {
namespace {

constexpr int kDomainRowsBlock = 64; // queries per workgroup of the rows form: one wave

// Where a grid launch writes.  The materialising form: distance (C, A) and nearest (C, A) or null; the mask form: words
// (C, W), bit = lo <= distance && distance <= hi.
struct DomainOut {
  float* distance;
  int32_t* nearest;
  uint32_t* words;
  float lo, hi;
  int W;
};

// MXR = 32 or 64 registers hold a pair's latent vector; a wave's four tile rows take 4 / P passes over the reference.
template <int MXR, bool MASK>
__global__ __launch_bounds__(256) void domain_grid_kernel(const float* __restrict__ mix_cat,
                                                          const float* __restrict__ mix_an,
                                                          const float* __restrict__ ref, DomainOut out, int C, int A,
                                                          int R, int Mx, int tiles_a) {
  extern __shared__ __align__(16) float sm[];
  constexpr int P = kDomainRegs / MXR;
  const int S = mix_row_stride(Mx), S2 = (int)align4(Mx);
  float* man = sm;                  // [kTileA][S]
  float* mcat = man + kTileA * S;   // [kTileC][S]
  float* chunk = mcat + kTileC * S; // [kDomainChunk][S2]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c0 = (int)(blockIdx.x / tiles_a) * kTileC, a0 = (int)(blockIdx.x % tiles_a) * kTileA;
  const int nc = min(kTileC, C - c0), na = min(kTileA, A - a0);

  // the tile's mixing rows: contiguous in global memory, padded rows in LDS, the pads of a quad zero
  domain_stage(man, mix_an + (int64_t)a0 * Mx, na, Mx, S2, S);
  domain_stage(mcat, mix_cat + (int64_t)c0 * Mx, nc, Mx, S2, S);
  __syncthreads();

  const float* pa = man + min(lane, na - 1) * S;  // a lane past the grid's edge computes its neighbour's pair, unstored
  for (int s = 0; s < 4 / P; ++s) {
    const int first = wave + 4 * s * P;           // the pass's rows: first, first + 4, ...
    const bool work = first < nc;                  // wave-uniform
    float z[P][MXR], best[P];
    int nearest[P], self[P];
#pragma unroll
    for (int q = 0; q < P; ++q) best[q] = __uint_as_float(0x7F800000u), nearest[q] = -1, self[q] = -1;
    domain_latent<MXR, P>(z, mcat, pa, first, nc, Mx, S);
    for (int p0 = 0; p0 < R; p0 += kDomainChunk) {
      const int n = min(kDomainChunk, R - p0);
      __syncthreads();  // the last chunk's readers
      domain_stage(chunk, ref + (int64_t)p0 * Mx, n, Mx, S2, S2);
      __syncthreads();
      if (work) domain_scan<MXR, P, false>(z, chunk, n, p0, Mx, S2, self, best, nearest);
    }
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const int ci = first + 4 * q;
      const float d = domain_result(best[q], nearest[q]);
      if constexpr (MASK) {  // a wave's 64 lanes are the 64 anions of one tile row, i.e. that row's two words
        uint32_t* row = out.words + (int64_t)(c0 + ci) * out.W + (a0 >> 5);
        mask_store_ballot(ci < nc && lane < na && out.lo <= d && d <= out.hi, ci < nc ? row : nullptr,
                          ci < nc && (a0 >> 5) + 1 < out.W ? row + 1 : nullptr);
      } else if (ci < nc && lane < na) {
        const int64_t e = (int64_t)(c0 + ci) * A + a0 + lane;
        out.distance[e] = d;
        if (out.nearest) out.nearest[e] = nearest[q];
      }
    }
  }
}

// The rows form: lane = query row, its vector in MXR registers, read as given (no sum).  EXCL: query q skips row q.
template <int MXR, bool EXCL>
__global__ __launch_bounds__(kDomainRowsBlock) void domain_rows_kernel(const float* __restrict__ zrows,
                                                                       const float* __restrict__ ref,
                                                                       float* __restrict__ distance,
                                                                       int32_t* __restrict__ nearest_out, int Q, int R,
                                                                       int Mx) {
  extern __shared__ __align__(16) float sm[];  // [kDomainChunk][S2]
  const int S2 = (int)align4(Mx);
  const int64_t query = (int64_t)blockIdx.x * kDomainRowsBlock + threadIdx.x;
  const float* src = zrows + min(query, (int64_t)Q - 1) * Mx;
  float z[1][MXR], best[1] = {__uint_as_float(0x7F800000u)};
  int nearest[1] = {-1}, self[1] = {(int)min(query, (int64_t)Q - 1)};
#pragma unroll
  for (int k = 0; k < MXR; ++k) z[0][k] = k < Mx ? src[k] : 0.f;
  for (int p0 = 0; p0 < R; p0 += kDomainChunk) {
    const int n = min(kDomainChunk, R - p0);
    __syncthreads();  // the last chunk's readers
    domain_stage(sm, ref + (int64_t)p0 * Mx, n, Mx, S2, S2);
    __syncthreads();
    domain_scan<MXR, 1, EXCL>(z, sm, n, p0, Mx, S2, self, best, nearest);
  }
  if (query < Q) {
    distance[query] = domain_result(best[0], nearest[0]);
    if (nearest_out) nearest_out[query] = nearest[0];
  }
}

}  // namespace

int domain_reference_chunk() { return kDomainChunk; }

int launch_domain_grid(const DomainGridCall& c) {
  const GridTiles tiles = grid_tiles(0, c.C, c.A);
  const char* what = c.words ? "domain_grid_mask" : "domain_grid";
  if (int rc = grid_tiles_fit(what, tiles)) return rc;
  const DomainOut out{c.distance, c.nearest, c.words, c.lo, c.hi, mask_row_words(c.A)};
  const size_t lds = sizeof(float) * domain_grid_lds_floats(c.Mx);  // at most 38 144 bytes
  auto launch = [&](auto kern) {
    kern<<<(unsigned)tiles.count(), 256, lds, c.stream>>>(c.mix_cat, c.mix_an, c.ref, out, c.C, c.A, c.R, c.Mx, tiles.a);
  };
  if (c.words)
    c.Mx <= 32 ? launch(domain_grid_kernel<32, true>) : launch(domain_grid_kernel<64, true>);
  else
    c.Mx <= 32 ? launch(domain_grid_kernel<32, false>) : launch(domain_grid_kernel<64, false>);
  return check_launch(what);
}

int launch_domain_rows(const DomainRowsCall& c) {
  const unsigned groups = (unsigned)(((int64_t)c.Q + kDomainRowsBlock - 1) / kDomainRowsBlock);
  const size_t lds = sizeof(float) * kDomainChunk * align4(c.Mx);
  auto launch = [&](auto kern) {
    kern<<<groups, kDomainRowsBlock, lds, c.stream>>>(c.z, c.ref, c.distance, c.nearest, c.Q, c.R, c.Mx);
  };
  if (c.exclude_self)
    c.Mx <= 32 ? launch(domain_rows_kernel<32, true>) : launch(domain_rows_kernel<64, true>);
  else
    c.Mx <= 32 ? launch(domain_rows_kernel<32, false>) : launch(domain_rows_kernel<64, false>);
  return check_launch("domain_rows");
}

}  // namespace impnn
