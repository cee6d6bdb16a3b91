// Row-restricted embedding gradient (include/impnn.h: impnn_embed_rows_bwd): the gradient of the listed rows of an
// embedding table and of no other row - what a frozen Embedding with trainable_rows hands to the optimizer.
//
//   dtable[v,:] = (accumulate ? dtable[v,:] : +0.0) + sum over the r with ids[r] == v of dout[r,:]     v = row_list[i]
//
// One workgroup per (listed token, tile of 64 columns), lane = column, kEmbedRowsWaves waves.  The rows are cut into
// chunks of 64; wave w takes the chunks w, w + kEmbedRowsWaves, ...: its lanes read the chunk's 64 ids with one load, a
// ballot marks the rows that hold the token, and the wave adds those rows of dout to its partial in ascending row order.
// The partials of the waves meet in LDS and wave 0 adds them in wave order, then the table row's old value when the
// call accumulates.  So the order of the sum is a function of (rows) alone - not of the schedule, and there is no float
// atomic: the same call gives the same bits.  Rows of dtable outside the list are never addressed.
//
// A token's workgroup returns at once when its id lies outside the vocabulary or an earlier entry of the list holds the
// same id (each listed row is written by exactly one workgroup, whatever the list holds); an ids[r] outside the
// vocabulary equals no listed token, so it is padding.  ids == NULL is the identity (row r holds token r).
#include "common.h"

namespace impnn {
namespace {

constexpr int kEmbedRowsWaves = 8;
constexpr int kEmbedRowsTile = 64;  // columns per workgroup: one per lane

__global__ __launch_bounds__(64 * kEmbedRowsWaves) void embed_rows_bwd_kernel(
    const int32_t* __restrict__ ids, const float* __restrict__ dout, const int32_t* __restrict__ row_list,
    float* __restrict__ dtable, long long rows, int vocab, int dim, int n_listed, int tiles, int accumulate) {
  __shared__ float partial[kEmbedRowsWaves][kEmbedRowsTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x / tiles, tile = blockIdx.x - i * tiles;  // (i < n_listed by the grid's size)
  const int v = row_list[i];
  if (v < 0 || v >= vocab) return;  // (uniform for the workgroup)
  for (int j = lane; j - lane < i; j += 64) {  // an earlier entry with the same id owns the row
    const bool same = j < i && row_list[j] == v;
    if (__ballot(same)) return;
  }
  const int col = tile * kEmbedRowsTile + lane;
  const bool live = col < dim;
  float acc = 0.f;
  const long long chunks = (rows + 63) >> 6;
  for (long long c = wave; c < chunks; c += kEmbedRowsWaves) {
    const long long r = (c << 6) + lane;
    const bool hit = r < rows && (ids ? ids[r] == v : r == (long long)v);
    unsigned long long mask = __ballot(hit);
    const float* base = dout + (c << 6) * dim + col;
    while (mask) {  // four rows a turn: the loads leave together, the adds keep the ascending order
      float x[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        x[k] = 0.f;
        if (mask) {
          const int b = __builtin_ctzll(mask);
          mask &= mask - 1;
          if (live) x[k] = base[(long long)b * dim];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += x[k];  // (+0.0 for a turn's missing rows: acc starts at +0.0, its bits stay)
    }
  }
  partial[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && live) {
    float sum = partial[0][lane];
#pragma unroll
    for (int w = 1; w < kEmbedRowsWaves; ++w) sum += partial[w][lane];
    float* out = dtable + (long long)v * dim + col;
    *out = (accumulate ? *out : 0.f) + sum;
  }
}

}  // namespace

int launch_embed_rows_bwd(const int32_t* ids, const float* dout, const int32_t* row_list, int n_listed, float* dtable,
                          int64_t rows, int vocab, int dim, int accumulate, hipStream_t s) {
  const int64_t tiles = ((int64_t)dim + kEmbedRowsTile - 1) / kEmbedRowsTile;
  const int64_t blocks = tiles * n_listed;
  if (blocks > 0x7fffffffLL)
    return fail(IMPNN_E_UNSUPPORTED, "embed_rows_bwd: %lld workgroups (n_listed x ceil(dim / 64) < 2^31 per call)",
                (long long)blocks);
  embed_rows_bwd_kernel<<<(unsigned)blocks, 64 * kEmbedRowsWaves, 0, s>>>(ids, dout, row_list, dtable, (long long)rows,
                                                                          vocab, dim, n_listed, (int)tiles, accumulate);
  return check_launch("embed_rows_bwd");
}

}  // namespace impnn
