// The k best pairs of a cation x anion grid without the grid (include/impnn.h: impnn_head_grid_topk,
// impnn_transfer_head_grid_topk).
//
// The selecting kernels are the grid kernels of grid_device.h with the GridSelect pack: the same tile arithmetic, so a
// selected value has the bits impnn_head_grid / impnn_transfer_head_grid write for that pair, and where those store a
// tile these test its values against the k-th best entry so far and append the survivors to a list in LDS
// (ballot, popcount, one integer LDS atomic per wave).  A list that cannot take another tile is sorted as 64-bit
// integers (bitonic) and cut to k.  Workgroups are persistent (tiles g, g + G, ...) and leave k sorted entries per
// temperature in the workspace; grid_select_merge_kernel, one workgroup per temperature, runs the same filter and sort
// over those G * k candidates and writes values and indices.  Entries are unique and totally ordered, so the result is
// the exact top k whatever the schedule.  No float atomics, no global atomics, no C x A buffer.
//
// The _where entries run the same kernels with the GridSelectWhere pack: a pair competes only where its bit of the
// packed mask is set (the bit joins `live`), and a persistent workgroup first loads its tile's mask words (at most 32)
// and passes over a tile without a set bit before it loads a row - a block-uniform decision (__syncthreads_or), so a
// selective constraint costs about the tiles it leaves.  The plain entries keep their own instantiations.
#include "grid_device.h"

namespace impnn {

namespace {

constexpr int kSelectGroups = 512;   // default workgroups: two per compute unit of the MI355X (256 CUs)
constexpr int kMergeRound = 1024;    // candidates per round of the merge: 4 per thread

__global__ __launch_bounds__(256) void grid_select_merge_kernel(const unsigned long long* __restrict__ ws, int G, int nT,
                                                                int k, int cap, int largest, uint32_t A,
                                                                float* __restrict__ values, int32_t* __restrict__ cation,
                                                                int32_t* __restrict__ anion) {
  extern __shared__ __align__(16) float sm[];
  const int tid = threadIdx.x, t = blockIdx.x;
  const SelectList s = select_list(sm, 1, cap, 0);
  if (tid == 0) *s.count = 0, *s.bound = kSelectNone;
  __syncthreads();
  const int64_t n = (int64_t)G * k;
  for (int64_t first = 0; first < n; first += kMergeRound) {
    select_make_room(s, k, cap, kMergeRound);
    const unsigned long long bound = *s.bound;
    for (int q = 0; q < kMergeRound / 256; ++q) {
      const int64_t e = first + q * 256 + tid;
      unsigned long long entry = kSelectNone;
      if (e < n) entry = ws[((e / k) * nT + t) * k + e % k];
      select_offer(s, bound, entry != kSelectNone, entry);
    }
    __syncthreads();
  }
  const int kept = select_compact(s, *s.count, k);
  for (int i = tid; i < k; i += blockDim.x) {
    const unsigned long long entry = s.buf[i];
    const uint32_t pair = (uint32_t)entry;
    const bool used = i < kept;
    values[(int64_t)t * k + i] = select_value(used ? (uint32_t)(entry >> 32) : 0xFFFFFFFFu, largest != 0);
    cation[(int64_t)t * k + i] = used ? (int32_t)(pair / A) : -1;
    anion[(int64_t)t * k + i] = used ? (int32_t)(pair % A) : -1;
  }
}

int64_t tiles_of(int family, int C, int A, int* tiles_a) {
  const int tc = family == 0 ? kTileC : kTgTileC, ta = family == 0 ? kTileA : kTgTileA;
  *tiles_a = (A + ta - 1) / ta;
  return (int64_t)((C + tc - 1) / tc) * *tiles_a;
}

template <class Kernel>
void raise_lds_limit(Kernel kern, size_t lds) {
  if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

}  // namespace

int grid_topk_workgroups(int family, int C, int A, int workgroups) {
  int tiles_a;
  const int64_t tiles = tiles_of(family, C, A, &tiles_a);
  const int64_t want = workgroups > 0 ? workgroups : kSelectGroups;
  return (int)(want < tiles ? want : tiles);
}

size_t grid_topk_workspace_bytes(int family, int C, int A, int nT, int k, int workgroups) {
  return sizeof(unsigned long long) * (size_t)grid_topk_workgroups(family, C, A, workgroups) * (nT > 0 ? nT : 1) * k;
}

int launch_grid_topk(const GridTopkCall& c) {
  int tiles_a;
  const int64_t tiles = tiles_of(c.family, c.C, c.A, &tiles_a);  // < 2^32 / 16 + 2^26: C * A < 2^32
  const int G = grid_topk_workgroups(c.family, c.C, c.A, c.workgroups);
  const int nT = c.nT > 0 ? c.nT : 1;
  const int cap = select_capacity(c.k, c.family == 0 ? kTilePairs : kTgTileC * kTgTileA);
  unsigned long long* ws = static_cast<unsigned long long*>(c.workspace);
  const GridSelect sel{ws, c.k, cap, c.largest, (unsigned)tiles};
  GridSelectWhere selw;
  static_cast<GridSelect&>(selw) = sel;
  selw.where = c.where, selw.W = mask_row_words(c.A);
  const size_t where_lds = c.masked ? sizeof(uint32_t) * kWhereTileWords : 0;  // the tile's mask words, behind the lists
  const size_t sel_lds = select_lds_bytes(nT, cap) + where_lds;  // <= 64.2 KiB (4 temperatures, k = 1024)
  if (c.family == 0) {
    const float* tail = c.w + 2 * ((size_t)c.D * c.F + c.F) + 2 * ((size_t)c.F * c.Mx + c.Mx);
    const size_t lds = sizeof(float) * grid_lds_floats(c.kind, c.nT, c.F, c.Mx) + sel_lds;  // <= 98.2 KiB
#define IMPNN_SELECT_AS(KIND, MXR, PACK, pack)                                                                        \
  do {                                                                                                                \
    raise_lds_limit(head_grid_kernel<KIND, MXR, PACK>, lds);                                                          \
    head_grid_kernel<KIND, MXR, PACK><<<G, 256, lds, c.stream>>>(c.mix_cat, c.mix_an, c.T, tail, nullptr, nullptr,    \
                                                                 c.C, c.A, c.nT, c.F, c.Mx, tiles_a, pack);           \
  } while (0)
#define IMPNN_SELECT(KIND, MXR)                                                                                       \
  do {                                                                                                                \
    if (c.masked)                                                                                                     \
      IMPNN_SELECT_AS(KIND, MXR, GridSelectWhere, selw);                                                              \
    else                                                                                                              \
      IMPNN_SELECT_AS(KIND, MXR, GridSelect, sel);                                                                    \
  } while (0)
    if (c.kind == 0)
      IMPNN_SELECT(0, 0);
    else if (c.Mx <= 32)
      IMPNN_SELECT(1, 32);
    else
      IMPNN_SELECT(1, 64);
#undef IMPNN_SELECT
#undef IMPNN_SELECT_AS
  } else {
    const size_t lds = sizeof(float) * kTgLdsFloats + sel_lds;  // <= 59.5 KiB
    if (c.masked) {
      raise_lds_limit(transfer_grid_kernel<GridSelectWhere>, lds);
      transfer_grid_kernel<GridSelectWhere><<<G, 256, lds, c.stream>>>(c.mix_cat, c.mix_an, c.w, nullptr, c.C, c.A, tiles_a, selw);
    } else {
      raise_lds_limit(transfer_grid_kernel<GridSelect>, lds);
      transfer_grid_kernel<GridSelect><<<G, 256, lds, c.stream>>>(c.mix_cat, c.mix_an, c.w, nullptr, c.C, c.A, tiles_a, sel);
    }
  }
  if (int rc = check_launch(c.family == 0 ? "head_grid_topk" : "transfer_head_grid_topk")) return rc;
  const int mcap = select_capacity(c.k, kMergeRound);
  grid_select_merge_kernel<<<nT, 256, select_lds_bytes(1, mcap), c.stream>>>(ws, G, nT, c.k, mcap, c.largest, (uint32_t)c.A,
                                                                           c.values, c.cation, c.anion);
  return check_launch("grid_select_merge");
}

}  // namespace impnn
