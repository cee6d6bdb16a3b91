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

}  // namespace

int grid_topk_workgroups(int family, int C, int A, int workgroups) {
  const int64_t tiles = grid_tiles(family, C, A).count();
  const int64_t want = workgroups > 0 ? workgroups : kSelectGroups;
  return (int)(want < tiles ? want : tiles);
}

size_t grid_topk_workspace_bytes(int family, int C, int A, int nT, int k, int workgroups) {
  return sizeof(unsigned long long) * (size_t)grid_topk_workgroups(family, C, A, workgroups) * (nT > 0 ? nT : 1) * k;
}

int launch_grid_topk(const GridTopkCall& c) {
  const GridOperands& g = c.g;
  const int64_t tiles = grid_tiles(g.family, g.C, g.A).count();  // < 2^32 / 16 + 2^26: C * A < 2^32
  const int G = grid_topk_workgroups(g.family, g.C, g.A, c.workgroups);
  const int nT = g.nT > 0 ? g.nT : 1;
  const int cap = select_capacity(c.k, g.family == 0 ? kTilePairs : kTgTileC * kTgTileA);
  unsigned long long* ws = static_cast<unsigned long long*>(c.workspace);
  const GridSelect sel{ws, c.k, cap, c.largest, (unsigned)tiles};
  // behind the tile's regions: the lists, <= 64.2 KiB (4 temperatures, k = 1024), then the tile's mask words; with the
  // tile <= 98.2 KiB (head grid), 59.5 KiB (transfer grid): the launcher raises the kernel's dynamic-LDS limit
  const size_t sel_lds = select_lds_bytes(nT, cap);
  if (c.masked) {
    GridSelectWhere selw;
    static_cast<GridSelect&>(selw) = sel;
    selw.where = c.where, selw.W = mask_row_words(g.A);
    launch_grid_kernel(g, G, sel_lds + sizeof(uint32_t) * kWhereTileWords, selw);
  } else {
    launch_grid_kernel(g, G, sel_lds, sel);
  }
  if (int rc = check_launch(g.family == 0 ? "head_grid_topk" : "transfer_head_grid_topk")) return rc;
  return launch_grid_topk_merge(ws, G, nT, c.k, c.largest, g.A, c.values, c.cation, c.anion, g.stream);
}

int launch_grid_topk_merge(const unsigned long long* ws, int G, int nT, int k, int largest, int A, float* values,
                           int32_t* cation, int32_t* anion, hipStream_t s) {
  const int mcap = select_capacity(k, kMergeRound);
  grid_select_merge_kernel<<<nT, 256, select_lds_bytes(1, mcap), s>>>(ws, G, nT, k, mcap, largest, (uint32_t)A, values,
                                                                    cation, anion);
  return check_launch("grid_select_merge");
}

}  // namespace impnn
