// The k-th best pair of a cation x anion grid, and the k best as a packed pair mask, without the grid (include/impnn.h:
// impnn_head_grid_rank, impnn_transfer_head_grid_rank).
//
// An entry (key << 32) | pair is a unique 64-bit integer under the selection's total order, so the k-th entry is an
// exact order statistic and a most-significant-digit radix select finds it: kRankDigitBits bits a pass, four passes
// over the key and one per byte that pairs - 1 needs (the index bytes above are zero in every entry).  A pass is the
// grid kernel of grid_device.h with the GridRank pack - the same tile arithmetic, so an entry has the bits
// impnn_head_grid / impnn_transfer_head_grid write for its pair - persistent over tiles: where those store a tile it
// counts the entries that share the digits found so far by their next digit, into an LDS histogram (integer LDS
// atomics, aggregated inside a wave first), and leaves its counters in hist [workgroups][planes][256].  Then
// grid_rank_step_kernel, one workgroup per plane: thread b sums bin b over the workgroups, a scan finds the bin that
// holds the remaining rank, and the plane's state in the workspace takes the digit.  The next pass reads the state from
// device memory: a call enqueues all of its launches without a host round trip.  Every slot of hist has one writer,
// nothing is zeroed first, nothing is a global or a float atomic: the result does not depend on workgroups or tile order.
// After the last pass the state's bound is the k-th entry (kSelectNone when fewer than k pairs compete), and the mask
// form (GridMaskRank, one tile per workgroup) sets entry <= bound: exactly the first min(k, competing) pairs.
#include "grid_device.h"

namespace impnn {

namespace {

constexpr int kRankGroups = 256;  // default workgroups: one per compute unit of the MI355X

// rank0 = k - 1, read by the first pass only; `A` turns the pair of the last pass into indices
__global__ __launch_bounds__(kRankBins) void grid_rank_step_kernel(const uint32_t* __restrict__ hist, int G, int planes,
                                                                   RankState* __restrict__ state, int shift, int last,
                                                                   unsigned long long rank0, int largest, uint32_t A,
                                                                   float* __restrict__ values, int32_t* __restrict__ cation,
                                                                   int32_t* __restrict__ anion, int64_t* __restrict__ count) {
  __shared__ unsigned long long scan[kRankBins];
  const int b = threadIdx.x, t = blockIdx.x;
  const bool first = shift + kRankDigitBits == 64;
  unsigned long long mine = 0;
  for (int g = 0; g < G; ++g) mine += hist[((size_t)g * planes + t) * kRankBins + b];
  scan[b] = mine;
  __syncthreads();
  for (int step = 1; step < kRankBins; step <<= 1) {  // inclusive scan
    const unsigned long long below = b >= step ? scan[b - step] : 0;
    __syncthreads();
    scan[b] += below;
    __syncthreads();
  }
  const unsigned long long before = scan[b] - mine, total = scan[kRankBins - 1];
  RankState* s = state + t;
  // the k-th entry, or none: the plane's outputs and the bound the mask form reads
  auto finish = [&](unsigned long long entry) {
    const bool none = entry == kSelectNone;
    const uint32_t pair = (uint32_t)entry;
    s->bound = entry;
    values[t] = select_value(none ? 0xFFFFFFFFu : (uint32_t)(entry >> 32), largest != 0);
    cation[t] = none ? -1 : (int32_t)(pair / A);
    anion[t] = none ? -1 : (int32_t)(pair % A);
    count[t] = (int64_t)s->count;
  };
  if (first) {  // the bins' total is the number of competing pairs; fewer than k: latched, later passes leave the state alone
    const bool none = rank0 >= total;
    if (b == 0) s->count = (uint32_t)total, s->none = none, s->bound = kSelectNone;
    if (none ? b == 0 : before <= rank0 && rank0 < before + mine)
      s->prefix = none ? 0ull : (unsigned long long)b << shift, s->rank = none ? 0ull : rank0 - before;
    return;  // (never the last pass: the key alone has four digits)
  }
  const bool none = s->none != 0;  // (no thread writes it in this launch)
  const unsigned long long rank = s->rank;
  __syncthreads();  // every thread has read the rank before the bin's thread replaces it
  if (none) {
    if (last && b == 0) finish(kSelectNone);
  } else if (before <= rank && rank < before + mine) {  // one thread: rank < total, by the pass before
    const unsigned long long prefix = s->prefix | ((unsigned long long)b << shift);
    s->prefix = prefix, s->rank = rank - before;
    if (last) finish(prefix);
  }
}

}  // namespace

int grid_rank_passes(int64_t pairs) {
  int passes = 32 / kRankDigitBits;
  for (uint64_t top = pairs > 0 ? (uint64_t)pairs - 1 : 0; top != 0; top >>= kRankDigitBits) ++passes;
  return passes;
}

int grid_rank_workgroups(int family, int C, int A, int workgroups) {
  const int64_t tiles = grid_tiles(family, C, A).count();
  const int64_t want = workgroups > 0 ? workgroups : kRankGroups;
  return (int)(want < tiles ? want : tiles);
}

size_t grid_rank_workspace_bytes(int family, int C, int A, int nT, int workgroups) {
  const size_t planes = nT > 0 ? nT : 1;
  if (C == 0 || A == 0) return 0;
  return planes * sizeof(RankState) + sizeof(uint32_t) * (size_t)grid_rank_workgroups(family, C, A, workgroups) * planes * kRankBins;
}

int launch_grid_rank(const GridRankCall& c) {
  const GridOperands& g = c.g;
  const int64_t tiles = grid_tiles(g.family, g.C, g.A).count();  // < 2^32 / 256 + 2^27: C * A < 2^32
  const int G = grid_rank_workgroups(g.family, g.C, g.A, c.workgroups);
  const int planes = g.nT > 0 ? g.nT : 1;
  const int W = mask_row_words(g.A);
  RankState* state = static_cast<RankState*>(c.workspace);
  uint32_t* hist = reinterpret_cast<uint32_t*>(state + planes);
  const size_t where_lds = c.where ? sizeof(uint32_t) * kWhereTileWords : 0;  // the tile's mask words, behind the histogram
  const char* what = g.family == 0 ? "head_grid_rank" : "transfer_head_grid_rank";
  const int passes = grid_rank_passes((int64_t)g.C * g.A);
  const int key_passes = 32 / kRankDigitBits;
  for (int p = 0; p < passes; ++p) {
    // the key's digits from bit 56 down to bit 32, then the index's from its highest non-zero byte down to bit 0
    const int shift = p < key_passes ? 64 - kRankDigitBits * (p + 1) : kRankDigitBits * (passes - 1 - p);
    const GridRank rank{state, hist, c.where, W, shift, c.largest, (unsigned)tiles};
    launch_grid_kernel(g, G, rank_lds_bytes(planes) + where_lds, rank);  // G persistent workgroups; <= 47.1 KiB of LDS
    if (int rc = check_launch(what)) return rc;
    grid_rank_step_kernel<<<planes, kRankBins, 0, g.stream>>>(hist, G, planes, state, shift, p == passes - 1,
                                                              (unsigned long long)(c.k - 1), c.largest, (uint32_t)g.A,
                                                              c.values, c.cation, c.anion, c.count);
    if (int rc = check_launch("grid_rank_step")) return rc;
  }
  if (c.mask_words) {
    const GridMaskRank mask{c.mask_words, state, c.where, W, c.largest};
    launch_grid_kernel(g, (unsigned)tiles, where_lds, mask);  // a workgroup per tile
    if (int rc = check_launch(what)) return rc;
  }
  return IMPNN_OK;
}

}  // namespace impnn
