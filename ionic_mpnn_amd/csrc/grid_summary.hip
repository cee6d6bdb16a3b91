// Per-ion statistics of a cation x anion grid without the grid (include/impnn.h: impnn_head_grid_summary,
// impnn_transfer_head_grid_summary, impnn_deep_ensemble_grid_summary, impnn_transfer_mc_grid_summary).
//
// The summary kernels are the grid kernels of grid_device.h (and transfer_mc_grid.hip) with the GridSummary pack: the
// same tile arithmetic, so a summarised value has the bits the materialising entry writes for that pair, one tile per
// workgroup, and where those store a tile these reduce it.  A tile row is a wave's 64 lanes (transfer: a 32-lane half):
// the count is one ballot popcount, the two double sums a butterfly over the row's lanes (the adjacent-pair tree), the
// least and the greatest value two 32-bit key minima.  A tile column is one thread that walks the tile's rows in
// ascending order.  Every workspace slot (rows [planes][tiles_a][C], cols [planes][tiles_c][A], 32 bytes each) has
// exactly one writing workgroup - a tile the mask lets its workgroup pass over writes the record of no pair - so nothing
// is zeroed first and nothing is atomic.  grid_summary_merge_kernel, one thread per (plane, ion), adds that ion's partial
// records in ascending tile order; an anion's sum may continue from the record an earlier range of cations left.  Every
// sum has one stated order, so the result's bits do not depend on the grid's size, the host tiling (at multiples of 16
// cations) or whether a masked-out tile was skipped or computed.
#include "grid_device.h"

namespace impnn {

namespace {

// ion < C: cation `ion`, its partial records in rows; otherwise anion ion - C, in cols
__global__ __launch_bounds__(256) void grid_summary_merge_kernel(const SummaryRecord* __restrict__ rows,
                                                                 const SummaryRecord* __restrict__ cols, int tiles_a,
                                                                 int tiles_c, int C, int A, int planes, int carry,
                                                                 uint32_t* __restrict__ cat_count,
                                                                 double* __restrict__ cat_sums,
                                                                 float* __restrict__ cat_range,
                                                                 uint32_t* __restrict__ an_count,
                                                                 double* __restrict__ an_sums,
                                                                 float* __restrict__ an_range) {
  const int64_t n = (int64_t)planes * ((int64_t)C + A);
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n) return;
  const int t = (int)(id / ((int64_t)C + A));
  const int ion = (int)(id - (int64_t)t * ((int64_t)C + A));
  const bool cation = ion < C;
  const int i = cation ? ion : ion - C, tiles = cation ? tiles_a : tiles_c, M = cation ? C : A;
  const SummaryRecord* src = cation ? rows : cols;
  const size_t at = (size_t)t * M + i;
  uint32_t* count = (cation ? cat_count : an_count) + at;
  double* sums = (cation ? cat_sums : an_sums) + 2 * at;
  float* range = (cation ? cat_range : an_range) + 2 * at;
  SummarySum sum;
  if (!cation && carry) {  // the record of the earlier ranges of cations
    sum.s = sums[0], sum.q = sums[1], sum.n = count[0];
    sum.lo = select_key(range[0], false), sum.hi = select_key(range[1], true);
  }
  for (int tile = 0; tile < tiles; ++tile) sum.add(src[((size_t)t * tiles + tile) * M + i]);
  count[0] = sum.n;
  sums[0] = sum.s, sums[1] = sum.q;
  range[0] = select_value(sum.lo, false), range[1] = select_value(sum.hi, true);
}

}  // namespace

int grid_summary_max_planes(int family, int M) {
  if (family == 0) return head_grid_max_temperatures();
  if (family == 2) return M < 1 || M > kEnsembleMaxMembers ? 0 : ensemble_summary_max_temperatures(M, head_grid_max_temperatures());
  return 1;  // the transfer grids have one plane
}

size_t grid_summary_workspace_bytes(int family, int C, int A, int planes) {
  const GridTiles tiles = grid_tiles(family, C, A);
  return sizeof(SummaryRecord) * (size_t)planes * ((size_t)tiles.a * C + (size_t)tiles.c * A);
}

int launch_grid_summary(const GridSummaryCall& c) {
  const GridOperands& g = c.g;
  static const char* const names[4] = {"head_grid_summary", "transfer_head_grid_summary", "ensemble_grid_summary",
                                       "transfer_mc_grid_summary"};
  const GridTiles tiles = grid_tiles(g.family, g.C, g.A);
  if (int rc = grid_tiles_fit(names[g.family], tiles)) return rc;
  const int planes = g.nT > 0 ? g.nT : 1;
  SummaryRecord* rows = static_cast<SummaryRecord*>(c.workspace);
  SummaryRecord* cols = rows + (size_t)planes * tiles.a * g.C;
  const GridSummary sel{rows, cols, c.where, mask_row_words(g.A)};
  const unsigned groups = (unsigned)tiles.count();
  const size_t words = sizeof(uint32_t) * kWhereTileWords;  // the tile's mask words sit behind its regions
  if (g.family == 0)
    launch_grid_family<0>(g, groups, words, GridOut{}, sel);
  else if (g.family == 1)
    launch_grid_family<1>(g, groups, words, GridOut{}, sel);
  else if (g.family == 2)
    launch_grid_family<2>(g, groups, words, GridOut{}, sel);
  else
    launch_transfer_mc_grid_summary_tiles(g, groups, sel);
  if (int rc = check_launch(names[g.family])) return rc;
  const int64_t ions = (int64_t)planes * ((int64_t)g.C + g.A);
  grid_summary_merge_kernel<<<(unsigned)((ions + 255) / 256), 256, 0, g.stream>>>(
      rows, cols, tiles.a, tiles.c, g.C, g.A, planes, c.carry, c.cat_count, c.cat_sums, c.cat_range, c.an_count, c.an_sums,
      c.an_range);
  return check_launch("grid_summary_merge");
}

}  // namespace impnn
