// Each ion's m best partners over a cation x anion grid without the grid (include/impnn.h: impnn_head_grid_partners,
// impnn_transfer_head_grid_partners).
//
// The partner-selecting kernels are the grid kernels of grid_device.h with the GridPartners pack: the same tile
// arithmetic, so a selected value has the bits impnn_head_grid / impnn_transfer_head_grid write for that pair, one tile
// per workgroup, and where those store a tile these select from its values in LDS.  A tile row is a wave's 64 lanes
// (transfer: a 32-lane half): m rounds of a 64-bit minimum across the row, the winner retiring after each.  A tile
// column is one thread that walks the tile's rows and keeps the m smallest entries in registers.  Every workspace slot
// (rows [nT][tiles_a][C][m], cols [nT][tiles_c][A][m]) has exactly one writing workgroup - a ragged tile writes
// kSelectNone where it has no pair, and so does a tile the mask lets its workgroup pass over - so nothing is zeroed
// first and nothing is atomic.  grid_partners_merge_kernel, one thread per (temperature, ion), keeps the m smallest of
// that ion's tiles x m candidates.  The entries are the selection's ((key << 32) | pair, unique, compared unsigned), so
// the result is exact and independent of tile order, launch and host tiling.
#include "grid_device.h"

namespace impnn {

namespace {

// ion < C: cation `ion`, its candidates in rows; otherwise anion ion - C, in cols
__global__ __launch_bounds__(256) void grid_partners_merge_kernel(const unsigned long long* __restrict__ rows,
                                                                  const unsigned long long* __restrict__ cols,
                                                                  int tiles_a, int tiles_c, int C, int A, int nT, int m,
                                                                  int largest, float* __restrict__ cat_values,
                                                                  int32_t* __restrict__ cat_partner,
                                                                  float* __restrict__ an_values,
                                                                  int32_t* __restrict__ an_partner) {
  const int64_t n = (int64_t)nT * ((int64_t)C + A);
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n) return;
  const int t = (int)(id / ((int64_t)C + A));
  const int ion = (int)(id - (int64_t)t * ((int64_t)C + A));
  const bool cation = ion < C;
  const int i = cation ? ion : ion - C, tiles = cation ? tiles_a : tiles_c, M = cation ? C : A;
  const unsigned long long* src = cation ? rows : cols;
  PartnersBest best;
  for (int tile = 0; tile < tiles; ++tile) {
    const unsigned long long* cand = src + (((size_t)t * tiles + tile) * M + i) * m;
    for (int s = 0; s < m; ++s) best.offer(cand[s]);
  }
  float* values = (cation ? cat_values : an_values) + ((size_t)t * M + i) * m;
  int32_t* partner = (cation ? cat_partner : an_partner) + ((size_t)t * M + i) * m;
#pragma unroll
  for (int s = 0; s < kPartnersMaxM; ++s)
    if (s < m) {
      const unsigned long long entry = best.e[s];
      const uint32_t pair = (uint32_t)entry;
      const bool used = entry != kSelectNone;
      values[s] = select_value(used ? (uint32_t)(entry >> 32) : 0xFFFFFFFFu, largest != 0);
      partner[s] = !used ? -1 : (int32_t)(cation ? pair % (uint32_t)A : pair / (uint32_t)A);
    }
}

}  // namespace

size_t grid_partners_workspace_bytes(int family, int C, int A, int nT, int m) {
  const GridTiles tiles = grid_tiles(family, C, A);
  return sizeof(unsigned long long) * (size_t)(nT > 0 ? nT : 1) * m * ((size_t)tiles.a * C + (size_t)tiles.c * A);
}

int launch_grid_partners(const GridPartnersCall& c) {
  const GridOperands& g = c.g;
  const GridTiles tiles = grid_tiles(g.family, g.C, g.A);  // < 2^32 / 256 + 2^27 of them: C * A < 2^32
  const int nT = g.nT > 0 ? g.nT : 1;
  unsigned long long* rows = static_cast<unsigned long long*>(c.workspace);
  unsigned long long* cols = rows + (size_t)nT * tiles.a * g.C * c.m;
  const GridPartners sel{rows, cols, c.m, c.largest};
  if (c.where) {  // the tile's mask words sit behind its regions
    GridPartnersWhere selw;
    static_cast<GridPartners&>(selw) = sel;
    selw.where = c.where, selw.W = mask_row_words(g.A);
    launch_grid_kernel(g, (unsigned)tiles.count(), sizeof(uint32_t) * kWhereTileWords, selw);
  } else {
    launch_grid_kernel(g, (unsigned)tiles.count(), 0, sel);
  }
  if (int rc = check_launch(g.family == 0 ? "head_grid_partners" : "transfer_head_grid_partners")) return rc;
  const int64_t ions = (int64_t)nT * ((int64_t)g.C + g.A);
  grid_partners_merge_kernel<<<(unsigned)((ions + 255) / 256), 256, 0, g.stream>>>(
      rows, cols, tiles.a, tiles.c, g.C, g.A, nT, c.m, c.largest, c.cat_values, c.cat_partner, c.an_values, c.an_partner);
  return check_launch("grid_partners_merge");
}

}  // namespace impnn
