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

void tiles_of(int family, int C, int A, int* tiles_c, int* tiles_a) {
  const int tc = family == 0 ? kTileC : kTgTileC, ta = family == 0 ? kTileA : kTgTileA;
  *tiles_c = (C + tc - 1) / tc;
  *tiles_a = (A + ta - 1) / ta;
}

}  // namespace

size_t grid_partners_workspace_bytes(int family, int C, int A, int nT, int m) {
  int tiles_c, tiles_a;
  tiles_of(family, C, A, &tiles_c, &tiles_a);
  return sizeof(unsigned long long) * (size_t)(nT > 0 ? nT : 1) * m * ((size_t)tiles_a * C + (size_t)tiles_c * A);
}

int launch_grid_partners(const GridPartnersCall& c) {
  int tiles_c, tiles_a;
  tiles_of(c.family, c.C, c.A, &tiles_c, &tiles_a);
  const int tiles = tiles_c * tiles_a;  // < 2^32 / 256 + 2^27: C * A < 2^32
  const int nT = c.nT > 0 ? c.nT : 1;
  unsigned long long* rows = static_cast<unsigned long long*>(c.workspace);
  unsigned long long* cols = rows + (size_t)nT * tiles_a * c.C * c.m;
  const GridPartners sel{rows, cols, c.m, c.largest};
  GridPartnersWhere selw;
  static_cast<GridPartners&>(selw) = sel;
  selw.where = c.where, selw.W = mask_row_words(c.A);
  const size_t where_lds = c.where ? sizeof(uint32_t) * kWhereTileWords : 0;  // the tile's mask words, behind its regions
  if (c.family == 0) {
    const float* tail = c.w + 2 * ((size_t)c.D * c.F + c.F) + 2 * ((size_t)c.F * c.Mx + c.Mx);
    const size_t lds = sizeof(float) * grid_lds_floats(c.kind, c.nT, c.F, c.Mx) + where_lds;  // as impnn_head_grid
#define IMPNN_PARTNERS_AS(KIND, MXR, PACK, pack)                                                                      \
  head_grid_kernel<KIND, MXR, PACK><<<tiles, 256, lds, c.stream>>>(c.mix_cat, c.mix_an, c.T, tail, nullptr, nullptr, c.C, \
                                                                   c.A, c.nT, c.F, c.Mx, tiles_a, pack)
#define IMPNN_PARTNERS(KIND, MXR)                                                                                     \
  do {                                                                                                                \
    if (c.where)                                                                                                      \
      IMPNN_PARTNERS_AS(KIND, MXR, GridPartnersWhere, selw);                                                          \
    else                                                                                                              \
      IMPNN_PARTNERS_AS(KIND, MXR, GridPartners, sel);                                                                \
  } while (0)
    if (c.kind == 0)
      IMPNN_PARTNERS(0, 0);
    else if (c.Mx <= 32)
      IMPNN_PARTNERS(1, 32);
    else
      IMPNN_PARTNERS(1, 64);
#undef IMPNN_PARTNERS
#undef IMPNN_PARTNERS_AS
  } else {
    const size_t lds = sizeof(float) * kTgLdsFloats + where_lds;
    if (c.where)
      transfer_grid_kernel<GridPartnersWhere><<<tiles, 256, lds, c.stream>>>(c.mix_cat, c.mix_an, c.w, nullptr, c.C, c.A, tiles_a, selw);
    else
      transfer_grid_kernel<GridPartners><<<tiles, 256, lds, c.stream>>>(c.mix_cat, c.mix_an, c.w, nullptr, c.C, c.A, tiles_a, sel);
  }
  if (int rc = check_launch(c.family == 0 ? "head_grid_partners" : "transfer_head_grid_partners")) return rc;
  const int64_t ions = (int64_t)nT * ((int64_t)c.C + c.A);
  grid_partners_merge_kernel<<<(unsigned)((ions + 255) / 256), 256, 0, c.stream>>>(
      rows, cols, tiles_a, tiles_c, c.C, c.A, nT, c.m, c.largest, c.cat_values, c.cat_partner, c.an_values, c.an_partner);
  return check_launch("grid_partners_merge");
}

}  // namespace impnn
