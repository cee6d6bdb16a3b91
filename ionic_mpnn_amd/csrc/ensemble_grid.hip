// A deep ensemble over a cation x anion grid (include/impnn.h: impnn_ensemble_grid, _mask, _topk, _topk_where).
//
// M members of one kind (viscosity or melting point) share the grid: member m has its own mixing rows (one
// impnn_head_ion_mix row per species, from its own encoder) and its own tail weights.  ensemble_grid_kernel
// (grid_device.h) is head_grid_kernel's tile with a loop over the members inside: it loads a member's tile rows and
// tail weights into the LDS regions the last member used, evaluates the tile's pairs with head_grid_kernel's
// arithmetic (a member's value has the bits impnn_head_grid gives it), keeps a pair's result - three VFT parameters,
// or one value - in LDS, and after the last member hands the statistic of the M values (mean, population standard
// deviation, score = mean + kappa * std; the order of every rounding step is in grid_device.h) to the form: the stores
// of impnn_head_grid, the mask words of impnn_head_grid_mask, or the running top k of impnn_head_grid_topk[_where].
// So an ensemble screen is one launch over the grid and never holds M grids.  No atomics on floats, every sum in a
// fixed order: an element's bits do not depend on the grid's size, the host tiling or the form.
//
// The kept results live in LDS for every form (12 KiB a member for viscosity, 4 KiB for melting point): the
// materialising form's stores run along the output rows, not by the thread that computed the pair, so it needs them
// there, and one storage keeps one value functor for the three forms.  What that costs is LDS: the temperatures of a
// selecting launch fall from kSelectMaxT as M grows (ensemble_select_max_temperatures), and at M = 8 a viscosity
// workgroup has a CU to itself.
#include "grid_device.h"

namespace impnn {

namespace {
constexpr int kEnsembleGridMaxT = 4096;  // as the head grid: T / 100 sits in LDS
}

int ensemble_grid_max_members() { return kEnsembleMaxMembers; }

int ensemble_grid_max_temperatures(int kind, int M) {
  if (kind != 0 || M < 1 || M > kEnsembleMaxMembers) return 0;
  return ensemble_max_temperatures(M, kEnsembleGridMaxT);
}

int ensemble_grid_topk_max_temperatures(int M) {
  return M < 1 || M > kEnsembleMaxMembers ? 0 : ensemble_select_max_temperatures(M);
}

int64_t ensemble_grid_tail_floats(int kind, int F, int Mx) { return (int64_t)ensemble_tail_floats(kind, F, Mx); }

int launch_ensemble_grid(const GridOperands& g, float* mean, float* std, float* score) {
  const GridTiles tiles = grid_tiles(2, g.C, g.A);
  if (int rc = grid_tiles_fit("ensemble_grid", tiles)) return rc;
  GridOut out;
  out.out = mean, out.std = std, out.score = score;
  launch_grid_family<2>(g, (unsigned)tiles.count(), 0, out);
  return check_launch("ensemble_grid");
}

int launch_ensemble_grid_mask(const GridMaskCall& c) {
  const GridTiles tiles = grid_tiles(2, c.g.C, c.g.A);
  if (int rc = grid_tiles_fit("ensemble_grid_mask", tiles)) return rc;
  launch_grid_family<2>(c.g, (unsigned)tiles.count(), 0, GridOut{}, GridMask{c.words, c.lo, c.hi, mask_row_words(c.g.A)});
  return check_launch("ensemble_grid_mask");
}

int launch_ensemble_grid_topk(const GridTopkCall& c) {
  const GridOperands& g = c.g;
  const int64_t tiles = grid_tiles(2, g.C, g.A).count();
  const int G = grid_topk_workgroups(2, g.C, g.A, c.workgroups);
  const int nT = g.nT > 0 ? g.nT : 1;
  const int cap = select_capacity(c.k, kTilePairs);
  unsigned long long* ws = static_cast<unsigned long long*>(c.workspace);
  const GridSelect sel{ws, c.k, cap, c.largest, (unsigned)tiles};
  const size_t sel_lds = select_lds_bytes(nT, cap);  // behind the tile's regions; api.hip holds nT to what fits
  if (c.masked) {
    GridSelectWhere selw;
    static_cast<GridSelect&>(selw) = sel;
    selw.where = c.where, selw.W = mask_row_words(g.A);
    launch_grid_family<2>(g, G, sel_lds + sizeof(uint32_t) * kWhereTileWords, GridOut{}, selw);
  } else {
    launch_grid_family<2>(g, G, sel_lds, GridOut{}, sel);
  }
  if (int rc = check_launch("ensemble_grid_topk")) return rc;
  return launch_grid_topk_merge(ws, G, nT, c.k, c.largest, g.A, c.values, c.cation, c.anion, g.stream);
}

}  // namespace impnn
