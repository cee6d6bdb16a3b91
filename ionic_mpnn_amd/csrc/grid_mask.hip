// A screen's constraint as a packed pair mask (include/impnn.h: impnn_grid_mask_row_words, impnn_head_grid_mask,
// impnn_transfer_head_grid_mask).
//
// The mask-writing kernels are the grid kernels of grid_device.h with the GridMask pack: the same tile arithmetic, so
// the tested value has the bits impnn_head_grid / impnn_transfer_head_grid write for that pair, and where those store a
// tile these test lo <= v && v <= hi, ballot, and one lane per 32-pair span stores the word.  A tile starts on a word
// boundary (64 and 32 anions), so every word has one writer and a launch writes every word of its output, pad bits 0:
// no atomics, no pre-zeroing, no C x A float buffer.
#include "grid_device.h"

namespace impnn {

int64_t grid_mask_row_words(int A) { return A > 0 ? mask_row_words(A) : 0; }

int launch_grid_mask(const GridMaskCall& c) {
  const GridTiles tiles = grid_tiles(c.g.family, c.g.C, c.g.A);
  const char* what = c.g.family == 0 ? "head_grid_mask" : "transfer_head_grid_mask";
  if (int rc = grid_tiles_fit(what, tiles)) return rc;
  launch_grid_kernel(c.g, (unsigned)tiles.count(), 0, GridMask{c.words, c.lo, c.hi, mask_row_words(c.g.A)});
  return check_launch(what);
}

}  // namespace impnn
