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
  const int tc = c.family == 0 ? kTileC : kTgTileC, ta = c.family == 0 ? kTileA : kTgTileA;
  const int tiles_a = (c.A + ta - 1) / ta;
  const int64_t tiles = (int64_t)((c.C + tc - 1) / tc) * tiles_a;
  const char* what = c.family == 0 ? "head_grid_mask" : "transfer_head_grid_mask";
  if (tiles > 0x7fffffff)
    return fail(IMPNN_E_UNSUPPORTED, "%s: %lld tiles of %d x %d pairs exceed one launch; split the cation axis", what,
                (long long)tiles, tc, ta);
  const GridMask mask{c.words, c.lo, c.hi, mask_row_words(c.A)};
  if (c.family == 0) {
    const float* tail = c.w + 2 * ((size_t)c.D * c.F + c.F) + 2 * ((size_t)c.F * c.Mx + c.Mx);
    const size_t lds = sizeof(float) * grid_lds_floats(c.kind, c.nT, c.F, c.Mx);  // as impnn_head_grid
#define IMPNN_MASK(KIND, MXR)                                                                                          \
  head_grid_kernel<KIND, MXR, GridMask><<<(int)tiles, 256, lds, c.stream>>>(c.mix_cat, c.mix_an, c.T, tail, nullptr,   \
                                                                            nullptr, c.C, c.A, c.nT, c.F, c.Mx, tiles_a, mask)
    if (c.kind == 0)
      IMPNN_MASK(0, 0);
    else if (c.Mx <= 32)
      IMPNN_MASK(1, 32);
    else
      IMPNN_MASK(1, 64);
#undef IMPNN_MASK
  } else {
    transfer_grid_kernel<GridMask><<<(int)tiles, 256, sizeof(float) * kTgLdsFloats, c.stream>>>(c.mix_cat, c.mix_an, c.w, nullptr,
                                                                                               c.C, c.A, tiles_a, mask);
  }
  return check_launch(what);
}

}  // namespace impnn
