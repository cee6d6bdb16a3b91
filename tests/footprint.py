"""Footprints of the C entries: where a kernel writes and what it reads before it has written it.

Three things live here, none of which needs a GPU to import:
  * Guarded / GuardLogic - a buffer of exactly n bytes between two guards in ONE allocation, so a kernel that overruns
    it lands in the guard and an assertion reports it (tests/test_gpu_footprint.py, and the screening files through
    test_gpu_screen's re-export);
  * entries() - the prototypes of include/impnn.h with their pointer parameters split into const and non-const;
  * COVERAGE - which test runs an entry on guarded buffers of exactly the documented size, or why it needs
    none.  tests/test_footprint_host.py holds the inventory against the header, so a new entry cannot be added
    without a line here.
"""
import ctypes as C
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "impnn.h"

GUARD = 4096         # guard bytes on either side of every buffer the entries write
FILL = 0xA5          # what they hold before the call: no float, index or entry the kernels write is 0xA5A5...


# ---------------------------------------------------------------- the guard logic (numpy and torch share it)
class GuardLogic:
    """`whole` = GUARD + offset guard bytes | n body bytes | GUARD guard bytes, one allocation.  Subclasses provide
    host() -> the whole buffer as a numpy uint8 array."""

    def _layout(self, nbytes, offset):
        assert nbytes >= 0 and 0 <= offset < 16
        self.n, self.lo = int(nbytes), GUARD + int(offset)
        return self.lo + self.n + GUARD

    def body(self, dtype, what):
        """The body as `dtype`, after checking that both guards still hold FILL."""
        host = self.host()
        before, after = host[:self.lo], host[self.lo + self.n:]
        assert (before == FILL).all(), f"write before {what}: {int((before != FILL).sum())} guard bytes changed, " \
                                       f"the nearest {self.lo - int(np.flatnonzero(before != FILL)[-1])} bytes ahead of it"
        assert (after == FILL).all(), f"write past {what}: {int((after != FILL).sum())} guard bytes changed, " \
                                      f"the first {int(np.flatnonzero(after != FILL)[0])} bytes behind its end"
        return host[self.lo:self.lo + self.n].view(dtype)

    def unchanged(self, snapshot, what):
        """The body still holds `snapshot` (bytes or an array of any dtype), bit for bit, and the guards FILL: for
        inputs, and for outputs of a refused call."""
        now = self.body(np.uint8, what)
        then = np.frombuffer(snapshot, np.uint8) if isinstance(snapshot, (bytes, bytearray)) \
            else np.ascontiguousarray(snapshot).view(np.uint8).reshape(-1)
        assert then.size == now.size, f"{what}: snapshot of {then.size} bytes for a body of {now.size}"
        diff = np.flatnonzero(now != then)
        assert diff.size == 0, f"{what} changed: {diff.size} bytes, the first at byte {int(diff[0])}"


class HostGuarded(GuardLogic):
    """The numpy-backed stand-in: the same layout and assertions on host memory (tests/test_footprint_host.py)."""

    def __init__(self, nbytes, fill=FILL, offset=0):
        self.whole = np.full(self._layout(nbytes, offset), FILL, np.uint8)
        self.whole[self.lo:self.lo + self.n] = fill

    def host(self):
        return self.whole


class Guarded(GuardLogic):
    """A device buffer of exactly `nbytes` between two guards.  fill: a byte value, or a uint8 tensor / array whose
    first nbytes bytes the body takes (what another call left behind; shorter sources are repeated).  offset: bytes
    past a 16-byte boundary at which the body starts, for entries whose header allows 4- or 8-byte alignment."""

    def __init__(self, nbytes, fill=FILL, offset=0):
        import torch
        total = self._layout(nbytes, offset)
        self.whole = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
        assert self.whole.data_ptr() % 16 == 0
        self.ptr = C.c_void_p(self.whole.data_ptr() + self.lo)
        self.fill(fill)

    def view(self):
        """The body as a uint8 device tensor (shares memory)."""
        return self.whole[self.lo:self.lo + self.n]

    def fill(self, fill):
        import torch
        if isinstance(fill, int):
            if fill != FILL:
                self.view().fill_(fill)
            return
        src = torch.as_tensor(fill).reshape(-1)
        src = src.view(torch.uint8) if src.dtype != torch.uint8 else src
        assert src.numel() > 0 or self.n == 0
        if self.n:
            reps = -(-self.n // src.numel())
            self.view().copy_(src.repeat(reps)[:self.n].to("cuda"))

    def host(self):
        return self.whole.cpu().numpy()


# ---------------------------------------------------------------- the header's entries
def entries(text=None):
    """{entry name: {"ret": type, "const": [names], "mutable": [names], "params": [(type, name)]}} of every function
    include/impnn.h (or `text`) declares.  A pointer parameter is const when what it (finally) points at is: `const
    float*`, `const float* const*`; `float* const*` - a host array of output pointers - is mutable."""
    text = HEADER.read_text() if text is None else text
    body = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.sub(r"^\s*#.*$", "", body, flags=re.M)
    out = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(impnn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", body):
        ret, name, plist = m.group(1).strip(), m.group(2), m.group(3).strip()
        if "typedef" in ret or not ret:
            continue
        params, const, mutable = [], [], []
        for p in ([] if plist in ("", "void") else plist.split(",")):
            p = " ".join(p.split())
            pm = re.match(r"(.*?)(\w+)(\[\d*\])?$", p)
            ptype, pname = pm.group(1).strip() + ("*" if pm.group(3) else ""), pm.group(2)
            params.append((ptype, pname))
            if "*" in ptype:
                (const if ptype.startswith("const ") else mutable).append(pname)
        out[name] = {"ret": ret, "const": const, "mutable": mutable, "params": params}
    return out


# ---------------------------------------------------------------- the inventory
QUERY = "exempt: a pure size / layout query, host memory only, launches nothing"
PROFILE = "exempt: profiler hook, host memory and HIP events of the calling thread only"
DEBUG = "exempt: debug hook, records a pointer and writes nothing itself"
_FP = "test_gpu_footprint::"

COVERAGE = {
    # queries that answer through a host pointer
    "impnn_encoder_workspace_bytes": QUERY,
    "impnn_encoder_plan_layout": QUERY,
    "impnn_encoder_plan_records": QUERY,
    "impnn_grid_topk_workspace_bytes": QUERY,
    "impnn_grid_partners_workspace_bytes": QUERY,
    "impnn_grid_rank_workspace_bytes": QUERY,
    "impnn_ensemble_grid_topk_workspace_bytes": QUERY,
    "impnn_transfer_mc_grid_topk_workspace_bytes": QUERY,
    "impnn_pareto_workspace_bytes": QUERY,
    "impnn_diverse_workspace_bytes": QUERY,
    "impnn_profile_collect": PROFILE,
    "impnn_debug_set_stamp_buffer": DEBUG,
    # the screening families: files that already pass exact-size guarded buffers
    "impnn_head_grid": "test_gpu_grid::test_grid_is_bitwise_the_head_kernel",
    "impnn_transfer_head_grid": "test_gpu_transfer_grid::test_grid_against_fp64_every_tile_edge_and_alignment",
    "impnn_head_grid_topk": "test_gpu_screen::test_head_topk_is_the_top_of_the_materialised_grid",
    "impnn_transfer_head_grid_topk": "test_gpu_screen::test_transfer_topk_is_the_top_of_the_materialised_grid",
    "impnn_head_grid_partners": "test_gpu_partners::test_head_partners_are_the_best_of_the_materialised_grid",
    "impnn_transfer_head_grid_partners": "test_gpu_partners::test_transfer_partners_are_the_best_of_the_materialised_grid",
    "impnn_head_grid_rank": "test_gpu_rank::test_head_rank_is_the_order_statistic_of_the_materialised_grid",
    "impnn_transfer_head_grid_rank": "test_gpu_rank::test_transfer_rank_is_the_order_statistic_of_the_materialised_grid",
    "impnn_head_grid_mask": "test_gpu_mask::test_head_mask_is_the_comparison_on_the_materialised_grid",
    "impnn_transfer_head_grid_mask": "test_gpu_mask::test_transfer_mask_is_the_comparison_on_the_materialised_grid",
    "impnn_head_grid_topk_where": "test_gpu_mask::test_head_topk_where_is_the_top_of_the_masked_grid",
    "impnn_transfer_head_grid_topk_where": "test_gpu_mask::test_transfer_topk_where_is_the_top_of_the_masked_grid",
    "impnn_pareto_begin": "test_gpu_pareto::test_the_filter_and_the_wrapper_give_the_reference_front",
    "impnn_pareto_range": "test_gpu_pareto::test_the_filter_and_the_wrapper_give_the_reference_front",
    "impnn_pareto_minima": "test_gpu_pareto::test_the_filter_and_the_wrapper_give_the_reference_front",
    "impnn_pareto_staircase": "test_gpu_pareto::test_the_filter_and_the_wrapper_give_the_reference_front",
    "impnn_pareto_collect": "test_gpu_pareto::test_the_filter_and_the_wrapper_give_the_reference_front",
    "impnn_domain_grid": "test_gpu_domain::test_nothing_is_written_outside_the_outputs",
    "impnn_domain_grid_mask": "test_gpu_domain::test_nothing_is_written_outside_the_outputs",
    "impnn_domain_rows": "test_gpu_domain::test_nothing_is_written_outside_the_outputs",
    "impnn_diverse_select": "test_gpu_diverse::test_nothing_is_written_outside_the_outputs_and_the_workspace",
    "impnn_transfer_mc_grid": "test_gpu_mc_dropout::test_output_alignment_does_not_change_a_bit",
    "impnn_state_rows": "test_gpu_frozen_states::test_state_rows_equals_index_select_bit_for_bit",
}

def _cover(test, *names):
    for n in names:
        assert n not in COVERAGE, n
        COVERAGE[n] = _FP + test


# tests/test_gpu_footprint.py: exact-size guarded outputs, workspaces, saved buffers and images
_cover("test_layer_kernels", "impnn_embed_gather", "impnn_bmm_message", "impnn_bmm_fused", "impnn_bond_type_matrices",
       "impnn_bond_type_matrices_multi", "impnn_bmm_message_typed", "impnn_reduce_scatter_add", "impnn_global_sum_pool",
       "impnn_gated_update", "impnn_gated_update_dropout", "impnn_gated_update_rows", "impnn_gated_update_rows_train",
       "impnn_gated_update_rows_train_dropout", "impnn_kept_rows", "impnn_row_index_fill", "impnn_dropout_step",
       "impnn_dropout_mask", "impnn_validate_indices")
_cover("test_adjoints", "impnn_embed_gather_bwd", "impnn_reduce_scatter_bwd", "impnn_global_sum_pool_bwd",
       "impnn_bond_type_matrices_bwd", "impnn_bond_type_matrices_multi_bwd", "impnn_bond_type_matrices_multi_bwd_ws",
       "impnn_gated_update_bwd", "impnn_gated_update_bwd_dropout", "impnn_gated_update_rows_bwd",
       "impnn_gated_update_rows_bwd_dropout", "impnn_gated_update_rows_bwd_saved",
       "impnn_gated_update_rows_bwd_saved_dropout", "impnn_bmm_message_typed_sorted", "impnn_bmm_message_typed_bwd",
       "impnn_message_reduce_typed_bwd", "impnn_message_reduce_typed_bwd_scratch")
_cover("test_encoder", "impnn_encoder_fused", "impnn_encoder_fused_prepared", "impnn_encoder_plan", "impnn_encoder_run")
_cover("test_prepared_images", "impnn_encoder_prepare_weights", "impnn_encoder_prepare_weights_atoms",
       "impnn_encoder_prepare_weights_gates")
_cover("test_heads", "impnn_model_head", "impnn_model_head_tensors", "impnn_head_ion_mix", "impnn_model_head_bwd",
       "impnn_model_head_loss", "impnn_weighted_model_head_loss", "impnn_model_head_loss_bwd",
       "impnn_weighted_model_head_loss_bwd", "impnn_transfer_head", "impnn_transfer_ion_half",
       "impnn_transfer_grid_prepare", "impnn_transfer_head_loss", "impnn_weighted_transfer_head_loss",
       "impnn_transfer_head_loss_rows", "impnn_transfer_head_loss_bwd", "impnn_weighted_transfer_head_loss_bwd",
       "impnn_transfer_head_loss_rows_bwd", "impnn_lr_schedule_eval")
# (impnn_adam_clipnorm_step has only const pointers - its table names the buffers it writes - and runs there too)
_cover("test_optimizer_metrics_loader", "impnn_adam_clipnorm_step", "impnn_adam_clipnorm_step_counted",
       "impnn_adam_step_scheduled", "impnn_regression_sums", "impnn_gather_rows", "impnn_batch_assemble")

# the screening entries whose own files reach them through the wrappers only
_cover("test_ensemble_and_mc_grids", "impnn_ensemble_grid", "impnn_ensemble_grid_mask", "impnn_ensemble_grid_topk",
       "impnn_ensemble_grid_topk_where", "impnn_transfer_mc_grid_mask", "impnn_transfer_mc_grid_topk",
       "impnn_transfer_mc_grid_topk_where")
