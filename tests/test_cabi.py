"""CPU: libimpnn.so loads without a GPU, exports every symbol include/impnn.h declares, and
rejects bad arguments before touching the device (no compute calls here)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from conftest import ROOT
from ionic_mpnn_amd import _lib

HEADER = (ROOT / "include" / "impnn.h").read_text()


def declared_symbols():
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    return sorted(set(re.findall(r"\b(impnn_[a-z0-9_]+)\s*\(", body)))


def test_library_is_built_in_tree():
    assert _lib.lib_path().exists(), "run python -m ionic_mpnn_amd.build (or __graft_entry__.build())"
    assert _lib.lib_path().parent == ROOT / "ionic_mpnn_amd" / "csrc"


def test_every_declared_symbol_is_exported_and_bound():
    names = declared_symbols()
    assert len(names) >= 15
    raw = C.CDLL(str(_lib.lib_path()))
    for n in names:
        assert hasattr(raw, n), f"{n} declared in impnn.h but not exported"
    assert set(names) == set(_lib.SIGNATURES), "ctypes binding table out of sync with impnn.h"


def test_identity():
    lib = _lib.load()
    assert lib.impnn_abi_version() == 3
    assert lib.impnn_target_arch() == b"gfx950"
    assert lib.impnn_encoder_step_floats(32, 8) == 8 * 1024 + 3 * (2048 + 32) + 64


def test_bad_arguments_are_status_codes_not_crashes():
    lib = _lib.load()
    null = None
    assert lib.impnn_embed_gather(null, null, null, 4, 10, 32, null) == -1
    assert b"null" in lib.impnn_last_error_string()
    assert lib.impnn_embed_gather(null, null, null, -1, 10, 32, null) == -1
    assert lib.impnn_gated_update(*([null] * 10), 1e-3, null, 5, 32, null) == -1
    assert lib.impnn_reduce_scatter_add(null, null, 0, null, 1, 4, 4, 8, null) == -1
    assert b"tgt_stride" in lib.impnn_last_error_string()
    assert lib.impnn_global_sum_pool(null, null, null, 2, 0, 8, null) == -1
    # zero-size work is a no-op success
    assert lib.impnn_embed_gather(null, null, null, 0, 10, 32, null) == 0
    assert lib.impnn_bmm_message(null, null, null, null, null, 0, 4, 4, 8, 2, null) == 0


def test_encoder_shape_coverage_is_reported():
    lib = _lib.load()
    need = C.c_size_t(0)
    F32, F16X2, TYPED = 0, 1, 2
    for mode in (F32, F16X2, TYPED):
        assert lib.impnn_encoder_workspace_bytes(2, 4096, 40, 80, 32, 8, 3, 72, mode, 0, C.byref(need)) == 0
        assert 0 < need.value < (64 << 20)
        # wide states (train_viscosity.py with atom_dim=128): the per-bond-type mode only (csrc/encoder_wide.hip, wide_*.hip)
        rc = lib.impnn_encoder_workspace_bytes(2, 4096, 40, 80, 128, 8, 6, 72, mode, 0, C.byref(need))
        assert rc == (0 if mode == TYPED else -2)
    assert (256 << 20) < need.value < (2 << 30)
    assert lib.impnn_encoder_workspace_bytes(2, 64, 40, 80, 64, 8, 3, 72, TYPED, 0, C.byref(need)) == 0        # D=64
    assert lib.impnn_encoder_workspace_bytes(2, 64, 40, 80, 48, 8, 3, 72, TYPED, 0, C.byref(need)) == -2       # D=48
    assert lib.impnn_encoder_workspace_bytes(2, 64, 40, 1100, 128, 8, 3, 72, TYPED, 0, C.byref(need)) == -2    # E > 1024
    assert lib.impnn_encoder_workspace_bytes(2, 64, 160, 640, 128, 8, 3, 72, TYPED, 0, C.byref(need)) == 0 and need.value > 0
    assert lib.impnn_encoder_workspace_bytes(2, 64, 40, 80, 128, 8, 3, 72, 3, 0, C.byref(need)) == 0           # f32x3 (round 3)
    # K = D*D (train_melting_point.py:146): the typed mode covers it (BASELINE config 3), the pull form does not
    assert lib.impnn_encoder_workspace_bytes(2, 8192, 40, 80, 32, 1024, 4, 72, TYPED, 0, C.byref(need)) == 0
    assert lib.impnn_encoder_workspace_bytes(2, 4096, 40, 80, 32, 1024, 3, 72, F32, 0, C.byref(need)) == -2
    assert b"not covered" in lib.impnn_last_error_string()
    # the typed records take any padded shape (explicit-H molecules: N = 160, E = 640, train_viscosity.py:288-289): a
    # chunk is bounded by what a molecule HOLDS, checked per batch by the plan kernels (round 3); K = D^2 included
    assert lib.impnn_encoder_workspace_bytes(2, 16, 40, 300, 32, 8, 3, 72, TYPED, 0, C.byref(need)) == 0
    assert lib.impnn_encoder_workspace_bytes(2, 4096, 160, 640, 32, 8, 3, 72, TYPED, 0, C.byref(need)) == 0 and need.value > 0
    assert lib.impnn_encoder_workspace_bytes(2, 4096, 160, 640, 32, 1024, 4, 72, TYPED, 0, C.byref(need)) == 0 and need.value > 0
    assert lib.impnn_encoder_workspace_bytes(2, 4096, 160, 640, 32, 8, 3, 72, F32, 0, C.byref(need)) == -2   # pull form: N <= 128
    assert lib.impnn_encoder_workspace_bytes(3, 16, 40, 80, 32, 8, 3, 72, F32, 0, C.byref(need)) == -1
    assert lib.impnn_encoder_workspace_bytes(2, 16, 40, 80, 32, 8, 3, 72, 3, 0, C.byref(need)) == 0        # f32x3
    assert lib.impnn_encoder_workspace_bytes(2, 16, 40, 80, 32, 8, 3, 72, 4, 0, C.byref(need)) == -1       # no mode 4
    assert lib.impnn_encoder_workspace_bytes(2, 16, 40, 80, 32, 8, 3, 72, F32, -1, C.byref(need)) == -1
    assert lib.impnn_encoder_prepared_bytes(32, 3, 72, 3) > lib.impnn_encoder_prepared_bytes(32, 3, 72, TYPED) > lib.impnn_encoder_prepared_bytes(32, 3, 72, F32) > 0
    assert lib.impnn_encoder_prepared_bytes(128, 6, 72, TYPED) == 6 * (72 * 128 * 128 + 6 * 128 * 128 + 5 * 128) * 4
    # mode 3, wide: f32 type matrices | gate kernels as three bf16 planes | vectors | the type matrices as three bf16 planes
    assert lib.impnn_encoder_prepared_bytes(128, 6, 72, 3) == 6 * (72 * 128 * 128 + 9 * 128 * 128 + 5 * 128 + 72 * 128 * 128 * 3 // 2) * 4
    assert lib.impnn_encoder_prepared_bytes(128, 6, 72, F32) == 0 and lib.impnn_encoder_prepared_bytes(48, 6, 72, TYPED) == 0


def test_wide_encoder_refuses_batches_beyond_its_32_bit_offsets():
    """The wide encoder's coverage of a BATCH (csrc/encoder_wide.hip, encoder_wide_batch_covered): its update kernels
    (csrc/wide_update.hip, wide_update_x3.hip) address a row's aggregated messages as 32-bit float offsets from `agg` - rows up to rmax, the row of zeros, times D -
    and sorted edge positions up to vmax are 32-bit indices.  With every row's sum in agg (the largest batches) nothing
    else bounds rmax * D, so impnn_encoder_workspace_bytes refuses such a batch before anything is allocated for it:
    one shape on each side of each bound."""
    lib = _lib.load()
    need = C.c_size_t(0)
    TYPED, X3, Vb = 2, 3, 72

    def rmax(B, N):            # compact rows of two ions: whole 128-row tiles, each ion aligned to 128
        return (2 * B * N + 2 * 128 + 127) // 128 * 128

    def vmax(B, E, D):         # sorted positions: a type's run is padded to whole message tiles
        return 2 * B * E + (2 * Vb + 2) * (64 if D == 128 else 128)

    def covered(B, N, E, D, mode=TYPED):
        rc = lib.impnn_encoder_workspace_bytes(2, B, N, E, D, 8, 6, Vb, mode, 0, C.byref(need))
        assert rc in (0, -2), rc
        if rc:
            assert b"32-bit" in lib.impnn_last_error_string()
        return rc == 0

    # rows: (rmax + 1) * D < 2^31.  The explicit-hydrogen shape at D = 128 passes it up to 52 427 pairs
    for B, N, E, D in ((52427, 160, 640, 128), (209710, 40, 80, 128), (104856, 160, 640, 64)):
        assert (rmax(B, N) + 1) * D < 2 ** 31 <= (rmax(B + 1, N) + 1) * D and vmax(B + 1, E, D) < 2 ** 31 - 1
        for mode in (TYPED, X3):
            assert covered(B, N, E, D, mode) and need.value > (rmax(B, N) * D * 4) * 2
            assert not covered(B + 1, N, E, D, mode)
    # edges: vmax < 2^31 - 1 (few rows, many edge slots)
    for D in (128, 64):
        B = (2 ** 31 - 2 - (2 * Vb + 2) * (64 if D == 128 else 128)) // (2 * 1024)
        assert vmax(B, 1024, D) < 2 ** 31 - 1 <= vmax(B + 1, 1024, D) and (rmax(B + 1, 1) + 1) * D < 2 ** 31
        assert covered(B, 1, 1024, D) and not covered(B + 1, 1, 1024, D)
    # the atom_dim 32 encoders have their own records and are not concerned
    assert lib.impnn_encoder_workspace_bytes(2, 60000, 160, 640, 32, 8, 3, Vb, TYPED, 0, C.byref(need)) == 0


def test_encoder_plan_layout_follows_the_size_query():
    """impnn_encoder_plan_layout: the refusals of impnn_encoder_workspace_bytes in the same order (plus: atom_dim 32
    only), every table inside the workspace the size query asks for, and the documented floor of 16 workgroups."""
    lib = _lib.load()
    need = C.c_size_t(0)
    out = (C.c_int64 * 8)()
    F32, F16X2, TYPED, X3 = 0, 1, 2, 3
    ok = (2, 4096, 40, 80, 32, 8, 3, 72, TYPED, 0)
    names = ("n_ions", "B", "N", "E", "D", "K", "S", "Vb", "mode", "workgroups")

    def both(**kw):
        args = [kw.get(n, v) for n, v in zip(names, ok)]
        for i in range(8):
            out[i] = -7
        rc_b, msg_b = lib.impnn_encoder_workspace_bytes(*args, C.byref(need)), lib.impnn_last_error_string()
        rc_l, msg_l = lib.impnn_encoder_plan_layout(*args, out), lib.impnn_last_error_string()
        if rc_l:
            assert list(out) == [-7] * 8, kw   # a refusal writes nothing
        return rc_b, msg_b, rc_l, msg_l, args

    assert lib.impnn_encoder_plan_layout(*ok, None) == -1 and b"null pointer" in lib.impnn_last_error_string()
    # the argument refusals: the same status and the same words
    for kw in (dict(n_ions=0), dict(n_ions=3), dict(B=-1), dict(N=0), dict(E=-1), dict(D=0), dict(K=0), dict(S=-1), dict(Vb=0),
               dict(mode=4), dict(mode=-1), dict(workgroups=-1), dict(n_ions=3, mode=4, workgroups=-1)):
        rc_b, msg_b, rc_l, msg_l, _ = both(**kw)
        assert rc_b == rc_l == -1 and msg_b == msg_l, kw
    # the coverage refusals
    for kw in (dict(K=1024, mode=F32), dict(N=160, E=640, mode=F32), dict(D=48), dict(D=128, mode=F32), dict(Vb=257),
               dict(D=128, E=1100)):
        rc_b, msg_b, rc_l, msg_l, _ = both(**kw)
        assert rc_b == rc_l == -2 and msg_b == msg_l and b"not covered" in msg_l, kw
    # wide states have no chunk plan: covered by the size query, refused here
    for kw in (dict(D=64), dict(D=128), dict(D=128, mode=X3), dict(D=128, N=160, E=640)):
        rc_b, _, rc_l, msg_l, _ = both(**kw)
        assert rc_b == 0 and rc_l == -2 and b"atom_dim 32 only" in msg_l, kw
    # atom_dim 32: every table lies inside what the size query asks for, in the order of the layout
    for kw in (dict(), dict(mode=F32), dict(mode=F16X2), dict(mode=X3), dict(B=0), dict(B=1), dict(B=3, workgroups=16),
               dict(n_ions=1, B=777), dict(N=160, E=640), dict(N=160, E=640, K=1024, S=4), dict(B=60000, N=160, E=640),
               dict(N=4, E=0, B=3000, workgroups=16), dict(workgroups=48), dict(workgroups=200), dict(S=0)):
        rc_b, _, rc_l, _, args = both(**kw)
        assert rc_b == 0 and rc_l == 0, kw
        nwg, max_sub, rows_off, vr_off, nsub_off, desc_off, ecap, vmin = list(out)
        n_ions, B, E, mode, wgs = args[0], args[1], args[3], args[8], args[9]
        total = need.value
        assert nwg >= 16, kw
        assert 1 <= max_sub <= 128 and 1 <= vmin <= 256, kw
        assert 256 <= rows_off and rows_off + 4 * n_ions * B <= vr_off and vr_off + 4 * n_ions * B <= nsub_off, kw
        assert nsub_off + 4 * nwg <= desc_off and desc_off + 16 * nwg * max_sub <= total, kw
        assert all(off % 256 == 0 and off <= total for off in (rows_off, vr_off, nsub_off, desc_off)), kw
        assert ecap == (0 if mode < TYPED else 640 if E > 512 else 512), kw
        if 0 < wgs <= 256:
            assert nwg % max(wgs, 16) == 0, kw
    # a request below 16 workgroups is a request for 16: the same layout, the same size
    for mode in (F32, TYPED):
        want = None
        for wgs in (1, 2, 3, 15, 16):
            rc_b, _, rc_l, _, _ = both(mode=mode, workgroups=wgs, B=200, N=12, E=24)
            assert rc_b == 0 and rc_l == 0 and out[0] == 16
            want = want or (list(out), need.value)
            assert (list(out), need.value) == want, wgs
        both(mode=mode, workgroups=17, B=200, N=12, E=24)
        assert out[0] == 17 and (list(out), need.value) != want


def test_encoder_sizing_has_no_hidden_state():
    """The workgroup count is an argument, not library state: two host threads sizing workspaces with different
    counts at the same time always get the answer that belongs to their own arguments."""
    import threading
    lib = _lib.load()

    def size(wgs, mode=2):
        need = C.c_size_t(0)
        assert lib.impnn_encoder_workspace_bytes(2, 4096, 40, 80, 32, 8, 3, 72, mode, wgs, C.byref(need)) == 0
        return need.value

    want = {w: size(w) for w in (0, 64, 128, 200)}
    assert len(set(want.values())) >= 3 and want[64] != want[128]
    errors = []

    def worker(wgs):
        for _ in range(3000):
            got = size(wgs)
            if got != want[wgs]:
                errors.append((wgs, got))
                return

    threads = [threading.Thread(target=worker, args=(w,)) for w in (64, 128, 200, 0)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    # neither entry exists any more: the mode and the workgroup count travel with every call
    raw = C.CDLL(str(_lib.lib_path()))
    assert not hasattr(raw, "impnn_encoder_set_workgroups") and not hasattr(raw, "impnn_encoder_set_mode")


def test_plan_info_is_checked_on_the_host():
    """impnn_encoder_run validates the plan info before anything is enqueued (no device needed: every failing
    call returns before its first launch; the pointers below are never dereferenced)."""
    lib = _lib.load()
    info = _lib.PlanInfo()
    fake = (C.c_void_p * 2)(0x1000, 0x1000)
    fp = C.c_void_p(0x1000)

    def run(B=4, N=10, E=20, S=1, Vb=5, mode=2):
        return lib.impnn_encoder_run(2, fake, fp, 10, fp, Vb, fake, mode, fake, B, N, E, 32, 8, S, 1e-3, C.byref(info),
                                     fp, 1 << 30, None)

    assert run() == -1 and b"not filled by impnn_encoder_plan" in lib.impnn_last_error_string()
    # B = 0 plans nothing on the device but still records what it was planned for
    rc = lib.impnn_encoder_plan(2, fake, fake, fake, 0, 10, 20, 32, 8, 1, 10, 5, 2, 96, fp, 1 << 30, None, C.byref(info))
    assert rc == 0 and info.v[3] == 0 and info.v[8] == 96 and info.v[1] == 1
    for kw in ({"B": 4}, {"N": 11}, {"E": 21}, {"S": 2}, {"Vb": 6}, {"mode": 0}):
        args = {"B": 0}
        args.update(kw)
        assert run(**args) == -1, kw
        assert b"planned for another" in lib.impnn_last_error_string(), kw
    assert run(B=0) == 0  # matching (empty) batch: accepted


def test_cpu_tensors_fail_loudly():
    import torch
    from ionic_mpnn_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.embed_gather(torch.zeros(2, 3, dtype=torch.int32), torch.zeros(5, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.global_sum_pool(torch.zeros(1, 2, 4), torch.ones(1, 2, dtype=torch.int32))


def test_row_list_backward_reports_its_coverage():
    """impnn_gated_update_rows_bwd covers atom_dim 64 / 128 (the wide matrix-core kernel); other widths are refused
    before anything is launched, and the workspace query answers 0 for them."""
    lib = _lib.load()
    null = None
    assert lib.impnn_gated_update_rows_bwd_workspace_floats(1000, 128) > lib.impnn_gated_update_bwd_workspace_floats(1000, 128) > 0
    assert lib.impnn_gated_update_rows_bwd_workspace_floats(1000, 32) == 0
    rc = lib.impnn_gated_update_rows_bwd(*([null] * 9), 1e-3, *([null] * 5), 0, null, null, 1000, 32, 0, null)
    assert rc == -2 and b"row-list" in lib.impnn_last_error_string()
    rc = lib.impnn_gated_update_rows_bwd(*([null] * 9), 1e-3, *([null] * 5), 0, null, null, 1000, 128, 0, null)
    assert rc == -1  # null pointers


# ---- the GatedUpdate family's argument rules, pinned entry by entry.  Every row is refused, or is a zero-row no-op,
# before anything is launched: the pointers are stand-ins that are never dereferenced.
_A = 0x100000  # a 16-byte aligned stand-in
_M = 0x100004  # a misaligned one
_GU_FWD = ["h", "agg", "Wz", "bz", "Wr", "br", "Wh", "bh", "gamma", "beta", "eps", "out"]
_GU_BWD = ["h", "agg", "Wz", "bz", "Wr", "br", "Wh", "bh", "gamma", "eps", "dout", "dh", "dagg", "dparams", "workspace",
           "workspace_floats"]
_ROWS = ["row_index", "n_rows"]
_DROP = ["rate", "seed", "step", "layer_word"]
_GU_PARAMS = {
    "impnn_gated_update": _GU_FWD + ["rows", "D"],
    "impnn_gated_update_rows": _GU_FWD + _ROWS + ["rows", "D"],
    "impnn_gated_update_rows_train": _GU_FWD + _ROWS + ["rows", "D", "saved"],
    "impnn_gated_update_dropout": _GU_FWD + ["rows", "D"] + _DROP,
    "impnn_gated_update_rows_train_dropout": _GU_FWD + _ROWS + ["rows", "D", "saved"] + _DROP,
    "impnn_gated_update_bwd": _GU_BWD + ["rows", "D", "accumulate"],
    "impnn_gated_update_rows_bwd": _GU_BWD + _ROWS + ["rows", "D", "accumulate"],
    "impnn_gated_update_rows_bwd_saved": _GU_BWD + _ROWS + ["rows", "D", "accumulate", "saved"],
    "impnn_gated_update_bwd_dropout": _GU_BWD + ["rows", "D", "accumulate"] + _DROP,
    "impnn_gated_update_rows_bwd_dropout": _GU_BWD + _ROWS + ["rows", "D", "accumulate"] + _DROP,
    "impnn_gated_update_rows_bwd_saved_dropout": _GU_BWD + _ROWS + ["rows", "D", "accumulate", "saved"] + _DROP,
}
_NULLS = {k: None for k in ("h", "agg", "Wz", "bz", "Wr", "br", "Wh", "bh", "gamma", "beta", "out", "dout", "dh", "dagg",
                            "dparams", "workspace")}
_BAD, _UNS, _WS = -1, -2, -4
_WS_PLAIN, _WS_ROWS = "impnn_gated_update_bwd_workspace_floats", "impnn_gated_update_rows_bwd_workspace_floats"
# (entry, arguments that differ from the defaults, expected status, substring of the error text or None)
_GU_CASES = [
    # null tensors; zero rows return before the null check in the forwards and the list / saving backwards only
    ("impnn_gated_update", dict(_NULLS), _BAD, b"null"),
    ("impnn_gated_update", dict(_NULLS, rows=0), 0, None),
    ("impnn_gated_update", dict(out=None), _BAD, b"null"),
    ("impnn_gated_update_rows", dict(gamma=None), _BAD, b"null"),
    ("impnn_gated_update_rows", dict(_NULLS, rows=0), 0, None),
    ("impnn_gated_update_rows_train", dict(saved=None), _BAD, b"null"),
    ("impnn_gated_update_rows_train", dict(_NULLS, saved=None, rows=0), 0, None),
    ("impnn_gated_update_dropout", dict(beta=None), _BAD, b"null"),
    ("impnn_gated_update_dropout", dict(_NULLS, rows=0), 0, None),
    ("impnn_gated_update_dropout", dict(_NULLS, rows=0, rate=0.0), 0, None),
    ("impnn_gated_update_rows_train_dropout", dict(h=None), _BAD, b"null"),
    ("impnn_gated_update_rows_train_dropout", dict(h=None, rate=0.0), _BAD, b"null"),
    ("impnn_gated_update_rows_train_dropout", dict(h=None, saved=None, rate=0.0), _BAD, b"null"),
    ("impnn_gated_update_rows_train_dropout", dict(_NULLS, rows=0), 0, None),
    ("impnn_gated_update_bwd", dict(dparams=None), _BAD, b"null"),
    ("impnn_gated_update_bwd", dict(_NULLS, rows=0), _BAD, b"null"),
    ("impnn_gated_update_rows_bwd", dict(workspace=None), _BAD, b"null"),
    ("impnn_gated_update_rows_bwd", dict(rows=0), 0, None),
    ("impnn_gated_update_rows_bwd", dict(_NULLS, rows=0), _BAD, b"null"),
    ("impnn_gated_update_rows_bwd_saved", dict(saved=None), _BAD, b"null"),
    ("impnn_gated_update_rows_bwd_saved", dict(rows=0), 0, None),
    ("impnn_gated_update_rows_bwd_saved", dict(rows=0, D=32, row_index=None, n_rows=None), 0, None),
    ("impnn_gated_update_bwd_dropout", dict(dh=None), _BAD, b"null"),
    ("impnn_gated_update_bwd_dropout", dict(_NULLS, rows=0), _BAD, b"null"),
    ("impnn_gated_update_bwd_dropout", dict(_NULLS, rows=0, rate=0.0), _BAD, b"null"),
    ("impnn_gated_update_rows_bwd_dropout", dict(dagg=None), _BAD, b"null"),
    ("impnn_gated_update_rows_bwd_dropout", dict(rows=0), 0, None),
    ("impnn_gated_update_rows_bwd_saved_dropout", dict(dout=None), _BAD, b"null"),
    ("impnn_gated_update_rows_bwd_saved_dropout", dict(rows=0), 0, None),
    ("impnn_gated_update_rows_bwd_saved_dropout", dict(rows=0, rate=0.0), 0, None),
    # a row list needs both row_index and n_rows
    ("impnn_gated_update_rows", dict(n_rows=None), _BAD, b"null"),
    ("impnn_gated_update_rows", dict(row_index=None), _BAD, b"null"),
    ("impnn_gated_update_rows_train", dict(n_rows=None), _BAD, b"both or neither"),
    ("impnn_gated_update_rows_train", dict(row_index=None), _BAD, b"both or neither"),
    ("impnn_gated_update_rows_train_dropout", dict(n_rows=None), _BAD, b"both or neither"),
    ("impnn_gated_update_rows_train_dropout", dict(row_index=None, saved=None), _BAD, b"both or neither"),
    ("impnn_gated_update_rows_train_dropout", dict(n_rows=None, saved=None, rate=0.0), _BAD, b"null"),
    ("impnn_gated_update_rows_bwd", dict(n_rows=None), _BAD, b"null"),
    ("impnn_gated_update_rows_bwd_saved", dict(row_index=None), _BAD, b"both or neither"),
    ("impnn_gated_update_rows_bwd_saved_dropout", dict(n_rows=None), _BAD, b"both or neither"),
    ("impnn_gated_update_rows_bwd_saved_dropout", dict(n_rows=None, rate=0.0), _BAD, b"both or neither"),
    ("impnn_gated_update_rows_bwd_dropout", dict(row_index=None), _BAD, b"null"),
    # atom_dim coverage per form
    ("impnn_gated_update", dict(D=0), _BAD, None),
    ("impnn_gated_update", dict(D=512), _UNS, None),
    ("impnn_gated_update_rows", dict(D=48), _UNS, None),
    ("impnn_gated_update_rows", dict(D=0), _BAD, None),
    ("impnn_gated_update_rows_train", dict(D=256), _UNS, None),
    ("impnn_gated_update_rows_train", dict(D=0), _UNS, None),
    ("impnn_gated_update_rows_train", dict(D=48, saved=None), _UNS, None),
    ("impnn_gated_update_rows_train", dict(D=48, rows=0), _UNS, None),
    ("impnn_gated_update_dropout", dict(D=0), _BAD, None),
    ("impnn_gated_update_rows_train_dropout", dict(D=256), _UNS, None),
    ("impnn_gated_update_rows_train_dropout", dict(D=256, rows=0), _UNS, None),
    ("impnn_gated_update_rows_train_dropout", dict(D=0), _BAD, None),
    ("impnn_gated_update_rows_train_dropout", dict(D=48, saved=None), _UNS, None),
    ("impnn_gated_update_rows_train_dropout", dict(D=48, saved=None, rows=0), 0, None),
    ("impnn_gated_update_rows_train_dropout", dict(D=256, rate=0.0), _UNS, None),
    ("impnn_gated_update_rows_train_dropout", dict(D=48, saved=None, rate=0.0), _UNS, None),
    ("impnn_gated_update_bwd", dict(D=48), _BAD, None),
    ("impnn_gated_update_bwd", dict(D=512), _BAD, None),
    ("impnn_gated_update_rows_bwd", dict(D=48), _UNS, b"row-list"),
    ("impnn_gated_update_rows_bwd", dict(D=32, rows=0), _UNS, b"row-list"),
    ("impnn_gated_update_rows_bwd", dict(_NULLS, D=256), _UNS, b"row-list"),
    ("impnn_gated_update_rows_bwd_saved", dict(D=256), _UNS, None),
    ("impnn_gated_update_rows_bwd_saved", dict(_NULLS, D=48), _UNS, None),
    ("impnn_gated_update_rows_bwd_saved", dict(D=32), _UNS, b"row list"),
    ("impnn_gated_update_rows_bwd_saved", dict(D=32, rows=0), _UNS, b"row list"),
    ("impnn_gated_update_bwd_dropout", dict(D=96), _BAD, None),
    ("impnn_gated_update_rows_bwd_dropout", dict(D=48), _UNS, b"row-list"),
    ("impnn_gated_update_rows_bwd_dropout", dict(D=48, rate=0.0), _UNS, b"row-list"),
    ("impnn_gated_update_rows_bwd_saved_dropout", dict(D=256), _UNS, None),
    ("impnn_gated_update_rows_bwd_saved_dropout", dict(D=32), _UNS, b"row list"),
    # 16-byte alignment of the row-list and saving forms
    ("impnn_gated_update_rows", dict(D=32, h=_M), _BAD, b"aligned"),
    ("impnn_gated_update_rows_train", dict(saved=_M), _BAD, b"aligned"),
    ("impnn_gated_update_rows_train", dict(D=32, out=_M), _BAD, b"aligned"),
    ("impnn_gated_update_rows_train", dict(D=32, agg=_M, row_index=None, n_rows=None), _BAD, b"aligned"),
    ("impnn_gated_update_rows_train_dropout", dict(saved=_M), _BAD, b"aligned"),
    ("impnn_gated_update_rows_train_dropout", dict(D=32, h=_M), _BAD, b"aligned"),
    ("impnn_gated_update_rows_train_dropout", dict(D=32, h=_M, saved=None), _BAD, b"aligned"),
    ("impnn_gated_update_rows_bwd", dict(h=_M), _BAD, b"aligned"),
    ("impnn_gated_update_rows_bwd", dict(workspace=_M), _BAD, b"aligned"),
    ("impnn_gated_update_rows_bwd_saved", dict(saved=_M), _BAD, b"aligned"),
    ("impnn_gated_update_rows_bwd_saved", dict(D=32, dout=_M, row_index=None, n_rows=None), _BAD, b"aligned"),
    ("impnn_gated_update_rows_bwd_saved", dict(dh=_M, row_index=None, n_rows=None), _BAD, b"aligned"),
    ("impnn_gated_update_rows_bwd_dropout", dict(dagg=_M), _BAD, b"aligned"),
    ("impnn_gated_update_rows_bwd_saved_dropout", dict(saved=_M), _BAD, b"aligned"),
    ("impnn_gated_update_rows_bwd_saved_dropout", dict(saved=_M, rate=0.0), _BAD, b"aligned"),
    # workspace one float too small (the saving backward takes the row-list size at 64 / 128, list or not)
    ("impnn_gated_update_bwd", dict(workspace_floats=(_WS_PLAIN, -1)), _WS, b"workspace"),
    ("impnn_gated_update_rows_bwd", dict(workspace_floats=(_WS_ROWS, -1)), _WS, b"workspace"),
    ("impnn_gated_update_rows_bwd", dict(workspace_floats=(_WS_ROWS, -1), rows=0), _WS, b"workspace"),
    ("impnn_gated_update_rows_bwd_saved", dict(workspace_floats=(_WS_ROWS, -1)), _WS, b"workspace"),
    ("impnn_gated_update_rows_bwd_saved", dict(workspace_floats=(_WS_ROWS, -1), row_index=None, n_rows=None), _WS, None),
    ("impnn_gated_update_rows_bwd_saved", dict(workspace_floats=(_WS_PLAIN, 0), D=128, row_index=None, n_rows=None),
     _WS, None),
    ("impnn_gated_update_rows_bwd_saved", dict(workspace_floats=(_WS_PLAIN, -1), D=32, row_index=None, n_rows=None),
     _WS, None),
    ("impnn_gated_update_bwd_dropout", dict(workspace_floats=(_WS_PLAIN, -1)), _WS, None),
    ("impnn_gated_update_bwd_dropout", dict(workspace_floats=(_WS_PLAIN, -1), rate=0.0), _WS, None),
    ("impnn_gated_update_rows_bwd_dropout", dict(workspace_floats=(_WS_ROWS, -1)), _WS, None),
    ("impnn_gated_update_rows_bwd_saved_dropout", dict(workspace_floats=(_WS_ROWS, -1)), _WS, None),
    # rows < 0
    ("impnn_gated_update", dict(rows=-1), _BAD, None),
    ("impnn_gated_update_rows", dict(rows=-1), _BAD, None),
    ("impnn_gated_update_rows_train", dict(rows=-1, D=48), _BAD, None),
    ("impnn_gated_update_dropout", dict(rows=-1), _BAD, None),
    ("impnn_gated_update_rows_train_dropout", dict(rows=-1), _BAD, None),
    ("impnn_gated_update_bwd", dict(rows=-1), _BAD, None),
    ("impnn_gated_update_rows_bwd", dict(rows=-1, D=48), _BAD, None),
    ("impnn_gated_update_rows_bwd_saved", dict(rows=-1), _BAD, None),
    ("impnn_gated_update_bwd_dropout", dict(rows=-1), _BAD, None),
    ("impnn_gated_update_rows_bwd_dropout", dict(rows=-1), _BAD, None),
    ("impnn_gated_update_rows_bwd_saved_dropout", dict(rows=-1), _BAD, None),
    # eps < 0 (the forwards check it; the backwards do not)
    ("impnn_gated_update", dict(eps=-1.0), _BAD, b"ln_eps"),
    ("impnn_gated_update_rows", dict(eps=-1.0), _BAD, b"ln_eps"),
    ("impnn_gated_update_rows_train", dict(eps=-1.0), _BAD, b"ln_eps"),
    ("impnn_gated_update_dropout", dict(eps=-1.0), _BAD, b"ln_eps"),
    ("impnn_gated_update_rows_train_dropout", dict(eps=-1.0), _BAD, b"ln_eps"),
    ("impnn_gated_update_rows_train_dropout", dict(eps=-1.0, rate=0.0, saved=None, row_index=None), _BAD, b"ln_eps"),
] + [
    # the dropout tail: a null step, then the rate, come before everything else
    (entry, dict(_NULLS, rows=-1, **kw), _BAD, what)
    for entry in [e for e in _GU_PARAMS if e.endswith("_dropout")]
    for kw, what in ((dict(step=None), b"step"), (dict(rate=-0.1), b"rate"), (dict(rate=1.0), b"rate"),
                     (dict(rate=float("nan")), b"rate"), (dict(step=None, rate=0.0), b"step"))
]


def _gu_args(lib, entry, kw):
    args = dict(eps=1e-3, rows=1000, D=64, accumulate=0, rate=0.5, seed=7, layer_word=3, step=_A,
                workspace_floats=1 << 40)
    args.update(kw)
    q = args["workspace_floats"]
    if isinstance(q, tuple):  # (size query, offset)
        args["workspace_floats"] = getattr(lib, q[0])(max(args["rows"], 0), args["D"]) + q[1]
    names = _GU_PARAMS[entry]
    return [args.get(n, _A) for n in names] + [None]


def test_gated_update_status_codes_are_pinned():
    """The status code of every GatedUpdate entry for each class of refusal (recorded on the entries as they were
    before their checks were shared).  Nothing here reaches a launch."""
    lib = _lib.load()
    assert set(_GU_PARAMS) == {n for n in _lib.SIGNATURES if n.startswith("impnn_gated_update") and
                               not n.endswith("_floats")}
    assert {c[0] for c in _GU_CASES} == set(_GU_PARAMS)
    for entry, kw, want, what in _GU_CASES:
        fn = getattr(lib, entry)
        args = _gu_args(lib, entry, kw)
        assert len(args) == len(fn.argtypes), entry
        assert fn(*args) == want, (entry, kw)
        if what is not None:
            assert what in lib.impnn_last_error_string(), (entry, kw)


# ---- the typed-message family's argument rules, pinned entry by entry (recorded on the entries as they were before
# their checks were shared).  Every call returns before any device call: pointers that must not be null are addresses
# inside a host buffer, and no case lets them be dereferenced.
_TM_GRAD = ["h", "bond_ids", "conn", "type_mats", "grad", "dh", "dtype_mats", "workspace", "workspace_bytes"]
_TM_SHAPE = ["B", "N", "E", "D", "Vb", "sorted_ready"]
_TM_PARAMS = {
    "impnn_bmm_message_typed_sorted": ["h", "bond_ids", "conn", "type_mats", "messages", "workspace", "workspace_bytes"]
                                      + _TM_SHAPE,
    "impnn_bmm_message_typed_bwd": _TM_GRAD + _TM_SHAPE,
    "impnn_message_reduce_typed_bwd": _TM_GRAD + _TM_SHAPE,
    "impnn_message_reduce_typed_bwd_scratch": _TM_GRAD + ["edge_scratch"] + _TM_SHAPE,
}
_TM_POINTERS = ("h", "bond_ids", "conn", "type_mats", "messages", "grad", "dh", "dtype_mats", "workspace", "edge_scratch")


def test_typed_message_status_codes_are_pinned():
    """Status code and error text of the four typed-message entries for each class of refusal, in the order the rules
    apply: shape, zero work, null pointers, workspace size, coverage (Vb, then D)."""
    lib = _lib.load()
    host = (C.c_char * 256)()
    at = C.addressof(host)  # 16-byte steps inside the buffer: distinct, never dereferenced
    ptrs = {n: at + 16 * (i + 1) for i, n in enumerate(_TM_POINTERS)}
    nulls = {n: None for n in _TM_POINTERS}
    need = lib.impnn_bmm_message_typed_bwd_workspace_bytes

    def call(entry, **kw):
        args = dict(ptrs, B=3, N=7, E=11, D=64, Vb=5, sorted_ready=0)
        args.update(kw)
        args.setdefault("workspace_bytes", 1 << 40)
        fn = getattr(lib, entry)
        row = [args[n] for n in _TM_PARAMS[entry]] + [None]
        assert len(row) == len(fn.argtypes), entry
        return fn(*row), lib.impnn_last_error_string()

    assert set(_TM_PARAMS) == {n for n in _lib.SIGNATURES if "message" in n and "typed_" in n and not n.endswith("_bytes")}
    for entry, names in _TM_PARAMS.items():
        short = entry[len("impnn_"):].encode()
        # 1. shape, before everything else
        for kw in (dict(N=0), dict(N=0, B=0, **nulls), dict(B=-1), dict(E=-1), dict(D=0), dict(Vb=0)):
            rc, msg = call(entry, **kw)
            assert rc == _BAD and b"bad shape" in msg and short in msg, (entry, kw, msg)
        # 2. zero work is a success with no pointer looked at
        for kw in (dict(B=0), dict(E=0), dict(B=0, E=0)):
            assert call(entry, workspace_bytes=0, **nulls, **kw)[0] == 0, (entry, kw)
        # 3. null pointers: all of them, each one alone, and before the workspace size
        for kw in [dict(nulls), dict(nulls, workspace_bytes=0)] + [{n: None} for n in names if n in _TM_POINTERS]:
            rc, msg = call(entry, **kw)
            assert rc == _BAD and b"null pointer" in msg and short in msg, (entry, kw, msg)
        # 4. a workspace one byte short, before the coverage rules
        for kw in (dict(), dict(Vb=4097), dict(D=129), dict(B=1, E=1, Vb=1)):
            args = dict(B=3, E=11, Vb=5)
            args.update(kw)
            size = need(args["B"], args["E"], args["Vb"])
            assert size == 4 * (4 * (args["Vb"] + 1) + args["B"] * args["E"])
            rc, msg = call(entry, workspace_bytes=size - 1, **kw)
            assert rc == _WS and b"too small" in msg and short in msg, (entry, kw, msg)
        # 5. coverage: more than 4096 bond types, then atom_dim above 128 (the claimed workspace is large enough)
        for kw, what in ((dict(Vb=4097), b"Vb=4097"), (dict(D=129), b"D=129"), (dict(Vb=4097, D=129), b"Vb=4097")):
            rc, msg = call(entry, **kw)
            assert rc == _UNS and what in msg, (entry, kw, msg)
            rc, msg = call(entry, workspace_bytes=need(3, 11, kw.get("Vb", 5)), **kw)  # exactly enough
            assert rc == _UNS and what in msg, (entry, kw, msg)
    rc, msg = call("impnn_message_reduce_typed_bwd_scratch", edge_scratch=None)
    assert rc == _BAD and b"null pointer" in msg


# ---- the model head family's argument rules, pinned entry by entry (recorded on the entries as they were before their
# checks were shared).  Every call returns before any device call: pointers that must not be null are addresses inside
# a host buffer that nothing dereferences, the two pointer tables and l2 are real host arrays, and a case that has to
# show that a check passed carries a width above the limit, so that it ends as unsupported.
_MH_SHAPE = ["B", "D", "F", "Mx"]
_MH_PARAMS = {
    "impnn_model_head": ["kind", "pc", "pa", "T", "w", "out"] + _MH_SHAPE,
    "impnn_model_head_tensors": ["kind", "pc", "pa", "T", "weights", "out"] + _MH_SHAPE,
    "impnn_model_head_bwd": ["kind", "pc", "pa", "T", "weights", "dout", "dpc", "dpa", "dweights"] + _MH_SHAPE,
    "impnn_model_head_loss": ["kind", "pc", "pa", "T", "weights", "l2", "y", "pred", "loss", "workspace",
                              "workspace_floats"] + _MH_SHAPE,
    "impnn_model_head_loss_bwd": ["kind", "pc", "pa", "T", "weights", "l2", "y", "dloss", "dpc", "dpa", "dweights"]
                                 + _MH_SHAPE,
}
_MH_POINTERS = ("pc", "pa", "T", "w", "out", "weights", "dout", "dpc", "dpa", "dweights", "l2", "y", "pred", "loss",
                "dloss", "workspace")
_MH_OPTIONAL = ("T", "pred")  # T: kind 1 takes none; pred: the loss forward may drop the predictions
_MH_KIND = b"kind must be 0 (viscosity) or 1 (melting point)"


def test_model_head_status_codes_are_pinned():
    """Status code and error text of the five model head entries for each class of refusal, in the order the rules
    apply: kind, shape, zero work, null pointers, workspace size (loss forward), then in the launcher widths, null
    weight / gradient tensor i, LDS fit."""
    lib = _lib.load()
    host = (C.c_char * 512)()
    at = C.addressof(host)
    n_t = {0: 10, 1: 12}

    def table(null_at=()):
        t = (C.c_void_p * 12)(*[at + 16 * (i + 1) for i in range(12)])
        for i in null_at:
            t[i] = None
        return C.cast(t, _lib.PP)

    ptrs = {n: at + 16 * (i + 1) for i, n in enumerate(_MH_POINTERS)}
    ptrs.update(weights=table(), dweights=table(), l2=(C.c_float * 12)())
    nulls = {n: None for n in _MH_POINTERS}
    need = lib.impnn_model_head_loss_workspace_floats

    def call(entry, **kw):
        args = dict(ptrs, kind=0, B=9, D=32, F=32, Mx=20)
        args.update(kw)
        args.setdefault("workspace_floats", 1 << 40)
        fn = getattr(lib, entry)
        row = [args[n] for n in _MH_PARAMS[entry]] + [None]
        assert len(row) == len(fn.argtypes), entry
        return fn(*row), lib.impnn_last_error_string()

    assert set(_MH_PARAMS) == {n for n in _lib.SIGNATURES if n.startswith("impnn_model_head") and
                               not n.endswith("_floats")}
    assert [need(b) for b in (-1, 0, 1, 8, 9)] == [4, 4, 5, 5, 6]
    for entry, names in _MH_PARAMS.items():
        short = entry.encode()
        loss = "_loss" in entry
        bwd = entry.endswith("_bwd")
        packed = entry == "impnn_model_head"
        launcher = b"model_head_bwd: " if bwd else b"model_head: "
        required = [n for n in names if n in _MH_POINTERS and n not in _MH_OPTIONAL]
        # 1. kind, before everything else
        for kw in (dict(kind=2), dict(kind=-1), dict(kind=2, B=-1, **nulls), dict(kind=2, B=0, D=0)):
            rc, msg = call(entry, **kw)
            assert rc == _BAD and msg == short + b": " + _MH_KIND, (entry, kw, msg)
        # 2. shape
        for kw in (dict(B=-1), dict(D=0), dict(F=0), dict(Mx=0), dict(B=-1, **nulls), dict(B=0, D=0, **nulls),
                   dict(D=-1, F=65)):
            rc, msg = call(entry, **kw)
            assert rc == _BAD and msg == short + b": bad shape", (entry, kw, msg)
        # 3. zero work: a success with no pointer looked at and no width judged (the plain entries); the loss entries
        # have no empty batch
        for kw in (dict(), dict(D=129), dict(F=65, Mx=65), dict(kind=1, D=129)):
            rc, msg = call(entry, B=0, workspace_floats=0, **nulls, **kw)
            if loss:
                assert rc == _BAD and msg == short + b": bad shape", (entry, kw, msg)
            else:
                assert rc == 0, (entry, kw, msg)
        # 4. null pointers: all of them, each required one alone, before the workspace size and the widths
        cases = [dict(nulls), dict(nulls, workspace_floats=0), dict(nulls, D=129)] + [{n: None} for n in required]
        cases += [dict(c, kind=1) for c in cases] + [dict(T=None), dict(T=None, D=129)]
        for kw in cases:
            rc, msg = call(entry, **kw)
            assert rc == _BAD and msg == short + b": null pointer", (entry, kw, msg)
        # the temperature is kind 0's alone, and the loss forward's predictions are optional: the call goes on to the
        # widths
        for kw in [dict(kind=1, T=None)] + ([dict(pred=None), dict(kind=1, pred=None, T=None)] if "pred" in names else []):
            rc, msg = call(entry, D=129, **kw)
            assert rc == _UNS and msg.startswith(launcher + b"dims D=129"), (entry, kw, msg)
        # 5. the loss forward's workspace one float short, before the widths; exactly enough passes
        if "workspace_floats" in names:
            for kw in (dict(), dict(D=129), dict(B=1), dict(B=8), dict(B=17, F=65), dict(kind=1, T=None)):
                size = need(kw.get("B", 9))
                rc, msg = call(entry, workspace_floats=size - 1, **kw)
                assert rc == _WS and msg == b"model_head_loss: workspace of %d floats is too small" % (size - 1), (entry, kw, msg)
            rc, msg = call(entry, workspace_floats=need(9), D=129)
            assert rc == _UNS, (entry, msg)
        # 6. widths, judged by the launcher, before the pointer tables are read
        for kw, dims in ((dict(D=129), (129, 32, 20)), (dict(F=65), (32, 65, 20)), (dict(Mx=65), (32, 32, 65)),
                         (dict(D=129, F=65, Mx=65), (129, 65, 65)), (dict(kind=1, D=4096), (4096, 32, 20))):
            for tables in (dict(), dict(weights=table(range(12)), dweights=table(range(12)))):
                rc, msg = call(entry, **kw, **tables)
                assert rc == _UNS and msg == launcher + b"dims D=%d (<= 128) F=%d Mx=%d (<= 64)" % dims, (entry, kw, msg)
        if packed:
            continue  # no table, and every width within the limits fits its LDS: the next step is the launch
        # 7. tensor i of a table is null: weight i, then gradient i, tensor by tensor; only the kind's own tensors count
        for kind in (0, 1):
            for i in range(n_t[kind]):
                rc, msg = call(entry, kind=kind, weights=table([i]), dweights=table([i]))
                assert rc == _BAD and msg == b"model_head: null weight tensor %d" % i, (entry, kind, i, msg)
                if not bwd:
                    continue
                rc, msg = call(entry, kind=kind, dweights=table([i]))
                assert rc == _BAD and msg == b"model_head_bwd: null gradient tensor %d" % i, (entry, kind, i, msg)
                if i + 1 < n_t[kind]:
                    rc, msg = call(entry, kind=kind, weights=table([i + 1]), dweights=table([i]))
                    assert rc == _BAD and msg == b"model_head_bwd: null gradient tensor %d" % i, (entry, kind, i, msg)
        if bwd:
            # a null past kind 0's ten tensors is not looked at: the call goes on to the LDS fit
            rc, msg = call(entry, kind=0, D=128, F=64, Mx=64, weights=table([10, 11]), dweights=table([10, 11]))
            assert rc == _UNS and msg == b"model_head_bwd: weights do not fit LDS", (entry, msg)
            # 8. LDS fit, after the tables: the backward keeps the weights and their gradient sums in LDS, 2 * padded
            # weight floats + 9216 floats of sample vectors against 156 KB, so 15 360 weight floats fit and 15 420 do not
            for kw in (dict(kind=0, D=128, F=64, Mx=64), dict(kind=1, D=128, F=64, Mx=64), dict(kind=0, D=128, F=48, Mx=30)):
                rc, msg = call(entry, **kw)
                assert rc == _UNS and msg == b"model_head_bwd: weights do not fit LDS", (entry, kw, msg)
                rc, msg = call(entry, dweights=table([3]), **kw)
                assert rc == _BAD and msg == b"model_head_bwd: null gradient tensor 3", (entry, kw, msg)
    assert lib.impnn_model_head_floats(0, 128, 48, 30) == 15417


def test_head_width_limits_match_the_library():
    """ops.HEAD_MAX_X / HEAD_MAX_DIM, which decide in model.py whether a head kernel is called, are the library's
    kHeadMaxX / kHeadMaxDim: impnn_head_ion_mix judges the widths before it finds that M = 0 leaves nothing to do."""
    from ionic_mpnn_amd import ops
    lib = _lib.load()
    X, Dm = ops.HEAD_MAX_X, ops.HEAD_MAX_DIM
    assert (X, Dm) == (128, 64)
    for kind in (0, 1):
        assert lib.impnn_head_ion_mix(kind, 0, None, None, None, 0, X, Dm, Dm, None) == 0
        for D, F, Mx in ((X + 1, Dm, Dm), (X, Dm + 1, Dm), (X, Dm, Dm + 1), (X + 1, Dm + 1, Dm + 1)):
            assert lib.impnn_head_ion_mix(kind, 0, None, None, None, 0, D, F, Mx, None) == _UNS, (D, F, Mx)
            assert lib.impnn_last_error_string() == b"impnn_head_ion_mix: dims D=%d (<= %d) F=%d Mx=%d (<= %d)" % (
                D, X, F, Mx, Dm)
