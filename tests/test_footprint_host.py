"""CPU: the footprint inventory (tests/footprint.py) against include/impnn.h, the guard logic on a numpy stand-in, and
the size queries at the shapes tests/test_gpu_footprint.py runs.  Nothing here needs a GPU, and the inventory checks
read the test files by AST, without importing torch."""
import ast
import ctypes as C
import re

import numpy as np
import pytest

import footprint as F
from conftest import ROOT
from ionic_mpnn_amd import _lib

TESTS = ROOT / "tests"


# ---------------------------------------------------------------- 1. the inventory
def inventory_gaps(entries):
    """Entries with a non-const pointer parameter that COVERAGE does not name."""
    return sorted(n for n, e in entries.items() if e["mutable"] and n not in F.COVERAGE)


def test_the_parser_reads_every_prototype():
    entries = F.entries()
    assert set(entries) == set(_lib.SIGNATURES), "entries() and the ctypes table disagree about the header"
    for name, e in entries.items():
        assert len(e["params"]) == len(_lib.SIGNATURES[name][1]), name
    gu = entries["impnn_gated_update_rows_bwd_saved"]
    assert gu["mutable"] == ["dh", "dagg", "dparams", "workspace", "saved"] and "row_index" in gu["const"]
    enc = entries["impnn_encoder_fused"]
    assert enc["mutable"] == ["pooled", "workspace"] and "weights" in enc["const"]   # float* const* is an output table
    assert entries["impnn_encoder_plan_layout"]["mutable"] == ["out"]                # int64_t out[8]
    assert entries["impnn_abi_version"] == {"ret": "int", "const": [], "mutable": [], "params": []}


def test_every_writing_entry_is_covered_or_exempt():
    entries = F.entries()
    assert inventory_gaps(entries) == []
    assert sorted(set(F.COVERAGE) - set(entries)) == [], "COVERAGE names an entry the header does not declare"
    for name, why in F.COVERAGE.items():
        if why.startswith("exempt: "):
            query = re.search(r"_(bytes|floats|layout|records)$", name) is not None
            assert query or name.startswith("impnn_profile_") or name == "impnn_debug_set_stamp_buffer", \
                f"{name}: only queries, the profiler and the debug hook are exempt"


def test_a_new_prototype_fails_the_inventory_with_its_name():
    text = F.HEADER.read_text().replace("#ifdef __cplusplus\n}", "int impnn_x(float* out, int32_t n, impnn_stream_t stream);\n"
                                        "#ifdef __cplusplus\n}", 1)
    assert inventory_gaps(F.entries(text)) == ["impnn_x"]
    text = text.replace("int impnn_x(float* out,", "int impnn_x(const float* in,")
    assert inventory_gaps(F.entries(text)) == [], "an entry that writes nothing needs no footprint test"


def _module_tree(module):
    return ast.parse((TESTS / f"{module}.py").read_text())


def test_every_named_test_exists_and_names_its_entry():
    trees, sources = {}, {}
    for name, where in F.COVERAGE.items():
        if where.startswith("exempt: "):
            continue
        module, test = where.split("::")
        if module not in trees:
            trees[module] = _module_tree(module)
            sources[module] = (TESTS / f"{module}.py").read_text()
        defs = {n.name for n in trees[module].body if isinstance(n, ast.FunctionDef)}
        assert test in defs, f"{name}: {where} does not exist"
        assert re.search(rf"\b{name}\b", sources[module]), f"{name}: {module}.py never names it"
        assert re.search(r"\bGuarded\(|\bguarded\(|GUARD", sources[module]), f"{module}.py has no guarded buffer"
    src = sources["test_gpu_footprint"]
    assert "max(need" not in src and "1 << 20" not in src, "a floor under a buffer size of the footprint file"


# ---------------------------------------------------------------- 2. the guard logic reports a planted write
def test_the_guard_logic_reports_a_planted_write():
    for offset in (0, 4, 8):
        g = F.HostGuarded(52, fill=0x00, offset=offset)
        assert len(g.whole) == 2 * F.GUARD + offset + 52 and F.GUARD >= 4096
        assert not g.body(np.uint8, "out").any()
        g.whole[g.lo - 1] ^= 0xFF
        with pytest.raises(AssertionError, match="write before the workspace.*nearest 1 bytes"):
            g.body(np.uint8, "the workspace")
        g.whole[g.lo - 1] ^= 0xFF
        g.whole[g.lo + g.n] ^= 0xFF
        with pytest.raises(AssertionError, match="write past dparams.*first 0 bytes"):
            g.body(np.float32, "dparams")
        g.whole[g.lo + g.n] ^= 0xFF
        g.whole[-1] = 0
        with pytest.raises(AssertionError, match="write past dparams"):
            g.body(np.float32, "dparams")
    snap = np.arange(13, dtype=np.float32)
    g = F.HostGuarded(52, fill=snap.view(np.uint8))
    g.unchanged(snap, "the input h")
    g.unchanged(snap.tobytes(), "the input h")
    g.whole[g.lo + 17] ^= 0x01
    with pytest.raises(AssertionError, match="the input h changed: 1 bytes, the first at byte 17"):
        g.unchanged(snap, "the input h")


# ---------------------------------------------------------------- 3. the size queries, on the CPU build
def encoder_bytes(lib, n_ions, B, D, mode, workgroups=0, N=13, E=27, K=8, S=2, Vb=5):
    need = C.c_size_t(0)
    rc = lib.impnn_encoder_workspace_bytes(n_ions, B, N, E, D, K, S, Vb, mode, workgroups, C.byref(need))
    assert rc == 0, (rc, lib.impnn_last_error_string())
    return need.value


BATCHES = (1, 3, 5, 9, 33, 70)


def monotone(f, what):
    vals = [int(f(b)) for b in BATCHES]
    assert all(v > 0 for v in vals), f"{what}: {vals}"
    assert all(a <= b for a, b in zip(vals, vals[1:])), f"{what} is not monotone in B: {vals}"


def test_the_size_queries_answer_without_a_device_positive_and_monotone():
    lib = _lib.load()
    for mode, D in ((0, 32), (2, 32), (3, 32), (2, 64), (3, 64), (2, 128), (3, 128)):
        for n_ions in (1, 2):
            for wgs in (0, 16):
                monotone(lambda b: encoder_bytes(lib, n_ions, b, D, mode, wgs), f"encoder workspace, mode {mode}, D {D}")
        for S, Va, Vb in ((2, 9, 5), (1, 1, 1), (1, 1, 5), (1, 9, 1)):
            plain = lib.impnn_encoder_prepared_bytes(D, S, Vb, mode)
            atoms = lib.impnn_encoder_prepared_bytes_atoms(D, S, Va, Vb, mode)
            gates = lib.impnn_encoder_prepared_bytes_gates(D, S, Va, Vb, mode)
            assert 0 < plain <= atoms <= gates and plain % 16 == 0 and gates % 16 == 0
            if D == 32 and mode >= 2:   # the documented sizes of the two step-0 tables
                assert atoms == plain + Vb * (Va + 1) * 128
                assert gates == (atoms + (Va + 1) * 256 + 15) // 16 * 16
            else:
                assert plain == atoms == gates
    assert lib.impnn_encoder_prepared_bytes(64, 2, 5, 0) == 0 and lib.impnn_encoder_prepared_bytes(40, 2, 5, 2) == 0
    for D in (8, 32, 64, 128):
        monotone(lambda b: lib.impnn_gated_update_bwd_workspace_floats(b * 7, D), f"gated_update_bwd workspace, D {D}")
        assert lib.impnn_gated_update_param_floats(D) == 3 * (2 * D * D + D) + 2 * D
    for D in (64, 128):
        monotone(lambda b: lib.impnn_gated_update_rows_bwd_workspace_floats(b * 7, D), f"rows_bwd workspace, D {D}")
        assert lib.impnn_gated_update_rows_bwd_workspace_floats(37, D) == \
            lib.impnn_gated_update_bwd_workspace_floats(37, D) + 37 * 2 * D   # + the compact copies of h and agg
    for D in (32, 64, 128):
        assert lib.impnn_gated_update_rows_saved_floats(37, D) == 4 * D * 37
    assert lib.impnn_gated_update_rows_saved_floats(37, 40) == 0
    for Vb in (1, 5, 1025):   # the three sort paths test_gpu_train_fuzz.py names
        monotone(lambda b: lib.impnn_bmm_message_typed_bwd_workspace_bytes(b, 11, Vb), f"typed message sort, Vb {Vb}")
        assert lib.impnn_bmm_message_typed_bwd_workspace_bytes(3, 11, Vb) == 4 * (4 * (Vb + 1) + 3 * 11)
    for D in (16, 64):
        assert lib.impnn_bond_type_matrices_multi_bwd_workspace_floats(4, 5, 8, D) > 0
    monotone(lib.impnn_model_head_loss_workspace_floats, "model_head_loss workspace")
    monotone(lib.impnn_transfer_head_loss_workspace_floats, "transfer_head_loss workspace")
    monotone(lambda b: lib.impnn_transfer_head_saved_floats(b, 32, 20), "transfer head saved")
    monotone(lambda b: lib.impnn_transfer_head_bwd_workspace_floats(b, 32, 20), "transfer head bwd workspace")
    assert lib.impnn_adam_step_scheduled_workspace_floats(3) > 0 and lib.impnn_transfer_grid_image_floats() > 0
    assert lib.impnn_regression_sums_words() == 8 and lib.impnn_model_head_floats(0, 32, 32, 20) > 0


def gu_bwd_regions(rows, D, row_list=False):
    """GuBwdPlan's regions (gated_update_bwd.hip), in floats and in workspace order."""
    wide = D in (64, 128)
    tile_rows = (16 if rows < 8192 else 64) if wide else 256 // D          # main-kernel tile
    nblk = min(max(-(-rows // tile_rows), 1), 1024)                          # one slice of `small` per workgroup
    big = D % 64 == 0 and (2 * D) % 128 == 0 and rows >= 8192                # 128 x 64 GEMM tiles, else 64 x 32
    gm, gn = (128, 64) if big else (64, 32)
    tiles = -(-2 * D // gm) * -(-D // gn)
    nchunk = max(min(-(-(768 if big else 1024) // (3 * tiles)), -(-rows // 256)), 1)
    regions = [("dpre", rows * 3 * D), ("rh", rows * D), ("small", nblk * 5 * D), ("gpart", 3 * nchunk * 2 * D * D),
               ("wt", 3 * 2 * D * D)]
    if row_list:
        regions += [("hc", rows * D), ("aggc", rows * D)]
    return regions


def test_the_gated_update_backward_workspace_is_the_sum_of_its_regions():
    lib = _lib.load()
    total = lambda *a: sum(n for _, n in gu_bwd_regions(*a))
    assert total(37, 32) == 17824 and dict(gu_bwd_regions(37, 32))["small"] == 5 * 5 * 32
    assert total(9000, 128) == 8335488 and total(9000, 128, True) == 10639488
    for D in (8, 16, 32, 64, 128, 256):
        for rows in (0, 1, 255, 256, 257, 8191, 8192, 8193, 16384 * 4 + 1, 70001):
            assert lib.impnn_gated_update_bwd_workspace_floats(rows, D) == total(rows, D), (rows, D)
            if D in (64, 128):
                assert lib.impnn_gated_update_rows_bwd_workspace_floats(rows, D) == total(rows, D, True), (rows, D)
