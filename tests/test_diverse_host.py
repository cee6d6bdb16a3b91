"""CPU: the host side of the diverse batch (include/impnn.h, impnn_diverse_select): data.grid_diverse on cases worked
out by hand, the tie rule on rows of small integers, the argument rules of ops.domain_diverse that fire before any
library call, the status codes of the two C entries in their order (every failing call returns before a launch; no
pointer is dereferenced), and the build list."""
import ctypes as C

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, build, data, ops

from diverse_cases import INTEGER_K, greedy, integer_rows

_BAD, _UNS, _WS = -1, -2, -4


def line(xs):
    """Mixing rows of width 1: z(i,j) = cat[i] + an[j] on a line."""
    return np.asarray(xs, np.float32).reshape(-1, 1)


def test_grid_diverse_on_a_line():
    """1 cation x 6 anions at 0, 1, 2, 4, 8, 16, the reference at 0.  The picks: 16 (distance 16), then 8 (8: halfway),
    then 4 (4), 2 (2), 1 (1); pair 0 is the reference pair and never competes."""
    mc, ma, ref = line([0]), line([0, 1, 2, 4, 8, 16]), line([0])
    sel = data.grid_diverse(mc, ma, ref, 3)
    assert isinstance(sel, data.DiverseSelection) and sel.cation.dtype == sel.anion.dtype == np.int64
    assert sel.cation.tolist() == [0, 0, 0] and sel.anion.tolist() == [5, 4, 3]
    assert sel.distance.dtype == np.float64 and sel.distance.tolist() == [16.0, 8.0, 4.0]
    assert sel.competing == 5, "the reference pair (distance 0) is no candidate"
    # k beyond the candidates: the selection ends early, a chosen pair is never chosen again, the reference pair never
    full = data.grid_diverse(mc, ma, ref, 10)
    assert full.anion.tolist() == [5, 4, 3, 2, 1] and full.competing == 5 and len(full.cation) == 5
    assert full.distance.tolist() == [16.0, 8.0, 4.0, 2.0, 1.0]
    assert (np.diff(full.distance) <= 0).all(), "distance is non-increasing"
    assert len(set(zip(full.cation.tolist(), full.anion.tolist()))) == 5


def test_grid_diverse_ties_go_to_the_lowest_pair_index():
    """2 cations (0, 10) x 3 anions (-4, 0, 4), the reference at 5: z = [[-4, 0, 4], [6, 10, 14]], distances
    [[9, 5, 1], [1, 5, 9]].  (0,0) and (1,2) tie at 9: the lower flat index wins; then (1,2) at 9 again; then (0,1) and
    (1,1) tie at min(5, 4) = 4 against the picks -4 and 14."""
    mc, ma, ref = line([0, 10]), line([-4, 0, 4]), line([5])
    sel = data.grid_diverse(mc, ma, ref, 6)
    pairs = list(zip(sel.cation.tolist(), sel.anion.tolist()))
    assert pairs[:4] == [(0, 0), (1, 2), (0, 1), (1, 1)] and sel.distance[:4].tolist() == [9.0, 9.0, 4.0, 4.0]
    assert sorted(pairs[4:]) == [(0, 2), (1, 0)] and sel.distance[4:].tolist() == [1.0, 1.0] and sel.competing == 6


def test_grid_diverse_passes_over_nan_and_masked_pairs():
    mc, ma, ref = line([0, np.nan]), line([0, 1, 2, 4, 8, 16]), line([0])
    sel = data.grid_diverse(mc, ma, ref, 10)
    assert sel.cation.tolist() == [0] * 5 and sel.anion.tolist() == [5, 4, 3, 2, 1] and sel.competing == 5, "a NaN row"
    mc = line([0, 100])
    where = np.zeros((2, 6), np.bool_)
    where[0, [0, 1, 4]] = where[1, 2] = True
    sel = data.grid_diverse(mc, ma, ref, 10, where=where)
    # (1,2) at 102, then (0,4) at 8, then (0,1) at 1; (0,0) has its bit but lies on the reference
    assert list(zip(sel.cation.tolist(), sel.anion.tolist())) == [(1, 2), (0, 4), (0, 1)] and sel.competing == 3
    assert sel.distance.tolist() == [102.0, 8.0, 1.0]
    packed = data.grid_diverse(mc, ma, ref, 10, where=data.PairMask.from_bool(where))
    assert packed.anion.tolist() == sel.anion.tolist() and packed.competing == 3
    none = data.grid_diverse(mc, ma, ref, 10, where=np.zeros((2, 6), np.bool_))
    assert len(none.cation) == len(none.anion) == len(none.distance) == 0 and none.competing == 0
    assert none.cation.dtype == np.int64 and none.distance.dtype == np.float64
    with pytest.raises(ValueError, match="k must be"):
        data.grid_diverse(mc, ma, ref, 0)
    with pytest.raises(ValueError, match="where must be"):
        data.grid_diverse(mc, ma, ref, 3, where=np.zeros((2, 5), np.bool_))
    with pytest.raises(ValueError, match="R must be at least 1"):
        data.grid_diverse(mc, ma, np.zeros((0, 1), np.float32), 3)


def test_the_tie_rule_on_rows_of_small_integers():
    """Every operation is exact there: float32 and float64 arithmetic make the same picks, and many steps have exactly
    tied maxima, so the lowest-index rule decides them."""
    mc, ma, ref = integer_rows()
    sel = data.grid_diverse(mc, ma, ref, INTEGER_K)
    state, _ = data.grid_domain(mc, ma, ref)
    z = mc[:, None, :] + ma[None, :, :]
    p64, d64, tied64 = greedy(state, z, INTEGER_K, np.float64)
    p32, d32, tied32 = greedy(state, z, INTEGER_K, np.float32)
    print("tied steps", tied64)
    assert tied64 >= 10 and tied32 == tied64, "the case must exercise the tie rule"
    assert len(p64) == INTEGER_K and p32 == p64, "float32 and float64 pick the same pairs"
    assert (sel.cation * 130 + sel.anion).tolist() == p64
    assert np.array_equal(sel.distance, np.asarray(d64)) and np.array_equal(sel.distance.astype(np.float32), np.asarray(d32))
    assert (np.diff(sel.distance) <= 0).all() and (sel.distance > 0).all()
    assert sel.competing == 17 * 130 - 2


def test_ops_rules_fire_before_any_library_call():
    """Every rule but the last is met on CPU tensors: the device is judged after the shapes."""
    f = lambda *shape: torch.zeros(*shape)
    cases = [
        (lambda: ops.domain_diverse(f(3, 20), f(4, 20), f(20), 3), ValueError, "ref must be 2-D"),
        (lambda: ops.domain_diverse(f(3, 20), f(4, 19), f(5, 20), 3), ValueError, "mix_an has width 19"),
        (lambda: ops.domain_diverse(f(3, 65), f(4, 65), f(5, 65), 3), ValueError, "Mx=65"),
        (lambda: ops.domain_diverse(f(3, 20), f(4, 20), f(0, 20), 3), ValueError, "R must be at least 1"),
        (lambda: ops.domain_diverse(f(3, 20).double(), f(4, 20), f(5, 20), 3), TypeError, "mix_cat must be float32"),
        (lambda: ops.domain_diverse(f(3, 20), f(4, 20), f(5, 20), 3), RuntimeError, "no CPU fallback"),
    ]
    for call, error, text in cases:
        with pytest.raises(error, match=text):
            call()


def test_c_entries_refuse_bad_arguments_in_order():
    """Shape and k < 1 (BADARG), the width, k and pair-count limits (UNSUPPORTED), zero work, null pointers, alignment,
    the workspace size."""
    lib = _lib.load()
    cap = lib.impnn_diverse_max_k()
    assert cap == ops.DIVERSE_MAX_K >= 1024
    P = 0x100000  # a stand-in that is never dereferenced
    msg = lib.impnn_last_error_string
    need = C.c_size_t(0)

    def size(Cn=3, An=4, k=5, out=need):
        return lib.impnn_diverse_workspace_bytes(Cn, An, k, None if out is None else C.byref(out))

    assert size() == 0 and need.value >= 3 * 4 * 4 + 6 * 8 + 4 and need.value % 16 == 0
    small = need.value
    assert size(Cn=17, An=130) == 0 and need.value >= 17 * 130 * 4 + 6 * 8 + 6 * 4
    assert size(k=cap) == 0 and need.value >= 12 * 4 + (cap + 1) * 8
    assert size(Cn=-1) == _BAD and b"bad shape" in msg()
    assert size(k=0) == _BAD and b"k=0" in msg()
    assert size(k=cap + 1) == _UNS and b"picks" in msg()
    assert size(Cn=1 << 16, An=1 << 16) == _UNS and b"pairs" in msg()
    assert size(Cn=(1 << 16) - 1, An=1 << 16) == 0
    assert size(Cn=0, k=0) == _BAD and size(Cn=0) == 0
    assert size(out=None) == _BAD and b"null pointer" in msg()

    def select(Cn=3, An=4, R=5, Mx=20, k=5, p=P, where=None, ws=P, ws_bytes=1 << 20, counts=P):
        return lib.impnn_diverse_select(p, p, p, where, k, p, p, p, counts, ws, ws_bytes, Cn, An, R, Mx, None)

    assert select(Cn=-1) == _BAD and b"bad shape" in msg()
    assert select(An=-1, p=None) == _BAD and b"bad shape" in msg()
    assert select(Mx=0) == _BAD and b"bad shape" in msg()
    assert select(R=0) == _BAD and b"R=0" in msg()
    assert select(k=0) == _BAD and b"k=0" in msg()
    assert select(k=0, Mx=65) == _BAD and b"k=0" in msg()                 # k < 1 before the width limit
    assert select(R=0, k=cap + 1) == _BAD and b"R=0" in msg()
    assert select(Mx=65) == _UNS and b"Mx=65 (<= 64)" in msg()
    assert select(k=cap + 1) == _UNS and b"picks" in msg()
    assert select(Cn=1 << 16, An=1 << 16) == _UNS and b"pairs" in msg()
    assert select(Mx=65, Cn=0, p=None) == _UNS                             # the limits come before zero work
    assert select(Cn=0, p=None, ws=None) == 0 and select(An=0, p=None, ws=None) == 0   # zero work: nothing looked at
    assert select(p=None) == _BAD and b"null pointer" in msg()
    assert select(ws=None) == _BAD and b"null pointer" in msg()
    assert select(counts=None) == _BAD and b"null pointer" in msg()
    assert select(ws=P + 8) == _BAD and b"16-byte aligned" in msg()
    assert select(ws=P + 8, ws_bytes=0) == _BAD                            # alignment before the workspace size
    assert select(counts=P + 4) == _BAD and b"8-byte aligned" in msg()
    assert select(where=P + 2) == _BAD and b"4-byte aligned" in msg()
    assert select(ws_bytes=small - 1) == _WS and b"too small" in msg()
    assert select(where=P, ws_bytes=0) == _WS


def test_the_kernels_are_in_the_build():
    assert "grid_diverse.hip" in build.SOURCES and (build.CSRC / "grid_diverse.hip").exists()
    assert (build.CSRC / "domain_device.h").exists()
    assert {"impnn_diverse_max_k", "impnn_diverse_workspace_bytes", "impnn_diverse_select"} <= set(_lib.SIGNATURES)
    from ionic_mpnn_amd import MPNNModel, ModelEnsemble
    assert callable(MPNNModel.screen_diverse) and callable(ModelEnsemble.screen_diverse)
