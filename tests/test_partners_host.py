"""CPU: the host side of the best-partner screen - the three entries (declared, exported, bound), the limit in common.h
and ops.py, the status codes of the shape rules and the workspace query (every failing call returns before a launch;
the stand-in pointers are never dereferenced), and the reference data.grid_best_partners against a plain double loop
over the 64-bit entries on hand-made grids: ties, signed zeros, NaNs, padding, masks, bad arguments."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import ROOT
from ionic_mpnn_amd import _lib, data, ops

_BAD, _UNS, _WS = -1, -2, -4
_P = 0x100000   # a stand-in pointer (16-byte aligned)
ENTRIES = ("impnn_grid_partners_workspace_bytes", "impnn_head_grid_partners", "impnn_transfer_head_grid_partners")
NONE = (1 << 64) - 1


def test_the_three_entries_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "impnn.h").read_text(), flags=re.S)
    raw = C.CDLL(str(_lib.lib_path()))
    for n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in impnn.h"
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} is not bound"
    assert _lib.load().impnn_abi_version() == 3  # additions only


def test_the_limit_in_common_h_and_ops_is_equal():
    text = (ROOT / "ionic_mpnn_amd" / "csrc" / "common.h").read_text()
    assert int(re.search(r"constexpr int kPartnersMaxM = (\d+);", text).group(1)) == ops.PARTNERS_MAX_M == 8


# ---------------------------------------------------------------- the workspace query and the shape rules
def _need(lib, family=0, C_=100, A=100, nT=2, m=3):
    n = C.c_size_t(0)
    return lib.impnn_grid_partners_workspace_bytes(family, C_, A, nT, m, C.byref(n)), n.value


def test_workspace_query():
    lib = _lib.load()
    # rows [nT][tiles_a][C][m] + cols [nT][tiles_c][A][m] of 8-byte entries; tiles of 16 x 64 and 8 x 32 pairs
    assert _need(lib, 0, 100, 100, 2, 3) == (0, 8 * 2 * 3 * (2 * 100 + 7 * 100))
    assert _need(lib, 0, 17, 130, 0, 8) == (0, 8 * 1 * 8 * (3 * 17 + 2 * 130))
    assert _need(lib, 1, 20, 70, 0, 1) == (0, 8 * (3 * 20 + 3 * 70))
    assert _need(lib, 0, 0, 5, 1, 1) == (0, 0)
    for kw, code in ((dict(family=2), _BAD), (dict(C_=-1), _BAD), (dict(m=0), _BAD), (dict(m=9), _UNS), (dict(nT=5), _UNS),
                     (dict(C_=1 << 16, A=1 << 16), _UNS)):
        assert _need(lib, **kw)[0] == code, kw
    assert _need(lib, C_=(1 << 16) - 1, A=1 << 16)[0] == 0
    assert lib.impnn_grid_partners_workspace_bytes(0, 4, 4, 1, 1, None) == _BAD


def _head(lib, **kw):
    a = dict(kind=0, mc=_P, ma=_P, T=_P, w=_P, where=None, m=2, largest=0, cv=_P, cp=_P, av=_P, ap=_P, ws=_P, ws_bytes=1 << 40,
             C=3, A=4, nT=2, D=32, F=32, Mx=20)
    a.update(kw)
    rc = lib.impnn_head_grid_partners(a["kind"], a["mc"], a["ma"], a["T"], a["w"], a["where"], a["m"], a["largest"], a["cv"],
                                      a["cp"], a["av"], a["ap"], a["ws"], a["ws_bytes"], a["C"], a["A"], a["nT"], a["D"],
                                      a["F"], a["Mx"], None)
    return rc, lib.impnn_last_error_string().decode()


def _transfer(lib, **kw):
    a = dict(uc=_P, ua=_P, image=_P, image_floats=lib.impnn_transfer_grid_image_floats(), where=None, m=2, largest=0, cv=_P,
             cp=_P, av=_P, ap=_P, ws=_P, ws_bytes=1 << 40, C=3, A=4)
    a.update(kw)
    rc = lib.impnn_transfer_head_grid_partners(a["uc"], a["ua"], a["image"], a["image_floats"], a["where"], a["m"],
                                               a["largest"], a["cv"], a["cp"], a["av"], a["ap"], a["ws"], a["ws_bytes"],
                                               a["C"], a["A"], None)
    return rc, lib.impnn_last_error_string().decode()


def test_entries_refuse_bad_requests_before_a_launch():
    lib = _lib.load()
    for call in (_head, _transfer):
        for kw, code, text in ((dict(m=0), _BAD, "m=0 must be at least 1"), (dict(m=9), _UNS, "m=9 partners (<= 8 per call)"),
                               (dict(C=-1), _BAD, "bad shape"), (dict(C=1 << 16, A=1 << 16), _UNS, "pairs (< 2^32 per call)"),
                               (dict(cv=None), _BAD, "null pointer"), (dict(ap=None), _BAD, "null pointer"),
                               (dict(ws=None), _BAD, "null pointer"), (dict(ws=_P + 4), _BAD, "8-byte aligned"),
                               (dict(where=_P + 2), _BAD, "4-byte aligned"), (dict(ws_bytes=8), _WS, "too small")):
            rc, msg = call(lib, **kw)
            assert rc == code and text in msg and call.__name__[1:] in msg, (call.__name__, kw, rc, msg)
        assert call(lib, C=0)[0] == 0 and call(lib, A=0, cv=None, ws=None)[0] == 0   # zero work: nothing touched
    for kw, code, text in ((dict(kind=2), _BAD, "kind must be"), (dict(nT=0), _BAD, "needs nT >= 1"),
                           (dict(nT=5), _UNS, "nT=5 temperatures (<= 4 per selecting call)"),
                           (dict(kind=1, nT=1), _BAD, "nT must be 0"), (dict(Mx=65), _UNS, "Mx=65"), (dict(D=0), _BAD, "bad shape"),
                           (dict(T=None), _BAD, "null pointer"), (dict(kind=1, nT=0), _BAD, "takes no temperatures")):
        rc, msg = _head(lib, **kw)
        assert rc == code and text in msg, (kw, rc, msg)
    assert _transfer(lib, image_floats=16)[0] == _WS and _transfer(lib, uc=_P + 4)[0] == _BAD
    # the exact size is enough to pass the size rule (the next failure is none: it would launch, so stop at the query)
    need = _need(lib, 0, 3, 4, 2, 2)[1]
    assert _head(lib, ws_bytes=need - 1)[0] == _WS


# ---------------------------------------------------------------- the reference against a plain double loop
def entry(v, flat, largest):
    """The selection's 64-bit entry of one float32, written out by hand."""
    u = int(np.float32(v).view(np.uint32))
    key = (~u & 0xFFFFFFFF) if u & 0x80000000 else u ^ 0x80000000
    if largest:
        key = ~key & 0xFFFFFFFF
    if v != v:
        key = 0xFFFFFFFF
    return (key << 32) | flat


def loop_reference(grid, m, largest, where):
    """by_cation / by_anion of a (C,A) plane with python loops and sorted() over the entries."""
    Cn, An = grid.shape
    out = []
    for n_ions, n_part, pair in ((Cn, An, lambda i, p: (i, p)), (An, Cn, lambda j, p: (p, j))):
        vals, part = np.full((n_ions, m), data.QUIET_NAN, np.float32), np.full((n_ions, m), -1, np.int64)
        for ion in range(n_ions):
            cand = []
            for p in range(n_part):
                i, j = pair(ion, p)
                if where is None or where[i, j]:
                    cand.append((entry(grid[i, j], i * An + j, largest), p, grid[i, j]))
            for s, (_, p, v) in enumerate(sorted(cand)[:m]):
                vals[ion, s], part[ion, s] = (data.QUIET_NAN if v != v else v), p
        out.append((vals, part))
    return out


def check(grid, m, largest, where_b=None, where=None):
    got = data.grid_best_partners(grid, m, largest, where=where if where is not None else where_b)
    planes = np.moveaxis(grid, 2, 0) if grid.ndim == 3 else grid[None]
    for side, name in enumerate(("by_cation", "by_anion")):
        gv, gp = (np.asarray(x) for x in got[side])
        assert gv.dtype == np.float32 and gp.dtype == np.int64, name
        if grid.ndim == 2:
            gv, gp = gv[None], gp[None]
        assert gv.shape == gp.shape == (len(planes), grid.shape[side], m), name
        for t, plane in enumerate(planes):
            wv, wp = loop_reference(plane, m, largest, where_b)[side]
            assert np.array_equal(gv[t].view(np.uint32), wv.view(np.uint32)), (name, t, m, largest)
            assert np.array_equal(gp[t], wp), (name, t, m, largest)
    return got


def tricky(shape, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(-3, 4, size=shape).astype(np.float32)      # few distinct values: ties along every row and column
    g.reshape(-1)[rng.choice(g.size, g.size // 6, replace=False)] = np.nan
    flat = g.reshape(-1)
    zeros = np.flatnonzero(flat == 0)
    flat[zeros[::2]] = -0.0                                       # both zeros, in an order that is not the index order
    neg_nan = np.array([0xFFC00001], np.uint32).view(np.float32)[0]
    flat[np.flatnonzero(np.isnan(flat))[::3]] = neg_nan          # NaNs of another sign and payload
    return g


@pytest.mark.parametrize("shape", [(5, 7), (5, 7, 3), (1, 1), (6, 1, 2)], ids=str)
def test_reference_is_the_order_on_hand_made_grids(shape):
    g = tricky(shape, 7)
    assert np.isnan(g).any() or g.size < 6
    rng = np.random.default_rng(3)
    half = rng.random(shape[:2]) < 0.5
    hole = np.ones(shape[:2], bool)
    hole[0, :] = False                                            # a cation with no set bit
    hole[:, -1] = False                                           # an anion with no set bit
    for largest in (False, True):
        for m in (1, 3, 9):                                       # 9: above every partner count here, padded
            check(g, m, largest)
            check(g, m, largest, half)
            check(g, m, largest, half, where=data.PairMask.from_bool(half))
            got = check(g, m, largest, hole)
            first = (np.asarray(got.by_cation.partner).reshape(-1, shape[0], m)[:, 0],
                     np.asarray(got.by_anion.partner).reshape(-1, shape[1], m)[:, -1])
            assert (first[0] == -1).all() and (first[1] == -1).all(), "an ion without a bit is all padding"
            none = check(g, m, largest, np.zeros(shape[:2], bool))
            assert (np.asarray(none.by_cation.partner) == -1).all()
            assert (np.asarray(none.by_anion.values).view(np.uint32) == 0x7FC00000).all()


def test_ties_zeros_and_nans_by_hand():
    nan = np.float32(np.nan)
    g = np.array([[1.0, 0.0, -0.0, 1.0],
                  [nan, 2.0, 2.0, nan],
                  [1.0, 0.0, -0.0, 1.0]], np.float32)
    b = data.grid_best_partners(g, 4)
    assert b.by_cation.partner.tolist() == [[2, 1, 0, 3], [1, 2, 0, 3], [2, 1, 0, 3]]     # -0.0 first; ties by index; NaN last
    assert np.signbit(b.by_cation.values[0, 0]) and not np.signbit(b.by_cation.values[0, 1])
    assert b.by_anion.partner.tolist() == [[0, 2, 1, -1], [0, 2, 1, -1], [0, 2, 1, -1], [0, 2, 1, -1]]
    assert b.by_anion.values.view(np.uint32)[0].tolist()[2:] == [0x7FC00000, 0x7FC00000]   # the NaN, then the padding
    b = data.grid_best_partners(g, 2, largest=True)
    assert b.by_cation.partner.tolist() == [[0, 3], [1, 2], [0, 3]]                        # NaN last in this direction too
    assert b.by_anion.partner.tolist() == [[0, 2], [1, 0], [1, 0], [0, 2]]


@pytest.mark.parametrize("shape", [(5, 7), (5, 7, 3), (9, 4)], ids=str)
def test_the_best_first_partner_is_the_top_1(shape):
    rng = np.random.default_rng(11)
    g = rng.integers(-2, 3, size=shape).astype(np.float32)
    for largest in (False, True):
        b = data.grid_best_partners(g, 1, largest)
        top = data.grid_top_k(g, 1, largest)
        vals = np.asarray(b.by_cation.values).reshape(-1, shape[0])
        part = np.asarray(b.by_cation.partner).reshape(-1, shape[0])
        for t in range(vals.shape[0]):
            i = int(data.top_k_order(vals[t], np.arange(shape[0]), 1, largest)[0])   # the smallest entry over the cations
            assert i == np.atleast_2d(top.cation)[t, 0] and part[t, i] == np.atleast_2d(top.anion)[t, 0]
            assert vals[t, i].view(np.uint32) == np.atleast_2d(top.values)[t, 0].view(np.uint32)


def test_bad_arguments():
    g = np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError, match="grid must be"):
        data.grid_best_partners(np.zeros(3, np.float32))
    with pytest.raises(ValueError, match="m must be >= 1"):
        data.grid_best_partners(g, 0)
    with pytest.raises(ValueError, match="where must be a bool array or PairMask of shape"):
        data.grid_best_partners(g, 1, where=np.ones((4, 3), bool))
    with pytest.raises(ValueError, match="where must be a bool array or PairMask of shape"):
        data.grid_best_partners(g, 1, where=np.ones((3, 4), np.int32))
    with pytest.raises(ValueError, match="2-D PairMask"):
        data.grid_best_partners(np.zeros((3, 4, 2), np.float32), 1, where=data.PairMask.from_bool(np.ones((3, 4, 2), bool)))
    empty = data.grid_best_partners(np.zeros((0, 4), np.float32), 2)
    assert empty.by_cation.values.shape == (0, 2) and (empty.by_anion.partner == -1).all()
