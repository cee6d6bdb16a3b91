"""CPU: the host side of top-k screening - the four entries of the selection family (declared, exported, bound), its
limits in common.h and ops.py, the status code and text of every argument rule in the rule order (every failing call
returns before a launch; the stand-in pointers are never dereferenced), the workspace query, the reference order
data.grid_top_k on hand-written grids, and the argument errors of MPNNModel.screen_top_k."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from ionic_mpnn_amd import _lib, data, model as MM, ops, synthetic

CPU = torch.device("cpu")
_BAD, _UNS, _WS = -1, -2, -4
_P = 0x100000   # a stand-in pointer (16-byte aligned)
ENTRIES = ("impnn_grid_topk_workspace_bytes", "impnn_grid_topk_max_temperatures", "impnn_head_grid_topk",
           "impnn_transfer_head_grid_topk")


def test_the_four_entries_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "impnn.h").read_text(), flags=re.S)
    raw = C.CDLL(str(_lib.lib_path()))
    for n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in impnn.h"
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} is not bound"
    assert _lib.load().impnn_abi_version() == 3  # additions only


def test_limits_in_common_h_and_ops_are_equal():
    text = (ROOT / "ionic_mpnn_amd" / "csrc" / "common.h").read_text()
    limit = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert limit("kSelectMaxK") == ops.SELECT_MAX_K == MM.SCREEN_MAX_K == 1024
    assert limit("kSelectMaxT") == ops.SELECT_MAX_T == _lib.load().impnn_grid_topk_max_temperatures() == 4


# ---------------------------------------------------------------- status codes, in the rule order
def _need(lib, family=0, C_=100, A=100, nT=2, k=100, workgroups=0):
    n = C.c_size_t(0)
    rc = lib.impnn_grid_topk_workspace_bytes(family, C_, A, nT, k, workgroups, C.byref(n))
    return rc, n.value


def _head(lib, **kw):
    a = dict(kind=0, mc=_P, ma=_P, T=_P, w=_P, k=5, largest=0, values=_P, cation=_P, anion=_P, ws=_P, ws_bytes=None,
             C=3, A=4, nT=2, D=32, F=32, Mx=20, workgroups=0)
    a.update(kw)
    if a["ws_bytes"] is None:
        rc, a["ws_bytes"] = _need(lib, 0, max(a["C"], 0), max(a["A"], 0), min(max(a["nT"], 0), 4), min(max(a["k"], 1), 1024),
                                  max(a["workgroups"], 0))
        if rc != 0:  # (a shape the query refuses too: the entry must refuse it before it looks at the size)
            a["ws_bytes"] = 1 << 40
    rc = lib.impnn_head_grid_topk(a["kind"], a["mc"], a["ma"], a["T"], a["w"], a["k"], a["largest"], a["values"], a["cation"],
                                  a["anion"], a["ws"], a["ws_bytes"], a["C"], a["A"], a["nT"], a["D"], a["F"], a["Mx"],
                                  a["workgroups"], None)
    return rc, lib.impnn_last_error_string()


def _transfer(lib, **kw):
    n = lib.impnn_transfer_grid_image_floats()
    a = dict(uc=_P, ua=_P, image=_P, image_floats=n, k=5, largest=0, values=_P, cation=_P, anion=_P, ws=_P, ws_bytes=None,
             C=3, A=4, workgroups=0)
    a.update(kw)
    if a["ws_bytes"] is None:
        rc, a["ws_bytes"] = _need(lib, 1, max(a["C"], 0), max(a["A"], 0), 0, min(max(a["k"], 1), 1024), max(a["workgroups"], 0))
        if rc != 0:
            a["ws_bytes"] = 1 << 40
    rc = lib.impnn_transfer_head_grid_topk(a["uc"], a["ua"], a["image"], a["image_floats"], a["k"], a["largest"], a["values"],
                                           a["cation"], a["anion"], a["ws"], a["ws_bytes"], a["C"], a["A"], a["workgroups"],
                                           None)
    return rc, lib.impnn_last_error_string()


_HEAD_NULLS = dict(mc=None, ma=None, T=None, w=None, values=None, cation=None, anion=None, ws=None)
_TRANSFER_NULLS = dict(uc=None, ua=None, image=None, values=None, cation=None, anion=None, ws=None)
# C * A = 2^32 exactly, and the largest product a call takes
_2_32 = dict(C=1 << 16, A=1 << 16)


def test_head_grid_topk_status_codes():
    lib = _lib.load()
    mp = dict(kind=1, nT=0, T=None)
    # 1. shape, before everything else (null pointers, zero work and a short workspace included)
    for kw, code, what in ((dict(C=-1), _BAD, b"bad shape"), (dict(A=-1), _BAD, b"bad shape"), (dict(nT=-1), _BAD, b"bad shape"),
                           (dict(D=0), _BAD, b"bad shape"), (dict(F=0), _BAD, b"bad shape"), (dict(Mx=-1), _BAD, b"bad shape"),
                           (dict(workgroups=-1), _BAD, b"bad shape"),
                           (dict(kind=2), _BAD, b"kind"), (dict(kind=-1), _BAD, b"kind"),
                           (dict(kind=1, nT=3), _BAD, b"nT must be 0"), (dict(kind=0, nT=0), _BAD, b"nT >= 1"),
                           (dict(k=0), _BAD, b"k=0"), (dict(k=-7), _BAD, b"k=-7"), (dict(k=1025), _UNS, b"k=1025"),
                           (dict(nT=5), _UNS, b"nT=5"), (dict(_2_32), _UNS, b"4294967296 pairs"),
                           (dict(D=129), _UNS, b"D=129"), (dict(Mx=65), _UNS, b"Mx=65"), (dict(F=65), _UNS, b"F=65"),
                           (dict(mp, D=129), _UNS, b"D=129")):
        for extra in ({}, _HEAD_NULLS, dict(_HEAD_NULLS, C=0), dict(_HEAD_NULLS, A=0), dict(ws_bytes=0)):
            args = dict(extra)
            args.update(kw)
            rc, msg = _head(lib, **args)
            assert rc == code and what in msg and b"impnn_head_grid_topk" in msg, (kw, extra, rc, msg)
    # 2. zero work: every pointer null, no workspace
    for kw in (dict(C=0), dict(A=0), dict(C=0, A=0), dict(mp, C=0), dict(mp, A=0), dict(C=0, k=1024, nT=4)):
        args = dict(_HEAD_NULLS, ws_bytes=0)
        args.update(kw)
        assert _head(lib, **args)[0] == 0, kw
    # 3. null pointers, before the workspace size: all, and each alone (the melting-point grid needs no temperatures)
    for kw in [_HEAD_NULLS] + [{n: None} for n in _HEAD_NULLS]:
        rc, msg = _head(lib, ws_bytes=0, **kw)
        assert rc == _BAD and b"null pointer" in msg, (kw, msg)
    for n in _HEAD_NULLS:
        if n != "T":
            rc, msg = _head(lib, **dict(mp, **{n: None}))
            assert rc == _BAD and b"null pointer" in msg, (n, msg)
    rc, msg = _head(lib, **dict(mp, T=_P))
    assert rc == _BAD and b"takes no temperatures" in msg
    rc, msg = _head(lib, ws=_P + 4)
    assert rc == _BAD and b"8-byte aligned" in msg
    # 4. the workspace, one byte short
    for kw in ({}, mp, dict(k=1024, nT=4, C=300, A=300, workgroups=7)):
        a = dict(C=3, A=4, nT=2, k=5, workgroups=0)
        a.update(kw)
        rc, need = _need(lib, 0, a["C"], a["A"], a["nT"], a["k"], a["workgroups"])
        assert rc == 0 and need > 0
        rc, msg = _head(lib, ws_bytes=need - 1, **kw)
        assert rc == _WS and b"workspace of %d bytes is too small (%d)" % (need - 1, need) in msg, (kw, msg)


def test_transfer_head_grid_topk_status_codes():
    lib = _lib.load()
    n = lib.impnn_transfer_grid_image_floats()
    for kw, code, what in ((dict(C=-1), _BAD, b"bad shape"), (dict(A=-2), _BAD, b"bad shape"),
                           (dict(image_floats=-1), _BAD, b"bad shape"), (dict(workgroups=-1), _BAD, b"bad shape"),
                           (dict(k=0), _BAD, b"k=0"), (dict(k=1025), _UNS, b"k=1025"),
                           (dict(_2_32), _UNS, b"4294967296 pairs")):
        for extra in ({}, _TRANSFER_NULLS, dict(_TRANSFER_NULLS, C=0), dict(ws_bytes=0)):
            args = dict(extra)
            args.update(kw)
            rc, msg = _transfer(lib, **args)
            assert rc == code and what in msg and b"impnn_transfer_head_grid_topk" in msg, (kw, extra, rc, msg)
    for kw in (dict(C=0), dict(A=0)):
        assert _transfer(lib, ws_bytes=0, image_floats=0, **dict(_TRANSFER_NULLS, **kw))[0] == 0, kw
    for kw in [_TRANSFER_NULLS] + [{x: None} for x in _TRANSFER_NULLS]:
        rc, msg = _transfer(lib, ws_bytes=0, image_floats=1, **kw)
        assert rc == _BAD and b"null pointer" in msg, (kw, msg)
    rc, msg = _transfer(lib, ua=_P + 4, ws_bytes=0)
    assert rc == _BAD and b"16-byte aligned" in msg
    rc, msg = _transfer(lib, image_floats=n - 1, ws_bytes=0)
    assert rc == _WS and b"image of %d floats is too small (%d)" % (n - 1, n) in msg
    rc, need = _need(lib, 1, 3, 4, 0, 5, 0)
    rc, msg = _transfer(lib, ws_bytes=need - 1)
    assert rc == _WS and b"workspace of %d bytes is too small (%d)" % (need - 1, need) in msg


def test_workspace_query():
    lib = _lib.load()
    # [workgroups][nT][k] entries of 8 bytes; one workgroup per tile at most (16 x 64 and 8 x 32 pairs)
    assert _need(lib, 0, 100, 100, 2, 100, 3) == (0, 3 * 2 * 100 * 8)
    assert _need(lib, 0, 16, 64, 1, 10, 9) == (0, 1 * 1 * 10 * 8)
    assert _need(lib, 0, 17, 65, 0, 10, 9) == (0, 4 * 1 * 10 * 8)
    assert _need(lib, 1, 9, 33, 0, 7, 0) == (0, 4 * 1 * 7 * 8)
    assert _need(lib, 0, 0, 5, 1, 10, 0) == (0, 0)
    big = dict(C_=5000, A=5000)
    for name, values in (("k", (1, 2, 100, 1023, 1024)), ("nT", (1, 2, 3, 4)), ("workgroups", (1, 2, 7, 300, 5000))):
        sizes = []
        for v in values:
            rc, need = _need(lib, **dict(big, **{name: v}))
            assert rc == 0
            sizes.append(need)
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1], (name, sizes)
    default = _need(lib, workgroups=0, **big)[1]
    assert default == _need(lib, workgroups=default // (2 * 100 * 8), **big)[1] > 0  # 0 is some positive count
    for kw, code in ((dict(family=2), _BAD), (dict(k=0), _BAD), (dict(k=1025), _UNS), (dict(nT=5), _UNS),
                     (dict(C_=1 << 16, A=1 << 16), _UNS), (dict(workgroups=-1), _BAD), (dict(C_=-1), _BAD)):
        assert _need(lib, **kw)[0] == code and b"impnn_grid_topk_workspace_bytes" in lib.impnn_last_error_string(), kw
    assert lib.impnn_grid_topk_workspace_bytes(0, 1, 1, 1, 1, 0, None) == _BAD
    assert _need(lib, 0, 65535, 65537, 1, 1, 0)[0] == 0   # 2^32 - 1 pairs


# ---------------------------------------------------------------- the reference order
def f32(*v):
    return np.array(v, np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_grid_top_k_ties_go_by_index():
    g = f32(2, 1, 2, 1, 1, 3).reshape(2, 3)
    got = data.grid_top_k(g, 4)
    assert got.values.tolist() == [1, 1, 1, 2] and got.cation.tolist() == [0, 1, 1, 0] and got.anion.tolist() == [1, 0, 1, 0]
    assert got.values.dtype == np.float32 and got.cation.dtype == np.int64 and got.anion.dtype == np.int64
    got = data.grid_top_k(g, 3, largest=True)
    assert got.values.tolist() == [3, 2, 2] and got.cation.tolist() == [1, 0, 0] and got.anion.tolist() == [2, 0, 2]
    flat = data.grid_top_k(np.full((4, 5), 7.0, np.float32), 6)
    assert (flat.cation * 5 + flat.anion).tolist() == [0, 1, 2, 3, 4, 5]


def test_grid_top_k_orders_the_zeros_and_puts_nans_last():
    g = f32(0.0, -0.0, np.nan, 1.0, -1.0, -0.0, -np.inf, np.inf).reshape(2, 4)
    lo = data.grid_top_k(g, 8)
    assert np.array_equal(bits(lo.values), bits(f32(-np.inf, -1.0, -0.0, -0.0, 0.0, 1.0, np.inf, np.nan)))
    assert (lo.cation * 4 + lo.anion).tolist() == [6, 4, 1, 5, 0, 3, 7, 2]
    hi = data.grid_top_k(g, 8, largest=True)
    assert np.array_equal(bits(hi.values), bits(f32(np.inf, 1.0, 0.0, -0.0, -0.0, -1.0, -np.inf, np.nan)))
    assert (hi.cation * 4 + hi.anion).tolist() == [7, 3, 0, 1, 5, 4, 6, 2]
    # every NaN is the quiet NaN on output, whatever its sign and payload, and NaNs go by index
    odd = np.array([0xFFC00001, 0x7F800001, 0x3F800000], np.uint32).view(np.float32).reshape(1, 3)
    for largest in (False, True):
        got = data.grid_top_k(odd, 3, largest)
        assert bits(got.values).tolist() == [0x3F800000, 0x7FC00000, 0x7FC00000] and got.anion.tolist() == [2, 0, 1]
    assert data.select_keys(f32(-0.0, 0.0)).tolist() == [0x7FFFFFFF, 0x80000000]
    assert data.select_keys(f32(np.nan, -np.nan), largest=True).tolist() == [0xFFFFFFFF] * 2


def test_grid_top_k_shapes():
    g = np.arange(6, dtype=np.float32).reshape(2, 3)
    got = data.grid_top_k(g, 10)                       # k > size
    assert got.values.tolist() == [0, 1, 2, 3, 4, 5] and got.cation.shape == (6,)
    g3 = np.stack([g, -g], axis=-1)                    # (C,A,nT): a row per temperature
    got = data.grid_top_k(g3, 2)
    assert got.values.tolist() == [[0, 1], [-5, -4]] and got.cation.tolist() == [[0, 0], [1, 1]] and got.anion.tolist() == [[0, 1], [2, 1]]
    assert data.grid_top_k(g3, 10).values.shape == (2, 6)
    empty = data.grid_top_k(np.empty((0, 3), np.float32), 4)
    assert empty.values.shape == (0,) and empty.cation.shape == (0,)
    with pytest.raises(ValueError, match="k must be"):
        data.grid_top_k(g, 0)
    with pytest.raises(ValueError, match="grid must be"):
        data.grid_top_k(np.zeros(4, np.float32), 1)


# ---------------------------------------------------------------- Python-side errors
def _species(n, seed, N=40, E=80):
    b = synthetic.make_batch(n, max_atoms=N, max_edges=E, seed=seed, with_temperature=False)
    return {k: b[f"cat_{k}"] for k in MM.ION_KEYS}, {k: b[f"an_{k}"] for k in MM.ION_KEYS}


def test_screen_top_k_argument_errors():
    cat, an = _species(2, 1)
    v = MM.build_model(synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, num_steps=1, device=CPU)
    with pytest.raises(KeyError, match="temperature"):
        v.screen_top_k(cat, an)
    with pytest.raises(ValueError, match="max_pairs_per_launch"):
        v.screen_top_k(cat, an, temperatures=[300.0], max_pairs_per_launch=0)
    with pytest.raises(ValueError, match="both"):
        v.screen_top_k(cat, None, temperatures=[300.0])
    with pytest.raises(ValueError, match="k must be"):
        v.screen_top_k(cat, an, temperatures=[300.0], k=0)
    with pytest.raises(ValueError, match="at least one"):
        v.screen_top_k(cat, an, temperatures=[])
    with pytest.raises(KeyError):
        v.screen_top_k({"atom": cat["atom"]}, an, temperatures=[300.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v.screen_top_k(cat, an, temperatures=[300.0, 310.0], k=3)
    w = torch.zeros(_lib.load().impnn_model_head_floats(0, 32, 32, 20))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.head_grid_topk("viscosity", torch.zeros(2, 20), torch.zeros(3, 20), torch.zeros(2), w, 32, 20, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.transfer_head_grid_topk(torch.zeros(2, 256), torch.zeros(3, 256), torch.zeros(8), 4)
