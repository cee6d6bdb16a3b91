"""CPU: the host side of constrained screening - the five entries of the pair-mask feature (declared, exported, bound),
the status code and text of every argument rule of the four launching entries in the rule order (every failing call
returns before a launch; the stand-in pointers are never dereferenced), data.PairMask against numpy on bool arrays, the
masked reference order data.grid_top_k(where=) on hand-written grids, and the argument errors of
MPNNModel.screen_mask / screen_top_k(where=)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from ionic_mpnn_amd import _lib, data, model as MM, synthetic

CPU = torch.device("cpu")
_BAD, _UNS, _WS = -1, -2, -4
_P = 0x100000   # a stand-in pointer (16-byte aligned)
NAN, INF = float("nan"), float("inf")
ENTRIES = ("impnn_grid_mask_row_words", "impnn_head_grid_mask", "impnn_transfer_head_grid_mask",
           "impnn_head_grid_topk_where", "impnn_transfer_head_grid_topk_where")
_2_32 = dict(C=1 << 16, A=1 << 16)   # C * A = 2^32 exactly


def test_the_five_entries_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "impnn.h").read_text(), flags=re.S)
    raw = C.CDLL(str(_lib.lib_path()))
    for n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in impnn.h"
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} is not bound"
    assert _lib.load().impnn_abi_version() == 3  # additions only


def test_row_words():
    lib = _lib.load()
    assert [lib.impnn_grid_mask_row_words(a) for a in (1, 32, 33)] == [1, 1, 2]
    assert [lib.impnn_grid_mask_row_words(a) for a in (0, 31, 64, 65, 130, 2 ** 31 - 1)] == [0, 1, 2, 3, 5, 2 ** 26]
    assert [data.mask_row_words(a) for a in (0, 1, 31, 32, 33, 130)] == [0, 1, 1, 1, 2, 5]


# ---------------------------------------------------------------- the mask-writing entries, in the rule order
def _head_mask(lib, **kw):
    a = dict(kind=0, mc=_P, ma=_P, T=_P, w=_P, lo=-1.0, hi=1.0, words=_P, C=3, A=4, nT=2, D=32, F=32, Mx=20)
    a.update(kw)
    rc = lib.impnn_head_grid_mask(a["kind"], a["mc"], a["ma"], a["T"], a["w"], a["lo"], a["hi"], a["words"], a["C"], a["A"],
                                  a["nT"], a["D"], a["F"], a["Mx"], None)
    return rc, lib.impnn_last_error_string()


def _transfer_mask(lib, **kw):
    a = dict(uc=_P, ua=_P, image=_P, image_floats=lib.impnn_transfer_grid_image_floats(), lo=-1.0, hi=1.0, words=_P, C=3, A=4)
    a.update(kw)
    rc = lib.impnn_transfer_head_grid_mask(a["uc"], a["ua"], a["image"], a["image_floats"], a["lo"], a["hi"], a["words"],
                                           a["C"], a["A"], None)
    return rc, lib.impnn_last_error_string()


_HM_NULLS = dict(mc=None, ma=None, T=None, w=None, words=None)
_TM_NULLS = dict(uc=None, ua=None, image=None, words=None)


def test_head_grid_mask_status_codes():
    lib = _lib.load()
    mp = dict(kind=1, nT=0, T=None)
    # 1. shape, a NaN bound included, before everything else (null pointers, zero work and the limits)
    for kw, what in ((dict(C=-1), b"bad shape"), (dict(A=-1), b"bad shape"), (dict(nT=-1), b"bad shape"),
                     (dict(D=0), b"bad shape"), (dict(F=0), b"bad shape"), (dict(Mx=-1), b"bad shape"),
                     (dict(kind=2), b"kind"), (dict(kind=-1), b"kind"),
                     (dict(kind=1, nT=3), b"nT must be 0"), (dict(kind=0, nT=0), b"nT >= 1"),
                     (dict(lo=NAN), b"NaN"), (dict(hi=NAN), b"NaN"), (dict(mp, lo=NAN, hi=NAN), b"NaN")):
        for extra in ({}, _HM_NULLS, dict(_HM_NULLS, C=0), dict(_HM_NULLS, A=0), dict(D=129)):
            args = dict(extra)
            args.update(kw)
            rc, msg = _head_mask(lib, **args)
            assert rc == _BAD and what in msg and b"impnn_head_grid_mask" in msg, (kw, extra, rc, msg)
    # 2. zero work: every pointer null, infinite bounds allowed, before the limits
    for kw in (dict(C=0), dict(A=0), dict(C=0, A=0), dict(mp, C=0), dict(C=0, lo=-INF, hi=INF), dict(A=0, D=129),
               dict(C=0, nT=5000)):
        assert _head_mask(lib, **dict(_HM_NULLS, **kw))[0] == 0, kw
    # 3. null pointers: all, and each alone (the melting-point grid needs no temperatures), before the limits; the
    #    number of pairs is no limit of a mask (C * A = 2^32 gets as far as its pointers)
    for kw in [_HM_NULLS] + [{n: None} for n in _HM_NULLS] + [dict(words=None, D=129), dict(words=None, nT=5000),
                                                             dict(words=None, **_2_32)]:
        rc, msg = _head_mask(lib, **kw)
        assert rc == _BAD and b"null pointer" in msg, (kw, msg)
    for n in _HM_NULLS:
        if n != "T":
            rc, msg = _head_mask(lib, **dict(mp, **{n: None}))
            assert rc == _BAD and b"null pointer" in msg, (n, msg)
    rc, msg = _head_mask(lib, **dict(mp, T=_P))
    assert rc == _BAD and b"takes no temperatures" in msg
    # 4. alignment, before the limits
    for kw in (dict(words=_P + 2), dict(words=_P + 1, D=129)):
        rc, msg = _head_mask(lib, **kw)
        assert rc == _BAD and b"4-byte aligned" in msg, (kw, msg)
    # 5. the limits of one launch
    for kw, what in ((dict(D=129), b"D=129"), (dict(F=65), b"F=65"), (dict(Mx=65), b"Mx=65"), (dict(mp, D=129), b"D=129"),
                     (dict(nT=4097), b"nT=4097")):
        rc, msg = _head_mask(lib, **kw)
        assert rc == _UNS and what in msg and b"impnn_head_grid_mask" in msg, (kw, rc, msg)


def test_transfer_head_grid_mask_status_codes():
    lib = _lib.load()
    n = lib.impnn_transfer_grid_image_floats()
    for kw, what in ((dict(C=-1), b"bad shape"), (dict(A=-2), b"bad shape"), (dict(image_floats=-1), b"bad shape"),
                     (dict(lo=NAN), b"NaN"), (dict(hi=NAN), b"NaN")):
        for extra in ({}, _TM_NULLS, dict(_TM_NULLS, C=0), dict(words=_P + 1)):
            args = dict(extra)
            args.update(kw)
            rc, msg = _transfer_mask(lib, **args)
            assert rc == _BAD and what in msg and b"impnn_transfer_head_grid_mask" in msg, (kw, extra, rc, msg)
    for kw in (dict(C=0), dict(A=0), dict(C=0, lo=INF, hi=INF)):
        assert _transfer_mask(lib, image_floats=0, **dict(_TM_NULLS, **kw))[0] == 0, kw
    for kw in [_TM_NULLS] + [{x: None} for x in _TM_NULLS] + [dict(words=None, **_2_32)]:
        rc, msg = _transfer_mask(lib, image_floats=1, **kw)
        assert rc == _BAD and b"null pointer" in msg, (kw, msg)
    rc, msg = _transfer_mask(lib, ua=_P + 4, image_floats=1)
    assert rc == _BAD and b"16-byte aligned" in msg
    rc, msg = _transfer_mask(lib, words=_P + 2, image_floats=1)
    assert rc == _BAD and b"4-byte aligned" in msg
    rc, msg = _transfer_mask(lib, image_floats=n - 1)
    assert rc == _WS and b"image of %d floats is too small (%d)" % (n - 1, n) in msg


# ---------------------------------------------------------------- the masked selecting entries, in the rule order
def _need(lib, family, C_, A, nT, k, workgroups):
    n = C.c_size_t(0)
    rc = lib.impnn_grid_topk_workspace_bytes(family, C_, A, nT, k, workgroups, C.byref(n))
    return rc, n.value


def _head_where(lib, **kw):
    a = dict(kind=0, mc=_P, ma=_P, T=_P, w=_P, where=_P, k=5, largest=0, values=_P, cation=_P, anion=_P, ws=_P, ws_bytes=None,
             C=3, A=4, nT=2, D=32, F=32, Mx=20, workgroups=0)
    a.update(kw)
    if a["ws_bytes"] is None:
        rc, a["ws_bytes"] = _need(lib, 0, max(a["C"], 0), max(a["A"], 0), min(max(a["nT"], 0), 4), min(max(a["k"], 1), 1024),
                                  max(a["workgroups"], 0))
        if rc != 0:  # (a shape the query refuses too: the entry must refuse it before it looks at the size)
            a["ws_bytes"] = 1 << 40
    rc = lib.impnn_head_grid_topk_where(a["kind"], a["mc"], a["ma"], a["T"], a["w"], a["where"], a["k"], a["largest"],
                                        a["values"], a["cation"], a["anion"], a["ws"], a["ws_bytes"], a["C"], a["A"], a["nT"],
                                        a["D"], a["F"], a["Mx"], a["workgroups"], None)
    return rc, lib.impnn_last_error_string()


def _transfer_where(lib, **kw):
    a = dict(uc=_P, ua=_P, image=_P, image_floats=lib.impnn_transfer_grid_image_floats(), where=_P, k=5, largest=0, values=_P,
             cation=_P, anion=_P, ws=_P, ws_bytes=None, C=3, A=4, workgroups=0)
    a.update(kw)
    if a["ws_bytes"] is None:
        rc, a["ws_bytes"] = _need(lib, 1, max(a["C"], 0), max(a["A"], 0), 0, min(max(a["k"], 1), 1024), max(a["workgroups"], 0))
        if rc != 0:
            a["ws_bytes"] = 1 << 40
    rc = lib.impnn_transfer_head_grid_topk_where(a["uc"], a["ua"], a["image"], a["image_floats"], a["where"], a["k"],
                                                 a["largest"], a["values"], a["cation"], a["anion"], a["ws"], a["ws_bytes"],
                                                 a["C"], a["A"], a["workgroups"], None)
    return rc, lib.impnn_last_error_string()


_HW_NULLS = dict(mc=None, ma=None, T=None, w=None, where=None, values=None, cation=None, anion=None, ws=None)
_TW_NULLS = dict(uc=None, ua=None, image=None, where=None, values=None, cation=None, anion=None, ws=None)


def test_head_grid_topk_where_status_codes():
    lib = _lib.load()
    mp = dict(kind=1, nT=0, T=None)
    for kw, code, what in ((dict(C=-1), _BAD, b"bad shape"), (dict(A=-1), _BAD, b"bad shape"), (dict(nT=-1), _BAD, b"bad shape"),
                           (dict(D=0), _BAD, b"bad shape"), (dict(workgroups=-1), _BAD, b"bad shape"),
                           (dict(kind=2), _BAD, b"kind"), (dict(kind=1, nT=3), _BAD, b"nT must be 0"),
                           (dict(kind=0, nT=0), _BAD, b"nT >= 1"), (dict(k=0), _BAD, b"k=0"), (dict(k=1025), _UNS, b"k=1025"),
                           (dict(nT=5), _UNS, b"nT=5"), (dict(_2_32), _UNS, b"4294967296 pairs"),
                           (dict(D=129), _UNS, b"D=129"), (dict(mp, Mx=65), _UNS, b"Mx=65")):
        for extra in ({}, _HW_NULLS, dict(_HW_NULLS, C=0), dict(where=None), dict(ws_bytes=0)):
            args = dict(extra)
            args.update(kw)
            rc, msg = _head_where(lib, **args)
            assert rc == code and what in msg and b"impnn_head_grid_topk_where" in msg, (kw, extra, rc, msg)
    for kw in (dict(C=0), dict(A=0), dict(mp, C=0)):
        assert _head_where(lib, **dict(_HW_NULLS, ws_bytes=0, **kw))[0] == 0, kw
    for kw in [_HW_NULLS] + [{n: None} for n in _HW_NULLS]:      # a null mask is a null pointer
        rc, msg = _head_where(lib, ws_bytes=0, **kw)
        assert rc == _BAD and b"null pointer" in msg, (kw, msg)
    rc, msg = _head_where(lib, **dict(mp, where=None))
    assert rc == _BAD and b"null pointer" in msg
    rc, msg = _head_where(lib, **dict(mp, T=_P))
    assert rc == _BAD and b"takes no temperatures" in msg
    rc, msg = _head_where(lib, ws=_P + 4, ws_bytes=0)
    assert rc == _BAD and b"8-byte aligned" in msg
    rc, msg = _head_where(lib, where=_P + 2, ws_bytes=0)
    assert rc == _BAD and b"mask must be 4-byte aligned" in msg
    rc, need = _need(lib, 0, 3, 4, 2, 5, 0)      # the one query serves both forms
    assert rc == 0 and need > 0
    rc, msg = _head_where(lib, ws_bytes=need - 1)
    assert rc == _WS and b"workspace of %d bytes is too small (%d)" % (need - 1, need) in msg


def test_transfer_head_grid_topk_where_status_codes():
    lib = _lib.load()
    n = lib.impnn_transfer_grid_image_floats()
    for kw, code, what in ((dict(C=-1), _BAD, b"bad shape"), (dict(image_floats=-1), _BAD, b"bad shape"),
                           (dict(workgroups=-1), _BAD, b"bad shape"), (dict(k=0), _BAD, b"k=0"), (dict(k=1025), _UNS, b"k=1025"),
                           (dict(_2_32), _UNS, b"4294967296 pairs")):
        for extra in ({}, _TW_NULLS, dict(_TW_NULLS, C=0), dict(where=None), dict(ws_bytes=0)):
            args = dict(extra)
            args.update(kw)
            rc, msg = _transfer_where(lib, **args)
            assert rc == code and what in msg and b"impnn_transfer_head_grid_topk_where" in msg, (kw, extra, rc, msg)
    for kw in (dict(C=0), dict(A=0)):
        assert _transfer_where(lib, ws_bytes=0, image_floats=0, **dict(_TW_NULLS, **kw))[0] == 0, kw
    for kw in [_TW_NULLS] + [{x: None} for x in _TW_NULLS]:
        rc, msg = _transfer_where(lib, ws_bytes=0, image_floats=1, **kw)
        assert rc == _BAD and b"null pointer" in msg, (kw, msg)
    rc, msg = _transfer_where(lib, where=_P + 1, ws_bytes=0, image_floats=1)
    assert rc == _BAD and b"mask must be 4-byte aligned" in msg
    rc, msg = _transfer_where(lib, ua=_P + 4, ws_bytes=0)
    assert rc == _BAD and b"16-byte aligned" in msg
    rc, msg = _transfer_where(lib, image_floats=n - 1, ws_bytes=0)
    assert rc == _WS and b"image of %d floats is too small (%d)" % (n - 1, n) in msg
    rc, need = _need(lib, 1, 3, 4, 0, 5, 0)
    rc, msg = _transfer_where(lib, ws_bytes=need - 1)
    assert rc == _WS and b"workspace of %d bytes is too small (%d)" % (need - 1, need) in msg


# ---------------------------------------------------------------- data.PairMask against numpy
@pytest.mark.parametrize("A", [1, 31, 32, 33, 130])
def test_pair_mask_against_numpy(A):
    rng = np.random.default_rng(A)
    Cn, W = 7, (A + 31) // 32
    a, b = rng.random((Cn, A)) < 0.5, rng.random((Cn, A)) < 0.3
    ma, mb = data.PairMask.from_bool(a), data.PairMask.from_bool(b)
    assert ma.shape == (Cn, A) and ma.words.dtype == torch.int32 and tuple(ma.words.shape) == (Cn, W)
    assert np.array_equal(ma.to_bool(), a) and ma.to_bool().dtype == np.bool_
    # the format: pair (i, j) is bit j & 31 of words[i][j >> 5]
    u = ma.words.numpy().view(np.uint32)
    for i, j in ((0, 0), (Cn - 1, A - 1), (3, A // 2)):
        assert bool((u[i, j >> 5] >> (j & 31)) & 1) == bool(a[i, j])
    pad = np.uint32(0) if A % 32 == 0 else ~np.uint32((1 << (A % 32)) - 1)
    for m, want in ((ma, a), (~ma, ~a), (~~ma, a), (ma & mb, a & b), (ma | mb, a | b), (~(ma | mb), ~(a | b)),
                    (~data.PairMask.from_bool(np.zeros_like(a)), np.ones_like(a))):
        assert np.array_equal(m.to_bool(), want) and m.count() == int(want.sum())
        assert not (m.words.numpy().view(np.uint32)[:, -1] & pad).any(), "a pad bit is set"
    assert np.array_equal(ma.rows(2, 5).to_bool(), a[2:5]) and ma.rows(2, 5).shape == (3, A)
    assert ma.rows(4, 4).count() == 0 and ma.rows(0, Cn).count() == int(a.sum())
    # a viscosity mask: a plane per temperature
    a3 = rng.random((Cn, A, 3)) < 0.5
    m3 = data.PairMask.from_bool(a3)
    assert m3.shape == (Cn, A, 3) and tuple(m3.words.shape) == (3, Cn, W) and np.array_equal(m3.to_bool(), a3)
    assert m3.count().tolist() == a3.sum(axis=(0, 1)).tolist() and (~m3).count().tolist() == (~a3).sum(axis=(0, 1)).tolist()
    for t in range(3):
        assert m3.temperature(t).shape == (Cn, A) and np.array_equal(m3.temperature(t).to_bool(), a3[:, :, t])
    assert np.array_equal(m3.rows(1, 6).to_bool(), a3[1:6])
    assert np.array_equal((m3.temperature(0) & ~m3.temperature(2)).to_bool(), a3[:, :, 0] & ~a3[:, :, 2])


def test_pair_mask_errors():
    a = np.zeros((3, 40), bool)
    m = data.PairMask.from_bool(a)
    for other in (np.zeros((3, 41), bool), np.zeros((4, 40), bool), np.zeros((3, 40, 1), bool)):
        with pytest.raises(ValueError, match="shapes"):
            m & data.PairMask.from_bool(other)
        with pytest.raises(ValueError, match="shapes"):
            m | data.PairMask.from_bool(other)
    with pytest.raises(ValueError, match="bool array"):
        data.PairMask.from_bool(np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match="words must be"):
        data.PairMask(torch.zeros(3, 1, dtype=torch.int32), (3, 40))
    with pytest.raises(ValueError, match="no temperature axis"):
        m.temperature(0)
    with pytest.raises(ValueError, match="rows"):
        m.rows(2, 4)
    with pytest.raises(TypeError):
        m & a


# ---------------------------------------------------------------- the masked reference order
def f32(*v):
    return np.array(v, np.float32)


def test_grid_top_k_where_on_hand_written_grids():
    g = f32(5, 0, 2, 2, 2, np.nan, 7, 1).reshape(2, 4)
    w = np.array([1, 0, 1, 1, 1, 1, 0, 1], bool).reshape(2, 4)       # the minimum 0 at (0, 1) is masked out
    for where in (w, data.PairMask.from_bool(w)):
        got = data.grid_top_k(g, 3, where=where)
        assert got.values.tolist() == [1, 2, 2] and got.cation.tolist() == [1, 0, 0] and got.anion.tolist() == [3, 2, 3]
        assert got.values.dtype == np.float32 and got.cation.dtype == np.int64
        # ties by index across the masked-out pair; the masked-in NaN last, in both directions; k > count: count entries
        got = data.grid_top_k(g, 100, where=where)
        assert got.values[:-1].tolist() == [1, 2, 2, 2, 5] and (got.cation * 4 + got.anion).tolist() == [7, 2, 3, 4, 0, 5]
        assert got.values[-1:].view(np.uint32).tolist() == [0x7FC00000]
        got = data.grid_top_k(g, 100, largest=True, where=where)
        assert got.values[:-1].tolist() == [5, 2, 2, 2, 1] and (got.cation * 4 + got.anion).tolist() == [0, 2, 3, 4, 7, 5]
        assert np.isnan(got.values[-1])
    w2 = w.copy()
    w2[0, 3] = False                                                  # a tie's middle member masked out
    assert (lambda t: (t.cation * 4 + t.anion).tolist())(data.grid_top_k(g, 3, where=w2)) == [7, 2, 4]
    none = data.grid_top_k(g, 3, where=np.zeros((2, 4), bool))
    assert none.values.shape == none.cation.shape == none.anion.shape == (0,)
    g3 = np.stack([g, -g], axis=-1)                                   # the one mask for every temperature row
    got = data.grid_top_k(g3, 2, where=w)
    assert got.values.tolist() == [[1, 2], [-5, -2]] and (got.cation * 4 + got.anion).tolist() == [[7, 2], [0, 2]]
    assert data.grid_top_k(g3, 100, where=w).values.shape == (2, 6)
    assert data.grid_top_k(g3, 5, where=np.zeros((2, 4), bool)).values.shape == (2, 0)
    full = data.grid_top_k(g, 5, where=np.ones((2, 4), bool))
    plain = data.grid_top_k(g, 5)
    assert np.array_equal(full.values.view(np.uint32), plain.values.view(np.uint32)) and np.array_equal(full.anion, plain.anion)
    with pytest.raises(ValueError, match="where must be"):
        data.grid_top_k(g, 3, where=np.ones((2, 5), bool))
    with pytest.raises(ValueError, match="temperature"):
        data.grid_top_k(g3, 3, where=data.PairMask.from_bool(np.ones((2, 4, 2), bool)))


# ---------------------------------------------------------------- Python-side errors
def _species(n, seed, N=40, E=80):
    b = synthetic.make_batch(n, max_atoms=N, max_edges=E, seed=seed, with_temperature=False)
    return {k: b[f"cat_{k}"] for k in MM.ION_KEYS}, {k: b[f"an_{k}"] for k in MM.ION_KEYS}


def test_screen_mask_and_where_argument_errors():
    cat, _ = _species(2, 1)
    _, an = _species(3, 2)
    v = MM.build_model(synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, num_steps=1, device=CPU)
    with pytest.raises(ValueError, match=r"temperature\(t\)"):
        v.screen_top_k(cat, an, temperatures=[300.0], where=data.PairMask.from_bool(np.ones((2, 3, 1), bool)))
    for shape in ((3, 2), (2, 4), (1, 3)):
        with pytest.raises(ValueError, match="where has shape"):
            v.screen_top_k(cat, an, temperatures=[300.0], where=data.PairMask.from_bool(np.ones(shape, bool)))
    with pytest.raises(TypeError, match="PairMask"):
        v.screen_top_k(cat, an, temperatures=[300.0], where=np.ones((2, 3), bool))
    with pytest.raises(ValueError, match="needs a bound"):
        v.screen_mask(cat, an, temperatures=[300.0])
    with pytest.raises(ValueError, match="NaN"):
        v.screen_mask(cat, an, temperatures=[300.0], at_most=NAN)
    with pytest.raises(KeyError, match="temperature"):
        v.screen_mask(cat, an, at_most=1.0)
    with pytest.raises(ValueError, match="both"):
        v.screen_mask(cat, None, temperatures=[300.0], at_least=0.0)
    with pytest.raises(ValueError, match="max_pairs_per_launch"):
        v.screen_mask(cat, an, temperatures=[300.0], at_least=0.0, max_pairs_per_launch=0)
    with pytest.raises(ValueError, match="at least one"):
        v.screen_mask(cat, an, temperatures=[], at_least=0.0)
    # a well-formed call gets as far as the GPU: there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v.screen_mask(cat, an, temperatures=[300.0], at_most=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v.screen_top_k(cat, an, temperatures=[300.0], k=3, where=data.PairMask.from_bool(np.ones((2, 3), bool)))
