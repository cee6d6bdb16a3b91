"""CPU: the host side of the Pareto front - the entries (declared, exported, bound), the bucket bits and the workspace
query, the status and text of every argument rule of the launching entries (every failing call returns before a launch;
the stand-in pointers are never dereferenced), data.pareto_front against a brute-force restatement of the definition
(ties, NaN in either plane, signed zeros, infinities, masks, four directions) and its properties, the argument rules of
screen_pareto, and the size of the reference front on the oracle's viscosity x melting-point grids."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import ionic_mpnn_amd as impnn
from ionic_mpnn_amd import _lib, data, model as MM, ops, pareto, synthetic

import ensemble_cases as EC

_BAD, _UNS, _WS = -1, -2, -4
_P = 0x100000   # a stand-in pointer (16-byte aligned)
ENTRIES = ("impnn_pareto_bucket_bits", "impnn_pareto_workspace_bytes", "impnn_pareto_begin", "impnn_pareto_range",
           "impnn_pareto_minima", "impnn_pareto_staircase", "impnn_pareto_collect")
DIRECTIONS = list(itertools.product((False, True), repeat=2))
CPU = torch.device("cpu")


def test_the_entries_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "impnn.h").read_text(), flags=re.S)
    raw = C.CDLL(str(_lib.lib_path()))
    for n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in impnn.h"
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} is not bound"
    assert _lib.load().impnn_abi_version() == 3  # additions only
    assert "grid_pareto.hip" in __import__("ionic_mpnn_amd.build", fromlist=["SOURCES"]).SOURCES


def _need(lib):
    n = C.c_size_t(0)
    assert lib.impnn_pareto_workspace_bytes(C.byref(n)) == 0
    return n.value


def test_bucket_bits_and_the_workspace_query():
    lib = _lib.load()
    bits = lib.impnn_pareto_bucket_bits()
    assert bits == 14
    # the 32-byte header, the bucket table and the staircase
    assert _need(lib) == 32 + 2 * 4 * (1 << bits)
    assert lib.impnn_pareto_workspace_bytes(None) == _BAD
    assert "impnn_pareto_workspace_bytes: null pointer" in lib.impnn_last_error_string().decode()


# ---------------------------------------------------------------- the argument rules of the launching entries
def _block(name):
    def call(lib, **kw):
        a = dict(f1=_P, f2=_P, where=None, l1=0, l2=1, row0=0, restart=0, v=_P, ci=_P, ai=_P, capacity=64, ws=_P,
                 ws_bytes=1 << 40, rows=3, A=4)
        a.update(kw)
        lead = (a["f1"], a["f2"], a["where"], a["l1"], a["l2"])
        tail = (a["ws"], a["ws_bytes"], a["rows"], a["A"], None)
        if name == "collect":
            rc = lib.impnn_pareto_collect(*lead, a["row0"], a["restart"], a["v"], a["ci"], a["ai"], a["capacity"], *tail)
        else:
            rc = getattr(lib, "impnn_pareto_" + name)(*lead, *tail)
        return rc, lib.impnn_last_error_string().decode()
    call.entry = "impnn_pareto_" + name
    return call


def _whole(name):
    def call(lib, **kw):
        a = dict(ws=_P, ws_bytes=1 << 40)
        a.update(kw)
        return getattr(lib, "impnn_pareto_" + name)(a["ws"], a["ws_bytes"], None), lib.impnn_last_error_string().decode()
    call.entry = "impnn_pareto_" + name
    return call


BLOCK_TABLE = ((dict(rows=-1), _BAD, "bad shape"), (dict(A=-1), _BAD, "bad shape"),
               (dict(l1=2), _BAD, "largest must be 0 or 1"), (dict(l2=-1), _BAD, "largest must be 0 or 1"),
               (dict(f1=None), _BAD, "null pointer"), (dict(f2=None), _BAD, "null pointer"), (dict(ws=None), _BAD, "null pointer"),
               (dict(f1=_P + 2), _BAD, "4-byte aligned"), (dict(f2=_P + 1), _BAD, "4-byte aligned"),
               (dict(where=_P + 2), _BAD, "4-byte aligned"), (dict(ws=_P + 4), _BAD, "8-byte aligned"),
               (dict(ws_bytes=8), _WS, "workspace of 8 bytes is too small"),
               (dict(rows=1 << 16, A=1 << 15), _UNS, "2147483648 pairs in one row-block"))
COLLECT_TABLE = ((dict(row0=-1), _BAD, "bad shape"), (dict(capacity=-1), _BAD, "bad shape"),
                 (dict(v=None), _BAD, "null pointer"), (dict(ci=None), _BAD, "null pointer"), (dict(ai=None), _BAD, "null pointer"),
                 (dict(v=_P + 2), _BAD, "4-byte aligned"), (dict(ai=_P + 3), _BAD, "4-byte aligned"),
                 (dict(row0=(1 << 31) - 3), _UNS, "a cation index has 31 bits"))
WHOLE_TABLE = ((dict(ws=None), _BAD, "null pointer"), (dict(ws=_P + 4), _BAD, "8-byte aligned"),
               (dict(ws_bytes=8), _WS, "workspace of 8 bytes is too small"))


def test_entries_refuse_bad_requests_before_a_launch():
    lib = _lib.load()
    need = _need(lib)
    for call in (_block("range"), _block("minima"), _block("collect")):
        for kw, code, text in BLOCK_TABLE + (COLLECT_TABLE if call.entry.endswith("collect") else ()):
            rc, msg = call(lib, **kw)
            assert rc == code and text in msg and msg.startswith(call.entry + ": "), (call.entry, kw, rc, msg)
        # zero work: nothing touched, whatever the pointers
        assert call(lib, rows=0, f1=None, ws=None, ws_bytes=0)[0] == 0 and call(lib, A=0, f2=None, v=None)[0] == 0
        # the order of the rules
        assert "bad shape" in call(lib, rows=-1, l1=2)[1] and "largest" in call(lib, l1=2, f1=None)[1]
        assert "null pointer" in call(lib, f1=None, ws=_P + 4)[1] and "aligned" in call(lib, f2=_P + 2, ws_bytes=8)[1]
        assert "too small" in call(lib, ws_bytes=need - 1, rows=1 << 16, A=1 << 15)[1]
        assert "pairs" in call(lib, ws_bytes=need, rows=1 << 16, A=1 << 15)[1], "the exact size passes the size rule"
    collect = _block("collect")
    assert collect(lib, capacity=0, v=None, ci=None, ai=None, rows=1 << 16, A=1 << 15)[0] == _UNS, "no outputs needed at capacity 0"
    for call in (_whole("begin"), _whole("staircase")):
        for kw, code, text in WHOLE_TABLE:
            rc, msg = call(lib, **kw)
            assert rc == code and text in msg and msg.startswith(call.entry + ": "), (call.entry, kw, rc, msg)
        assert call(lib, ws_bytes=need - 1)[0] == _WS


# ---------------------------------------------------------------- the reference against the definition
def keys(a, b, largest):
    return (data.select_keys(a, largest[0]).astype(np.int64).reshape(-1),
            data.select_keys(b, largest[1]).astype(np.int64).reshape(-1))


def dominates(k1, k2, q, p):
    return k1[q] <= k1[p] and k2[q] <= k2[p] and (k1[q] < k1[p] or k2[q] < k2[p] or q < p)


def brute_front(a, b, largest, where):
    """The definition, restated in O(n^2) -> (flat indices of the front in listing order, competing)."""
    k1, k2 = keys(a, b, largest)
    live = ~(np.isnan(a) | np.isnan(b)).reshape(-1)
    if where is not None:
        live &= np.asarray(where).reshape(-1)
    idx = [int(i) for i in np.flatnonzero(live)]
    front = [p for p in idx if not any(dominates(k1, k2, q, p) for q in idx)]
    return np.array(sorted(front, key=lambda p: (k1[p], k2[p], p)), np.int64), len(idx)


def tricky(shape, seed):
    """Two tie-heavy planes with NaN in either, signed zeros and infinities."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-2, 3, shape).astype(np.float32)
    b = rng.integers(-2, 3, shape).astype(np.float32)
    a[rng.random(shape) < 0.08] = np.nan
    b[rng.random(shape) < 0.08] = np.nan
    a[(a == 0) & (rng.random(shape) < 0.5)] = -0.0
    b[(b == 0) & (rng.random(shape) < 0.5)] = -0.0
    for plane in (a, b):
        plane[rng.random(shape) < 0.04] = np.inf
        plane[rng.random(shape) < 0.04] = -np.inf
    return a, b


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("largest", DIRECTIONS, ids=lambda d: "%d%d" % d)
def test_pareto_front_is_the_definition(largest):
    for seed in range(40):
        rng = np.random.default_rng(100 + seed)
        shape = (int(rng.integers(1, 7)), int(rng.integers(1, 9)))
        a, b = tricky(shape, seed) if seed % 4 else (rng.standard_normal(shape).astype(np.float32),
                                                     rng.standard_normal(shape).astype(np.float32))
        for where in (None, rng.random(shape) < 0.6, np.zeros(shape, np.bool_)):
            want, competing = brute_front(a, b, largest, where)
            for wh in (where, data.PairMask.from_bool(where)) if where is not None else (None,):
                got = data.pareto_front(a, b, largest, wh)
                flat = got.cation * shape[1] + got.anion
                assert got.competing == competing and np.array_equal(flat, want), (seed, largest)
                assert got.values.shape == (len(want), 2) and got.values.dtype == np.float32
                assert np.array_equal(bits(got.values[:, 0]), bits(a.reshape(-1)[flat]))
                assert np.array_equal(bits(got.values[:, 1]), bits(b.reshape(-1)[flat]))
                assert got.cation.dtype == got.anion.dtype == np.int64 and isinstance(got.competing, int)


@pytest.mark.parametrize("largest", DIRECTIONS, ids=lambda d: "%d%d" % d)
def test_the_front_has_the_properties_of_a_front(largest):
    a, b = tricky((9, 21), 7)
    where = np.random.default_rng(3).random(a.shape) < 0.7
    got = data.pareto_front(a, b, largest, where)
    k1, k2 = keys(a, b, largest)
    flat = got.cation * a.shape[1] + got.anion
    assert len(flat) >= 2
    # listing order: ascending (k1, k2, flat); k1 strictly improves while k2 strictly worsens; distinct (k1, k2)
    assert (np.diff(k1[flat]) > 0).all() and (np.diff(k2[flat]) < 0).all()
    # members are mutually non-dominated; every competing non-member is dominated by a member
    assert not any(dominates(k1, k2, q, p) for q in flat for p in flat if q != p)
    live = np.flatnonzero(where.reshape(-1) & ~(np.isnan(a) | np.isnan(b)).reshape(-1))
    assert got.competing == len(live)
    for p in set(live.tolist()) - set(flat.tolist()):
        assert any(dominates(k1, k2, q, p) for q in flat), p
    # -0.0 < +0.0 and infinities are ordinary values
    z = data.pareto_front(np.array([[0.0, -0.0]], np.float32), np.array([[1.0, 1.0]], np.float32))
    assert z.anion.tolist() == [1]
    z = data.pareto_front(np.array([[-np.inf, 1.0, np.inf]], np.float32), np.array([[np.inf, 0.0, -np.inf]], np.float32))
    assert z.anion.tolist() == [0, 1, 2]
    # of equal (v1, v2) only the lowest flat index
    z = data.pareto_front(np.ones((3, 4), np.float32), np.ones((3, 4), np.float32))
    assert (z.cation.tolist(), z.anion.tolist(), z.competing) == ([0], [0], 12)


def test_pareto_front_argument_errors_and_empty_grids():
    g = np.zeros((2, 3), np.float32)
    with pytest.raises(ValueError, match="one shape"):
        data.pareto_front(g, np.zeros((3, 2), np.float32))
    with pytest.raises(ValueError, match="one shape"):
        data.pareto_front(np.zeros(4, np.float32), np.zeros(4, np.float32))
    with pytest.raises(ValueError, match="one flag per objective"):
        data.pareto_front(g, g, largest=(False,))
    with pytest.raises(ValueError, match="where must be"):
        data.pareto_front(g, g, where=np.zeros((2, 2), np.bool_))
    for shape in ((0, 3), (3, 0)):
        e = data.pareto_front(np.zeros(shape, np.float32), np.zeros(shape, np.float32))
        assert e.values.shape == (0, 2) and len(e.cation) == len(e.anion) == 0 and e.competing == 0
    e = data.pareto_front(g, g, where=np.zeros((2, 3), np.bool_))
    assert e.values.shape == (0, 2) and e.competing == 0
    e = data.pareto_front(np.full((2, 3), np.nan, np.float32), g)
    assert e.values.shape == (0, 2) and e.competing == 0


# ---------------------------------------------------------------- Python-side errors
def _species(n, seed, N=40, E=80):
    b = synthetic.make_batch(n, max_atoms=N, max_edges=E, seed=seed, with_temperature=False)
    return {k: b[f"cat_{k}"] for k in MM.ION_KEYS}, {k: b[f"an_{k}"] for k in MM.ION_KEYS}


def test_screen_pareto_argument_errors():
    assert impnn.screen_pareto is pareto.screen_pareto and impnn.Objective is pareto.Objective
    cat, an = _species(2, 1)
    v = MM.build_model(synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, num_steps=1, device=CPU)
    m = MM.build_melting_point_model(synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, num_steps=1, device=CPU)
    ens = impnn.ModelEnsemble([m])
    O = pareto.Objective
    with pytest.raises(TypeError, match="MPNNModel or a ModelEnsemble"):
        O("viscosity")
    for T in (None, [298.15, 310.0], []):
        with pytest.raises(ValueError, match="exactly one temperature"):
            O(v, T)
    with pytest.raises(ValueError, match="takes no temperature"):
        O(m, 298.15)
    with pytest.raises(ValueError, match="takes no temperature"):
        O(ens, [298.15])
    with pytest.raises(ValueError, match="ModelEnsemble objective only"):
        O(m, kappa=1.0)
    with pytest.raises(ValueError, match="kappa must be finite"):
        O(ens, kappa=float("inf"))
    assert O(ens).kappa == 0.0 and O(ens, kappa=1.5, largest=True).largest and O(v, [298.15]).temperature == np.float32(298.15)
    two = [O(v, 298.15), O(m)]
    for objs in ([], two[:1], two + two[:1]):
        with pytest.raises(ValueError, match="fronts of more objectives are not built"):
            pareto.screen_pareto(objs, cat, an)
    with pytest.raises(TypeError, match="Objective instances"):
        pareto.screen_pareto([two[0], m], cat, an)
    with pytest.raises(ValueError, match="both"):
        pareto.screen_pareto(two, cat, None)
    with pytest.raises(ValueError, match="max_pairs_per_launch"):
        pareto.screen_pareto(two, cat, an, max_pairs_per_launch=0)
    with pytest.raises(ValueError, match="capacity"):
        pareto.screen_pareto(two, cat, an, capacity=0)
    with pytest.raises(TypeError, match="data.PairMask"):
        pareto.screen_pareto(two, cat, an, where=np.ones((2, 2), np.bool_))
    with pytest.raises(ValueError, match="where has shape"):
        pareto.screen_pareto(two, cat, an, where=data.PairMask.from_bool(np.ones((2, 3), np.bool_)))
    with pytest.raises(ValueError, match="2-D mask"):
        pareto.screen_pareto(two, cat, an, where=data.PairMask.from_bool(np.ones((2, 2, 1), np.bool_)))
    # only then the device: nothing here computes on the CPU
    for objs in (two, [O(ens, kappa=1.0), O(ens, kappa=-1.0)]):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pareto.screen_pareto(objs, cat, an)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pareto_front(torch.zeros(2, 3), torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ParetoFilter(3, (False, False), 16, CPU)


# ---------------------------------------------------------------- the reference front on the oracle's grids
@pytest.mark.parametrize("shape", [(7, 63), (17, 130)], ids=lambda s: "%dx%d" % s)
def test_the_reference_front_of_viscosity_and_melting_point_is_neither_trivial_nor_everything(shape):
    Cn, An = shape
    cat, an = EC.species(Cn, An)
    visc = EC.cpu_member_grid("viscosity", EC.member_weights("viscosity", 0), cat, an, np.array([298.15], np.float32))[..., 0]
    mp = EC.cpu_member_grid("melting_point", EC.member_weights("melting_point", 0), cat, an, None)
    for largest in DIRECTIONS:
        front = data.pareto_front(visc, mp, largest)
        n = len(front.cation)
        print(f"{shape} largest={largest}: front of {n} of {front.competing}")
        assert front.competing == Cn * An and 5 <= n <= Cn * An / 2, (shape, largest, n)
