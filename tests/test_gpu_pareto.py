"""The Pareto front on the GPU: the impnn_pareto_* stages against data.pareto_front of the same planes, and
screen_pareto against data.pareto_front(predict_grid(...), predict_grid(...)).

Everything here is exact: the filter compares integer keys and copies its inputs' bits, and a screen's tile has the bits
predict_grid gives, so values are compared by their uint32 view and indices for equality.  No tolerance appears."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import ionic_mpnn_amd as impnn
from ionic_mpnn_amd import _lib, data, ops
from ionic_mpnn_amd.pareto import Objective, screen_pareto

import ensemble_cases as EC
from test_gpu_grid import make_model
from test_gpu_screen import FILL, Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIRECTIONS = list(itertools.product((False, True), repeat=2))
SHAPES = [(1, 1), (7, 63), (17, 130), (65, 130)]
T0, T1 = 298.15, 353.15


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(got, want, what):
    assert got.competing == want.competing, (what, got.competing, want.competing)
    assert got.values.shape == want.values.shape, (what, got.values.shape, want.values.shape)
    assert np.array_equal(bits(got.values), bits(want.values)), f"{what}: values"
    assert np.array_equal(got.cation, want.cation) and np.array_equal(got.anion, want.anion), f"{what}: indices"
    assert got.cation.dtype == got.anion.dtype == np.int64 and got.values.dtype == np.float32


# ---------------------------------------------------------------- planes and masks
def tie_planes(shape, seed):
    """Tie-heavy integer planes with 5 % NaN in either and signed zeros."""
    rng = np.random.default_rng(seed)
    planes = []
    for _ in range(2):
        p = rng.integers(-3, 4, shape).astype(np.float32)
        p[(p == 0) & (rng.random(shape) < 0.5)] = -0.0
        p[rng.random(shape) < 0.05] = np.nan
        planes.append(p)
    return planes


def smooth_planes(shape, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape).astype(np.float32)
    return a, (0.6 * a + 0.8 * rng.standard_normal(shape)).astype(np.float32)


def masks(shape, seed):
    """None, all-zero, a single bit, a random 30 %."""
    one = np.zeros(shape, np.bool_)
    one[shape[0] // 2, shape[1] - 1] = True
    return None, np.zeros(shape, np.bool_), one, np.random.default_rng(seed).random(shape) < 0.3


# ---------------------------------------------------------------- guarded calls of the entries
def run_filter(f1, f2, largest, where=None, block_rows=None, capacity=None, spare=0):
    """The stages over row-blocks of ``block_rows`` rows, workspace and candidate arrays guarded at exactly the queried
    sizes (``spare`` more entries than the capacity passed, to see them untouched) -> (the candidates written as sorted
    rows (flat, v1 bits, v2 bits), count, competing, header keys)."""
    lib = _lib.load()
    Cn, An = f1.shape
    capacity = Cn * An if capacity is None else capacity
    need = C.c_size_t(0)
    _lib.check(lib.impnn_pareto_workspace_bytes(C.byref(need)))
    ws = Guarded(need.value)
    v, ci, ai = Guarded((capacity + spare) * 8), Guarded((capacity + spare) * 4), Guarded((capacity + spare) * 4)
    d1, d2 = dev(f1), dev(f2)
    words = data.PairMask.from_bool(where, device=DEV).words if where is not None else None
    step = Cn if block_rows is None else block_rows
    blocks = [(lo, min(Cn, lo + step)) for lo in range(0, Cn, step)]
    l1, l2 = int(largest[0]), int(largest[1])
    s = _lib.stream_ptr()

    def lead(lo, hi):
        return (_lib.ptr(d1[lo:hi]), _lib.ptr(d2[lo:hi]), _lib.ptr(words[lo:hi]) if words is not None else None, l1, l2)

    _lib.check(lib.impnn_pareto_begin(ws.ptr, need.value, s))
    for lo, hi in blocks:
        _lib.check(lib.impnn_pareto_range(*lead(lo, hi), ws.ptr, need.value, hi - lo, An, s))
    for lo, hi in reversed(blocks):   # any order of the blocks
        _lib.check(lib.impnn_pareto_minima(*lead(lo, hi), ws.ptr, need.value, hi - lo, An, s))
    _lib.check(lib.impnn_pareto_staircase(ws.ptr, need.value, s))
    for lo, hi in blocks:
        _lib.check(lib.impnn_pareto_collect(*lead(lo, hi), lo, 0, v.ptr, ci.ptr, ai.ptr, capacity, ws.ptr, need.value,
                                            hi - lo, An, s))
    torch.cuda.synchronize()
    head = ws.body(np.uint64, "the workspace")[:4]
    kmin, kmax = (int(x) for x in head[:1].view(np.uint32))
    competing, count = int(head[1]), int(head[2])
    assert 0 <= count <= Cn * An and 0 <= competing <= Cn * An and count <= competing
    n = min(count, capacity)
    vals = v.body(np.uint32, "values").reshape(-1, 2)
    cat, an = ci.body(np.int32, "cation"), ai.body(np.int32, "anion")
    filled = np.uint32(FILL * 0x01010101)
    assert (vals[n:] == filled).all() and (cat[n:].view(np.uint32) == filled).all() and (an[n:].view(np.uint32) == filled).all(), \
        "an entry past the count or the capacity was written"
    assert (cat[:n] >= 0).all() and (cat[:n] < Cn).all() and (an[:n] >= 0).all() and (an[:n] < An).all()
    flat = cat[:n].astype(np.int64) * An + an[:n]
    rows = np.stack([flat, vals[:n, 0].astype(np.int64), vals[:n, 1].astype(np.int64)], axis=1)
    return rows[np.argsort(flat, kind="stable")], count, competing, (kmin, kmax)


def front_of(rows, largest, A, competing):
    """The exact front of the candidate rows of ``run_filter``, by data.pareto_front's rule."""
    v = rows[:, 1:].astype(np.uint32).view(np.float32).reshape(-1, 2)
    keep = data.pareto_front_of(data.select_keys(v[:, 0], largest[0]), data.select_keys(v[:, 1], largest[1]), rows[:, 0])
    return data.ParetoFront(v[keep], rows[keep, 0] // A, rows[keep, 0] % A, competing)


def check_sound(rows, f1, f2, largest, where, want, what):
    """The candidates are competing pairs with their planes' bits, no pair twice, and hold the reference front."""
    A = f1.shape[1]
    flat = rows[:, 0]
    assert len(np.unique(flat)) == len(flat), f"{what}: a pair twice"
    live = ~(np.isnan(f1) | np.isnan(f2)).reshape(-1)
    if where is not None:
        live &= where.reshape(-1)
    assert live[flat].all(), f"{what}: a candidate that does not compete"
    assert np.array_equal(rows[:, 1], bits(f1).reshape(-1)[flat]) and np.array_equal(rows[:, 2], bits(f2).reshape(-1)[flat]), what
    assert np.isin(want.cation * A + want.anion, flat).all(), f"{what}: a member of the front was dropped"


# ---------------------------------------------------------------- 1. the stages against the reference
@pytest.mark.parametrize("planes", [tie_planes, smooth_planes], ids=["ties", "smooth"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_filter_and_the_wrapper_give_the_reference_front(shape, planes):
    f1, f2 = planes(shape, 3 + shape[1])
    d1, d2 = dev(f1), dev(f2)
    for largest in DIRECTIONS:
        for where in masks(shape, 11):
            what = f"{planes.__name__} {shape} {largest} where={None if where is None else int(where.sum())}"
            want = data.pareto_front(f1, f2, largest, where)
            rows, count, competing, (kmin, kmax) = run_filter(f1, f2, largest, where)
            assert competing == want.competing and count == len(rows), what
            if competing == 0:
                assert count == 0 and (kmin, kmax) == (0xFFFFFFFF, 0), what
            else:
                live = np.ones(shape, np.bool_) if where is None else where
                k1 = data.select_keys(f1, largest[0])[live & ~(np.isnan(f1) | np.isnan(f2))]
                assert (kmin, kmax) == (int(k1.min()), int(k1.max())), what
            check_sound(rows, f1, f2, largest, where, want, what)
            same(front_of(rows, largest, shape[1], competing), want, what)
            words = data.PairMask.from_bool(where, device=DEV).words if where is not None else None
            same(ops.pareto_front(d1, d2, largest, words), want, what + " (ops.pareto_front)")


# ---------------------------------------------------------------- 2. row-blocks
@pytest.mark.parametrize("planes", [tie_planes, smooth_planes], ids=["ties", "smooth"])
def test_row_blocks_do_not_change_the_result(planes):
    shape = (65, 130)
    f1, f2 = planes(shape, 21)
    where = masks(shape, 5)[3]
    for largest in ((False, False), (True, False)):
        for wh in (None, where):
            whole = run_filter(f1, f2, largest, wh)
            for block_rows in (1, 16):
                part = run_filter(f1, f2, largest, wh, block_rows=block_rows)
                assert np.array_equal(part[0], whole[0]) and part[1:] == whole[1:], (planes.__name__, largest, block_rows)
    # the wrapper's filter, fed in blocks through ops.pareto_run
    d1, d2 = dev(f1), dev(f2)
    words = data.PairMask.from_bool(where, device=DEV).words
    want = data.pareto_front(f1, f2, (False, True), where)
    for step in (1, 16, 65):
        filt = ops.ParetoFilter(shape[1], (False, True), 32, DEV)
        blocks = lambda: [(d1[lo:lo + step], d2[lo:lo + step], words[lo:lo + step], lo) for lo in range(0, shape[0], step)]
        same(ops.pareto_run(filt, blocks), want, f"pareto_run in blocks of {step}")


# ---------------------------------------------------------------- 3. capacity
def test_the_count_runs_past_the_capacity_and_the_wrapper_regrows():
    shape = (17, 130)
    rng = np.random.default_rng(9)
    f1 = rng.permutation(shape[0] * shape[1]).astype(np.float32).reshape(shape)
    f2 = -f1                                   # anti-correlated: every pair is on the front
    want = data.pareto_front(f1, f2)
    assert len(want.cation) == want.competing == shape[0] * shape[1]
    rows, count, competing, _ = run_filter(f1, f2, (False, False), capacity=64, spare=64, block_rows=5)
    assert count == competing == shape[0] * shape[1] and len(rows) == 64   # (run_filter saw entries 64 .. 127 untouched)
    check_sound(rows, f1, f2, (False, False), None, data.ParetoFront(*[x[:0] for x in want[:3]], 0), "capacity 64")
    d1, d2 = dev(f1), dev(f2)
    same(ops.pareto_front(d1, d2, capacity=64), want, "regrown from capacity 64")
    same(ops.pareto_front(d1, d2, (True, True), capacity=1), data.pareto_front(f1, f2, (True, True)), "regrown from capacity 1")
    # the filter object: a count above the capacity, then collect alone at the size it reports
    filt = ops.ParetoFilter(shape[1], (False, False), 64, DEV)
    filt.begin(), filt.range(d1, d2), filt.minima(d1, d2), filt.staircase(), filt.collect(d1, d2)
    assert filt.candidates()[3] == shape[0] * shape[1] and len(filt.candidates()[1]) == 64
    filt.grow(filt.candidates()[3])
    filt.collect(d1[:9], d2[:9]), filt.collect(d1[9:], d2[9:], None, 9)
    values, cation, anion, count, competing = filt.candidates()
    assert count == competing == len(cation) == shape[0] * shape[1]
    assert np.array_equal(np.sort(cation * shape[1] + anion), np.arange(count))


# ---------------------------------------------------------------- 4. soundness and determinism of the set
def test_the_candidate_set_is_sound_small_and_the_same_every_run():
    shape = (65, 130)
    for planes in (tie_planes, smooth_planes):
        f1, f2 = planes(shape, 33)
        for largest in DIRECTIONS:
            want = data.pareto_front(f1, f2, largest)
            a = run_filter(f1, f2, largest)
            b = run_filter(f1, f2, largest, block_rows=16)
            assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], (planes.__name__, largest)
            check_sound(a[0], f1, f2, largest, None, want, f"{planes.__name__} {largest}")
            print(f"{planes.__name__} {largest}: {a[1]} candidates for a front of {len(want.cation)} of {a[2]}")


# ---------------------------------------------------------------- 5. screen_pareto against the two materialised grids
@pytest.fixture(scope="module")
def models():
    return {"visc": EC.build_members("viscosity", 3, DEV), "mp": EC.build_members("melting_point", 1, DEV)[0]}


def reference(objectives, cat, an, where=None):
    grids = []
    for o in objectives:
        T = None if o.temperature is None else [o.temperature]
        if o.ensemble:
            grids.append(o.model.predict_grid(cat, an, T, kappa=o.kappa)[2])
        else:
            grids.append(o.model.predict_grid(cat, an, T))
    grids = [g.reshape(g.shape[0], g.shape[1]) for g in grids]
    return data.pareto_front(grids[0], grids[1], (objectives[0].largest, objectives[1].largest), where)


@pytest.mark.parametrize("shape", [(7, 63), (17, 130)], ids=lambda s: "%dx%d" % s)
def test_screen_pareto_viscosity_against_melting_point(models, shape):
    cat, an = EC.species(*shape)
    for largest in DIRECTIONS:
        objs = [Objective(models["visc"][0], T0, largest[0]), Objective(models["mp"], largest=largest[1])]
        want = reference(objs, cat, an)
        assert len(want.cation) >= 5 and want.competing == shape[0] * shape[1], (shape, largest, len(want.cation))
        same(screen_pareto(objs, cat, an), want, f"visc x mp {shape} {largest}")
    assert impnn.screen_pareto is screen_pareto


def test_screen_pareto_one_model_at_two_temperatures_regrows(models):
    cat, an = EC.species(7, 63)
    v = models["visc"][0]
    objs = [Objective(v, [T0], largest=True), Objective(v, T1)]
    want = reference(objs, cat, an)
    assert len(want.cation) > 64, "the large front: more than the first capacity"
    same(screen_pareto(objs, cat, an, capacity=64), want, "visc at T0 (largest) x visc at T1")
    same(screen_pareto(objs, cat, an, capacity=64, max_pairs_per_launch=2 * 63), want, "the same, tiled")


def test_screen_pareto_transfer_ensemble_and_the_gathered_fallback(models, tmp_path):
    from test_gpu_transfer import make_transfer
    cat, an = EC.species(7, 63)
    v = models["visc"][0]
    t = make_transfer(tmp_path, S=2)
    for largest in ((False, False), (True, False)):
        objs = [Objective(t, largest=largest[0]), Objective(v, T0, largest[1])]
        same(screen_pareto(objs, cat, an), reference(objs, cat, an), f"transfer x visc {largest}")
    ens = impnn.ModelEnsemble(models["visc"])
    for largest in ((False, False), (False, True)):
        objs = [Objective(ens, T0, largest[0], kappa=EC.KAPPA), Objective(models["mp"], largest=largest[1])]
        same(screen_pareto(objs, cat, an), reference(objs, cat, an), f"ensemble score x mp {largest}")
    # the pessimistic against the optimistic score of one ensemble: its encoders run once
    objs = [Objective(ens, T0, kappa=EC.KAPPA), Objective(ens, T0, kappa=-EC.KAPPA)]
    same(screen_pareto(objs, cat, an), reference(objs, cat, an), "ensemble score at kappa and -kappa")
    wide, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=1, fp_size=32, mixing_size=72, seed=6)
    assert not wide._grid_kernels_cover()
    for pairs in (None, 3 * 63):
        objs = [Objective(wide, T0), Objective(models["mp"], largest=True)]
        same(screen_pareto(objs, cat, an, max_pairs_per_launch=pairs), reference(objs, cat, an), f"gathered x mp, {pairs}")


# ---------------------------------------------------------------- 6. tiling and where
def test_screen_pareto_tiling_and_where(models, monkeypatch):
    shape = (17, 130)
    cat, an = EC.species(*shape)
    objs = [Objective(models["visc"][0], T0), Objective(models["mp"])]
    rng = np.random.default_rng(2)
    some = rng.random(shape) < 0.3
    one = np.zeros(shape, np.bool_)
    one[11, 77] = True
    for where_b in (None, some, one, np.zeros(shape, np.bool_)):
        where = None if where_b is None else data.PairMask.from_bool(where_b, device=DEV)
        want = reference(objs, cat, an, where_b)
        for pairs in (None, 130, 5 * 130, 16 * 130 + 7):
            same(screen_pareto(objs, cat, an, where=where, max_pairs_per_launch=pairs), want,
                 f"where={None if where_b is None else int(where_b.sum())} pairs={pairs}")
    empty = screen_pareto(objs, cat, an, where=data.PairMask.from_bool(np.zeros(shape, np.bool_), device=DEV))
    assert empty.values.shape == (0, 2) and empty.competing == 0
    # a mask on another device is moved
    same(screen_pareto(objs, cat, an, where=data.PairMask.from_bool(some)), reference(objs, cat, an, some), "a host mask")
    # planes that do not fit the budget are evaluated again per stage: the same front
    monkeypatch.setattr("ionic_mpnn_amd.pareto.GRID_OUTPUT_BUDGET", 2 * shape[0] * shape[1] - 1)
    same(screen_pareto(objs, cat, an, where=data.PairMask.from_bool(some), max_pairs_per_launch=4 * 130),
         reference(objs, cat, an, some), "re-evaluated per stage")
    # no species on one side: an empty front
    none = {k: a[:0] for k, a in cat.items()}
    empty = screen_pareto(objs, none, an)
    assert empty.values.shape == (0, 2) and len(empty.cation) == 0 and empty.competing == 0


# ---------------------------------------------------------------- 7. NaN confinement
def test_a_poisoned_cation_leaves_the_competition_and_nothing_else_changes(models, monkeypatch):
    shape = (7, 63)
    cat, an = EC.species(*shape)
    v, mp = models["visc"][0], models["mp"]
    objs = [Objective(v, T0), Objective(mp)]
    g1 = v.predict_grid(cat, an, [T0])[:, :, 0].copy()
    g2 = mp.predict_grid(cat, an)
    clean = data.pareto_front(g1, g2)
    row = int(clean.cation[0])              # a cation of the clean front
    encode = v.encode_ions

    def encode_with_nan(*args, **kw):
        pc, pa = encode(*args, **kw)
        pc = pc.clone()
        pc[row, 3] = float("nan")
        return pc, pa

    monkeypatch.setattr(v, "encode_ions", encode_with_nan)
    got = screen_pareto(objs, cat, an)
    g1[row] = np.nan
    want = data.pareto_front(g1, g2)
    assert want.competing == (shape[0] - 1) * shape[1] and not (want.cation == row).any()
    same(got, want, "one cation's row poisoned")
