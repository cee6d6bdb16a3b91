"""The host layer of a screen without a device: screening._Screen around a stand-in model whose fallback paths run on
the CPU - the cation and temperature tiling, the top-k merge across tiles, the per-anion partner merge, the carried
summary records, the mask assembly and the rank fallback, each held bit for bit (NaNs included) to the data.*
references on the once-materialised grid, under every tiling - and the three argument helpers and the range generators
on their own.  The stand-in's rows are small integers, so every sum is exact and the grid is full of ties, of both
signs."""
import ast
import functools
import warnings

import numpy as np
import pytest
import torch

from conftest import ROOT
from ionic_mpnn_amd import data, ops, screening

CPU = torch.device("cpu")
SHAPE = (37, 70)   # crosses a 32-bit mask word and the 64-anion block; summary ranges 16 + 16 + 5
EMPTY = ((0, 70), (37, 0))
TILINGS = (None, 1, 70, 211, 1120, 2590)
TEMPERATURES = {"viscosity": [250.0, 300.0, 420.0], "melting_point": None}
BOUNDS = (-2.0, 3.0)


class StubModel:
    """What screening.py requires of a model, with no kernel behind it: nothing covers, so every screen takes its
    fallback through ``_grid_gathered``."""

    def __init__(self, kind):
        self.kind, self.device, self.grid_head_mode = kind, CPU, "auto"

    def encode_ions(self, cations, anions, batch_size=4096):
        def rows(ion, seed):
            return torch.from_numpy(np.random.default_rng(seed).integers(-3, 4, (len(ion["atom"]), 4)).astype(np.float32))
        return rows(cations, 1), rows(anions, 2)

    def _grid_kernels_cover(self):
        return False

    def _transfer_grid_covers(self):
        return False

    def _grid_gathered(self, pc, pa, T):
        v = (pc[:, None, :] * pa[None, :, :]).sum(-1)
        v = torch.where(v == 5, torch.full_like(v, float("nan")), v)
        return v if T is None else v[:, :, None] + torch.round(T / 100)[None, None, :]


class Screen(screening._Screen):
    grid_max_t = 2  # three temperatures: the fallback's temperature split runs too


def ions(n):
    return {"atom": np.zeros((n, 3), np.int32), "bond": np.zeros((n, 2), np.int32), "connectivity": np.zeros((n, 2, 2), np.int32)}


@functools.lru_cache(maxsize=None)
def case(kind, shape):
    """-> (build: where -> Screen, grid: the stand-in's head over all pairs at once, where: a mask of ~60 % of them)."""
    model, cat, an = StubModel(kind), ions(shape[0]), ions(shape[1])
    T = screening._screen_request(kind, "test", cat, an, TEMPERATURES[kind], None, None)
    pc, pa = model.encode_ions(cat, an)
    grid = model._grid_gathered(pc, pa, T).numpy()
    grid.setflags(write=False)
    where = data.PairMask.from_bool(np.random.default_rng(3).random(shape) < 0.6)
    return (lambda wh: Screen(model, cat, an, T, wh, 4096)), grid, where


def flat(x):
    """The arrays of a result (TopK, BestPartners, IonSummary and its records, RankCut, PairMask, ...) in order."""
    if isinstance(x, data.PairMask):
        return [x.words.numpy()]
    if isinstance(x, data.IonSummary):
        return [a for y in (*x, *x.records) for a in flat(y)]
    if isinstance(x, tuple):
        return [a for y in x for a in flat(y)]
    return [x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)]


def same_bits(got, want):
    got, want = flat(got), flat(want)
    return len(got) == len(want) and all(a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
                                         for a, b in zip(got, want))


def tiled_outputs(kind, shape, mp):
    """Every tiled operation of the screen under ``max_pairs_per_launch = mp`` -> {name: (result, reference)}."""
    build, grid, where = case(kind, shape)
    blocks = ops.SUMMARY_BLOCKS[0]
    out = {"values": (build(None).values(mp), grid),
           "pair_mask": (build(None).pair_mask(np.float32(BOUNDS[0]), np.float32(BOUNDS[1]), mp).to_bool(),
                         (grid >= BOUNDS[0]) & (grid <= BOUNDS[1]))}
    for name, wh in (("all", None), ("where", where)):
        s = build(wh)
        for largest in (False, True):
            for k in (9, 3000):
                out[f"{name}/{int(largest)}/top_k{k}"] = s.top_k(k, largest, mp), data.grid_top_k(grid, k, largest, wh)
            out[f"{name}/{int(largest)}/best_partners"] = (s.best_partners(3, largest, mp),
                                                           data.grid_best_partners(grid, 3, largest, where=wh))
        out[f"{name}/ion_summary"] = s.ion_summary(mp), data.grid_ion_summary(grid, wh, blocks)
    return out


def rank_outputs(kind, shape):
    """The rank cut and the best-k mask, for k inside and above the competing count -> {name: (result, reference)}."""
    build, grid, where = case(kind, shape)
    planes = grid.shape[2] if grid.ndim == 3 else 1
    out = {}
    for name, wh in (("all", None), ("where", where)):
        for largest in (False, True):
            for k in (100, 3000):
                cut, words = build(wh).rank(k, largest, True)
                assert same_bits(build(wh).rank(k, largest, False), (cut, None))
                want = data.PairMask.from_bool(data.grid_best_mask(grid, k, largest, wh)).words.reshape(planes, shape[0], -1)
                out[f"{name}/{int(largest)}/rank{k}"] = ((cut, words.numpy()),
                                                         (tuple(np.atleast_1d(x) for x in data.grid_rank(grid, k, largest, wh)), want.numpy()))
    return out


def test_the_stand_in_grid_has_nans_ties_and_both_signs():
    for kind in TEMPERATURES:
        grid = case(kind, SHAPE)[1]
        plane = grid[..., 0] if grid.ndim == 3 else grid
        live = plane[~np.isnan(plane)]
        assert 0 < np.isnan(plane).sum() < plane.size // 10
        assert live.min() < 0 < live.max() and len(np.unique(live)) < live.size // 20
        assert np.array_equal(live, np.round(live))


@pytest.mark.parametrize("mp", TILINGS)
@pytest.mark.parametrize("kind", sorted(TEMPERATURES))
def test_every_tiling_gives_the_references_bits(kind, mp):
    out = tiled_outputs(kind, SHAPE, mp)
    assert len(out) == 2 + 2 * (2 * 3 + 1)
    wrong = [name for name, (got, want) in out.items() if not same_bits(got, want)]
    assert not wrong, wrong


@pytest.mark.parametrize("kind", sorted(TEMPERATURES))
def test_rank_fallback_gives_the_references_bits(kind):
    _, grid, where = case(kind, SHAPE)
    assert 100 < where.count() < 3000 and grid[..., 0].size < 3000  # k = 3000: more than compete, with and without the mask
    wrong = [name for name, (got, want) in rank_outputs(kind, SHAPE).items() if not same_bits(got, want)]
    assert not wrong, wrong


@pytest.mark.parametrize("shape", EMPTY)
@pytest.mark.parametrize("kind", sorted(TEMPERATURES))
def test_empty_grids(kind, shape):
    """0 x 70 and 37 x 0: no tile, nothing competes, and every result has its stated shape."""
    build, grid, where = case(kind, shape)
    C_, A_ = shape
    visc = kind == "viscosity"
    P = 3 if visc else 1
    lead = lambda *dims: (P, *dims) if visc else dims
    nan, none = (lambda *d: np.full(d, data.QUIET_NAN, np.float32)), (lambda *d: np.full(d, -1, np.int64))
    stats = lambda *d: data.IonStats(np.zeros(d, np.int64), nan(*d), nan(*d), nan(*d), nan(*d))
    for wh in (None, where):
        s = build(wh)
        for mp in TILINGS:
            assert list(s.tiles(mp, False)) == [] and list(s.tiles(mp, True)) == []
            assert same_bits(s.values(mp), grid) and grid.shape == ((C_, A_, 3) if visc else (C_, A_))
            mask = s.pair_mask(np.float32(BOUNDS[0]), np.float32(BOUNDS[1]), mp)
            assert mask.shape == grid.shape
            assert same_bits(mask, torch.zeros(*lead(C_, data.mask_row_words(A_)), dtype=torch.int32))
            for largest in (False, True):
                for k in (9, 3000):
                    assert same_bits(s.top_k(k, largest, mp), data.TopK(nan(*lead(0)), none(*lead(0)), none(*lead(0))))
                assert same_bits(s.best_partners(3, largest, mp),
                                 data.BestPartners(data.Partners(nan(*lead(C_, 3)), none(*lead(C_, 3))),
                                                   data.Partners(nan(*lead(A_, 3)), none(*lead(A_, 3)))))
            assert same_bits(tuple(s.ion_summary(mp)), (stats(*lead(C_)), stats(*lead(A_)), stats(*lead())))
        for largest in (False, True):
            for k in (100, 3000):
                cut, words = s.rank(k, largest, True)
                assert same_bits(cut, data.RankCut(nan(P), none(P), none(P), np.zeros(P, np.int64)))
                assert same_bits(words, torch.zeros(P, C_, data.mask_row_words(A_), dtype=torch.int32))
                assert same_bits(s.rank(k, largest, False), (cut, None))


# ---------------------------------------------------------------- the range generators
def test_cation_ranges_cover_the_axis_once_and_in_order():
    for C_ in (0, 1, 15, 16, 37, 100):
        for A_ in (1, 7, 70):
            for pairs in (1, A_, 3 * A_ + 1, 16 * A_, 33 * A_, C_ * A_ + 1, 1 << 40):
                for multiple in (1, screening.SUMMARY_RANGE):
                    got = list(screening.cation_ranges(C_, A_, pairs, multiple=multiple))
                    assert [i for lo, hi in got for i in range(lo, hi)] == list(range(C_))
                    assert all(lo < hi for lo, hi in got)
                    step = max(multiple, pairs // A_ // multiple * multiple)
                    assert all(hi - lo == step for lo, hi in got[:-1]) and all(hi - lo <= step for lo, hi in got[-1:])
                    assert all(lo % multiple == 0 for lo, _ in got)
    assert list(screening.cation_ranges(37, 70, 1120, multiple=16)) == [(0, 16), (16, 32), (32, 37)]
    assert list(screening.cation_ranges(37, 70, 1, multiple=16)) == [(0, 16), (16, 32), (32, 37)]  # at least one range of 16
    assert list(screening.cation_ranges(37, 70, 211)) == [(lo, min(37, lo + 3)) for lo in range(0, 37, 3)]
    assert list(screening.cation_ranges(37, 70, 1 << 40, most=140)) == [(lo, min(37, lo + 2)) for lo in range(0, 37, 2)]
    assert list(screening.cation_ranges(37, 0, 100)) == []  # an empty grid: nothing


def test_temperature_ranges():
    assert list(screening.ranges(0, 4)) == []
    assert list(screening.ranges(3, 2)) == [(0, 2), (2, 3)]
    assert list(screening.ranges(8, 4)) == [(0, 4), (4, 8)]


def test_tiles_visit_every_cation_and_temperature_row_once():
    build, _, where = case("viscosity", SHAPE)
    s = build(where)
    for mp, select in ((211, False), (211, True), (None, False)):
        seen = np.zeros((SHAPE[0], 3), np.int64)
        for lo, hi, t0, t1, g, wh in s.tiles(mp, select):
            seen[lo:hi, t0:t1] += 1
            assert g is None and wh.shape == (hi - lo, SHAPE[1]) and t1 - t0 <= (ops.SELECT_MAX_T if select else 2)
        assert (seen == 1).all()


# ---------------------------------------------------------------- the argument helpers
def test_mask_bounds():
    lo, hi = screening.mask_bounds("screen_mask", None, 2.5)
    assert (lo, hi) == (-np.inf, 2.5) and type(lo) is np.float32 and type(hi) is np.float32
    assert screening.mask_bounds("screen_mask", 0.1, None) == (np.float32(0.1), np.inf)  # as float32
    assert screening.mask_bounds("screen_mask", float("-inf"), float("inf")) == (-np.inf, np.inf)
    with pytest.raises(ValueError, match="^screen_mask needs a bound: at_least, at_most or both$"):
        screening.mask_bounds("screen_mask", None, None)
    with pytest.raises(ValueError, match="^screen_domain_mask needs a bound: at_most, at_least or both$"):
        screening.mask_bounds("screen_domain_mask", None, None, "at_most, at_least")
    for bounds in ((float("nan"), None), (None, float("nan")), (0.0, float("nan"))):
        with pytest.raises(ValueError, match="^a screen_mask bound is NaN$"):
            screening.mask_bounds("screen_mask", *bounds)


def test_at_least_one():
    assert screening.at_least_one("k", 1) == 1 and type(screening.at_least_one("k", np.int64(7))) is int
    assert screening.at_least_one("m", 3.9) == 3
    for name, v in (("k", 0), ("m", -2), ("k", 0.5)):
        with pytest.raises(ValueError, match=f"^{name} must be >= 1$"):
            screening.at_least_one(name, v)


def test_score_kappa():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert screening.score_kappa(1.5) == 1.5 and type(screening.score_kappa(1.5)) is float
        assert screening.score_kappa(0.1) == float(np.float32(0.1))  # as the kernels see it
        for bad in (1e40, -1e40, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="kappa must be finite"):
                screening.score_kappa(bad)


def test_screening_does_not_import_the_model():
    tree = ast.parse((ROOT / "ionic_mpnn_amd" / "screening.py").read_text())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.level:
            names |= {node.module} if node.module else {a.name for a in node.names}
    assert names <= {"data", "ops", "_lib"}, names
