"""GPU: ensemble screening (ionic_mpnn_amd.ensemble.ModelEnsemble over impnn_ensemble_grid*, csrc/ensemble_grid.hip)
through every instantiation of ensemble_grid_kernel - viscosity <0,0>, melting point <1,32> (mixing_size 20) and <1,64>
(64); the materialising, mask-writing, selecting and masked selecting forms - at one tile, an exact tile, a ragged tile
and several tiles, with 1, 2, 3 and 8 members, and with one temperature more than a selecting launch takes.

What is compared with a tolerance is the statistic's arithmetic alone: the members' own float32 ``predict_grid`` outputs
are the exact member values (the kernel evaluates a member with the head grid's statements), so the float64 statistics
of those are the reference, under the project's bound (1e-5, floor 0.3; tests/test_ensemble_host.py shows the bound
attainable on these member grids and sensitive to a wrong denominator).  Everything else is exact: bits, indices, words."""
import numpy as np
import pytest
import torch

import ensemble_cases as E
from conftest import assert_close
from ionic_mpnn_amd import ModelEnsemble, _lib, data

pytestmark = pytest.mark.gpu
DEV = "cuda"
_members, _grids = {}, {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def members(kind, M, mixing=20, mixed_dims=False):
    """The first M members of a kind (built once, never changed)."""
    key = (kind, mixing, mixed_dims)
    have = _members.setdefault(key, [])
    if len(have) < M:
        have.extend(E.build_members(kind, M, torch.device(DEV), mixing, mixed_dims)[len(have):])
    return have[:M]


def case(name, kappa=E.KAPPA):
    """-> (ensemble, cations, anions, temperatures, the members' own grids (M, ...), (mean, std, score)); computed once."""
    if (name, kappa) not in _grids:
        kind, mixing, M, (C, A), nT = E.CASES[name]
        ms = members(kind, M, mixing)
        cat, an = E.species(C, A)
        T = E.temperatures(nT)
        own = np.stack([m.predict_grid(cat, an, T) for m in ms])
        ens = ModelEnsemble(ms)
        _grids[(name, kappa)] = ens, cat, an, T, own, ens.predict_grid(cat, an, T, kappa=kappa)
    return _grids[(name, kappa)]


@pytest.mark.parametrize("kind,mixing,nT", [("viscosity", 20, 3), ("melting_point", 20, 0), ("melting_point", 64, 0)])
def test_one_member_is_the_model(kind, mixing, nT):
    m = members(kind, 1, mixing)[0]
    cat, an = E.species(17, 65)
    T = E.temperatures(nT)
    want = m.predict_grid(cat, an, T)
    for kappa in (0.0, 2.5, -1.0):
        mean, std, score = ModelEnsemble([m]).predict_grid(cat, an, T, kappa=kappa)
        assert np.array_equal(bits(mean), bits(want)), kappa
        assert np.array_equal(std, np.zeros_like(std)) and np.array_equal(score, mean), kappa
    assert len(ModelEnsemble([m]).predict_grid(cat, an, T)) == 2


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_statistics_against_float64_of_the_members_own_grids(name):
    ens, cat, an, T, own, got = case(name)
    assert own.shape[0] == len(ens) > 1
    for g, want, what in zip(got, E.stats64(own, E.KAPPA), ("mean", "std", "score")):
        print(f"{name} {what}: max abs err {np.max(np.abs(g - want)):.3e}, max |ref| {np.max(np.abs(want)):.3e}")
        assert_close(g, want, rel=1e-5, what=f"{name} {what}", floor=0.3)
    # and bit for bit what the host restatement gives for the same member values
    for g, want, what in zip(got, data.ensemble_grid_stats(own, E.KAPPA), ("mean", "std", "score")):
        assert np.array_equal(bits(g), bits(want)), f"{name} {what}"


def test_members_of_different_atom_dim():
    ms = members("viscosity", 2, mixed_dims=True)
    assert [m.atom_dim for m in ms] == [32, 64]
    cat, an = E.species(17, 65)
    T = E.temperatures(1)
    own = np.stack([m.predict_grid(cat, an, T) for m in ms])
    for g, want, what in zip(ModelEnsemble(ms).predict_grid(cat, an, T, kappa=E.KAPPA), E.stats64(own, E.KAPPA), ("mean", "std", "score")):
        assert_close(g, want, rel=1e-5, what=what, floor=0.3)


def test_bits_do_not_depend_on_the_host_tiling():
    ens, cat, an, T, _, whole = case("visc-M3-33x130")
    tiled = ens.predict_grid(cat, an, T, kappa=E.KAPPA, max_pairs_per_launch=16 * 130)  # one tile row of cations a launch
    for a, b in zip(whole, tiled):
        assert np.array_equal(bits(a), bits(b))
    ens, cat, an, _, _, _ = case("mp64-M8-33x130")
    a, b = ens.predict_grid(cat, an, kappa=0.5), ens.predict_grid(cat, an, kappa=0.5, max_pairs_per_launch=16 * 130)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_bits_do_not_depend_on_the_temperature_split():
    """4097 temperatures: one more than a materialising launch takes, so the host splits the rows at 4096."""
    ens, cat, an, _, _, _ = case("visc-M8-17x65")
    most = _lib.load().impnn_ensemble_grid_max_temperatures(0, len(ens))
    T = np.linspace(250.0, 450.0, most + 1).astype(np.float32)
    cat, an = {k: v[:3] for k, v in cat.items()}, {k: v[:5] for k, v in an.items()}
    whole = ens.predict_grid(cat, an, T, kappa=E.KAPPA)
    assert whole[0].shape == (3, 5, most + 1)
    for lo, hi in ((0, 7), (most - 3, most + 1)):
        part = ens.predict_grid(cat, an, T[lo:hi], kappa=E.KAPPA, max_pairs_per_launch=5)
        for a, b in zip(whole, part):
            assert np.array_equal(bits(a[:, :, lo:hi]), bits(b))


def where_mask(C, A):
    """No pair of the first tile, one pair of the second, two in three of the rest."""
    w = np.random.default_rng(3).random((C, A)) < 0.66
    w[:16, :64] = False
    w[:16, 64:128] = False
    w[7, 100] = True
    return w


@pytest.mark.parametrize("name,kappa", [("visc-M3-33x130", 1.0), ("visc-M8-17x65", -0.5), ("mp64-M8-33x130", 2.0),
                                        ("mp20-M2-17x65", 0.0)])
def test_top_k_is_the_score_grids(name, kappa):
    ens, cat, an, T, _, (_, _, score) = case(name, kappa)
    C, A = score.shape[:2]
    if T is not None:
        assert len(T) == _lib.load().impnn_ensemble_grid_topk_max_temperatures(len(ens)) + 1  # the host splits the rows
    masks = (None, data.PairMask.from_bool(where_mask(C, A), device=DEV)) if C > 16 and A > 100 else (None,)
    for k in (1, 100, 1024, C * A + 5):
        for largest in (False, True):
            for where in masks:
                got = ens.screen_top_k(cat, an, T, k=k, kappa=kappa, largest=largest, where=where)
                want = data.grid_top_k(score, k, largest, where)
                what = (name, k, largest, where is not None)
                assert np.array_equal(bits(got.values), bits(want.values)), what
                assert np.array_equal(got.cation, want.cation) and np.array_equal(got.anion, want.anion), what


@pytest.mark.parametrize("name,kappa", [("visc-M3-33x130", 1.0), ("mp64-M8-33x130", 2.0), ("visc-M2-1x1", E.KAPPA)])
def test_mask_is_the_score_grids(name, kappa):
    ens, cat, an, T, _, (_, _, score) = case(name, kappa)
    lo, hi = np.quantile(score, [0.25, 0.6]).astype(np.float32)
    for at_least, at_most in ((lo, hi), (None, hi), (lo, None)):
        got = ens.screen_mask(cat, an, T, at_least=at_least, at_most=at_most, kappa=kappa)
        want = (score >= (-np.inf if at_least is None else at_least)) & (score <= (np.inf if at_most is None else at_most))
        assert got.shape == score.shape and np.array_equal(got.to_bool(), want), (name, at_least, at_most)
        A = score.shape[1]
        if A % 32:  # the pad bits of a row's last word
            last = got.words.cpu().numpy()[..., -1].astype(np.int64) & 0xFFFFFFFF
            assert not np.any(last >> (A % 32)), name


def test_a_nan_row_of_one_member_stays_in_its_row(monkeypatch):
    ens, cat, an, T, _, clean = case("visc-M3-16x64")
    poisoned = ens.models[1]
    encode = poisoned.encode_ions

    def encode_with_nan(*args, **kw):
        pc, pa = encode(*args, **kw)
        pc = pc.clone()
        pc[5, 3] = float("nan")
        return pc, pa

    monkeypatch.setattr(poisoned, "encode_ions", encode_with_nan)
    got = ens.predict_grid(cat, an, T, kappa=E.KAPPA)
    for g, c in zip(got, clean):
        nan = np.isnan(g)
        assert nan[5].all() and not np.delete(nan, 5, axis=0).any()
        assert np.array_equal(bits(np.delete(g, 5, axis=0)), bits(np.delete(c, 5, axis=0)))
    C, A = 16, 64
    top = ens.screen_top_k(cat, an, T, k=C * A, kappa=E.KAPPA)
    assert np.isnan(top.values[:, -A:]).all() and not np.isnan(top.values[:, :-A]).any()
    assert (top.cation[:, -A:] == 5).all() and np.array_equal(top.anion[0, -A:], np.arange(A))
    mask = ens.screen_mask(cat, an, T, at_least=-np.inf, at_most=np.inf, kappa=E.KAPPA).to_bool()
    assert not mask[5].any() and np.delete(mask, 5, axis=0).all()


@pytest.mark.parametrize("name", ["visc-M3-16x64", "mp20-M2-17x65"])
def test_predict_pairs_reads_the_mean_and_spread_of_a_top_k(name):
    ens, cat, an, T, _, (mean, std, _) = case(name)
    top = ens.screen_top_k(cat, an, T, k=50, kappa=E.KAPPA)
    if T is None:
        got = ens.predict_pairs(cat, an, top.cation, top.anion)
        want = mean[top.cation, top.anion], std[top.cation, top.anion]
    else:
        got = ens.predict_pairs(cat, an, top.cation[1], top.anion[1], T)
        want = mean[top.cation[1], top.anion[1], :], std[top.cation[1], top.anion[1], :]
    for g, w, what in zip(got, want, ("mean", "std")):
        assert_close(g, w, rel=1e-5, what=f"{name} {what}", floor=0.3)
