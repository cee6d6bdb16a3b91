"""Monte-Carlo dropout of the transfer head over a cation x anion grid on the GPU (csrc/transfer_mc_grid.hip,
ionic_mpnn_amd/mc_dropout.py): impnn_transfer_mc_grid and its mask / top-k forms against impnn_transfer_head_grid
(bitwise, all-ones table), against the fp64 reference of tests/transfer_ref.py with the numpy Philox masks of
tests/philox_ref.py (1e-5), and against ``data.ensemble_grid_stats`` / ``data.grid_top_k`` / ``PairMask.from_bool`` on
the returned samples and score (bitwise).

The case is tests/mc_dropout_cases.py's: one transfer model with random weights and non-trivial moving statistics, 19
cations x 70 anions; every grid of GRIDS is the corner of that product (the transfer tile is 8 x 32), S is in
{1, 2, 7, max}.  The fp64 reference is computed once per module for max samples and shared; tests/test_mc_dropout_host.py
holds the case's preconditions (a plain float32 walk at half the bound, a spread on at least 90 % of the pairs)."""
import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, data, ops
from conftest import assert_close

import mc_dropout_cases as K
from mc_dropout_cases import AN, CN, DRAW, GRIDS, RATE, corner
from test_gpu_grid import SENTINEL, bits, guarded, split_guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
KAPPAS = (0.0, 1.5, -1.0)


def sample_counts():
    most = int(_lib.load().impnn_transfer_mc_grid_max_samples())
    return [1, 2, 7, most]


@pytest.fixture(scope="module")
def mc(tmp_path_factory):
    t = K.make_transfer(tmp_path_factory.mktemp("mc_dropout"), DEV)
    assert t.mp_dropout.rate == RATE and t.mp_dropout.seed == K.SEED
    cat, an = K.species()
    most = sample_counts()[-1]
    pc, pa = t.encode_ions(cat, an)
    tensors = t._head_tensors()
    uc = ops.transfer_ion_half("cat", pc, tensors, t.fp_size, t.mixing_size)
    ua = ops.transfer_ion_half("an", pa, tensors, t.fp_size, t.mixing_size)
    return {"t": t, "cat": cat, "an": an, "masks": K.masks(DRAW, most), "ref": K.reference(t.state_dict(), cat, an, DRAW, most),
            "uc": uc, "ua": ua, "image": t._transfer_image(), "most": most}


def run(mc, Cn, An, table, kappa=0.0):
    """impnn_transfer_mc_grid on the corner Cn x An -> numpy (mean, std, score, samples)."""
    g = ops.transfer_mc_grid_operands(mc["uc"][:Cn], mc["ua"][:An], mc["image"], table, kappa)
    return tuple(x.cpu().numpy() for x in ops.transfer_mc_grid(g, return_samples=True))


# ---------------------------------------------------------------- 1. the all-ones table
@pytest.mark.parametrize("shape", GRIDS, ids=lambda s: "%dx%d" % s)
def test_all_ones_table_is_the_transfer_grid_bitwise(mc, shape):
    """With every multiplier 1 every sample plane has the bits of ops.transfer_head_grid for the same operands: the new
    tile is the old one bit for bit, for every S.

    The mean and std of S equal values: the statistic's pinned order sums them one by one in float32 (s = v; s = s + v;
    ...), and the running sum k * v is not a float32 for every k (3 v needs up to two more mantissa bits), so from S = 3
    on the mean of S copies of v is not v bit for bit and the std not exactly 0 (data.ensemble_grid_stats of 7 / 64
    copies of normal(0, 1) floats: half / nine tenths of the means differ from v in the last bits, std up to 4e-6).
    Asserted, therefore: for S in {1, 2}, where the sums are exact, the mean has the grid's bits and std is exactly +0;
    for every S the three have the bits of data.ensemble_grid_stats of S copies of the grid, the mean is within S
    roundings (S * 2^-24 relative) of the grid and the std within the same of 0."""
    Cn, An = shape
    want = ops.transfer_head_grid(mc["uc"][:Cn], mc["ua"][:An], mc["image"]).cpu().numpy()
    for S in sample_counts():
        ones = torch.ones(S, 128, dtype=torch.float32, device=DEV)
        mean, std, score, samples = run(mc, Cn, An, ones, kappa=1.5)
        assert samples.shape == (S, Cn, An)
        for s in range(S):
            assert np.array_equal(bits(samples[s]), bits(want)), f"sample plane {s} of {S}, {shape}"
        for got, stat, what in zip((mean, std, score), data.ensemble_grid_stats(np.broadcast_to(want, (S, Cn, An)), 1.5),
                                   ("mean", "std", "score")):
            assert np.array_equal(bits(got), bits(stat)), f"{what} of {S} equal samples, {shape}"
        if S <= 2:
            assert np.array_equal(bits(mean), bits(want)) and np.array_equal(bits(std), bits(np.zeros_like(std))), (S, shape)
        slack = S * 2.0 ** -24 * np.abs(want)
        assert (np.abs(mean.astype(np.float64) - want) <= slack).all() and (std <= slack).all(), (S, shape)


# ---------------------------------------------------------------- 2. samples against fp64
def test_reference_spread_is_not_trivial(mc):
    """Precondition, from the fp64 reference alone: the spread a test below checks exists on at least 90 % of the pairs."""
    for S in sample_counts()[1:]:
        got = K.spread_fraction(mc["ref"][:S])
        print(f"S={S}: fp64 std > 1e-3 max|mean| on {100 * got:.1f} % of the pairs")
        assert got >= 0.9, (S, got)


def test_the_table_is_the_training_mask(mc):
    t = mc["t"]
    for S in sample_counts():
        table = t.mc_dropout(S, DRAW).multipliers()
        assert table.shape == (S, 128) and table.dtype == torch.float32 and table.is_cuda
        assert np.array_equal(bits(table.cpu().numpy()), bits(mc["masks"][:S])), f"S={S}: the table is reference_mask's rows"
    kept = mc["masks"] != 0
    assert 0.6 < kept.mean() < 0.8 and (mc["masks"][kept] == np.float32(1.0) / (np.float32(1.0) - np.float32(RATE))).all()
    # and it is what the Dropout layer applies in a training pass at that step, row for row
    counter = torch.tensor([DRAW], dtype=torch.int64, device=DEV)
    ones = torch.ones(7, 128, dtype=torch.float32, device=DEV)
    applied = t.mp_dropout(ones, training=True, counter=counter).cpu().numpy()
    assert np.array_equal(bits(applied), bits(mc["masks"][:7]))


@pytest.mark.parametrize("shape", GRIDS, ids=lambda s: "%dx%d" % s)
def test_samples_against_fp64(mc, shape):
    Cn, An = shape
    mcd = mc["t"].mc_dropout(mc["most"], DRAW)
    out = mcd.predict_grid(corner(mc["cat"], Cn), corner(mc["an"], An), return_samples=True)
    assert len(out) == 3 and out[2].shape == (mc["most"], Cn, An)
    for s in range(mc["most"]):
        assert_close(out[2][s], mc["ref"][s, :Cn, :An], 1e-5, f"sample {s} vs transfer_ref, {shape}")
    # fewer samples are the first rows of the same table: the same planes
    for S in sample_counts()[:-1]:
        few = mc["t"].mc_dropout(S, DRAW).predict_grid(corner(mc["cat"], Cn), corner(mc["an"], An), return_samples=True)[2]
        assert np.array_equal(bits(few), bits(out[2][:S])), f"S={S} of {shape}"


# ---------------------------------------------------------------- 3. the statistic
@pytest.mark.parametrize("shape", GRIDS, ids=lambda s: "%dx%d" % s)
def test_statistic_is_ensemble_grid_stats_of_the_samples(mc, shape):
    """mean / std / score have the bits of data.ensemble_grid_stats(returned samples, kappa).  Against fp64: the mean at
    1e-5; the std at 1e-5 with the tensor scale taken as max|mean| - the std is a difference of sample values each good
    to 1e-5 of that scale, so that is the scale its error has, not its own (smaller) magnitude."""
    Cn, An = shape
    for S in sample_counts():
        table = torch.from_numpy(mc["masks"][:S]).to(DEV)
        for kappa in KAPPAS:
            mean, std, score, samples = run(mc, Cn, An, table, kappa)
            for got, stat, what in zip((mean, std, score), data.ensemble_grid_stats(samples, kappa), ("mean", "std", "score")):
                assert np.array_equal(bits(got), bits(stat)), f"{what} S={S} kappa={kappa} {shape}"
        ref = mc["ref"][:S, :Cn, :An]
        mean64, std64 = ref.mean(0), ref.std(0)
        assert_close(mean, mean64, 1e-5, f"mean vs fp64 S={S} {shape}")
        scale = np.abs(mean64).max()
        err = np.abs(std.astype(np.float64) - std64).max() / scale
        print(f"S={S} {shape}: std error {err:.2e} of max|mean|")
        assert err <= 1e-5, f"std vs fp64 S={S} {shape}: {err:.2e} of max|mean| (rel=1e-5)"
        if S == 1:
            assert np.array_equal(bits(std), bits(np.zeros_like(std)))


def test_model_statistic_and_kappa(mc):
    cat, an = mc["cat"], mc["an"]
    mcd = mc["t"].mc_dropout(7, DRAW)
    pair = mcd.predict_grid(cat, an)
    assert len(pair) == 2 and pair[0].shape == (CN, AN) and pair[0].dtype == np.float32
    for kappa in KAPPAS:
        mean, std, score, samples = mcd.predict_grid(cat, an, kappa=kappa, return_samples=True)
        assert np.array_equal(bits(mean), bits(pair[0])) and np.array_equal(bits(std), bits(pair[1]))
        for got, stat in zip((mean, std, score), data.ensemble_grid_stats(samples, kappa)):
            assert np.array_equal(bits(got), bits(stat)), kappa


# ---------------------------------------------------------------- 4. placement
def test_placement_does_not_change_a_bit(mc):
    t, cat, an = mc["t"], mc["cat"], mc["an"]
    mcd = t.mc_dropout(7, DRAW)
    whole = mcd.predict_grid(cat, an, kappa=1.5, return_samples=True)
    again = mcd.predict_grid(cat, an, kappa=1.5, return_samples=True)
    for a, b in zip(whole, again):
        assert np.array_equal(bits(a), bits(b)), "two runs"
    for pairs in (20, AN, 3 * AN + 1):
        tiled = mcd.predict_grid(cat, an, kappa=1.5, return_samples=True, max_pairs_per_launch=pairs)
        for a, b in zip(whole, tiled):
            assert np.array_equal(bits(a), bits(b)), f"host tiles of {pairs} pairs"
    # a sub-grid that starts inside a tile is the grid's block
    table = mcd.multipliers()
    sub = ops.transfer_mc_grid(ops.transfer_mc_grid_operands(mc["uc"][5:14], mc["ua"][30:69], mc["image"], table, 1.5), True)
    for a, b in zip(whole, sub):
        assert np.array_equal(bits(b.cpu().numpy()), bits(a[..., 5:14, 30:69])), "a sub-grid"
    # listed pairs: the grid's bits
    rng = np.random.default_rng(4)
    ci, ai = rng.integers(0, CN, size=41), rng.integers(0, AN, size=41)
    mean, std = mcd.predict_pairs(cat, an, ci, ai)
    assert mean.shape == std.shape == (41,) and mean.dtype == np.float32
    assert np.array_equal(bits(mean), bits(whole[0][ci, ai])) and np.array_equal(bits(std), bits(whole[1][ci, ai]))
    empty = mcd.predict_pairs(cat, an, [], [])
    assert empty[0].shape == (0,) and empty[1].shape == (0,)
    with pytest.raises(IndexError):
        mcd.predict_pairs(cat, an, [CN], [0])


def test_output_alignment_does_not_change_a_bit(mc):
    """Every output at each 4-byte phase of a 16-byte boundary: every element written, none outside, the same bits."""
    lib = _lib.load()
    Cn, An, S = 9, 33, 7
    uc, ua, image = mc["uc"][:Cn].contiguous(), mc["ua"][:An].contiguous(), mc["image"]
    table = torch.from_numpy(mc["masks"][:S]).to(DEV)
    first = run(mc, Cn, An, table, 1.5)
    for offset in range(1, 4):
        bufs = [guarded(Cn * An, offset) for _ in range(3)] + [guarded(S * Cn * An, offset)]
        _lib.check(lib.impnn_transfer_mc_grid(_lib.ptr(uc), _lib.ptr(ua), _lib.ptr(image), image.numel(), _lib.ptr(table),
                                              S, 1.5, *[b[1] for b in bufs], Cn, An, _lib.stream_ptr()))
        torch.cuda.synchronize()
        for (whole, _), want in zip(bufs, first):
            got = split_guarded(whole, want.size, offset)
            assert np.array_equal(bits(got), bits(want.reshape(-1))), f"offset {offset}"
    # a null output is skipped: only the score
    whole, ptr = guarded(Cn * An, 1)
    _lib.check(lib.impnn_transfer_mc_grid(_lib.ptr(uc), _lib.ptr(ua), _lib.ptr(image), image.numel(), _lib.ptr(table), S,
                                          1.5, None, None, ptr, None, Cn, An, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(bits(split_guarded(whole, Cn * An, 1)), bits(first[2].reshape(-1)))
    # zero work touches nothing
    whole, ptr = guarded(16, 0)
    assert lib.impnn_transfer_mc_grid(_lib.ptr(uc), _lib.ptr(ua), _lib.ptr(image), image.numel(), _lib.ptr(table), S, 1.5,
                                      ptr, None, None, None, 0, An, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert (whole.cpu().numpy().view(np.uint32) == SENTINEL.view(np.uint32)).all()
    g0 = ops.transfer_mc_grid_operands(uc[:0], ua, image, table)
    assert all(x.shape == (0, An) for x in ops.grid_values(g0))


def test_a_nan_row_and_a_nan_column_stay_where_they_are(mc):
    S = 7
    table = torch.from_numpy(mc["masks"][:S]).to(DEV)
    clean = run(mc, CN, AN, table, 1.5)
    assert all(np.isfinite(x).all() for x in clean)
    uc, ua = mc["uc"].clone(), mc["ua"].clone()
    uc[17, 3], ua[40, 200] = float("nan"), float("nan")
    g = ops.transfer_mc_grid_operands(uc, ua, mc["image"], table, 1.5)
    got = [x.cpu().numpy() for x in ops.transfer_mc_grid(g, return_samples=True)]
    keep = np.ones((CN, AN), bool)
    keep[17], keep[:, 40] = False, False
    for what, a, b in zip(("mean", "std", "score", "samples"), got, clean):
        assert np.isnan(a[..., 17, :]).all() and np.isnan(a[..., :, 40]).all(), f"{what}: the NaN row and the NaN column"
        assert np.array_equal(bits(a[..., keep]), bits(b[..., keep])), f"{what}: every other pair keeps its bits"


# ---------------------------------------------------------------- 5. forms
@pytest.mark.parametrize("shape", GRIDS, ids=lambda s: "%dx%d" % s)
def test_screen_mask_is_the_thresholded_score(mc, shape):
    Cn, An = shape
    cat, an = corner(mc["cat"], Cn), corner(mc["an"], An)
    for S in sample_counts():
        mcd = mc["t"].mc_dropout(S, DRAW)
        for kappa in (0.0, 1.5):
            score = mcd.predict_grid(cat, an, kappa=kappa)[2]
            lo, hi = np.float32(np.quantile(score, 0.3)), np.float32(np.quantile(score, 0.8))
            for at_least, at_most in ((lo, hi), (None, hi), (lo, None), (hi, lo)):
                got = mcd.screen_mask(cat, an, at_least=at_least, at_most=at_most, kappa=kappa)
                want = np.ones_like(score, bool)
                if at_least is not None:
                    want &= score >= at_least
                if at_most is not None:
                    want &= score <= at_most
                assert got.shape == (Cn, An)
                assert np.array_equal(got.words.cpu().numpy(), data.PairMask.from_bool(want).words.cpu().numpy()), (S, kappa, shape)
    tiled = mcd.screen_mask(cat, an, at_most=hi, kappa=1.5, max_pairs_per_launch=An + 1)
    assert np.array_equal(tiled.words.cpu().numpy(), mcd.screen_mask(cat, an, at_most=hi, kappa=1.5).words.cpu().numpy())


def _where_cases(Cn, An, rng):
    """Masks over (Cn, An): random, one with whole empty tiles (only the last cation row and the first anions), one pair."""
    sparse = np.zeros((Cn, An), bool)
    sparse[Cn - 1, :min(An, 5)] = True
    one = np.zeros((Cn, An), bool)
    one[Cn // 2, An // 2] = True
    return {"random": rng.random((Cn, An)) < 0.4, "empty tiles": sparse, "one pair": one}


@pytest.mark.parametrize("shape", GRIDS, ids=lambda s: "%dx%d" % s)
def test_screen_top_k_is_grid_top_k_of_the_score(mc, shape):
    Cn, An = shape
    cat, an = corner(mc["cat"], Cn), corner(mc["an"], An)
    rng = np.random.default_rng(Cn * 100 + An)
    for S in sample_counts():
        mcd = mc["t"].mc_dropout(S, DRAW)
        score = mcd.predict_grid(cat, an, kappa=1.5)[2]
        wheres = {None: None, **_where_cases(Cn, An, rng)}
        for name, where in wheres.items():
            live = Cn * An if where is None else int(where.sum())
            for k in sorted({1, live + 3, min(live + 3, 40)}):
                for largest in (False, True):
                    mask = None if where is None else data.PairMask.from_bool(where, device=DEV)
                    got = mcd.screen_top_k(cat, an, k=k, kappa=1.5, largest=largest, where=mask)
                    want = data.grid_top_k(score, k, largest, where)
                    assert got.values.shape == (min(k, live),), (S, name, k)
                    assert np.array_equal(bits(got.values), bits(want.values)), (S, name, k, largest, shape)
                    assert np.array_equal(got.cation, want.cation) and np.array_equal(got.anion, want.anion), (S, name, k, largest)
    # host tiles and few workgroups: the same selection
    want = data.grid_top_k(score, 5, False)
    got = mcd.screen_top_k(cat, an, k=5, kappa=1.5, max_pairs_per_launch=An + 1)
    assert np.array_equal(bits(got.values), bits(want.values)) and np.array_equal(got.cation, want.cation)
    g = ops.transfer_mc_grid_operands(mc["uc"][:Cn], mc["ua"][:An], mc["image"], mcd.multipliers(), 1.5)
    v, ci, ai = (x.cpu().numpy() for x in ops.grid_topk(g, 5, workgroups=2))
    m = min(5, Cn * An)
    assert np.array_equal(bits(v[0, :m]), bits(want.values)) and np.array_equal(ci[0, :m], want.cation) and np.array_equal(ai[0, :m], want.anion)


# ---------------------------------------------------------------- 6. draws, weights
def test_another_draw_is_another_set_of_samples(mc):
    t, cat, an = mc["t"], corner(mc["cat"], 9), corner(mc["an"], 33)
    a = t.mc_dropout(7, DRAW).predict_grid(cat, an, return_samples=True)
    same = t.mc_dropout(7, DRAW).predict_grid(cat, an, return_samples=True)
    other = t.mc_dropout(7, DRAW + 1).predict_grid(cat, an, return_samples=True)
    for x, y in zip(a, same):
        assert np.array_equal(bits(x), bits(y)), "the same draw: the same bits"
    assert not np.array_equal(bits(t.mc_dropout(7, DRAW).multipliers().cpu().numpy()),
                              bits(t.mc_dropout(7, DRAW + 1).multipliers().cpu().numpy()))
    for s in range(7):
        assert np.abs(a[2][s] - other[2][s]).max() > 1e-3 * np.abs(a[2]).max(), f"sample {s} must change with the draw"
    assert not np.array_equal(bits(a[0]), bits(other[0])) and not np.array_equal(bits(a[1]), bits(other[1]))
    ref = K.reference(t.state_dict(), cat, an, DRAW + 1, 7)
    for s in range(7):
        assert_close(other[2][s], ref[s], 1e-5, f"draw {DRAW + 1}, sample {s} vs transfer_ref")


def test_the_table_follows_the_dropout_and_the_image_the_weights(mc, tmp_path):
    t = K.make_transfer(tmp_path, DEV)
    cat, an = corner(mc["cat"], 9), corner(mc["an"], 33)
    mcd = t.mc_dropout(7, DRAW)
    before = mcd.predict_grid(cat, an, return_samples=True)
    first = mcd.multipliers()
    assert mcd.multipliers() is first, "cached while nothing changes"
    t.mp_dropout.seed += 1
    assert not np.array_equal(bits(mcd.multipliers().cpu().numpy()), bits(first.cpu().numpy())), "another seed: another table"
    t.mp_dropout.seed -= 1
    t.mp_dropout.rate = 0.0
    try:
        plain = t.predict_grid(cat, an)
        mean, std, samples = mcd.predict_grid(cat, an, return_samples=True)
        assert (mcd.multipliers() == 1.0).all()
        assert all(np.array_equal(bits(s), bits(plain)) for s in samples), "rate 0: every sample is predict_grid"
    finally:
        t.mp_dropout.rate = RATE
    state = t.state_dict()
    state["mp_dense_3/kernel"] = (state["mp_dense_3/kernel"] * 1.25).astype(np.float32)
    t.load_weights(state)
    after = mcd.predict_grid(cat, an, return_samples=True)
    assert np.abs(after[2] - before[2]).max() > 1e-2 * np.abs(before[2]).max(), "the changed head must change the samples"
    ref = K.reference(t.state_dict(), cat, an, DRAW, 7)
    for s in range(7):
        assert_close(after[2][s], ref[s], 1e-5, f"after load_weights, sample {s} vs transfer_ref")
