"""Per-sample weights on the CPU: (1) attainability - every kernel-level case of tests/test_gpu_sample_weight.py, the
weighted reference (tests/weighted_ref.py) in fp32 against itself in fp64 under the very checks the GPU test applies to
the kernels, on exactly its inputs and weights; (2) no relu pre-activation, clipped softplus value or Huber |e| of the
fp64 reference within a relative 1e-4 of its kink, for every case (none is skipped); (3) the cases cover the batches,
widths, settings and weight patterns they are meant for; (4) train.mse / train.Huber with weights are the formula and
without them the bits they were; (5) data.balanced_weights / data.bootstrap_weights; (6) bad weights are a ValueError
before any library call, and what the C entries can see (null, alignment) is a status code."""
import ctypes as C

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, autograd, data, model as MM, synthetic, train

import test_gpu_head_fuzz as FZ
import weighted_ref as WR

F32, F64 = torch.float32, torch.float64
HEAD_CASES, TH_CASES = WR.model_head_cases(), WR.transfer_cases()
_BAD, _UNS = -1, -2


def ids(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------------------- (1) (2) attainability
@pytest.mark.parametrize("wc", HEAD_CASES, ids=ids(HEAD_CASES))
def test_f32_attains_the_weighted_model_head_bounds(wc):
    inp = FZ.model_head_inputs(wc.base)
    sw = WR.case_weights(wc)
    ref64, ref32 = WR.model_head_reference(wc, inp, sw, F64), WR.model_head_reference(wc, inp, sw, F32)
    WR.model_head_kinks(wc, ref64)
    WR.check_model_head(wc, ref32, ref64)


@pytest.mark.parametrize("wc", TH_CASES, ids=ids(TH_CASES))
def test_f32_attains_the_weighted_transfer_head_bounds(wc):
    inp = FZ.transfer_inputs(wc.base)
    sw = WR.case_weights(wc)
    ref64, ref32 = WR.transfer_reference(wc, inp, sw, F64), WR.transfer_reference(wc, inp, sw, F32)
    WR.transfer_kinks(wc, ref64)
    WR.check_transfer(wc, ref32, ref64)


# ------------------------------------------------------------------------------------------------- (3) coverage
def test_cases_cover_batches_widths_settings_and_patterns():
    for kind in (0, 1):
        k = [c for c in HEAD_CASES if c.base.kind == kind]
        small = [c for c in k if (c.base.D, c.base.F, c.base.Mx) == (8, 5, 3)]
        assert {c.base.B for c in small} == {1, 7, 8, 9, 2049, 4097}
        assert any((c.base.D, c.base.F, c.base.Mx) == (64, 33, 64) and c.base.lanes == 2 for c in k)
        assert {c.base.loss_sum for c in k} == {"first is last", "one stride", "second stride"}
        assert {c.base.passes for c in k} == {1, 2}
        for B in (1, 7, 8, 9, 2049, 4097):
            assert {c.pattern for c in small if c.base.B == B} == set(WR.patterns_for(B))
    th = TH_CASES
    for s, bn, loss in WR.TH_SETTINGS:
        k = [c for c in th if c.base.bn == bn and c.base.loss == loss]
        assert {c.base.B for c in k if (c.base.D, c.base.F, c.base.Mx) == (8, 5, 3)} == {1, 7, 8, 9, 2049, 4097}, s
        assert any((c.base.D, c.base.F, c.base.Mx) == (64, 33, 64) for c in k), s
        assert {c.pattern for c in k} == set(WR.PATTERNS), s
    assert {c.base.loss[0] for c in th} == {"mse", "huber"} and {c.base.bn for c in th} == {0, 1}
    assert any(c.base.rate > 0 and c.base.bn for c in th), "a Dropout mask beside the weights"
    assert WR.patterns_for(1) == ["fractional", "counts", "zero last"] and WR.patterns_for(8) == ["fractional", "counts"]
    assert WR.patterns_for(9) == list(WR.PATTERNS) == WR.patterns_for(2049) == WR.patterns_for(4097)


@pytest.mark.parametrize("B", [1, 7, 8, 9, 2049, 4097])
def test_weight_patterns_are_what_they_are_named(B):
    spb = WR.SPB
    for p in WR.patterns_for(B):
        w = WR.sample_weights(p, B, 0)
        assert w.dtype == np.float32 and w.shape == (B,) and np.isfinite(w).all() and (w >= 0).all()
        assert np.array_equal(w, WR.sample_weights(p, B, 0))
        if p == "fractional":
            assert (w > 0).all() and (B < 4 or (w != np.round(w)).any())
        elif p == "counts":
            assert np.array_equal(w, np.round(w)) and w.max() <= 3 and w.any() and (B < 64 or set(w) == {0, 1, 2, 3})
        elif p == "zero workgroup":
            zero = [g for g in range(-(-B // spb)) if not w[g * spb:(g + 1) * spb].any()]
            assert len(zero) == 1 and len(w[zero[0] * spb:(zero[0] + 1) * spb]) == spb and np.count_nonzero(w) == B - spb
        else:
            assert B % spb and w[B - 1] == 0 and np.count_nonzero(w) == B - 1


# ------------------------------------------------------------------------------------------------- (4) train.mse / Huber
def test_weighted_mse_and_huber_are_the_formula_and_none_keeps_the_bits():
    rng = np.random.default_rng(3)
    B = 37
    y = torch.tensor(rng.normal(1.0, 0.5, (B, 1)), dtype=F32)
    pred = torch.tensor(rng.normal(1.0, 1.5, (B, 1)), dtype=F32)
    w = rng.uniform(0.0, 3.0, B).astype(np.float32)
    w[5] = 0.0
    e = pred.double().reshape(-1) - y.double().reshape(-1)
    want_mse = float((torch.tensor(w, dtype=F64) * e * e).sum() / B)
    assert abs(float(train.mse(y, pred, w)) - want_mse) <= 1e-6 * want_mse
    assert abs(float(train.mse(y, pred, torch.tensor(w))) - want_mse) <= 1e-6 * want_mse
    for delta in (0.25, 1.0):
        hub = train.Huber(delta)
        a = e.abs()
        per = torch.where(a <= delta, 0.5 * e * e, delta * (a - 0.5 * delta))
        assert (a <= delta).any() and (a > delta).any()
        want = float((torch.tensor(w, dtype=F64) * per).sum() / B)
        assert abs(float(hub(y, pred, w)) - want) <= 1e-6 * want
        assert abs(float(hub(y, pred, sample_weight=w)) - float(hub(y, pred)) * 1.0) > 1e-3 * want   # (weights matter)
        # no weights: the tensor bits of the unweighted form, as it was
        old = torch.mean(torch.where((pred - y).abs() <= delta, 0.5 * (pred - y) * (pred - y),
                                     delta * ((pred - y).abs() - 0.5 * delta)))
        assert torch.equal(hub(y, pred), old) and torch.equal(hub(y, pred, None), old)
    old = torch.mean((pred.reshape(B, -1) - y.reshape(B, -1)) ** 2)
    assert torch.equal(train.mse(y, pred), old) and torch.equal(train.mse(y, pred, None), old)
    # B counts the samples of weight 0: zeroing a weight does not renormalise the others
    w2 = w.copy()
    w2[7] = 0.0
    drop = float(w[7] * e[7] * e[7] / B)
    assert abs(float(train.mse(y, pred, w)) - float(train.mse(y, pred, w2)) - drop) <= 1e-5 * want_mse
    # gradients reach the prediction, none is asked of the weight
    p = pred.clone().requires_grad_(True)
    train.mse(y, p, w).backward()
    want_g = (2.0 * torch.tensor(w, dtype=F64) * e / B).reshape(B, 1)
    assert float((p.grad.double() - want_g).abs().max()) <= 1e-6 * float(want_g.abs().max())
    with pytest.raises(ValueError):
        train.mse(y, pred, w[:-1])


# ------------------------------------------------------------------------------------------------- (5) data helpers
def test_balanced_weights_give_every_group_the_same_total_and_mean_one():
    rng = np.random.default_rng(0)
    groups = np.concatenate([np.full(40, 7), np.full(1, 3), rng.integers(10, 25, 200)])
    rng.shuffle(groups)
    w = data.balanced_weights(groups)
    assert w.dtype == np.float32 and w.shape == groups.shape
    totals = [float(w[groups == g].astype(np.float64).sum()) for g in np.unique(groups)]
    assert np.allclose(totals, len(groups) / len(totals), rtol=1e-6)
    assert abs(float(w.astype(np.float64).mean()) - 1.0) <= 1e-6
    assert np.allclose(w[groups == 7], len(groups) / (len(totals) * 40.0)) and np.allclose(w[groups == 3], len(groups) / len(totals))
    assert np.allclose(data.balanced_weights(["a", "b", "a", "c"]), [2 / 3, 4 / 3, 2 / 3, 4 / 3])
    with pytest.raises(ValueError):
        data.balanced_weights([])


def test_bootstrap_weights_are_counts_that_reproduce_from_the_seed():
    n = 500
    w = data.bootstrap_weights(n, 11)
    assert w.dtype == np.float32 and w.shape == (n,) and float(w.sum()) == n
    assert np.array_equal(w, np.round(w)) and (w >= 0).all() and (w == 0).any() and (w > 1).any()
    assert abs(float((w == 0).mean()) - np.exp(-1.0)) < 0.08, "about 1/e of a bootstrap sample is left out"
    assert np.array_equal(w, data.bootstrap_weights(n, 11)) and not np.array_equal(w, data.bootstrap_weights(n, 12))
    groups = np.random.default_rng(1).integers(0, 60, n)
    wg = data.bootstrap_weights(n, 11, groups)
    assert wg.dtype == np.float32 and wg.shape == (n,) and np.array_equal(wg, np.round(wg))
    for g in np.unique(groups):
        assert len(set(wg[groups == g])) == 1, "all samples of a group carry the group's count"
    per_group = np.array([wg[groups == g][0] for g in np.unique(groups)])
    assert per_group.sum() == len(per_group) and (per_group == 0).any()
    assert np.array_equal(wg, data.bootstrap_weights(n, 11, groups))
    assert not np.array_equal(wg, data.bootstrap_weights(n, 12, groups))
    for bad in (dict(n=0, seed=1), dict(n=5, seed=1, groups=[1, 2])):
        with pytest.raises(ValueError):
            data.bootstrap_weights(**bad)


# ------------------------------------------------------------------------------------------------- (6) refusals
BAD_WEIGHTS = {"negative": lambda n: np.r_[np.ones(n - 1), -0.5], "nan": lambda n: np.r_[np.ones(n - 1), np.nan],
               "inf": lambda n: np.r_[np.inf, np.ones(n - 1)], "short": lambda n: np.ones(n - 1),
               "long": lambda n: np.ones(n + 1), "matrix": lambda n: np.ones((2, n))}


@pytest.mark.parametrize("what", sorted(BAD_WEIGHTS))
def test_bad_weights_raise_before_any_library_call(what, monkeypatch):
    n = 6
    bad = BAD_WEIGHTS[what](n).astype(np.float32)
    with pytest.raises(ValueError):
        train.checked_sample_weight(bad, n)
    with pytest.raises(ValueError):
        train.checked_sample_weight(torch.tensor(bad), n)
    m = MM.build_model(11, 6, atom_dim=8, bond_dim=4, fp_size=6, mixing_size=5, num_steps=1, device=torch.device("cpu"))
    m.compile(train.Adam(1e-3, clipnorm=1.0))
    x = synthetic.make_batch(n, max_atoms=6, max_edges=8, atom_vocab_size=11, bond_vocab_size=6, min_atoms=2, seed=1)
    y = np.zeros(n, np.float32)

    def no_library():
        raise AssertionError("the library was reached before the weights were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    with pytest.raises(ValueError):
        m.fit(x, y, sample_weight=bad, graph=False)
    with pytest.raises(ValueError):
        m.fit(x, y, validation_data=(x, y, bad), graph=False)
    with pytest.raises(ValueError):
        m.evaluate(x, y, sample_weight=bad)
    with pytest.raises(ValueError):
        m.train_on_batch(x, y, sample_weight=bad)
    with pytest.raises(ValueError):
        m.train_on_batch(x, y, bad)


def test_good_weights_come_back_as_float32():
    w = train.checked_sample_weight([0, 1, 2.5], 3)
    assert w.dtype == torch.float32 and w.tolist() == [0.0, 1.0, 2.5]
    assert train.checked_sample_weight(None, 3) is None
    assert train.checked_sample_weight(np.arange(4).reshape(4, 1), 4).shape == (4,)
    l2 = autograd.WeightedL2([0.1, 0.0], w)
    assert tuple(l2) == (0.1, 0.0) and l2.sample_weight is w and len(l2) == 2


def test_weighted_entries_status_codes():
    """What the C side can see of a weight: null is the unweighted call (it goes on to the widths), a misaligned pointer
    is IMPNN_E_BADARG behind the null pointers; the other rules answer in the weighted entry's name.  Every call returns
    before any device call: the pointers are addresses inside a host buffer that nothing dereferences."""
    lib = _lib.load()
    host = (C.c_char * 1024)()
    at = C.addressof(host)
    p = lambda i: at + 16 * (i + 1)
    table = C.cast((C.c_void_p * 18)(*[p(20 + i) for i in range(18)]), _lib.PP)
    lam = (C.c_float * 18)()

    def head(entry, sw, y=p(4), D=32, kind=0):
        if entry.endswith("_bwd"):
            rc = getattr(lib, entry)(kind, p(0), p(1), p(2), table, lam, y, sw, p(5), p(6), p(7), table, 9, D, 32, 20, None)
        else:
            rc = getattr(lib, entry)(kind, p(0), p(1), p(2), table, lam, y, sw, None, p(5), p(6), 1 << 40, 9, D, 32, 20, None)
        return rc, lib.impnn_last_error_string()

    def transfer(entry, sw, y=p(4), D=32):
        if entry.endswith("_bwd"):
            rc = getattr(lib, entry)(p(0), p(1), table, table, lam, 1, y, sw, 1, 1.0, p(5), 0.0, 0, None, 0, p(6), 1 << 40,
                                     p(7), 1 << 40, p(8), p(9), 9, D, 32, 20, None)
        else:
            rc = getattr(lib, entry)(p(0), p(1), table, lam, p(2), p(3), 0.99, 1e-3, 1, y, sw, 1, 1.0, 0.0, 0, None, 0,
                                     p(6), 1 << 40, None, p(7), p(8), 1 << 40, 9, D, 32, 20, None)
        return rc, lib.impnn_last_error_string()

    for call, entries in ((head, ("impnn_weighted_model_head_loss", "impnn_weighted_model_head_loss_bwd")),
                          (transfer, ("impnn_weighted_transfer_head_loss", "impnn_weighted_transfer_head_loss_bwd"))):
        for entry in entries:
            assert entry in _lib.SIGNATURES
            short = entry.encode()
            for sw in (None, p(10)):   # null: valid, the unweighted loss; both go on to the widths
                rc, msg = call(entry, sw, D=129)
                assert rc == _UNS and b"D=129" in msg, (entry, sw, msg)
            for off in (1, 2, 3):
                rc, msg = call(entry, p(10) + off)
                assert rc == _BAD and msg == short + b": sample_weight must be 4-byte aligned", (entry, off, msg)
            rc, msg = call(entry, p(10) + 2, y=None)   # the null pointers come first
            assert rc == _BAD and msg == short + b": null pointer", (entry, msg)
    assert lib.impnn_abi_version() == 3   # additions only
