"""Regression metrics on the GPU: impnn_regression_sums against train.regression_sums_reference on the same float32
arrays, and compile(metrics=...) through evaluate, fit (captured and eager steps), the transfer model's loss node and
model.error_table.  Cases and bounds: tests/metrics_ref.py - per word (n_s + 4) 2^-52 sum |term|, words 0 and 7 exact."""
import numpy as np
import pytest
import torch

from ionic_mpnn_amd import data, ops, synthetic, train
from conftest import ROOT

import metrics_ref as MR
from test_gpu_transfer import make_transfer, stage2

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE, OFFSET = MR.SCALE, MR.OFFSET


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sums(pred, y, w=None, order=None, off=None, **kw):
    return ops.regression_sums(_dev(pred), _dev(y), _dev(w), order=_dev(order), seg_offsets=_dev(off), offset=OFFSET,
                               scale=SCALE, **kw)


# =====================================================================================================================
# Kernel level
# =====================================================================================================================
@pytest.mark.parametrize("n", MR.ONE_SEGMENT_N + (MR.LARGE_N,))
def test_one_segment(n):
    """One segment at every size at which the launcher takes another path (one wave up to 64, a workgroup of 256 up to
    16 384, one of 1 024 above), with and without weights, with and without ``order``; two calls give the same bits;
    an overwriting call does not see what the record held."""
    pred, y, w = MR.arrays(n, n)
    perm = np.random.default_rng(n).permutation(n).astype(np.int32)
    for sw in (None, w):
        ref = train.regression_sums_reference(pred, y, sw, offset=OFFSET, scale=SCALE)
        for order in (None, perm):
            got = _sums(pred, y, sw, order)
            again = _sums(pred, y, sw, order, out=torch.full((1, 8), 123.0, dtype=torch.float64, device=DEV))
            assert torch.equal(got, again), "the same call, the same bits"
            MR.check_record(got.cpu().numpy(), ref, pred, y, sw, [np.arange(n) if order is None else perm], SCALE,
                            OFFSET, f"n={n} weights={sw is not None} order={order is not None}")


@pytest.mark.parametrize("n", [65, 4097])
def test_accumulate_three_calls_equal_one_on_the_concatenation(n):
    pred, y, w = MR.arrays(n, n + 1)
    cuts = [0, n // 3, n // 3, n]   # the second call is empty: it launches nothing and adds nothing
    for sw in (None, w):
        out = torch.zeros(1, 8, dtype=torch.float64, device=DEV)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            r = ops.regression_sums(_dev(pred[lo:hi]), _dev(y[lo:hi]), None if sw is None else _dev(sw[lo:hi]),
                                    offset=OFFSET, scale=SCALE, out=out, accumulate=True)
            assert r is out
        one = _sums(pred, y, sw)
        ref = train.regression_sums_reference(pred, y, sw, offset=OFFSET, scale=SCALE)
        for got in (out, one):
            MR.check_record(got.cpu().numpy(), ref, pred, y, sw, [np.arange(n)], SCALE, OFFSET, f"accumulate n={n}")
    with pytest.raises(ValueError):
        ops.regression_sums(_dev(pred), _dev(y), accumulate=True)


def _segment_reference(pred, y, w, segments):
    return np.concatenate([train.regression_sums_reference(pred[i], y[i], None if w is None else w[i], offset=OFFSET,
                                                           scale=SCALE) for i in segments])


@pytest.mark.parametrize("lengths", [MR.drawn_lengths(), list(MR.LONG_SEGMENTS)], ids=["wave_per_segment", "workgroup_per_segment"])
def test_segments_under_a_permutation(lengths):
    """37 segments of lengths from {0, 1, 2, 63, 64, 65, 300, 1500} (a wave each), and three long ones (a workgroup
    each), under a random permutation as ``order``; with ``accumulate`` a second call doubles the sums and keeps the
    maximum; one NaN prediction makes words 2, 3, 4 and 7 of its segment NaN and leaves the neighbours alone."""
    order, off, segments = MR.segmented_case(lengths, len(lengths))
    n = int(off[-1])
    assert (n // len(lengths) > 512) == (len(lengths) == 3)
    pred, y, w = MR.arrays(n, 11)
    for sw in (None, w):
        ref = _segment_reference(pred, y, sw, segments)
        got = _sums(pred, y, sw, order, off)
        assert torch.equal(got, _sums(pred, y, sw, order, off)), "the same call, the same bits"
        MR.check_record(got.cpu().numpy(), ref, pred, y, sw, segments, SCALE, OFFSET, "segmented")
        twice = _sums(pred, y, sw, order, off, out=got.clone(), accumulate=True).cpu().numpy()
        assert np.array_equal(twice[:, :7], 2 * got.cpu().numpy()[:, :7]) and np.array_equal(twice[:, 7], ref[:, 7])
    s_nan = int(np.argmax(np.asarray(lengths) == 300)) if 300 in lengths else 0
    bad = int(segments[s_nan][len(segments[s_nan]) // 2])
    pred[bad], w[bad] = np.nan, 1.0
    got = _sums(pred, y, w, order, off).cpu().numpy()
    ref = _segment_reference(pred, y, w, segments)
    assert np.isnan(got[s_nan, [2, 3, 4, 7]]).all() and np.isfinite(got[s_nan, [0, 1, 5, 6]]).all()
    assert np.isfinite(np.delete(got, s_nan, axis=0)).all()
    MR.check_record(got, ref, pred, y, w, segments, SCALE, OFFSET, "segmented, one NaN")


def test_wrapper_validation():
    pred, y, w = (_dev(a) for a in MR.arrays(10, 0))
    with pytest.raises(RuntimeError):
        ops.regression_sums(pred.cpu(), y)
    with pytest.raises(TypeError):
        ops.regression_sums(pred.double(), y)
    with pytest.raises(ValueError):
        ops.regression_sums(pred, y[:5])
    with pytest.raises(TypeError):
        ops.regression_sums(pred, y, order=torch.arange(10, device=DEV))   # int64
    with pytest.raises(TypeError):
        ops.regression_sums(pred, y, out=torch.zeros(2, 8, dtype=torch.float64, device=DEV))
    with pytest.raises(Exception, match="scale"):
        ops.regression_sums(pred, y, scale=0.0)
    empty = ops.regression_sums(pred[:0], y[:0], out=torch.ones(1, 8, dtype=torch.float64, device=DEV))
    assert float(empty.abs().sum()) == 0.0


# =====================================================================================================================
# Model level: the tiny viscosity model, 70 samples in batches of 24 (two captured steps, one eager step of 22)
# =====================================================================================================================
N, BS = MR.N_SAMPLES, MR.BATCH
WEIGHTS = data.bootstrap_weights(N, 0)
METRICS = ["mae", "mse", "rmse", "bias", "max_error", "r2"]


def _expected(model, x, y, w=None, scale=1.0, offset=0.0, names=METRICS):
    """{name: (value, tolerance)} from the reference on model.predict."""
    pred = model.predict(x, batch_size=BS).reshape(-1)
    rec = train.regression_sums_reference(pred, y, w, offset=offset, scale=scale)[0]
    tol = MR.metric_tolerances(pred, y, w, scale, offset)
    return {k: (type(train.get_metric(k))(scale=scale, offset=offset).result(rec), tol[k]) for k in names}


def test_evaluate_against_predict():
    m, x, y = MR.tiny_viscosity()
    m.compile(train.Adam(1e-3, clipnorm=1.0))
    plain = m.evaluate(x, y, batch_size=BS)
    plain_w = m.evaluate(x, y, batch_size=BS, sample_weight=WEIGHTS)
    assert isinstance(plain, float) and m.evaluate(x, y, batch_size=BS, return_dict=True) == {"loss": plain}
    kelvin = [train.MeanAbsoluteError("mae_k", SCALE, OFFSET), train.R2Score("r2_k", scale=SCALE, offset=OFFSET)]
    m.compile(train.Adam(1e-3, clipnorm=1.0), metrics=METRICS + kelvin, weighted_metrics=["mae", "r2"])
    for sw, base in ((None, plain), (WEIGHTS, plain_w)):
        d = m.evaluate(x, y, batch_size=BS, sample_weight=sw, return_dict=True)
        assert d["loss"] == base, "the loss is computed exactly as without metrics"
        assert list(d) == ["loss"] + METRICS + ["mae_k", "r2_k", "weighted_mae", "weighted_r2"]
        assert m.evaluate(x, y, batch_size=BS, sample_weight=sw) == list(d.values())
        want = _expected(m, x, y)
        want.update({k + "_k": v for k, v in _expected(m, x, y, None, SCALE, OFFSET, ["mae", "r2"]).items()})
        want.update({"weighted_" + k: v for k, v in _expected(m, x, y, sw, names=["mae", "r2"]).items()})
        for k, (v, tol) in want.items():
            print(f"{k}: evaluate {d[k]!r} reference {v!r} tolerance {tol:.2e}")
            assert abs(d[k] - v) <= tol, (k, d[k], v, tol)


def _fixed_weights_fit(graph, w=None):
    m, x, y = MR.tiny_viscosity()
    m.compile(train.Adam(0.0), metrics=["mae", "r2"], weighted_metrics=["mae"])
    h = m.fit(x, y, epochs=2, batch_size=BS, seed=3, graph=graph, sample_weight=w)
    return m, x, y, h.history


@pytest.fixture(scope="module")
def fixed_fits():
    return {(g, wt): _fixed_weights_fit(g, WEIGHTS if wt else None) for g in (True, False) for wt in (True, False)}


@pytest.mark.parametrize("weighted", [False, True])
def test_fit_running_metrics_with_fixed_weights(fixed_fits, weighted):
    """Adam(0.0): the weights stay, dropout is 0, so every epoch's running metrics - added up inside the captured step
    from the TRAINING pass's predictions (layered encoder) and in the eager step of the ragged batch - are the metrics
    of predict (fused encoder): 1e-5 relative, the forward parity of the two encoders.  Captured against eager: 1e-4."""
    w = WEIGHTS if weighted else None
    m, x, y, hg = fixed_fits[(True, weighted)]
    _, _, _, he = fixed_fits[(False, weighted)]
    assert sorted(hg) == ["loss", "mae", "r2", "weighted_mae"]
    want = _expected(m, x, y, names=["mae", "r2"])
    want["weighted_mae"] = _expected(m, x, y, w, names=["mae"])["mae"]
    for k, (v, _) in want.items():
        for epoch in range(2):
            print(f"{k} epoch {epoch}: graph {hg[k][epoch]!r} eager {he[k][epoch]!r} predict {v!r}")
            assert abs(hg[k][epoch] - v) <= 1e-5 * abs(v) and abs(he[k][epoch] - v) <= 1e-5 * abs(v)
            assert abs(hg[k][epoch] - he[k][epoch]) <= 1e-4 * abs(he[k][epoch])
    if not weighted:
        assert hg["weighted_mae"] == hg["mae"], "without sample_weight a weighted metric has w = 1"


def test_fit_validation_metrics_and_early_stopping_on_r2():
    m, x, y = MR.tiny_viscosity()
    xv, yv = MR.tiny_set(seed=9, n=30)
    m.compile(train.Adam(1e-3, clipnorm=1.0), metrics=["mae", "r2"])

    class Probe(train.Callback):
        def __init__(self):
            super().__init__()
            self.seen, self.states = [], []

        def on_epoch_end(self, epoch, logs=None):
            self.seen.append((dict(logs), self.model.evaluate(xv, yv, batch_size=4096, return_dict=True)))
            self.states.append(self.model.state_dict())

    probe = Probe()
    es = train.EarlyStopping(monitor="val_r2", patience=10, restore_best_weights=True)
    h = m.fit(x, y, validation_data=(xv, yv), epochs=3, batch_size=BS, seed=0, callbacks=[probe, es]).history
    assert sorted(h) == ["loss", "mae", "r2", "val_loss", "val_mae", "val_r2"] and len(h["val_r2"]) == 3
    for logs, sep in probe.seen:
        assert {k: logs["val_" + k] for k in sep} == sep, "val_<name> is evaluate() at the end of the epoch"
    best = int(np.argmax(h["val_r2"]))
    assert es.mode == "max" and es.best_epoch == best and es.best == h["val_r2"][best]
    now = m.state_dict()
    assert all(np.array_equal(now[k], probe.states[best][k]) for k in now), "the epoch of the largest val_r2 is restored"


def test_a_model_without_metrics_builds_the_step_it_always_built():
    m, x, y = MR.tiny_viscosity()
    m.compile(train.Adam(1e-3, clipnorm=1.0))
    h = m.fit(x, y, epochs=1, batch_size=BS, seed=0)
    assert sorted(h.history) == ["loss"] and m._metric_set is None
    assert getattr(m, "_metric_pred_buf", None) is None, "no prediction buffer: the loss kernels got the null pointer"
    g = train.GraphedTrainStep(m, {k: v[:BS] for k, v in x.items()}, y[:BS])
    assert g.metrics is None


def test_fit_without_metrics_is_the_parent_run_bit_for_bit():
    """tests/golden/metrics_parent_fit.npz (tests/golden/make_metrics_golden.py, recorded on the commit before metrics
    existed): loss history and final weights of tests/metrics_ref.py::parent_fit - captured and eager steps, with and
    without sample weights - bit for bit.

    The recorded runs are at learning rate 0 because only such a run has bits to compare.  At rate 1e-3 the parent
    commit does not repeat ITSELF: twelve runs of this fit on that commit (two processes, three captured and three
    eager runs each) gave twelve different sets of final weights (max |dw| 3.0e-8 to 6.0e-8) and loss histories that
    part at the 8th digit (13.08903294 / 4.40266113 / 3.53896276 against 13.08903309 / 4.40266150 / 3.53896324) - the
    backward's float atomics add in an order that changes from run to run - and this commit's runs scatter among
    them in the same way.  At rate 0 every launch of the step still runs, the weights stay, and the losses are the
    forward and loss kernels' fixed-order sums; the recipe made each run three times with equal bits before writing."""
    z = np.load(ROOT / "tests" / "golden" / MR.GOLDEN)
    for tag, graph, weighted in MR.PARENT_RUNS:
        loss, w = MR.parent_fit(graph, weighted)
        print(f"{tag}: loss {loss.tolist()} recorded {z[tag + '/loss'].tolist()}")
        assert np.array_equal(loss, z[f"{tag}/loss"]), (tag, loss, z[f"{tag}/loss"])
        assert sorted(f"{tag}/w/{k}" for k in w) == sorted(k for k in z.files if k.startswith(tag + "/w/"))
        assert all(np.array_equal(w[k], z[f"{tag}/w/{k}"]) for k in w), tag
    assert len(set(z["graph_plain/loss"].tolist())) == 3, "three shuffles, three different sums"
    assert not np.array_equal(z["graph_plain/loss"], z["graph_weighted/loss"])


def test_transfer_model_metrics_in_kelvin_from_the_training_pass(tmp_path):
    """The transfer model, Huber, BatchNormalization on the batch statistics: the loss node writes the training pass's
    predictions into the model's buffer (an eager step, so they can be read back) and the record in kelvin equals the
    reference on exactly those predictions."""
    t = make_transfer(tmp_path, S=1)
    stage2(t)
    mets = [train.MeanAbsoluteError(scale=SCALE, offset=OFFSET), train.R2Score(scale=SCALE, offset=OFFSET)]
    t.compile(train.Adam(1e-3), loss=train.Huber(delta=1.0), metrics=mets, weighted_metrics=mets)
    B = 24
    x = synthetic.make_batch(B, seed=4)
    y = np.random.default_rng(4).normal(0.0, 1.0, size=B).astype(np.float32)
    w = data.bootstrap_weights(B, 1)
    ms = t._metric_set
    assert ms.keys == ["mae", "r2", "weighted_mae", "weighted_r2"] and len(ms.records) == 2
    rec = ms.buffer("train", t.device).zero_()
    inference = t.predict(x).reshape(-1)
    loss = t.train_on_batch(x, y, sample_weight=w, metric_slot="train")
    pred = t._metric_pred(B).cpu().numpy().copy()
    assert np.isfinite(float(loss)) and np.isfinite(pred).all()
    assert np.max(np.abs(pred - inference)) > 1e-3, "batch statistics: not the inference predictions"
    got = rec.cpu().numpy()
    for i, sw in enumerate((None, w)):
        ref = train.regression_sums_reference(pred, y, sw, offset=OFFSET, scale=SCALE)
        MR.check_record(got[i:i + 1], ref, pred, y, sw, [np.arange(B)], SCALE, OFFSET, f"transfer record {i}")
    out = ms.results(got)
    assert abs(out["mae"] - train.MeanAbsoluteError(scale=SCALE, offset=OFFSET).result(
        train.regression_sums_reference(pred, y, offset=OFFSET, scale=SCALE))) <= MR.metric_tolerances(
            pred, y, None, SCALE, OFFSET)["mae"]
    # and through fit: one captured step of 24 and an eager one of 8
    x2 = synthetic.make_batch(32, seed=6)
    y2 = np.random.default_rng(6).normal(0.0, 1.0, size=32).astype(np.float32)
    h = t.fit(x2, y2, epochs=2, batch_size=B, seed=0).history
    assert sorted(h) == ["loss", "mae", "r2", "weighted_mae", "weighted_r2"]
    assert all(np.isfinite(v).all() for v in h.values()) and h["mae"][0] > 1.0, "kelvin, not standardised units"


def test_error_table_on_the_device_against_the_host_reference():
    m, x, y = MR.tiny_viscosity()
    rng = np.random.default_rng(2)
    groups = np.concatenate([[999], 100 + rng.permutation(np.arange(69) % 10)]) * 3   # 11 groups, one of one sample
    assert len(np.unique(groups)) == 11
    pred = m.predict(x, batch_size=BS).reshape(-1)
    for sw in (None, WEIGHTS):
        ref = data.error_table(pred, y, groups, sw, scale=SCALE, offset=OFFSET)
        tab = m.error_table(x, y, groups, sample_weight=sw, batch_size=BS, scale=SCALE, offset=OFFSET)
        assert isinstance(tab, data.ErrorTable) and np.array_equal(tab.group, np.unique(groups))
        assert np.array_equal(tab.count, ref.count) and tab.count[-1] == 1 and np.array_equal(tab.max_error, ref.max_error)
        for g in range(11):   # a group of n_g samples: (n_g + 8) 2^-52 relative to the sum of the terms' magnitudes
            rel = (tab.count[g] + 8) * MR.EPS
            assert abs(tab.weight[g] - ref.weight[g]) <= rel * ref.weight[g]
            assert abs(tab.mae[g] - ref.mae[g]) <= rel * ref.mae[g] and abs(tab.rmse[g] - ref.rmse[g]) <= rel * ref.rmse[g]
            assert abs(tab.bias[g] - ref.bias[g]) <= rel * ref.mae[g]
        assert np.array_equal(tab.worst(3).group, ref.worst(3).group)
