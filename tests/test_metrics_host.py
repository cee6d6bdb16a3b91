"""CPU: the regression metrics' host side - train.regression_sums_reference and every metric's result against plain
numpy, data.error_table against a per-group loop, compile(metrics=...) validation and config round trips, the
monitoring callbacks' ``mode``, the status codes of impnn_regression_sums in their documented order (host addresses
that nothing dereferences), and dist.all_reduce_metric_sums_ in a world of 2 under gloo.  Cases: tests/metrics_ref.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT
from ionic_mpnn_amd import _lib, data, model as MM, train
from oracle import mpnn_oracle as O

import metrics_ref as MR
from test_dist_cpu import _free_port

F64 = np.float64
NAMES = ("mae", "mse", "rmse", "bias", "max_error", "r2")


def _plain(pred, y, w, scale, offset, eps=1e-6):
    """The metrics straight from their formulas in numpy fp64 (no record in between)."""
    p, t = pred.astype(F64), y.astype(F64)
    w = np.ones_like(p) if w is None else w.astype(F64)
    e, yr, sw = scale * (p - t), offset + scale * t, w.sum()
    if sw == 0.0:
        return dict(mae=0.0, mse=0.0, rmse=0.0, bias=0.0, max_error=0.0, r2=0.0)
    mean_y = (w * yr).sum() / sw
    live = np.abs(e)[w > 0]
    return dict(mae=(w * np.abs(e)).sum() / sw, mse=(w * e * e).sum() / sw, rmse=np.sqrt((w * e * e).sum() / sw),
                bias=(w * e).sum() / sw, max_error=live.max() if live.size else 0.0,
                r2=1.0 - (w * e * e).sum() / ((w * (yr - mean_y) ** 2).sum() + eps))


CASES = [(n, seed, weights, scale, offset)
         for n, seed, weights, scale, offset in [
             (1, 0, "none", 1.0, 0.0), (2, 1, "poisson", 1.0, 0.0), (17, 2, "none", MR.SCALE, MR.OFFSET),
             (64, 3, "poisson", MR.SCALE, MR.OFFSET), (65, 4, "none", 1.0, 0.0), (300, 5, "poisson", 2.0, -1.0),
             (300, 6, "zero", 1.0, 0.0), (1000, 7, "poisson", MR.SCALE, MR.OFFSET), (1000, 8, "none", -3.0, 5.0),
             (33, 9, "zero", MR.SCALE, MR.OFFSET), (4097, 10, "poisson", 1.0, 0.0), (70, 11, "none", 1.0, 0.0)]]


@pytest.mark.parametrize("n,seed,weights,scale,offset", CASES)
def test_reference_and_metric_results_against_plain_numpy(n, seed, weights, scale, offset):
    """The record's words are the sums they are named after, and every metric's result(record) is its formula.  The
    record sums and the plain sums add the same fp64 terms in numpy's one order, so the means agree to a few ulp; R^2 is
    formed from sum yr^2 - (sum yr)^2 / sum w instead of the centred sum, which cancels: bounded by 8 eps (sum w yr^2) /
    denominator on top of the quotient's own rounding."""
    pred, y, w = MR.arrays(n, seed)
    w = None if weights == "none" else np.zeros_like(w) if weights == "zero" else w
    rec = train.regression_sums_reference(pred, y, w, offset=offset, scale=scale)
    assert rec.shape == (1, 8) and rec.dtype == F64
    ww = np.ones(n) if w is None else w.astype(F64)
    e, yr = scale * (pred.astype(F64) - y.astype(F64)), offset + scale * y.astype(F64)
    want = [n, ww.sum(), (ww * e).sum(), (ww * np.abs(e)).sum(), (ww * (e * e)).sum(), (ww * yr).sum(),
            (ww * (yr * yr)).sum(), np.abs(e)[ww > 0].max() if (ww > 0).any() else 0.0]
    assert np.array_equal(rec[0], np.array(want, F64))
    ref = _plain(pred, y, w, scale, offset)
    for name in NAMES:
        m = train.get_metric(name)
        m = type(m)(scale=scale, offset=offset)
        got = m.result(rec[0])
        assert isinstance(got, float)
        if name == "r2" and ww.sum() > 0:
            ss_tot = (ww * (yr - (ww * yr).sum() / ww.sum()) ** 2).sum() + 1e-6
            tol = (8 * MR.EPS * (ww * yr * yr).sum() / ss_tot + 16 * MR.EPS) * max(1.0, abs(1.0 - ref[name]))
            assert abs(got - ref[name]) <= tol, (name, got, ref[name], tol)
        else:
            assert abs(got - ref[name]) <= 8 * MR.EPS * abs(ref[name]), (name, got, ref[name])
    if weights == "zero":
        assert all(train.get_metric(k).result(rec) == 0.0 for k in NAMES), "a weight sum of 0 gives 0 (divide_no_nan)"


def test_one_nan_prediction():
    pred, y, w = MR.arrays(50, 3, nan_at=7)
    groups = np.arange(50) // 10
    rec = train.regression_sums_reference(pred, y, w, groups=groups)
    assert np.isnan(rec[0, [2, 3, 4, 7]]).all() and np.isfinite(rec[0, [0, 1, 5, 6]]).all()
    assert np.isfinite(rec[1:]).all(), "the neighbours are untouched"
    assert np.isnan(train.MaxError().result(rec[0])) and np.isnan(train.MeanAbsoluteError().result(rec[0]))
    w[7] = 0.0   # a NaN of weight 0: not in the maximum, but 0 * NaN is NaN in the sums
    rec = train.regression_sums_reference(pred, y, w, groups=groups)
    assert np.isfinite(rec[0, 7]) and np.isnan(rec[0, 2])


@pytest.mark.parametrize("seed", range(4))
def test_r2_is_the_reference_formula_on_unit_weights(seed):
    """R2Score() against oracle.mpnn_oracle.r2_numpy (the reference's own, with its + 1e-6).  Same numerator terms; the
    denominator is sum y^2 - (sum y)^2 / n against the centred sum: off by at most ~4 eps sum y^2, relative to ss_tot."""
    pred, y, _ = MR.arrays(200, seed)
    rec = train.regression_sums_reference(pred, y)
    want = O.r2_numpy(y.astype(F64), pred.astype(F64))
    ss_tot = ((y.astype(F64) - y.astype(F64).mean()) ** 2).sum()
    tol = (8 * MR.EPS * (y.astype(F64) ** 2).sum() / ss_tot + 32 * MR.EPS) * max(1.0, abs(1.0 - want))
    assert abs(train.R2Score().result(rec) - want) <= tol
    assert train.R2Score().epsilon == 1e-6


def test_error_table_against_a_loop_over_the_groups():
    rng = np.random.default_rng(0)
    pred, y, w = MR.arrays(70, 1)
    groups = rng.integers(100, 111, size=70) * 7
    groups[0] = 5   # a group of one sample
    for sw in (None, w):
        tab = data.error_table(pred, y, groups, sw, scale=MR.SCALE, offset=MR.OFFSET)
        ids = np.unique(groups)
        assert np.array_equal(tab.group, ids) and tab.count.dtype == np.int64 and tab.count[0] == 1
        for g, gid in enumerate(ids):
            sel = groups == gid
            ref = _plain(pred[sel], y[sel], None if sw is None else sw[sel], MR.SCALE, MR.OFFSET)
            ws = float(sel.sum()) if sw is None else float(sw[sel].astype(F64).sum())
            assert tab.count[g] == sel.sum() and abs(tab.weight[g] - ws) <= 8 * MR.EPS * ws
            for name in ("bias", "mae", "rmse", "max_error"):
                assert abs(getattr(tab, name)[g] - ref[name]) <= 16 * MR.EPS * abs(ref[name]), (gid, name)


def test_worst_is_a_stable_descending_order():
    tab = data.ErrorTable(np.array([10, 11, 12, 13, 14]), np.ones(5, np.int64), np.ones(5),
                          np.array([0.1, -0.9, 0.2, 0.0, 0.3]), np.array([2.0, 1.0, 2.0, np.nan, 2.0]),
                          np.array([1.0, 2.0, 3.0, 4.0, 5.0]), np.array([5.0, 4.0, 3.0, 2.0, 1.0]))
    assert tab.worst(4).group.tolist() == [13, 10, 12, 14], "a NaN first, equal values in the table's order"
    assert tab.worst(2, by="bias").group.tolist() == [11, 14] and tab.worst(1, by="bias").bias.tolist() == [-0.9]
    assert tab.worst(99, by="rmse").group.tolist() == [14, 13, 12, 11, 10] and len(tab.worst(0).group) == 0
    assert tab.worst(2, by="max_error").max_error.tolist() == [5.0, 4.0]
    with pytest.raises(ValueError):
        tab.worst(1, by="count")


def _cpu_model():
    return MM.build_model(11, 6, atom_dim=8, bond_dim=4, fp_size=6, mixing_size=5, num_steps=1, device=torch.device("cpu"))


def test_compile_validation_and_configs():
    m = _cpu_model()
    m.compile(train.Adam(1e-3))
    opt = m.optimizer
    assert m._metric_set is None
    with pytest.raises(ValueError, match="unknown metric"):
        m.compile(train.Adam(1e-3), metrics=["mae", "accuracy"])
    assert m.optimizer is opt and m._metric_set is None, "an unknown name raises before anything is touched"
    with pytest.raises(ValueError, match="unknown metric"):
        m.compile(weighted_metrics=[3.0])
    four = [train.MeanAbsoluteError(name=f"mae{i}", scale=1.0 + i) for i in range(4)]
    m.compile(train.Adam(1e-3), metrics=four + ["r2"], weighted_metrics=["mae"])
    ms = m._metric_set
    assert ms.keys == ["mae0", "mae1", "mae2", "mae3", "r2", "weighted_mae"]
    assert len(ms.records) == 5, "four (scale, offset) records, and the weighted twin of (1, 0)"
    with pytest.raises(ValueError, match="at most 4"):
        m.compile(metrics=four + [train.R2Score(scale=9.0)])
    with pytest.raises(ValueError, match="at most 4"):
        m.compile(metrics=four, weighted_metrics=[train.MeanError(offset=1.0)])
    with pytest.raises(ValueError, match="logged as"):
        m.compile(metrics=["mae", train.MeanAbsoluteError(scale=2.0)])
    with pytest.raises(ValueError):
        train.MeanSquaredError(scale=0.0)
    with pytest.raises(ValueError):
        train.MeanSquaredError(offset=float("inf"))
    m.compile(metrics="mae")
    assert m._metric_set.keys == ["mae"]
    for name, cls in train.METRICS.items():
        a = cls(name="x_" + name, scale=MR.SCALE, offset=MR.OFFSET)
        b = cls.from_config(a.get_config())
        assert type(b) is cls and b.get_config() == a.get_config() and b.name == "x_" + name
        assert train.get_metric(name).name == name and (cls().scale, cls().offset) == (1.0, 0.0)
    assert train.R2Score.from_config(train.R2Score(epsilon=1e-3).get_config()).epsilon == 1e-3
    rec = train.regression_sums_reference(*MR.arrays(20, 0)[:2])
    out = train.MetricSet(["mae", "r2"], ["rmse"]).results(np.concatenate([rec, rec]), prefix="val_")
    assert list(out) == ["val_mae", "val_r2", "val_weighted_rmse"]


class _Fake:
    def __init__(self):
        self.w, self.stop_training = 0, False
        self.optimizer = train.Adam(1e-2)

    def state_dict(self):
        return {"w": self.w}

    def load_weights(self, d):
        self.w = d["w"]


def _run(cb, key, values):
    m = _Fake()
    cb.set_model(m)
    cb.on_train_begin()
    stopped = None
    for epoch, v in enumerate(values):
        m.w = epoch
        cb.on_epoch_end(epoch, {key: v})
        if m.stop_training:
            stopped = epoch
            break
    cb.on_train_end()
    return m, stopped


def test_callback_modes():
    # "max" stops on a falling R^2 and restores the epoch of the largest value
    es = train.EarlyStopping(monitor="val_r2", patience=2, restore_best_weights=True, mode="max")
    m, stopped = _run(es, "val_r2", [0.1, 0.6, 0.5, 0.4, 0.9])
    assert stopped == 3 and es.best == 0.6 and es.best_epoch == 1 and m.w == 1
    # "min" on the sequence of tests/test_dist_cpu.py: the outcome that test pins
    es = train.EarlyStopping(monitor="val_loss", patience=2, restore_best_weights=True, mode="min")
    m, stopped = _run(es, "val_loss", [3.0, 2.0, 2.5, 2.2, 1.9, 5.0])
    assert stopped == 3 and es.best == 2.0 and m.w == 1
    # "auto" resolves by the monitor's name
    assert train.EarlyStopping(monitor="val_r2").mode == "max" and train.EarlyStopping(monitor="r2").mode == "max"
    assert train.EarlyStopping().mode == "min" and train.EarlyStopping(monitor="val_mae").mode == "min"
    assert train.ReduceLROnPlateau(monitor="val_weighted_r2").mode == "max" and train.ReduceLROnPlateau().mode == "min"
    assert train.EarlyStopping(monitor="val_r2", mode="min").mode == "min"
    assert train.EarlyStopping().best == np.inf and train.EarlyStopping(monitor="val_r2").best == -np.inf
    for cls in (train.EarlyStopping, train.ReduceLROnPlateau):
        with pytest.raises(ValueError):
            cls(mode="up")
    # ReduceLROnPlateau: "max" cuts the rate where R^2 stalls, "min" where a loss does
    rl = train.ReduceLROnPlateau(monitor="val_r2", factor=0.5, patience=2, min_delta=0.0)
    m, _ = _run(rl, "val_r2", [0.1, 0.5, 0.4, 0.3, 0.6])
    assert [e for e, _ in rl.rates] == [3] and rl.best == 0.6 and m.optimizer.learning_rate == 5e-3
    rl = train.ReduceLROnPlateau(monitor="val_loss", factor=0.5, patience=2, min_delta=0.0, mode="min")
    m, _ = _run(rl, "val_loss", [3.0, 2.0, 2.5, 2.2, 1.9])
    assert [e for e, _ in rl.rates] == [3] and rl.best == 1.9


def test_c_entry_status_codes_in_order():
    lib = _lib.load()
    assert lib.impnn_regression_sums_words() == 8 == train.RECORD_WORDS
    buf = (C.c_double * 64)()
    a = C.addressof(buf)   # 8-byte aligned host memory; no call below gets far enough to read it
    p, y, w, s = a, a + 64, a + 128, a + 256
    ok = dict(pred=p, y=y, w=w, order=None, off=None, n=5, n_seg=1, offset=0.0, scale=1.0, acc=0, sums=s)

    def call(**kw):
        k = dict(ok, **kw)
        rc = lib.impnn_regression_sums(k["pred"], k["y"], k["w"], k["order"], k["off"], k["n"], k["n_seg"], k["offset"],
                                       k["scale"], k["acc"], k["sums"], None)
        return rc, lib.impnn_last_error_string()

    # every rule alone, and ahead of the ones after it
    later = dict(scale=0.0)
    for bad, word in ((dict(n=-1), b"n must"), (dict(n_seg=0), b"n_seg"), (dict(pred=None), b"null"),
                      (dict(y=None), b"null"), (dict(sums=None), b"null"), (dict(n_seg=3, off=None), b"seg_offsets"),
                      (dict(pred=p + 2), b"aligned"), (dict(w=w + 1), b"aligned"), (dict(order=a + 2), b"aligned"),
                      (dict(n_seg=2, off=a + 4), b"8-byte"), (dict(sums=s + 4), b"8-byte")):
        for extra in ({}, later):
            rc, text = call(**dict(extra, **bad))
            assert rc == -1 and word in text and b"impnn_regression_sums" in text, (bad, text)
    assert call(n=-1, n_seg=0, pred=None)[1].count(b"n must") == 1, "n < 0 comes first"
    assert b"n_seg" in call(n_seg=0, pred=None)[1] and b"null" in call(pred=None, n_seg=2)[1]
    assert b"seg_offsets" in call(n_seg=2, pred=p + 2)[1] and b"aligned" in call(pred=p + 2, scale=0.0)[1]
    for bad in (dict(scale=0.0), dict(scale=float("inf")), dict(scale=float("nan")), dict(offset=float("nan")),
                dict(offset=float("-inf"))):
        rc, text = call(**bad)
        assert rc == -1 and (b"scale" in text or b"offset" in text), (bad, text)
        assert call(n=0, **bad)[0] == -1, "the checks come before the n == 0 success"
    assert call(n=0, pred=None)[0] == -1
    # n == 0 with one segment is a success that launches nothing under accumulate
    assert call(n=0, acc=1)[0] == 0


def _metric_worker(rank, world, port, n_rows, out_dir):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ.update({"RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": str(world),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    from pathlib import Path
    from ionic_mpnn_amd import dist as idist, train as T
    import metrics_ref as R
    idist.init_distributed(backend="gloo")
    for nan_at in (None, 0):
        pred, y, w = R.arrays(n_rows, 4, nan_at=nan_at)
        lo, hi = idist.shard_bounds(n_rows, world, rank)
        local = np.concatenate([T.regression_sums_reference(pred[lo:hi], y[lo:hi], sw[lo:hi] if sw is not None else None,
                                                            offset=R.OFFSET, scale=R.SCALE) for sw in (None, w)])
        full = np.concatenate([T.regression_sums_reference(pred, y, sw, offset=R.OFFSET, scale=R.SCALE)
                               for sw in (None, w)])
        rec = torch.from_numpy(local.copy())
        out = idist.all_reduce_metric_sums_(rec)
        assert out is rec and rec.shape == (2, 8)
        got = rec.numpy()
        assert np.array_equal(got[:, [0, 7]], full[:, [0, 7]], equal_nan=True), (got, full)
        assert np.array_equal(np.isnan(got), np.isnan(full))
        for r, sw in enumerate((None, w)):   # two partial sums against one sum of the same terms
            with np.errstate(invalid="ignore"):
                bound = (n_rows + 4) * R.EPS * R.term_abs_sums(pred, y, sw, np.arange(n_rows), R.SCALE, R.OFFSET)
            for k in range(1, 7):
                assert np.isnan(full[r, k]) or abs(got[r, k] - full[r, k]) <= bound[k - 1], (r, k, got, full)
    Path(out_dir, f"mok_{rank}").write_text("ok")
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("n_rows", [8, 7, 1])         # even, uneven, and a rank with an empty shard
def test_world2_gloo_metric_sums(tmp_path, n_rows):
    world, port = 2, _free_port()
    mp.spawn(_metric_worker, args=(world, port, n_rows, str(tmp_path)), nprocs=world, join=True)
    assert all((tmp_path / f"mok_{r}").exists() for r in range(world))
    rec = torch.arange(16.0, dtype=torch.float64).reshape(2, 8)
    assert torch.equal(__import__("ionic_mpnn_amd.dist", fromlist=["x"]).all_reduce_metric_sums_(rec.clone()), rec)
