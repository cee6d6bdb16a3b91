"""The reference trainer of the fit fuzz on the CPU (tests/fit_ref.py, tests/fit_cases.py; the GPU side is
tests/test_gpu_fit_fuzz.py):

  * consistency: an epoch of fit_ref in fp64 is tests/optimizer_ref.py's ``adam_update`` applied to its own gradients,
    its first gradients are grad_ref's / transfer_ref's, an epoch's metrics are data.error_table's and the metric
    classes' on the collected predictions;
  * the conditions on every row's inputs;
  * attainability: fit_ref in fp32 passes the GPU test's checks at one eighth of each bound;
  * the reference is alive: every option a row turns on and every knock-out it lists moves the fp64 run by at least
    ten times a bound."""
import dataclasses

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import data, train

import fit_cases as FC
import fit_ref as FR
import grad_ref as GR
import optimizer_ref as OR
import transfer_ref as R
from weighted_ref import weighted_batch_mean

NAMES = [c.name for c in FC.CASES]


def _scale_close(a, e, what, tol=1e-12):
    a, e = np.asarray(a, np.float64), np.asarray(e, np.float64)
    scale = max(float(np.abs(e).max()), 1e-300)
    assert float(np.abs(a - e).max()) <= tol * scale, f"{what}: {np.abs(a - e).max():.3e} of scale {scale:.3e}"


def test_table_and_bounds():
    assert len(set(NAMES)) == len(NAMES)
    assert FC.LOSS_BOUND <= FC.LOSS_CAP and FC.DISPLACEMENT_BOUND <= FC.DISPLACEMENT_CAP
    for c in FC.CASES:
        assert c.batch == 16 and set(c.knocks) <= set(FR.KNOCKOUTS), c.name
    by = FC.BY_NAME
    assert by["plain"].n == 50 and by["plain"].n % 16 == 2 and by["remainder-1"].n % 16 == 1
    assert by["no-remainder"].n % 16 == 0 and by["no-graph"].n < 16
    # every knock-out has a row that must notice it
    assert {k for c in FC.CASES for k in c.knocks} == set(FR.KNOCKOUTS)


def test_fit_ref_uses_nothing_of_the_library_under_test():
    """fit_ref and every test module that loading it loads import none of model, train, ops, autograd (fit_cases takes
    ``synthetic`` and ``weights`` from the package, as the other reference modules do)."""
    import ast
    import pathlib
    here = pathlib.Path(FR.__file__).parent
    seen, todo, banned = set(), ["fit_ref", "fit_cases"], []   # (fit_ref loads fit_cases inside run)
    while todo:
        mod = todo.pop()
        if mod in seen:
            continue
        seen.add(mod)
        path = here / (mod + ".py") if "." not in mod else here.parent / (mod.replace(".", "/") + ".py")
        for node in ast.parse(path.read_text()).body:   # what loading the module loads
            names = []
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                names = [f"{node.module}.{a.name}" for a in node.names] + [node.module]
            for n in names:
                if n.startswith("ionic_mpnn_amd") and n.split(".")[-1] in ("model", "train", "ops", "autograd"):
                    banned.append((mod, n))
                if (here / (n + ".py")).exists() or (n.startswith("oracle.") and (here.parent / (n.replace(".", "/") + ".py")).exists()):
                    todo.append(n)
    assert {"philox_ref", "grad_ref", "head_ref", "transfer_ref", "optimizer_ref", "fit_cases"} <= seen
    assert not banned, banned


def test_weighted_batch_mean_is_weighted_refs():
    rng = np.random.default_rng(3)
    per, w = torch.tensor(rng.normal(size=17)), rng.uniform(0, 2, size=17)
    assert float(FR.weighted_batch_mean(per, w)) == float(weighted_batch_mean(per, torch.tensor(w)))


@pytest.mark.parametrize("name", NAMES)
def test_an_epoch_is_the_optimizer_reference_on_its_own_gradients(name):
    case = FC.BY_NAME[name]
    steps = []
    got = FR.run(case, torch.float64, max_epochs=1, collect=steps)
    assert got["iterations"] == len(steps) == case.steps_per_epoch
    names = got["trainable"]
    w0 = FC.case_weights(case)
    ws = [np.asarray(w0[n], np.float64) for n in names]
    ms, vs = [np.zeros_like(w) for w in ws], [np.zeros_like(w) for w in ws]
    opt = case.opt
    decays = [not any(s in n for s in opt.get("exclude", ())) for n in names]
    for t, st in enumerate(steps, 1):
        assert st["t"] == t
        lr = case.epoch_rate[0] if case.epoch_rate is not None else OR.schedule_rate(opt["lr"], t - 1)
        assert st["lr"] == float(lr)
        ws, ms, vs = OR.adam_update(ws, [st["grads"][n] for n in names], ms, vs, t, float(lr),
                                    clipnorm=opt.get("clipnorm"), global_clipnorm=opt.get("global_clipnorm"),
                                    weight_decay=opt.get("weight_decay"), decays=decays)
    for n, w, m, v in zip(names, ws, ms, vs):
        _scale_close(got["weights"][n], w, f"{name}: {n}")
        _scale_close(got["m"][n], m, f"{name}: m of {n}")
        _scale_close(got["v"][n], v, f"{name}: v of {n}")
    for n in w0:
        if n not in names and n not in FR.MOVING:
            assert np.array_equal(got["weights"][n], np.asarray(w0[n], np.float64)), f"{name}: frozen {n} moved"


@pytest.mark.parametrize("name", [c.name for c in FC.CASES if c.dropout is None])
def test_the_first_gradients_are_the_gradient_references(name):
    """Step 1 of the run against grad_ref.model_loss (viscosity / melting point, plain MSE) or transfer_ref's head
    on its pooled vectors, weighted where the row is.  The rows with GatedUpdate dropout are not here: the masked
    GatedUpdate has no second restatement (tests/test_gpu_dropout.py holds the same composition against the kernels)."""
    case = FC.BY_NAME[name]
    steps = []
    FR.run(dataclasses.replace(case, epochs=1), torch.float64, collect=steps)
    st = steps[0]
    x, y, sw, _ = FC.case_data(case)
    xb = {k: v[st["rows"]] for k, v in x.items()}
    w0 = FC.case_weights(case)
    w = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in w0.items()
         if k not in FR.MOVING}
    if case.kind == "transfer":
        mask = FR.reference_mask(case.head_dropout_seed, 0, R.HEAD_LAYER_ID, 0.3, len(st["rows"]), 128)
        full = dict(w, **{k: torch.tensor(np.asarray(w0[k]), dtype=torch.float64) for k in FR.MOVING})
        pc, pa = R.pooled(full, xb)
        pred, _, _ = R.head(full, pc, pa, True, mask)
        e = pred - torch.tensor(y[st["rows"]], dtype=torch.float64)
        per = R.huber(e, case.loss[1]) if case.loss[0] == "huber" else e * e
        data_term = per.mean() if sw is None else weighted_batch_mean(per, torch.tensor(sw[st["rows"]], dtype=torch.float64))
        loss = data_term + case.fp_l2 * ((w["cat_fp/kernel"] ** 2).sum() + (w["an_fp/kernel"] ** 2).sum())
    elif case.loss[0] == "mse" and sw is None:
        loss = GR.model_loss(case.kind, w, xb, y[st["rows"]], case.fp_l2)
    else:
        pred = GR.viscosity_forward(w, xb).reshape(-1)
        e = pred - torch.tensor(y[st["rows"]], dtype=torch.float64)
        per = R.huber(e, case.loss[1]) if case.loss[0] == "huber" else e * e
        data_term = per.mean() if sw is None else weighted_batch_mean(per, torch.tensor(sw[st["rows"]], dtype=torch.float64))
        loss = data_term + case.fp_l2 * ((w["cat_fp/kernel"] ** 2).sum() + (w["an_fp/kernel"] ** 2).sum())
    _scale_close(st["loss"], float(loss), f"{name}: loss", 1e-12)
    loss.backward()
    for n, g in st["grads"].items():
        want = w[n].grad if w[n].grad is not None else torch.zeros_like(w[n])
        _scale_close(g, want.numpy(), f"{name}: gradient of {n}", 1e-10)


@pytest.mark.parametrize("name", ["remainder-1", "weighted-huber", "transfer-stage1"])
def test_an_epochs_metrics_are_the_error_table_and_the_metric_classes(name):
    case = FC.BY_NAME[name]
    steps = []
    got = FR.run(case, torch.float64, max_epochs=1, collect=steps)
    _, y, sw, _ = FC.case_data(case)
    rows = np.concatenate([st["rows"] for st in steps])
    pred = np.concatenate([st["pred"] for st in steps]).astype(np.float32)   # (the record is defined on float32)
    assert sorted(rows) == list(range(case.n))
    for specs, weights, prefix in ((case.metrics, None, ""), (case.weighted_metrics, sw[rows], "weighted_")):
        mine = FR.metric_values(specs, pred, y[rows], weights, prefix)
        for key, scale, offset in specs:
            rec = train.regression_sums_reference(pred, y[rows], weights, None, offset, scale)[0]
            want = train.get_metric(key).__class__(scale=scale, offset=offset).result(rec)
            _scale_close(mine[prefix + key], want, f"{name}: {prefix + key}", 1e-12)
            if key in ("bias", "mae", "rmse", "max_error"):
                table = data.error_table(pred, y[rows], np.zeros(case.n, np.int64), weights, scale, offset)
                _scale_close(mine[prefix + key], getattr(table, key)[0], f"{name}: error_table {key}", 1e-12)
            # the run's own log is the same value up to the float32 cast of the predictions
            assert abs(got["history"][prefix + key][0] - mine[prefix + key]) <= 1e-6 * max(abs(mine[prefix + key]), 1e-30) \
                or key in ("bias", "r2"), (name, key)
    tot = sum(len(st["rows"]) * st["loss"] for st in steps) / case.n
    assert got["history"]["loss"][0] == pytest.approx(tot, rel=1e-15)


# ------------------------------------------------------------------------------------------------ conditions on the inputs
@pytest.mark.parametrize("name", NAMES)
def test_input_conditions(name):
    case = FC.BY_NAME[name]
    ref = FC.reference(case)
    x, y, sw, val = FC.case_data(case)
    steps = ref["steps"]
    assert ref["iterations"] == len(steps)
    kept = total = 0
    floor = lambda n: 0.5 if n == "mp_dense_1/bias" and case.bn_trains else 0.85   # (fit_cases.reference says why)
    for n in ref["trainable"]:
        keep = ref["compared"][n]
        d = (ref["weights"][n] - ref["initial"][n])[keep]
        assert keep.any() and np.abs(d).max() > 0.0, f"{name}: {n} has no compared displacement"
        assert keep.mean() >= floor(n), f"{name}: only {keep.mean():.2f} of {n} is compared"
        kept, total = kept + int(keep.sum()), total + keep.size
    assert kept >= 0.98 * total, f"{name}: only {kept} of {total} elements are compared"
    if "global_clip" in case.options:   # low enough to clip every step
        assert all(ref["clipped"]), name
    if case.weighted:
        order = np.random.default_rng(case.seed).permutation(case.n) if case.shuffle else np.arange(case.n)
        assert sw[order[min(case.batch, case.n) - 1]] == 0.0 and (sw > 0).sum() > case.n // 2
    if case.early_stop is not None:
        v = ref["history"]["val_loss"]
        assert ref["stopped_epoch"] is not None and len(v) < case.epochs, "the row is to stop early"
        for a, b in zip(v, v[1:]):
            assert abs(a - b) >= 100 * FC.LOSS_BOUND * max(abs(a), abs(b)), (name, v)
    if case.loss[0] == "huber":
        e = np.concatenate([st["e"] for st in steps])
        r = np.abs(e) / case.loss[1]
        assert (r < 1).any() and (r > 1).any(), f"{name}: both of Huber's branches are to occur"
        assert np.abs(r - 1).min() > FC.LOSS_BOUND, f"{name}: an |e| within the bound of Huber's kink"
    for s, st in enumerate(steps):   # no relu pre-activation within the loss bound (of the layer's scale) of its kink
        for layer, z in st["trace"].items():
            if layer in ("vp", "sp_b", "sp_c", "melting_point"):
                continue
            margin = np.abs(z).min() / np.abs(z).max()
            assert margin > FC.LOSS_BOUND, f"{name}: step {s + 1}, a pre-activation of {layer} within {margin:.1e} of 0"


# ---------------------------------------------------------------------------------------------------------- attainability
def _float32(case):
    return FC._cached(("float32", repr(case)), lambda: FR.run(case, torch.float32))


@pytest.mark.parametrize("name", NAMES)
def test_float32_reference_meets_an_eighth_of_every_bound(name):
    case = FC.BY_NAME[name]
    ref = FC.reference(case)
    got = _float32(case)
    assert got["iterations"] == ref["iterations"] and got["stopped_epoch"] == ref["stopped_epoch"]
    d = FC.distances(got, ref)
    print(f"\n{name}: " + " | ".join(f"{k} {v:.2e} ({w})" for k, (v, w) in d.items()))
    FC.check(case, got, ref, fraction=1.0 / 8, what="float32 reference")


def test_bounds_cover_eight_times_the_largest_float32_distance():
    """Each class bound is 8 x the largest float32-against-float64 distance over the rows, rounded up: at least that
    product and less than twice it (another BLAS or thread count moves the float32 runs by a few percent), and
    within its cap."""
    worst = {k: max(FC.distances(_float32(c), FC.reference(c))[k][0] for c in FC.CASES) for k in FC.BOUNDS}
    for k, bound in FC.BOUNDS.items():
        assert 8 * worst[k] <= bound < 16 * worst[k], f"{k}: 8 x {worst[k]:.3e} against the table's {bound:g}"
    assert FC.LOSS_BOUND <= FC.LOSS_CAP and FC.DISPLACEMENT_BOUND <= FC.DISPLACEMENT_CAP


# --------------------------------------------------------------------------------------------------- the reference is alive
def _moved(case, other):
    """The largest distance of ``other`` from the row's reference in units of the class bounds."""
    ref = FC.reference(case)
    return max(v / FC.BOUNDS[k] for k, (v, _) in FC.distances(other, ref).items())


ALIVE = [(c.name, "off:" + o) for c in FC.CASES for o in c.options] + [(c.name, k) for c in FC.CASES for k in c.knocks]


@pytest.mark.parametrize("name,knock", ALIVE)
def test_the_reference_notices(name, knock):
    case = FC.BY_NAME[name]
    other = FR.run(case, torch.float64, knock=knock)
    if knock == "off:frozen":   # (more variables train: compare what the row trains, and see the frozen ones move)
        ref = FC.reference(case)
        frozen = [n for n in ref["initial"] if n not in ref["trainable"] and n not in FR.MOVING]
        assert any(not np.array_equal(other["weights"][n], ref["initial"][n]) for n in frozen)
    moved = _moved(case, other)
    assert moved >= 10.0, f"{name}: {knock} moves the run by {moved:.2f} bounds only - the row does not test it"
