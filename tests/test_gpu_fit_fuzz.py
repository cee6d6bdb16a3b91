"""Fit fuzz: whole ``MPNNModel.fit`` runs against the independent fp64 trainer of tests/fit_ref.py, one per row of
tests/fit_cases.py, graph mode and cache flag.  Every other multi-step test compares the library with itself; here the
other side shares no code with it, so the batch order and cut, the eager remainder between replays, the epoch loss, the
running metrics, the step a schedule sees, the mask a replay draws, the moving statistics and the optimizer state are
all held against a restatement of fit's documented contract.

Exact: history keys and length (the early stop included), optimizer.iterations, the dropout counter, frozen tensors bit
for bit, the next rate within the schedule bound of tests/test_gpu_lr_schedule.py.  Bounded (fit_cases.BOUNDS, 8 x the
float32 reference trainer's own distance from the fp64 one, tests/test_fit_ref_host.py): every logged value, the
displacement of every trainable tensor, Adam's moments, the moving statistics.  DESIGN.md 2 "Fit fuzz" has the table."""
import numpy as np
import pytest

from ionic_mpnn_amd import layers as L, model as MM, train, weights
from conftest import assert_close

import fit_cases as FC
import fit_ref as FR
import optimizer_ref as OR

pytestmark = pytest.mark.gpu
DEV = "cuda"
RUNS = [pytest.param(c.name, graph, cache, id=f"{c.name}-{'graph' if graph else 'eager'}" + "".join(f"-{k}" for k in cache))
        for c in FC.CASES for cache in c.caches for graph in c.graphs]


def build(case, tmp_path):
    """The row's model with its initial variables, as the existing tests build theirs."""
    d = case.dims
    rate, seed = case.dropout if case.dropout is not None else (0.0, None)
    w = FC.case_weights(case)
    L.reset_uids()
    if case.kind == "melting_point":
        assert d["K"] == d["D"] ** 2
        m = MM.build_melting_point_model(d["Va"], d["Vb"], atom_dim=d["D"], fp_size=d["F"], mixing_size=d["Mx"],
                                         num_steps=d["S"], device=DEV, dropout_rate=rate, dropout_seed=seed)
    else:
        m = MM.build_model(d["Va"], d["Vb"], atom_dim=d["D"], bond_dim=d["K"], fp_size=d["F"], mixing_size=d["Mx"],
                           num_steps=d["S"], device=DEV, dropout_rate=rate, dropout_seed=seed)
    if case.kind == "transfer":   # tests/test_gpu_transfer.py::make_transfer: the saved viscosity model, cut, with the head
        m.load_weights(weights.init_weights("viscosity", d["Va"], d["Vb"], atom_dim=d["D"], bond_dim=d["K"],
                                            fp_size=d["F"], mixing_size=d["Mx"], num_steps=d["S"],
                                            seed=case.weight_seed, perturb=True))
        path = tmp_path / "viscosity_final.keras"
        m.save(str(path))
        m = MM.build_transfer_model(str(path), device=DEV, dropout_seed=case.head_dropout_seed)
    assert set(m.state_dict()) == set(w)
    m.load_weights(w)
    for layer in m.layers:
        layer.trainable = FC.layer_trainable(case, layer.name, d["S"])
    return m


def schedule(spec):
    kind = spec["kind"]
    if kind == "constant":
        return spec["lr"]
    if kind == "exponential":
        return train.ExponentialDecay(spec["lr0"], spec["decay_steps"], spec["decay_rate"], staircase=spec["staircase"])
    if kind == "cosine":
        return train.CosineDecay(spec["lr0"], spec["decay_steps"], alpha=spec["alpha"],
                                 warmup_target=spec["warmup_target"], warmup_steps=spec["warmup_steps"])
    return train.PiecewiseConstantDecay(list(spec["boundaries"]), list(spec["values"]))


def compiled(case, tmp_path):
    m = build(case, tmp_path)
    o = case.opt
    opt = train.Adam(schedule(o["lr"]), clipnorm=o.get("clipnorm"), global_clipnorm=o.get("global_clipnorm"),
                     weight_decay=o.get("weight_decay"))
    if o.get("exclude"):
        opt.exclude_from_weight_decay(list(o["exclude"]))
    metric = lambda spec: train.METRICS[spec[0]](scale=spec[1], offset=spec[2])
    m.compile(opt, loss="mse" if case.loss[0] == "mse" else train.Huber(case.loss[1]),
              metrics=[metric(s) for s in case.metrics] or None,
              weighted_metrics=[metric(s) for s in case.weighted_metrics] or None)
    return m


def next_rate(case, ref):
    """(the rate the step after the run would use, its bound: 8 x the float32 restatement's error on the run's steps)."""
    if case.epoch_rate is not None:
        lr0, factor = case.epoch_rate
        last = lr0 * factor ** (len(ref["history"]["loss"]) - 1)
        return last, 8.0 * OR.f32_error(FC.CONSTANT(last), [0])
    spec = case.opt["lr"]
    return float(OR.schedule_rate(spec, ref["iterations"])), 8.0 * OR.f32_error(spec, range(ref["iterations"] + 2))


@pytest.mark.parametrize("name,graph,cache", RUNS)
def test_fit_follows_the_independent_trainer(tmp_path, name, graph, cache):
    case = FC.BY_NAME[name]
    ref = FC.reference(case)
    x, y, sw, val = FC.case_data(case)
    m = compiled(case, tmp_path)
    initial = m.state_dict()
    assert {n for n, _ in m.trainable_variables()} == set(ref["trainable"]), "the row's freezing pattern"
    callbacks = []
    if case.epoch_rate is not None:
        lr0, factor = case.epoch_rate
        callbacks.append(train.LearningRateScheduler(lambda epoch, lr: lr0 * factor ** epoch))
    if case.early_stop is not None:
        callbacks.append(train.EarlyStopping("val_loss", patience=case.early_stop["patience"], restore_best_weights=True))
    validation = None if val is None else tuple(v for v in val if v is not None)
    h = m.fit(x, y, validation_data=validation, epochs=case.epochs, batch_size=case.batch, callbacks=callbacks,
              shuffle=case.shuffle, seed=case.seed, graph=graph, sample_weight=sw, **cache)
    # ---- exact
    assert list(h.history) == list(ref["history"])
    assert {k: len(v) for k, v in h.history.items()} == {k: len(v) for k, v in ref["history"].items()}
    assert m.optimizer.iterations == ref["iterations"]
    counter = m.dropout_counter()
    if case.dropout is not None or case.kind == "transfer":
        assert int(counter.item()) == ref["dropout_steps"] == ref["iterations"]
    else:
        assert counter is None
    state = m.state_dict()
    trained = [n for n, _ in m.trainable_variables()]
    for n, a in initial.items():
        if n not in trained and n not in FR.MOVING:
            assert np.array_equal(state[n], a), f"frozen {n} changed"
    rate, bound = next_rate(case, ref)
    got_rate = m.optimizer.current_learning_rate()
    assert abs(got_rate - rate) <= bound * abs(rate), f"next rate {got_rate!r} against {rate!r} (bound {bound:.2e})"
    # ---- bounded
    sizes = [int(t.numel()) for _, t in m.trainable_variables()]
    cuts = np.cumsum([0] + sizes)
    flat_m, flat_v = m.optimizer.m.cpu().numpy(), m.optimizer.v.cpu().numpy()
    got = dict(history=h.history, weights=state, moving={k: state[k] for k in ref["moving"]},
               m={n: flat_m[cuts[i]:cuts[i + 1]].reshape(state[n].shape) for i, n in enumerate(trained)},
               v={n: flat_v[cuts[i]:cuts[i + 1]].reshape(state[n].shape) for i, n in enumerate(trained)})
    d = FC.distances(got, ref)
    print(f"\nFITFUZZ {name} graph={int(graph)} cache={'+'.join(cache) or '-'} "
          + " ".join(f"{k}={v / FC.BOUNDS[k]:.3f}" for k, (v, _) in d.items())
          + " | " + " ; ".join(f"{k} at {w}" for k, (_, w) in d.items()))
    for k in ref["history"]:
        print(f"  {k}: got {[f'{v:.7g}' for v in h.history[k]]} ref {[f'{v:.7g}' for v in ref['history'][k]]}")
    FC.check(case, got, ref, what=f"graph={graph} {cache}")
    for n in trained:
        assert_close(got["m"][n], ref["m"][n], FC.MOMENT_BOUND, f"{name}: m of {n}", floor=FC.FLOOR)
        assert_close(got["v"][n], ref["v"][n], FC.MOMENT_BOUND, f"{name}: v of {n}", floor=FC.FLOOR)
