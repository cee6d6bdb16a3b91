"""Learning-rate schedules, the rate-setting callbacks and the new Adam arguments on the host (no GPU): the schedules'
float64 ``__call__`` against hand-computed values and against tests/optimizer_ref.py, config round trips, the device
record's words, ReduceLROnPlateau against its rule on scripted monitors, LearningRateScheduler's call order, argument
errors, and the pin of today's ``get_config``."""
import math

import numpy as np
import pytest

from ionic_mpnn_amd import train

import optimizer_ref as OR


# ---------------------------------------------------------------------------------------------------------------------
# Schedules
# ---------------------------------------------------------------------------------------------------------------------
def test_exponential_decay_values():
    e = train.ExponentialDecay(1e-2, decay_steps=4, decay_rate=0.5)
    assert e(0) == 1e-2
    assert e(4) == pytest.approx(5e-3, rel=1e-15)            # decay_steps
    assert e(2) == pytest.approx(1e-2 * math.sqrt(0.5), rel=1e-15)
    assert e(12) == pytest.approx(1e-2 / 8, rel=1e-15)       # beyond decay_steps
    st = train.ExponentialDecay(1e-2, decay_steps=4, decay_rate=0.5, staircase=True)
    assert [st(s) for s in (0, 3, 4, 7, 8)] == pytest.approx([1e-2, 1e-2, 5e-3, 5e-3, 2.5e-3], rel=1e-15)


def test_cosine_decay_values():
    c = train.CosineDecay(1e-2, decay_steps=10, alpha=0.1)
    assert c(0) == pytest.approx(1e-2, rel=1e-15)
    assert c(5) == pytest.approx(1e-2 * (0.9 * 0.5 + 0.1), rel=1e-14)     # cos(pi / 2) = 0
    assert c(10) == pytest.approx(1e-3, rel=1e-14)                         # decay_steps: alpha * lr0
    assert c(11) == c(10) == c(10 ** 6)                                    # beyond decay_steps
    w = train.CosineDecay(1e-3, decay_steps=10, alpha=0.0, warmup_target=1e-2, warmup_steps=4)
    assert [w(s) for s in (0, 1, 2, 3)] == pytest.approx([1e-3, 3.25e-3, 5.5e-3, 7.75e-3], rel=1e-14)   # the warm-up
    assert w(4) == pytest.approx(1e-2, rel=1e-15)                          # its end: the cosine starts at the target
    assert w(9) == pytest.approx(1e-2 * 0.5, rel=1e-14)                    # half-way
    assert w(14) == pytest.approx(0.0, abs=1e-18) and w(15) == w(14)
    # warmup_steps without a target: keras ignores them
    assert train.CosineDecay(1e-2, 10, warmup_steps=4)(2) == train.CosineDecay(1e-2, 10)(2)


def test_piecewise_constant_values():
    p = train.PiecewiseConstantDecay([3, 6], [1e-2, 1e-3, 1e-4])
    assert [p(s) for s in (0, 3, 4, 6, 7, 10 ** 6)] == [1e-2, 1e-2, 1e-3, 1e-3, 1e-4, 1e-4]
    assert train.PiecewiseConstantDecay([], [2e-3])(5) == 2e-3


SCHEDULES = [
    (train.ExponentialDecay(1e-3, 7, 0.9), {"kind": "exponential", "lr0": 1e-3, "decay_steps": 7, "decay_rate": 0.9}),
    (train.ExponentialDecay(1e-3, 7, 0.9, staircase=True),
     {"kind": "exponential", "lr0": 1e-3, "decay_steps": 7, "decay_rate": 0.9, "staircase": True}),
    (train.CosineDecay(1e-3, 9, alpha=0.05), {"kind": "cosine", "lr0": 1e-3, "decay_steps": 9, "alpha": 0.05}),
    (train.CosineDecay(1e-4, 9, warmup_target=2e-3, warmup_steps=5),
     {"kind": "cosine", "lr0": 1e-4, "decay_steps": 9, "alpha": 0.0, "warmup_target": 2e-3, "warmup_steps": 5}),
    (train.PiecewiseConstantDecay([2, 5, 11], [1e-2, 5e-3, 1e-3, 1e-4]),
     {"kind": "piecewise", "boundaries": [2, 5, 11], "values": [1e-2, 5e-3, 1e-3, 1e-4]}),
]


@pytest.mark.parametrize("sched,spec", SCHEDULES, ids=[f"{type(s).__name__}-{i}" for i, (s, _) in enumerate(SCHEDULES)])
def test_schedule_follows_the_reference_and_round_trips(sched, spec):
    for s in list(range(0, 20)) + [10 ** 6]:
        assert sched(s) == pytest.approx(OR.schedule_rate(spec, s), rel=1e-14, abs=1e-20), s
    again = type(sched).from_config(sched.get_config())
    assert again.get_config() == sched.get_config()
    assert [again(s) for s in range(20)] == [sched(s) for s in range(20)]
    assert np.array_equal(again._record(), sched._record())
    opt = train.Adam.from_config(train.Adam(sched, clipnorm=1.0).get_config())
    assert opt.get_config() == train.Adam(sched, clipnorm=1.0).get_config()
    assert opt.get_config()["learning_rate"] == {"class_name": type(sched).__name__, "config": sched.get_config()}


def test_record_words():
    """The layout that include/impnn.h documents."""
    r = train.ExponentialDecay(1e-3, 7, 0.9, staircase=True)._record()
    f = r.view(np.float32)
    assert r.dtype == np.int32 and r.shape == (32,)
    assert (r[0], r[1], r[4]) == (1, 1, 7) and f[2] == np.float32(1e-3) and f[3] == np.float32(0.9)
    r = train.CosineDecay(1e-4, 9, alpha=0.25, warmup_target=2e-3, warmup_steps=5)._record()
    f = r.view(np.float32)
    assert (r[0], r[4], r[5]) == (2, 9, 5) and (f[2], f[3], f[6]) == (np.float32(1e-4), np.float32(0.25), np.float32(2e-3))
    r = train.CosineDecay(1e-4, 9, warmup_steps=5)._record()
    assert r[5] == 0 and r.view(np.float32)[6] == np.float32(1e-4)
    r = train.PiecewiseConstantDecay([2, 5], [1e-2, 5e-3, 1e-3])._record()
    assert (r[0], r[7]) == (3, 2) and list(r[8:10]) == [2, 5]
    assert list(r.view(np.float32)[16:19]) == [np.float32(1e-2), np.float32(5e-3), np.float32(1e-3)]
    r = train.Adam(3e-4)._record()
    assert r[0] == 0 and r.view(np.float32)[2] == np.float32(3e-4) and not r[3:].any()


# ---------------------------------------------------------------------------------------------------------------------
# Callbacks
# ---------------------------------------------------------------------------------------------------------------------
class _Opt:
    def __init__(self, lr):
        self.learning_rate = lr


class _Model:
    def __init__(self, lr):
        self.optimizer = _Opt(lr)


def _plateau_rule(seq, lr, factor, patience, min_delta, cooldown, min_lr):
    """The rule as the issue states it, restated: [(epoch, new rate)]."""
    best, wait, cool, out = np.inf, 0, 0, []
    for epoch, cur in enumerate(seq):
        if cool > 0:
            cool -= 1
            wait = 0
        if cur < best - min_delta:
            best, wait = cur, 0
        elif cool <= 0:
            wait += 1
            if wait >= patience and lr > min_lr:
                lr = max(lr * factor, min_lr)
                out.append((epoch, lr))
                cool, wait = cooldown, 0
    return out


def _drive(cb, seq, lr):
    m = _Model(lr)
    cb.set_model(m)
    cb.on_train_begin({})
    for epoch, v in enumerate(seq):
        cb.on_epoch_begin(epoch, {})
        cb.on_epoch_end(epoch, {"val_loss": v, "loss": 0.0})
    return m


def test_reduce_lr_on_plateau_halves_after_patience():
    cb = train.ReduceLROnPlateau(factor=0.5, patience=2, min_delta=0.0)
    m = _drive(cb, [1.0, 0.9, 0.9, 0.9, 0.9, 0.9], 1e-2)
    assert cb.rates == [(3, 5e-3), (5, 2.5e-3)] and m.optimizer.learning_rate == 2.5e-3


def test_reduce_lr_on_plateau_cooldown():
    seq = [1.0] * 9
    cb = train.ReduceLROnPlateau(factor=0.1, patience=2, min_delta=0.0, cooldown=3)
    _drive(cb, seq, 1.0)
    # epoch 0 improves on inf; waits at 1, 2 -> reduce at 2; cooldown covers 3, 4 and ends while 5 is read; 5, 6 wait
    assert cb.rates == [(2, 0.1), (6, pytest.approx(0.01))]
    assert cb.rates == _plateau_rule(seq, 1.0, 0.1, 2, 0.0, 3, 0.0)


def test_reduce_lr_on_plateau_min_lr_floor():
    cb = train.ReduceLROnPlateau(factor=0.1, patience=1, min_delta=0.0, min_lr=5e-4)
    m = _drive(cb, [1.0] * 6, 1e-2)
    assert cb.rates == [(1, pytest.approx(1e-3)), (2, 5e-4)] and m.optimizer.learning_rate == 5e-4


def test_reduce_lr_on_plateau_improvement_resets_wait():
    seq = [1.0, 1.0, 0.5, 0.5, 0.5, 0.4, 0.4, 0.4]
    cb = train.ReduceLROnPlateau(factor=0.5, patience=2, min_delta=0.0)
    _drive(cb, seq, 1.0)
    assert cb.rates == [(4, 0.5), (7, 0.25)] == _plateau_rule(seq, 1.0, 0.5, 2, 0.0, 0, 0.0)


def test_reduce_lr_on_plateau_min_delta():
    seq = [1.0, 0.99995, 0.99993, 0.99991]          # improves, but never by min_delta = 1e-4 against the best (1.0)...
    cb = train.ReduceLROnPlateau(factor=0.5, patience=3)
    _drive(cb, seq, 1.0)
    assert cb.rates == [(3, 0.5)] and cb.best == 1.0
    seq2 = [1.0, 0.9998, 0.9996, 0.9994]            # ... and steps of 2e-4 do count
    cb2 = train.ReduceLROnPlateau(factor=0.5, patience=3)
    _drive(cb2, seq2, 1.0)
    assert cb2.rates == [] and cb2.best == 0.9994


def test_reduce_lr_on_plateau_follows_the_rule_on_random_monitors():
    rng = np.random.default_rng(3)
    for trial in range(20):
        seq = list(np.round(rng.uniform(0.5, 1.0, 40), 2))
        kw = dict(factor=float(rng.choice([0.1, 0.5])), patience=int(rng.integers(1, 5)),
                  min_delta=float(rng.choice([0.0, 0.05])), cooldown=int(rng.integers(0, 4)), min_lr=1e-3)
        cb = train.ReduceLROnPlateau(**kw)
        _drive(cb, seq, 0.1)
        want = _plateau_rule(seq, 0.1, kw["factor"], kw["patience"], kw["min_delta"], kw["cooldown"], kw["min_lr"])
        assert cb.rates == want, (trial, kw)


def test_learning_rate_scheduler_call_order():
    calls = []

    def fn(epoch, lr):
        calls.append((epoch, lr))
        return lr * 0.5

    cb = train.LearningRateScheduler(fn)
    m = _drive(cb, [1.0, 1.0, 1.0], 0.8)
    assert calls == [(0, 0.8), (1, 0.4), (2, 0.2)]          # before each epoch, with the rate then in force
    assert cb.rates == [(0, 0.4), (1, 0.2), (2, 0.1)] and m.optimizer.learning_rate == 0.1
    assert train.Callback().on_epoch_begin(0) is None      # the no-op that fit calls


# ---------------------------------------------------------------------------------------------------------------------
# Arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    with pytest.raises(ValueError):
        train.Adam(1e-3, clipnorm=1.0, global_clipnorm=1.0)
    with pytest.raises(ValueError):
        train.Adam(1e-3, weight_decay=-1e-4)
    with pytest.raises(ValueError):
        train.Adam(1e-3, global_clipnorm=0.0)
    with pytest.raises(ValueError):
        train.ExponentialDecay(1e-3, 10, -0.5)
    with pytest.raises(ValueError):
        train.ExponentialDecay(1e-3, 0, 0.5)
    with pytest.raises(ValueError):
        train.CosineDecay(1e-3, -3)
    with pytest.raises(ValueError):
        train.PiecewiseConstantDecay(list(range(9)), [1e-3] * 10)
    with pytest.raises(ValueError):
        train.PiecewiseConstantDecay([5, 3], [1e-3] * 3)
    with pytest.raises(ValueError):
        train.PiecewiseConstantDecay([1, 2], [1e-3] * 2)
    with pytest.raises(ValueError):
        train.Adam(float("nan"))
    with pytest.raises(ValueError):
        train.ReduceLROnPlateau(factor=1.0)
    sched = train.ExponentialDecay(1e-3, 10, 0.5)
    with pytest.raises(ValueError):
        _drive(train.ReduceLROnPlateau(patience=1), [1.0, 1.0], sched)
    with pytest.raises(ValueError):
        _drive(train.LearningRateScheduler(lambda e, lr: lr), [1.0], sched)
    train.PiecewiseConstantDecay(list(range(8)), [1e-3] * 9)   # 8 boundaries are fine


def test_rate_before_build_is_a_host_value():
    a = train.Adam(2e-3, clipnorm=1.0)
    assert a.learning_rate == 2e-3 and a.current_learning_rate() == float(np.float32(2e-3))
    a.learning_rate = 5e-4
    assert a.learning_rate == 5e-4 and a.get_config()["learning_rate"] == 5e-4
    s = train.CosineDecay(1e-2, 10)
    a.learning_rate = s
    assert a.learning_rate is s and a.current_learning_rate() == float(np.float32(1e-2))
    a.exclude_from_weight_decay(["bias"])                    # allowed before build


def test_config_pin():
    assert train.Adam(1e-3, clipnorm=1.0).get_config() == {
        "name": "Adam", "learning_rate": 1e-3, "beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7, "clipnorm": 1.0}
    assert train.Adam(1e-3, global_clipnorm=2.0, weight_decay=4e-3).get_config() == {
        "name": "Adam", "learning_rate": 1e-3, "beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7, "clipnorm": None,
        "global_clipnorm": 2.0, "weight_decay": 4e-3}
