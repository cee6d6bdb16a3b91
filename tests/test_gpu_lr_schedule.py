"""The scheduled optimizer step on the GPU (impnn_adam_step_scheduled, impnn_lr_schedule_eval): the learning rate and its
schedule in device memory, tf.clip_by_global_norm and keras's decoupled weight decay in the optimizer launch, and what
model.fit builds on them - a rate assigned between replays of a captured step, a schedule inside a captured fit,
ReduceLROnPlateau.

References: tests/optimizer_ref.py (float64, restated from the Keras / TensorFlow definitions) and, for the existing
entries, the library itself.  Bounds: 1e-5 for values (tests/test_gpu_head_fuzz.py::VALUE_TOL, through
conftest.assert_close); for a device schedule value, 8 times the largest error that the float32 restatement of the same
formula shows against float64 on the same grid of steps (``schedule_bound``, from the reference alone); for two training
runs whose gradients are float atomics, the whole-model bound of tests/test_gpu_sample_weight.py (MODEL_TOL).

Variable set: 4096, 70 000 (more than one updating workgroup, 16-byte loads), 1, 259 (its gradient view starts 4 bytes
off a 16-byte boundary: scalar loads), 5, 4097 (ragged ends) elements in train.Adam's flat block."""
import ctypes as C

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, model as MM, synthetic, train, weights
from conftest import assert_close

import optimizer_ref as OR
import test_gpu_head_fuzz as FZ
import test_gpu_sample_weight as SW

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
VALUE_TOL = FZ.VALUE_TOL
SIZES = [4096, 70000, 1, 259, 5, 4097]
BIG = 1                       # the 70 000-element variable
NAMES = [f"layer{i}/{'bias' if i in (2, 4) else 'kernel'}" for i in range(len(SIZES))]
LR = 5e-2                     # steps of about 5e-2 against weights of about 1: the value bound is 1e-3 of a step
BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -4


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _weights(seed=21):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=n).astype(F32) for n in SIZES]


def _grads(seed, norm=None):
    """One gradient per variable; ``norm``: the global norm of the set."""
    rng = np.random.default_rng(seed)
    gs = [rng.normal(size=n) for n in SIZES]
    if norm is not None:
        k = norm / np.sqrt(sum((g * g).sum() for g in gs))
        gs = [g * k for g in gs]
    return [g.astype(F32) for g in gs]


class _Run:
    """train.Adam built on device copies of a weight set; ``step(gs)`` loads the gradients and applies one update."""

    def __init__(self, ws, opt=None, **kw):
        self.opt = opt if opt is not None else train.Adam(**kw)
        self.vars = [torch.tensor(w, device=DEV, requires_grad=True) for w in ws]
        self.opt.build(self.vars, names=NAMES[:len(ws)])
        self.off = np.concatenate([[0], np.cumsum([w.size for w in ws])])
        if len(ws) == len(SIZES):   # the layout this file's cases rely on
            g0 = self.opt.flat_grad.data_ptr()
            assert g0 % 16 == 0 and (g0 + 4 * self.off[BIG]) % 16 == 0 and (g0 + 4 * self.off[3]) % 16 == 4

    def load(self, gs):
        for v, g in zip(self.vars, gs):
            v.grad.copy_(torch.from_numpy(np.ascontiguousarray(g)))

    def step(self, gs):
        self.load(gs)
        self.opt.apply_gradients()
        self.opt.zero_grad()
        return self.state()

    def state(self):
        torch.cuda.synchronize()
        cut = lambda flat: [flat[a:b].cpu().numpy() for a, b in zip(self.off[:-1], self.off[1:])]
        return [v.detach().cpu().numpy().copy() for v in self.vars], cut(self.opt.m), cut(self.opt.v)


def _same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{what}: variable {i}"


# =====================================================================================================================
# 1. constant record against the counted entry
# =====================================================================================================================
@pytest.mark.parametrize("clip", [1.0, None])
def test_constant_record_keeps_the_bits_of_the_counted_entry(clip):
    ws = _weights()
    new = _Run(ws, learning_rate=1e-3, clipnorm=clip)
    old = _Run(ws, learning_rate=1e-3, clipnorm=clip)
    for t in range(3):
        gs = _grads(30 + t, norm=[0.5, 3.0, 40.0][t])
        got = new.step(gs)
        old.load(gs)
        o = old.opt
        _lib.check(_lib.load().impnn_adam_clipnorm_step_counted(
            _p(o._table), _p(o._sizes), len(ws), _p(o._step_dev), 1e-3, o.beta_1, o.beta_2, o.epsilon, clip or 0.0,
            _lib.stream_ptr()))
        o.zero_grad()
        want = old.state()
        for part, a, b in zip("wmv", got, want):
            _same_bits(a, b, f"step {t + 1}, {part}")
        assert new.opt.iterations == old.opt.iterations == t + 1


# =====================================================================================================================
# 2. device schedule values
# =====================================================================================================================
SCHEDULES = {
    "constant": (3e-4, {"kind": "constant", "lr": 3e-4}, []),
    "exponential": (train.ExponentialDecay(1e-3, 1000, 0.96),
                    {"kind": "exponential", "lr0": 1e-3, "decay_steps": 1000, "decay_rate": 0.96}, [1000]),
    "exponential staircase": (train.ExponentialDecay(1e-3, 1000, 0.96, staircase=True),
                              {"kind": "exponential", "lr0": 1e-3, "decay_steps": 1000, "decay_rate": 0.96,
                               "staircase": True}, [1000, 2000]),
    "exponential 2": (train.ExponentialDecay(LR, 2, 0.5), {"kind": "exponential", "lr0": LR, "decay_steps": 2,
                                                          "decay_rate": 0.5}, [2, 3, 4, 5]),
    "cosine": (train.CosineDecay(1e-3, 1000, alpha=0.1),
               {"kind": "cosine", "lr0": 1e-3, "decay_steps": 1000, "alpha": 0.1}, [500, 1000]),
    "cosine warm-up": (train.CosineDecay(1e-4, 1000, alpha=0.05, warmup_target=2e-3, warmup_steps=100),
                       {"kind": "cosine", "lr0": 1e-4, "decay_steps": 1000, "alpha": 0.05, "warmup_target": 2e-3,
                        "warmup_steps": 100}, [50, 99, 100, 101, 600, 1100]),
    "piecewise": (train.PiecewiseConstantDecay([3, 6, 10, 20, 40, 80, 160, 320], [10 ** -(2 + 0.25 * i) for i in range(9)]),
                  {"kind": "piecewise", "boundaries": [3, 6, 10, 20, 40, 80, 160, 320],
                   "values": [10 ** -(2 + 0.25 * i) for i in range(9)]}, [3, 6, 10, 20, 40, 80, 160, 320]),
}


def schedule_grid(marks):
    """Steps 0, 1, every boundary / decay_steps with its neighbours, and 10^6."""
    return sorted({0, 1, 10 ** 6} | {max(m + d, 0) for m in marks for d in (-1, 0, 1)})


def schedule_bound(name):
    """8 times the float32 restatement's largest relative error against float64 on the schedule's grid."""
    _, spec, marks = SCHEDULES[name]
    return 8.0 * OR.f32_error(spec, schedule_grid(marks))


def _device_rates(rate, steps):
    rec = torch.from_numpy(train.Adam(rate)._record()).to(DEV)
    st = torch.tensor(steps, dtype=torch.int64, device=DEV)
    out = torch.full((len(steps),), -1.0, dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().impnn_lr_schedule_eval(_p(rec), _p(st), _p(out), len(steps), _lib.stream_ptr()))
    return out.cpu().numpy()


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_device_schedule_values(name):
    rate, spec, marks = SCHEDULES[name]
    grid = schedule_grid(marks)
    want = np.array([OR.schedule_rate(spec, s) for s in grid])
    if not isinstance(rate, float):   # the reference and train's float64 definition are one function
        np.testing.assert_allclose([rate(s) for s in grid], want, rtol=1e-14, atol=0)
    got = _device_rates(rate, grid)
    bound = schedule_bound(name)
    err = OR.rel_err(got, want)
    print(f"{name}: bound {bound:.3e}, worst device error {err.max():.3e} at step {grid[int(err.argmax())]}")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), f"{name}: relative error {err.max():.3e} > {bound:.3e} at step {grid[int(err.argmax())]}"


# =====================================================================================================================
# Model level: atom_dim 32, 2 steps, N = 6, E = 10, batch 4
# =====================================================================================================================
def _model(seed=5):
    Va, Vb = 11, 6
    w = weights.init_weights("viscosity", Va, Vb, atom_dim=32, bond_dim=8, fp_size=12, mixing_size=10, num_steps=2,
                             seed=seed, perturb=True)
    m = MM.build_model(Va, Vb, atom_dim=32, bond_dim=8, fp_size=12, mixing_size=10, num_steps=2, device=DEV)
    m.load_weights(w)
    inp = synthetic.make_batch(4, max_atoms=6, max_edges=10, atom_vocab_size=Va, bond_vocab_size=Vb, min_atoms=3,
                               seed=seed)
    y = np.random.default_rng(seed).normal(1.0, 0.5, size=4).astype(F32)
    return m, inp, y


class _Counting(torch.cuda.CUDAGraph):
    captures = 0
    replays = 0

    def capture_begin(self, *a, **k):
        _Counting.captures += 1
        return super().capture_begin(*a, **k)

    def replay(self):
        _Counting.replays += 1
        return super().replay()


def _bits(m):
    return {k: v.copy() for k, v in m.state_dict().items()}


def test_rate_written_between_replays_of_a_captured_step(monkeypatch):
    """3.  An assignment to optimizer.learning_rate reaches the next replay: with rate 0 every weight keeps its bits
    while m, v and the counter advance; no recapture."""
    monkeypatch.setattr(torch.cuda, "CUDAGraph", _Counting)
    _Counting.captures = _Counting.replays = 0
    m, inp, y = _model()
    m.compile(train.Adam(1e-3, clipnorm=1.0))
    opt = m.optimizer
    x = m._to_device(inp)
    record0 = opt._record_dev.clone()
    g = train.GraphedTrainStep(m, x, y)
    assert torch.equal(opt._record_dev, record0) and opt.iterations == 0, "the warm-up leaves record and counter alone"
    names = [n for n, _ in m.trainable_variables()]
    w0 = _bits(m)
    g(x, y)
    w1, m1, v1 = _bits(m), opt.m.clone(), opt.v.clone()
    assert all(not np.array_equal(w1[n], w0[n]) for n in names), "the first replay moves every variable"
    opt.learning_rate = 0.0
    assert opt.current_learning_rate() == 0.0
    g(x, y)
    w2 = _bits(m)
    for n in names:
        assert np.array_equal(w2[n].view(np.uint32), w1[n].view(np.uint32)), f"rate 0 moved {n}"
    assert not torch.equal(opt.m, m1) and not torch.equal(opt.v, v1) and opt.iterations == 2
    opt.learning_rate = 1e-3
    assert opt.current_learning_rate() == float(F32(1e-3))
    g(x, y)
    w3 = _bits(m)
    assert all(not np.array_equal(w3[n], w2[n]) for n in names) and opt.iterations == 3
    assert (_Counting.captures, _Counting.replays) == (1, 3)


class _Weights(train.Callback):
    """Keeps the weights at every epoch's end."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def on_epoch_end(self, epoch, logs=None):
        self.seen.append(self.model.state_dict())


def _delta_bound(rel, d_ref, w_ref):
    """|delta - delta_ref| per element: the schedule bound times |delta_ref|, plus the whole-model bound of
    test_gpu_sample_weight.py for two runs whose gradients are float atomics (MODEL_TOL of the tensor's largest weight)."""
    return rel * np.abs(d_ref) + SW.MODEL_TOL * np.abs(w_ref).max()


def test_captured_fit_with_exponential_decay_follows_the_scheduled_eager_steps():
    """4a.  Six captured steps (six one-batch epochs) with ExponentialDecay(decay_steps=2) against the same batches run
    eagerly through impnn_adam_clipnorm_step with each step's float64 rate rounded to float32.  Adam's epsilon is
    test_gpu_sample_weight.py's STEP_EPS, which makes a step Lipschitz in the gradient (see there)."""
    sched, spec, _ = SCHEDULES["exponential 2"]
    m, inp, y = _model()
    m.compile(train.Adam(sched, epsilon=SW.STEP_EPS, clipnorm=1.0))
    before = _bits(m)
    rec = _Weights()
    m.fit(inp, y, epochs=6, batch_size=4, shuffle=False, graph=True, callbacks=[rec])
    assert m.optimizer.iterations == 6
    assert m.optimizer.current_learning_rate() == pytest.approx(sched(6), rel=schedule_bound("exponential 2") + 1e-7)
    e, _, _ = _model()
    e.compile(train.Adam(LR, epsilon=SW.STEP_EPS, clipnorm=1.0))
    o = e.optimizer
    x = e._to_device(inp)
    eager, rates = [], []
    for t in range(1, 7):
        loss = e._loss(x, y, training=True)
        loss.backward()
        e.join_training_streams()
        rates.append(float(F32(OR.schedule_rate(spec, t - 1))))
        _lib.check(_lib.load().impnn_adam_clipnorm_step(_p(o._table), _p(o._sizes), len(o._vars), t, rates[-1], o.beta_1,
                                                        o.beta_2, o.epsilon, 1.0, _lib.stream_ptr()))
        o.zero_grad()
        e.weights_updated()
        eager.append(_bits(e))
    assert rates[0] == float(F32(LR)) and rates[5] < 0.2 * rates[0]
    rel = schedule_bound("exponential 2")
    names = [n for n, _ in m.trainable_variables()]
    seen = 0
    for t in range(6):
        for n in names:
            prev_c = (before if t == 0 else rec.seen[t - 1])[n].astype(np.float64)
            prev_e = (before if t == 0 else eager[t - 1])[n].astype(np.float64)
            d_c, d_e = rec.seen[t][n] - prev_c, eager[t][n] - prev_e
            bound = _delta_bound(rel, d_e, eager[t][n])
            worst = float((np.abs(d_c - d_e) / bound).max())
            assert worst <= 1.0, f"step {t + 1}, {n}: delta off by {worst:.2f} x its bound"
            if t == 5:   # would a fit that ignored the schedule be seen?  its step is rates[0] / rates[5] times this one
                seen += int(((rates[0] / rates[5] - 1.0) * np.abs(d_e) > 4 * bound).any())
    print(f"a constant rate would be seen in {seen} of {len(names)} tensors")
    assert seen >= 3, "a constant rate would be seen in several tensors"


class _Script(train.Callback):
    """Overwrites logs["val_loss"] with a scripted value (ahead of the callback under test in the list)."""

    def __init__(self, values):
        super().__init__()
        self.values = values

    def on_epoch_end(self, epoch, logs=None):
        logs["val_loss"] = self.values[epoch]


def test_reduce_lr_on_plateau_halves_the_step_of_a_captured_fit():
    """4b.  fit(graph=True) with ReduceLROnPlateau(factor=0.5, patience=2) on a scripted flat monitor: the rate is
    halved after epoch 2, and the update of epoch 3 is half of the same update of a fit without the callback (beta_1 = 0:
    the step is proportional to the rate; both fits walk the same trajectory up to the atomics' noise)."""
    runs = {}
    for with_cb in (False, True):
        m, inp, y = _model()
        m.compile(train.Adam(LR, beta_1=0.0, epsilon=SW.STEP_EPS, clipnorm=1.0))
        rec, plateau = _Weights(), train.ReduceLROnPlateau(factor=0.5, patience=2, min_delta=0.0)
        cbs = [_Script([1.0] * 4), rec] + ([plateau] if with_cb else [])
        h = m.fit(inp, y, epochs=4, batch_size=4, shuffle=False, graph=True, callbacks=cbs)
        assert sorted(h.history) == ["loss"], "History keeps its keys"
        runs[with_cb] = rec.seen
        if with_cb:
            assert plateau.rates == [(2, 0.5 * LR)] and m.optimizer.learning_rate == 0.5 * LR
            assert m.optimizer.current_learning_rate() == float(F32(0.5 * LR))
    names = list(runs[True][0])
    seen = 0
    for n in names:
        d_plain = runs[False][3][n].astype(np.float64) - runs[False][2][n]
        d_half = runs[True][3][n].astype(np.float64) - runs[True][2][n]
        if not np.abs(d_plain).max() > 0:
            continue   # (not a trained variable)
        bound = SW.MODEL_TOL * np.abs(runs[False][3][n]).max()
        assert (np.abs(d_half - 0.5 * d_plain) <= bound).all(), f"{n}: not half the step"
        seen += int((0.5 * np.abs(d_plain) > 4 * bound).any())
    print(f"the halving is several times the bound in {seen} of {len(names)} tensors")
    assert seen >= 3, "the halving is several times the bound in several tensors"


# =====================================================================================================================
# 5. global_clipnorm
# =====================================================================================================================
def _reference_steps(ws, grads, rates, **kw):
    """The float64 reference run.  beta_1, beta_2 and epsilon are the values the C entry receives - its arguments are
    floats, and 1 - float32(0.999) is 1.3e-5 (relative) from 1e-3, which the second moment shows in full."""
    kw = dict(kw, b1=float(F32(0.9)), b2=float(F32(0.999)), eps=float(F32(1e-7)))
    w = [a.astype(np.float64) for a in ws]
    m = [np.zeros(a.shape) for a in ws]
    v = [np.zeros(a.shape) for a in ws]
    out = []
    for t, (gs, lr) in enumerate(zip(grads, rates), 1):
        w, m, v = OR.adam_update(w, gs, m, v, t, lr, **kw)
        out.append((w, m, v))
    return out


def _check(what, got, want):
    for part, a, b in zip(("w", "m", "v"), got, want):
        for i, (x, y) in enumerate(zip(a, b)):
            assert_close(x, y, VALUE_TOL, f"{what}: {part} of variable {i} ({x.size} elements)")


GLOBAL_C = 2.0
GLOBAL_GRADS = [("below", 0.5), ("above", 40.0), ("zero", 0.0), ("just above", 2.002)]


def test_global_clipnorm_against_fp64():
    """Four steps in a row - global norm below c, far above, all-zero, just above - against the float64 reference."""
    ws = _weights()
    grads = [[np.zeros(n, F32) for n in SIZES] if norm == 0.0 else _grads(50 + i, norm)
             for i, (_, norm) in enumerate(GLOBAL_GRADS)]
    ref = _reference_steps(ws, grads, [LR] * len(grads), global_clipnorm=GLOBAL_C)
    scales = [OR.clip_scales(gs, global_clipnorm=GLOBAL_C)[0] for gs in grads]
    assert scales[0] == 1.0 and scales[1] < 0.06 and scales[2] == 1.0 and 0.998 < scales[3] < 1.0
    runs = [_Run(ws, learning_rate=LR, global_clipnorm=GLOBAL_C) for _ in range(2)]
    for t, gs in enumerate(grads):
        got = runs[0].step(gs)
        again = runs[1].step(gs)
        _check(f"global_clipnorm, step {t + 1} ({GLOBAL_GRADS[t][0]})", got, ref[t])
        for part, a, b in zip("wmv", got, again):
            _same_bits(a, b, f"two runs, step {t + 1}, {part}")
    assert runs[0].opt.iterations == len(grads)


def test_global_clipnorm_scales_every_element_alike():
    """First step from m = 0: m = (1 - beta_1) * (g * scale), so m divided by the unclipped reference moment
    (1 - beta_1) * g is the scale each element saw.  The two float32 products round by at most 2^-24 each (relative), so
    the ratios of all 70 000 elements lie within 4 * 2^-24 of each other, and near c / ||g|| of the float64 reference
    (the norm's float32 sum: within VALUE_TOL)."""
    ws = _weights()
    gs = _grads(61, 40.0)
    run = _Run(ws, learning_rate=LR, global_clipnorm=GLOBAL_C)
    _, m, _ = run.step(gs)
    for i in (BIG, 3, 5):
        g = gs[i].astype(np.float64)
        keep = np.abs(g) > 1e-3 * np.abs(g).max()       # (no ratio from a denormal product)
        ratio = m[i].astype(np.float64)[keep] / ((1.0 - float(F32(0.9))) * g[keep])
        assert keep.sum() > 0.9 * g.size
        assert ratio.max() - ratio.min() <= 4 * 2.0 ** -24 * ratio.max(), f"variable {i}: more than one scale"
        assert abs(ratio.mean() / (GLOBAL_C / OR.global_norm(gs)) - 1.0) <= VALUE_TOL


def test_global_clipnorm_non_finite_norm_gives_nan_everywhere():
    ws = _weights()
    gs = _grads(62, 1.0)
    gs[4][2] = np.inf
    run = _Run(ws, learning_rate=LR, global_clipnorm=GLOBAL_C)
    w, m, v = run.step(gs)
    for i in range(len(SIZES)):
        assert np.isnan(w[i]).all() and np.isnan(m[i]).all() and np.isnan(v[i]).all(), f"variable {i}"
    assert run.opt.iterations == 1


def test_global_clipnorm_of_one_variable_is_clipnorm():
    ws = [_weights()[BIG]]
    for norm in (0.5, 40.0):
        gs = [_grads(63, norm)[BIG]]
        a = _Run(ws, learning_rate=LR, global_clipnorm=GLOBAL_C).step(gs)
        b = _Run(ws, learning_rate=LR, clipnorm=GLOBAL_C).step(gs)
        _check(f"one variable, norm {norm}", a, b)


# =====================================================================================================================
# 6. weight_decay
# =====================================================================================================================
WD = 4e-2
DECAYS = [int("bias" not in n) for n in NAMES]


def test_weight_decay_against_fp64_and_exclusions():
    ws = _weights()
    grads = [_grads(70 + t, [0.5, 3.0, 0.8][t]) for t in range(3)]
    ref = _reference_steps(ws, grads, [LR] * 3, clipnorm=1.0, weight_decay=WD, decays=DECAYS)
    opt = train.Adam(LR, clipnorm=1.0, weight_decay=WD)
    opt.exclude_from_weight_decay(["bias"])
    run = _Run(ws, opt=opt)
    plain = _Run(ws, learning_rate=LR, clipnorm=1.0)
    zero = _Run(ws, learning_rate=LR, clipnorm=1.0, weight_decay=0.0)
    assert opt._decay_flags.tolist() == DECAYS and 0 in DECAYS and 1 in DECAYS
    with pytest.raises(RuntimeError):
        opt.exclude_from_weight_decay(["kernel"])
    for t, gs in enumerate(grads):
        got, p, z = run.step(gs), plain.step(gs), zero.step(gs)
        _check(f"weight_decay, step {t + 1}", got, ref[t])
        for part, a, b in zip("wmv", z, p):
            _same_bits(a, b, f"weight_decay=0.0 against none, step {t + 1}, {part}")
        for i, flag in enumerate(DECAYS):
            same = np.array_equal(got[0][i].view(np.uint32), p[0][i].view(np.uint32))
            assert same == (not flag), f"step {t + 1}: variable {i} ({NAMES[i]})"
    # the decay is seen: lr * wd * |w| = 2e-3 |w| per step against the bound of 1e-5 max|w|
    assert np.abs(got[0][BIG] - p[0][BIG]).max() > 100 * VALUE_TOL * np.abs(p[0][BIG]).max()


def test_weight_decay_uses_the_rate_of_the_step():
    sched, spec, _ = SCHEDULES["exponential 2"]
    ws = _weights()
    grads = [_grads(80 + t, 0.7) for t in range(5)]
    rates = [OR.schedule_rate(spec, t) for t in range(5)]
    assert rates[4] == pytest.approx(LR / 4)
    ref = _reference_steps(ws, grads, rates, weight_decay=WD)
    run = _Run(ws, learning_rate=sched, weight_decay=WD)
    for t, gs in enumerate(grads):
        assert run.opt.current_learning_rate() == pytest.approx(rates[t], rel=1e-6)
        _check(f"scheduled weight_decay, step {t + 1}", run.step(gs), ref[t])
    # a decay at the first rate would be seen: (LR - rates[4]) * wd * |w| in the last step alone
    assert (LR - rates[4]) * WD > 100 * VALUE_TOL


# =====================================================================================================================
# 7. C ABI
# =====================================================================================================================
def _status(code):
    return code, _lib.load().impnn_last_error_string().decode()


def test_cabi_statuses():
    lib = _lib.load()
    assert lib.impnn_abi_version() == 3
    assert lib.impnn_adam_step_scheduled(None, None, 0, None, None, 0.9, 0.999, 1e-7, 0.0, 0.0, 0.0, None, None, 0,
                                         None) == 0
    assert lib.impnn_lr_schedule_eval(None, None, None, 0, None) == 0
    assert lib.impnn_adam_step_scheduled_workspace_floats(0) == 0
    assert lib.impnn_adam_step_scheduled_workspace_floats(3) >= 3

    def checked(rec):
        return _status(lib.impnn_lr_schedule_check(C.c_void_p(rec.ctypes.data)))

    good = train.ExponentialDecay(1e-3, 10, 0.5)._record()
    assert checked(good)[0] == 0
    bad = good.copy(); bad[0] = 7
    code, text = checked(bad)
    assert code == UNSUPPORTED and "kind" in text
    bad = good.copy(); bad[4] = 0
    code, text = checked(bad)
    assert code == BADARG and "decay_steps" in text
    bad = train.CosineDecay(1e-3, 10)._record(); bad[4] = -5
    assert checked(bad)[0] == BADARG
    bad = train.PiecewiseConstantDecay([1], [1e-3, 1e-4])._record(); bad[7] = 9
    assert checked(bad)[0] == UNSUPPORTED

    run = _Run(_weights(), learning_rate=1e-3, global_clipnorm=1.0)
    o = run.opt
    before = run.state()
    need = lib.impnn_adam_step_scheduled_workspace_floats(len(SIZES))
    small = torch.zeros(need - 1, dtype=torch.float32, device=DEV)
    args = lambda clip, gclip, ws, n: (_p(o._table), _p(o._sizes), len(SIZES), _p(o._step_dev), _p(o._record_dev), 0.9,
                                       0.999, 1e-7, clip, gclip, 0.0, None, _p(ws), n, _lib.stream_ptr())
    code, text = _status(lib.impnn_adam_step_scheduled(*args(0.0, 1.0, small, small.numel())))
    assert code == WORKSPACE and "workspace" in text
    code, text = _status(lib.impnn_adam_step_scheduled(*args(1.0, 1.0, o._norm_ws, o._norm_ws.numel())))
    assert code == BADARG and "exclude" in text
    after = run.state()
    for a, b in zip(before, after):
        _same_bits(a, b, "a refused call touches nothing")
    assert o.iterations == 0
    with pytest.raises(_lib.ImpnnError):   # the setter validates through the library before it writes
        bad_rate = train.ExponentialDecay(1e-3, 10, 0.5)
        bad_rate.decay_steps = 0
        o.learning_rate = bad_rate
