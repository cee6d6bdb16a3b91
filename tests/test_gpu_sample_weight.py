"""Per-sample weights on the GPU: the weighted loss entries of the model head and of the transfer head
(impnn_weighted_model_head_loss[_bwd], impnn_weighted_transfer_head_loss[_bwd]) against fp64, and fit / evaluate /
train_on_batch / GraphedTrainStep with ``sample_weight`` against the fp64 oracle.

  loss = (1/B) * sum_b w_b * L(pred_b - y_b) + sum_t l2[t] * sum(W_t^2),  B counting the samples of weight 0

Reference: tests/weighted_ref.py (tests/head_ref.py::forward and tests/transfer_ref.py::head underneath), fp64 with torch
autograd.  Bounds: the project's existing ones through conftest.assert_close - 1e-5 for values and losses, 1e-4 for
kernel gradients, 2e-4 through the whole model.  tests/test_sample_weight_host.py walks the same case tables on the CPU:
the reference in fp32 meets these bounds against fp64 on exactly these inputs and weights, and no relu pre-activation,
clipped softplus value or Huber |e| of the fp64 reference lies within a relative 1e-4 of a kink - nothing below is
skipped or excluded."""
import ctypes as C

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, autograd, layers as L, model as MM, ops, synthetic, train
from ionic_mpnn_amd._lib import ptr, stream_ptr
from oracle import torch_ref as TR, train_oracle as TO
from conftest import assert_close

import test_gpu_head_fuzz as FZ
import transfer_ref as R
import weighted_ref as WR
from test_gpu_train import _tiny_model
from test_gpu_transfer import head_mask, make_transfer, stage2

pytestmark = pytest.mark.gpu
DEV = "cuda"
VALUE_TOL, GRAD_TOL, MODEL_TOL, DLOSS = FZ.VALUE_TOL, FZ.GRAD_TOL, FZ.MODEL_TOL, FZ.DLOSS
F32 = np.float32
HEAD_CASES, TH_CASES = WR.model_head_cases(), WR.transfer_cases()
_dev, _np = FZ._dev, FZ._np


def _table(tensors):
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _ws(floats):
    return torch.zeros(int(floats), dtype=torch.float32, device=DEV)


# =====================================================================================================================
# Kernel level, against fp64
# =====================================================================================================================
@pytest.mark.parametrize("wc", HEAD_CASES, ids=[c.name for c in HEAD_CASES])
def test_weighted_model_head_against_fp64(wc):
    """autograd.ModelHeadLoss with weights, forward and backward with dloss = 0.37 as a device scalar: the loss,
    dpooled_cat / dpooled_an and every parameter gradient; the loss twice on one workspace with equal bits."""
    c = wc.base
    inp = FZ.model_head_inputs(c)
    sw = WR.case_weights(wc)
    ref = WR.model_head_reference(wc, inp, sw, torch.float64)
    pc, pa = _dev(inp["pc"], True), _dev(inp["pa"], True)
    y, w_dev = _dev(inp["y"]), _dev(sw)
    T = _dev(inp["T"]).reshape(-1, 1) if c.kind == 0 else None
    params = [_dev(a, True) for a in inp["w"]]
    ws = _ws(_lib.load().impnn_model_head_loss_workspace_floats(c.B))
    l2 = autograd.WeightedL2(inp["l2"], w_dev)
    loss = autograd.ModelHeadLoss.apply(c.kind, c.F, c.Mx, l2, ws, pc, pa, T, y, *params)
    (loss * torch.tensor(DLOSS, device=DEV)).backward()
    with torch.no_grad():
        again = autograd.ModelHeadLoss.apply(c.kind, c.F, c.Mx, l2, ws, pc, pa, T, y, *params)
    assert torch.equal(loss.detach(), again), "one workspace, the same loss bits at every call"
    assert int(ws[:1].view(torch.int32).item()) == 0, "the arrival counter is back at zero"
    assert w_dev.grad is None and np.array_equal(w_dev.cpu().numpy(), sw), "the weights get no gradient and stay"
    got = dict(loss=_np(loss).reshape(1), grads=[_np(p.grad) for p in params] + [_np(pc.grad), _np(pa.grad)])
    print(f"{wc.name}: loss {float(loss):.8f} ref {float(ref['loss'][0]):.8f}")
    WR.check_model_head(wc, got, ref)


def _transfer_cfg(c, inp, mm, mv, sw=None):
    step = torch.tensor([FZ.TH_STEP], dtype=torch.int64, device=DEV)
    drop = ops.Dropout(c.rate, FZ.TH_SEED, ops.dropout_layer_word(L.Dropout.LAYER_ID), step) if c.rate else None
    cfg = {"fp_size": c.F, "mixing_size": c.Mx, "l2": inp["l2"], "moving_mean": mm, "moving_variance": mv,
           "momentum": R.BN_MOMENTUM, "epsilon": R.BN_EPS, "bn_batch": bool(c.bn), "dropout": drop,
           "loss_kind": 0 if c.loss[0] == "mse" else 1, "delta": c.loss[1]}
    if sw is not None:
        cfg["sample_weight"] = sw
    return cfg


@pytest.mark.parametrize("wc", TH_CASES, ids=[c.name for c in TH_CASES])
def test_weighted_transfer_head_against_fp64(wc):
    """autograd.TransferHeadLoss with cfg["sample_weight"]: squared error and Huber, BatchNormalization with the batch
    statistics and with the moving ones, a Dropout mask on the small Huber passes.  The moving statistics move as in the
    unweighted pass: the weights do not reach them."""
    c = wc.base
    inp = FZ.transfer_inputs(c)
    sw = WR.case_weights(wc)
    ref = WR.transfer_reference(wc, inp, sw, torch.float64)
    want = FZ.asked(c)
    weights = [_dev(a, t in want) for t, a in enumerate(inp["w"])]
    pc, pa = _dev(inp["pc"], True), _dev(inp["pa"], True)
    y, mm, mv, w_dev = _dev(inp["y"]), _dev(inp["mm"]), _dev(inp["mv"]), _dev(sw)
    cfg = _transfer_cfg(c, inp, mm, mv, w_dev)
    ws = _ws(_lib.load().impnn_transfer_head_loss_workspace_floats(c.B))
    loss = autograd.TransferHeadLoss.apply(cfg, ws, pc, pa, y, *weights)
    (loss * torch.tensor(DLOSS, device=DEV)).backward()
    got = dict(loss=_np(loss).reshape(1), mm=_np(mm), mv=_np(mv), dpooled=[_np(pc.grad), _np(pa.grad)],
               grads={t: _np(weights[t].grad) for t in want if t != "pooled"})
    if c.bn:   # the statistics of the unweighted pass, bit for bit
        mm0, mv0 = _dev(inp["mm"]), _dev(inp["mv"])
        with torch.no_grad():
            autograd.TransferHeadLoss.apply(_transfer_cfg(c, inp, mm0, mv0), ws, pc, pa, y, *weights)
        assert torch.equal(mm, mm0) and torch.equal(mv, mv0), "the weights moved BatchNormalization's statistics"
    else:
        assert torch.equal(mm, _dev(inp["mm"])) and torch.equal(mv, _dev(inp["mv"])), "frozen statistics, bit for bit"
        assert weights[10].grad is None and weights[11].grad is None
    assert int(ws[:1].view(torch.int32).item()) == 0, "the arrival counter is back at zero"
    assert w_dev.grad is None and np.array_equal(w_dev.cpu().numpy(), sw)
    print(f"{wc.name}: loss {float(loss):.8f} ref {float(ref['loss'][0]):.8f}")
    WR.check_transfer(wc, got, ref)


# =====================================================================================================================
# Unweighted bits: the weighted entry with a null weight, and with a weight of ones
# =====================================================================================================================
def _head_pass(c, inp, entry, sw):
    """One forward and backward through the C entries themselves -> (loss, dpooled_cat, dpooled_an, gradients).
    ``entry``: "impnn_model_head_loss" (takes no weight) or "impnn_weighted_model_head_loss" (``sw`` may be None)."""
    lib = _lib.load()
    weighted = "weighted" in entry
    pc, pa, y = _dev(inp["pc"]), _dev(inp["pa"]), _dev(inp["y"])
    T = _dev(inp["T"]) if c.kind == 0 else None
    w = [_dev(a) for a in inp["w"]]
    grads = [torch.zeros_like(t) for t in w]
    lam = (C.c_float * len(w))(*inp["l2"])
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    ws = _ws(lib.impnn_model_head_loss_workspace_floats(c.B))
    dloss = torch.tensor([DLOSS], dtype=torch.float32, device=DEV)
    dpc, dpa = torch.empty_like(pc), torch.empty_like(pa)
    extra = ((ptr(sw) if sw is not None else None,) if weighted else ())
    Tp = ptr(T) if T is not None else None
    _lib.check(getattr(lib, entry)(c.kind, ptr(pc), ptr(pa), Tp, _table(w), lam, ptr(y), *extra, None, ptr(loss), ptr(ws),
                                   ws.numel(), c.B, c.D, c.F, c.Mx, stream_ptr()))
    _lib.check(getattr(lib, entry + "_bwd")(c.kind, ptr(pc), ptr(pa), Tp, _table(w), lam, ptr(y), *extra, ptr(dloss),
                                           ptr(dpc), ptr(dpa), _table(grads), c.B, c.D, c.F, c.Mx, stream_ptr()))
    torch.cuda.synchronize()
    return loss, dpc, dpa, grads


BITS_HEAD = [c for c in FZ.model_head_cases() if c.name.rsplit(" kind", 1)[0] in ("B=7", "B=9", "B=2049", "B=4097", "widths 64 33 64")]


@pytest.mark.parametrize("c", BITS_HEAD, ids=[c.name for c in BITS_HEAD])
def test_model_head_null_and_unit_weights_keep_the_unweighted_bits(c):
    """impnn_weighted_model_head_loss[_bwd] with sample_weight == NULL, and with a weight of ones, against
    impnn_model_head_loss[_bwd]: the loss and dpooled bit for bit; the parameter gradients are float atomics over
    workgroups, so they are held to the gradient bound."""
    inp = FZ.model_head_inputs(c)
    base = _head_pass(c, inp, "impnn_model_head_loss", None)
    ones = torch.ones(c.B, dtype=torch.float32, device=DEV)
    for what, sw in (("null weight", None), ("weight of ones", ones)):
        got = _head_pass(c, inp, "impnn_weighted_model_head_loss", sw)
        assert torch.equal(got[0], base[0]), f"{c.name}, {what}: loss bits"
        assert torch.equal(got[1], base[1]) and torch.equal(got[2], base[2]), f"{c.name}, {what}: dpooled bits"
        for t, (a, e) in enumerate(zip(got[3], base[3])):
            assert_close(_np(a), _np(e), GRAD_TOL, f"{c.name}, {what}: gradient of tensor {t}")


def _transfer_pass(c, inp, entry, sw):
    """As _head_pass, for impnn_transfer_head_loss / impnn_weighted_transfer_head_loss and their backwards."""
    lib = _lib.load()
    weighted = "weighted" in entry
    B, D, F, Mx = c.B, c.D, c.F, c.Mx
    pc, pa, y = _dev(inp["pc"]), _dev(inp["pa"]), _dev(inp["y"])
    mm, mv = _dev(inp["mm"]), _dev(inp["mv"])
    w = [_dev(a) for a in inp["w"]]
    grads = [None if (not c.bn and t in (10, 11)) else torch.zeros_like(a) for t, a in enumerate(w)]
    lam = (C.c_float * 18)(*inp["l2"])
    step = torch.tensor([FZ.TH_STEP], dtype=torch.int64, device=DEV)
    dargs = (c.rate, C.c_uint64(FZ.TH_SEED), ptr(step), ops.dropout_layer_word(L.Dropout.LAYER_ID)) if c.rate else \
        (0.0, C.c_uint64(0), None, 0)
    n_saved = int(lib.impnn_transfer_head_saved_floats(B, F, Mx))
    saved = torch.empty(n_saved, dtype=torch.float32, device=DEV)
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    ws = _ws(lib.impnn_transfer_head_loss_workspace_floats(B))
    wsn = int(lib.impnn_transfer_head_bwd_workspace_floats(B, F, Mx))
    work = torch.empty(wsn, dtype=torch.float32, device=DEV)
    dloss = torch.tensor([DLOSS], dtype=torch.float32, device=DEV)
    dpc, dpa = torch.empty_like(pc), torch.empty_like(pa)
    extra = ((ptr(sw) if sw is not None else None,) if weighted else ())
    kind = 0 if c.loss[0] == "mse" else 1
    _lib.check(getattr(lib, entry)(ptr(pc), ptr(pa), _table(w), lam, ptr(mm), ptr(mv), R.BN_MOMENTUM, R.BN_EPS, int(c.bn),
                                   ptr(y), *extra, kind, c.loss[1], *dargs, ptr(saved), n_saved, None, ptr(loss), ptr(ws),
                                   ws.numel(), B, D, F, Mx, stream_ptr()))
    _lib.check(getattr(lib, entry + "_bwd")(ptr(pc), ptr(pa), _table(w), _table(grads), lam, int(c.bn), ptr(y), *extra, kind,
                                           c.loss[1], ptr(dloss), *dargs, ptr(saved), n_saved, ptr(work), wsn, ptr(dpc),
                                           ptr(dpa), B, D, F, Mx, stream_ptr()))
    torch.cuda.synchronize()
    return loss, dpc, dpa, [g for g in grads if g is not None], mm, mv


BITS_TH = [c for c in WR.transfer_bases() if c.B in (7, 9, 2049)]


@pytest.mark.parametrize("c", BITS_TH, ids=[c.name for c in BITS_TH])
def test_transfer_head_null_and_unit_weights_keep_the_unweighted_bits(c):
    """impnn_weighted_transfer_head_loss[_bwd] with sample_weight == NULL, and with a weight of ones, against
    impnn_transfer_head_loss[_bwd]: loss, moving statistics and dpooled bit for bit, the parameter gradients at the
    gradient bound (this head sums them without atomics; the bound is the issue's)."""
    inp = FZ.transfer_inputs(c)
    base = _transfer_pass(c, inp, "impnn_transfer_head_loss", None)
    ones = torch.ones(c.B, dtype=torch.float32, device=DEV)
    for what, sw in (("null weight", None), ("weight of ones", ones)):
        got = _transfer_pass(c, inp, "impnn_weighted_transfer_head_loss", sw)
        assert torch.equal(got[0], base[0]), f"{c.name}, {what}: loss bits"
        assert torch.equal(got[1], base[1]) and torch.equal(got[2], base[2]), f"{c.name}, {what}: dpooled bits"
        assert torch.equal(got[4], base[4]) and torch.equal(got[5], base[5]), f"{c.name}, {what}: moving statistics"
        for t, (a, e) in enumerate(zip(got[3], base[3])):
            assert_close(_np(a), _np(e), GRAD_TOL, f"{c.name}, {what}: gradient {t}")


# =====================================================================================================================
# Repetition: integer weights are repeated rows
# =====================================================================================================================
def _repeat(inp, counts, keys):
    idx = np.repeat(np.arange(len(counts)), counts.astype(np.int64))
    out = dict(inp)
    for k in keys:
        out[k] = inp[k][idx]
    return out, len(idx)


@pytest.mark.parametrize("name", ["B=9 kind 0", "B=9 kind 1", "B=2049 kind 0", "B=2049 kind 1"])
def test_model_head_integer_weights_are_repeated_rows(name):
    """B * (the data term of a batch with integer weights) == sum(w) * (the unweighted data term of the batch with
    every row repeated by its count), at the value bound.  No penalties, so a loss is its data term."""
    c = next(c for c in FZ.model_head_cases() if c.name == name)
    inp = dict(FZ.model_head_inputs(c), l2=[0.0] * (10 if c.kind == 0 else 12))
    counts = WR.sample_weights("counts", c.B, c.seed)
    weighted = _head_pass(c, inp, "impnn_weighted_model_head_loss", _dev(counts))[0]
    rep, n = _repeat(inp, counts, ("pc", "pa", "T", "y"))
    assert n == int(counts.sum()) and n != c.B
    repeated = _head_pass(c._replace(B=n), rep, "impnn_model_head_loss", None)[0]
    assert_close(np.array([float(weighted) * c.B]), np.array([float(repeated) * n]), VALUE_TOL, f"{name}: repetition")


@pytest.mark.parametrize("loss", [FZ.MSE, FZ.HUBER025])
def test_transfer_head_integer_weights_are_repeated_rows(loss):
    """The same for the transfer head, with the moving statistics and no Dropout (batch statistics and a mask per
    sample index would see a different batch)."""
    c = next(c for c in WR.transfer_bases() if c.B == 9 and c.D == 8 and c.bn == 0 and c.loss == loss)._replace(rate=0.0)
    inp = dict(FZ.transfer_inputs(c), l2=[0.0] * 18)
    counts = WR.sample_weights("counts", c.B, c.seed)
    weighted = _transfer_pass(c, inp, "impnn_weighted_transfer_head_loss", _dev(counts))[0]
    rep, n = _repeat(inp, counts, ("pc", "pa", "y"))
    assert n == int(counts.sum()) and n != c.B
    repeated = _transfer_pass(c._replace(B=n), rep, "impnn_transfer_head_loss", None)[0]
    assert_close(np.array([float(weighted) * c.B]), np.array([float(repeated) * n]), VALUE_TOL, f"{loss}: repetition")


# =====================================================================================================================
# Model level
# =====================================================================================================================
def _model_weights(B, seed):
    """Fractional weights with a zero and a repeated sample among them."""
    w = np.random.default_rng(seed).uniform(0.25, 2.0, B).astype(F32)
    w[1], w[B - 1] = 0.0, 3.0
    return w


# The optimizer of the post-step comparisons.  Adam's first step is lr * g / (|g| + epsilon / sqrt(1 - beta_2)): with
# keras's epsilon of 1e-7 that is lr * sign(g), and an element whose gradient passes through zero moves by up to lr
# whatever the size of the gradient's error - no bound on gradients carries to such a step, for the fp32 reference as
# for a kernel.  With epsilon = sqrt(1 - beta_2) the step is lr * g / (|g| + 1), Lipschitz lr in g: gradients inside
# the model bound, |dg| <= 2e-4 max|g|, give weights inside it, lr * 2e-4 max|g| <= 2e-4 max|w|, wherever
# lr * max|g| <= max|w| - which _check_post_step asserts of the fp64 reference for every tensor, along with steps that
# are themselves several times the bound (so the check sees them).
STEP_LR, STEP_EPS = 1e-2, float(np.sqrt(1.0 - 0.999))


def _check_post_step(names, before, after, grads, clipnorm):
    seen = 0
    for name in names:
        g = TO.clip_by_norm(np.asarray(grads[name], np.float64), clipnorm)
        want, _, _ = TO.adam_step(before[name], g, np.zeros_like(g), np.zeros_like(g), 1, lr=STEP_LR, eps=STEP_EPS)
        scale = np.abs(before[name]).max()
        assert STEP_LR * np.abs(g).max() <= scale, f"{name}: the step is not well conditioned against max|w|"
        seen += int(np.abs(want - before[name]).max() > 4 * MODEL_TOL * scale)
        assert_close(after[name], want, MODEL_TOL, f"post-step {name}")
        assert not np.array_equal(after[name], before[name]), name
    assert 2 * seen >= len(names), "most tensors move by several times the bound"


def _viscosity_oracle(w, inp, y, sw, loss="mse", delta=1.0, fp_l2=1e-4):
    wo = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in w.items()}
    e = TR.viscosity_forward(wo, inp, torch.float64).reshape(-1) - torch.tensor(y, dtype=torch.float64)
    per = e * e if loss == "mse" else R.huber(e, delta)
    lo = WR.weighted_batch_mean(per, torch.tensor(sw, dtype=torch.float64)) \
        + fp_l2 * ((wo["cat_fp/kernel"] ** 2).sum() + (wo["an_fp/kernel"] ** 2).sum())
    lo.backward()
    return wo, lo, e.detach().numpy()


def test_viscosity_train_on_batch_and_evaluate_with_weights_match_the_oracle():
    """A small viscosity model, batch 9 (a second, partial workgroup): the weighted loss and every gradient of
    _loss(sample_weight=w), then train_on_batch(sample_weight=w) - loss and post-step weights - and
    evaluate(sample_weight=w) over uneven batches, against fp64 at the whole-model bounds."""
    B = 9
    m, w, inp, y = _tiny_model()
    inp = {k: v[:B] for k, v in inp.items()}
    y = y[:B]
    sw = _model_weights(B, 1)
    m.compile(train.Adam(STEP_LR, epsilon=STEP_EPS, clipnorm=1.0))
    wo, lo, _ = _viscosity_oracle(w, inp, y, sw)
    loss = m._loss(m._to_device(inp), y, training=True, sample_weight=sw)
    loss.backward()
    m.join_training_streams()
    assert_close(_np(loss).reshape(1), _np(lo).reshape(1), VALUE_TOL, "weighted loss")
    for name, t in m.trainable_variables():
        assert_close(_np(t.grad), _np(wo[name].grad), MODEL_TOL, f"grad {name}")
    m.optimizer.zero_grad()
    # evaluate: forward only, batches of 4 + 4 + 1; the batch-size-weighted mean of weighted batch losses
    got = m.evaluate(m._to_device(inp), y, batch_size=4, sample_weight=sw)
    assert_close(np.array([got]), _np(lo).reshape(1), VALUE_TOL, "evaluate with weights")
    assert abs(m.evaluate(m._to_device(inp), y, batch_size=4) - got) > 1e-3 * got, "the weights change the value"
    step_loss = m.train_on_batch(inp, y, sample_weight=sw)
    assert_close(_np(step_loss).reshape(1), _np(lo).reshape(1), VALUE_TOL, "train_on_batch loss")
    names = [name for name, _ in m.trainable_variables()]
    _check_post_step(names, w, m.state_dict(), {n: _np(wo[n].grad) for n in names}, 1.0)


def test_viscosity_huber_on_the_unfused_path_matches_the_oracle():
    """A base model compiled with Huber takes train.Huber behind the layered head, not the fused node: the weighted loss
    and its gradients against fp64."""
    B = 9
    m, w, inp, y = _tiny_model()
    inp = {k: v[:B] for k, v in inp.items()}
    sw = _model_weights(B, 2)
    delta = 0.5
    with torch.no_grad():
        pred0 = TR.viscosity_forward({k: torch.tensor(v, dtype=torch.float64) for k, v in w.items()}, inp, torch.float64)
    off = np.where(np.arange(B) % 2 == 0, 2.5, 0.4) * delta * np.where(np.arange(B) % 3 == 0, -1.0, 1.0)
    y = (pred0.numpy().reshape(-1) - off).astype(F32)
    m.compile(train.Adam(1e-3, clipnorm=1.0), loss=train.Huber(delta))
    wo, lo, e = _viscosity_oracle(w, inp, y, sw, "huber", delta)
    assert (np.abs(e) > delta).any() and (np.abs(e) < delta).any() and np.abs(np.abs(e) / delta - 1.0).min() > FZ.KINK
    loss = m._loss(m._to_device(inp), y, training=True, sample_weight=sw)
    loss.backward()
    m.join_training_streams()
    assert_close(_np(loss).reshape(1), _np(lo).reshape(1), VALUE_TOL, "weighted Huber loss")
    for name, t in m.trainable_variables():
        assert_close(_np(t.grad), _np(wo[name].grad), MODEL_TOL, f"grad {name}")
    got = m.evaluate(m._to_device(inp), y, batch_size=5, sample_weight=sw)
    assert_close(np.array([got]), _np(lo).reshape(1), VALUE_TOL, "evaluate with weights, Huber")


def test_transfer_train_on_batch_and_evaluate_with_weights_match_the_oracle(tmp_path):
    """The transfer model (stage 2 of the reference's schedule: head and the last message-passing steps train):
    the gradients of _loss(sample_weight=w) and train_on_batch(sample_weight=w) against the fp64 reference with the
    step's Dropout mask - loss, post-step weights, moving statistics - and evaluate(sample_weight=w) with the moving
    statistics."""
    B = 9
    t = make_transfer(tmp_path, seed=3)
    stage2(t)
    t.compile(train.Adam(STEP_LR, epsilon=STEP_EPS), loss=train.Huber(delta=1.0))
    inp = synthetic.make_batch(B, seed=7)
    sw = _model_weights(B, 3)
    l2 = [1e-4, 0, 1e-4] + [0] * 15
    state = t.state_dict()
    w = R.leaves(state)
    mask = head_mask(9, B)
    with torch.no_grad():
        pred0, _, _ = R.head(w, *R.pooled(w, inp), True, mask)
    off = np.where(np.arange(B) % 2 == 0, 0.4, 2.5) * np.where(np.arange(B) % 3 == 0, -1.0, 1.0)
    y = (pred0.numpy() - off).astype(F32)
    # evaluate first (it changes nothing): inference statistics, no Dropout
    with torch.no_grad():
        lo_eval, e_eval, _, _, _ = WR.transfer_head_loss(w, *R.pooled(w, inp), y, l2, sw, False, None, 1.0, "huber")
    assert np.abs(np.abs(e_eval.numpy()) - 1.0).min() > 1e-3
    got = t.evaluate(t._to_device(inp), y, batch_size=4, sample_weight=sw)
    assert_close(np.array([got]), _np(lo_eval).reshape(1), VALUE_TOL, "evaluate with weights")
    lo, e, mm, mv, _ = WR.transfer_head_loss(w, *R.pooled(w, inp), y, l2, sw, True, mask, 1.0, "huber")
    assert np.abs(np.abs(e.detach().numpy()) - 1.0).min() > 1e-3
    lo.backward()
    trained = dict(t.trainable_variables())
    moving = t.mp_bn_1.moving_mean.clone(), t.mp_bn_1.moving_variance.clone()
    t.dropout_counter().fill_(9)
    pass_loss = t._loss(t._to_device(inp), y, training=True, sample_weight=sw)
    pass_loss.backward()
    t.join_training_streams()
    assert_close(_np(pass_loss).reshape(1), _np(lo).reshape(1), VALUE_TOL, "weighted loss")
    for name, tensor in trained.items():
        assert_close(_np(tensor.grad), _np(w[name].grad), MODEL_TOL, f"grad {name}")
    t.optimizer.zero_grad()
    with torch.no_grad():   # the same pass again as one step: the statistics and the step counter back where they were
        t.mp_bn_1.moving_mean.copy_(moving[0]), t.mp_bn_1.moving_variance.copy_(moving[1])
    t.dropout_counter().fill_(9)
    loss = t.train_on_batch(inp, y, sample_weight=sw)
    assert_close(_np(loss).reshape(1), _np(lo).reshape(1), VALUE_TOL, "train_on_batch loss")
    after = t.state_dict()
    _check_post_step(list(trained), state, after, {n: _np(w[n].grad) for n in trained}, None)
    for name in state:
        if name not in trained and "moving" not in name:
            assert np.array_equal(after[name], state[name]), f"frozen {name} moved"
    assert_close(after["mp_bn_1/moving_mean"], _np(mm), VALUE_TOL, "moving mean")
    assert_close(after["mp_bn_1/moving_variance"], _np(mv), VALUE_TOL, "moving variance")


def _fit_data():
    big = synthetic.make_batch(72, max_atoms=10, max_edges=16, atom_vocab_size=11, bond_vocab_size=6, min_atoms=3, seed=8)
    yb = np.random.default_rng(8).normal(1.0, 0.5, size=72).astype(F32)
    return big, yb


def test_weighted_resident_fit_follows_the_weighted_eager_fit():
    """fit(graph=True, sample_weight=w) - the captured step gathers the rows of the 8 batch tensors and, with a second
    launch, of the weights - walks the trajectory of fit(graph=False, sample_weight=w) on the same seed: the comparison
    and tolerance of tests/test_gpu_train.py::test_gather_rows_and_resident_fit_follow_the_eager_fit.  The weights are
    half bootstrap counts: the mean weight is 1/2 and the loss divides by B, not by sum(w), so the logged loss is about
    half the unweighted one."""
    from ionic_mpnn_amd import data
    big, yb = _fit_data()
    sw = 0.5 * data.bootstrap_weights(72, 4, groups=np.arange(72) // 3)
    assert (sw == 0).any() and (sw > 0.5).any() and abs(float(sw.mean()) - 0.5) < 1e-6
    hist, val = {}, {}
    for graph in (False, True, None):
        m, _, _, _ = _tiny_model()
        m.compile(train.Adam(1e-3, clipnorm=1.0))
        if graph is None:   # the unweighted fit, for contrast
            hist[graph] = m.fit(big, yb, epochs=3, batch_size=24, seed=5, graph=False).history["loss"]
            continue
        h = m.fit(big, yb, validation_data=(big, yb, sw), epochs=3, batch_size=24, seed=5, graph=graph,
                  sample_weight=sw).history
        hist[graph], val[graph] = h["loss"], h["val_loss"]
    np.testing.assert_allclose(hist[True], hist[False], rtol=2e-4)
    np.testing.assert_allclose(val[True], val[False], rtol=2e-4)
    assert 0.25 * hist[None][0] < hist[False][0] < 0.75 * hist[None][0], "the weights reach the training loss"


def test_captured_step_takes_weights_by_rows_and_by_value():
    """train.GraphedTrainStep with a static weight buffer: __call__(inputs, y, sample_weight) and step_on_rows(..., w_dev)
    follow train_on_batch(sample_weight=...) step by step; a step captured with weights refuses a call without them."""
    B = 24
    steps = {}
    for graphed in (False, True):
        m, _, inp, y = _tiny_model()
        m.compile(train.Adam(1e-3, clipnorm=1.0))
        x = m._to_device(inp)
        y_dev = torch.tensor(y, device=DEV).reshape(-1, 1)
        ws = [_model_weights(B, s) for s in (5, 6, 7)]
        rows = torch.arange(B - 1, -1, -1, device=DEV)
        if not graphed:
            out = [float(m.train_on_batch(x, y, sample_weight=w)) for w in ws[:2]]
            out.append(float(m.train_on_batch({k: v[rows] for k, v in x.items()}, y_dev[rows],
                                              sample_weight=torch.tensor(ws[2], device=DEV)[rows])))
        else:
            g = train.GraphedTrainStep(m, x, y, sample_weight=ws[0])
            out = [float(g(x, y, ws[0])), float(g(x, y, sample_weight=ws[1]))]
            out.append(float(g.step_on_rows(x, y_dev, rows, torch.tensor(ws[2], device=DEV))))
            with pytest.raises(ValueError):
                g(x, y)
            with pytest.raises(ValueError):
                g.step_on_rows(x, y_dev, rows)
        steps[graphed] = out
    np.testing.assert_allclose(steps[True], steps[False], rtol=2e-4)


def test_fit_without_weights_is_the_fit_it_was():
    """fit(..., sample_weight=None) against fit(...) on the same seed, graph=False, one process.  Bit equality of the
    trained weights is not a property the unweighted fit itself has - the parameter gradients of the head and of the
    encoder's backward kernels are float atomics over workgroups - so the two are held to the whole-model bound."""
    big, yb = _fit_data()
    out = {}
    for key, kw in (("plain", {}), ("none", dict(sample_weight=None))):
        m, _, _, _ = _tiny_model()
        m.compile(train.Adam(1e-3, clipnorm=1.0))
        h = m.fit(big, yb, epochs=2, batch_size=24, seed=5, graph=False, **kw).history["loss"]
        out[key] = (h, m.state_dict())
    assert_close(np.array(out["none"][0]), np.array(out["plain"][0]), MODEL_TOL, "loss history")
    for name, a in out["plain"][1].items():
        assert_close(out["none"][1][name], a, MODEL_TOL, f"trained {name}")


def _weighted_fit_rank(rank, world, port, out_dir):
    """One data-parallel rank of model.fit(sample_weight=...): ranks share cuda:0, gloo carries the collectives
    (tests/test_gpu_train.py::_fit_rank with weights)."""
    import os
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    os.environ.update({"RANK": str(rank), "LOCAL_RANK": "0", "WORLD_SIZE": str(world), "MASTER_ADDR": "127.0.0.1",
                       "MASTER_PORT": str(port), "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    from ionic_mpnn_amd import dist as idist
    idist.init_distributed(backend="gloo")
    m, _, inp, y = _tiny_model(S=1, seed=7)
    m.compile(train.Adam(1e-2, clipnorm=1.0))
    sub = {k: v[:23] for k, v in inp.items()}
    hist = m.fit(sub, y[:23], epochs=3, batch_size=10, seed=11 if rank == 0 else None,
                 sample_weight=0.5 * _model_weights(23, 9))
    np.savez(Path(out_dir) / f"fit_{rank}.npz", loss=np.array(hist.history["loss"]), **m.state_dict())
    torch.distributed.destroy_process_group()


def test_weighted_fit_under_torch_distributed_two_ranks(tmp_path):
    """The weights are cut with y (data.shard_bounds) and the n_local / n_global factor turns the shard means into the
    global (1/B) sum w L: two ranks end with identical weights and the logged loss of the single-process weighted fit -
    the comparison and tolerances of tests/test_gpu_train.py::test_fit_under_torch_distributed_two_ranks."""
    import socket
    import torch.multiprocessing as mp
    from test_gpu_train import close
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_weighted_fit_rank, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=240)
    for r, p in enumerate(procs):
        if p.is_alive():
            p.kill()
            pytest.fail(f"rank {r} hung")
        assert p.exitcode == 0, f"rank {r} exit code {p.exitcode}"
    a, b = np.load(tmp_path / "fit_0.npz"), np.load(tmp_path / "fit_1.npz")
    for k in a.files:
        assert np.array_equal(a[k], b[k]), f"ranks disagree on {k}"
    sub_w = 0.5 * _model_weights(23, 9)   # mean weight about 1/2: the loss divides by B, not by sum(w)
    out = {}
    for key, kw in (("weighted", dict(sample_weight=sub_w)), ("plain", {})):
        m, _, inp, y = _tiny_model(S=1, seed=7)
        m.compile(train.Adam(1e-2, clipnorm=1.0))
        out[key] = (m.fit({k: v[:23] for k, v in inp.items()}, y[:23], epochs=3, batch_size=10, seed=11, graph=False,
                          **kw).history["loss"], m.state_dict())
    close(a["loss"], np.array(out["weighted"][0]), 1e-4, "distributed vs single-process weighted loss history")
    for k in ("cat_gu_0/dense_z/kernel", "atom_embedding", "visc_params/kernel"):
        close(a[k], out["weighted"][1][k], 2e-3, f"distributed vs single-process {k}")
    assert out["weighted"][0][0] < 0.8 * out["plain"][0][0], "the weights reach the loss"
