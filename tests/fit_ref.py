"""An independent trainer: ``MPNNModel.fit``'s contract, restated from its docstring on the torch-CPU references the
other fuzz tests already hold against the kernels one by one (tests/test_gpu_fit_fuzz.py, tests/test_fit_ref_host.py).

Nothing of ionic_mpnn_amd.model, .train, .ops or .autograd is used here: the loss is tests/grad_ref.py's encoder with
tests/head_ref.py's or tests/transfer_ref.py's head, gradients are torch autograd's, the rate is
tests/optimizer_ref.py's ``schedule_rate``, the masks are tests/philox_ref.py's numpy Philox.  What this file
adds is the string that ties them into a run:

  * per epoch ``np.random.default_rng(seed).permutation(n)`` (one generator for the run; ``arange`` without shuffle),
    batches ``order[lo:lo + bs]``, the last one smaller, logged ``loss`` = sum len * batch_loss / n;
  * batch loss = keras mean of the per-sample MSE / Huber, or (1/B) sum_b w_b L_b with sample weights (B counts the
    samples of weight 0 too), plus the l2 penalties; the transfer head with batch-statistics BatchNormalization, its
    moving update carried from step to step, and the head's Dropout mask;
  * the dropout counter starts at 0 and every training pass uses its value and advances it by one;
  * per-variable or global clip over the trainable variables, decoupled decay with the exclusion list matched on the
    variables' names, Adam with t counted over all steps at the rate ``schedule_rate(spec, t - 1)`` or the rate a
    per-epoch scheduler function set; frozen variables get no update;
  * the epoch's running metrics from every step's training-pass predictions, validation from an inference pass over
    the validation set after the epoch, EarlyStopping(restore_best_weights=True).

``run(case, dtype)``: float64 is the reference; float32 runs loss, gradients and optimizer arithmetic in float32 and is
the attainability probe.  ``knock`` names one deliberate defect (KNOCKOUTS) for the "reference is alive" test."""
import numpy as np
import torch

import grad_ref as GR
import head_ref as HR
import optimizer_ref as OR
import transfer_ref as R
from oracle import torch_ref as TR
from philox_ref import reference_mask

HEAD_DROPOUT_RATE, HEAD_WIDTH = 0.3, 128   # mp_dropout behind mp_dense_2 (train_melting_point_transfer.py:95-103)
MOVING = ("mp_bn_1/moving_mean", "mp_bn_1/moving_variance")
VISC_HEAD = ["cat_fp/kernel", "cat_fp/bias", "an_fp/kernel", "an_fp/bias", "cat_proj/kernel", "cat_proj/bias",
             "an_proj/kernel", "an_proj/bias", "visc_params/kernel", "visc_params/bias"]
MP_HEAD = VISC_HEAD[:8] + ["mp_hidden/kernel", "mp_hidden/bias", "mp_out/kernel", "mp_out/bias"]
B1, B2, EPS = 0.9, 0.999, 1e-7

# one deliberate defect each (tests/test_fit_ref_host.py: the reference must notice every one of them)
KNOCKOUTS = ("rotate_order", "drop_remainder", "adam_t_off", "schedule_off", "dropout_stuck", "moving_not_carried",
             "weights_metrics_only", "decay_excluded", "norm_over_frozen")


def weighted_batch_mean(per, w):
    """(1/B) sum_b w_b per_b (tests/weighted_ref.py's, which tests/test_fit_ref_host.py holds equal to this one)."""
    return (torch.as_tensor(w, dtype=per.dtype).reshape(-1) * per.reshape(-1)).sum() / per.numel()


def _sl(x, idx):
    return {k: np.asarray(v)[idx] for k, v in x.items()}


class _Pass:
    """One forward pass of the case's model on a batch: predictions, per-sample errors, traces."""

    def __init__(self, case, w, x, dtype, training, step, state):
        self.trace, self.moving = {}, None
        S, D = case.dims["S"], case.dims["D"]
        B, N = np.asarray(x["cat_atom"]).shape
        gu = None
        if training and case.dropout is not None:
            rate, seed = case.dropout
            calls = []

            def gu(h, agg, p, eps=1e-3):   # cation step i: layer i, anion step i: layer S + i (the order of the calls)
                k = len(calls)
                calls.append(k)
                m = reference_mask(seed, step, k, rate, h.shape[0] * h.shape[1], D)
                return TR.gated_update(h, agg, p, eps) * torch.tensor(m, dtype=h.dtype).view(h.shape)
        pc = GR.encode(w, "cat", x["cat_atom"], x["cat_bond"], x["cat_connectivity"], dtype, True, gu)
        pa = GR.encode(w, "an", x["an_atom"], x["an_bond"], x["an_connectivity"], dtype, True, gu)
        if gu is not None:
            assert len(calls) == 2 * S
        if case.kind == "transfer":
            mask = None
            if training:
                mask = reference_mask(case.head_dropout_seed, step, R.HEAD_LAYER_ID, HEAD_DROPOUT_RATE, B, HEAD_WIDTH)
            hw = dict(w, **{k: torch.as_tensor(state[k], dtype=dtype) for k in MOVING})
            self.pred, mm, mv = R.head(hw, pc, pa, training, mask, training and case.bn_trains, self.trace)
            self.moving = {MOVING[0]: mm, MOVING[1]: mv}
        else:
            names = VISC_HEAD if case.kind == "viscosity" else MP_HEAD
            T = torch.as_tensor(np.asarray(x["temperature"]), dtype=dtype) if case.kind == "viscosity" else None
            self.pred = HR.forward(HR.KINDS[case.kind], [w[n] for n in names], pc, pa, T, self.trace)


def batch_loss(case, w, ps, y, sw, dtype):
    """-> (loss, per-sample errors) of a pass ``ps``: the data term (weighted or not) plus the l2 penalties."""
    e = ps.pred.reshape(-1) - torch.as_tensor(np.asarray(y), dtype=dtype).reshape(-1)
    per = e * e if case.loss[0] == "mse" else R.huber(e, case.loss[1])
    data = per.mean() if sw is None else weighted_batch_mean(per, torch.as_tensor(np.asarray(sw), dtype=dtype))
    return data + case.fp_l2 * sum((w[n] ** 2).sum() for n in penalised(case)), e


def penalised(case):
    """The kernels that carry keras's l2 penalty."""
    return ["cat_fp/kernel", "an_fp/kernel"] + (["mp_hidden/kernel"] if case.kind == "melting_point" else [])


def metric_values(specs, pred, y, sw, prefix=""):
    """{key: value} of metric specs [(name, scale, offset)] over predictions / targets / weights (None: unweighted),
    the formulas of ionic_mpnn_amd.train's metric classes in fp64: e = scale (pred - y), yr = offset + scale y."""
    p, t = np.asarray(pred, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    w = np.ones_like(p) if sw is None else np.asarray(sw, np.float64).reshape(-1)
    out = {}
    for name, scale, offset in specs:
        e, yr, s1 = scale * (p - t), offset + scale * t, w.sum()
        mean = lambda v: float((w * v).sum() / s1) if s1 != 0.0 else 0.0
        if name == "mae":
            v = mean(np.abs(e))
        elif name == "mse":
            v = mean(e * e)
        elif name == "rmse":
            v = float(np.sqrt(mean(e * e)))
        elif name == "bias":
            v = mean(e)
        elif name == "max_error":
            live = np.abs(e)[w > 0]
            v = float(live.max()) if live.size else 0.0
        elif name == "r2":
            v = 0.0 if s1 == 0.0 else float(1.0 - (w * e * e).sum() / (
                (w * yr * yr).sum() - (w * yr).sum() ** 2 / s1 + 1e-6))
        else:
            raise ValueError(name)
        out[prefix + name] = v
    return out


def adam_apply(case, names, w, grads, m, v, t, lr, dtype, knock=None, frozen_grads=()):
    """Update number ``t`` (from 1) of the trainable variables ``names`` in place, all arithmetic in ``dtype``."""
    opt = case.opt
    f = lambda a: torch.tensor(a, dtype=dtype)
    norms = {n: torch.sqrt((grads[n] ** 2).sum()) for n in names}
    if opt.get("global_clipnorm") is not None:
        sq = sum(norms[n] ** 2 for n in names)
        if knock == "norm_over_frozen":
            sq = sq + sum((g ** 2).sum() for g in frozen_grads)
        c = f(opt["global_clipnorm"])
        gn = torch.sqrt(sq)
        scales = {n: c / torch.maximum(gn, c) for n in names}
        clipped = bool(gn > c)
    elif opt.get("clipnorm") is not None:
        c = f(opt["clipnorm"])
        scales = {n: c / torch.maximum(norms[n], c) for n in names}
        clipped = any(bool(norms[n] > c) for n in names)
    else:
        scales, clipped = {n: f(1.0) for n in names}, False
    lr = f(lr)
    alpha = lr * torch.sqrt(1.0 - f(B2) ** t) / (1.0 - f(B1) ** t)
    wd = opt.get("weight_decay")
    for n in names:
        g = grads[n] * scales[n]
        decays = wd and (knock == "decay_excluded" or not any(s in n for s in opt.get("exclude", ())))
        with torch.no_grad():
            if decays:
                w[n] -= lr * f(wd) * w[n]
            m[n] = f(B1) * m[n] + (1.0 - f(B1)) * g
            v[n] = f(B2) * v[n] + (1.0 - f(B2)) * g * g
            w[n] -= alpha * m[n] / (torch.sqrt(v[n]) + f(EPS))
    return clipped


def step_rate(case, s, dtype, epoch_rate=None):
    """The rate of update number ``s`` (updates already applied): the schedule's, or the one the epoch's callback set."""
    if epoch_rate is not None:
        return float(epoch_rate)
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    return float(OR.schedule_rate(case.opt["lr"], s, np_dtype))


def run(case, dtype=torch.float64, knock=None, max_epochs=None, collect=None):
    """The whole fit of ``case`` -> dict(history, weights, m, v, iterations, rates, moving, dropout_steps, clipped,
    stopped_epoch).  ``collect``: a list that receives one dict per training step (rows, pred, errors, traces, loss, gradients, the l2 penalties' share of them)."""
    import fit_cases as FC
    assert knock is None or knock in KNOCKOUTS or knock.startswith("off:"), knock
    if knock is not None and knock.startswith("off:"):
        case, knock = FC.option_off(case, knock[4:]), None
    x, y, sw, val = FC.case_data(case)
    w0 = FC.case_weights(case)
    state = {k: np.asarray(w0[k], np.float64) for k in MOVING if k in w0}
    if dtype != torch.float64:
        state = {k: v.astype(np.float32) for k, v in state.items()}
    trainable = [n for n in w0 if n not in MOVING and FC.trainable(case, n)]
    w = {n: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=n in trainable) for n, a in w0.items()
         if n not in MOVING}
    if knock == "norm_over_frozen":   # (the defect needs the frozen variables' gradients)
        for n in w:
            w[n].requires_grad_(True)
    m = {n: torch.zeros_like(w[n]) for n in trainable}
    v = {n: torch.zeros_like(w[n]) for n in trainable}
    n, bs = len(y), case.batch
    rng = np.random.default_rng(case.seed)
    hist, rates, clipped = {}, [], []
    t = drop_step = 0
    eager_seen = False
    epoch_rate = None
    best = dict(value=np.inf, weights=None, wait=0)
    stopped_epoch = None
    loss_sw = None if knock == "weights_metrics_only" else sw
    for epoch in range(case.epochs if max_epochs is None else max_epochs):
        if case.epoch_rate is not None:
            lr0, factor = case.epoch_rate
            epoch_rate = lr0 * factor ** epoch
        order = rng.permutation(n) if case.shuffle else np.arange(n)
        if knock == "rotate_order":
            order = np.roll(order, -1)
        tot, preds, rows = 0.0, [], []
        for lo in range(0, n, bs):
            idx = order[lo:lo + bs]
            if knock == "drop_remainder" and len(idx) < bs:
                continue
            ps = _Pass(case, w, _sl(x, idx), dtype, True, drop_step, state)
            loss, e = batch_loss(case, w, ps, y[idx], None if loss_sw is None else loss_sw[idx], dtype)
            names = list(w) if knock == "norm_over_frozen" else trainable
            grads = dict(zip(names, torch.autograd.grad(loss, [w[k] for k in names], allow_unused=True)))
            grads = {k: torch.zeros_like(w[k]) if g is None else g for k, g in grads.items()}
            penalty = {k: (2.0 * case.fp_l2 * w[k].detach()).numpy().copy() for k in penalised(case) if k in grads}
            if ps.moving is not None and knock != "moving_not_carried":
                state = {k: a.detach().numpy().copy() for k, a in ps.moving.items()}
            if knock != "dropout_stuck":
                drop_step += 1
            t += 1
            off = 1 if eager_seen else 0   # the two step-index defects set in behind the first eager (smaller) batch
            lr = step_rate(case, t - 1 + (off if knock == "schedule_off" else 0), dtype, epoch_rate)
            rates.append(lr)
            clipped.append(adam_apply(case, trainable, w, grads, m, v, t + (off if knock == "adam_t_off" else 0), lr,
                                      dtype, knock, [grads[k] for k in names if k not in trainable]))
            eager_seen = eager_seen or len(idx) < bs
            tot += len(idx) * float(loss.detach())
            preds.append(ps.pred.detach().numpy().astype(np.float64).reshape(-1))
            rows.append(idx)
            if collect is not None:
                collect.append(dict(epoch=epoch, rows=idx, pred=preds[-1], e=e.detach().numpy().astype(np.float64),
                                    loss=float(loss.detach()), trace={k: z.numpy() for k, z in ps.trace.items()},
                                    grads={k: g.numpy().copy() for k, g in grads.items()}, penalty=penalty, lr=lr, t=t))
        logs = {"loss": tot / max(n, 1)}
        seen = np.concatenate(rows)
        pr = np.concatenate(preds)
        logs.update(metric_values(case.metrics, pr, y[seen], None))
        logs.update(metric_values(case.weighted_metrics, pr, y[seen], None if sw is None else sw[seen], "weighted_"))
        if val is not None:
            vx, vy, vw = val
            with torch.no_grad():
                ps = _Pass(case, w, vx, dtype, False, None, state)
                vloss, _ = batch_loss(case, w, ps, vy, vw, dtype)
            vp = ps.pred.numpy().astype(np.float64).reshape(-1)
            logs["val_loss"] = float(vloss)
            logs.update(metric_values(case.metrics, vp, vy, None, "val_"))
            logs.update(metric_values(case.weighted_metrics, vp, vy, vw, "val_weighted_"))
        for k, val_k in logs.items():
            hist.setdefault(k, []).append(float(val_k))
        if case.early_stop is not None:   # keras EarlyStopping(val_loss, patience, restore_best_weights=True)
            snap = lambda: ({k: a.detach().clone() for k, a in w.items()}, {k: a.copy() for k, a in state.items()})
            if best["weights"] is None:
                best["weights"] = snap()
            best["wait"] += 1
            if logs["val_loss"] < best["value"]:
                best.update(value=logs["val_loss"], weights=snap(), wait=0)
            elif best["wait"] >= case.early_stop["patience"] and epoch > 0:
                stopped_epoch = epoch
                break
    if case.early_stop is not None and best["weights"] is not None:
        with torch.no_grad():
            for k, a in best["weights"][0].items():
                w[k].copy_(a)
        state = best["weights"][1]
    num = lambda a: a.detach().numpy().astype(np.float64)
    return dict(history=hist, weights={k: num(a) for k, a in w.items()}, m={k: num(a) for k, a in m.items()},
                v={k: num(a) for k, a in v.items()}, iterations=t, rates=rates, dropout_steps=drop_step,
                moving={k: np.asarray(a, np.float64) for k, a in state.items()}, clipped=clipped,
                stopped_epoch=stopped_epoch, trainable=trainable, initial={k: np.asarray(a, np.float64) for k, a in w0.items()})
