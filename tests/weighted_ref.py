"""The per-sample-weighted losses in plain torch, for tests/test_gpu_sample_weight.py and its CPU twin
tests/test_sample_weight_host.py, with the cases the two share.

  loss = (1/B) * sum_b w_b * L(pred_b - y_b) + sum_t l2[t] * sum(W_t^2)

keras's sum_over_batch_size: B counts every sample of the batch, those of weight 0 included; the penalties are not
weighted; BatchNormalization's statistics and the dropout mask do not see the weights.  The predictions come from
tests/head_ref.py::forward (model head) and tests/transfer_ref.py::head (transfer head), in the dtype of the tensors;
gradients are torch autograd's.

The kernel-level cases reuse the inputs of tests/test_gpu_head_fuzz.py: the model head's cases are that file's rows of
the same shape (its seeds included), the transfer head's are new rows of its ThCase with seeds chosen on the CPU so that
no relu pre-activation and no Huber |e| of the fp64 reference lies within a relative 1e-4 of its kink
(tests/test_sample_weight_host.py holds every case to that, none is skipped)."""
from collections import namedtuple

import numpy as np
import torch

import head_ref as HR
import test_gpu_head_fuzz as FZ
import transfer_ref as R

F32 = np.float32
SPB = FZ.HEAD_SPB   # samples of a workgroup, both heads


def weighted_batch_mean(per, w):
    """(1/B) sum_b w_b per_b."""
    return (torch.as_tensor(w, dtype=per.dtype).reshape(-1) * per.reshape(-1)).sum() / per.numel()


def model_head_loss(kind, w, pc, pa, T, y, l2, sw, trace=None):
    """-> (loss, pred, data term): head_ref's loss with the batch mean replaced by the weighted one."""
    pred = HR.forward(kind, w, pc, pa, T, trace)
    data = weighted_batch_mean((pred - y.reshape(-1)) ** 2, sw)
    reg = sum(float(lam) * (t ** 2).sum() for t, lam in zip(w, l2) if lam)
    return data + reg, pred, data


def transfer_head_loss(w, pc, pa, y, l2, sw, training=True, mask=None, delta=1.0, kind="huber", bn_batch=None, trace=None):
    """-> (loss, per-sample errors, moving mean, moving variance, data term): transfer_ref.head_loss, weighted."""
    pred, mm, mv = R.head(w, pc, pa, training, mask, bn_batch, trace)
    e = pred - torch.as_tensor(y, dtype=pred.dtype).reshape(-1)
    per = R.huber(e, delta) if kind == "huber" else e * e
    data = weighted_batch_mean(per, sw)
    reg = sum(float(lam) * (w[n] ** 2).sum() for n, lam in zip(R.HEAD_TENSORS, l2) if lam)
    return data + reg, e, mm, mv, data


# ---------------------------------------------------------------------------------------------------- weight patterns
PATTERNS = ("fractional", "counts", "zero workgroup", "zero last")


def patterns_for(B):
    """The patterns a batch can carry: a whole workgroup of zeros needs a second workgroup, a zero on the last live
    sample of a partial workgroup needs a partial one."""
    return [p for p in PATTERNS if (p != "zero workgroup" or B > SPB) and (p != "zero last" or B % SPB)]


def sample_weights(pattern, B, seed):
    """float32 (B): fractional in [0.25, 2); integer counts 0..3 (one sample at least counted); fractional with the
    middle workgroup of 8 samples at zero; fractional with a zero on the last sample."""
    rng = np.random.default_rng([seed, 3, B, PATTERNS.index(pattern)])
    w = F32(rng.uniform(0.25, 2.0, B))
    if pattern == "counts":
        w = F32(rng.integers(0, 4, B))
        if not w.any():
            w[0] = 2.0
    elif pattern == "zero workgroup":
        g = (-(-B // SPB) - 1) // 2
        w[g * SPB:(g + 1) * SPB] = 0.0
    elif pattern == "zero last":
        w[B - 1] = 0.0
    return w


# The weights' seed of a case whose own seed lets the weighted output-gradient seeds cancel (seed_sum_condition): the
# gradient of a one-element tensor (the output bias) is their plain sum, and a sum that cancels to a few percent of its
# terms has no relative 1e-4 in fp32, for the reference as for a kernel.
WEIGHT_SEEDS = {"B=7 widths 8 5 3 batch huber fractional": 2, "B=7 widths 8 5 3 frozen huber fractional": 2,
                "B=8 widths 8 5 3 batch mse counts": 1, "B=8 widths 8 5 3 frozen mse counts": 1,
                "B=9 widths 8 5 3 batch mse counts": 1, "B=9 widths 8 5 3 batch huber counts": 1,
                "B=9 widths 8 5 3 frozen mse counts": 1, "B=9 widths 8 5 3 frozen huber counts": 1}


def case_weights(wc):
    return sample_weights(wc.pattern, wc.base.B, WEIGHT_SEEDS.get(wc.name, wc.base.seed))


def seed_sum_condition(wc, terms):
    """terms: w_b * dL/dpred_b of the fp64 reference.  An fp32 sum of B terms errs by about 1e-7 * sum|terms|; held
    against |sum terms| >= 0.05 * sum|terms| that is 2e-6 relative, well inside the gradient bound."""
    terms = np.asarray(terms, np.float64)
    if not terms.any():
        return   # (every weight zero: B = 1 with a zero on the last sample - the sum is an exact zero)
    assert abs(terms.sum()) >= 0.05 * np.abs(terms).sum(), f"{wc.name}: the weighted gradient seeds cancel"


# ---------------------------------------------------------------------------------------------------- model head cases
# B = 1, 7, 8, 9: the edges of the 8-sample workgroup; 2049: the last workgroup's partial sum takes a second stride;
# 4097: backward workgroup 0 takes a second group; widths (64, 33, 64): the lane's second output
HEAD_ROWS = ("B=1", "B=7", "B=8", "B=9", "B=2049", "B=4097", "widths 64 33 64")
WCase = namedtuple("WCase", "name base pattern")


def model_head_cases():
    base = {c.name: c for c in FZ.model_head_cases()}
    out = []
    for row in HEAD_ROWS:
        for kind in (0, 1):
            c = base[f"{row} kind {kind}"]
            out += [WCase(f"{c.name} {p}", c, p) for p in patterns_for(c.B)]
    return out


def model_head_reference(wc, inp, sw, dtype):
    """-> loss (1,), data term, "grads" of FZ.DLOSS * loss (the weight tensors in order, dpooled_cat, dpooled_an), trace."""
    c = wc.base
    w = [torch.tensor(a, dtype=dtype, requires_grad=True) for a in inp["w"]]
    pc, pa = (torch.tensor(inp[k], dtype=dtype, requires_grad=True) for k in ("pc", "pa"))
    T, y = (torch.tensor(inp[k], dtype=dtype) for k in ("T", "y"))
    trace = {}
    lo, pred, data = model_head_loss(c.kind, w, pc, pa, T, y, inp["l2"], torch.tensor(sw, dtype=dtype), trace)
    (lo * FZ.DLOSS).backward()
    return dict(loss=FZ._np(lo).reshape(1), data=float(data.detach()), pred=FZ._np(pred),
                seeds=np.asarray(sw, np.float64) * 2.0 * (FZ._np(pred) - np.asarray(inp["y"], np.float64)),
                grads=[FZ._np(t.grad) for t in w + [pc, pa]], trace={k: FZ._np(v) for k, v in trace.items()})


def check_model_head(wc, got, ref):
    assert_close = FZ.assert_close
    assert_close(got["loss"], ref["loss"], FZ.VALUE_TOL, f"{wc.name}: loss")
    names = [f"tensor {i}" for i in range(len(ref["grads"]) - 2)] + ["dpooled_cat", "dpooled_an"]
    for n, a, e in zip(names, got["grads"], ref["grads"]):
        assert_close(a, e, FZ.GRAD_TOL, f"{wc.name}: {n}")


def model_head_kinks(wc, ref64):
    """No relu pre-activation and no clipped softplus value of the fp64 reference within FZ.KINK of its kink."""
    tr = ref64["trace"]
    for layer in ("cat_fp", "an_fp", "cat_proj", "an_proj") + (("hidden",) if wc.base.kind == 1 else ()):
        margin = FZ.relu_layer_state(tr[layer])[1]
        assert margin > FZ.KINK, f"{wc.name}: a pre-activation of {layer} within {margin:.1e} of its kink"
    if wc.base.kind == 0:
        assert FZ.clip_margin(tr["sp_b"], HR.B_CLIP) > FZ.KINK and FZ.clip_margin(tr["sp_c"], HR.C_CLIP) > FZ.KINK, wc.name
    seed_sum_condition(wc, ref64["seeds"])


# ---------------------------------------------------------------------------------------------------- transfer head cases
# loss and BatchNormalization mode; Dropout (rate 0.3) on the Huber passes of the small batches (a mask per sample makes
# every sample's mp_dense_3 pre-activations its own: beyond a few hundred samples some value always sits on a kink)
TH_SETTINGS = (("batch mse", 1, FZ.MSE), ("batch huber", 1, FZ.HUBER1), ("frozen mse", 0, FZ.MSE),
               ("frozen huber", 0, FZ.HUBER025))
TH_SHAPES = ((1, (8, 5, 3)), (7, (8, 5, 3)), (8, (8, 5, 3)), (9, (8, 5, 3)), (2049, (8, 5, 3)), (4097, (8, 5, 3)),
             (9, (64, 33, 64)))
# the seed of a (shape, setting) whose seed 0 puts a value of the fp64 reference within 1e-4 of a kink
TH_SEEDS = {f"B={B} widths {w} {s}": seed for B, w, seed in ((4097, "8 5 3", 3), (9, "64 33 64", 1))
            for s, _, _ in TH_SETTINGS}


def _th_base(B, widths, setting, bn, loss):
    D, F, Mx = widths
    name = f"B={B} widths {D} {F} {Mx} {setting}"
    rate = 0.3 if loss[0] == "huber" and B <= 9 else 0.0
    head = (name, B, D, F, Mx, bn, loss, rate, FZ.KERAS_L2, False, "everything")
    br = FZ.transfer_branch(FZ.ThCase(*head, None, None, None, None, None, 0))
    return FZ.ThCase(*head, br.loss_sum, br.stats, br.flags, br.jobs, br.dense, TH_SEEDS.get(name, 0))


def transfer_bases():
    return [_th_base(B, widths, s, bn, loss) for B, widths in TH_SHAPES for s, bn, loss in TH_SETTINGS]


def transfer_cases():
    return [WCase(f"{c.name} {p}", c, p) for c in transfer_bases() for p in patterns_for(c.B)]


def transfer_reference(wc, inp, sw, dtype):
    """The training pass of the case, weighted: loss, data term, errors, moving statistics, the gradients of
    FZ.DLOSS * loss for every tensor that asks (a frozen BatchNormalization: not gamma / beta) and the pooled vectors."""
    c = wc.base
    want = FZ.asked(c)
    w, pc, pa = FZ._transfer_tensors(inp, dtype, want)
    trace = {}
    lo, e, mm, mv, data = transfer_head_loss(w, pc, pa, inp["y"], inp["l2"], torch.tensor(sw, dtype=dtype), True,
                                             FZ.transfer_mask(c), c.loss[1], c.loss[0], bool(c.bn), trace)
    (lo * FZ.DLOSS).backward()
    grads = {t: FZ._np(w[R.HEAD_TENSORS[t]].grad if w[R.HEAD_TENSORS[t]].grad is not None
                       else torch.zeros_like(w[R.HEAD_TENSORS[t]])) for t in want if t != "pooled"}
    e64 = FZ._np(e)
    lgrad = 2.0 * e64 if c.loss[0] == "mse" else np.clip(e64, -c.loss[1], c.loss[1])
    return dict(loss=FZ._np(lo).reshape(1), data=float(data.detach()), e=e64, mm=FZ._np(mm), mv=FZ._np(mv), grads=grads,
                seeds=np.asarray(sw, np.float64) * lgrad,
                dpooled=[FZ._np(pc.grad), FZ._np(pa.grad)],
                trace={k: FZ._np(v) for k, v in trace.items() if k != "melting_point"})


def check_transfer(wc, got, ref):
    assert_close = FZ.assert_close
    assert_close(got["loss"], ref["loss"], FZ.VALUE_TOL, f"{wc.name}: loss")
    assert_close(got["mm"], ref["mm"], FZ.VALUE_TOL, f"{wc.name}: moving mean")
    assert_close(got["mv"], ref["mv"], FZ.VALUE_TOL, f"{wc.name}: moving variance")
    assert set(got["grads"]) == set(ref["grads"]), wc.name
    for t, e in ref["grads"].items():
        assert_close(got["grads"][t], e, FZ.GRAD_TOL, f"{wc.name}: gradient of tensor {t} ({R.HEAD_TENSORS[t]})")
    for n, a, e in zip(("cat", "an"), got["dpooled"], ref["dpooled"]):
        assert_close(a, e, FZ.GRAD_TOL, f"{wc.name}: dpooled_{n}")


def transfer_kinks(wc, ref64):
    """No relu pre-activation and no Huber |e| of the fp64 reference within FZ.KINK of its kink."""
    for layer, z in ref64["trace"].items():
        margin = FZ.relu_layer_state(z)[1]
        assert margin > FZ.KINK, f"{wc.name}: a pre-activation of {layer} within {margin:.1e} of its kink"
    if wc.base.loss[0] == "huber":
        assert np.abs(np.abs(ref64["e"]) / wc.base.loss[1] - 1.0).min() > FZ.KINK, f"{wc.name}: an |e| on Huber's kink"
    seed_sum_condition(wc, ref64["seeds"])
