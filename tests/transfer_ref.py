"""fp64 torch reference of the transfer model (train_melting_point_transfer.py:95-103) for tests/test_gpu_transfer.py:
oracle/torch_ref.py's encode() up to GlobalSumPool, then the head with tf.keras 2.12's BatchNormalization (momentum
0.99, epsilon 1e-3, biased batch variance in the normalisation and in the moving update), Dropout through a GIVEN mask
(scale where kept, 0 where dropped: tests/test_dropout_host.py's numpy Philox) and Huber / squared error."""
import numpy as np
import torch

from oracle import torch_ref as TR

DT = torch.float64
HEAD_LAYER_ID = 0xFFFF
BN_MOMENTUM, BN_EPS = 0.99, 1e-3


def leaves(state):
    """state_dict (numpy) -> fp64 leaf tensors that ask for a gradient."""
    return {k: torch.tensor(np.asarray(v), dtype=DT, requires_grad=True) for k, v in state.items()}


def huber(e, delta):
    a = e.abs()
    return torch.where(a <= delta, 0.5 * e * e, delta * (a - 0.5 * delta))


# the 18 tensors in the order of impnn_transfer_head's `weights` (include/impnn.h)
HEAD_TENSORS = ["cat_fp/kernel", "cat_fp/bias", "an_fp/kernel", "an_fp/bias", "cat_proj/kernel", "cat_proj/bias",
                "an_proj/kernel", "an_proj/bias", "mp_dense_1/kernel", "mp_dense_1/bias", "mp_bn_1/gamma", "mp_bn_1/beta",
                "mp_dense_2/kernel", "mp_dense_2/bias", "mp_dense_3/kernel", "mp_dense_3/bias", "melting_point/kernel",
                "melting_point/bias"]


def head(w, pc, pa, training=False, mask=None, bn_batch=None, trace=None):
    """-> (pred (B,), new moving mean, new moving variance).  bn_batch: batch statistics (default: ``training``);
    trace: a dict that receives every relu layer's pre-activations.  Runs in the dtype of ``w``."""
    def dense(x, n):
        z = x @ w[f"{n}/kernel"] + w[f"{n}/bias"]
        if trace is not None:
            trace[n] = z.detach()
        return z
    fc, fa = torch.relu(dense(pc, "cat_fp")), torch.relu(dense(pa, "an_fp"))
    mix = torch.relu(dense(fc, "cat_proj")) + torch.relu(dense(fa, "an_proj"))
    a1 = torch.relu(dense(mix, "mp_dense_1"))
    mm, mv = w["mp_bn_1/moving_mean"].detach(), w["mp_bn_1/moving_variance"].detach()
    if training if bn_batch is None else bn_batch:
        mean, var = a1.mean(0), a1.var(0, unbiased=False)
        mm = mm - (mm - mean.detach()) * (1.0 - BN_MOMENTUM)
        mv = mv - (mv - var.detach()) * (1.0 - BN_MOMENTUM)
    else:
        mean, var = mm, mv
    bn = (a1 - mean) / torch.sqrt(var + BN_EPS) * w["mp_bn_1/gamma"] + w["mp_bn_1/beta"]
    a2 = torch.relu(dense(bn, "mp_dense_2"))
    if training and mask is not None:
        a2 = a2 * torch.as_tensor(mask, dtype=a2.dtype)
    a3 = torch.relu(dense(a2, "mp_dense_3"))
    return dense(a3, "melting_point").reshape(-1), mm, mv


def pooled(w, inputs):
    return TR.pooled_pair(w, inputs, DT)


def loss(w, inputs, y, training=True, mask=None, delta=1.0, fp_l2=1e-4, kind="huber", bn_batch=None):
    """-> (loss, per-sample errors, moving mean, moving variance) of one pass of the whole model."""
    pc, pa = pooled(w, inputs)
    pred, mm, mv = head(w, pc, pa, training, mask, bn_batch)
    e = pred - torch.as_tensor(np.asarray(y, np.float64).reshape(-1))
    per = huber(e, delta) if kind == "huber" else e * e
    reg = fp_l2 * ((w["cat_fp/kernel"] ** 2).sum() + (w["an_fp/kernel"] ** 2).sum())
    return per.mean() + reg, e, mm, mv


def head_loss(w, pc, pa, y, l2, training=True, mask=None, delta=1.0, kind="huber", bn_batch=None, trace=None):
    """The head alone on given pooled vectors, one lambda per tensor of HEAD_TENSORS:
    -> (mean L(pred - y) + sum_t l2_t sum(W_t^2), per-sample errors, moving mean, moving variance)."""
    pred, mm, mv = head(w, pc, pa, training, mask, bn_batch, trace)
    e = pred - torch.as_tensor(y, dtype=pred.dtype).reshape(-1)
    per = huber(e, delta) if kind == "huber" else e * e
    reg = sum(float(lam) * (w[n] ** 2).sum() for n, lam in zip(HEAD_TENSORS, l2) if lam)
    return per.mean() + reg, e, mm, mv
