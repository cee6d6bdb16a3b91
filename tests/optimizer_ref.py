"""Reference of the scheduled optimizer step (impnn_adam_step_scheduled), restated from the published Keras / TensorFlow
definitions and independent of ionic_mpnn_amd.train:

  * ``schedule_rate(spec, s, dtype)``: the learning rate of update number ``s`` (updates already applied).  In float64 it
    is the definition; in float32 it is the same formula with every operand and operation in float32, whose error
    against float64 on a grid of steps sets the bound of the device comparison (``f32_error``).
  * ``adam_update``: one update of a set of variables in float64 - tf.clip_by_norm per variable or
    tf.clip_by_global_norm over all of them, keras's decoupled weight decay, then Adam.

A spec is a dict: {"kind": "constant", "lr"}, {"kind": "exponential", "lr0", "decay_steps", "decay_rate", "staircase"},
{"kind": "cosine", "lr0", "decay_steps", "alpha", "warmup_target", "warmup_steps"} or {"kind": "piecewise",
"boundaries", "values"}."""
import numpy as np


def schedule_rate(spec, s, dtype=np.float64):
    f = dtype
    kind = spec["kind"]
    if kind == "constant":
        return f(spec["lr"])
    if kind == "exponential":
        p = f(s) / f(spec["decay_steps"])
        if spec.get("staircase"):
            p = np.floor(p)
        return f(spec["lr0"]) * np.power(f(spec["decay_rate"]), p)
    if kind == "cosine":
        lr0 = f(spec["lr0"])
        target = lr0 if spec.get("warmup_target") is None else f(spec["warmup_target"])
        warm = 0 if spec.get("warmup_target") is None else int(spec.get("warmup_steps", 0))
        if s < warm:
            return (target - lr0) * (f(s) / f(warm)) + lr0
        frac = f(min(s - warm, spec["decay_steps"])) / f(spec["decay_steps"])
        alpha = f(spec.get("alpha", 0.0))
        return target * ((f(1) - alpha) * (f(0.5) * (f(1) + np.cos(f(np.pi) * frac))) + alpha)
    if kind == "piecewise":
        for b, v in zip(spec["boundaries"], spec["values"]):
            if s <= b:
                return f(v)
        return f(spec["values"][-1])
    raise ValueError(kind)


def rel_err(got, want):
    """|got - want| / |want| (0 where both are 0): the error measure of the schedule comparisons."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = np.abs(got - want)
    return np.where(d == 0, 0.0, d / np.maximum(np.abs(want), 1e-300))


def f32_error(spec, steps):
    """The largest relative error of the float32 restatement against float64 over ``steps``."""
    want = [schedule_rate(spec, s) for s in steps]
    got = [schedule_rate(spec, s, np.float32) for s in steps]
    return float(rel_err(got, want).max())


def global_norm(gs):
    return float(np.sqrt(sum(np.sum(np.asarray(g, np.float64) ** 2) for g in gs)))


def clip_scales(gs, clipnorm=None, global_clipnorm=None):
    """One scale per variable: tf.clip_by_norm, or tf.clip_by_global_norm (NaN for a non-finite global norm)."""
    if global_clipnorm is not None:
        n = global_norm(gs)
        s = global_clipnorm / max(n, global_clipnorm) if np.isfinite(n) else np.nan
        return [s] * len(gs)
    if clipnorm is None:
        return [1.0] * len(gs)
    return [clipnorm / max(global_norm([g]), clipnorm) for g in gs]


def adam_update(ws, gs, ms, vs, t, lr, b1=0.9, b2=0.999, eps=1e-7, clipnorm=None, global_clipnorm=None,
                weight_decay=None, decays=None):
    """Update number ``t`` (counted from 1) with the rate ``lr`` of that step.  Returns (ws, ms, vs) in float64."""
    scales = clip_scales(gs, clipnorm, global_clipnorm)
    alpha = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    out = []
    for i, (w, g, m, v) in enumerate(zip(ws, gs, ms, vs)):
        w, g, m, v = (np.asarray(a, np.float64) for a in (w, g, m, v))
        with np.errstate(invalid="ignore"):
            g = g * scales[i]
            if weight_decay and (decays is None or decays[i]):
                w = w - lr * weight_decay * w
            m = b1 * m + (1.0 - b1) * g
            v = b2 * v + (1.0 - b2) * g * g
            out.append((w - alpha * m / (np.sqrt(v) + eps), m, v))
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]
