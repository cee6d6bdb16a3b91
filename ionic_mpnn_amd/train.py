"""model.compile / fit / evaluate as the reference's trainers use them:
Adam(1e-3, clipnorm=1.0) + MSE (+ the l2(1e-4) penalty of the fingerprint Dense kernels), mini-batches of
32 in a fresh shuffle per epoch, EarlyStopping(monitor="val_loss", patience=50, restore_best_weights=True)
(train_viscosity.py:189,227-230,328-338; train_melting_point.py:173,205-208,300-311).

Forward and backward of the message-passing layers run in libimpnn (ionic_mpnn_amd.autograd); the
optimizer step of all variables is one launch (impnn_adam_step_scheduled); the head after GlobalSumPool, the
mse and the l2 penalties are one node too (impnn_model_head_loss[_bwd]) - torch.autograd only keeps the graph, no
torch arithmetic kernel runs in a step.  Multi-GPU: one process per GPU, every rank takes
its contiguous shard of each mini-batch, and the flat gradient buffer is averaged with ONE all-reduce
per step (RCCL; gloo in the CPU tests) before the replicated optimizer step."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, stream_ptr


# ---- learning-rate schedules (keras.optimizers.schedules).  __call__(step) in float64 on the host is the definition;
# the optimizer kernel evaluates the same formula in float32 from a 32-word device record (include/impnn.h,
# impnn_adam_step_scheduled), ``step`` being the number of updates already applied.
LR_RECORD_WORDS, LR_MAX_BOUNDARIES = 32, 8
LR_CONSTANT, LR_EXPONENTIAL, LR_COSINE, LR_PIECEWISE = 0, 1, 2, 3


def _lr_record(kind, lr0, flags=0, param=0.0, decay_steps=0, warmup_steps=0, target=0.0, boundaries=(), values=()):
    rec = np.zeros(LR_RECORD_WORDS, np.int32)
    f = rec.view(np.float32)
    rec[0], rec[1], rec[4], rec[5], rec[7] = kind, flags, decay_steps, warmup_steps, len(boundaries)
    f[2], f[3], f[6] = lr0, param, target
    rec[8:8 + len(boundaries)] = boundaries
    f[16:16 + len(values)] = values
    return rec


def _finite(x, what):
    x = float(x)
    if not np.isfinite(x):
        raise ValueError(f"{what} must be finite, got {x}")
    return x


def _steps(x, what, low):
    if int(x) != x or not low <= int(x) < 2 ** 31:
        raise ValueError(f"{what} must be an integer >= {low} (and below 2^31), got {x!r}")
    return int(x)


class LearningRateSchedule:
    """Base of the schedules: ``__call__(step)`` -> rate (float64), ``get_config`` / ``from_config``, and ``_record()``,
    the device record of the schedule."""

    def __call__(self, step):
        raise NotImplementedError

    def get_config(self):
        raise NotImplementedError

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class ExponentialDecay(LearningRateSchedule):
    """keras ExponentialDecay: lr0 * decay_rate ** (step / decay_steps), floor(step / decay_steps) with staircase."""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name="ExponentialDecay"):
        self.initial_learning_rate = _finite(initial_learning_rate, "initial_learning_rate")
        self.decay_steps = _steps(decay_steps, "decay_steps", 1)
        self.decay_rate = _finite(decay_rate, "decay_rate")
        if self.decay_rate < 0.0:
            raise ValueError(f"decay_rate must be >= 0, got {self.decay_rate}")
        self.staircase, self.name = bool(staircase), name

    def __call__(self, step):
        p = float(step) / float(self.decay_steps)
        return self.initial_learning_rate * self.decay_rate ** (np.floor(p) if self.staircase else p)

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps,
                "decay_rate": self.decay_rate, "staircase": self.staircase, "name": self.name}

    def _record(self):
        return _lr_record(LR_EXPONENTIAL, self.initial_learning_rate, flags=int(self.staircase), param=self.decay_rate,
                          decay_steps=self.decay_steps)


class CosineDecay(LearningRateSchedule):
    """keras CosineDecay: with ``warmup_target`` a linear warm-up from initial_learning_rate to warmup_target over
    ``warmup_steps``, then, from ``target`` (warmup_target, or initial_learning_rate without one),
    target * ((1 - alpha) * 0.5 * (1 + cos(pi * min(step', decay_steps) / decay_steps)) + alpha), step' counted from the
    end of the warm-up."""

    def __init__(self, initial_learning_rate, decay_steps, alpha=0.0, name="CosineDecay", warmup_target=None,
                 warmup_steps=0):
        self.initial_learning_rate = _finite(initial_learning_rate, "initial_learning_rate")
        self.decay_steps = _steps(decay_steps, "decay_steps", 1)
        self.alpha, self.name = _finite(alpha, "alpha"), name
        self.warmup_target = None if warmup_target is None else _finite(warmup_target, "warmup_target")
        self.warmup_steps = _steps(warmup_steps, "warmup_steps", 0)

    def _warmup(self):
        return self.warmup_steps if self.warmup_target is not None else 0

    def __call__(self, step):
        step, warm = float(step), self._warmup()
        target = self.initial_learning_rate if self.warmup_target is None else self.warmup_target
        if step < warm:
            return (target - self.initial_learning_rate) * (step / warm) + self.initial_learning_rate
        frac = min(step - warm, float(self.decay_steps)) / float(self.decay_steps)
        return target * ((1.0 - self.alpha) * 0.5 * (1.0 + np.cos(np.pi * frac)) + self.alpha)

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps,
                "alpha": self.alpha, "name": self.name, "warmup_target": self.warmup_target,
                "warmup_steps": self.warmup_steps}

    def _record(self):
        target = self.initial_learning_rate if self.warmup_target is None else self.warmup_target
        return _lr_record(LR_COSINE, self.initial_learning_rate, param=self.alpha, decay_steps=self.decay_steps,
                          warmup_steps=self._warmup(), target=target)


class PiecewiseConstantDecay(LearningRateSchedule):
    """keras PiecewiseConstantDecay: values[i] while step <= boundaries[i], the last value after the last boundary; at
    most 8 boundaries (the device record holds no more)."""

    def __init__(self, boundaries, values, name="PiecewiseConstant"):
        self.boundaries = [_steps(b, "a boundary", 0) for b in boundaries]
        self.values = [_finite(v, "a value") for v in values]
        self.name = name
        if len(self.values) != len(self.boundaries) + 1:
            raise ValueError("values must have one element more than boundaries")
        if len(self.boundaries) > LR_MAX_BOUNDARIES:
            raise ValueError(f"at most {LR_MAX_BOUNDARIES} boundaries, got {len(self.boundaries)}")
        if any(a >= b for a, b in zip(self.boundaries, self.boundaries[1:])):
            raise ValueError("boundaries must increase")

    def __call__(self, step):
        for b, v in zip(self.boundaries, self.values):
            if step <= b:
                return v
        return self.values[-1]

    def get_config(self):
        return {"boundaries": list(self.boundaries), "values": list(self.values), "name": self.name}

    def _record(self):
        return _lr_record(LR_PIECEWISE, self.values[0], boundaries=self.boundaries, values=self.values)


_SCHEDULES = {c.__name__: c for c in (ExponentialDecay, CosineDecay, PiecewiseConstantDecay)}


def _checked_rate(value):
    """A learning rate as the optimizer keeps it: a schedule object as it is, anything else as a finite float."""
    return value if isinstance(value, LearningRateSchedule) else _finite(value, "learning_rate")


class Adam:
    """keras.optimizers.Adam(learning_rate, clipnorm): per-variable tf.clip_by_norm, then Adam with
    epsilon 1e-7 and the bias-corrected step size lr*sqrt(1-b2^t)/(1-b1^t).

    ``learning_rate`` is a float or a schedule (ExponentialDecay, CosineDecay, PiecewiseConstantDecay).  Once built, the
    rate lives in a small device record that the optimizer kernel reads on every step, so an assignment to
    ``optimizer.learning_rate`` reaches the next update, also the next replay of a captured step.  ``global_clipnorm``
    (tf.clip_by_global_norm over all variables; excludes ``clipnorm``; a non-finite global norm makes the whole update
    NaN, as in TensorFlow) and ``weight_decay`` (keras's decoupled w <- w - lr_t * wd * w ahead of the update; see
    ``exclude_from_weight_decay``) run in the same launch."""

    def __init__(self, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None, global_clipnorm=None,
                 weight_decay=None):
        self._vars = None
        self._step_dev = None
        self._lr = _checked_rate(learning_rate)
        self.beta_1, self.beta_2 = float(beta_1), float(beta_2)
        self.epsilon, self.clipnorm = float(epsilon), (None if clipnorm is None else float(clipnorm))
        self.global_clipnorm = None if global_clipnorm is None else float(global_clipnorm)
        self.weight_decay = None if weight_decay is None else _finite(weight_decay, "weight_decay")
        if self.clipnorm is not None and self.global_clipnorm is not None:
            raise ValueError("clipnorm and global_clipnorm exclude each other")
        if self.global_clipnorm is not None and not self.global_clipnorm > 0.0:
            raise ValueError(f"global_clipnorm must be > 0, got {self.global_clipnorm}")
        if self.weight_decay is not None and self.weight_decay < 0.0:
            raise ValueError(f"weight_decay must be >= 0, got {self.weight_decay}")
        self._no_decay = []

    @property
    def learning_rate(self):
        """The host copy of the rate: a float, or the schedule object."""
        return self._lr

    @learning_rate.setter
    def learning_rate(self, value):
        value = _checked_rate(value)
        if self._vars is not None:
            self._write_record(value)
        self._lr = value

    def _record(self, rate=None):
        rate = self._lr if rate is None else rate
        return rate._record() if isinstance(rate, LearningRateSchedule) else _lr_record(LR_CONSTANT, rate)

    def _write_record(self, rate=None):
        """The device record <- the host rate: one small copy on the current stream, which the next update (or replay
        of a captured step) reads.  No recapture, no synchronisation of the device."""
        rec = self._record(rate)
        check(_lib.load().impnn_lr_schedule_check(C.c_void_p(rec.ctypes.data)))
        self._record_dev.copy_(torch.from_numpy(rec))

    def current_learning_rate(self):
        """The rate the next update will use, as the optimizer kernel's own function computes it from the device record
        and the device counter (synchronises)."""
        if self._vars is None:
            lr = self._lr(0) if isinstance(self._lr, LearningRateSchedule) else self._lr
            return float(np.float32(lr))
        out = torch.empty(1, dtype=torch.float32, device=self._record_dev.device)
        with torch.cuda.device(out.device):
            check(_lib.load().impnn_lr_schedule_eval(C.c_void_p(self._record_dev.data_ptr()),
                                                     C.c_void_p(self._step_dev.data_ptr()),
                                                     C.c_void_p(out.data_ptr()), 1, stream_ptr()))
        return float(out.item())

    def exclude_from_weight_decay(self, var_names):
        """Variables whose name (as ``model.trainable_variables()`` gives it) contains one of ``var_names`` do not
        decay.  Before ``compile`` / ``build`` only."""
        if self._vars is not None:
            raise RuntimeError("exclude_from_weight_decay must be called before the optimizer is built")
        self._no_decay = [str(s) for s in var_names]

    @property
    def iterations(self):
        """Number of updates applied (the counter lives in device memory; reading it synchronises)."""
        return int(self._step_dev.item()) if self._step_dev is not None else 0

    def get_config(self):
        lr = self._lr
        if isinstance(lr, LearningRateSchedule):
            lr = {"class_name": type(lr).__name__, "config": lr.get_config()}
        cfg = {"name": "Adam", "learning_rate": lr, "beta_1": self.beta_1, "beta_2": self.beta_2,
               "epsilon": self.epsilon, "clipnorm": self.clipnorm}
        if self.global_clipnorm is not None:
            cfg["global_clipnorm"] = self.global_clipnorm
        if self.weight_decay is not None:
            cfg["weight_decay"] = self.weight_decay
        return cfg

    @classmethod
    def from_config(cls, config):
        config = {k: v for k, v in config.items() if k != "name"}
        lr = config.get("learning_rate")
        if isinstance(lr, dict):
            config["learning_rate"] = _SCHEDULES[lr["class_name"]].from_config(lr["config"])
        return cls(**config)

    def build(self, variables, names=None):
        """variables: list of leaf tensors on one GPU.  Gradients live in ONE flat buffer (views become the
        variables' .grad), so the data-parallel average is a single collective and the kernel's pointer table
        stays valid for the whole run (also inside a captured hipGraph).  ``names``: the variables' names, which
        ``exclude_from_weight_decay`` matches.
        A row-restricted embedding table (autograd.restrict_rows: a frozen Embedding with ``trainable_rows``) never
        decays, whatever ``exclude_from_weight_decay`` says: decay would move the rows that are to keep their bits.
        Nothing else about it is special - its unlisted rows arrive with a gradient of +0.0, which leaves m, v and the
        weight as they are."""
        variables = list(variables)
        if self._no_decay and self.weight_decay is not None and names is None:
            raise ValueError("exclude_from_weight_decay needs the variables' names: build(variables, names=[...])")
        dev = variables[0].device
        sizes = [int(v.numel()) for v in variables]
        total = sum(sizes)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.m = torch.zeros(total, dtype=torch.float32, device=dev)
        self.v = torch.zeros(total, dtype=torch.float32, device=dev)
        self._step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        table, off = [], 0
        for var, n in zip(variables, sizes):
            if var.dtype != torch.float32 or not var.is_contiguous():
                raise ValueError("optimizer variables must be contiguous float32 tensors")
            var.grad = self.flat_grad[off:off + n].view_as(var)
            table += [var.data_ptr(), self.flat_grad.data_ptr() + 4 * off, self.m.data_ptr() + 4 * off,
                      self.v.data_ptr() + 4 * off]
            off += n
        # data_ptr values are < 2^63: store them as int64 bit patterns
        self._table = torch.tensor(table, dtype=torch.int64, device=dev)
        self._sizes = torch.tensor(sizes, dtype=torch.int64, device=dev)
        self._record_dev = torch.zeros(LR_RECORD_WORDS, dtype=torch.int32, device=dev)
        self._decay_flags = self._norm_ws = None
        if self.weight_decay is not None:
            names = [""] * len(variables) if names is None else list(names)
            if len(names) != len(variables):
                raise ValueError("names must have one entry per variable")
            self._decay_flags = torch.tensor([int(not any(s in n for s in self._no_decay)
                                                  and getattr(var, "_impnn_rows", None) is None)
                                              for n, var in zip(names, variables)], dtype=torch.int32, device=dev)
        if self.global_clipnorm is not None:
            need = int(_lib.load().impnn_adam_step_scheduled_workspace_floats(len(variables)))
            self._norm_ws = torch.zeros(max(need, 1), dtype=torch.float32, device=dev)
        self._vars = variables
        self._write_record()

    def zero_grad(self):
        self.flat_grad.zero_()

    def state(self):
        return {"m": self.m.clone(), "v": self.v.clone(), "step": self._step_dev.clone()}

    def load_state(self, st):
        self.m.copy_(st["m"]); self.v.copy_(st["v"]); self._step_dev.copy_(st["step"])

    def apply_gradients(self):
        """One launch: clip, moments, update for every variable (gradients are read from the flat buffer);
        the step counter is advanced on the device and the rate is read from the device record, so the call can sit
        inside a captured graph.  ``global_clipnorm`` adds one launch ahead of it (the sums of squares)."""
        if self._vars is None:
            raise RuntimeError("Adam.build(variables) has not been called")
        lo, hi = self.flat_grad.data_ptr(), self.flat_grad.data_ptr() + 4 * self.flat_grad.numel()
        for var in self._vars:  # autograd swaps .grad for a fresh tensor if it was reset to None
            if var.grad is None or not (lo <= var.grad.data_ptr() < hi):
                raise RuntimeError("a variable's .grad no longer points into the optimizer's flat buffer; "
                                   "use optimizer.zero_grad() instead of setting .grad = None")
        dev = self.flat_grad.device
        with torch.cuda.device(dev):
            ws = self._norm_ws
            check(_lib.load().impnn_adam_step_scheduled(
                C.c_void_p(self._table.data_ptr()), C.c_void_p(self._sizes.data_ptr()), len(self._vars),
                C.c_void_p(self._step_dev.data_ptr()), C.c_void_p(self._record_dev.data_ptr()), self.beta_1,
                self.beta_2, self.epsilon, self.clipnorm if self.clipnorm else 0.0, self.global_clipnorm or 0.0,
                self.weight_decay or 0.0,
                None if self._decay_flags is None else C.c_void_p(self._decay_flags.data_ptr()),
                None if ws is None else C.c_void_p(ws.data_ptr()), 0 if ws is None else ws.numel(), stream_ptr()))


class GraphedTrainStep:
    """One training step (forward, backward, optimizer) of a fixed batch shape captured in a hipGraph
    (torch.cuda.CUDAGraph) and replayed per mini-batch: the reference trains with batches of 32
    (train_viscosity.py:332), where a step is ~150 small launches and the host, not the GPU, sets the pace.
    Inputs are copied into static buffers; every kernel argument that changes between steps lives in device
    memory (the Adam step counter, the dropout step counter that the captured snapshot launch advances).  A model
    compiled with metrics keeps the training pass's predictions in a persistent buffer and the captured step ends
    with one impnn_regression_sums launch per metric record, adding the batch to the epoch's running record."""

    def __init__(self, model, inputs, y, resident=None, sample_weight=None, states=None):
        """``resident=(x, y_dev)``: the whole padded training set lives on the device; the captured step then starts
        with the gather of the rows in ``self.static_rows`` (impnn_gather_rows) and ``step_on_rows`` only refreshes
        those 8*batch bytes between replays.  ``sample_weight`` (one value per sample of the batch) makes it the
        weighted step: the weights sit in a static buffer like y, and ``resident=(x, y_dev, w_dev)`` gathers their
        rows inside the capture too, with a second gather launch behind the first (the first takes at most 8 tensors
        and stays as the unweighted step has it).
        ``resident=(enc, y_dev[, w_dev])`` with a data.FrozenEncodings (stage 1 of transfer learning; the model's
        ``frozen_encodings`` names the refusals): ``inputs`` is the first batch's sample rows (device int64).  The
        captured step is then one gather of the batch's two ion indices, targets and weights, the head's loss over
        indexed rows, its backward and the optimizer: no encoder launch, and ``step_on_rows`` copies only the rows.
        ``states=st`` (a data.FrozenStates of the resident ``x``; the model's ``frozen_states`` names the refusals):
        each ion's encoder resumes behind its frozen steps.  The batch's two ion indices ride in the second gather
        launch, with the weights where there are any; then one impnn_state_rows node gathers the states and the
        layered pass starts there.  ``step_on_rows`` still refreshes only the sample rows, and refuses to replay once
        the states are stale."""
        from .data import FrozenEncodings
        self.model = model
        dev = model.device
        self.states = states
        if states is not None:
            model._frozen_steps_check()
            if resident is None or isinstance(resident[0], FrozenEncodings):
                raise ValueError("cache_frozen_steps: states=st goes with resident=(x, y_dev[, w_dev])")
            if states.stale(model):
                raise ValueError("cache_frozen_steps: the states are older than the model's frozen weights or were "
                                 "made for another prefix: build them again")
        self.enc = resident[0] if resident is not None and isinstance(resident[0], FrozenEncodings) else None
        if self.enc is not None:
            model._frozen_cache_check()
            if self.enc.stale(model):
                raise ValueError("the encodings are older than the model's encoder weights: build them again")
            rows0 = torch.as_tensor(inputs, dtype=torch.int64).to(dev).reshape(-1)
            inputs = {}
        self.static_in = {k: v.clone() for k, v in model._to_device(inputs).items()}
        self.static_y = torch.as_tensor(np.asarray(y, np.float32)).to(dev).reshape(-1, 1).clone()
        self.batch = int(self.static_y.shape[0])
        self.static_w = None
        if sample_weight is not None:
            self.static_w = checked_sample_weight(sample_weight, self.batch, dev).reshape(-1, 1).clone()
        self.resident = None
        self.resident_w = None
        if self.enc is not None:
            if (len(resident) == 3) != (self.static_w is not None):
                raise ValueError("resident=(enc, y_dev, w_dev) goes with sample_weight, resident=(enc, y_dev) without")
            enc, y_dev = self.enc, resident[1]
            if rows0.numel() != self.batch:
                raise ValueError("inputs must hold one sample row per value of y")
            if not (y_dev.is_contiguous() and y_dev.dtype == torch.float32 and y_dev.numel() == len(enc)):
                raise ValueError("resident targets must be a contiguous float32 tensor, one value per sample")
            self.static_rows = rows0.clone()
            self.static_cat_row = torch.index_select(enc.cat_row, 0, rows0)
            self.static_an_row = torch.index_select(enc.an_row, 0, rows0)
            srcs, dsts = [enc.cat_row, enc.an_row, y_dev.reshape(-1, 1)], [self.static_cat_row, self.static_an_row, self.static_y]
            if self.static_w is not None:
                w_dev = resident[2]
                if not (w_dev.is_contiguous() and w_dev.dtype == torch.float32 and w_dev.numel() == len(enc)):
                    raise ValueError("resident weights must be a contiguous float32 tensor, one value per sample")
                srcs, dsts = srcs + [w_dev.reshape(-1, 1)], dsts + [self.static_w]
            self.enc_gather = (srcs, dsts)
        elif resident is not None:
            if (len(resident) == 3) != (self.static_w is not None):
                raise ValueError("resident=(x, y_dev, w_dev) goes with sample_weight, resident=(x, y_dev) without")
            x, y_dev = resident[0], resident[1]
            keys = list(self.static_in)
            ok = len(keys) + 1 <= 8 and all(
                x[k].is_contiguous() and x[k].dtype == self.static_in[k].dtype and x[k].element_size() == 4
                for k in keys) and y_dev.is_contiguous() and y_dev.dtype == torch.float32
            if ok:
                self.resident = ([x[k] for k in keys] + [y_dev], [self.static_in[k] for k in keys] + [self.static_y])
                self.static_rows = torch.zeros(self.batch, dtype=torch.int64, device=dev)
                if self.static_w is not None:
                    w_dev = resident[2]
                    if not (w_dev.is_contiguous() and w_dev.dtype == torch.float32 and w_dev.numel() == y_dev.numel()):
                        raise ValueError("resident weights must be a contiguous float32 tensor, one value per sample")
                    self.resident_w = ([w_dev.reshape(-1, 1)], [self.static_w])
            if states is not None:
                if not ok or len(states) != y_dev.numel():
                    raise ValueError("cache_frozen_steps: the captured step gathers from resident 4-byte tensors, and "
                                     "the states hold one index per resident sample")
                self.static_cat_row = torch.zeros(self.batch, dtype=torch.int32, device=dev)
                self.static_an_row = torch.zeros(self.batch, dtype=torch.int32, device=dev)
                srcs, dsts = self.resident_w if self.resident_w is not None else ([], [])
                self.resident_w = (srcs + [states.cat_row.reshape(-1, 1), states.an_row.reshape(-1, 1)],
                                   dsts + [self.static_cat_row.reshape(-1, 1), self.static_an_row.reshape(-1, 1)])
        opt = model.optimizer
        saved_w = [t.detach().clone() for _, t in model.variables()]  # (with BatchNormalization's moving statistics)
        saved_o = opt.state()
        ctr = model.dropout_counter()  # the dropout step counter: the warm-up steps advance it, like the Adam state
        saved_c = ctr.clone() if ctr is not None else None
        # with compiled metrics the step ends with their regression_sums launches, which add to the epoch's records
        self.metrics = model._metric_set if getattr(model, "_metric_set", None) else None
        saved_m = self.metrics.buffer("train", dev).clone() if self.metrics else None
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):  # warm-up off the default stream, as graph capture requires
            for _ in range(3):
                self._step()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.static_loss = self._step()
        with torch.no_grad():  # the warm-up steps were real updates: undo them
            for (_, t), w0 in zip(model.variables(), saved_w):
                t.copy_(w0)
        opt.load_state(saved_o)
        if ctr is not None:
            ctr.copy_(saved_c)
        if saved_m is not None:
            self.metrics.buffer("train", dev).copy_(saved_m)
        opt.zero_grad()
        self._cache_refs = model._cache_refs()  # frozen layers' cached tensors the captured kernels read
        model.weights_updated()

    def _step(self):
        m = self.model
        if self.enc is not None:
            from . import ops
            ops.gather_rows(self.enc_gather[0], self.enc_gather[1], self.static_rows)
            kw = {"metric_slot": "train"} if self.metrics else {}
            loss = m._loss_encoded(self.enc, self.static_cat_row, self.static_an_row, self.static_y, True,
                                   self.static_w, **kw)
            loss.backward()
            m.optimizer.apply_gradients()
            m.optimizer.zero_grad()
            return loss.detach()
        if self.resident is not None:
            from . import ops
            ops.gather_rows(self.resident[0], self.resident[1], self.static_rows)
            if self.resident_w is not None:
                ops.gather_rows(self.resident_w[0], self.resident_w[1], self.static_rows)
        kw = {"metric_slot": "train"} if self.metrics else {}  # without metrics: the call, and the graph, as ever
        if self.states is not None:
            kw["states"] = (self.states, self.static_cat_row, self.static_an_row)
        if self.static_w is None:
            loss = m._loss(self.static_in, self.static_y, training=True, **kw)
        else:
            loss = m._loss(self.static_in, self.static_y, training=True, sample_weight=self.static_w, **kw)
        loss.backward()
        m.join_training_streams()
        m.optimizer.apply_gradients()
        m.optimizer.zero_grad()
        return loss.detach()

    def matches(self, inputs):
        if self.enc is not None:
            return inputs is self.enc
        return all(tuple(inputs[k].shape) == tuple(v.shape) for k, v in self.static_in.items())

    def step_on_rows(self, x, y_dev, rows, w_dev=None):
        """One step on the mini-batch ``rows`` (device int64 tensor, len = batch) of a device-resident data set:
        the rows are gathered straight into the static buffers (one index_select per tensor, no staging copy, no
        host round trip).  ``w_dev``: the data set's weights, for a step that was built with ``sample_weight``."""
        if (w_dev is not None) != (self.static_w is not None):
            raise ValueError("a step captured with sample_weight takes weights on every call, one without takes none")
        if self.enc is not None:
            if x is not self.enc or self.enc.stale(self.model):
                raise ValueError("a step captured over encodings replays on those encodings, while they are current")
            self.static_rows.copy_(rows)  # the gather of the batch's indices, targets and weights is the first node
        elif self.states is not None:
            if x[next(iter(self.static_in))] is not self.resident[0][0] or self.states.stale(self.model):
                raise ValueError("cache_frozen_steps: a step captured over states replays on the resident data it was "
                                 "built with, while the states are current")
            self.static_rows.copy_(rows)
        elif self.resident is not None and x[next(iter(self.static_in))] is self.resident[0][0]:
            self.static_rows.copy_(rows)  # the gather is the first node of the graph
        else:
            for k, v in self.static_in.items():
                torch.index_select(x[k], 0, rows, out=v)
            torch.index_select(y_dev, 0, rows, out=self.static_y)
            if w_dev is not None:
                torch.index_select(w_dev.reshape(-1, 1), 0, rows, out=self.static_w)
        self.graph.replay()
        self.model.weights_updated()
        return self.static_loss

    def __call__(self, inputs, y, sample_weight=None):
        if self.enc is not None:
            raise ValueError("a step captured over encodings takes sample rows: step_on_rows(enc, y_dev, rows)")
        if self.states is not None:
            raise ValueError("a step captured over states takes sample rows: step_on_rows(x, y_dev, rows)")
        if (sample_weight is not None) != (self.static_w is not None):
            raise ValueError("a step captured with sample_weight takes weights on every call, one without takes none")
        for k, v in self.static_in.items():
            v.copy_(inputs[k], non_blocking=True)
        self.static_y.copy_(torch.as_tensor(np.asarray(y, np.float32)).reshape(-1, 1), non_blocking=True)
        if sample_weight is not None:
            self.static_w.copy_(checked_sample_weight(sample_weight, self.batch).reshape(-1, 1), non_blocking=True)
        self.graph.replay()
        self.model.weights_updated()
        return self.static_loss


class History:
    def __init__(self):
        self.history = {}
        self.epoch = []

    def _log(self, epoch, logs):
        self.epoch.append(epoch)
        for k, v in logs.items():
            self.history.setdefault(k, []).append(float(v))


class Callback:
    """keras.callbacks.Callback protocol as the trainers use it (train_viscosity.py:112-132 subclasses it):
    ``set_model`` is called once, then ``on_train_begin(logs)``, ``on_epoch_end(epoch, logs)`` per epoch and
    ``on_train_end(logs)``; a callback stops training by setting ``self.model.stop_training = True``."""

    def __init__(self):
        self.model = None

    def set_model(self, model):
        self.model = model

    def on_train_begin(self, logs=None):
        pass

    def on_epoch_begin(self, epoch, logs=None):
        pass

    def on_epoch_end(self, epoch, logs=None):
        pass

    def on_train_end(self, logs=None):
        pass


def _constant_rate(optimizer, who):
    lr = optimizer.learning_rate
    if isinstance(lr, LearningRateSchedule):
        raise ValueError(f"{who} sets a constant learning rate: the optimizer's rate is a {type(lr).__name__} schedule")
    return float(lr)


def _monitor_mode(mode, monitor):
    """keras's ``mode`` of a monitoring callback -> "min" or "max": "auto" is "max" for a monitor whose name ends in
    ``r2`` (R^2 grows as the model improves) and "min" for every other one (losses and errors)."""
    if mode not in ("auto", "min", "max"):
        raise ValueError(f"mode must be 'auto', 'min' or 'max', got {mode!r}")
    if mode == "auto":
        return "max" if str(monitor).endswith("r2") else "min"
    return mode


class ReduceLROnPlateau(Callback):
    """keras.callbacks.ReduceLROnPlateau: when ``monitor`` has not improved by ``min_delta`` for
    ``patience`` epochs, the rate becomes max(rate * factor, min_lr) and ``cooldown`` epochs pass before the count
    starts again.  The assignment reaches a captured step's next replay (Adam keeps the rate in device memory).
    ``mode``: "min" (an improvement is a smaller value), "max" (a larger one: R^2) or "auto" (by the monitor's name,
    _monitor_mode).  ``self.rates``: [(epoch, rate)] of the rates it set."""

    def __init__(self, monitor="val_loss", factor=0.1, patience=10, min_delta=1e-4, cooldown=0, min_lr=0.0, mode="auto"):
        super().__init__()
        if float(factor) >= 1.0:
            raise ValueError("ReduceLROnPlateau does not support a factor >= 1.0")
        self.monitor, self.factor, self.patience = monitor, float(factor), int(patience)
        self.min_delta, self.cooldown, self.min_lr = float(min_delta), int(cooldown), float(min_lr)
        self.mode = _monitor_mode(mode, monitor)
        self.best, self.wait, self.cooldown_counter, self.rates = self._worst(), 0, 0, []

    def _worst(self):
        return np.inf if self.mode == "min" else -np.inf

    def _improved(self, cur):
        if self.mode == "min":
            return cur < self.best - self.min_delta
        return cur > self.best + self.min_delta

    def on_train_begin(self, logs=None):
        self.best, self.wait, self.cooldown_counter, self.rates = self._worst(), 0, 0, []
        _constant_rate(self.model.optimizer, "ReduceLROnPlateau")

    def on_epoch_end(self, epoch, logs=None):
        cur = (logs or {}).get(self.monitor)
        if cur is None:
            return
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.wait = 0
        if self._improved(cur):
            self.best, self.wait = cur, 0
        elif self.cooldown_counter <= 0:
            self.wait += 1
            if self.wait >= self.patience:
                old = _constant_rate(self.model.optimizer, "ReduceLROnPlateau")
                if old > self.min_lr:
                    new = max(old * self.factor, self.min_lr)
                    self.model.optimizer.learning_rate = new
                    self.rates.append((epoch, new))
                    self.cooldown_counter, self.wait = self.cooldown, 0


class LearningRateScheduler(Callback):
    """keras.callbacks.LearningRateScheduler: at the start of every epoch the rate becomes ``schedule(epoch, rate)``.
    ``self.rates``: [(epoch, rate)] of the rates it set."""

    def __init__(self, schedule):
        super().__init__()
        self.schedule, self.rates = schedule, []

    def on_train_begin(self, logs=None):
        self.rates = []

    def on_epoch_begin(self, epoch, logs=None):
        new = float(self.schedule(epoch, _constant_rate(self.model.optimizer, "LearningRateScheduler")))
        self.model.optimizer.learning_rate = new
        self.rates.append((epoch, new))


class EarlyStopping(Callback):
    """keras.callbacks.EarlyStopping(monitor, patience, restore_best_weights) (train_viscosity.py:334).  ``mode``:
    "min", "max" (the best epoch is the one of the largest value: ``monitor="val_r2"``) or "auto" (_monitor_mode)."""

    def __init__(self, monitor="val_loss", patience=0, restore_best_weights=False, min_delta=0.0, mode="auto"):
        super().__init__()
        self.monitor, self.patience, self.restore_best_weights = monitor, int(patience), bool(restore_best_weights)
        self.min_delta = abs(float(min_delta))
        self.mode = _monitor_mode(mode, monitor)
        self.on_train_begin()

    def _improved(self, cur):
        if self.mode == "min":
            return cur < self.best - self.min_delta
        return cur > self.best + self.min_delta

    def on_train_begin(self, logs=None):
        worst = np.inf if self.mode == "min" else -np.inf
        self.best, self.wait, self.best_weights, self.stopped_epoch, self.best_epoch = worst, 0, None, 0, 0

    def on_epoch_end(self, epoch, logs=None):
        cur = (logs or {}).get(self.monitor)
        if cur is None:
            return
        if self.restore_best_weights and self.best_weights is None:
            self.best_weights = self.model.state_dict()
        self.wait += 1
        if self._improved(cur):
            self.best, self.best_epoch, self.wait = cur, epoch, 0
            if self.restore_best_weights:
                self.best_weights = self.model.state_dict()
            return
        if self.wait >= self.patience and epoch > 0:
            self.stopped_epoch = epoch
            self.model.stop_training = True

    def on_train_end(self, logs=None):
        if self.restore_best_weights and self.best_weights is not None:
            self.model.load_weights(self.best_weights)


class Huber:
    """keras.losses.Huber(delta): per sample e^2 / 2 where |e| <= delta, else delta * (|e| - delta / 2); mean over
    the batch (train_melting_point_transfer.py:195).  ``model.compile(loss=Huber(1.0))``; the transfer model computes
    it inside its head kernels, the other models through this call."""

    def __init__(self, delta=1.0):
        self.delta = float(delta)
        if not self.delta > 0.0:
            raise ValueError("Huber delta must be positive")

    def get_config(self):
        return {"name": "huber_loss", "delta": self.delta}

    def __call__(self, y_true, y_pred, sample_weight=None):
        e = y_pred.reshape(y_true.shape[0], -1) - y_true.reshape(y_true.shape[0], -1)
        a = e.abs()
        per = torch.where(a <= self.delta, 0.5 * e * e, self.delta * (a - 0.5 * self.delta))
        if sample_weight is None:
            return torch.mean(per)
        return _weighted_batch_mean(per, sample_weight)


# ---- regression metrics (model.compile(metrics=[...], weighted_metrics=[...])).  Everything a metric needs is in one
# 8-word fp64 record per set of samples, which the device adds up batch by batch (ops.regression_sums,
# include/impnn.h: impnn_regression_sums) and the host reads once per evaluate / epoch.
RECORD_WORDS = 8
MAX_METRIC_SCALES = 4   # distinct (scale, offset) pairs of one compile
W_COUNT, W_SUM_W, W_SUM_E, W_SUM_ABS, W_SUM_SQ, W_SUM_Y, W_SUM_YY, W_MAX_ABS = range(RECORD_WORDS)


def regression_sums_reference(pred, y, sample_weight=None, groups=None, offset=0.0, scale=1.0):
    """The definition of the record, and the host reference of ops.regression_sums: numpy fp64 -> (n_seg, 8).

    With e = scale * (pred - y), yr = offset + scale * y and w = sample_weight (1 without), every term formed in
    float64 from the float32 values, a segment's record is
        0 samples | 1 sum w | 2 sum w*e | 3 sum w*|e| | 4 sum w*(e*e) | 5 sum w*yr | 6 sum w*(yr*yr) |
        7 max |e| over the samples with w > 0: NaN if one of those e is NaN, 0 for an empty segment.
    ``groups`` (one id per sample) cuts the samples into one segment per distinct id, in ``np.unique`` order; without
    it all samples are the one segment.  ``offset`` / ``scale`` carry a standardised target back to its unit."""
    p = np.asarray(pred, np.float32).reshape(-1).astype(np.float64)
    t = np.asarray(y, np.float32).reshape(-1).astype(np.float64)
    if p.shape != t.shape:
        raise ValueError("pred and y must hold one value per sample")
    w = np.ones_like(p) if sample_weight is None else np.asarray(sample_weight, np.float32).reshape(-1).astype(np.float64)
    if w.shape != p.shape:
        raise ValueError("sample_weight must hold one value per sample")
    scale, offset = float(scale), float(offset)
    if groups is None:
        segments = [np.arange(len(p))]
    else:
        g = np.asarray(groups).reshape(-1)
        if g.shape != p.shape:
            raise ValueError("groups must hold one id per sample")
        ids, inv = np.unique(g, return_inverse=True)
        order = np.argsort(inv, kind="stable")
        cuts = np.searchsorted(inv[order], np.arange(len(ids) + 1))
        segments = [order[cuts[s]:cuts[s + 1]] for s in range(len(ids))]
    out = np.zeros((len(segments), RECORD_WORDS), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s, idx in enumerate(segments):
            e = scale * (p[idx] - t[idx])
            yr = offset + scale * t[idx]
            ws, ae = w[idx], np.abs(e)
            live = ae[ws > 0]
            out[s] = [len(idx), ws.sum(), (ws * e).sum(), (ws * ae).sum(), (ws * (e * e)).sum(), (ws * yr).sum(),
                      (ws * (yr * yr)).sum(), live.max() if live.size else 0.0]
    return out


class Metric:
    """A regression metric: ``result(record)`` turns one 8-word record (regression_sums_reference) into the value, in
    float64 on the host.  ``scale`` / ``offset`` name the unit the errors are reported in (e = scale * (pred - y), the
    true value is offset + scale * y): metrics of one (scale, offset) share one device record.  Means are the word
    over the sum of the weights, and 0 where that sum is 0 (keras's divide_no_nan)."""

    default_name = None

    def __init__(self, name=None, scale=1.0, offset=0.0):
        self.name = str(name if name is not None else self.default_name)
        self.scale, self.offset = _finite(scale, "scale"), _finite(offset, "offset")
        if self.scale == 0.0:
            raise ValueError("scale must not be zero")

    @staticmethod
    def _record(record):
        r = np.asarray(record, np.float64).reshape(-1)
        if r.size != RECORD_WORDS:
            raise ValueError(f"a metric takes one record of {RECORD_WORDS} words, got {np.shape(record)}")
        return r

    @staticmethod
    def _mean(r, word):
        return float(r[word] / r[W_SUM_W]) if r[W_SUM_W] != 0.0 else 0.0

    def result(self, record):
        raise NotImplementedError

    def get_config(self):
        return {"name": self.name, "scale": self.scale, "offset": self.offset}

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class MeanAbsoluteError(Metric):
    """sum w |e| / sum w."""
    default_name = "mae"

    def result(self, record):
        return self._mean(self._record(record), W_SUM_ABS)


class MeanSquaredError(Metric):
    """sum w e^2 / sum w."""
    default_name = "mse"

    def result(self, record):
        return self._mean(self._record(record), W_SUM_SQ)


class RootMeanSquaredError(Metric):
    """sqrt(sum w e^2 / sum w)."""
    default_name = "rmse"

    def result(self, record):
        return float(np.sqrt(self._mean(self._record(record), W_SUM_SQ)))


class MeanError(Metric):
    """The bias, sum w e / sum w: positive where the model predicts too high."""
    default_name = "bias"

    def result(self, record):
        return self._mean(self._record(record), W_SUM_E)


class MaxError(Metric):
    """max |e| over the samples of weight > 0 (NaN if one of them is NaN)."""
    default_name = "max_error"

    def result(self, record):
        return float(self._record(record)[W_MAX_ABS])


class R2Score(Metric):
    """The reference's R^2 (utils/mp_utils.py r2_numpy, with its + 1e-6) from the sums, with weights:
    1 - sum w e^2 / (sum w yr^2 - (sum w yr)^2 / sum w + epsilon); 0 where sum w is 0."""
    default_name = "r2"

    def __init__(self, name=None, epsilon=1e-6, scale=1.0, offset=0.0):
        super().__init__(name, scale, offset)
        self.epsilon = _finite(epsilon, "epsilon")

    def result(self, record):
        r = self._record(record)
        if r[W_SUM_W] == 0.0:
            return 0.0
        ss_tot = r[W_SUM_YY] - r[W_SUM_Y] * r[W_SUM_Y] / r[W_SUM_W]
        return float(1.0 - r[W_SUM_SQ] / (ss_tot + self.epsilon))

    def get_config(self):
        return dict(super().get_config(), epsilon=self.epsilon)


METRICS = {"mae": MeanAbsoluteError, "mse": MeanSquaredError, "rmse": RootMeanSquaredError, "bias": MeanError,
           "max_error": MaxError, "r2": R2Score}


def get_metric(m):
    """A name of METRICS or a Metric object -> the object; anything else is a ValueError."""
    if isinstance(m, Metric):
        return m
    if isinstance(m, str) and m in METRICS:
        return METRICS[m]()
    raise ValueError(f"unknown metric {m!r}: a train.Metric object or one of {sorted(METRICS)}")


class MetricSet:
    """What ``compile(metrics=, weighted_metrics=)`` resolves to: the metrics in compile order under their log keys
    (``<name>``, ``weighted_<name>``) and the device records behind them - one per (scale, offset, weighted), in one
    persistent (n_records, 8) float64 buffer per ``slot`` ("train": the epoch's running record, "eval": evaluate's).
    A metric of ``metrics`` never sees ``sample_weight``; one of ``weighted_metrics`` does."""

    def __init__(self, metrics=None, weighted_metrics=None):
        self.entries, self.records = [], []   # (key, metric, record index); (scale, offset, weighted)
        for weighted, given in ((False, metrics), (True, weighted_metrics)):
            for m in ([] if given is None else [given] if isinstance(given, (str, Metric)) else list(given)):
                m = get_metric(m)
                rec = (m.scale, m.offset, weighted)
                if rec not in self.records:
                    self.records.append(rec)
                key = ("weighted_" if weighted else "") + m.name
                if key in self.keys:
                    raise ValueError(f"two metrics are logged as {key!r}: give one of them another name")
                self.entries.append((key, m, self.records.index(rec)))
        if len({(s, o) for s, o, _ in self.records}) > MAX_METRIC_SCALES:
            raise ValueError(f"at most {MAX_METRIC_SCALES} distinct (scale, offset) pairs in one compile")
        self._buffers = {}

    @property
    def keys(self):
        return [k for k, _, _ in self.entries]

    def __len__(self):
        return len(self.entries)

    def buffer(self, slot, device):
        """The slot's records: allocated once and kept (a captured step holds their address), on the model's device."""
        buf = self._buffers.get(slot)
        if buf is None:
            buf = self._buffers[slot] = torch.zeros(len(self.records), RECORD_WORDS, dtype=torch.float64, device=device)
        return buf

    def accumulate(self, slot, pred, y, sample_weight=None):
        """One impnn_regression_sums launch per record on the current stream: adds the batch to the slot's records."""
        from . import ops
        buf = self.buffer(slot, pred.device)
        for i, (scale, offset, weighted) in enumerate(self.records):
            ops.regression_sums(pred, y, sample_weight if weighted else None, offset=offset, scale=scale,
                                out=buf[i:i + 1], accumulate=True)

    def results(self, records, prefix=""):
        """The host copy (n_records, 8) of a slot -> {prefix + key: value} in compile order."""
        records = np.asarray(records, np.float64).reshape(len(self.records), RECORD_WORDS)
        return {prefix + key: m.result(records[i]) for key, m, i in self.entries}


def mse(y_true, y_pred, sample_weight=None):
    """keras "mse": mean over the last axis, then over the batch; with ``sample_weight`` (one value per sample)
    (1/B) sum_b w_b * mean_last(e_b^2), keras's sum_over_batch_size: B counts the samples of weight 0 too."""
    per = (y_pred.reshape(y_true.shape[0], -1) - y_true.reshape(y_true.shape[0], -1)) ** 2
    if sample_weight is None:
        return torch.mean(per)
    return _weighted_batch_mean(per, sample_weight)


def _weighted_batch_mean(per, sample_weight):
    """(1/B) sum_b w_b * mean over the last axis of per[b]: the weighted twin of torch.mean(per)."""
    w = torch.as_tensor(sample_weight, dtype=per.dtype, device=per.device).reshape(-1)
    if w.numel() != per.shape[0]:
        raise ValueError("sample_weight must hold one value per sample")
    return torch.sum(w * per.mean(dim=1)) / per.shape[0]


def checked_sample_weight(sample_weight, n, device=None):
    """``sample_weight`` as fit / evaluate / train_on_batch take it -> a float32 (n) tensor on ``device`` (host when
    None), or None.  Weights are one finite value >= 0 per sample: anything else is a ValueError here, before any
    library call.  A tensor that already lives on a GPU is only checked for its length - fit checked its values on
    the host when it uploaded them, and reading them back would stall every step."""
    if sample_weight is None:
        return None
    if isinstance(sample_weight, torch.Tensor) and sample_weight.device.type != "cpu":
        if sample_weight.numel() != n:
            raise ValueError(f"sample_weight holds {sample_weight.numel()} values for {n} samples")
        w = sample_weight.detach().to(torch.float32).reshape(-1)
        return w if device is None else w.to(device)
    w = np.asarray(sample_weight.detach().numpy() if isinstance(sample_weight, torch.Tensor) else sample_weight)
    if w.dtype == object or not (np.issubdtype(w.dtype, np.number) or w.dtype == bool):
        raise ValueError("sample_weight must be numeric")
    if w.size != n or (w.ndim > 1 and w.shape[0] != n):
        raise ValueError(f"sample_weight holds {w.size} values for {n} samples")
    w = w.astype(np.float32).reshape(-1)
    if not np.all(np.isfinite(w)):
        raise ValueError("sample_weight must be finite (no NaN, no infinity)")
    if np.any(w < 0):
        raise ValueError("sample_weight must not be negative")
    t = torch.from_numpy(np.ascontiguousarray(w))
    return t if device is None else t.to(device)


def slice_inputs(inputs, idx):
    return {k: v[idx] for k, v in inputs.items()}
