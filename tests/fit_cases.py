"""The case table of the fit fuzz (tests/test_gpu_fit_fuzz.py on the GPU, tests/test_fit_ref_host.py on the CPU), the
inputs of every case, the bounds and the comparison both tests apply.

Shapes: the metrics_ref.TINY widths, batch 16, 3 epochs, n = 50 - three full batches (captured under graph=True) and
a remainder of 2 that runs eagerly, so replays follow an eager step in epochs 2 and 3.  Deviations are in the rows.

Bounds ("Fit fuzz"): per class 8 x the largest distance of the float32 reference trainer from the float64
one over all rows, rounded up to one significant digit; tests/test_fit_ref_host.py measures them again on every run
(test_bounds_cover_eight_times_the_largest_float32_distance) and prints the per-row values.  The loss bound may not
exceed 1e-5, the displacement bound not 1e-3.

Inputs.  Targets are the initial model's own predictions minus an offset and a wide spread (``target``): the loss is
then a well-conditioned function of the weights - with targets near 1 the tiny models' gradients are so large that the
rounding of the float32 weights alone moves an epoch loss by 1e-5 - and the mean error keeps its sign.  Seeds were
chosen on the CPU so that no relu pre-activation and no Huber error of the fp64 run lies within the loss bound of its
kink and the early-stopping row's validation losses lie far apart (test_input_conditions)."""
import dataclasses

import numpy as np

from ionic_mpnn_amd import synthetic, weights

import metrics_ref as MR

# class bounds: 8 x the largest float32-against-float64 distance of the reference trainer (DESIGN.md holds the table)
LOSS_BOUND = 6e-6
DISPLACEMENT_BOUND = 8e-4
MOMENT_BOUND = 1e-3
MOVING_BOUND = 4e-4
LOSS_CAP, DISPLACEMENT_CAP = 1e-5, 1e-3
BOUNDS = {"loss": LOSS_BOUND, "displacement": DISPLACEMENT_BOUND, "moments": MOMENT_BOUND, "moving": MOVING_BOUND}
FLOOR = 0.3   # conftest.assert_close's floor: the per-element scale of the moments

TINY = dict(Va=MR.TINY["Va"], Vb=MR.TINY["Vb"], D=MR.TINY["D"], K=MR.TINY["K"], F=MR.TINY["F"], Mx=MR.TINY["Mx"], S=2)
N_ATOMS, N_EDGES = MR.TINY["N"], MR.TINY["E"]
ALL_METRICS = tuple((k, 1.0, 0.0) for k in ("mae", "mse", "rmse", "bias", "max_error", "r2"))
KELVIN = tuple((k, MR.SCALE, MR.OFFSET) for k in ("mae", "rmse", "max_error"))
CONSTANT = lambda lr: {"kind": "constant", "lr": lr}


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    kind: str = "viscosity"
    dims: dict = dataclasses.field(default_factory=lambda: dict(TINY))
    n: int = 50
    batch: int = 16
    epochs: int = 3
    shuffle: bool = True
    seed: int = 0                 # fit's shuffle seed
    data_seed: int = 5
    weight_seed: int = 5
    target: tuple = (8.0, 16.0)   # y = the initial model's prediction - mean - spread * N(0, 1)
    loss: tuple = ("mse", None)
    weighted: bool = False        # sample_weight with zeros, one of them on a batch's last sample
    metrics: tuple = ()
    weighted_metrics: tuple = ()
    validation: tuple = None      # (n, seed, weighted)
    opt: dict = dataclasses.field(default_factory=lambda: _opt(1e-3, clipnorm=1.0))
    epoch_rate: tuple = None      # (first rate, factor per epoch): a LearningRateScheduler
    early_stop: dict = None       # {"patience": 1}
    dropout: tuple = None         # (rate, seed) of GatedUpdate's dropout
    head_dropout_seed: int = 0x5EED0BADCAFE
    frozen: str = None            # None | "step0" | "stage1" | "stage2"
    caches: tuple = ({},)         # fit's cache flags the row runs with (the reference is the same run)
    graphs: tuple = (False, True)
    options: tuple = ()           # what the row turns on (option_off), each of which must move the run
    knocks: tuple = ()            # fit_ref.KNOCKOUTS the row must notice

    @property
    def fp_l2(self):
        return 1e-5 if self.kind == "melting_point" else 1e-4

    @property
    def bn_trains(self):
        return self.kind == "transfer"   # every transfer row trains mp_bn_1: batch statistics in training passes

    @property
    def steps_per_epoch(self):
        return -(-self.n // self.batch)


def _opt(lr=1e-3, **kw):
    return dict(lr=CONSTANT(lr) if not isinstance(lr, dict) else lr, **kw)


def _dims(**kw):
    return dict(TINY, **kw)


EXP = {"kind": "exponential", "lr0": 5e-2, "decay_steps": 2, "decay_rate": 0.5, "staircase": False}
COS = {"kind": "cosine", "lr0": 1e-3, "decay_steps": 9, "alpha": 0.1, "warmup_target": 1e-2, "warmup_steps": 3}
PIECE = {"kind": "piecewise", "boundaries": [4, 8], "values": [1e-2, 3e-3, 1e-3]}
COS_T = {"kind": "cosine", "lr0": 1e-3, "decay_steps": 12, "alpha": 0.0, "warmup_target": None, "warmup_steps": 0}
ORDER = ("rotate_order", "drop_remainder", "adam_t_off")

CASES = [
    Case("plain", options=("clip", "shuffle"), knocks=ORDER),
    Case("remainder-1", n=49, shuffle=False, weighted=True, metrics=ALL_METRICS, weighted_metrics=ALL_METRICS,
         validation=(21, 11, True), target=(64.0, 16.0),
         options=("sample_weight", "val_weight"),
         knocks=ORDER + ("weights_metrics_only",)),
    Case("no-remainder", n=48, knocks=("rotate_order",)),
    Case("no-graph", n=10, options=("clip",)),
    Case("weighted-huber", weighted=True, loss=("huber", 0.25), weighted_metrics=(("mae", 1.0, 0.0), ("rmse", 1.0, 0.0)),
         target=(0.5, 1.0),
         options=("sample_weight", "huber"), knocks=ORDER + ("weights_metrics_only",)),
    Case("sched-exp", target=(32.0, 64.0), opt=_opt(EXP, global_clipnorm=0.05, weight_decay=0.05, exclude=("bias", "layernorm")),
         options=("schedule", "global_clip", "weight_decay", "exclude"),
         knocks=ORDER + ("schedule_off", "decay_excluded")),
    Case("sched-cos", opt=_opt(COS, clipnorm=1.0), options=("schedule",), knocks=ORDER + ("schedule_off",)),
    Case("sched-piecewise", target=(32.0, 64.0), opt=_opt(PIECE, clipnorm=1.0), options=("schedule",), knocks=ORDER + ("schedule_off",)),
    Case("epoch-rate", data_seed=9, weight_seed=9, epochs=4, target=(32.0, 64.0), opt=_opt(3e-2, clipnorm=1.0), epoch_rate=(3e-2, 0.5), early_stop={"patience": 1},
         validation=(21, 11, False), options=("epoch_rate", "early_stop"), knocks=ORDER),
    Case("dropout", dims=_dims(D=32), dropout=(0.2, 2024), options=("dropout",), knocks=ORDER + ("dropout_stuck",)),
    Case("wide", dims=_dims(D=64), n=40, knocks=ORDER),
    Case("frozen-steps", data_seed=8, weight_seed=8, dims=_dims(S=3), frozen="step0", weighted=True, opt=_opt(1e-3, clipnorm=1.0, weight_decay=0.05),
         caches=({}, {"cache_frozen_steps": True}), options=("frozen", "weight_decay", "sample_weight"),
         knocks=ORDER + ("weights_metrics_only",)),
    Case("melting", data_seed=8, weight_seed=8, kind="melting_point", dims=_dims(D=8, K=64), knocks=ORDER),
    Case("transfer-stage1", data_seed=36, weight_seed=36, kind="transfer", frozen="stage1", loss=("huber", 1.0), weighted=True, metrics=KELVIN,
         weighted_metrics=KELVIN, opt=_opt(1e-3), target=(4.0, 4.0),
         caches=({}, {"cache_frozen_encoder": True}),
         options=("frozen", "huber", "sample_weight", "metric_unit"),
         knocks=ORDER + ("dropout_stuck", "moving_not_carried", "weights_metrics_only")),
    Case("transfer-stage2", kind="transfer", dims=_dims(S=4), frozen="stage2", loss=("huber", 1.0), data_seed=59,
         weight_seed=59, opt=_opt(COS_T, global_clipnorm=0.5), caches=({}, {"cache_frozen_steps": True}),
         options=("frozen", "schedule", "global_clip"),
         knocks=ORDER + ("schedule_off", "dropout_stuck", "moving_not_carried", "norm_over_frozen")),
    Case("transfer-all", data_seed=26, weight_seed=26, kind="transfer", dropout=(0.2, 77), loss=("huber", 1.0), opt=_opt(1e-3, global_clipnorm=0.5), target=(4.0, 4.0),
         options=("dropout", "global_clip"), knocks=ORDER + ("dropout_stuck", "moving_not_carried")),
]
BY_NAME = {c.name: c for c in CASES}


def option_off(case, option):
    """``case`` with one of its ``options`` switched off: what the option's absence would compute."""
    r = lambda **kw: dataclasses.replace(case, **kw)
    opt = case.opt
    if option == "clip":
        return r(opt=dict(opt, clipnorm=None))
    if option == "global_clip":
        return r(opt=dict(opt, global_clipnorm=None))
    if option == "weight_decay":
        return r(opt=dict(opt, weight_decay=None))
    if option == "exclude":
        return r(opt=dict(opt, exclude=()))
    if option == "schedule":
        lr = opt["lr"]
        return r(opt=dict(opt, lr=CONSTANT(lr["values"][0] if lr["kind"] == "piecewise" else lr["lr0"])))
    if option == "shuffle":
        return r(shuffle=False)
    if option == "sample_weight":
        return r(weighted=False)
    if option == "val_weight":
        return r(validation=case.validation[:2] + (False,))
    if option == "huber":
        return r(loss=("mse", None))
    if option == "epoch_rate":
        return r(epoch_rate=(case.epoch_rate[0], 1.0))
    if option == "early_stop":
        return r(early_stop=None)
    if option == "dropout":
        return r(dropout=None)
    if option == "frozen":
        return r(frozen=None)
    if option == "metric_unit":
        unit = lambda ms: tuple((k, 1.0, 0.0) for k, _, _ in ms)
        return r(metrics=unit(case.metrics), weighted_metrics=unit(case.weighted_metrics))
    raise ValueError(option)


# ---------------------------------------------------------------------------------------------------------------- inputs
def trainable(case, name):
    """Whether the variable ``name`` trains under the row's freezing pattern (the patterns of
    tests/test_gpu_transfer.py; "step0": both embeddings and message-passing step 0 of both ions frozen)."""
    head = name.startswith("mp_") or name.startswith("melting_point")
    if case.frozen is None:
        return True
    if case.frozen == "step0":
        return not (name.endswith("_embedding") or "_bmm_0/" in name or "_gu_0/" in name)
    if case.frozen == "stage1":
        return head
    if case.frozen == "stage2":
        return head or any(f"{p}_{l}_{i}/" in name for p in ("cat", "an") for l in ("bmm", "gu") for i in (2, 3))
    raise ValueError(case.frozen)


def layer_trainable(case, layer_name, num_steps):
    """The same patterns by layer name, for the model under test: GatedUpdates carry keras's automatic names
    (cation step i: gated_update[_i], anion step i: gated_update_{S+i})."""
    head = layer_name.startswith("mp_") or layer_name == "melting_point"
    gu = lambda k: "gated_update" if k == 0 else f"gated_update_{k}"
    if case.frozen is None:
        return True
    if case.frozen == "step0":
        return not (layer_name.startswith("embedding") or layer_name in ("cat_bmm_0", "an_bmm_0", gu(0), gu(num_steps)))
    if case.frozen == "stage1":
        return head
    if case.frozen == "stage2":
        return head or layer_name == "mix_cat_an" or layer_name in (
            "cat_bmm_2", "cat_bmm_3", "an_bmm_2", "an_bmm_3", gu(2), gu(3), gu(num_steps + 2), gu(num_steps + 3))
    raise ValueError(case.frozen)


def _set(case, n, seed):
    """n samples: random molecules, and targets around the initial model's own (inference) predictions - an offset, so
    that the mean error keeps its sign through the run, and a spread so wide that the loss is a well-conditioned
    function of the weights (its relative sensitivity to a weight's rounding falls as 1 / spread)."""
    import torch
    import fit_ref as FR
    d = case.dims
    x = synthetic.make_batch(n, max_atoms=N_ATOMS, max_edges=N_EDGES, atom_vocab_size=d["Va"],
                             bond_vocab_size=d["Vb"], min_atoms=3, seed=seed)
    if case.kind != "viscosity":
        x = {k: v for k, v in x.items() if k != "temperature"}
    w0 = case_weights(case)
    w = {k: torch.tensor(v, dtype=torch.float64) for k, v in w0.items()}
    with torch.no_grad():
        pred = FR._Pass(case, w, x, torch.float64, False, None, w0).pred.numpy().reshape(-1)
    mean, spread = case.target
    y = (pred - mean - spread * np.random.default_rng([seed, 7]).normal(size=n)).astype(np.float32)
    return x, y


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _make_data(case):
    n, data_seed, seed, shuffle, batch, weighted, validation = (case.n, case.data_seed, case.seed, case.shuffle,
                                                                case.batch, case.weighted, case.validation)
    x, y = _set(case, n, data_seed)
    sw = None
    if weighted:   # fractional weights with zeros: on the last sample of epoch 1's first batch and of its last one
        rng = np.random.default_rng([data_seed, 3])
        sw = rng.uniform(0.25, 2.0, size=n).astype(np.float32)
        order = np.random.default_rng(seed).permutation(n) if shuffle else np.arange(n)
        sw[order[min(batch, n) - 1]] = 0.0
        sw[order[n - 1]] = 0.0
        sw[rng.integers(0, n, size=3)] = 0.0
    val = None
    if validation is not None:
        vn, vseed, vweighted = validation
        vx, vy = _set(case, vn, vseed)
        vw = None
        if vweighted:
            vw = np.random.default_rng([vseed, 4]).integers(0, 3, size=vn).astype(np.float32)
        val = (vx, vy, vw)
    return x, y, sw, val


def case_data(case):
    """-> (x, y, sample_weight or None, (val_x, val_y, val_w or None) or None) as numpy arrays; shared, not to be written."""
    key = ("data", case.target, case.weight_seed, case.n, case.data_seed, case.seed, case.shuffle, case.batch, case.weighted, case.validation, case.kind,
           repr(sorted(case.dims.items())))
    return _cached(key, lambda: _make_data(case))


def _make_weights(kind, d, seed):
    base = "melting_point" if kind == "melting_point" else "viscosity"
    w = weights.init_weights(base, d["Va"], d["Vb"], atom_dim=d["D"], bond_dim=d["K"], fp_size=d["F"],
                             mixing_size=d["Mx"], num_steps=d["S"], seed=seed, perturb=True)
    if kind == "transfer":   # the viscosity model cut at mix_cat_an, and a head with every variable randomised
        w = {k: v for k, v in w.items() if not k.startswith("visc_params")}
        rng = np.random.default_rng(seed + 100)
        width = d["Mx"]
        for name, units in (("mp_dense_1", 256), ("mp_dense_2", 128), ("mp_dense_3", 64), ("melting_point", 1)):
            w[f"{name}/kernel"] = (1.5 * weights.glorot_uniform(rng, (width, units))).astype(np.float32)
            w[f"{name}/bias"] = rng.normal(0.0, 0.2, size=units).astype(np.float32)
            width = units
        w["mp_bn_1/gamma"] = rng.uniform(0.5, 1.5, size=256).astype(np.float32)
        w["mp_bn_1/beta"] = rng.normal(0.0, 0.2, size=256).astype(np.float32)
        w["mp_bn_1/moving_mean"] = rng.normal(0.0, 0.2, size=256).astype(np.float32)
        w["mp_bn_1/moving_variance"] = rng.uniform(0.5, 2.0, size=256).astype(np.float32)
    return w


def case_weights(case):
    """The initial variables (and moving statistics) of the row's model, float32 numpy; shared, not to be written."""
    key = ("weights", case.kind, repr(sorted(case.dims.items())), case.weight_seed)
    return _cached(key, lambda: _make_weights(case.kind, case.dims, case.weight_seed))


# ------------------------------------------------------------------------------------------------------------ comparison
def _rel(a, e):
    a, e = float(a), float(e)
    return 0.0 if a == e else abs(a - e) / max(abs(e), 1e-300)


def _close_distance(a, e):
    """The smallest ``rel`` at which conftest.assert_close(a, e, rel) passes."""
    a, e = np.asarray(a, np.float64), np.asarray(e, np.float64)
    if e.size == 0:
        return 0.0
    scale = max(float(np.abs(e).max()), 1e-30)
    return float(np.max(np.abs(a - e) / np.maximum(np.abs(e), FLOOR * scale)))


KAPPA = 1.0 / 4096   # a compared element's sqrt(v) never falls below this fraction of its tensor's root mean v


def reference(case):
    """The float64 run of the row (fit_ref.run) with ``compared``: per trainable tensor, the elements whose
    displacement the gradients determine.  Adam moves an element by rate * m / (sqrt(v) + 1e-7): the step depends on the
    gradient's size relative to its own history, so an absolute error d in a gradient entry changes the step by about
    d / sqrt(v) of itself.  For an entry that is a sum over samples and units, d scales with the tensor's typical entry,
    so an entry thousands of times below it is the one rounding decides: at the extreme, mp_dense_1's bias under batch
    statistics has an exactly zero gradient for every unit that is active on the whole batch (the normalisation
    removes a common shift), float32 leaves rounding noise there, and the element walks by about the rate per step in a
    direction no two implementations share.  An element is left out of the displacement check - of that check only, its
    m and v are compared like everyone's - when, at some step, the square root of its second-moment estimate v (from the
    float64 gradients) lies below KAPPA of the square root of the tensor's mean v.  Steps up to which the element's
    gradient has held no sum at all do not count: an exact zero (a unit dead so far, an id not seen yet) makes no
    step, and a gradient that is the l2 penalty alone, 2 lambda w, is one exact product however small.
    KAPPA = 1/4096 is the loosest threshold tried at which the float32 trainer's largest distance has not begun to move
    (9.7e-5 from 1/32 to 1/4096, 4.1e-4 at 1/16384).  That compares at least 98 % of every row's elements and at least
    85 % of every tensor's, except mp_dense_1's bias (61 - 78 %); tests/test_fit_ref_host.py asserts those fractions.
    Shared, not to be written."""
    import torch
    import fit_ref as FR

    def make():
        steps = []
        ref = FR.run(case, torch.float64, collect=steps)
        ref["steps"] = steps
        ref["compared"] = {}
        for n in ref["trainable"]:
            v, keep = np.zeros_like(ref["initial"][n]), np.ones(ref["initial"][n].shape, bool)
            summed = np.zeros(v.shape, bool)   # the element's gradient has held a sum over samples so far
            for st in steps:
                g = st["grads"][n]
                pen = st["penalty"].get(n, 0.0)
                summed |= np.abs(g - pen) > 1e-12 * np.abs(pen)
                v = FR.B2 * v + (1.0 - FR.B2) * g ** 2
                keep &= ~summed | (np.sqrt(v) >= KAPPA * np.sqrt(v.mean()))
            ref["compared"][n] = keep
        return ref
    return _cached(("reference", repr(case)), make)


def distances(got, ref):
    """The largest distance of a run ``got`` from the reference run ``ref`` per class, as {class: (value, where)}.
    Both: dict(history, weights, m, v, moving, initial, trainable).
      loss:          per epoch and key of the history, |a - e| / |e|
      displacement:  per trainable tensor, of d = w_T - w_0 over the elements ``ref["compared"]`` (``reference``):
                     ||d_a - d_e|| / ||d_e|| and max |d_a - d_e| / max |d_e|
      moments:       Adam's m and v per tensor, the smallest rel of conftest.assert_close
      moving:        the moving statistics, max |a - e| / max |e|
    A history of another length or with other keys is an infinite distance."""
    out = {k: (0.0, "") for k in BOUNDS}

    def offer(cls, value, where):
        if not value <= out[cls][0]:   # (a NaN counts)
            out[cls] = (float(value) if np.isfinite(value) else np.inf, where)

    hg, hr = got["history"], ref["history"]
    if list(hg) != list(hr) or any(len(hg[k]) != len(hr[k]) for k in hr):
        offer("loss", np.inf, "history keys / length")
    else:
        for k in hr:
            for ep, (a, e) in enumerate(zip(hg[k], hr[k])):
                offer("loss", _rel(a, e), f"{k} epoch {ep + 1}")
    for n in ref["trainable"]:
        keep = ref["compared"][n] if "compared" in ref else np.ones(ref["initial"][n].shape, bool)
        de = (ref["weights"][n] - ref["initial"][n])[keep]
        da = (np.asarray(got["weights"][n], np.float64) - ref["initial"][n])[keep]
        if not de.size:
            continue
        offer("displacement", np.linalg.norm(da - de) / max(np.linalg.norm(de), 1e-300), f"{n} (L2)")
        offer("displacement", np.abs(da - de).max() / max(np.abs(de).max(), 1e-300), f"{n} (element)")
        for mom in ("m", "v"):
            offer("moments", _close_distance(got[mom][n], ref[mom][n]), f"{mom} of {n}")
    for k, e in ref["moving"].items():
        offer("moving", np.abs(np.asarray(got["moving"][k], np.float64) - e).max() / max(np.abs(e).max(), 1e-300), k)
    return out


def check(case, got, ref, fraction=1.0, what=""):
    """Every class of ``distances`` within ``fraction`` of its bound; returns the distances as fractions of the bound."""
    d = distances(got, ref)
    for cls, (value, where) in d.items():
        assert value <= fraction * BOUNDS[cls], (f"{case.name} {what}: {cls} distance {value:.3e} at {where} > "
                                                 f"{fraction:g} x {BOUNDS[cls]:g}")
    return {cls: value / BOUNDS[cls] for cls, (value, _) in d.items()}
