"""The table of the cache fuzz (tests/test_gpu_cache_fuzz.py on the GPU, tests/test_cache_cases_host.py on the CPU):
sequences of weight-changing events on one long-lived model, the freezing patterns they run under, and DEPENDS - for
every derived copy of the weights the model keeps, the variables it is built from.

Plain Python, no device, deterministic from a seed: ``generate(seed)`` walks ROWS, draws each event's free parameters
(the variable an in-place write hits, the mode a switch goes to, the perturbation of a reload) and the order of the
events between two recompiles from ``default_rng([seed, row])``.  What a row covers does not depend on that order, so
the coverage properties hold for every seed; CASES is ``generate(0)``.

DEPENDS is written from the documented inputs of what builds each copy, not from ``MPNNModel.weights_updated``:
  packed            ops.pack_step_weights(steps): every step's bond_transform and GatedUpdate weights, both ions
  split_deg_limit   ops.split_mode_degree_limit(atom_table, bond_table, steps, D)
  prepared:<mode>   include/impnn.h, impnn_encoder_prepare_weights[_gates]: the packed weights; the bond table is read
                    by the typed modes only (f32t, f32x3); the atom table is folded in by the typed modes at atom_dim 32
  head_packed       MPNNModel._head_tensors(): the packed layout of impnn_model_head
  transfer_image    ops.transfer_grid_prepare: mp_dense_2, mp_dense_3, melting_point, BatchNormalization's gamma, beta
                    and moving statistics - not mp_dense_1, which impnn_transfer_ion_half reads from the variables
  mats:<ion>_<i>    ops.bond_type_matrices(bond table, the layer's bond_transform)
  frozen_encodings  data.FrozenEncodings: the pooled rows of encode_ions, i.e. every encoder variable
data.FrozenStates has no fixed source set (it depends on the prefix it was built for): ``states_sources``."""
import dataclasses

import numpy as np

GU = ("dense_z/kernel", "dense_z/bias", "dense_r/kernel", "dense_r/bias", "dense_h/kernel", "dense_h/bias",
      "layernorm/gamma", "layernorm/beta")
MOVING = ("mp_bn_1/moving_mean", "mp_bn_1/moving_variance")
# the smallest widths at which every cache exists ("Cache fuzz"); WIDE: the wide encoder's prepared weights
DIMS = dict(Va=11, Vb=6, D=32, K=8, F=32, Mx=20, S=3)
WIDE = dict(DIMS, D=64)
# odd batches: Huber's gradient of the last bias is a mean of signs once every error is beyond delta, and over an even
# batch that mean can be exactly zero - a trainable variable that a step leaves where it was
N_ATOMS, N_EDGES, BATCH = 12, 24, 7
FIT_SAMPLES, FIT_BATCH = 10, 5
GRID = {"viscosity": (17, 65), "melting_point": (17, 65), "transfer": (9, 33)}   # the 2 x 2 ragged tile grids
TYPED = ("f32t", "f32x3")
MODES = {32: ("f32t", "f32", "f32x3", "f16x2"), 64: ("f32t", "f32x3")}   # fused modes a probe asks for, by atom_dim
# "forward": a differentiable call, model(x, training=True), without an optimizer step - not a weight change by name,
# but a trainable BatchNormalization moves its moving statistics in it, which the transfer grid image holds
EVENT_KINDS = ("eager", "graphed", "stage1", "stage2", "fit", "reload", "inplace", "recompile", "mode", "forward")
TRAINING = ("eager", "graphed", "stage1", "stage2", "fit", "recompile")   # events that end in optimizer steps
# events after which a slot none of whose sources changed must hold the same object (the others go through
# invalidate_packed_weights, whose contract is to drop everything)
KEEPING = ("eager", "graphed", "stage1", "stage2", "recompile", "mode", "forward")
RATE = 1e-2          # Adam's rate in every event: a step moves every element with a gradient by about this much
LAST_EPOCH_RATE = 0.3   # the early-stop fit's last epoch: its variables end far from the best epoch's, which the restore brings back


# ------------------------------------------------------------------------------------------------------------ variables
def group(name):
    return name.split("/")[0]


def variable_names(kind, S):
    """The names of ``MPNNModel._named_tensors()`` (weights; the moving statistics are MOVING)."""
    dense = lambda g: [f"{g}/kernel", f"{g}/bias"]
    names = ["atom_embedding", "bond_embedding"]
    for p in ("cat", "an"):
        for i in range(S):
            names.append(f"{p}_bmm_{i}/bond_transform")
            names += [f"{p}_gu_{i}/{w}" for w in GU]
        names += dense(f"{p}_fp")
    names += dense("cat_proj") + dense("an_proj")
    if kind == "transfer":
        names += dense("mp_dense_1") + ["mp_bn_1/gamma", "mp_bn_1/beta"] + dense("mp_dense_2") + dense("mp_dense_3") \
            + dense("melting_point")
    elif kind == "viscosity":
        names += dense("visc_params")
    else:
        names += dense("mp_hidden") + dense("mp_out")
    return names


def step_names(kind, S, ions=("cat", "an"), steps=None):
    return [n for n in variable_names(kind, S) for p in ions for i in (range(S) if steps is None else steps)
            if group(n) in (f"{p}_bmm_{i}", f"{p}_gu_{i}")]


def encoder_names(kind, S):
    return ["atom_embedding", "bond_embedding"] + step_names(kind, S)


def head_names(kind, S):
    enc = set(encoder_names(kind, S))
    return [n for n in variable_names(kind, S) if n not in enc]


TRANSFER_TAIL = ("mp_bn_1/gamma", "mp_bn_1/beta", "mp_dense_2/kernel", "mp_dense_2/bias", "mp_dense_3/kernel",
                 "mp_dense_3/bias", "melting_point/kernel", "melting_point/bias")


def depends(kind, dims):
    """{slot: frozenset of the variable names it is built from} for a model of this kind and these dims."""
    S, D = dims["S"], dims["D"]
    steps = set(step_names(kind, S))
    out = {"packed": steps, "split_deg_limit": steps | {"atom_embedding", "bond_embedding"}}
    for mode in MODES[D]:
        src = set(steps)
        if mode in TYPED:
            src.add("bond_embedding")
            if D == 32:
                src.add("atom_embedding")
        out[f"prepared:{mode}"] = src
    out["head_packed"] = set(head_names(kind, S))
    if kind == "transfer":
        out["transfer_image"] = set(TRANSFER_TAIL) | set(MOVING)
    for p in ("cat", "an"):
        for i in range(S):
            out[f"mats:{p}_{i}"] = {"bond_embedding", f"{p}_bmm_{i}/bond_transform"}
    out["frozen_encodings"] = set(encoder_names(kind, S))
    return {k: frozenset(v) for k, v in out.items()}


def slot_class(slot):
    return slot.split(":")[0]


def slot_classes(kind):
    return ("packed", "split_deg_limit", "prepared", "head_packed", "mats", "frozen_encodings") + (
        ("transfer_image",) if kind == "transfer" else ())


# -------------------------------------------------------------------------------------------------------------- patterns
def _steps_groups(ions, steps):
    return {f"{p}_{l}_{i}" for p in ions for l in ("bmm", "gu") for i in steps}


def pattern_groups(pattern, kind, S):
    """The variable groups (a name up to its "/": one layer's variables) that train under a freezing pattern."""
    everything = {group(n) for n in variable_names(kind, S)}
    head = {group(n) for n in head_names(kind, S)}
    stage1 = {"mp_dense_1", "mp_bn_1", "mp_dense_2", "mp_dense_3", "melting_point"}
    table = {
        "everything": everything,
        "head": head,                                        # everything behind GlobalSumPool
        "cat_last": _steps_groups(("cat",), (S - 1,)),       # one ion's last step only
        "bmm_only": {"an_bmm_1"},                            # bond_transform of one layer only
        "atom_emb": {"atom_embedding"},
        "bond_emb": {"bond_embedding"},
        "lower_frozen": everything - {"atom_embedding", "bond_embedding"} - _steps_groups(("cat", "an"), (0,)),
    }
    if kind == "transfer":
        table.update({
            "stage1": stage1,                                # train_melting_point_transfer.py, stage 1
            # tests/test_frozen_states_host.py's stage2 and mixed, moved to S steps: the last two steps of both ions;
            # the cation's last bmm, the anion's bmm 1 and its GatedUpdates 1 and S-1, the anion's fingerprint Dense,
            # the head without mp_dense_2
            "stage2": stage1 | _steps_groups(("cat", "an"), (S - 2, S - 1)),
            "mixed": (stage1 - {"mp_dense_2"}) | {f"cat_bmm_{S - 1}", "an_bmm_1", "an_gu_1", f"an_gu_{S - 1}", "an_fp"},
            "bn_only": {"mp_bn_1"},                          # BatchNormalization trains, the tail is frozen
            "dense1_only": {"mp_dense_1"},                   # the grid image must survive
            "tail_one": {"mp_dense_3"},                      # the grid image must go
        })
    if pattern not in table:
        raise ValueError(f"no pattern {pattern!r} for a {kind} model")
    return frozenset(table[pattern])


def patterns(kind):
    base = ["everything", "head", "cat_last", "bmm_only", "atom_emb", "bond_emb", "lower_frozen"]
    return base + (["stage1", "stage2", "mixed", "bn_only", "dense1_only", "tail_one"] if kind == "transfer" else [])


def trainable(pattern, kind, S):
    """The variable names that train under the pattern, in the model's order."""
    groups = pattern_groups(pattern, kind, S)
    return [n for n in variable_names(kind, S) if group(n) in groups]


def prefix(pattern, kind, S):
    """``MPNNModel.frozen_prefix()`` under the pattern."""
    groups = pattern_groups(pattern, kind, S)
    if groups & {"atom_embedding", "bond_embedding"}:
        return {"cat": 0, "an": 0}
    first = lambda p: next((i for i in range(S) if groups & {f"{p}_bmm_{i}", f"{p}_gu_{i}"}), None)
    return {"cat": first("cat"), "an": first("an")}


def states_sources(pre, kind, S):
    """The variables a data.FrozenStates built for the prefix ``pre`` holds copies of."""
    src = set()
    for p in ("cat", "an"):
        if pre[p] == 0:
            continue
        src |= {"atom_embedding", "bond_embedding"} | set(step_names(kind, S, (p,), None if pre[p] is None else range(pre[p])))
    return frozenset(src)


def valid(event_kind, pattern, kind, dims):
    """Whether the model accepts the event under the pattern in force."""
    pre = prefix(pattern, kind, dims["S"])
    if event_kind == "stage1":   # MPNNModel._frozen_cache_check
        return kind == "transfer" and pre == {"cat": None, "an": None}
    if event_kind == "stage2":   # MPNNModel._frozen_steps_check (every event compiles mse, or Huber for transfer)
        return dims["D"] == 32 and not (pre["cat"] == 0 and pre["an"] == 0) and not (pre["cat"] is None and pre["an"] is None)
    return True


# ---------------------------------------------------------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    kind: str
    dims: dict
    pattern: str       # compiled at construction
    events: tuple      # of dicts: {"kind": ..., parameters}
    seed: int

    @property
    def S(self):
        return self.dims["S"]

    def in_force(self):
        """The pattern in force while event i runs (a recompile's own pattern for the recompile)."""
        out, cur = [], self.pattern
        for ev in self.events:
            if ev["kind"] == "recompile":
                cur = ev["pattern"]
            out.append(cur)
        return out

    def changes(self, i):
        """The variables (and moving statistics) event i changes."""
        ev, pattern = self.events[i], self.in_force()[i]
        if ev["kind"] == "mode":
            return frozenset()
        if ev["kind"] == "forward":
            bn = self.kind == "transfer" and "mp_bn_1" in pattern_groups(pattern, self.kind, self.S)
            return frozenset(MOVING) if bn else frozenset()
        if ev["kind"] == "inplace":
            return frozenset([ev["variable"]])
        if ev["kind"] == "reload":
            return frozenset(variable_names(self.kind, self.S)) | (frozenset(MOVING) if self.kind == "transfer" else frozenset())
        names = set(trainable(pattern, self.kind, self.S))
        if self.kind == "transfer" and "mp_bn_1" in pattern_groups(pattern, self.kind, self.S):
            names |= set(MOVING)   # a trainable BatchNormalization runs on batch statistics and moves its own
        return frozenset(names)

    def touched(self, i):
        """{slot: True where event i changes a source of the slot}."""
        ch = self.changes(i)
        return {slot: bool(ch & src) for slot, src in depends(self.kind, self.dims).items()}


# kind, dims, [(pattern, [event kinds under it])]: the first pattern is compiled at construction, every later one is
# a recompile event (a compile and a step) in front of its events.  "reload_file" is a reload through save / load_model.
ROWS = [
    ("visc-all", "viscosity", DIMS, [("everything", ["eager", "graphed", "mode"]), ("head", ["inplace:cat_bmm_1/bond_transform", "fit"]),
                                     ("cat_last", ["stage2"])]),
    ("visc-embeddings", "viscosity", DIMS, [("bond_emb", ["eager", "mode", "forward"]), ("bmm_only", ["eager", "reload"]),
                                            ("atom_emb", ["graphed"])]),
    ("visc-wide", "viscosity", WIDE, [("everything", ["eager", "reload_file", "mode"]), ("head", ["fit", "inplace:cat_fp/kernel"]),
                                      ("atom_emb", [])]),
    ("melting", "melting_point", DIMS, [("everything", ["fit", "inplace:bond_embedding"]),
                                        ("cat_last", ["stage2", "graphed", "mode"]), ("head", ["eager"])]),
    ("visc-lower", "viscosity", DIMS, [("lower_frozen", ["stage2", "fit+steps", "eager"]), ("atom_emb", ["eager"]),
                                       ("lower_frozen", ["stage2"])]),
    ("transfer-stage1", "transfer", DIMS, [("stage1", ["stage1", "graphed", "mode", "fit+encoder"]), ("everything", []),
                                           ("stage1", ["stage1"])]),
    ("transfer-stage2", "transfer", DIMS, [("stage2", ["stage2", "fit+steps", "forward"]), ("everything", ["eager"]),
                                           ("stage2", ["stage2", "mode"])]),
    ("transfer-mixed", "transfer", DIMS, [("mixed", ["stage2", "eager"]), ("bn_only", ["eager"]),
                                          ("dense1_only", ["graphed"]), ("tail_one", ["eager"])]),
    ("transfer-reload", "transfer", DIMS, [("everything", ["reload", "inplace:mp_dense_2/kernel", "mode"]),
                                           ("bn_only", ["fit"]), ("stage1", ["stage1"])]),
    ("transfer-tail", "transfer", DIMS, [("dense1_only", ["eager", "stage1", "inplace:mp_dense_1/bias"]),
                                         ("tail_one", ["stage1", "graphed"]), ("bond_emb", [])]),
]


def _event(spec, kind, dims, mode_at, rng):
    name, _, arg = spec.partition(":")
    name, _, flag = name.partition("+")
    if name == "inplace":
        return {"kind": "inplace", "variable": arg, "factor": float(rng.uniform(1.01, 1.05)), "shift": float(rng.uniform(0.005, 0.02))}
    if name in ("reload", "reload_file"):
        return {"kind": "reload", "via_file": name == "reload_file", "seed": int(rng.integers(1, 1 << 30))}
    if name == "mode":
        modes = MODES[dims["D"]] + ("auto",)
        ev = {"kind": "mode", "encoder_mode": modes[(mode_at + int(rng.integers(0, len(modes) - 1))) % len(modes)]}
        if kind == "transfer":
            ev["grid_head_mode"] = "flip"   # auto <-> gathered
        return ev
    if name == "fit":
        return {"kind": "fit", "epochs": 3, "cache": {"encoder": {"cache_frozen_encoder": True},
                                                      "steps": {"cache_frozen_steps": True}}.get(flag, {}),
                "seed": int(rng.integers(0, 1 << 16))}
    return {"kind": name}


def generate(seed=0):
    """The sequences of ROWS for this seed."""
    cases = []
    for r, (name, kind, dims, segments) in enumerate(ROWS):
        rng = np.random.default_rng([seed, r])
        events, cur = [], None
        for pattern, specs in segments:
            if cur is not None:
                events.append({"kind": "recompile", "pattern": pattern})
            cur = pattern
            for at in rng.permutation(len(specs)):
                ev = _event(specs[at], kind, dims, len(events), rng)
                assert valid(ev["kind"], cur, kind, dims), (name, ev, cur)
                events.append(ev)
        assert 5 <= len(events) <= 8 and sum(e["kind"] == "graphed" for e in events) <= 1, (name, len(events))
        cases.append(Case(name, kind, dict(dims), segments[0][0], tuple(events), seed))
    return cases


CASES = generate(0)
BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------------------------------------------------------- cells
def possible_cells():
    """The (event kind, slot class) pairs for which an event of that kind CAN change a source of a slot of that class:
    some kind of model, some pattern the event is valid under, some variable."""
    out = set()
    for kind in ("viscosity", "melting_point", "transfer"):
        dep = depends(kind, DIMS)
        names = set(variable_names(kind, DIMS["S"])) | (set(MOVING) if kind == "transfer" else set())
        for ek in EVENT_KINDS:
            if ek == "mode":
                continue
            for pattern in patterns(kind):
                if not valid(ek, pattern, kind, DIMS):
                    continue
                changed = names if ek in ("reload", "inplace") else Case("", kind, DIMS, pattern, ({"kind": ek, "pattern": pattern},), 0).changes(0)
                for slot, src in dep.items():
                    if changed & src:
                        out.add((ek, slot_class(slot)))
    return out


def covered_cells(cases):
    """-> (touched, spared): the (event kind, slot class) pairs some sequence's event changes a source of, and the slot
    classes of which some event of some sequence leaves every source of every slot alone."""
    touched, spared = set(), set()
    for c in cases:
        for i, ev in enumerate(c.events):
            per_class = {}
            for slot, hit in c.touched(i).items():
                per_class.setdefault(slot_class(slot), []).append(hit)
            for cls, hits in per_class.items():
                if any(hits):
                    touched.add((ev["kind"], cls))
                else:
                    spared.add(cls)
    return touched, spared


# ------------------------------------------------------------------------------------------------------ the frozen caches
def frozen_expectation(case):
    """[(event i, "enc" | "st", must_be_stale)] for the sequence's data.FrozenEncodings / data.FrozenStates object.  The
    GPU test builds each where the pattern in force allows it (``valid`` "stage1" / "stage2"), before the first event
    and again after any event that leaves it missing or stale, so an object that exists before event i was current
    then: it must report stale after the event when the event changed a variable it holds copies of, and may report
    either otherwise (a conservative True is allowed)."""
    out, before = [], case.pattern
    for i, after in enumerate(case.in_force()):
        ch = case.changes(i)
        if valid("stage1", before, case.kind, case.dims):
            out.append((i, "enc", bool(ch & set(encoder_names(case.kind, case.S)))))
        if valid("stage2", before, case.kind, case.dims):
            moved = prefix(after, case.kind, case.S) != prefix(before, case.kind, case.S)
            out.append((i, "st", moved or bool(ch & states_sources(prefix(before, case.kind, case.S), case.kind, case.S))))
        before = after
    return out


def apply_pattern(model, pattern):
    """Sets every weighted layer's ``trainable`` flag to the pattern's (``compile()`` then reads them)."""
    groups = pattern_groups(pattern, model.kind, model.num_steps)
    for name, _, layer in model._owned_tensors():
        layer.trainable = group(name) in groups


# --------------------------------------------------------------------------------------------------------------- inputs
def perturbed(state, seed):
    """A state dict near ``state`` with every variable changed: the dict of a reload event."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, v in state.items():
        a = np.asarray(v, np.float32)
        b = a * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=a.shape)) + 0.01 * rng.choice([-1.0, 1.0], size=a.shape)
        out[k] = (np.abs(b) + 0.1 if k.endswith("moving_variance") else b).astype(np.float32)
    return out
