"""Cache fuzz: sequences of weight-changing events (tests/cache_cases.py) on one long-lived model; after construction and
after every event every inference path gives the bits of a model built fresh from the same variables.  Every other
fuzz builds a fresh model per case and runs it once, so none of them can see a stale derived copy of the weights: the
packed and prepared encoder weights (with the step-0 tables behind the typed images), the packed head, the transfer
grid image, each message layer's type matrices, data.FrozenEncodings / data.FrozenStates, what a captured step reads by
address, and what an ensemble reads from its members.

Exact: every output of the probe against the twin, by bit pattern (no tolerance appears); the set of variables an event
changes; the identity of every cached object none of whose sources an event changed; the tables of a frozen cache that
reports itself current.  Bounded: one fp64 check of ``predict`` at the end of a sequence (grad_ref.encode +
head_ref.forward / transfer_ref.head, 1e-5 through assert_close as the layer and head fuzzes hold the same widths), so
that the twin cannot be wrong in the same way as the model.  DESIGN.md 2 "Cache fuzz" has the mutant table."""
import numpy as np
import pytest
import torch

from ionic_mpnn_amd import data, layers as L, model as MM, synthetic, train
from ionic_mpnn_amd.ensemble import ModelEnsemble
from conftest import assert_close

import cache_cases as CC
import fit_cases as FC
import grad_ref as GR
import head_ref as HR
import transfer_ref as TRF

pytestmark = pytest.mark.gpu
DEV = "cuda"
METRICS = ["mae", "rmse"]
TEMPERATURES = np.array([298.15, 343.0], np.float32)
MODE_ID = {None: -1, "f32": 0, "f16x2": 1, "f32t": 2, "f32x3": 3}
OUTCOMES = {"enc": set(), "st": set()}   # what stale() answered over the sequences that ran
RAN = set()
WEIGHT_SEED = 11   # of the long-lived model's initial variables


# ------------------------------------------------------------------------------------------------------------ the inputs
class Data:
    """The fixed inputs of a kind: the probe's batch, the grids' species, the fit's set.  Shared, not to be written."""

    def __init__(self, kind, dims):
        mk = lambda n, seed: synthetic.make_batch(n, max_atoms=CC.N_ATOMS, max_edges=CC.N_EDGES, atom_vocab_size=dims["Va"],
                                                  bond_vocab_size=dims["Vb"], min_atoms=3, seed=seed)
        cut = lambda b: b if kind == "viscosity" else {k: v for k, v in b.items() if k != "temperature"}
        # targets around the initial model's own predictions, moved away from zero (tests/fit_cases.py): the steps then
        # do not train the output into a cancellation of the head's large intermediates, which no float32 head holds
        # to 1e-5 (with targets ~ N(0,1) the plain float32 reference itself sat at 0.5 x the bound of the end check)
        w0 = FC._make_weights(kind, dims, WEIGHT_SEED)
        target = lambda x, seed: (fp64_predict(kind, w0, x) - 8.0 - 16.0 * np.random.default_rng(seed).normal(
            size=len(x["cat_atom"]))).astype(np.float32)
        self.x = cut(mk(CC.BATCH, 21))
        self.y = target(self.x, 22)
        self.fx = cut(mk(CC.FIT_SAMPLES, 23))
        self.fy = target(self.fx, 24)
        C, A = CC.GRID[kind]
        b = mk(A, 25)
        ion = lambda p, n: {k: b[f"{p}_{k}"][:n] for k in ("atom", "bond", "connectivity")}
        self.cations, self.anions = ion("cat", C), ion("an", A)
        self.grid_kw = {"temperatures": TEMPERATURES} if kind == "viscosity" else {}
        self.x_dev = {k: torch.from_numpy(v).to(DEV).contiguous() for k, v in self.x.items()}
        self.rows = torch.arange(CC.BATCH, device=DEV)


_data = {}


def data_of(case):
    key = (case.kind, case.dims["D"])
    if key not in _data:
        _data[key] = Data(case.kind, case.dims)
    return _data[key]


def loss_of(kind):
    return train.Huber(1.0) if kind == "transfer" else "mse"


def build(case, seed):
    d = case.dims
    L.reset_uids()   # keras auto-names as from_config gives them: the twin finds every layer's flag by name
    m = MM.MPNNModel(case.kind, d["Va"], d["Vb"], d["D"], d["K"], d["F"], d["Mx"], d["S"],
                     1e-5 if case.kind == "melting_point" else 1e-4, device=DEV, head_dropout_seed=0x5EED)
    m.load_weights(FC._make_weights(case.kind, d, seed))
    return m


def compile_under(m, pattern):
    CC.apply_pattern(m, pattern)
    m.compile(train.Adam(CC.RATE), loss=loss_of(m.kind), metrics=METRICS)


def twin_of(m):
    """A model with no history: built from the config, loaded from the variables themselves."""
    t = MM.MPNNModel.from_config(m.get_config(), device=DEV)
    t.load_weights(m.state_dict())
    t.encoder_mode, t.grid_head_mode = m.encoder_mode, m.grid_head_mode
    assert (t.dropout_seed, t.dropout_rate) == (m.dropout_seed, m.dropout_rate)
    if m.kind == "transfer":
        assert t.mp_dropout.seed == m.mp_dropout.seed
    t.compile(train.Adam(CC.RATE), loss=m.loss, metrics=METRICS)   # the same flags: from_config carried the layers'
    assert [n for n, _ in t.trainable_variables()] == [n for n, _ in m.trainable_variables()]
    return t


# ------------------------------------------------------------------------------------------------------------- the probe
def probe(m, D, second):
    """Every inference path of the model -> {path: numpy array}."""
    out = {}
    N, E = D.x["cat_atom"].shape[1], D.x["cat_bond"].shape[1]
    current = m.encoder_mode
    for mode in CC.MODES[m.atom_dim]:
        m.encoder_mode = mode
        resolved = m.resolve_encoder_mode(N, E)
        out[f"resolved:{mode}"] = np.array([MODE_ID[resolved]])
        if resolved is not None:
            out[f"predict:{mode}"] = m.predict(D.x, fused=True)
    m.encoder_mode = current
    out["predict:layered"] = m.predict(D.x, fused=False)
    out["predict"] = m.predict(D.x)
    pc, pa = m.encode_ions(D.cations, D.anions)
    out["encode_ions:cat"], out["encode_ions:an"] = pc.cpu().numpy(), pa.cpu().numpy()
    ev = m.evaluate(D.x, D.y, batch_size=4, return_dict=True)
    assert list(ev) == ["loss"] + METRICS
    out["evaluate"] = np.array(list(ev.values()), np.float64)
    grid_mode = m.grid_head_mode
    for gm in (MM.MPNNModel.GRID_HEAD_MODES if m.kind == "transfer" else (grid_mode,)):
        m.grid_head_mode = gm
        tag = f"[{gm}]" if m.kind == "transfer" else ""
        if m.kind == "viscosity":
            out["predict_grid" + tag], out["predict_grid:params" + tag] = m.predict_grid(
                D.cations, D.anions, return_params=True, **D.grid_kw)
        else:
            out["predict_grid" + tag] = m.predict_grid(D.cations, D.anions)
        top = m.screen_top_k(D.cations, D.anions, k=5, **D.grid_kw)
        out["top_k:values" + tag], out["top_k:cation" + tag], out["top_k:anion" + tag] = top.values, top.cation, top.anion
    m.grid_head_mode = grid_mode
    out["predict_grid:current"] = m.predict_grid(D.cations, D.anions, **D.grid_kw)
    if second is not None:
        out["ensemble:mean"], out["ensemble:std"] = ModelEnsemble([m, second]).predict_grid(D.cations, D.anions, **D.grid_kw)
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(got, want, what):
    assert list(got) == list(want), what
    bad = [k for k in got if got[k].shape != want[k].shape or got[k].dtype != want[k].dtype
           or not np.array_equal(bits(got[k]), bits(want[k]))]
    assert not bad, f"{what}: other bits than the fresh model on {bad}"


# ------------------------------------------------------------------------------------------------------------- the slots
def held(m, slot):
    cls, _, arg = slot.partition(":")
    if cls == "prepared":
        return m._prepared.get(arg)
    if cls == "mats":
        p, i = arg.split("_")
        return getattr(m.branches[p]["bmm"][int(i)], "_mats_cache", None)
    return {"packed": m._packed, "split_deg_limit": m._split_deg_limit, "head_packed": getattr(m, "_head_packed", None),
            "transfer_image": m._transfer_grid_image}[cls]


def fillable(m, slot, probed):
    """The slots the probe fills: every one but the packed head of a transfer model (its head reads the variables;
    only an ensemble packs them), the images of modes the shape does not resolve to, and the frozen encodings."""
    cls, _, arg = slot.partition(":")
    if cls == "frozen_encodings" or (cls == "head_packed" and m.kind == "transfer"):
        return False
    return cls != "prepared" or arg in probed


def addresses(obj):
    """data_ptr of every tensor inside a cached object (a tensor, a list of them, a (key, tensor) pair)."""
    if torch.is_tensor(obj):
        return [obj.data_ptr()]
    if isinstance(obj, (list, tuple)):
        return [a for o in obj for a in addresses(o)]
    return []


def state_bits(m):
    return {k: bits(v).copy() for k, v in m.state_dict().items()}


# ------------------------------------------------------------------------------------------------------------ the events
class RestoreWitness(train.Callback):
    """Keeps the variables as the last epoch left them - the early stop's restore must replace them - and logs the
    epoch's number as ``epoch_rank``: monitored with mode "min", the best epoch is the first whatever the losses do."""

    def on_epoch_end(self, epoch, logs=None):
        self.last, self.epoch = state_bits(self.model), epoch
        logs["epoch_rank"] = float(epoch)


def run_event(m, case, i, D, ctx, tmp_path):
    ev = case.events[i]
    kind = ev["kind"]
    if kind == "recompile":
        compile_under(m, ev["pattern"])
        m.train_on_batch(D.x, D.y)
    elif kind == "eager":
        m.train_on_batch(D.x, D.y)
    elif kind == "graphed":
        step = ctx["captured"] = train.GraphedTrainStep(m, D.x, D.y)
        for _ in range(2):
            step(D.x_dev, D.y)
    elif kind == "stage1":
        assert ctx["enc"] is not None and not ctx["enc"].stale(m)
        for _ in range(2):
            m.train_on_encoded_batch(ctx["enc"], D.rows, D.y)
    elif kind == "stage2":
        assert ctx["st"] is not None and not ctx["st"].stale(m)
        for _ in range(2):
            m.train_on_state_batch(ctx["st"], D.x_dev, D.rows, D.y)
    elif kind == "fit":
        epochs = ev["epochs"]
        witness = RestoreWitness()
        stop = train.EarlyStopping("epoch_rank", patience=epochs + 1, restore_best_weights=True, mode="min")
        rate = train.LearningRateScheduler(lambda epoch, lr: CC.LAST_EPOCH_RATE if epoch == epochs - 1 else CC.RATE)
        h = m.fit(D.fx, D.fy, validation_data=(D.fx, D.fy), epochs=epochs, batch_size=CC.FIT_BATCH, callbacks=[rate, witness, stop],
                  seed=ev["seed"], graph=False, **ev["cache"])
        assert len(h.history["loss"]) == epochs and witness.epoch == epochs - 1
        assert stop.best_epoch == 0
        now, best = state_bits(m), {k: bits(v) for k, v in stop.best_weights.items()}
        trained = [n for n, _ in m.trainable_variables()]
        assert all(np.array_equal(now[k], best[k]) for k in now), "the restore did not bring the best epoch's variables"
        assert all(not np.array_equal(now[k], witness.last[k]) for k in trained), "the restore replaced nothing"
        m.optimizer.learning_rate = CC.RATE
    elif kind == "reload":
        w = CC.perturbed(m.state_dict(), ev["seed"])
        if ev["via_file"]:
            scratch = MM.MPNNModel.from_config(m.get_config(), device=DEV)
            scratch.load_weights(w)
            path = str(tmp_path / f"event{i}.keras")
            scratch.save(path)
            m.load_weights(path)
            loaded = MM.load_model(path, device=DEV)
            assert ({k: v for k, v in loaded.get_config().items() if k != "layers"}
                    == {k: v for k, v in m.get_config().items() if k != "layers"})
            loaded.encoder_mode, loaded.grid_head_mode = m.encoder_mode, m.grid_head_mode
            loaded.compile(train.Adam(CC.RATE), loss=m.loss, metrics=METRICS)
            ctx["loaded"] = loaded
        else:
            m.load_weights(w)
    elif kind == "inplace":
        with torch.no_grad():
            m._named_tensors()[ev["variable"]].mul_(ev["factor"]).add_(ev["shift"])
        m.invalidate_packed_weights()   # the documented contract of a write from outside
    elif kind == "forward":
        with torch.enable_grad():
            m(D.x, training=True)
    elif kind == "mode":
        m.encoder_mode = ev["encoder_mode"]
        if "grid_head_mode" in ev:
            m.grid_head_mode = "gathered" if m.grid_head_mode == "auto" else "auto"
    else:
        raise ValueError(kind)


def fp64_predict(kind, w, x):
    w64 = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in w.items()}
    pc = GR.encode(w, "cat", x["cat_atom"], x["cat_bond"], x["cat_connectivity"], torch.float64, pooled_only=True)
    pa = GR.encode(w, "an", x["an_atom"], x["an_bond"], x["an_connectivity"], torch.float64, pooled_only=True)
    if kind == "transfer":
        return TRF.head(w64, pc, pa)[0].numpy().reshape(-1)
    names = TRF.HEAD_TENSORS[:8] + (["visc_params/kernel", "visc_params/bias"] if kind == "viscosity" else
                                    ["mp_hidden/kernel", "mp_hidden/bias", "mp_out/kernel", "mp_out/bias"])
    T = torch.tensor(x["temperature"], dtype=torch.float64) if kind == "viscosity" else None
    return HR.forward(HR.KINDS[kind], [w64[n] for n in names], pc, pa, T).numpy().reshape(-1)


def same_tables(obj, fresh, what):
    for table in ("cat", "an", "cat_row", "an_row"):
        a, b = getattr(obj, table), getattr(fresh, table)
        assert (a is None) == (b is None), f"{what}: {table}"
        if a is not None:
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), \
                f"{what} reports itself current and its {table} differs from the table made now"


def check_frozen(m, t, case, i, D, ctx, must):
    """The frozen caches after event i (-1: construction): one that reports itself current holds, bit for bit, the
    tables the twin builds now; then the sequence's objects are made again where they are missing or stale."""
    pattern = case.pattern if i < 0 else case.in_force()[i]
    def made_now(cls, obj):
        """The object's tables from the twin, in the encoder mode the object was made in: a mode switch changes no
        weight, and cached rows keep the arithmetic they were made with."""
        t.encoder_mode, keep = ctx["made_in"][id(obj)], t.encoder_mode
        try:
            return cls.build(t, D.x)
        finally:
            t.encoder_mode = keep

    for name, cls, old in ctx["retired"]:   # an object that went stale once may never call itself current wrongly again
        if not old.stale(m):
            same_tables(old, made_now(cls, old), f"event {i}: a retired {name} object")
    for name, cls, ek in (("enc", data.FrozenEncodings, "stage1"), ("st", data.FrozenStates, "stage2")):
        obj = ctx[name]
        if obj is not None:
            stale = obj.stale(m)
            OUTCOMES[name].add(bool(stale))
            if must.get((i, name)):
                assert stale, f"event {i}: the {name} object holds copies of changed variables and reports itself current"
            if not stale:
                same_tables(obj, made_now(cls, obj), f"event {i}: the {name} object")
            else:
                ctx["retired"].append((name, cls, obj))
                ctx[name] = None
        if ctx[name] is None and CC.valid(ek, pattern, case.kind, case.dims):
            ctx[name] = m.frozen_encodings(D.x) if name == "enc" else m.frozen_states(D.x_dev)
            assert not ctx[name].stale(m)
            ctx["made_in"][id(ctx[name])] = m.encoder_mode
        assert (ctx[name] is not None) == CC.valid(ek, pattern, case.kind, case.dims), (i, name)


# --------------------------------------------------------------------------------------------------------------- the test
def run_sequence(case, tmp_path):
    D = data_of(case)
    m = build(case, WEIGHT_SEED)
    compile_under(m, case.pattern)
    second = build(case, 12) if case.kind != "transfer" else None
    dep = CC.depends(case.kind, case.dims)
    N, E = D.x["cat_atom"].shape[1], D.x["cat_bond"].shape[1]
    ctx = {"enc": None, "st": None, "captured": None, "loaded": None, "retired": [], "made_in": {}}
    must = {(i, name): stale for i, name, stale in CC.frozen_expectation(case)}

    # control: two fresh models agree bit for bit on every path, so bit equality is a fair demand of each
    t = twin_of(m)
    want = probe(t, D, second)
    same_bits(probe(twin_of(m), D, second), want, f"{case.name}: control, twin against twin")
    same_bits(probe(m, D, second), want, f"{case.name}: after construction")
    check_frozen(m, t, case, -1, D, ctx, must)

    for i, ev in enumerate(case.events):
        what = f"{case.name}: event {i} ({ev['kind']}, under {case.in_force()[i]})"
        # ---- every slot the probe can fill is warm: the event has something to invalidate
        m.encoder_mode, keep = "auto", m.encoder_mode
        probed = {m.resolve_encoder_mode(N, E)}
        for mode in CC.MODES[m.atom_dim]:
            m.encoder_mode = mode
            probed.add(m.resolve_encoder_mode(N, E))
        m.encoder_mode = keep
        before = {slot: held(m, slot) for slot in dep if fillable(m, slot, probed)}
        assert all(v is not None for v in before.values()), f"{what}: cold before the event: {[s for s, v in before.items() if v is None]}"
        assert {s for s in before if s.startswith("prepared:")} and {s for s in before if s.startswith("mats:")}
        where = {slot: addresses(v) for slot, v in before.items()}
        state = state_bits(m)

        run_event(m, case, i, D, ctx, tmp_path)

        # ---- the event changed exactly the variables it claims (moving statistics aside, as in the fit fuzz)
        after = state_bits(m)
        changed = {k for k in after if not np.array_equal(after[k], state[k])} - set(CC.MOVING)
        assert changed == case.changes(i) - set(CC.MOVING), (
            f"{what}: changed {sorted(changed - case.changes(i))} unclaimed, left {sorted(case.changes(i) - set(CC.MOVING) - changed)}")
        # ---- a slot none of whose sources changed holds the same object at the same addresses
        if ev["kind"] in CC.KEEPING:
            touched = case.touched(i)
            for slot, obj in before.items():
                if not touched[slot]:
                    assert held(m, slot) is obj and addresses(held(m, slot)) == where[slot], f"{what}: {slot} was rebuilt"
            if ctx["captured"] is not None and ev["kind"] == "graphed":
                refs = ctx["captured"]._cache_refs   # what the replays read by address
                kept = {id(o) for o in refs[1:] if o is not None} | {id(o) for o in refs[0].values()}
                for slot, obj in before.items():
                    if not touched[slot] and slot_class(slot) in ("packed", "prepared", "mats"):
                        assert id(obj) in kept, f"{what}: the captured step does not hold {slot}"
        # ---- every path against a model built now from the variables
        t = twin_of(m)
        check_frozen(m, t, case, i, D, ctx, must)
        want = probe(t, D, second)
        same_bits(probe(m, D, second), want, what)
        if ctx["loaded"] is not None:   # the save / load_model round trip is one more fresh model
            same_bits(probe(ctx["loaded"], D, second), want, f"{what}: load_model")
            ctx["loaded"] = None

    # ---- the twin cannot be wrong in the same way: fp64 on the final variables
    ref = fp64_predict(case.kind, m.state_dict(), D.x)
    assert_close(m.predict(D.x).reshape(-1), ref, 1e-5, f"{case.name}: predict against fp64 at the end")


def slot_class(slot):
    return CC.slot_class(slot)


@pytest.mark.parametrize("name", [c.name for c in CC.CASES])
def test_every_path_follows_the_variables(name, tmp_path):
    run_sequence(CC.BY_NAME[name], tmp_path)
    RAN.add(name)


def test_both_answers_of_stale_occurred():
    """Over the whole table a frozen cache reports itself stale at least once and current at least once, each kind.
    (Says nothing when only part of the table ran in this process.)"""
    if RAN == {c.name for c in CC.CASES}:
        assert OUTCOMES == {"enc": {True, False}, "st": {True, False}}, OUTCOMES
