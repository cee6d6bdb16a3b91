"""The cache fuzz on the CPU: (1) the generator of tests/cache_cases.py is deterministic and covers every event kind and
every (event kind, slot) cell an event can reach; (2) its names, patterns and prefixes are the model's; (3) the
invalidation rules of MPNNModel against cache_cases.DEPENDS, without a kernel: sentinel objects in every slot, a
freezing pattern through compile(), weights_updated() - a slot survives exactly when none of its sources trains;
invalidate_packed_weights() and load_weights clear everything; (4) data.FrozenStates made before a compile that moved
the prefix stay stale when a later compile brings the prefix back."""
import numpy as np
import pytest
import torch

from ionic_mpnn_amd import data, layers as L, model as MM, train

import cache_cases as CC
from test_frozen_states_host import _Tables, _set

CPU = torch.device("cpu")
KINDS = ("viscosity", "melting_point", "transfer")


def model(kind, dims=CC.DIMS):
    L.reset_uids()
    return MM.MPNNModel(kind, dims["Va"], dims["Vb"], dims["D"], dims["K"], dims["F"], dims["Mx"], dims["S"], 1e-4,
                        device=CPU, head_dropout_seed=3)


def compiled(m, pattern):
    CC.apply_pattern(m, pattern)
    return m.compile(train.Adam(CC.RATE), loss="huber" if m.kind == "transfer" else "mse")


# ------------------------------------------------------------------------------------------------------- (1) the generator
def test_the_generator_is_deterministic_and_every_row_is_well_formed():
    assert CC.generate(0) == CC.generate(0) == CC.CASES and CC.generate(7) == CC.generate(7)
    assert [c.events for c in CC.generate(7)] != [c.events for c in CC.CASES]   # the seed reaches the sequences
    kinds = lambda cases: sorted((c.name, sorted(e["kind"] for e in c.events)) for c in cases)
    assert kinds(CC.generate(7)) == kinds(CC.CASES)   # ... their order and parameters, not what a row holds
    assert len({c.name for c in CC.CASES}) == len(CC.CASES)
    assert {c.kind for c in CC.CASES} == set(KINDS)
    assert sum(c.dims["D"] == 64 for c in CC.CASES) == 1 and all(c.dims["D"] in (32, 64) for c in CC.CASES)
    for c in CC.CASES:
        assert {k: c.dims[k] for k in ("K", "F", "Mx", "S", "Va", "Vb")} == dict(K=8, F=32, Mx=20, S=3, Va=11, Vb=6)
        assert 5 <= len(c.events) <= 8 and sum(e["kind"] == "graphed" for e in c.events) <= 1, c.name
        for ev, pattern in zip(c.events, c.in_force()):
            assert ev["kind"] in CC.EVENT_KINDS and CC.valid(ev["kind"], pattern, c.kind, c.dims), (c.name, ev)
            assert CC.trainable(pattern, c.kind, c.S), (c.name, pattern)
            if ev["kind"] == "inplace":
                assert ev["variable"] in CC.variable_names(c.kind, c.S), (c.name, ev)
            if ev["kind"] == "fit" and "cache_frozen_encoder" in ev["cache"]:
                assert CC.valid("stage1", pattern, c.kind, c.dims), c.name
            if ev["kind"] == "fit" and "cache_frozen_steps" in ev["cache"]:
                assert CC.valid("stage2", pattern, c.kind, c.dims), c.name


def test_every_event_kind_and_every_required_pattern_appears():
    events = [e for c in CC.CASES for e in c.events]
    assert {e["kind"] for e in events} == set(CC.EVENT_KINDS)
    assert any(e["kind"] == "reload" and e["via_file"] for e in events) and any(
        e["kind"] == "reload" and not e["via_file"] for e in events)
    fits = [e["cache"] for e in events if e["kind"] == "fit"]
    assert {} in fits and {"cache_frozen_encoder": True} in fits and {"cache_frozen_steps": True} in fits
    used = {(c.kind == "transfer", p) for c in CC.CASES for p in c.in_force() + [c.pattern]}
    for p in ("everything", "head", "cat_last", "bmm_only", "atom_emb", "bond_emb"):
        assert any(q == p for _, q in used), p
    for p in ("stage1", "stage2", "mixed", "bn_only", "dense1_only", "tail_one", "everything"):
        assert (True, p) in used, p
    modes = {e["encoder_mode"] for e in events if e["kind"] == "mode"}
    assert len(modes) >= 3 and any(e.get("grid_head_mode") for e in events if e["kind"] == "mode")


def test_every_reachable_cell_is_covered_and_every_slot_is_spared_once():
    possible = CC.possible_cells()
    touched, spared = CC.covered_cells(CC.CASES)
    assert not [cell for cell in possible if cell[0] == "mode"] and not [cell for cell in touched if cell[0] == "mode"]
    assert {cell for cell in possible if cell[0] == "forward"} == {("forward", "transfer_image")}
    assert touched <= possible, sorted(touched - possible)
    assert possible <= touched, f"cells no sequence covers: {sorted(possible - touched)}"
    # what an event cannot reach is not in the table by construction: stage 1 needs a frozen encoder
    assert not {("stage1", s) for s in ("packed", "prepared", "mats", "frozen_encodings", "split_deg_limit")} & possible
    assert ("stage1", "transfer_image") in possible and ("stage2", "packed") in possible
    for kind in KINDS:
        assert set(CC.slot_classes(kind)) <= spared, kind
    for seed in (1, 2, 3):   # the coverage does not depend on the seed
        assert CC.covered_cells(CC.generate(seed))[0] == touched


def test_both_answers_of_stale_are_asked_of_both_frozen_caches():
    asked = {(obj, must) for c in CC.CASES for _, obj, must in CC.frozen_expectation(c)}
    assert asked == {("enc", True), ("enc", False), ("st", True), ("st", False)}
    # the sequence that leaves a prefix and comes back to it: the states exist before, something below them trains
    back = [c for c in CC.CASES for (i, obj, must) in CC.frozen_expectation(c)
            if obj == "st" and must and c.events[i]["kind"] == "recompile"
            and CC.prefix(c.in_force()[i], c.kind, c.S) in [CC.prefix(p, c.kind, c.S) for p in [c.pattern] + c.in_force()[:i]]]
    assert back


# ------------------------------------------------------------------------------------------------ (2) names and patterns
@pytest.mark.parametrize("kind", KINDS)
def test_names_patterns_and_prefixes_are_the_models(kind):
    m = model(kind)
    S = m.num_steps
    assert CC.variable_names(kind, S) == list(m._named_tensors())
    assert set(m._named_state()) == (set(CC.MOVING) if kind == "transfer" else set())
    for pattern in CC.patterns(kind):
        compiled(m, pattern)
        assert [n for n, _ in m.trainable_variables()] == CC.trainable(pattern, kind, S), pattern
        assert [n for n, t in m._named_tensors().items() if t.requires_grad] == CC.trainable(pattern, kind, S), pattern
        assert m.frozen_prefix() == CC.prefix(pattern, kind, S), pattern
        for ek, check in (("stage1", m._frozen_cache_check), ("stage2", m._frozen_steps_check)):
            try:
                check()
                accepted = True
            except ValueError:
                accepted = False
            assert accepted == CC.valid(ek, pattern, kind, CC.DIMS), (pattern, ek)
    # the head's packed order by name: what the packed head and the transfer grid image are documented to hold
    by_id = {id(t): n for n, t in m._named_tensors().items()}
    head = [by_id[id(t)] for t in m._head_tensors()]
    dep = CC.depends(kind, CC.DIMS)
    assert set(head) == dep["head_packed"] and len(head) == len(set(head))
    if kind == "transfer":
        import transfer_ref
        assert head == transfer_ref.HEAD_TENSORS
        assert dep["transfer_image"] == set(head[10:]) | set(CC.MOVING) == set(CC.TRANSFER_TAIL) | set(CC.MOVING)
        assert "mp_dense_1/kernel" not in dep["transfer_image"]
    assert dep["frozen_encodings"] == set(CC.variable_names(kind, S)) - dep["head_packed"]
    assert CC.depends(kind, CC.WIDE)["prepared:f32t"] == dep["prepared:f32t"] - {"atom_embedding"}


# --------------------------------------------------------------------------------------------------- (3) the invalidation
class Sentinel:
    def __init__(self, slot):
        self.slot = slot


def plant(m, dims):
    """A sentinel in every slot of cache_cases.depends -> {slot: sentinel}."""
    dep = CC.depends(m.kind, dims)
    s = {slot: Sentinel(slot) for slot in dep if slot != "frozen_encodings"}
    m._packed, m._split_deg_limit, m._head_packed = s["packed"], s["split_deg_limit"], s["head_packed"]
    m._prepared = {slot.split(":")[1]: v for slot, v in s.items() if slot.startswith("prepared:")}
    if m.kind == "transfer":
        m._transfer_grid_image = s["transfer_image"]
    for p in ("cat", "an"):
        for i, layer in enumerate(m.branches[p]["bmm"]):
            layer._mats_cache = s[f"mats:{p}_{i}"]
    return s


def held(m, slot):
    cls, _, arg = slot.partition(":")
    if cls == "prepared":
        return m._prepared.get(arg)
    if cls == "mats":
        p, i = arg.split("_")
        return getattr(m.branches[p]["bmm"][int(i)], "_mats_cache", None)
    return {"packed": m._packed, "split_deg_limit": m._split_deg_limit, "head_packed": m._head_packed,
            "transfer_image": m._transfer_grid_image}[cls]


def training(m):
    """The names whose values a step changes: what asks for a gradient, and the moving statistics of a
    BatchNormalization that runs on batch statistics."""
    names = {n for n, t in m._named_tensors().items() if t.requires_grad}
    if m.kind == "transfer" and m._bn_training:
        names |= set(CC.MOVING)
    return names


def check_weights_updated(m, dims, what):
    planted = plant(m, dims)
    dep = CC.depends(m.kind, dims)
    v_enc, v_st = m.encoder_version, m.frozen_state_version
    m.weights_updated()
    trains = training(m)
    for slot, sentinel in planted.items():
        survives = not (trains & dep[slot])
        assert (held(m, slot) is sentinel) == survives, (
            f"{what}: {slot} {'was dropped' if survives else 'survived'}; trains {sorted(trains & dep[slot])[:4]}")
        if not survives:
            assert held(m, slot) is None
    assert (m.encoder_version > v_enc) == bool(trains & dep["frozen_encodings"]), what
    assert m.frozen_state_version == v_st, what


RULE_ROWS = [(kind, dims, p) for kind in KINDS for dims in (CC.DIMS, CC.WIDE) for p in CC.patterns(kind)]


@pytest.mark.parametrize("kind,dims,pattern", RULE_ROWS, ids=[f"{k}-D{d['D']}-{p}" for k, d, p in RULE_ROWS])
def test_weights_updated_keeps_exactly_what_no_trained_variable_feeds(kind, dims, pattern):
    m = model(kind, dims)
    compiled(m, pattern)
    assert training(m) - set(CC.MOVING) == set(CC.trainable(pattern, kind, dims["S"]))
    check_weights_updated(m, dims, f"{kind} {pattern}")


def test_each_term_of_the_grid_image_rule_holds_alone():
    """compile() sets BatchNormalization's mode and its gamma / beta from one flag, so under every pattern the two terms
    of the image's rule cover for each other.  Held apart here: batch statistics with nothing of the image asking for a
    gradient (the moving statistics still change), and each tail variable asking alone with the layer in inference
    mode."""
    m = model("transfer")
    compiled(m, "dense1_only")
    m._bn_training = True
    check_weights_updated(m, CC.DIMS, "batch statistics alone")
    for name in CC.TRANSFER_TAIL + ("mp_dense_1/kernel", "cat_proj/bias"):
        compiled(m, "dense1_only")
        m._named_tensors()[name].requires_grad_(True)
        assert not m._bn_training
        check_weights_updated(m, CC.DIMS, f"{name} alone")


@pytest.mark.parametrize("kind", KINDS)
def test_invalidate_and_load_weights_clear_every_slot_and_move_both_versions(kind):
    m = model(kind)
    compiled(m, "head")   # (whatever trains: these two do not ask)
    for call in (m.invalidate_packed_weights, lambda: m.load_weights(m.state_dict())):
        planted = plant(m, CC.DIMS)
        v_enc, v_st = m.encoder_version, m.frozen_state_version
        call()
        for slot in planted:
            assert held(m, slot) is None, slot
        assert m._prepared == {} and m.encoder_version > v_enc and m.frozen_state_version > v_st


# ------------------------------------------------------------------------------------------- (4) a prefix left and regained
def test_states_stay_stale_when_the_prefix_comes_back(monkeypatch):
    """States made under one prefix, a compile under which what lies below it trains, a compile back: no version moved
    and the prefix is the states' own again, but a step in between may have changed every table row."""
    m = model("transfer")
    compiled(m, "stage2")
    _Tables.patch(m, monkeypatch)
    x, _ = _set(5)
    st = data.FrozenStates.build(m, x)
    assert not st.stale(m) and st.steps == {"cat": 1, "an": 1}
    compiled(m, "stage2")                    # the same prefix again: the states stay
    m.weights_updated()
    assert not st.stale(m)
    v = m.frozen_state_version
    compiled(m, "everything")
    m.weights_updated()                      # a step that trains step 0 and the embeddings
    assert st.stale(m)
    compiled(m, "stage2")
    assert m.frozen_state_version == v and m.frozen_prefix() == st.steps and st.stale(m)
    again = data.FrozenStates.build(m, x)
    assert not again.stale(m)
    plain = data.FrozenStates(again.cat, again.an, again.cat_row, again.an_row, again.steps, again.version)
    compiled(m, "everything")
    compiled(m, "stage2")
    assert again.stale(m) and not plain.stale(m)   # (a record made by hand carries no epoch: version and prefix alone)
