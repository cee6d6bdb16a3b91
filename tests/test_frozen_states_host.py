"""Cached frozen steps on the CPU: (1) MPNNModel.frozen_prefix() for the freezing patterns of stage 2; (2) every
refusal of cache_frozen_steps=True names its reason before any library call, and cache_frozen_encoder keeps its own;
(3) what makes data.FrozenStates stale: load_weights and a recompile that moves the prefix, never an optimizer step;
(4) the status codes of impnn_state_rows, seen without a device; (5) the name include/impnn.h declares is exported and
mirrored in _lib.SIGNATURES; (6) the record refuses what the kernel would have to trust."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, data, layers as L, model as MM, synthetic, train

_BAD = -1
CPU = torch.device("cpu")
UNFREEZE_KEYS = ["cat_bmm_2", "cat_bmm_3", "an_bmm_2", "an_bmm_3", "gated_update_2", "gated_update_3",
                 "gated_update_6", "gated_update_7", "mix_cat_an"]   # train_melting_point_transfer.py, stage 2


def model(kind="transfer", dropout_rate=0.0, fp_size=6, S=4):
    L.reset_uids()
    return MM.MPNNModel(kind, 11, 6, 8, 4, fp_size, 5, S, 1e-4, device=CPU, dropout_rate=dropout_rate, dropout_seed=1)


def head_only(m):
    for layer in m.layers:
        layer.trainable = layer.name.startswith("mp_") or layer.name == "melting_point"


def unfreeze(m, names):
    head_only(m)
    for layer in m.layers:
        if any(k in layer.name for k in names):
            layer.trainable = True


def stage2(m):
    unfreeze(m, UNFREEZE_KEYS)


def mixed(m):
    """tests/test_gpu_transfer.py's pattern of the same name."""
    head_only(m)
    for name in ("cat_bmm_3", "an_bmm_1", "gated_update_5", "gated_update_7", "dense_1"):
        m.get_layer(name).trainable = True
    m.get_layer("mp_dense_2").trainable = False


def cation_only(m):
    unfreeze(m, ["cat_bmm_2", "cat_bmm_3", "gated_update_2", "gated_update_3"])


# ------------------------------------------------------------------------------------------------- (1) prefixes
def test_frozen_prefix_of_the_freezing_patterns():
    m = model()
    for pattern, want in ((stage2, {"cat": 2, "an": 2}), (mixed, {"cat": 3, "an": 1}),
                          (cation_only, {"cat": 2, "an": None}), (head_only, {"cat": None, "an": None})):
        pattern(m)
        m.compile(train.Adam(1e-3), loss="huber")
        with torch.no_grad():   # read from the flags, whatever the grad mode of the caller
            assert m.frozen_prefix() == want, pattern.__name__
        assert m.frozen_prefix() == want, pattern.__name__
    stage2(m)
    m.bond_emb.trainable = True   # the bond embedding feeds every step's type matrices
    m.compile(train.Adam(1e-3), loss="huber")
    assert m.frozen_prefix() == {"cat": 0, "an": 0}
    stage2(m)
    m.get_layer("gated_update").trainable = True   # step 0 of the cation
    m.compile(train.Adam(1e-3), loss="huber")
    assert m.frozen_prefix() == {"cat": 0, "an": 2}


# ------------------------------------------------------------------------------------------------- (2) refusals
def _everything(m):
    for layer in m.layers:
        layer.trainable = True


def _visc_lower_frozen(m):
    for layer in m.layers:
        layer.trainable = not (layer.name.startswith("embedding") or layer.name in (
            "cat_bmm_0", "cat_bmm_1", "an_bmm_0", "an_bmm_1", "gated_update", "gated_update_1", "gated_update_4",
            "gated_update_5"))


REFUSALS = {
    "nothing frozen": (model, _everything, "mse", "nothing below the first trained step is frozen"),
    "all frozen": (model, head_only, "huber", "the whole encoder is frozen"),
    "all frozen points on": (model, head_only, "huber", "cache_frozen_encoder=True"),
    "encoder dropout": (lambda: model(dropout_rate=0.2), stage2, "huber", "GatedUpdate dropout rate is 0.2"),
    "widths": (lambda: model(fp_size=65), stage2, "huber", "not one of the fused loss nodes: the head kernels do not cover"),
    "viscosity huber": (lambda: model("viscosity"), _visc_lower_frozen, "huber",
                        "not one of the fused loss nodes: a viscosity model compiled with huber"),
    "melting point huber": (lambda: model("melting_point"), _visc_lower_frozen, "huber",
                            "not one of the fused loss nodes: a melting_point model compiled with huber"),
}


def _no_library():
    raise AssertionError("the library was reached before the flag was refused")


def _set(n=6):
    x = synthetic.make_batch(n, max_atoms=6, max_edges=8, atom_vocab_size=11, bond_vocab_size=6, min_atoms=2, seed=1)
    return x, np.zeros(n, np.float32)


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_steps_flag_is_refused_with_its_reason(what, monkeypatch):
    make, pattern, loss, reason = REFUSALS[what]
    m = make()
    pattern(m)
    m.compile(train.Adam(1e-3), loss=loss)
    x, y = _set()
    if m.kind == "viscosity":
        x["temperature"] = np.full(len(y), 300.0, np.float32)
    monkeypatch.setattr(_lib, "load", _no_library)
    rows = torch.arange(4)
    for call in (lambda: m.fit(x, y, cache_frozen_steps=True), lambda: m.frozen_states(x),
                 lambda: m.fit(x, y, validation_data=(x, y), cache_frozen_steps=True, graph=False),
                 lambda: m.train_on_state_batch(None, x, rows, y[:4]),
                 lambda: train.GraphedTrainStep(m, x, y, resident=(x, y), states=object())):
        with pytest.raises(ValueError) as err:
            call()
        assert "cache_frozen_steps" in str(err.value) and reason in str(err.value), str(err.value)


def test_distributed_and_both_flags_are_refused_and_the_encoder_flag_keeps_its_message(monkeypatch):
    from ionic_mpnn_amd import dist as idist
    m = model()
    stage2(m)
    m.compile(train.Adam(1e-4), loss="huber")
    m._frozen_steps_check()   # a stage-2 transfer model in one process is accepted
    x, y = _set()
    v = model("viscosity")
    _visc_lower_frozen(v)
    v.compile(train.Adam(1e-3), loss="mse")
    v._frozen_steps_check()   # a viscosity model with its lower steps frozen and mse is accepted too
    assert v.frozen_prefix() == {"cat": 2, "an": 2}
    monkeypatch.setattr(_lib, "load", _no_library)
    with pytest.raises(ValueError) as err:
        m.fit(x, y, cache_frozen_steps=True, cache_frozen_encoder=True)
    assert "cache_frozen_steps" in str(err.value) and "together with cache_frozen_encoder" in str(err.value)
    with pytest.raises(ValueError) as err:   # the stage-1 flag on a stage-2 model: its own refusal, as before
        m.fit(x, y, cache_frozen_encoder=True)
    assert "cache_frozen_encoder" in str(err.value) and "an encoder layer is trainable (stage 2)" in str(err.value)
    monkeypatch.setattr(idist, "is_distributed", lambda: True)
    for mdl in (m, v):
        with pytest.raises(ValueError, match="cache_frozen_steps.*torch.distributed is initialised"):
            mdl.fit(x, y, cache_frozen_steps=True)


# ------------------------------------------------------------------------------------------------- (3) staleness
class _Tables:
    """data.FrozenStates.build over a stand-in for the two device routes: the tables are functions of the ion arrays."""

    @staticmethod
    def patch(m, monkeypatch):
        def states(prefix, ions, steps, batch_size=4096):
            a = torch.as_tensor(np.asarray(ions["atom"], np.float32))
            return (a[:, :, None] * torch.arange(1, m.atom_dim + 1) + steps).contiguous()

        def encode_ions(cations=None, anions=None, batch_size=4096):
            row = lambda s: None if s is None else torch.as_tensor(np.asarray(s["atom"], np.float32)).sum(1, keepdim=True) \
                * torch.ones(1, m.atom_dim)
            return row(cations), row(anions)
        monkeypatch.setattr(m, "frozen_step_states", states)
        monkeypatch.setattr(m, "encode_ions", encode_ions)


def test_what_makes_states_stale(monkeypatch):
    m = model()
    stage2(m)
    m.compile(train.Adam(1e-4), loss="huber")
    _Tables.patch(m, monkeypatch)
    x, _ = _set(9)
    x = {k: np.concatenate([v, v[:4]]) for k, v in x.items()}   # 13 samples over 9 + 9 ions
    st = data.FrozenStates.build(m, x)
    assert len(st) == 13 and st.steps == {"cat": 2, "an": 2} and st.version == m.frozen_state_version
    assert st.cat.shape == (9, 6, 8) and st.an.shape == (9, 6, 8) and st.device == CPU
    assert st.cat_row.dtype == torch.int32 and st.cat_row.tolist() == list(range(9)) + [0, 1, 2, 3]
    assert st.nbytes == 2 * 9 * 6 * 8 * 4 + 2 * 13 * 4
    assert torch.equal(st.cat[st.cat_row.long()][:, :, 0] - 2, torch.as_tensor(x["cat_atom"], dtype=torch.float32))
    # an optimizer step of a stage-2 model: the encoder's version moves (and must), the frozen-state version does not
    v_enc, v_st = m.encoder_version, m.frozen_state_version
    m.weights_updated()
    assert m.encoder_version > v_enc and m.frozen_state_version == v_st and not st.stale(m)
    # load_weights moves both
    v_enc = m.encoder_version
    m.load_weights(m.state_dict())
    assert m.encoder_version > v_enc and m.frozen_state_version > v_st and st.stale(m)
    st = data.FrozenStates.build(m, x)
    assert not st.stale(m)
    # a recompile that changes the prefix: stale without a version change
    v_st = m.frozen_state_version
    cation_only(m)
    m.compile(train.Adam(1e-4), loss="huber")
    assert m.frozen_state_version == v_st and st.stale(m)
    st = data.FrozenStates.build(m, x)   # the anion's whole encoder is frozen: one pooled row per anion
    assert st.steps == {"cat": 2, "an": None} and st.cat.shape == (9, 6, 8) and st.an.shape == (9, 1, 8)
    assert not st.stale(m)
    m.get_layer("cat_bmm_1").trainable = True
    m.compile(train.Adam(1e-4), loss="huber")
    assert m.frozen_prefix() == {"cat": 1, "an": None} and st.stale(m)
    # a recompile that leaves the prefix keeps the states
    st = data.FrozenStates.build(m, x)
    m.get_layer("mp_dense_2").trainable = False
    m.compile(train.Adam(1e-4), loss="huber")
    assert not st.stale(m)


def test_states_from_records_follow_unique_ions(monkeypatch):
    records, vocab = synthetic.make_id_records(9, seed=2, kind="melting_point")
    records = records + [dict(records[3]), dict(records[0], anion=records[5]["anion"])]
    ds = data.IonPairDataset(records, vocab)
    m = model()
    stage2(m)
    m.compile(train.Adam(1e-4), loss="huber")
    _Tables.patch(m, monkeypatch)
    st = data.FrozenStates.from_records(m, ds)
    cations, anions, cat_index, an_index = data.unique_ions(records)
    assert st.cat.shape[0] == len(cations) and st.an.shape[0] == len(anions) and len(st) == len(records)
    assert np.array_equal(st.cat_row.numpy(), cat_index) and np.array_equal(st.an_row.numpy(), an_index)
    built = data.FrozenStates.build(m, ds.build_inputs(range(len(ds))))   # the padded route finds the same ions
    assert torch.equal(built.cat_row, st.cat_row) and torch.equal(built.an_row, st.an_row)


# ------------------------------------------------------------------------------------------------- (6) the record
def test_the_record_refuses_what_the_kernel_would_have_to_trust():
    cat, an = torch.zeros(3, 5, 8), torch.zeros(2, 1, 8)
    cr, ar = torch.tensor([0, 2, 1, 1], dtype=torch.int32), torch.tensor([1, 0, 0, 1], dtype=torch.int32)
    ok = dict(cat=cat, an=an, cat_row=cr, an_row=ar, steps={"cat": 2, "an": None})
    st = data.FrozenStates(**ok, version=3)
    assert len(st) == 4 and st.version == 3 and st.steps == {"cat": 2, "an": None}
    only = data.FrozenStates(cat, None, cr, ar, {"cat": 1, "an": 0})
    assert only.an is None and only.nbytes == 3 * 5 * 8 * 4 + 2 * 4 * 4
    for bad in (dict(cat_row=torch.tensor([0, 3, 1, 1], dtype=torch.int32)),
                dict(an_row=torch.tensor([1, 0, -1, 1], dtype=torch.int32)), dict(cat_row=cr.long()),
                dict(an_row=ar[:-1].contiguous()), dict(an=torch.zeros(2, 5, 8)), dict(an=torch.zeros(2, 1, 4)),
                dict(cat=cat.double()), dict(cat=torch.zeros(3, 5, 6)), dict(cat=None),
                dict(steps={"cat": 0, "an": None}), dict(cat=None, an=None, steps={"cat": 0, "an": 0})):
        with pytest.raises(ValueError):
            data.FrozenStates(**{**ok, **bad})


# ------------------------------------------------------------------------------------------------- (4) status codes
def test_state_rows_status_codes():
    """Every call returns before any device call: the pointers are addresses inside a host buffer that nothing
    dereferences.  Order: n_ions, B (0 is IMPNN_OK whatever else is passed), the host arrays, then per ion the null
    pointers, row_floats, table_rows, the alignment of tables / out (16 bytes) and of rows (4 bytes)."""
    lib = _lib.load()
    host = (C.c_char * 1024)()
    at = (C.addressof(host) + 63) & ~63
    p = lambda i: at + 64 * i
    entry = b"impnn_state_rows"

    def call(n=2, tables=(p(1), p(2)), rows=(p(3), p(4)), out=(p(5), p(6)), rf=(8, 1028), tr=(3, 50), B=9, arrays=True):
        arr = lambda v: C.cast((C.c_void_p * 2)(*v), _lib.PP) if v is not None else None
        i64 = lambda v: (C.c_int64 * 2)(*v) if v is not None else None
        rc = lib.impnn_state_rows(n, arr(tables), arr(rows), arr(out), i64(rf), i64(tr), B, None)
        return rc, lib.impnn_last_error_string()

    for n in (0, 3, -1):
        rc, msg = call(n=n)
        assert rc == _BAD and msg == entry + b": n_ions must be 1 or 2", (n, msg)
    rc, msg = call(B=-1)
    assert rc == _BAD and msg == entry + b": bad shape", msg
    # B == 0: nothing to do, nothing looked at - not even null pointers
    rc, _ = call(B=0, tables=None, rows=None, out=None, rf=None, tr=None)
    assert rc == 0
    rc, _ = call(B=0, rf=(0, 3))
    assert rc == 0
    for kw in (dict(tables=None), dict(rows=None), dict(out=None), dict(rf=None), dict(tr=None),
               dict(tables=(p(1), None)), dict(rows=(None, p(4))), dict(out=(p(5), None))):
        rc, msg = call(**kw)
        assert rc == _BAD and msg == entry + b": null pointer", (kw, msg)
    for rf in ((0, 8), (8, -4), (8, 6), (1027, 8), (8, 2)):
        rc, msg = call(rf=rf)
        assert rc == _BAD and msg == entry + b": row_floats must be a positive multiple of 4", (rf, msg)
    rc, msg = call(tr=(3, -1))
    assert rc == _BAD and msg == entry + b": table_rows must not be negative", msg
    for off in (4, 8, 12, 1):
        for kw in (dict(tables=(p(1) + off, p(2))), dict(out=(p(5), p(6) + off))):
            rc, msg = call(**kw)
            assert rc == _BAD and msg == entry + b": tables and out must be 16-byte aligned", (kw, msg)
    for off in (1, 2, 3):
        rc, msg = call(rows=(p(3), p(4) + off))
        assert rc == _BAD and msg == entry + b": rows must be 4-byte aligned", (off, msg)
    rc, msg = call(rf=(8, 6), rows=(None, p(4)))   # the first ion's null pointer comes before the second's row_floats
    assert rc == _BAD and msg == entry + b": null pointer", msg
    assert lib.impnn_abi_version() == 3   # additions only


# ------------------------------------------------------------------------------------------------- (5) exports
def test_declared_name_is_exported():
    text = (pathlib.Path(__file__).resolve().parents[1] / "include" / "impnn.h").read_text()
    name = "impnn_state_rows"
    assert len(re.findall(r"\bint " + name + r"\(", text)) == 1
    assert name in _lib.SIGNATURES
    fn = getattr(_lib.load(), name)   # AttributeError where the symbol is not exported
    params = re.search(r"\bint " + name + r"\((.*?)\);", text, re.S).group(1)
    assert len(params.split(",")) == len(_lib.SIGNATURES[name][1]) == len(fn.argtypes)
