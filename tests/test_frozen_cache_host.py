"""Cached encodings of a frozen encoder on the CPU: (1) data.unique_padded_ions / data.FrozenEncodings - tables[rows] are
the per-sample rows, first-occurrence order, a graph that is both a cation and an anion is a row of each table, bad
indices are refused; (2) every refusal of cache_frozen_encoder=True names its reason before any library call; (3) what
the indexed C entries can see without a device is a status code, in the documented order; (4) the names include/impnn.h
declares for them are exported and mirrored in _lib.SIGNATURES."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, data, layers as L, model as MM, synthetic, train

_BAD, _UNS, _WORKSPACE = -1, -2, -4
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------- (1) the record
def repeated_inputs(n=23, n_cat=5, n_an=4, N=7, E=6, seed=0):
    """Padded inputs whose samples draw from n_cat + n_an ion graphs; graph 0 of the cations IS graph 0 of the anions.
    -> (inputs, cat_of, an_of): which graph each sample holds."""
    rng = np.random.default_rng(seed)
    pool = synthetic.make_batch(n_cat + n_an, max_atoms=N, max_edges=E, atom_vocab_size=11, bond_vocab_size=6,
                                min_atoms=2, seed=seed + 1)
    cats = [tuple(pool[f"cat_{k}"][i] for k in ("atom", "bond", "connectivity")) for i in range(n_cat)]
    ans = [cats[0]] + [tuple(pool[f"an_{k}"][i] for k in ("atom", "bond", "connectivity")) for i in range(1, n_an)]
    cat_of, an_of = rng.integers(0, n_cat, n), rng.integers(0, n_an, n)
    cat_of[:3], an_of[:3] = [2, 0, 2], [1, 1, 0]   # first occurrences out of graph order; sample 1 / 2 share graph 0
    inputs = {}
    for p, graphs, of in (("cat", cats, cat_of), ("an", ans, an_of)):
        for j, k in enumerate(("atom", "bond", "connectivity")):
            inputs[f"{p}_{k}"] = np.stack([graphs[g][j] for g in of]).astype(np.int32)
    return inputs, cat_of, an_of


def first_occurrence(of):
    order = []
    for g in of:
        if g not in order:
            order.append(int(g))
    return order


def test_unique_padded_ions_round_trip_and_order():
    inputs, cat_of, an_of = repeated_inputs()
    cations, anions, cat_row, an_row = data.unique_padded_ions(inputs)
    assert cat_row.dtype == np.int32 and an_row.dtype == np.int32 and cat_row.shape == (len(cat_of),)
    for p, species, row, of in (("cat", cations, cat_row, cat_of), ("an", anions, an_row, an_of)):
        order = first_occurrence(of)
        assert len(species["atom"]) == len(order), "one row per distinct graph"
        for k in ("atom", "bond", "connectivity"):
            assert species[k].dtype == np.int32
            assert np.array_equal(species[k][row], inputs[f"{p}_{k}"]), f"{p}_{k}: tables[rows] are the samples' rows"
        assert np.array_equal(row, [order.index(int(g)) for g in of]), "first-occurrence order"
    # the graph both sides share is a row of each table, once
    shared = [inputs["cat_atom"][1], inputs["cat_bond"][1], inputs["cat_connectivity"][1]]
    for species in (cations, anions):
        hits = [i for i in range(len(species["atom"]))
                if all(np.array_equal(species[k][i], s) for k, s in zip(("atom", "bond", "connectivity"), shared))]
        assert len(hits) == 1
    # torch tensors are taken as numpy arrays are
    again = data.unique_padded_ions({k: torch.from_numpy(v) for k, v in inputs.items()})
    assert np.array_equal(again[2], cat_row) and np.array_equal(again[3], an_row)
    with pytest.raises(ValueError):
        data.unique_padded_ions(dict(inputs, cat_bond=inputs["cat_bond"][:-1]))


class _RowSumEncoder:
    """Stands in for a model: an ion's 'pooled row' is a fixed function of its padded arrays."""
    device, encoder_version = CPU, 7

    def encode_ions(self, cations, anions, batch_size=4096):
        def rows(s):
            flat = np.concatenate([s[k].reshape(len(s["atom"]), -1) for k in ("atom", "bond", "connectivity")], 1)
            w = np.arange(1, flat.shape[1] + 1, dtype=np.float32)
            return torch.from_numpy(np.stack([flat * w, flat + w], 1).sum(2).astype(np.float32))
        return rows(cations), rows(anions)


def test_frozen_encodings_tables_indexed_are_the_per_sample_rows():
    inputs, cat_of, an_of = repeated_inputs()
    m = _RowSumEncoder()
    enc = data.FrozenEncodings.build(m, inputs)
    assert len(enc) == len(cat_of) and enc.version == 7 and not enc.stale(m)
    assert enc.cat.shape == (len(set(cat_of)), 2) and enc.an.shape == (len(set(an_of)), 2)
    assert enc.cat_row.dtype == torch.int32 and enc.an_row.dtype == torch.int32
    per_cat, per_an = m.encode_ions({k: inputs[f"cat_{k}"] for k in ("atom", "bond", "connectivity")},
                                    {k: inputs[f"an_{k}"] for k in ("atom", "bond", "connectivity")})
    assert torch.equal(enc.cat[enc.cat_row.long()], per_cat) and torch.equal(enc.an[enc.an_row.long()], per_an)
    m.encoder_version = 8
    assert enc.stale(m)
    # a record refuses what a kernel would have to trust
    ok = dict(cat=enc.cat, an=enc.an, cat_row=enc.cat_row, an_row=enc.an_row)
    for bad in (dict(cat_row=enc.cat_row.clone().index_fill_(0, torch.tensor([2]), enc.cat.shape[0])),
                dict(an_row=enc.an_row.clone().index_fill_(0, torch.tensor([0]), -1)),
                dict(cat_row=enc.cat_row.long()), dict(an_row=enc.an_row[:-1].contiguous()),
                dict(an=enc.an[:, :1].contiguous()), dict(cat=enc.cat.double())):
        with pytest.raises(ValueError):
            data.FrozenEncodings(**{**ok, **bad})


def test_frozen_encodings_from_records_follow_unique_ions():
    records, vocab = synthetic.make_id_records(9, seed=2, kind="melting_point")
    records = records + [dict(records[3]), dict(records[0], anion=records[5]["anion"])]   # repeated ions, a new pairing
    ds = data.IonPairDataset(records, vocab)
    m = _RowSumEncoder()
    enc = data.FrozenEncodings.from_records(m, ds)
    cations, anions, cat_index, an_index = data.unique_ions(records)
    assert enc.cat.shape[0] == len(cations) and enc.an.shape[0] == len(anions) and len(enc) == len(records)
    assert np.array_equal(enc.cat_row.numpy(), cat_index) and np.array_equal(enc.an_row.numpy(), an_index)
    built = data.FrozenEncodings.build(m, ds.build_inputs(range(len(ds))))   # the padded route finds the same ions
    assert torch.equal(built.cat[built.cat_row.long()], enc.cat[enc.cat_row.long()])
    assert torch.equal(built.an_row, enc.an_row) and torch.equal(built.cat_row, enc.cat_row)


def test_model_encoder_version_moves_with_load_weights():
    m = transfer_model()
    v0 = m.encoder_version
    m.load_weights(m.state_dict())
    assert m.encoder_version > v0
    v1 = m.encoder_version
    stage1(m)
    m.compile(train.Adam(1e-3), loss="huber")
    m.weights_updated()   # a step that trains the head alone leaves the encoder's version
    assert m.encoder_version == v1
    m.get_layer("cat_bmm_1").trainable = True
    m.compile(train.Adam(1e-3), loss="huber")
    m.weights_updated()   # a step that trains an encoder layer moves it on
    assert m.encoder_version > v1


# ------------------------------------------------------------------------------------------------- (2) refusals
def transfer_model(dropout_rate=0.0, kind="transfer", fp_size=6):
    L.reset_uids()
    return MM.MPNNModel(kind, 11, 6, 8, 4, fp_size, 5, 2, 1e-4, device=CPU, dropout_rate=dropout_rate, dropout_seed=1)


def stage1(m):
    for layer in m.layers:
        layer.trainable = layer.name.startswith("mp_") or layer.name == "melting_point"


REFUSALS = {
    "base model": (lambda: transfer_model(kind="melting_point"), lambda m: None, "melting_point model"),
    "trainable encoder step": (transfer_model, lambda m: setattr(m.get_layer("an_bmm_1"), "trainable", True),
                               "an encoder layer is trainable"),
    "encoder dropout": (lambda: transfer_model(dropout_rate=0.2), lambda m: None, "GatedUpdate dropout rate is 0.2"),
    "widths": (lambda: transfer_model(fp_size=65), lambda m: None, "head kernels do not cover"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_cache_flag_is_refused_with_its_reason(what, monkeypatch):
    make, change, reason = REFUSALS[what]
    m = make()
    if m.kind == "transfer":
        stage1(m)
    change(m)
    m.compile(train.Adam(1e-3))
    n = 6
    x = synthetic.make_batch(n, max_atoms=6, max_edges=8, atom_vocab_size=11, bond_vocab_size=6, min_atoms=2, seed=1)
    y = np.zeros(n, np.float32)

    def no_library():
        raise AssertionError("the library was reached before the flag was refused")
    monkeypatch.setattr(_lib, "load", no_library)
    for call in (lambda: m.fit(x, y, cache_frozen_encoder=True), lambda: m.evaluate(x, y, cache_frozen_encoder=True),
                 lambda: m.fit(x, y, validation_data=(x, y), cache_frozen_encoder=True, graph=False),
                 lambda: m.frozen_encodings(x)):
        with pytest.raises(ValueError) as err:
            call()
        assert "cache_frozen_encoder" in str(err.value) and reason in str(err.value), str(err.value)


def test_distributed_refusal_names_its_reason(monkeypatch):
    from ionic_mpnn_amd import dist as idist
    m = transfer_model()
    stage1(m)
    m.compile(train.Adam(1e-3))
    m._frozen_cache_check()   # a stage-1 transfer model in one process is accepted
    monkeypatch.setattr(idist, "is_distributed", lambda: True)
    with pytest.raises(ValueError, match="torch.distributed is initialised"):
        m._frozen_cache_check()


# ------------------------------------------------------------------------------------------------- (3) status codes
def test_indexed_entries_status_codes():
    """Every call returns before any device call: the pointers are addresses inside a host buffer that nothing
    dereferences.  Order: dropout, shape (B == 0 is IMPNN_OK), loss kind, null pointers, the weights' alignment, the
    index (null, alignment, C / A), buffer sizes, widths."""
    lib = _lib.load()
    host = (C.c_char * 1024)()
    at = C.addressof(host)
    p = lambda i: at + 16 * (i + 1)
    table = C.cast((C.c_void_p * 18)(*[p(20 + i) for i in range(18)]), _lib.PP)
    lam = (C.c_float * 18)()
    WS = 1 << 40

    def fwd(cat_row=p(10), an_row=p(11), sw=None, y=p(4), B=9, Cn=3, An=2, D=32, ws=WS, saved=WS, rate=0.0):
        rc = lib.impnn_transfer_head_loss_rows(p(0), p(1), cat_row, an_row, table, lam, p(2), p(3), 0.99, 1e-3, 1, y, sw,
                                               1, 1.0, rate, 0, None, 0, p(6), saved, None, p(7), p(8), ws, B, Cn, An, D,
                                               32, 20, None)
        return rc, lib.impnn_last_error_string()

    def bwd(cat_row=p(10), an_row=p(11), sw=None, y=p(4), B=9, Cn=3, An=2, D=32, ws=WS, saved=WS, rate=0.0):
        rc = lib.impnn_transfer_head_loss_rows_bwd(p(0), p(1), cat_row, an_row, table, table, lam, 1, y, sw, 1, 1.0, p(5),
                                                   rate, 0, None, 0, p(6), saved, p(7), ws, B, Cn, An, D, 32, 20, None)
        return rc, lib.impnn_last_error_string()

    for call, entry in ((fwd, b"impnn_transfer_head_loss_rows"), (bwd, b"impnn_transfer_head_loss_rows_bwd")):
        for kw in (dict(cat_row=None), dict(an_row=None)):
            rc, msg = call(**kw)
            assert rc == _BAD and msg == entry + b": null row index", (entry, kw, msg)
        for off in (1, 2, 3):
            rc, msg = call(an_row=p(11) + off)
            assert rc == _BAD and msg == entry + b": cat_row and an_row must be 4-byte aligned", (entry, off, msg)
        for kw in (dict(Cn=0), dict(An=0), dict(Cn=-1)):
            rc, msg = call(**kw)
            assert rc == _BAD and b"C, A >= 1" in msg, (entry, kw, msg)
        rc, msg = call(cat_row=None, y=None)          # the null pointers come before the index
        assert rc == _BAD and msg == entry + b": null pointer", (entry, msg)
        rc, msg = call(cat_row=None, sw=p(12) + 2)    # and so does the weights' alignment
        assert rc == _BAD and msg == entry + b": sample_weight must be 4-byte aligned", (entry, msg)
        rc, msg = call(Cn=0, rate=1.5)                # the dropout arguments come first of all
        assert rc == _BAD and b"C, A" not in msg, (entry, msg)
        for sw in (None, p(12)):                      # with or without weights the call goes on to the widths
            rc, msg = call(D=129, sw=sw)
            assert rc == _UNS and b"D=129" in msg, (entry, msg)
        rc, msg = call(D=129, ws=3)                   # a short workspace answers before the widths
        assert rc == _WORKSPACE and b"workspace" in msg, (entry, rc, msg)
        rc, msg = call(saved=5)
        assert rc == _WORKSPACE and b"saved" in msg, (entry, rc, msg)
        # B == 0: nothing to do, nothing looked at - not even null pointers or empty tables
        rc, _ = call(B=0, cat_row=None, an_row=None, y=None, Cn=0, An=0, ws=0, saved=0)
        assert rc == 0, entry
        rc, msg = call(B=-1)
        assert rc == _BAD and msg == entry + b": bad shape", (entry, msg)
    # the entries they stand beside still refuse an empty batch
    rc = lib.impnn_weighted_transfer_head_loss(p(0), p(1), table, lam, p(2), p(3), 0.99, 1e-3, 1, p(4), None, 1, 1.0, 0.0,
                                               0, None, 0, p(6), WS, None, p(7), p(8), WS, 0, 32, 32, 20, None)
    assert rc == _BAD and lib.impnn_last_error_string() == b"impnn_weighted_transfer_head_loss: bad shape"
    assert lib.impnn_abi_version() == 3   # additions only


# ------------------------------------------------------------------------------------------------- (4) exports
def test_declared_names_are_exported():
    text = (pathlib.Path(__file__).resolve().parents[1] / "include" / "impnn.h").read_text()
    declared = sorted(set(re.findall(r"\bint (impnn_transfer_head_loss_rows\w*)\(", text)))
    assert declared == ["impnn_transfer_head_loss_rows", "impnn_transfer_head_loss_rows_bwd"]
    lib = _lib.load()
    for name in declared:
        assert name in _lib.SIGNATURES, name
        fn = getattr(lib, name)   # AttributeError where the symbol is not exported
        assert fn.argtypes is not None and len(fn.argtypes) == len(_lib.SIGNATURES[name][1])
        params = re.search(r"\bint " + name + r"\((.*?)\);", text, re.S).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[name][1]), name
