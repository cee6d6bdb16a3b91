"""Row-restricted embedding training, host side: which tokens a data set uses (data.token_usage / unseen_tokens), the
validation and persistence of Embedding.trainable_rows, what compile() makes of it without a device, and the argument
checks of impnn_embed_rows_bwd in their documented order (none of them reaches a launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

import footprint as F
from ionic_mpnn_amd import _lib, autograd, data, layers as L, model as MM, synthetic, train

CPU = torch.device("cpu")
VA, VB = 11, 6
_BAD, _UNSUPPORTED = -1, -2


# ------------------------------------------------------------------------------------------------- (1) token usage
def _inputs(cat_atom, cat_bond, cat_conn, an_atom, an_bond, an_conn):
    i32 = lambda a: np.asarray(a, np.int32)
    return {"cat_atom": i32(cat_atom), "cat_bond": i32(cat_bond), "cat_connectivity": i32(cat_conn),
            "an_atom": i32(an_atom), "an_bond": i32(an_bond), "an_connectivity": i32(an_conn)}


def _hand_made():
    """Two samples.  Cation atoms 3, 3, 4 | 5; anion atoms 7 | 7, 0 (a padding atom between real ones is no token).
    Cation edges: bond 2 valid, bond 1 with source 0, bond 4 with target 0, bond VB (outside) | bond 2 and bond 0 valid,
    bond -1 outside.  The anions have one valid edge of bond 5 in sample 1."""
    cat_atom = [[3, 3, 4, 0], [5, 0, 0, 0]]
    cat_bond = [[2, 1, 4, VB], [2, 0, -1, 3]]
    cat_conn = [[[1, 2], [0, 1], [2, 0], [1, 2]], [[1, 1], [2, 3], [1, 2], [0, 0]]]
    an_atom = [[7, 0], [7, 0]]
    an_bond = [[3, 3], [5, 1]]
    an_conn = [[[0, 0], [0, 1]], [[1, 1], [1, 0]]]
    return _inputs(cat_atom, cat_bond, cat_conn, an_atom, an_bond, an_conn)


def test_token_usage_counts_real_atoms_and_message_edges_only():
    u = data.token_usage(_hand_made(), VA, VB)
    assert u.atom.dtype == np.int64 and u.bond.dtype == np.int64 and u.atom.shape == (VA,) and u.bond.shape == (VB,)
    want_atom = np.zeros(VA, np.int64)
    want_atom[[3, 4, 5, 7]] = (2, 1, 1, 2)
    assert np.array_equal(u.atom, want_atom)                        # id 0, the padding atom, counts nowhere
    want_bond = np.zeros(VB, np.int64)
    want_bond[[0, 2, 5]] = (1, 2, 1)                                # source 0, target 0, id VB, id -1: no message
    assert np.array_equal(u.bond, want_bond)
    assert u._fields == ("atom", "bond")
    x = _hand_made()
    x["cat_atom"][0, 3] = VA                                        # an id outside the vocabulary reads a zero row
    assert np.array_equal(data.token_usage(x, VA, VB).atom, want_atom)
    with pytest.raises(ValueError):
        data.token_usage({**x, "cat_connectivity": x["cat_connectivity"][:, :3]}, VA, VB)


def test_unseen_tokens_names_the_new_ids_and_the_exact_fraction():
    base = _hand_made()
    same = data.unseen_tokens(base, base, VA, VB)
    assert same.atom.size == 0 and same.bond.size == 0 and same.samples == 0.0
    # four new samples: [0] nothing new; [1] atom 9 on the anion; [2] bond 4 on a valid cation edge; [3] bond 1 only on
    # an edge that carries no message and atom id 0 - nothing new
    new = _inputs(cat_atom=[[3, 4, 0, 0], [3, 0, 0, 0], [4, 3, 0, 0], [5, 0, 0, 0]],
                  cat_bond=[[2, 2, 0, 0], [2, 0, 0, 0], [4, 0, 0, 0], [1, 0, 0, 0]],
                  cat_conn=[[[1, 2], [2, 1], [0, 0], [0, 0]], [[0, 0]] * 4, [[1, 2], [0, 0], [0, 0], [0, 0]],
                            [[0, 1], [0, 0], [0, 0], [0, 0]]],
                  an_atom=[[7, 0], [9, 0], [7, 0], [7, 0]],
                  an_bond=[[0, 0]] * 4, an_conn=[[[0, 0], [0, 0]]] * 4)
    u = data.unseen_tokens(base, new, VA, VB)
    assert u.atom.tolist() == [9] and u.bond.tolist() == [4] and u.samples == 0.5
    assert u.atom.dtype == np.int64 and u._fields == ("atom", "bond", "samples")
    # bond id 0 on a valid edge is used by `new` alone here, and id 0 is never reported
    lone = {k: v[:1] for k, v in new.items()}
    lone["cat_bond"] = np.zeros_like(lone["cat_bond"])
    none = {k: np.zeros_like(v) for k, v in lone.items()}
    assert data.token_usage(lone, VA, VB).bond[0] == 2
    u0 = data.unseen_tokens(none, lone, VA, VB)
    assert u0.bond.tolist() == [] and u0.atom.tolist() == [3, 4, 7] and u0.samples == 1.0


# ------------------------------------------------------------------------------------------------- (2) the attribute
def test_trainable_rows_validation():
    e = L.Embedding(VA, 4, device=CPU)
    assert e.trainable_rows is None and e.get_config()["trainable_rows"] is None
    e.trainable_rows = [0, 3, VA - 1]
    assert e.trainable_rows == (0, 3, VA - 1) and e.get_config()["trainable_rows"] == [0, 3, VA - 1]
    e.trainable_rows = np.array([2, 5], np.int64)
    assert e.trainable_rows == (2, 5)
    for bad in ([VA], [-1], [1, 1], [3, 2], [], [1.0], ["1"], [True], 3, "12"):
        with pytest.raises(ValueError):
            e.trainable_rows = bad
        assert e.trainable_rows == (2, 5)                            # a refused value leaves the old one
    e.trainable_rows = None
    assert e.trainable_rows is None
    again = L.Embedding.from_config({**L.Embedding(VA, 4, trainable_rows=[1, 2], device=CPU).get_config()})
    assert again.trainable_rows == (1, 2)
    with pytest.raises(ValueError):
        L.Embedding(VA, 4, trainable_rows=[VA], device=CPU)


def model(kind="transfer", S=2):
    L.reset_uids()
    return MM.MPNNModel(kind, VA, VB, 8, 4, 6, 5, S, 1e-4, device=CPU, dropout_seed=1)


def head_only(m):
    for layer in m.layers:
        layer.trainable = layer.name.startswith("mp_") or layer.name == "melting_point"


def test_rows_round_trip_through_config_and_file(tmp_path):
    m = model()
    head_only(m)
    m.atom_emb.trainable_rows = [2, 9]
    cfg = m.get_config()
    assert cfg["embedding_trainable_rows"] == {m.atom_emb.name: [2, 9], m.bond_emb.name: None}
    again = MM.MPNNModel.from_config(cfg, device=CPU)
    assert again.atom_emb.trainable_rows == (2, 9) and again.bond_emb.trainable_rows is None
    assert again.atom_emb.trainable is False
    old = {k: v for k, v in cfg.items() if k != "embedding_trainable_rows"}   # a file written before this key
    older = MM.MPNNModel.from_config(old, device=CPU)
    assert older.atom_emb.trainable_rows is None and older.bond_emb.trainable_rows is None
    m.bond_emb.trainable_rows = [5]
    path = tmp_path / "transfer.keras"
    m.save(str(path))
    back = MM.load_model(str(path), device=CPU)
    assert back.atom_emb.trainable_rows == (2, 9) and back.bond_emb.trainable_rows == (5,)
    for n, a in m.state_dict().items():
        assert np.array_equal(back.state_dict()[n], a), n


# ------------------------------------------------------------------------------------------------- (3) compile()
HEAD = ["mp_dense_1/kernel", "mp_dense_1/bias", "mp_bn_1/gamma", "mp_bn_1/beta", "mp_dense_2/kernel", "mp_dense_2/bias",
        "mp_dense_3/kernel", "mp_dense_3/bias", "melting_point/kernel", "melting_point/bias"]


def test_compile_lists_a_frozen_embedding_with_rows_and_the_caches_refuse():
    m = model()
    head_only(m)
    m.compile(train.Adam(1e-3), loss="huber")
    assert [n for n, _ in m.trainable_variables()] == HEAD and m.frozen_prefix() == {"cat": None, "an": None}
    m._frozen_cache_check()                                          # stage 1 as it stands: cacheable
    epoch = m.frozen_prefix_epoch
    m.atom_emb.trainable_rows = [3]
    m.bond_emb.trainable_rows = [1, 4]
    assert m.frozen_prefix() == {"cat": None, "an": None}            # counts from the next compile
    opt = train.Adam(1e-3, weight_decay=1e-2)
    opt.exclude_from_weight_decay(["bias"])
    m.compile(opt, loss="huber")
    assert [n for n, _ in m.trainable_variables()] == ["atom_embedding", "bond_embedding"] + HEAD
    atom, bond = m.atom_emb.embeddings, m.bond_emb.embeddings
    assert atom.requires_grad and bond.requires_grad and atom.grad is not None
    assert autograd._listed_rows(atom).tolist() == [3] and autograd._listed_rows(bond).tolist() == [1, 4]
    assert autograd._listed_rows(atom).dtype == torch.int32
    assert m.frozen_prefix() == {"cat": 0, "an": 0} and m.frozen_prefix_epoch == epoch + 1
    # a row-restricted table never decays; the other variables follow exclude_from_weight_decay
    names = [n for n, _ in m.trainable_variables()]
    assert opt._decay_flags.tolist() == [0, 0] + [int("bias" not in n) for n in names[2:]]
    x = synthetic.make_batch(6, max_atoms=6, max_edges=8, atom_vocab_size=VA, bond_vocab_size=VB, min_atoms=2, seed=1)
    y = np.zeros(6, np.float32)
    with pytest.raises(ValueError) as err:
        m.fit(x, y, cache_frozen_encoder=True)
    assert "cache_frozen_encoder" in str(err.value) and "an encoder layer is trainable (stage 2)" in str(err.value)
    with pytest.raises(ValueError) as err:
        m.fit(x, y, cache_frozen_steps=True)
    assert "cache_frozen_steps" in str(err.value) and "nothing below the first trained step is frozen" in str(err.value)
    # weights_updated drops what was built from a table that trains (here: stand-ins for the typed images)
    m._prepared = {"f32t": object(), "f32": object()}
    m._split_deg_limit = 7
    m.weights_updated()
    assert set(m._prepared) == {"f32"} and m._split_deg_limit is None
    # the rows count only while the layer is frozen; clearing them brings stage 1 back
    m.atom_emb.trainable = True
    m.bond_emb.trainable_rows = None
    m.compile(train.Adam(1e-3), loss="huber")
    assert [n for n, _ in m.trainable_variables()] == ["atom_embedding"] + HEAD
    assert autograd._listed_rows(atom) is None and autograd._listed_rows(bond) is None
    assert not bond.requires_grad and bond.grad is None
    m.atom_emb.trainable = False
    m.atom_emb.trainable_rows = None
    m.compile(train.Adam(1e-3), loss="huber")
    assert [n for n, _ in m.trainable_variables()] == HEAD and m.frozen_prefix() == {"cat": None, "an": None}
    m._frozen_cache_check()


def test_train_unseen_tokens_sets_both_layers():
    m = model()
    head_only(m)
    base = synthetic.make_batch(12, max_atoms=6, max_edges=8, atom_vocab_size=VA - 3, bond_vocab_size=VB - 2,
                                min_atoms=2, seed=2)
    new = synthetic.make_batch(12, max_atoms=6, max_edges=8, atom_vocab_size=VA, bond_vocab_size=VB, min_atoms=2, seed=3)
    want = data.unseen_tokens(base, new, VA, VB)
    assert want.atom.size and want.bond.size and 0.0 < want.samples <= 1.0
    got = m.train_unseen_tokens(base, new)
    assert got.atom.tolist() == want.atom.tolist() and got.bond.tolist() == want.bond.tolist()
    assert got.samples == want.samples
    assert m.atom_emb.trainable_rows == tuple(want.atom.tolist())
    assert m.bond_emb.trainable_rows == tuple(want.bond.tolist())
    assert m.train_unseen_tokens(new, new).atom.size == 0            # nothing unseen: no rows, not an empty list
    assert m.atom_emb.trainable_rows is None and m.bond_emb.trainable_rows is None


# ------------------------------------------------------------------------------------------------- (4) the C entry
def test_the_prototype_parses_and_writes_through_a_const_table():
    e = F.entries()["impnn_embed_rows_bwd"]
    assert e["mutable"] == [] and e["const"] == ["ids", "dout", "row_list", "buffers"]
    assert [n for _, n in e["params"]] == ["ids", "dout", "row_list", "n_listed", "buffers", "rows", "vocab", "dim",
                                           "accumulate", "stream"]
    assert len(_lib.SIGNATURES["impnn_embed_rows_bwd"][1]) == len(e["params"])
    assert _lib.load().impnn_abi_version() == 3
    from ionic_mpnn_amd import build
    assert "embed_rows.hip" in build.SOURCES and (build.CSRC / "embed_rows.hip").exists()


def test_argument_refusals_come_in_the_documented_order():
    lib = _lib.load()
    P = C.c_void_p
    ok, odd = P(0x1000), P(0x1002)                                   # never dereferenced: every call ends before a launch
    table = lambda p: (C.c_void_p * 1)(p)

    def call(ids=ok, dout=ok, row_list=ok, n_listed=2, buffers=table(0x2000), rows=5, vocab=4, dim=3, accumulate=0):
        rc = lib.impnn_embed_rows_bwd(ids, dout, row_list, n_listed, buffers, rows, vocab, dim, accumulate, None)
        return rc, lib.impnn_last_error_string().decode()

    # 1. shape, ahead of everything (null pointers included)
    for kw in (dict(rows=-1), dict(vocab=0), dict(dim=-1), dict(n_listed=-1), dict(accumulate=2)):
        rc, text = call(ids=None, dout=None, row_list=None, buffers=None, **kw)
        assert rc == _BAD and "bad shape" in text, (kw, rc, text)
    rc, text = call(ids=None, rows=5, vocab=4)                        # the identity needs rows == vocab
    assert rc == _BAD and "rows must equal vocab" in text
    # 2. zero work, ahead of the null pointers
    for kw in (dict(n_listed=0), dict(rows=0), dict(dim=0)):
        assert call(dout=None, row_list=None, buffers=None, **kw)[0] == 0, kw
    assert call(ids=None, dout=None, row_list=None, buffers=None, rows=4, vocab=4, n_listed=0)[0] == 0
    # 3. null pointers, ahead of the alignment
    for kw in (dict(buffers=None), dict(buffers=table(None)), dict(dout=None), dict(row_list=None)):
        rc, text = call(ids=odd, **kw)
        assert rc == _BAD and "null pointer" in text, (kw, rc, text)
    # 4. alignment
    for kw in (dict(ids=odd), dict(dout=odd), dict(row_list=odd), dict(buffers=table(0x2002))):
        rc, text = call(**kw)
        assert rc == _BAD and "4-byte aligned" in text, (kw, rc, text)
    # the launch's own limit: n_listed * ceil(dim / 64) workgroups
    rc, text = call(n_listed=2 ** 31 - 1, dim=129)
    assert rc == _UNSUPPORTED and "workgroups" in text
