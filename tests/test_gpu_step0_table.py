"""GPU: the typed encoder's step-0 message table (impnn_encoder_prepare_weights_atoms).

Every case runs ops.encoder_fused twice - with an image that carries the table and with one built without it (the
arithmetic the other encoder tests hold) - and the pooled outputs must be the same BITS (compared as int32, so NaNs
count).  Finite cases are also held against oracle/torch_ref.pooled_pair in fp64 within the project's 1e-5."""
import numpy as np
import pytest
import torch

from conftest import assert_close
from ionic_mpnn_amd import _lib
from ionic_mpnn_amd import model as MM
from ionic_mpnn_amd import ops, synthetic, weights
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ["f32t", "f32x3"]
_REF = {}  # case name -> fp64 pooled pair, computed once and shared by the modes


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _model(w, Va, Vb, K, S):
    m = MM.build_model(Va, Vb, atom_dim=32, bond_dim=K, fp_size=32, mixing_size=20, num_steps=S, device=DEV)
    m.load_weights(w)
    return m


def _reference(name, w, inp, table_rows=None):
    """fp64 pooled pair, in slices of 64 molecules (the per-edge matrices of a slice stay small).  table_rows: zero rows
    appended to the atom table up to that many rows - what the library reads for an id outside [0, Va)."""
    if name not in _REF:
        w = dict(w)
        if table_rows is not None:
            t = np.zeros((table_rows, w["atom_embedding"].shape[1]), w["atom_embedding"].dtype)
            t[:w["atom_embedding"].shape[0]] = w["atom_embedding"]
            w["atom_embedding"] = t
        B = inp["cat_atom"].shape[0]
        parts = [R.pooled_pair(w, {k: v[i:i + 64] for k, v in inp.items() if k != "temperature"}, dtype=torch.float64)
                 for i in range(0, B, 64)]
        _REF[name] = tuple(torch.cat([p[g] for p in parts]).numpy() for g in range(2))
    return _REF[name]


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _run(w, inp, Va, Vb, K, S, mode, workgroups=0, expect_table=True, image_rows=None):
    """-> (pooled with the table image, pooled with the plain image), after asserting they are the same bits.
    image_rows: build the table image from the first image_rows rows of the atom table only (a mismatched Va)."""
    m = _model(w, Va, Vb, K, S)
    atab, btab = m.atom_emb.embeddings, m.bond_emb.embeddings
    ions = [tuple(_dev(inp[f"{p}_{k}"]) for k in ("atom", "bond", "connectivity")) for p in ("cat", "an")]
    img_atab = atab if image_rows is None else atab[:image_rows].contiguous()
    lib = _lib.load()
    old = int(lib.impnn_encoder_prepared_bytes(32, S, Vb, ops.ENCODER_MODES[mode]))
    new = int(lib.impnn_encoder_prepared_bytes_atoms(32, S, img_atab.shape[0], Vb, ops.ENCODER_MODES[mode]))
    if expect_table:
        assert new == old + Vb * (img_atab.shape[0] + 1) * 128
    else:
        assert new == old
    out = []
    for table in (img_atab, None):
        prep = [ops.prepare_encoder_weights(pk, btab, 32, K, S, mode, atom_table=table) for pk in m._packed_weights()]
        out.append(ops.encoder_fused(ions, atab, btab, None, S, mode=mode, prepared=prep, workgroups=workgroups))
    torch.cuda.synchronize()
    for g in range(2):
        assert np.array_equal(_bits(out[0][g]), _bits(out[1][g])), f"ion {g}: table and MFMA step 0 differ"
    return out[0]


def _check(name, w, inp, Va, Vb, K, S, mode, table_rows=None, **kw):
    got = _run(w, inp, Va, Vb, K, S, mode, **kw)
    ref = _reference(name, w, inp, table_rows)
    for g in range(2):
        assert_close(got[g].cpu().numpy(), ref[g], what=f"{name} ion {g}")


def _weights(Va, Vb, K, S, seed):
    return weights.init_weights("viscosity", Va, Vb, atom_dim=32, bond_dim=K, num_steps=S, seed=seed, perturb=True)


def _batch(B, N, E, Va, Vb, seed, min_atoms=3):
    inp = synthetic.make_batch(B, max_atoms=N, max_edges=E, atom_vocab_size=Va, bond_vocab_size=Vb, min_atoms=min_atoms,
                               seed=seed)
    return {k: v for k, v in inp.items() if k != "temperature"}


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("mode", MODES)
def test_base_case(mode, S):
    Va, Vb = 5, 3
    _check(f"base{S}", _weights(Va, Vb, 8, S, 11), _batch(8, 12, 24, Va, Vb, 1), Va, Vb, 8, S, mode)


def _group_fill_batch(Vb, types):
    """Molecule 0 of both ions: bond type types[j] on j + 1 edges (1, 2, 3, 4, 5 edges per type), one type of the
    vocabulary on no edge; the other molecules random."""
    inp = _batch(8, 12, 24, 9, min(Vb, 7), 2)
    rng = np.random.default_rng(5)
    for p in ("cat", "an"):
        inp[f"{p}_atom"][0] = np.arange(12) % 8 + 1
        conn = np.zeros((24, 2), np.int32)
        bond = np.zeros(24, np.int32)
        e = 0
        for j, t in enumerate(types):
            for _ in range(j + 1):
                conn[e] = (rng.integers(1, 12), rng.integers(1, 12))
                bond[e] = t
                e += 1
        inp[f"{p}_connectivity"][0], inp[f"{p}_bond"][0] = conn, bond
    return inp


@pytest.mark.parametrize("mode", MODES)
def test_group_fill_one_to_five_edges_per_type_and_a_type_without_edges(mode):
    Va, Vb = 9, 7  # types 1-5 carry 1-5 edges in molecule 0; type 0 is on no valid edge of the batch
    _check("fill", _weights(Va, Vb, 8, 3, 12), _group_fill_batch(Vb, [1, 2, 3, 4, 5]), Va, Vb, 8, 3, mode)


@pytest.mark.parametrize("mode", MODES)
def test_one_bond_type(mode):
    Va, Vb = 9, 1
    inp = _batch(8, 12, 24, Va, 2, 3)
    for p in ("cat", "an"):
        inp[f"{p}_bond"][:] = 0  # the only id of the vocabulary
    _check("vb1", _weights(Va, Vb, 8, 3, 13), inp, Va, Vb, 8, 3, mode)


@pytest.mark.parametrize("mode", MODES)
def test_256_bond_types(mode):
    Va, Vb = 9, 256
    inp = _batch(8, 12, 24, Va, Vb, 4)
    inp["cat_bond"][0, :6] = [255, 255, 254, 0, 128, 255]
    _check("vb256", _weights(Va, Vb, 8, 3, 14), inp, Va, Vb, 8, 3, mode)


@pytest.mark.parametrize("mode", MODES)
def test_source_ids_at_the_ends_of_the_vocabulary_beyond_it_and_padding_rows(mode):
    Va, Vb = 5, 3
    inp = _batch(8, 12, 24, Va, Vb, 5, min_atoms=8)
    for p in ("cat", "an"):
        ids = inp[f"{p}_atom"]
        ids[0, 1], ids[0, 2], ids[0, 3] = Va - 1, Va, Va + 7   # the last row of the table, two ids beyond it
        ids[1, 1], ids[1, 2] = 0, -3                           # a hole (row 0 of the table) and a negative id
        ids[2, 1:] = 0                                         # edges out of padding rows only
        conn = inp[f"{p}_connectivity"]
        conn[0, :6] = [(1, 2), (2, 1), (3, 1), (2, 3), (3, 4), (1, 4)]
        conn[1, :4] = [(1, 2), (2, 1), (1, 3), (2, 3)]
        inp[f"{p}_bond"][0, :6] = 1
        inp[f"{p}_bond"][1, :4] = 2
    # the oracle's embedding has no row for an id outside the table: the library reads zeros there, and so does a
    # table padded with zero rows (a negative id stays outside any table: the oracle sees it as the padded row Va)
    ref_inp = {k: (np.where(v < 0, Va, v) if k.endswith("_atom") else v) for k, v in inp.items()}
    got = _run(_weights(Va, Vb, 8, 3, 15), inp, Va, Vb, 8, 3, mode)
    ref = _reference("ids", _weights(Va, Vb, 8, 3, 15), ref_inp, table_rows=Va + 8)
    for g in range(2):
        # a negative id is not pooled (atom id > 0 is), the padded row Va of the oracle would be: leave molecule 1 to
        # the bitwise comparison
        keep = np.arange(8) != 1
        assert_close(got[g].cpu().numpy()[keep], ref[g][keep], what=f"ids ion {g}")


@pytest.mark.parametrize("mode", MODES)
def test_molecules_without_edges_and_a_chunk_without_any_edge(mode):
    Va, Vb = 5, 3
    inp = _batch(8, 12, 24, Va, Vb, 6)
    # the anion: single atoms, no bond at all - every chunk of that ion is a chunk without any edge
    inp["an_atom"][:, 1:] = 0
    inp["an_atom"][:, 0] = np.arange(8) % (Va - 1) + 1
    inp["an_connectivity"][:] = 0
    inp["an_bond"][:] = 0
    inp["cat_connectivity"][3] = 0  # and one such molecule among the cations
    inp["cat_bond"][3] = 0
    _check("noedge", _weights(Va, Vb, 8, 3, 16), inp, Va, Vb, 8, 3, mode)


@pytest.mark.parametrize("mode", MODES)
def test_several_chunks_per_workgroup(mode):
    """B = 600 at the benchmark's padded shape on 16 workgroups: every workgroup runs several chunks, so the message
    buffer and the record are rebuilt between them."""
    Va, Vb = synthetic.DEFAULT_VA, synthetic.DEFAULT_VB
    _check("chunks", _weights(Va, Vb, 8, 3, 17), _batch(600, 40, 80, Va, Vb, 7), Va, Vb, 8, 3, mode, workgroups=16)


@pytest.mark.parametrize("mode", MODES)
def test_640_edge_instantiation(mode):
    Va, Vb = 20, 6
    inp = _batch(8, 160, 640, Va, Vb, 8, min_atoms=120)
    _check("e640", _weights(Va, Vb, 8, 3, 18), inp, Va, Vb, 8, 3, mode)


@pytest.mark.parametrize("mode", MODES)
def test_atom_table_beyond_lds_with_a_table(mode):
    Va, Vb = 1500, 3
    inp = _batch(8, 12, 24, Va, Vb, 9)
    inp["cat_atom"][0, :3] = [1499, 1, 750]
    _check("va1500", _weights(Va, Vb, 8, 3, 19), inp, Va, Vb, 8, 3, mode)


@pytest.mark.parametrize("mode", MODES)
def test_beyond_the_cap_no_table_is_built(mode):
    Va, Vb = 300, 72  # 72 x 301 x 128 B > 2 MiB: the size query must equal the old one
    _check("cap", _weights(Va, Vb, 8, 3, 20), _batch(8, 12, 24, Va, Vb, 10), Va, Vb, 8, 3, mode, expect_table=False)


@pytest.mark.parametrize("what", ["inf_in_bond_transform", "nan_atom_row"])
@pytest.mark.parametrize("mode", MODES)
def test_non_finite_values_give_the_same_bits(mode, what):
    Va, Vb = 5, 3
    w = _weights(Va, Vb, 8, 3, 21)
    if what == "inf_in_bond_transform":  # 0 * inf = NaN in the zero row's column as well
        for p in ("cat", "an"):
            w[f"{p}_bmm_0/bond_transform"][1, 3, 5] = np.inf
    else:
        w["atom_embedding"][2, :] = np.nan
    inp = _batch(8, 12, 24, Va, Vb, 11)
    inp["cat_atom"][0, 1] = 2
    got = _run(w, inp, Va, Vb, 8, 3, mode)
    assert not np.isfinite(got[0].cpu().numpy()).all()  # the case does reach the outputs


@pytest.mark.parametrize("mode", MODES)
def test_an_image_for_another_atom_vocabulary_is_not_used(mode):
    """An image prepared for Va = 5, launched with a table of 6 rows: the kernel must take the MFMA path."""
    Va, Vb = 6, 3
    inp = _batch(8, 12, 24, Va, Vb, 12)
    inp["cat_atom"][0, 1] = 5
    _check("vamis", _weights(Va, Vb, 8, 3, 22), inp, Va, Vb, 8, 3, mode, image_rows=5)


@pytest.mark.parametrize("mode", MODES)
def test_model_rebuilds_the_table_after_the_atom_embedding_changes(mode):
    Va, Vb = 5, 3
    w = _weights(Va, Vb, 8, 3, 23)
    inp = _batch(8, 12, 24, Va, Vb, 13)
    m = _model(w, Va, Vb, 8, 3)
    m.encoder_mode = mode
    dinp = {k: _dev(v) for k, v in inp.items()}
    got = m.encode_pooled(dinp, fused=True)
    ref = _reference("model0", w, inp)
    for g in range(2):
        assert_close(got[g].cpu().numpy(), ref[g], what=f"before, ion {g}")
    with torch.no_grad():
        m.atom_emb.embeddings.mul_(1.5).add_(0.25)
    m.invalidate_packed_weights()
    w2 = dict(w)
    w2["atom_embedding"] = m.atom_emb.embeddings.detach().cpu().numpy()
    got = m.encode_pooled(dinp, fused=True)
    ref = _reference("model1", w2, inp)
    for g in range(2):
        assert_close(got[g].cpu().numpy(), ref[g], what=f"after, ion {g}")
