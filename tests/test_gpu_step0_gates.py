"""GPU: the typed encoder's step-0 gate table (impnn_encoder_prepare_weights_gates) and the pool's batched reads.

In step 0 the z and r accumulators after the bias and the W_h h half depend on (weights, atom id) only; an image of the
with-gates entry carries them as a table behind the step-0 message table, and the atom phase of step 0 loads a row of it
instead of multiplying.  Every case runs ops.encoder_fused with four images per ion -

    gates    message table + gate table            (what MPNNModel keeps)
    atoms    message table alone                   (impnn_encoder_prepare_weights_atoms: second header zeros)
    orphan   a with-gates image whose message-table header was cleared: the gate table must not be used without it
    plain    no table                              (the MFMA step 0 every other encoder test holds)

- and the pooled outputs must be the same BITS (compared as int32, so NaNs count).  The cases also state, from the image
itself, that the tables they mean to exercise are there (the two headers in the tail of step 0's update slot)."""
import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib
from ionic_mpnn_amd import model as MM
from ionic_mpnn_amd import ops, synthetic, weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ["f32t", "f32x3"]
HDR = {"f32t": 6400, "f32x3": 9472}  # float offset of the message-table header in the image; the gate header: + 4
M0_MAGIC, G0_MAGIC = 0x6d30746d, 0x67307467
KINDS = ("gates", "atoms", "orphan", "plain")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _weights(Va, Vb, S, seed):
    return weights.init_weights("viscosity", Va, Vb, atom_dim=32, bond_dim=8, num_steps=S, seed=seed, perturb=True)


def _batch(B, N, E, Va, Vb, seed, min_atoms=3):
    inp = synthetic.make_batch(B, max_atoms=N, max_edges=E, atom_vocab_size=Va, bond_vocab_size=Vb, min_atoms=min_atoms,
                               seed=seed)
    return {k: v for k, v in inp.items() if k != "temperature"}


def _headers(img, mode):
    h = img.view(torch.int32)[HDR[mode]:HDR[mode] + 8].cpu().numpy()
    return [int(v) for v in h]


def _image(kind, pk, atab, btab, S, mode, Va, Vb, expect_tables):
    if kind == "plain":
        return ops.prepare_encoder_weights(pk, btab, 32, 8, S, mode)
    img = ops.prepare_encoder_weights(pk, btab, 32, 8, S, mode, atom_table=atab, gates=kind != "atoms")
    h = _headers(img, mode)
    if not expect_tables:
        assert h == [0] * 8, f"{kind}: a table header where no table is built: {h}"
        return img
    assert h[:4] == [M0_MAGIC, Va, Vb, S], f"{kind}: message-table header {h[:4]}"
    if kind == "atoms":
        assert h[4:] == [0, 0, 0, 0], f"the with-atoms image has a second header: {h[4:]}"
    else:
        assert h[4:] == [G0_MAGIC, Va, Vb, S], f"{kind}: gate-table header {h[4:]}"
    if kind == "orphan":
        img.view(torch.int32)[HDR[mode]:HDR[mode] + 4] = 0
    return img


def _run(w, inp, Va, Vb, S, mode, workgroups=0, tables=(True, True), ions=("cat", "an"), expect_tables=True, walk=None):
    """-> pooled outputs of the `gates` images, after asserting that every kind of image gives the same bits.
    tables: which ion's image is of the kind under test (the others: plain) - both bits of the kernel's mask."""
    m = MM.build_model(Va, Vb, atom_dim=32, bond_dim=8, fp_size=32, mixing_size=20, num_steps=S, device=DEV)
    m.load_weights(w)
    atab, btab = m.atom_emb.embeddings, m.bond_emb.embeddings
    packed = m._packed_weights()
    sel = [("cat", "an").index(p) for p in ions]
    data = [tuple(_dev(inp[f"{p}_{k}"]) for k in ("atom", "bond", "connectivity")) for p in ions]
    lib = _lib.load()
    code = ops.ENCODER_MODES[mode]
    atoms_bytes = int(lib.impnn_encoder_prepared_bytes_atoms(32, S, Va, Vb, code))
    gates_bytes = int(lib.impnn_encoder_prepared_bytes_gates(32, S, Va, Vb, code))
    assert gates_bytes == atoms_bytes + ((Va + 1) * 256 if expect_tables and S > 0 else 0)
    out = {}
    for kind in KINDS:
        prep = [_image(kind if tables[i] else "plain", packed[g], atab, btab, S, mode, Va, Vb, expect_tables)
                for i, g in enumerate(sel)]
        out[kind] = ops.encoder_fused(data, atab, btab, None, S, mode=mode, prepared=prep, workgroups=workgroups)
        if walk is not None and kind == "gates":
            torch.cuda.synchronize()
            B, N = data[0][0].shape
            layout = ops.encoder_plan_layout(len(ions), B, N, data[0][1].shape[1], 32, 8, S, Vb, mode, workgroups)
            walk(layout, ops.read_plan(ops._workspace(DEV, 1), layout, len(ions), B))
    torch.cuda.synchronize()
    for kind in KINDS[:-1]:
        for i, p in enumerate(ions):
            assert np.array_equal(_bits(out[kind][i]), _bits(out["plain"][i])), f"{p}: {kind} and plain images differ"
    return out["gates"]


# ---- small batches: one molecule (a chunk of fewer than 16 rows), three, forty (row counts that are no multiple of 16,
#      slack rows in the last tile), for every number of steps
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("B", [1, 3, 40])
@pytest.mark.parametrize("mode", MODES)
def test_small_batches(mode, B, S):
    Va, Vb = 7, 3
    inp = _batch(B, 12, 24, Va, Vb, 40 + B)
    rows = [int((inp[f"{p}_atom"] > 0).sum()) for p in ("cat", "an")]
    if B == 1:
        assert max(rows) < 16, rows
    else:
        assert any(r % 16 for r in rows), rows
    _run(_weights(Va, Vb, S, 50 + S), inp, Va, Vb, S, mode)


@pytest.mark.parametrize("tables", [(True, False), (False, True)])
@pytest.mark.parametrize("mode", MODES)
def test_two_ions_one_image_with_the_tables(mode, tables):
    Va, Vb = 7, 3
    _run(_weights(Va, Vb, 3, 54), _batch(40, 12, 24, Va, Vb, 44), Va, Vb, 3, mode, tables=tables)


@pytest.mark.parametrize("ion", ["cat", "an"])
@pytest.mark.parametrize("mode", MODES)
def test_one_ion_alone(mode, ion):
    Va, Vb = 7, 3
    _run(_weights(Va, Vb, 2, 55), _batch(40, 12, 24, Va, Vb, 45), Va, Vb, 2, mode, tables=(True,), ions=(ion,))


@pytest.mark.parametrize("mode", MODES)
def test_atom_ids_zero_negative_and_beyond_the_vocabulary_take_the_zero_row(mode):
    Va, Vb = 5, 3
    inp = _batch(40, 12, 24, Va, Vb, 46, min_atoms=8)
    for p in ("cat", "an"):
        ids, conn = inp[f"{p}_atom"], inp[f"{p}_connectivity"]
        for b in (0, 17, 39):
            ids[b, 1:7] = [Va - 1, Va, Va + 7, -3, (1 << 24) + 5, 0]
            conn[b, :8] = [(1, 2), (2, 1), (3, 1), (4, 3), (5, 4), (6, 5), (1, 6), (2, 7)]
            inp[f"{p}_bond"][b, :8] = 1
        ids[1, 1:] = 0  # a molecule of one atom and padding rows
    _run(_weights(Va, Vb, 3, 56), inp, Va, Vb, 3, mode)


@pytest.mark.parametrize("what", ["inf_atom_entry", "nan_atom_row", "inf_in_gate_kernel_h_half", "nan_in_gate_kernel",
                                  "nan_gate_bias", "inf_gate_bias"])
@pytest.mark.parametrize("mode", MODES)
def test_non_finite_values_give_the_same_pattern(mode, what):
    """Row Va of the gate table is computed from a zero row, not copied from the bias: 0 * inf = NaN must appear in it as
    it does in the atom phase (slack rows, ids outside the vocabulary)."""
    Va, Vb = 5, 3
    w = _weights(Va, Vb, 3, 57)
    if what == "inf_atom_entry":
        w["atom_embedding"][2, 7] = np.inf
    elif what == "nan_atom_row":
        w["atom_embedding"][2, :] = np.nan
    elif what == "inf_in_gate_kernel_h_half":
        for p in ("cat", "an"):
            w[f"{p}_gu_0/dense_z/kernel"][3, 5] = np.inf    # rows 0..31 multiply h
            w[f"{p}_gu_0/dense_r/kernel"][9, 20] = -np.inf
    elif what == "nan_in_gate_kernel":
        for p in ("cat", "an"):
            w[f"{p}_gu_0/dense_r/kernel"][40, 2] = np.nan   # rows 32..63 multiply agg
            w[f"{p}_gu_0/dense_z/kernel"][1, 30] = np.nan
    elif what == "nan_gate_bias":
        for p in ("cat", "an"):
            w[f"{p}_gu_0/dense_r/bias"][4] = np.nan
    else:
        for p in ("cat", "an"):
            w[f"{p}_gu_0/dense_z/bias"][4] = np.inf
    inp = _batch(40, 12, 24, Va, Vb, 47)
    inp["cat_atom"][0, 1] = 2
    inp["an_atom"][3, 2] = Va + 2  # a zero row that is pooled
    got = _run(w, inp, Va, Vb, 3, mode)
    if what != "inf_gate_bias":  # (an infinite bias of z saturates the gate: sigmoid(inf) = 1, finite outputs)
        assert not all(np.isfinite(g.cpu().numpy()).all() for g in got)  # the case does reach the outputs


@pytest.mark.parametrize("mode", MODES)
def test_vocabulary_beyond_the_cap_has_no_tables(mode):
    Va, Vb = 300, 72  # 72 x 301 x 128 B > 2 MiB: no message table, hence no gate table
    _run(_weights(Va, Vb, 3, 58), _batch(8, 12, 24, Va, Vb, 48), Va, Vb, 3, mode, expect_tables=False)


@pytest.mark.parametrize("mode", MODES)
def test_atom_vocabulary_beyond_the_lds_copy(mode):
    Va, Vb = 1500, 3
    inp = _batch(40, 12, 24, Va, Vb, 49)
    inp["cat_atom"][0, :3] = [1499, 1, 750]
    _run(_weights(Va, Vb, 3, 59), inp, Va, Vb, 3, mode)


@pytest.mark.parametrize("mode", MODES)
def test_640_edge_chunks(mode):
    """Padded E > 512: mode f32x3 runs the instantiation with unpadded h rows."""
    Va, Vb = 20, 6
    _run(_weights(Va, Vb, 3, 60), _batch(8, 160, 640, Va, Vb, 50, min_atoms=120), Va, Vb, 3, mode)


@pytest.mark.parametrize("N", [41, 97, 160])
@pytest.mark.parametrize("mode", MODES)
def test_molecules_of_more_than_forty_rows(mode, N):
    """The pool reads a lane's rows five at a time: 8 lanes x 5 rows cover 40 rows per turn, so these molecules take 2,
    3 and 4 turns - with ids that are not positive among them (the pool takes rows of atom id > 0 only)."""
    Va, Vb = 20, 6
    inp = synthetic.make_explicit_h_batch(6, max_atoms=N, max_edges=4 * N, atom_vocab_size=Va, bond_vocab_size=Vb,
                                          min_atoms=N, seed=51 + N, with_temperature=False)
    for p in ("cat", "an"):
        assert int((inp[f"{p}_atom"] > 0).sum(axis=1).max()) == N
        inp[f"{p}_atom"][0, [3, 40, N - 1]] = -2   # rows that the pool leaves out
        inp[f"{p}_atom"][1, 5] = Va + 3             # a zero row that is pooled
    _run(_weights(Va, Vb, 3, 61), inp, Va, Vb, 3, mode)


@pytest.mark.parametrize("mode", MODES)
def test_a_workgroup_walks_three_chunks_or_more(mode):
    """2000 molecules of up to 40 atoms on the floor of 16 workgroups: each walks several chunks, so the gate path of
    step 0 runs right behind the previous chunk's pool and the transfers sent under it."""
    Va, Vb = synthetic.DEFAULT_VA, synthetic.DEFAULT_VB

    def walk(layout, plan):
        assert layout.nwg == 16, "sized for the floor of 16 workgroups"
        assert int(plan.nsub.max()) >= 3 and int(plan.nsub.min()) >= 2, [int(v) for v in plan.nsub]

    _run(_weights(Va, Vb, 3, 62), _batch(2000, 40, 80, Va, Vb, 52, min_atoms=30), Va, Vb, 3, mode, workgroups=16,
         walk=walk)


@pytest.mark.parametrize("mode", MODES)
def test_the_model_keeps_images_with_both_tables(mode):
    Va, Vb = 7, 3
    m = MM.build_model(Va, Vb, atom_dim=32, bond_dim=8, fp_size=32, mixing_size=20, num_steps=3, device=DEV)
    m.load_weights(_weights(Va, Vb, 3, 63))
    for img in m._prepared_weights(mode):
        assert _headers(img, mode) == [M0_MAGIC, Va, Vb, 3, G0_MAGIC, Va, Vb, 3]
