"""GPU: step 0's inputs by LDS-DMA from the plan's slot-ordered source list (encoder_typed.hip: fetch_step0).

The step-0 messages of a chunk, and step 0's update image, are sent into LDS while the PREVIOUS chunk of the workgroup is
pooled, so what these cases vary is what one workgroup walks through: several chunks in a row, chunks with and without
edges next to each other, edge counts around the 8-slot granule of a transfer, an ion with the table beside one without.
The library never runs fewer than 16 persistent workgroups (a request below 16 is a request for 16: encoder_workgroups),
eight per ion here, so the batches are sized for EIGHT workgroups per ion to walk the sequences the case names - and each
case asserts that premise (`walk=`) from the chunk descriptors of the plan its run walked, read back out of the workspace
through the layout query (ops.encoder_plan_layout / ops.read_plan).  Every run compares the pooled outputs of images that carry the table with those of
plain images (the MFMA step 0, which every other encoder test holds) as int32, so NaNs count; every run starts from a
workspace filled with 0xff bytes, so a list word or a record byte the plan did not write cannot go unnoticed.  One case
per mode is also held against oracle/torch_ref.pooled_pair in fp64 within the project's 1e-5."""
import numpy as np
import pytest
import torch

from conftest import assert_close
from ionic_mpnn_amd import model as MM
from ionic_mpnn_amd import ops, synthetic, weights
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ["f32t", "f32x3"]
_REF = {}  # case name -> fp64 pooled pair, computed once and shared by the modes


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


def _dirty_workspace():
    """Fills the workspace encoder_fused takes on this stream with 0xff bytes; -> that buffer (see _same_workspace)."""
    ws = ops._workspace(DEV, 64 << 20)
    ws.fill_(0xff)
    return ws


def _same_workspace(ws):
    """The encoder did run on the dirtied buffer: had it asked for more than that holds, ops would have replaced its cached
    workspace by a fresh one and the fill would have tested nothing."""
    assert ops._workspace(DEV, 1).data_ptr() == ws.data_ptr(), "the encoder took another workspace than the dirtied one"


def _walks(ws, n_ions, B, N, E, S, Vb, mode, workgroups):
    """The plan the last run on workspace `ws` walked -> per workgroup, its chunks in walking order as
    (first molecule, molecules, valid edges, virtual rows, ion)."""
    layout = ops.encoder_plan_layout(n_ions, B, N, E, 32, 8, S, Vb, mode, workgroups)
    assert layout.nwg == 16, "these cases are sized for the floor of 16 workgroups"
    plan = ops.read_plan(ws, layout, n_ions, B)
    assert (plan.nsub >= 0).all() and (plan.nsub <= layout.max_sub).all()
    walks = [[tuple(int(v) for v in plan.desc[j, c]) + (int(plan.ion[j, c]),) for c in range(int(plan.nsub[j]))]
             for j in range(layout.nwg)]
    assert sorted(m for wk in walks for (m0, M, _, _, g) in wk for m in range(g * B + m0, g * B + m0 + M)) == \
        list(range(n_ions * B)), "the chunks read back do not tile the batch"
    return walks


def walks_chunks(k):
    def premise(walks):
        assert max(len(wk) for wk in walks) >= k, f"no workgroup walks {k} chunks: {[len(wk) for wk in walks]}"
        assert min(len(wk) for wk in walks) >= 2, f"a workgroup walks a single chunk: {[len(wk) for wk in walks]}"
    return premise


def walks_edge_free_chunks_between_chunks_with_edges(walks):
    """On each ion some workgroup walks: a chunk with edges, at least two whole chunks without any, a chunk with edges."""
    found = set()
    for wk in walks:
        z = [c[2] > 0 for c in wk]
        for a in range(1, len(wk) - 2):
            b = a
            while b < len(wk) and not z[b]:
                b += 1
            if z[a - 1] and b - a >= 2 and b < len(wk):
                found.add(wk[0][4])
    assert found == {0, 1}, f"ions with such a walk: {sorted(found)}; valid edges per chunk: {[[c[2] for c in wk] for wk in walks]}"


def walks_one_molecule_chunks(k):
    def premise(walks):
        assert all(c[1] == 1 for wk in walks for c in wk), "a chunk holds more than one molecule"
        best = max(len({c[2] for c in wk}) for wk in walks)
        assert best >= k, f"no workgroup walks {k} different edge counts: {[[c[2] for c in wk] for wk in walks]}"
    return premise


def _run(w, inp, Va, Vb, S, mode, workgroups=2, tables=(True, True), ions=("cat", "an"), walk=None):
    """-> pooled outputs (one per ion of `ions`) with images that carry the table where `tables` says so, after asserting
    that they are the bits of a run with plain images.  workgroups: what the call asks for; below 16 the library runs 16.
    walk: the premise of the calling case, asserted on the chunks every workgroup of the run walked (_walks)."""
    m = MM.build_model(Va, Vb, atom_dim=32, bond_dim=8, fp_size=32, mixing_size=20, num_steps=S, device=DEV)
    m.load_weights(w)
    atab, btab = m.atom_emb.embeddings, m.bond_emb.embeddings
    packed = m._packed_weights()
    sel = [("cat", "an").index(p) for p in ions]
    data = [tuple(_dev(inp[f"{p}_{k}"]) for k in ("atom", "bond", "connectivity")) for p in ions]
    out = []
    for use in (tables, (False,) * len(tables)):
        prep = [ops.prepare_encoder_weights(packed[g], btab, 32, 8, S, mode, atom_table=atab if use[i] else None)
                for i, g in enumerate(sel)]
        ws = _dirty_workspace()
        out.append(ops.encoder_fused(data, atab, btab, None, S, mode=mode, prepared=prep, workgroups=workgroups))
        _same_workspace(ws)
        if walk is not None and use is tables:
            torch.cuda.synchronize()
            B, N = data[0][0].shape
            walk(_walks(ws, len(ions), B, N, data[0][1].shape[1], S, Vb, mode, workgroups))
    torch.cuda.synchronize()
    for i, p in enumerate(ions):
        assert np.array_equal(_bits(out[0][i]), _bits(out[1][i])), f"{p}: table and MFMA step 0 differ"
    return out[0]


def _reference(name, w, inp):
    if name not in _REF:
        B = inp["cat_atom"].shape[0]
        parts = [R.pooled_pair(w, {k: v[i:i + 64] for k, v in inp.items()}, dtype=torch.float64) for i in range(0, B, 64)]
        _REF[name] = tuple(torch.cat([p[g] for p in parts]).numpy() for g in range(2))
    return _REF[name]


# ---- few workgroups: workgroups=2 is the floor of 16, eight per ion; each walks about ten chunks of ~25 molecules
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("mode", MODES)
def test_two_workgroups_walk_many_chunks(mode, S):
    Va, Vb = 9, 5
    w, inp = _weights(Va, Vb, S, 31), _batch(1700, 12, 24, Va, Vb, 21, min_atoms=8)
    got = _run(w, inp, Va, Vb, S, mode, walk=walks_chunks(8))
    if S == 3:  # the fp64 oracle, once per mode
        ref = _reference("many", w, inp)
        for g in range(2):
            assert_close(got[g].cpu().numpy(), ref[g], what=f"many chunks, ion {g}")


# ---- mixed table bits: one ion's image with the table, the other's without.  The kernel takes the table bit of the chunk it
#      fetches for (the next one), not of the chunk it is pooling.  These cases cannot tell the two apart: the plan deals
#      every workgroup a share of ONE ion, so consecutive chunks of a workgroup always have the same bit - the property
#      holds by construction of the plan.  What they do show is that each ion follows its own image's header.
@pytest.mark.parametrize("tables", [(True, False), (False, True)])
@pytest.mark.parametrize("mode", MODES)
def test_one_ion_with_the_table_one_without(mode, tables):
    Va, Vb = 9, 5
    # (workgroups=3 is the floor of 16 as well: eight per ion, three or four chunks each)
    _run(_weights(Va, Vb, 3, 32), _batch(600, 12, 24, Va, Vb, 22, min_atoms=8), Va, Vb, 3, mode, workgroups=3,
         tables=tables, walk=walks_chunks(3))


@pytest.mark.parametrize("mode", MODES)
def test_a_single_ion(mode):
    Va, Vb = 9, 5
    # (workgroups=1 is the floor of 16: all sixteen on the one ion, three or four chunks each)
    _run(_weights(Va, Vb, 3, 33), _batch(1200, 12, 24, Va, Vb, 23, min_atoms=8), Va, Vb, 3, mode, workgroups=1,
         tables=(True,), ions=("an",), walk=walks_chunks(3))


# ---- chunks without any edge before and behind chunks with edges, in one workgroup's walk
@pytest.mark.parametrize("mode", MODES)
def test_chunks_without_edges_between_chunks_with_edges(mode):
    Va, Vb = 9, 5
    inp = _batch(1200, 12, 24, Va, Vb, 24, min_atoms=10)
    # ~23 molecules fill a chunk and a workgroup walks ~150 molecules: 80 molecules without edges inside one workgroup's
    # share are three whole chunks of its walk, with chunks that have edges before and behind them
    for p, (lo, hi) in (("cat", (180, 260)), ("an", (630, 710))):
        inp[f"{p}_connectivity"][lo:hi] = 0
        inp[f"{p}_bond"][lo:hi] = 0
    _run(_weights(Va, Vb, 3, 34), inp, Va, Vb, 3, mode, walk=walks_edge_free_chunks_between_chunks_with_edges)


# ---- edge counts around the 8-slot granule: one molecule per chunk (130 atoms: no two fit 256 rows), its first
#      edges // 4 atoms with in-degree 4 (then one with the remainder), the others with in-degree 0 - their aggregates
#      are read from the slot of zeros, which lies right behind the message slots (and the dump slot) a transfer fills
def _granule_batch(N, E, Va, Vb, counts, natoms, seed):
    rng = np.random.default_rng(seed)
    B = len(counts)
    inp = {}
    for p in ("cat", "an"):
        atom = np.zeros((B, N), np.int32)
        atom[:, :natoms] = rng.integers(1, Va, size=(B, natoms))
        conn = np.zeros((B, E, 2), np.int32)
        bond = np.zeros((B, E), np.int32)
        for b, n_e in enumerate(counts if p == "cat" else counts[::-1]):
            e = np.arange(n_e)
            conn[b, :n_e, 1] = 1 + (e // 4) % (natoms - 1)      # target: in-degree 4 from atom 1 on
            conn[b, :n_e, 0] = 1 + (7 * e + 3) % (natoms - 1)   # source: any atom but index 0
            bond[b, :n_e] = rng.integers(0, Vb, size=n_e)
        inp[f"{p}_atom"], inp[f"{p}_connectivity"], inp[f"{p}_bond"] = atom, conn, bond
    return inp


@pytest.mark.parametrize("mode", MODES)
def test_edge_counts_around_the_granule_and_a_full_chunk(mode):
    Va, Vb = 9, 5
    # edges % 8 = 0, 1, 7 (short and long lists), no edge at all, and ecap = 512 exactly; the list eight times over, so
    # that each of the eight workgroups of an ion walks about ten one-molecule chunks with these counts in a row
    inp = _granule_batch(140, 512, Va, Vb, [256, 257, 263, 512, 8, 1, 7, 0, 505, 512] * 8, 130, 25)
    _run(_weights(Va, Vb, 3, 35), inp, Va, Vb, 3, mode, walk=walks_one_molecule_chunks(6))


@pytest.mark.parametrize("mode", MODES)
def test_640_edge_chunks_256_bond_types(mode):
    Va, Vb = 20, 256
    inp = _granule_batch(160, 640, Va, Vb, [640, 633, 1, 512, 639, 640, 320, 15] * 8, 160, 26)
    _run(_weights(Va, Vb, 3, 36), inp, Va, Vb, 3, mode, walk=walks_one_molecule_chunks(5))


@pytest.mark.parametrize("mode", MODES)
def test_atom_vocabulary_beyond_the_lds_copy(mode):
    Va, Vb = 1500, 3
    inp = _batch(120, 12, 24, Va, Vb, 27)
    inp["cat_atom"][0, :3] = [1499, 1, 750]
    _run(_weights(Va, Vb, 3, 37), inp, Va, Vb, 3, mode)


# ---- source ids at the ends of the vocabulary and outside it (read as a zero row), also beyond the list's 24 bits
@pytest.mark.parametrize("mode", MODES)
def test_source_ids_out_of_range(mode):
    Va, Vb = 5, 3
    inp = _batch(120, 12, 24, Va, Vb, 28, min_atoms=8)
    for p in ("cat", "an"):
        ids, conn = inp[f"{p}_atom"], inp[f"{p}_connectivity"]
        for b in (0, 40, 119):  # in the first chunk of the ion, one in the middle and the last
            ids[b, 1:7] = [Va - 1, Va, Va + 7, -3, (1 << 24) + 5, (1 << 24) - 1]
            conn[b, :8] = [(1, 2), (2, 1), (3, 1), (4, 3), (5, 4), (6, 5), (1, 6), (2, 7)]
            inp[f"{p}_bond"][b, :8] = 1
        ids[1, 1:] = 0  # edges out of padding rows only
    _run(_weights(Va, Vb, 3, 38), inp, Va, Vb, 3, mode)


@pytest.mark.parametrize("what", ["inf_in_bond_transform", "nan_atom_row"])
@pytest.mark.parametrize("mode", MODES)
def test_non_finite_table_entries_give_the_same_bits(mode, what):
    Va, Vb = 5, 3
    w = _weights(Va, Vb, 3, 39)
    if what == "inf_in_bond_transform":  # 0 * inf = NaN in the zero row's column as well
        for p in ("cat", "an"):
            w[f"{p}_bmm_0/bond_transform"][1, 3, 5] = np.inf
    else:
        w["atom_embedding"][2, :] = np.nan
    inp = _batch(120, 12, 24, Va, Vb, 29)
    inp["cat_atom"][0, 1] = 2
    got = _run(w, inp, Va, Vb, 3, mode)
    assert not np.isfinite(got[0].cpu().numpy()).all()  # the case does reach the outputs
