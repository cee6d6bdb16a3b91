"""GPU: the start of a table-fed chunk of the typed encoder (encoder_typed.hip: step 0 peeled out of the step loop).

A chunk whose ion's image carries both step-0 tables (messages M0, gate halves G0) fills no h buffer: the wave of a tile
takes its rows' h quads and Reduce's record words into registers in front of the prologue barrier, runs step 0's atom
phase outside the step loop without a mid-step barrier, and writes h for the first time at the end of that step.  Rows
of the h buffer that belong to no tile of the chunk keep the previous chunk's bytes.  So what these cases vary is what one
workgroup walks through - chunks in a row, a small chunk between two full ones, chunks without edges, a single chunk, no
chunk at all - and what a row's atom id can be.  As in test_gpu_step0_prefetch.py the library runs its floor of 16
persistent workgroups (eight per ion: the plan deals every workgroup a share of ONE ion, so no walk crosses from ion 0
to ion 1 - the walks of both ions are checked instead), every case asserts its premise from the chunk descriptors of the
plan its run walked (`walk=`), every run starts from a workspace of 0xff bytes, and the pooled outputs of the images
under test are compared as int32 - NaNs count - with those of plain images (the MFMA step 0 with fill_h0, which every
other encoder test holds).  A build with the second record buffer
(-DIMPNN_T_REC2=1: measured and dropped) keeps two record buffers where both images carry both tables and a
second record fits in place of the LDS copy of the atom table - (Va + 1) x 128 bytes against a record of at most 7.2 KB
at 72 bond types - so the cases that are about the walk use the benchmark's 124 atom types (VA) and hold such a build
too; the mixed-image, 256-type and 640-edge cases are the ones that fall back to one buffer there.  One case per mode is also held against oracle/torch_ref.pooled_pair in fp64 within 1e-5."""
import numpy as np
import pytest
import torch

import plan_cases as PC
from conftest import assert_close
from ionic_mpnn_amd import model as MM
from ionic_mpnn_amd import ops, synthetic, weights
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ["f32t", "f32x3"]
HDR = {"f32t": 6400, "f32x3": 9472}  # float offset of the message-table header in the image; the gate header: + 4
VA = synthetic.DEFAULT_VA  # 124: room for the second record buffer
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


def _sized(sizes_per_ion, N, E, Va, Vb, seed, edges_of):
    """Molecules of the given atom counts (plan_cases._fill: atoms in rows 0 .. n - 1, edges among rows >= 1)."""
    rng = np.random.default_rng(seed)
    inp = {}
    for p, sizes in zip(("cat", "an"), sizes_per_ion):
        ion = PC._ion(len(sizes), N, E)
        for b, n in enumerate(sizes):
            PC._fill(rng, ion, b, int(n), min(E, int(edges_of(int(n)))), Va, Vb)
        inp[f"{p}_atom"], inp[f"{p}_bond"], inp[f"{p}_connectivity"] = ion
    return inp


def _dirty_workspace():
    ws = ops._workspace(DEV, 64 << 20)
    ws.fill_(0xff)
    return ws


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
    assert all(len({c[4] for c in wk}) <= 1 for wk in walks), "a workgroup's walk crosses from one ion to the other"
    return walks


def _image(kind, pk, atab, btab, S, mode):
    """gates: both tables; atoms: M0 only; orphan: both tables, the message-table header cleared; plain: no table."""
    if kind == "plain":
        return ops.prepare_encoder_weights(pk, btab, 32, 8, S, mode)
    img = ops.prepare_encoder_weights(pk, btab, 32, 8, S, mode, atom_table=atab, gates=kind != "atoms")
    h = [int(v) for v in img.view(torch.int32)[HDR[mode]:HDR[mode] + 8].cpu().numpy()]
    assert h[0] != 0 and (h[4] != 0) == (kind != "atoms"), f"{kind}: headers {h}"
    if kind == "orphan":
        img.view(torch.int32)[HDR[mode]:HDR[mode] + 4] = 0
    return img


def _run(w, inp, Va, Vb, S, mode, kinds=("gates", "gates"), workgroups=2, walk=None):
    """-> pooled outputs (cation, anion) with images of `kinds`, after asserting that they are the bits of a run with plain
    images.  workgroups: what the call asks for; below 16 the library runs 16.  walk: the premise of the calling case,
    asserted on the chunks every workgroup of the run walked (_walks)."""
    m = MM.build_model(Va, Vb, atom_dim=32, bond_dim=8, fp_size=32, mixing_size=20, num_steps=S, device=DEV)
    m.load_weights(w)
    atab, btab = m.atom_emb.embeddings, m.bond_emb.embeddings
    packed = m._packed_weights()
    data = [tuple(_dev(inp[f"{p}_{k}"]) for k in ("atom", "bond", "connectivity")) for p in ("cat", "an")]
    out = []
    for use in (kinds, ("plain", "plain")):
        prep = [_image(use[g], packed[g], atab, btab, S, mode) for g in range(2)]
        ws = _dirty_workspace()
        out.append(ops.encoder_fused(data, atab, btab, None, S, mode=mode, prepared=prep, workgroups=workgroups))
        assert ops._workspace(DEV, 1).data_ptr() == ws.data_ptr(), "the encoder took another workspace than the dirtied one"
        if walk is not None and use is kinds:
            torch.cuda.synchronize()
            B, N = data[0][0].shape
            walk(_walks(ws, 2, B, N, data[0][1].shape[1], S, Vb, mode, workgroups))
    torch.cuda.synchronize()
    for g, p in enumerate(("cat", "an")):
        assert np.array_equal(_bits(out[0][g]), _bits(out[1][g])), f"{p}: images {kinds} and plain images differ"
    return out[0]


def _reference(name, w, inp):
    if name not in _REF:
        B = inp["cat_atom"].shape[0]
        parts = [R.pooled_pair(w, {k: v[i:i + 64] for k, v in inp.items()}, dtype=torch.float64) for i in range(0, B, 64)]
        _REF[name] = tuple(torch.cat([p[g] for p in parts]).numpy() for g in range(2))
    return _REF[name]


# ---- several chunks per workgroup: 320 molecules of 30 - 40 atoms per ion, about seven to a chunk, eight workgroups per
#      ion; every chunk but a workgroup's first starts right behind the previous chunk's pool
def walks_three_chunks_on_both_ions(walks):
    for g in (0, 1):
        n = [len(wk) for wk in walks if wk and wk[0][4] == g]
        assert n and max(n) >= 3, f"ion {g}: no workgroup walks three chunks: {n}"


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("mode", MODES)
def test_several_chunks_per_workgroup(mode, S):
    Va, Vb = synthetic.DEFAULT_VA, synthetic.DEFAULT_VB
    w, inp = _weights(Va, Vb, S, 71), _batch(320, 40, 80, Va, Vb, 61, min_atoms=30)
    got = _run(w, inp, Va, Vb, S, mode, walk=walks_three_chunks_on_both_ions)
    if S == 3:  # the fp64 oracle, once per mode
        ref = _reference("several", w, inp)
        for g in range(2):
            assert_close(got[g].cpu().numpy(), ref[g], what=f"several chunks, ion {g}")


# ---- stale rows: a chunk of 16 tiles, then one of at most 3 tiles whose row count is no multiple of 16, then 16 tiles
#      again - the h rows of tiles 3 .. 15 keep the first chunk's last state while the small chunk runs
def walks_full_small_full(walks):
    found = set()
    for wk in walks:
        for x, y, z in zip(wk, wk[1:], wk[2:]):
            if x[3] > 240 and y[3] <= 48 and y[3] % 16 and z[3] > 240:
                found.add(x[4])
    assert found == {0, 1}, f"ions with a 16-tile, <= 3-tile, 16-tile walk: {sorted(found)}; rows: {[[c[3] for c in wk] for wk in walks]}"


@pytest.mark.parametrize("mode", MODES)
def test_stale_rows_of_a_small_chunk_between_full_ones(mode):
    Va, Vb = VA, 5
    sizes = [250, 37, 250] * 8  # one triple per workgroup of the ion: equal shares of 537 virtual rows
    inp = _sized([sizes, sizes], 256, 512, Va, Vb, 62, edges_of=lambda n: n + n // 2)
    _run(_weights(Va, Vb, 3, 72), inp, Va, Vb, 3, mode, walk=walks_full_small_full)


# ---- edge-free chunks of single atoms between chunks with edges
def walks_edge_free_chunks_between_chunks_with_edges(walks):
    found = set()
    for wk in walks:
        e = [c[2] > 0 for c in wk]
        for i in range(1, len(wk) - 1):
            j = i
            while j < len(wk) and not e[j]:
                j += 1
            if e[i - 1] and j > i and j < len(wk):
                found.add(wk[0][4])
    assert found == {0, 1}, f"ions with such a walk: {sorted(found)}; valid edges per chunk: {[[c[2] for c in wk] for wk in walks]}"


@pytest.mark.parametrize("mode", MODES)
def test_edge_free_chunks_of_single_atoms_between_chunks_with_edges(mode):
    Va, Vb = VA, 5
    # a workgroup's share is about 1750 virtual rows (a molecule counts at least plan_vmin of them, one atom or not): 150
    # single atoms in a row inside a share are whole chunks without an edge, with chunks of 12-atom molecules before and
    # behind them in the same walk
    sizes = [[12] * 40 + [1] * 150 + [12] * 1060, [12] * 600 + [1] * 150 + [12] * 500]
    inp = _sized(sizes, 12, 24, Va, Vb, 63, edges_of=lambda n: 2 * (n - 1))
    _run(_weights(Va, Vb, 3, 73), inp, Va, Vb, 3, mode, walk=walks_edge_free_chunks_between_chunks_with_edges)


# ---- short walks: fewer molecules than workgroups - shares without a chunk, and workgroups with a single chunk
def walks_one_chunk_or_none(walks):
    n = [len(wk) for wk in walks]
    assert 0 in n and 1 in n and max(n) == 1, f"chunks per workgroup: {n}"


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("mode", MODES)
def test_short_walks(mode, S):
    Va, Vb = VA, 5
    inp = _sized([[5, 12, 8], [12, 3, 7]], 12, 24, Va, Vb, 64, edges_of=lambda n: 2 * (n - 1))
    _run(_weights(Va, Vb, S, 74), inp, Va, Vb, S, mode, walk=walks_one_chunk_or_none)


# ---- atom ids: 0 inside the kept rows, negative, Va, Va + 7 and 0x7fffffff all read the zero row (of G0, and of h)
@pytest.mark.parametrize("mode", MODES)
def test_atom_ids_outside_the_vocabulary(mode):
    Va, Vb = VA, 3
    inp = _batch(700, 12, 24, Va, Vb, 65, min_atoms=10)
    for p in ("cat", "an"):
        ids, conn = inp[f"{p}_atom"], inp[f"{p}_connectivity"]
        for b in (0, 350, 699):  # in a workgroup's first chunk, in a later one, in the ion's last
            ids[b, 1:8] = [Va - 1, 0, -3, Va, Va + 7, 0x7fffffff, 1]
            conn[b, :8] = [(1, 2), (2, 1), (3, 1), (4, 3), (5, 4), (6, 5), (1, 6), (2, 7)]
            inp[f"{p}_bond"][b, :8] = 1
    _run(_weights(Va, Vb, 3, 75), inp, Va, Vb, 3, mode, walk=walks_three_chunks_on_both_ions)


# ---- non-finite atom-table rows: 0 * inf = NaN in column Va of M0 and in row Va of G0 is reproduced, and a row of h that
#      holds an inf or a NaN reaches r h, the blend and the residual from the registers as it did from the h buffer
@pytest.mark.parametrize("mode", MODES)
def test_non_finite_atom_table_rows(mode):
    Va, Vb = VA, 3
    w = _weights(Va, Vb, 3, 76)
    w["atom_embedding"][7, 5] = np.inf
    w["atom_embedding"][8, :] = np.nan
    inp = _batch(700, 12, 24, Va, Vb, 66, min_atoms=10)
    for p in ("cat", "an"):  # the two rows only where they are placed, so that most molecules stay finite
        inp[f"{p}_atom"][inp[f"{p}_atom"] >= 7] = 1
    inp["cat_atom"][0, 1], inp["cat_atom"][400, 2] = 7, 8
    inp["an_atom"][3, 2], inp["an_atom"][697, 1] = 8, 7
    got = _run(w, inp, Va, Vb, 3, mode, walk=walks_three_chunks_on_both_ions)
    for g in got:  # the case does reach the outputs, and not all of them
        fin = np.isfinite(g.cpu().numpy()).all(axis=1)
        assert not fin.all() and fin.sum() >= 600, int(fin.sum())


# ---- mixed images: the peeled step 0 only where the ion's image carries BOTH tables, the old hand-over everywhere else
@pytest.mark.parametrize("kinds", [("gates", "plain"), ("plain", "gates"), ("atoms", "gates"), ("atoms", "atoms"),
                                   ("orphan", "gates"), ("orphan", "orphan")])
@pytest.mark.parametrize("mode", MODES)
def test_mixed_images(mode, kinds):
    Va, Vb = VA, 5
    _run(_weights(Va, Vb, 3, 77), _batch(320, 40, 80, Va, Vb, 67, min_atoms=30), Va, Vb, 3, mode, kinds=kinds,
         walk=walks_three_chunks_on_both_ions)


# ---- fall-back layouts: 256 bond types (the largest record), and 640-edge chunks (mode f32x3: unpadded h rows) - the LDS
#      budget is full there
@pytest.mark.parametrize("mode", MODES)
def test_256_bond_types(mode):
    Va, Vb = 20, 256
    _run(_weights(Va, Vb, 3, 78), _batch(320, 40, 80, Va, Vb, 68, min_atoms=30), Va, Vb, 3, mode,
         walk=walks_three_chunks_on_both_ions)


@pytest.mark.parametrize("mode", MODES)
def test_640_edge_chunks_256_bond_types(mode):
    Va, Vb = 20, 256
    sizes = [150, 40, 150] * 8
    inp = _sized([sizes, sizes], 160, 640, Va, Vb, 69, edges_of=lambda n: 4 * n)

    def walks_640_edge_chunks(walks):
        walks_three_chunks_on_both_ions(walks)
        assert max(c[2] for wk in walks for c in wk) > 512, "no chunk holds more than 512 valid edges"

    _run(_weights(Va, Vb, 3, 79), inp, Va, Vb, 3, mode, walk=walks_640_edge_chunks)


@pytest.mark.parametrize("mode", MODES)
def test_atom_vocabulary_beyond_the_lds_copy(mode):
    """No LDS copy of the atom table: the h quads come from the table in global memory, zeros for ids outside it."""
    Va, Vb = 1500, 3
    assert (Va + 1) * 32 * 4 > 160 * 1024, "the table alone must exceed a workgroup's LDS"
    inp = _batch(700, 12, 24, Va, Vb, 70, min_atoms=10)
    inp["cat_atom"][0, :5] = [1499, 1, 750, Va, -1]
    inp["an_atom"][699, :3] = [Va + 7, 1499, 0x7fffffff]
    _run(_weights(Va, Vb, 3, 80), inp, Va, Vb, 3, mode, walk=walks_three_chunks_on_both_ions)


# ---- S = 0 is unchanged: pooled = GlobalSumPool(Embedding(atom ids)), no step machinery
@pytest.mark.parametrize("mode", MODES)
def test_no_message_passing_steps(mode):
    Va, Vb = 9, 5
    inp = _batch(320, 40, 80, Va, Vb, 71, min_atoms=30)
    inp["cat_atom"][5, 3], inp["an_atom"][7, 2] = Va + 2, -4
    atab = np.random.default_rng(81).standard_normal((Va, 32)).astype(np.float32)
    btab = np.zeros((Vb, 8), np.float32)
    data = [tuple(_dev(inp[f"{p}_{k}"]) for k in ("atom", "bond", "connectivity")) for p in ("cat", "an")]
    _dirty_workspace()
    got = ops.encoder_fused(data, _dev(atab), _dev(btab), [None, None], 0, mode=mode, workgroups=2)
    torch.cuda.synchronize()
    for g, p in enumerate(("cat", "an")):
        ids = inp[f"{p}_atom"].astype(np.int64)
        rows = np.where(((ids > 0) & (ids < Va))[..., None], atab.astype(np.float64)[np.clip(ids, 0, Va - 1)], 0.0)
        assert_close(got[g].cpu().numpy(), rows.sum(axis=1), what=f"S = 0, {p}")
