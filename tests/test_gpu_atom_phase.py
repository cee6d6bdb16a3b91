"""GPU: the atom phase of the typed encoder (encoder_typed.hip) at the smallest shapes at which it can go wrong.

The atom phase gives each wave one tile of 16 atoms; lane l holds atom l & 15 and feature quad l >> 4, and LayerNorm adds
four numbers across lanes l, l ^ 16, l ^ 32, l ^ 48 with two lane swaps on the vector ALU (encoder_device.h:
sum_xor16_xor32).  A swap that mixed atoms or feature quads, a tile boundary handled wrongly, or a wave without a tile
that took the wrong path would all show here:

  * one tile of 16 atoms with 16 different atom ids and in-degrees 0..4;
  * an ion whose only chunk has 17 rows (two tiles, the second with one row), 1 row, 70 rows (five tiles: eleven waves
    take the path without a tile), 255 and 256 rows (sixteen tiles: every wave has one);
  * zero variance: every GatedUpdate kernel and bias zero and the atom embedding constant across features, so that
    LayerNorm's argument is exactly zero in step 0 and the rsqrt sees ln_eps alone;
  * isolation: a NaN and an Inf in one embedding row that exactly one molecule of a multi-molecule tile uses.

Every case runs in modes f32t and f32x3, with S = 1 and S = 3 steps, with and without the step-0 table in the image, on
16 workgroups, against the fp64 run of oracle/torch_ref.py within the project's 1e-5 of the output scale (conftest.
assert_close), and f32x3 has to stay within twice f32t's error (the condition under which mode f32x3 was admitted, in the
form tests/test_gpu_encoder.py states it: 2 x + 1e-7, one f32 ulp of the scale).  The premise of each shape - one chunk of
so many rows, a chunk of one tile with several molecules - is asserted from the plan the run walked."""
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
VA, VB = synthetic.DEFAULT_VA, synthetic.DEFAULT_VB
WORKGROUPS = 16
_REF = {}  # (case, S) -> fp64 pooled pair, computed once


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _weights(S, seed=71):
    return weights.init_weights("viscosity", VA, VB, atom_dim=32, bond_dim=8, num_steps=S, seed=seed, perturb=True)


def _molecule(rng, n, indeg, N, E, ids=None):
    """One molecule: atoms at indices 0 .. n-1 (ids > 0, so all n rows are kept), atom v >= 1 with indeg[v] in-edges from
    atoms 1 .. n-1 (an edge that touches index 0 is not valid in the reference: models/layers.py:114), the valid edges
    spread over the E slots in random order."""
    atom = np.zeros(N, np.int32)
    atom[:n] = rng.integers(1, VA - 1, size=n) if ids is None else ids  # (id VA - 1 is kept for the poisoned row)
    tgt = np.repeat(np.arange(n), indeg)
    assert len(tgt) <= E and (n < 2 or indeg[0] == 0)
    conn = np.zeros((E, 2), np.int32)
    bond = np.zeros(E, np.int32)
    slots = np.sort(rng.choice(E, size=len(tgt), replace=False))
    conn[slots, 1] = tgt
    conn[slots, 0] = rng.integers(1, max(n, 2), size=len(tgt))
    bond[slots] = rng.integers(0, VB, size=len(tgt))
    return atom, bond, conn


def _single(n, seed, kind="random"):
    """A batch of ONE molecule per ion with n kept rows: its only chunk has n rows."""
    rng = np.random.default_rng(seed)
    inp = {}
    for p in ("cat", "an"):
        ids = None
        if kind == "tile16":  # 16 different ids, in-degrees 0, 1, 2, 3, 4, 0, 1, ...
            indeg = np.arange(n) % 5
            indeg[0] = 0
            ids = rng.permutation(np.arange(1, VA - 1))[:n]
        else:
            indeg = rng.integers(0, 5 if n <= 70 else 4, size=n)
            indeg[0] = 0
            if n > 2:
                indeg[n // 2] = 9  # three rounds of the Reduce loop for that tile
        E = 512 if n > 70 else 4 * n + 16  # the same for both ions; some slots stay padding
        a, b, c = _molecule(rng, n, indeg, n + 3 if n < 256 else n, E, ids)
        inp[f"{p}_atom"], inp[f"{p}_bond"], inp[f"{p}_connectivity"] = a[None], b[None], c[None]
    return inp


SHAPES = {
    "tile16": lambda: _single(16, 1, "tile16"),
    "rows17": lambda: _single(17, 2),
    "rows1": lambda: _single(1, 3),
    "rows70": lambda: _single(70, 4),
    "rows255": lambda: _single(255, 5),
    "rows256": lambda: _single(256, 6),
}
ROWS = {"tile16": 16, "rows17": 17, "rows1": 1, "rows70": 70, "rows255": 255, "rows256": 256}


def _plan(ws, inp, S, mode):
    B, N = inp["cat_atom"].shape
    layout = ops.encoder_plan_layout(2, B, N, inp["cat_bond"].shape[1], 32, 8, S, VB, mode, WORKGROUPS)
    assert layout.nwg == WORKGROUPS
    return layout, ops.read_plan(ws, layout, 2, B)


def _chunks(layout, plan):
    """-> [(ion, first molecule, molecules)] of every chunk of the plan."""
    return [(int(plan.ion[j, c]), int(plan.desc[j, c, 0]), int(plan.desc[j, c, 1]))
            for j in range(layout.nwg) for c in range(int(plan.nsub[j]))]


def one_chunk_of(rows):
    def premise(layout, plan):
        ch = _chunks(layout, plan)
        assert sorted(ch) == [(0, 0, 1), (1, 0, 1)], f"not one chunk per ion: {ch}"
        assert [int(plan.rows[g, 0]) for g in range(2)] == [rows, rows], plan.rows
    return premise


def _run(w, inp, S, mode, table, premise=None):
    """-> the two pooled outputs as numpy arrays."""
    m = MM.build_model(VA, VB, atom_dim=32, bond_dim=8, fp_size=32, mixing_size=20, num_steps=S, device=DEV)
    m.load_weights(w)
    atab, btab = m.atom_emb.embeddings, m.bond_emb.embeddings
    packed = m._packed_weights()
    data = [tuple(_dev(inp[f"{p}_{k}"]) for k in ("atom", "bond", "connectivity")) for p in ("cat", "an")]
    prep = [ops.prepare_encoder_weights(packed[g], btab, 32, 8, S, mode, atom_table=atab if table else None)
            for g in range(2)]
    ws = ops._workspace(DEV, 64 << 20)
    ws.fill_(0xff)
    out = ops.encoder_fused(data, atab, btab, None, S, mode=mode, prepared=prep, workgroups=WORKGROUPS)
    torch.cuda.synchronize()
    assert ops._workspace(DEV, 1).data_ptr() == ws.data_ptr(), "the encoder took another workspace than the dirtied one"
    if premise is not None:
        premise(*_plan(ws, inp, S, mode))
    return [o.cpu().numpy() for o in out]


def _reference(key, w, inp):
    if key not in _REF:
        _REF[key] = tuple(t.numpy() for t in R.pooled_pair(w, inp, dtype=torch.float64))
    return _REF[key]


def _errors(got, ref):
    """max / rms / elementwise error against the oracle, relative to the tensor's scale (as tests/test_gpu_encoder.py)."""
    g, r = np.concatenate(got).astype(np.float64), np.concatenate(ref)
    d, scale = np.abs(g - r), max(float(np.abs(r).max()), 1e-30)
    return (float(d.max() / scale), float(np.sqrt(np.mean(d * d)) / max(np.sqrt(np.mean(r * r)), 1e-30)),
            float(np.max(d / np.maximum(np.abs(r), 1e-3 * scale))))


def _check_both_modes(key, w, inp, S, table, premise):
    ref = _reference(key, w, inp)
    err = {}
    for mode in MODES:
        got = _run(w, inp, S, mode, table, premise)
        err[mode] = _errors(got, ref)
        print(f"{key} table={table} {mode}: max / rms / elementwise error {err[mode]}")
        for g in range(2):
            assert_close(got[g], ref[g], what=f"{key}, {mode}, ion {g}")
    for i in range(3):
        assert err["f32x3"][i] <= 2.0 * err["f32t"][i] + 1e-7, err


@pytest.mark.parametrize("table", [True, False], ids=["table", "plain"])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tile_shapes_against_fp64(shape, S, table):
    _check_both_modes((shape, S), _weights(S), SHAPES[shape](), S, table, one_chunk_of(ROWS[shape]))


@pytest.mark.parametrize("table", [True, False], ids=["table", "plain"])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("shape", ["tile16", "rows17"])
def test_zero_variance_rests_on_ln_eps(shape, S, table):
    w = _weights(S, seed=72)
    for k in w:
        if "/dense_" in k:
            w[k][...] = 0.0
    rng = np.random.default_rng(9)
    w["atom_embedding"][...] = rng.uniform(-0.05, 0.05, size=(VA, 1)).astype(np.float32)  # constant across features
    _check_both_modes(("zero_variance_" + shape, S), w, SHAPES[shape](), S, table, one_chunk_of(ROWS[shape]))


# ---- isolation: 32 molecules of 3 atoms per ion, four or so to a workgroup: every chunk is ONE tile that several molecules
#      share.  Atom id VA - 1 occurs once per ion, in molecule 5 (atom 1, which has an edge to atom 2 and one from it).
POISONED = 5


def _isolation_batch():
    rng = np.random.default_rng(7)
    B, inp = 32, {}
    for p in ("cat", "an"):
        mols = [_molecule(rng, 3, np.array([0, 1, 1]), 4, 4) for _ in range(B)]
        a, b, c = (np.stack([m[i] for m in mols]) for i in range(3))
        a[POISONED, 1] = VA - 1
        c[POISONED, :2] = [(1, 2), (2, 1)]
        c[POISONED, 2:] = 0
        inp[f"{p}_atom"], inp[f"{p}_bond"], inp[f"{p}_connectivity"] = a, b, c
    return inp


def poisoned_molecule_shares_a_tile(layout, plan):
    for g in range(2):
        mine = [(m0, M) for (ion, m0, M) in _chunks(layout, plan) if ion == g and m0 <= POISONED < m0 + M]
        assert len(mine) == 1, mine
        m0, M = mine[0]
        rows = int(plan.rows[g, m0:m0 + M].sum())
        assert M >= 2 and rows <= 16, f"ion {g}: the poisoned molecule's chunk has {M} molecules, {rows} rows"


@pytest.mark.parametrize("table", [True, False], ids=["table", "plain"])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("mode", MODES)
def test_a_poisoned_atom_stays_in_its_molecule(mode, S, table):
    inp = _isolation_batch()
    clean = _weights(S, seed=73)
    bad = {k: v.copy() for k, v in clean.items()}
    bad["atom_embedding"][VA - 1, 3] = np.nan
    bad["atom_embedding"][VA - 1, 7] = np.inf
    want = _run(clean, inp, S, mode, table, poisoned_molecule_shares_a_tile)
    got = _run(bad, inp, S, mode, table, poisoned_molecule_shares_a_tile)
    others = np.arange(want[0].shape[0]) != POISONED
    for g in range(2):
        assert np.isfinite(want[g]).all()
        assert np.array_equal(_bits(got[g][others]), _bits(want[g][others])), f"ion {g}: the poison left its molecule"
        assert not np.isfinite(got[g][POISONED]).any(), f"ion {g}: {got[g][POISONED]}"
