"""GPU: the order of the typed encoder's atom phase (encoder_typed.hip) - what moves when Reduce takes a form chosen by the
tile's largest in-degree and, in mode f32x3, the h halves of the gate GEMMs are issued in front of Reduce.

Reduce reads one in-edge rank per round trip for a tile whose largest in-degree is 1, two for 2, and runs the loop of four
ranks per round otherwise; every form starts agg at +0 and adds the ranks in order, so the forms differ only in adds of the
slot of zeros that are left out.  The cases put every form, and the thresholds between them, into tiles of their own:

  * a chunk of 40 rows (three tiles of 16, 16 and 8 rows) whose tiles ALL have largest in-degree d, for d = 0, 1, 2, 3, 4, 5
    (one round of the loop, two rounds from 5 on) and 17 (five rounds); the other rows' in-degrees are spread below d;
  * one tile whose rows alternate between in-degree 0 and 4;
  * plan_cases.hubs(17): 24 molecules with in-degrees 15 .. 18, 40 and one of 17, several chunks per ion, tiles that
    straddle molecules.

Every case runs in modes f32t and f32x3, S = 1 and 3, with the step-0 table in the image and without it, against the
fp64 run of oracle/torch_ref.py within 1e-5 of the output scale (conftest.assert_close); f32x3 stays within twice f32t's
error (2 x + 1e-7, as tests/test_gpu_encoder.py states it); 16 against 48 workgroups and table against no table give
equal bits.  The premise of a case - one chunk of 40 rows, these tile maxima - is asserted from the plan the run walked
and from the in-degrees plan_cases counts.

Signed zeros: a row whose only in-edge message is -0.0 in every feature.  The oracle's agg = 0 + m is +0 (asserted on
its bits as integers); the encoder's agg is not an output, and no later operation of GatedUpdate tells -0 from +0 (the
GEMM accumulators start at a bias, sigmoid and tanh are followed by sums), so what a one-step model can show is that the
row's output bits equal those of the same batch with the edge slot turned into padding, where agg is +0 by construction.
Two constructions: the zero source row under a matrix of negative entries (products 0 * -w = -0), and a source row and
matrix so small that every product underflows to -0 - the one the MFMA accumulator really rounds to -0.

NaN / inf: the gates' products of h are issued in front of the messages' sum in mode f32x3; which rows come out
non-finite stays what tests/test_gpu_encoder.py::test_f32x3_propagates_nan_and_inf_like_f32t states."""
import numpy as np
import pytest
import torch

import plan_cases as PC
from conftest import assert_close
from ionic_mpnn_amd import model as MM
from ionic_mpnn_amd import ops, weights
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ["f32t", "f32x3"]
VA, VB = 24, 6
ROWS = 40
_OUT = {}  # (case, S, mode, table, workgroups) -> pooled pair
_REF = {}  # (case, S) -> fp64 pooled pair


def _weights(Va, Vb, S, seed=91):
    return weights.init_weights("viscosity", Va, Vb, atom_dim=32, bond_dim=8, num_steps=S, seed=seed, perturb=True)


def _molecule(rng, indeg, N, E, Va=VA, Vb=VB):
    """One molecule of len(indeg) atoms (ids > 0: every row is kept), atom v with indeg[v] in-edges from atoms >= 1 (index 0
    marks a padding slot, so row 0 lies on no edge), the valid edges spread over the E slots."""
    n = len(indeg)
    assert indeg[0] == 0 and n <= N
    atom = np.zeros(N, np.int32)
    atom[:n] = rng.integers(1, Va, size=n)
    tgt = rng.permutation(np.repeat(np.arange(n), indeg))
    assert len(tgt) <= E
    conn, bond = np.zeros((E, 2), np.int32), np.zeros(E, np.int32)
    slots = np.sort(rng.choice(E, size=len(tgt), replace=False))
    conn[slots, 1] = tgt
    conn[slots, 0] = rng.integers(1, n, size=len(tgt))
    bond[slots] = rng.integers(0, Vb, size=len(tgt))
    return atom, bond, conn


def _one_molecule_case(name, indeg_per_ion, seed):
    rng = np.random.default_rng(seed)
    ions = []
    for indeg in indeg_per_ion:
        a, b, c = _molecule(rng, indeg, len(indeg) + 3, 160)
        ions.append((a[None], b[None], c[None]))
    n = len(indeg_per_ion[0])
    return PC._case(name, ions, n + 3, 160, Va=VA, Vb=VB)


def tiles_of_degree(d):
    """40 rows per ion; each of the three tiles has one row (not row 0) of in-degree d, the others at most min(d, 3)."""
    rng = np.random.default_rng(200 + d)
    per_ion = []
    for _ in PC.IONS:
        indeg = rng.integers(0, min(d, 3) + 1, size=ROWS)
        for first, rows in ((0, 16), (16, 16), (32, 8)):
            indeg[first + 1 + rng.integers(0, rows - 1)] = d
        indeg[0] = 0
        per_ion.append(indeg)
    return _one_molecule_case(f"deg{d}", per_ion, 300 + d)


def mixed_0_and_4():
    indeg = np.array([0, 4] * 8)
    return _one_molecule_case("mixed04", [indeg, indeg], 310)


CASES = {f"deg{d}": (lambda d=d: tiles_of_degree(d)) for d in (0, 1, 2, 3, 4, 5, 17)}
CASES["mixed04"] = mixed_0_and_4
CASES["hubs17"] = lambda: PC.hubs(17)
TILE_MAXIMA = {**{f"deg{d}": [d, d, d] for d in (0, 1, 2, 3, 4, 5, 17)}, "mixed04": [4]}
_CASE = {}


def _case(name):
    if name not in _CASE:
        _CASE[name] = CASES[name]()
    return _CASE[name]


def _tile_maxima(case, p):
    deg = PC.in_degrees(case, p)[0]
    rows = int(PC.kept_rows(case.inp[f"{p}_atom"])[0])
    return [int(deg[t:min(t + 16, rows)].max()) for t in range(0, rows, 16)]


def _premise(name, case, layout, plan):
    chunks = sorted((int(plan.ion[j, c]), int(plan.desc[j, c, 0]), int(plan.desc[j, c, 1]))
                    for j in range(layout.nwg) for c in range(int(plan.nsub[j])))
    if name == "hubs17":
        for g, p in enumerate(PC.IONS):
            assert sum(1 for ch in chunks if ch[0] == g) >= 2, chunks
            deg = PC.in_degrees(case, p)
            assert (deg == 17).any() and deg.max() == 40
        return
    assert chunks == [(0, 0, 1), (1, 0, 1)], f"not one chunk per ion: {chunks}"
    want = TILE_MAXIMA[name]
    rows = 16 * (len(want) - 1) + (8 if len(want) == 3 else 16)
    assert [int(plan.rows[g, 0]) for g in range(2)] == [rows, rows], plan.rows
    for p in PC.IONS:
        assert _tile_maxima(case, p) == want, (name, p, _tile_maxima(case, p))


def _encode(w, inp, Va, Vb, S, mode, table, workgroups, premise=None):
    m = MM.build_model(Va, Vb, atom_dim=32, bond_dim=8, fp_size=32, mixing_size=20, num_steps=S, device=DEV)
    m.load_weights(w)
    atab, btab = m.atom_emb.embeddings, m.bond_emb.embeddings
    packed = m._packed_weights()
    data = [tuple(torch.from_numpy(np.ascontiguousarray(inp[f"{p}_{k}"])).to(DEV) for k in ("atom", "bond", "connectivity"))
            for p in PC.IONS]
    prep = [ops.prepare_encoder_weights(packed[g], btab, 32, 8, S, mode, atom_table=atab if table else None)
            for g in range(2)]
    out = ops.encoder_fused(data, atab, btab, None, S, mode=mode, prepared=prep, workgroups=workgroups)
    torch.cuda.synchronize()
    if premise is not None:
        B, N = inp["cat_atom"].shape
        layout = ops.encoder_plan_layout(2, B, N, inp["cat_bond"].shape[1], 32, 8, S, Vb, mode, workgroups)
        assert layout.nwg == workgroups
        premise(layout, ops.read_plan(ops._workspace(DEV, 1), layout, 2, B))
    return [o.cpu().numpy() for o in out]


def _run(name, S, mode, table, workgroups):
    key = (name, S, mode, table, workgroups)
    if key not in _OUT:
        case = _case(name)
        premise = (lambda layout, plan: _premise(name, case, layout, plan)) if workgroups == 16 else None
        _OUT[key] = _encode(_weights(case.Va, case.Vb, S), case.inp, case.Va, case.Vb, S, mode, table, workgroups, premise)
    return _OUT[key]


def _reference(name, S):
    if (name, S) not in _REF:
        case = _case(name)
        _REF[(name, S)] = tuple(t.numpy() for t in R.pooled_pair(_weights(case.Va, case.Vb, S), case.inp, dtype=torch.float64))
    return _REF[(name, S)]


def _errors(got, ref):
    """max / rms / elementwise error against the oracle, relative to the tensor's scale (as tests/test_gpu_encoder.py)."""
    g, r = np.concatenate(got).astype(np.float64), np.concatenate(ref)
    d, scale = np.abs(g - r), max(float(np.abs(r).max()), 1e-30)
    return (float(d.max() / scale), float(np.sqrt(np.mean(d * d)) / max(np.sqrt(np.mean(r * r)), 1e-30)),
            float(np.max(d / np.maximum(np.abs(r), 1e-3 * scale))))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("table", [True, False], ids=["table", "plain"])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_in_degree_forms_against_fp64(name, S, table):
    ref = _reference(name, S)
    err = {}
    for mode in MODES:
        got = _run(name, S, mode, table, 16)
        err[mode] = _errors(got, ref)
        print(f"{name} S={S} table={table} {mode}: max / rms / elementwise error {err[mode]}")
        for g in range(2):
            assert_close(got[g], ref[g], what=f"{name}, {mode}, ion {g}")
    for i in range(3):
        assert err["f32x3"][i] <= 2.0 * err["f32t"][i] + 1e-7, err


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_workgroups_and_table_leave_the_bits(name, mode, S):
    base = _run(name, S, mode, True, 16)
    for what, other in (("48 workgroups", _run(name, S, mode, True, 48)), ("no table", _run(name, S, mode, False, 16))):
        for g in range(2):
            assert np.array_equal(_bits(base[g]), _bits(other[g])), f"{name}, {mode}, S={S}, ion {g}: {what} changes the bits"


# ---- signed zeros: molecule of 4 atoms, the only valid edge 1 -> 2, bond type 0 whose matrix is bond_transform[0]
ZERO_ID = VA - 1


def _signed_zero_setup(kind):
    w = _weights(VA, VB, 1, seed=92)
    for p in PC.IONS:
        w["bond_embedding"][0, :] = 0.0
        w["bond_embedding"][0, 0] = 1.0
        bt = w[f"{p}_bmm_0/bond_transform"]
        if kind == "zero_row":  # 0 * -|w| = -0 in every product
            bt[0] = -np.abs(bt[0]) - 1e-3
            w["atom_embedding"][ZERO_ID, :] = 0.0
        else:                   # 1e-30 * -1e-30 underflows: the accumulator rounds the product to -0
            bt[0] = np.float32(-1e-30)
            w["atom_embedding"][ZERO_ID, :] = np.float32(1e-30)
    inp = {}
    for p in PC.IONS:
        atom = np.array([[3, ZERO_ID, 5, 7, 0]], np.int32)
        conn = np.zeros((1, 8, 2), np.int32)
        bond = np.zeros((1, 8), np.int32)
        conn[0, 3] = (1, 2)
        inp[f"{p}_atom"], inp[f"{p}_bond"], inp[f"{p}_connectivity"] = atom, bond, conn
    return w, inp


@pytest.mark.parametrize("table", [True, False], ids=["table", "plain"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["zero_row", "underflow"])
def test_a_lone_message_of_minus_zero_sums_to_plus_zero(kind, mode, table):
    w, inp = _signed_zero_setup(kind)
    for p in PC.IONS:  # the oracle, in float32: the message is (+-)0 in every feature and agg = 0 + m is +0, bit for bit
        h = torch.nn.functional.embedding(torch.as_tensor(inp[f"{p}_atom"]).long(), torch.as_tensor(w["atom_embedding"]))
        be = torch.nn.functional.embedding(torch.as_tensor(inp[f"{p}_bond"]).long(), torch.as_tensor(w["bond_embedding"]))
        conn = torch.as_tensor(inp[f"{p}_connectivity"])
        m = R.bond_matrix_message(h, be, conn, torch.as_tensor(w[f"{p}_bmm_0/bond_transform"]))
        assert (m[0, 3] == 0).all(), m[0, 3]
        agg = R.reduce_messages(m, conn[:, :, 1], h.shape[1])
        assert not _bits(agg[0, 2].numpy()).any(), _bits(agg[0, 2].numpy())
    with_edge = _encode(w, inp, VA, VB, 1, mode, table, 16)
    bare = {k: v.copy() for k, v in inp.items()}
    for p in PC.IONS:
        bare[f"{p}_connectivity"][0, 3] = 0
    without = _encode(w, bare, VA, VB, 1, mode, table, 16)
    for g in range(2):
        assert np.isfinite(with_edge[g]).all()
        assert np.array_equal(_bits(with_edge[g]), _bits(without[g])), (kind, mode, g, with_edge[g], without[g])


# ---- NaN / inf rows: 48 molecules of 6 atoms; id VA - 1 (a NaN in its row) in molecules 5 and 20, id VA - 2 (an inf)
#      in molecules 9, 20 and 33, each as an atom that has an out-edge and an in-edge
NAN_IN, INF_IN = (5, 20), (9, 20, 33)


def _poison_batch():
    rng = np.random.default_rng(95)
    inp = {}
    for p in PC.IONS:
        mols = []
        for b in range(48):
            indeg = rng.integers(0, 4, size=6)
            indeg[0] = 0
            mols.append(_molecule(rng, indeg, 6, 20, Va=VA - 2))
        a, b_, c = (np.stack([m[i] for m in mols]) for i in range(3))
        for ids, bad in ((NAN_IN, VA - 1), (INF_IN, VA - 2)):
            for i in ids:
                row = 1 if bad == VA - 1 else 2
                a[i, row] = bad
                c[i, 18] = (row, 3)
                c[i, 19] = (4, row)
        inp[f"{p}_atom"], inp[f"{p}_bond"], inp[f"{p}_connectivity"] = a, b_, c
    return inp


@pytest.mark.parametrize("table", [True, False], ids=["table", "plain"])
def test_nan_and_inf_rows_stay_what_they_were(table):
    inp = _poison_batch()
    clean = _weights(VA, VB, 3, seed=93)
    bad = {k: v.copy() for k, v in clean.items()}
    bad["atom_embedding"][VA - 1, 3] = np.nan
    bad["atom_embedding"][VA - 2, 7] = np.inf
    res, ok = {}, {}
    for mode in MODES:
        res[mode] = np.concatenate(_encode(bad, inp, VA, VB, 3, mode, table, 16))
        ok[mode] = np.concatenate(_encode(clean, inp, VA, VB, 3, mode, table, 16))
        assert np.isfinite(ok[mode]).all()
    fin_t, fin_x = np.isfinite(res["f32t"]).all(axis=1), np.isfinite(res["f32x3"]).all(axis=1)
    poisoned = np.zeros(48, bool)
    poisoned[list(NAN_IN + INF_IN)] = True
    poisoned = np.concatenate([poisoned, poisoned])
    with_nan = np.zeros(48, bool)
    with_nan[list(NAN_IN)] = True
    with_nan = np.concatenate([with_nan, with_nan])
    assert not fin_t[with_nan].any() and not fin_x[with_nan].any()   # a NaN row: NaN in both modes
    assert not (fin_x & ~fin_t).any()                                # never finite where exact f32 is not
    assert fin_t[~poisoned].all() and fin_x[~poisoned].all()         # and the poison stays in its molecules
    only_nan = with_nan & ~np.concatenate([np.isin(np.arange(48), INF_IN)] * 2)   # (molecule 5 of each ion)
    assert only_nan.sum() == 2 and np.array_equal(np.isnan(res["f32t"][only_nan]), np.isnan(res["f32x3"][only_nan]))
    both = fin_t & fin_x
    assert_close(res["f32x3"][both], res["f32t"][both].astype(np.float64), what="rows finite in both modes")
    for mode in MODES:
        assert np.array_equal(_bits(res[mode][~poisoned]), _bits(ok[mode][~poisoned])), mode
