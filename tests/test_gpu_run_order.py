"""GPU: the run and group tables of the typed chunk records (csrc/encoder_plan.hip, plan_chunks_typed) read back and held
against the host reference (tests/run_order_ref.py), on batches composed for the run order: many types, few types cut into
pieces with remainders, one type, a chunk without edges between chunks with edges, ties, the last lane's types, the
640-edge record.

Every composition is planned with ops.EncoderPipeline.plan (16 workgroups: one launch) into a workspace of 0xff bytes; then
  * for every chunk of the plan (nsub, desc) the run table, nrun and every group's type and edge count are the host
    reference's, in both typed modes (their workspaces differ in front of the records), and hold its properties;
  * the pooled outputs agree with the fp64 oracle within the project's 1e-5 (conftest.assert_close) in f32t and f32x3;
  * a relabelling of the bond types - ids permuted, bond-table rows with them - moves runs around in the table and gives
    the same pooled bits, with and without the step-0 tables."""
import ctypes as C

import numpy as np
import pytest
import torch

import plan_cases as PC
import run_order_ref as RO
from conftest import assert_close
from ionic_mpnn_amd import _lib
from ionic_mpnn_amd import model as MM
from ionic_mpnn_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = tuple(RO.COMPOSITIONS)
TYPED = ("f32t", "f32x3")
_PLANS, _MODELS, _PREPARED = {}, {}, {}


def _model(Va, Vb):
    if (Va, Vb) not in _MODELS:
        m = MM.build_model(Va, Vb, atom_dim=32, bond_dim=PC.K, fp_size=32, mixing_size=20, num_steps=PC.S, device=DEV)
        m.load_weights(PC.case_weights(Va, Vb))
        _MODELS[(Va, Vb)] = (m.atom_emb.embeddings, m.bond_emb.embeddings, m._packed_weights())
    return _MODELS[(Va, Vb)]


def _bond_table(case, perm):
    _, btab, _ = _model(case.Va, case.Vb)
    if perm is None:
        return btab
    out = torch.empty_like(btab)
    out[torch.from_numpy(perm.astype(np.int64)).to(DEV)] = btab   # new_table[perm[v]] = table[v]
    return out


def _prepared(case, mode, table, perm):
    key = (case.name, mode, table)
    if key not in _PREPARED:
        atab, _, packed = _model(case.Va, case.Vb)
        _PREPARED[key] = [ops.prepare_encoder_weights(packed[g], _bond_table(case, perm), 32, PC.K, PC.S, mode,
                                                      atom_table=atab if table else None) for g in range(2)]
    return _PREPARED[key]


def _planned(case, mode):
    """-> (pipeline, plan handle, layout, plan read back, records layout, workspace), planned once per (case, mode)."""
    key = (case.name, mode)
    if key not in _PLANS:
        B = case.inp["cat_atom"].shape[0]
        args = (2, B, case.N, case.E, 32, PC.K, PC.S, case.Vb, mode, case.workgroups)
        layout, records = ops.encoder_plan_layout(*args), ops.encoder_plan_records(*args)
        need = C.c_size_t(0)
        ops.check(_lib.load().impnn_encoder_workspace_bytes(2, B, case.N, case.E, 32, PC.K, PC.S, case.Vb,
                                                            ops.ENCODER_MODES[mode], case.workgroups, C.byref(need)))
        assert records.rec_off + layout.nwg * layout.max_sub * records.rec_stride <= need.value
        pipe = ops.EncoderPipeline(DEV, depth=1)
        dirty = torch.full((max(need.value, 1 << 20),), 0xff, dtype=torch.uint8, device=DEV)
        pipe.slots[0]["ws"] = dirty
        data = [tuple(torch.from_numpy(np.ascontiguousarray(case.inp[f"{p}_{k}"])).to(DEV)
                      for k in ("atom", "bond", "connectivity")) for p in PC.IONS]
        h = pipe.plan(data, 32, PC.K, PC.S, case.Va, case.Vb, mode=mode, workgroups=case.workgroups)
        assert h.slot["ws"].data_ptr() == dirty.data_ptr(), "the plan took another workspace than the dirtied one"
        h.ready.synchronize()
        _PLANS[key] = (pipe, h, layout, ops.read_plan(dirty, layout, 2, B), records, dirty)
    return _PLANS[key]


def _run(case, mode, table=True, perm=None):
    pipe, h = _planned(case, mode)[:2]
    atab, _, _ = _model(case.Va, case.Vb)
    out = pipe.run(h, atab, _bond_table(case, perm), _prepared(case, mode, table, perm))
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


# ---- the tables
@pytest.mark.parametrize("mode", TYPED)
@pytest.mark.parametrize("name", NAMES)
def test_run_and_group_tables_are_the_host_reference(name, mode):
    case = RO.COMPOSITIONS[name]()
    _, _, layout, plan, records, ws = _planned(case, mode)
    PC.check_plan(case, layout, plan)
    assert layout.ecap == (640 if name == "big_record" else 512)
    nchunks, nruns, gmaxes = 0, [], set()
    for j in range(layout.nwg):
        for c, (m0, M, z, R, g) in enumerate(PC.chunks_of(plan, j)):
            at = f"{name} [{mode}]: ion {g}, workgroup {j}, chunk {c} (molecules {m0} .. {m0 + M - 1})"
            want = RO.chunk_run_table(case, g, m0, M)
            got = ops.read_plan_records(ws, records, j * layout.max_sub + c)
            assert int(want.hist.sum()) == z, f"{at}: the descriptor counts {z} valid edges, the host {int(want.hist.sum())}"
            assert got.nrun == want.nrun, f"{at}: nrun {got.nrun}, the reference has {want.nrun}"
            assert np.array_equal(got.runs, want.runs), f"{at}: run table {got.runs.tolist()}, reference {want.runs.tolist()}"
            assert np.array_equal(got.grp_type, want.grp_type), f"{at}: group types differ from the reference"
            assert np.array_equal(got.grp_edges, want.grp_edges), f"{at}: group edge counts differ from the reference"
            RO.check_run_table(want.hist, got.nrun, got.runs, got.grp_type, got.grp_edges, what=at)
            nchunks += 1
            nruns.append(got.nrun)
            gmaxes.add(want.gmax)
    print(f"{name} [{mode}]: {nchunks} chunks, runs per chunk {min(nruns)} .. {max(nruns)}, gmax {sorted(gmaxes)}")
    assert nchunks >= 2
    if name in ("three_long", "big_record"):
        assert max(gmaxes) >= 3
    if name == "empty_between":   # a chunk without a run between two chunks of its workgroup that have runs
        per_wg = [[ops.read_plan_records(ws, records, j * layout.max_sub + c).nrun for c in range(int(plan.nsub[j]))]
                  for j in range(layout.nwg)]
        assert any(n[c] == 0 and n[c - 1] > 0 and n[c + 1] > 0 for n in per_wg for c in range(1, len(n) - 1)), per_wg


# ---- the encoder on these records, against fp64
@pytest.mark.parametrize("mode", TYPED)
@pytest.mark.parametrize("name", NAMES)
def test_pooled_pair_against_fp64(name, mode):
    case = RO.COMPOSITIONS[name]()
    got = _run(case, mode)
    ref = RO.reference(name)
    for g, p in enumerate(PC.IONS):
        a = got[g].cpu().numpy()
        scale = max(float(np.abs(ref[g]).max()), 1e-30)
        print(f"{name} [{mode}] {p}: max abs err / scale = {float(np.abs(a - ref[g]).max()) / scale:.3e}")
        assert_close(a, ref[g], what=f"{name}, {mode}, {p} pooled")


# ---- a relabelling of the bond types moves runs around in the table, not a result
@pytest.mark.parametrize("mode", TYPED)
@pytest.mark.parametrize("name", NAMES)
def test_relabelled_bond_types_give_the_same_bits(name, mode):
    case = RO.COMPOSITIONS[name]()
    other, perm = RO.relabelled(case)
    # the tables' type columns themselves differ - but where every type present has the same pieces (one type; equal
    # counts), so that the relabelling moves edges between runs and leaves the column as it was
    if name not in ("one_type", "equal_counts"):
        _, _, la, pa, ra, wa = _planned(case, mode)
        _, _, lb, pb, rb, wb = _planned(other, mode)
        assert [PC.chunks_of(pa, j) for j in range(la.nwg)] == [PC.chunks_of(pb, j) for j in range(lb.nwg)]
        types = [[ops.read_plan_records(w, r, j * l.max_sub).grp_type.tolist() for j in range(l.nwg) if p.nsub[j] > 0]
                 for (l, p, r, w) in ((la, pa, ra, wa), (lb, pb, rb, wb))]
        assert types[0] != types[1], f"{name}: the relabelling leaves every first chunk's group table as it was"
    for table in (True, False):
        base, moved = _run(case, mode, table=table), _run(other, mode, table=table, perm=perm)
        for g, p in enumerate(PC.IONS):
            assert np.array_equal(_bits(base[g]), _bits(moved[g])), \
                f"{name}, {mode}, {p}, step-0 tables {table}: relabelling the bond types changes the bits"
