"""GPU: the plan kernels (csrc/encoder_plan.hip) read back and held against host rules, on batches composed to steer
every share and chunk path (tests/plan_cases.py).

Every composition is planned with ops.EncoderPipeline.plan into a workspace filled with 0xff bytes; the plan is read
back through the layout query (ops.encoder_plan_layout / ops.read_plan) and
  * holds the invariants of plan_cases.check_plan, as typed records (f32t) and as pull-form records (f32, where the
    padded shape is inside that form's limits);
  * went through the paths the composition was built for (plan_cases.paths), and all compositions together through
    every path, per record kind;
  * run by pipeline.run, gives the fp64 pooled pair of oracle/torch_ref within the project's 1e-5 (conftest.assert_close)
    in f32t, f32x3 and f32;
  * gives the same bits whatever the placement: 16 against 48 workgroups (other shares, other chunks - asserted from the
    descriptors), with and without the step-0 message table.
An in-degree of 256 raises ops.EncoderOverflow; 255 (the `hubs` composition) runs and matches fp64."""
import ctypes as C

import numpy as np
import pytest
import torch

import plan_cases as PC
from conftest import assert_close
from ionic_mpnn_amd import _lib
from ionic_mpnn_amd import model as MM
from ionic_mpnn_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = tuple(PC.COMPOSITIONS)
TYPED = ("f32t", "f32x3")
PULL = tuple(n for n in NAMES if PC.pull_form_covers(PC.COMPOSITIONS[n]()))
RUNS = [(n, m) for n in NAMES for m in TYPED] + [(n, "f32") for n in PULL]
_PLANS, _MODELS, _PREPARED, _DATA = {}, {}, {}, {}


def _case(name):
    return PC.hubs_overflow() if name == "hubs_256" else PC.COMPOSITIONS[name]()


def _data(name):
    if name not in _DATA:
        inp = _case(name).inp
        _DATA[name] = [tuple(torch.from_numpy(np.ascontiguousarray(inp[f"{p}_{k}"])).to(DEV)
                             for k in ("atom", "bond", "connectivity")) for p in PC.IONS]
    return _DATA[name]


def _model(Va, Vb):
    if (Va, Vb) not in _MODELS:
        m = MM.build_model(Va, Vb, atom_dim=32, bond_dim=PC.K, fp_size=32, mixing_size=20, num_steps=PC.S, device=DEV)
        m.load_weights(PC.case_weights(Va, Vb))
        _MODELS[(Va, Vb)] = (m, m.atom_emb.embeddings, m.bond_emb.embeddings, m._packed_weights())
    return _MODELS[(Va, Vb)]


def _prepared(Va, Vb, mode, table):
    key = (Va, Vb, mode, table)
    if key not in _PREPARED:
        _, atab, btab, packed = _model(Va, Vb)
        _PREPARED[key] = [ops.prepare_encoder_weights(packed[g], btab, 32, PC.K, PC.S, mode,
                                                      atom_table=atab if table else None) for g in range(2)]
    return _PREPARED[key]


def _planned(name, mode, workgroups=None):
    """-> (pipeline, plan handle, layout, plan read back) of the composition, planned once per (mode, workgroups) into a
    workspace of 0xff bytes."""
    case = _case(name)
    wgs = case.workgroups if workgroups is None else workgroups
    key = (name, mode, wgs)
    if key not in _PLANS:
        B = case.inp["cat_atom"].shape[0]
        layout = ops.encoder_plan_layout(2, B, case.N, case.E, 32, PC.K, PC.S, case.Vb, mode, wgs)
        need = C.c_size_t(0)
        ops.check(_lib.load().impnn_encoder_workspace_bytes(2, B, case.N, case.E, 32, PC.K, PC.S, case.Vb,
                                                            ops.ENCODER_MODES[mode], wgs, C.byref(need)))
        pipe = ops.EncoderPipeline(DEV, depth=1)
        dirty = torch.full((max(need.value, 1 << 20),), 0xff, dtype=torch.uint8, device=DEV)
        pipe.slots[0]["ws"] = dirty
        h = pipe.plan(_data(name), 32, PC.K, PC.S, case.Va, case.Vb, mode=mode, workgroups=wgs)
        assert h.slot["ws"].data_ptr() == dirty.data_ptr(), "the plan took another workspace than the dirtied one"
        assert h.info.v[8] == layout.nwg, "the layout query and the plan resolve different workgroup counts"
        h.ready.synchronize()
        _PLANS[key] = (pipe, h, layout, ops.read_plan(dirty, layout, 2, B))
    return _PLANS[key]


def _run(name, mode, workgroups=None, table=True):
    case = _case(name)
    pipe, h, _, _ = _planned(name, mode, workgroups)
    _, atab, btab, _ = _model(case.Va, case.Vb)
    out = pipe.run(h, atab, btab, _prepared(case.Va, case.Vb, mode, table and mode in TYPED))
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _kind_mode_names(kind):
    return ("f32t", NAMES) if kind == "typed" else ("f32", PULL)


# ---- the plan itself
@pytest.mark.parametrize("name,mode", [(n, "f32t") for n in NAMES] + [(n, "f32") for n in PULL])
def test_plan_holds_the_invariants_and_takes_its_paths(name, mode):
    case = _case(name)
    _, _, layout, plan = _planned(name, mode)
    PC.check_plan(case, layout, plan)
    got = PC.paths(case, layout, plan)
    print(f"{name} [{mode}]: nwg {layout.nwg}, max_sub {layout.max_sub}, vmin {layout.plan_vmin}, "
          f"most chunks of a workgroup {int(plan.nsub.max())}, paths {sorted(got)}")
    assert PC.BUILT_FOR[name] <= got, f"{name}: built for {sorted(PC.BUILT_FOR[name] - got)}, which the plan did not take"
    if name == "unequal_ions":   # part of its window misses are shares on the other ion than the guess (g != gg)
        assert PC.guessed_other_ion(layout, plan, 2, case.inp["cat_atom"].shape[0])


@pytest.mark.parametrize("kind", ["typed", "pull"])
def test_the_compositions_reach_every_path(kind):
    mode, names = _kind_mode_names(kind)
    got = set()
    for name in names:
        _, _, layout, plan = _planned(name, mode)
        got |= PC.paths(_case(name), layout, plan)
    print(f"{kind}: paths reached {sorted(got)}")
    assert got == set(PC.PATHS), f"{kind} records: no composition reaches {sorted(set(PC.PATHS) - got)}"


@pytest.mark.parametrize("name", NAMES)
def test_f32x3_plans_are_the_f32t_plans(name):
    """The two typed modes share the record kind; their workspaces differ in the image area in front of the plan."""
    _, _, la, pa = _planned(name, "f32t")
    _, _, lb, pb = _planned(name, "f32x3")
    assert (la.nwg, la.max_sub, la.ecap, la.plan_vmin) == (lb.nwg, lb.max_sub, lb.ecap, lb.plan_vmin)
    PC.check_plan(_case(name), lb, pb)
    assert [PC.chunks_of(pa, j) for j in range(la.nwg)] == [PC.chunks_of(pb, j) for j in range(lb.nwg)]


# ---- the encoder on these plans, against fp64
@pytest.mark.parametrize("name,mode", RUNS)
def test_pooled_pair_against_fp64(name, mode):
    got = _run(name, mode)
    ref = PC.reference(name)
    for g, p in enumerate(PC.IONS):
        a = got[g].cpu().numpy()
        scale = max(float(np.abs(ref[g]).max()), 1e-30)
        print(f"{name} [{mode}] {p}: max abs err / scale = {float(np.abs(a - ref[g]).max()) / scale:.3e}")
        assert_close(a, ref[g], what=f"{name}, {mode}, {p} pooled")


# ---- placement does not show in the bits
@pytest.mark.parametrize("mode", TYPED)
@pytest.mark.parametrize("name", NAMES)
def test_other_workgroup_counts_and_the_step0_table_give_the_same_bits(name, mode):
    case = _case(name)
    _, _, la, pa = _planned(name, mode)
    _, _, lb, pb = _planned(name, mode, 48)
    PC.check_plan(case, lb, pb)
    cuts = [[(j,) + c for j in range(l.nwg) for c in PC.chunks_of(p, j)] for l, p in ((la, pa), (lb, pb))]
    assert la.nwg != lb.nwg and cuts[0] != cuts[1], f"{name}: {la.nwg} and {lb.nwg} workgroups walk the same chunks"
    base = _run(name, mode)
    for what, other in (("48 workgroups", _run(name, mode, 48)), ("no step-0 table", _run(name, mode, table=False)),
                        ("48 workgroups, no step-0 table", _run(name, mode, 48, table=False))):
        for g, p in enumerate(PC.IONS):
            assert np.array_equal(_bits(base[g]), _bits(other[g])), f"{name}, {mode}, {p}: {what} changes the bits"


# ---- overflow: an in-degree of 256 does not travel in a typed record (255 does: `hubs` above)
@pytest.mark.parametrize("mode", TYPED)
def test_in_degree_256_raises_overflow(mode):
    with pytest.raises(ops.EncoderOverflow):
        _run("hubs_256", mode)
    assert all(np.isfinite(t.cpu().numpy()).all() for t in _run("hubs", mode))
