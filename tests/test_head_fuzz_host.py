"""tests/test_gpu_head_fuzz.py on the CPU: (1) attainability - every case of its two tables, the reference in fp32
against the reference in fp64 under the very checks the GPU tests apply to the kernels, on exactly their inputs: a
plain f32 implementation stays inside the bounds, so a kernel that does not has a defect, not a hard case; (2) every
case's restated branch equals what its row claims, and the claims together cover a literal set of branches; (3) every
case's content condition and the kink condition hold in the fp64 reference (a seed that violates one fails here, not on
the GPU); (4) head_ref is the oracle's head; (5) the rule that decides whether a training pass takes the fused head
nodes reads the launcher's own LDS fit."""
import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, model as MM, ops
from oracle import torch_ref as TR

import head_ref as HR
import test_gpu_head_fuzz as FZ
import transfer_ref as R

F32, F64 = torch.float32, torch.float64
HEAD_CASES, TH_CASES = FZ.model_head_cases(), FZ.transfer_cases()


def ids(cases):
    return [c.name for c in cases]


# --------------------------------------------------------------------------------------------- model head
@pytest.mark.parametrize("c", HEAD_CASES, ids=ids(HEAD_CASES))
def test_f32_attains_the_model_head_bounds(c):
    br = FZ.model_head_branch(c)
    assert br == FZ.HeadBranch(c.groups, c.loss_sum, c.passes, c.lanes, c.lds, c.backward), br
    assert FZ.head_floats(c.kind, c.D, c.F, c.Mx) == _lib.load().impnn_model_head_floats(c.kind, c.D, c.F, c.Mx)
    assert br.fits == ops.model_head_bwd_fits(c.kind, c.D, c.F, c.Mx)
    inp = FZ.model_head_inputs(c)
    ref64, ref32 = FZ.model_head_reference(c, inp, F64), FZ.model_head_reference(c, inp, F32)
    FZ.model_head_content(c, inp, ref64)
    FZ.check_model_head(c, ref32, ref64)
    live = min(c.B, FZ.POOL_ROWS)
    assert len(np.unique(inp["pc"], axis=0)) == live and len(np.unique(inp["y"])) >= 0.99 * c.B   # (fp32 collisions)


def test_model_head_cases_cover_the_branches():
    cs = HEAD_CASES
    assert {c.kind for c in cs} == {0, 1}
    for kind in (0, 1):
        k = [c for c in cs if c.kind == kind]
        assert {c.B for c in k if (c.D, c.F, c.Mx) == (8, 5, 3)} == {1, 7, 8, 9, 2049, 4097, 8200}
        assert {c.loss_sum for c in k} == {"first is last", "one stride", "second stride"}
        assert {c.passes for c in k} == {1, 2, 3} and {c.lanes for c in k if c.backward} == {1, 2}
        assert {c.lds for c in k} == {"ddd", "dda", "daa", "aaa", "aa-"}
        assert any(c.F > 32 and c.Mx > 32 and c.backward for c in k), "the second output of a lane is differentiated"
        assert {(c.D, c.F, c.Mx) for c in k if c.B == 9} >= {(1, 1, 1), (33, 31, 33), (32, 32, 32), (64, 33, 64), (128, 64, 64)}
    # B = 4097: workgroup 0 takes a second group that holds one live sample
    c = next(c for c in cs if c.B == 4097)
    assert c.groups == FZ.BWD_MAX_WORKGROUPS + 1 and c.B - FZ.BWD_MAX_WORKGROUPS * FZ.HEAD_SPB == 1
    # the widest heads the backward holds, and the refused neighbour tests/test_cabi.py sends
    wide = {c.kind: c for c in cs if c.name.startswith("widest backward")}
    assert (wide[0].D, wide[0].F, wide[0].Mx) == (128, 48, 29) and FZ.head_floats(0, 128, 48, 29) == 15316
    assert FZ.head_floats(0, 128, 48, 30) == 15417 and not ops.model_head_bwd_fits(0, 128, 48, 30)
    assert wide[1].F == 64 and wide[1].Mx > 32 and ops.model_head_bwd_fits(1, wide[1].D, 64, wide[1].Mx)
    assert not ops.model_head_bwd_fits(1, wide[1].D + 1, 64, wide[1].Mx)


@pytest.mark.parametrize("kind", [0, 1])
def test_head_ref_is_the_oracle_head(kind):
    """head_ref.forward against oracle/torch_ref.py's whole-model forward on a model without message-passing steps,
    whose pooled vector of a one-atom ion is that atom's embedding row."""
    B, D, F, Mx = 11, 7, 6, 5
    rng = np.random.default_rng(kind)
    w = [torch.tensor(rng.normal(0.0, 0.7, s)) for s in HR.tensor_shapes(kind, D, F, Mx)]
    table = rng.normal(0.0, 1.0, (2 * B + 1, D))
    T = rng.uniform(250.0, 400.0, (B, 1))
    names = ["cat_fp", "an_fp", "cat_proj", "an_proj"] + (["visc_params"] if kind == 0 else ["mp_hidden", "mp_out"])
    ow = {"atom_embedding": table, "bond_embedding": np.zeros((2, 3))}
    for i, n in enumerate(names):
        ow[f"{n}/kernel"], ow[f"{n}/bias"] = w[2 * i].numpy(), w[2 * i + 1].numpy()
    cat = np.arange(1, B + 1).reshape(B, 1)
    inputs = {"cat_atom": cat, "an_atom": cat + B, "cat_bond": np.zeros((B, 1), np.int64), "an_bond": np.zeros((B, 1), np.int64),
              "cat_connectivity": np.zeros((B, 1, 2), np.int64), "an_connectivity": np.zeros((B, 1, 2), np.int64),
              "temperature": T}
    want = (TR.viscosity_forward if kind == 0 else TR.melting_point_forward)(ow, inputs, F64).reshape(-1)
    got = HR.forward(kind, w, torch.tensor(table[1:B + 1]), torch.tensor(table[B + 1:]), torch.tensor(T))
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    x = torch.linspace(-700.0, 700.0, 3501, dtype=F64)   # (the oracle's form overflows beyond 709)
    naive = torch.nn.functional.softplus(x, threshold=1e9)
    assert float(((HR.softplus(x) - naive).abs() / naive.clamp(min=1.0)).max()) <= 1e-15


# --------------------------------------------------------------------------------------------- transfer head
@pytest.mark.parametrize("c", TH_CASES, ids=ids(TH_CASES))
def test_f32_attains_the_transfer_head_bounds(c):
    br = FZ.transfer_branch(c)
    assert br[0:2] + br[3:] == (c.loss_sum, c.stats, c.flags, c.jobs, c.dense), br
    assert br.launches == (3 + 4 if c.bn else 1 + 3) - (0 if c.jobs else 1)   # forward + backward; no job: no th_param_grads
    inp = FZ.transfer_inputs(c)
    assert [a.shape for a in inp["w"]] == FZ.transfer_shapes(c.D, c.F, c.Mx)
    ref64, ref32 = FZ.transfer_reference(c, inp, F64), FZ.transfer_reference(c, inp, F32)
    FZ.transfer_content(c, inp, ref64)
    FZ.check_transfer(c, ref32, ref64)


def test_transfer_cases_cover_the_branches():
    cs = TH_CASES
    base = [c for c in cs if (c.D, c.F, c.Mx) == (32, 32, 20)]
    assert {c.B for c in base} >= {1, 2, 7, 8, 9, 15, 16, 17, 33, 300, 2049}
    assert {(c.D, c.F, c.Mx) for c in cs if c.B == 9} >= {(1, 1, 1), (3, 5, 3), (33, 31, 33), (64, 48, 24), (128, 64, 64)}
    assert {c.loss_sum for c in cs} == {"first is last", "one stride", "second stride"}
    assert {c.stats for c in cs} == {"idle lanes", "one each", "strided"}
    assert {c.dense for c in cs} == {"even", "idle", "empty", "idle+empty"}
    assert FZ.dense_parts(3, 5) == (51, 1, 48) and FZ.dense_parts(64, 48)[:2] == (5, 16)
    for B in (9, 17):   # every value of every setting, with both batch sizes
        k = [c for c in base if c.B == B]
        assert {c.bn for c in k} == {0, 1} and {c.loss for c in k} == {FZ.HUBER1, FZ.HUBER025, FZ.MSE}
        assert {c.rate for c in k} == {0.0, 0.3} and {c.sinks for c in k} == {False, True}
        assert {id(c.l2) for c in k} == {id(FZ.KERAS_L2), id(FZ.ANY_L2)}
        assert {c.wants for c in k} == set(FZ.WANTS)
        assert {(c.flags, c.jobs) for c in k} == {("base+pooled", 16), ("none", 8), ("base", 1), ("base+pooled", 0), ("none", 1)}
    # l2 on arbitrary tensors: kernels, biases, gamma and beta, and tensors without one
    lam = FZ.ANY_L2
    assert all(lam[t] > 0 for t in (0, 1, 4, 8, 9, 10, 11, 12, 15, 16, 17)) and lam[6] == 0 and lam[13] == 0
    assert any(c.l2 is lam and c.bn and 11 in FZ.asked(c) for c in cs)


def test_transfer_ref_head_loss_is_its_whole_model_loss():
    """head_loss with the model's lambdas on the pooled vectors is transfer_ref.loss's value past the encoder."""
    c = next(c for c in TH_CASES if c.name == "B=17 batch huber.25 drop keras")
    inp = FZ.transfer_inputs(c)
    w, pc, pa = FZ._transfer_tensors(inp, F64)
    mask = FZ.transfer_mask(c)
    a = R.head_loss(w, pc, pa, inp["y"], [1e-4, 0, 1e-4] + [0] * 15, True, mask, 0.25)
    pred, mm, mv = R.head(w, pc, pa, True, mask)
    e = pred - torch.tensor(inp["y"], dtype=F64)
    want = R.huber(e, 0.25).mean() + 1e-4 * ((w["cat_fp/kernel"] ** 2).sum() + (w["an_fp/kernel"] ** 2).sum())
    assert float(a[0]) == float(want) and torch.equal(a[2], mm) and torch.equal(a[3], mv)


# --------------------------------------------------------------------------------------------- the shared rule
def test_the_training_rule_reads_the_backward_lds_fit():
    """ops.HEAD_BWD_MAX_FLOATS, which decides in model.py whether a training pass takes the fused head nodes, is the
    launcher's own limit (impnn_model_head_bwd_max_floats); inference and the grids keep the width rule alone."""
    lib = _lib.load()
    assert ops.HEAD_BWD_MAX_FLOATS == lib.impnn_model_head_bwd_max_floats() == FZ.BWD_MAX_FLOATS == 15360
    cpu = torch.device("cpu")
    for kw, fits in ((dict(atom_dim=64, fp_size=64, mixing_size=64), False), (dict(atom_dim=128, fp_size=48, mixing_size=29), True),
                     (dict(atom_dim=128, fp_size=48, mixing_size=30), False), (dict(atom_dim=32, fp_size=32, mixing_size=20), True),
                     (dict(atom_dim=128, fp_size=64, mixing_size=65), False)):
        m = MM.build_model(11, 6, bond_dim=4, num_steps=1, device=cpu, **kw)
        assert m._head_kernels_cover() == (kw["mixing_size"] <= ops.HEAD_MAX_DIM)
        assert m._head_nodes_cover() == fits, kw
        assert m._grid_kernels_cover() == m._head_kernels_cover()
    m = MM.build_melting_point_model(11, 6, atom_dim=16, fp_size=64, mixing_size=64, num_steps=1, device=cpu)
    assert m._head_nodes_cover() == ops.model_head_bwd_fits(1, 16, 64, 64)
