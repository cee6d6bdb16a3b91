"""tests/grad_ref.py on the CPU: (1) equal to oracle/torch_ref.py in fp64 - forward and every autograd gradient - on small
random dense multigraphs with holes and masked edges; (2) attainability: every case of tests/test_gpu_train_fuzz.py,
grad_ref in fp32 against grad_ref in fp64 under the very checks the GPU tests apply to the kernels - a plain f32
implementation stays inside the bounds on these inputs, so a kernel that does not has a defect, not a hard case."""
import numpy as np
import pytest
import torch

from ionic_mpnn_amd import weights
from oracle import torch_ref as TR, train_oracle as TO

import grad_ref as GR
import test_gpu_train_fuzz as FZ

DT = torch.float64


def tight(got, ref, what):
    """1e-12 of the tensor's scale."""
    got, ref = got.detach().numpy(), ref.detach().numpy()
    assert got.shape == ref.shape, what
    assert got.size == 0 or np.abs(got - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300), what


def small_case(seed):
    rng = np.random.default_rng(seed)
    D = (3, 8, 16)[seed % 3]
    kind = "melting_point" if seed % 4 == 3 and D <= 8 else "viscosity"
    K = D * D if kind == "melting_point" else int(rng.integers(1, 6))
    B, N = int(rng.integers(1, 7)), int(rng.integers(1, 12))
    E = int(rng.integers(0, 3 * N + 1))
    Va, Vb, S = int(rng.integers(2, 9)), int(rng.integers(1, 7)), int(rng.integers(1, 4))
    inp = {}
    for p in ("cat", "an"):
        ids = rng.integers(0, Va, size=(B, N)).astype(np.int32)
        ids[rng.random((B, N)) < 0.25] = 0                                   # holes anywhere
        inp[p + "_atom"] = ids
        inp[p + "_connectivity"] = rng.integers(0, N, size=(B, E, 2)).astype(np.int32)   # index 0: masked edges
        inp[p + "_bond"] = rng.integers(0, Vb, size=(B, E)).astype(np.int32)
    if kind == "viscosity":
        inp["temperature"] = rng.uniform(280.0, 400.0, size=(B, 1)).astype(np.float32)
    w = weights.init_weights(kind, Va, Vb, atom_dim=D, bond_dim=K, fp_size=6, mixing_size=5, num_steps=S, seed=seed,
                             perturb=True)
    y = rng.normal(1.0, 0.5, size=B)
    return kind, D, K, B, N, E, Vb, inp, w, y, rng


@pytest.mark.parametrize("seed", range(20))
def test_grad_ref_equals_the_oracle_in_fp64(seed):
    kind, D, K, B, N, E, Vb, inp, w, y, rng = small_case(seed)
    # the message step: forward, dh, dbond_table, dW
    vals = [rng.normal(size=s) for s in ((B, N, D), (Vb, K), (K, D, D))]
    go = torch.tensor(rng.normal(size=(B, N, D)))
    conn, bond = torch.tensor(inp["cat_connectivity"]), torch.tensor(inp["cat_bond"])
    leaves = lambda: [torch.tensor(v, dtype=DT, requires_grad=True) for v in vals]
    h0, tb0, W0 = leaves()
    m = TR.bond_matrix_message(h0, torch.nn.functional.embedding(bond.long(), tb0), conn, W0)
    agg0 = TR.reduce_messages(m, conn[:, :, 1], N)
    h1, tb1, W1 = leaves()
    agg1 = GR.message_reduce(h1, tb1, W1, bond, conn, N)
    tight(agg1, agg0, "message + reduce")
    tight(GR.messages_from_matrices(h1, GR.type_matrices(tb1, W1), bond, conn), m, "messages")
    if E:
        (agg0 * go).sum().backward()
        if agg1.requires_grad:
            (agg1 * go).sum().backward()
        for a, b, what in ((h1, h0, "dh"), (tb1, tb0, "dbond_table"), (W1, W0, "dW")):
            z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad   # (no valid edge: no graph at all)
            tight(z(a), z(b), what)
    # the whole model: loss and every weight's gradient
    fwd = TR.viscosity_forward if kind == "viscosity" else TR.melting_point_forward
    l2 = 1e-4 if kind == "viscosity" else 1e-5
    names = ["cat_fp/kernel", "an_fp/kernel"] + (["mp_hidden/kernel"] if kind == "melting_point" else [])
    wa = {k: torch.tensor(v, dtype=DT, requires_grad=True) for k, v in w.items()}
    la = torch.mean((fwd(wa, inp, DT).reshape(-1) - torch.tensor(y)) ** 2) + l2 * sum((wa[n] ** 2).sum() for n in names)
    la.backward()
    wb = {k: torch.tensor(v, dtype=DT, requires_grad=True) for k, v in w.items()}
    lb = GR.model_loss(kind, wb, inp, y, l2, DT)
    lb.backward()
    assert TR.encode.__module__ == TR.__name__, "grad_ref puts oracle/torch_ref.py's encode back"
    tight(lb, la, "loss")
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad   # (an ion without a valid edge: no path at all)
    for k in w:
        tight(z(wb[k]), z(wa[k]), f"grad {k}")


def test_out_of_range_bond_ids_carry_no_message():
    rng = np.random.default_rng(0)
    B, N, E, D, Vb = 3, 6, 14, 4, 5
    h, A = torch.tensor(rng.normal(size=(B, N, D))), torch.tensor(rng.normal(size=(Vb, D, D)))
    conn = torch.tensor(rng.integers(1, N, size=(B, E, 2)))
    bond = torch.tensor(rng.integers(0, Vb, size=(B, E)))
    bad = bond.clone()
    bad[:, ::3] = torch.tensor([-1, Vb, Vb + 7, -1, Vb])[None, :]
    masked = conn.clone()
    masked[:, ::3] = 0
    tight(GR.message_reduce_from_matrices(h, A, bad, conn, N), GR.message_reduce_from_matrices(h, A, bond, masked, N),
          "ids outside [0, Vb) act as masked edges")


# --------------------------------------------------------------------------------------------- attainability
@pytest.mark.parametrize("c", FZ.message_cases(), ids=[c.name for c in FZ.message_cases()])
def test_f32_attains_the_message_adjoint_bounds(c):
    assert FZ.message_branch(c) == (c.sort, c.kernel)
    inp = FZ.message_inputs(c)
    FZ.check_message(c, *FZ.message_reference(c, inp, torch.float32), *FZ.message_reference(c, inp, DT))


@pytest.mark.parametrize("D,rows,kept", FZ.gated_update_cases())
def test_f32_attains_the_gated_update_bounds(D, rows, kept):
    inp = FZ.gated_update_inputs(D, rows, kept)
    FZ.check_gated_update(f"D={D} rows={rows}", FZ.gated_update_reference(inp, torch.float32),
                          FZ.gated_update_reference(inp, DT))


def _adam_f32(ws, steps, clip, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
    """oracle/train_oracle.adam_step's arithmetic with every value held in float32."""
    f = np.float32
    state = [(w.copy(), np.zeros_like(w), np.zeros_like(w)) for w in ws]
    out = []
    for t, gs in enumerate(steps, 1):
        alpha = f(lr) * np.sqrt(f(1) - f(b2) ** f(t)) / (f(1) - f(b1) ** f(t))
        new = []
        for (w, m, v), g in zip(state, gs):
            if clip:
                g = g * (f(clip) / max(np.sqrt(np.sum(g * g, dtype=f)), f(clip)))
            m = f(b1) * m + (f(1) - f(b1)) * g
            v = f(b2) * v + (f(1) - f(b2)) * g * g
            new.append((w - alpha * m / (np.sqrt(v) + f(eps)), m, v))
            assert new[-1][0].dtype == np.float32
        state = new
        out.append([s[0] for s in state])
    return out


@pytest.mark.parametrize("form,clip", FZ.adam_cases())
def test_f32_attains_the_adam_bound(form, clip):
    ws, steps = FZ.adam_inputs()
    ref = FZ.adam_reference(ws, steps, clip)
    for t, (got, want) in enumerate(zip(_adam_f32(ws, steps, clip), ref), 1):
        FZ.check_adam(f"clipnorm {clip}, step {t}", got, want)
    # the table holds what the issue asks of it
    norms = [np.sqrt(np.sum(g.astype(np.float64) ** 2)) for g in steps[0]]
    assert any(n > 1.5 for n in norms) and any(n < 0.5 for n in norms)
    for gs in steps:   # variables 0, 2 and 5 clip at clipnorm 1, variables 1, 4 and 6 do not
        norms = [np.sqrt(np.sum(g.astype(np.float64) ** 2)) for g in gs]
        assert all(norms[i] > 1.5 for i in (0, 2, 5)) and all(norms[i] < 0.5 for i in (1, 4, 6))
        for i in (0, 2, 5):
            assert not np.array_equal(TO.clip_by_norm(gs[i], 1.0), gs[i])
        for i in (1, 4, 6):
            assert np.array_equal(TO.clip_by_norm(gs[i], 1.0), gs[i])


@pytest.mark.parametrize("D,V", FZ.embedding_cases())
def test_f32_attains_the_embedding_bounds(D, V):
    inp = FZ.embedding_inputs(D, V)
    share = [(inp["ids"] == v).mean() for v in (0, FZ.EMBED_HOT)]
    assert abs(share[0] - 0.6) < 0.01 and abs(share[1] - 0.3) < 0.01
    assert FZ.embedding_form(D, V) == ("global atomics" if V == 200 else "lds")
    FZ.check_embedding(f"D={D} V={V}", FZ.embedding_reference(inp, torch.float32)[1], FZ.embedding_reference(inp, DT)[1])


@pytest.mark.parametrize("seed", FZ.model_cases())
def test_f32_attains_the_whole_model_bounds(seed):
    c = FZ.model_case(seed)
    if seed < 8:
        assert FZ.threshold_sides(c) == FZ.THRESHOLD_SIDES[seed % 4]
    for y in c["y"]:
        loss32, g32 = FZ.model_reference(c, y, torch.float32)
        loss64, g64 = FZ.model_reference(c, y, DT)
        FZ.assert_reference_is_alive(f"seed {seed}", g64)   # (no seed may compare zeros with zeros)
        FZ.check_model(f"seed {seed}", loss32, g32, loss64, g64)


def test_the_seed_plan_covers_what_it_claims():
    cs = [FZ.model_case(s) for s in FZ.model_cases()]
    assert len(cs) == 32
    assert {c["D"] for c in cs} == {8, 16, 32, 64, 128} and {c["kind"] for c in cs} == {"viscosity", "melting_point"}
    assert all(c["D"] <= 16 and c["K"] == c["D"] ** 2 for c in cs if c["kind"] == "melting_point")
    assert sum(c["frozen"] for c in cs) == 8 and sum(c["single"] for c in cs) == 8
    assert sum(c["dropout"] for c in cs) == 2 and sum(c["interleaved"] for c in cs) == 2
    for c in cs:
        if c["frozen"]:
            assert "bond_embedding" in c["frozen_layers"] and any("_gu_" in n for n in c["frozen_layers"])
        assert not (c["interleaved"] and (c["frozen"] or c["dropout"]))
        if c["interleaved"]:   # on the wide kernels, with an ion at or above each threshold of the training pass
            sides = FZ.threshold_sides(c)
            assert c["D"] in (64, 128) and any(s[0] for s in sides) and any(s[1] for s in sides)
        for p in ("cat", "an"):   # all-padding molecules stay a fraction of a batch: some molecule pools a real atom
            assert (c["inputs"][p + "_atom"] > 0).any(), (c["seed"], p)
    assert {c["D"] for c in cs if c["interleaved"]} == {64, 128}
    for D, seeds in ((64, range(0, 4)), (128, range(4, 8))):
        sides = [s for i in seeds for s in FZ.threshold_sides(cs[i])]
        assert all(cs[i]["D"] == D for i in seeds)
        assert {s[0] for s in sides} == {True, False} and {s[1] for s in sides} == {True, False}
        shapes = [(cs[i]["B"] * n, cs[i]["B"] * e) for i in seeds for n, e in (cs[i]["cat"], cs[i]["an"])]
        assert {4095, 4096} <= {r for r, _ in shapes} and {8191, 8192} <= {e for _, e in shapes}
    # holes that matter: id 0 inside the kept prefix on a valid edge, and all-padding molecules
    c = cs[9]
    ids, conn = c["inputs"]["cat_atom"], c["inputs"]["cat_connectivity"]
    assert conn.shape[1] > 0
    src_id = np.take_along_axis(ids, conn[:, :, 0], 1)
    assert ((src_id == 0) & (conn[:, :, 0] > 0) & (conn[:, :, 1] > 0)).any()
    assert any((c["inputs"]["cat_atom"] == 0).all(1).any() for c in cs)
