"""GatedUpdate dropout on the GPU: the mask fused into the forward and backward kernels against the
numpy Philox reference, its statistics, rate 0 / inference as the dropout-free path bit for bit, gradients against
fp64 autograd over oracle/torch_ref.py with the same masks, and the captured training step."""
import numpy as np
import pytest
import torch

from ionic_mpnn_amd import layers as L, model as MM, ops, synthetic, train, weights
from oracle import torch_ref as TR

from test_dropout_host import reference_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"


def close(got, ref, tol=1e-4, what=""):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = ref.detach().cpu().double().numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(np.abs(ref).max(), 1e-12)
    err = np.abs(got - ref).max() / scale
    assert err <= tol, f"{what}: rel err {err:.3e} > {tol}"


def step_tensor(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def layer_and_inputs(D, B=7, N=23, seed=0, rate=0.5):
    g = L.GatedUpdate(D, dropout_rate=rate, dropout_seed=0x1234_5678_9ABC + D, device=DEV)
    g.build(None)
    g.built = True
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for t in g.weights:
            t.copy_(torch.tensor(rng.normal(0.0, 0.3, size=tuple(t.shape)), dtype=torch.float32))
    h = torch.tensor(rng.normal(size=(B, N, D)), dtype=torch.float32, device=DEV)
    agg = torch.tensor(rng.normal(size=(B, N, D)), dtype=torch.float32, device=DEV)
    return g, h, agg


@pytest.mark.parametrize("rate", [0.1, 0.5])
@pytest.mark.parametrize("D", [8, 32, 64, 128])
def test_drop_in_layer_applies_the_philox_mask(D, rate):
    g, h, agg = layer_and_inputs(D, rate=rate)
    with torch.no_grad():
        ref = g([h, agg], training=False)
        out = g([h, agg], training=True)           # the layer's first training call: step 0
    rows = h.numel() // D
    want = reference_mask(g.dropout_seed, 0, 0, rate, rows, D)
    mask = ops.dropout_mask(ops.Dropout(rate, g.dropout_seed, 0, step_tensor(0)), rows, D)
    assert np.array_equal(mask.cpu().numpy(), want)
    assert torch.equal(out, ref * mask.view_as(ref))
    assert int(g.dropout_counter().item()) == 1


def test_mask_statistics_and_freshness():
    rate, rows, D = 0.3, 4096, 64
    d = lambda step, lw=0, seed=5: ops.Dropout(rate, seed, lw, step_tensor(step))
    m = ops.dropout_mask(d(0), rows, D)
    keep = float((m > 0).double().mean())
    assert abs(keep - (1 - rate)) <= 5 * np.sqrt(rate * (1 - rate) / m.numel())
    assert torch.equal(m, ops.dropout_mask(d(0), rows, D))              # same seed and step: same mask
    for other in (d(1), d(0, lw=ops.dropout_layer_word(3)), d(0, lw=ops.dropout_layer_word(0, rank=1)), d(0, seed=6),
                  d(1 << 32)):
        assert not torch.equal(m, ops.dropout_mask(other, rows, D))
    # the row-list form draws the rows the list names
    idx = torch.tensor([5, 17, 4000], dtype=torch.int32, device=DEV)
    ml = ops.dropout_mask(d(0), rows, D, row_list=(idx, torch.tensor([3], dtype=torch.int32, device=DEV)))
    assert torch.equal(ml[idx.long()], m[idx.long()]) and float(ml.abs().sum()) == float(m[idx.long()].abs().sum())
    # consecutive training calls of a layer draw different masks
    g, h, agg = layer_and_inputs(32, rate=0.5)
    with torch.no_grad():
        a, b = g([h, agg], training=True), g([h, agg], training=True)
    assert not torch.equal(a == 0, b == 0)


@pytest.mark.parametrize("D", [8, 32, 128])
def test_rate_zero_and_inference_are_the_plain_layer(D):
    g0, h, agg = layer_and_inputs(D, rate=0.0)
    g1 = L.GatedUpdate(D, dropout_rate=0.4, device=DEV)
    g1.build(None)
    g1.built = True
    g1.set_weights(g0.get_weights())
    with torch.no_grad():
        plain = ops.gated_update(h, agg, *g0.weights, eps=g0.epsilon)
        assert torch.equal(g0([h, agg], training=True), plain)
        assert torch.equal(g1([h, agg], training=False), plain)
        assert torch.equal(g1([h, agg]), plain)


@pytest.mark.parametrize("D", [8, 32, 64, 128])
def test_layer_backward_against_fp64_oracle(D):
    rate = 0.35
    g, h, agg = layer_and_inputs(D, B=5, N=19, seed=D, rate=rate)
    ws = [t.detach().clone().requires_grad_(True) for t in g.weights]
    hg, ag = h.clone().requires_grad_(True), agg.clone().requires_grad_(True)
    step = step_tensor(41)
    drop = ops.Dropout(rate, g.dropout_seed, 9, step)
    out = ops.gated_update(hg, ag, *ws, eps=g.epsilon, dropout=drop)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(D)).to(DEV)
    (out * go).sum().backward()
    mask = torch.tensor(reference_mask(g.dropout_seed, 41, 9, rate, h.numel() // D, D), dtype=torch.float64).view(h.shape)
    ho, ao = (t.detach().cpu().double().requires_grad_(True) for t in (h, agg))
    wo = [t.detach().cpu().double().requires_grad_(True) for t in g.weights]
    p = dict(zip(("Wz", "bz", "Wr", "br", "Wh", "bh", "gamma", "beta"), wo))
    ref = TR.gated_update(ho, ao, p) * mask
    close(out, ref, 1e-5, "out")
    (ref * go.cpu().double()).sum().backward()
    close(hg.grad, ho.grad, what="dh")
    close(ag.grad, ao.grad, what="dagg")
    for n, a, b in zip(g.weight_names(), ws, wo):
        close(a.grad, b.grad, what=f"d{n}")


def _masked_oracle(monkeypatch, seed, step, rate, S, B, N, D):
    """oracle/torch_ref.py's encode with every GatedUpdate output times the mask of its layer (cation i: i, anion i:
    S + i - the order in which viscosity_forward calls them)."""
    calls = []
    plain = TR.gated_update

    def masked(h, agg, p, eps=1e-3):
        k = len(calls)
        calls.append(k)
        m = reference_mask(seed, step, ops.dropout_layer_word(k), rate, B * N, D)
        return plain(h, agg, p, eps) * torch.tensor(m, dtype=h.dtype).view(B, N, D)

    monkeypatch.setattr(TR, "gated_update", masked)
    return calls


@pytest.mark.parametrize("D,B", [(32, 40), (128, 120)])
def test_model_gradients_with_dropout_against_the_oracle(monkeypatch, D, B):
    """Whole-model gradients with dropout: atom_dim 32 (no row list) and 128 with B * N above the row-list threshold
    (row list, saved activations), against fp64 autograd with each layer's mask reproduced from the pass's step."""
    Va, Vb, K, S, rate, seed = 13, 6, 4, 2, 0.2, 2024
    w = weights.init_weights("viscosity", Va, Vb, atom_dim=D, bond_dim=K, fp_size=12, mixing_size=10, num_steps=S,
                             seed=19, perturb=True)
    m = MM.build_model(Va, Vb, atom_dim=D, bond_dim=K, fp_size=12, mixing_size=10, num_steps=S, device=DEV,
                       dropout_rate=rate, dropout_seed=seed)
    m.load_weights(w)
    inp = synthetic.make_batch(B, max_atoms=36, max_edges=72, atom_vocab_size=Va, bond_vocab_size=Vb, min_atoms=3,
                               seed=19)
    N = inp["cat_atom"].shape[1]
    assert inp["an_atom"].shape[1] == N
    if D == 128:
        assert B * N >= MM.TRAIN_ROW_LIST_MIN_ROWS
    y = np.random.default_rng(19).normal(1.0, 0.5, size=B).astype(np.float32)
    m.compile(train.Adam(1e-3, clipnorm=1.0))
    m.dropout_counter().fill_(7)
    loss = m._loss(m._to_device(inp), y, training=True)   # the pass's step: 7
    loss.backward()
    assert int(m.dropout_counter().item()) == 8
    calls = _masked_oracle(monkeypatch, seed, 7, rate, S, B, N, D)
    wo = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in w.items()}
    pred = TR.viscosity_forward(wo, inp, torch.float64)
    assert len(calls) == 2 * S
    lo = torch.mean((pred.reshape(-1) - torch.tensor(y, dtype=torch.float64)) ** 2) \
        + 1e-4 * ((wo["cat_fp/kernel"] ** 2).sum() + (wo["an_fp/kernel"] ** 2).sum())
    lo.backward()
    close(loss, lo, 1e-5, "loss")
    for name, t in m.trainable_variables():
        close(t.grad, wo[name].grad, 2e-4, f"grad {name}")


def test_model_inference_and_rate_zero_are_unchanged():
    Va, Vb, D, S, B = 13, 6, 32, 2, 24
    w = weights.init_weights("viscosity", Va, Vb, atom_dim=D, bond_dim=4, fp_size=12, mixing_size=10, num_steps=S, seed=3)
    inp = synthetic.make_batch(B, max_atoms=36, max_edges=72, atom_vocab_size=Va, bond_vocab_size=Vb, seed=3)
    y = np.random.default_rng(3).normal(1.0, 0.5, size=B).astype(np.float32)
    out = {}
    for rate in (0.0, 0.3):
        m = MM.build_model(Va, Vb, atom_dim=D, bond_dim=4, fp_size=12, mixing_size=10, num_steps=S, device=DEV,
                           dropout_rate=rate, dropout_seed=1)
        m.load_weights(w)
        out[rate] = (m.predict(inp), m(inp, fused=False).cpu(), m.evaluate(inp, y),
                     float(m._loss(m._to_device(inp), y, training=True)))
    for a, b in zip(out[0.0][:3], out[0.3][:3]):   # inference never applies dropout
        assert np.array_equal(np.asarray(a), np.asarray(b))
    plain = MM.build_model(Va, Vb, atom_dim=D, bond_dim=4, fp_size=12, mixing_size=10, num_steps=S, device=DEV)
    plain.load_weights(w)
    assert out[0.0][3] == float(plain._loss(plain._to_device(inp), y, training=True))   # rate 0 trains as before
    assert out[0.3][3] != out[0.0][3]


def test_fit_graphed_follows_eager_with_dropout():
    Va, Vb, D, S, n, bs = 13, 6, 32, 2, 96, 32
    w = weights.init_weights("viscosity", Va, Vb, atom_dim=D, bond_dim=4, fp_size=12, mixing_size=10, num_steps=S, seed=4)
    inp = synthetic.make_batch(n, max_atoms=36, max_edges=72, atom_vocab_size=Va, bond_vocab_size=Vb, seed=4)
    y = np.random.default_rng(4).normal(1.0, 0.5, size=n).astype(np.float32)
    hist = {}
    for rate, graph in ((0.2, False), (0.2, True), (0.0, False)):
        m = MM.build_model(Va, Vb, atom_dim=D, bond_dim=4, fp_size=12, mixing_size=10, num_steps=S, device=DEV,
                           dropout_rate=rate, dropout_seed=12)
        m.load_weights(w)
        m.compile(train.Adam(1e-3, clipnorm=1.0))
        hist[(rate, graph)] = m.fit(inp, y, epochs=3, batch_size=bs, seed=0, graph=graph).history["loss"]
        if rate:
            assert int(m.dropout_counter().item()) == 3 * n // bs
    np.testing.assert_allclose(hist[(0.2, True)], hist[(0.2, False)], rtol=1e-4, atol=1e-4)
    assert not np.allclose(hist[(0.2, False)], hist[(0.0, False)], rtol=1e-4, atol=1e-4)


def test_interleaved_training_passes_keep_their_own_masks():
    """Two differentiable passes of a dropout model with interleaved backwards (forward A, forward B, backward B,
    backward A): each pass draws its own mask (its own snapshot of the step counter) and gets the loss and gradients
    of that pass run alone with the same step."""
    Va, Vb, D, K, S, B = 13, 6, 128, 4, 2, 120
    w = weights.init_weights("viscosity", Va, Vb, atom_dim=D, bond_dim=K, fp_size=12, mixing_size=10, num_steps=S, seed=21,
                             perturb=True)
    m = MM.build_model(Va, Vb, atom_dim=D, bond_dim=K, fp_size=12, mixing_size=10, num_steps=S, device=DEV,
                       dropout_rate=0.25, dropout_seed=31)
    m.load_weights(w)
    d = m._to_device(synthetic.make_batch(B, max_atoms=36, max_edges=72, atom_vocab_size=Va, bond_vocab_size=Vb,
                                          min_atoms=3, seed=21))
    y = np.random.default_rng(1).normal(1.0, 0.5, size=B).astype(np.float32)
    params = [t.requires_grad_(True) for _, t in m.trainable_variables()]
    alone = []
    for step in (0, 1):
        m.dropout_counter().fill_(step)
        loss = m._loss(d, y, training=True)
        alone.append((loss.detach(), torch.autograd.grad(loss, params)))
    assert not torch.equal(alone[0][0], alone[1][0])
    m.dropout_counter().fill_(0)
    loss_a = m._loss(d, y, training=True)
    loss_b = m._loss(d, y, training=True)
    got_b = torch.autograd.grad(loss_b, params)
    got_a = torch.autograd.grad(loss_a, params)
    for what, loss, got, (loss0, want) in (("A", loss_a, got_a, alone[0]), ("B", loss_b, got_b, alone[1])):
        assert torch.equal(loss.detach(), loss0), what
        for (name, _), g_, g0 in zip(m.trainable_variables(), got, want):
            close(g_, g0, 2e-4, f"pass {what}: grad {name}")
