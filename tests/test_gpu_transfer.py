"""Transfer learning on the GPU: the fused head (impnn_transfer_head*) against the fp64 reference of
tests/transfer_ref.py, its Philox Dropout mask, whole-model gradients under the freezing patterns of
train_melting_point_transfer.py, frozen variables staying bit for bit, the encoder graph ending where training ends,
graphed against eager fit, EarlyStopping, save / load.  Tolerances: conftest's assert_close at 1e-5 for forward
values, the 2e-4 scale tolerance of tests/test_gpu_train.py::close for gradients and loss histories."""
import json

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import autograd, layers as L, model as MM, ops, synthetic, train, weights
from conftest import assert_close

import transfer_ref as R
from test_dropout_host import reference_mask
from test_gpu_train import close

pytestmark = pytest.mark.gpu
DEV = "cuda"
UNFREEZE_KEYS = ["cat_bmm_2", "cat_bmm_3", "an_bmm_2", "an_bmm_3", "gated_update_2", "gated_update_3",
                 "gated_update_6", "gated_update_7", "mix_cat_an"]
SEED = 0x5EED_0BAD_CAFE


def make_transfer(tmp_path, D=32, S=4, K=8, F=32, Mx=20, Va=synthetic.DEFAULT_VA, Vb=synthetic.DEFAULT_VB, seed=1):
    """A viscosity model with perturbed weights, saved, cut and given the head; head variables randomised too."""
    L.reset_uids()
    L.set_init_seed(seed)   # (the head's initial kernels come from the package's init stream: same model every call)
    v = MM.build_model(Va, Vb, atom_dim=D, bond_dim=K, fp_size=F, mixing_size=Mx, num_steps=S, device=DEV)
    v.load_weights(weights.init_weights("viscosity", Va, Vb, atom_dim=D, bond_dim=K, fp_size=F, mixing_size=Mx,
                                        num_steps=S, seed=seed, perturb=True))
    path = tmp_path / "viscosity_final.keras"
    v.save(str(path))
    t = MM.build_transfer_model(str(path), device=DEV, dropout_seed=SEED)
    rng = np.random.default_rng(seed + 100)
    head = {n: a for n, a in t.state_dict().items() if n.startswith("mp_") or n.startswith("melting_point")}
    for n, a in head.items():
        if n.endswith("kernel"):
            head[n] = (a * 1.5).astype(np.float32)
        elif n.endswith("moving_variance"):
            head[n] = rng.uniform(0.5, 2.0, size=a.shape).astype(np.float32)
        elif n.endswith("gamma"):
            head[n] = rng.uniform(0.5, 1.5, size=a.shape).astype(np.float32)
        else:
            head[n] = rng.normal(0.0, 0.2, size=a.shape).astype(np.float32)
    t.load_weights({**t.state_dict(), **head})
    return t


def stage1(t):
    for layer in t.layers:
        layer.trainable = layer.name.startswith("mp_") or layer.name == "melting_point"


def stage2(t):
    stage1(t)
    for layer in t.layers:
        if any(k in layer.name for k in UNFREEZE_KEYS):
            layer.trainable = True


def everything(t):
    for layer in t.layers:
        layer.trainable = True


def mixed(t):
    """A frozen layer inside the trained range: cat_bmm_3 trains, gated_update_3 does not; one head layer frozen."""
    stage1(t)
    for name in ("cat_bmm_3", "an_bmm_1", "gated_update_5", "gated_update_7", "dense_1"):
        t.get_layer(name).trainable = True
    t.get_layer("mp_dense_2").trainable = False


PATTERNS = {"stage1": stage1, "stage2": stage2, "everything": everything, "mixed": mixed}


def head_mask(step, B):
    return reference_mask(SEED, step, ops.dropout_layer_word(L.Dropout.LAYER_ID), 0.3, B, 128)


@pytest.mark.parametrize("B", [1, 5, 32, 33, 300, 4096])
def test_head_forward_against_fp64(tmp_path, B):
    t = make_transfer(tmp_path, S=1)
    t.compile(train.Adam(1e-3), loss=train.Huber(delta=1.0))
    rng = np.random.default_rng(B)
    pc = torch.tensor(rng.normal(0.0, 1.0, size=(B, 32)), dtype=torch.float32, device=DEV)
    pa = torch.tensor(rng.normal(0.0, 1.0, size=(B, 32)), dtype=torch.float32, device=DEV)
    y = torch.tensor(rng.normal(0.0, 1.0, size=(B, 1)), dtype=torch.float32, device=DEV)
    w = {k: torch.tensor(v, dtype=R.DT) for k, v in t.state_dict().items()}
    with torch.no_grad():
        out = t.head(pc, pa)
        again = t.head(pc, pa)
    ref, _, _ = R.head(w, pc.cpu().double(), pa.cpu().double())
    assert torch.equal(out, again)
    assert_close(out.cpu().numpy().reshape(-1), ref.numpy(), 1e-5, f"inference head B={B}")
    # three training passes: batch statistics, the mask of steps 0..2, the moving statistics move
    ws = torch.zeros(1024, dtype=torch.float32, device=DEV)
    losses = []
    for step in range(3):
        snap = torch.tensor([step], dtype=torch.int64, device=DEV)
        cfg = t._transfer_cfg(True, snap)
        before = t.mp_bn_1.moving_mean.clone(), t.mp_bn_1.moving_variance.clone()
        with torch.no_grad():
            loss = autograd.TransferHeadLoss.apply(cfg, ws, pc, pa, y, *t._head_tensors())
            t.mp_bn_1.moving_mean.copy_(before[0]); t.mp_bn_1.moving_variance.copy_(before[1])
            loss2 = autograd.TransferHeadLoss.apply(cfg, ws, pc, pa, y, *t._head_tensors())
        assert torch.equal(loss, loss2), "two runs on the same inputs must agree bitwise"
        pred, mm, mv = R.head(w, pc.cpu().double(), pa.cpu().double(), True, head_mask(step, B))
        e = pred - y.cpu().double().reshape(-1)
        want = R.huber(e, 1.0).mean() + 1e-4 * ((w["cat_fp/kernel"] ** 2).sum() + (w["an_fp/kernel"] ** 2).sum())
        print(f"B={B} step={step} loss {float(loss):.8f} ref {float(want):.8f}")
        assert_close(np.array([float(loss)]), np.array([float(want)]), 1e-5, f"training loss B={B} step {step}")
        w["mp_bn_1/moving_mean"], w["mp_bn_1/moving_variance"] = mm, mv
        losses.append(float(loss))
    assert_close(t.mp_bn_1.moving_mean.cpu().numpy(), w["mp_bn_1/moving_mean"].numpy(), 1e-5, "moving mean")
    assert_close(t.mp_bn_1.moving_variance.cpu().numpy(), w["mp_bn_1/moving_variance"].numpy(), 1e-5, "moving variance")
    if B > 1:
        assert len(set(losses)) == 3, "every step draws a fresh mask"


def test_head_dropout_mask_is_the_numpy_philox(tmp_path):
    t = make_transfer(tmp_path, S=2)
    t.compile(train.Adam(1e-3), loss="huber")
    lw = ops.dropout_layer_word(L.Dropout.LAYER_ID)
    assert all(lw != ops.dropout_layer_word(i) for i in range(2 * t.num_steps))
    B = 37
    d = ops.Dropout(0.3, SEED, lw, torch.tensor([5], dtype=torch.int64, device=DEV))
    assert np.array_equal(ops.dropout_mask(d, B, 128).cpu().numpy(), head_mask(5, B))
    # the head kernels drop exactly those units: the fp64 model with the step-5 mask gives the fused loss, the
    # step-6 mask does not
    inp = t._to_device(synthetic.make_batch(B, seed=4))
    y = torch.zeros(B, 1, device=DEV)
    t.dropout_counter().fill_(5)
    with torch.no_grad():
        fused = t._loss(inp, y, training=True)
    assert int(t.dropout_counter().item()) == 6
    w = {k: torch.tensor(v, dtype=R.DT) for k, v in t.state_dict().items()}
    cpu = {k: v.cpu() for k, v in inp.items()}
    want, _, _, _ = R.loss(w, cpu, np.zeros(B), True, head_mask(5, B))
    assert_close(np.array([float(fused)]), np.array([float(want)]), 1e-5, "loss with the step-5 mask")
    wrong, _, _, _ = R.loss(w, cpu, np.zeros(B), True, head_mask(6, B))
    assert abs(float(wrong) - float(want)) > 1e-4 * abs(float(want))


@pytest.mark.parametrize("D", [32, 128])
@pytest.mark.parametrize("pattern", ["stage1", "stage2", "everything", "mixed"])
def test_whole_model_gradients_against_fp64(tmp_path, pattern, D):
    B = 24
    t = make_transfer(tmp_path, D=D, seed=3)
    PATTERNS[pattern](t)
    t.compile(train.Adam(1e-3), loss=train.Huber(delta=1.0))
    inp = synthetic.make_batch(B, seed=7)
    w = R.leaves(t.state_dict())
    mask = head_mask(9, B)
    # targets on both Huber branches in the reference itself, none within 1e-3 of |e| = delta
    with torch.no_grad():
        pred0, _, _ = R.head(w, *R.pooled(w, inp), True, mask)
    off = np.where(np.arange(B) % 2 == 0, 0.4, 2.5) * np.where(np.arange(B) % 3 == 0, -1.0, 1.0)
    y = (pred0.numpy() - off).astype(np.float32)
    lo, e, _, _ = R.loss(w, inp, y, True, mask)
    ae = e.detach().abs().numpy()
    assert (ae <= 1.0).any() and (ae > 1.0).any() and np.all(np.abs(ae - 1.0) > 1e-3)
    lo.backward()
    t.dropout_counter().fill_(9)
    before = {n: a.copy() for n, a in t.state_dict().items()}
    loss = t._loss(t._to_device(inp), y, training=True)
    loss.backward()
    t.join_training_streams()
    close(loss, lo, 1e-5, "loss")
    trained = dict(t.trainable_variables())
    assert len(t.optimizer._vars) == len(trained)
    for name, tensor in t._named_tensors().items():
        if name in trained:
            close(tensor.grad, w[name].grad, 2e-4, f"{pattern} D={D}: grad {name}")
        else:
            assert tensor.grad is None and not tensor.requires_grad, name
            assert np.array_equal(tensor.detach().cpu().numpy(), before[name]), name


def _graph_nodes(loss):
    seen, stack, names = set(), [loss.grad_fn], []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        stack += [f for f, _ in fn.next_functions]
    return names


def test_encoder_graph_ends_where_training_ends(tmp_path):
    t = make_transfer(tmp_path)
    B = 32
    inp = t._to_device(synthetic.make_batch(B, seed=2))
    y = np.zeros(B, np.float32)
    stage1(t)
    t.compile(train.Adam(1e-3), loss=train.Huber())
    loss = t._loss(inp, y, training=True)
    names = _graph_nodes(loss)
    assert not any(k in n for n in names for k in ("MessagePassingStep", "EmbedGather", "BondTypeMatricesAll")), names
    # the pooled vectors of the pass are inference's, bit for bit
    with torch.no_grad():
        pc, pa = t.encode_pooled(inp)
        cfg = t._transfer_cfg(True, torch.tensor([0], dtype=torch.int64, device=DEV))
        t.dropout_counter().fill_(0)
        mm, mv = t.mp_bn_1.moving_mean.clone(), t.mp_bn_1.moving_variance.clone()
        a = t._loss(inp, y, training=True)
        t.mp_bn_1.moving_mean.copy_(mm); t.mp_bn_1.moving_variance.copy_(mv)
        b = autograd.TransferHeadLoss.apply(cfg, t._loss_ws, pc, pa, torch.zeros(B, 1, device=DEV), *t._head_tensors())
    assert torch.equal(a, b)
    stage2(t)
    t.compile(train.Adam(1e-4), loss=train.Huber())
    names = _graph_nodes(t._loss(inp, y, training=True))
    assert sum("MessagePassingStep" in n for n in names) == 4, names   # steps 2 and 3 of each ion
    assert sum("BondTypeMatricesAll" in n for n in names) == 1 and not any("EmbedGather" in n for n in names), names
    assert t._first_trained_step("cat") == 2 and t._first_trained_step("an") == 2


@pytest.mark.parametrize("pattern", ["stage1", "stage2"])
def test_frozen_means_frozen_eager_and_graphed(tmp_path, pattern):
    t = make_transfer(tmp_path)
    PATTERNS[pattern](t)
    t.compile(train.Adam(1e-3 if pattern == "stage1" else 1e-4), loss=train.Huber(delta=1.0))
    n_train = len(t.trainable_variables())
    assert n_train == (10 if pattern == "stage1" else 46) and len(t.optimizer._vars) == n_train
    B = 32
    inp = t._to_device(synthetic.make_batch(B, seed=5))
    y = np.random.default_rng(5).normal(0.0, 1.0, size=B).astype(np.float32)
    before = {n: a.copy() for n, a in t.state_dict().items()}
    for _ in range(5):
        t.train_on_batch(inp, y)
    step = train.GraphedTrainStep(t, inp, y)
    for _ in range(5):
        step(inp, y)
    torch.cuda.synchronize()
    after = t.state_dict()
    trained = {n for n, _ in t.trainable_variables()}
    for n, a in before.items():
        if n in trained or "moving" in n:
            assert not np.array_equal(after[n], a), f"{n} did not move"
        else:
            assert np.array_equal(after[n], a), f"frozen {n} changed"
    assert int(t.dropout_counter().item()) == 10 and t.optimizer.iterations == 10


def _data(n, seed):
    x = synthetic.make_batch(n, seed=seed)
    y = np.random.default_rng(seed).normal(0.0, 1.0, size=n).astype(np.float32)
    return x, y


@pytest.mark.parametrize("pattern", ["stage1", "stage2"])
def test_graphed_fit_follows_eager_fit(tmp_path, pattern):
    x, y = _data(100, 11)   # 3 full batches of 32 and a last one of 4
    hist, state = {}, {}
    for graph in (False, True):
        t = make_transfer(tmp_path)
        PATTERNS[pattern](t)
        t.compile(train.Adam(1e-3), loss=train.Huber(delta=1.0))
        h = t.fit(x, y, validation_data=(x, y), epochs=3, batch_size=32, seed=3, graph=graph)
        hist[graph], state[graph] = h.history, t.state_dict()
        assert int(t.dropout_counter().item()) == 12, "one fresh mask per step, replayed or not"
    print(pattern, "eager", hist[False], "graphed", hist[True])
    for k in ("loss", "val_loss"):
        close(np.array(hist[True][k]), np.array(hist[False][k]), 2e-4, f"{pattern} {k}")
    for n in ("mp_bn_1/moving_mean", "mp_bn_1/moving_variance"):
        close(state[True][n], state[False][n], 2e-4, n)
    assert len(set(hist[True]["loss"])) == 3


def test_early_stopping_restores_moving_statistics(tmp_path):
    x, y = _data(64, 13)
    t = make_transfer(tmp_path)
    stage1(t)
    t.compile(train.Adam(1e-3), loss="huber")
    snaps = []

    class Snap(train.Callback):
        def on_epoch_end(self, epoch, logs=None):
            snaps.append((logs["val_loss"], self.model.state_dict()))

    es = train.EarlyStopping(patience=100, restore_best_weights=True)
    t.fit(x, y, validation_data=(x, y), epochs=4, batch_size=32, seed=1, callbacks=[es, Snap()])
    best = min(range(len(snaps)), key=lambda i: snaps[i][0])
    assert es.best_epoch == best
    for n, a in snaps[best][1].items():
        assert np.array_equal(t.state_dict()[n], a), n
    if best != len(snaps) - 1:
        assert not np.array_equal(snaps[-1][1]["mp_bn_1/moving_mean"], t.state_dict()["mp_bn_1/moving_mean"])


def test_save_load_round_trip_and_old_viscosity_files(tmp_path):
    t = make_transfer(tmp_path)
    stage2(t)
    t.compile(train.Adam(1e-4), loss=train.Huber())
    x, y = _data(40, 17)
    t.fit(x, y, epochs=1, batch_size=32, seed=1)
    path = tmp_path / "transfer.keras"
    t.save(str(path))
    back = MM.load_model(str(path), device=DEV)
    assert [(l.name, l.trainable) for l in back.layers] == [(l.name, l.trainable) for l in t.layers]
    assert np.array_equal(back.predict(x), t.predict(x))
    back.compile(train.Adam(1e-4), loss=train.Huber())
    assert back.evaluate(x, y) == t.evaluate(x, y)
    # a viscosity file written before this change: no layer_trainable key in its config
    cfg, w = MM.MPNNModel.load_weight_file(str(tmp_path / "viscosity_final.keras"))
    old = {k: v for k, v in cfg.items() if k != "layer_trainable"}
    old_path = tmp_path / "old.keras"
    with open(old_path, "wb") as f:
        np.savez(f, __config__=np.frombuffer(json.dumps(old).encode(), dtype=np.uint8), **w)
    v = MM.load_model(str(old_path), device=DEV)
    assert all(l.trainable for l in v.layers)
    t2 = MM.build_transfer_model(str(old_path), device=DEV, dropout_seed=1)
    assert t2.predict(x).shape == (40, 1)


def test_nothing_moves_for_existing_models():
    for m in (MM.build_model(synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, device=DEV),
              MM.build_melting_point_model(synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, atom_dim=8, num_steps=2, device=DEV)):
        m.compile()
        assert [n for n, _ in m.trainable_variables()] == list(m._named_tensors())
        assert [id(v) for v in m.optimizer._vars] == [id(v) for v in m._named_tensors().values()]
        assert [n for n, _ in m.variables()] == [n for n, _ in m.trainable_variables()]
    m = MM.build_model(synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, num_steps=2, device=DEV)
    m.compile(train.Adam(1e-3, clipnorm=1.0), loss=train.Huber(delta=0.5))   # the layer-by-layer loss route
    x, y = _data(32, 19)
    l0 = float(m.train_on_batch(x, y))
    assert np.isfinite(l0) and float(m.train_on_batch(x, y)) != l0
