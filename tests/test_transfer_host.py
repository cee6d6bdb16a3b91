"""Transfer learning, host side: Huber, the configs of the new layers and of per-layer ``trainable``, the freezing
rules of trainable_variables(), and the status codes of the impnn_transfer_head* entries for bad arguments."""
import ctypes as C

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, layers as L, model as MM, train

CPU = torch.device("cpu")
UNFREEZE_KEYS = ["cat_bmm_2", "cat_bmm_3", "an_bmm_2", "an_bmm_3", "gated_update_2", "gated_update_3",
                 "gated_update_6", "gated_update_7", "mix_cat_an"]


def test_huber_values_and_derivative():
    h = train.Huber(delta=1.5)
    y = torch.zeros(6, 1, dtype=torch.float64)
    p = torch.tensor([[0.5], [-1.0], [1.5], [-1.5], [2.0], [-4.0]], dtype=torch.float64, requires_grad=True)
    per = [0.125, 0.5, 1.125, 1.125, 1.5 * (2.0 - 0.75), 1.5 * (4.0 - 0.75)]
    v = h(y, p)
    assert abs(float(v.detach()) - sum(per) / 6) < 1e-15
    v.backward()
    assert np.allclose(p.grad.numpy().reshape(-1) * 6, [0.5, -1.0, 1.5, -1.5, 1.5, -1.5], atol=1e-15)
    assert h.get_config()["delta"] == 1.5
    with pytest.raises(ValueError):
        train.Huber(0.0)


def test_new_layer_configs_round_trip():
    bn = L.BatchNormalization(name="mp_bn_1", device=CPU)
    assert (bn.momentum, bn.epsilon) == (0.99, 1e-3)
    again = L.BatchNormalization.from_config(bn.get_config())
    assert again.get_config() == bn.get_config()
    bn.build((None, 16)); again.trainable = False
    assert bn.weight_names() == ["gamma", "beta", "moving_mean", "moving_variance"]
    assert len(bn.trainable_weights) == 2 and again.trainable_weights == []
    dp = L.Dropout(0.3, seed=11, name="mp_dropout", device=CPU)
    cfg = dp.get_config()
    assert cfg["rate"] == 0.3 and cfg["seed"] == 11
    assert L.Dropout.from_config(cfg).get_config() == cfg
    x = torch.ones(3, 4)
    assert dp(x, training=False) is x
    with pytest.raises(ValueError):
        L.Dropout(1.0, device=CPU)


def test_batch_normalization_layer_semantics():
    bn = L.BatchNormalization(device=CPU)
    x = torch.tensor(np.random.default_rng(0).normal(2.0, 3.0, size=(10, 4)), dtype=torch.float32)
    out = bn(x, training=True)
    mean, var = x.mean(0), x.var(0, unbiased=False)
    assert torch.allclose(out, (x - mean) / torch.sqrt(var + 1e-3), atol=1e-6)
    assert torch.allclose(bn.moving_mean, 0.01 * mean, atol=1e-6)
    assert torch.allclose(bn.moving_variance, 0.99 + 0.01 * var, atol=1e-6)
    inf = bn(x, training=False)
    assert torch.allclose(inf, (x - bn.moving_mean) / torch.sqrt(bn.moving_variance + 1e-3), atol=1e-6)


def _transfer(tmp_path, **kw):
    L.reset_uids()
    v = MM.build_model(9, 5, device=CPU, **kw)
    path = tmp_path / "viscosity_final.keras"
    v.save(str(path))
    return v, MM.build_transfer_model(str(path), device=CPU, dropout_seed=5)


def test_transfer_model_layers_and_stage_variable_counts(tmp_path):
    v, t = _transfer(tmp_path)
    names = [l.name for l in t.layers]
    base = [l.name for l in v.layers]
    assert names[:base.index("mix_cat_an") + 1] == base[:base.index("mix_cat_an") + 1]
    assert names[-6:] == ["mp_dense_1", "mp_bn_1", "mp_dense_2", "mp_dropout", "mp_dense_3", "melting_point"]
    for n, a in v.state_dict().items():
        if not n.startswith("visc_params"):
            assert np.array_equal(t.state_dict()[n], a), n
    assert len(t.variables()) == len(t.trainable_variables()) + 2
    for layer in t.layers:                                     # stage 1
        if not layer.name.startswith("mp_") and layer.name != "melting_point":
            layer.trainable = False
    assert [n for n, _ in t.trainable_variables()] == [
        "mp_dense_1/kernel", "mp_dense_1/bias", "mp_bn_1/gamma", "mp_bn_1/beta", "mp_dense_2/kernel", "mp_dense_2/bias",
        "mp_dense_3/kernel", "mp_dense_3/bias", "melting_point/kernel", "melting_point/bias"]
    for layer in t.layers:                                     # stage 2
        if any(k in layer.name for k in UNFREEZE_KEYS):
            layer.trainable = True
    tv = [n for n, _ in t.trainable_variables()]
    assert len(tv) == 46                                       # 10 head + 4 bond_transform + 4 x 8 GatedUpdate
    order = [n for n, _ in t.variables()]
    assert tv == [n for n in order if n in set(tv)]
    assert all(n.split("/")[0] in ("cat_bmm_2", "cat_bmm_3", "an_bmm_2", "an_bmm_3", "cat_gu_2", "cat_gu_3", "an_gu_2",
                                   "an_gu_3") for n in tv[:36])


def test_trainable_flags_and_moving_statistics_round_trip(tmp_path):
    _, t = _transfer(tmp_path, atom_dim=16, bond_dim=4, fp_size=8, mixing_size=6, num_steps=2)
    t.get_layer("cat_bmm_1").trainable = False
    t.get_layer("mp_bn_1").trainable = False
    with torch.no_grad():
        t.mp_bn_1.moving_mean.add_(0.25)
    cfg = t.get_config()
    assert cfg["kind"] == "transfer" and cfg["layer_trainable"]["cat_bmm_1"] is False
    assert [c["class_name"] for c in cfg["layers"]][-6:] == ["Dense", "BatchNormalization", "Dense", "Dropout", "Dense",
                                                             "Dense"]
    again = MM.MPNNModel.from_config(cfg, device=CPU)
    assert [l.trainable for l in again.layers] == [l.trainable for l in t.layers]
    assert again.mp_dropout.seed == 5 and again.mp_dropout.rate == 0.3
    path = tmp_path / "transfer.keras"
    t.save(str(path))
    back = MM.load_model(str(path), device=CPU)
    assert [(l.name, l.trainable) for l in back.layers] == [(l.name, l.trainable) for l in t.layers]
    for n, a in t.state_dict().items():
        assert np.array_equal(back.state_dict()[n], a), n
    assert "mp_bn_1/moving_mean" in back.state_dict()


def test_default_models_list_every_variable(tmp_path):
    for m in (MM.build_model(9, 5, num_steps=2, device=CPU), MM.build_melting_point_model(9, 5, atom_dim=8, num_steps=1, device=CPU)):
        assert [n for n, _ in m.trainable_variables()] == list(m._named_tensors())
        assert [n for n, _ in m.variables()] == [n for n, _ in m.trainable_variables()]
        assert "layer_trainable" in m.get_config()
    old = {k: v for k, v in MM.build_model(9, 5, num_steps=1, device=CPU).get_config().items()
           if k not in ("layer_trainable", "layers")}          # a file written before layers could be frozen
    assert all(l.trainable for l in MM.MPNNModel.from_config(old, device=CPU).layers)


def test_compile_rejects_unknown_losses_and_all_frozen_models():
    m = MM.build_model(9, 5, atom_dim=8, num_steps=1, device=CPU)
    with pytest.raises(ValueError):
        m.compile(loss="mae")
    for layer in m.layers:
        layer.trainable = False
    with pytest.raises(ValueError):
        m.compile(loss="mse")


def test_transfer_head_entries_return_status_codes():
    lib = _lib.load()
    assert lib.impnn_transfer_head_saved_floats(0, 32, 20) == -1
    assert lib.impnn_transfer_head_saved_floats(32, 32, 20) == 32 * (2 * 32 + 3 * 20 + 2 * 256 + 128 + 64 + 1) + 512
    assert lib.impnn_transfer_head_bwd_workspace_floats(32, 32, 20) > 0
    assert lib.impnn_transfer_head_loss_workspace_floats(33) == 5 + 4
    one = C.c_void_p(64)  # a non-null pointer that no call below dereferences
    table = (C.c_void_p * 18)(*[64] * 18)
    lam = (C.c_float * 18)(*[0.0] * 18)
    BAD, UNS, WSP = -1, _lib.IMPNN_E_UNSUPPORTED, -4
    assert lib.impnn_transfer_head(one, one, table, one, one, 1e-3, one, -1, 32, 32, 20, None) == BAD
    assert lib.impnn_transfer_head(None, one, table, one, one, 1e-3, one, 4, 32, 32, 20, None) == BAD
    assert lib.impnn_transfer_head(one, one, table, one, one, 1e-3, one, 0, 32, 32, 20, None) == 0
    assert lib.impnn_transfer_head(one, one, table, one, one, 1e-3, one, 4, 129, 32, 20, None) == UNS
    assert lib.impnn_transfer_head(one, one, table, one, one, 1e-3, one, 4, 32, 65, 20, None) == UNS
    assert b"transfer_head" in lib.impnn_last_error_string()

    def fwd(rate=0.0, step=None, B=4, kind=1, delta=1.0, y=one, saved=one, nsaved=1 << 30, nws=64, F=32, bn=1):
        return lib.impnn_transfer_head_loss(one, one, table, lam, one, one, 0.99, 1e-3, bn, y, kind, delta, rate,
                                            C.c_uint64(1), step, 0, saved, nsaved, None, one, one, nws, B, 32, F, 20, None)
    assert fwd(rate=0.3, step=None) == BAD          # dropout without a step
    assert fwd(rate=1.0, step=one) == BAD
    assert fwd(B=0) == BAD and fwd(kind=2) == BAD and fwd(delta=0.0) == BAD and fwd(y=None) == BAD
    assert fwd(saved=None, bn=1) == BAD             # the batch statistics pass through the saved buffer
    assert fwd(nsaved=10) == WSP and fwd(nws=2) == WSP
    assert fwd(F=65) == UNS

    def bwd(rate=0.0, step=None, dpc=one, dpa=one, nsaved=1 << 30, nws=1 << 30, Mx=20, dw=table):
        return lib.impnn_transfer_head_loss_bwd(one, one, table, dw, lam, 1, one, 1, 1.0, one, rate, C.c_uint64(1), step,
                                                0, one, nsaved, one, nws, dpc, dpa, 4, 32, 32, Mx, None)
    assert bwd(rate=0.5) == BAD and bwd(dpa=None) == BAD and bwd(dw=None) == BAD
    assert bwd(nsaved=3) == WSP and bwd(nws=3) == WSP
    assert bwd(Mx=65) == UNS
