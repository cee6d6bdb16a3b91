"""GatedUpdate dropout, host side: the numpy Philox4x32-10 the GPU tests compare the kernels' masks
against, the layer-word packing, rate validation and the configs that carry the rate."""
import numpy as np
import pytest
import torch

from ionic_mpnn_amd import layers as L, model as MM, ops

from philox_ref import M32, philox4x32_10, reference_mask  # noqa: F401  (the GPU tests import the mask from here)

CPU = torch.device("cpu")


def test_philox_known_answer():
    # Random123's kat_vectors (philox4x32_10, counter = key = 0); rocRAND's engine gives the same words
    got = philox4x32_10(np.zeros(4, np.uint32), np.zeros(2, np.uint32))
    assert [int(v) for v in got] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


def test_reference_mask_rate_and_scale():
    m = reference_mask(1234567, 3, 5, 0.25, 400, 32)
    assert set(np.unique(m)) <= {0.0, np.float32(1.0) / np.float32(0.75)}
    keep = (m > 0).mean()
    assert abs(keep - 0.75) < 5 * np.sqrt(0.75 * 0.25 / m.size)
    assert np.all(reference_mask(1234567, 3, 5, 0.0, 10, 8) == 1.0)


def test_layer_word_packing():
    assert ops.dropout_layer_word(0) == 0
    assert ops.dropout_layer_word(5) == 5
    assert ops.dropout_layer_word(7, rank=3) == 7 | (3 << 16)
    for bad in ((1 << 16, 0), (-1, 0), (0, -1), (0, 1 << 15)):
        with pytest.raises(ValueError):
            ops.dropout_layer_word(*bad)


@pytest.mark.parametrize("rate", [-0.1, 1.0, 1.5, float("nan"), 1.0 - 1e-9])
def test_rates_outside_zero_one_raise(rate):
    with pytest.raises(ValueError):
        ops.check_dropout_rate(rate)
    with pytest.raises(ValueError):
        L.GatedUpdate(16, dropout_rate=rate, device=CPU)
    with pytest.raises(ValueError):
        MM.build_model(9, 5, atom_dim=16, num_steps=1, device=CPU, dropout_rate=rate)


def test_rate_zero_draws_no_seed():
    torch.manual_seed(3)
    a = torch.rand(1)
    torch.manual_seed(3)
    g = L.GatedUpdate(16, device=CPU)
    assert g.dropout_seed is None and torch.equal(torch.rand(1), a)


def test_gated_update_config_round_trip():
    L.reset_uids()
    torch.manual_seed(11)
    g = L.GatedUpdate(32, dropout_rate=0.3, device=CPU)
    torch.manual_seed(11)
    assert L.GatedUpdate(32, dropout_rate=0.3, device=CPU).dropout_seed == g.dropout_seed  # torch.manual_seed decides
    cfg = g.get_config()
    assert cfg["dropout_rate"] == 0.3 and cfg["dropout_seed"] == g.dropout_seed
    again = L.GatedUpdate.from_config(cfg | {"device": CPU})
    assert again.get_config() == cfg
    assert L.GatedUpdate(8, dropout_rate=0.5, dropout_seed=99, device=CPU).dropout_seed == 99


def test_model_config_round_trip_and_old_files(tmp_path):
    m = MM.build_model(9, 5, atom_dim=16, bond_dim=4, fp_size=8, mixing_size=6, num_steps=2, device=CPU,
                       dropout_rate=0.2, dropout_seed=77)
    cfg = m.get_config()
    assert cfg["dropout_rate"] == 0.2 and cfg["dropout_seed"] == 77
    for p in ("cat", "an"):
        assert all(u.dropout_rate == 0.2 and u.dropout_seed == 77 for u in m.branches[p]["update"])
    m2 = MM.MPNNModel.from_config(cfg, device=CPU)
    assert (m2.dropout_rate, m2.dropout_seed) == (0.2, 77)
    path = tmp_path / "m.keras"
    m.save(str(path))
    cfg_file, _ = MM.MPNNModel.load_weight_file(str(path))
    assert cfg_file["dropout_rate"] == 0.2
    m3 = MM.load_model(str(path), device=CPU)
    assert (m3.dropout_rate, m3.dropout_seed) == (0.2, 77)
    old = {k: v for k, v in cfg.items() if k not in ("dropout_rate", "dropout_seed")}   # written before the keyword
    m4 = MM.MPNNModel.from_config(old, device=CPU)
    assert m4.dropout_rate == 0.0 and m4.dropout_seed is None
    mp = MM.build_melting_point_model(9, 5, atom_dim=8, num_steps=1, device=CPU, dropout_rate=0.1, dropout_seed=5)
    assert mp.get_config()["dropout_rate"] == 0.1
