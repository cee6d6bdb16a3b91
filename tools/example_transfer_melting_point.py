"""The reference's transfer trainer (train_melting_point_transfer.py main(), :150-260) on this package: train a small
viscosity model, save it, cut it at mix_cat_an and put the melting-point head on it (build_transfer_model), stage 1
with the base frozen, stage 2 with the last two message-passing steps unfrozen, Huber loss, early stopping, R2 / MAE in
kelvin from the device records (metrics with scale = the targets' std, offset = their mean).
Data are synthetic (ionic_mpnn_amd.synthetic) with targets that are known functions of the graphs - the point is the
plumbing, not chemistry.
    python tools/example_transfer_melting_point.py [--records 600] [--epochs 30]"""
import argparse
import json
import sys
import tempfile
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from ionic_mpnn_amd import build_model, data, synthetic  # noqa: E402
from ionic_mpnn_amd.model import build_transfer_model  # noqa: E402
from ionic_mpnn_amd.train import Adam, EarlyStopping, Huber, MeanAbsoluteError, R2Score  # noqa: E402

UNFREEZE_KEYS = ["cat_bmm_2", "cat_bmm_3", "an_bmm_2", "an_bmm_3", "gated_update_2", "gated_update_3",
                 "gated_update_6", "gated_update_7", "mix_cat_an"]                     # :214-220


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=600)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--seed", type=int, default=42)
    a = ap.parse_args()
    recs, vocab = synthetic.make_id_records(a.records, seed=a.seed, min_atoms=4, max_atoms=24, atom_vocab=30, bond_vocab=6)
    for r in recs:
        n_c, n_a = r["cation"]["num_atoms"], r["anion"]["num_atoms"]
        r["log_eta"] = 0.08 * n_c + 0.05 * n_a + 0.02 * sum(r["cation"]["atom_ids"]) / n_c + 300.0 / r["T"]
        r["mp"] = 0.1 * n_c - 0.07 * n_a + 0.03 * sum(r["anion"]["atom_ids"]) / n_a   # the "melting point"
    ds = data.ResidentIonPairDataset(recs, vocab)
    idx = np.random.RandomState(a.seed).permutation(len(ds))
    n_tr, n_dev = int(0.8 * len(ds)), int(0.1 * len(ds))
    parts = {"train": idx[:n_tr], "dev": idx[n_tr:n_tr + n_dev], "test": idx[n_tr + n_dev:]}
    x = {k: ds.build_inputs(v.tolist()) for k, v in parts.items()}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = str(Path(tmp) / "viscosity_final.keras")
        base = build_model(ds.atom_vocab_size, ds.bond_vocab_size)                     # 4 steps: gated_update_0..7
        base.compile(Adam(1e-3, clipnorm=1.0))
        y_v = np.asarray(ds.log_eta, np.float32)
        base.fit(x["train"], y_v[parts["train"]], validation_data=(x["dev"], y_v[parts["dev"]]), epochs=a.epochs,
                 batch_size=32, seed=a.seed)
        base.save(path)                                                                # train_viscosity.py:354
        model = build_transfer_model(path)                                             # :73-106
    y = np.asarray([r["mp"] for r in recs], np.float32)
    mean, std = y[parts["train"]].mean(), y[parts["train"]].std()
    ys = (y - mean) / std                                                              # :176-181
    cb = lambda: [EarlyStopping(patience=50, restore_best_weights=True)]
    for layer in model.layers:                                                         # stage 1, :189-205
        if not layer.name.startswith("mp_") and layer.name != "melting_point":
            layer.trainable = False
    kelvin = lambda: [MeanAbsoluteError(scale=float(std), offset=float(mean)), R2Score(scale=float(std), offset=float(mean))]
    model.compile(optimizer=Adam(1e-3), loss=Huber(delta=1.0), metrics=kelvin())
    h1 = model.fit(x["train"], ys[parts["train"]], validation_data=(x["dev"], ys[parts["dev"]]), epochs=a.epochs,
                   batch_size=32, callbacks=cb(), seed=a.seed)
    for layer in model.layers:                                                         # stage 2, :222-238
        if any(k in layer.name for k in UNFREEZE_KEYS):
            layer.trainable = True
    model.compile(optimizer=Adam(1e-4), loss=Huber(delta=1.0), metrics=kelvin())
    h2 = model.fit(x["train"], ys[parts["train"]], validation_data=(x["dev"], ys[parts["dev"]]), epochs=a.epochs,
                   batch_size=32, callbacks=cb(), seed=a.seed)
    out["stage1_val_loss"] = [h1.history["val_loss"][0], min(h1.history["val_loss"])]
    out["stage2_val_loss"] = [h2.history["val_loss"][0], min(h2.history["val_loss"])]
    out["stage2_trained_variables"] = len(model.trainable_variables())
    for name, ids in parts.items():
        res = model.evaluate(x[name], ys[ids], batch_size=4096, return_dict=True)   # "loss" in Huber units, the rest in K
        print(name, res)
        out[f"{name}_r2"], out[f"{name}_mae"] = res["r2"], res["mae"]
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
