"""Cation x anion screening: MPNNModel.predict_grid against MPNNModel.predict on the explicitly expanded pair list
(the only inference entry before the grid existed), plus the grid kernel alone against the HBM write rate.  For the
transfer model: predict_grid with grid_head_mode "gathered" (self.head on gathered tiles of pairs) against "auto" (the
matrix-core grid, impnn_transfer_head_grid), plus that kernel alone against the f32 MFMA peak.

python tools/screen_bench.py [--quick] [--only viscosity|transfer]      -> one JSON line per configuration, appended to profiles/screen_bench.jsonl

Method: three alternating rounds (expanded, grid, expanded, grid, ...) after one warm-up of each, HIP events around each
call on the current stream plus a host synchronisation (both entries end with a device-to-host copy), median per side.
The expanded inputs are built once and stay on the device, so the baseline pays no host-to-device copy; predict_grid
gets host arrays of C + A molecules, as a caller would hand them over."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from ionic_mpnn_amd import model as MM, ops, synthetic, weights  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="the first configuration only")
ap.add_argument("--only", choices=("viscosity", "transfer"), help="one family of configurations")
ap.add_argument("--out", default=str(ROOT / "profiles" / "screen_bench.jsonl"))
args = ap.parse_args()
dev = torch.device("cuda:0")
Va, Vb = synthetic.DEFAULT_VA, synthetic.DEFAULT_VB
# (name, atom_dim, steps, C, A, nT, predict batch)
CONFIGS = [("config2 256x256x8", 32, 3, 256, 256, 8, 65536),
           ("config2 512x512x8", 32, 3, 512, 512, 8, 65536),
           ("D128 S6 256x256x8", 128, 6, 256, 256, 8, 16384)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def species(n, seed):
    b = synthetic.make_batch(n, seed=seed, with_temperature=False)
    return {k: b[f"cat_{k}"] for k in MM.ION_KEYS}, {k: b[f"an_{k}"] for k in MM.ION_KEYS}


lines = []
for name, D, S, C, A, nT, bs in [] if args.only == "transfer" else CONFIGS[:1] if args.quick else CONFIGS:
    m = MM.build_model(Va, Vb, atom_dim=D, num_steps=S, device=dev)
    m.load_weights(weights.init_weights("viscosity", Va, Vb, atom_dim=D, num_steps=S, seed=1, perturb=True))
    cat, _ = species(C, 1)
    _, an = species(A, 2)
    T = np.linspace(263.15, 393.15, nT).astype(np.float32)
    ci = torch.arange(C, device=dev).repeat_interleave(A * nT)
    ai = torch.arange(A, device=dev).repeat_interleave(nT).repeat(C)
    exp = {f"cat_{k}": torch.from_numpy(cat[k]).to(dev)[ci] for k in MM.ION_KEYS}
    exp.update({f"an_{k}": torch.from_numpy(an[k]).to(dev)[ai] for k in MM.ION_KEYS})
    exp["temperature"] = torch.from_numpy(T).to(dev).repeat(C * A)[:, None]
    run_exp = lambda: m.predict(exp, batch_size=bs)
    run_grid = lambda: m.predict_grid(cat, an, T)
    _, y_exp = timed(run_exp)
    _, y_grid = timed(run_grid)
    err = float(np.max(np.abs(y_exp.reshape(C, A, nT) - y_grid)) / np.max(np.abs(y_exp)))
    t_exp, t_grid = [], []
    for _ in range(3):
        t_exp.append(timed(run_exp)[0])
        t_grid.append(timed(run_grid)[0])
    # the grid launch alone: mixing rows resident, 20 launches between one event pair
    with torch.no_grad():
        pc, pa = m.encode_ions(cat, an)
        w = m._packed_head()
        mc = ops.head_ion_mix("viscosity", "cat", pc, w, m.fp_size, m.mixing_size)
        ma = ops.head_ion_mix("viscosity", "an", pa, w, m.fp_size, m.mixing_size)
        Td = torch.from_numpy(T).to(dev)
        launch = lambda: [ops.head_grid("viscosity", mc, ma, Td, w, m.fp_size, m.mixing_size) for _ in range(20)]
        timed(launch)
        k_ms = statistics.median(timed(launch)[0] for _ in range(3)) / 20
    ms_exp, ms_grid = statistics.median(t_exp), statistics.median(t_grid)
    line = {"config": name, "atom_dim": D, "steps": S, "C": C, "A": A, "nT": nT, "pairs": C * A * nT,
            "predict_expanded_ms": round(ms_exp, 3), "predict_grid_ms": round(ms_grid, 3),
            "speedup": round(ms_exp / ms_grid, 1), "rounds_expanded_ms": [round(t, 3) for t in t_exp],
            "rounds_grid_ms": [round(t, 3) for t in t_grid], "grid_kernel_us": round(k_ms * 1e3, 2),
            "grid_kernel_write_GBps": round(C * A * nT * 4 / (k_ms * 1e-3) / 1e9, 1), "max_rel_diff": err}
    print(json.dumps(line), flush=True)
    lines.append(line)
    del exp, m
    torch.cuda.empty_cache()

# ---- the transfer model: "gathered" against "auto", then the matrix-core grid kernel alone
# (name, atom_dim, steps, C, A)
TRANSFER_CONFIGS = [("transfer 256x256", 32, 3, 256, 256),
                    ("transfer 1024x1024", 32, 3, 1024, 1024),
                    ("transfer D128 S6 256x256", 128, 6, 256, 256)]
PAIR_FLOP = 2 * (256 * 128 + 128 * 64 + 64)  # executed per pair by the grid kernel
MFMA_F32_PEAK = 157.3e12


def build_transfer(D, S):
    import tempfile
    v = MM.build_model(Va, Vb, atom_dim=D, num_steps=S, device=dev)
    v.load_weights(weights.init_weights("viscosity", Va, Vb, atom_dim=D, num_steps=S, seed=1, perturb=True))
    with tempfile.TemporaryDirectory() as d:
        path = str(Path(d) / "viscosity_final.keras")
        v.save(path)
        return MM.build_transfer_model(path, device=dev)


for name, D, S, C, A in [] if args.only == "viscosity" else TRANSFER_CONFIGS[:1] if args.quick else TRANSFER_CONFIGS:
    t = build_transfer(D, S)
    cat, _ = species(C, 1)
    _, an = species(A, 2)

    def run(mode):
        t.grid_head_mode = mode
        return t.predict_grid(cat, an)

    _, y_g = timed(lambda: run("gathered"))
    _, y_a = timed(lambda: run("auto"))
    err = float(np.max(np.abs(y_g - y_a)) / np.max(np.abs(y_g)))
    t_g, t_a = [], []
    for _ in range(3):
        t_g.append(timed(lambda: run("gathered"))[0])
        t_a.append(timed(lambda: run("auto"))[0])
    with torch.no_grad():
        pc, pa = t.encode_ions(cat, an)
        tensors, image = t._head_tensors(), t._transfer_image()
        uc = ops.transfer_ion_half("cat", pc, tensors, t.fp_size, t.mixing_size)
        ua = ops.transfer_ion_half("an", pa, tensors, t.fp_size, t.mixing_size)
        launch = lambda: [ops.transfer_head_grid(uc, ua, image) for _ in range(20)]
        timed(launch)
        k_ms = statistics.median(timed(launch)[0] for _ in range(3)) / 20
    ms_g, ms_a = statistics.median(t_g), statistics.median(t_a)
    flops = C * A * PAIR_FLOP / (k_ms * 1e-3)
    line = {"config": name, "atom_dim": D, "steps": S, "C": C, "A": A, "pairs": C * A,
            "predict_grid_gathered_ms": round(ms_g, 3), "predict_grid_auto_ms": round(ms_a, 3),
            "speedup": round(ms_g / ms_a, 2), "rounds_gathered_ms": [round(x, 3) for x in t_g],
            "rounds_auto_ms": [round(x, 3) for x in t_a], "gathered_spread_ms": round(max(t_g) - min(t_g), 3),
            "grid_kernel_us": round(k_ms * 1e3, 2), "grid_kernel_GFLOPs": round(flops / 1e9, 1),
            "grid_kernel_of_f32_mfma_peak": round(flops / MFMA_F32_PEAK, 3), "max_rel_diff": err}
    print(json.dumps(line), flush=True)
    lines.append(line)
    del t
    torch.cuda.empty_cache()
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
with open(args.out, "a") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
