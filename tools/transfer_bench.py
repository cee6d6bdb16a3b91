"""Transfer-learning step timing beside the full viscosity training step ("Transfer learning"): a stage-1
step (base frozen: fused inference encoder + head kernels + Adam over 10 tensors), a stage-2 step (the last two
message-passing steps of each ion train) and the full viscosity step, at the default sizes on synthetic padded graphs,
alternating in one job; median of --rounds runs each with the spread.  One JSON line per (contender, graph mode).
    python tools/transfer_bench.py [--batch 32] [--rounds 3] [--iters 200] [--explicit-h] [--out FILE]"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from ionic_mpnn_amd import model, synthetic, train, weights  # noqa: E402

UNFREEZE_KEYS = ["cat_bmm_2", "cat_bmm_3", "an_bmm_2", "an_bmm_3", "gated_update_2", "gated_update_3",
                 "gated_update_6", "gated_update_7", "mix_cat_an"]

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--atom-dim", type=int, default=32)
ap.add_argument("--steps", type=int, default=4, help="message-passing steps")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--explicit-h", action="store_true", help="N = 160 / E = 640 instead of N = 40 / E = 80")
ap.add_argument("--one-step", choices=["stage1", "stage2", "viscosity"],
                help="run a few graphed steps of one contender and exit (for a kernel trace)")
ap.add_argument("--out")
a = ap.parse_args()
dev = torch.device("cuda:0")
B, D, S = a.batch, a.atom_dim, a.steps
inp = synthetic.make_explicit_h_batch(B, seed=0) if a.explicit_h else synthetic.make_batch(B, seed=0)
y = np.random.default_rng(0).normal(0.0, 1.0, size=B).astype(np.float32)
w = weights.init_weights("viscosity", synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, atom_dim=D, num_steps=S, seed=1)


def viscosity():
    m = model.build_model(synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, atom_dim=D, num_steps=S, device=dev)
    m.load_weights(w)
    return m


def transfer(stage):
    with tempfile.TemporaryDirectory() as tmp:
        path = str(Path(tmp) / "viscosity_final.keras")
        viscosity().save(path)
        m = model.build_transfer_model(path, device=dev, dropout_seed=7)
    for layer in m.layers:
        layer.trainable = layer.name.startswith("mp_") or layer.name == "melting_point"
    if stage == 2:
        for layer in m.layers:
            if any(k in layer.name for k in UNFREEZE_KEYS):
                layer.trainable = True
    return m.compile(train.Adam(1e-3 if stage == 1 else 1e-4), loss=train.Huber(delta=1.0))


makers = {"stage1": lambda: transfer(1), "stage2": lambda: transfer(2),
          "viscosity": lambda: viscosity().compile(train.Adam(1e-3, clipnorm=1.0))}
if a.one_step:
    m = makers[a.one_step]()
    step = train.GraphedTrainStep(m, m._to_device(inp), y)
    for _ in range(3):
        step(m._to_device(inp), y)
    torch.cuda.synchronize()
    sys.exit(0)

lines = []
for graph in (True, False):
    steps = {}
    for name, make in makers.items():
        m = make()
        d = m._to_device(inp)
        steps[name] = (train.GraphedTrainStep(m, d, y) if graph else m.train_on_batch, d, m)
    times = {name: [] for name in steps}
    for r in range(a.rounds + 1):                  # round 0 warms up and is dropped
        for name, (step, d, _) in steps.items():   # alternating: every round times every contender once
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                step(d, y)
            torch.cuda.synchronize()
            if r:
                times[name].append((time.perf_counter() - t0) / a.iters * 1e3)
    for name, ts in times.items():
        m = steps[name][2]
        lines.append({"step": name, "graph": graph, "batch": B, "shape": "N160_E640" if a.explicit_h else "N40_E80",
                      "atom_dim": D, "mp_steps": S, "ms_median": float(np.median(ts)), "ms_min": min(ts),
                      "ms_max": max(ts), "ms_all": [round(t, 4) for t in ts],
                      "trained_tensors": len(m.optimizer._vars),
                      "trained_params": int(sum(v.numel() for v in m.optimizer._vars))})
for ln in lines:
    print(json.dumps(ln), flush=True)
if a.out:
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
