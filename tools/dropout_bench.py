"""GatedUpdate dropout cost: one training step (forward + backward + Adam), eager and graphed, at
dropout rate 0 and 0.1 - config 5 (atom_dim 128, 6 steps) at batch 32 and 4096 and the config-2 shape (atom_dim 32,
batch 32).  One JSON line per case; the two rates alternate within each shape so drift hits both.
python tools/dropout_bench.py [--iters 30] [--reps 3]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from ionic_mpnn_amd import model, synthetic, train, weights  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--reps", type=int, default=3, help="alternating timing rounds per case (median reported)")
a = ap.parse_args()
dev = torch.device("cuda:0")
CASES = [("config5_b32", 128, 8, 6, 32), ("config5_b4096", 128, 8, 6, 4096), ("config2_b32", 32, 8, 4, 32)]
for name, D, K, S, B in CASES:
    inp = synthetic.make_batch(B, seed=0)
    y = np.random.default_rng(0).normal(4.0, 1.0, size=B).astype(np.float32)
    w = weights.init_weights("viscosity", synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, atom_dim=D, bond_dim=K,
                             num_steps=S, seed=1)
    runs = {}
    for rate in (0.0, 0.1):
        m = model.build_model(synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, atom_dim=D, bond_dim=K, num_steps=S,
                              device=dev, dropout_rate=rate, dropout_seed=7)
        m.load_weights(w)
        m.compile(train.Adam(1e-3, clipnorm=1.0))
        d = m._to_device(inp)
        for graph in (False, True):
            step = train.GraphedTrainStep(m, d, y) if graph else m.train_on_batch
            for _ in range(3):
                step(d, y)
            runs[(rate, graph)] = (step, d)
    times = {k: [] for k in runs}
    iters = a.iters if B <= 256 else max(5, a.iters // 3)
    for _ in range(a.reps):
        for k, (step, d) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                step(d, y)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / iters * 1e3)
    for graph in (False, True):
        t0, t1 = float(np.median(times[(0.0, graph)])), float(np.median(times[(0.1, graph)]))
        print(json.dumps({"case": name, "atom_dim": D, "mp_steps": S, "batch": B, "graph": graph,
                          "ms_rate0": round(t0, 4), "ms_rate0.1": round(t1, 4),
                          "overhead_pct": round(100.0 * (t1 / t0 - 1.0), 2),
                          "ms_rate0_all": [round(v, 4) for v in times[(0.0, graph)]],
                          "ms_rate0.1_all": [round(v, 4) for v in times[(0.1, graph)]]}), flush=True)
