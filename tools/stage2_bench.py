"""Stage 2 of transfer learning with and without cached frozen steps ("Cached frozen steps"): the captured
stage-2 step and a whole epoch of ``fit``, the plain path (every step recomputes the atom embedding and the frozen steps
0 and 1 of both ions) beside ``cache_frozen_steps=True`` (every distinct ion through its frozen steps once, one
impnn_state_rows launch per step, the layered pass resumed at step 2), alternating in one process; medians of --rounds
runs with the spread.  Synthetic explicit-hydrogen graphs at the reference's padded shape N = 160 / E = 640, the
reference's UNFREEZE_KEYS; --samples samples drawn from --cations + --anions distinct ions (default 2048 over 256 + 64).
--configs lists atom_dim:batch pairs for the captured step (default 32:32, 128:32, 32:4096); the fit epoch is timed for
the first.  Reads nothing outside the repository.  One JSON line per measurement.
    python tools/stage2_bench.py [--configs 32:32,128:32,32:4096] [--rounds 5] [--iters 300] [--epochs 10] [--out FILE]"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from ionic_mpnn_amd import _lib, model, synthetic, train, weights  # noqa: E402

UNFREEZE_KEYS = ["cat_bmm_2", "cat_bmm_3", "an_bmm_2", "an_bmm_3", "gated_update_2", "gated_update_3",
                 "gated_update_6", "gated_update_7", "mix_cat_an"]   # train_melting_point_transfer.py, stage 2

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="32:32,128:32,32:4096", help="atom_dim:batch pairs of the captured step")
ap.add_argument("--steps", type=int, default=4, help="message-passing steps")
ap.add_argument("--samples", type=int, default=2048)
ap.add_argument("--cations", type=int, default=256)
ap.add_argument("--anions", type=int, default=64)
ap.add_argument("--max-atoms", type=int, default=160)
ap.add_argument("--max-edges", type=int, default=640)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=300, help="captured steps per timed window at batch 32 (fewer above)")
ap.add_argument("--epochs", type=int, default=10, help="timed epochs per fit (one more runs first and is reported apart)")
ap.add_argument("--out")
a = ap.parse_args()
dev = torch.device("cuda:0")
S, n = a.steps, a.samples
configs = [tuple(int(v) for v in c.split(":")) for c in a.configs.split(",")]
rng = np.random.default_rng(0)
pool = synthetic.make_explicit_h_batch(max(a.cations, a.anions), max_atoms=a.max_atoms, max_edges=a.max_edges, seed=0)
ci, ai = rng.integers(0, a.cations, n), rng.integers(0, a.anions, n)
x = {f"{p}_{k}": pool[f"{p}_{k}"][idx] for p, idx in (("cat", ci), ("an", ai)) for k in ("atom", "bond", "connectivity")}
y = rng.normal(0.0, 1.0, n).astype(np.float32)
shape = f"N{x['cat_atom'].shape[1]}_E{x['cat_bond'].shape[1]}"
if not torch.cuda.is_available():
    sys.exit(f"stage2_bench needs a GPU: a timing without one says nothing ({n} samples of shape {shape} were made)")


def stage2_model(D):
    w0 = weights.init_weights("viscosity", synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, atom_dim=D, num_steps=S, seed=1)
    with tempfile.TemporaryDirectory() as tmp:
        path = str(Path(tmp) / "viscosity_final.keras")
        v = model.build_model(synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, atom_dim=D, num_steps=S, device=dev)
        v.load_weights(w0)
        v.save(path)
        m = model.build_transfer_model(path, device=dev, dropout_seed=7)
    for layer in m.layers:
        layer.trainable = (layer.name.startswith("mp_") or layer.name == "melting_point"
                           or any(k in layer.name for k in UNFREEZE_KEYS))
    return m.compile(train.Adam(1e-4), loss=train.Huber(delta=1.0))


def library_calls(fn):
    """The library entries one call of ``fn`` goes through, in order (size queries left out)."""
    lib, names, saved = _lib.load(), [], {}
    for name, (restype, _) in _lib.SIGNATURES.items():
        if restype is _lib.C.c_int and not name.endswith(("_bytes", "_floats", "_layout", "_check")):
            saved[name] = getattr(lib, name)
            setattr(lib, name, (lambda nm, f: lambda *args: (names.append(nm), f(*args))[1])(name, saved[name]))
    try:
        fn()
    finally:
        for name, f in saved.items():
            setattr(lib, name, f)
    torch.cuda.synchronize()
    return names


lines = []
y_dev = torch.from_numpy(y).to(dev).reshape(-1, 1)


def common(D, B):
    return {"batch": B, "shape": shape, "atom_dim": D, "mp_steps": S, "samples": n, "distinct_cations": len(set(ci)),
            "distinct_anions": len(set(ai)), "samples_per_distinct_ion": round(n / (len(set(ci)) + len(set(ai))), 2)}


# ---- the captured step: plain (the batch gathered from the resident set, the whole layered pass) against resumed
for D, B in configs:
    plain, cached = stage2_model(D), stage2_model(D)
    xd = {k: v.contiguous() for k, v in plain._to_device(x).items()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = cached.frozen_states(xd)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    rows = [torch.from_numpy(rng.integers(0, n, B)).to(dev) for _ in range(16)]
    first = {k: v[rows[0]] for k, v in xd.items()}
    calls = {"plain": library_calls(lambda: plain.train_on_batch(first, y_dev[rows[0]])),
             "cached": library_calls(lambda: cached.train_on_state_batch(st, xd, rows[0], y_dev[rows[0]]))}
    y0 = y[rows[0].cpu().numpy()]
    steps = {"plain": train.GraphedTrainStep(plain, first, y0, resident=(xd, y_dev)),
             "cached": train.GraphedTrainStep(cached, first, y0, resident=(xd, y_dev), states=st)}
    iters = max(10, a.iters * 32 // max(B, 32))
    times = {name: [] for name in steps}
    for r in range(a.rounds + 1):                       # round 0 warms up and is dropped
        for name, step in steps.items():                # alternating: every round times every contender once
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(iters):
                step.step_on_rows(xd, y_dev, rows[i % len(rows)])
            torch.cuda.synchronize()
            if r:
                times[name].append((time.perf_counter() - t0) / iters * 1e3)
    for name, ts in times.items():
        lines.append({"what": "captured step", "path": name, **common(D, B), "ms_median": float(np.median(ts)),
                      "ms_min": min(ts), "ms_max": max(ts), "ms_all": [round(t, 4) for t in ts], "iters": iters,
                      "library_calls_per_eager_step": len(calls[name]), "library_calls": calls[name]})
    lines.append({"what": "every distinct ion through its frozen steps once", "path": "cached", **common(D, B),
                  "ms": round(build_ms, 3), "table_bytes": st.nbytes})
    for ln in lines[-3:]:
        print(json.dumps(ln), flush=True)
    del steps, plain, cached, st, xd


# ---- a whole epoch of fit: n / batch steps and the host work around them
class EpochClock(train.Callback):
    def __init__(self):
        super().__init__()
        self.marks = []

    def on_train_begin(self, logs=None):
        torch.cuda.synchronize()
        self.marks = [time.perf_counter()]

    def on_epoch_end(self, epoch, logs=None):   # (the epoch's loss was read on the host: the device is idle)
        self.marks.append(time.perf_counter())


D, B = configs[0]
first_ep, later = {"plain": [], "cached": []}, {"plain": [], "cached": []}
models = {"plain": stage2_model(D), "cached": stage2_model(D)}
for r in range(a.rounds + 1):
    for name, m in models.items():
        clock = EpochClock()
        m.fit(x, y, epochs=a.epochs + 1, batch_size=B, seed=r, callbacks=[clock], cache_frozen_steps=name == "cached")
        d = np.diff(clock.marks) * 1e3
        if r:
            first_ep[name].append(float(d[0]))
            later[name] += [float(v) for v in d[1:]]
for name in models:
    lines.append({"what": "fit epoch", "path": name, **common(D, B), "steps_per_epoch": -(-n // B),
                  "ms_median": float(np.median(later[name])), "ms_min": min(later[name]), "ms_max": max(later[name]),
                  "first_epoch_ms_median": float(np.median(first_ep[name])),
                  "note": "the first epoch holds the capture of the step and, cached, every distinct ion's frozen steps"})
    print(json.dumps(lines[-1]), flush=True)
if a.out:
    with open(a.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
