"""Stage 1 of transfer learning with and without cached encodings ("Cached encodings"): the captured
batch-32 step and a whole epoch of ``fit``, the plain path (fused inference encoder + head kernels + Adam per step)
beside ``cache_frozen_encoder=True`` (every distinct ion encoded once, the head's loss over indexed rows), alternating
in one process; medians of --rounds runs with the spread.  Synthetic explicit-hydrogen graphs at the reference's padded
shape N = 160 / E = 640; --samples samples drawn from --cations + --anions distinct ions (default 2048 over 256 + 64:
6.4 samples per distinct ion, the repeat rate of a melting-point set of a few thousand salts over a few hundred ions).
--only embeddings (README.md, "Training the unseen tokens"): what it costs to train embedding rows in stage 1 - the
captured step three ways, alternating: the head alone over cached encodings, both embeddings fully trainable (the
whole layered step with an encoder backward), and both embeddings frozen with a sixth of the tokens the set uses listed
as ``trainable_rows``.
Reads nothing outside the repository.  One JSON line per measurement.
    python tools/stage1_bench.py [--batch 32] [--rounds 5] [--iters 300] [--epochs 10] [--only all|stage1|embeddings]
                                 [--out FILE]"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from ionic_mpnn_amd import _lib, data, model, synthetic, train, weights  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--atom-dim", type=int, default=32)
ap.add_argument("--steps", type=int, default=4, help="message-passing steps")
ap.add_argument("--samples", type=int, default=2048)
ap.add_argument("--cations", type=int, default=256)
ap.add_argument("--anions", type=int, default=64)
ap.add_argument("--max-atoms", type=int, default=160)
ap.add_argument("--max-edges", type=int, default=640)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=300, help="captured steps per timed window")
ap.add_argument("--epochs", type=int, default=10, help="timed epochs per fit (one more runs first and is reported apart)")
ap.add_argument("--only", choices=("all", "stage1", "embeddings"), default="all")
ap.add_argument("--out")
a = ap.parse_args()
dev = torch.device("cuda:0")
B, D, S, n = a.batch, a.atom_dim, a.steps, a.samples
rng = np.random.default_rng(0)
pool = synthetic.make_explicit_h_batch(max(a.cations, a.anions), max_atoms=a.max_atoms, max_edges=a.max_edges, seed=0)
ci, ai = rng.integers(0, a.cations, n), rng.integers(0, a.anions, n)
x = {f"{p}_{k}": pool[f"{p}_{k}"][idx] for p, idx in (("cat", ci), ("an", ai)) for k in ("atom", "bond", "connectivity")}
y = rng.normal(0.0, 1.0, n).astype(np.float32)
shape = f"N{x['cat_atom'].shape[1]}_E{x['cat_bond'].shape[1]}"
w0 = weights.init_weights("viscosity", synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, atom_dim=D, num_steps=S, seed=1)
if not torch.cuda.is_available():
    sys.exit(f"stage1_bench needs a GPU: a timing without one says nothing ({n} samples of shape {shape} were made)")


def stage1_model(embeddings=None):
    """embeddings: None (frozen: stage 1 as the reference has it), "trainable" (both layers train every row) or "rows"
    (both frozen, every sixth token the set uses listed as trainable_rows)."""
    with tempfile.TemporaryDirectory() as tmp:
        path = str(Path(tmp) / "viscosity_final.keras")
        v = model.build_model(synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, atom_dim=D, num_steps=S, device=dev)
        v.load_weights(w0)
        v.save(path)
        m = model.build_transfer_model(path, device=dev, dropout_seed=7)
    for layer in m.layers:
        layer.trainable = layer.name.startswith("mp_") or layer.name == "melting_point"
    if embeddings == "trainable":
        m.atom_emb.trainable = m.bond_emb.trainable = True
    elif embeddings == "rows":
        use = data.token_usage(x, synthetic.DEFAULT_VA, synthetic.DEFAULT_VB)
        sixth = lambda counts: [int(v) for v in np.flatnonzero(counts[1:] > 0)[::6] + 1]
        m.atom_emb.trainable_rows, m.bond_emb.trainable_rows = sixth(use.atom), sixth(use.bond)
    return m.compile(train.Adam(1e-3), loss=train.Huber(delta=1.0))


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


def timed_rounds(steps):
    """{name: [ms per step, one value per round]} of {name: (GraphedTrainStep, its resident source)}, the contenders
    alternating inside every round; round 0 warms up and is dropped."""
    times = {name: [] for name in steps}
    for r in range(a.rounds + 1):
        for name, (step, src) in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.iters):
                step.step_on_rows(src, y_dev, rows[i % len(rows)])
            torch.cuda.synchronize()
            if r:
                times[name].append((time.perf_counter() - t0) / a.iters * 1e3)
    return times


def finish():
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


lines = []
common = {"batch": B, "shape": shape, "atom_dim": D, "mp_steps": S, "samples": n, "distinct_cations": len(set(ci)),
          "distinct_anions": len(set(ai)), "samples_per_distinct_ion": round(n / (len(set(ci)) + len(set(ai))), 2)}

# ---- the captured step: plain (the batch gathered from the resident set, encoder, head) against cached
plain, cached = stage1_model(), stage1_model()
xd = {k: v.contiguous() for k, v in plain._to_device(x).items()}
y_dev = torch.from_numpy(y).to(dev).reshape(-1, 1)
t0 = time.perf_counter()
enc = cached.frozen_encodings(x)
torch.cuda.synchronize()
encode_ms = (time.perf_counter() - t0) * 1e3
rows = [torch.from_numpy(rng.integers(0, n, B)).to(dev) for _ in range(16)]
calls = {"plain": library_calls(lambda: plain.train_on_batch({k: v[rows[0]] for k, v in xd.items()}, y_dev[rows[0]])),
         "cached": library_calls(lambda: cached.train_on_encoded_batch(enc, rows[0], y_dev[rows[0]]))}
batch0 = ({k: v[rows[0]] for k, v in xd.items()}, y[rows[0].cpu().numpy()])
if a.only != "embeddings":
    steps = {"plain": (train.GraphedTrainStep(plain, *batch0, resident=(xd, y_dev)), xd),
             "cached": (train.GraphedTrainStep(cached, rows[0], batch0[1], resident=(enc, y_dev)), enc)}
    for name, ts in timed_rounds(steps).items():
        lines.append({"what": "captured step", "path": name, **common, "ms_median": float(np.median(ts)), "ms_min": min(ts),
                      "ms_max": max(ts), "ms_all": [round(t, 4) for t in ts],
                      "library_calls_per_eager_step": len(calls[name]), "library_calls": calls[name]})
    lines.append({"what": "encode every distinct ion once", "path": "cached", **common, "ms": round(encode_ms, 3)})
    del steps

# ---- training embedding rows in stage 1: the head over cached encodings, both embeddings trainable, listed rows only
if a.only != "stage1":
    full, listed = stage1_model("trainable"), stage1_model("rows")
    n_rows = {"atom": len(listed.atom_emb.trainable_rows), "bond": len(listed.bond_emb.trainable_rows)}
    step_of = lambda m: m.train_on_batch({k: v[rows[0]] for k, v in xd.items()}, y_dev[rows[0]])
    calls = {"head only, cached encodings": calls["cached"], "embeddings trainable": library_calls(lambda: step_of(full)),
             "rows restricted": library_calls(lambda: step_of(listed))}
    steps = {"head only, cached encodings": (train.GraphedTrainStep(cached, rows[0], batch0[1], resident=(enc, y_dev)), enc),
             "embeddings trainable": (train.GraphedTrainStep(full, *batch0, resident=(xd, y_dev)), xd),
             "rows restricted": (train.GraphedTrainStep(listed, *batch0, resident=(xd, y_dev)), xd)}
    for name, ts in timed_rounds(steps).items():
        lines.append({"what": "captured step, embedding rows", "path": name, **common, "listed_rows": n_rows,
                      "ms_median": float(np.median(ts)), "ms_min": min(ts), "ms_max": max(ts),
                      "ms_all": [round(t, 4) for t in ts], "library_calls_per_eager_step": len(calls[name]),
                      "library_calls": calls[name]})
    del steps, full, listed
del plain, cached
if a.only == "embeddings":
    finish()
    sys.exit(0)


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


first, later = {"plain": [], "cached": []}, {"plain": [], "cached": []}
models = {"plain": stage1_model(), "cached": stage1_model()}
for r in range(a.rounds + 1):
    for name, m in models.items():
        clock = EpochClock()
        m.fit(x, y, epochs=a.epochs + 1, batch_size=B, seed=r, callbacks=[clock], cache_frozen_encoder=name == "cached")
        d = np.diff(clock.marks) * 1e3
        if r:
            first[name].append(float(d[0]))
            later[name] += [float(v) for v in d[1:]]
for name in models:
    lines.append({"what": "fit epoch", "path": name, **common, "steps_per_epoch": -(-n // B),
                  "ms_median": float(np.median(later[name])), "ms_min": min(later[name]), "ms_max": max(later[name]),
                  "first_epoch_ms_median": float(np.median(first[name])),
                  "note": "the first epoch holds the capture of the step and, cached, the encoding of every distinct ion"})
finish()
