"""Cation x anion screening: MPNNModel.predict_grid against MPNNModel.predict on the explicitly expanded pair list
(the only inference entry before the grid existed), plus the grid kernel alone against the HBM write rate.  For the
transfer model: predict_grid with grid_head_mode "gathered" (self.head on gathered tiles of pairs) against "auto" (the
matrix-core grid, impnn_transfer_head_grid), plus that kernel alone against the f32 MFMA peak.

python tools/screen_bench.py [--quick] [--only viscosity|transfer]      -> one JSON line per configuration, appended to profiles/screen_bench.jsonl
python tools/screen_bench.py --select [--quick] [--only ...]            -> the top-k selection instead (see below)
python tools/screen_bench.py --select --where FRACTION [--quick]        -> the constrained screen instead (see below)
python tools/screen_bench.py --partners [--where FRACTION] [--quick]    -> each ion's best partners instead (see below)
python tools/screen_bench.py --summary [--where FRACTION] [--size N] [--ensemble M | --mc S]  -> per-ion statistics (see below)
python tools/screen_bench.py --rank [--where FRACTION] [--quick]        -> the best-k pair mask instead (see below)
python tools/screen_bench.py --ensemble M [--select] [--where FRACTION] [--size N]  -> a deep ensemble instead (see below)
python tools/screen_bench.py --mc S [--select] [--where FRACTION] [--size N]        -> Monte-Carlo dropout instead (see below)
python tools/screen_bench.py --pareto [--where FRACTION] [--size N]     -> the Pareto front of two models instead (see below)
python tools/screen_bench.py --domain R [--size N]                       -> the applicability domain instead (see below)

Method: three alternating rounds (expanded, grid, expanded, grid, ...) after one warm-up of each, HIP events around each
call on the current stream plus a host synchronisation (both entries end with a device-to-host copy), median per side.
The expanded inputs are built once and stay on the device, so the baseline pays no host-to-device copy; predict_grid
gets host arrays of C + A molecules, as a caller would hand them over.

--select: MPNNModel.screen_top_k(k = 100) against the way to the same answer without it, predict_grid followed by
data.grid_top_k on the host, at the configurations above and at two larger ones (C * A * nT in the 10^7 range); the
same three alternating rounds, wall time around each side (the host sort is part of the old way).  Plus the selecting
launches alone (impnn_head_grid_topk / impnn_transfer_head_grid_topk with their merge; a viscosity sweep above
ops.SELECT_MAX_T temperatures takes several) against the materialising launch of the same C x A x nT, 10 calls
between two HIP events.

--select --where F: the constrained screen "of the pairs the melting-point model puts below a limit, the k least viscous
at 298.15 K", the limit being the F quantile of the melting-point grid.  Three alternating rounds after a warm-up, wall
time, of (a) mp.screen_mask + visc.screen_top_k(where=) against (b) the way to the same answer without them: two
predict_grid calls and data.grid_top_k(where=) on the host; screen_mask and screen_top_k(where=) also on their own.  Then
the selecting launches alone, 10 calls between two HIP events, five rounds each in turn: plain, an all-ones mask, a
random mask of density F, and a block-structured mask of the same density (whole tiles of the kernel set or clear), for
the head grid and the transfer grid; and the mask-writing launch against the materialising one.

--partners: MPNNModel.screen_best_partners(m = 3) against predict_grid followed by data.grid_best_partners on the host,
at the configurations of --select: three alternating rounds after a warm-up of each, wall time, median and spread; the
two ways must return the same bits.  Plus the partner-selecting launches alone (impnn_head_grid_partners /
impnn_transfer_head_grid_partners with their merge; a sweep above ops.SELECT_MAX_T temperatures takes several) against
the materialising launch of the same C x A x nT, 10 calls between two HIP events, three rounds each in turn.  With
--where F both ways run under one random pair mask of density F.

--summary: the per-ion summary launches (ops.grid_summary: impnn_*_grid_summary's tile launch and merge) on resident
operands over N x N pairs (--size, default 4096) at one temperature, against the materialised route in the same run:
ops.grid_values on the same operands, then torch count / sum / sum of squares in float64 and amin / amax along both
axes.  The head grid and the transfer grid, or with --ensemble M / --mc S that family on its score (kappa = 1).  Five
alternating rounds after a warm-up of each, HIP events, median and spread; "ratio_exceeds_spread" says whether the
difference of the medians is larger than the widest spread between rounds.  The counts of the two routes must be equal
(the sums differ by rounding: torch's order of summation is its own).  Also the workspace per pair.  With --where F both
run under one block-structured pair mask of density F.

--rank: MPNNModel.screen_best_mask(k = 1 % of the grid, or of the mask's pairs) against predict_grid followed by
data.grid_best_mask on the host, at the large configurations of --select (all of them with --all-configs): three
alternating rounds after a warm-up of each, wall time, median and spread; the two ways must return the same words.  Plus
the launches of one rank call alone (impnn_head_grid_rank / impnn_transfer_head_grid_rank: a counting and a step launch
per digit, ops.rank_passes of them, and the mask launch; a sweep above ops.SELECT_MAX_T temperatures takes several calls)
against the materialising launch of the same C x A x nT, 10 calls between two HIP events, three rounds each in turn, and
the rank cut alone (no mask launch).  With --where F both ways run under one random pair mask of density F.

--ensemble M: ModelEnsemble of M viscosity models (atom_dim 32, 3 steps, seeds 1 .. M) over N x N pairs (--size, default
4096) at 298.15 K.  Three alternating rounds after a warm-up of each, wall time, median and spread, of
ensemble.predict_grid(kappa = 1) against the way to the same three grids without it: M predict_grid calls and
data.ensemble_grid_stats on the host (the two must agree bit for bit).  With --select: ensemble.screen_top_k(k = 100,
kappa = 1) against the same M grids, the host statistic and data.grid_top_k; with --where F both under one random pair
mask of density F.

--mc S: MPNNModel.mc_dropout(S) of a transfer model (atom_dim 32, 3 steps) over N x N pairs (--size, default 4096).  Five
alternating rounds after a warm-up of each, wall time, median and spread, of mc.predict_grid(kappa = 1) beside the
deterministic predict_grid of the same model and species (one grid against the mean, spread and score of S).  Then the
launches alone over resident u rows, 10 calls between two HIP events, five rounds each in turn: impnn_transfer_mc_grid
(mean, std and score written) beside impnn_transfer_head_grid, their ratio beside the MFMA-count expectation
(1024 + 256 S) / 1280, and the f32 MFMA rate of both.  With --select: mc.screen_top_k(k = 100, kappa = 1) beside the
model's screen_top_k, and the selecting launches of both; with --where F under one random pair mask of density F.

--pareto: screen_pareto of a viscosity model at 298.15 K against a melting-point model (atom_dim 32, 3 steps) over N x N
pairs (--size, default 4096), both minimised, against the way to the same front without it: two predict_grid calls and
data.pareto_front on the host.  Three alternating rounds after a warm-up of each, wall time, median and spread; the two
ways must return the same front.  Plus the filter's stages alone over the two resident planes (begin, range, minima,
staircase, collect: 10 runs between two HIP events, three rounds), and the candidate count against the front size.  With
--where F both ways run under one random pair mask of density F.

--domain R: the applicability domain of a viscosity model (atom_dim 32, 3 steps) over N x N pairs (--size, default 4096)
against R reference pairs drawn from the grid: MPNNModel.screen_domain_mask(at_most = radius(0.95)) and
MPNNModel.domain_grid against the torch path a user would write without them - gathered tiles of z = mix_cat[i] +
mix_an[j], torch.cdist against the reference rows, min - from the same encode_ions and head_ion_mix rows.  Three
alternating rounds after a warm-up of each, wall time, median and spread.  Plus the launches alone over resident mixing
rows (impnn_domain_grid, impnn_domain_grid_mask, and the torch tile loop), 5 calls between two HIP events, three rounds
each in turn, the kernel's 2 * R * Mx lane operations per pair over its time, and how far the torch distances lie from
the kernel's (torch.cdist expands |z|^2 - 2 z.r + |r|^2 on the matrix cores: a training pair is not at exactly 0).

--diverse K: MPNNModel.screen_diverse (K picks by farthest-point selection, impnn_diverse_select) of the same model over
N x N pairs against R reference pairs (--reference, default 7700), against the torch loop a user would write from the
same mixing rows: D from ops.domain_grid, then K times an argmax under the mask (one host round trip each) and
torch.minimum with the distances to z[pick] over a materialised z (N x N x Mx floats).  Three alternating rounds after a
warm-up of each, wall time, median and spread; how many picks the two ways share (the torch loop orders its own float32
distances and breaks ties as torch.argmax does).  Plus the launches alone over resident mixing rows, 3 calls between
two HIP events, three rounds each in turn: the whole selection, the selection with k = 1 (the init pass) beside
impnn_domain_grid, and from the two the time of one step and its 8 bytes of state traffic per pair over that time.
With --where F both ways run under one random pair mask of density F."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from ionic_mpnn_amd import _lib, data, model as MM, ops, screening, synthetic, weights  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="the first configuration only")
ap.add_argument("--only", choices=("viscosity", "transfer"), help="one family of configurations")
ap.add_argument("--select", action="store_true", help="time screen_top_k against predict_grid + host selection")
ap.add_argument("--partners", action="store_true", help="time screen_best_partners against predict_grid + host reference")
ap.add_argument("--rank", action="store_true", help="time screen_best_mask against predict_grid + host reference")
ap.add_argument("--summary", action="store_true", help="time the per-ion summary launches against the materialised grid + torch "
                "reductions; with --ensemble M or --mc S that family, else the head grid and the transfer grid; --size, --where")
ap.add_argument("--all-configs", action="store_true", help="with --rank: the small configurations of --select too")
ap.add_argument("--where", type=float, metavar="FRACTION", help="with --select: the constrained screen at this mask density; "
                "with --partners, --rank: a random mask of this density")
ap.add_argument("--ensemble", type=int, metavar="M", help="a ModelEnsemble of M viscosity models against M predict_grid calls "
                "and the host statistic; with --select the top-k on the score")
ap.add_argument("--mc", type=int, metavar="S", help="MC dropout of a transfer model with S samples beside its deterministic grid; "
                "with --select the top-k on the score")
ap.add_argument("--pareto", action="store_true", help="time screen_pareto (viscosity x melting point) against two predict_grid "
                "calls and data.pareto_front on the host")
ap.add_argument("--domain", type=int, metavar="R", help="time screen_domain_mask and domain_grid over R reference pairs "
                "against gathered tiles, torch.cdist and min")
ap.add_argument("--diverse", type=int, metavar="K", help="time screen_diverse (K picks by farthest-point selection) against "
                "the torch loop over a materialised z; --reference R reference pairs, --where F a random mask of that density")
ap.add_argument("--reference", type=int, default=7700, metavar="R", help="with --diverse: the reference pairs")
ap.add_argument("--size", type=int, default=4096, help="with --ensemble, --mc, --pareto, --domain, --diverse: cations = anions = this many")
ap.add_argument("--out", default=str(ROOT / "profiles" / "screen_bench.jsonl"))
args = ap.parse_args()
other = args.summary or args.select or args.partners or args.rank or args.ensemble or args.pareto or args.domain or args.mc or args.diverse  # another table than the default one
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
for name, D, S, C, A, nT, bs in [] if args.only == "transfer" or other else CONFIGS[:1] if args.quick else CONFIGS:
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


for name, D, S, C, A in [] if args.only == "viscosity" or other else TRANSFER_CONFIGS[:1] if args.quick else TRANSFER_CONFIGS:
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

# ---- --select: screen_top_k against predict_grid + data.grid_top_k, then the launches alone
SELECT_K = 100
SELECT_CONFIGS = [("viscosity",) + c[:6] for c in CONFIGS] + [("viscosity", "config2 2048x2048x4", 32, 3, 2048, 2048, 4)] \
    + [("transfer",) + c + (0,) for c in TRANSFER_CONFIGS] + [("transfer", "transfer 4096x4096", 32, 3, 4096, 4096, 0)]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def same_top(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32) if x.dtype == np.float32 else x, np.asarray(y).view(np.uint32)
                              if y.dtype == np.float32 else y) for x, y in zip(a, b))


# ---- --select --where F: the constrained screen
# (name, atom_dim, steps, C, A)
WHERE_CONFIGS = [("where 1024x1024", 32, 3, 1024, 1024), ("where 4096x4096", 32, 3, 4096, 4096)]
T_ROOM = np.array([298.15], np.float32)


def block_mask(C, A, tile, fraction, rng):
    """Whole tiles of tile = (rows, anions) set with probability `fraction`: the density of a random mask, in blocks."""
    tc, ta = tile
    on = rng.random(((C + tc - 1) // tc, (A + ta - 1) // ta)) < fraction
    return np.repeat(np.repeat(on, tc, axis=0), ta, axis=1)[:C, :A]


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


PARTNERS_M = 3


def same_partners(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32) if x.dtype == np.float32 else x, np.asarray(y).view(np.uint32)
                              if y.dtype == np.float32 else y) for sa, sb in zip(a, b) for x, y in zip(sa, sb))


RANK_CONFIGS = ("config2 2048x2048x4", "transfer 1024x1024", "transfer 4096x4096")  # the rows of the selection table

DOMAIN_TILE_FLOATS = 1 << 28  # the torch path's pairs x R distance tile: 1 GiB of float32

if args.summary:
    # One temperature, cations = anions = --size.  The fused route: ops.grid_summary on resident operands (the tile
    # launch and the merge).  The materialised route, in the same run: ops.grid_values on the same operands, then torch
    # count / sum / sum of squares in float64 and amin / amax along both axes.  Medians of 5 alternating rounds.
    N = args.size
    cat, _ = species(N, 1)
    _, an = species(N, 2)
    rng = np.random.default_rng(0)
    T1 = torch.tensor([298.15], dtype=torch.float32)
    if args.ensemble:
        from ionic_mpnn_amd import ModelEnsemble
        from ionic_mpnn_amd.ensemble import _EnsembleScreen
        members = []
        for i in range(args.ensemble):
            m = MM.build_model(Va, Vb, atom_dim=32, num_steps=3, device=dev)
            m.load_weights(weights.init_weights("viscosity", Va, Vb, atom_dim=32, num_steps=3, seed=1 + i, perturb=True))
            members.append(m)
        families = [("ensemble M=%d" % args.ensemble, _EnsembleScreen(ModelEnsemble(members), cat, an, T1, None, 4096, 1.0).operands)]
    elif args.mc:
        from ionic_mpnn_amd.mc_dropout import _McScreen
        families = [("mc S=%d" % args.mc, _McScreen(build_transfer(32, 3).mc_dropout(args.mc), cat, an, None, 4096, 1.0).operands)]
    else:
        m = MM.build_model(Va, Vb, atom_dim=32, num_steps=3, device=dev)
        m.load_weights(weights.init_weights("viscosity", Va, Vb, atom_dim=32, num_steps=3, seed=1, perturb=True))
        families = [("head", screening._Screen(m, cat, an, T1, None, 4096).operands),
                    ("transfer", screening._Screen(build_transfer(32, 3), cat, an, None, None, 4096).operands)]
    for name, g in families:
        blocks = ops.SUMMARY_BLOCKS[g.family]
        where_b = block_mask(N, N, blocks, args.where, rng) if args.where is not None else None
        where = data.PairMask.from_bool(where_b, device=dev) if where_b is not None else None
        live_d = torch.from_numpy(where_b).to(dev) if where_b is not None else None
        fused = lambda: ops.grid_summary(g, where=where.words if where is not None else None)

        def materialised():
            v = ops.grid_values(g)
            v = (v[2] if g.family >= 2 else v).reshape(N, N).double()
            live = ~torch.isnan(v) if live_d is None else live_d & ~torch.isnan(v)
            x = torch.where(live, v, torch.zeros_like(v))
            lo = torch.where(live, v, torch.full_like(v, float("inf")))
            hi = torch.where(live, v, torch.full_like(v, float("-inf")))
            return [f(axis) for axis in (1, 0) for f in (lambda a: live.sum(a), lambda a: x.sum(a), lambda a: (x * x).sum(a),
                                                         lambda a: lo.amin(a), lambda a: hi.amax(a))]

        timed(fused), timed(materialised)
        t_f, t_m = [], []
        for _ in range(5):
            t_m.append(timed(materialised)[0])
            t_f.append(timed(fused)[0])
        rec, ref = fused(), materialised()
        torch.cuda.synchronize()
        count_ok = bool(torch.equal(rec[0][0].long(), ref[0]) and torch.equal(rec[3][0].long(), ref[5]))
        mean_diff = float((rec[1][0, :, 0] - ref[1]).abs().max() / ref[1].abs().max().clamp_min(1e-300))
        need = int(_lib.load().impnn_grid_summary_workspace_bytes(g.family, N, N, 1))
        spread_ms = max(max(t_f) - min(t_f), max(t_m) - min(t_m))
        line = {"config": "summary %s %dx%d" % (name, N, N) + ("" if args.where is None else " F=%g" % args.where),
                "family": g.family, "C": N, "A": N, "nT": 1, "where": args.where,
                "materialised_plus_torch_reductions_ms": spread(t_m), "grid_summary_ms": spread(t_f),
                "ratio": round(statistics.median(t_m) / statistics.median(t_f), 2),
                "ratio_exceeds_spread": bool(abs(statistics.median(t_m) - statistics.median(t_f)) > spread_ms),
                "workspace_bytes": need, "workspace_bytes_per_pair": need / (N * N),
                "expected_bytes_per_pair": 32 * (1 / blocks[0] + 1 / blocks[1]),
                "counts_equal": count_ok, "sum_max_rel_diff": mean_diff}
        print(json.dumps(line), flush=True)
        lines.append(line)

elif args.diverse:
    N, R, K = args.size, args.reference, args.diverse
    m = MM.build_model(Va, Vb, atom_dim=32, num_steps=3, device=dev)
    m.load_weights(weights.init_weights("viscosity", Va, Vb, atom_dim=32, num_steps=3, seed=1, perturb=True))
    cat, _ = species(N, 1)
    _, an = species(N, 2)
    rng = np.random.default_rng(3)
    flat = rng.choice(N * N, size=R, replace=False)
    dom = m.fit_domain(cat, an, flat // N, flat % N)
    Mx = m.mixing_size
    where_h = None if args.where is None else rng.random((N, N)) < args.where
    where = None if where_h is None else data.PairMask.from_bool(where_h, device=dev)
    live = None if where_h is None else torch.from_numpy(where_h).to(dev)

    def mixing_rows():
        with torch.no_grad():
            pc, pa = m.encode_ions(cat, an)
            w = m._packed_head()
            return ops.head_ion_mix("viscosity", "cat", pc, w, m.fp_size, Mx), ops.head_ion_mix("viscosity", "an", pa, w, m.fp_size, Mx)

    def torch_way():
        mc, ma = mixing_rows()
        D, _ = ops.domain_grid(mc, ma, dom.rows)
        z = mc[:, None, :] + ma[None, :, :]                       # materialised: N x N x Mx floats
        picks, dist = [], []
        for _ in range(K):
            cand = D > 0 if live is None else live & (D > 0)
            score = torch.where(cand, D, torch.full_like(D, -1.0))
            at = int(torch.argmax(score))                         # the host round trip of a pick
            top = float(score.view(-1)[at])
            if not top > 0:
                break
            picks.append(at)
            dist.append(top)
            D = torch.minimum(D, (z - z[at // N, at % N]).square().sum(dim=2).sqrt())
        return np.asarray(picks, np.int64), np.asarray(dist, np.float32)

    new_way = lambda: m.screen_diverse(cat, an, dom, k=K, where=where)
    (p_t, d_t), sel = wall(torch_way)[1], wall(new_way)[1]
    t_torch, t_new = [], []
    for _ in range(3):
        t_torch.append(wall(torch_way)[0])
        t_new.append(wall(new_way)[0])
    mc, ma = mixing_rows()
    words = None if where is None else where.words
    REP = 3
    runs = {"diverse_select": lambda: [ops.domain_diverse(mc, ma, dom.rows, K, where=words) for _ in range(REP)],
            "diverse_select_k1": lambda: [ops.domain_diverse(mc, ma, dom.rows, 1, where=words) for _ in range(REP)],
            "domain_grid": lambda: [ops.domain_grid(mc, ma, dom.rows) for _ in range(REP)]}
    got = {n: [] for n in runs}
    for fn in runs.values():
        timed(fn)
    for _ in range(3):
        for n, fn in runs.items():
            got[n].append(timed(fn)[0] / REP * 1e3)
    p_k = sel.cation * N + sel.anion
    shared = min(len(p_t), len(p_k))
    step_us = (statistics.median(got["diverse_select"]) - statistics.median(got["diverse_select_k1"])) / max(K - 1, 1)
    line = {"config": f"diverse {N}x{N} R={len(dom)} Mx={Mx} K={K}" + ("" if args.where is None else f" where={args.where}"),
            "C": N, "A": N, "R": len(dom), "Mx": Mx, "K": K, "where": args.where, "picks": int(len(p_k)),
            "competing": int(sel.competing), "torch_loop_ms": spread(t_torch), "screen_diverse_ms": spread(t_new),
            "speedup": round(statistics.median(t_torch) / statistics.median(t_new), 2),
            "launch_us": {n: spread(x) for n, x in got.items()}, "step_us": round(step_us, 2),
            "step_state_GBps": round(8.0 * N * N / (step_us * 1e-6) / 1e9, 1) if step_us > 0 else None,
            "torch_picks": int(len(p_t)), "same_leading_picks": int(np.argmin(np.append(p_t[:shared] == p_k[:shared], False))),
            "same_picks_as_sets": int(len(set(p_t.tolist()) & set(p_k.tolist()))),
            "last_distance": float(sel.distance[-1]) if len(p_k) else None,
            "torch_last_distance": float(d_t[-1]) if len(p_t) else None}
    print(json.dumps(line), flush=True)
    lines.append(line)
elif args.domain:
    N, R = args.size, args.domain
    m = MM.build_model(Va, Vb, atom_dim=32, num_steps=3, device=dev)
    m.load_weights(weights.init_weights("viscosity", Va, Vb, atom_dim=32, num_steps=3, seed=1, perturb=True))
    cat, _ = species(N, 1)
    _, an = species(N, 2)
    flat = np.random.default_rng(3).choice(N * N, size=R, replace=False)
    dom = m.fit_domain(cat, an, flat // N, flat % N)
    radius = dom.radius(0.95)
    Mx = m.mixing_size

    def mixing_rows():
        with torch.no_grad():
            pc, pa = m.encode_ions(cat, an)
            w = m._packed_head()
            return ops.head_ion_mix("viscosity", "cat", pc, w, m.fp_size, Mx), ops.head_ion_mix("viscosity", "an", pa, w, m.fp_size, Mx)

    def torch_tiles(mc, ma):
        """Gathered tiles of z, torch.cdist, min -> (distance, nearest) (N,N) on the device."""
        rows = max(1, DOMAIN_TILE_FLOATS // (N * len(dom)))
        ds, ns = [], []
        for lo in range(0, N, rows):
            z = (mc[lo:lo + rows, None, :] + ma[None, :, :]).reshape(-1, Mx)
            d, n = torch.cdist(z, dom.rows).min(dim=1)
            ds.append(d)
            ns.append(n)
        return torch.cat(ds).reshape(N, N), torch.cat(ns).reshape(N, N)

    def torch_way():
        d, n = torch_tiles(*mixing_rows())
        return d.cpu().numpy(), n.cpu().numpy(), data.PairMask.from_bool((d <= float(radius)).cpu().numpy())

    new_mask = lambda: m.screen_domain_mask(cat, an, dom, at_most=radius)
    new_grid = lambda: m.domain_grid(cat, an, dom)
    (d_t, n_t, mask_t), mask_k, (d_k, n_k) = wall(torch_way)[1], wall(new_mask)[1], wall(new_grid)[1]
    t_torch, t_mask, t_grid = [], [], []
    for _ in range(3):
        t_torch.append(wall(torch_way)[0])
        t_mask.append(wall(new_mask)[0])
        t_grid.append(wall(new_grid)[0])
    mc, ma = mixing_rows()
    runs = {"domain_grid": lambda: [ops.domain_grid(mc, ma, dom.rows) for _ in range(5)],
            "domain_grid_mask": lambda: [ops.domain_grid_mask(mc, ma, dom.rows, -np.inf, radius) for _ in range(5)],
            "torch_tiles": lambda: [torch_tiles(mc, ma) for _ in range(5)]}
    got = {n: [] for n in runs}
    for fn in runs.values():
        timed(fn)
    for _ in range(3):
        for n, fn in runs.items():
            got[n].append(timed(fn)[0] / 5 * 1e3)
    far = d_k > 0
    line = {"config": f"domain {N}x{N} R={len(dom)} Mx={Mx}", "C": N, "A": N, "R": len(dom), "Mx": Mx, "radius": float(radius),
            "inside": int(mask_k.count()), "torch_cdist_min_ms": spread(t_torch), "screen_domain_mask_ms": spread(t_mask),
            "domain_grid_ms": spread(t_grid),
            "speedup_mask": round(statistics.median(t_torch) / statistics.median(t_mask), 2),
            "speedup_grid": round(statistics.median(t_torch) / statistics.median(t_grid), 2),
            "launch_us": {n: spread(x) for n, x in got.items()},
            "kernel_lane_ops_per_s": round(N * N * 2.0 * len(dom) * Mx / (statistics.median(got["domain_grid"]) * 1e-6), 0),
            "torch_max_rel_diff": float(np.max(np.abs(d_t[far] - d_k[far]) / d_k[far])),
            "torch_max_at_training_pairs": float(d_t[dom.cation, dom.anion].max()),
            "kernel_max_at_training_pairs": float(d_k[dom.cation, dom.anion].max()),
            "torch_nearest_differs": int((n_t != n_k).sum()),
            "torch_mask_bits_differ": int((mask_t.to_bool() != mask_k.to_bool()).sum())}
    print(json.dumps(line), flush=True)
    lines.append(line)
elif args.pareto:
    from ionic_mpnn_amd import Objective, screen_pareto
    N = args.size
    v = MM.build_model(Va, Vb, atom_dim=32, num_steps=3, device=dev)
    v.load_weights(weights.init_weights("viscosity", Va, Vb, atom_dim=32, num_steps=3, seed=1, perturb=True))
    mp = MM.build_melting_point_model(Va, Vb, atom_dim=32, num_steps=3, device=dev)
    mp.load_weights(weights.init_weights("melting_point", Va, Vb, atom_dim=32, bond_dim=32 * 32, num_steps=3, seed=2, perturb=True))
    cat, _ = species(N, 1)
    _, an = species(N, 2)
    where_b = None if args.where is None else np.random.default_rng(5).random((N, N)) < float(args.where)
    where = None if where_b is None else data.PairMask.from_bool(where_b, device=dev)
    objectives = [Objective(v, T_ROOM), Objective(mp)]
    old_way = lambda: data.pareto_front(v.predict_grid(cat, an, T_ROOM)[:, :, 0], mp.predict_grid(cat, an), where=where_b)
    new_way = lambda: screen_pareto(objectives, cat, an, where=where)
    a, b = wall(old_way)[1], wall(new_way)[1]
    t_old, t_new = [], []
    for _ in range(3):
        t_old.append(wall(old_way)[0])
        t_new.append(wall(new_way)[0])
    # the stages alone, the two planes resident
    with torch.no_grad():
        f1 = torch.from_numpy(np.ascontiguousarray(v.predict_grid(cat, an, T_ROOM)[:, :, 0])).to(dev)
        f2 = torch.from_numpy(mp.predict_grid(cat, an)).to(dev)
    words = None if where is None else where.words
    filt = ops.ParetoFilter(N, (False, False), ops.PARETO_DEFAULT_CAPACITY, dev)
    stages = {"begin": filt.begin, "range": lambda: filt.range(f1, f2, words), "minima": lambda: filt.minima(f1, f2, words),
              "staircase": filt.staircase, "collect": lambda: filt.collect(f1, f2, words, 0)}
    for fn in stages.values():
        fn()
    _, _, _, count, competing = filt.candidates()
    stage_us = {n: [] for n in stages}
    for _ in range(3):
        for n, fn in stages.items():
            stage_us[n].append(timed(lambda: [fn() for _ in range(10)])[0] / 10 * 1e3)
    line = {"config": f"pareto visc x mp {N}x{N}" + ("" if where is None else " F=%g" % args.where), "C": N, "A": N,
            "bucket_bits": int(ops._lib.load().impnn_pareto_bucket_bits()), "competing": int(b.competing), "front": int(len(b.cation)),
            "candidates": int(count), "two_grids_plus_host_front_ms": spread(t_old), "screen_pareto_ms": spread(t_new),
            "speedup": round(statistics.median(t_old) / statistics.median(t_new), 2),
            "stage_launch_us": {n: spread(x) for n, x in stage_us.items()},
            "same_answer": bool(a.competing == b.competing and same_top(a[:3], b[:3]))}
    print(json.dumps(line), flush=True)
    lines.append(line)
elif args.mc:
    S, N, kappa = args.mc, args.size, 1.0
    t = build_transfer(32, 3)
    mcd = t.mc_dropout(S)
    cat, _ = species(N, 1)
    _, an = species(N, 2)
    where = None
    if args.where is not None:
        where = data.PairMask.from_bool(np.random.default_rng(0).random((N, N)) < args.where, device=dev)
    if args.select:
        plain = lambda: t.screen_top_k(cat, an, k=SELECT_K, where=where)
        sampled = lambda: mcd.screen_top_k(cat, an, k=SELECT_K, kappa=kappa, where=where)
    else:
        plain = lambda: t.predict_grid(cat, an)
        sampled = lambda: mcd.predict_grid(cat, an, kappa=kappa)
    wall(plain), wall(sampled)
    t_plain, t_mc = [], []
    for _ in range(5):
        t_plain.append(wall(plain)[0])
        t_mc.append(wall(sampled)[0])
    with torch.no_grad():
        pc, pa = t.encode_ions(cat, an)
        tensors, image = t._head_tensors(), t._transfer_image()
        uc = ops.transfer_ion_half("cat", pc, tensors, t.fp_size, t.mixing_size)
        ua = ops.transfer_ion_half("an", pa, tensors, t.fp_size, t.mixing_size)
        g1, g3 = ops.transfer_grid_operands(uc, ua, image), ops.transfer_mc_grid_operands(uc, ua, image, mcd.multipliers(), kappa)
        words = None if where is None else where.words
        if args.select:
            k_plain = lambda: [ops.grid_topk(g1, SELECT_K, where=words) for _ in range(10)]
            k_mc = lambda: [ops.grid_topk(g3, SELECT_K, where=words) for _ in range(10)]
        else:
            k_plain = lambda: [ops.grid_values(g1) for _ in range(10)]
            k_mc = lambda: [ops.grid_values(g3) for _ in range(10)]
        timed(k_plain), timed(k_mc)
        us_plain, us_mc = [], []
        for _ in range(5):
            us_plain.append(timed(k_plain)[0] / 10 * 1e3)
            us_mc.append(timed(k_mc)[0] / 10 * 1e3)
    ratio = statistics.median(us_mc) / statistics.median(us_plain)
    expect = (1024 + 256 * S) / 1280
    live = N * N if where is None or not args.select else None  # (a masked selection passes over empty tiles)
    mc_flop = 2 * (256 * 128 + S * (128 * 64 + 64))
    line = {"config": f"mc S={S} {N}x{N}" + (" select" if args.select else "") + (f" where {args.where}" if where is not None else ""),
            "samples": S, "C": N, "A": N, "deterministic_ms": spread(t_plain), "mc_dropout_ms": spread(t_mc),
            "wall_ratio": round(statistics.median(t_mc) / statistics.median(t_plain), 2),
            "deterministic_launch_us": spread(us_plain), "mc_launch_us": spread(us_mc), "launch_ratio": round(ratio, 2),
            "mfma_count_ratio": round(expect, 2), "launch_ratio_over_expected": round(ratio / expect, 2)}
    if live is not None:
        line["deterministic_of_f32_mfma_peak"] = round(live * PAIR_FLOP / (statistics.median(us_plain) * 1e-6) / MFMA_F32_PEAK, 3)
        line["mc_of_f32_mfma_peak"] = round(live * mc_flop / (statistics.median(us_mc) * 1e-6) / MFMA_F32_PEAK, 3)
    print(json.dumps(line), flush=True)
    lines.append(line)
elif args.ensemble:
    from ionic_mpnn_amd import ModelEnsemble
    M, N, kappa = args.ensemble, args.size, 1.0
    members = []
    for i in range(M):
        m = MM.build_model(Va, Vb, atom_dim=32, num_steps=3, device=dev)
        m.load_weights(weights.init_weights("viscosity", Va, Vb, atom_dim=32, num_steps=3, seed=1 + i, perturb=True))
        members.append(m)
    ens = ModelEnsemble(members)
    cat, _ = species(N, 1)
    _, an = species(N, 2)
    where = None
    if args.where is not None:
        where = data.PairMask.from_bool(np.random.default_rng(0).random((N, N)) < args.where, device=dev)

    def old_way():
        stats = data.ensemble_grid_stats(np.stack([m.predict_grid(cat, an, T_ROOM) for m in members]), kappa)
        return data.grid_top_k(stats[2], 100, False, where) if args.select else stats

    def new_way():
        if args.select:
            return ens.screen_top_k(cat, an, T_ROOM, k=100, kappa=kappa, where=where)
        return ens.predict_grid(cat, an, T_ROOM, kappa=kappa)

    a, b = wall(old_way)[1], wall(new_way)[1]
    t_old, t_new = [], []
    for _ in range(3):
        t_old.append(wall(old_way)[0])
        t_new.append(wall(new_way)[0])
    line = {"config": f"ensemble M={M} {N}x{N}x1" + (" select" if args.select else "") +
            (f" where {args.where}" if where is not None else ""), "members_grids_host_ms": spread(t_old),
            "ensemble_ms": spread(t_new), "speedup": round(statistics.median(t_old) / statistics.median(t_new), 2),
            "same_answer": same_top(a, b)}
    print(json.dumps(line), flush=True)
    lines.append(line)
elif args.rank:
    todo = [c for c in SELECT_CONFIGS if args.only in (None, c[0]) and (args.all_configs or c[1] in RANK_CONFIGS)]
    for kind, name, D, S, C, A, nT in todo[:1] if args.quick else todo:
        if kind == "viscosity":
            m = MM.build_model(Va, Vb, atom_dim=D, num_steps=S, device=dev)
            m.load_weights(weights.init_weights("viscosity", Va, Vb, atom_dim=D, num_steps=S, seed=1, perturb=True))
            T = np.linspace(263.15, 393.15, nT).astype(np.float32)
        else:
            m, T = build_transfer(D, S), None
        cat, _ = species(C, 1)
        _, an = species(A, 2)
        where_b = None if args.where is None else np.random.default_rng(5).random((C, A)) < float(args.where)
        where = None if where_b is None else data.PairMask.from_bool(where_b, device=dev)
        k = max((C * A if where is None else where.count()) // 100, 1)
        old_way = lambda: data.PairMask.from_bool(data.grid_best_mask(m.predict_grid(cat, an, T), k, where=where_b))
        new_way = lambda: m.screen_best_mask(cat, an, T, k=k, where=where)
        _, best_old = wall(old_way)
        _, best_new = wall(new_way)
        t_old, t_new = [], []
        for _ in range(3):
            t_old.append(wall(old_way)[0])
            t_new.append(wall(new_way)[0])
        words = None if where is None else where.words
        with torch.no_grad():
            pc, pa = m.encode_ions(cat, an)
            if kind == "viscosity":
                w = m._packed_head()
                mc = ops.head_ion_mix(kind, "cat", pc, w, m.fp_size, m.mixing_size)
                ma = ops.head_ion_mix(kind, "an", pa, w, m.fp_size, m.mixing_size)
                Td = torch.from_numpy(T).to(dev)
                store = lambda: [ops.head_grid(kind, mc, ma, Td, w, m.fp_size, m.mixing_size) for _ in range(10)]
                rank = lambda mask: [ops.head_grid_rank(kind, mc, ma, Td[t0:t0 + ops.SELECT_MAX_T], w, m.fp_size, m.mixing_size, k,
                                                        where=words, mask=mask)
                                     for _ in range(10) for t0 in range(0, nT, ops.SELECT_MAX_T)]
            else:
                tensors, image = m._head_tensors(), m._transfer_image()
                uc = ops.transfer_ion_half("cat", pc, tensors, m.fp_size, m.mixing_size)
                ua = ops.transfer_ion_half("an", pa, tensors, m.fp_size, m.mixing_size)
                store = lambda: [ops.transfer_head_grid(uc, ua, image) for _ in range(10)]
                rank = lambda mask: [ops.transfer_head_grid_rank(uc, ua, image, k, where=words, mask=mask) for _ in range(10)]
            timed(store), timed(lambda: rank(True)), timed(lambda: rank(False))
            k_store, k_rank, k_cut = [], [], []
            for _ in range(3):
                k_store.append(timed(store)[0] / 10 * 1e3)
                k_rank.append(timed(lambda: rank(True))[0] / 10 * 1e3)
                k_cut.append(timed(lambda: rank(False))[0] / 10 * 1e3)
        passes = ops.rank_passes(C, A)
        calls = (max(nT, 1) + ops.SELECT_MAX_T - 1) // ops.SELECT_MAX_T if kind == "viscosity" else 1
        line = {"config": "rank " + name + ("" if args.where is None else " F=%g" % args.where), "kind": kind, "atom_dim": D,
                "steps": S, "C": C, "A": A, "nT": nT, "k": int(k), "values": C * A * max(nT, 1), "passes": passes,
                "mask_density": None if where is None else round(where.count() / (C * A), 4),
                "predict_grid_plus_host_best_mask_ms": spread(t_old), "screen_best_mask_ms": spread(t_new),
                "speedup": round(statistics.median(t_old) / statistics.median(t_new), 2),
                "materialising_launch_us": spread(k_store), "rank_launches_us": spread(k_rank), "rank_cut_launches_us": spread(k_cut),
                "per_pass_over_materialising": round(statistics.median(k_cut) / (passes * calls * statistics.median(k_store)), 3),
                "mask_launch_us": round(statistics.median(k_rank) - statistics.median(k_cut), 2),
                "same_answer": bool(np.array_equal(best_old.words.numpy(), best_new.words.cpu().numpy()))}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del m
        torch.cuda.empty_cache()
elif args.partners:
    todo = [c for c in SELECT_CONFIGS if args.only in (None, c[0])]
    for kind, name, D, S, C, A, nT in todo[:1] if args.quick else todo:
        if kind == "viscosity":
            m = MM.build_model(Va, Vb, atom_dim=D, num_steps=S, device=dev)
            m.load_weights(weights.init_weights("viscosity", Va, Vb, atom_dim=D, num_steps=S, seed=1, perturb=True))
            T = np.linspace(263.15, 393.15, nT).astype(np.float32)
        else:
            m, T = build_transfer(D, S), None
        cat, _ = species(C, 1)
        _, an = species(A, 2)
        where_b = None if args.where is None else np.random.default_rng(5).random((C, A)) < float(args.where)
        where = None if where_b is None else data.PairMask.from_bool(where_b, device=dev)
        old_way = lambda: data.grid_best_partners(m.predict_grid(cat, an, T), PARTNERS_M, where=where_b)
        new_way = lambda: m.screen_best_partners(cat, an, T, m=PARTNERS_M, where=where)
        _, best_old = wall(old_way)
        _, best_new = wall(new_way)
        t_old, t_new = [], []
        for _ in range(3):
            t_old.append(wall(old_way)[0])
            t_new.append(wall(new_way)[0])
        words = None if where is None else where.words
        with torch.no_grad():
            pc, pa = m.encode_ions(cat, an)
            if kind == "viscosity":
                w = m._packed_head()
                mc = ops.head_ion_mix(kind, "cat", pc, w, m.fp_size, m.mixing_size)
                ma = ops.head_ion_mix(kind, "an", pa, w, m.fp_size, m.mixing_size)
                Td = torch.from_numpy(T).to(dev)
                store = lambda: [ops.head_grid(kind, mc, ma, Td, w, m.fp_size, m.mixing_size) for _ in range(10)]
                select = lambda: [ops.head_grid_partners(kind, mc, ma, Td[t0:t0 + ops.SELECT_MAX_T], w, m.fp_size, m.mixing_size,
                                                         PARTNERS_M, where=words)
                                  for _ in range(10) for t0 in range(0, nT, ops.SELECT_MAX_T)]
            else:
                tensors, image = m._head_tensors(), m._transfer_image()
                uc = ops.transfer_ion_half("cat", pc, tensors, m.fp_size, m.mixing_size)
                ua = ops.transfer_ion_half("an", pa, tensors, m.fp_size, m.mixing_size)
                store = lambda: [ops.transfer_head_grid(uc, ua, image) for _ in range(10)]
                select = lambda: [ops.transfer_head_grid_partners(uc, ua, image, PARTNERS_M, where=words) for _ in range(10)]
            timed(store), timed(select)
            k_store, k_select = [], []
            for _ in range(3):
                k_store.append(timed(store)[0] / 10 * 1e3)
                k_select.append(timed(select)[0] / 10 * 1e3)
        line = {"config": "partners " + name + ("" if args.where is None else " F=%g" % args.where), "kind": kind, "atom_dim": D,
                "steps": S, "C": C, "A": A, "nT": nT, "m": PARTNERS_M, "values": C * A * max(nT, 1),
                "mask_density": None if where is None else round(where.count() / (C * A), 4),
                "predict_grid_plus_host_best_partners_ms": spread(t_old), "screen_best_partners_ms": spread(t_new),
                "speedup": round(statistics.median(t_old) / statistics.median(t_new), 2),
                "materialising_launch_us": spread(k_store), "partner_launches_us": spread(k_select),
                "partners_over_materialising": round(statistics.median(k_select) / statistics.median(k_store), 3),
                "same_answer": same_partners(best_old, best_new)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del m
        torch.cuda.empty_cache()
elif args.select and args.where is not None:
    F = float(args.where)
    for name, D, S, C, A in WHERE_CONFIGS[:1] if args.quick else WHERE_CONFIGS:
        m = MM.build_model(Va, Vb, atom_dim=D, num_steps=S, device=dev)
        m.load_weights(weights.init_weights("viscosity", Va, Vb, atom_dim=D, num_steps=S, seed=1, perturb=True))
        mp = MM.build_melting_point_model(Va, Vb, atom_dim=D, num_steps=S, device=dev)
        mp.load_weights(weights.init_weights("melting_point", Va, Vb, atom_dim=D, bond_dim=D * D, num_steps=S, seed=2, perturb=True))
        t = build_transfer(D, S)
        cat, _ = species(C, 1)
        _, an = species(A, 2)
        limit = np.float32(np.quantile(mp.predict_grid(cat, an), F))
        new_mask = lambda: mp.screen_mask(cat, an, at_most=limit)
        new_way = lambda: m.screen_top_k(cat, an, T_ROOM, k=SELECT_K, where=new_mask())
        old_way = lambda: data.grid_top_k(m.predict_grid(cat, an, T_ROOM), SELECT_K, where=mp.predict_grid(cat, an) <= limit)
        _, liquid = wall(new_mask)
        new_top = lambda: m.screen_top_k(cat, an, T_ROOM, k=SELECT_K, where=liquid)
        _, top_old = wall(old_way)
        _, top_new = wall(new_way)
        wall(new_top)
        t_old, t_new, t_mask, t_top = [], [], [], []
        for _ in range(3):
            t_old.append(wall(old_way)[0])
            t_new.append(wall(new_way)[0])
            t_mask.append(wall(new_mask)[0])
            t_top.append(wall(new_top)[0])
        line = {"config": name + " F=%g" % F, "atom_dim": D, "steps": S, "C": C, "A": A, "k": SELECT_K, "fraction": F,
                "mask_density": round(liquid.count() / (C * A), 4),
                "two_grids_plus_host_top_k_ms": spread(t_old), "screen_mask_plus_top_k_where_ms": spread(t_new),
                "speedup": round(statistics.median(t_old) / statistics.median(t_new), 2),
                "screen_mask_ms": spread(t_mask), "screen_top_k_where_ms": spread(t_top), "same_answer": same_top(top_old, top_new)}
        # the launches alone
        rng = np.random.default_rng(5)
        with torch.no_grad():
            pc, pa = m.encode_ions(cat, an)
            w = m._packed_head()
            mc = ops.head_ion_mix("viscosity", "cat", pc, w, m.fp_size, m.mixing_size)
            ma = ops.head_ion_mix("viscosity", "an", pa, w, m.fp_size, m.mixing_size)
            Td = torch.from_numpy(T_ROOM).to(dev)
            tensors, image = t._head_tensors(), t._transfer_image()
            tpc, tpa = t.encode_ions(cat, an)
            uc = ops.transfer_ion_half("cat", tpc, tensors, t.fp_size, t.mixing_size)
            ua = ops.transfer_ion_half("an", tpa, tensors, t.fp_size, t.mixing_size)
            for fam, tile, topk, grid, mask in (
                    ("head", (16, 64), lambda wh: ops.head_grid_topk("viscosity", mc, ma, Td, w, m.fp_size, m.mixing_size, SELECT_K, where=wh),
                     lambda: ops.head_grid("viscosity", mc, ma, Td, w, m.fp_size, m.mixing_size),
                     lambda: ops.head_grid_mask("viscosity", mc, ma, Td, w, m.fp_size, m.mixing_size, -np.inf, 0.0)),
                    ("transfer", (8, 32), lambda wh: ops.transfer_head_grid_topk(uc, ua, image, SELECT_K, where=wh),
                     lambda: ops.transfer_head_grid(uc, ua, image), lambda: ops.transfer_head_grid_mask(uc, ua, image, -np.inf, 0.0))):
                masks = {"plain": None, "ones": data.PairMask.from_bool(np.ones((C, A), bool), device=dev).words,
                         "random": data.PairMask.from_bool(rng.random((C, A)) < F, device=dev).words,
                         "block": data.PairMask.from_bool(block_mask(C, A, tile, F, rng), device=dev).words}
                runs = {n: (lambda wh=wh: [topk(wh) for _ in range(10)]) for n, wh in masks.items()}
                runs["materialise"] = lambda: [grid() for _ in range(10)]
                runs["mask"] = lambda: [mask() for _ in range(10)]
                got = {n: [] for n in runs}
                for fn in runs.values():
                    timed(fn)
                for _ in range(5):
                    for n, fn in runs.items():
                        got[n].append(timed(fn)[0] / 10 * 1e3)
                line[fam + "_launch_us"] = {n: spread(x) for n, x in got.items()}
                line[fam + "_block_density"] = round(data.PairMask(masks["block"], (C, A)).count() / (C * A), 4)
        print(json.dumps(line), flush=True)
        lines.append(line)
        del m, mp, t
        torch.cuda.empty_cache()
elif args.select:
    todo = [c for c in SELECT_CONFIGS if args.only in (None, c[0])]
    for kind, name, D, S, C, A, nT in todo[:1] if args.quick else todo:
        if kind == "viscosity":
            m = MM.build_model(Va, Vb, atom_dim=D, num_steps=S, device=dev)
            m.load_weights(weights.init_weights("viscosity", Va, Vb, atom_dim=D, num_steps=S, seed=1, perturb=True))
            T = np.linspace(263.15, 393.15, nT).astype(np.float32)
        else:
            m, T = build_transfer(D, S), None
        cat, _ = species(C, 1)
        _, an = species(A, 2)
        old_way = lambda: data.grid_top_k(m.predict_grid(cat, an, T), SELECT_K)
        new_way = lambda: m.screen_top_k(cat, an, T, k=SELECT_K)
        _, top_old = wall(old_way)
        _, top_new = wall(new_way)
        t_old, t_new = [], []
        for _ in range(3):
            t_old.append(wall(old_way)[0])
            t_new.append(wall(new_way)[0])
        with torch.no_grad():
            pc, pa = m.encode_ions(cat, an)
            if kind == "viscosity":
                w = m._packed_head()
                mc = ops.head_ion_mix(kind, "cat", pc, w, m.fp_size, m.mixing_size)
                ma = ops.head_ion_mix(kind, "an", pa, w, m.fp_size, m.mixing_size)
                Td = torch.from_numpy(T).to(dev)
                store = lambda: [ops.head_grid(kind, mc, ma, Td, w, m.fp_size, m.mixing_size) for _ in range(10)]
                select = lambda: [ops.head_grid_topk(kind, mc, ma, Td[t0:t0 + ops.SELECT_MAX_T], w, m.fp_size, m.mixing_size,
                                                     SELECT_K) for _ in range(10) for t0 in range(0, nT, ops.SELECT_MAX_T)]
            else:
                tensors, image = m._head_tensors(), m._transfer_image()
                uc = ops.transfer_ion_half("cat", pc, tensors, m.fp_size, m.mixing_size)
                ua = ops.transfer_ion_half("an", pa, tensors, m.fp_size, m.mixing_size)
                store = lambda: [ops.transfer_head_grid(uc, ua, image) for _ in range(10)]
                select = lambda: [ops.transfer_head_grid_topk(uc, ua, image, SELECT_K) for _ in range(10)]
            timed(store), timed(select)
            k_store, k_select = [], []
            for _ in range(3):
                k_store.append(timed(store)[0] / 10)
                k_select.append(timed(select)[0] / 10)
        ms_old, ms_new = statistics.median(t_old), statistics.median(t_new)
        us_store, us_select = statistics.median(k_store) * 1e3, statistics.median(k_select) * 1e3
        line = {"config": "select " + name, "kind": kind, "atom_dim": D, "steps": S, "C": C, "A": A, "nT": nT, "k": SELECT_K,
                "values": C * A * max(nT, 1), "predict_grid_plus_host_top_k_ms": round(ms_old, 3),
                "screen_top_k_ms": round(ms_new, 3), "speedup": round(ms_old / ms_new, 2),
                "rounds_old_ms": [round(x, 3) for x in t_old], "rounds_new_ms": [round(x, 3) for x in t_new],
                "materialising_launch_us": round(us_store, 2), "selecting_launches_us": round(us_select, 2),
                "selecting_over_materialising": round(us_select / us_store, 3),
                "rounds_materialising_us": [round(x * 1e3, 2) for x in k_store],
                "rounds_selecting_us": [round(x * 1e3, 2) for x in k_select], "same_answer": same_top(top_old, top_new)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del m
        torch.cuda.empty_cache()

Path(args.out).parent.mkdir(parents=True, exist_ok=True)
with open(args.out, "a") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
