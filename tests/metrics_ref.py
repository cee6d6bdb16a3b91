"""Cases, bounds and the tiny models of the regression-metric tests (tests/test_metrics_host.py on the CPU,
tests/test_gpu_metrics.py on the GPU, tests/golden/make_metrics_golden.py for the recorded parent run).

The record (include/impnn.h, impnn_regression_sums; train.regression_sums_reference is the definition): per segment
    0 samples | 1 sum w | 2 sum w e | 3 sum w |e| | 4 sum w e^2 | 5 sum w yr | 6 sum w yr^2 | 7 max |e| over w > 0
with e = scale * (pred - y), yr = offset + scale * y, everything in fp64.

Bound per word of a segment of n_s samples, kernel against reference on the same float32 arrays:
    (n_s + 4) * 2^-52 * sum |term|
Both sides add the same fp64 terms and differ in the order only: each is off by at most (n_s - 1) * 2^-53 * sum |term|
from the exact sum; the + 4 covers a term whose product a compiler contracted into the add.  Words 0 and 7 are equal
exactly (a count, and a maximum of values that no addition touched)."""
import numpy as np

SCALE, OFFSET = 37.5, 310.0            # a standardised melting point back to kelvin
ONE_SEGMENT_N = (1, 63, 64, 65, 255, 256, 257, 4097, 16384, 16385)   # every path of one segment below the large one
LARGE_N = 300_000
SEGMENT_LENGTHS = (0, 1, 2, 63, 64, 65, 300, 1500)
N_SEGMENTS = 37
LONG_SEGMENTS = (1500, 0, 700)         # mean length above 512: a workgroup per segment
EPS = 2.0 ** -52

TINY = dict(Va=11, Vb=6, D=16, K=4, F=12, Mx=10, N=10, E=16)
N_SAMPLES, BATCH = 70, 24              # two captured batches and a ragged one of 22 that runs eagerly
GOLDEN = "metrics_parent_fit.npz"


def arrays(n, seed, nan_at=None):
    """(pred, y, w) float32: standardised targets, predictions near them, bootstrap-like weights with zeros."""
    rng = np.random.default_rng(seed)
    y = rng.normal(0.0, 1.0, size=n).astype(np.float32)
    pred = (y + rng.normal(0.0, 0.3, size=n)).astype(np.float32)
    w = rng.poisson(1.0, size=n).astype(np.float32)
    if nan_at is not None:
        pred[nan_at] = np.nan
        w[nan_at] = 1.0
    return pred, y, w


def term_abs_sums(pred, y, w, idx, scale, offset):
    """sum |term| of the words 1..6 over the samples ``idx`` (fp64): what the bound scales with."""
    p, t = pred[idx].astype(np.float64), y[idx].astype(np.float64)
    ww = np.ones(len(idx)) if w is None else w[idx].astype(np.float64)
    e = scale * (p - t)
    yr = offset + scale * t
    return np.array([np.abs(ww).sum(), np.abs(ww * e).sum(), np.abs(ww * np.abs(e)).sum(), np.abs(ww * (e * e)).sum(),
                     np.abs(ww * yr).sum(), np.abs(ww * (yr * yr)).sum()])


def check_record(got, ref, pred, y, w, segments, scale, offset, what=""):
    """``got`` (kernel) against ``ref`` (train.regression_sums_reference), both (n_seg, 8); ``segments``: per segment
    the sample indices in summation order.  Words 0 and 7 exactly, words 1..6 within (n_s + 4) 2^-52 sum |term|; a NaN
    where, and only where, the reference has one."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape == (len(segments), 8), (what, got.shape, ref.shape)
    for s, idx in enumerate(segments):
        idx = np.asarray(idx, np.int64)
        assert np.array_equal(got[s, [0, 7]], ref[s, [0, 7]], equal_nan=True), (what, s, got[s], ref[s])
        assert np.array_equal(np.isnan(got[s]), np.isnan(ref[s])), (what, s, got[s], ref[s])
        with np.errstate(invalid="ignore"):
            bound = (len(idx) + 4) * EPS * term_abs_sums(pred, y, w, idx, scale, offset)
        for k in range(1, 7):
            if np.isnan(ref[s, k]):
                continue
            err = abs(got[s, k] - ref[s, k])
            assert err <= bound[k - 1], f"{what} segment {s} word {k}: |{got[s, k]!r} - {ref[s, k]!r}| = {err:.3e} > {bound[k - 1]:.3e}"


def segmented_case(lengths, seed):
    """Segments of the given lengths under a random permutation -> (order int32, seg_offsets int64, groups): ``groups``
    labels every sample with its segment, so that a stable argsort of it is NOT ``order`` in general - the reference
    is given the segments' index lists directly."""
    rng = np.random.default_rng(seed)
    n = int(np.sum(lengths))
    order = rng.permutation(n).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    segments = [order[off[s]:off[s + 1]].astype(np.int64) for s in range(len(lengths))]
    return order, off, segments


def drawn_lengths(seed=37):
    rng = np.random.default_rng(seed)
    ls = list(SEGMENT_LENGTHS) + list(rng.choice(SEGMENT_LENGTHS, size=N_SEGMENTS - len(SEGMENT_LENGTHS)))
    return [int(v) for v in rng.permutation(ls)]


# ---- the tiny models -------------------------------------------------------------------------------------------------
def tiny_viscosity(device="cuda", seed=5):
    """The tiny viscosity model of tests/test_gpu_train.py (perturbed weights) and a 70-sample set."""
    from ionic_mpnn_amd import layers as L, model as MM, synthetic, weights
    t = TINY
    L.reset_uids()
    w = weights.init_weights("viscosity", t["Va"], t["Vb"], atom_dim=t["D"], bond_dim=t["K"], fp_size=t["F"],
                             mixing_size=t["Mx"], num_steps=2, seed=seed, perturb=True)
    m = MM.build_model(t["Va"], t["Vb"], atom_dim=t["D"], bond_dim=t["K"], fp_size=t["F"], mixing_size=t["Mx"],
                       num_steps=2, device=device)
    m.load_weights(w)
    x, y = tiny_set(seed)
    return m, x, y


def tiny_set(seed=5, n=N_SAMPLES):
    from ionic_mpnn_amd import synthetic
    t = TINY
    x = synthetic.make_batch(n, max_atoms=t["N"], max_edges=t["E"], atom_vocab_size=t["Va"], bond_vocab_size=t["Vb"],
                             min_atoms=3, seed=seed)
    y = np.random.default_rng(seed).normal(1.0, 0.5, size=n).astype(np.float32)
    return x, y


PARENT_RUNS = [(f"{g}_{w}", g == "graph", w == "weighted") for g in ("graph", "eager") for w in ("plain", "weighted")]


def parent_fit(graph, weighted=False):
    """The run whose loss history and final weights tests/golden/metrics_parent_fit.npz holds: the tiny viscosity
    model compiled WITHOUT metrics, 3 epochs (a fresh shuffle each), batch 24 of 70 samples, seed 0, with or without
    bootstrap sample weights - at learning rate 0.  Every step still runs its forward, loss, backward and optimizer
    launches, captured or eager, but the weights stay, so the run is a function of the forward and loss kernels
    alone, which add in a fixed order: it repeats its bits.  At any other rate it does not, on any commit: the
    backward kernels add gradients with float atomics (embedding rows, per-type matrices, head weights across
    workgroups), the sums differ in the last bits from run to run, and Adam carries that into every weight."""
    from ionic_mpnn_amd import data, train
    m, x, y = tiny_viscosity()
    m.compile(train.Adam(0.0, clipnorm=1.0))
    sw = data.bootstrap_weights(N_SAMPLES, 0) if weighted else None
    h = m.fit(x, y, epochs=3, batch_size=BATCH, seed=0, graph=graph, sample_weight=sw)
    return np.asarray(h.history["loss"], np.float64), m.state_dict()


def metric_tolerances(pred, y, w, scale, offset, epsilon=1e-6):
    """The record bound carried to the metrics, for records added up over all of (pred, y, w) in any order: a word is
    off by at most d_k = (n + 4) 2^-52 sum |term_k| on each side.  Means divide by sum w (the weights used here are
    small integers: that sum is exact), a square root halves a relative error, R^2 = 1 - A / D with
    D = S6 - S5^2 / S1 + epsilon moves by (A / D) (d_4 / A + d_D / D), d_D <= d_6 + 2 |S5| d_5 / S1; a few 2^-52 of
    the value are added for the divisions and the root.  The maximum is exact."""
    n = len(pred)
    idx = np.arange(n)
    d = (n + 4) * EPS * term_abs_sums(pred, y, w, idx, scale, offset)   # words 1..6
    p, t = pred.astype(np.float64), y.astype(np.float64)
    ww = np.ones(n) if w is None else w.astype(np.float64)
    e, yr, s1 = scale * (p - t), offset + scale * t, ww.sum()
    A, S5, S6 = (ww * e * e).sum(), (ww * yr).sum(), (ww * yr * yr).sum()
    D = S6 - S5 * S5 / s1 + epsilon
    dD = d[5] + 2 * abs(S5) * d[4] / s1 + 4 * EPS * S6
    mse = A / s1
    return {"mae": d[2] / s1 + 4 * EPS * (ww * np.abs(e)).sum() / s1, "mse": d[3] / s1 + 4 * EPS * mse,
            "rmse": (d[3] / s1 + 8 * EPS * mse) / (2 * np.sqrt(mse)), "bias": d[1] / s1 + 4 * EPS * abs((ww * e).sum()) / s1,
            "max_error": 0.0, "r2": (A / D) * (d[3] / A + dD / D) + 8 * EPS * max(1.0, A / D)}
