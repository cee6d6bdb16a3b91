"""Monte-Carlo dropout of the transfer head (ionic_mpnn_amd/mc_dropout.py, csrc/transfer_mc_grid.hip), on the host: the
argument errors of ``MPNNModel.mc_dropout`` and of the screens it returns, the refusals of the operations the family
does not have, the status codes of the C entries on stand-in pointers (every row returns before a launch), and the
statistic of hand-written samples through ``data.ensemble_grid_stats`` - the host reference of the kernel's statistic -
for S = 1 and for S = 33, longer than the ensemble's 8.  And the preconditions of the GPU tests' case
(tests/mc_dropout_cases.py), from references that do not touch the kernels: a plain float32 walk of every sample plane
stays at or below half of the 1e-5 bound, and the fp64 spread exceeds 1e-3 of max|mean| on at least 90 % of the pairs."""
import ctypes as C

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import McDropout, _lib, data, model as MM, ops

import ensemble_cases as E
import mc_dropout_cases as K
from test_transfer_grid_host import closeness

CPU = torch.device("cpu")


def _transfer(**kw):
    return MM.MPNNModel("transfer", E.VA, E.VB, kw.pop("atom_dim", 32), 8, kw.pop("fp_size", 32), 20, 1, 1e-4, device=CPU, **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- Python-side errors
def test_mc_dropout_construction_errors():
    most = _lib.load().impnn_transfer_mc_grid_max_samples()
    assert most >= 32
    t = _transfer()
    mc = t.mc_dropout()
    assert isinstance(mc, McDropout) and (mc.samples, mc.draw, len(mc)) == (32, 0, 32) and mc.model is t
    assert t.mc_dropout(1).samples == 1 and t.mc_dropout(most, draw=7).draw == 7
    for kind, build in (("viscosity", lambda: MM.build_model(E.VA, E.VB, num_steps=1, device=CPU)),
                        ("melting_point", lambda: MM.build_melting_point_model(E.VA, E.VB, num_steps=1, device=CPU))):
        with pytest.raises(ValueError, match=f"a {kind} model has no head Dropout"):
            build().mc_dropout()
    with pytest.raises(ValueError, match="do not cover atom_dim 32, fp_size 96"):
        _transfer(fp_size=96).mc_dropout()
    for bad in (0, -1, most + 1, 2.5, True):
        with pytest.raises(ValueError, match=f"samples must be an integer from 1 to {most}"):
            t.mc_dropout(bad)
    for bad in (-1, 0.5):
        with pytest.raises(ValueError, match="draw must be a non-negative integer"):
            t.mc_dropout(4, draw=bad)


def test_mc_dropout_argument_errors():
    cat, an = E.species(2, 3)
    mc = _transfer().mc_dropout(4)
    with pytest.raises(ValueError, match="both"):
        mc.screen_top_k(cat, None)
    for kappa in (float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="kappa must be finite"):
            mc.predict_grid(cat, an, kappa=kappa)
        with pytest.raises(ValueError, match="kappa must be finite"):
            mc.screen_mask(cat, an, at_most=0.0, kappa=kappa)
    with pytest.raises(ValueError, match="k must be"):
        mc.screen_top_k(cat, an, k=0)
    with pytest.raises(ValueError, match="needs a bound"):
        mc.screen_mask(cat, an)
    with pytest.raises(ValueError, match="bound is NaN"):
        mc.screen_mask(cat, an, at_least=float("nan"))
    with pytest.raises(TypeError, match="PairMask"):
        mc.screen_top_k(cat, an, where=np.ones((2, 3), bool))
    with pytest.raises(ValueError, match="max_pairs_per_launch"):
        mc.predict_grid(cat, an, max_pairs_per_launch=0)
    with pytest.raises(ValueError, match="differ in length"):
        mc.predict_pairs(cat, an, [0, 1], [0])
    # nothing here computes on the CPU
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mc.predict_grid(cat, an)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mc.screen_top_k(cat, an, k=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.transfer_mc_grid_operands(torch.zeros(2, 256), torch.zeros(3, 256), torch.zeros(41732), torch.ones(4, 128))


def test_partners_and_rank_refuse_a_transfer_mc_grid_before_any_library_call():
    g = ops.GridOperands(3, 1, torch.zeros(3, 256), torch.zeros(4, 256), None, torch.zeros(41732), (), 0.5, torch.ones(7, 128))
    assert (g.family, g.kind, g.samples, g.members, g.C, g.A, g.nT, g.D, g.kappa) == (3, 1, 7, 1, 3, 4, 0, None, 0.5)
    assert g.trail == (3, 4) and g.lead[3] == 41732 and g.lead[-2:] == (7, 0.5) and len(g.lead) == 7
    narrowed = g.rows(1, 3)
    assert narrowed.C == 2 and narrowed.samples == 7 and narrowed.multipliers is g.multipliers and narrowed.kappa == 0.5
    assert g.temperatures(0, 1) is g
    for call in (lambda: ops.grid_partners(g), lambda: ops.grid_rank(g, 3), lambda: ops.grid_rank(g, 3, mask=True)):
        with pytest.raises(NotImplementedError, match="transfer MC grids: partners / rank are not built"):
            call()
    # the ensemble's pinned refusal stays as it is
    e = ops.GridOperands(2, 0, torch.zeros(2, 3, 20), torch.zeros(2, 4, 20), torch.zeros(1), torch.zeros(2, 63), (32, 20), 0.5)
    with pytest.raises(NotImplementedError, match="ensemble grids: partners / rank are not built"):
        ops.grid_partners(e)
    with pytest.raises(ValueError, match="takes the operands of transfer_mc_grid_operands"):
        ops.transfer_mc_grid(e)


# ---------------------------------------------------------------- status codes
_A = 0x100000  # a 16-byte aligned stand-in
_M = 0x100004  # a misaligned one
OK, BADARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4


def _call(fn, names, defaults):
    return lambda **k: fn(*[{**defaults, **k}[a] for a in names])


def test_status_codes_are_pinned():
    lib = _lib.load()
    n, most = lib.impnn_transfer_grid_image_floats(), lib.impnn_transfer_mc_grid_max_samples()
    vp = C.c_void_p
    common = {"u_cat": vp(_A), "u_an": vp(_A), "image": vp(_A), "image_floats": n, "mult": vp(_A), "S": 8, "kappa": 1.0,
              "C": 3, "A": 4, "stream": None}
    grid = _call(lib.impnn_transfer_mc_grid, ("u_cat", "u_an", "image", "image_floats", "mult", "S", "kappa", "mean", "std",
                                              "score", "samples", "C", "A", "stream"),
                 {**common, "mean": vp(_M), "std": None, "score": None, "samples": None})
    mask = _call(lib.impnn_transfer_mc_grid_mask, ("u_cat", "u_an", "image", "image_floats", "mult", "S", "kappa", "lo", "hi",
                                                   "words", "C", "A", "stream"),
                 {**common, "lo": 0.0, "hi": 1.0, "words": vp(_M)})
    topk_names = ("u_cat", "u_an", "image", "image_floats", "mult", "S", "kappa", "k", "largest", "values", "cation", "anion",
                  "ws", "ws_bytes", "C", "A", "workgroups", "stream")
    topk_defaults = {**common, "k": 5, "largest": 0, "values": vp(_A), "cation": vp(_A), "anion": vp(_A), "ws": vp(_A),
                     "ws_bytes": 1 << 20, "workgroups": 0, "where": vp(_M)}
    topk = _call(lib.impnn_transfer_mc_grid_topk, topk_names, topk_defaults)
    topk_where = _call(lib.impnn_transfer_mc_grid_topk_where, topk_names[:7] + ("where",) + topk_names[7:], topk_defaults)
    cases = [
        # shape, then S and kappa
        (grid, dict(C=-1), BADARG, "impnn_transfer_mc_grid: bad shape"),
        (grid, dict(image_floats=-1, S=0), BADARG, "impnn_transfer_mc_grid: bad shape"),
        (grid, dict(S=0), BADARG, "impnn_transfer_mc_grid: S=0 samples must be at least 1"),
        (grid, dict(S=most + 1, C=0), UNSUPPORTED, f"impnn_transfer_mc_grid: S={most + 1} samples (<= {most} per call)"),
        (grid, dict(kappa=float("inf")), BADARG, "impnn_transfer_mc_grid: kappa must be finite"),
        (grid, dict(kappa=float("nan"), A=0), BADARG, "impnn_transfer_mc_grid: kappa must be finite"),
        # zero work comes before the pointers
        (grid, dict(C=0, mean=None, u_cat=None), OK, None),
        (grid, dict(A=0, image=None, mult=None, image_floats=0), OK, None),
        # null pointers, alignment, the image size
        (grid, dict(mean=None), BADARG, "impnn_transfer_mc_grid: null pointer"),
        (grid, dict(mult=None, image_floats=1), BADARG, "impnn_transfer_mc_grid: null pointer"),
        (grid, dict(u_an=vp(_M)), BADARG, "impnn_transfer_mc_grid: u rows and the image must be 16-byte aligned"),
        (grid, dict(mult=vp(_M)), BADARG, "impnn_transfer_mc_grid: the multipliers must be 16-byte aligned"),
        (grid, dict(image_floats=n - 1), WORKSPACE, f"impnn_transfer_mc_grid: image of {n - 1} floats is too small ({n})"),
        # the mask: shape; S and kappa; a NaN bound; zero work; null pointers; alignment
        (mask, dict(A=-1), BADARG, "impnn_transfer_mc_grid_mask: bad shape"),
        (mask, dict(S=-3, lo=float("nan")), BADARG, "impnn_transfer_mc_grid_mask: S=-3 samples must be at least 1"),
        (mask, dict(lo=float("nan"), C=0), BADARG, "impnn_transfer_mc_grid_mask: a bound is NaN (an infinity means no limit)"),
        (mask, dict(C=0, words=None), OK, None),
        (mask, dict(words=None), BADARG, "impnn_transfer_mc_grid_mask: null pointer"),
        (mask, dict(words=vp(0x100002)), BADARG, "impnn_transfer_mc_grid_mask: the mask must be 4-byte aligned"),
        (mask, dict(mult=vp(_M)), BADARG, "impnn_transfer_mc_grid_mask: the multipliers must be 16-byte aligned"),
        # top-k: shape; S and kappa; k, C * A; zero work; null pointers; alignment; the workspace size
        (topk, dict(workgroups=-1), BADARG, "impnn_transfer_mc_grid_topk: bad shape"),
        (topk, dict(S=most + 1, k=0), UNSUPPORTED, f"impnn_transfer_mc_grid_topk: S={most + 1} samples (<= {most} per call)"),
        (topk, dict(k=0), BADARG, "impnn_transfer_mc_grid_topk: k=0 must be at least 1"),
        (topk, dict(k=1025), UNSUPPORTED, "impnn_transfer_mc_grid_topk: k=1025 entries (<= 1024 per call)"),
        (topk, dict(C=1 << 16, A=1 << 16), UNSUPPORTED, None),
        (topk, dict(A=0, values=None), OK, None),
        (topk, dict(values=None), BADARG, "impnn_transfer_mc_grid_topk: null pointer"),
        (topk, dict(ws=vp(_M)), BADARG, "impnn_transfer_mc_grid_topk: the workspace must be 8-byte aligned"),
        (topk, dict(image=vp(_M)), BADARG, "impnn_transfer_mc_grid_topk: u rows and the image must be 16-byte aligned"),
        (topk, dict(ws_bytes=8), WORKSPACE, "impnn_transfer_mc_grid_topk: workspace of 8 bytes is too small (40)"),
        (topk_where, dict(where=None), BADARG, "impnn_transfer_mc_grid_topk_where: null pointer"),
        (topk_where, dict(where=vp(0x100002)), BADARG, "impnn_transfer_mc_grid_topk_where: the mask must be 4-byte aligned"),
        (topk_where, dict(kappa=float("-inf")), BADARG, "impnn_transfer_mc_grid_topk_where: kappa must be finite"),
    ]
    for fn, kw, code, text in cases:
        rc = fn(**kw)
        assert rc == code, (kw, rc, lib.impnn_last_error_string().decode())
        if text is not None:
            assert lib.impnn_last_error_string().decode() == text, kw
    # the workspace query: its own entry (the families' shared one does not serve this family)
    need = C.c_size_t(0)
    assert lib.impnn_transfer_mc_grid_topk_workspace_bytes(8, 3, 4, 5, 0, C.byref(need)) == OK and need.value == 40
    assert lib.impnn_transfer_mc_grid_topk_workspace_bytes(8, 9, 33, 5, 0, C.byref(need)) == OK and need.value == 4 * 40  # 2 x 2 tiles of 8 x 32
    assert lib.impnn_transfer_mc_grid_topk_workspace_bytes(8, 3, 4, 5, 0, None) == BADARG
    assert lib.impnn_transfer_mc_grid_topk_workspace_bytes(0, 3, 4, 5, 0, C.byref(need)) == BADARG
    assert lib.impnn_grid_topk_workspace_bytes(3, 3, 4, 0, 5, 0, C.byref(need)) == BADARG


# ---------------------------------------------------------------- the statistic (data.ensemble_grid_stats, any length)
def test_stats_of_one_sample():
    v = np.array([[1.5, -2.25, 3e-39, 7e37]], np.float32)
    for kappa in (0.0, 1.5, -1.0):
        mean, std, score = data.ensemble_grid_stats(v, kappa)
        assert np.array_equal(bits(mean), bits(v[0])) and np.array_equal(bits(score), bits(v[0]))
        assert np.array_equal(bits(std), bits(np.zeros(4, np.float32))), "S = 1: the spread is exactly +0"


def test_stats_of_33_samples_by_hand():
    """33 samples, more than the ensemble's 8: the float32 walk in the kernel's order, written out here."""
    rng = np.random.default_rng(33)
    v = rng.normal(2.0, 0.7, size=(33, 5)).astype(np.float32)
    v[:, 4] = np.arange(33, dtype=np.float32)  # exact: mean 16, q = 2 * (1 + 4 + ... + 256) = 2992
    f32 = np.float32
    for kappa in (0.0, 1.5, -1.0):
        mean, std, score = data.ensemble_grid_stats(v, kappa)
        for j in range(5):
            s = v[0, j]
            for i in range(1, 33):
                s = f32(s + v[i, j])
            m = f32(s / f32(33))
            q = np.float64(0.0)
            for i in range(33):
                d = f32(v[i, j] - m)
                q = np.float64(f32(np.float64(d) * np.float64(d) + q))  # fmaf: one rounding (the product of two float32 is exact in float64)
            sd = f32(np.sqrt(f32(f32(q) / f32(33))))
            sc = f32(np.float64(f32(kappa)) * np.float64(sd) + np.float64(m))
            assert (bits(mean)[j], bits(std)[j], bits(score)[j]) == (bits(m), bits(sd), bits(sc)), (j, kappa)
        assert mean[4] == 16.0 and bits(std)[4] == bits(np.sqrt(f32(2992.0) / f32(33.0)))
    m64, s64 = v.astype(np.float64).mean(0), v.astype(np.float64).std(0)
    mean, std, _ = data.ensemble_grid_stats(v, 0.0)
    assert np.abs(mean - m64).max() < 1e-5 * np.abs(m64).max() and np.abs(std - s64).max() < 1e-5 * np.abs(m64).max()
    # a NaN sample poisons its own pair only
    w = v.copy()
    w[20, 2] = np.nan
    out, clean = data.ensemble_grid_stats(w, 1.5), data.ensemble_grid_stats(v, 1.5)
    for o, c in zip(out, clean):
        assert np.isnan(o[2]) and np.array_equal(bits(np.delete(o, 2)), bits(np.delete(c, 2)))


# ---------------------------------------------------------------- the preconditions of tests/test_gpu_mc_dropout.py
@pytest.fixture(scope="module")
def case(tmp_path_factory):
    t = K.make_transfer(tmp_path_factory.mktemp("mc_case"), CPU)
    cat, an = K.species()
    most = int(_lib.load().impnn_transfer_mc_grid_max_samples())
    state = t.state_dict()
    return {"ref": K.reference(state, cat, an, K.DRAW, most), "walk": K.fp32_walk(state, cat, an, K.DRAW, most), "most": most,
            "state": state}


def test_case_fp32_walk_stays_at_half_the_bound(case):
    """Every sample plane of every grid of the GPU tests, as assert_close judges it (per tensor and per element)."""
    assert (case["state"]["melting_point/kernel"] >= 0).all() and case["state"]["mp_bn_1/moving_variance"].std() > 0.1
    for Cn, An in K.GRIDS:
        worst = max(max(closeness(case["walk"][s, :Cn, :An], case["ref"][s, :Cn, :An])) for s in range(case["most"]))
        print(f"{Cn} x {An}: fp32 walk, worst of {case['most']} planes {worst:.2e}")
        assert worst <= K.HALF_BOUND, (Cn, An, worst)
    # and its statistic: the mean at the bound's half, the std against max|mean| (what the GPU test asks of the kernel)
    mean, std, _ = data.ensemble_grid_stats(case["walk"], 0.0)
    m64, s64 = case["ref"].mean(0), case["ref"].std(0)
    assert max(closeness(mean, m64)) <= K.HALF_BOUND
    assert np.abs(std - s64).max() <= K.HALF_BOUND * np.abs(m64).max()


def test_case_spread_is_not_trivial(case):
    for Cn, An in K.GRIDS:
        for S in (2, 7, case["most"]):
            got = K.spread_fraction(case["ref"][:S, :Cn, :An])
            assert got >= 0.9, (Cn, An, S, got)
    assert np.ptp(case["ref"].mean(0)) > 0.05 * np.abs(case["ref"].mean(0)).max(), "a flat grid checks nothing"
