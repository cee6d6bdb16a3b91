"""The transfer head over a cation x anion grid, on the host: the case generators of tests/test_gpu_transfer_grid.py
and what they must satisfy before a kernel is judged on them.

* fp32 precondition.  The project's rule: a bound that a plain f32 implementation misses marks a hard input, not a
  kernel defect.  Every head-only case is walked here in fp32 numpy, in the kernels' factored order, against the fp64
  reference (tests/transfer_ref.py::head on the explicitly expanded pairs) under conftest.assert_close's two criteria.
  The bound of the GPU tests is 1e-5; the cases are seeded so that the fp32 walk stays at or below 5e-6, half of it.
* Factorisation identity, fp64 at 1e-12: relu(Uc[i] + Ua[j]) == relu((mc[i] + ma[j]) W1 + b1).
* The header / export / binding agreement of the three new entries (tests/test_cabi.py enforces it for every symbol;
  here: that they are declared at all, and that the ABI version stayed at 3)."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import transfer_ref as R

ROOT = Path(__file__).resolve().parents[1]

DIMS = [(32, 32, 20), (128, 64, 64), (8, 8, 5)]  # (D, F, Mx): the reference's, the widest, Mx no multiple of 4
SCALES = (1.0, 10.0)                              # pooled rows: normal(0, 1) and 10 x that
HOST_SHAPES = [(65, 130), (130, 1), (7, 63)]
HALF_BOUND = 5e-6
HEAD_NAMES = ["cat_fp", "an_fp", "cat_proj", "an_proj", "mp_dense_1", "mp_bn_1", "mp_dense_2", "mp_dense_3",
              "melting_point"]


def head_state(D, F, Mx, seed):
    """Head variables by name, randomised as test_gpu_transfer.make_transfer does: Glorot-uniform kernels x 1.5,
    normal(0, 0.2) biases / beta / moving mean, gamma in [0.5, 1.5], moving variance in [0.5, 2]."""
    rng = np.random.default_rng(seed)

    def kernel(i, o):
        lim = np.sqrt(6.0 / (i + o))
        return (rng.uniform(-lim, lim, size=(i, o)) * 1.5).astype(np.float32)

    vec = lambda n: rng.normal(0.0, 0.2, size=n).astype(np.float32)
    w = {}
    for name, (i, o) in (("cat_fp", (D, F)), ("an_fp", (D, F)), ("cat_proj", (F, Mx)), ("an_proj", (F, Mx)),
                         ("mp_dense_1", (Mx, 256)), ("mp_dense_2", (256, 128)), ("mp_dense_3", (128, 64)),
                         ("melting_point", (64, 1))):
        w[f"{name}/kernel"], w[f"{name}/bias"] = kernel(i, o), vec(o)
    w["mp_bn_1/gamma"] = rng.uniform(0.5, 1.5, size=256).astype(np.float32)
    w["mp_bn_1/beta"] = vec(256)
    w["mp_bn_1/moving_mean"] = vec(256)
    w["mp_bn_1/moving_variance"] = rng.uniform(0.5, 2.0, size=256).astype(np.float32)
    return w


def weight_list(w):
    """The 18 tensors in the order of impnn_transfer_head's `weights` (include/impnn.h)."""
    names = ["cat_fp", "an_fp", "cat_proj", "an_proj", "mp_dense_1"]
    out = [w[f"{n}/{part}"] for n in names for part in ("kernel", "bias")]
    out += [w["mp_bn_1/gamma"], w["mp_bn_1/beta"]]
    for n in ("mp_dense_2", "mp_dense_3", "melting_point"):
        out += [w[f"{n}/kernel"], w[f"{n}/bias"]]
    return out


def case_seed(dims, shape, scale):
    return 1000 * DIMS.index(tuple(dims)) + 10 * shape[0] + shape[1] + (500 if scale != 1.0 else 0)


def make_case(dims, shape, scale):
    """-> (weights by name, pooled_cat (C,D), pooled_an (A,D)), all float32."""
    (D, F, Mx), (Cn, An) = dims, shape
    seed = case_seed(dims, shape, scale)
    rng = np.random.default_rng(seed + 7)
    pc = (rng.normal(0.0, 1.0, size=(Cn, D)) * scale).astype(np.float32)
    pa = (rng.normal(0.0, 1.0, size=(An, D)) * scale).astype(np.float32)
    return head_state(D, F, Mx, seed), pc, pa


def ref_grid(w, pc, pa):
    """fp64: transfer_ref.head on the explicitly expanded pairs (pc[i], pa[j]) -> (C,A)."""
    Cn, An = len(pc), len(pa)
    w64 = {k: torch.tensor(np.asarray(v), dtype=R.DT) for k, v in w.items()}
    pcg = torch.tensor(np.repeat(pc, An, axis=0), dtype=R.DT)
    pag = torch.tensor(np.tile(pa, (Cn, 1)), dtype=R.DT)
    return R.head(w64, pcg, pag)[0].numpy().reshape(Cn, An)


def ion_half(w, ion, pooled, dt):
    """u rows in dtype dt: relu(relu(pooled Wfp + bfp) Wp + bp) W1, + b1 for the anion only."""
    c = lambda n: np.asarray(w[n], dt)
    relu = lambda x: np.maximum(x, dt(0))
    fp = relu(pooled.astype(dt) @ c(f"{ion}_fp/kernel") + c(f"{ion}_fp/bias"))
    mix = relu(fp @ c(f"{ion}_proj/kernel") + c(f"{ion}_proj/bias"))
    u = mix @ c("mp_dense_1/kernel")
    return (u + c("mp_dense_1/bias")) if ion == "an" else u, mix


def factored_walk(w, pc, pa, dt):
    """The kernels' order in dtype dt: u rows per ion, a1 = relu(Uc[i] + Ua[j]), BatchNormalization as scale / shift,
    then the three Dense layers."""
    c = lambda n: np.asarray(w[n], dt)
    relu = lambda x: np.maximum(x, dt(0))
    uc, ua = ion_half(w, "cat", pc, dt)[0], ion_half(w, "an", pa, dt)[0]
    scale = c("mp_bn_1/gamma") / np.sqrt(c("mp_bn_1/moving_variance") + dt(R.BN_EPS))
    shift = c("mp_bn_1/beta") - c("mp_bn_1/moving_mean") * scale
    bn = relu(uc[:, None, :] + ua[None, :, :]) * scale + shift
    a2 = relu(bn @ c("mp_dense_2/kernel") + c("mp_dense_2/bias"))
    a3 = relu(a2 @ c("mp_dense_3/kernel") + c("mp_dense_3/bias"))
    return (a3 @ c("melting_point/kernel") + c("melting_point/bias"))[..., 0]


def closeness(actual, expected, floor=0.3):
    """conftest.assert_close's two figures: the per-tensor error against max|e| and the worst per-element error against
    max(|e_i|, floor * max|e|).  assert_close(rel) holds iff both are <= rel."""
    a, e = np.asarray(actual, np.float64), np.asarray(expected, np.float64)
    scale = max(float(np.max(np.abs(e))), 1e-30)
    diff = np.abs(a - e)
    return float(diff.max()) / scale, float(np.max(diff / np.maximum(np.abs(e), floor * scale)))


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "D%d-F%d-Mx%d" % d)
@pytest.mark.parametrize("shape", HOST_SHAPES, ids=lambda s: "%dx%d" % s)
def test_fp32_walk_stays_at_half_the_bound(shape, dims, scale):
    w, pc, pa = make_case(dims, shape, scale)
    ref = ref_grid(w, pc, pa)
    per_tensor, per_element = closeness(factored_walk(w, pc, pa, np.float32), ref)
    print(f"{shape} {dims} x{scale:g}: fp32 walk per tensor {per_tensor:.2e}, per element {per_element:.2e}")
    assert np.ptp(ref) > 0.05 * np.abs(ref).max(), "a flat grid checks nothing"
    assert per_tensor <= HALF_BOUND and per_element <= HALF_BOUND


@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "D%d-F%d-Mx%d" % d)
def test_factorisation_identity(dims):
    w, pc, pa = make_case(dims, (7, 63), 1.0)
    f64 = np.float64
    (uc, mc), (ua, ma) = ion_half(w, "cat", pc, f64), ion_half(w, "an", pa, f64)
    left = np.maximum(uc[:, None, :] + ua[None, :, :], 0.0)
    right = np.maximum((mc[:, None, :] + ma[None, :, :]) @ w["mp_dense_1/kernel"].astype(f64)
                       + w["mp_dense_1/bias"].astype(f64), 0.0)
    np.testing.assert_allclose(left, right, rtol=1e-12, atol=1e-12)
    # and the factored fp64 walk is the reference itself
    np.testing.assert_allclose(factored_walk(w, pc, pa, f64), ref_grid(w, pc, pa), rtol=1e-11, atol=1e-11)


def test_entries_are_declared_and_bound():
    from ionic_mpnn_amd import _lib
    header = (ROOT / "include" / "impnn.h").read_text()
    for name in ("impnn_transfer_grid_image_floats", "impnn_transfer_grid_prepare", "impnn_transfer_ion_half",
                 "impnn_transfer_head_grid"):
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared"
        assert name in _lib.SIGNATURES, f"{name} is not bound"
    assert re.search(r"#define IMPNN_ABI_VERSION 3\b", header) and _lib.ABI_VERSION == 3
