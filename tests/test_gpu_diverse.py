"""GPU: the diverse batch (include/impnn.h, impnn_diverse_select; csrc/grid_diverse.hip) - k pairs by farthest-point
selection over the domain distance.

1. exact, against the existing kernel: at every step the pick and the bits of its distance are what the definition
   gives on ops.domain_grid(mc, ma, cat(ref, z[picks so far])) - candidates D > 0, the first of equal maxima;
2. against float64: the device's pick is within (1 - 2 * RTOL) of the farthest float64 candidate at every step;
3. edge cases: rows of small integers (exact ties) equal to data.grid_diverse pick for pick, a sparse mask with whole
   tiles empty and an all-zero mask, a NaN cation row and anion column, k = 1, k beyond the candidates, two runs bitwise;
4. nothing is written outside the outputs and the workspace;
5. the model: screen_diverse is ops.domain_diverse on the model's own mixing rows; the refusals.

The shapes are test_gpu_domain's - one tile to several, ragged on both axes - and one whose A is a multiple of 4, where
the state plane moves 16 bytes per lane (the others take the 4-byte path); both register templates of the init kernel
(Mx <= 32, Mx = 64) and an Mx that is no multiple of 4; R = 1 and one more than the kernels' reference chunk."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, data, ops
from ionic_mpnn_amd.ensemble import ModelEnsemble

from diverse_cases import INTEGER_K, integer_rows
from test_gpu_domain import reference_rows
from test_gpu_grid import DIMS, bits, make_model, species
from test_gpu_screen import Guarded, head_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("viscosity", "melting_point")
SHAPES = [(1, 1), (7, 63), (17, 130), (65, 130), (33, 132)]
K = 24
RTOL = 1e-5  # the project's bound in test_gpu_domain; the winner and the runner-up each carry it
ids_dims = lambda d: "D%d-F%d-Mx%d" % d
ids_shape = lambda s: "%dx%d" % s


def reference_sizes():
    return (1, ops.domain_reference_chunk() + 1)


def run(mc, ma, ref, k, where=None):
    """ops.domain_diverse -> host arrays (cation, anion, distance) of all k slots, n, competing."""
    words = None if where is None else data.PairMask.from_bool(where, device=DEV)
    ci, ai, d, counts = ops.domain_diverse(mc, ma, ref, k, where=words)
    assert ci.shape == ai.shape == d.shape == (k,) and counts.shape == (2,) and ci.is_cuda
    assert ci.dtype == ai.dtype == torch.int32 and d.dtype == torch.float32 and counts.dtype == torch.int64
    n, competing = (int(v) for v in counts.cpu().numpy())
    ci, ai, d = ci.cpu().numpy(), ai.cpu().numpy(), d.cpu().numpy()
    assert 0 <= n <= k and (ci[n:] == -1).all() and (ai[n:] == -1).all() and (bits(d[n:]) == 0x7FC00000).all(), "slots past n"
    return ci, ai, d, n, competing


def check_exact(mc, ma, ref, k, where=None, what=""):
    """Runs the selection and replays it on the existing kernel: the state of step t is ops.domain_grid against ref plus
    the latent vectors of the picks so far, the definition is applied with numpy.  -> run()'s result."""
    ci, ai, d, n, competing = got = run(mc, ma, ref, k, where)
    A = int(ma.shape[0])
    rows = ref
    for t in range(k):
        state = ops.domain_grid(mc, ma, rows)[0].cpu().numpy()
        cand = state > 0                                            # (a NaN is none)
        if where is not None:
            cand &= where
        if t == 0:
            assert competing == int(cand.sum()), f"{what}: competing"
        if not cand.any():
            assert n == t, f"{what}: the selection ends at step {t}, got n = {n}"
            break
        assert n > t, f"{what}: {int(cand.sum())} candidates at step {t}, got n = {n}"
        flat = int(np.argmax(np.where(cand, state, -np.inf)))      # the first of equal maxima
        assert (int(ci[t]), int(ai[t])) == (flat // A, flat % A), f"{what}: pick {t}"
        assert bits(d[t]) == bits(state.reshape(-1)[flat]), f"{what}: distance {t}"
        z = (mc[int(ci[t])] + ma[int(ai[t])]).reshape(1, -1)       # torch on the device: the float32 sum
        rows = torch.cat([rows, z])
    else:
        assert n == k, what
    assert (np.diff(d[:n]) <= 0).all() and (d[:n] > 0).all(), f"{what}: distance is positive and non-increasing"
    assert len({(int(c), int(a)) for c, a in zip(ci[:n], ai[:n])}) == n, f"{what}: a pair was chosen twice"
    return got


@functools.lru_cache(maxsize=None)
def case(kind, dims, shape, R):
    wp, mc, ma = head_case(kind, dims, shape)
    return mc, ma, reference_rows(kind, dims, wp, mc, ma, R, seed=7 + R)


# ---------------------------------------------------------------- 1. exact, against the existing kernel
@pytest.mark.parametrize("dims", DIMS, ids=ids_dims)
@pytest.mark.parametrize("shape", SHAPES, ids=ids_shape)
def test_every_pick_is_the_definition_on_the_domain_grid(shape, dims):
    picked = 0
    for kind in KINDS:
        for R in reference_sizes():
            mc, ma, ref = case(kind, dims, shape, R)
            _, _, _, n, _ = check_exact(mc, ma, ref, K, what=f"{kind} {shape} {dims} R={R}")
            picked += n
    assert picked > 0 or shape == (1, 1), "the grids hold candidates"   # (1,1): the pair is a reference row


# ---------------------------------------------------------------- 2. against float64
@pytest.mark.parametrize("dims", DIMS, ids=ids_dims)
@pytest.mark.parametrize("shape", SHAPES, ids=ids_shape)
def test_every_pick_is_the_farthest_in_float64(shape, dims):
    worst = np.inf
    for kind, R in zip(KINDS, reference_sizes()):
        mc, ma, ref = case(kind, dims, shape, R)
        ci, ai, _, n, _ = run(mc, ma, ref, K)
        state, _ = data.grid_domain(mc.cpu().numpy(), ma.cpu().numpy(), ref.cpu().numpy())
        z = (mc.cpu().numpy()[:, None, :] + ma.cpu().numpy()[None, :, :]).astype(np.float64)
        for t in range(n):
            cand = state > 0
            assert cand.any(), f"{kind} {shape} {dims} R={R}: step {t} has no float64 candidate"
            ratio = state[ci[t], ai[t]] / state[cand].max()
            worst = min(worst, ratio)
            assert ratio >= 1 - 2 * RTOL, f"{kind} {shape} {dims} R={R}: step {t} picks a pair at {ratio} of the farthest"
            diff = z - z[ci[t], ai[t]]
            state = np.minimum(state, np.sqrt((diff * diff).sum(axis=2)))
        if n < K:
            assert not (state > 0).any(), "the selection ended with float64 candidates left"
    print(f"{shape} {dims}: smallest ratio of the pick's float64 distance to the farthest candidate's: {worst}")


# ---------------------------------------------------------------- 3. edge cases
def test_integer_rows_equal_the_host_reference_pick_for_pick():
    mc_h, ma_h, ref_h = integer_rows()
    mc, ma, ref = (torch.from_numpy(x).to(DEV) for x in (mc_h, ma_h, ref_h))
    want = data.grid_diverse(mc_h, ma_h, ref_h, INTEGER_K)
    ci, ai, d, n, competing = check_exact(mc, ma, ref, INTEGER_K, what="integer rows")
    assert n == INTEGER_K == len(want.cation) and competing == want.competing
    assert np.array_equal(ci, want.cation) and np.array_equal(ai, want.anion)
    assert np.array_equal(d, want.distance.astype(np.float32))
    # the same rows with A a multiple of 4 (the 16-byte plane path): two more anions, copies of the first two
    ma4_h = np.concatenate([ma_h, ma_h[:2]])
    want4 = data.grid_diverse(mc_h, ma4_h, ref_h, INTEGER_K)
    ci, ai, d, n, competing = check_exact(mc, torch.from_numpy(ma4_h).to(DEV), ref, INTEGER_K, what="integer rows, A = 132")
    assert n == INTEGER_K and competing == want4.competing
    assert np.array_equal(ci, want4.cation) and np.array_equal(ai, want4.anion)
    assert np.array_equal(d, want4.distance.astype(np.float32))


@pytest.mark.parametrize("dims", DIMS[:2], ids=ids_dims)
@pytest.mark.parametrize("shape", [(65, 130), (33, 132)], ids=ids_shape)
def test_a_sparse_mask_with_empty_tiles_and_an_empty_mask(shape, dims):
    mc, ma, ref = case("viscosity", dims, shape, reference_sizes()[1])
    rng = np.random.default_rng(3)
    where = rng.random(shape) < 0.01
    where[16:32, :] = False    # a row of tiles
    where[:, 64:128] = False   # a column of tiles
    assert 10 <= where.sum() and not where[:16, :64].all()
    ci, ai, _, n, competing = check_exact(mc, ma, ref, K, where, what=f"sparse mask {shape} {dims}")
    assert 1 <= n <= min(K, competing) and where[ci[:n], ai[:n]].all(), "a pick left the mask"
    # k beyond the candidates: the selection ends early (check_exact holds n to the definition)
    few = np.zeros(shape, np.bool_)
    few.reshape(-1)[rng.choice(shape[0] * shape[1], 10, replace=False)] = True
    ci, ai, _, n, competing = check_exact(mc, ma, ref, K, few, what=f"ten candidates {shape} {dims}")
    assert 1 <= n <= competing <= 10 < K and few[ci[:n], ai[:n]].all()
    _, _, _, n, competing = run(mc, ma, ref, K, np.zeros(shape, np.bool_))
    assert n == 0 and competing == 0, "an all-zero mask"


@pytest.mark.parametrize("dims", DIMS[:2], ids=ids_dims)
def test_a_nan_row_and_column_never_compete(dims):
    shape = (17, 130)
    mc, ma, ref = case("melting_point", dims, shape, reference_sizes()[1])
    mc, ma = mc.clone(), ma.clone()
    mc[5, dims[2] - 1] = float("nan")     # one element is enough
    ma[70] = float("nan")
    ci, ai, _, n, competing = check_exact(mc, ma, ref, K, what=f"NaN {dims}")
    assert n == K and not (ci[:n] == 5).any() and not (ai[:n] == 70).any()
    assert competing <= 16 * 129


@pytest.mark.parametrize("dims", DIMS, ids=ids_dims)
def test_k_of_one_and_two_runs_agree_bitwise(dims):
    for shape in ((17, 130), (33, 132)):
        mc, ma, ref = case("viscosity", dims, shape, 1)
        first = check_exact(mc, ma, ref, 1, what=f"k = 1 {shape} {dims}")
        a, b = run(mc, ma, ref, K), run(mc, ma, ref, K)
        assert first[3] == 1 and (first[0][0], first[1][0], bits(first[2])[0]) == (a[0][0], a[1][0], bits(a[2])[0])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))
        assert a[3:] == b[3:]


# ---------------------------------------------------------------- 4. guarded outputs
@pytest.mark.parametrize("dims", DIMS[:2], ids=ids_dims)
@pytest.mark.parametrize("shape", [(7, 63), (65, 130), (33, 132)], ids=ids_shape)
def test_nothing_is_written_outside_the_outputs_and_the_workspace(shape, dims):
    lib = _lib.load()
    (Cn, An), Mx, R = shape, dims[2], reference_sizes()[1]
    mc, ma, ref = case("melting_point", dims, shape, R)
    rng = np.random.default_rng(5)
    for where in (None, rng.random(shape) < 0.3):
        want = run(mc, ma, ref, K, where)
        words = None if where is None else data.PairMask.from_bool(where, device=DEV).words
        need = C.c_size_t(0)
        _lib.check(lib.impnn_diverse_workspace_bytes(Cn, An, K, C.byref(need)))
        ci, ai, d, counts, ws = Guarded(K * 4), Guarded(K * 4), Guarded(K * 4), Guarded(16), Guarded(need.value)
        _lib.check(lib.impnn_diverse_select(_lib.ptr(mc), _lib.ptr(ma), _lib.ptr(ref), None if words is None else _lib.ptr(words),
                                            K, ci.ptr, ai.ptr, d.ptr, counts.ptr, ws.ptr, need.value, Cn, An, R, Mx,
                                            _lib.stream_ptr()))
        torch.cuda.synchronize()
        ws.body(np.uint8, "the workspace")
        n, competing = counts.body(np.int64, "counts")
        assert (int(n), int(competing)) == want[3:]
        assert np.array_equal(ci.body(np.int32, "cation"), want[0]) and np.array_equal(ai.body(np.int32, "anion"), want[1])
        assert np.array_equal(d.body(np.uint32, "distance"), bits(want[2]))


# ---------------------------------------------------------------- 5. the model
@pytest.mark.parametrize("kind", KINDS)
def test_screen_diverse_is_the_kernel_on_the_models_mixing_rows(kind):
    kw = dict(atom_dim=32, bond_dim=8, num_steps=2) if kind == "viscosity" else dict(atom_dim=32, num_steps=2)
    m, _ = make_model(kind, seed=3, **kw)
    cat, _ = species(19, 70)
    _, an = species(70, 71)
    rng = np.random.default_rng(9)
    dom = m.fit_domain(cat, an, rng.integers(0, 19, 30), rng.integers(0, 70, 30))
    mc, ma = m._domain_mix(cat, an, 4096)
    where = rng.random((19, 70)) < 0.2
    for mask in (None, where):
        sel = m.screen_diverse(cat, an, dom, where=None if mask is None else data.PairMask.from_bool(mask, device=DEV))
        ci, ai, d, n, competing = check_exact(mc, ma, dom.rows, K, mask, what=f"{kind} model")
        assert isinstance(sel, data.DiverseSelection) and sel.competing == competing and n == K
        assert sel.cation.dtype == sel.anion.dtype == np.int64 and sel.distance.dtype == np.float32
        assert np.array_equal(sel.cation, ci[:n]) and np.array_equal(sel.anion, ai[:n])
        assert np.array_equal(bits(sel.distance), bits(d[:n]))
        assert not set(zip(sel.cation.tolist(), sel.anion.tolist())) & set(zip(dom.cation.tolist(), dom.anion.tolist())), \
            "a training pair was chosen"
    assert len(m.screen_diverse(cat, an, dom, k=3).cation) == 3
    with pytest.raises(ValueError, match="k must be"):
        m.screen_diverse(cat, an, dom, k=0)
    with pytest.raises(TypeError, match="PairMask"):
        m.screen_diverse(cat, an, dom, where=where)
    with pytest.raises(ValueError, match="shape"):
        m.screen_diverse(cat, an, dom, where=data.PairMask.from_bool(where[:, :69], device=DEV))
    other = data.DomainReference(torch.zeros(3, m.mixing_size + 1, device=DEV), [0, 1, 2], [0, 1, 2], [0, 0, 0])
    with pytest.raises(ValueError, match="width"):
        m.screen_diverse(cat, an, other)
    with pytest.raises(ValueError, match="member model"):
        ModelEnsemble([m]).screen_diverse(cat, an, dom)


def test_the_transfer_model_is_refused(tmp_path):
    from test_gpu_transfer import make_transfer
    cat, _ = species(5, 80)
    _, an = species(6, 81)
    dom = data.DomainReference(torch.zeros(3, 20, device=DEV), [0, 1, 2], [3, 4, 5], [1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="base viscosity model"):
        make_transfer(tmp_path, S=2).screen_diverse(cat, an, dom)
