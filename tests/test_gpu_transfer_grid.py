"""The transfer head over a cation x anion grid on the GPU: impnn_transfer_grid_prepare, impnn_transfer_ion_half and
impnn_transfer_head_grid (csrc/transfer_grid.hip) against the fp64 reference of tests/transfer_ref.py on the explicitly
expanded pairs, and MPNNModel.predict_grid's "auto" / "gathered" modes for the transfer model.

Tolerances: conftest's assert_close at 1e-5 against fp64, the bound every forward value of this project meets
(tests/test_transfer_grid_host.py shows a plain fp32 walk of the same cases at or below half of it); bitwise wherever
the same kernel evaluates the same pair (position in a grid, host tiling, two runs, the clean part of a NaN run) and
for "gathered" against the head kernel it is defined to call."""
import ctypes as C

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, model as MM, ops, synthetic, train
from conftest import assert_close

import transfer_ref as R
from test_gpu_grid import SENTINEL, bits, expanded, guarded, species, split_guarded
from test_transfer_grid_host import DIMS, SCALES, ion_half, make_case, ref_grid, weight_list

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE_C, TILE_A = 8, 32  # the grid kernel's tile is 8 cations x 32 anions (csrc/transfer_grid.hip)
SHAPES = [(1, 1), (7, 63), (TILE_C - 1, 5), (TILE_C, 2), (TILE_C + 1, TILE_A + 2), (65, 130), (130, 1)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def head_on_device(w):
    """-> (the 18 weight tensors, the cfg ops.transfer_head / ops.transfer_grid_prepare read)."""
    tensors = [dev(a) for a in weight_list(w)]
    cfg = {"moving_mean": dev(w["mp_bn_1/moving_mean"]), "moving_variance": dev(w["mp_bn_1/moving_variance"]),
           "epsilon": R.BN_EPS}
    return tensors, cfg


def gathered(pc, pa, tensors, cfg, F, Mx):
    """ops.transfer_head (impnn_transfer_head, what MPNNModel.head runs) on the explicit pairs -> (C,A)."""
    Cn, An, D = pc.shape[0], pa.shape[0], pc.shape[1]
    pcg = pc[:, None, :].expand(Cn, An, D).reshape(-1, D).contiguous()
    pag = pa[None, :, :].expand(Cn, An, D).reshape(-1, D).contiguous()
    return ops.transfer_head(pcg, pag, tensors, {**cfg, "fp_size": F, "mixing_size": Mx}).reshape(Cn, An)


def grid(pc, pa, tensors, image, F, Mx):
    return ops.transfer_head_grid(ops.transfer_ion_half("cat", pc, tensors, F, Mx),
                                  ops.transfer_ion_half("an", pa, tensors, F, Mx), image)


# ---------------------------------------------------------------- 1. shapes, head only
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "D%d-F%d-Mx%d" % d)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_grid_against_fp64_every_tile_edge_and_alignment(shape, dims):
    (Cn, An), (D, F, Mx) = shape, dims
    lib = _lib.load()
    for scale in SCALES:
        w, pc_h, pa_h = make_case(dims, shape, scale)
        ref = ref_grid(w, pc_h, pa_h)
        tensors, cfg = head_on_device(w)
        pc, pa = dev(pc_h), dev(pa_h)
        # precondition: the head kernel itself meets the bound on these pairs, so a hard input shows as such
        assert_close(gathered(pc, pa, tensors, cfg, F, Mx).cpu().numpy(), ref, 1e-5, f"precondition: transfer_head {shape} {dims} x{scale:g}")
        image = ops.transfer_grid_prepare(tensors, cfg)
        assert image.numel() == lib.impnn_transfer_grid_image_floats()
        uc, ua = ops.transfer_ion_half("cat", pc, tensors, F, Mx), ops.transfer_ion_half("an", pa, tensors, F, Mx)
        first = None
        for offset in range(4):
            whole, out_ptr = guarded(Cn * An, offset)
            _lib.check(lib.impnn_transfer_head_grid(_lib.ptr(uc), _lib.ptr(ua), _lib.ptr(image), image.numel(), out_ptr,
                                                    Cn, An, _lib.stream_ptr()))
            torch.cuda.synchronize()
            got = split_guarded(whole, Cn * An, offset).reshape(Cn, An)  # every element written, none outside
            assert_close(got, ref, 1e-5, f"grid vs fp64 {shape} {dims} x{scale:g} offset {offset}")
            first = got if first is None else first
            assert np.array_equal(bits(got), bits(first)), "the output alignment must not change a value"
        assert np.array_equal(bits(ops.transfer_head_grid(uc, ua, image).cpu().numpy()), bits(first)), "the public wrapper"


# ---------------------------------------------------------------- 2. u rows
@pytest.mark.parametrize("M", [1, 9, 300])
def test_ion_half_against_fp64(M):
    for dims in DIMS:
        D, F, Mx = dims
        w, rows, _ = make_case(dims, (M, 1), 1.0)
        tensors, _ = head_on_device(w)
        for ion in ("cat", "an"):
            got = ops.transfer_ion_half(ion, dev(rows), tensors, F, Mx)
            assert got.shape == (M, 256)
            assert_close(got.cpu().numpy(), ion_half(w, ion, rows, np.float64)[0], 1e-5, f"u rows {ion} M={M} {dims}")
        # the bias enters on the anion side only: with equal per-ion weights the two rows differ by b1 exactly there
        same = dict(w)
        for part in ("fp/kernel", "fp/bias", "proj/kernel", "proj/bias"):
            same[f"an_{part}"] = w[f"cat_{part}"]
        t2, _ = head_on_device(same)
        diff = (ops.transfer_ion_half("an", dev(rows), t2, F, Mx) - ops.transfer_ion_half("cat", dev(rows), t2, F, Mx)).cpu().numpy()
        assert_close(diff, np.broadcast_to(w["mp_dense_1/bias"], diff.shape), 1e-5, "anion - cation rows = b1")


# ---------------------------------------------------------------- 3. position independence (head level), 4. NaN
def test_a_pair_has_the_same_bits_wherever_it_sits():
    dims = D, F, Mx = DIMS[0]
    w, pc_h, pa_h = make_case(dims, (40, 77), 1.0)
    tensors, cfg = head_on_device(w)
    image = ops.transfer_grid_prepare(tensors, cfg)
    big = grid(dev(pc_h), dev(pa_h), tensors, image, F, Mx).cpu().numpy()
    assert np.array_equal(bits(grid(dev(pc_h), dev(pa_h), tensors, image, F, Mx).cpu().numpy()), bits(big)), "two runs"
    # the pair (cation 37, anion 70) of the 40 x 77 grid at four other places of other-sized grids
    for Cn, An, i, j in ((1, 1, 0, 0), (3, 5, 1, 2), (9, 33, 8, 32), (17, 64, 0, 63)):
        _, qc, qa = make_case(dims, (Cn, An), 10.0)
        qc[i], qa[j] = pc_h[37], pa_h[70]
        small = grid(dev(qc), dev(qa), tensors, image, F, Mx).cpu().numpy()
        assert bits(small[i, j]) == bits(big[37, 70]), f"pair moved to ({i},{j}) of {Cn} x {An}"
    # a sub-grid is the grid's block
    sub = grid(dev(pc_h[5:14]), dev(pa_h[30:71]), tensors, image, F, Mx).cpu().numpy()
    assert np.array_equal(bits(sub), bits(big[5:14, 30:71]))


def test_a_nan_row_and_a_nan_column_stay_where_they_are():
    dims = D, F, Mx = DIMS[0]
    w, pc_h, pa_h = make_case(dims, (19, 67), 1.0)
    tensors, cfg = head_on_device(w)
    image = ops.transfer_grid_prepare(tensors, cfg)
    clean = grid(dev(pc_h), dev(pa_h), tensors, image, F, Mx).cpu().numpy()
    assert np.isfinite(clean).all()
    bc, ba = pc_h.copy(), pa_h.copy()
    bc[17], ba[40] = np.nan, np.nan
    got = grid(dev(bc), dev(ba), tensors, image, F, Mx).cpu().numpy()
    assert np.isnan(got[17]).all() and np.isnan(got[:, 40]).all(), "the NaN cation's row and the NaN anion's column"
    keep = np.ones_like(got, bool)
    keep[17], keep[:, 40] = False, False
    assert np.array_equal(bits(got[keep]), bits(clean[keep])), "every other element keeps its bits"


# ---------------------------------------------------------------- 5. whole model
@pytest.fixture(scope="module")
def transfer(tmp_path_factory):
    """make_transfer(S=2) with 33 x 70 species; the fp64 reference over the product and predict on the expanded list,
    computed once."""
    from test_gpu_transfer import make_transfer
    t = make_transfer(tmp_path_factory.mktemp("transfer_grid"), S=2)
    cat, _ = species(33, 50)
    _, an = species(70, 51)
    w = {k: torch.tensor(v, dtype=R.DT) for k, v in t.state_dict().items()}
    # one encoder pass per species in fp64: anion j beside cation j % 33
    pair = {f"cat_{k}": cat[k][np.arange(70) % 33] for k in MM.ION_KEYS}
    pair.update({f"an_{k}": an[k] for k in MM.ION_KEYS})
    with torch.no_grad():
        pc64, pa64 = R.pooled(w, pair)
        pc64 = pc64[:33]
        ref = R.head(w, pc64.repeat_interleave(70, dim=0), pa64.repeat(33, 1))[0].numpy().reshape(33, 70)
    pred = t.predict(expanded(cat, an)).reshape(33, 70)
    return {"t": t, "cat": cat, "an": an, "ref": ref, "pred": pred}


def test_model_grid_auto(transfer):
    t, cat, an = transfer["t"], transfer["cat"], transfer["an"]
    assert t.grid_head_mode == "auto" and t._transfer_grid_covers() and not t._grid_kernels_cover()
    got = t.predict_grid(cat, an)
    assert got.shape == (33, 70) and got.dtype == np.float32
    assert_close(got, transfer["ref"], 1e-5, "predict_grid (auto) vs transfer_ref")
    assert_close(got, transfer["pred"], 1e-5, "predict_grid (auto) vs predict on the expanded list")
    assert np.array_equal(bits(t.predict_grid(cat, an)), bits(got)), "two runs must agree bitwise"
    for pairs in (20, 70, 3 * 70 + 1):
        assert np.array_equal(bits(t.predict_grid(cat, an, max_pairs_per_launch=pairs)), bits(got)), f"host tiles of {pairs} pairs"
    # 7 x 9: a corner of the same species is the corner of the grid
    sub_c, sub_a = {k: v[:7] for k, v in cat.items()}, {k: v[:9] for k, v in an.items()}
    small = t.predict_grid(sub_c, sub_a)
    assert_close(small, transfer["ref"][:7, :9], 1e-5, "7 x 9 vs transfer_ref")
    assert_close(small, transfer["pred"][:7, :9], 1e-5, "7 x 9 vs predict")
    with pytest.raises(ValueError, match="return_params"):
        t.predict_grid(cat, an, return_params=True)


def test_model_grid_gathered_is_the_head_kernel_bitwise(transfer):
    t, cat, an = transfer["t"], transfer["cat"], transfer["an"]
    with pytest.raises(ValueError, match="grid_head_mode"):
        t.grid_head_mode = "mfma?"
    t.grid_head_mode = "gathered"
    try:
        got = t.predict_grid(cat, an)
    finally:
        t.grid_head_mode = "auto"
    pc, pa = t.encode_ions(cat, an)
    with torch.no_grad():
        want = t.head(pc[:, None, :].expand(33, 70, 32).reshape(-1, 32).contiguous(),
                      pa[None, :, :].expand(33, 70, 32).reshape(-1, 32).contiguous()).reshape(33, 70).cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    assert_close(got, transfer["ref"], 1e-5, "predict_grid (gathered) vs transfer_ref")


def test_wide_atom_dim_and_an_uncovered_width(tmp_path):
    from test_gpu_transfer import make_transfer
    cat, _ = species(5, 40)
    _, an = species(6, 41)
    wide = make_transfer(tmp_path, D=128, S=1)
    assert wide._transfer_grid_covers()
    assert_close(wide.predict_grid(cat, an), wide.predict(expanded(cat, an)).reshape(5, 6), 1e-5, "atom_dim 128 vs predict")
    f96 = make_transfer(tmp_path, S=1, F=96)
    assert not f96._transfer_grid_covers() and f96.grid_head_mode == "auto"
    assert_close(f96.predict_grid(cat, an), f96.predict(expanded(cat, an)).reshape(5, 6), 1e-5, "fp_size 96: the gathered path")


# ---------------------------------------------------------------- 6. weight versions
def test_the_image_follows_the_weights(tmp_path):
    from test_gpu_transfer import make_transfer, stage1
    t = make_transfer(tmp_path, S=1)
    cat, _ = species(9, 60)
    _, an = species(11, 61)
    pairs = expanded(cat, an)
    before = t.predict_grid(cat, an)
    assert t._transfer_grid_image is not None
    state = t.state_dict()
    rng = np.random.default_rng(3)
    for n in ("mp_dense_2/kernel", "mp_dense_3/bias", "melting_point/kernel", "mp_bn_1/moving_mean", "mp_bn_1/beta"):
        state[n] = (state[n] + rng.normal(0.0, 0.3, size=state[n].shape)).astype(np.float32)
    state["mp_bn_1/moving_variance"] = rng.uniform(0.3, 3.0, size=256).astype(np.float32)
    t.load_weights(state)
    after = t.predict_grid(cat, an)
    assert np.abs(after - before).max() > 1e-2 * np.abs(before).max(), "the changed head must change the grid"
    assert_close(after, t.predict(pairs).reshape(9, 11), 1e-5, "after load_weights: grid vs predict")
    # one stage-1 training step (the head trains, the moving statistics move): the grid follows again
    stage1(t)
    t.compile(train.Adam(1e-2), loss=train.Huber(delta=1.0))
    inp = t._to_device(synthetic.make_batch(32, seed=2))
    t.train_on_batch(inp, np.random.default_rng(5).normal(0.0, 1.0, size=32).astype(np.float32))
    trained = t.predict_grid(cat, an)
    assert not np.array_equal(bits(trained), bits(after)), "a training step changes the head"
    assert_close(trained, t.predict(pairs).reshape(9, 11), 1e-5, "after a training step: grid vs predict")


# ---------------------------------------------------------------- 7. status codes
_A = 0x100000  # a 16-byte aligned stand-in
_M = 0x100004  # a misaligned one
OK, BADARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4


def test_status_codes_are_pinned():
    """The family's rules in their order - shape, zero work, null pointers (then alignment and the image size), ranges -
    on stand-in pointers: every row returns before a launch."""
    lib = _lib.load()
    n = lib.impnn_transfer_grid_image_floats()
    assert n == 256 * 128 + 128 * 64 + 2 * 256 + 128 + 64 + 64 + 4
    table = (C.c_void_p * 18)(*([_A] * 18))
    hole = (C.c_void_p * 18)(*([_A] * 12 + [0] + [_A] * 5))
    vp = C.c_void_p
    half = lambda **k: lib.impnn_transfer_ion_half(*[{"ion": 0, "pooled": vp(_A), "weights": table, "u": vp(_A), "M": 5,
                                                      "D": 32, "F": 32, "Mx": 20, "stream": None, **k}[a]
                                                     for a in ("ion", "pooled", "weights", "u", "M", "D", "F", "Mx", "stream")])
    head = lambda **k: lib.impnn_transfer_head_grid(*[{"u_cat": vp(_A), "u_an": vp(_A), "image": vp(_A), "image_floats": n,
                                                       "out": vp(_M), "C": 3, "A": 4, "stream": None, **k}[a]
                                                      for a in ("u_cat", "u_an", "image", "image_floats", "out", "C", "A", "stream")])
    prep = lambda **k: lib.impnn_transfer_grid_prepare(*[{"weights": table, "mean": vp(_A), "var": vp(_A), "eps": 1e-3,
                                                          "image": vp(_A), "image_floats": n, "stream": None, **k}[a]
                                                         for a in ("weights", "mean", "var", "eps", "image", "image_floats", "stream")])
    cases = [
        # rule 1: shape
        (half, dict(ion=2), BADARG, "impnn_transfer_ion_half: bad shape"),
        (half, dict(M=-1), BADARG, "impnn_transfer_ion_half: bad shape"),
        (half, dict(D=0, M=0, pooled=None), BADARG, "impnn_transfer_ion_half: bad shape"),
        (head, dict(C=-1), BADARG, "impnn_transfer_head_grid: bad shape"),
        (head, dict(A=-2, C=0), BADARG, "impnn_transfer_head_grid: bad shape"),
        (prep, dict(eps=-1.0), BADARG, "impnn_transfer_grid_prepare: bad shape"),
        # rule 2: zero work comes before the pointers and the ranges
        (half, dict(M=0, pooled=None, u=None, D=4096), OK, None),
        (head, dict(C=0, out=None, u_cat=None), OK, None),
        (head, dict(A=0, image=None, image_floats=0), OK, None),
        # rule 3: null pointers, then alignment, then the image size
        (half, dict(pooled=None, D=4096), BADARG, "impnn_transfer_ion_half: null pointer"),
        (half, dict(weights=None), BADARG, "impnn_transfer_ion_half: null pointer"),
        (half, dict(weights=hole), BADARG, "impnn_transfer_ion_half: null weight tensor 12"),
        (head, dict(out=None, image_floats=1), BADARG, "impnn_transfer_head_grid: null pointer"),
        (head, dict(u_an=vp(_M)), BADARG, "impnn_transfer_head_grid: u rows and the image must be 16-byte aligned"),
        (head, dict(image_floats=n - 1), WORKSPACE, f"impnn_transfer_head_grid: image of {n - 1} floats is too small ({n})"),
        (prep, dict(var=None), BADARG, "impnn_transfer_grid_prepare: null pointer"),
        (prep, dict(weights=hole, image_floats=1), BADARG, "impnn_transfer_grid_prepare: null weight tensor 12"),
        (prep, dict(image=vp(_M)), BADARG, "impnn_transfer_grid_prepare: u rows and the image must be 16-byte aligned"),
        (prep, dict(image_floats=16), WORKSPACE, f"impnn_transfer_grid_prepare: image of 16 floats is too small ({n})"),
        # rule 4: ranges
        (half, dict(D=129), UNSUPPORTED, "impnn_transfer_ion_half: dims D=129 (<= 128) F=32 Mx=20 (<= 64)"),
        (half, dict(F=65), UNSUPPORTED, "impnn_transfer_ion_half: dims D=32 (<= 128) F=65 Mx=20 (<= 64)"),
        (half, dict(Mx=96), UNSUPPORTED, "impnn_transfer_ion_half: dims D=32 (<= 128) F=32 Mx=96 (<= 64)"),
    ]
    for fn, kw, code, text in cases:
        rc = fn(**kw)
        assert rc == code, (kw, rc, lib.impnn_last_error_string().decode())
        if text is not None:
            assert lib.impnn_last_error_string().decode() == text, kw


def test_zero_work_launches_nothing_and_cpu_tensors_raise():
    dims = D, F, Mx = DIMS[0]
    w, pc_h, pa_h = make_case(dims, (3, 4), 1.0)
    tensors, cfg = head_on_device(w)
    image = ops.transfer_grid_prepare(tensors, cfg)
    assert ops.transfer_ion_half("cat", dev(pc_h[:0]), tensors, F, Mx).shape == (0, 256)
    uc, ua = ops.transfer_ion_half("cat", dev(pc_h), tensors, F, Mx), ops.transfer_ion_half("an", dev(pa_h), tensors, F, Mx)
    assert ops.transfer_head_grid(uc[:0], ua, image).shape == (0, 4)
    assert ops.transfer_head_grid(uc, ua[:0], image).shape == (3, 0)
    # zero work touches nothing: a sentinel buffer stays as it is
    whole, out_ptr = guarded(16, 0)
    lib = _lib.load()
    assert lib.impnn_transfer_head_grid(_lib.ptr(uc), _lib.ptr(ua), _lib.ptr(image), image.numel(), out_ptr, 0, 4,
                                        _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert (whole.cpu().numpy().view(np.uint32) == SENTINEL.view(np.uint32)).all()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.transfer_ion_half("cat", torch.from_numpy(pc_h), tensors, F, Mx)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.transfer_head_grid(uc.cpu(), ua, image)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.transfer_grid_prepare([t.cpu() for t in tensors], cfg)
    with pytest.raises(ValueError, match="u rows"):
        ops.transfer_head_grid(uc[:, :128], ua, image)
    with pytest.raises(ValueError, match="wrong length"):
        ops.transfer_head_grid(uc, ua, image[:-4])
    with pytest.raises(ValueError, match="pooled must be"):
        ops.transfer_ion_half("an", dev(pa_h).reshape(-1), tensors, F, Mx)
