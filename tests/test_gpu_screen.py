"""Top-k screening on the GPU: impnn_head_grid_topk / impnn_transfer_head_grid_topk against data.grid_top_k of the
materialised grid (impnn_head_grid / impnn_transfer_head_grid), and MPNNModel.screen_top_k against
data.grid_top_k(predict_grid(...)).

Everything here is exact: a selected value is computed by the tile code of the materialising kernel, so values are
compared by their uint32 view, and the order (value, cation index, anion index; NaN last) is total, so indices are
compared for equality.  No tolerance appears."""
import ctypes as C

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, data, model as MM, ops

from footprint import FILL, GUARD, Guarded   # (test_gpu_pareto, _diverse, _rank, ... import them from here)
from test_gpu_grid import DIMS, T5, bits, head_weights, make_model, pack, pooled_rows, species
from test_transfer_grid_host import make_case
from test_gpu_transfer_grid import dev, head_on_device

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("viscosity", "melting_point")
MAX_T = ops.SELECT_MAX_T
T_MAX = np.array([263.15, 298.15, 313.0, 390.0], np.float32)
assert len(T_MAX) == MAX_T


# ---------------------------------------------------------------- guarded calls of the two entries
def call_topk(family, launch, Cn, An, nT, k, workgroups):
    """Runs one entry on guarded outputs and a guarded workspace of exactly the queried size -> data.TopK of the
    meaningful slots, (rows, min(k, C*A)); checks that every slot was written and that the rest is NaN / -1."""
    lib = _lib.load()
    rows, m = max(nT, 1), min(k, Cn * An)
    need = C.c_size_t(0)
    _lib.check(lib.impnn_grid_topk_workspace_bytes(family, Cn, An, nT, k, workgroups, C.byref(need)))
    out = [Guarded(rows * k * 4) for _ in range(3)]
    ws = Guarded(need.value)
    _lib.check(launch(lib, out[0].ptr, out[1].ptr, out[2].ptr, ws.ptr, need.value))
    torch.cuda.synchronize()
    v = out[0].body(np.uint32, "values").reshape(rows, k)
    ci = out[1].body(np.int32, "cation").reshape(rows, k)
    ai = out[2].body(np.int32, "anion").reshape(rows, k)
    entries = ws.body(np.uint64, "the workspace")
    filled = np.uint32(0xA5A5A5A5)
    assert not (v == filled).any() and not (ci.view(np.uint32) == filled).any() and not (ai.view(np.uint32) == filled).any(), \
        "an output slot was not written"
    assert not (entries == np.uint64(0xA5A5A5A5A5A5A5A5)).any(), "a workspace slot was not written"
    assert (v[:, m:] == 0x7FC00000).all() and (ci[:, m:] == -1).all() and (ai[:, m:] == -1).all(), "slots past C * A"
    assert (ci[:, :m] >= 0).all() and (ci[:, :m] < Cn).all() and (ai[:, :m] >= 0).all() and (ai[:, :m] < An).all()
    return data.TopK(v[:, :m].view(np.float32), ci[:, :m].astype(np.int64), ai[:, :m].astype(np.int64))


def head_topk(kind, mc, ma, T, wp, dims, k, largest, workgroups=0):
    D, F, Mx = dims
    Cn, An, nT = mc.shape[0], ma.shape[0], 0 if T is None else T.numel()
    launch = lambda lib, v, c, a, ws, nb: lib.impnn_head_grid_topk(
        ops.HEAD_KINDS[kind], _lib.ptr(mc), _lib.ptr(ma), _lib.ptr(T) if T is not None else None, _lib.ptr(wp), k,
        int(largest), v, c, a, ws, nb, Cn, An, nT, D, F, Mx, workgroups, _lib.stream_ptr())
    return call_topk(0, launch, Cn, An, nT, k, workgroups)


def transfer_topk(uc, ua, image, k, largest, workgroups=0):
    Cn, An = uc.shape[0], ua.shape[0]
    launch = lambda lib, v, c, a, ws, nb: lib.impnn_transfer_head_grid_topk(
        _lib.ptr(uc), _lib.ptr(ua), _lib.ptr(image), image.numel(), k, int(largest), v, c, a, ws, nb, Cn, An, workgroups,
        _lib.stream_ptr())
    return call_topk(1, launch, Cn, An, 0, k, workgroups)


def same(got, want, what):
    """got (rows, m) against data.grid_top_k's (m,) or (rows, m): values by bits, indices exactly."""
    wv, wc, wa = (np.atleast_2d(x) for x in want)
    assert got.values.shape == wv.shape, (what, got.values.shape, wv.shape)
    assert np.array_equal(bits(got.values), bits(wv)), f"{what}: values"
    assert np.array_equal(got.cation, wc) and np.array_equal(got.anion, wa), f"{what}: indices"


def head_case(kind, dims, shape, seed=5):
    (D, F, Mx), (Cn, An) = dims, shape
    wp = torch.from_numpy(pack(kind, head_weights(kind, D, F, Mx, seed=seed))).to(DEV)
    pc = torch.from_numpy(pooled_rows(Cn, D, 11 + Cn)).to(DEV)
    pa = torch.from_numpy(pooled_rows(An, D, 23 + An)).to(DEV)
    return wp, ops.head_ion_mix(kind, "cat", pc, wp, F, Mx), ops.head_ion_mix(kind, "an", pa, wp, F, Mx)


# ---------------------------------------------------------------- 1. the kernels against the materialised grid
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "D%d-F%d-Mx%d" % d)
@pytest.mark.parametrize("shape", [(1, 1), (7, 63), (17, 130), (65, 130)], ids=lambda s: "%dx%d" % s)
def test_head_topk_is_the_top_of_the_materialised_grid(shape, dims):
    D, F, Mx = dims
    Cn, An = shape
    ks = [1, 5, 64, 1024] + ([Cn * An + 3] if Cn * An + 3 < 1024 else [])   # (and one k above C * A where one call can)
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, shape)
        for T_h in ((T_MAX[:1], T_MAX[:3], T_MAX) if kind == "viscosity" else (None,)):
            T = None if T_h is None else torch.from_numpy(T_h).to(DEV)
            grid = ops.head_grid(kind, mc, ma, T, wp, F, Mx).cpu().numpy()
            for largest in (False, True):
                for k in ks:
                    got = head_topk(kind, mc, ma, T, wp, dims, k, largest)
                    same(got, data.grid_top_k(grid, k, largest), f"{kind} {shape} {dims} nT={0 if T is None else len(T_h)} k={k} largest={largest}")
    # the public wrapper returns the same rows, on the device, padded to k
    kind = "viscosity"
    wp, mc, ma = head_case(kind, dims, shape)
    T = torch.from_numpy(T_MAX[:3]).to(DEV)
    v, ci, ai = ops.head_grid_topk(kind, mc, ma, T, wp, F, Mx, 5)
    assert v.shape == ci.shape == ai.shape == (3, 5) and v.is_cuda and ci.dtype == torch.int32
    m = min(5, Cn * An)
    want = data.grid_top_k(ops.head_grid(kind, mc, ma, T, wp, F, Mx).cpu().numpy(), 5)
    same(data.TopK(v.cpu().numpy()[:, :m], ci.cpu().numpy()[:, :m], ai.cpu().numpy()[:, :m]), want, "ops.head_grid_topk")


def transfer_case(dims, shape, scale=1.0):
    D, F, Mx = dims
    w, pc_h, pa_h = make_case(dims, shape, scale)
    tensors, cfg = head_on_device(w)
    image = ops.transfer_grid_prepare(tensors, cfg)
    return ops.transfer_ion_half("cat", dev(pc_h), tensors, F, Mx), ops.transfer_ion_half("an", dev(pa_h), tensors, F, Mx), image


@pytest.mark.parametrize("shape", [(1, 1), (9, 33), (20, 70)], ids=lambda s: "%dx%d" % s)
def test_transfer_topk_is_the_top_of_the_materialised_grid(shape):
    Cn, An = shape
    for dims in DIMS[:2]:
        uc, ua, image = transfer_case(dims, shape)
        grid = ops.transfer_head_grid(uc, ua, image).cpu().numpy()
        for largest in (False, True):
            for k in (1, 50, 1024):
                same(transfer_topk(uc, ua, image, k, largest), data.grid_top_k(grid, k, largest), f"transfer {shape} {dims} k={k} largest={largest}")
    v, ci, ai = ops.transfer_head_grid_topk(uc, ua, image, 3, largest=True)
    m = min(3, Cn * An)
    same(data.TopK(v.cpu().numpy()[:, :m], ci.cpu().numpy()[:, :m], ai.cpu().numpy()[:, :m]), data.grid_top_k(grid, 3, True),
         "ops.transfer_head_grid_topk")


# ---------------------------------------------------------------- 2. independence of the schedule
def test_the_result_does_not_depend_on_the_workgroups():
    dims, shape = DIMS[0], (65, 130)    # 5 x 3 tiles of the head grid
    T = torch.from_numpy(T_MAX[:3]).to(DEV)
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, shape)
        Tk = T if kind == "viscosity" else None
        for k, largest in ((64, False), (1024, True)):
            first = head_topk(kind, mc, ma, Tk, wp, dims, k, largest, workgroups=0)
            same(first, data.grid_top_k(ops.head_grid(kind, mc, ma, Tk, wp, dims[1], dims[2]).cpu().numpy(), k, largest), kind)
            for g in (1, 2, 7, 1000):
                same(head_topk(kind, mc, ma, Tk, wp, dims, k, largest, workgroups=g), first, f"{kind} workgroups={g}")
    uc, ua, image = transfer_case(DIMS[0], (20, 70))   # 3 x 3 tiles of the transfer grid
    first = transfer_topk(uc, ua, image, 50, False)
    for g in (1, 2, 7):
        same(transfer_topk(uc, ua, image, 50, False, workgroups=g), first, f"transfer workgroups={g}")


# ---------------------------------------------------------------- 3. a bound that never helps, one that always does
def test_a_bound_that_never_helps_and_one_that_always_does():
    """C = 96, A = 64: six cation tiles, one anion tile, one workgroup.  Every value of tile t + 1 exceeds every value
    of tile t (asserted on the materialised grid), so with largest every candidate of every tile passes the bound and
    each tile forces a compaction, and with smallest nothing passes after the first tile."""
    kind, dims, (Cn, An) = "melting_point", DIMS[0], (96, 64)
    D, F, Mx = dims
    w = {n: np.abs(a) + np.float32(0.05) for n, a in head_weights(kind, D, F, Mx, seed=9).items()}   # Wh, Wo and the rest > 0
    wp = torch.from_numpy(pack(kind, w)).to(DEV)
    rng = np.random.default_rng(3)
    pc_h = (rng.uniform(1.0, 1.1, size=(Cn, D)) * (2.0 ** (np.arange(Cn) // 16))[:, None]).astype(np.float32)
    pa_h = rng.uniform(0.0, 0.01, size=(An, D)).astype(np.float32)
    mc = ops.head_ion_mix(kind, "cat", torch.from_numpy(pc_h).to(DEV), wp, F, Mx)
    ma = ops.head_ion_mix(kind, "an", torch.from_numpy(pa_h).to(DEV), wp, F, Mx)
    grid = ops.head_grid(kind, mc, ma, None, wp, F, Mx).cpu().numpy()
    tiles = grid.reshape(6, 16 * An)
    assert (tiles[1:].min(axis=1) > tiles[:-1].max(axis=1)).all(), "precondition: the tiles' values are separated"
    for largest in (True, False):
        same(head_topk(kind, mc, ma, None, wp, dims, 1024, largest, workgroups=1), data.grid_top_k(grid, 1024, largest),
             f"largest={largest}")
    same(head_topk(kind, mc, ma, None, wp, dims, 100, True, workgroups=1), data.grid_top_k(grid, 100, True), "k=100")


# ---------------------------------------------------------------- 4. ties
def test_ties_go_by_index():
    dims, (Cn, An) = DIMS[0], (20, 70)
    D, F, Mx = dims
    T = torch.from_numpy(T_MAX[:2]).to(DEV)
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, (Cn, An))
        mc[[3, 17, 19]] = mc[0].clone()          # duplicate cation rows and duplicate anion rows: equal values, other indices
        ma[[5, 64, 69]] = ma[2].clone()
        Tk = T if kind == "viscosity" else None
        grid = ops.head_grid(kind, mc, ma, Tk, wp, F, Mx).cpu().numpy()
        assert np.array_equal(bits(grid[3]), bits(grid[0])) and np.array_equal(bits(grid[:, 64]), bits(grid[:, 2]))
        for largest in (False, True):
            for k in (100, 1024):
                same(head_topk(kind, mc, ma, Tk, wp, dims, k, largest), data.grid_top_k(grid, k, largest), f"{kind} ties k={k}")
        # a head whose kernels are zero: every pair has the same value, the result is the first k flat indices
        w0 = head_weights(kind, D, F, Mx, seed=2)
        for n in w0:
            if n.endswith("kernel"):
                w0[n] = np.zeros_like(w0[n])
        wz = torch.from_numpy(pack(kind, w0)).to(DEV)
        flat_grid = ops.head_grid(kind, mc, ma, Tk, wz, F, Mx).cpu().numpy()
        assert len(np.unique(bits(flat_grid[..., 0] if kind == "viscosity" else flat_grid))) == 1
        for largest in (False, True):
            got = head_topk(kind, mc, ma, Tk, wz, dims, 100, largest)
            assert np.array_equal(got.cation * An + got.anion, np.broadcast_to(np.arange(100), got.cation.shape)), (kind, largest)
            same(got, data.grid_top_k(flat_grid, 100, largest), f"{kind} flat")
    uc, ua, image = transfer_case(DIMS[0], (20, 70))
    uc[[3, 19]] = uc[0].clone()
    ua[[33, 69]] = ua[1].clone()
    grid = ops.transfer_head_grid(uc, ua, image).cpu().numpy()
    for largest in (False, True):
        same(transfer_topk(uc, ua, image, 100, largest), data.grid_top_k(grid, 100, largest), "transfer ties")


# ---------------------------------------------------------------- 5. NaN
def test_a_nan_row_comes_last_in_both_directions():
    dims, (Cn, An) = DIMS[0], (17, 70)
    D, F, Mx = dims
    T = torch.from_numpy(T_MAX[:2]).to(DEV)
    row = 9
    cases = []
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, (Cn, An))
        mc[row] = float("nan")
        Tk = T if kind == "viscosity" else None
        grid = ops.head_grid(kind, mc, ma, Tk, wp, F, Mx).cpu().numpy()
        cases.append((kind, grid, lambda k, largest, a=(kind, mc, ma, Tk, wp): head_topk(*a, dims, k, largest)))
    uc, ua, image = transfer_case(DIMS[0], (Cn, An))
    uc[row] = float("nan")
    cases.append(("transfer", ops.transfer_head_grid(uc, ua, image).cpu().numpy(),
                  lambda k, largest: transfer_topk(uc, ua, image, k, largest)))
    assert 1024 <= (Cn - 1) * An
    for kind, grid, run in cases:
        assert np.isnan(grid[row]).all() and np.isfinite(np.delete(grid, row, axis=0)).all(), kind
        for largest in (False, True):
            for k in (500, 1024):        # k within the finite pairs: no pair of the NaN row appears
                got = run(k, largest)
                assert not (got.cation == row).any() and np.isfinite(got.values).all(), (kind, k, largest)
                same(got, data.grid_top_k(grid, k, largest), f"{kind} NaN k={k} largest={largest}")
    # k = C * A: the NaN pairs are the tail, as the quiet NaN, with their true indices
    dims, (Cn, An) = DIMS[0], (9, 33)
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, (Cn, An))
        mc[4] = float("nan")
        Tk = T if kind == "viscosity" else None
        grid = ops.head_grid(kind, mc, ma, Tk, wp, F, Mx).cpu().numpy()
        for largest in (False, True):
            got = head_topk(kind, mc, ma, Tk, wp, dims, Cn * An, largest)
            same(got, data.grid_top_k(grid, Cn * An, largest), f"{kind} k = C * A")
            tail = slice((Cn - 1) * An, None)
            assert (bits(got.values[:, tail]) == 0x7FC00000).all() and (got.cation[:, tail] == 4).all()
            assert np.array_equal(got.anion[:, tail], np.broadcast_to(np.arange(An), got.anion[:, tail].shape))
            assert np.isfinite(got.values[:, :(Cn - 1) * An]).all()
    uc, ua, image = transfer_case(DIMS[0], (Cn, An))
    uc[4] = float("nan")
    grid = ops.transfer_head_grid(uc, ua, image).cpu().numpy()
    for largest in (False, True):
        got = transfer_topk(uc, ua, image, Cn * An, largest)
        same(got, data.grid_top_k(grid, Cn * An, largest), "transfer k = C * A")
        assert (bits(got.values[:, (Cn - 1) * An:]) == 0x7FC00000).all() and (got.cation[:, (Cn - 1) * An:] == 4).all()


# ---------------------------------------------------------------- 6. model level
T2 = T5[[1, 3]]


def check_model(m, cat, an, T, ks, **kw):
    grid = m.predict_grid(cat, an, **({"temperatures": T} if T is not None else {}))
    Cn, An = grid.shape[:2]
    for k in ks:
        for largest in (False, True):
            got = m.screen_top_k(cat, an, temperatures=T, k=k, largest=largest, **kw)
            want = data.grid_top_k(grid, k, largest)
            assert got.values.shape == want.values.shape == ((len(T), min(k, Cn * An)) if T is not None else (min(k, Cn * An),))
            assert got.values.dtype == np.float32 and got.cation.dtype == np.int64 and got.anion.dtype == np.int64
            assert np.array_equal(bits(got.values), bits(want.values)), (k, largest, kw)
            assert np.array_equal(got.cation, want.cation) and np.array_equal(got.anion, want.anion), (k, largest, kw)


@pytest.fixture(scope="module")
def small_species():
    cat, _ = species(12, 70)
    _, an = species(9, 71)
    return cat, an


def test_model_viscosity_and_host_tiling(small_species):
    cat, an = small_species
    m, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=2)
    assert m._grid_kernels_cover()
    check_model(m, cat, an, T2, (1, 10, 100, 200))
    check_model(m, cat, an, T5, (7,))                         # five temperatures: two selecting launches per tile
    for pairs in (12 * 9, 4 * 9, 9):                          # 1, 3 and C cation tiles
        check_model(m, cat, an, T2, (10, 100), max_pairs_per_launch=pairs)
    empty = {k: v[:0] for k, v in cat.items()}
    got = m.screen_top_k(empty, an, temperatures=T2, k=5)
    assert got.values.shape == (2, 0) and got.cation.shape == (2, 0)


def test_model_melting_point(small_species):
    cat, an = small_species
    m, _ = make_model("melting_point", atom_dim=16, num_steps=2)
    check_model(m, cat, an, None, (1, 10, 200))
    check_model(m, cat, an, None, (10,), max_pairs_per_launch=2 * 9)


def test_model_transfer_and_its_gathered_mode(small_species, tmp_path):
    from test_gpu_transfer import make_transfer
    cat, an = small_species
    t = make_transfer(tmp_path, S=2)
    assert t._transfer_grid_covers() and t.grid_head_mode == "auto"
    check_model(t, cat, an, None, (1, 10, 200))
    check_model(t, cat, an, None, (10,), max_pairs_per_launch=3 * 9)
    t.grid_head_mode = "gathered"
    try:
        check_model(t, cat, an, None, (10, 200))
        check_model(t, cat, an, None, (10,), max_pairs_per_launch=9)
    finally:
        t.grid_head_mode = "auto"


def test_model_fallbacks_hold_the_same_order():
    cat, _ = species(40, 72)
    _, an = species(40, 73)
    m, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=1)
    assert 1500 > MM.SCREEN_MAX_K
    check_model(m, cat, an, T2, (1500,))                       # k above the kernels' limit, 40 x 40
    check_model(m, cat, an, T2, (1500,), max_pairs_per_launch=7 * 40)
    wide, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=1, fp_size=32, mixing_size=72, seed=6)
    assert not wide._grid_kernels_cover()
    sub_c, sub_a = {k: v[:12] for k, v in cat.items()}, {k: v[:9] for k, v in an.items()}
    check_model(wide, sub_c, sub_a, T2, (10, 200))
    check_model(wide, sub_c, sub_a, T2, (10,), max_pairs_per_launch=2 * 9)
