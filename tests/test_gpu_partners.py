"""Each ion's best partners on the GPU: impnn_head_grid_partners / impnn_transfer_head_grid_partners against
data.grid_best_partners of the materialised grid (impnn_head_grid / impnn_transfer_head_grid), with and without a pair
mask, and MPNNModel.screen_best_partners against data.grid_best_partners(predict_grid(...)).

Everything here is exact: a selected value is computed by the tile code of the materialising kernel, so values are
compared by their uint32 view, and the order (value, partner index; NaN last) is total, so indices are compared for
equality.  No tolerance appears."""
import ctypes as C

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, data, ops

from test_gpu_grid import DIMS, T5, bits, make_model, species
from test_gpu_screen import Guarded, T_MAX, head_case, transfer_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("viscosity", "melting_point")
HEAD_SHAPES = [(1, 1), (7, 63), (17, 130), (65, 130)]
TRANSFER_SHAPES = [(1, 1), (9, 33), (20, 70)]
MS = (1, 3, 8)
shape_id = lambda s: "%dx%d" % s
dims_id = lambda d: "D%d-F%d-Mx%d" % d


def dev_mask(b):
    return data.PairMask.from_bool(b, device=DEV)


# ---------------------------------------------------------------- guarded calls of the two entries
def call_partners(family, launch, Cn, An, nT, m):
    """One entry on guarded, pre-filled outputs and a guarded workspace of exactly the queried size -> BestPartners
    (planes, C, m) / (planes, A, m); no write outside, every output and workspace slot written, indices in range or
    -1 (then the value is the quiet NaN)."""
    lib = _lib.load()
    planes = max(nT, 1)
    need = C.c_size_t(0)
    _lib.check(lib.impnn_grid_partners_workspace_bytes(family, Cn, An, nT, m, C.byref(need)))
    out = [Guarded(planes * n * m * 4) for n in (Cn, Cn, An, An)]
    ws = Guarded(need.value)
    _lib.check(launch(lib, out[0].ptr, out[1].ptr, out[2].ptr, out[3].ptr, ws.ptr, need.value))
    torch.cuda.synchronize()
    filled = np.uint32(0xA5A5A5A5)
    sides = []
    for (v, p), n, others, what in ((out[:2], Cn, An, "cation"), (out[2:], An, Cn, "anion")):
        v = v.body(np.uint32, f"{what} values").reshape(planes, n, m)
        p = p.body(np.int32, f"{what} partners").reshape(planes, n, m)
        assert not (v == filled).any() and not (p.view(np.uint32) == filled).any(), f"a {what} output slot was not written"
        assert ((p >= -1) & (p < others)).all(), f"{what}: a partner index out of range"
        assert (v[p == -1] == 0x7FC00000).all(), f"{what}: an empty slot without the quiet NaN"
        sides.append(data.Partners(v.view(np.float32), p.astype(np.int64)))
    assert not (ws.body(np.uint64, "the workspace") == np.uint64(0xA5A5A5A5A5A5A5A5)).any(), "a workspace slot was not written"
    return data.BestPartners(*sides)


def head_partners(kind, mc, ma, T, wp, dims, m, largest, mask_b=None):
    D, F, Mx = dims
    Cn, An, nT = mc.shape[0], ma.shape[0], 0 if T is None else T.numel()
    words = dev_mask(mask_b).words if mask_b is not None else None
    launch = lambda lib, cv, cp, av, ap, ws, nb: lib.impnn_head_grid_partners(
        ops.HEAD_KINDS[kind], _lib.ptr(mc), _lib.ptr(ma), _lib.ptr(T) if T is not None else None, _lib.ptr(wp),
        _lib.ptr(words) if words is not None else None, m, int(largest), cv, cp, av, ap, ws, nb, Cn, An, nT, D, F, Mx,
        _lib.stream_ptr())
    return call_partners(0, launch, Cn, An, nT, m)


def transfer_partners(uc, ua, image, m, largest, mask_b=None):
    Cn, An = uc.shape[0], ua.shape[0]
    words = dev_mask(mask_b).words if mask_b is not None else None
    launch = lambda lib, cv, cp, av, ap, ws, nb: lib.impnn_transfer_head_grid_partners(
        _lib.ptr(uc), _lib.ptr(ua), _lib.ptr(image), image.numel(), _lib.ptr(words) if words is not None else None, m,
        int(largest), cv, cp, av, ap, ws, nb, Cn, An, _lib.stream_ptr())
    return call_partners(1, launch, Cn, An, 0, m)


def same(got, want, what):
    """got (planes, n, m) per side against data.grid_best_partners' (n, m) or (planes, n, m): values by bits."""
    for side, name in enumerate(("by_cation", "by_anion")):
        gv, gp = (np.asarray(x) for x in got[side])
        wv, wp = (np.asarray(x) for x in want[side])
        wv, wp = wv.reshape(gv.shape), wp.reshape(gp.shape)
        assert np.array_equal(bits(gv), bits(wv)), f"{what}: {name} values"
        assert np.array_equal(gp, wp), f"{what}: {name} partners"


def same_ops(got, want, what):
    """the four device tensors of an ops wrapper against the reference"""
    cv, cp, av, ap = got
    assert cv.is_cuda and cv.dtype == torch.float32 and cp.dtype == torch.int32 and av.shape == ap.shape
    same(data.BestPartners(data.Partners(cv.cpu().numpy(), cp.cpu().numpy().astype(np.int64)),
                           data.Partners(av.cpu().numpy(), ap.cpu().numpy().astype(np.int64))), want, what)


# ---------------------------------------------------------------- 1. the entries against the materialised grid
@pytest.mark.parametrize("dims", DIMS, ids=dims_id)
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=shape_id)
def test_head_partners_are_the_best_of_the_materialised_grid(shape, dims):
    D, F, Mx = dims
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, shape)
        for T_h in ((T_MAX[:1], T_MAX[:3], T_MAX) if kind == "viscosity" else (None,)):
            T = None if T_h is None else torch.from_numpy(T_h).to(DEV)
            grid = ops.head_grid(kind, mc, ma, T, wp, F, Mx).cpu().numpy()
            for largest in (False, True):
                for m in MS:
                    got = head_partners(kind, mc, ma, T, wp, dims, m, largest)
                    same(got, data.grid_best_partners(grid, m, largest),
                         f"{kind} {shape} {dims} nT={0 if T is None else len(T_h)} m={m} largest={largest}")
    kind = "viscosity"
    wp, mc, ma = head_case(kind, dims, shape)
    T = torch.from_numpy(T_MAX[:3]).to(DEV)
    got = ops.head_grid_partners(kind, mc, ma, T, wp, F, Mx, 3)
    assert tuple(got[0].shape) == (3, shape[0], 3) and tuple(got[3].shape) == (3, shape[1], 3)
    same_ops(got, data.grid_best_partners(ops.head_grid(kind, mc, ma, T, wp, F, Mx).cpu().numpy(), 3), "ops.head_grid_partners")


@pytest.mark.parametrize("shape", TRANSFER_SHAPES, ids=shape_id)
def test_transfer_partners_are_the_best_of_the_materialised_grid(shape):
    for dims in DIMS[:2]:
        uc, ua, image = transfer_case(dims, shape)
        grid = ops.transfer_head_grid(uc, ua, image).cpu().numpy()
        for largest in (False, True):
            for m in MS:
                same(transfer_partners(uc, ua, image, m, largest), data.grid_best_partners(grid, m, largest),
                     f"transfer {shape} {dims} m={m} largest={largest}")
    got = ops.transfer_head_grid_partners(uc, ua, image, 3, largest=True)
    assert tuple(got[0].shape) == (1, shape[0], 3) and tuple(got[2].shape) == (1, shape[1], 3)
    same_ops(got, data.grid_best_partners(grid, 3, True), "ops.transfer_head_grid_partners")


# ---------------------------------------------------------------- 2. masks
def masks_of(shape, tile):
    """density 0.5, empty, one set bit, and - on a shape with several tiles both ways - a block structure that leaves
    whole tiles (the skipped-tile path), one whole cation and one whole anion without a bit."""
    Cn, An = shape
    rng = np.random.default_rng(Cn * 1000 + An)
    one = np.zeros(shape, bool)
    one[Cn // 2, An - 1] = True
    out = [("half", rng.random(shape) < 0.5), ("empty", np.zeros(shape, bool)), ("one bit", one)]
    tc, ta = tile
    if Cn > 2 * tc and An > 2 * ta:
        blocks = rng.random(shape) < 0.5
        blocks[tc:2 * tc, :ta] = False           # whole tiles without a bit: a first, an interior and a ragged last one
        blocks[:tc, ta:2 * ta] = False
        blocks[2 * tc:, 2 * ta:] = False
        blocks[tc + 1, :] = False                # a cation and an anion without a bit
        blocks[:, ta + 3] = False
        assert blocks[:tc, :ta].any() and blocks[2 * tc:, :ta].any()
        out.append(("blocks", blocks))
    return out


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=shape_id)
def test_head_partners_under_a_mask(shape):
    dims = DIMS[0]
    D, F, Mx = dims
    masks = masks_of(shape, (16, 64))
    assert (shape == (65, 130)) == (len(masks) == 4)
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, shape)
        T = torch.from_numpy(T_MAX[:3]).to(DEV) if kind == "viscosity" else None
        grid = ops.head_grid(kind, mc, ma, T, wp, F, Mx).cpu().numpy()
        for name, mb in masks:
            for largest in (False, True):
                for m in MS:
                    want = data.grid_best_partners(grid, m, largest, where=mb)
                    same(head_partners(kind, mc, ma, T, wp, dims, m, largest, mb), want, f"{kind} {shape} {name} m={m} largest={largest}")
            for where in (dev_mask(mb), dev_mask(mb).words):
                same_ops(ops.head_grid_partners(kind, mc, ma, T, wp, F, Mx, 3, where=where),
                         data.grid_best_partners(grid, 3, where=mb), f"ops {kind} {name}")


@pytest.mark.parametrize("shape", TRANSFER_SHAPES, ids=shape_id)
def test_transfer_partners_under_a_mask(shape):
    masks = masks_of(shape, (8, 32))
    assert (shape == (20, 70)) == (len(masks) == 4)
    uc, ua, image = transfer_case(DIMS[0], shape)
    grid = ops.transfer_head_grid(uc, ua, image).cpu().numpy()
    for name, mb in masks:
        for largest in (False, True):
            for m in MS:
                same(transfer_partners(uc, ua, image, m, largest, mb), data.grid_best_partners(grid, m, largest, where=mb),
                     f"transfer {shape} {name} m={m} largest={largest}")
        same_ops(ops.transfer_head_grid_partners(uc, ua, image, 3, where=dev_mask(mb)),
                 data.grid_best_partners(grid, 3, where=mb), f"ops transfer {name}")


# ---------------------------------------------------------------- 3. ties and NaN
def test_ties_go_to_the_lower_index_on_both_axes():
    dims, (Cn, An) = DIMS[0], (20, 70)
    D, F, Mx = dims
    T = torch.from_numpy(T_MAX[:2]).to(DEV)
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, (Cn, An))
        mc[[3, 17, 19]] = mc[0].clone()          # equal rows: across two tiles of cations
        ma[[5, 64, 69]] = ma[2].clone()          # equal columns: across two tiles of anions
        Tk = T if kind == "viscosity" else None
        grid = ops.head_grid(kind, mc, ma, Tk, wp, F, Mx).cpu().numpy()
        assert np.array_equal(bits(grid[3]), bits(grid[0])) and np.array_equal(bits(grid[:, 64]), bits(grid[:, 2]))
        for largest in (False, True):
            got = head_partners(kind, mc, ma, Tk, wp, dims, 8, largest)
            same(got, data.grid_best_partners(grid, 8, largest), f"{kind} ties largest={largest}")
            for part, tied in ((got.by_cation.partner, (2, 5, 64, 69)), (got.by_anion.partner, (0, 3, 17, 19))):
                for row in part.reshape(-1, 8):   # where the tied partners appear they appear by index
                    seen = [int(x) for x in row if x in tied]
                    assert seen == sorted(seen)
    uc, ua, image = transfer_case(dims, (Cn, An))
    uc[[3, 19]] = uc[0].clone()
    ua[[33, 69]] = ua[1].clone()
    grid = ops.transfer_head_grid(uc, ua, image).cpu().numpy()
    assert np.array_equal(bits(grid[19]), bits(grid[0])) and np.array_equal(bits(grid[:, 69]), bits(grid[:, 1]))
    for largest in (False, True):
        same(transfer_partners(uc, ua, image, 8, largest), data.grid_best_partners(grid, 8, largest), "transfer ties")


def test_a_nan_ion_comes_last_for_every_partner():
    dims, (Cn, An), row = DIMS[0], (17, 70), 9
    D, F, Mx = dims
    T = torch.from_numpy(T_MAX[:2]).to(DEV)
    cases = []
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, (Cn, An))
        mc[row] = float("nan")
        Tk = T if kind == "viscosity" else None
        grid = ops.head_grid(kind, mc, ma, Tk, wp, F, Mx).cpu().numpy()
        cases.append((kind, grid, lambda m, largest, a=(kind, mc, ma, Tk, wp): head_partners(*a, dims, m, largest)))
    uc, ua, image = transfer_case(dims, (Cn, An))
    uc[row] = float("nan")
    cases.append(("transfer", ops.transfer_head_grid(uc, ua, image).cpu().numpy(),
                  lambda m, largest: transfer_partners(uc, ua, image, m, largest)))
    for kind, grid, run in cases:
        assert np.isnan(grid[row]).all()
        for largest in (False, True):
            got = run(8, largest)
            same(got, data.grid_best_partners(grid, 8, largest), f"{kind} NaN largest={largest}")
            assert not (got.by_anion.partner == row).any(), "16 finite cations come before the NaN one"
            assert (got.by_cation.partner[:, row] == np.arange(8)).all(), "its own row: all NaN, in order of index"
            assert (bits(got.by_cation.values[:, row]) == 0x7FC00000).all()
    # fewer finite cations than m: the NaN one is every anion's last partner
    wp, mc, ma = head_case("melting_point", dims, (3, An))
    mc[2] = float("nan")
    got = head_partners("melting_point", mc, ma, None, wp, dims, 3, False)
    same(got, data.grid_best_partners(ops.head_grid("melting_point", mc, ma, None, wp, F, Mx).cpu().numpy(), 3), "three cations")
    assert (got.by_anion.partner[0, :, 2] == 2).all()


# ---------------------------------------------------------------- 4. model level
T2 = T5[[1, 3]]


@pytest.fixture(scope="module")
def small_species():
    cat, _ = species(20, 70)
    _, an = species(9, 71)
    return cat, an


def check_model(m_, cat, an, T, ms=(1, 3), where_b=None, **kw):
    tk = {"temperatures": T} if T is not None else {}
    grid = m_.predict_grid(cat, an, **tk)
    for where in ((None,) if where_b is None else (dev_mask(where_b), data.PairMask.from_bool(where_b))):
        for m in ms:
            for largest in (False, True):
                got = m_.screen_best_partners(cat, an, m=m, largest=largest, where=where, **tk, **kw)
                want = data.grid_best_partners(grid, m, largest, where=where_b)
                for side in range(2):
                    assert got[side].values.shape == want[side].values.shape and got[side].partner.dtype == np.int64
                    assert np.array_equal(bits(got[side].values), bits(want[side].values)), (m, largest, kw, side)
                    assert np.array_equal(got[side].partner, want[side].partner), (m, largest, kw, side)
    return grid


def test_model_viscosity_and_melting_point(small_species):
    cat, an = small_species
    v, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=2)
    assert v._grid_kernels_cover()
    check_model(v, cat, an, T5)                                   # five temperatures: a split sweep
    mp, _ = make_model("melting_point", atom_dim=16, num_steps=2)
    grid = check_model(mp, cat, an, None, ms=(1, 8))
    assert grid.shape == (20, 9)
    check_model(v, cat, an, T2, ms=(9,))                          # m above the kernels' limit: the fallback
    check_model(v, cat, an, T2, ms=(9,), max_pairs_per_launch=7 * 9)
    empty = {k: x[:0] for k, x in cat.items()}
    got = v.screen_best_partners(empty, an, temperatures=T2, m=2)
    assert got.by_cation.values.shape == (2, 0, 2) and (got.by_anion.partner == -1).all() and got.by_anion.partner.shape == (2, 9, 2)
    with pytest.raises(ValueError, match="m must be >= 1"):
        v.screen_best_partners(cat, an, temperatures=T2, m=0)
    with pytest.raises(ValueError, match="screen_best_partners needs both"):
        v.screen_best_partners(cat, None, temperatures=T2)
    with pytest.raises(TypeError, match="data.PairMask"):
        v.screen_best_partners(cat, an, temperatures=T2, where=np.ones((20, 9), bool))


def test_the_result_does_not_depend_on_the_host_tiling(small_species):
    cat, an = small_species
    rng = np.random.default_rng(8)
    half = rng.random((20, 9)) < 0.5
    v, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=2)
    for where in (None, dev_mask(half)):
        whole = v.screen_best_partners(cat, an, temperatures=T2, m=3, where=where)
        for pairs in (7 * 9, 16 * 9):                             # a cut inside a 16-cation kernel tile, and one on its edge
            got = v.screen_best_partners(cat, an, temperatures=T2, m=3, where=where, max_pairs_per_launch=pairs)
            for side in range(2):
                assert np.array_equal(bits(got[side].values), bits(whole[side].values)), (pairs, side)
                assert np.array_equal(got[side].partner, whole[side].partner), (pairs, side)
    check_model(v, cat, an, T2, ms=(3,), where_b=half, max_pairs_per_launch=7 * 9)


def test_model_transfer_modes_and_an_uncovered_width(small_species, tmp_path):
    from test_gpu_transfer import make_transfer
    cat, an = small_species
    half = np.random.default_rng(9).random((20, 9)) < 0.5
    t = make_transfer(tmp_path, S=2)
    assert t._transfer_grid_covers() and t.grid_head_mode == "auto"
    check_model(t, cat, an, None)
    check_model(t, cat, an, None, ms=(2,), where_b=half, max_pairs_per_launch=5 * 9)
    t.grid_head_mode = "gathered"
    try:
        check_model(t, cat, an, None, ms=(2,))
        check_model(t, cat, an, None, ms=(2,), where_b=half, max_pairs_per_launch=5 * 9)
    finally:
        t.grid_head_mode = "auto"
    wide, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=1, fp_size=32, mixing_size=72, seed=6)
    assert not wide._grid_kernels_cover()
    check_model(wide, cat, an, T2, ms=(2,), max_pairs_per_launch=6 * 9)


def test_model_where_from_screen_mask_and_the_top_1(small_species):
    cat, an = small_species
    v, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=2)
    grid = v.predict_grid(cat, an, temperatures=T2[:1])
    liquid = v.screen_mask(cat, an, temperatures=T2[:1], at_most=float(np.median(grid))).temperature(0)
    where_b = grid[:, :, 0] <= np.float32(np.median(grid))
    assert np.array_equal(liquid.to_bool(), where_b) and where_b.any() and not where_b.all()
    check_model(v, cat, an, T2, ms=(2,), where_b=where_b)
    got = v.screen_best_partners(cat, an, temperatures=T2, m=2, where=liquid)
    want = data.grid_best_partners(v.predict_grid(cat, an, temperatures=T2), 2, where=where_b)
    assert np.array_equal(got.by_anion.partner, want.by_anion.partner) and np.array_equal(got.by_cation.partner, want.by_cation.partner)
    for largest in (False, True):                                 # by_cation at m = 1, reduced over the cations, is the top 1
        b = v.screen_best_partners(cat, an, temperatures=T2, m=1, largest=largest)
        top = v.screen_top_k(cat, an, temperatures=T2, k=1, largest=largest)
        for t in range(2):
            i = int(data.top_k_order(b.by_cation.values[t, :, 0], np.arange(20), 1, largest)[0])
            assert i == top.cation[t, 0] and b.by_cation.partner[t, i, 0] == top.anion[t, 0]
            assert bits(b.by_cation.values[t, i, 0]) == bits(top.values[t, 0])
