"""The rank cut and the best-k pair mask on the GPU: impnn_head_grid_rank / impnn_transfer_head_grid_rank against
data.grid_rank and data.grid_best_mask of the materialised grid (impnn_head_grid / impnn_transfer_head_grid), with and
without a pair mask, and MPNNModel.screen_rank / screen_best_mask against the same references on predict_grid(...).

Everything here is exact: an entry's value is computed by the tile code of the materialising kernel, so values are
compared by their uint32 view, and the order (value, cation index, anion index; NaN last) is total, so indices and
mask words are compared for equality.  No tolerance appears."""
import ctypes as C

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, data, ops

from test_gpu_grid import DIMS, T5, bits, make_model, species
from test_gpu_screen import FILL, GUARD, Guarded, T_MAX, head_case, transfer_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("viscosity", "melting_point")
HEAD_SHAPES = [(1, 1), (7, 63), (17, 130), (65, 130)]
TRANSFER_SHAPES = [(1, 1), (9, 33), (20, 70)]
shape_id = lambda s: "%dx%d" % s
dims_id = lambda d: "D%d-F%d-Mx%d" % d


def ks_of(n):
    """1, 2, the middle, the last but one, the last, and past the end"""
    return sorted({1, 2, max(n // 2, 1), max(n - 1, 1), n, n + 5})


def dev_mask(b):
    return data.PairMask.from_bool(b, device=DEV)


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


# ---------------------------------------------------------------- guarded calls of the two entries
def call_rank(family, launch, Cn, An, nT, workgroups=0, ones=False):
    """One entry on guarded, pre-filled outputs, mask words and a guarded workspace of exactly the queried size ->
    (data.RankCut of arrays (planes,), words uint32 (planes, C, W)); no write outside, every output and every mask word
    written.  ``ones``: the mask words hold all ones before the call (what a tile that is passed over must replace)."""
    lib = _lib.load()
    planes, W = max(nT, 1), (An + 31) // 32
    need = C.c_size_t(0)
    _lib.check(lib.impnn_grid_rank_workspace_bytes(family, Cn, An, nT, workgroups, C.byref(need)))
    v, ci, ai, n = Guarded(planes * 4), Guarded(planes * 4), Guarded(planes * 4), Guarded(planes * 8)
    words, ws = Guarded(planes * Cn * W * 4), Guarded(need.value)
    if ones:
        words.whole[GUARD:GUARD + words.n] = 0xFF
    _lib.check(launch(lib, v.ptr, ci.ptr, ai.ptr, n.ptr, words.ptr, ws.ptr, need.value))
    torch.cuda.synchronize()
    v, ci, ai = v.body(np.uint32, "values"), ci.body(np.int32, "cation"), ai.body(np.int32, "anion")
    n, words = n.body(np.int64, "count"), words.body(np.uint32, "the mask words").reshape(planes, Cn, W)
    ws.body(np.uint8, "the workspace")
    filled = np.uint32(FILL * 0x01010101)
    assert not (v == filled).any() and not (ci.view(np.uint32) == filled).any() and not (ai.view(np.uint32) == filled).any() \
        and (n >= 0).all() and (n <= Cn * An).all(), "an output slot was not written"
    if not ones:  # (a word of all ones can be a result)
        assert not (words == filled).any(), "a mask word was not written"
    if An % 32:
        assert not (words[:, :, -1] >> np.uint32(An % 32)).any(), "a pad bit is set"
    assert ((ci >= 0) & (ci < Cn) & (ai >= 0) & (ai < An) | (ci == -1) & (ai == -1) & (v == 0x7FC00000)).all()
    return data.RankCut(v.view(np.float32), ci.astype(np.int64), ai.astype(np.int64), n.copy()), words


def head_rank(kind, mc, ma, T, wp, dims, k, largest, mask_b=None, **kw):
    D, F, Mx = dims
    Cn, An, nT = mc.shape[0], ma.shape[0], 0 if T is None else T.numel()
    where = dev_mask(mask_b).words if mask_b is not None else None
    launch = lambda lib, v, ci, ai, n, words, ws, nb: lib.impnn_head_grid_rank(
        ops.HEAD_KINDS[kind], _lib.ptr(mc), _lib.ptr(ma), _lib.ptr(T) if T is not None else None, _lib.ptr(wp), k, int(largest),
        _lib.ptr(where) if where is not None else None, v, ci, ai, n, words, ws, nb, Cn, An, nT, D, F, Mx,
        kw.get("workgroups", 0), _lib.stream_ptr())
    return call_rank(0, launch, Cn, An, nT, **kw)


def transfer_rank(uc, ua, image, k, largest, mask_b=None, **kw):
    Cn, An = uc.shape[0], ua.shape[0]
    where = dev_mask(mask_b).words if mask_b is not None else None
    launch = lambda lib, v, ci, ai, n, words, ws, nb: lib.impnn_transfer_head_grid_rank(
        _lib.ptr(uc), _lib.ptr(ua), _lib.ptr(image), image.numel(), k, int(largest),
        _lib.ptr(where) if where is not None else None, v, ci, ai, n, words, ws, nb, Cn, An, kw.get("workgroups", 0),
        _lib.stream_ptr())
    return call_rank(1, launch, Cn, An, 0, **kw)


def same(got, grid, k, largest, what, where_b=None):
    """(cut, words) of call_rank against the references on the materialised grid: values by bits, the rest exactly; the
    mask holds exactly min(k, competing) bits per plane."""
    cut, words = got
    want = data.grid_rank(grid, k, largest, where=where_b)
    wv, wc, wa, wn = (np.atleast_1d(x) for x in want)
    assert np.array_equal(bits(cut.values), bits(wv)), f"{what}: values"
    assert np.array_equal(cut.cation, wc) and np.array_equal(cut.anion, wa), f"{what}: indices"
    assert np.array_equal(cut.count, wn), f"{what}: count"
    ref = data.PairMask.from_bool(data.grid_best_mask(grid, k, largest, where=where_b))._host_words().reshape(words.shape)
    assert np.array_equal(words, ref), f"{what}: mask words"
    competing = grid.shape[0] * grid.shape[1] if where_b is None else int(where_b.sum())
    for t in range(words.shape[0]):
        assert popcount(words[t]) == min(k, competing), f"{what}: bits of plane {t}"


# ---------------------------------------------------------------- 1. the entries against the materialised grid
@pytest.mark.parametrize("dims", DIMS, ids=dims_id)
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=shape_id)
def test_head_rank_is_the_order_statistic_of_the_materialised_grid(shape, dims):
    D, F, Mx = dims
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, shape)
        for T_h in ((T_MAX[:1], T_MAX[:3], T_MAX) if kind == "viscosity" else (None,)):
            T = None if T_h is None else torch.from_numpy(T_h).to(DEV)
            grid = ops.head_grid(kind, mc, ma, T, wp, F, Mx).cpu().numpy()
            for largest in (False, True):
                for k in ks_of(shape[0] * shape[1]):
                    same(head_rank(kind, mc, ma, T, wp, dims, k, largest), grid, k, largest,
                         f"{kind} {shape} {dims} nT={0 if T is None else len(T_h)} k={k} largest={largest}")
    # the public wrapper: the same results on the device, with and without the mask
    kind = "viscosity"
    wp, mc, ma = head_case(kind, dims, shape)
    T = torch.from_numpy(T_MAX[:3]).to(DEV)
    grid = ops.head_grid(kind, mc, ma, T, wp, F, Mx).cpu().numpy()
    k = max(shape[0] * shape[1] // 3, 1)
    v, ci, ai, n, words = ops.head_grid_rank(kind, mc, ma, T, wp, F, Mx, k, mask=True)
    assert v.is_cuda and tuple(v.shape) == (3,) and ci.dtype == torch.int32 and n.dtype == torch.int64
    assert tuple(words.shape) == (3, shape[0], (shape[1] + 31) // 32) and words.dtype == torch.int32
    got = data.RankCut(v.cpu().numpy(), ci.cpu().numpy().astype(np.int64), ai.cpu().numpy().astype(np.int64), n.cpu().numpy())
    same((got, words.cpu().numpy().view(np.uint32)), grid, k, False, "ops.head_grid_rank")
    assert ops.head_grid_rank(kind, mc, ma, T, wp, F, Mx, k)[4] is None
    mask = data.PairMask(words, shape + (3,))
    assert np.array_equal(mask.to_bool(), data.grid_best_mask(grid, k)) and mask.count().tolist() == [k] * 3


@pytest.mark.parametrize("shape", TRANSFER_SHAPES, ids=shape_id)
def test_transfer_rank_is_the_order_statistic_of_the_materialised_grid(shape):
    for dims in DIMS[:2]:
        uc, ua, image = transfer_case(dims, shape)
        grid = ops.transfer_head_grid(uc, ua, image).cpu().numpy()
        for largest in (False, True):
            for k in ks_of(shape[0] * shape[1]):
                same(transfer_rank(uc, ua, image, k, largest), grid, k, largest, f"transfer {shape} {dims} k={k} largest={largest}")
    k = max(shape[0] * shape[1] // 3, 1)
    v, ci, ai, n, words = ops.transfer_head_grid_rank(uc, ua, image, k, largest=True, mask=True)
    assert tuple(v.shape) == (1,) and tuple(words.shape) == (shape[0], (shape[1] + 31) // 32)
    got = data.RankCut(v.cpu().numpy(), ci.cpu().numpy().astype(np.int64), ai.cpu().numpy().astype(np.int64), n.cpu().numpy())
    same((got, words.cpu().numpy().view(np.uint32)[None]), grid, k, True, "ops.transfer_head_grid_rank")


# ---------------------------------------------------------------- 2. ties and NaN
def test_the_k_th_entry_inside_a_run_of_equal_values():
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
        plane = grid.reshape(Cn, An, -1)[:, :, 0]
        for largest in (False, True):
            first = data.grid_top_k(plane, Cn * An, largest)
            run = np.flatnonzero(bits(first.values) == bits(plane[0, 2]))   # sixteen equal values: 4 rows x 4 columns
            assert len(run) == 16 and run[-1] - run[0] == 15
            for k in (int(run[0]) + 1, int(run[0]) + 2, int(run[7]) + 1, int(run[15]) + 1):   # k-th entries inside the run
                same(head_rank(kind, mc, ma, Tk, wp, dims, k, largest), grid, k, largest, f"{kind} ties k={k} largest={largest}")
    uc, ua, image = transfer_case(dims, (Cn, An))
    uc[[3, 19]] = uc[0].clone()
    ua[[33, 69]] = ua[1].clone()
    grid = ops.transfer_head_grid(uc, ua, image).cpu().numpy()
    first = data.grid_top_k(grid, Cn * An)
    run = np.flatnonzero(bits(first.values) == bits(grid[0, 1]))
    assert len(run) == 9
    for largest in (False, True):
        for k in (int(run[0]) + 2, int(run[4]) + 1, Cn * An - int(run[4])):
            same(transfer_rank(uc, ua, image, k, largest), grid, k, largest, f"transfer ties k={k} largest={largest}")


def test_a_grid_of_one_value_is_cut_by_index_alone():
    dims, (Cn, An), k = DIMS[0], (17, 130), 1105
    D, F, Mx = dims
    T = torch.from_numpy(T_MAX[:2]).to(DEV)
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, (Cn, An))
        mc[:] = mc[0].clone()                    # identical pooled rows: the key passes see one bin
        ma[:] = ma[0].clone()
        Tk = T if kind == "viscosity" else None
        grid = ops.head_grid(kind, mc, ma, Tk, wp, F, Mx).cpu().numpy()
        assert len(np.unique(bits(grid.reshape(Cn * An, -1)[:, 0]))) == 1
        for largest in (False, True):
            got = head_rank(kind, mc, ma, Tk, wp, dims, k, largest)
            same(got, grid, k, largest, f"{kind} one value largest={largest}")
            assert (got[0].cation == (k - 1) // An).all() and (got[0].anion == (k - 1) % An).all()
    uc, ua, image = transfer_case(dims, (Cn, An))
    uc[:] = uc[0].clone()
    ua[:] = ua[0].clone()
    grid = ops.transfer_head_grid(uc, ua, image).cpu().numpy()
    assert len(np.unique(bits(grid))) == 1
    got = transfer_rank(uc, ua, image, k, True)
    same(got, grid, k, True, "transfer one value")
    assert got[0].cation[0] == (k - 1) // An and got[0].anion[0] == (k - 1) % An


def test_nan_ions_come_last_in_both_directions():
    dims, (Cn, An), row, col = DIMS[0], (17, 70), 9, 40
    D, F, Mx = dims
    T = torch.from_numpy(T_MAX[:2]).to(DEV)
    n_nan, n = An + Cn - 1, Cn * An
    cases = []
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, (Cn, An))
        mc[row], ma[col] = float("nan"), float("nan")
        Tk = T if kind == "viscosity" else None
        grid = ops.head_grid(kind, mc, ma, Tk, wp, F, Mx).cpu().numpy()
        cases.append((kind, grid, lambda k, largest, a=(kind, mc, ma, Tk, wp): head_rank(*a, dims, k, largest)))
    uc, ua, image = transfer_case(dims, (Cn, An))
    uc[row], ua[col] = float("nan"), float("nan")
    cases.append(("transfer", ops.transfer_head_grid(uc, ua, image).cpu().numpy(),
                  lambda k, largest: transfer_rank(uc, ua, image, k, largest)))
    for kind, grid, run in cases:
        assert np.isnan(grid[row]).all() and np.isnan(grid[:, col]).all() and np.isnan(grid).sum() == n_nan * grid[0, 0].size
        for largest in (False, True):
            for k in (n - n_nan, n - n_nan + 1, n - 3, n):       # the last finite entry, the first NaN, inside them, the last
                got = run(k, largest)
                same(got, grid, k, largest, f"{kind} NaN k={k} largest={largest}")
                nan_set = got[1][0, row].any() or (got[1][0, :, col // 32] >> np.uint32(col % 32) & 1).any()
                assert nan_set == (k > n - n_nan), "NaN pairs are set once k reaches them, not before"
            first_nan = run(n - n_nan + 1, largest)[0]
            assert (first_nan.cation == 0).all() and (first_nan.anion == col).all() and (bits(first_nan.values) == 0x7FC00000).all()


# ---------------------------------------------------------------- 3. masks
def masks_of(shape, tile):
    """density 0.5, empty, all ones, and - on a shape with several tiles both ways - a block structure that leaves whole
    tiles (the passed-over path: a first, an interior and a ragged last one)."""
    Cn, An = shape
    rng = np.random.default_rng(Cn * 1000 + An)
    out = [("half", rng.random(shape) < 0.5), ("empty", np.zeros(shape, bool)), ("ones", np.ones(shape, bool))]
    tc, ta = tile
    if Cn > 2 * tc and An > 2 * ta:
        blocks = rng.random(shape) < 0.5
        blocks[tc:2 * tc, :ta] = False
        blocks[:tc, ta:2 * ta] = False
        blocks[2 * tc:, 2 * ta:] = False
        assert blocks[:tc, :ta].any() and blocks[2 * tc:, :ta].any()
        out.append(("blocks", blocks))
    return out


def check_masks(shape, masks, grid, run):
    for name, mb in masks:
        n = int(mb.sum())
        for largest in (False, True):
            for k in ks_of(max(n, 1)):
                got = run(k, largest, mb, ones=name in ("blocks", "empty"))
                same(got, grid, k, largest, f"{shape} {name} k={k} largest={largest}", where_b=mb)
                if name == "empty":
                    assert (got[0].count == 0).all() and not got[1].any() and (got[0].cation == -1).all()
                if name == "ones":
                    assert np.array_equal(got[1], run(k, largest, None)[1]), "all ones: the words of the unmasked call"


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=shape_id)
def test_head_rank_under_a_mask(shape):
    dims = DIMS[0]
    D, F, Mx = dims
    masks = masks_of(shape, (16, 64))
    assert (shape == (65, 130)) == (len(masks) == 4)
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, shape)
        T = torch.from_numpy(T_MAX[:3]).to(DEV) if kind == "viscosity" else None
        grid = ops.head_grid(kind, mc, ma, T, wp, F, Mx).cpu().numpy()
        check_masks(shape, masks, grid, lambda k, largest, mb, **kw: head_rank(kind, mc, ma, T, wp, dims, k, largest, mb, **kw))
        mb = masks[0][1]
        for where in (dev_mask(mb), dev_mask(mb).words):
            words = ops.head_grid_rank(kind, mc, ma, T, wp, F, Mx, 5, where=where, mask=True)[4]
            want = data.PairMask.from_bool(data.grid_best_mask(grid, 5, where=mb))
            assert np.array_equal(words.cpu().numpy(), want.words.numpy())


@pytest.mark.parametrize("shape", TRANSFER_SHAPES, ids=shape_id)
def test_transfer_rank_under_a_mask(shape):
    masks = masks_of(shape, (8, 32))
    assert (shape == (20, 70)) == (len(masks) == 4)
    uc, ua, image = transfer_case(DIMS[0], shape)
    grid = ops.transfer_head_grid(uc, ua, image).cpu().numpy()
    check_masks(shape, masks, grid, lambda k, largest, mb, **kw: transfer_rank(uc, ua, image, k, largest, mb, **kw))


# ---------------------------------------------------------------- 4. the schedule
def test_the_result_does_not_depend_on_the_workgroups():
    dims, shape = DIMS[0], (65, 130)
    D, F, Mx = dims
    half = np.random.default_rng(4).random(shape) < 0.5
    T = torch.from_numpy(T_MAX).to(DEV)
    wp, mc, ma = head_case("viscosity", dims, shape)
    grid = ops.head_grid("viscosity", mc, ma, T, wp, F, Mx).cpu().numpy()
    uc, ua, image = transfer_case(dims, (20, 70))
    tgrid = ops.transfer_head_grid(uc, ua, image).cpu().numpy()
    for mb, tb in ((None, None), (half, half[:20, :70])):
        for k in (77, 4000):
            for g in (1, 3, 0):
                same(head_rank("viscosity", mc, ma, T, wp, dims, k, False, mb, workgroups=g), grid, k, False,
                     f"head workgroups={g} k={k}", where_b=mb)
                same(transfer_rank(uc, ua, image, k // 7, True, tb, workgroups=g), tgrid, k // 7, True,
                     f"transfer workgroups={g} k={k // 7}", where_b=tb)


# ---------------------------------------------------------------- 5. model level
T2 = T5[[1, 3]]


@pytest.fixture(scope="module")
def small_species():
    cat, _ = species(20, 70)
    _, an = species(9, 71)
    return cat, an


def check_model(m_, cat, an, T, ks, where_b=None):
    tk = {"temperatures": T} if T is not None else {}
    grid = m_.predict_grid(cat, an, **tk)
    for where in ((None,) if where_b is None else (dev_mask(where_b), data.PairMask.from_bool(where_b))):
        for k in ks:
            for largest in (False, True):
                mask = m_.screen_best_mask(cat, an, k=k, largest=largest, where=where, **tk)
                want = data.PairMask.from_bool(data.grid_best_mask(grid, k, largest, where=where_b))
                assert mask.shape == want.shape == grid.shape and mask.words.is_cuda
                assert np.array_equal(mask.words.cpu().numpy(), want.words.numpy()), (k, largest)
                cut = m_.screen_rank(cat, an, k=k, largest=largest, where=where, **tk)
                ref = data.grid_rank(grid, k, largest, where=where_b)
                assert np.shape(cut.values) == np.shape(ref.values) == ((len(T),) if T is not None else ())
                assert np.array_equal(bits(cut.values), bits(ref.values)), (k, largest)
                assert np.array_equal(cut.cation, ref.cation) and np.array_equal(cut.anion, ref.anion), (k, largest)
                assert np.array_equal(cut.count, ref.count) and np.asarray(cut.cation).dtype == np.int64
    return grid


def test_model_viscosity_and_melting_point(small_species):
    cat, an = small_species
    half = np.random.default_rng(8).random((20, 9)) < 0.5
    v, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=2)
    assert v._grid_kernels_cover()
    check_model(v, cat, an, T5, ks=(1, 60, 180, 200))             # five temperatures: a split sweep
    check_model(v, cat, an, T2, ks=(40,), where_b=half)
    mp, _ = make_model("melting_point", atom_dim=16, num_steps=2)
    grid = check_model(mp, cat, an, None, ks=(1, 90, 2000))
    assert grid.shape == (20, 9)
    check_model(mp, cat, an, None, ks=(30,), where_b=half)
    empty = {k: x[:0] for k, x in cat.items()}
    got = v.screen_best_mask(empty, an, temperatures=T2, k=2)
    assert got.shape == (0, 9, 2) and tuple(got.words.shape) == (2, 0, 1)
    cut = v.screen_rank(empty, an, temperatures=T2, k=2)
    assert cut.count.tolist() == [0, 0] and cut.cation.tolist() == [-1, -1] and (bits(cut.values) == 0x7FC00000).all()


def test_model_transfer_modes_and_an_uncovered_width(small_species, tmp_path):
    from test_gpu_transfer import make_transfer
    cat, an = small_species
    half = np.random.default_rng(9).random((20, 9)) < 0.5
    t = make_transfer(tmp_path, S=2)
    assert t._transfer_grid_covers() and t.grid_head_mode == "auto"
    check_model(t, cat, an, None, ks=(1, 45, 181))
    check_model(t, cat, an, None, ks=(20,), where_b=half)
    t.grid_head_mode = "gathered"
    try:
        check_model(t, cat, an, None, ks=(45,))
        check_model(t, cat, an, None, ks=(20,), where_b=half)
    finally:
        t.grid_head_mode = "auto"
    wide, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=1, fp_size=32, mixing_size=72, seed=6)
    assert not wide._grid_kernels_cover()
    check_model(wide, cat, an, T2, ks=(45,))
    check_model(wide, cat, an, T2, ks=(20,), where_b=half)


def test_the_best_of_the_liquid_pairs_then_each_cations_partners(small_species):
    cat, an = small_species
    mp_model, _ = make_model("melting_point", atom_dim=16, num_steps=2)
    visc_model, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=2)
    mp_grid = mp_model.predict_grid(cat, an)
    limit_scaled = float(np.median(mp_grid))
    liquid = mp_model.screen_mask(cat, an, at_most=limit_scaled)
    k = liquid.count() // 10
    assert k >= 5
    best = visc_model.screen_best_mask(cat, an, [298.15], k=k, where=liquid).temperature(0)
    per_cation = visc_model.screen_best_partners(cat, an, [298.15], m=3, where=best)
    grid = visc_model.predict_grid(cat, an, temperatures=[298.15])
    want_best = data.grid_best_mask(grid, k, where=mp_grid <= np.float32(limit_scaled))[:, :, 0]
    assert best.count() == k and np.array_equal(best.to_bool(), want_best)
    want = data.grid_best_partners(grid, 3, where=want_best)
    assert np.array_equal(per_cation.by_cation.partner, want.by_cation.partner)
    assert np.array_equal(bits(per_cation.by_cation.values), bits(want.by_cation.values))
    top = visc_model.screen_top_k(cat, an, [298.15], k=k, where=liquid)
    assert np.array_equal(np.sort(top.cation[0] * 9 + top.anion[0]), np.flatnonzero(want_best.reshape(-1)))
