"""Constrained screening on the GPU: the mask-writing entries (impnn_head_grid_mask, impnn_transfer_head_grid_mask)
against the comparison on the materialised grid, the masked selecting entries (impnn_head_grid_topk_where,
impnn_transfer_head_grid_topk_where) against data.grid_top_k(grid, where=), and MPNNModel.screen_mask /
screen_top_k(where=) against the same on predict_grid.

Everything here is exact: the kernels run the materialising kernel's tile code, so a tested or selected value has the
grid's bits; mask words are compared as integers, values by their uint32 view, indices for equality.  No tolerance
appears."""
import ctypes as C

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, data, model as MM, ops

from test_gpu_grid import DIMS, T5, bits, make_model, species
from test_gpu_screen import Guarded, T_MAX, head_case, same, transfer_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("viscosity", "melting_point")
GUARD = 256
INF = np.float32(np.inf)
HEAD_SHAPES = [(1, 1), (7, 63), (17, 130), (65, 130)]
TRANSFER_SHAPES = [(1, 1), (9, 33), (20, 70)]
shape_id = lambda s: "%dx%d" % s
dims_id = lambda d: "D%d-F%d-Mx%d" % d


def words_of(b):
    """The reference words of a bool array (C,A) or (C,A,nT) -> uint32 (C,W) or (nT,C,W)."""
    return data.PairMask.from_bool(b).words.numpy().view(np.uint32)


# ---------------------------------------------------------------- 1. the mask entries against the materialised grid
def run_mask(launch, planes, Cn, An):
    """One mask entry on a buffer that holds 0xFF everywhere, guards included -> uint32 words (planes, C, W)."""
    W = (An + 31) // 32
    n = planes * Cn * W * 4
    whole = torch.full((GUARD + n + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    assert whole.data_ptr() % 4 == 0
    _lib.check(launch(_lib.load(), C.c_void_p(whole.data_ptr() + GUARD)))
    torch.cuda.synchronize()
    host = whole.cpu().numpy()
    assert (host[:GUARD] == 0xFF).all() and (host[GUARD + n:] == 0xFF).all(), "a write outside the mask"
    return host[GUARD:GUARD + n].view(np.uint32).reshape(planes, Cn, W)


def bounds_of(g):
    """The bounds every mask case runs: no limit, nothing, one value of the grid (inclusive), a median split."""
    fin = g[np.isfinite(g)]
    one = fin[len(fin) // 3]
    return [(-INF, INF), (INF, INF), (one, one), (-INF, np.float32(np.median(fin))), (np.float32(np.median(fin)), INF)]


def check_mask(run, g, what):
    Cn, An = g.shape[:2]
    with np.errstate(invalid="ignore"):
        for lo, hi in bounds_of(g):
            want = (g >= lo) & (g <= hi)
            got = run(float(lo), float(hi))
            assert np.array_equal(got, words_of(want).reshape(got.shape)), f"{what} [{lo}, {hi}]"
            if lo == hi and np.isfinite(lo):
                assert want.any(), "the inclusive test hits the pair the value came from"
            if lo == -INF and hi == INF:
                assert int(want.sum()) == int((~np.isnan(g)).sum())
            if lo == INF:
                assert not got.any()


@pytest.mark.parametrize("dims", DIMS, ids=dims_id)
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=shape_id)
def test_head_mask_is_the_comparison_on_the_materialised_grid(shape, dims):
    D, F, Mx = dims
    Cn, An = shape
    lib = _lib.load()
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, shape)
        for T_h in ((T_MAX[:1], T_MAX[:3]) if kind == "viscosity" else (None,)):
            T = None if T_h is None else torch.from_numpy(T_h).to(DEV)
            nT = 0 if T is None else T.numel()
            g = ops.head_grid(kind, mc, ma, T, wp, F, Mx).cpu().numpy()
            run = lambda lo, hi: run_mask(lambda lib, words: lib.impnn_head_grid_mask(
                ops.HEAD_KINDS[kind], _lib.ptr(mc), _lib.ptr(ma), _lib.ptr(T) if T is not None else None, _lib.ptr(wp), lo, hi,
                words, Cn, An, nT, D, F, Mx, _lib.stream_ptr()), max(nT, 1), Cn, An)
            check_mask(run, g, f"{kind} {shape} {dims} nT={nT}")     # (viscosity: each plane against its temperature)
    # the public wrapper: the words of a PairMask
    wp, mc, ma = head_case("viscosity", dims, shape)
    T = torch.from_numpy(T_MAX[:3]).to(DEV)
    g = ops.head_grid("viscosity", mc, ma, T, wp, F, Mx).cpu().numpy()
    med = np.float32(np.median(g))
    words = ops.head_grid_mask("viscosity", mc, ma, T, wp, F, Mx, -np.inf, med)
    assert words.dtype == torch.int32 and tuple(words.shape) == (3, Cn, lib.impnn_grid_mask_row_words(An)) and words.is_cuda
    m = data.PairMask(words, (Cn, An, 3))
    assert np.array_equal(m.to_bool(), g <= med) and m.count().tolist() == (g <= med).sum(axis=(0, 1)).tolist()
    for t in range(3):
        assert np.array_equal(m.temperature(t).to_bool(), g[:, :, t] <= med)


@pytest.mark.parametrize("shape", TRANSFER_SHAPES, ids=shape_id)
def test_transfer_mask_is_the_comparison_on_the_materialised_grid(shape):
    Cn, An = shape
    for dims in DIMS[:2]:
        uc, ua, image = transfer_case(dims, shape)
        g = ops.transfer_head_grid(uc, ua, image).cpu().numpy()
        run = lambda lo, hi: run_mask(lambda lib, words: lib.impnn_transfer_head_grid_mask(
            _lib.ptr(uc), _lib.ptr(ua), _lib.ptr(image), image.numel(), lo, hi, words, Cn, An, _lib.stream_ptr()), 1, Cn, An)
        check_mask(run, g, f"transfer {shape} {dims}")
    med = np.float32(np.median(g))
    m = data.PairMask(ops.transfer_head_grid_mask(uc, ua, image, med, np.inf), (Cn, An))
    assert np.array_equal(m.to_bool(), g >= med)


def test_a_nan_row_or_column_has_no_bits():
    dims, (Cn, An), row, col = DIMS[0], (17, 70), 9, 65
    D, F, Mx = dims
    T = torch.from_numpy(T_MAX[:2]).to(DEV)
    cases = []
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, (Cn, An))
        mc[row] = float("nan")
        ma[col] = float("nan")
        Tk = T if kind == "viscosity" else None
        g = ops.head_grid(kind, mc, ma, Tk, wp, F, Mx).cpu().numpy()
        cases.append((kind, g, lambda lo, hi, a=(kind, mc, ma, Tk, wp): ops.head_grid_mask(*a, F, Mx, lo, hi)))
    uc, ua, image = transfer_case(dims, (Cn, An))
    uc[row] = float("nan")
    ua[col] = float("nan")
    cases.append(("transfer", ops.transfer_head_grid(uc, ua, image).cpu().numpy(),
                  lambda lo, hi: ops.transfer_head_grid_mask(uc, ua, image, lo, hi)))
    for kind, g, run in cases:
        assert np.isnan(g[row]).all() and np.isnan(g[:, col]).all(), kind
        with np.errstate(invalid="ignore"):
            for lo, hi in bounds_of(g):
                b = data.PairMask(run(lo, hi), g.shape).to_bool()
                assert np.array_equal(b, (g >= lo) & (g <= hi)), (kind, lo, hi)
                assert not b[row].any() and not b[:, col].any(), (kind, lo, hi)
        everything = data.PairMask(run(-np.inf, np.inf), g.shape).to_bool()
        planes = g.shape[2] if g.ndim == 3 else 1
        assert np.array_equal(everything, ~np.isnan(g)) and everything.sum() == (Cn - 1) * (An - 1) * planes, kind


# ---------------------------------------------------------------- 2. the masked selection against the masked reference
def call_where(family, launch, Cn, An, nT, k, workgroups, count):
    """One _where entry on guarded outputs and a guarded workspace of exactly the queried size -> data.TopK of the
    meaningful slots, (rows, min(k, count)); every slot written, the rest NaN / -1 / -1."""
    lib = _lib.load()
    rows, m = max(nT, 1), min(k, count)
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
    assert (v[:, m:] == 0x7FC00000).all() and (ci[:, m:] == -1).all() and (ai[:, m:] == -1).all(), "slots past the mask's pairs"
    assert (ci[:, :m] >= 0).all() and (ci[:, :m] < Cn).all() and (ai[:, :m] >= 0).all() and (ai[:, :m] < An).all()
    return data.TopK(v[:, :m].view(np.float32), ci[:, :m].astype(np.int64), ai[:, :m].astype(np.int64))


def dev_mask(b):
    return data.PairMask.from_bool(b, device=DEV)


def head_where(kind, mc, ma, T, wp, dims, mask_b, k, largest, workgroups=0):
    D, F, Mx = dims
    Cn, An, nT = mc.shape[0], ma.shape[0], 0 if T is None else T.numel()
    words = dev_mask(mask_b).words
    launch = lambda lib, v, c, a, ws, nb: lib.impnn_head_grid_topk_where(
        ops.HEAD_KINDS[kind], _lib.ptr(mc), _lib.ptr(ma), _lib.ptr(T) if T is not None else None, _lib.ptr(wp), _lib.ptr(words),
        k, int(largest), v, c, a, ws, nb, Cn, An, nT, D, F, Mx, workgroups, _lib.stream_ptr())
    return call_where(0, launch, Cn, An, nT, k, workgroups, int(mask_b.sum()))


def transfer_where(uc, ua, image, mask_b, k, largest, workgroups=0):
    Cn, An = uc.shape[0], ua.shape[0]
    words = dev_mask(mask_b).words
    launch = lambda lib, v, c, a, ws, nb: lib.impnn_transfer_head_grid_topk_where(
        _lib.ptr(uc), _lib.ptr(ua), _lib.ptr(image), image.numel(), _lib.ptr(words), k, int(largest), v, c, a, ws, nb, Cn, An,
        workgroups, _lib.stream_ptr())
    return call_where(1, launch, Cn, An, 0, k, workgroups, int(mask_b.sum()))


def masks_of(shape, tile):
    """all ones, all zeros, density 0.5, the last pair alone and - where the grid has an interior tile of `tile` pairs -
    bits in that tile only (every other tile takes the skip path; the only live tile is not the first)."""
    Cn, An = shape
    rng = np.random.default_rng(Cn * 1000 + An)
    last = np.zeros(shape, bool)
    last[-1, -1] = True
    out = [("ones", np.ones(shape, bool)), ("zeros", np.zeros(shape, bool)), ("half", rng.random(shape) < 0.5), ("last", last)]
    tc, ta = tile
    if Cn > 2 * tc and An > 2 * ta:
        inner = np.zeros(shape, bool)
        inner[tc:2 * tc, ta:2 * ta] = rng.random((tc, ta)) < 0.5
        assert inner.any()
        out.append(("one interior tile", inner))
    return out


@pytest.mark.parametrize("dims", DIMS, ids=dims_id)
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=shape_id)
def test_head_topk_where_is_the_top_of_the_masked_grid(shape, dims):
    D, F, Mx = dims
    masks = masks_of(shape, (16, 64))
    assert (shape == (65, 130)) == (len(masks) == 5)
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, shape)
        T = torch.from_numpy(T_MAX[:3]).to(DEV) if kind == "viscosity" else None
        grid = ops.head_grid(kind, mc, ma, T, wp, F, Mx).cpu().numpy()
        for largest in (False, True):
            for k in (1, 5, 1024):
                for name, mb in masks:
                    got = head_where(kind, mc, ma, T, wp, dims, mb, k, largest)
                    same(got, data.grid_top_k(grid, k, largest, where=mb), f"{kind} {shape} {dims} {name} k={k} largest={largest}")
                    if name == "ones":     # the plain entry's result, bit for bit
                        v, ci, ai = (x.cpu().numpy() for x in ops.head_grid_topk(kind, mc, ma, T, wp, F, Mx, k, largest))
                        m = got.values.shape[1]
                        assert np.array_equal(bits(v[:, :m]), bits(got.values)) and np.array_equal(ci[:, :m], got.cation) \
                            and np.array_equal(ai[:, :m], got.anion) and (ci[:, m:] == -1).all()
    # the public wrapper takes a PairMask or its words
    kind, (name, mb) = "melting_point", masks[2]
    wp, mc, ma = head_case(kind, dims, shape)
    grid = ops.head_grid(kind, mc, ma, None, wp, F, Mx).cpu().numpy()
    want = data.grid_top_k(grid, 5, where=mb)
    for where in (dev_mask(mb), dev_mask(mb).words):
        v, ci, ai = (x.cpu().numpy() for x in ops.head_grid_topk(kind, mc, ma, None, wp, F, Mx, 5, where=where))
        m = len(want.values)
        same(data.TopK(v[:, :m], ci[:, :m], ai[:, :m]), want, "ops.head_grid_topk(where=)")
        assert (ci[:, m:] == -1).all() and np.isnan(v[:, m:]).all()


@pytest.mark.parametrize("shape", TRANSFER_SHAPES, ids=shape_id)
def test_transfer_topk_where_is_the_top_of_the_masked_grid(shape):
    masks = masks_of(shape, (8, 32))
    assert (shape == (20, 70)) == (len(masks) == 5)
    for dims in DIMS[:2]:
        uc, ua, image = transfer_case(dims, shape)
        grid = ops.transfer_head_grid(uc, ua, image).cpu().numpy()
        for largest in (False, True):
            for k in (1, 5, 1024):
                for name, mb in masks:
                    got = transfer_where(uc, ua, image, mb, k, largest)
                    same(got, data.grid_top_k(grid, k, largest, where=mb), f"transfer {shape} {dims} {name} k={k} largest={largest}")
                    if name == "ones":
                        v, ci, ai = (x.cpu().numpy() for x in ops.transfer_head_grid_topk(uc, ua, image, k, largest))
                        m = got.values.shape[1]
                        assert np.array_equal(bits(v[:, :m]), bits(got.values)) and np.array_equal(ci[:, :m], got.cation) \
                            and np.array_equal(ai[:, :m], got.anion)
    mb = masks[2][1]
    v, ci, ai = (x.cpu().numpy() for x in ops.transfer_head_grid_topk(uc, ua, image, 3, largest=True, where=dev_mask(mb)))
    want = data.grid_top_k(grid, 3, True, where=mb)
    m = len(want.values)
    same(data.TopK(v[:, :m], ci[:, :m], ai[:, :m]), want, "ops.transfer_head_grid_topk(where=)")


def test_the_masked_result_does_not_depend_on_the_workgroups():
    dims, shape = DIMS[0], (65, 130)    # 5 x 3 tiles of the head grid
    T = torch.from_numpy(T_MAX[:3]).to(DEV)
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, shape)
        Tk = T if kind == "viscosity" else None
        grid = ops.head_grid(kind, mc, ma, Tk, wp, dims[1], dims[2]).cpu().numpy()
        for name, mb in masks_of(shape, (16, 64))[2:]:
            for k, largest in ((5, False), (1024, True)):
                first = head_where(kind, mc, ma, Tk, wp, dims, mb, k, largest, workgroups=0)
                same(first, data.grid_top_k(grid, k, largest, where=mb), f"{kind} {name}")
                for g in (1, 3):
                    same(head_where(kind, mc, ma, Tk, wp, dims, mb, k, largest, workgroups=g), first, f"{kind} {name} workgroups={g}")
    uc, ua, image = transfer_case(DIMS[0], (20, 70))   # 3 x 3 tiles of the transfer grid
    for name, mb in masks_of((20, 70), (8, 32))[2:]:
        first = transfer_where(uc, ua, image, mb, 50, False)
        for g in (1, 3):
            same(transfer_where(uc, ua, image, mb, 50, False, workgroups=g), first, f"transfer {name} workgroups={g}")


def test_ties_across_a_masked_out_pair_go_by_index():
    dims, (Cn, An) = DIMS[0], (20, 70)
    D, F, Mx = dims
    T = torch.from_numpy(T_MAX[:2]).to(DEV)
    mb = np.ones((Cn, An), bool)
    mb[3] = False                    # one whole member of every tie of rows 0, 3, 17, 19 ...
    mb[17, ::2] = False              # ... half of another ...
    mb[:, 64] = False                # ... and one of the tied columns 2, 5, 64, 69
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, (Cn, An))
        mc[[3, 17, 19]] = mc[0].clone()
        ma[[5, 64, 69]] = ma[2].clone()
        Tk = T if kind == "viscosity" else None
        grid = ops.head_grid(kind, mc, ma, Tk, wp, F, Mx).cpu().numpy()
        assert np.array_equal(bits(grid[3]), bits(grid[0])) and np.array_equal(bits(grid[:, 64]), bits(grid[:, 2]))
        for largest in (False, True):
            for k in (100, 1024):
                same(head_where(kind, mc, ma, Tk, wp, dims, mb, k, largest), data.grid_top_k(grid, k, largest, where=mb),
                     f"{kind} ties k={k}")
    uc, ua, image = transfer_case(DIMS[0], (Cn, An))
    uc[[3, 19]] = uc[0].clone()
    ua[[33, 69]] = ua[1].clone()
    grid = ops.transfer_head_grid(uc, ua, image).cpu().numpy()
    mt = np.ones((Cn, An), bool)
    mt[3], mt[:, 33] = False, False
    for largest in (False, True):
        same(transfer_where(uc, ua, image, mt, 100, largest), data.grid_top_k(grid, 100, largest, where=mt), "transfer ties")


def test_a_masked_in_nan_pair_comes_last_in_both_directions():
    dims, (Cn, An), row = DIMS[0], (17, 70), 9
    D, F, Mx = dims
    T = torch.from_numpy(T_MAX[:2]).to(DEV)
    mb = np.zeros((Cn, An), bool)
    mb[row, [0, 40, 69]] = True          # three NaN pairs
    mb[[0, 5, 16], [1, 66, 69]] = True   # and three finite ones
    cases = []
    for kind in KINDS:
        wp, mc, ma = head_case(kind, dims, (Cn, An))
        mc[row] = float("nan")
        Tk = T if kind == "viscosity" else None
        grid = ops.head_grid(kind, mc, ma, Tk, wp, F, Mx).cpu().numpy()
        cases.append((kind, grid, lambda k, largest, a=(kind, mc, ma, Tk, wp): head_where(*a, dims, mb, k, largest)))
    uc, ua, image = transfer_case(dims, (Cn, An))
    uc[row] = float("nan")
    cases.append(("transfer", ops.transfer_head_grid(uc, ua, image).cpu().numpy(),
                  lambda k, largest: transfer_where(uc, ua, image, mb, k, largest)))
    for kind, grid, run in cases:
        assert np.isnan(grid[row]).all()
        for largest in (False, True):
            got = run(3, largest)
            assert np.isfinite(got.values).all() and not (got.cation == row).any(), (kind, largest)
            same(got, data.grid_top_k(grid, 3, largest, where=mb), f"{kind} k=3")
            got = run(10, largest)                                     # k above the six pairs: the NaN pairs are the tail
            same(got, data.grid_top_k(grid, 10, largest, where=mb), f"{kind} k=10")
            assert got.values.shape[1] == 6 and (bits(got.values[:, 3:]) == 0x7FC00000).all()
            assert (got.cation[:, 3:] == row).all() and (got.anion[:, 3:] == [0, 40, 69]).all()


# ---------------------------------------------------------------- 3. model level
T2 = T5[[1, 3]]


@pytest.fixture(scope="module")
def small_species():
    cat, _ = species(12, 70)
    _, an = species(9, 71)
    return cat, an


def check_screen_mask(m, cat, an, T, **kw):
    """screen_mask against the comparison on predict_grid, for a split at the median and a band around it."""
    tk = {"temperatures": T} if T is not None else {}
    grid = m.predict_grid(cat, an, **tk)
    q = np.quantile(grid, [0.25, 0.5, 0.75]).astype(np.float32)
    for at_least, at_most in ((None, q[1]), (q[1], None), (q[0], q[2]), (float(grid.flat[3]), float(grid.flat[3]))):
        got = m.screen_mask(cat, an, at_least=at_least, at_most=at_most, **tk, **kw)
        lo = np.float32(-np.inf if at_least is None else at_least)
        hi = np.float32(np.inf if at_most is None else at_most)
        want = (grid >= lo) & (grid <= hi)
        assert isinstance(got, data.PairMask) and got.shape == grid.shape and got.words.is_cuda
        assert np.array_equal(got.words.cpu().numpy().view(np.uint32), words_of(want)), (at_least, at_most, kw)
        assert want.any() and not want.all()
    return grid


def check_where(m, cat, an, T, where_b, ks, **kw):
    tk = {"temperatures": T} if T is not None else {}
    grid = m.predict_grid(cat, an, **tk)
    for where in (dev_mask(where_b), data.PairMask.from_bool(where_b)):     # on the device, and (one k) on the host
        for k in ks if where.words.is_cuda else ks[:1]:
            for largest in (False, True):
                got = m.screen_top_k(cat, an, k=k, largest=largest, where=where, **tk, **kw)
                want = data.grid_top_k(grid, k, largest, where=where_b)
                assert got.values.shape == want.values.shape
                assert got.values.shape[-1] == min(k, int(where_b.sum()))
                assert np.array_equal(bits(got.values), bits(want.values)), (k, largest, kw)
                assert np.array_equal(got.cation, want.cation) and np.array_equal(got.anion, want.anion), (k, largest, kw)


def test_model_screen_mask_viscosity_and_melting_point(small_species):
    cat, an = small_species
    v, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=2)
    assert v._grid_kernels_cover()
    check_screen_mask(v, cat, an, T2)
    check_screen_mask(v, cat, an, T2, max_pairs_per_launch=4 * 9)           # three host tiles of the cation axis
    mp, _ = make_model("melting_point", atom_dim=16, num_steps=2)
    check_screen_mask(mp, cat, an, None)
    check_screen_mask(mp, cat, an, None, max_pairs_per_launch=9)
    empty = {k: x[:0] for k, x in cat.items()}
    got = v.screen_mask(empty, an, temperatures=T2, at_most=0.0)
    assert got.shape == (0, 9, 2) and tuple(got.words.shape) == (2, 0, 1)


def test_model_screen_mask_transfer_modes_and_an_uncovered_width(small_species, tmp_path):
    from test_gpu_transfer import make_transfer
    cat, an = small_species
    t = make_transfer(tmp_path, S=2)
    assert t._transfer_grid_covers() and t.grid_head_mode == "auto"
    check_screen_mask(t, cat, an, None)
    check_screen_mask(t, cat, an, None, max_pairs_per_launch=3 * 9)
    t.grid_head_mode = "gathered"
    try:
        check_screen_mask(t, cat, an, None)
        check_screen_mask(t, cat, an, None, max_pairs_per_launch=2 * 9)
    finally:
        t.grid_head_mode = "auto"
    wide, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=1, fp_size=32, mixing_size=72, seed=6)
    assert not wide._grid_kernels_cover()
    check_screen_mask(wide, cat, an, T2)
    check_screen_mask(wide, cat, an, T2, max_pairs_per_launch=2 * 9)


def test_model_screen_top_k_where(small_species, tmp_path):
    from test_gpu_transfer import make_transfer
    cat, an = small_species
    rng = np.random.default_rng(8)
    half = rng.random((12, 9)) < 0.5
    few = np.zeros((12, 9), bool)
    few[[1, 7, 11], [0, 4, 8]] = True
    v, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=2)
    for wb in (half, few, np.zeros((12, 9), bool)):
        check_where(v, cat, an, T2, wb, (1, 10, 200))
    check_where(v, cat, an, T5, half, (7,))                                 # five temperatures: two selecting launches
    for pairs in (4 * 9, 9):                                                # 3 and C host tiles of the cation axis
        check_where(v, cat, an, T2, half, (10, 100), max_pairs_per_launch=pairs)
    assert 1500 > MM.SCREEN_MAX_K
    check_where(v, cat, an, T2, half, (1500,))                              # k above the kernels' limit: the fallback
    check_where(v, cat, an, T2, half, (1500,), max_pairs_per_launch=5 * 9)
    t = make_transfer(tmp_path, S=2)
    check_where(t, cat, an, None, half, (10, 200))
    check_where(t, cat, an, None, half, (10,), max_pairs_per_launch=3 * 9)
    t.grid_head_mode = "gathered"
    try:
        check_where(t, cat, an, None, half, (10,), max_pairs_per_launch=2 * 9)
    finally:
        t.grid_head_mode = "auto"
    wide, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=1, fp_size=32, mixing_size=72, seed=6)
    check_where(wide, cat, an, T2, half, (10,), max_pairs_per_launch=2 * 9)


def test_two_models_compose(small_species):
    """The intended use: of the pairs the melting-point model puts below a limit and nobody has made yet, the k least
    viscous at one temperature - against the same question asked of the two materialised grids."""
    cat, an = small_species
    mp, _ = make_model("melting_point", atom_dim=16, num_steps=2)
    v, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=2)
    g_mp, g_v = mp.predict_grid(cat, an), v.predict_grid(cat, an, temperatures=[298.15])
    limit = np.float32(np.quantile(g_mp, 0.6))
    already_made = np.random.default_rng(4).random((12, 9)) < 0.3
    liquid = mp.screen_mask(cat, an, at_most=limit)
    known = data.PairMask.from_bool(already_made, device=liquid.words.device)
    where_b = (g_mp <= limit) & ~already_made
    assert np.array_equal((liquid & ~known).to_bool(), where_b) and 0 < where_b.sum() < where_b.size
    for k in (5, 100):
        best = v.screen_top_k(cat, an, [298.15], k=k, where=liquid & ~known)
        want = data.grid_top_k(g_v, k, where=where_b)
        assert best.values.shape == (1, min(k, int(where_b.sum())))
        assert np.array_equal(bits(best.values), bits(want.values))
        assert np.array_equal(best.cation, want.cation) and np.array_equal(best.anion, want.anion)
        assert where_b[best.cation[0], best.anion[0]].all()
