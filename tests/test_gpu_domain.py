"""GPU: the applicability domain (include/impnn.h, impnn_domain_grid / _grid_mask / _rows; csrc/grid_domain.hip) - the
distance from a pair's latent vector mix_cat[i] + mix_an[j] to the nearest row of a reference set.

1. against float64 (data.grid_domain): 1e-5 relative, exact zeros, the index, the lower of identical rows;
2. guarded outputs, nearest = null;  3. the mask is the comparison on the materialised distance, exactly;
4. the rows form has the grid form's bits; exclude_self;  5. a NaN row and column stay where they are;
6. the model: fit_domain, domain_grid, screen_domain_mask, screen_top_k(where=), domain_distance, the refusals.

The shapes cross every edge of the kernels: partial tiles on both axes and a second mask word per row, both register
templates (Mx <= 32, Mx = 64) and an Mx that is no multiple of 4, and R = 1, one more than the kernels' reference chunk,
and three chunks plus a remainder.  Half of a reference set's rows are sums of the grid's own mixing rows (exact zeros
occur), half come from other pooled rows."""
import functools

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, data, ops
from ionic_mpnn_amd.ensemble import ModelEnsemble

from test_gpu_grid import DIMS, bits, make_model, pooled_rows, species
from test_gpu_screen import Guarded, head_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("viscosity", "melting_point")
SHAPES = [(1, 1), (7, 63), (17, 130), (65, 130)]
RTOL = 1e-5  # the project's bound


def reference_sizes():
    chunk = ops.domain_reference_chunk()
    return (1, chunk + 1, 3 * chunk + 7)


def reference_rows(kind, dims, wp, mc, ma, R, seed):
    """(R,Mx) on the device: ceil(R / 2) sums of the grid's own mixing rows, the rest from other pooled rows, shuffled."""
    D, F, Mx = dims
    rng = np.random.default_rng(seed)
    own = (R + 1) // 2
    ci = torch.from_numpy(rng.integers(0, mc.shape[0], own)).to(DEV)
    ai = torch.from_numpy(rng.integers(0, ma.shape[0], own)).to(DEV)
    parts = [mc[ci] + ma[ai]]
    if R > own:
        pc = torch.from_numpy(pooled_rows(R - own, D, seed + 100)).to(DEV)
        pa = torch.from_numpy(pooled_rows(R - own, D, seed + 200)).to(DEV)
        parts.append(ops.head_ion_mix(kind, "cat", pc, wp, F, Mx) + ops.head_ion_mix(kind, "an", pa, wp, F, Mx))
    order = torch.from_numpy(rng.permutation(R)).to(DEV)
    return torch.cat(parts)[order].contiguous()


@functools.lru_cache(maxsize=None)
def case(kind, dims, shape, R):
    """One grid and reference set, the kernel's answer and the float64 reference, computed once and left unchanged."""
    wp, mc, ma = head_case(kind, dims, shape)
    ref = reference_rows(kind, dims, wp, mc, ma, R, seed=7 + R)
    d, n = ops.domain_grid(mc, ma, ref)
    want_d, _ = data.grid_domain(mc.cpu().numpy(), ma.cpu().numpy(), ref.cpu().numpy())
    return {"mc": mc, "ma": ma, "ref": ref, "d": d.cpu().numpy(), "n": n.cpu().numpy(), "want_d": want_d}


def exact_distance(mc, ma, ref, nearest):
    """float64 distance from z (the float32 sum) to the reference row ``nearest`` names, (C,A)."""
    z = (mc.cpu().numpy()[:, None, :] + ma.cpu().numpy()[None, :, :]).astype(np.float64)
    diff = z - ref.cpu().numpy().astype(np.float64)[nearest]
    return np.sqrt((diff * diff).sum(axis=2))


# ---------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "D%d-F%d-Mx%d" % d)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_grid_against_fp64(shape, dims):
    zeros = 0
    for kind in KINDS:
        for R in reference_sizes():
            c = case(kind, dims, shape, R)
            d, n, want = c["d"], c["n"], c["want_d"]
            what = f"{kind} {shape} {dims} R={R}"
            assert d.shape == n.shape == shape and d.dtype == np.float32 and n.dtype == np.int32
            assert np.isfinite(d).all() and (n >= 0).all() and (n < R).all(), what
            err = np.abs(d.astype(np.float64) - want)
            print(what, "max relative error", float((err[want > 0] / want[want > 0]).max()) if (want > 0).any() else 0.0)
            assert (err <= RTOL * want).all(), what
            assert (d[want == 0] == 0).all(), f"{what}: an exact hit must be exactly 0"
            zeros += int((want == 0).sum())
            # the index, on every pair: the row it names is as near as the distance says
            at = exact_distance(c["mc"], c["ma"], c["ref"], n)
            assert (np.abs(at - d.astype(np.float64)) <= RTOL * at).all(), f"{what}: nearest"
    assert zeros > 0, "the reference sets hold pairs of the grid"


@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "D%d-F%d-Mx%d" % d)
def test_the_lower_of_identical_rows_is_nearest(dims):
    shape, R = (17, 130), reference_sizes()[1]
    c = case("viscosity", dims, shape, R)
    # every row twice, next to each other: the copy shares its original's chunk (but for the one that straddles two)
    d2, n2 = ops.domain_grid(c["mc"], c["ma"], c["ref"].repeat_interleave(2, dim=0))
    assert np.array_equal(bits(d2.cpu().numpy()), bits(c["d"])) and np.array_equal(n2.cpu().numpy(), 2 * c["n"])
    # the whole set twice: the copy is a chunk and more away
    d2, n2 = ops.domain_grid(c["mc"], c["ma"], torch.cat([c["ref"], c["ref"]]))
    assert np.array_equal(bits(d2.cpu().numpy()), bits(c["d"])) and np.array_equal(n2.cpu().numpy(), c["n"])


# ---------------------------------------------------------------- 2. guarded outputs
@pytest.mark.parametrize("dims", DIMS[:2], ids=lambda d: "D%d-F%d-Mx%d" % d)
@pytest.mark.parametrize("shape", [(7, 63), (65, 130)], ids=lambda s: "%dx%d" % s)
def test_nothing_is_written_outside_the_outputs(shape, dims):
    lib = _lib.load()
    (Cn, An), Mx, R = shape, dims[2], reference_sizes()[1]
    c = case("melting_point", dims, shape, R)
    mc, ma, ref = c["mc"], c["ma"], c["ref"]
    W = data.mask_row_words(An)
    filled = np.uint32(0xA5A5A5A5)  # no distance (>= 0 or the quiet NaN) and no index has these bits
    dist, near, alone, words = Guarded(Cn * An * 4), Guarded(Cn * An * 4), Guarded(Cn * An * 4), Guarded(Cn * W * 4)
    args = (Cn, An, R, Mx, _lib.stream_ptr())
    _lib.check(lib.impnn_domain_grid(_lib.ptr(mc), _lib.ptr(ma), _lib.ptr(ref), dist.ptr, near.ptr, *args))
    _lib.check(lib.impnn_domain_grid(_lib.ptr(mc), _lib.ptr(ma), _lib.ptr(ref), alone.ptr, None, *args))
    med = float(np.median(c["d"]))
    _lib.check(lib.impnn_domain_grid_mask(_lib.ptr(mc), _lib.ptr(ma), _lib.ptr(ref), 0.0, med, words.ptr, *args))
    torch.cuda.synchronize()
    d = dist.body(np.uint32, "distance")
    n = near.body(np.int32, "nearest")
    assert not (d == filled).any() and not (n.view(np.uint32) == filled).any(), "an element was not written"
    assert np.array_equal(d.reshape(Cn, An), bits(c["d"])) and np.array_equal(n.reshape(Cn, An), c["n"])
    assert np.array_equal(alone.body(np.uint32, "distance (nearest = null)"), d), "nearest = null changes the distance"
    w = words.body(np.int32, "the mask words").reshape(Cn, W)
    assert np.array_equal(w, data.PairMask.from_bool(c["d"] <= np.float32(med)).words.numpy())
    # the rows form
    z = (mc[:, None, :] + ma[None, :, :]).reshape(-1, Mx).contiguous()
    Q = Cn * An
    rd, rn = Guarded(Q * 4), Guarded(Q * 4)
    _lib.check(lib.impnn_domain_rows(_lib.ptr(z), _lib.ptr(ref), 0, rd.ptr, rn.ptr, Q, R, Mx, _lib.stream_ptr()))
    ra = Guarded(Q * 4)
    _lib.check(lib.impnn_domain_rows(_lib.ptr(z), _lib.ptr(ref), 0, ra.ptr, None, Q, R, Mx, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(rd.body(np.uint32, "rows distance"), d) and np.array_equal(rn.body(np.int32, "rows nearest"), n)
    assert np.array_equal(ra.body(np.uint32, "rows distance (nearest = null)"), d)


# ---------------------------------------------------------------- 3. the mask
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "D%d-F%d-Mx%d" % d)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_mask_is_the_comparison_on_the_materialised_distance(shape, dims):
    inf = np.float32(np.inf)
    for kind in KINDS:
        for R in reference_sizes():
            c = case(kind, dims, shape, R)
            d = c["d"]
            med, one = np.float32(np.median(d)), d.reshape(-1)[d.size // 3]
            for lo, hi in ((-inf, inf), (inf, inf), (one, one), (-inf, med), (med, inf)):
                words = ops.domain_grid_mask(c["mc"], c["ma"], c["ref"], lo, hi)
                assert words.dtype == torch.int32 and tuple(words.shape) == (shape[0], data.mask_row_words(shape[1]))
                want = data.PairMask.from_bool((d >= lo) & (d <= hi))
                assert np.array_equal(words.cpu().numpy(), want.words.numpy()), (kind, shape, dims, R, lo, hi)
                got = data.PairMask(words, shape)
                assert got.count() == int(((d >= lo) & (d <= hi)).sum())
                if (lo, hi) == (-inf, inf):  # every pair, and not one pad bit
                    assert got.count() == shape[0] * shape[1] and (~got).count() == 0
                    pad = np.unpackbits(words.cpu().numpy().view(np.uint8).reshape(shape[0], -1), axis=1, bitorder="little")
                    assert not pad[:, shape[1]:].any(), "pad bits must be 0"
                if (lo, hi) == (one, one):
                    assert got.count() >= 1


# ---------------------------------------------------------------- 4. the rows form
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "D%d-F%d-Mx%d" % d)
def test_rows_form_has_the_grid_forms_bits(dims):
    for kind, shape in (("viscosity", (17, 130)), ("melting_point", (7, 63))):
        for R in reference_sizes():
            c = case(kind, dims, shape, R)
            z = (c["mc"][:, None, :] + c["ma"][None, :, :]).reshape(-1, dims[2])  # gathered with torch: the float32 sum
            d, n = ops.domain_rows(z, c["ref"])
            assert d.shape == n.shape == (shape[0] * shape[1],) and n.dtype == torch.int32
            assert np.array_equal(bits(d.cpu().numpy()), bits(c["d"].reshape(-1))), (kind, dims, R)
            assert np.array_equal(n.cpu().numpy(), c["n"].reshape(-1)), (kind, dims, R)


@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "D%d-F%d-Mx%d" % d)
def test_exclude_self(dims):
    for R in reference_sizes():
        c = case("viscosity", dims, (17, 130), R)
        planted = R > 1
        ref = torch.cat([c["ref"], c["ref"][:1]]) if planted else c["ref"]   # the last row is row 0 again
        n_ref = int(ref.shape[0])
        d, n = (x.cpu().numpy() for x in ops.domain_rows(ref, ref, exclude_self=True))
        if n_ref == 1:
            assert np.isnan(d).all() and (n == -1).all(), "a set of one row has no other row"
            continue
        assert (n != np.arange(n_ref)).all() and (n >= 0).all() and (n < n_ref).all()
        assert d[0] == 0 and n[0] != 0 and torch.equal(ref[int(n[0])], ref[0]), "row 0 finds a copy of itself"
        assert d[-1] == 0 and n[-1] == 0, "the planted copy finds row 0, the first of its kind"
        r64 = ref.cpu().numpy().astype(np.float64)
        diff = r64[:, None, :] - r64[None, :, :]
        d2 = (diff * diff).sum(axis=2)
        np.fill_diagonal(d2, np.inf)                                          # row p removed for query p
        want = np.sqrt(d2.min(axis=1))
        assert (np.abs(d.astype(np.float64) - want) <= RTOL * want).all(), (dims, R)
        assert (d[want == 0] == 0).all() and ((d > 0) | (want == 0)).all(), "a zero comes from identical rows only"
        at = np.sqrt(d2[np.arange(n_ref), n])
        assert (np.abs(at - d.astype(np.float64)) <= RTOL * at).all(), "nearest"
        # without the exclusion every row finds itself, or an identical row before it
        d0, n0 = (x.cpu().numpy() for x in ops.domain_rows(ref, ref))
        assert (d0 == 0).all() and (n0 <= np.arange(n_ref)).all() and n0[-1] == 0


# ---------------------------------------------------------------- 5. NaN
@pytest.mark.parametrize("dims", DIMS[:2], ids=lambda d: "D%d-F%d-Mx%d" % d)
def test_a_nan_row_and_column_stay_where_they_are(dims):
    shape, R = (17, 130), reference_sizes()[2]
    c = case("melting_point", dims, shape, R)
    mc, ma = c["mc"].clone(), c["ma"].clone()
    mc[5, dims[2] - 1] = float("nan")     # one element is enough
    ma[70] = float("nan")
    d, n = (x.cpu().numpy() for x in ops.domain_grid(mc, ma, c["ref"]))
    bad = np.zeros(shape, np.bool_)
    bad[5, :] = bad[:, 70] = True
    assert np.isnan(d[bad]).all() and (n[bad] == -1).all()
    assert np.array_equal(bits(d[~bad]), bits(c["d"][~bad])) and np.array_equal(n[~bad], c["n"][~bad])
    every = data.PairMask(ops.domain_grid_mask(mc, ma, c["ref"], -np.inf, np.inf), shape).to_bool()
    assert np.array_equal(every, ~bad), "a NaN distance passes no bound"
    z = (mc[:, None, :] + ma[None, :, :]).reshape(-1, dims[2])
    rd, rn = (x.cpu().numpy() for x in ops.domain_rows(z, c["ref"]))
    assert np.array_equal(bits(rd), bits(d.reshape(-1))) and np.array_equal(rn, n.reshape(-1))


# ---------------------------------------------------------------- 6. the model
def records_of(cat, an, ci, ai):
    out = {f"cat_{k}": v[ci] for k, v in cat.items()}
    out.update({f"an_{k}": v[ai] for k, v in an.items()})
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_model_domain(kind):
    kw = dict(atom_dim=32, bond_dim=8, num_steps=2) if kind == "viscosity" else dict(atom_dim=32, num_steps=2)
    m, _ = make_model(kind, seed=3, **kw)
    cat, _ = species(19, 70)
    _, an = species(70, 71)
    rng = np.random.default_rng(9)
    ci, ai = rng.integers(0, 19, 30), rng.integers(0, 70, 30)
    ci, ai = np.concatenate([ci, ci[:10]]), np.concatenate([ai, ai[:10]])   # 40 listed pairs, 10 of them repeats
    distinct = sorted(set(zip(ci.tolist(), ai.tolist())))
    dom = m.fit_domain(cat, an, ci, ai)
    R = len(distinct)
    assert len(dom) == R < 40 and dom.width == m.mixing_size and dom.rows.is_cuda
    assert list(zip(dom.cation.tolist(), dom.anion.tolist())) == distinct
    assert dom.self_distance.shape == (R,) and np.isfinite(dom.self_distance).all()
    radius = dom.radius(0.95)
    assert np.isfinite(radius) and radius >= 0

    d, n = m.domain_grid(cat, an, dom)
    assert d.shape == n.shape == (19, 70) and d.dtype == np.float32 and n.dtype == np.int32
    assert (d[dom.cation, dom.anion] == 0).all(), "a training pair lies at distance 0"
    hit = n[dom.cation, dom.anion]
    assert (hit <= np.arange(R)).all() and torch.equal(dom.rows[torch.from_numpy(hit.astype(np.int64)).to(DEV)], dom.rows), \
        "nearest names the pair itself (or an identical row before it)"
    d1, n1 = m.domain_grid(cat, an, dom, max_pairs_per_launch=64)           # below one row of anions: a row at a time
    assert np.array_equal(bits(d1), bits(d)) and np.array_equal(n1, n)

    inside = m.screen_domain_mask(cat, an, dom, at_most=radius)
    assert isinstance(inside, data.PairMask) and inside.shape == (19, 70) and inside.words.is_cuda
    assert np.array_equal(inside.to_bool(), d <= radius)
    assert inside.to_bool()[dom.cation, dom.anion].all()
    tiled = m.screen_domain_mask(cat, an, dom, at_most=radius, max_pairs_per_launch=5 * 70)
    assert torch.equal(tiled.words, inside.words)
    ring = m.screen_domain_mask(cat, an, dom, at_least=radius, at_most=2 * radius)
    assert np.array_equal(ring.to_bool(), (d >= radius) & (d <= np.float32(2 * radius)))
    with pytest.raises(ValueError, match="needs a bound"):
        m.screen_domain_mask(cat, an, dom)
    with pytest.raises(ValueError, match="NaN"):
        m.screen_domain_mask(cat, an, dom, at_most=float("nan"))

    # the composition the feature exists for
    T = {"temperatures": [298.15]} if kind == "viscosity" else {}
    k = 50
    top = m.screen_top_k(cat, an, k=k, where=inside, **T)
    assert top.cation.shape[-1] == min(k, inside.count()) >= 1
    assert inside.to_bool()[top.cation.reshape(-1), top.anion.reshape(-1)].all(), "screen_top_k left the mask"

    # listed pairs as records
    got_d, got_n = m.domain_distance(records_of(cat, an, ci, ai), dom)
    assert got_d.shape == got_n.shape == (40,) and got_d.dtype == np.float32 and got_n.dtype == np.int32
    assert (got_d == 0).all(), "records of training pairs lie at distance 0"
    oc, oa = rng.integers(0, 19, 25), rng.integers(0, 70, 25)
    got_d, got_n = m.domain_distance(records_of(cat, an, oc, oa), dom, batch_size=16)
    assert np.array_equal(bits(got_d), bits(d[oc, oa])) and np.array_equal(got_n, n[oc, oa])

    # a reference set of another width
    other = data.DomainReference(torch.zeros(3, m.mixing_size + 1, device=DEV), [0, 1, 2], [0, 1, 2], [0, 0, 0])
    for call in (lambda: m.domain_grid(cat, an, other), lambda: m.screen_domain_mask(cat, an, other, at_most=1.0),
                 lambda: m.domain_distance(records_of(cat, an, oc, oa), other)):
        with pytest.raises(ValueError, match="width"):
            call()
    # an ensemble has no one latent space
    ens = ModelEnsemble([m])
    for call in (lambda: ens.fit_domain(cat, an, ci, ai), lambda: ens.domain_grid(cat, an, dom),
                 lambda: ens.screen_domain_mask(cat, an, dom, at_most=radius),
                 lambda: ens.domain_distance(records_of(cat, an, oc, oa), dom)):
        with pytest.raises(ValueError, match="member model"):
            call()


def test_models_without_the_latent_space_are_refused(tmp_path):
    from test_gpu_transfer import make_transfer
    cat, _ = species(5, 80)
    _, an = species(6, 81)
    ci, ai = np.array([0, 1, 2]), np.array([3, 4, 5])
    dom = data.DomainReference(torch.zeros(3, 20, device=DEV), ci, ai, [1.0, 1.0, 1.0])
    t = make_transfer(tmp_path, S=2)
    for call in (lambda: t.fit_domain(cat, an, ci, ai), lambda: t.domain_grid(cat, an, dom),
                 lambda: t.screen_domain_mask(cat, an, dom, at_most=1.0),
                 lambda: t.domain_distance(records_of(cat, an, ci, ai), dom)):
        with pytest.raises(ValueError, match="base viscosity model"):
            call()
    wide, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=1, fp_size=96, mixing_size=20, seed=6)
    assert not wide._grid_kernels_cover()
    for call in (lambda: wide.fit_domain(cat, an, ci, ai), lambda: wide.domain_grid(cat, an, dom)):
        with pytest.raises(ValueError, match="do not cover"):
            call()
