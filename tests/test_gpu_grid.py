"""Cation x anion screening on the GPU: impnn_head_ion_mix + impnn_head_grid bit for bit against impnn_model_head on
the gathered pairs (every tile edge, store alignment and width path; sentinels and guard regions around the outputs),
the VFT parameters against fp64, non-finite isolation, and MPNNModel.encode_ions / predict_grid against the fp64 oracle
and against predict on the explicitly expanded pair list.

Tolerances: bitwise where two kernels evaluate the same fmaf chains; conftest's assert_close at 1e-5 against fp64 (the
bound every forward value of this project meets); 1e-6 for `out` against its own fp32 parameters recomputed in fp64
(three fp32 roundings of the last expression, 2^-24 each, against the tensor scale)."""
import ctypes as C

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, data, model as MM, ops, synthetic, weights
from conftest import assert_close
from oracle import mpnn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("viscosity", "melting_point")
SENTINEL = np.float32(-1.2345e30)
GUARD = 64
TILE_C = 16  # the grid kernel's tile is 16 cations x 64 anions (csrc/head_grid.hip)
SHAPES = [(1, 1), (7, 63), (64, 64), (65, 130), (130, 1), (TILE_C - 1, 5), (TILE_C, 2), (TILE_C + 1, 66)]
DIMS = [(32, 32, 20), (128, 64, 64), (8, 8, 5)]


# ---------------------------------------------------------------- head-only fixtures (no encoder)
def head_weights(kind, D, F, Mx, seed):
    """Random head weights by name, wide enough that the viscosity parameters leave every clip."""
    rng = np.random.default_rng(seed)
    u = lambda *shape: rng.uniform(-0.4, 0.4, size=shape).astype(np.float32)
    w = {}
    for p in ("cat", "an"):
        w[f"{p}_fp/kernel"], w[f"{p}_fp/bias"] = u(D, F), u(F)
    for p in ("cat", "an"):
        w[f"{p}_proj/kernel"], w[f"{p}_proj/bias"] = u(F, Mx), u(Mx)
    if kind == "viscosity":
        # mixed is a sum of relus (>= 0): alternating signs let vp[1] and vp[2] go far to either side
        sign = np.where((np.arange(Mx)[:, None] + np.arange(3)[None, :]) % 2 == 0, 1.0, -1.0).astype(np.float32)
        w["visc_params/kernel"], w["visc_params/bias"] = np.abs(u(Mx, 3)) * sign, u(3)
    else:
        w["mp_hidden/kernel"], w["mp_hidden/bias"] = u(Mx, F), u(F)
        w["mp_out/kernel"], w["mp_out/bias"] = u(F, 1), u(1)
    return w


def pack(kind, w):
    names = ["cat_fp", "an_fp", "cat_proj", "an_proj"] + (["visc_params"] if kind == "viscosity" else ["mp_hidden", "mp_out"])
    return np.concatenate([w[f"{n}/{part}"].reshape(-1) for n in names for part in ("kernel", "bias")])


WIDE = (0.02, 0.3, 1.0, 4.0, 25.0, 150.0, 600.0)


def pooled_rows(n, D, seed, scales=WIDE):
    """Rows whose scale cycles over four decades: vp[1] and vp[2] then lie on both sides of the softplus branch at
    20 and beyond both clips (checked by branch_coverage on the fp64 values)."""
    rng = np.random.default_rng(seed)
    scale = np.array(scales, np.float32)[np.arange(n) % len(scales)]
    return (rng.normal(0.0, 1.0, size=(n, D)).astype(np.float32) * scale[:, None] / np.float32(np.sqrt(D / 8.0)))


def ref_mix(w, p, pooled):
    fp = O.dense(pooled.astype(np.float64), w[f"{p}_fp/kernel"].astype(np.float64), w[f"{p}_fp/bias"].astype(np.float64), "relu")
    return O.dense(fp, w[f"{p}_proj/kernel"].astype(np.float64), w[f"{p}_proj/bias"].astype(np.float64), "relu")


def ref_grid(kind, w, pc, pa, T=None):
    """fp64 head over the product, with the oracle's own pieces -> out (C,A[,nT]), and for viscosity vp (C,A,3) and
    the clipped parameters (C,A,3)."""
    d = lambda a: np.asarray(a, np.float64)
    mixed = ref_mix(w, "cat", pc)[:, None, :] + ref_mix(w, "an", pa)[None, :, :]
    if kind == "viscosity":
        vp = O.dense(mixed, d(w["visc_params/kernel"]), d(w["visc_params/bias"]))
        A = vp[..., 0]
        B = np.clip(O._softplus(vp[..., 1]), 0.0, 20.0)
        Cc = np.clip(O._softplus(vp[..., 2]), 0.1, 50.0)
        out = A[..., None] + B[..., None] / (d(T)[None, None, :] / 100.0 + Cc[..., None] + 1e-6)
        return out, vp, np.stack([A, B, Cc], axis=-1)
    hid = O.dense(mixed, d(w["mp_hidden/kernel"]), d(w["mp_hidden/bias"]), "relu")
    return O.dense(hid, d(w["mp_out/kernel"]), d(w["mp_out/bias"]))[..., 0], None, None


def branch_coverage(vp):
    sp1, sp2 = O._softplus(vp[..., 1]), O._softplus(vp[..., 2])
    return {"softplus x > 20": bool((vp[..., 1:] > 20).any()), "softplus x <= 20": bool((vp[..., 1:] <= 20).any()),
            "B clipped at 20": bool((sp1 > 20).any()), "B inside": bool((sp1 < 20).any()),
            "C clipped at 0.1": bool((sp2 < 0.1).any()), "C clipped at 50": bool((sp2 > 50).any()),
            "C inside": bool(((sp2 > 0.1) & (sp2 < 50)).any())}


def guarded(n, offset):
    """A sentinel-filled buffer of n floats whose start is `offset` floats past a 16-byte boundary, with GUARD
    sentinel floats before and after -> (whole tensor, data pointer of the n floats)."""
    whole = torch.full((GUARD + offset + n + GUARD,), float(SENTINEL), dtype=torch.float32, device=DEV)
    assert whole.data_ptr() % 16 == 0
    return whole, C.c_void_p(whole.data_ptr() + 4 * (GUARD + offset))


def split_guarded(whole, n, offset):
    host = whole.cpu().numpy()
    lo = GUARD + offset
    assert np.array_equal(host[:lo].view(np.uint32), np.full(lo, SENTINEL).view(np.uint32)), "write before the output"
    assert np.array_equal(host[lo + n:].view(np.uint32), np.full(GUARD, SENTINEL).view(np.uint32)), "write past the output"
    body = host[lo:lo + n]
    assert not (body.view(np.uint32) == SENTINEL.view(np.uint32)).any(), "an output element was not written"
    return body


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def gathered_head(kind, pc, pa, T, wp, F, Mx):
    """ops.model_head on the explicit pairs (pc[i], pa[j], T[t]) -> (C,A[,nT])."""
    Cn, An, D = pc.shape[0], pa.shape[0], pc.shape[1]
    nT = 1 if T is None else T.numel()
    pcg = pc[:, None, None, :].expand(Cn, An, nT, D).reshape(-1, D).contiguous()
    pag = pa[None, :, None, :].expand(Cn, An, nT, D).reshape(-1, D).contiguous()
    Tg = None if T is None else T[None, None, :].expand(Cn, An, nT).reshape(-1, 1).contiguous()
    out = ops.model_head(kind, pcg, pag, Tg, wp, F, Mx)
    return out.reshape(Cn, An, nT) if T is not None else out.reshape(Cn, An)


@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "D%d-F%d-Mx%d" % d)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_grid_is_bitwise_the_head_kernel(shape, dims):
    """1. head_grid(head_ion_mix(pc), head_ion_mix(pa), T) against impnn_model_head on the gathered rows: the raw
    float bits, both kinds, nT in {1, 3, 8}, outputs at every 16-byte phase, every element written, none outside."""
    (Cn, An), (D, F, Mx) = shape, dims
    lib = _lib.load()
    pc_h, pa_h = pooled_rows(Cn, D, 11 + Cn), pooled_rows(An, D, 23 + An)
    pc, pa = torch.from_numpy(pc_h).to(DEV), torch.from_numpy(pa_h).to(DEV)
    for kind in KINDS:
        k = ops.HEAD_KINDS[kind]
        w = head_weights(kind, D, F, Mx, seed=5)
        wp = torch.from_numpy(pack(kind, w)).to(DEV)
        mc = ops.head_ion_mix(kind, "cat", pc, wp, F, Mx)
        ma = ops.head_ion_mix(kind, "an", pa, wp, F, Mx)
        assert mc.shape == (Cn, Mx) and ma.shape == (An, Mx)
        assert_close(mc.cpu().numpy(), ref_mix(w, "cat", pc_h), 1e-5, f"{kind} mix_cat")
        assert_close(ma.cpu().numpy(), ref_mix(w, "an", pa_h), 1e-5, f"{kind} mix_an")
        for case, nT in enumerate((1, 3, 8) if k == 0 else (0,)):
            T_h = np.linspace(253.0, 393.0, nT).astype(np.float32) if k == 0 else None
            T = torch.from_numpy(T_h).to(DEV) if k == 0 else None
            want = gathered_head(kind, pc, pa, T, wp, F, Mx).cpu().numpy()
            n = Cn * An * max(nT, 1)
            offset = (Cn + An + case) % 4
            whole, out_ptr = guarded(n, offset)
            pwhole, params_ptr = guarded(Cn * An * 3, (offset + 1) % 4) if k == 0 else (None, None)
            _lib.check(lib.impnn_head_grid(k, _lib.ptr(mc), _lib.ptr(ma), _lib.ptr(T) if k == 0 else None, _lib.ptr(wp),
                                           out_ptr, params_ptr, Cn, An, nT, D, F, Mx, _lib.stream_ptr()))
            torch.cuda.synchronize()
            got = split_guarded(whole, n, offset).reshape(want.shape)
            assert np.array_equal(bits(got), bits(want)), f"{kind} {shape} {dims} nT={nT}: grid != head kernel bitwise"
            # the public wrapper gives the same bits
            again = ops.head_grid(kind, mc, ma, T, wp, F, Mx)
            assert np.array_equal(bits(again.cpu().numpy()), bits(want))
            ref, vp, pref = ref_grid(kind, w, pc_h, pa_h, T_h)
            assert_close(got, ref, 1e-5, f"{kind} {shape} {dims} grid vs fp64")
            if k == 0:
                params = split_guarded(pwhole, Cn * An * 3, (offset + 1) % 4).reshape(Cn, An, 3)
                p64 = params.astype(np.float64)  # (against fp64 itself: test_params_..., on well-conditioned rows)
                own = p64[..., 0:1] + p64[..., 1:2] / (T_h.astype(np.float64)[None, None, :] / 100.0 + p64[..., 2:3] + 1e-6)
                assert_close(got, own, 1e-6, "out against its own parameters")
                assert (params[..., 1] >= 0).all() and (params[..., 1] <= 20).all()
                assert (params[..., 2] >= np.float32(0.1)).all() and (params[..., 2] <= 50).all()
                cover = branch_coverage(vp)
                print(f"{shape} {dims} nT={nT} branches: {cover}")
                if Cn * An >= 400:  # large enough for every scale of pooled_rows on both sides
                    assert all(cover.values()), cover


def test_params_against_fp64_and_out_against_params():
    """2. The VFT parameters against the fp64 oracle pieces (1e-5), and `out` against A + B / (T/100 + C + 1e-6)
    recomputed in fp64 from the returned fp32 parameters (1e-6)."""
    D, F, Mx, Cn, An = 32, 32, 20, 33, 70
    w = head_weights("viscosity", D, F, Mx, seed=9)
    wp = torch.from_numpy(pack("viscosity", w)).to(DEV)
    # scales that keep |vp| near 100: the fp32 sums then carry ~1e-5 absolute error, 1e-6 of the parameters' range
    # (the four-decade rows of test 1 cancel 1e3-sized terms, which no fp32 sum holds to 1e-5 of B's range of 20)
    scales = (0.05, 0.5, 2.0, 8.0, 30.0, 60.0)
    pc_h, pa_h = pooled_rows(Cn, D, 1, scales), pooled_rows(An, D, 2, scales)
    T_h = np.array([253.0, 298.15, 300.0, 350.5, 393.0], np.float32)
    mc = ops.head_ion_mix("viscosity", 0, torch.from_numpy(pc_h).to(DEV), wp, F, Mx)
    ma = ops.head_ion_mix("viscosity", 1, torch.from_numpy(pa_h).to(DEV), wp, F, Mx)
    out, params = ops.head_grid("viscosity", mc, ma, torch.from_numpy(T_h).to(DEV), wp, F, Mx, return_params=True)
    out, params = out.cpu().numpy(), params.cpu().numpy()
    assert out.shape == (Cn, An, 5) and params.shape == (Cn, An, 3)
    ref, vp, pref = ref_grid("viscosity", w, pc_h, pa_h, T_h)
    cover = branch_coverage(vp)
    assert all(v for k, v in cover.items() if k != "C clipped at 50"), cover  # (that clip: the bitwise test's rows)
    for c, name in enumerate("ABC"):
        assert_close(params[..., c], pref[..., c], 1e-5, f"param {name}")
    assert params[..., 1].min() >= 0.0 and params[..., 1].max() == 20.0
    assert params[..., 2].min() == np.float32(0.1) and params[..., 2].max() <= 50.0
    p = params.astype(np.float64)
    again = p[..., 0:1] + p[..., 1:2] / (T_h.astype(np.float64)[None, None, :] / 100.0 + p[..., 2:3] + 1e-6)
    assert_close(out, again, 1e-6, "out against its own parameters")
    assert_close(out, ref, 1e-5, "out against fp64")
    with pytest.raises(ValueError, match="return_params"):
        ops.head_grid("melting_point", mc, ma, None, wp, F, Mx, return_params=True)


@pytest.mark.parametrize("kind", KINDS)
def test_a_nan_row_stays_in_its_row(kind):
    """3. One cation's pooled row is NaN: exactly that row of the grid is NaN, everything else keeps its bits."""
    D, F, Mx, Cn, An = 32, 32, 20, 19, 67
    w = head_weights(kind, D, F, Mx, seed=4)
    wp = torch.from_numpy(pack(kind, w)).to(DEV)
    pc, pa = torch.from_numpy(pooled_rows(Cn, D, 5)).to(DEV), torch.from_numpy(pooled_rows(An, D, 6)).to(DEV)
    T = torch.tensor([280.0, 300.0, 333.0], device=DEV) if kind == "viscosity" else None

    def run(pc):
        return ops.head_grid(kind, ops.head_ion_mix(kind, "cat", pc, wp, F, Mx), ops.head_ion_mix(kind, "an", pa, wp, F, Mx),
                             T, wp, F, Mx).cpu().numpy()

    clean = run(pc)
    assert np.isfinite(clean).all()
    bad = pc.clone()
    bad[17] = float("nan")
    got = run(bad)
    assert np.isnan(got[17]).all(), "the NaN cation's row must be NaN everywhere"
    keep = np.arange(Cn) != 17
    assert np.array_equal(bits(got[keep]), bits(clean[keep]))


# ---------------------------------------------------------------- model level
def species(n, seed, N=40, E=80):
    b = synthetic.make_batch(n, max_atoms=N, max_edges=E, seed=seed, with_temperature=False)
    return {k: b[f"cat_{k}"] for k in MM.ION_KEYS}, {k: b[f"an_{k}"] for k in MM.ION_KEYS}


def expanded(cat, an, T=None):
    """The explicit pair list of the product, row (i * A + j) * nT + t."""
    Cn, An, nT = len(cat["atom"]), len(an["atom"]), 1 if T is None else len(T)
    ci = np.repeat(np.arange(Cn), An * nT)
    ai = np.tile(np.repeat(np.arange(An), nT), Cn)
    inp = {f"cat_{k}": cat[k][ci] for k in MM.ION_KEYS}
    inp.update({f"an_{k}": an[k][ai] for k in MM.ION_KEYS})
    if T is not None:
        inp["temperature"] = np.tile(np.asarray(T, np.float32), Cn * An)[:, None]
    return inp


def oracle_grid(kind, w, cat, an, T=None):
    """The fp64 oracle on every pair: its encode() once per species (a pair's rows do not depend on the batch), then
    its head pieces over the product; check_oracle_grid ties it to the oracle's own forward on explicit pairs."""
    fp = {p: O.encode(w, p, s["atom"], s["bond"], s["connectivity"], np.float64) for p, s in (("cat", cat), ("an", an))}
    d = lambda n: np.asarray(w[n], np.float64)
    mixed = (O.dense(fp["cat"], d("cat_proj/kernel"), d("cat_proj/bias"), "relu")[:, None, :]
             + O.dense(fp["an"], d("an_proj/kernel"), d("an_proj/bias"), "relu")[None, :, :])
    if kind == "viscosity":
        vp = O.dense(mixed, d("visc_params/kernel"), d("visc_params/bias"))
        B = np.clip(O._softplus(vp[..., 1]), 0.0, 20.0)
        Cc = np.clip(O._softplus(vp[..., 2]), 0.1, 50.0)
        return vp[..., 0, None] + B[..., None] / (np.asarray(T, np.float64)[None, None, :] / 100.0 + Cc[..., None] + 1e-6)
    hid = O.dense(mixed, d("mp_hidden/kernel"), d("mp_hidden/bias"), "relu")
    return O.dense(hid, d("mp_out/kernel"), d("mp_out/bias"))[..., 0]


def check_oracle_grid(kind, w, cat, an, T, grid, rows=48, seed=0):
    """oracle_grid against the oracle's forward on a sample of explicit pairs."""
    inp = expanded(cat, an, T)
    pick = np.random.default_rng(seed).choice(len(inp["cat_atom"]), size=min(rows, len(inp["cat_atom"])), replace=False)
    sub = {k: v[pick] for k, v in inp.items()}
    fwd = O.viscosity_forward if kind == "viscosity" else O.melting_point_forward
    np.testing.assert_allclose(grid.reshape(-1)[pick], fwd(w, sub, np.float64).reshape(-1), rtol=1e-11, atol=1e-11)


def make_model(kind, seed=1, **kw):
    Va, Vb = synthetic.DEFAULT_VA, synthetic.DEFAULT_VB
    if kind == "viscosity":
        w = weights.init_weights(kind, Va, Vb, seed=seed, perturb=True, **kw)
        m = MM.build_model(Va, Vb, device=DEV, **kw)
    else:
        w = weights.init_weights(kind, Va, Vb, bond_dim=kw["atom_dim"] ** 2, seed=seed, perturb=True, **kw)
        m = MM.build_melting_point_model(Va, Vb, device=DEV, **kw)
    m.load_weights(w)
    return m, w


T5 = np.array([263.15, 298.15, 313.0, 353.15, 390.0], np.float32)


@pytest.fixture(scope="module")
def config2():
    """Config-2 shape (D=32, K=8, S=3, N=40, E=80), C=37 x A=23 x nT=5: model, inputs, and the references computed
    once (the fp64 oracle over the product; predict on the 4 255 expanded pairs)."""
    m, w = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=3)
    cat, _ = species(37, 10)
    _, an = species(23, 11)
    ref = oracle_grid("viscosity", w, cat, an, T5)
    check_oracle_grid("viscosity", w, cat, an, T5, ref)
    pred = m.predict(expanded(cat, an, T5)).reshape(37, 23, 5)
    return {"m": m, "w": w, "cat": cat, "an": an, "ref": ref, "pred": pred}


def test_model_grid_viscosity(config2):
    """4. predict_grid against the oracle and against predict on the expanded list; run-to-run bits; encode_ions."""
    m, cat, an = config2["m"], config2["cat"], config2["an"]
    got = m.predict_grid(cat, an, T5)
    assert got.shape == (37, 23, 5) and got.dtype == np.float32
    assert_close(got, config2["ref"], 1e-5, "predict_grid vs fp64 oracle")
    assert_close(got, config2["pred"], 1e-5, "predict_grid vs predict on the expanded list")
    print("predict_grid == predict bitwise:", bool(np.array_equal(bits(got), bits(config2["pred"]))))
    assert np.array_equal(bits(m.predict_grid(cat, an, T5)), bits(got)), "two runs must agree bitwise"
    got_t = m.predict_grid({k: torch.from_numpy(v) for k, v in cat.items()}, an, torch.from_numpy(T5))
    assert np.array_equal(bits(got_t), bits(got)), "torch inputs"
    out, params = m.predict_grid(cat, an, T5, return_params=True)
    assert np.array_equal(bits(out), bits(got)) and params.shape == (37, 23, 3)
    # encode_ions against encode_pooled on paired rows
    pc, pa = m.encode_ions(cat, an)
    assert pc.shape == (37, 32) and pa.shape == (23, 32)
    pair = {f"cat_{k}": torch.from_numpy(cat[k][:23]).to(DEV) for k in MM.ION_KEYS}
    pair.update({f"an_{k}": torch.from_numpy(an[k]).to(DEV) for k in MM.ION_KEYS})
    with torch.no_grad():
        qc, qa = m.encode_pooled(pair)
    assert_close(pc[:23].cpu().numpy(), qc.cpu().numpy(), 1e-5, "encode_ions cations vs encode_pooled")
    assert_close(pa.cpu().numpy(), qa.cpu().numpy(), 1e-5, "encode_ions anions vs encode_pooled")
    print("encode_ions == encode_pooled bitwise:", torch.equal(pc[:23], qc) and torch.equal(pa, qa))
    only_c, none = m.encode_ions(cations=cat)
    assert none is None
    assert_close(only_c.cpu().numpy(), pc.cpu().numpy(), 1e-5, "cations alone")
    none, only_a = m.encode_ions(anions=an)
    assert none is None
    assert_close(only_a.cpu().numpy(), pa.cpu().numpy(), 1e-5, "anions alone")
    for p, s, t in (("cat", cat, pc), ("an", an, pa)):
        ref = O.encode(config2["w"], p, s["atom"], s["bond"], s["connectivity"], np.float64, pooled_only=True)
        assert_close(t.cpu().numpy(), ref, 1e-5, f"encode_ions {p} vs oracle")


def test_max_pairs_per_launch_gives_the_same_bits(config2):
    """7. Three host tiles of the cation axis (13 + 13 + 11 rows of 23 pairs) against one launch."""
    m, cat, an = config2["m"], config2["cat"], config2["an"]
    one, p1 = m.predict_grid(cat, an, T5, return_params=True)
    three, p3 = m.predict_grid(cat, an, T5, return_params=True, max_pairs_per_launch=13 * 23)
    assert np.array_equal(bits(one), bits(three)) and np.array_equal(bits(p1), bits(p3))
    assert_close(one, config2["ref"], 1e-5, "tiled grid vs oracle")
    rows = m.predict_grid(cat, an, T5, max_pairs_per_launch=1)  # below one row of anions: a row at a time
    assert np.array_equal(bits(rows), bits(one))


def test_unequal_species():
    """5. Anions padded to N=12, E=16, cations to N=40, E=80; A = 300 > C = 5 with batch_size 128: padding molecules
    on the cation side, three encoder chunks."""
    m, w = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=3, seed=2)
    cat, _ = species(5, 20)
    _, an = species(300, 21, N=12, E=16)
    T = np.array([298.15, 350.0], np.float32)
    ref = oracle_grid("viscosity", w, cat, an, T)
    got = m.predict_grid(cat, an, T, batch_size=128)
    assert got.shape == (5, 300, 2)
    assert_close(got, ref, 1e-5, "unequal species vs oracle")
    pc, pa = m.encode_ions(cat, an, batch_size=128)
    assert pc.shape == (5, 32) and pa.shape == (300, 32)
    for p, s, t in (("cat", cat, pc), ("an", an, pa)):
        assert_close(t.cpu().numpy(), O.encode(w, p, s["atom"], s["bond"], s["connectivity"], np.float64, pooled_only=True),
                     1e-5, f"pooled {p} vs oracle")


@pytest.mark.parametrize("atom_dim", [8, 32])
def test_melting_point_model(atom_dim):
    """6a. atom_dim 8 (the layered path) and 32, C = 9 x A = 11."""
    m, w = make_model("melting_point", atom_dim=atom_dim, num_steps=2, seed=3)
    cat, _ = species(9, 30)
    _, an = species(11, 31)
    ref = oracle_grid("melting_point", w, cat, an)
    check_oracle_grid("melting_point", w, cat, an, None, ref)
    got = m.predict_grid(cat, an)
    assert got.shape == (9, 11)
    assert_close(got, ref, 1e-5, "melting point grid vs oracle")
    assert_close(got, m.predict(expanded(cat, an)).reshape(9, 11), 1e-5, "melting point grid vs predict")
    with pytest.raises(ValueError, match="return_params"):
        m.predict_grid(cat, an, return_params=True)


def test_wide_model():
    """6b. atom_dim 128, S = 2, C = 5 x A = 6 x nT = 2."""
    m, w = make_model("viscosity", atom_dim=128, bond_dim=8, num_steps=2, seed=4)
    cat, _ = species(5, 40)
    _, an = species(6, 41)
    T = np.array([280.0, 360.0], np.float32)
    got = m.predict_grid(cat, an, T)
    assert_close(got, oracle_grid("viscosity", w, cat, an, T), 1e-5, "wide grid vs oracle")
    assert_close(got, m.predict(expanded(cat, an, T)).reshape(5, 6, 2), 1e-5, "wide grid vs predict")


def test_transfer_model_takes_the_gathered_path(tmp_path):
    """6c. The transfer model (its own 256-128-64 head with moving statistics): gathered tiles through self.head,
    against its own predict on the expanded list; tiled and untiled agree bitwise."""
    from test_gpu_transfer import make_transfer
    t = make_transfer(tmp_path, S=2)
    cat, _ = species(7, 50)
    _, an = species(9, 51)
    assert not t._grid_kernels_cover()
    got = t.predict_grid(cat, an)
    assert got.shape == (7, 9)
    assert_close(got, t.predict(expanded(cat, an)).reshape(7, 9), 1e-5, "transfer grid vs predict")
    assert np.array_equal(bits(t.predict_grid(cat, an, max_pairs_per_launch=20)), bits(got))
    with pytest.raises(ValueError, match="return_params"):
        t.predict_grid(cat, an, return_params=True)


def test_wide_head_takes_the_gathered_path():
    """fp_size 96 is beyond the head kernels (<= 64): the gathered tiles go through the layer-by-layer head."""
    m, w = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=1, fp_size=96, mixing_size=20, seed=6)
    cat, _ = species(4, 60)
    _, an = species(5, 61)
    T = np.array([300.0, 310.0, 320.0], np.float32)
    assert not m._grid_kernels_cover()
    got = m.predict_grid(cat, an, T)
    assert_close(got, oracle_grid("viscosity", w, cat, an, T), 1e-5, "fp_size 96 grid vs oracle")


def test_data_set_round_trip():
    """8. Records with repeated pairs at several temperatures: predict_grid on unique_ions, indexed by
    (cat_index, an_index, t), against predict on the records."""
    base, vocab = synthetic.make_id_records(6, seed=8)
    temps = [273.15, 298.15, 323.15, 348.15]
    recs = []
    for k, (a, b) in enumerate([(0, 0), (1, 0), (0, 1), (2, 2), (3, 1), (1, 0), (4, 5), (2, 2), (0, 0), (5, 3)]):
        for t in temps[k % 2::2] if k % 3 else temps:
            recs.append({"pair_id": f"p{k}", "cation": base[a]["cation"], "anion": base[b]["anion"], "T": t, "log_eta": 0.0})
    ds = data.IonPairDataset(recs, vocab)
    w = weights.init_weights("viscosity", ds.atom_vocab_size, ds.bond_vocab_size, num_steps=2, seed=5, perturb=True)
    m = MM.build_model(ds.atom_vocab_size, ds.bond_vocab_size, num_steps=2, device=DEV)
    m.load_weights(w)
    want = m.predict(ds.build_inputs(range(len(ds))))[:, 0]
    cats, ans, ci, ai = ds.unique_ions()
    assert len(cats["atom"]) == 6 and len(ans["atom"]) == 5 and len(ci) == len(recs)
    ti = np.array([temps.index(r["T"]) for r in recs])
    grid = m.predict_grid(cats, ans, np.array(temps, np.float32))
    assert grid.shape == (6, 5, 4)
    assert_close(grid[ci, ai, ti], want, 1e-5, "grid indexed by the records vs predict")
    # the record-level helper names the same species
    rc, ra, ci0, ai0 = data.unique_ions(recs)
    assert len(rc) == 6 and len(ra) == 5 and np.array_equal(ci, ci0) and np.array_equal(ai, ai0)
