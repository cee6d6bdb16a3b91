"""Per-ion statistics of the grid on the GPU: impnn_head_grid_summary, impnn_transfer_head_grid_summary,
impnn_deep_ensemble_grid_summary and impnn_transfer_mc_grid_summary against data.grid_ion_records of the materialised grid
(ops.grid_values on the same operands; the ensemble and MC families' score), with and without a pair mask, and the three
screen_ion_summary surfaces against data.grid_ion_summary(predict_grid(...)).

Everything here is exact.  A summarised value is computed by the tile code of the materialising kernel, the sums run in
double in one stated order that data.grid_ion_records restates, counts are integers and the least / greatest value are
selected, not computed: the six record tensors are compared bit for bit (the doubles as uint64).  No tolerance appears."""
import ctypes as C

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, data, ops

from footprint import FILL, Guarded
from test_gpu_grid import T5, make_model, species
from test_gpu_screen import T_MAX, head_case, transfer_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("viscosity", "melting_point")
DIMS = (32, 32, 20)
HEAD_SHAPES = [(1, 1, 1), (16, 64, 1), (17, 65, 3), (37, 130, 2)]
TRANSFER_SHAPES = [(1, 1), (8, 32), (9, 33), (37, 130)]
# the four entries by family: each is called below on Guarded( outputs and a Guarded( workspace of exactly the queried size
ENTRIES = {0: "impnn_head_grid_summary", 1: "impnn_transfer_head_grid_summary", 2: "impnn_deep_ensemble_grid_summary",
           3: "impnn_transfer_mc_grid_summary"}
RECORD_BYTES = (4, 16, 8)   # per ion and plane: count uint32, sums 2 x double, range 2 x float
VIEWS = (np.uint32, np.uint64, np.uint32)
NAMES = ("cat_count", "cat_sums", "cat_range", "an_count", "an_sums", "an_range")
shape_id = lambda s: "x".join(str(n) for n in s)


def as_bits(rec):
    out = []
    for f, x in enumerate(rec):
        x = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x)
        out.append(x.view(VIEWS[f % 3]))
    return out


def same(got, want, what):
    for name, g, w in zip(NAMES, as_bits(got), as_bits(want)):
        assert g.shape == w.shape, f"{what}: {name} has shape {g.shape}, the reference {w.shape}"
        assert np.array_equal(g, w), f"{what}: {name} differs in {int((g != w).sum())} of {g.size} words"


def score_grid(g):
    """The values the summary of ``g`` is about, materialised: the grid, or the score of the ensemble and MC families."""
    v = ops.grid_values(g)
    return (v[2] if g.family >= 2 else v).cpu().numpy()


def reference(g, where=None):
    return data.grid_ion_summary(score_grid(g), where, ops.SUMMARY_BLOCKS[g.family]).records


def dev_words(where):
    return None if where is None else data.PairMask.from_bool(where, device=DEV).words


def masks_of(Cn, An, tile):
    """none, all clear, random half, one whole tile clear, one cation row clear, one anion column clear"""
    rng = np.random.default_rng(1000 * Cn + An)
    out = {"none": None, "clear": np.zeros((Cn, An), bool), "half": rng.random((Cn, An)) < 0.5}
    t = np.ones((Cn, An), bool)
    t[:tile[0], :tile[1]] = False
    out["tile"] = t
    r = rng.random((Cn, An)) < 0.7
    r[Cn // 2] = False
    out["row"] = r
    c = rng.random((Cn, An)) < 0.7
    c[:, An // 2] = False
    out["column"] = c
    return out


# ---------------------------------------------------------------- the operands of the four families
def head_operands(kind, shape, seed=5):
    Cn, An, nT = shape
    wp, mc, ma = head_case(kind, DIMS, (Cn, An), seed=seed)
    T = torch.from_numpy(T_MAX[:nT].copy()).to(DEV) if kind == "viscosity" else None
    return ops.head_grid_operands(kind, mc, ma, T, wp, DIMS[1], DIMS[2])


def transfer_operands(shape):
    return ops.transfer_grid_operands(*transfer_case(DIMS, shape))


def ensemble_operands(kind, M, shape, kappa, T=None):
    Cn, An, nT = shape
    k = ops.HEAD_KINDS[kind]
    n = int(_lib.load().impnn_ensemble_grid_tail_floats(k, DIMS[1], DIMS[2]))
    members = [head_case(kind, DIMS, (Cn, An), seed=5 + 3 * m) for m in range(M)]
    if T is None and kind == "viscosity":
        T = torch.from_numpy(T_MAX[:nT].copy()).to(DEV)
    return ops.ensemble_grid_operands(kind, torch.stack([m[1] for m in members]), torch.stack([m[2] for m in members]), T,
                                      torch.stack([m[0][-n:] for m in members]), DIMS[1], DIMS[2], kappa)


def mc_operands(S, shape, kappa):
    uc, ua, image = transfer_case(DIMS, shape)
    rng = np.random.default_rng(77 + S)
    mult = np.where(rng.random((S, ops.TRANSFER_MC_WIDTH)) < 0.3, 0.0, 1.0 / 0.7).astype(np.float32)
    return ops.transfer_mc_grid_operands(uc, ua, image, torch.from_numpy(mult).to(DEV), kappa)


# ---------------------------------------------------------------- 1. head grid
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=shape_id)
@pytest.mark.parametrize("kind", KINDS)
def test_head_summary_is_the_reference_on_the_materialised_grid(kind, shape):
    g = head_operands(kind, shape)
    grid = score_grid(g)
    for name, where in masks_of(shape[0], shape[1], ops.SUMMARY_BLOCKS[0]).items():
        got = ops.grid_summary(g, where=dev_words(where))
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.float64 and got[2].dtype == torch.float32
        assert tuple(got[1].shape) == (max(g.nT, 1), shape[0], 2) and tuple(got[4].shape) == (max(g.nT, 1), shape[1], 2)
        same(got, data.grid_ion_summary(grid, where, ops.SUMMARY_BLOCKS[0]).records, f"{kind} {shape} mask {name}")


# ---------------------------------------------------------------- 2. transfer grid
@pytest.mark.parametrize("shape", TRANSFER_SHAPES, ids=shape_id)
def test_transfer_summary_is_the_reference_on_the_materialised_grid(shape):
    g = transfer_operands(shape)
    grid = score_grid(g)
    for name, where in masks_of(shape[0], shape[1], ops.SUMMARY_BLOCKS[1]).items():
        same(ops.grid_summary(g, where=dev_words(where)), data.grid_ion_summary(grid, where, ops.SUMMARY_BLOCKS[1]).records,
             f"transfer {shape} mask {name}")


# ---------------------------------------------------------------- 3. NaN operand rows
def with_nan_rows(g, ci, aj):
    cat, an = g.cat.clone(), g.an.clone()
    cat[..., ci, :] = float("nan")
    an[..., aj, :] = float("nan")
    return ops.GridOperands(g.family, g.kind, cat, an, g.T, g.w, g.widths, g.kappa, g.multipliers)


@pytest.mark.parametrize("family", ("viscosity", "melting_point", "transfer"))
def test_a_nan_ion_has_count_zero_and_its_partners_exclude_it(family):
    g = head_operands(family, (17, 65, 2)) if family != "transfer" else transfer_operands((9, 33))
    g = with_nan_rows(g, 3, 7)
    want = reference(g)
    assert (want.cat_count[:, 3] == 0).all() and (want.an_count[:, 7] == 0).all(), "the reference holds no ion with count 0"
    assert (np.delete(want.cat_count, 3, axis=1) == g.A - 1).all() and g.A - 1 > 1
    assert (np.delete(want.an_count, 7, axis=1) == g.C - 1).all() and g.C - 1 > 1
    assert np.isnan(want.cat_range[:, 3]).all() and not want.cat_sums[:, 3].any()
    same(ops.grid_summary(g), want, f"{family} with a NaN cation and a NaN anion")
    where = np.random.default_rng(3).random((g.C, g.A)) < 0.5
    same(ops.grid_summary(g, where=dev_words(where)), reference(g, where), f"{family} with NaN ions and a mask")


# ---------------------------------------------------------------- 4. ensemble grid
@pytest.mark.parametrize("kind", KINDS)
def test_ensemble_summary_is_the_reference_on_the_score(kind):
    shape = (17, 65, 2)
    single = ops.grid_summary(head_operands(kind, shape))
    same(ops.grid_summary(ensemble_operands(kind, 1, shape, 0.0)), single, f"{kind}: one member, kappa 0, against the model's own")
    where = masks_of(17, 65, ops.SUMMARY_BLOCKS[2])
    for kappa in (1.0, -1.0):
        g = ensemble_operands(kind, 3, shape, kappa)
        for name in ("none", "half", "tile"):
            same(ops.grid_summary(g, where=dev_words(where[name])), reference(g, where[name]), f"{kind} M=3 kappa {kappa} mask {name}")


def test_ensemble_summary_at_the_most_temperatures_a_launch_takes():
    lib = _lib.load()
    most = int(lib.impnn_ensemble_grid_max_temperatures(0, 8))
    assert most >= 1 and lib.impnn_grid_summary_workspace_bytes(2, 17, 65, most) > 0
    assert lib.impnn_grid_summary_workspace_bytes(2, 17, 65, most + 1) == 0
    T = torch.linspace(250.0, 420.0, most, device=DEV)
    g = ensemble_operands("viscosity", 8, (17, 65, most), 0.5, T=T)
    same(ops.grid_summary(g), reference(g), f"M=8 at {most} temperatures")


# ---------------------------------------------------------------- 5. transfer MC grid
@pytest.mark.parametrize("S", (1, 4))
def test_mc_summary_is_the_reference_on_the_score(S):
    where = masks_of(19, 70, ops.SUMMARY_BLOCKS[3])
    for kappa in (0.0, 1.0):
        g = mc_operands(S, (19, 70), kappa)
        for name in ("none", "half", "tile"):
            same(ops.grid_summary(g, where=dev_words(where[name])), reference(g, where[name]), f"MC S={S} kappa {kappa} mask {name}")


# ---------------------------------------------------------------- 6. the model surfaces and the host tiling
def same_summary(got, want, what):
    same(got.records, want.records, what)
    for side in ("by_cation", "by_anion", "overall"):
        for f, (a, b) in enumerate(zip(getattr(got, side), getattr(want, side))):
            a, b = np.asarray(a), np.asarray(b)
            assert a.shape == b.shape and a.dtype == b.dtype, (what, side, f)
            assert a.tobytes() == b.tobytes(), (what, side, f)


@pytest.fixture(scope="module")
def screen_species():
    cat, _ = species(40, 70)
    _, an = species(9, 71)
    return cat, an


def test_model_summary_does_not_depend_on_the_host_tiling(screen_species):
    cat, an = screen_species
    m, _ = make_model("viscosity", atom_dim=32, bond_dim=8, num_steps=1)
    T = T5[[1, 3]]
    assert m._grid_kernels_cover()
    want = data.grid_ion_summary(m.predict_grid(cat, an, temperatures=T), None, ops.SUMMARY_BLOCKS[0])
    assert want.by_cation.mean.shape == (2, 40) and want.by_anion.mean.shape == (2, 9) and want.overall.mean.shape == (2,)
    for pairs in (None, 16 * 9, 32 * 9, 40 * 9, 5 * 9, 1):   # ranges of everything, 16, 32, everything, and two below 16 x A
        same_summary(m.screen_ion_summary(cat, an, temperatures=T, max_pairs_per_launch=pairs), want, f"max_pairs_per_launch={pairs}")
    rng = np.random.default_rng(9)
    where = data.PairMask.from_bool(rng.random((40, 9)) < 0.6, device=DEV)
    want = data.grid_ion_summary(m.predict_grid(cat, an, temperatures=T), where, ops.SUMMARY_BLOCKS[0])
    for pairs in (None, 16 * 9):
        same_summary(m.screen_ion_summary(cat, an, temperatures=T, where=where, max_pairs_per_launch=pairs), want, f"masked, {pairs}")
    order = want.by_cation.order("mean")
    assert order.shape == (2, 40) and sorted(order[0]) == list(range(40))


def test_the_gathered_fallback_agrees_with_the_kernels(screen_species, monkeypatch):
    cat, an = screen_species
    for kind, kw, tk in (("viscosity", dict(atom_dim=32, bond_dim=8, num_steps=1), dict(temperatures=T5[[1, 3]])),
                         ("melting_point", dict(atom_dim=16, num_steps=1), {})):
        m, _ = make_model(kind, **kw)
        fused = m.screen_ion_summary(cat, an, **tk)
        with monkeypatch.context() as mp:
            mp.setattr(m, "_grid_kernels_cover", lambda: False)
            for pairs in (None, 16 * 9):
                same_summary(m.screen_ion_summary(cat, an, max_pairs_per_launch=pairs, **tk), fused, f"{kind} gathered, {pairs}")


def test_ensemble_and_mc_surfaces(screen_species, tmp_path):
    from ionic_mpnn_amd.ensemble import ModelEnsemble
    from mc_dropout_cases import make_transfer
    cat, an = screen_species
    T = T5[[1, 3]]
    ens = ModelEnsemble([make_model("viscosity", seed=s, atom_dim=32, bond_dim=8, num_steps=1)[0] for s in (1, 2, 3)])
    score = ens.predict_grid(cat, an, temperatures=T, kappa=1.0)[2]
    want = data.grid_ion_summary(score, None, ops.SUMMARY_BLOCKS[2])
    for pairs in (None, 16 * 9):
        same_summary(ens.screen_ion_summary(cat, an, temperatures=T, kappa=1.0, max_pairs_per_launch=pairs), want, f"ensemble, {pairs}")
    mc = make_transfer(tmp_path, DEV).mc_dropout(samples=4, draw=3)
    score = mc.predict_grid(cat, an, kappa=1.0)[2]
    want = data.grid_ion_summary(score, None, ops.SUMMARY_BLOCKS[3])
    assert want.by_cation.mean.shape == (40,) and np.ndim(want.overall.mean) == 0
    for pairs in (None, 16 * 9):
        same_summary(mc.screen_ion_summary(cat, an, kappa=1.0, max_pairs_per_launch=pairs), want, f"MC dropout, {pairs}")


# ---------------------------------------------------------------- 7. footprints
def guarded_summary(g, where=None, carry=0, ws_fill=FILL, an_fill=FILL, short=0):
    """The family's entry on outputs and a workspace of exactly the documented size between two guards -> (status, the six
    record arrays, the workspace bytes).  Every const operand is compared afterwards."""
    lib = _lib.load()
    planes = max(g.nT, 1)
    need = int(lib.impnn_grid_summary_workspace_bytes(g.family, g.C, g.A, planes))
    assert need == 32 * planes * (-(-g.A // ops.SUMMARY_BLOCKS[g.family][1]) * g.C + -(-g.C // ops.SUMMARY_BLOCKS[g.family][0]) * g.A)
    out = [Guarded(planes * n * b, fill=FILL if n == g.C else an_fill) for n in (g.C, g.A) for b in RECORD_BYTES]
    ws = Guarded(need, fill=ws_fill)
    words = dev_words(where)
    consts = [t for t in (g.cat, g.an, g.T, g.w, g.multipliers, words) if t is not None]
    before = [t.clone() for t in consts]
    table = (C.c_void_p * 7)(*[o.ptr.value for o in out], ws.ptr.value)
    rc = getattr(lib, ENTRIES[g.family])(*g.lead, _lib.ptr(words) if words is not None else None, carry, need - short, table,
                                         *g.trail, _lib.stream_ptr())
    torch.cuda.synchronize()
    for t, b in zip(consts, before):
        assert torch.equal(t.view(torch.int32), b.view(torch.int32)), "a const operand changed"
    shapes = [(planes, n, *tail) for n in (g.C, g.A) for tail in ((), (2,), (2,))]
    rec = [o.body(VIEWS[f % 3], NAMES[f]).reshape(shapes[f]) for f, o in enumerate(out)]
    return rc, rec, ws.body(np.uint8, "the workspace")


def footprint_cases():
    yield "head viscosity", lambda s: head_operands("viscosity", s + (2,))
    yield "head melting point", lambda s: head_operands("melting_point", s + (0,))
    yield "transfer", transfer_operands
    yield "ensemble", lambda s: ensemble_operands("viscosity", 2, s + (2,), 1.0)
    yield "transfer MC", lambda s: mc_operands(3, s, 1.0)


@pytest.mark.parametrize("name,make", list(footprint_cases()), ids=[n for n, _ in footprint_cases()])
def test_nothing_is_written_outside_the_outputs_and_the_workspace(name, make):
    g, other = make((19, 70)), make((9, 33))
    where = masks_of(19, 70, ops.SUMMARY_BLOCKS[g.family])["tile"]
    want = reference(g, where)
    rc, _, leftover = guarded_summary(other)                      # another shape's workspace, to be left behind
    assert rc == 0
    for what, fill in (("0x00", 0x00), ("0xFF", 0xFF), ("another shape's leftover", leftover)):
        rc, rec, ws = guarded_summary(g, where, ws_fill=fill)
        assert rc == 0, _lib.load().impnn_last_error_string()
        same(rec, want, f"{name}: workspace pre-filled {what}")
    # carry = 0 writes the anion records without reading them
    for fill in (0x00, 0xA5):
        rc, rec, _ = guarded_summary(g, where, an_fill=fill)
        assert rc == 0
        same(rec, want, f"{name}: anion records pre-filled {fill:#x}, carry 0")
    # carry = 1 continues: the first 16 cations, then the rest on top of their anion records
    first = ops.grid_summary(g.rows(0, 16), where=dev_words(where[:16]))
    rest = g.rows(16, 19)
    planes = max(g.nT, 1)
    an_bytes = torch.cat([t.contiguous().view(torch.uint8).reshape(-1) for t in first[3:]])
    sizes = [planes * g.A * b for b in RECORD_BYTES]
    lib = _lib.load()
    need = int(lib.impnn_grid_summary_workspace_bytes(g.family, 3, g.A, planes))
    out = [Guarded(planes * 3 * b) for b in RECORD_BYTES]
    at = np.cumsum([0] + sizes)
    out += [Guarded(sizes[f], fill=an_bytes[at[f]:at[f + 1]]) for f in range(3)]
    ws = Guarded(need)
    words = dev_words(where[16:])
    table = (C.c_void_p * 7)(*[o.ptr.value for o in out], ws.ptr.value)
    assert getattr(lib, ENTRIES[g.family])(*rest.lead, _lib.ptr(words), 1, need, table, *rest.trail, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    for f in range(3):
        got = out[3 + f].body(VIEWS[f], NAMES[3 + f])
        assert np.array_equal(got.reshape(-1), as_bits(want)[3 + f].reshape(-1)), f"{name}: carried {NAMES[3 + f]}"
    # a workspace one byte short is refused before anything is touched
    rc, rec, ws = guarded_summary(g, where, short=1)
    assert rc == -4 and b"too small" in lib.impnn_last_error_string()
    assert (ws == FILL).all() and all((r.view(np.uint8) == FILL).all() for r in rec), f"{name}: a refused call wrote"


# ---------------------------------------------------------------- 8. run to run
def test_two_streams_give_the_same_bits():
    g = head_operands("viscosity", (37, 130, 2))
    where = dev_words(masks_of(37, 130, ops.SUMMARY_BLOCKS[0])["half"])
    torch.cuda.synchronize()
    results = []
    for _ in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            results.append(ops.grid_summary(g, where=where))
        s.synchronize()
    same(results[0], results[1], "two streams")
