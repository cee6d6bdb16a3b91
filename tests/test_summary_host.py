"""Per-ion statistics of the grid, on the host: data.grid_ion_records / grid_ion_summary - the reference the summary
kernels are held to bit for bit (tests/test_gpu_summary.py) - against exact sums and plain loops, the rule that lets a
caller cut the cation axis, the records of masked-out blocks, the edge records, the argument errors of
ops.grid_summary and the three screen_ion_summary surfaces, the status codes of the C entries on stand-in pointers
(every row returns before a launch), and the footprint inventory of the new entries."""
import ast
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from ionic_mpnn_amd import _lib, data, model as MM, ops, synthetic
from ionic_mpnn_amd.ensemble import ModelEnsemble

CPU = torch.device("cpu")
BLOCKS = ((16, 64), (8, 32))


def bits(rec):
    views = (np.uint32, np.uint64, np.uint32)
    return [np.ascontiguousarray(x).view(views[f % 3]) for f, x in enumerate(rec)]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))


def case(C_, A_, nT, seed, scale=30.0):
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal((C_, A_, nT)) * scale).astype(np.float32)
    g[rng.random(g.shape) < 0.05] = np.nan
    return (g if nT else g[..., 0]), rng.random((C_, A_)) < 0.6


# ---------------------------------------------------------------- 1. the reference against exact sums and plain loops
@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("shape", [(1, 1, 1), (17, 65, 2), (37, 130, 1), (9, 33, 3)])
def test_the_reference_against_exact_sums(shape, blocks):
    """s and q against math.fsum of the same terms.  The bound is derived: every sum is n - 1 (or fewer, in the tree)
    float64 additions of its terms in some order, each of which rounds its partial sum by at most 2^-53 of it, and no
    partial sum exceeds sum|term|; so |s - exact| <= (n - 1) * 2^-53 * sum|term| < n * 2^-52 * sum|term|.  The terms
    themselves are exact: a float32 as a double, and the product of two float32 values in double."""
    grid, where = case(*shape, seed=sum(shape))
    for wh in (None, where):
        rec = data.grid_ion_records(grid, wh, blocks)
        planes = np.moveaxis(grid, 2, 0)
        live = ~np.isnan(planes) & (True if wh is None else wh[None])
        for axis, (count, sums, rng) in ((2, rec[:3]), (1, rec[3:])):
            for t in range(planes.shape[0]):
                for i in range(planes.shape[3 - axis]):
                    line = planes[t, i, :] if axis == 2 else planes[t, :, i]
                    keep = live[t, i, :] if axis == 2 else live[t, :, i]
                    vals = [float(x) for x in line[keep]]
                    n = len(vals)
                    assert count[t, i] == n
                    for f, terms in enumerate((vals, [x * x for x in vals])):
                        exact, bound = math.fsum(terms), n * 2.0 ** -52 * math.fsum(abs(x) for x in terms)
                        assert abs(sums[t, i, f] - exact) <= bound, (axis, t, i, f)
                    if n == 0:
                        assert rng[t, i].view(np.uint32).tolist() == [0x7FC00000] * 2 and not sums[t, i].any()
                        assert not np.signbit(sums[t, i]).any()
                    else:  # a plain loop under the key order
                        lo = hi = line[keep][0]
                        for x in line[keep][1:]:
                            if data.select_keys(np.array([x]))[0] < data.select_keys(np.array([lo]))[0]:
                                lo = x
                            if data.select_keys(np.array([x]))[0] > data.select_keys(np.array([hi]))[0]:
                                hi = x
                        assert rng[t, i].view(np.uint32).tolist() == [np.float32(lo).view(np.uint32), np.float32(hi).view(np.uint32)]


def test_the_finishing_and_the_shapes():
    grid, where = case(17, 65, 2, seed=4)
    s = data.grid_ion_summary(grid, where)
    assert isinstance(s, data.IonSummary) and isinstance(s.by_cation, data.IonStats)
    assert s.by_cation.mean.shape == (2, 17) and s.by_anion.max.shape == (2, 65) and s.overall.count.shape == (2,)
    assert s.by_cation.count.dtype == np.int64 and all(x.dtype == np.float32 for x in s.by_cation[1:])
    live = ~np.isnan(grid) & where[:, :, None]
    for t in range(2):
        for i in range(17):
            v = grid[i, :, t][live[i, :, t]].astype(np.float64)
            assert s.by_cation.count[t, i] == len(v)
            assert np.isclose(s.by_cation.mean[t, i], v.mean(), rtol=1e-6) and np.isclose(s.by_cation.std[t, i], v.std(), rtol=1e-5)
            assert s.by_cation.min[t, i] == v.min() and s.by_cation.max[t, i] == v.max()
        v = grid[:, :, t][live[:, :, t]].astype(np.float64)
        assert s.overall.count[t] == len(v) and np.isclose(s.overall.mean[t], v.mean(), rtol=1e-6)
        assert np.isclose(s.overall.std[t], v.std(), rtol=1e-5) and s.overall.min[t] == v.min() and s.overall.max[t] == v.max()
    flat = data.grid_ion_summary(grid[:, :, 0], where, (8, 32))
    assert flat.by_cation.mean.shape == (17,) and flat.by_anion.mean.shape == (65,) and np.ndim(flat.overall.mean) == 0
    # IonStats.order: by value, then index, NaN last; largest turns the values round, not the NaNs
    st = data.IonStats(np.array([1, 1, 0, 1, 1]), *[np.array([2.0, -1.0, np.nan, 2.0, -0.0], np.float32)] * 4)
    assert st.order().tolist() == [1, 4, 0, 3, 2] and st.order("max", largest=True).tolist() == [0, 3, 4, 1, 2]
    assert s.by_anion.order("std").shape == (2, 65)
    with pytest.raises(ValueError, match="by must be"):
        st.order("median")


# ---------------------------------------------------------------- 2. carry-over
@pytest.mark.parametrize("blocks", BLOCKS)
def test_cutting_at_block_multiples_and_carrying_gives_the_whole_grid(blocks):
    grid, where = case(53, 70, 2, seed=8)
    for wh in (None, where):
        whole = data.grid_ion_records(grid, wh, blocks)
        for cuts in ((16,), (32,), (16, 32, 48), (48,)):
            carry, cat = None, []
            for lo, hi in zip((0,) + cuts, cuts + (53,)):
                part = data.grid_ion_records(grid[lo:hi], None if wh is None else wh[lo:hi], blocks, carry=carry)
                cat.append(part[:3])
                carry = part[3:]
            got = [np.concatenate([c[f] for c in cat], axis=1) for f in range(3)] + list(carry)
            assert same(got, whole), cuts


def test_a_cut_that_is_no_multiple_changes_bits():
    """The rule is not vacuous: on this input a cut at cation 10 rounds some anion sum differently."""
    grid, _ = case(53, 70, 2, seed=8)
    whole = data.grid_ion_records(grid)
    first = data.grid_ion_records(grid[:10])
    got = data.grid_ion_records(grid[10:], carry=first[3:])
    assert np.array_equal(got.an_count, whole.an_count) and np.array_equal(bits(got)[5], bits(whole)[5])
    assert not np.array_equal(bits(got)[4], bits(whole)[4])
    assert np.allclose(got.an_sums, whole.an_sums, rtol=1e-12)


# ---------------------------------------------------------------- 3. skipped tiles
@pytest.mark.parametrize("blocks", BLOCKS)
def test_a_masked_out_block_gives_what_computing_it_gives(blocks):
    """A block the mask clears contributes +0.0 partials with n = 0: the records equal those of the same mask applied
    term by term, i.e. of a grid whose masked-out values are anything at all."""
    grid, where = case(37, 130, 1, seed=2)
    bc, ba = blocks
    where[bc:2 * bc, ba:2 * ba] = False
    where[:, 5] = False
    want = data.grid_ion_records(grid, where, blocks)
    junk = grid.copy()
    junk[~where] = np.float32(1e30)          # what a skipped tile never evaluates
    assert same(data.grid_ion_records(junk, where, blocks), want)
    # term by term: the same sums from the competing values alone, blocks of the same extent
    planes = np.moveaxis(grid, 2, 0)
    for j in (5, ba, ba + 3):
        s = 0.0
        for b0 in range(0, 37, bc):
            part = 0.0
            for i in range(b0, min(b0 + bc, 37)):
                if where[i, j] and not np.isnan(planes[0, i, j]):
                    part = part + float(planes[0, i, j])
            s = s + part
        assert want.an_sums[0, j, 0] == s
    assert want.an_count[0, 5] == 0 and not want.an_sums[0, 5].any()


# ---------------------------------------------------------------- 4. edge records
def test_edge_records():
    g = np.array([[1.5, -0.0, np.nan, 0.0], [np.nan] * 4, [2.0, 3.0, 4.0, 5.0]], np.float32)
    where = np.ones((3, 4), bool)
    where[2] = False                          # a mask row of zeros
    s = data.grid_ion_summary(g, where, (8, 32))
    c = s.by_cation
    assert c.count.tolist() == [3, 0, 0]
    for i in (1, 2):                          # the NaN row and the masked row
        assert all(x[i].view(np.uint32) == 0x7FC00000 for x in (c.mean, c.std, c.min, c.max))
        assert not s.records.cat_sums[0, i].any() and not np.signbit(s.records.cat_sums[0, i]).any()
    assert c.min[0].view(np.uint32) == 0x80000000 and c.max[0] == 1.5      # -0.0 < +0.0 < 1.5
    a = s.by_anion
    assert a.count.tolist() == [1, 1, 0, 1]
    assert a.std[[0, 1, 3]].tolist() == [0.0, 0.0, 0.0] and np.isnan(a.std[2])   # one competing pair: std exactly 0
    assert a.min[1].view(np.uint32) == 0x80000000 and a.max[3].view(np.uint32) == 0
    zeros = data.grid_ion_summary(np.array([[0.0, -0.0]], np.float32))
    assert zeros.by_cation.min[0].view(np.uint32) == 0x80000000 and zeros.by_cation.max[0].view(np.uint32) == 0
    assert zeros.overall.count == 2 and s.overall.count == 3 and s.overall.min.view(np.uint32) == 0x80000000
    one = data.grid_ion_summary(np.array([[np.float32(0.1)]], np.float32))
    assert one.overall.std == 0.0 and one.overall.mean == np.float32(0.1)
    empty = data.grid_ion_summary(np.zeros((0, 4), np.float32))
    assert empty.by_cation.mean.shape == (0,) and empty.by_anion.count.tolist() == [0] * 4 and empty.overall.count == 0


def test_reference_argument_errors():
    g = np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError, match="grid must be"):
        data.grid_ion_summary(np.zeros(4, np.float32))
    with pytest.raises(ValueError, match="blocks"):
        data.grid_ion_summary(g, blocks=(16, 48))
    with pytest.raises(ValueError, match="where must be"):
        data.grid_ion_summary(g, where=np.ones((4, 3), bool))
    with pytest.raises(ValueError, match="carry"):
        data.grid_ion_records(g, carry=(np.zeros((1, 3)), np.zeros((1, 3, 2)), np.zeros((1, 3, 2))))


# ---------------------------------------------------------------- 5. the wrappers' errors, without a GPU
def _species(n, seed):
    b = synthetic.make_batch(n, max_atoms=24, max_edges=48, seed=seed, with_temperature=False)
    return {k: b[f"cat_{k}"] for k in MM.ION_KEYS}, {k: b[f"an_{k}"] for k in MM.ION_KEYS}


def test_ops_grid_summary_errors():
    assert ops.SUMMARY_BLOCKS == {0: (16, 64), 1: (8, 32), 2: (16, 64), 3: (8, 32)}
    g = ops.GridOperands(1, 1, torch.zeros(3, 256), torch.zeros(4, 256), None, torch.zeros(8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grid_summary(g)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grid_summary(g, where=torch.zeros(3, 1, dtype=torch.int32))


def test_screen_ion_summary_argument_errors():
    VA, VB = synthetic.DEFAULT_VA, synthetic.DEFAULT_VB
    cat, an = _species(2, 1)
    v = MM.build_model(VA, VB, num_steps=1, device=CPU)
    t = MM.MPNNModel("transfer", VA, VB, 32, 8, 32, 20, 1, 1e-4, device=CPU)
    with pytest.raises(KeyError, match="temperature"):
        v.screen_ion_summary(cat, an)
    with pytest.raises(ValueError, match="both"):
        v.screen_ion_summary(cat, None, temperatures=[300.0])
    with pytest.raises(ValueError, match="max_pairs_per_launch"):
        v.screen_ion_summary(cat, an, temperatures=[300.0], max_pairs_per_launch=0)
    with pytest.raises(TypeError, match="PairMask"):
        v.screen_ion_summary(cat, an, temperatures=[300.0], where=np.ones((2, 2), bool))
    with pytest.raises(ValueError, match="at least one"):
        v.screen_ion_summary(cat, an, temperatures=[])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        v.screen_ion_summary(cat, an, temperatures=[300.0])
    ens = ModelEnsemble([v, MM.build_model(VA, VB, num_steps=1, device=CPU)])
    with pytest.raises(ValueError, match="kappa"):
        ens.screen_ion_summary(cat, an, temperatures=[300.0], kappa=float("inf"))
    with pytest.raises(KeyError, match="temperature"):
        ens.screen_ion_summary(cat, an)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ens.screen_ion_summary(cat, an, temperatures=[300.0])
    mc = t.mc_dropout(4)
    with pytest.raises(ValueError, match="kappa"):
        mc.screen_ion_summary(cat, an, kappa=float("nan"))
    with pytest.raises(TypeError, match="PairMask"):
        mc.screen_ion_summary(cat, an, where=np.ones((2, 2), bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mc.screen_ion_summary(cat, an)


# ---------------------------------------------------------------- 6. the C entries on stand-in pointers
_P = 0x100000   # 16-byte aligned, never dereferenced: every call below returns before a launch
_BAD, _UNS, _WS = -1, -2, -4
ENTRIES = ("impnn_head_grid_summary", "impnn_transfer_head_grid_summary", "impnn_deep_ensemble_grid_summary",
           "impnn_transfer_mc_grid_summary")


def _call(lib, family, **kw):
    a = dict(kind=0, M=3, S=4, kappa=1.0, cat=_P, an=_P, T=_P, w=_P, mult=_P, image_floats=1 << 20, where=None, carry=0,
             ws_bytes=None, C=19, A=70, nT=2, D=32, F=32, Mx=20, table=[_P] * 7)
    a.update(kw)
    nT = a["nT"] if family in (0, 2) else 0
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(int(lib.impnn_grid_summary_workspace_bytes(family, max(a["C"], 0), max(a["A"], 0), max(nT, 1))), 0)
    table = C.cast((C.c_void_p * 7)(*a["table"]), _lib.PP) if a["table"] is not None else None
    tail = (a["where"], a["carry"], a["ws_bytes"], table)
    if family == 0:
        rc = lib.impnn_head_grid_summary(a["kind"], a["cat"], a["an"], a["T"], a["w"], *tail, a["C"], a["A"], nT, a["D"],
                                         a["F"], a["Mx"], None)
    elif family == 1:
        rc = lib.impnn_transfer_head_grid_summary(a["cat"], a["an"], a["w"], a["image_floats"], *tail, a["C"], a["A"], None)
    elif family == 2:
        rc = lib.impnn_deep_ensemble_grid_summary(a["kind"], a["M"], a["cat"], a["an"], a["T"], a["w"], a["kappa"], *tail, a["C"],
                                             a["A"], nT, a["F"], a["Mx"], None)
    else:
        rc = lib.impnn_transfer_mc_grid_summary(a["cat"], a["an"], a["w"], a["image_floats"], a["mult"], a["S"], a["kappa"],
                                                *tail, a["C"], a["A"], None)
    return rc, lib.impnn_last_error_string()


def test_the_workspace_query():
    lib = _lib.load()
    q = lib.impnn_grid_summary_workspace_bytes
    for family, (bc, ba) in ops.SUMMARY_BLOCKS.items():
        for C_, A_, planes in ((1, 1, 1), (19, 70, 2 if family in (0, 2) else 1), (16, 64, 1), (4096, 4096, 1)):
            assert q(family, C_, A_, planes) == 32 * planes * (-(-A_ // ba) * C_ + -(-C_ // bc) * A_)
        assert q(family, 4096, 4096, 1) / 4096 ** 2 == 32 * (1 / bc + 1 / ba)      # the workspace per pair
        assert q(family, 0, 5, 1) == 0 and q(family, -1, 5, 1) == 0 and q(family, 5, 5, 0) == 0
        assert (q(family, 5, 5, 2) > 0) == (family in (0, 2)) and q(family, 5, 5, 4097) == 0
    assert q(4, 5, 5, 1) == 0 and q(-1, 5, 5, 1) == 0
    assert lib.impnn_abi_version() == 3


@pytest.mark.parametrize("family", (0, 1, 2, 3))
def test_status_codes_in_the_partners_entries_order(family):
    lib = _lib.load()
    name = ENTRIES[family].encode()
    assert _call(lib, family, C=0, table=None, cat=None)[0] == 0                    # zero work touches nothing
    rc, msg = _call(lib, family, C=-1)
    assert rc == _BAD and msg == name + b": bad shape"
    rc, msg = _call(lib, family, carry=2)
    assert rc == _BAD and b"carry" in msg
    if family in (0, 2):
        rc, msg = _call(lib, family, kind=2)
        assert rc == _BAD and b"kind must be" in msg
        rc, msg = _call(lib, family, nT=4097, ws_bytes=1 << 40)
        assert rc == _UNS and b"nT=4097" in msg
        rc, msg = _call(lib, family, Mx=65)
        assert rc == _UNS and b"Mx=65" in msg
        rc, msg = _call(lib, family, Mx=65, C=0)                                    # the widths come before zero work
        assert rc == _UNS
    if family == 2:
        assert _call(lib, family, M=0)[0] == _BAD and _call(lib, family, M=9)[0] == _UNS
    if family == 3:
        assert _call(lib, family, S=0)[0] == _BAD and _call(lib, family, S=65)[0] == _UNS
    if family >= 2:
        rc, msg = _call(lib, family, kappa=float("nan"))
        assert rc == _BAD and b"kappa" in msg
    for kw in (dict(cat=None), dict(table=None), dict(table=[_P] * 6 + [None]), dict(table=[None] + [_P] * 6)):
        rc, msg = _call(lib, family, **kw)
        assert rc == _BAD and msg == name + b": null pointer", kw
    rc, msg = _call(lib, family, table=[_P] * 6 + [_P + 4])
    assert rc == _BAD and b"workspace must be 8-byte aligned" in msg
    rc, msg = _call(lib, family, where=_P + 2)
    assert rc == _BAD and b"mask must be 4-byte aligned" in msg
    if family in (1, 3):
        rc, msg = _call(lib, family, image_floats=8)
        assert rc == _WS and b"image" in msg
    need = int(lib.impnn_grid_summary_workspace_bytes(family, 19, 70, 2 if family in (0, 2) else 1))
    rc, msg = _call(lib, family, ws_bytes=need - 1)
    assert rc == _WS and b"too small" in msg and name in msg
    rc, msg = _call(lib, family, table=[_P, _P + 4] + [_P] * 5)                    # after the workspace size: the outputs
    assert rc == _BAD and b"sums must be 8-byte aligned" in msg


def test_partners_and_rank_still_refuse_the_ensemble_and_mc_families():
    for g in (ops.GridOperands(2, 0, torch.zeros(2, 3, 20), torch.zeros(2, 4, 20), torch.zeros(1), torch.zeros(2, 63), (32, 20), 0.5),
              ops.GridOperands(3, 1, torch.zeros(3, 256), torch.zeros(4, 256), None, torch.zeros(8), (), 0.5, torch.ones(2, 128))):
        with pytest.raises(NotImplementedError, match="partners / rank are not built"):
            ops.grid_partners(g)
        with pytest.raises(NotImplementedError, match="partners / rank are not built"):
            ops.grid_rank(g, 1)


# ---------------------------------------------------------------- 7. the footprint inventory of the new entries
def test_every_summary_entry_is_called_on_guarded_buffers():
    """The entries name the buffers they write in a const host table, so tests/footprint.py's inventory (entries with a
    non-const pointer parameter) does not list them; their footprint tests live in tests/test_gpu_summary.py, and this
    holds that every one of them is named there, in a file that builds Guarded( buffers and calls what it names."""
    import footprint as F
    entries = F.entries()
    names = sorted(n for n in entries if re.fullmatch(r"impnn_\w+_grid_summary", n))
    assert names == sorted(ENTRIES)
    for n in names:
        assert entries[n]["mutable"] == [] and "buffers" in entries[n]["const"], n
    assert entries["impnn_grid_summary_workspace_bytes"]["ret"] == "int64_t"
    path = ROOT / "tests" / "test_gpu_summary.py"
    src = path.read_text()
    tree = ast.parse(src)
    strings = {n.value for n in ast.walk(tree) if isinstance(n, ast.Constant) and isinstance(n.value, str)}
    for n in names:
        assert n in strings, f"{n} is not named in test_gpu_summary.py"
    fn = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    assert "test_nothing_is_written_outside_the_outputs_and_the_workspace" in fn and "guarded_summary" in fn
    body = ast.get_source_segment(src, fn["guarded_summary"])
    assert len(re.findall(r"\bGuarded\(", body)) >= 2 and "ENTRIES[g.family]" in body
    assert "impnn_grid_summary_workspace_bytes" in body and "max(need" not in src and "1 << 20" not in src
