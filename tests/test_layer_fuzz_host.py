"""tests/test_gpu_layer_fuzz.py on the CPU: (1) attainability - every case of its tables, the oracle in fp32 against the
oracle in fp64 under the very checks the GPU tests apply to the kernels: a plain f32 implementation stays inside 1e-5
on exactly these inputs, so a kernel that does not has a defect, not a hard case; (2) coverage - a literal set of
branch names per operation, one per branch of the dispatch, which the cases' claimed branches must cover and outside
of which no restatement may answer; (3) sensitivity - per operation, a reference whose last ragged rows are off by 3e-5
of the tensor's scale must fail the shared check."""
import numpy as np
import pytest

import test_gpu_layer_fuzz as FZ

F32, F64 = np.float32, np.float64


def ids(cases):
    return [c.name for c in cases]


# --------------------------------------------------------------------------------------------- attainability
@pytest.mark.parametrize("c", FZ.gated_update_cases(), ids=ids(FZ.gated_update_cases()))
def test_f32_attains_the_gated_update_bound(c):
    assert FZ.gated_update_branch(c) == c.branch
    inp = FZ.gated_update_inputs(c)
    FZ.check_gated_update(c, FZ.gated_update_reference(inp, F32), FZ.gated_update_reference(inp, F64))
    if c.row_list:   # a list that fills no whole tile, holds row 0, in ascending order, and leaves rows out
        n, idx = inp["n"], inp["idx"]
        assert n % 64 and 0 < n < c.rows and idx[0] == 0 and (np.diff(idx[:n]) > 0).all()
        assert np.array_equal(np.nonzero(inp["keep"])[0], idx[:n])


@pytest.mark.parametrize("c", FZ.message_cases(), ids=ids(FZ.message_cases()))
def test_f32_attains_the_typed_message_bound(c):
    assert FZ.message_branch(c) == (c.kernel, c.sort)
    inp = FZ.message_inputs(c)
    if c.E == 0:
        return
    for h, A in (("h", "A"), ("h2", "A2")) if c.flags else (("h", "A"),):
        FZ.check_messages(c, FZ.message_reference(inp[h], inp[A], inp["bond"], inp["conn"], F32),
                          FZ.message_reference(inp[h], inp[A], inp["bond"], inp["conn"], F64), inp["bond"], inp["conn"])
    valid = FZ.GR.valid_edges(inp["bond"], inp["conn"], c.Vb).numpy()
    assert valid.any() and (~valid).any(), "every case has edges that carry a message and masked ones"
    if c.graph == "oor":
        assert ((inp["bond"] < 0) | (inp["bond"] >= c.Vb)).any()


def test_both_message_references_agree_in_fp64():
    """The oracle's BondMatrixMessage on a one-hot bond state and grad_ref's per-type step are one function."""
    c = FZ.M("agree", 24, 5, 9, 11, 40, "seg valu", FZ.ONE, graph="oor")
    rng = np.random.default_rng(1)
    conn, bond = FZ.make_graph(c.graph, c.B, c.N, c.E, c.Vb, rng)
    h, A = rng.normal(size=(c.B, c.N, c.D)), rng.normal(size=(c.Vb, c.D, c.D))
    a = FZ.message_reference(h, A, bond, conn, F64)
    saved = FZ.ORACLE_MAX_ELEMS
    try:
        FZ.ORACLE_MAX_ELEMS = 0
        b = FZ.message_reference(h, A, bond, conn, F64)
    finally:
        FZ.ORACLE_MAX_ELEMS = saved
    assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()


@pytest.mark.parametrize("c", FZ.type_matrices_cases(), ids=ids(FZ.type_matrices_cases()))
def test_f32_attains_the_type_matrix_bound(c):
    assert FZ.type_matrices_branch(c) == c.branch
    inp = FZ.type_matrices_inputs(c)
    FZ.check_type_matrices(c, FZ.type_matrices_reference(inp, F32), FZ.type_matrices_reference(inp, F64))


@pytest.mark.parametrize("c", FZ.dense_message_cases(), ids=ids(FZ.dense_message_cases()))
def test_f32_attains_the_dense_message_bound(c):
    assert FZ.dense_message_branch(c) == c.branch
    inp = FZ.dense_message_inputs(c)
    FZ.check_dense_message(c, FZ.dense_message_reference(c, inp, F32), FZ.dense_message_reference(c, inp, F64), inp["conn"])


@pytest.mark.parametrize("c", FZ.pool_cases(), ids=ids(FZ.pool_cases()))
def test_f32_attains_the_pool_bound(c):
    assert FZ.pool_branch(c) == c.branch
    inp = FZ.pool_inputs(c)
    FZ.check_pool(c, FZ.pool_reference(inp, F32), FZ.pool_reference(inp, F64))


@pytest.mark.parametrize("c", FZ.reduce_cases(), ids=ids(FZ.reduce_cases()))
def test_the_reduce_reference_is_the_sequential_scatter(c):
    """reduce_reference against a literal walk of the edge slots, on the first and the last molecule."""
    assert FZ.reduce_branch(c) == c.branch
    inp = FZ.reduce_inputs(c)
    ref = FZ.reduce_reference(inp, c.N)
    tgt = inp["tgt"]
    assert (tgt == 0).any() and (tgt < 0).any() and (tgt >= c.N).any() and (tgt == 3).mean() > 0.2
    for b in {0, c.B - 1}:
        want = np.zeros((c.N, c.D), F32)
        for e in range(c.E):
            if 0 < tgt[b, e] < c.N:
                want[tgt[b, e]] += inp["m"][b, e]
        np.testing.assert_array_equal(ref[b], want)


@pytest.mark.parametrize("c", FZ.embed_cases(), ids=ids(FZ.embed_cases()))
def test_the_embed_reference_is_the_table_lookup(c):
    assert FZ.embed_branch(c) == c.branch
    inp = FZ.embed_inputs(c)
    ref = FZ.embed_reference(inp)
    assert ref.dtype == F32 and ref.shape == (c.rows, c.dim)
    bad = (inp["ids"] < 0) | (inp["ids"] >= c.vocab)
    assert bad.any() and not ref[bad].any()
    np.testing.assert_array_equal(ref[~bad], inp["table"][inp["ids"][~bad]])


# --------------------------------------------------------------------------------------------- coverage
GATED_UPDATE_BRANCHES = {
    "wide NT=3", "wide NT=5", "wide NT=6", "wide NT=7",
    "wide16 tile16", "wide16 tile16 ragged", "wide16 tile64", "wide16 tile64 ragged",
    "generic<8>", "generic<8> idle threads", "generic<4>", "generic<4> idle threads", "generic<4> misaligned",
    "d32", "d32 grid-stride",
    "d32 row list", "wide16 tile16 row list", "wide16 tile64 row list",
}
MESSAGE_KERNELS = {
    "d32 tm=1", "d32 tm=2", "d32 tm=2 ragged", "d32 tm=3 ragged", "d32 tm=4 ragged", "d32 tm=32 ragged",
    "seg mfma 256", "seg mfma 1024 spw=1", "seg mfma 1024 spw=2", "seg valu", "generic", "no launch",
}
MESSAGE_SORTS = {FZ.ONE, FZ.FOUR, FZ.IN_KERNEL, FZ.NONE}
# (kernel, D) pairs and (kernel, what) features the issue names one by one
MESSAGE_WIDTHS = {("seg mfma 256", 16), ("seg mfma 256", 48), ("seg mfma 1024 spw=1", 80),
                  ("seg mfma 1024 spw=1", 96), ("seg mfma 1024 spw=1", 112), ("seg mfma 1024 spw=1", 64), ("seg mfma 1024 spw=1", 128),
                  ("seg mfma 1024 spw=2", 64), ("seg valu", 8), ("seg valu", 24), ("seg valu", 40), ("generic", 144),
                  ("generic", 32)}
TYPE_MATRIX_BRANCHES = {"valu", "mfma<2>", "mfma<5>", "mfma<8>", "strided gemm"}
REDUCE_BRANCHES = {
    "small P=8", "small P=5", "small P=4", "small P=2",
    "large list, one range", "large list, ranges", "large list, ranges ragged",
    "large list, ranges ragged, sums in global memory",
    "large walk, one range", "large walk, ranges",
    "large cols<D, ranges", "large cols<D, ranges ragged",
}
DENSE_MESSAGE_BRANCHES = {("message", "h in lds"), ("message", "h in global memory"), ("fused", "h in lds"),
                          ("fused", "h in global memory")}
EMBED_BRANCHES = {"embed_gather<4>", "embed_gather<1>", "embed_gather<4> grid-stride", "embed_gather<1> grid-stride"}
POOL_BRANCHES = {"global_sum_pool", "global_sum_pool grid-stride"}


def covered(cases, claimed, restated, names):
    assert {claimed(c) for c in cases} == names, "the cases' claimed branches are the dispatch's branches"
    for c in cases:
        assert restated(c) in names and restated(c) == claimed(c), c.name


def test_the_case_tables_cover_every_branch():
    covered(FZ.gated_update_cases(), lambda c: c.branch, FZ.gated_update_branch, GATED_UPDATE_BRANCHES)
    covered(FZ.message_cases(), lambda c: c.kernel, lambda c: FZ.message_branch(c)[0], MESSAGE_KERNELS)
    covered(FZ.message_cases(), lambda c: c.sort, lambda c: FZ.message_branch(c)[1], MESSAGE_SORTS)
    covered(FZ.type_matrices_cases(), lambda c: c.branch, FZ.type_matrices_branch, TYPE_MATRIX_BRANCHES)
    covered(FZ.reduce_cases(), lambda c: c.branch, FZ.reduce_branch, REDUCE_BRANCHES)
    covered(FZ.dense_message_cases(), lambda c: (c.op, c.branch), lambda c: (c.op, FZ.dense_message_branch(c)),
            DENSE_MESSAGE_BRANCHES)
    covered(FZ.embed_cases(), lambda c: c.branch, FZ.embed_branch, EMBED_BRANCHES)
    covered(FZ.pool_cases(), lambda c: c.branch, FZ.pool_branch, POOL_BRANCHES)


def test_the_case_tables_hold_what_the_dispatch_turns_on():
    gu = FZ.gated_update_cases()
    has = lambda cases, **kw: any(all(getattr(c, k) == v for k, v in kw.items()) for c in cases)
    # GatedUpdate: the smallest shapes of the 64-row tiles and of the D = 32 grid-stride regime, both widths, row lists
    for D in (64, 128):
        assert has(gu, D=D, rows=8192 + 5, row_list=False) and has(gu, D=D, rows=8192 + 5, row_list=True)
    assert has(gu, D=64, rows=8191) and has(gu, D=64, rows=8192) and has(gu, D=32, rows=65536 + 16 + 3)
    assert {c.D for c in gu if c.branch.startswith("generic<8>")} == {72, 136, 256}
    assert {24, 40} <= {c.D for c in gu if c.branch == "generic<4> idle threads"}
    assert {c.misalign for c in gu if c.D == 32} == {None, "h", "agg"}
    # typed messages
    ms = FZ.message_cases()
    assert MESSAGE_WIDTHS <= {(c.kernel, c.D) for c in ms}
    assert has(ms, D=32, E=128, kernel="d32 tm=1") and has(ms, D=32, E=129, kernel="generic")
    assert has(ms, D=32, Vb=1024, kernel="d32 tm=1") and has(ms, D=32, Vb=1025, kernel="generic")
    assert has(ms, D=32, misalign="h", kernel="generic") and has(ms, B=16384 + 7, kernel="d32 tm=32 ragged")
    assert any(c.E <= 8 for c in ms if c.kernel == "d32 tm=32 ragged")
    spw2 = [c for c in ms if c.kernel == "seg mfma 1024 spw=2"]
    assert all(131072 < c.B * c.E < 131072 + 1024 and c.N <= 8 for c in spw2)
    assert {c.misalign for c in ms if c.kernel == "seg valu"} == {None, "h", "A"}
    assert {c.graph for c in ms} == {"dense", "oor", "one_type", "half_types", "star", "dup4"}
    flags = [c for c in ms if c.flags]
    assert {c.kernel for c in flags} == {"seg mfma 1024 spw=1", "seg mfma 256", "seg valu"} and {c.sort for c in flags} == {FZ.ONE, FZ.FOUR}
    for kernel in ("seg mfma 256", "seg mfma 1024 spw=1", "seg valu"):
        assert {c.sort for c in ms if c.kernel == kernel} == {FZ.ONE, FZ.FOUR}, kernel
    assert has(ms, E=0)
    # type matrices: the matrix-core kernels on vocabularies that fill no whole 16-row tile; every way into the GEMM
    tm = FZ.type_matrices_cases()
    for b in ("mfma<2>", "mfma<5>", "mfma<8>"):
        assert any(c.Vb % 16 for c in tm if c.branch == b) and any(c.Vb % 16 == 0 for c in tm if c.branch == b)
    gemm = [c for c in tm if c.branch == "strided gemm"]
    assert any(c.K % 64 for c in gemm) and any((c.D * c.D) % 16 for c in gemm) and any(c.Vb > 128 for c in gemm)
    assert any(c.misalign for c in gemm)
    # reduce: P = 5 at D = 48, P = 2 at D = 100 and 128; the large kernel below 2048 molecules
    rs = FZ.reduce_cases()
    assert has(rs, D=48, branch="small P=5") and has(rs, D=100, branch="small P=2") and has(rs, D=128, branch="small P=2")
    assert has(rs, D=8, E=300, branch="large walk, one range") and has(rs, D=32, E=1100, branch="large walk, ranges")
    assert any(c.B < 2048 and c.D <= 128 and c.branch.startswith("large") for c in rs)
    assert any(128 < c.D <= 256 and c.B < 2048 for c in rs) and any(c.D > 256 for c in rs)
    # embedding: a width that is no multiple of 4, a misaligned table
    assert any(c.dim % 4 for c in FZ.embed_cases()) and any(c.misalign for c in FZ.embed_cases())


# --------------------------------------------------------------------------------------------- sensitivity
def off_by(ref, where):
    """ref with ``where`` off by 3e-5 of the tensor's scale."""
    out = np.array(ref, dtype=F64)
    out[where] += 3e-5 * np.abs(out).max()
    return out


def case(cases, name):
    return next(c for c in cases if c.name == name)


def test_the_checks_see_a_wrong_ragged_tail():
    """One ragged-tail case per operation: the f32 oracle passes against the fp64 reference and fails against the same
    reference with its last ragged rows off by 3e-5 of the tensor's scale (bit-exact checks: by one ulp-sized step)."""
    # GatedUpdate: the five rows of the last 64-row tile
    c = case(FZ.gated_update_cases(), "wide16 D=128 64-row tiles ragged")
    inp = FZ.gated_update_inputs(c)
    got, ref = FZ.gated_update_reference(inp, F32), FZ.gated_update_reference(inp, F64)
    tail = FZ.gated_update_tail(c)
    assert (tail.start, tail.stop) == (8192, 8197)
    FZ.check_gated_update(c, got, ref)
    with pytest.raises(AssertionError):
        FZ.check_gated_update(c, got, off_by(ref, tail))
    with pytest.raises(AssertionError):
        FZ.check_gated_update(c, got, off_by(ref, (c.rows - 1, c.D - 1)))
    # typed messages: the valid edges of the last workgroup's molecules (B % tm of them)
    c = case(FZ.message_cases(), "d32 tm=32 B=16384+7")
    inp = FZ.message_inputs(c)
    got, ref = (FZ.message_reference(inp["h"], inp["A"], inp["bond"], inp["conn"], t) for t in (F32, F64))
    valid = FZ.GR.valid_edges(inp["bond"], inp["conn"], c.Vb).numpy()
    last = np.zeros_like(valid)
    last[c.B - c.B % 32:] = valid[c.B - c.B % 32:]
    assert c.B % 32 == 7 and last.any()
    FZ.check_messages(c, got, ref, inp["bond"], inp["conn"])
    with pytest.raises(AssertionError):
        FZ.check_messages(c, got, off_by(ref, last), inp["bond"], inp["conn"])
    one = np.zeros_like(valid)   # a single message, and a masked edge's row that is not zero
    one[tuple(np.argwhere(last)[-1])] = True
    with pytest.raises(AssertionError):
        FZ.check_messages(c, got, off_by(ref, one), inp["bond"], inp["conn"])
    dirty = got.copy()
    dirty[tuple(np.argwhere(~valid)[-1])] = 1e-30
    with pytest.raises(AssertionError):
        FZ.check_messages(c, dirty, ref, inp["bond"], inp["conn"])
    # type matrices: the one vocabulary row of the second 16-row tile
    c = case(FZ.type_matrices_cases(), "mfma<2> Vb=17")
    inp = FZ.type_matrices_inputs(c)
    got, ref = FZ.type_matrices_reference(inp, F32), FZ.type_matrices_reference(inp, F64)
    FZ.check_type_matrices(c, got, ref)
    with pytest.raises(AssertionError):
        FZ.check_type_matrices(c, got, off_by(ref, slice(16, 17)))
    # dense messages: the last molecule
    c = case(FZ.dense_message_cases(), "fused (N + E) * D past 160 KiB")
    inp = FZ.dense_message_inputs(c)
    got, ref = FZ.dense_message_reference(c, inp, F32), FZ.dense_message_reference(c, inp, F64)
    FZ.check_dense_message(c, got, ref, inp["conn"])
    with pytest.raises(AssertionError):
        FZ.check_dense_message(c, got, off_by(ref, (c.B - 1, c.N - 1)), inp["conn"])
    # pool: the molecules past the last whole grid stride
    c = case(FZ.pool_cases(), "past the grid cap")
    inp = FZ.pool_inputs(c)
    got, ref = FZ.pool_reference(inp, F32), FZ.pool_reference(inp, F64)
    FZ.check_pool(c, got, ref)
    with pytest.raises(AssertionError):
        FZ.check_pool(c, got, off_by(ref, slice(FZ.GRID_CAP_ITEMS // c.D, c.B)))
    # reduce (bit for bit): the rows of the last, shorter row range
    c = case(FZ.reduce_cases(), "D=64 N=300: past the 64 KiB of the small kernel")
    inp = FZ.reduce_inputs(c)
    ref = FZ.reduce_reference(inp, c.N)
    FZ.check_reduce(c, ref.copy(), ref)
    wrong = ref.copy()
    wrong[:, 285:] = np.nextafter(wrong[:, 285:], F32(np.inf))
    with pytest.raises(AssertionError):
        FZ.check_reduce(c, wrong, ref)
    # embedding (bit for bit): the rows past the last whole grid stride
    c = case(FZ.embed_cases(), "dim=32 past the grid cap")
    inp = FZ.embed_inputs(c)
    ref = FZ.embed_reference(inp)
    FZ.check_embed(c, ref.copy(), ref)
    wrong = ref.copy()
    wrong[65536:] = np.nextafter(wrong[65536:], F32(np.inf))
    with pytest.raises(AssertionError):
        FZ.check_embed(c, wrong, ref)
