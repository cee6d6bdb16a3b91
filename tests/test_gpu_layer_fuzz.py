"""Forward fuzz of the drop-in layer kernels: every branch of their dispatch against fp64 ("Tests").

Reference: oracle/mpnn_oracle.py in fp64; tests/grad_ref.py's O(B E D) message step where the oracle's (B,E,D,D) tensor
would not fit (ORACLE_MAX_ELEMS).  Bounds are the project's existing ones, through conftest.assert_close (1e-5 per
tensor AND per element, floor 0.3); reduce_scatter_add and embed_gather are integer-indexed sums / copies and are
checked bit for bit.  tests/test_layer_fuzz_host.py walks every ``*_cases()`` of this module on the CPU and holds the
oracle in fp32 to the same checks against the oracle in fp64: the bound is attainable by a plain f32 implementation on
exactly these inputs.

How a case is mapped to a branch: each table names, per case, the branch it is meant for; ``*_branch`` restates the
dispatch of launch_* (csrc/layer_kernels.hip), launch_bmm_message_typed_sorted (csrc/message_typed.hip) and the routing
of ops.bmm_message_typed from the shape, with the constants named, and every case asserts that the restatement gives
the branch its row claims.  Every case is seeded by its place in its table."""
from collections import namedtuple

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, ops
from oracle import mpnn_oracle as O
from conftest import assert_close

import grad_ref as GR
from test_gpu_train_fuzz import _dev, make_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL, FLOOR = 1e-5, 0.3

KIB = 1024
K_BLOCK = 256                        # kBlock
LDS_MAX = 160 * KIB                  # kMaxLds
GRID_CAP_ITEMS = 256 * 8 * K_BLOCK   # grid_for: at most 2048 workgroups of kBlock threads, a grid-stride loop beyond
ORACLE_MAX_ELEMS = 1 << 22           # elements of the oracle's (B,E,D,D) tensor (+ one-hot bond state) a case may take


def ceil_div(a, b):
    return -(-a // b)


def _f32(rng, *shape):
    return rng.normal(size=shape).astype(np.float32)


# =====================================================================================================================
# GatedUpdate (launch_gated_update_impl)
# =====================================================================================================================
GU_TILE64_MIN_ROWS = 8192            # gu_wide_tile_rows: 64-row tiles from here, 16-row tiles below
GU_D32_ROWS_PER_BLOCK = 4 * 16       # four waves of 16-row tiles
GU_D32_MAX_BLOCKS = 256 * 4          # grid-stride beyond
GU_ROW_LIST_DIMS = (32, 64, 128)
GU_NAMES = ["Wz", "bz", "Wr", "br", "Wh", "bh", "gamma", "beta"]

GuCase = namedtuple("GuCase", "name D rows branch misalign row_list")


def G(name, D, rows, branch, misalign=None, row_list=False):
    return GuCase(name, D, rows, branch, misalign, row_list)


def gated_update_branch(c):
    """The kernel launch_gated_update_impl takes for a case - its dispatch restated from the shape."""
    assert not c.row_list or c.D in GU_ROW_LIST_DIMS
    if c.D == 32 and c.misalign is None:
        if c.row_list:
            return "d32 row list"
        return "d32 grid-stride" if ceil_div(c.rows, GU_D32_ROWS_PER_BLOCK) > GU_D32_MAX_BLOCKS else "d32"
    if c.D % 16 == 0 and 48 <= c.D <= 128:
        if c.D % 64 == 0:
            tile = 64 if c.rows >= GU_TILE64_MIN_ROWS else 16
            if c.row_list:
                return f"wide16 tile{tile} row list"
            return f"wide16 tile{tile}" + (" ragged" if c.rows % tile else "")
        return f"wide NT={c.D // 16}"
    assert c.D <= K_BLOCK and not c.row_list
    rb = 8 if c.D >= 64 else 4
    return f"generic<{rb}>" + (" idle threads" if K_BLOCK % c.D else "") + (" misaligned" if c.misalign else "")


GU_CASES = [
    # --- gated_update_wide_kernel<NT>: D = 48, 80, 96, 112; 64-row workgroups with a ragged last one
    G("wide D=48", 48, 130, "wide NT=3"),
    G("wide D=80", 80, 130, "wide NT=5"),
    G("wide D=96", 96, 67, "wide NT=6"),
    G("wide D=112", 112, 193, "wide NT=7"),
    # --- gated_update_wide16_kernel on both tile sizes, whole and ragged last tiles, both sides of the 8192-row threshold
    G("wide16 D=64 16-row tiles", 64, 80, "wide16 tile16"),
    G("wide16 D=64 16-row tiles ragged", 64, 83, "wide16 tile16 ragged"),
    G("wide16 D=128 16-row tiles ragged", 128, 37, "wide16 tile16 ragged"),
    G("wide16 D=64 8191 rows", 64, 8191, "wide16 tile16 ragged"),
    G("wide16 D=64 8192 rows", 64, 8192, "wide16 tile64"),
    G("wide16 D=64 64-row tiles ragged", 64, 8192 + 5, "wide16 tile64 ragged"),
    G("wide16 D=128 64-row tiles ragged", 128, 8192 + 5, "wide16 tile64 ragged"),
    # --- gated_update_kernel<8>: D >= 64 outside the matrix-core path
    G("generic D=72", 72, 29, "generic<8> idle threads"),
    G("generic D=136", 136, 19, "generic<8> idle threads"),
    G("generic D=256", 256, 21, "generic<8>"),
    # --- gated_update_kernel<4>: D that does not divide 256 (G = 10 and 6 row groups, threads left over), and one that does
    G("generic D=24", 24, 87, "generic<4> idle threads"),
    G("generic D=40", 40, 50, "generic<4> idle threads"),
    G("generic D=16", 16, 70, "generic<4>"),
    # --- D = 32: the matrix-core kernel, its grid-stride regime (65 536 + 16 + 3 rows: 1025 > 1024 workgroups), and
    #     h or agg one float into its allocation, which the generic kernel serves
    G("d32", 32, 83, "d32"),
    G("d32 grid-stride", 32, 65536 + 16 + 3, "d32 grid-stride"),
    G("d32 h off by one float", 32, 75, "generic<4> misaligned", misalign="h"),
    G("d32 agg off by one float", 32, 33, "generic<4> misaligned", misalign="agg"),
    # --- row lists (rows=): both sides of the tile threshold, which the launch takes from the buffer's rows, not the list's
    G("row list D=64 64-row tiles", 64, 8192 + 5, "wide16 tile64 row list", row_list=True),
    G("row list D=128 64-row tiles", 128, 8192 + 5, "wide16 tile64 row list", row_list=True),
    G("row list D=128 16-row tiles", 128, 333, "wide16 tile16 row list", row_list=True),
    G("row list D=32", 32, 300, "d32 row list", row_list=True),
]


def gated_update_cases():
    return GU_CASES


def gated_update_inputs(c):
    """Weights scaled by 1/sqrt(fan-in); with a row list: ``keep`` (about 0.6 of the rows, row 0 among them, a count
    that fills no whole tile) and the list as the kernels take it."""
    rng = np.random.default_rng(3000 + GU_CASES.index(c))
    D, s = c.D, 1.0 / np.sqrt(2 * c.D)
    p = {"Wz": _f32(rng, 2 * D, D) * np.float32(s), "bz": _f32(rng, D) * np.float32(0.1),
         "Wr": _f32(rng, 2 * D, D) * np.float32(s), "br": _f32(rng, D) * np.float32(0.1),
         "Wh": _f32(rng, 2 * D, D) * np.float32(s), "bh": _f32(rng, D) * np.float32(0.1),
         "gamma": rng.uniform(0.5, 1.5, size=D).astype(np.float32), "beta": _f32(rng, D) * np.float32(0.1)}
    inp = {"p": p, "h": _f32(rng, c.rows, D), "agg": _f32(rng, c.rows, D)}
    if c.row_list:
        keep = rng.random(c.rows) < 0.6
        keep[0] = True
        if int(keep.sum()) % 64 == 0:
            keep[np.nonzero(~keep)[0][0]] = True
        idx = np.zeros(c.rows, np.int32)
        idx[:int(keep.sum())] = np.nonzero(keep)[0]
        inp.update(keep=keep, idx=idx, n=int(keep.sum()))
    return inp


def gated_update_reference(inp, dtype):
    return O.gated_update(inp["h"].astype(dtype), inp["agg"].astype(dtype), {k: v.astype(dtype) for k, v in inp["p"].items()})


def gated_update_tail(c):
    """The rows of the last, partly filled tile of a case's kernel (what a wrong ragged tail would get wrong)."""
    tile = {"wide": 64, "wide16": 64 if c.rows >= GU_TILE64_MIN_ROWS else 16, "d32": 16}[c.branch.split()[0]]
    assert c.rows % tile
    return slice(c.rows - c.rows % tile, c.rows)


def check_gated_update(c, got, ref):
    assert_close(got, ref, TOL, f"{c.name}: GatedUpdate", FLOOR)


@pytest.mark.parametrize("c", GU_CASES, ids=[c.name for c in GU_CASES])
def test_gated_update_fuzz(c):
    """ops.gated_update on the branch the row names against fp64; with a row list the listed rows equal the full call
    bit for bit while every unlisted row of h and agg holds NaN: an unlisted row that is read shows in a listed one."""
    assert gated_update_branch(c) == c.branch
    inp = gated_update_inputs(c)
    ref = gated_update_reference(inp, np.float64)
    w = [_dev(inp["p"][k]) for k in GU_NAMES]
    h, agg = _dev(inp["h"], c.misalign == "h"), _dev(inp["agg"], c.misalign == "agg")
    full = ops.gated_update(h, agg, *w)
    check_gated_update(c, full.cpu().numpy(), ref)
    if c.row_list:
        keep = torch.from_numpy(inp["keep"]).to(DEV)
        assert inp["n"] % 64 and bool(keep[0])
        hn, an = h.clone(), agg.clone()
        hn[~keep] = float("nan")
        an[~keep] = float("nan")
        part = ops.gated_update(hn, an, *w, rows=(_dev(inp["idx"]), _dev(np.array([inp["n"]], np.int32))))
        assert torch.equal(part[keep], full[keep]), f"{c.name}: listed rows differ from the full call"


def test_gated_update_row_list_refuses_misaligned_d32():
    """A row list at atom_dim 32 has no generic kernel to fall to: impnn_gated_update_rows refuses an operand one float
    into its allocation (IMPNN_E_BADARG) before it launches."""
    rng = np.random.default_rng(0)
    c = G("refused", 32, 40, "d32 row list", row_list=True)
    p = [_dev(_f32(rng, *s)) for s in ((64, 32), (32,), (64, 32), (32,), (64, 32), (32,), (32,), (32,))]
    h, agg = _dev(_f32(rng, c.rows, 32), off_by_one=True), _dev(_f32(rng, c.rows, 32))
    rows = (_dev(np.arange(c.rows, dtype=np.int32)), _dev(np.array([7], np.int32)))
    with pytest.raises(_lib.ImpnnError) as e:
        ops.gated_update(h, agg, *p, rows=rows)
    assert e.value.code == -1   # IMPNN_E_BADARG
    assert "impnn_gated_update_rows: a row list or saved buffer at atom_dim 32 needs 16-byte aligned tensors" in str(e.value)


# =====================================================================================================================
# Typed messages, forward (ops.bmm_message_typed -> launch_bmm_message_typed | launch_bmm_message_typed_sorted)
# =====================================================================================================================
K_TM = 32                    # kTM: molecules per workgroup of the D = 32 kernel
K_TSLOTS = 4096              # kTSlots: edge slots a workgroup of it holds in LDS
K_TVB = 1024                 # kTVb: bond types of its LDS histogram
K_SEG = 64                   # kSeg: edges of one type per segment
K_SORT_SMALL_PER = 16        # kSortSmallPer: slots per thread of the one-workgroup sort (1024 threads)
SORT_SMALL_MAX_TYPES = 1024  # it scans one type per thread
SORTED_MAX_D = 128           # ops.bmm_message_typed: the sorted entry serves D != 32 up to here
TM_BATCH_PER_MOLECULE = 512  # tm = clamp(B / 512, 1, kTM)
SPW_SEGS_PER_STEP = 1024     # spw = clamp(max_segs / 1024, 1, 8) at D >= 64
ONE, FOUR, IN_KERNEL, NONE = "one workgroup", "four kernels", "in the kernel", "none"

MsgCase = namedtuple("MsgCase", "name D Vb B N E kernel sort graph misalign flags")


def M(name, D, Vb, B, N, E, kernel, sort, graph="dense", misalign=None, flags=False):
    return MsgCase(name, D, Vb, B, N, E, kernel, sort, graph, misalign, flags)


def message_branch(c):
    """(message kernel, edge sort) ops.bmm_message_typed reaches for a case - routing and dispatch restated."""
    if c.B == 0 or c.E == 0:
        return "no launch", NONE
    if c.D == 32 or c.D > SORTED_MAX_D:   # impnn_bmm_message_typed
        if (c.D == 32 and c.Vb <= K_TVB and K_TM * c.E <= K_TSLOTS and c.E < 1 << 15 and c.N < 1 << 12
                and c.misalign is None):
            tm = min(max(c.B // TM_BATCH_PER_MOLECULE, 1), K_TM)
            return f"d32 tm={tm}" + (" ragged" if c.B % tm else ""), IN_KERNEL
        return "generic", NONE
    sort = ONE if c.B * c.E <= 1024 * K_SORT_SMALL_PER and c.Vb <= SORT_SMALL_MAX_TYPES else FOUR
    if c.D % 16 == 0 and c.misalign is None:
        if c.D < 64:
            return "seg mfma 256", sort
        max_segs = ceil_div(c.B * c.E, K_SEG) + c.Vb
        return f"seg mfma 1024 spw={min(max(max_segs // SPW_SEGS_PER_STEP, 1), 8)}", sort
    return "seg valu", sort


MESSAGE_CASES = [
    # --- bmm_message_typed_d32_kernel: tm = clamp(B / 512, 1, 32) and a last workgroup with fewer molecules
    M("d32 tm=1", 32, 7, 37, 23, 61, "d32 tm=1", IN_KERNEL),
    M("d32 tm=2 B=1101", 32, 6, 1101, 9, 12, "d32 tm=2 ragged", IN_KERNEL),
    M("d32 tm=3 B=1537 oor", 32, 9, 1537, 7, 10, "d32 tm=3 ragged", IN_KERNEL, graph="oor"),
    M("d32 tm=32 B=16384+7", 32, 5, 16384 + 7, 6, 8, "d32 tm=32 ragged", IN_KERNEL),
    M("d32 E=128 (kTM*E == kTSlots)", 32, 6, 40, 30, 128, "d32 tm=1", IN_KERNEL),
    M("d32 E=128 tm=4 (512 slots a workgroup)", 32, 11, 2050, 5, 128, "d32 tm=4 ragged", IN_KERNEL, graph="half_types"),
    M("d32 E=129 falls to the generic kernel", 32, 6, 40, 30, 129, "generic", NONE),
    M("d32 Vb=1024", 32, 1024, 30, 20, 50, "d32 tm=1", IN_KERNEL),
    M("d32 Vb=1025 falls to the generic kernel", 32, 1025, 30, 20, 50, "generic", NONE),
    M("d32 h off by one float", 32, 7, 37, 23, 61, "generic", NONE, misalign="h"),
    M("d32 one type", 32, 12, 600, 12, 30, "d32 tm=1", IN_KERNEL, graph="one_type"),
    M("d32 star", 32, 6, 1030, 9, 40, "d32 tm=2", IN_KERNEL, graph="star"),
    M("d32 dup4", 32, 6, 50, 30, 80, "d32 tm=1", IN_KERNEL, graph="dup4"),
    # --- bmm_message_typed_seg_mfma_kernel: 256 threads below D = 64 (16, 48), 1024 threads from there (80, 96, 112 with
    #     5, 6, 7 feature tiles dealt over 16 waves; 64; 128)
    M("seg mfma D=16", 16, 7, 37, 23, 61, "seg mfma 256", ONE),
    M("seg mfma D=48 four-kernel sort", 48, 9, 300, 23, 61, "seg mfma 256", FOUR),       # 18 300 slots > 16 384
    M("seg mfma D=80 half the types unused", 80, 12, 60, 30, 70, "seg mfma 1024 spw=1", ONE, graph="half_types"),
    M("seg mfma D=96 dup4", 96, 6, 50, 30, 80, "seg mfma 1024 spw=1", ONE, graph="dup4"),
    M("seg mfma D=112 oor", 112, 12, 40, 30, 70, "seg mfma 1024 spw=1", ONE, graph="oor"),
    # --- spw = 2 from max_segs >= 2048 (B * E = 131 136 slots, small N)
    M("seg mfma D=64", 64, 9, 50, 30, 70, "seg mfma 1024 spw=1", ONE),
    M("seg mfma D=128 one type", 128, 12, 60, 30, 70, "seg mfma 1024 spw=1", ONE, graph="one_type"),
    M("seg mfma D=128 star four-kernel sort", 128, 6, 90, 30, 200, "seg mfma 1024 spw=1", FOUR, graph="star"),
    M("seg mfma D=64 spw=2", 64, 5, 2049, 5, 64, "seg mfma 1024 spw=2", FOUR),
    M("seg mfma D=64 Vb=1025", 64, 1025, 30, 20, 50, "seg mfma 1024 spw=1", FOUR),       # Vb > 1024: four kernels
    # --- bmm_message_typed_seg_kernel: D = 8, 24, 40 and misaligned operands at matrix-core widths
    M("seg valu D=8", 8, 7, 37, 23, 61, "seg valu", ONE),
    M("seg valu D=24 four-kernel sort oor", 24, 5, 300, 17, 61, "seg valu", FOUR, graph="oor"),
    M("seg valu D=40 star", 40, 6, 40, 30, 200, "seg valu", ONE, graph="star"),
    M("seg valu D=64 h off by one float", 64, 9, 60, 30, 70, "seg valu", ONE, misalign="h"),
    M("seg valu D=128 matrices off by one float", 128, 9, 60, 30, 70, "seg valu", ONE, misalign="A"),
    # --- sort_ready | zero_rows_ready: two layers' calls on one IonGraph and its one message buffer
    M("flags D=64", 64, 9, 120, 30, 70, "seg mfma 1024 spw=1", ONE, flags=True),
    M("flags D=16 four-kernel sort half the types unused", 16, 12, 300, 30, 70, "seg mfma 256", FOUR, graph="half_types",
      flags=True),
    M("flags D=40 oor", 40, 12, 60, 30, 70, "seg valu", ONE, graph="oor", flags=True),
    # --- the generic kernel beyond the sorted entry's widths, and no edge slot at all
    M("generic D=144", 144, 6, 5, 20, 30, "generic", NONE),
    M("E=0", 64, 5, 7, 20, 0, "no launch", NONE),
    M("E=0 D=32", 32, 5, 7, 20, 0, "no launch", NONE),
]


def message_cases():
    return MESSAGE_CASES


def message_inputs(c):
    """h, type matrices A scaled by 1/sqrt(D) and - the second layer's call of a ``flags`` case - h2, A2."""
    rng = np.random.default_rng(5000 + MESSAGE_CASES.index(c))
    conn, bond = make_graph(c.graph, c.B, c.N, c.E, c.Vb, rng)
    s = np.float32(1.0 / np.sqrt(c.D))
    return {"conn": conn, "bond": bond, "h": _f32(rng, c.B, c.N, c.D), "A": _f32(rng, c.Vb, c.D, c.D) * s,
            "h2": _f32(rng, c.B, c.N, c.D), "A2": _f32(rng, c.Vb, c.D, c.D) * s}


def message_reference(h, A, bond, conn, dtype):
    """(B,E,D) messages in ``dtype``: the oracle's BondMatrixMessage on a one-hot bond state (an id outside [0, Vb) is a
    zero state: the edge carries nothing) while its (B,E,D,D) tensor fits, grad_ref's per-type step beyond."""
    (B, N, D), E, Vb = h.shape, conn.shape[1], A.shape[0]
    if B * E * (D * D + Vb) <= ORACLE_MAX_ELEMS:
        onehot = (bond[..., None] == np.arange(Vb, dtype=bond.dtype)).astype(dtype)
        return O.bond_matrix_message(h.astype(dtype), onehot, conn, A.astype(dtype))
    t = torch.float64 if dtype == np.float64 else torch.float32
    return GR.messages_from_matrices(torch.tensor(h, dtype=t), torch.tensor(A, dtype=t), bond, conn).numpy()


def check_messages(c, m, ref, bond, conn):
    """The whole tensor at 1e-5; with few types every type's messages on their own (a rare type must not hide under
    the busiest one); rows of masked edges exactly zero."""
    m = np.asarray(m)
    assert_close(m, ref, TOL, f"{c.name}: messages", FLOOR)
    valid = GR.valid_edges(bond, conn, c.Vb).numpy()
    if c.Vb <= 72:
        for v in range(c.Vb):
            sel = valid & (bond == v)
            assert_close(m[sel], ref[sel], TOL, f"{c.name}: messages of type {v}", FLOOR)
    assert not m[~valid].any(), f"{c.name}: a masked edge's row is not exactly zero"


@pytest.mark.parametrize("c", MESSAGE_CASES, ids=[c.name for c in MESSAGE_CASES])
def test_typed_message_fuzz(c):
    """ops.bmm_message_typed on the branch the row names against fp64.  ``flags``: layer one's call sorts into the
    IonGraph and writes the zero rows of its message buffer, layer two's call (other states, other matrices) comes with
    sort_ready | zero_rows_ready and must find both as they were left."""
    assert message_branch(c) == (c.kernel, c.sort)
    inp = message_inputs(c)
    bond, conn = inp["bond"], inp["conn"]
    h, A = _dev(inp["h"], c.misalign == "h"), _dev(inp["A"], c.misalign == "A")
    bg, cg = _dev(bond), _dev(conn)
    if c.E == 0:
        assert tuple(ops.bmm_message_typed(h, bg, cg, A).shape) == (c.B, 0, c.D)
        return
    ref = message_reference(inp["h"], inp["A"], bond, conn, np.float64)
    if not c.flags:
        check_messages(c, ops.bmm_message_typed(h, bg, cg, A).cpu().numpy(), ref, bond, conn)
        return
    graph = ops.IonGraph(None, bg, cg, c.Vb)
    out = graph.message_buffer(c.D)
    assert out[1] is False
    m1 = ops.bmm_message_typed(h, bg, cg, A, graph, out=out)
    check_messages(c, m1.cpu().numpy(), ref, bond, conn)
    buf, zero_rows_ready = graph.message_buffer(c.D)
    assert zero_rows_ready and buf is m1 and graph.edge_sort()[1]
    m2 = ops.bmm_message_typed(_dev(inp["h2"]), bg, cg, _dev(inp["A2"]), graph, out=(buf, True))
    assert m2 is buf
    check_messages(c, m2.cpu().numpy(), message_reference(inp["h2"], inp["A2"], bond, conn, np.float64), bond, conn)


# =====================================================================================================================
# bond_type_matrices (launch_bond_type_matrices)
# =====================================================================================================================
TM_GEMM_MIN_K = 64           # K >= 64: GEMM-shaped
TM_MFMA_MAX_VB = 128         # bond_type_matrices_mfma_kernel<8>: eight 16-row tiles of the vocabulary

TmCase = namedtuple("TmCase", "name Vb K D branch misalign")


def T(name, Vb, K, D, branch, misalign=False):
    return TmCase(name, Vb, K, D, branch, misalign)


def type_matrices_branch(c):
    if c.K < TM_GEMM_MIN_K:
        return "valu"
    if c.K % 64 == 0 and (c.D * c.D) % 16 == 0 and 1 <= c.Vb <= TM_MFMA_MAX_VB and not c.misalign:
        vt = ceil_div(c.Vb, 16)
        return "mfma<2>" if vt <= 2 else "mfma<5>" if vt <= 5 else "mfma<8>"
    return "strided gemm"


TYPE_MATRIX_CASES = [
    T("valu K=8", 7, 8, 32, "valu"),
    T("valu K=63", 72, 63, 8, "valu"),
    T("valu D=5", 3, 2, 5, "valu"),
    T("mfma<2> Vb=17", 17, 64, 8, "mfma<2>"),
    T("mfma<2> Vb=1", 1, 128, 8, "mfma<2>"),
    T("mfma<2> Vb=32", 32, 64, 12, "mfma<2>"),
    T("mfma<5> Vb=33", 33, 128, 12, "mfma<5>"),
    T("mfma<5> Vb=72 K=256", 72, 256, 16, "mfma<5>"),
    T("mfma<5> Vb=80", 80, 64, 8, "mfma<5>"),
    T("mfma<8> Vb=81", 81, 64, 8, "mfma<8>"),
    T("mfma<8> Vb=127", 127, 192, 8, "mfma<8>"),
    T("mfma<8> Vb=128", 128, 64, 8, "mfma<8>"),
    T("gemm K=65", 20, 65, 8, "strided gemm"),
    T("gemm K=100", 70, 100, 12, "strided gemm"),
    T("gemm D*D=36", 20, 64, 6, "strided gemm"),
    T("gemm Vb=129", 129, 64, 8, "strided gemm"),
    T("gemm table off by one float", 40, 64, 8, "strided gemm", misalign=True),
]


def type_matrices_cases():
    return TYPE_MATRIX_CASES


def type_matrices_inputs(c):
    rng = np.random.default_rng(6000 + TYPE_MATRIX_CASES.index(c))
    return {"table": _f32(rng, c.Vb, c.K), "W": _f32(rng, c.K, c.D, c.D) * np.float32(1.0 / np.sqrt(c.D * c.K))}


def type_matrices_reference(inp, dtype):
    return np.tensordot(inp["table"].astype(dtype), inp["W"].astype(dtype), axes=[[1], [0]])   # models/layers.py:108


def check_type_matrices(c, got, ref):
    assert_close(got, ref, TOL, f"{c.name}: type matrices", FLOOR)


@pytest.mark.parametrize("c", TYPE_MATRIX_CASES, ids=[c.name for c in TYPE_MATRIX_CASES])
def test_bond_type_matrices_fuzz(c):
    assert type_matrices_branch(c) == c.branch
    inp = type_matrices_inputs(c)
    got = ops.bond_type_matrices(_dev(inp["table"], c.misalign), _dev(inp["W"]))
    check_type_matrices(c, got.cpu().numpy(), type_matrices_reference(inp, np.float64))


# =====================================================================================================================
# reduce_scatter_add (launch_reduce_scatter_add)
# =====================================================================================================================
K_RS_P = 8                        # kRsP: thread groups per column of reduce_scatter_small_kernel
RS_SMALL_MAX_B = 2048             # batches below take the small kernel ...
RS_SMALL_MAX_D = 128              # ... up to this width ...
RS_SMALL_LDS = 64 * KIB           # ... while a molecule's sums and edge lists fit
RS_MIN_THREADS = 131072           # row ranges (gridDim.y) until the launch has this many threads
RS_RANGE_LDS = 64 * KIB           # and until a workgroup's accumulators fit
RS_LIST_MAX_BYTES = 32 * KIB      # the compacted slot lists of a workgroup's molecules

RsCase = namedtuple("RsCase", "name B N E D branch")


def reduce_branch(c):
    if c.B < RS_SMALL_MAX_B and c.D <= RS_SMALL_MAX_D and 0 < c.E < 65536 and c.N < 65536:
        P = min(K_BLOCK // c.D, K_RS_P)
        if P >= 2 and 4 * c.N * c.D + 2 * (P * c.E + c.E) <= RS_SMALL_LDS:
            return f"small P={P}"
    cols = min(c.D, K_BLOCK)
    mpb = K_BLOCK // cols
    K, threads = 1, c.B * cols
    if threads < RS_MIN_THREADS:
        K = ceil_div(RS_MIN_THREADS, threads)
    while mpb * ceil_div(c.N, K) * c.D * 4 > RS_RANGE_LDS and ceil_div(c.N, K) > 8:
        K += 1
    K = min(K, 16)
    if K > c.N // 8:
        K = max(c.N // 8, 1)
    rows_per = ceil_div(c.N, K)
    K = ceil_div(c.N, rows_per)
    lds = mpb * rows_per * c.D * 4
    use_lds = lds <= LDS_MAX
    lbytes = 4 * (mpb * c.E + mpb)
    use_list = (cols == c.D and 0 < c.E < 65536 and c.N < 65536 and lbytes <= RS_LIST_MAX_BYTES
                and (lds if use_lds else 0) + lbytes <= LDS_MAX)
    form = "list" if use_list else "walk" if cols == c.D else "cols<D"
    ranges = "one range" if K == 1 else "ranges ragged" if c.N % rows_per else "ranges"
    return f"large {form}, {ranges}" + ("" if use_lds else ", sums in global memory")


REDUCE_CASES = [
    RsCase("small D=16", 37, 33, 77, 16, "small P=8"),
    RsCase("small D=48", 20, 21, 90, 48, "small P=5"),
    RsCase("small D=64 E=300", 9, 20, 300, 64, "small P=4"),
    RsCase("small D=100", 11, 17, 70, 100, "small P=2"),
    RsCase("small D=128 E=513", 5, 9, 513, 128, "small P=2"),
    RsCase("D=64 N=300: past the 64 KiB of the small kernel", 5, 300, 50, 64, "large list, ranges ragged"),
    RsCase("D=136 > 128 at a small batch", 3, 20, 30, 136, "large list, ranges"),
    RsCase("D=8 E=300 B=2050: lists past 32 KiB", 2050, 10, 300, 8, "large walk, one range"),
    RsCase("D=32 E=1100 N=400: lists past 32 KiB", 3, 400, 1100, 32, "large walk, ranges"),
    RsCase("D=32 B=4100: one range", 4100, 12, 30, 32, "large list, one range"),
    RsCase("D=256 N=2600: sums past 160 KiB", 2, 2600, 40, 256, "large list, ranges ragged, sums in global memory"),
    RsCase("D=300 > 256", 2, 20, 30, 300, "large cols<D, ranges"),
    RsCase("D=300 N=37", 3, 37, 45, 300, "large cols<D, ranges ragged"),
]


def reduce_cases():
    return REDUCE_CASES


def reduce_inputs(c):
    """Targets over the rows, a tenth of them 0 (padding), negative or >= N (skipped), with a crowded row 3; odd cases
    hand the targets over as the strided view conn[:, :, 1]."""
    i = REDUCE_CASES.index(c)
    rng = np.random.default_rng(7000 + i)
    tgt = rng.integers(1, c.N, size=(c.B, c.E)).astype(np.int32)
    tgt[:, rng.integers(0, c.E, size=c.E // 3)] = 3
    out = rng.random((c.B, c.E)) < 0.1
    tgt[out] = rng.choice(np.array([0, 0, -1, c.N, c.N + 1], np.int32), size=int(out.sum()))
    tgt[-1, 1:5] = (0, -1, c.N, c.N + 1)   # (every kind in every case, the smallest included)
    return {"m": _f32(rng, c.B, c.E, c.D), "tgt": tgt, "strided": i % 2 == 1}


def reduce_reference(inp, N):
    """The sequential f32 scatter in edge-slot order (np.add.at walks its updates in order)."""
    m, tgt = inp["m"], inp["tgt"]
    B, E, D = m.shape
    ok = (tgt > 0) & (tgt < N)
    b = np.broadcast_to(np.arange(B)[:, None], (B, E))
    out = np.zeros((B, N, D), np.float32)
    np.add.at(out, (b[ok], tgt[ok]), m[ok])
    return out


def check_reduce(c, got, ref):
    np.testing.assert_array_equal(got, ref, err_msg=f"{c.name}: not the sequential scatter bit for bit")


@pytest.mark.parametrize("c", REDUCE_CASES, ids=[c.name for c in REDUCE_CASES])
def test_reduce_scatter_add_fuzz(c):
    assert reduce_branch(c) == c.branch
    inp = reduce_inputs(c)
    tgt = _dev(inp["tgt"])
    if inp["strided"]:
        tgt = torch.stack([torch.zeros_like(tgt), tgt], dim=-1)[:, :, 1]
        assert not tgt.is_contiguous() or c.B * c.E <= 1
    got = ops.reduce_scatter_add(_dev(inp["m"]), tgt, c.N)
    check_reduce(c, got.cpu().numpy(), reduce_reference(inp, c.N))


# =====================================================================================================================
# bmm_message / bmm_fused with a dense bond state (launch_bmm_message)
# =====================================================================================================================
DmCase = namedtuple("DmCase", "name op B N E D K branch")


def dense_message_branch(c):
    hbytes, mbytes = 4 * c.N * c.D, (4 * c.E * c.D if c.op == "fused" else 0)
    assert mbytes <= LDS_MAX
    return "h in lds" if hbytes + mbytes <= LDS_MAX else "h in global memory"


DENSE_MESSAGE_CASES = [
    DmCase("message", "message", 6, 40, 80, 32, 8, "h in lds"),
    DmCase("message N*D = 160 KiB", "message", 2, 640, 20, 64, 3, "h in lds"),
    DmCase("message N*D past 160 KiB", "message", 2, 700, 20, 64, 3, "h in global memory"),
    DmCase("fused", "fused", 5, 9, 30, 48, 2, "h in lds"),
    DmCase("fused (N + E) * D = 160 KiB", "fused", 2, 600, 40, 64, 3, "h in lds"),
    DmCase("fused (N + E) * D past 160 KiB", "fused", 2, 600, 41, 64, 3, "h in global memory"),
]


def dense_message_cases():
    return DENSE_MESSAGE_CASES


def dense_message_inputs(c):
    rng = np.random.default_rng(8000 + DENSE_MESSAGE_CASES.index(c))
    conn = rng.integers(0, c.N, size=(c.B, c.E, 2)).astype(np.int32)
    return {"h": _f32(rng, c.B, c.N, c.D), "bs": _f32(rng, c.B, c.E, c.K), "conn": conn,
            "W": _f32(rng, c.K, c.D, c.D) * np.float32(1.0 / np.sqrt(c.D * c.K))}


def dense_message_reference(c, inp, dtype):
    m = O.bond_matrix_message(inp["h"].astype(dtype), inp["bs"].astype(dtype), inp["conn"], inp["W"].astype(dtype))
    return m if c.op == "message" else O.reduce_messages(m, inp["conn"][:, :, 1], inp["h"])


def check_dense_message(c, got, ref, conn):
    assert_close(got, ref, TOL, f"{c.name}: {c.op}", FLOOR)
    if c.op == "message":
        assert not np.asarray(got)[~((conn[..., 0] > 0) & (conn[..., 1] > 0))].any(), f"{c.name}: masked rows not zero"


@pytest.mark.parametrize("c", DENSE_MESSAGE_CASES, ids=[c.name for c in DENSE_MESSAGE_CASES])
def test_dense_message_fuzz(c):
    assert dense_message_branch(c) == c.branch
    inp = dense_message_inputs(c)
    fn = ops.bmm_message if c.op == "message" else ops.bmm_fused
    got = fn(_dev(inp["h"]), _dev(inp["bs"]), _dev(inp["conn"]), _dev(inp["W"]))
    check_dense_message(c, got.cpu().numpy(), dense_message_reference(c, inp, np.float64), inp["conn"])


# =====================================================================================================================
# embed_gather (launch_embed_gather) and global_sum_pool (launch_global_sum_pool)
# =====================================================================================================================
EgCase = namedtuple("EgCase", "name rows vocab dim branch misalign")


def embed_branch(c):
    vec = 4 if c.dim % 4 == 0 and not c.misalign else 1
    return f"embed_gather<{vec}>" + (" grid-stride" if c.rows * (c.dim // vec) > GRID_CAP_ITEMS else "")


EMBED_CASES = [
    EgCase("dim=32", 333, 50, 32, "embed_gather<4>", False),
    EgCase("dim=6", 333, 50, 6, "embed_gather<1>", False),
    EgCase("dim=8 table off by one float", 333, 50, 8, "embed_gather<1>", True),
    EgCase("dim=32 past the grid cap", 65536 + 3, 50, 32, "embed_gather<4> grid-stride", False),
    EgCase("dim=6 past the grid cap", 87400, 50, 6, "embed_gather<1> grid-stride", False),
]


def embed_cases():
    return EMBED_CASES


def embed_inputs(c):
    """A twentieth of the ids outside [0, vocab): zero rows (the kernel's rule)."""
    rng = np.random.default_rng(9000 + EMBED_CASES.index(c))
    ids = rng.integers(0, c.vocab, size=c.rows).astype(np.int32)
    bad = rng.random(c.rows) < 0.05
    ids[bad] = rng.choice(np.array([-1, c.vocab, c.vocab + 9], np.int32), size=int(bad.sum()))
    return {"ids": ids, "table": _f32(rng, c.vocab, c.dim)}


def embed_reference(inp):
    ids, table = inp["ids"], inp["table"]
    ok = (ids >= 0) & (ids < table.shape[0])
    return np.where(ok[:, None], table[np.where(ok, ids, 0)], np.float32(0))


def check_embed(c, got, ref):
    np.testing.assert_array_equal(got, ref, err_msg=f"{c.name}: not the table's rows bit for bit")


@pytest.mark.parametrize("c", EMBED_CASES, ids=[c.name for c in EMBED_CASES])
def test_embed_gather_fuzz(c):
    assert embed_branch(c) == c.branch
    inp = embed_inputs(c)
    got = ops.embed_gather(_dev(inp["ids"]), _dev(inp["table"], c.misalign))
    check_embed(c, got.cpu().numpy(), embed_reference(inp))


PoolCase = namedtuple("PoolCase", "name B N D branch")


def pool_branch(c):
    return "global_sum_pool" + (" grid-stride" if c.B * c.D > GRID_CAP_ITEMS else "")


POOL_CASES = [
    PoolCase("N=11", 37, 11, 48, "global_sum_pool"),
    PoolCase("N=8", 5, 8, 32, "global_sum_pool"),
    PoolCase("past the grid cap", 4096 + 1, 3, 128, "global_sum_pool grid-stride"),
    PoolCase("past the grid cap N=19", 16384 + 5, 19, 32, "global_sum_pool grid-stride"),
]


def pool_cases():
    return POOL_CASES


def pool_inputs(c):
    rng = np.random.default_rng(9500 + POOL_CASES.index(c))
    return {"h": _f32(rng, c.B, c.N, c.D), "ids": rng.integers(0, 3, size=(c.B, c.N)).astype(np.int32)}


def pool_reference(inp, dtype):
    return O.global_sum_pool(inp["h"].astype(dtype), inp["ids"])


def check_pool(c, got, ref):
    assert_close(got, ref, TOL, f"{c.name}: pooled", FLOOR)


@pytest.mark.parametrize("c", POOL_CASES, ids=[c.name for c in POOL_CASES])
def test_global_sum_pool_fuzz(c):
    assert pool_branch(c) == c.branch
    inp = pool_inputs(c)
    got = ops.global_sum_pool(_dev(inp["h"]), _dev(inp["ids"]))
    check_pool(c, got.cpu().numpy(), pool_reference(inp, np.float64))
