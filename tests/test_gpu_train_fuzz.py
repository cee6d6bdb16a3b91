"""Gradient fuzz of the training path: every adjoint kernel and the whole differentiated model against fp64 on
arbitrary multigraphs ("Tests").

Reference: tests/grad_ref.py in fp64 - oracle/torch_ref.py with a message step of O(B E D) memory, so it reaches the
shapes at which the kernels switch branches.  Bounds are the project's existing ones, through conftest.assert_close
(per tensor AND per element, floor 0.3): 1e-4 for kernel gradients, 2e-4 for whole-model gradients, 1e-5 for the loss,
2e-6 for Adam.  tests/test_grad_ref_host.py walks every ``*_cases()`` of this module on the CPU and holds grad_ref in
fp32 to the same bounds against grad_ref in fp64: the bounds are attainable by a plain f32 implementation on exactly
these inputs.

How a case is mapped to a branch: the tables below name, per case, the branch it is meant for; ``message_branch``
restates the dispatch of launch_edge_type_sort / launch_bmm_message_typed_bwd (csrc/message_typed.hip) from the
shape, with the constants named, and every case asserts that the restatement gives the branch its row claims.  Whole
model seeds 0-7 sit exactly on the two thresholds of the training pass (autograd.MESSAGE_BWD_EDGE_BUFFER_MIN_SLOTS,
model.TRAIN_ROW_LIST_MIN_ROWS), one side per ion."""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, autograd, model as MM, ops, train, weights
from oracle import torch_ref as TR, train_oracle as TO
from conftest import assert_close

import grad_ref as GR
from test_dropout_host import reference_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRAD_TOL, MODEL_TOL, LOSS_TOL, ADAM_TOL, FLOOR = 1e-4, 2e-4, 1e-5, 2e-6, 0.3


def _np(t):
    return t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64)


# =====================================================================================================================
# Message + Reduce adjoint
# =====================================================================================================================
SORT_SMALL_MAX_SLOTS = 1024 * 16   # 1024 threads x kSortSmallPer: above it launch_edge_type_sort takes four kernels
SORT_SMALL_MAX_TYPES = 1024        # edge_type_sort_small_kernel scans one type per thread
BWD_MFMA_MAX_TYPES = 1024          # kBwdMfmaMaxTypes
VALU_SMALL_BLOCK, VALU_WIDE_BLOCK = 256, 1024   # kBlock below D = 64, 1024 threads from there

MsgCase = namedtuple("MsgCase", "name D Vb B N E entry sort kernel graph force misalign forward_first")


def M(name, D, Vb, B, N, E, entry, sort, kernel, graph="dense", force=None, misalign=None, forward_first=False):
    return MsgCase(name, D, Vb, B, N, E, entry, sort, kernel, graph, force, misalign, forward_first)


def message_branch(c):
    """(edge sort, adjoint kernel) the library takes for a case - the dispatch restated from the shape."""
    small = c.B * c.E <= SORT_SMALL_MAX_SLOTS and c.Vb <= SORT_SMALL_MAX_TYPES
    mfma = c.D in (64, 128) and c.Vb <= BWD_MFMA_MAX_TYPES and c.misalign is None and c.force != "valu"
    if mfma:
        return ("one workgroup" if small else "four kernels"), "mfma"
    block = VALU_WIDE_BLOCK if c.D >= 64 else VALU_SMALL_BLOCK
    acc = -(-c.D * c.D // block)                       # ACC = ceil(D*D / blockDim): LAUNCH(1 / 4 / 16 / 64)
    return ("one workgroup" if small else "four kernels"), "valu%d" % (1 if acc <= 1 else 4 if acc <= 4 else 16 if acc <= 16 else 64)


ONE, FOUR = "one workgroup", "four kernels"
MESSAGE_CASES = [
    # --- the VALU kernel's ACC instantiations (entries: "reduce" from_agg = 1, "bmm" from_agg = 0, "scratch" edge buffer)
    M("valu D=8", 8, 7, 37, 23, 61, "reduce", ONE, "valu1"),
    M("valu D=16", 16, 7, 37, 23, 61, "bmm", ONE, "valu1"),
    M("valu D=24", 24, 5, 20, 17, 50, "scratch", ONE, "valu4"),
    M("valu D=40", 40, 7, 37, 23, 61, "scratch", ONE, "valu16"),
    M("valu D=48", 48, 9, 37, 23, 61, "reduce", ONE, "valu16"),
    M("valu D=56", 56, 4, 300, 23, 61, "bmm", FOUR, "valu16"),                      # 18 300 slots > 16 384
    M("valu D=96", 96, 7, 37, 23, 61, "reduce", ONE, "valu16"),
    M("valu D=120", 120, 11, 37, 23, 61, "scratch", ONE, "valu16"),
    M("valu forced D=64", 64, 12, 90, 30, 70, "reduce", ONE, "valu4", force="valu"),
    M("valu forced D=128", 128, 6, 260, 30, 70, "scratch", FOUR, "valu16", force="valu"),  # 18 200 slots
    # --- the matrix-core kernel: D in {64, 128} x Vb in {1, 3, 72, 1024}; Vb = 1025 > kBwdMfmaMaxTypes falls to the VALU one
    M("mfma D=64 Vb=1", 64, 1, 50, 30, 70, "reduce", ONE, "mfma"),
    M("mfma D=128 Vb=1", 128, 1, 300, 24, 60, "scratch", FOUR, "mfma"),                # 18 000 slots
    M("mfma D=64 Vb=3", 64, 3, 300, 24, 60, "bmm", FOUR, "mfma"),
    M("mfma D=128 Vb=3", 128, 3, 50, 30, 70, "reduce", ONE, "mfma"),
    M("mfma D=64 Vb=72", 64, 72, 120, 40, 80, "scratch", ONE, "mfma"),
    M("mfma D=128 Vb=72", 128, 72, 250, 40, 80, "bmm", FOUR, "mfma"),                  # 20 000 slots
    M("mfma D=64 Vb=1024", 64, 1024, 250, 40, 80, "reduce", FOUR, "mfma"),
    M("mfma D=128 Vb=1024", 128, 1024, 100, 40, 80, "scratch", ONE, "mfma"),
    M("D=64 Vb=1025", 64, 1025, 60, 30, 70, "reduce", FOUR, "valu4"),                  # Vb > 1024: no one-workgroup sort either
    # --- sorted_ready = 1 on the sort (and the message buffer) a FORWARD message call of the same IonGraph made
    M("forward sort D=64", 64, 9, 120, 30, 70, "scratch", ONE, "mfma", forward_first=True),
    M("forward sort D=128", 128, 9, 250, 30, 70, "reduce", FOUR, "mfma", forward_first=True),
    M("forward sort D=48", 48, 9, 40, 30, 70, "bmm", ONE, "valu16", forward_first=True),
    # --- h or dm as a contiguous view one float into its allocation: not 16-byte aligned, the VALU kernel serves it
    M("h off by one float D=64", 64, 9, 60, 30, 70, "reduce", ONE, "valu4", misalign="h"),
    M("dm off by one float D=128", 128, 9, 60, 30, 70, "scratch", ONE, "valu16", misalign="dm"),
    M("h off by one float D=16", 16, 9, 60, 30, 70, "bmm", ONE, "valu1", misalign="h"),
    # --- shapes
    M("B=1", 64, 5, 1, 20, 50, "reduce", ONE, "mfma"),
    M("B=1 D=8", 8, 5, 1, 20, 50, "bmm", ONE, "valu1"),
    M("E=0", 64, 5, 7, 20, 0, "scratch", ONE, "mfma"),
    M("N=160 E=640 D=64", 64, 6, 6, 160, 640, "scratch", ONE, "mfma"),
    M("N=160 E=640 D=128", 128, 6, 30, 160, 640, "reduce", FOUR, "mfma"),              # 19 200 slots
    # --- graph content
    M("out-of-range bond ids D=64", 64, 12, 120, 30, 70, "scratch", ONE, "mfma", graph="oor"),
    M("out-of-range bond ids D=40", 40, 12, 300, 30, 70, "reduce", FOUR, "valu16", graph="oor"),
    M("one type owns every edge D=128", 128, 12, 120, 30, 70, "reduce", ONE, "mfma", graph="one_type"),
    M("one type owns every edge D=16", 16, 12, 300, 30, 70, "bmm", FOUR, "valu1", graph="one_type"),
    M("half the types unused D=64", 64, 12, 300, 30, 70, "bmm", FOUR, "mfma", graph="half_types"),
    M("half the types unused D=56", 56, 12, 60, 30, 70, "scratch", ONE, "valu16", graph="half_types"),
    M("in-degree E D=128", 128, 6, 40, 30, 200, "scratch", ONE, "mfma", graph="star"),
    M("in-degree E D=8", 8, 6, 40, 30, 200, "reduce", ONE, "valu1", graph="star"),
    M("4x duplicated edges D=64", 64, 6, 120, 30, 80, "reduce", ONE, "mfma", graph="dup4"),
    M("4x duplicated edges D=96", 96, 6, 120, 30, 80, "scratch", ONE, "valu16", graph="dup4"),
]


def message_cases():
    return MESSAGE_CASES


def make_graph(kind, B, N, E, Vb, rng):
    """conn (B,E,2), bond (B,E): an arbitrary dense multigraph (self loops, index 0 = masked edges) with ``kind``'s twist."""
    conn = rng.integers(0, N, size=(B, E, 2)).astype(np.int32)
    bond = rng.integers(0, Vb, size=(B, E)).astype(np.int32)
    if kind == "oor":          # a tenth of the bond ids outside [0, Vb): those edges carry nothing
        bad = rng.random((B, E)) < 0.1
        bond[bad] = rng.choice(np.array([-1, Vb, Vb + 7], np.int32), size=int(bad.sum()))
    elif kind == "one_type":
        bond[:] = Vb // 2
    elif kind == "half_types":  # types 0, 2, 4, ... and the last one own no edge
        used = np.arange(1, Vb - 1, 2, dtype=np.int32)
        bond = used[rng.integers(0, len(used), size=(B, E))]
    elif kind == "star":        # every edge of a molecule points at one atom
        conn[:, :, 1] = rng.integers(1, N, size=(B, 1))
    elif kind == "dup4":
        q = E // 4
        for r in range(1, 4):
            conn[:, r * q:(r + 1) * q] = conn[:, :q]
            bond[:, r * q:(r + 1) * q] = bond[:, :q]
    else:
        assert kind == "dense", kind
    return conn, bond


def message_inputs(c):
    rng = np.random.default_rng(7000 + MESSAGE_CASES.index(c))   # (the row's place in the table: the same on every machine)
    conn, bond = make_graph(c.graph, c.B, c.N, c.E, c.Vb, rng)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    g_shape = (c.B, c.N, c.D) if c.entry != "bmm" else (c.B, c.E, c.D)
    return {"conn": conn, "bond": bond, "h": f(c.B, c.N, c.D), "A": f(c.Vb, c.D, c.D) / np.float32(np.sqrt(c.D)),
            "g": f(*g_shape), "dh0": f(c.B, c.N, c.D), "dA0": f(c.Vb, c.D, c.D), "edge": f(c.B, c.E, c.D)}


def message_reference(c, inp, dtype):
    """(dh, dA) of sum(out * g) in ``dtype``; out = Reduce o message (from_agg) or the per-edge messages."""
    h = torch.tensor(inp["h"], dtype=dtype, requires_grad=True)
    A = torch.tensor(inp["A"], dtype=dtype, requires_grad=True)
    if c.entry == "bmm":
        out = GR.messages_from_matrices(h, A, inp["bond"], inp["conn"])
    else:
        out = GR.message_reduce_from_matrices(h, A, inp["bond"], inp["conn"], c.N)
    if out.requires_grad:
        (out * torch.tensor(inp["g"], dtype=dtype)).sum().backward()
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return z(h), z(A)


def check_message(c, dh, dA, ref_dh, ref_dA):
    """Both gradients at 1e-4, and - a rare type must not hide under the busiest one - every type's dA on its own."""
    assert_close(_np(dh), _np(ref_dh), GRAD_TOL, f"{c.name}: dh", FLOOR)
    assert_close(_np(dA), _np(ref_dA), GRAD_TOL, f"{c.name}: dA", FLOOR)
    if c.Vb <= 72:
        for v in range(c.Vb):
            assert_close(_np(dA[v]), _np(ref_dA[v]), GRAD_TOL, f"{c.name}: dA of type {v}", FLOOR)


def _dev(a, off_by_one=False):
    """A device copy; ``off_by_one``: a contiguous view that starts one float into its allocation."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not off_by_one:
        return t.to(DEV)
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("c", MESSAGE_CASES, ids=[c.name for c in MESSAGE_CASES])
def test_message_adjoint_fuzz(c):
    """impnn_message_reduce_typed_bwd, ..._bwd_scratch and impnn_bmm_message_typed_bwd against fp64: dh and dA ADDED
    into random contents, on the branch the row names; the edge-buffer form bitwise equal from run to run."""
    assert message_branch(c) == (c.sort, c.kernel), (c.name, message_branch(c))
    inp = message_inputs(c)
    ref_dh, ref_dA = message_reference(c, inp, torch.float64)
    lib = _lib.load()
    h, g = _dev(inp["h"], c.misalign == "h"), _dev(inp["g"], c.misalign == "dm")
    A, cg, bg = _dev(inp["A"]), _dev(inp["conn"]), _dev(inp["bond"])
    valid = GR.valid_edges(inp["bond"], inp["conn"], c.Vb).to(DEV)
    graph = ops.IonGraph(None, bg, cg, c.Vb)
    scratch = None
    if c.forward_first:
        with torch.no_grad():
            buf = graph.message_buffer(c.D)
            m = ops.bmm_message_typed(h, bg, cg, A, graph, out=buf)
        assert_close(_np(m), _np(GR.messages_from_matrices(torch.tensor(inp["h"], dtype=torch.float64),
                                                            torch.tensor(inp["A"], dtype=torch.float64),
                                                            inp["bond"], inp["conn"])), 1e-5, f"{c.name}: forward")
        if c.entry == "scratch":
            scratch = graph.written_message_buffer(c.D)
            assert scratch is m
    elif c.entry == "scratch":   # as a forward leaves it: anything at valid edges, zero rows elsewhere
        scratch = _dev(inp["edge"]) * valid[..., None]
    ws, ready = graph.edge_sort()
    assert ready == c.forward_first
    fn = {"reduce": lib.impnn_message_reduce_typed_bwd, "scratch": lib.impnn_message_reduce_typed_bwd_scratch,
          "bmm": lib.impnn_bmm_message_typed_bwd}[c.entry]

    def run(sorted_ready):
        dh, dA = _dev(inp["dh0"]), _dev(inp["dA0"])
        _lib.check(fn(ops.ptr(h), ops.ptr(bg), ops.ptr(cg), ops.ptr(A), ops.ptr(g), ops.ptr(dh), ops.ptr(dA), ops.ptr(ws),
                      ws.numel(), *(() if scratch is None else (ops.ptr(scratch),)), c.B, c.N, c.E, c.D, c.Vb,
                      1 if sorted_ready else 0, _lib.stream_ptr()))
        torch.cuda.synchronize()
        return dh, dA

    saved = os.environ.get("IMPNN_MESSAGE_BWD")
    try:
        if c.force:
            os.environ["IMPNN_MESSAGE_BWD"] = c.force
        dh, dA = run(ready)
        dh2, dA2 = run(True) if c.entry == "scratch" else (None, None)   # the sort and the buffer as they come back
    finally:
        if c.force:
            if saved is None:
                del os.environ["IMPNN_MESSAGE_BWD"]
            else:
                os.environ["IMPNN_MESSAGE_BWD"] = saved
    check_message(c, _np(dh) - inp["dh0"], _np(dA) - inp["dA0"], ref_dh, ref_dA)
    if dh2 is not None:
        assert torch.equal(dh, dh2), f"{c.name}: the edge-buffer form must give equal bits from run to run"
        check_message(c, _np(dh2) - inp["dh0"], _np(dA2) - inp["dA0"], ref_dh, ref_dA)
        if c.E and bool((~valid).any()):
            assert float(scratch[~valid].abs().max()) == 0.0, "masked edges' rows of the buffer stay zero"


# =====================================================================================================================
# GatedUpdate backward adding into the optimizer's flat gradient block
# =====================================================================================================================
GU_NAMES = ["Wz", "bz", "Wr", "br", "Wh", "bh", "gamma", "beta"]
GU_CASES = [(D, rows, kept) for D in (32, 64, 128) for rows in (1, 15, 16, 17, 127, 128, 129, 255, 257)
            for kept in (False, True)]


def gated_update_cases():
    return GU_CASES


def gated_update_inputs(D, rows, kept):
    rng = np.random.default_rng(1000 * D + 2 * rows + kept)
    f = lambda a: np.asarray(a, np.float32)
    s = 1.0 / np.sqrt(2 * D)
    vals = {"Wz": f(rng.normal(size=(2 * D, D)) * s), "bz": f(rng.normal(size=D) * 0.1),
            "Wr": f(rng.normal(size=(2 * D, D)) * s), "br": f(rng.normal(size=D) * 0.1),
            "Wh": f(rng.normal(size=(2 * D, D)) * s), "bh": f(rng.normal(size=D) * 0.1),
            "gamma": f(1 + 0.1 * rng.normal(size=D)), "beta": f(0.1 * rng.normal(size=D))}
    return {"p": vals, "h": f(rng.normal(size=(rows, D))), "agg": f(rng.normal(size=(rows, D))),
            "go": f(rng.normal(size=(rows, D))), "fill": f(rng.normal(size=6 * D * D + 5 * D))}


def gated_update_reference(inp, dtype):
    """{"out", "dh", "dagg", the eight parameter gradients} of sum(GatedUpdate(h, agg) * go) in ``dtype``."""
    p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in inp["p"].items()}
    h, agg = (torch.tensor(inp[k], dtype=dtype, requires_grad=True) for k in ("h", "agg"))
    out = TR.gated_update(h, agg, p)
    (out * torch.tensor(inp["go"], dtype=dtype)).sum().backward()
    return {"out": out.detach(), "dh": h.grad, "dagg": agg.grad, **{k: p[k].grad for k in GU_NAMES}}


def check_gated_update(what, got, ref):
    for k in ["dh", "dagg"] + GU_NAMES:     # every tensor on its own scale: a bias gradient is not hidden by a kernel's
        assert_close(_np(got[k]), _np(ref[k]), GRAD_TOL, f"{what}: {k}", FLOOR)


@pytest.mark.parametrize("D,rows,kept", GU_CASES)
def test_gated_update_backward_into_the_flat_gradient_block(D, rows, kept):
    """The eight .grad buffers laid out as train.Adam's flat block and pre-filled: the kernel takes the direct path
    (accumulate = 1, nothing handed back to autograd) and the block ends as fp64's gradients plus the pre-fill."""
    inp = gated_update_inputs(D, rows, kept)
    ref = gated_update_reference(inp, torch.float64)
    ps = [torch.tensor(inp["p"][k], device=DEV, requires_grad=True) for k in GU_NAMES]
    flat = torch.tensor(inp["fill"], device=DEV)
    assert flat.numel() == sum(t.numel() for t in ps)
    off = 0
    for t in ps:
        t.grad = flat[off:off + t.numel()].view_as(t)
        off += t.numel()
    h, agg, go = (torch.tensor(inp[k], device=DEV) for k in ("h", "agg", "go"))
    with torch.no_grad():
        saved = None
        if kept:
            out, saved = ops.gated_update(h, agg, *ps, 1e-3, save=True)
            assert_close(_np(out), _np(ref["out"]), 1e-5, "forward that keeps its activations")
        res = autograd._gated_update_backward((h, agg, *ps), 1e-3, go, None, saved)
    torch.cuda.synchronize()
    assert all(r is None for r in res[2:10]), "the parameter gradients went into the sinks"
    got = {"dh": res[0], "dagg": res[1]}
    off = 0
    for k, t in zip(GU_NAMES, ps):
        n = t.numel()
        got[k] = (_np(flat[off:off + n]) - inp["fill"][off:off + n].astype(np.float64)).reshape(tuple(t.shape))
        off += n
    check_gated_update(f"D={D} rows={rows} kept={kept}", got, ref)


# The main-kernel routes of the backward (choose_gu_bwd) that GU_CASES cannot reach: an atom_dim outside
# {32, 64, 128}, or a tensor that starts one float into its allocation.  The id names the expected route.
GuRoute = namedtuple("GuRoute", "name D rows misalign")
GU_ROUTE_CASES = [
    GuRoute("D=16 generic in-LDS", 16, 37, None),
    GuRoute("D=256 generic 1024-thread transposed", 256, 21, None),
    GuRoute("D=128 h off by one float: wide16 refused, 1024-thread transposed", 128, 75, "h"),
    GuRoute("D=64 agg off by one float: wide16 refused, generic in-LDS at 110 KB", 64, 33, "agg"),
    GuRoute("D=32 h off by one float: d32 refused, generic in-LDS", 32, 75, "h"),
]


@pytest.mark.parametrize("c", GU_ROUTE_CASES, ids=[c.name for c in GU_ROUTE_CASES])
def test_gated_update_backward_routes(c):
    """Plain backward (no row list, no kept activations), gradients handed back to the caller."""
    inp = gated_update_inputs(c.D, c.rows, False)
    ref = gated_update_reference(inp, torch.float64)
    ps = [_dev(inp["p"][k]) for k in GU_NAMES]
    h, agg = _dev(inp["h"], c.misalign == "h"), _dev(inp["agg"], c.misalign == "agg")
    with torch.no_grad():
        res = autograd._gated_update_backward((h, agg, *ps), 1e-3, _dev(inp["go"]))
    torch.cuda.synchronize()
    got = {"dh": res[0], "dagg": res[1], **dict(zip(GU_NAMES, res[2:10]))}
    check_gated_update(c.name, got, ref)


# =====================================================================================================================
# Adam
# =====================================================================================================================
ADAM_SIZES = [1, 3, 1023, 1025, 2 * 128 * 128, 8 * 128 * 128, 72 * 8]
ADAM_STEPS = 12
ADAM_NEAR = 3       # the variable whose gradient norm stays within 1e-3 of clipnorm, on both sides
ADAM_CASES = [(form, clip) for form in ("host step", "device step") for clip in (1.0, None)]


def adam_cases():
    return ADAM_CASES


def adam_inputs():
    """(initial weights, gradients per step): variables 0, 2, 5 clip (norm 3), 1, 4, 6 do not (norm 0.3), ADAM_NEAR sits on
    the edge; the flat block puts most variables at odd float offsets (the kernel's norm has a 16-byte path)."""
    rng = np.random.default_rng(12)
    ws = [rng.normal(size=n).astype(np.float32) for n in ADAM_SIZES]
    steps = []
    for t in range(ADAM_STEPS):
        gs = []
        for i, n in enumerate(ADAM_SIZES):
            g = rng.normal(size=n)
            norm = (1.0 + (5e-4 if t % 2 else -5e-4)) if i == ADAM_NEAR else 3.0 if i in (0, 2, 5) else 0.3
            g *= norm / np.sqrt((g * g).sum())
            gs.append(g.astype(np.float32))
        steps.append(gs)
    near = [float(np.sqrt((gs[ADAM_NEAR].astype(np.float64) ** 2).sum())) for gs in steps]
    assert all(abs(v - 1.0) < 1e-3 for v in near) and min(near) < 1.0 < max(near)
    return ws, steps


def adam_reference(ws, steps, clip):
    """[per step: the weights of every variable] from oracle/train_oracle.adam_step (fp64)."""
    state = [(w.astype(np.float64), np.zeros(w.shape), np.zeros(w.shape)) for w in ws]
    out = []
    for t, gs in enumerate(steps, 1):
        state = [TO.adam_step(w, g, m, v, t, clipnorm=clip) for (w, m, v), g in zip(state, gs)]
        out.append([s[0] for s in state])
    return out


def check_adam(what, got, ref):
    for i, (a, b) in enumerate(zip(got, ref)):
        assert_close(_np(a), b, ADAM_TOL, f"{what}: variable {i} ({ADAM_SIZES[i]} elements)", FLOOR)


@pytest.mark.parametrize("form,clip", ADAM_CASES)
def test_adam_fuzz(form, clip):
    """adam_clipnorm_kernel's (n_vars, kAdamSplit) grid on variables from 1 to 8*128*128 elements: every split piece of
    a variable must agree on the norm of the whole; the step from the host (impnn_adam_clipnorm_step) and from the
    device counter (impnn_adam_clipnorm_step_counted, what a captured step replays)."""
    ws, steps = adam_inputs()
    ref = adam_reference(ws, steps, clip)
    vars_ = [torch.tensor(w, device=DEV, requires_grad=True) for w in ws]
    opt = train.Adam(1e-3, clipnorm=clip)
    opt.build(vars_)
    import ctypes as C
    for t, gs in enumerate(steps, 1):
        for v, g in zip(vars_, gs):
            v.grad.copy_(torch.from_numpy(g))
        if form == "device step":
            opt.apply_gradients()
        else:
            _lib.check(_lib.load().impnn_adam_clipnorm_step(
                C.c_void_p(opt._table.data_ptr()), C.c_void_p(opt._sizes.data_ptr()), len(vars_), t, opt.learning_rate,
                opt.beta_1, opt.beta_2, opt.epsilon, clip if clip else 0.0, _lib.stream_ptr()))
        opt.zero_grad()
        check_adam(f"{form}, clipnorm {clip}, step {t}", vars_, ref[t - 1])
    if form == "device step":
        assert opt.iterations == ADAM_STEPS


# =====================================================================================================================
# Embedding and pool backward under contention
# =====================================================================================================================
# (D, vocabulary): launch_embed_gather_bwd sums in LDS while the table fits 64 KB (50 rows do at every D) and adds
# straight into the table with global float atomics beyond (200 rows of 128 floats: 100 KB) - both forms are run
EMBED_LDS_MAX_BYTES = 64 * 1024
EMBED_CASES = [(8, 50), (32, 50), (128, 50), (128, 200)]
EMBED_B, EMBED_N, EMBED_HOT = 4096, 40, 7


def embedding_cases():
    return EMBED_CASES


def embedding_form(D, V):
    """The form launch_embed_gather_bwd takes (its use_lds rule restated)."""
    return "lds" if 4 * V * D <= EMBED_LDS_MAX_BYTES and EMBED_B * EMBED_N >= 8 * V else "global atomics"


def embedding_inputs(D, V):
    """60 % of the 4096 * 40 rows carry id 0, 30 % id EMBED_HOT: two table rows take nine tenths of the float atomics."""
    rng = np.random.default_rng(D + V)
    u = rng.random((EMBED_B, EMBED_N))
    ids = np.where(u < 0.6, 0, np.where(u < 0.9, EMBED_HOT, rng.integers(0, V, size=u.shape))).astype(np.int32)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    return {"ids": ids, "table": f(V, D), "gp": f(EMBED_B, D), "gh": f(EMBED_B, EMBED_N, D)}


def embedding_reference(inp, dtype):
    """dtable of sum(pool(embed(ids)) * gp) + sum(embed(ids) * gh): the second term reaches the id-0 rows as well."""
    table = torch.tensor(inp["table"], dtype=dtype, requires_grad=True)
    ids = torch.tensor(inp["ids"])
    h = torch.nn.functional.embedding(ids.long(), table)
    p = TR.global_sum_pool(h, ids)
    ((p * torch.tensor(inp["gp"], dtype=dtype)).sum() + (h * torch.tensor(inp["gh"], dtype=dtype)).sum()).backward()
    return p.detach(), table.grad


def check_embedding(what, got, ref):
    assert_close(_np(got), _np(ref), GRAD_TOL, f"{what}: dtable", FLOOR)
    for row in (0, EMBED_HOT, 1):
        assert_close(_np(got[row]), _np(ref[row]), GRAD_TOL, f"{what}: dtable row {row}", FLOOR)


@pytest.mark.parametrize("D,V", EMBED_CASES)
def test_embedding_and_pool_backward_under_contention(D, V):
    """impnn_embed_gather_bwd behind impnn_global_sum_pool_bwd against fp64, in the LDS-accumulating form and - the last
    case - with global float atomics on two hot table rows."""
    assert embedding_form(D, V) == ("global atomics" if V == 200 else "lds")
    inp = embedding_inputs(D, V)
    pooled, dtable = embedding_reference(inp, torch.float64)
    table = torch.tensor(inp["table"], device=DEV, requires_grad=True)
    ids = torch.tensor(inp["ids"], device=DEV)
    h = ops.embed_gather(ids, table)
    p = ops.global_sum_pool(h, ids)
    assert_close(_np(p), _np(pooled), 1e-5, "pooled")
    ((p * torch.tensor(inp["gp"], device=DEV)).sum() + (h * torch.tensor(inp["gh"], device=DEV)).sum()).backward()
    torch.cuda.synchronize()
    check_embedding(f"D={D} V={V}", table.grad, dtable)


# =====================================================================================================================
# Whole model
# =====================================================================================================================
MODEL_SEEDS = list(range(32))
DROPOUT_SEED, DROPOUT_STEP, DROPOUT_RATE = 0xD0_5EED, 7, 0.2
EDGE_BUFFER_MIN, ROW_LIST_MIN = 8192, 4096   # asserted against the library's values in the GPU test

# seeds 0-7: D = 64 (0-3) and 128 (4-7); per variant (B, cation (N, E), anion (N, E)) - each ion on one side of
# MESSAGE_BWD_EDGE_BUFFER_MIN_SLOTS (B * E) and of TRAIN_ROW_LIST_MIN_ROWS (B * N), the exact values included
THRESHOLD_SHAPES = [
    (1, (97, 8191), (53, 8192)),      # no row list; edge buffer: one slot below / exactly at
    (64, (64, 128), (63, 127)),       # 4096 rows, 8192 slots: both exactly at | 4032 rows, 8128 slots: both below
    (63, (65, 131), (66, 129)),       # 4095 rows (below), 8253 slots (above) | 4158 rows (above), 8127 slots (below)
    (1, (4096, 8192), (4095, 8191)),  # one molecule: both exactly at | both one below
]
# (row list on?, edge buffer on?) of (cation, anion), per variant - what run_model_case asserts of the shapes above
THRESHOLD_SIDES = [((False, False), (False, True)), ((True, True), (False, False)), ((False, True), (True, False)),
                   ((True, True), (False, False))]


def model_cases():
    return MODEL_SEEDS


def _ion(rng, B, N, E, Va, Vb, single_atom=False):
    """atom ids (B,N), bond ids (B,E), conn (B,E,2) of a dense multigraph with holes: molecule b has ``real`` leading
    atoms (a sixth of them id 0 all the same: holes INSIDE the molecule that send and receive), its edges name indices
    below real + extra (extra in 0..2: holes past the last real atom, named by an edge), everything behind is padding
    that nothing names.  A tenth of the molecules are all padding, half of those with edges among the holes - but never
    molecule ``keep``, which (N > 1, E > 0) also gets a real atom at index 1 and one valid edge into it: every batch
    carries a gradient to the embeddings and the message layers, a batch of one included."""
    ids = rng.integers(1, max(Va, 2), size=(B, N)).astype(np.int32)
    real = rng.integers(1, N + 1, size=B)
    ids[np.arange(N)[None, :] >= real[:, None]] = 0
    ids[rng.random((B, N)) < 1.0 / 6.0] = 0
    lim = np.minimum(real + rng.integers(0, 3, size=B), N)
    conn = np.floor(rng.random((B, E, 2)) * lim[:, None, None]).astype(np.int32)
    bond = rng.integers(0, Vb, size=(B, E)).astype(np.int32)
    gone = rng.random(B) < 0.1
    keep = int(rng.integers(0, B))
    gone[keep] = False
    ids[gone] = 0
    conn[gone & (rng.random(B) < 0.5)] = 0
    ids[keep, 0] = max(int(ids[keep, 0]), 1)
    if N > 1 and E > 0:
        ids[keep, 1] = max(int(ids[keep, 1]), 1)
        conn[keep, int(rng.integers(0, E))] = (min(2, N - 1), 1)
    if single_atom:   # halide-like: one atom, no bond
        ids[:, 1:] = 0
        ids[:, 0] = np.maximum(ids[:, 0], 1)
        bond[:] = 0
        conn[:] = 0
    return ids, bond, conn


def model_case(seed):
    """Everything a seed decides, as numpy: the model's shape, its weights, the batch, what is frozen, dropout,
    whether the passes interleave."""
    rng = np.random.default_rng(50_000 + seed)
    c = {"seed": seed, "frozen": seed % 4 == 1, "dropout": seed in (2, 19) or (seed >= 32 and seed % 16 == 3),
         "interleaved": seed in (3, 6) or (seed >= 32 and seed % 16 == 6)}
    S = int(rng.integers(1, 4))
    Va, Vb = int(rng.integers(2, 60)), int(rng.integers(1, 40))
    if seed < 8:
        D, kind = (64 if seed < 4 else 128), "viscosity"
        B, cat, an = THRESHOLD_SHAPES[seed % 4]
        single = False
    else:
        D = (8, 16, 32, 64, 128)[seed % 5]
        kind = "melting_point" if D <= 16 and seed % 2 == 0 else "viscosity"
        B = int(rng.integers(1, 97))
        shape = lambda: (lambda n: (n, int(rng.integers(0, min(4 * n, 200) + 1))))(int(rng.integers(1, 61)))
        cat, an = shape(), shape()
        single = seed % 4 == 2 or seed in (11, 23)
        if seed == 13:
            cat = (cat[0], 0)          # an ion without a single edge slot
        if seed == 17:
            B = 1
        if seed == 21:
            an = (1, 5)                # one atom row: no edge can be valid
    K = D * D if kind == "melting_point" else int(rng.integers(1, 9))
    ca, cb, cc = _ion(rng, B, *cat, Va, Vb)
    aa, ab, ac = _ion(rng, B, *an, Va, Vb, single_atom=single)
    inputs = {"cat_atom": ca, "cat_bond": cb, "cat_connectivity": cc, "an_atom": aa, "an_bond": ab, "an_connectivity": ac}
    if kind == "viscosity":
        inputs["temperature"] = rng.uniform(280.0, 400.0, size=(B, 1)).astype(np.float32)
    frozen = []
    if c["frozen"]:   # the bond embedding and one GatedUpdate inside the trained range, then a random subset of the rest
        frozen = ["bond_embedding", f"{('cat', 'an')[int(rng.integers(0, 2))]}_gu_{int(rng.integers(0, S))}"]
        rest = [f"{p}_{what}_{i}" for p in ("cat", "an") for what in ("gu", "bmm") for i in range(S)] \
            + ["cat_fp", "an_fp", "cat_proj", "an_proj"]
        frozen += [n for n in rest if n not in frozen and rng.random() < 0.3]
    w = weights.init_weights(kind, Va, Vb, atom_dim=D, bond_dim=K, fp_size=12, mixing_size=10, num_steps=S, seed=seed,
                             perturb=True)
    if kind == "viscosity":
        # sum pools of up to thousands of atoms drive the head's pre-activations past 88, where the fp32 run of the
        # reference's own softplus, log1p(exp(x)), overflows (the attainability walk needs it finite): a smaller
        # kernel - smaller still where a molecule has more than 64 atom rows to pool - keeps them there finite and
        # still reaches both clip plateaus of B and C
        scale = 0.05 * min(1.0, 64.0 / max(cat[0], an[0]))
        w["visc_params/kernel"] = (w["visc_params/kernel"] * np.float32(scale)).astype(np.float32)
    c.update(kind=kind, D=D, K=K, S=S, Va=Va, Vb=Vb, B=B, cat=cat, an=an, single=single, inputs=inputs, frozen_layers=frozen,
             fp_l2=1e-4 if kind == "viscosity" else 1e-5, w=w,
             y=[rng.normal(1.0, 0.5, size=B).astype(np.float32) for _ in range(2 if c["interleaved"] else 1)])
    return c


def threshold_sides(c):
    return tuple((c["B"] * N >= ROW_LIST_MIN, c["B"] * E >= EDGE_BUFFER_MIN) for N, E in (c["cat"], c["an"]))


def model_reference(c, y, dtype):
    """(loss, {name: gradient}) of one training pass from tests/grad_ref.py; with dropout every GatedUpdate output goes
    through its layer's mask (cation step i: layer i, anion step i: S + i - the order of the calls)."""
    w = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in c["w"].items()}
    gu, calls = None, []
    if c["dropout"]:
        def gu(h, agg, p, eps=1e-3):
            k = len(calls)
            calls.append(k)
            B, N, D = h.shape
            m = reference_mask(DROPOUT_SEED, DROPOUT_STEP, ops.dropout_layer_word(k), DROPOUT_RATE, B * N, D)
            return TR.gated_update(h, agg, p, eps) * torch.tensor(m, dtype=h.dtype).view(B, N, D)
    loss = GR.model_loss(c["kind"], w, c["inputs"], y, c["fp_l2"], dtype, gu)
    loss.backward()
    assert not c["dropout"] or len(calls) == 2 * c["S"]
    return loss.detach(), {k: (torch.zeros_like(t) if t.grad is None else t.grad) for k, t in w.items()}


def assert_reference_is_alive(what, ref_grads):
    """A seed whose reference gradients vanish compares zeros with zeros: every seed must reach the atom embedding, the
    bond embedding and a message layer."""
    live = lambda n: float(ref_grads[n].abs().max()) > 0.0
    assert live("atom_embedding") and live("bond_embedding"), f"{what}: no gradient reaches the embeddings"
    assert any(live(n) for n in ref_grads if n.endswith("/bond_transform")), f"{what}: no gradient reaches a message layer"


def check_model(what, loss, grads, ref_loss, ref_grads):
    """The loss at 1e-5, every gradient ``grads`` holds at 2e-4 on its own scale, atom_embedding[0] (what the holes
    collect) on ITS own scale."""
    assert_close(np.array([float(loss)]), np.array([float(ref_loss)]), LOSS_TOL, f"{what}: loss", FLOOR)
    for name, g in grads.items():
        assert_close(_np(g), _np(ref_grads[name]), MODEL_TOL, f"{what}: grad {name}", FLOOR)
    if "atom_embedding" in grads:
        assert_close(_np(grads["atom_embedding"][0]), _np(ref_grads["atom_embedding"][0]), MODEL_TOL,
                     f"{what}: grad atom_embedding[0]", FLOOR)


def _layer_of(m, name):
    if name == "bond_embedding":
        return m.bond_emb
    p, what, *i = name.split("_")
    br = m.branches[p]
    return {"gu": br["update"], "bmm": br["bmm"]}[what][int(i[0])] if i else {"fp": br["fp"], "proj": getattr(m, f"{p}_proj")}[what]


def run_model_case(seed):
    c = model_case(seed)
    kw = dict(atom_dim=c["D"], fp_size=12, mixing_size=10, num_steps=c["S"], device=DEV)
    if c["dropout"]:
        kw.update(dropout_rate=DROPOUT_RATE, dropout_seed=DROPOUT_SEED)
    if c["kind"] == "viscosity":
        m = MM.build_model(c["Va"], c["Vb"], bond_dim=c["K"], **kw)
    else:
        m = MM.build_melting_point_model(c["Va"], c["Vb"], **kw)
    m.load_weights(c["w"])
    assert m.fp_l2 == c["fp_l2"]
    for name in c["frozen_layers"]:
        _layer_of(m, name).trainable = False
    d = m._to_device(c["inputs"])
    what = f"seed {seed} ({c['kind']} D={c['D']} K={c['K']} S={c['S']} B={c['B']} cat N,E={c['cat']} an N,E={c['an']})"
    if seed < 8:   # each ion on the side of each threshold its row of THRESHOLD_SHAPES names
        assert (autograd.MESSAGE_BWD_EDGE_BUFFER_MIN_SLOTS, MM.TRAIN_ROW_LIST_MIN_ROWS) == (EDGE_BUFFER_MIN, ROW_LIST_MIN)
        assert threshold_sides(c) == THRESHOLD_SIDES[seed % 4], what
    refs = [model_reference(c, y, torch.float64) for y in c["y"]]
    for _, rg in refs:
        assert_reference_is_alive(what, rg)
    if c["interleaved"]:   # forward A, forward B, backward B, backward A on the same input tensors; no gradient sinks
        names = [n for n, _ in m.trainable_variables()]
        params = [t.requires_grad_(True) for _, t in m.trainable_variables()]
        loss_a = m._loss(d, c["y"][0], training=True)
        loss_b = m._loss(d, c["y"][1], training=True)
        got_b = torch.autograd.grad(loss_b, params)
        got_a = torch.autograd.grad(loss_a, params)
        torch.cuda.synchronize()
        for tag, loss, got, (rl, rg) in (("pass A", loss_a, got_a, refs[0]), ("pass B", loss_b, got_b, refs[1])):
            check_model(f"{what} {tag}", loss, dict(zip(names, got)), rl, rg)
    else:
        m.compile(train.Adam(1e-3, clipnorm=1.0))
        if c["dropout"]:
            m.dropout_counter().fill_(DROPOUT_STEP)
        loss = m._loss(d, c["y"][0], training=True)
        loss.backward()
        m.join_training_streams()
        torch.cuda.synchronize()
        trainable = dict(m.trainable_variables())
        if c["frozen"]:
            assert "bond_embedding" not in trainable and len(trainable) < len(m._named_tensors())
        check_model(what, loss, {n: t.grad for n, t in trainable.items()}, *refs[0])
        for n, t in m._named_tensors().items():
            if n not in trainable:
                assert t.grad is None and not t.requires_grad, f"{what}: frozen {n} took a gradient"
                assert np.array_equal(t.detach().cpu().numpy(), c["w"][n]), f"{what}: frozen {n} changed"
    for k, t in d.items():
        assert not vars(t), f"{what}: input {k} carries {sorted(vars(t))}"
    return c


@pytest.mark.parametrize("seed", MODEL_SEEDS)
def test_training_gradients_fuzz(seed):
    """m._loss(..., training=True).backward() on random models and dense multigraphs with holes against fp64: the loss,
    every trainable variable's gradient, atom_embedding[0] on its own; frozen variables untouched; nothing of the
    library left on the input tensors."""
    run_model_case(seed)
