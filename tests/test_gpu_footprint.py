"""Footprints on the GPU: every C entry below runs through _lib.load() on buffers of EXACTLY the documented size, each
between two guards of one allocation (tests/footprint.py), and its workspace is exactly what its own query returns.

A case asserts, without a tolerance anywhere:
  a. the guards around every output, workspace, saved buffer and image are intact;
  b. every const input holds the bits it held before;
  c. the result does not depend on what the workspace held: body 0x00, body 0xFF (NaN as float, -1 as int) and the
     leftover of the same entry at a larger shape give the same bits.  Preconditions the header documents (the ZERO
     first word of the loss workspaces, sorted_ready, the (+=) buffers, a consumed saved buffer) are set up after the
     fill;
  d. the bits equal what the ops / autograd wrapper returns for the same inputs (that path is held against fp64 by the
     fuzz files).  Entries that accumulate with float atomics get inputs whose sums are exact in any order;
  e. with a size argument one unit below the query the call is refused with IMPNN_E_WORKSPACE and every buffer, 0xA5
     filled, is unchanged;
  f. the row-list forms leave the rows outside the list alone.

The shapes are the smallest at which the footprint arithmetic can go wrong: no multiple of a tile or an alignment.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, autograd, ops, train

import plan_cases as PC
from footprint import FILL, Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
E_WORKSPACE = -4
B, N, E, VB, K = 3, 7, 11, 5, 3      # the layer kernels' batch: nothing a multiple of anything
VA = 9
ROWS, LISTED = 37, 19                # the row-list forms: 37 rows, 19 of them listed
DIMS = (8, 32, 40, 64, 128)


# ---------------------------------------------------------------- one guarded call
class Run:
    """The buffers of one call of one entry.  inp(): a const operand (snapshot now, compared in finish()); out(): a
    written buffer of exactly nbytes between guards; work(): the same for a workspace, saved buffer or image, whose
    body takes this run's fill and whose content is no result; table(): a host array of device pointers."""

    def __init__(self, fill=0x00, track=False):
        self.track = track        # keep what every buffer held at its creation (a call that must be refused)
        self.fill, self.inputs, self.outs, self.works, self.keep = fill, [], {}, {}, []
        self.want = None          # () -> {output name: tensor of the wrapper}
        self.listed = {}          # output name -> bool mask over its bytes, True where the list lets it be written: f
        self.initial = {}

    def inp(self, name, array, dtype=None):
        t = array if isinstance(array, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(array))
        t = t.to(DEV).contiguous()
        if dtype is not None:
            t = t.to(dtype)
        self.inputs.append((name, t, t.clone()))
        return t

    def out(self, name, nbytes, fill=FILL, offset=0):
        g = self.outs[name] = Guarded(int(nbytes), fill, offset)
        self._keep_initial(name, g)
        return g.ptr

    def work(self, name, nbytes, offset=0):
        f = self.fill.get(name, 0xFF) if isinstance(self.fill, dict) else self.fill
        g = self.works[name] = Guarded(int(nbytes), f, offset)
        self._keep_initial(name, g)
        return g

    def table(self, items):
        arr = (C.c_void_p * len(items))(*[(i.value if isinstance(i, C.c_void_p) else
                                           (i.data_ptr() if isinstance(i, torch.Tensor) else i)) for i in items])
        self.keep.append(arr)
        return arr

    def settle(self, name):
        """The case has set up a documented precondition inside the buffer `name` after its fill."""
        self._keep_initial(name, {**self.outs, **self.works}[name])

    def _keep_initial(self, name, g):
        if self.track:
            self.initial[name] = g.host()[g.lo:g.lo + g.n].copy()

    def finish(self, refused=False):
        """-> {output name: its bytes}; a, b (and for a refused call: nothing changed at all)."""
        torch.cuda.synchronize()
        res = {n: g.body(np.uint8, n).copy() for n, g in self.outs.items()}
        for n, g in self.works.items():
            g.body(np.uint8, n)
        for n, t, snap in self.inputs:
            assert torch.equal(t.view(torch.uint8), snap.view(torch.uint8)), f"the input {n} was modified"
        if refused:
            for n, g in {**self.outs, **self.works}.items():
                g.unchanged(self.initial[n], f"{n} of a refused call")
        return res


def bits(t):
    return t.detach().contiguous().reshape(-1).cpu().numpy().view(np.uint8)


def compare(got, want, run, what):
    """d (and f): the bytes of every output `want` names against the wrapper's tensor."""
    for name, t in want.items():
        g, w = got[name], bits(t)
        assert g.size == w.size, f"{what}: {name} has {g.size} bytes, the wrapper returns {w.size}"
        if name in run.listed:
            mask = run.listed[name]
            assert np.array_equal(g[mask], w[mask]), f"{what}: the listed part of {name} differs from the wrapper's bits"
            assert (g[~mask] == FILL).all(), f"{what}: {name} was written outside the listed rows"
        else:
            diff = np.flatnonzero(g != w)
            assert diff.size == 0, f"{what}: {name} differs from the wrapper's bits in {diff.size} bytes, first {diff[0]}"


def check_case(fn, p, big=None, sizes=(), refusal=E_WORKSPACE):
    """fn(run, p, short) -> status: runs one case at shape `p` under every fill and checks a - f.  big: a larger shape
    whose leftover workspace is the third fill.  sizes: the names of its size arguments (short=name passes one less)."""
    lib = _lib.load()
    fills = [0x00]
    probe = Run(0xFF)
    rc = fn(probe, p, None)
    assert rc == 0, (rc, lib.impnn_last_error_string().decode())
    results = [(0xFF, probe, probe.finish())]
    if probe.works:
        if big is not None:
            rb = Run(0xFF)
            rc = fn(rb, big, None)
            assert rc == 0, ("the larger shape", rc, lib.impnn_last_error_string().decode())
            rb.finish()
            fills.append({n: g.view().clone() for n, g in rb.works.items()})
        for f in fills:
            r = Run(f)
            rc = fn(r, p, None)
            assert rc == 0, (rc, lib.impnn_last_error_string().decode())
            results.append(("leftover" if isinstance(f, dict) else f, r, r.finish()))
    else:
        assert big is None, "a case without a workspace has no fill to vary"
    first = results[0][2]
    for f, _, res in results[1:]:
        for name in first:
            assert np.array_equal(first[name], res[name]), \
                f"{fn.__name__}{p}: {name} depends on what the workspace held (0xFF against {f})"
    assert probe.want is not None, "every case names the wrapper's result"
    compare(first, probe.want(), probe, f"{fn.__name__}{p}")
    for name in sizes:
        r = Run(FILL, track=True)
        rc = fn(r, p, name)
        assert rc == refusal, f"{fn.__name__}{p}: {name} one below the query returned {rc}, not {refusal}"
        r.finish(refused=True)


# ---------------------------------------------------------------- inputs
def rng_of(*key):
    return np.random.default_rng([int(k) for k in key])


def normal(rng, *shape, scale=1.0):
    return (rng.normal(size=shape) * scale).astype(np.float32)


def exact(rng, *shape):
    """Small integers times a power of two: every product of two of them and every sum of a few thousand such
    products is exact in float32 in any order."""
    return (rng.integers(-4, 5, size=shape) * 0.125).astype(np.float32)


def assert_exact(ref64, terms_abs_sum, unit):
    """The fp64 result is a float32, and no partial sum of the terms can round: every term is a multiple of `unit` and
    the sum of their magnitudes stays below 2^24 units."""
    assert np.array_equal(ref64.astype(np.float32).astype(np.float64), ref64)
    assert np.all(np.abs(ref64 / unit - np.round(ref64 / unit)) == 0)
    assert np.max(terms_abs_sum) / unit < 2 ** 24


def graph(rng, b=B, n=N, e=E, vb=VB):
    """atom_ids (b,n) with padding tails and an id outside the vocabulary, bond_ids (b,e) with ids outside [0,vb), conn
    (b,e,2) with masked edges (index 0), self loops and indices outside [0,n): the header's 'never trusted' rule."""
    atom = rng.integers(1, VA, size=(b, n)).astype(np.int32)
    for i in range(b):
        atom[i, rng.integers(1, n + 1):] = 0
    bond = rng.integers(0, vb, size=(b, e)).astype(np.int32)
    conn = rng.integers(0, n, size=(b, e, 2)).astype(np.int32)
    if e >= 4:
        bond[0, 1], bond[-1, 2] = vb, -1
        conn[0, 0], conn[-1, 3] = (n, 1), (1, -1)
    return atom, bond, conn


def gu_params(rng, D):
    s = np.float32(1.0 / np.sqrt(2 * D))
    return [normal(rng, 2 * D, D, scale=s), normal(rng, D, scale=0.1), normal(rng, 2 * D, D, scale=s),
            normal(rng, D, scale=0.1), normal(rng, 2 * D, D, scale=s), normal(rng, D, scale=0.1),
            (1.0 + normal(rng, D, scale=0.1)).astype(np.float32), normal(rng, D, scale=0.1)]


def row_mask(rows, row_bytes, total_rows=ROWS):
    """bool mask over the bytes of a (total_rows, row_bytes) buffer: True in `rows`."""
    m = np.zeros((total_rows, row_bytes), bool)
    m[rows] = True
    return m.reshape(-1)


def row_list(rng, rows=ROWS, listed=LISTED):
    """row_index (rows,) int32: `listed` distinct rows first, the unlisted ones behind them (a kernel that ran past
    *n_rows would write a row whose sentinel the case checks), and n_rows (1,) = listed."""
    perm = rng.permutation(rows).astype(np.int32)
    return perm, np.array([listed], np.int32)


S = lambda: _lib.stream_ptr()
P = _lib.ptr


# ---------------------------------------------------------------- the layer kernels (forward)
def embed_gather(r, D, short):
    rng = rng_of(1, D)
    ids = rng.integers(-1, VA + 1, size=(B, N)).astype(np.int32)
    ids_d, tab = r.inp("ids", ids), r.inp("table", normal(rng, VA, D))
    r.want = lambda: {"out": ops.embed_gather(ids_d, tab)}
    return _lib.load().impnn_embed_gather(P(ids_d), P(tab), r.out("out", B * N * D * 4), B * N, VA, D, S())


def bmm_message(r, D, short):
    rng = rng_of(2, D)
    _, _, conn = graph(rng)
    h, bs, cn, W = (r.inp("h", normal(rng, B, N, D)), r.inp("bond_state", normal(rng, B, E, K)), r.inp("conn", conn),
                    r.inp("W", normal(rng, K, D, D, scale=D ** -0.5)))
    r.want = lambda: {"messages": ops.bmm_message(h, bs, cn, W)}
    return _lib.load().impnn_bmm_message(P(h), P(bs), P(cn), P(W), r.out("messages", B * E * D * 4), B, N, E, D, K, S())


def bmm_fused(r, D, short):
    rng = rng_of(3, D)
    _, _, conn = graph(rng)
    h, bs, cn, W = (r.inp("h", normal(rng, B, N, D)), r.inp("bond_state", normal(rng, B, E, K)), r.inp("conn", conn),
                    r.inp("W", normal(rng, K, D, D, scale=D ** -0.5)))
    r.want = lambda: {"agg": ops.bmm_fused(h, bs, cn, W)}
    return _lib.load().impnn_bmm_fused(P(h), P(bs), P(cn), P(W), r.out("agg", B * N * D * 4), B, N, E, D, K, S())


def bond_type_matrices(r, D, short):
    rng = rng_of(4, D)
    tb, W = r.inp("bond_table", normal(rng, VB, K)), r.inp("W", normal(rng, K, D, D))
    r.want = lambda: {"out": ops.bond_type_matrices(tb, W)}
    return _lib.load().impnn_bond_type_matrices(P(tb), P(W), r.out("out", VB * D * D * 4), VB, K, D, S())


def bond_type_matrices_multi(r, D, short):
    rng, n = rng_of(5, D), 4
    tb = r.inp("bond_table", normal(rng, VB, K))
    Ws = [r.inp(f"W{i}", normal(rng, K, D, D)) for i in range(n)]
    outs = [r.out(f"type_mats{i}", VB * D * D * 4) for i in range(n)]
    r.want = lambda: {f"type_mats{i}": ops.bond_type_matrices(tb, Ws[i]) for i in range(n)}   # "bitwise equal A_p"
    return _lib.load().impnn_bond_type_matrices_multi(P(tb), r.table(Ws), r.table(outs), n, VB, K, D, S())


def exact_messages(hh, AA, bond, conn):
    """m[b,e] = A[type] h[b,src] in fp64 on exact inputs: every product is a multiple of 2^-6 of magnitude <= 1/4 and D
    of them meet in a sum, so any float32 order gives these values - the reference shares no code with a kernel."""
    b, e, D, vb = conn.shape[0], conn.shape[1], hh.shape[-1], AA.shape[0]
    ref = np.zeros((b, e, D))
    for i in range(b):
        for j in range(e):
            s_, t_, ty = conn[i, j, 0], conn[i, j, 1], bond[i, j]
            if 0 < s_ < hh.shape[1] and 0 < t_ < hh.shape[1] and 0 <= ty < vb:
                ref[i, j] = AA[ty].astype(np.float64) @ hh[i, s_].astype(np.float64) + 0.0   # (+ 0.0: no negative zero)
    assert_exact(ref, np.full(1, 0.25 * D), 2.0 ** -6)
    return torch.from_numpy(ref.astype(np.float32))


def bmm_message_typed(r, D, short):
    rng = rng_of(6, D)
    _, bond, conn = graph(rng)
    hh, AA = exact(rng, B, N, D), exact(rng, VB, D, D)
    h, bd, cn, A = r.inp("h", hh), r.inp("bond_ids", bond), r.inp("conn", conn), r.inp("type_mats", AA)
    # the wrapper takes this entry at atom_dim 32 and the sorted one elsewhere: exact inputs hold both by the fp64 result
    ref = exact_messages(hh, AA, bond, conn)

    def want():
        assert np.array_equal(bits(ops.bmm_message_typed(h, bd, cn, A)), bits(ref)), "the wrapper against the exact result"
        return {"messages": ref}
    r.want = want
    return _lib.load().impnn_bmm_message_typed(P(h), P(bd), P(cn), P(A), r.out("messages", B * E * D * 4), B, N, E, D,
                                               VB, S())


def reduce_scatter_add(r, p, short):
    D, stride = p
    rng = rng_of(7, D, stride)
    _, _, conn = graph(rng)
    m = exact(rng, B, E, D)
    tgt = conn[:, :, 1]
    ref = np.zeros((B, N, D), np.float64)
    mag = np.zeros((B, N, D), np.float64)
    for b in range(B):
        for e in range(E):
            if 0 < tgt[b, e] < N:
                ref[b, tgt[b, e]] += m[b, e]
                mag[b, tgt[b, e]] += np.abs(m[b, e])
    assert_exact(ref, mag, 0.125)
    md, cn = r.inp("messages", m), r.inp("conn", conn)
    view = cn[:, :, 1]
    tg = view if stride == 2 else r.inp("tgt", np.ascontiguousarray(tgt))
    r.want = lambda: {"agg": ops.reduce_scatter_add(md, tg, N)}
    rc = _lib.load().impnn_reduce_scatter_add(P(md), C.c_void_p(cn.data_ptr() + 4) if stride == 2 else P(tg), stride,
                                              r.out("agg", B * N * D * 4), B, N, E, D, S())
    if rc == 0:
        torch.cuda.synchronize()
        got = r.outs["agg"].body(np.float32, "agg").reshape(B, N, D)
        assert np.array_equal(got.astype(np.float64), ref), "reduce_scatter_add against the exact fp64 sums"
    return rc


def global_sum_pool(r, D, short):
    rng = rng_of(8, D)
    atom, _, _ = graph(rng)
    h, ids = r.inp("h", normal(rng, B, N, D)), r.inp("atom_ids", atom)
    r.want = lambda: {"out": ops.global_sum_pool(h, ids)}
    return _lib.load().impnn_global_sum_pool(P(h), P(ids), r.out("out", B * D * 4), B, N, D, S())


def gated_update_inputs(r, rng, D, rows=ROWS):
    h, agg = r.inp("h", normal(rng, rows, D)), r.inp("agg", normal(rng, rows, D))
    ps = [r.inp(n, a) for n, a in zip(("Wz", "bz", "Wr", "br", "Wh", "bh", "gamma", "beta"), gu_params(rng, D))]
    return h, agg, ps


def gated_update(r, D, short):
    rng = rng_of(9, D)
    h, agg, ps = gated_update_inputs(r, rng, D)
    r.want = lambda: {"out": ops.gated_update(h, agg, *ps)}
    return _lib.load().impnn_gated_update(P(h), P(agg), *[P(t) for t in ps], ops.LN_EPS, r.out("out", ROWS * D * 4), ROWS,
                                          D, S())


def dropout_of(r, rate=0.25, layer=3):
    step = r.inp("step", np.array([5], np.int64))
    return ops.Dropout(rate, 0x123456789ABCDEF, ops.dropout_layer_word(layer), step)


def gated_update_dropout(r, D, short):
    rng = rng_of(10, D)
    h, agg, ps = gated_update_inputs(r, rng, D)
    drop = dropout_of(r)
    r.want = lambda: {"out": ops.gated_update(h, agg, *ps, dropout=drop)}
    return _lib.load().impnn_gated_update_dropout(P(h), P(agg), *[P(t) for t in ps], ops.LN_EPS,
                                                  r.out("out", ROWS * D * 4), ROWS, D, *drop.args(), S())


def gated_update_rows(r, p, short):
    """_rows, _rows_train and _rows_train_dropout: p = (D, saved?, dropout?, listed?)."""
    D, save, drop, with_list = p
    rng = rng_of(11, D, save, drop, with_list)
    h, agg, ps = gated_update_inputs(r, rng, D)
    idx, cnt = row_list(rng)
    ri, rn = (r.inp("row_index", idx), r.inp("n_rows", cnt)) if with_list else (None, None)
    dr = dropout_of(r) if drop else None
    lib = _lib.load()
    out = r.out("out", ROWS * D * 4)
    n_saved = int(lib.impnn_gated_update_rows_saved_floats(ROWS, D))
    assert n_saved == (4 * D * ROWS if D in (32, 64, 128) else 0)
    saved = r.out("saved", n_saved * 4) if save else None
    if with_list:
        r.listed["out"] = row_mask(idx[:LISTED], D * 4)
        if save:   # by list POSITION p < *n_rows: z | r | candidate at p * 3 D, r * h at max_rows * 3 D + p * D
            m = np.zeros(n_saved, bool)
            m[:LISTED * 3 * D] = True
            m[ROWS * 3 * D:ROWS * 3 * D + LISTED * D] = True
            r.listed["saved"] = np.repeat(m, 4)
    rows_arg = (ri, rn) if with_list else None

    def want():
        res = ops.gated_update(h, agg, *ps, rows=rows_arg, save=save, dropout=dr)
        return {"out": res[0], "saved": res[1]} if save else {"out": res}
    r.want = want
    tail = [P(ri) if with_list else None, P(rn) if with_list else None, ROWS, D]
    args = [P(h), P(agg), *[P(t) for t in ps], ops.LN_EPS, out]
    if drop:
        return lib.impnn_gated_update_rows_train_dropout(*args, *tail, saved, *dr.args(), S())
    if save:
        return lib.impnn_gated_update_rows_train(*args, *tail, saved, S())
    return lib.impnn_gated_update_rows(*args, *tail, S())


def kept_rows_and_fill(r, _, short):
    rng = rng_of(12)
    atom, bond, conn = graph(rng)
    a, bd, cn = r.inp("atom_ids", atom), r.inp("bond_ids", bond), r.inp("conn", conn)
    lib = _lib.load()
    rc = lib.impnn_kept_rows(P(a), P(bd), P(cn), r.out("rows_out", B * 4), B, N, E, VB, S())
    if rc:
        return rc
    torch.cuda.synchronize()
    kept = r.outs["rows_out"].body(np.int32, "rows_out").copy()
    assert ((kept >= 0) & (kept <= N)).all()
    kd = r.inp("kept_rows", kept)
    incl = r.inp("prefix", np.cumsum(kept).astype(np.int32))
    total = int(kept.sum())
    # the list's documented length is *n_rows = sum r_b entries: a buffer of exactly that many
    rc = lib.impnn_row_index_fill(P(kd), P(incl), r.out("row_index", total * 4), r.out("n_rows", 4), B, N, S())

    def want():
        idx, cnt = ops.kept_row_index(a, bd, cn, VB)
        return {"n_rows": cnt, "row_index": idx[:total]}
    r.want = want
    return rc


def dropout_step(r, _, short):
    lib = _lib.load()
    counter = torch.tensor([41], dtype=torch.int64, device=DEV)
    r.want = lambda: {"snapshot": ops.dropout_step(counter.clone()), "counter": counter + 1}
    g = Guarded(8, counter.view(torch.uint8))
    r.outs["counter"] = g
    return lib.impnn_dropout_step(g.ptr, r.out("snapshot", 8), S())


def dropout_mask(r, p, short):
    D, with_list = p
    rng = rng_of(13, D, with_list)
    idx, cnt = row_list(rng)
    drop = dropout_of(r)
    ri, rn = (r.inp("row_index", idx), r.inp("n_rows", cnt)) if with_list else (None, None)
    if with_list:
        r.listed["out"] = row_mask(idx[:LISTED], D * 4)
    r.want = lambda: {"out": ops.dropout_mask(drop, ROWS, D, (ri, rn) if with_list else None)}
    rate, seed, step, lw = drop.args()
    return _lib.load().impnn_dropout_mask(seed, step, lw, rate, P(ri) if with_list else None, P(rn) if with_list else None,
                                          ROWS, D, r.out("out", ROWS * D * 4), S())


def validate_indices(r, _, short):
    rng = rng_of(14)
    atom, bond, conn = graph(rng)
    atom[1, 0] = VA + 3
    a, bd, cn = r.inp("atom_ids", atom), r.inp("bond_ids", bond), r.inp("conn", conn)
    want = np.array([((conn < 0) | (conn >= N)).sum(), ((atom < 0) | (atom >= VA)).sum(), ((bond < 0) | (bond >= VB)).sum()],
                    np.int32)
    assert want.all()
    r.want = lambda: {"counts": torch.from_numpy(want)}
    return _lib.load().impnn_validate_indices(P(cn), P(a), P(bd), r.out("counts", 12, fill=0), B, N, E, VA, VB, S())


LAYER_CASES = (
    [(embed_gather, D) for D in DIMS] + [(bmm_message, D) for D in DIMS] + [(bmm_fused, D) for D in DIMS]
    + [(bond_type_matrices, D) for D in DIMS] + [(bond_type_matrices_multi, D) for D in DIMS]
    + [(bmm_message_typed, D) for D in DIMS] + [(reduce_scatter_add, (D, s)) for D in DIMS for s in (1, 2)]
    + [(global_sum_pool, D) for D in DIMS] + [(gated_update, D) for D in DIMS]
    + [(gated_update_dropout, D) for D in DIMS]
    + [(gated_update_rows, (D, False, False, True)) for D in (32, 64, 128)]
    + [(gated_update_rows, (D, True, False, wl)) for D in (32, 64, 128) for wl in (True, False)]
    + [(gated_update_rows, (D, True, True, wl)) for D in (32, 64, 128) for wl in (True, False)]
    + [(gated_update_rows, (40, False, True, False))]
    + [(kept_rows_and_fill, 0), (dropout_step, 0), (validate_indices, 0)]
    + [(dropout_mask, (D, wl)) for D in (8, 40, 128) for wl in (True, False)])

case_id = lambda c: f"{c[0].__name__}-{c[1]}".replace(" ", "")


@pytest.mark.parametrize("case", LAYER_CASES, ids=case_id)
def test_layer_kernels(case):
    check_case(*case)


# ---------------------------------------------------------------- the adjoints
def grads_of(out, inputs, seed):
    return torch.autograd.grad(out, inputs, seed)


def embed_gather_bwd(r, D, short):
    rng = rng_of(20, D)
    ids = rng.integers(-1, VA + 1, size=(B * N,)).astype(np.int32)
    dout = exact(rng, B * N, D)
    ref, mag = np.zeros((VA, D)), np.zeros((VA, D))
    ok = (ids >= 0) & (ids < VA)
    np.add.at(ref, ids[ok], dout[ok].astype(np.float64))
    np.add.at(mag, ids[ok], np.abs(dout[ok]).astype(np.float64))
    assert_exact(ref, mag, 0.125)
    i_d, d_d = r.inp("ids", ids), r.inp("dout", dout)

    def want():
        table = torch.zeros(VA, D, device=DEV, requires_grad=True)
        return {"dtable": grads_of(ops.embed_gather(i_d, table), table, d_d.view(B * N, D))[0]}
    r.want = want
    rc = _lib.load().impnn_embed_gather_bwd(P(i_d), P(d_d), r.out("dtable", VA * D * 4, fill=0), B * N, VA, D, S())
    if rc == 0:
        torch.cuda.synchronize()
        got = r.outs["dtable"].body(np.float32, "dtable").reshape(VA, D)
        assert np.array_equal(got.astype(np.float64), ref), "embed_gather_bwd against the exact fp64 sums"
    return rc


def reduce_scatter_bwd(r, p, short):
    D, stride = p
    rng = rng_of(21, D, stride)
    _, _, conn = graph(rng)
    dagg, cn = r.inp("dagg", normal(rng, B, N, D)), r.inp("conn", conn)
    tg = r.inp("tgt", np.ascontiguousarray(conn[:, :, 1]))

    def want():
        m = torch.zeros(B, E, D, device=DEV, requires_grad=True)
        return {"dmessages": grads_of(ops.reduce_scatter_add(m, tg, N), m, dagg)[0]}
    r.want = want
    return _lib.load().impnn_reduce_scatter_bwd(P(dagg), C.c_void_p(cn.data_ptr() + 4) if stride == 2 else P(tg), stride,
                                                r.out("dmessages", B * E * D * 4), B, N, E, D, S())


def global_sum_pool_bwd(r, D, short):
    rng = rng_of(22, D)
    atom, _, _ = graph(rng)
    dp, ids = r.inp("dpooled", normal(rng, B, D)), r.inp("atom_ids", atom)

    def want():
        h = torch.zeros(B, N, D, device=DEV, requires_grad=True)
        return {"dh": grads_of(ops.global_sum_pool(h, ids), h, dp)[0]}
    r.want = want
    return _lib.load().impnn_global_sum_pool_bwd(P(dp), P(ids), r.out("dh", B * N * D * 4), B, N, D, S())


def bond_type_matrices_bwd(r, p, short):
    D, k = p
    rng = rng_of(23, D, k)
    tb, W, dA = r.inp("bond_table", normal(rng, VB, k)), r.inp("W", normal(rng, k, D, D)), r.inp("dA", normal(rng, VB, D, D))

    def want():
        t, w = tb.clone().requires_grad_(), W.clone().requires_grad_()
        dtb, dW = grads_of(ops.bond_type_matrices(t, w), (t, w), dA)
        return {"dW": dW, "dbond_table": dtb}
    r.want = want
    return _lib.load().impnn_bond_type_matrices_bwd(P(tb), P(W), P(dA), r.out("dW", k * D * D * 4),
                                                    r.out("dbond_table", VB * k * 4), VB, k, D, 0, S())


MULTI_N, MULTI_K = 4, 8


def multi_inputs(r, rng, D):
    tb = r.inp("bond_table", normal(rng, VB, MULTI_K))
    Ws = [r.inp(f"W{i}", normal(rng, MULTI_K, D, D)) for i in range(MULTI_N)]
    dAs = [r.inp(f"dA{i}", normal(rng, VB, D, D)) for i in range(MULTI_N)]
    return tb, Ws, dAs


def single_layer_dW(tb, Ws, dAs):
    """'bitwise equal dW_p': the single-layer entry's dW of every layer, through its autograd node."""
    res = {}
    for i, (W, dA) in enumerate(zip(Ws, dAs)):
        t, w = tb.clone().requires_grad_(), W.clone().requires_grad_()
        res[f"dW{i}"] = grads_of(ops.bond_type_matrices(t, w), (t, w), dA)[1]
    return res


def bond_type_matrices_multi_bwd(r, D, short):
    rng = rng_of(24, D)
    tb, Ws, dAs = multi_inputs(r, rng, D)
    dW = [r.out(f"dW{i}", MULTI_K * D * D * 4) for i in range(MULTI_N)]
    r.want = lambda: single_layer_dW(tb, Ws, dAs)
    return _lib.load().impnn_bond_type_matrices_multi_bwd(P(tb), r.table(Ws), r.table(dAs), r.table(dW),
                                                          r.out("dbond_table", VB * MULTI_K * 4), MULTI_N, VB, MULTI_K, D,
                                                          0, S())


def bond_type_matrices_multi_bwd_ws(r, p, short):
    D, n = p
    rng = rng_of(24, D)   # the inputs of the case above at n = MULTI_N
    tb, Ws, dAs = multi_inputs(r, rng, D)
    extra = [(r.inp(f"W{i}", normal(rng, MULTI_K, D, D)), r.inp(f"dA{i}", normal(rng, VB, D, D))) for i in range(MULTI_N, n)]
    Ws, dAs = Ws + [e[0] for e in extra], dAs + [e[1] for e in extra]
    lib = _lib.load()
    need = int(lib.impnn_bond_type_matrices_multi_bwd_workspace_floats(n, VB, MULTI_K, D))
    assert need > 0
    ws = r.work("workspace", need * 4)
    dW = [r.out(f"dW{i}", MULTI_K * D * D * 4) for i in range(n)]

    def want():
        leaves = [tb.clone().requires_grad_()] + [W.clone().requires_grad_() for W in Ws]
        outs = autograd.BondTypeMatricesAll.apply(*leaves)
        g = grads_of(outs[:n], leaves, dAs)
        return {"dbond_table": g[0], **{f"dW{i}": g[1 + i] for i in range(n)}}
    r.want = want
    return lib.impnn_bond_type_matrices_multi_bwd_ws(P(tb), r.table(Ws), r.table(dAs), r.table(dW),
                                                     r.out("dbond_table", VB * MULTI_K * 4), n, VB, MULTI_K, D, 0, ws.ptr,
                                                     need - (short == "workspace"), S())


def gated_update_bwd(r, p, short):
    """Every backward form: p = (D, listed?, saved?, dropout?[, rows])."""
    D, with_list, kept, drop = p[:4]
    ROWS = p[4] if len(p) > 4 else globals()["ROWS"]
    rng = rng_of(25, *p)
    h, agg, ps = gated_update_inputs(r, rng, D, ROWS)
    dout = r.inp("dout", normal(rng, ROWS, D))
    idx, cnt = row_list(rng, ROWS)
    ri, rn = (r.inp("row_index", idx), r.inp("n_rows", cnt)) if with_list else (None, None)
    rows_arg = (ri, rn) if with_list else None
    dr = dropout_of(r) if drop else None
    lib = _lib.load()
    query = lib.impnn_gated_update_rows_bwd_workspace_floats if (with_list or (kept and D != 32)) \
        else lib.impnn_gated_update_bwd_workspace_floats
    need, n_par = int(query(ROWS, D)), int(lib.impnn_gated_update_param_floats(D))
    assert need > 0 and n_par == 3 * (2 * D * D + D) + 2 * D
    ws = r.work("workspace", need * 4)
    saved = None
    if kept:   # the forward's buffer: its listed positions, the run's fill everywhere else; the backward consumes it
        src = ops.gated_update(h, agg, *ps, rows=rows_arg, save=True, dropout=dr)[1]
        saved = r.work("saved", src.numel() * 4)
        if with_list:
            m = torch.zeros(src.numel(), dtype=torch.bool, device=DEV)
            m[:LISTED * 3 * D] = True
            m[ROWS * 3 * D:ROWS * 3 * D + LISTED * D] = True
            body = saved.view().view(torch.float32)
            body[m] = src[m]
        else:
            saved.view().copy_(src.view(torch.uint8))
        r.settle("saved")
        kept_copy = saved.view().view(torch.float32).clone()
    if with_list:
        r.listed["dh"] = r.listed["dagg"] = row_mask(idx[:LISTED], D * 4, ROWS)

    def want():
        g = autograd._gated_update_backward((h, agg, *ps), ops.LN_EPS, dout, row_list=rows_arg,
                                            kept=kept_copy if kept else None, dropout=dr)
        return {"dh": g[0], "dagg": g[1], "dparams": torch.cat([t.reshape(-1) for t in g[2:10]])}
    r.want = want
    args = [P(h), P(agg), *[P(t) for t in ps[:7]], ops.LN_EPS, P(dout), r.out("dh", ROWS * D * 4),
            r.out("dagg", ROWS * D * 4), r.out("dparams", n_par * 4), ws.ptr, need - (short == "workspace")]
    lst = [P(ri) if with_list else None, P(rn) if with_list else None]
    d = dr.args() if drop else ()
    if kept:
        fn = lib.impnn_gated_update_rows_bwd_saved_dropout if drop else lib.impnn_gated_update_rows_bwd_saved
        return fn(*args, *lst, ROWS, D, 0, saved.ptr, *d, S())
    if with_list:
        fn = lib.impnn_gated_update_rows_bwd_dropout if drop else lib.impnn_gated_update_rows_bwd
        return fn(*args, *lst, ROWS, D, 0, *d, S())
    fn = lib.impnn_gated_update_bwd_dropout if drop else lib.impnn_gated_update_bwd
    return fn(*args, ROWS, D, 0, *d, S())


def typed_graph(rng, b, e, vb):
    _, bond, conn = graph(rng, b, N, e, vb)
    return bond, conn


def bmm_message_typed_sorted(r, p, short):
    D, vb, b, e = p
    rng = rng_of(26, *p)
    bond, conn = typed_graph(rng, b, e, vb)
    hh, AA = exact(rng, b, N, D), exact(rng, vb, D, D)
    h, bd, cn, A = r.inp("h", hh), r.inp("bond_ids", bond), r.inp("conn", conn), r.inp("type_mats", AA)
    lib = _lib.load()
    need = int(lib.impnn_bmm_message_typed_bwd_workspace_bytes(b, e, vb))
    assert need == 4 * (4 * (vb + 1) + b * e)
    ws = r.work("workspace", need)
    ref = exact_messages(hh, AA, bond, conn)

    def want():   # (the wrapper takes this entry at every width but 32)
        assert np.array_equal(bits(ops.bmm_message_typed(h, bd, cn, A)), bits(ref)), "the wrapper against the exact result"
        return {"messages": ref}
    r.want = want
    return lib.impnn_bmm_message_typed_sorted(P(h), P(bd), P(cn), P(A), r.out("messages", b * e * D * 4), ws.ptr,
                                              need - (short == "workspace"), b, N, e, D, vb, 0, S())


def typed_message_bwd(r, p, short):
    """impnn_bmm_message_typed_bwd ("bmm"), impnn_message_reduce_typed_bwd ("reduce") and its _scratch form: exact
    inputs, so the float atomics on dh and dtype_mats give the fp64 sums in any order."""
    entry, D, vb, b, e = p
    rng = rng_of(27, D, vb, b, e)
    bond, conn = typed_graph(rng, b, e, vb)
    from_agg = entry != "bmm"
    hh, AA, gg = exact(rng, b, N, D), exact(rng, vb, D, D), exact(rng, *((b, N, D) if from_agg else (b, e, D)))
    dh_ref, dA_ref = np.zeros((b, N, D)), np.zeros((vb, D, D))
    for i in range(b):
        for j in range(e):
            s_, t_, ty = conn[i, j, 0], conn[i, j, 1], bond[i, j]
            if 0 < s_ < N and 0 < t_ < N and 0 <= ty < vb:
                g = (gg[i, t_] if from_agg else gg[i, j]).astype(np.float64)
                dh_ref[i, s_] += AA[ty].astype(np.float64).T @ g
                dA_ref[ty] += np.outer(g, hh[i, s_].astype(np.float64))
    # every term is a multiple of 2^-6 of magnitude <= 1/4; fewer than D * b * e of them meet in one sum
    bound = np.full(1, 0.25 * D * b * e)
    assert_exact(dh_ref, bound, 2.0 ** -6)
    assert_exact(dA_ref, bound, 2.0 ** -6)
    h, bd, cn, A, g = r.inp("h", hh), r.inp("bond_ids", bond), r.inp("conn", conn), r.inp("type_mats", AA), r.inp("grad", gg)
    lib = _lib.load()
    need = int(lib.impnn_bmm_message_typed_bwd_workspace_bytes(b, e, vb))
    ws = r.work("workspace", need)

    def want():
        hl, Al = h.clone().requires_grad_(), A.clone().requires_grad_()
        node = autograd.BmmMessageTyped if entry == "bmm" else autograd.MessageReduceTyped
        dh, dA = grads_of(node.apply(hl, bd, cn, Al), (hl, Al), g)
        return {"dh": dh, "dtype_mats": dA}
    if entry == "scratch":   # no wrapper below its batch threshold: the exact fp64 sums are the whole reference
        want = lambda: {"dh": torch.from_numpy(dh_ref.astype(np.float32) + np.float32(0)),
                        "dtype_mats": torch.from_numpy(dA_ref.astype(np.float32) + np.float32(0))}
    r.want = want
    args = [P(h), P(bd), P(cn), P(A), P(g), r.out("dh", b * N * D * 4, fill=0), r.out("dtype_mats", vb * D * D * 4, fill=0),
            ws.ptr, need - (short == "workspace")]
    if entry == "scratch":   # a (B,E,D) buffer whose rows at masked edges are ZERO (the header's precondition)
        args.append(r.out("edge_scratch", b * e * D * 4, fill=0))
    fn = {"bmm": lib.impnn_bmm_message_typed_bwd, "reduce": lib.impnn_message_reduce_typed_bwd,
          "scratch": lib.impnn_message_reduce_typed_bwd_scratch}[entry]
    rc = fn(*args, b, N, e, D, vb, 0, S())
    if rc == 0:
        torch.cuda.synchronize()
        assert np.array_equal(r.outs["dh"].body(np.float32, "dh").reshape(b, N, D).astype(np.float64), dh_ref), "dh"
        assert np.array_equal(r.outs["dtype_mats"].body(np.float32, "dtype_mats").reshape(vb, D, D).astype(np.float64),
                              dA_ref), "dtype_mats"
    return rc


GU_BWD = ([(D, False, False, dr) for D in (8, 32, 64, 128) for dr in (False, True)]
          + [(D, True, False, dr) for D in (64, 128) for dr in (False, True)]
          + [(32, False, True, False), (32, False, True, True)]
          + [(D, wl, True, dr) for D in (64, 128) for wl in (True, False) for dr in (False, True)])
BIG = (5, 17)   # the larger batch whose leftover sort a case runs on: (B, E)
ADJOINT_CASES = (
    [(embed_gather_bwd, D) for D in DIMS] + [(reduce_scatter_bwd, (D, s)) for D in DIMS for s in (1, 2)]
    + [(global_sum_pool_bwd, D) for D in DIMS] + [(bond_type_matrices_bwd, (D, k)) for D in DIMS for k in (K, 64)]
    + [(bond_type_matrices_multi_bwd, D) for D in (16, 64)]
    + [(bond_type_matrices_multi_bwd_ws, (D, MULTI_N), (D, MULTI_N + 3), ("workspace",)) for D in (16, 64)]
    + [(gated_update_bwd, p, (*p, 61), ("workspace",)) for p in GU_BWD]
    + [(bmm_message_typed_sorted, (D, VB, B, E), (D, VB, *BIG), ("workspace",)) for D in DIMS]
    + [(bmm_message_typed_sorted, (8, vb, B, E), (8, vb, *BIG), ("workspace",)) for vb in (1, 1025)]
    + [(typed_message_bwd, (en, D, VB, B, E), (en, D, VB, *BIG), ("workspace",))
       for en in ("bmm", "reduce", "scratch") for D in DIMS]
    + [(typed_message_bwd, (en, 8, vb, B, E), (en, 8, vb, *BIG), ("workspace",)) for en in ("bmm", "reduce")
       for vb in (1, 1025)])


@pytest.mark.parametrize("case", ADJOINT_CASES, ids=case_id)
def test_adjoints(case):
    check_case(*case)


# ---------------------------------------------------------------- the fused encoder and its weight images
ENC = dict(B=5, N=13, E=27, K=8, S=2, Va=VA, Vb=VB)       # the issue's shape
ENC_BIG = dict(B=9, N=17, E=31, K=8, S=2, Va=VA, Vb=VB)   # whose leftover workspace the third run starts from
MODE_NAMES = {0: "f32", 2: "f32t", 3: "f32x3"}
MODE_DIMS = [(0, 32), (2, 32), (3, 32), (2, 64), (3, 64), (2, 128), (3, 128)]


def packed_weights(rng, D, k, steps):
    out = []
    for _ in range(steps):
        out += [normal(rng, k * D * D, scale=(k * D) ** -0.5)]
        for _ in range(3):
            out += [normal(rng, 2 * D * D, scale=(2 * D) ** -0.5), normal(rng, D, scale=0.1)]
        out += [(1.0 + normal(rng, D, scale=0.1)).astype(np.float32), normal(rng, D, scale=0.1)]
    return np.concatenate(out) if out else np.zeros(1, np.float32)


def encoder_operands(r, rng, shape, D, n_ions):
    """shape: a dict as ENC, or the name of a composition of tests/plan_cases.py (two ions, its own workgroups)."""
    if isinstance(shape, str):
        case = PC.COMPOSITIONS[shape]()
        ions = [tuple(r.inp(f"{p}_{k}", case.inp[f"{p}_{k}"]) for k in ("atom", "bond", "connectivity")) for p in PC.IONS]
        ions = ions[:n_ions]
        sh = dict(B=int(case.inp["cat_atom"].shape[0]), N=case.N, E=case.E, K=PC.K, S=PC.S, Va=case.Va, Vb=case.Vb)
    else:
        sh = shape
        ions = []
        for g in range(n_ions):
            atom, bond, conn = graph(rng, sh["B"], sh["N"], sh["E"], sh["Vb"])
            ions.append((r.inp(f"atom{g}", atom), r.inp(f"bond{g}", bond), r.inp(f"conn{g}", conn)))
    atab, btab = r.inp("atom_table", normal(rng, sh["Va"], D)), r.inp("bond_table", normal(rng, sh["Vb"], sh["K"], scale=0.5))
    packed = [r.inp(f"weights{g}", packed_weights(rng, D, sh["K"], sh["S"])) for g in range(n_ions)]
    return sh, ions, atab, btab, packed


def encoder(r, p, short):
    """entry: "fused" (impnn_encoder_fused), "prepared" (_fused_prepared from the wrapper's image) or "plan_run"
    (impnn_encoder_plan, then impnn_encoder_run on the planned workspace)."""
    entry, mode, D, n_ions, wgs, shape = p
    rng = rng_of(30, mode, D, n_ions)
    sh, ions, atab, btab, packed = encoder_operands(r, rng, shape, D, n_ions)
    Bq, Nq, Eq, Kq, Sq, Va, Vb = (sh[k] for k in ("B", "N", "E", "K", "S", "Va", "Vb"))
    lib = _lib.load()
    need = C.c_size_t(0)
    _lib.check(lib.impnn_encoder_workspace_bytes(n_ions, Bq, Nq, Eq, D, Kq, Sq, Vb, mode, wgs, C.byref(need)))
    assert need.value > 0
    ws = r.work("workspace", need.value)
    pooled = [r.out(f"pooled{g}", Bq * D * 4) for g in range(n_ions)]
    name = MODE_NAMES[mode]
    images = None
    if entry != "fused":
        images = [ops.prepare_encoder_weights(packed[g], btab, D, Kq, Sq, name, atom_table=atab if D == 32 and mode >= 2 else None)
                  for g in range(n_ions)]
        images = [r.inp(f"image{g}", im) for g, im in enumerate(images)]

    def want():
        out = ops.encoder_fused(ions, atab, btab, None if images else packed, Sq, mode=name, prepared=images, workgroups=wgs)
        return {f"pooled{g}": out[g] for g in range(n_ions)}
    r.want = want
    tab = lambda k: r.table([ion[k] for ion in ions])
    shape_args = (Bq, Nq, Eq, D, Kq, Sq)
    if entry == "fused":
        return lib.impnn_encoder_fused(n_ions, tab(0), tab(1), tab(2), P(atab), Va, P(btab), Vb, r.table(packed), mode,
                                       r.table(pooled), *shape_args, ops.LN_EPS, wgs, ws.ptr,
                                       need.value - (short == "workspace"), S())
    if entry == "prepared":
        return lib.impnn_encoder_fused_prepared(n_ions, tab(0), tab(1), tab(2), P(atab), Va, P(btab), Vb, r.table(images),
                                                mode, r.table(pooled), *shape_args, ops.LN_EPS, wgs, ws.ptr,
                                                need.value - (short == "workspace"), S())
    info = _lib.PlanInfo()
    rc = lib.impnn_encoder_plan(n_ions, tab(0), tab(1), tab(2), Bq, Nq, Eq, D, Kq, Sq, Va, Vb, mode, wgs, ws.ptr,
                                need.value - (short == "plan"), S(), C.byref(info))
    if rc:
        return rc
    if short == "run":
        r.settle("workspace")     # the plan is the run's documented input: the refused run leaves it as it is
    return lib.impnn_encoder_run(n_ions, tab(0), P(atab), Va, P(btab), Vb, r.table(images), mode, r.table(pooled),
                                 *shape_args, ops.LN_EPS, C.byref(info), ws.ptr, need.value - (short == "run"), S())


def prepared_image(r, p, short):
    """form: "plain", "atoms" or "gates"; the image in a buffer of exactly the query's bytes, then the encoder from it."""
    form, mode, D, steps, Va, Vb = p
    rng = rng_of(31, mode, D, steps, Va, Vb)
    sh = dict(ENC, S=steps, Va=Va, Vb=Vb)
    atom, bond, conn = graph(rng, sh["B"], sh["N"], sh["E"], Vb)
    atom = np.minimum(atom, Va - 1)
    ion = (r.inp("atom", atom), r.inp("bond", bond), r.inp("conn", conn))
    atab, btab = r.inp("atom_table", normal(rng, Va, D)), r.inp("bond_table", normal(rng, Vb, sh["K"], scale=0.5))
    packed = r.inp("weights", packed_weights(rng, D, sh["K"], steps))
    lib = _lib.load()
    plain = int(lib.impnn_encoder_prepared_bytes(D, steps, Vb, mode))
    with_atoms = int(lib.impnn_encoder_prepared_bytes_atoms(D, steps, Va, Vb, mode))
    nbytes = {"plain": plain, "atoms": with_atoms,
              "gates": int(lib.impnn_encoder_prepared_bytes_gates(D, steps, Va, Vb, mode))}[form]
    assert plain > 0 and plain % 16 == 0
    table = D == 32 and mode >= 2 and steps >= 1 and Vb * (Va + 1) * 128 < (2 << 20)
    assert with_atoms == plain + (Vb * (Va + 1) * 128 if table else 0), "the documented size of the step-0 message table"
    if form == "gates":   # "plus (Va + 1) * 256 bytes, rounded up to 16"
        assert nbytes == (with_atoms + (Va + 1) * 256 + 15) // 16 * 16 if table else nbytes == with_atoms
    head = [P(packed), P(btab)] + ([] if form == "plain" else [P(atab), Va])
    fn = {"plain": lib.impnn_encoder_prepare_weights, "atoms": lib.impnn_encoder_prepare_weights_atoms,
          "gates": lib.impnn_encoder_prepare_weights_gates}[form]
    rc = fn(*head, D, sh["K"], steps, Vb, mode, r.out("image", nbytes), nbytes - (short == "prepared"), S())
    if rc or short:
        return rc
    name = MODE_NAMES[mode]
    need = C.c_size_t(0)
    _lib.check(lib.impnn_encoder_workspace_bytes(1, sh["B"], sh["N"], sh["E"], D, sh["K"], steps, Vb, mode, 0, C.byref(need)))
    ws = r.work("workspace", need.value)
    tab = lambda k: r.table([ion[k]])
    rc = lib.impnn_encoder_fused_prepared(1, tab(0), tab(1), tab(2), P(atab), Va, P(btab), Vb, r.table([r.outs["image"].ptr]),
                                          mode, r.table([r.out("pooled", sh["B"] * D * 4)]), sh["B"], sh["N"], sh["E"], D,
                                          sh["K"], steps, ops.LN_EPS, 0, ws.ptr, need.value, S())

    def want():
        im = ops.prepare_encoder_weights(packed, btab, D, sh["K"], steps, name, atom_table=None if form == "plain" else atab,
                                         gates=form == "gates")
        assert im.numel() == max(nbytes, 16)
        out = ops.encoder_fused([ion], atab, btab, None, steps, mode=name, prepared=[im])
        return {"image": im[:nbytes], "pooled": out[0]}
    r.want = want
    return rc


ENCODER_CASES = (
    [(encoder, (en, m, D, n, w, ENC), (en, m, D, n, w, ENC_BIG), ("workspace",) if en != "plan_run" else ("plan", "run"))
     for en in ("fused", "prepared", "plan_run") for m, D in MODE_DIMS for n in (1, 2)
     for w in ((0, 16) if D == 32 else (0,))]
    + [(encoder, (en, m, 32, 2, PC.COMPOSITIONS[c]().workgroups, c), None, ())
       for en in ("fused", "plan_run") for c in ("fewer_than_workgroups", "one_giant_among_tiny") for m in (2, 3)]
    + [(encoder, ("plan_run", 0, 32, 2, 0, "fewer_than_workgroups"), None, ())])
IMAGE_CASES = [(prepared_image, (f, m, D, st, va, vb), None, ("prepared",))
               for m, D in MODE_DIMS for f in (("plain", "atoms", "gates") if D == 32 and m >= 2 else ("plain",))
               for st in (1, 2) for va in (1, 9) for vb in (1, 5)]


def encoder_id(c):
    p = c[1]
    return f"{c[0].__name__}-" + "-".join(str(x if not isinstance(x, dict) else "B%d" % x["B"]) for x in p)


@pytest.mark.parametrize("case", ENCODER_CASES, ids=encoder_id)
def test_encoder(case):
    check_case(*case)


@pytest.mark.parametrize("case", IMAGE_CASES, ids=encoder_id)
def test_prepared_images(case):
    check_case(*case)


# ---------------------------------------------------------------- optimizer, metrics, loader
VAR_SIZES = (1, 37, 1025)


def adam(r, p, short):
    """form: "step" (host step number), "counted" (device counter) or "scheduled" (device rate, global clip norm with
    its workspace, decoupled weight decay).  Slots, moments, gradients and the counter are guarded."""
    form = p
    rng = rng_of(40)
    lr, b1, b2, eps, clip, step0 = 1e-2, 0.9, 0.999, 1e-7, 0.5, 3
    init = {}
    for i, n in enumerate(VAR_SIZES):
        init[i] = (normal(rng, n), normal(rng, n), normal(rng, n, scale=0.1), np.abs(normal(rng, n, scale=0.1)))
    ptrs = []
    for i, n in enumerate(VAR_SIZES):
        for name, a in zip("wgmv", init[i]):
            ptrs.append(r.out(f"{name}{i}", 4 * n, fill=torch.from_numpy(a).view(torch.uint8)).value)
    table = r.inp("var_table", np.array(ptrs, np.int64))
    sizes = r.inp("sizes", np.array(VAR_SIZES, np.int64))
    lib = _lib.load()
    scheduled = form == "scheduled"

    def want():
        vs = [torch.from_numpy(init[i][0]).to(DEV) for i in range(len(VAR_SIZES))]
        opt = train.Adam(lr, b1, b2, eps, clipnorm=None if scheduled else clip, global_clipnorm=clip if scheduled else None,
                         weight_decay=0.01 if scheduled else None)
        opt.build(vs)
        opt.flat_grad.copy_(torch.from_numpy(np.concatenate([init[i][1] for i in init])))
        opt.m.copy_(torch.from_numpy(np.concatenate([init[i][2] for i in init])))
        opt.v.copy_(torch.from_numpy(np.concatenate([init[i][3] for i in init])))
        opt._step_dev.fill_(step0)
        opt.apply_gradients()
        res, off = {"counter": opt._step_dev}, 0
        for i, n in enumerate(VAR_SIZES):
            res.update({f"w{i}": vs[i], f"g{i}": opt.flat_grad[off:off + n], f"m{i}": opt.m[off:off + n],
                        f"v{i}": opt.v[off:off + n]})
            off += n
        if form == "step":   # the host forms the bias correction there: its own bits; test_gpu_train_fuzz.py::test_adam_fuzz holds its values
            return {k: v for k, v in res.items() if k[0] == "g"}
        return res
    r.want = want
    if form == "step":
        return lib.impnn_adam_clipnorm_step(P(table), P(sizes), len(VAR_SIZES), step0 + 1, lr, b1, b2, eps, clip, S())
    counter = r.out("counter", 8, fill=torch.tensor([step0], dtype=torch.int64).view(torch.uint8))
    if form == "counted":
        return lib.impnn_adam_clipnorm_step_counted(P(table), P(sizes), len(VAR_SIZES), counter, lr, b1, b2, eps, clip, S())
    rec = r.inp("lr_record", train._lr_record(train.LR_CONSTANT, lr))
    flags = r.inp("decay_flags", np.ones(len(VAR_SIZES), np.int32))
    need = int(lib.impnn_adam_step_scheduled_workspace_floats(len(VAR_SIZES)))
    assert need > 0
    ws = r.work("workspace", 4 * need)
    return lib.impnn_adam_step_scheduled(P(table), P(sizes), len(VAR_SIZES), counter, P(rec), b1, b2, eps, 0.0, clip, 0.01,
                                         P(flags), ws.ptr, need - (short == "workspace"), S())


def regression_sums(r, n, short):
    rng = rng_of(41, n)
    pred, y, w = r.inp("pred", normal(rng, n)), r.inp("y", normal(rng, n)), r.inp("w", np.abs(normal(rng, n)))
    order = r.inp("order", rng.permutation(n).astype(np.int32))
    n_seg = 1 if n == 1 else 3
    seg = r.inp("seg_offsets", np.array([0, n] if n == 1 else [0, 7, 7, n], np.int64))
    assert _lib.load().impnn_regression_sums_words() == 8
    r.want = lambda: {"sums": ops.regression_sums(pred, y, w, order, seg, offset=0.5, scale=2.0)}
    return _lib.load().impnn_regression_sums(P(pred), P(y), P(w), P(order), P(seg), n, n_seg, 0.5, 2.0, 0,
                                             r.out("sums", n_seg * 8 * 8, offset=8), S())   # "8 bytes: seg_offsets, sums"


def gather_rows(r, _, short):
    rng = rng_of(42)
    row_bytes, n_rows, M = (4, 52, 4100), 5, 11
    srcs = [r.inp(f"src{i}", rng.integers(-2 ** 31, 2 ** 31 - 1, size=(M, rb // 4)).astype(np.int32))
            for i, rb in enumerate(row_bytes)]
    rows = r.inp("rows", rng.integers(0, M, size=n_rows).astype(np.int64))
    dsts = [r.out(f"dst{i}", n_rows * rb) for i, rb in enumerate(row_bytes)]

    def want():
        out = [torch.empty(n_rows, rb // 4, dtype=torch.int32, device=DEV) for rb in row_bytes]
        ops.gather_rows(srcs, out, rows)
        return {f"dst{i}": t for i, t in enumerate(out)}
    r.want = want
    return _lib.load().impnn_gather_rows(3, r.table(srcs), r.table(dsts), (C.c_int64 * 3)(*row_bytes), P(rows), n_rows, S())


def batch_assemble(r, _, short):
    rng = rng_of(43)
    Bq, Nq, L, M = 5, 7, 9, 6
    ions = []
    for g in range(2):
        n_atoms = rng.integers(1, Nq + 3, size=M)        # some samples hold more than N atoms: cut at N
        n_edges = rng.integers(0, 7, size=M)             # and more than L / 2 edges: cut at L slots
        n_bonds = n_edges + rng.integers(-1, 2, size=M).clip(-n_edges, 1)   # lists of unequal length: zip() cuts them
        m_e = np.minimum(n_edges, n_bonds)
        ions.append({
            "atom_flat": r.inp(f"atom_flat{g}", rng.integers(0, VA - 1, size=int(n_atoms.sum())).astype(np.int32)),
            "atom_off": r.inp(f"atom_off{g}", np.concatenate([[0], np.cumsum(n_atoms)]).astype(np.int32)),
            "edge_flat": r.inp(f"edge_flat{g}", rng.integers(0, Nq, size=(int(m_e.sum()), 2)).astype(np.int32)),
            "bond_flat": r.inp(f"bond_flat{g}", rng.integers(0, VB - 1, size=int(m_e.sum())).astype(np.int32)),
            "edge_off": r.inp(f"edge_off{g}", np.concatenate([[0], np.cumsum(m_e)]).astype(np.int32))})
    idx = r.inp("sample_idx", np.array([4, 0, M, 2, -1], np.int32))     # two indices outside the data set
    t_flat = r.inp("t_flat", normal(rng, M))
    a = [r.out(f"atom_ids{g}", Bq * Nq * 4) for g in range(2)]
    b = [r.out(f"bond_ids{g}", Bq * L * 4) for g in range(2)]
    c = [r.out(f"conn{g}", Bq * L * 2 * 4) for g in range(2)]

    def want():
        outs, t = ops.batch_assemble(idx, ions, Nq, L, id_shift=1, t_flat=t_flat)
        res = {"t_out": t}
        for g in range(2):
            res.update({f"atom_ids{g}": outs[g][0], f"bond_ids{g}": outs[g][1], f"conn{g}": outs[g][2]})
        return res
    r.want = want
    mk = lambda k: r.table([ion[k] for ion in ions])
    return _lib.load().impnn_batch_assemble(2, P(idx), Bq, M, mk("atom_flat"), mk("atom_off"), mk("edge_flat"),
                                            mk("bond_flat"), mk("edge_off"), 1, Nq, L, r.table(a), r.table(b), r.table(c),
                                            P(t_flat), r.out("t_out", Bq * 4), S())


TRAIN_CASES = [(adam, "step"), (adam, "counted"), (adam, "scheduled", None, ("workspace",)), (regression_sums, 1),
               (regression_sums, 33), (gather_rows, 0), (batch_assemble, 0)]


@pytest.mark.parametrize("case", TRAIN_CASES, ids=case_id)
def test_optimizer_metrics_loader(case):
    check_case(*case)


# ---------------------------------------------------------------- the heads
HD, HF, HMX = 32, 32, 20          # atom_dim, fp_size, mixing_size
HEAD_B = (1, 5, 33)               # 33 crosses one 32-sample block


def head_tensors(r, rng, kind):
    """The model head's individual tensors in the packed order (10 for kind 0, 12 for kind 1)."""
    u = lambda *sh: r.inp(f"w{len(r.inputs)}", rng.uniform(-0.4, 0.4, size=sh).astype(np.float32))
    ws = [u(HD, HF), u(HF), u(HD, HF), u(HF), u(HF, HMX), u(HMX), u(HF, HMX), u(HMX)]
    return ws + ([u(HMX, 3), u(3)] if kind == 0 else [u(HMX, HF), u(HF), u(HF, 1), u(1)])


def head_batch(r, rng, kind, b):
    pc, pa = r.inp("pooled_cat", normal(rng, b, HD)), r.inp("pooled_an", normal(rng, b, HD))
    T = r.inp("temperature", rng.uniform(260.0, 400.0, size=b).astype(np.float32)) if kind == 0 else None
    return pc, pa, T


KIND_NAMES = ("viscosity", "melting_point")


def model_head(r, p, short):
    """form "packed" (impnn_model_head), "tensors" (impnn_model_head_tensors), "mix" (impnn_head_ion_mix, ion = b % 2)."""
    form, kind, b = p
    rng = rng_of(50, kind, b)
    ws = head_tensors(r, rng, kind)
    pc, pa, T = head_batch(r, rng, kind, b)
    lib = _lib.load()
    packed = r.inp("packed", torch.cat([w.reshape(-1) for w in ws]))
    assert packed.numel() == lib.impnn_model_head_floats(kind, HD, HF, HMX)
    Tp = P(T) if kind == 0 else None
    if form == "mix":
        ion = b % 2
        r.want = lambda: {"mix": ops.head_ion_mix(KIND_NAMES[kind], ion, pc, packed, HF, HMX)}
        return lib.impnn_head_ion_mix(kind, ion, P(pc), P(packed), r.out("mix", b * HMX * 4), b, HD, HF, HMX, S())
    if form == "packed":
        r.want = lambda: {"out": ops.model_head(KIND_NAMES[kind], pc, pa, T, packed, HF, HMX)}
        return lib.impnn_model_head(kind, P(pc), P(pa), Tp, P(packed), r.out("out", b * 4), b, HD, HF, HMX, S())
    r.want = lambda: {"out": autograd.ModelHead.apply(kind, HF, HMX, pc, pa, T, *ws)}
    return lib.impnn_model_head_tensors(kind, P(pc), P(pa), Tp, r.table(ws), r.out("out", b * 4), b, HD, HF, HMX, S())


def model_head_bwd(r, p, short):
    """impnn_model_head_bwd ("plain") and impnn_[weighted_]model_head_loss_bwd ("loss", "weighted").  The parameter
    gradients are added with float atomics, one addend per workgroup of 8 samples (kHeadSPB): up to 16 samples that is
    at most two addends into a zeroed buffer, whose sum does not depend on their order, and the bits are the wrapper's.
    Beyond that the header promises no order ("fp32 rounding-level run-to-run differences"): there the gradient
    buffers are held by their guards alone, and dpooled, which has one writer per element, by its bits."""
    form, kind, b = p
    rng = rng_of(51, kind, b)
    ws = head_tensors(r, rng, kind)
    pc, pa, T = head_batch(r, rng, kind, b)
    lib = _lib.load()
    Tp = P(T) if kind == 0 else None
    dw = [r.out(f"dw{i}", w.numel() * 4, fill=0) for i, w in enumerate(ws)]
    dpc, dpa = r.out("dpooled_cat", b * HD * 4), r.out("dpooled_an", b * HD * 4)
    l2v = [0.0 if w.dim() == 1 else 1e-3 * (1 + i) for i, w in enumerate(ws)]
    lam = (C.c_float * len(ws))(*l2v)

    def want():
        leaves = [t.clone().requires_grad_() for t in (pc, pa, *ws)]
        if form == "plain":
            out = autograd.ModelHead.apply(kind, HF, HMX, leaves[0], leaves[1], T, *leaves[2:])
            g = grads_of(out, leaves, seed.view(b, 1))
        else:
            wsp = torch.zeros(int(lib.impnn_model_head_loss_workspace_floats(b)), device=DEV)
            l2 = autograd.WeightedL2(l2v, sw if form == "weighted" else None)
            out = autograd.ModelHeadLoss.apply(kind, HF, HMX, l2, wsp, leaves[0], leaves[1], T, y, *leaves[2:])
            g = grads_of(out, leaves, seed.reshape(()))
        res = {"dpooled_cat": g[0], "dpooled_an": g[1]}
        if b <= 16:
            res.update({f"dw{i}": g[2 + i] for i in range(len(ws))})
        return res
    r.want = want
    if form == "plain":
        seed = r.inp("dout", normal(rng, b))
        return lib.impnn_model_head_bwd(kind, P(pc), P(pa), Tp, r.table(ws), P(seed), dpc, dpa, r.table(dw), b, HD, HF, HMX,
                                        S())
    y, seed = r.inp("y", normal(rng, b)), r.inp("dloss", np.array([0.75], np.float32))
    if form == "loss":
        return lib.impnn_model_head_loss_bwd(kind, P(pc), P(pa), Tp, r.table(ws), lam, P(y), P(seed), dpc, dpa, r.table(dw),
                                             b, HD, HF, HMX, S())
    sw = r.inp("sample_weight", np.abs(normal(rng, b)))
    return lib.impnn_weighted_model_head_loss_bwd(kind, P(pc), P(pa), Tp, r.table(ws), lam, P(y), P(sw), P(seed), dpc, dpa,
                                                  r.table(dw), b, HD, HF, HMX, S())


def zero_first_word(r, ws):
    """'the first 4 bytes ZERO before the first call': the documented precondition, set up after the fill."""
    ws.view()[:4] = 0
    r.settle("workspace")


def model_head_loss(r, p, short):
    weighted, kind, b = p
    rng = rng_of(52, kind, b)
    ws = head_tensors(r, rng, kind)
    pc, pa, T = head_batch(r, rng, kind, b)
    y = r.inp("y", normal(rng, b))
    sw = r.inp("sample_weight", np.abs(normal(rng, b))) if weighted else None
    lib = _lib.load()
    l2v = [0.0 if w.dim() == 1 else 1e-3 * (1 + i) for i, w in enumerate(ws)]
    lam = (C.c_float * len(ws))(*l2v)
    need = int(lib.impnn_model_head_loss_workspace_floats(b))
    assert need > 0
    wsp = r.work("workspace", 4 * need)
    zero_first_word(r, wsp)

    def want():
        pred = torch.empty(b, device=DEV)
        loss = autograd.ModelHeadLoss.apply(kind, HF, HMX, autograd.WeightedL2(l2v, sw, pred), torch.zeros(need, device=DEV),
                                            pc, pa, T, y, *ws)
        return {"loss": loss, "pred": pred}
    r.want = want
    head = [kind, P(pc), P(pa), P(T) if kind == 0 else None, r.table(ws), lam, P(y)]
    tail = [r.out("pred", 4 * b), r.out("loss", 4), wsp.ptr, need - (short == "workspace"), b, HD, HF, HMX, S()]
    if weighted:
        rc = lib.impnn_weighted_model_head_loss(*head, P(sw), *tail)
    else:
        rc = lib.impnn_model_head_loss(*head, *tail)
    if rc == 0:   # "every call leaves them zero"
        torch.cuda.synchronize()
        assert (wsp.host()[wsp.lo:wsp.lo + 4] == 0).all(), "the call did not leave the workspace's first word zero"
    return rc


def transfer_tensors(r, rng):
    k = lambda i, o: r.inp(f"w{len(r.inputs)}", (rng.uniform(-1, 1, size=(i, o)) * 1.5 * np.sqrt(6.0 / (i + o))).astype(np.float32))
    v = lambda n: r.inp(f"w{len(r.inputs)}", normal(rng, n, scale=0.2))
    ws = [k(HD, HF), v(HF), k(HD, HF), v(HF), k(HF, HMX), v(HMX), k(HF, HMX), v(HMX), k(HMX, 256), v(256),
          r.inp("gamma", rng.uniform(0.5, 1.5, size=256).astype(np.float32)), v(256), k(256, 128), v(128), k(128, 64), v(64),
          k(64, 1), v(1)]
    mean, var = normal(rng, 256, scale=0.2), rng.uniform(0.5, 2.0, size=256).astype(np.float32)
    return ws, mean, var


def transfer_cfg(mean, var, bn_batch=False, dropout=None, loss_kind=1):
    return {"fp_size": HF, "mixing_size": HMX, "l2": [0.0 if i % 2 else 1e-3 for i in range(18)], "moving_mean": mean,
            "moving_variance": var, "momentum": 0.9, "epsilon": 1e-3, "bn_batch": bn_batch, "dropout": dropout,
            "loss_kind": loss_kind, "delta": 0.7}


def transfer_inference(r, p, short):
    """form "head" (impnn_transfer_head), "half" (impnn_transfer_ion_half, ion = b % 2), "image"
    (impnn_transfer_grid_prepare)."""
    form, b = p
    rng = rng_of(53, b)
    ws, mean, var = transfer_tensors(r, rng)
    mean, var = r.inp("moving_mean", mean), r.inp("moving_var", var)
    cfg = transfer_cfg(mean, var)
    pc, pa = r.inp("pooled_cat", normal(rng, b, HD)), r.inp("pooled_an", normal(rng, b, HD))
    lib = _lib.load()
    if form == "head":
        r.want = lambda: {"out": ops.transfer_head(pc, pa, ws, cfg)}
        return lib.impnn_transfer_head(P(pc), P(pa), r.table(ws), P(mean), P(var), cfg["epsilon"], r.out("out", 4 * b), b,
                                       HD, HF, HMX, S())
    if form == "half":
        r.want = lambda: {"u": ops.transfer_ion_half(b % 2, pc, ws, HF, HMX)}
        return lib.impnn_transfer_ion_half(b % 2, P(pc), r.table(ws), r.out("u", b * 256 * 4), b, HD, HF, HMX, S())
    n = int(lib.impnn_transfer_grid_image_floats())
    r.want = lambda: {"image": ops.transfer_grid_prepare(ws, cfg)}
    return lib.impnn_transfer_grid_prepare(r.table(ws), P(mean), P(var), cfg["epsilon"], r.out("image", 4 * n),
                                           n - (short == "image"), S())


def transfer_rows(r, rng, form, b):
    """-> (cat, an, cat_row, an_row): the samples' own rows, or for "rows" two tables and the batch's indices (one of
    them outside its table: a row of zeros)."""
    if form != "rows":
        return r.inp("pooled_cat", normal(rng, b, HD)), r.inp("pooled_an", normal(rng, b, HD)), None, None
    Cn, An = 4, 3
    cr, ar = rng.integers(0, Cn, size=b).astype(np.int32), rng.integers(0, An, size=b).astype(np.int32)
    return (r.inp("cat_table", normal(rng, Cn, HD)), r.inp("an_table", normal(rng, An, HD)), r.inp("cat_row", cr),
            r.inp("an_row", ar))


def transfer_loss(r, p, short):
    """impnn_transfer_head_loss ("plain"), impnn_weighted_transfer_head_loss ("weighted"), impnn_transfer_head_loss_rows
    ("rows"): p = (form, B, bn_batch, dropout rate)."""
    form, b, bn_batch, rate = p
    rng = rng_of(54, b, bn_batch)
    ws, mean0, var0 = transfer_tensors(r, rng)
    cat, an, cr, ar = transfer_rows(r, rng, form, b)
    y = r.inp("y", normal(rng, b))
    sw = r.inp("sample_weight", np.abs(normal(rng, b))) if form != "plain" else None
    drop = dropout_of(r, rate) if rate else None
    lib = _lib.load()
    n_saved, need = int(lib.impnn_transfer_head_saved_floats(b, HF, HMX)), int(lib.impnn_transfer_head_loss_workspace_floats(b))
    assert n_saved > 0 and need > 0
    mean = r.out("moving_mean", 1024, fill=torch.from_numpy(mean0).view(torch.uint8))
    var = r.out("moving_var", 1024, fill=torch.from_numpy(var0).view(torch.uint8))
    saved, wsp = r.work("saved", 4 * n_saved), r.work("workspace", 4 * need)
    zero_first_word(r, wsp)
    cfg = transfer_cfg(None, None, bn_batch, drop)
    lam = (C.c_float * 18)(*cfg["l2"])

    def want():
        c2 = dict(cfg, moving_mean=torch.from_numpy(mean0).to(DEV), moving_variance=torch.from_numpy(var0).to(DEV))
        loss, pred, _ = ops.transfer_head_loss_rows(cat, an, cr, ar, ws, c2, y, torch.zeros(need, device=DEV), sample_weight=sw)
        return {"loss": loss, "pred": pred, "moving_mean": c2["moving_mean"], "moving_var": c2["moving_variance"]}
    r.want = want
    dargs = drop.args() if drop else (0.0, C.c_uint64(0), None, 0)
    head = [r.table(ws), lam, mean, var, cfg["momentum"], cfg["epsilon"], int(bn_batch), P(y)]
    tail = [cfg["loss_kind"], cfg["delta"], *dargs, saved.ptr, n_saved - (short == "saved"), r.out("pred", 4 * b),
            r.out("loss", 4), wsp.ptr, need - (short == "workspace")]
    if form == "rows":
        rc = lib.impnn_transfer_head_loss_rows(P(cat), P(an), P(cr), P(ar), *head, P(sw), *tail, b, cat.shape[0], an.shape[0],
                                               HD, HF, HMX, S())
    elif form == "weighted":
        rc = lib.impnn_weighted_transfer_head_loss(P(cat), P(an), *head, P(sw), *tail, b, HD, HF, HMX, S())
    else:
        rc = lib.impnn_transfer_head_loss(P(cat), P(an), *head, *tail, b, HD, HF, HMX, S())
    if rc == 0:
        torch.cuda.synchronize()
        assert (wsp.host()[wsp.lo:wsp.lo + 4] == 0).all(), "the call did not leave the workspace's first word zero"
    return rc


def transfer_loss_bwd(r, p, short):
    """The three backward entries on the `saved` buffer of the wrapper's forward: p as transfer_loss.  dweights are (+=)
    buffers, zeroed; entry 2 (Wfp_an) is null, a frozen tensor."""
    form, b, bn_batch, rate = p
    rng = rng_of(54, b, bn_batch)     # the forward case's operands
    ws, mean0, var0 = transfer_tensors(r, rng)
    cat, an, cr, ar = transfer_rows(r, rng, form, b)
    y = r.inp("y", normal(rng, b))
    sw = r.inp("sample_weight", np.abs(normal(rng, b))) if form != "plain" else None
    drop = dropout_of(r, rate) if rate else None
    dloss = r.inp("dloss", np.array([0.75], np.float32))
    lib = _lib.load()
    cfg = transfer_cfg(torch.from_numpy(mean0).to(DEV), torch.from_numpy(var0).to(DEV), bn_batch, drop)
    fwd_ws = torch.zeros(int(lib.impnn_transfer_head_loss_workspace_floats(b)), device=DEV)
    saved = r.inp("saved", ops.transfer_head_loss_rows(cat, an, cr, ar, ws, cfg, y, fwd_ws, sample_weight=sw)[2])
    assert saved.numel() == lib.impnn_transfer_head_saved_floats(b, HF, HMX)
    need = int(lib.impnn_transfer_head_bwd_workspace_floats(b, HF, HMX))
    assert need > 0
    wsp = r.work("workspace", 4 * need)
    frozen = 2
    dw = [None if i == frozen else r.out(f"dw{i}", w.numel() * 4, fill=0) for i, w in enumerate(ws)]
    lam = (C.c_float * 18)(*cfg["l2"])

    def want():
        g = [None if i == frozen else torch.zeros_like(w) for i, w in enumerate(ws)]
        ops.transfer_head_loss_rows_bwd(cat, an, cr, ar, ws, g, cfg, y, dloss, saved, sample_weight=sw)
        return {f"dw{i}": t for i, t in enumerate(g) if t is not None}
    r.want = want
    dargs = drop.args() if drop else (0.0, C.c_uint64(0), None, 0)
    mid = [r.table(ws), r.table([d if d is not None else 0 for d in dw]), lam, int(bn_batch), P(y)]
    tail = [cfg["loss_kind"], cfg["delta"], P(dloss), *dargs, P(saved), saved.numel() - (short == "saved"), wsp.ptr,
            need - (short == "workspace")]
    if form == "rows":
        return lib.impnn_transfer_head_loss_rows_bwd(P(cat), P(an), P(cr), P(ar), *mid, P(sw), *tail, b, cat.shape[0],
                                                     an.shape[0], HD, HF, HMX, S())
    pooled = [r.out("dpooled_cat", b * HD * 4), r.out("dpooled_an", b * HD * 4)]
    if form == "weighted":
        return lib.impnn_weighted_transfer_head_loss_bwd(P(cat), P(an), *mid, P(sw), *tail, *pooled, b, HD, HF, HMX, S())
    return lib.impnn_transfer_head_loss_bwd(P(cat), P(an), *mid, *tail, *pooled, b, HD, HF, HMX, S())


def lr_schedule_eval(r, _, short):
    """A piecewise-constant schedule: the rate is one of the record's float32 values, so the host's closed form
    (train.PiecewiseConstantDecay.__call__, which shares no code with the kernel) gives its bits."""
    sched = train.PiecewiseConstantDecay([3, 10, 11, 40], [1e-2, 3e-3, 7e-4, 1e-4, 5e-5])
    rec = r.inp("record", sched._record())
    host_steps = np.array([0, 1, 3, 4, 9, 10, 11, 12, 39, 40, 41, 1000, 2 ** 33], np.int64)
    steps = r.inp("steps", host_steps)
    n = len(host_steps)
    r.want = lambda: {"out": torch.tensor([sched(int(t)) for t in host_steps], dtype=torch.float32)}
    return _lib.load().impnn_lr_schedule_eval(P(rec), P(steps), r.out("out", 4 * n), n, S())


TL = [(f, b, bn, rate) for f in ("plain", "weighted", "rows") for b in HEAD_B for bn, rate in ((False, 0.0), (True, 0.25))]
HEAD_CASES = (
    [(model_head, (f, k, b)) for f in ("packed", "tensors", "mix") for k in (0, 1) for b in HEAD_B]
    + [(model_head_bwd, (f, k, b)) for f in ("plain", "loss", "weighted") for k in (0, 1) for b in HEAD_B]
    + [(model_head_loss, (w, k, b), (w, k, 70), ("workspace",)) for w in (False, True) for k in (0, 1) for b in HEAD_B]
    + [(transfer_inference, (f, b)) for f in ("head", "half") for b in HEAD_B]
    + [(transfer_inference, ("image", 1), None, ("image",))]
    + [(transfer_loss, p, (p[0], 70, p[2], p[3]), ("saved", "workspace")) for p in TL]
    + [(transfer_loss_bwd, p, (p[0], 70, p[2], p[3]), ("saved", "workspace")) for p in TL]
    + [(lr_schedule_eval, 0)])


@pytest.mark.parametrize("case", HEAD_CASES, ids=case_id)
def test_heads(case):
    check_case(*case)


# ---------------------------------------------------------------- the ensemble and the MC-dropout grid
GC, GA = 7, 37     # 37 anions: a second mask word, no multiple of a tile


def grid_operands(r, family, kind, GC):
    """-> ops.GridOperands of family 2 (ensemble, 3 members) or 3 (transfer MC, 3 samples) on this run's inputs."""
    rng = rng_of(60, family, kind)
    if family == 2:
        M = 3
        tail = int(_lib.load().impnn_ensemble_grid_tail_floats(kind, HF, HMX))
        T = r.inp("temperatures", np.array([273.15, 333.0], np.float32)) if kind == 0 else None
        return ops.ensemble_grid_operands(KIND_NAMES[kind], r.inp("mix_cat", np.abs(normal(rng, M, GC, HMX))),
                                          r.inp("mix_an", np.abs(normal(rng, M, GA, HMX))), T,
                                          r.inp("tails", rng.uniform(-0.4, 0.4, size=(M, tail)).astype(np.float32)), HF, HMX,
                                          kappa=1.5)
    ws, mean, var = transfer_tensors(r, rng)
    cfg = transfer_cfg(r.inp("moving_mean", mean), r.inp("moving_var", var))
    image = r.inp("image", ops.transfer_grid_prepare(ws, cfg))
    mult = r.inp("multipliers", (rng.random((3, 128)) >= 0.25).astype(np.float32) / np.float32(0.75))
    return ops.transfer_mc_grid_operands(r.inp("u_cat", normal(rng, GC, 256)), r.inp("u_an", normal(rng, GA, 256)), image,
                                         mult, kappa=1.5)


GRID_ENTRIES = {(2, "values"): "impnn_ensemble_grid", (2, "mask"): "impnn_ensemble_grid_mask",
                (2, "topk"): "impnn_ensemble_grid_topk", (2, "topk_where"): "impnn_ensemble_grid_topk_where",
                (3, "mask"): "impnn_transfer_mc_grid_mask", (3, "topk"): "impnn_transfer_mc_grid_topk",
                (3, "topk_where"): "impnn_transfer_mc_grid_topk_where"}


def grid_entry(r, p, short):
    """op "values" (impnn_ensemble_grid), "mask", "topk", "topk_where" of the two families: p = (family, kind, op)."""
    family, kind, op = p[:3]
    GC = p[3] if len(p) > 3 else globals()["GC"]     # (the larger grid whose leftover workspace a case starts from)
    g = grid_operands(r, family, kind, GC)
    lib = _lib.load()
    planes = max(g.nT, 1)
    fn = getattr(lib, GRID_ENTRIES[family, op])
    if op == "values":
        n = GC * GA * planes * 4
        r.want = lambda: dict(zip(("mean", "std", "score"), ops.grid_values(g)))
        return fn(*g.lead, r.out("mean", n), r.out("std", n), r.out("score", n), *g.trail, S())
    W = int(lib.impnn_grid_mask_row_words(GA))
    if op == "mask":
        r.want = lambda: {"words": ops.grid_mask(g, -0.25, 0.5)}
        return fn(*g.lead, -0.25, 0.5, r.out("words", planes * GC * W * 4), *g.trail, S())
    k, wgs = 5, 3
    need = C.c_size_t(0)
    if family == 2:
        _lib.check(lib.impnn_ensemble_grid_topk_workspace_bytes(g.members, GC, GA, g.nT, k, wgs, C.byref(need)))
    else:
        _lib.check(lib.impnn_transfer_mc_grid_topk_workspace_bytes(g.samples, GC, GA, k, wgs, C.byref(need)))
    assert need.value > 0
    ws = r.work("workspace", need.value)
    where = None
    if op == "topk_where":
        b = rng_of(61).random((GC, GA)) < 0.4
        words = np.zeros((GC, W), np.uint32)
        for j in range(GA):
            words[:, j >> 5] |= b[:, j].astype(np.uint32) << np.uint32(j & 31)
        where = r.inp("where", words.view(np.int32))
    r.want = lambda: dict(zip(("values", "cation", "anion"), ops.grid_topk(g, k, largest=True, workgroups=wgs, where=where)))
    outs = [r.out(nm, planes * k * 4) for nm in ("values", "cation", "anion")]
    return fn(*g.lead, *(() if where is None else (P(where),)), k, 1, *outs, ws.ptr, need.value - (short == "workspace"),
              *g.trail, wgs, S())


GRID_CASES = ([(grid_entry, (2, kind, "values")) for kind in (0, 1)]
              + [(grid_entry, (f, kind, "mask")) for f, kind in ((2, 0), (2, 1), (3, 1))]
              + [(grid_entry, (f, kind, op), (f, kind, op, 40), ("workspace",)) for f, kind in ((2, 0), (2, 1), (3, 1))
                 for op in ("topk", "topk_where")])


@pytest.mark.parametrize("case", GRID_CASES, ids=case_id)
def test_ensemble_and_mc_grids(case):
    check_case(*case)
