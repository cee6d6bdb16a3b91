"""Autograd nodes of the layer-at-a-time path: each forward is the libimpnn entry of
the reference layer, each backward the matching ``impnn_*_bwd`` entry (csrc/layer_adjoints.hip,
bond_matrices_train.hip, gated_update_bwd.hip; the message adjoint and its edge sort: csrc/message_typed.hip).
``ops.*`` routes through these nodes whenever an input requires grad and grad mode is on; with no grad
the calls are the plain forward entries.  torch.autograd only keeps the graph - no torch op computes here.
A model's training pass uses the larger nodes at the end of this file (a batch-32 step is bound by the number of
launches): BondTypeMatricesAll (every layer's type matrices), MessagePassingStep (message -> Reduce -> GatedUpdate)
and ModelHeadLoss (head + mse + l2 penalties); the per-layer nodes serve the drop-in layers called one by one.
The message nodes take the ion's ``ops.IonGraph`` of the pass: their forwards and backwards share its edge sort by
bond type and its message buffer, which live as long as the autograd graph that holds them."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, ops
from ._lib import check, f32c, i32c, ptr, stream_ptr


def _sink(param):
    """The existing gradient buffer of a leaf parameter, when a backward kernel may add into it directly
    (float32, contiguous, same device): ionic_mpnn_amd.train.Adam keeps every .grad as a view of one flat buffer.
    Returning None for that input afterwards tells autograd there is nothing left to accumulate."""
    g = getattr(param, "grad", None)
    if g is None or not param.is_leaf or g.dtype != torch.float32 or not g.is_contiguous() or g.device != param.device:
        return None
    return g


def _lib_call(device, fn, *args):
    with torch.cuda.device(device):
        check(fn(*args, stream_ptr()))


def restrict_rows(table, rows):
    """Marks an embedding table (a leaf tensor) as row-restricted: its backward nodes then produce the gradient of the
    listed rows only and +0.0 in every other row (impnn_embed_rows_bwd).  ``rows``: sorted, duplicate-free ids inside
    the table (layers.Embedding.trainable_rows), or None to clear the mark.  The list becomes an int32 tensor on the
    table's device that lives until the mark is cleared or replaced, so a captured step may read it on every replay;
    MPNNModel.compile() sets and clears it.  A tensor without the mark behaves as it always did."""
    table._impnn_rows = None if rows is None else torch.tensor(list(rows), dtype=torch.int32, device=table.device)


def _listed_rows(table):
    return getattr(table, "_impnn_rows", None)


def _listed_rows_grad(table, rows, ids, dout, to_sink=True):
    """The row-restricted gradient of ``table`` from ``dout`` (one row per id; ids None: dout is a full (V,dim) gradient
    and row r belongs to token r): added into the table's sink, or (no sink, or ``to_sink`` false) returned as a dense
    tensor that is +0.0 outside the list.  -> what the node returns for the table.
    The kernel adds without atomics, so two calls that add into one sink must run in stream order: a model's nodes that
    do so sit on one stream (MPNNModel._encode_two_streams looks both ions' atoms up ahead of the fork)."""
    V, dim = table.shape
    sink = _sink(table) if to_sink else None
    dtable = sink if sink is not None else torch.zeros(V, dim, dtype=torch.float32, device=dout.device)
    buffers = (C.c_void_p * 1)(dtable.data_ptr())
    _lib_call(dout.device, _lib.load().impnn_embed_rows_bwd, None if ids is None else ptr(ids), ptr(dout), ptr(rows),
              rows.numel(), buffers, V if ids is None else ids.numel(), V, dim, 1 if sink is not None else 0)
    return None if sink is not None else dtable


class EmbedGather(torch.autograd.Function):
    """Embedding lookup (train_viscosity.py:171-172)."""

    @staticmethod
    def forward(ctx, ids, table):
        ids = i32c(ids)
        ctx.save_for_backward(ids, table)
        return ops.embed_gather(ids, table)

    @staticmethod
    def backward(ctx, dout):
        ids, table = ctx.saved_tensors
        V, dim = table.shape
        rows = _listed_rows(table)
        if rows is not None:
            return None, _listed_rows_grad(table, rows, ids, f32c(dout))
        sink = _sink(table)  # the kernel accumulates (atomics): add straight into the gradient buffer
        dtable = sink if sink is not None else torch.zeros(V, dim, dtype=torch.float32, device=dout.device)
        dout = f32c(dout)
        _lib_call(dout.device, _lib.load().impnn_embed_gather_bwd, ptr(ids), ptr(dout), ptr(dtable), ids.numel(), V, dim)
        return None, (None if sink is not None else dtable)


class BondTypeMatrices(torch.autograd.Function):
    """A[v] = sum_k Tb[v,k] W[k] (models/layers.py:108, once per vocabulary entry)."""

    @staticmethod
    def forward(ctx, bond_table, W):
        bond_table, W = f32c(bond_table), f32c(W)
        ctx.save_for_backward(bond_table, W)
        return ops.bond_type_matrices(bond_table, W)

    @staticmethod
    def backward(ctx, dmats):
        bond_table, W = ctx.saved_tensors
        Vb, K = bond_table.shape
        D = W.shape[-1]
        dmats = f32c(dmats)
        sw, st = _sink(W), _sink(bond_table)
        rows = _listed_rows(bond_table)
        if rows is not None:
            # a row-restricted table: the full table gradient goes to a scratch buffer, its listed rows from there
            # into the sink where the layer's dW goes to its own (K < 64), else into a dense gradient that is +0.0
            # elsewhere and that autograd adds up, as it does this node's unrestricted dtb: a model keeps one such node
            # per layer and ion, on two streams, and the row kernel adds into a sink without atomics
            direct = sw is not None and K < 64  # (the kernel then ADDS into both outputs: the scratch starts at zero)
            dW = sw if direct else torch.empty_like(W)
            dtb = torch.zeros_like(bond_table) if direct else torch.empty_like(bond_table)
            _lib_call(W.device, _lib.load().impnn_bond_type_matrices_bwd, ptr(bond_table), ptr(W), ptr(dmats), ptr(dW),
                      ptr(dtb), Vb, K, D, 1 if direct else 0)
            return _listed_rows_grad(bond_table, rows, None, dtb, to_sink=direct), (None if direct else dW)
        if sw is not None and st is not None and K < 64:
            _lib_call(W.device, _lib.load().impnn_bond_type_matrices_bwd, ptr(bond_table), ptr(W), ptr(dmats), ptr(sw),
                      ptr(st), Vb, K, D, 1)
            return None, None
        dW, dtb = torch.empty_like(W), torch.empty_like(bond_table)
        _lib_call(W.device, _lib.load().impnn_bond_type_matrices_bwd, ptr(bond_table), ptr(W), ptr(dmats), ptr(dW),
                  ptr(dtb), Vb, K, D, 0)
        return dtb, dW


class BondTypeMatricesAll(torch.autograd.Function):
    """The type matrices of all message layers (both ions, every step) as one node: one forward launch, two backward
    launches (impnn_bond_type_matrices_multi[_bwd]) instead of three per layer.  Returns the n matrices and, as a
    non-differentiable last output, their gradient pool (n,Vb,D,D), zeroed for all layers at once (None without grad):
    MessagePassingStep adds each layer's type-matrix gradient into its slice and hands that slice back here."""

    @staticmethod
    def forward(ctx, bond_table, *Ws):
        bond_table = f32c(bond_table)
        Ws = tuple(f32c(W) for W in Ws)
        Vb, K = bond_table.shape
        D = Ws[0].shape[-1]
        outs = tuple(torch.empty(Vb, D, D, dtype=torch.float32, device=bond_table.device) for _ in Ws)
        wt = (C.c_void_p * len(Ws))(*[W.data_ptr() for W in Ws])
        ot = (C.c_void_p * len(Ws))(*[o.data_ptr() for o in outs])
        _lib_call(bond_table.device, _lib.load().impnn_bond_type_matrices_multi, ptr(bond_table), wt, ot, len(Ws), Vb, K, D)
        ctx.save_for_backward(bond_table, *Ws)
        pool = None
        if any(W.requires_grad for W in Ws) or bond_table.requires_grad:
            pool = torch.zeros(len(Ws), Vb, D, D, dtype=torch.float32, device=bond_table.device)  # one fill per step
            ctx.mark_non_differentiable(pool)
        ctx.set_materialize_grads(False)  # (no zero fill for the pool's gradient; a missing dmats is filled below)
        return (*outs, pool)

    @staticmethod
    def backward(ctx, *dmats):
        bond_table, *Ws = ctx.saved_tensors
        Vb, K = bond_table.shape
        D = Ws[0].shape[-1]
        dmats = [f32c(d) if d is not None else torch.zeros(Vb, D, D, dtype=torch.float32, device=bond_table.device)
                 for d in dmats[:-1]]
        sinks = [_sink(W) for W in Ws]
        st = _sink(bond_table)
        # a frozen bond embedding (no gradient asked for): the kernel's table gradient goes to a scratch buffer and
        # the layers' dW still go straight into their sinks
        frozen_table = not ctx.needs_input_grad[0]
        # a row-restricted table takes the frozen table's path - its full gradient goes to a scratch buffer, which the
        # adding form of the kernel needs zeroed - and its listed rows go from there to the sink or a dense gradient
        rows = None if frozen_table else _listed_rows(bond_table)
        if rows is not None:
            # (the table's gradient needs every layer's matrices, frozen layers included: a frozen layer's dW goes to a
            #  scratch buffer as a frozen table's gradient does, so the trained layers keep their sinks)
            use_sinks = all(sk is not None or not ctx.needs_input_grad[1 + j] for j, sk in enumerate(sinks))
            dWs = [sk if use_sinks and sk is not None else torch.empty_like(W) for sk, W in zip(sinks, Ws)]
            dtb = torch.zeros_like(bond_table) if use_sinks else torch.empty_like(bond_table)
        else:
            use_sinks = (st is not None or frozen_table) and all(sk is not None for sk in sinks)
            dWs = sinks if use_sinks else [torch.empty_like(W) for W in Ws]
            dtb = st if use_sinks and st is not None else torch.empty_like(bond_table)
        n = len(Ws)
        wt = (C.c_void_p * n)(*[W.data_ptr() for W in Ws])
        dt = (C.c_void_p * n)(*[d.data_ptr() for d in dmats])
        gt = (C.c_void_p * n)(*[g.data_ptr() for g in dWs])
        lib = _lib.load()
        wsn = int(lib.impnn_bond_type_matrices_multi_bwd_workspace_floats(n, Vb, K, D))
        ws = torch.empty(max(wsn, 1), dtype=torch.float32, device=bond_table.device)
        _lib_call(bond_table.device, lib.impnn_bond_type_matrices_multi_bwd_ws, ptr(bond_table), wt, dt, gt, ptr(dtb),
                  n, Vb, K, D, 1 if use_sinks else 0, ptr(ws), wsn)
        if rows is not None:
            return (_listed_rows_grad(bond_table, rows, None, dtb), *((None,) * n if use_sinks else dWs))
        if use_sinks:
            return (None,) * (n + 1)
        return (None if frozen_table else dtb, *dWs)


def _message_adjoint(entry, graph, h, bond_ids, conn, mats, grad, dh, dmats, scratch=None):
    """One message-adjoint launch (``entry``: an impnn_*_bwd name) that ADDS into dh and dmats, on the edge sort of
    the ion's graph - sorted by an earlier message call of the pass, or by this one."""
    B, N, D = h.shape
    E, Vb = conn.shape[1], mats.shape[0]
    ws, ready = (graph or ops.IonGraph(None, bond_ids, conn, Vb)).edge_sort()
    _lib_call(h.device, getattr(_lib.load(), entry), ptr(h), ptr(bond_ids), ptr(conn), ptr(mats), ptr(grad), ptr(dh),
              ptr(dmats), ptr(ws), ws.numel(), *(() if scratch is None else (ptr(scratch),)), B, N, E, D, Vb,
              1 if ready else 0)


def _message_node_backward(entry, ctx, grad):
    """The backward of the two message nodes below: (dh, dmats) of ``entry`` for the node's five inputs."""
    h, bond_ids, conn, mats = ctx.saved_tensors
    both = torch.zeros(h.numel() + mats.numel(), dtype=torch.float32, device=h.device)  # one fill for both sums
    dh, dmats = both[:h.numel()].view_as(h), both[h.numel():].view_as(mats)
    _message_adjoint(entry, ctx.graph, h, bond_ids, conn, mats, f32c(grad), dh, dmats)
    return dh, None, None, dmats, None


class BmmMessageTyped(torch.autograd.Function):
    """BondMatrixMessage.call in the per-bond-type schedule (models/layers.py:100-117)."""

    @staticmethod
    def forward(ctx, h, bond_ids, conn, type_mats, graph=None):
        h, type_mats, bond_ids, conn = f32c(h), f32c(type_mats), i32c(bond_ids), i32c(conn)
        ctx.save_for_backward(h, bond_ids, conn, type_mats)
        ctx.graph = graph
        return ops.bmm_message_typed(h, bond_ids, conn, type_mats, graph)

    @staticmethod
    def backward(ctx, dm):
        return _message_node_backward("impnn_bmm_message_typed_bwd", ctx, dm)


class MessageReduceTyped(torch.autograd.Function):
    """Reduce o BondMatrixMessage as one node (models/layers.py:100-117 then :57-83): the forward runs the two entries
    and keeps no messages; the backward reads the aggregate's gradient at every edge's target row
    (impnn_message_reduce_typed_bwd), so neither the (B,E,D) messages nor their gradient outlive the forward."""

    @staticmethod
    def forward(ctx, h, bond_ids, conn, type_mats, graph=None):
        h, type_mats, bond_ids, conn = f32c(h), f32c(type_mats), i32c(bond_ids), i32c(conn)
        ctx.save_for_backward(h, bond_ids, conn, type_mats)
        ctx.graph = graph
        m = ops.bmm_message_typed(h, bond_ids, conn, type_mats, graph)
        return ops.reduce_scatter_add(m, conn[:, :, 1], h.shape[1])

    @staticmethod
    def backward(ctx, dagg):
        return _message_node_backward("impnn_message_reduce_typed_bwd", ctx, dagg)


class ReduceScatterAdd(torch.autograd.Function):
    """Reduce.call (models/layers.py:57-83)."""

    @staticmethod
    def forward(ctx, messages, tgt_idx, num_atoms):
        tgt = i32c(tgt_idx)
        ctx.save_for_backward(tgt)
        ctx.num_atoms = int(num_atoms)
        return ops.reduce_scatter_add(messages, tgt, num_atoms)

    @staticmethod
    def backward(ctx, dagg):
        (tgt,) = ctx.saved_tensors
        B, E = tgt.shape
        dagg = f32c(dagg)
        D = dagg.shape[-1]
        dm = torch.empty(B, E, D, dtype=torch.float32, device=dagg.device)
        _lib_call(dagg.device, _lib.load().impnn_reduce_scatter_bwd, ptr(dagg), ptr(tgt), 1, ptr(dm), B, ctx.num_atoms, E, D)
        return dm, None, None


class GatedUpdate(torch.autograd.Function):
    """GatedUpdate.call (models/layers.py:142-156); ``dropout``: an ops.Dropout whose mask the backward regenerates."""

    @staticmethod
    def forward(ctx, h, agg, Wz, bz, Wr, br, Wh, bh, gamma, beta, eps, *dropout):
        ts = [f32c(t) for t in (h, agg, Wz, bz, Wr, br, Wh, bh, gamma)]
        ctx.save_for_backward(*ts, beta)
        ctx.eps = float(eps)
        ctx.extra = len(dropout)  # (0 or 1: the node's inputs, so its gradients, end with eps or with the dropout)
        ctx.dropout = dropout[0] if dropout else None
        return ops.gated_update(*ts, beta, eps, dropout=ctx.dropout)

    @staticmethod
    def backward(ctx, dout):
        return _gated_update_backward(ctx.saved_tensors, ctx.eps, dout, dropout=ctx.dropout) + (None,) * ctx.extra


def _gated_update_backward(saved, eps, dout, row_list=None, kept=None, unlisted_undefined=False, dropout=None):
    """(dh, dagg, 8 parameter gradients or None where the kernel added into the sink, None for eps).
    row_list = (row_index, n_rows) of ops.kept_row_index: gradients of those rows only (impnn_gated_update_rows_bwd);
    dh is zero elsewhere (padding atoms carry no gradient), dagg is undefined there and never read.
    kept: the buffer the training forward filled (ops.gated_update(.., save=True)) - the backward then skips its
    recompute passes (impnn_gated_update_rows_bwd_saved) and overwrites the buffer.
    dropout: the forward's ops.Dropout (rate > 0) - the *_dropout entries read dout through its mask."""
    h, agg, Wz, bz, Wr, br, Wh, bh, gamma, beta = saved
    D = h.shape[-1]
    rows = h.numel() // D
    lib = _lib.load()
    dout = f32c(dout)
    dh = torch.zeros_like(h) if row_list is not None and not unlisted_undefined else torch.empty_like(h)
    dagg = torch.empty_like(agg)
    P = int(lib.impnn_gated_update_param_floats(D))
    if row_list is not None or (kept is not None and D != 32):
        wsn = int(lib.impnn_gated_update_rows_bwd_workspace_floats(rows, D))
    else:
        wsn = int(lib.impnn_gated_update_bwd_workspace_floats(rows, D))
    ws = torch.empty(max(wsn, 1), dtype=torch.float32, device=h.device)


    def call(dparams, accumulate):
        entry, tail = _gated_update_bwd_entry(lib, row_list, kept, dropout, rows, D, accumulate)
        _lib_call(h.device, entry, ptr(h), ptr(agg), ptr(Wz), ptr(bz), ptr(Wr), ptr(br), ptr(Wh), ptr(bh), ptr(gamma),
                  eps, ptr(dout), ptr(dh), ptr(dagg), ptr(dparams), ptr(ws), wsn, *tail)
    # the eight parameter gradients leave the kernel as one block in the canonical order; when the existing
    # .grad buffers form exactly that block (train.Adam's flat buffer does), the kernel adds into it directly
    params = (Wz, bz, Wr, br, Wh, bh, gamma, beta)
    sinks = [_sink(t) for t in params]
    direct = all(g is not None for g in sinks)
    if direct:
        base, off = sinks[0].data_ptr(), 0
        for t, g in zip(params, sinks):
            direct = direct and g.data_ptr() == base + 4 * off and g.numel() == t.numel()
            off += t.numel()
    if direct:
        call(sinks[0], 1)
        return (dh, dagg, *([None] * 8), None)
    dparams = torch.empty(P, dtype=torch.float32, device=h.device)
    call(dparams, 0)
    n_w, o = 2 * D * D, 0
    grads = []
    for _ in range(3):
        grads.append(dparams[o:o + n_w].view(2 * D, D))
        grads.append(dparams[o + n_w:o + n_w + D])
        o += n_w + D
    grads.append(dparams[o:o + D])
    grads.append(dparams[o + D:o + 2 * D])
    return (dh, dagg, *grads, None)


def _gated_update_bwd_entry(lib, row_list, kept, dropout, max_rows, D, accumulate):
    """(row list?, kept?, dropout?) -> the backward entry and its arguments between the workspace size and the stream.
    A ``dropout`` of rate 0 takes the plain entry."""
    ri, rn = (ptr(row_list[0]), ptr(row_list[1])) if row_list is not None else (None, None)
    d = dropout.args() if dropout is not None and dropout.rate > 0.0 else ()
    if kept is not None:
        entry = lib.impnn_gated_update_rows_bwd_saved_dropout if d else lib.impnn_gated_update_rows_bwd_saved
        return entry, (ri, rn, max_rows, D, accumulate, ptr(kept), *d)
    if row_list is not None:
        entry = lib.impnn_gated_update_rows_bwd_dropout if d else lib.impnn_gated_update_rows_bwd
        return entry, (ri, rn, max_rows, D, accumulate, *d)
    return (lib.impnn_gated_update_bwd_dropout if d else lib.impnn_gated_update_bwd), (max_rows, D, accumulate, *d)


# edge slots per ion from which the message adjoint writes per-edge vectors and sums them in slot order instead of adding
# into dh with float atomics (impnn_message_reduce_typed_bwd_scratch): 15.5 -> 14.4 ms per step at batch 4096, 2.25 -> 1.89
# ms at batch 256; at the reference's batch 32 the second launch costs more than the atomics (1.13 -> 1.19 ms)
MESSAGE_BWD_EDGE_BUFFER_MIN_SLOTS = 8192


class MessagePassingStep(torch.autograd.Function):
    """One message-passing step as one node (train_viscosity.py:179-186: BondMatrixMessage -> Reduce -> GatedUpdate).
    Backward: impnn_gated_update_bwd writes dh and dagg, then impnn_message_reduce_typed_bwd ADDS the message path's
    share into the same dh - no separate sum of the two consumers of h, no zero fill of dh.  ``graph``: the ion's
    ops.IonGraph of this pass (edge sort and message buffer shared with the ion's other steps); ``dmats``: this
    layer's slice of BondTypeMatricesAll's gradient pool, where the type-matrix gradient goes when there is one."""

    @staticmethod
    def forward(ctx, h, bond_ids, conn, type_mats, Wz, bz, Wr, br, Wh, bh, gamma, beta, eps, graph, dmats=None,
                row_index=None, n_rows=None, inner=False, dropout=None):
        """row_index / n_rows (ops.kept_row_index; atom_dim 64 / 128): GatedUpdate forward and backward on the kept rows
        only - padding atoms reach neither a message nor the pool, so their rows of the output are left undefined
        and their gradient is zero (include/impnn.h, impnn_gated_update_rows[_bwd]).
        dropout: an ops.Dropout of this layer and pass (training) - fused into the GatedUpdate forward and backward."""
        h, type_mats, bond_ids, conn = f32c(h), f32c(type_mats), i32c(bond_ids), i32c(conn)
        gu = [f32c(t) for t in (Wz, bz, Wr, br, Wh, bh, gamma)]
        # inner (with a row list): this step's input is the output of another MessagePassingStep on the SAME list - that
        # node reads its incoming gradient at the listed rows only, so the rows outside the list need no zero fill here
        ctx.inner = bool(inner) and row_index is not None
        # one message buffer per ion and pass (the Reduce behind each layer consumes it at once; at atom_dim 64 / 128
        # the message adjoint writes its per-edge vectors there)
        buf = graph.message_buffer(h.shape[-1]) if h.shape[-1] != 32 else None
        m = ops.bmm_message_typed(h, bond_ids, conn, type_mats, graph, out=buf)
        agg = ops.reduce_scatter_add(m, conn[:, :, 1], h.shape[1])
        del m
        ctx.row_list = (row_index, n_rows) if row_index is not None else None
        ctx.kept = None
        if h.shape[-1] in (64, 128) or (h.shape[-1] == 32 and ctx.row_list is None):
            # the gates, the candidate and r * h of the (kept) rows stay for the backward (4 D floats per row and step)
            # instead of being recomputed there with half of its matrix work
            out, ctx.kept = ops.gated_update(h, agg, *gu, beta, eps, rows=ctx.row_list, save=True, dropout=dropout)
        else:
            out = ops.gated_update(h, agg, *gu, beta, eps, rows=ctx.row_list, dropout=dropout)
        ctx.dropout = dropout
        ctx.save_for_backward(h, agg, *gu, beta, bond_ids, conn, type_mats)
        ctx.eps = float(eps)
        ctx.graph, ctx.dmats = graph, dmats
        return out

    @staticmethod
    def backward(ctx, dout):
        saved = ctx.saved_tensors
        h, bond_ids, conn, mats = saved[0], saved[10], saved[11], saved[12]
        kept = ctx.kept
        if kept is not None:
            if kept is False:
                raise RuntimeError("MessagePassingStep: the kept activations were consumed by an earlier backward "
                                   "(run the forward again instead of retain_graph)")
            ctx.kept = False
        dh, dagg, *dparams = _gated_update_backward(saved[:10], ctx.eps, dout, ctx.row_list, kept, ctx.inner,
                                                    ctx.dropout)
        del kept
        B, N, D = h.shape
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[3]):
            # the lowest trained step with a frozen message layer: neither h nor the type matrices take a gradient
            return (None, None, None, None, *dparams) + (None,) * 6
        dmats = ctx.dmats if ctx.dmats is not None else torch.zeros_like(mats)
        scratch = None
        # (atom_dim 32: measured slower that way - 1.71 -> 1.88 ms per step at batch 4096 - the rows are a quarter as
        #  long, the atomics a quarter as many, and the buffer's round trip through HBM costs the same launch)
        if D in (64, 128) and B * conn.shape[1] >= MESSAGE_BWD_EDGE_BUFFER_MIN_SLOTS:
            # the forward's message buffer of this ion and pass: zero rows at masked edges, free since the Reduce
            scratch = ctx.graph.written_message_buffer(D)
        entry = "impnn_message_reduce_typed_bwd" if scratch is None else "impnn_message_reduce_typed_bwd_scratch"
        _message_adjoint(entry, ctx.graph, h, bond_ids, conn, mats, dagg, dh, dmats, scratch)
        return (dh, None, None, dmats, *dparams) + (None,) * 6


class GlobalSumPool(torch.autograd.Function):
    """GlobalSumPool.call (models/layers.py:161-164)."""

    @staticmethod
    def forward(ctx, h, atom_ids):
        ids = i32c(atom_ids)
        ctx.save_for_backward(ids)
        ctx.D = int(h.shape[-1])
        return ops.global_sum_pool(h, ids)

    @staticmethod
    def backward(ctx, dp):
        (ids,) = ctx.saved_tensors
        B, N = ids.shape
        dp = f32c(dp)
        dh = torch.empty(B, N, ctx.D, dtype=torch.float32, device=dp.device)
        _lib_call(dp.device, _lib.load().impnn_global_sum_pool_bwd, ptr(dp), ptr(ids), ptr(dh), B, N, ctx.D)
        return dh, None


class ModelHead(torch.autograd.Function):
    """Everything after GlobalSumPool as one node (SURVEY.md 8 f1 + f4): forward impnn_model_head_tensors, backward
    impnn_model_head_bwd, both reading the individual Dense kernels/biases (train_viscosity.py:189-214 /
    train_melting_point.py:173-198)."""

    @staticmethod
    def forward(ctx, kind, fp_size, mixing_size, pooled_cat, pooled_an, temperature, *weights):
        pooled_cat, pooled_an = f32c(pooled_cat), f32c(pooled_an)
        weights = tuple(f32c(w) for w in weights)
        B, D = pooled_cat.shape
        T = f32c(temperature).reshape(-1) if kind == 0 else None
        if T is not None and T.numel() != B:
            raise ValueError("temperature must hold one value per sample")
        out = torch.empty(B, 1, dtype=torch.float32, device=pooled_cat.device)
        table = (C.c_void_p * len(weights))(*[w.data_ptr() for w in weights])
        _lib_call(pooled_cat.device, _lib.load().impnn_model_head_tensors, kind, ptr(pooled_cat), ptr(pooled_an),
                  ptr(T) if T is not None else None, table, ptr(out), B, D, fp_size, mixing_size)
        ctx.save_for_backward(pooled_cat, pooled_an, *(() if T is None else (T,)), *weights)
        ctx.meta = (kind, fp_size, mixing_size, weights)
        return out

    @staticmethod
    def backward(ctx, dout):
        kind, F, Mx, params = ctx.meta
        saved = ctx.saved_tensors
        pooled_cat, pooled_an = saved[0], saved[1]
        T = saved[2] if kind == 0 else None
        weights = saved[3 if kind == 0 else 2:]
        B, D = pooled_cat.shape
        dout = f32c(dout).reshape(-1)
        sinks = [_sink(p) for p in params]
        grads = [s if s is not None else torch.zeros_like(w) for s, w in zip(sinks, weights)]
        dpc, dpa = torch.empty_like(pooled_cat), torch.empty_like(pooled_an)
        wt = (C.c_void_p * len(weights))(*[w.data_ptr() for w in weights])
        gt = (C.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
        _lib_call(dout.device, _lib.load().impnn_model_head_bwd, kind, ptr(pooled_cat), ptr(pooled_an),
                  ptr(T) if T is not None else None, wt, ptr(dout), ptr(dpc), ptr(dpa), gt, B, D, F, Mx)
        return (None, None, None, dpc, dpa, None) + tuple(None if s is not None else g for s, g in zip(sinks, grads))


class WeightedL2(tuple):
    """ModelHeadLoss's ``l2`` argument with the batch's per-sample weights attached: the lambdas as a tuple, the
    weights (a (B) float32 device tensor, or None) as ``.sample_weight``.  A plain sequence of lambdas is the unweighted
    loss.  ``pred``: a persistent (B) float32 device buffer that the loss kernel fills with the pass's predictions (the
    metrics of compile(metrics=...) read it); None, as from a plain sequence, passes the null pointer."""

    def __new__(cls, l2, sample_weight, pred=None):
        self = super().__new__(cls, l2)
        self.sample_weight = sample_weight
        self.pred = pred
        return self


def _sample_weight(w, B, device):
    """The weight tensor a loss node hands to the library: contiguous float32 (B) on the node's device, or None."""
    if w is None:
        return None
    w = f32c(w.detach()).reshape(-1)
    if w.numel() != B or w.device != device:
        raise ValueError("sample_weight must hold one value per sample, on the batch's device")
    return w


def _pred_buffer(pred, B, device):
    """The predictions' buffer a loss node hands to the library: contiguous float32 (B) on the node's device, or None."""
    if pred is None:
        return None
    if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.numel() != B or pred.device != device:
        raise ValueError("pred must be a contiguous float32 buffer of one value per sample, on the batch's device")
    return pred


def _table_rows(rows, cat_table, an_table):
    """The index pair an indexed loss node hands to the library: contiguous int32 (B) each on the tables' device, or
    None.  Their range is the caller's to check (data.FrozenEncodings does, on the host, when it is built)."""
    if rows is None:
        return None
    cat_row, an_row = rows
    for r in (cat_row, an_row):
        if r.dtype != torch.int32 or r.dim() != 1 or not r.is_contiguous() or r.device != cat_table.device:
            raise ValueError("cat_row / an_row must be contiguous 1-d int32 tensors on the tables' device")
    if cat_row.numel() != an_row.numel():
        raise ValueError("cat_row and an_row must hold one index per sample each")
    if cat_table.shape[0] < 1 or an_table.shape[0] < 1 or cat_table.shape[1] != an_table.shape[1]:
        raise ValueError("the tables need at least one row each and one width")
    return cat_row, an_row


class ModelHeadLoss(torch.autograd.Function):
    """Head + keras "mse" + l2 penalties as one node -> the scalar loss (impnn_model_head_loss[_bwd]).  ``l2``: one
    lambda per weight tensor; ``workspace``: a persistent float tensor whose first word is zero (the kernel's arrival
    counter; see include/impnn.h).  Per-sample weights ride in ``l2``: pass ``WeightedL2(l2, sample_weight)`` and the
    node calls impnn_weighted_model_head_loss[_bwd]: loss = (1/B) sum_b w_b (pred_b - y_b)^2 + penalties.  The weight
    is kept for the backward and gets no gradient."""

    @staticmethod
    def forward(ctx, kind, fp_size, mixing_size, l2, workspace, pooled_cat, pooled_an, temperature, y, *weights):
        pooled_cat, pooled_an, y = f32c(pooled_cat), f32c(pooled_an), f32c(y).reshape(-1)
        weights = tuple(f32c(w) for w in weights)
        B, D = pooled_cat.shape
        T = f32c(temperature).reshape(-1) if kind == 0 else None
        if y.numel() != B or (T is not None and T.numel() != B):
            raise ValueError("y / temperature must hold one value per sample")
        sw = _sample_weight(getattr(l2, "sample_weight", None), B, pooled_cat.device)
        pred = _pred_buffer(getattr(l2, "pred", None), B, pooled_cat.device)
        pp = None if pred is None else ptr(pred)
        lib = _lib.load()
        if workspace.numel() < lib.impnn_model_head_loss_workspace_floats(B):
            raise ValueError("loss workspace too small")
        loss = torch.empty((), dtype=torch.float32, device=pooled_cat.device)
        lam = (C.c_float * len(weights))(*[float(v) for v in l2])
        table = (C.c_void_p * len(weights))(*[w.data_ptr() for w in weights])
        if sw is None:
            _lib_call(pooled_cat.device, lib.impnn_model_head_loss, kind, ptr(pooled_cat), ptr(pooled_an),
                      ptr(T) if T is not None else None, table, lam, ptr(y), pp, ptr(loss), ptr(workspace),
                      workspace.numel(), B, D, fp_size, mixing_size)
        else:
            _lib_call(pooled_cat.device, lib.impnn_weighted_model_head_loss, kind, ptr(pooled_cat), ptr(pooled_an),
                      ptr(T) if T is not None else None, table, lam, ptr(y), ptr(sw), pp, ptr(loss), ptr(workspace),
                      workspace.numel(), B, D, fp_size, mixing_size)
        ctx.save_for_backward(pooled_cat, pooled_an, y, *(() if T is None else (T,)), *weights)
        ctx.meta = (kind, fp_size, mixing_size, tuple(float(v) for v in l2), weights)
        ctx.sample_weight = sw  # no gradient flows to it: kept beside the saved tensors
        return loss

    @staticmethod
    def backward(ctx, dloss):
        kind, F, Mx, l2, params = ctx.meta
        saved = ctx.saved_tensors
        pooled_cat, pooled_an, y = saved[0], saved[1], saved[2]
        T = saved[3] if kind == 0 else None
        weights = saved[4 if kind == 0 else 3:]
        B, D = pooled_cat.shape
        dloss = f32c(dloss).reshape(1)
        sinks = [_sink(p) for p in params]
        grads = [s if s is not None else torch.zeros_like(w) for s, w in zip(sinks, weights)]
        dpc, dpa = torch.empty_like(pooled_cat), torch.empty_like(pooled_an)
        lam = (C.c_float * len(weights))(*l2)
        wt = (C.c_void_p * len(weights))(*[w.data_ptr() for w in weights])
        gt = (C.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
        sw = ctx.sample_weight
        if sw is None:
            _lib_call(dloss.device, _lib.load().impnn_model_head_loss_bwd, kind, ptr(pooled_cat), ptr(pooled_an),
                      ptr(T) if T is not None else None, wt, lam, ptr(y), ptr(dloss), ptr(dpc), ptr(dpa), gt, B, D, F,
                      Mx)
        else:
            _lib_call(dloss.device, _lib.load().impnn_weighted_model_head_loss_bwd, kind, ptr(pooled_cat),
                      ptr(pooled_an), ptr(T) if T is not None else None, wt, lam, ptr(y), ptr(sw), ptr(dloss), ptr(dpc),
                      ptr(dpa), gt, B, D, F, Mx)
        return (None, None, None, None, None, dpc, dpa, None, None) + tuple(
            None if s is not None else g for s, g in zip(sinks, grads))



class TransferHeadLoss(torch.autograd.Function):
    """The transfer model's head + Huber / squared error + l2 penalties as one node -> the scalar loss
    (impnn_transfer_head_loss[_bwd]).  ``cfg``: MPNNModel._transfer_cfg (widths, l2, the moving statistics, which
    the forward moves in place when cfg["bn_batch"], the pass's ops.Dropout or None, the loss, and optionally
    cfg["sample_weight"]: (B) per-sample weights, which select impnn_weighted_transfer_head_loss[_bwd] and get no
    gradient, and cfg["pred"]: a (B) float32 buffer the forward fills with the pass's predictions);
    cfg["rows"] = (cat_row, an_row), (B) int32 device tensors: ``pooled_cat`` (C,D) / ``pooled_an`` (A,D) are tables of
    ion rows and sample b reads pooled_cat[cat_row[b]], pooled_an[an_row[b]] (impnn_transfer_head_loss_rows[_bwd]; the
    tables get no gradient: a trainable encoder is the plain form);
    ``workspace``: a persistent float tensor whose first word is zero.  The backward adds the gradients of the tensors that ask for one
    into their sinks and leaves the frozen ones alone; it writes the pooled vectors' gradients only when they ask."""

    @staticmethod
    def forward(ctx, cfg, workspace, pooled_cat, pooled_an, y, *weights):
        pooled_cat, pooled_an, y = f32c(pooled_cat), f32c(pooled_an), f32c(y).reshape(-1)
        weights = tuple(f32c(w) for w in weights)
        B, D = pooled_cat.shape
        rows = _table_rows(cfg.get("rows"), pooled_cat, pooled_an)
        if rows is not None:
            if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
                raise ValueError("the indexed transfer loss has no gradient for its tables")
            B = int(rows[0].numel())
        if y.numel() != B:
            raise ValueError("y must hold one value per sample")
        sw = _sample_weight(cfg.get("sample_weight"), B, pooled_cat.device)
        pred = _pred_buffer(cfg.get("pred"), B, pooled_cat.device)
        lib = _lib.load()
        F, Mx = cfg["fp_size"], cfg["mixing_size"]
        keep = any(ctx.needs_input_grad) or cfg["bn_batch"]
        n_saved = int(lib.impnn_transfer_head_saved_floats(B, F, Mx)) if keep else 0
        saved = torch.empty(n_saved, dtype=torch.float32, device=pooled_cat.device) if keep else None
        loss = torch.empty((), dtype=torch.float32, device=pooled_cat.device)
        lam = (C.c_float * len(weights))(*[float(v) for v in cfg["l2"]])
        table = (C.c_void_p * len(weights))(*[w.data_ptr() for w in weights])
        drop = cfg["dropout"]
        dargs = drop.args() if drop is not None and drop.rate > 0.0 else (0.0, C.c_uint64(0), None, 0)
        if rows is not None:
            _lib_call(pooled_cat.device, lib.impnn_transfer_head_loss_rows, ptr(pooled_cat), ptr(pooled_an),
                      ptr(rows[0]), ptr(rows[1]), table, lam, ptr(cfg["moving_mean"]), ptr(cfg["moving_variance"]),
                      cfg["momentum"], cfg["epsilon"], 1 if cfg["bn_batch"] else 0, ptr(y),
                      None if sw is None else ptr(sw), cfg["loss_kind"], cfg["delta"], *dargs,
                      ptr(saved) if keep else None, n_saved, None if pred is None else ptr(pred), ptr(loss),
                      ptr(workspace), workspace.numel(), B, pooled_cat.shape[0], pooled_an.shape[0], D, F, Mx)
        else:
            entry = lib.impnn_transfer_head_loss if sw is None else lib.impnn_weighted_transfer_head_loss
            _lib_call(pooled_cat.device, entry, ptr(pooled_cat), ptr(pooled_an), table, lam,
                      ptr(cfg["moving_mean"]), ptr(cfg["moving_variance"]), cfg["momentum"], cfg["epsilon"],
                      1 if cfg["bn_batch"] else 0, ptr(y), *(() if sw is None else (ptr(sw),)), cfg["loss_kind"],
                      cfg["delta"], *dargs, ptr(saved) if keep else None, n_saved, None if pred is None else ptr(pred),
                      ptr(loss), ptr(workspace),
                      workspace.numel(), B, D, F, Mx)
        ctx.save_for_backward(pooled_cat, pooled_an, y, *weights)
        ctx.meta = (cfg, saved, dargs, weights)
        ctx.rows = rows  # integer tensors: kept beside the saved tensors
        ctx.sample_weight = sw  # no gradient flows to it: kept beside the saved tensors
        return loss

    @staticmethod
    def backward(ctx, dloss):
        cfg, saved, dargs, params = ctx.meta
        pooled_cat, pooled_an, y, *weights = ctx.saved_tensors
        B, D = pooled_cat.shape
        rows = ctx.rows
        if rows is not None:
            B = int(rows[0].numel())
        F, Mx = cfg["fp_size"], cfg["mixing_size"]
        dloss = f32c(dloss).reshape(1)
        lib = _lib.load()
        wants = ctx.needs_input_grad[5:]
        sinks = [_sink(p) if w else None for p, w in zip(params, wants)]
        grads = [None if not w else (s if s is not None else torch.zeros_like(t))
                 for w, s, t in zip(wants, sinks, weights)]
        pooled = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        dpc = torch.empty_like(pooled_cat) if pooled else None
        dpa = torch.empty_like(pooled_an) if pooled else None
        wsn = int(lib.impnn_transfer_head_bwd_workspace_floats(B, F, Mx))
        ws = torch.empty(wsn, dtype=torch.float32, device=dloss.device)
        lam = (C.c_float * len(weights))(*[float(v) for v in cfg["l2"]])
        wt = (C.c_void_p * len(weights))(*[w.data_ptr() for w in weights])
        gt = (C.c_void_p * len(weights))(*[g.data_ptr() if g is not None else None for g in grads])
        sw = ctx.sample_weight
        if rows is not None:
            _lib_call(dloss.device, lib.impnn_transfer_head_loss_rows_bwd, ptr(pooled_cat), ptr(pooled_an), ptr(rows[0]),
                      ptr(rows[1]), wt, gt, lam, 1 if cfg["bn_batch"] else 0, ptr(y), None if sw is None else ptr(sw),
                      cfg["loss_kind"], cfg["delta"], ptr(dloss), *dargs, ptr(saved), saved.numel(), ptr(ws), wsn, B,
                      pooled_cat.shape[0], pooled_an.shape[0], D, F, Mx)
            return (None, None, None, None, None) + tuple(None if s is not None else g for s, g in zip(sinks, grads))
        entry = lib.impnn_transfer_head_loss_bwd if sw is None else lib.impnn_weighted_transfer_head_loss_bwd
        _lib_call(dloss.device, entry, ptr(pooled_cat), ptr(pooled_an), wt, gt, lam,
                  1 if cfg["bn_batch"] else 0, ptr(y), *(() if sw is None else (ptr(sw),)), cfg["loss_kind"],
                  cfg["delta"], ptr(dloss), *dargs, ptr(saved), saved.numel(), ptr(ws), wsn,
                  ptr(dpc) if pooled else None, ptr(dpa) if pooled else None, B, D, F, Mx)
        return (None, None, dpc, dpa, None) + tuple(None if s is not None else g for s, g in zip(sinks, grads))
