"""Functional wrappers: torch CUDA tensors in, torch CUDA tensors out, every one a libimpnn call on
the tensor's device and torch's current stream.  Shapes/dtypes follow the reference tensors
(int32 ids and connectivity, float32 state)."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
import torch

from . import _lib, data
from ._lib import check, f32c, i32c, ptr, require_gpu, stream_ptr

LN_EPS = 1e-3  # keras LayerNormalization default (models/layers.py:139)
DEBUG_VALIDATE = False  # True: raise like TF-CPU on out-of-range indices (costs a device sync)


def _wants_grad(*tensors):
    """Training: an input requires grad and grad mode is on -> go through ionic_mpnn_amd.autograd."""
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


class NoBackward(NotImplementedError):
    """Raised when a forward-only entry (dense bond_state message, fused encoder) is asked for gradients."""


def embed_gather(ids, table):
    """Embedding(mask_zero=False) lookup, train_viscosity.py:171-172."""
    if _wants_grad(table):
        from . import autograd
        return autograd.EmbedGather.apply(ids, table)
    require_gpu(ids, table)
    ids = i32c(ids)
    table = f32c(table)
    out = torch.empty(*ids.shape, table.shape[1], dtype=torch.float32, device=table.device)
    with torch.cuda.device(table.device):
        check(_lib.load().impnn_embed_gather(ptr(ids), ptr(table), ptr(out), ids.numel(), table.shape[0],
                                             table.shape[1], stream_ptr()))
    return out


def _check_bmm_shapes(h, conn):
    if h.dim() != 3:
        raise ValueError(f"atom_state must be (B,N,D), got {tuple(h.shape)}")
    if conn.dim() != 3 or conn.shape[-1] != 2 or conn.shape[0] != h.shape[0]:
        raise ValueError(f"connectivity must be (B,E,2) with the batch of atom_state, got {tuple(conn.shape)}")


def validate_indices(conn=None, atom_ids=None, bond_ids=None, N=None, Va=1 << 30, Vb=1 << 30):
    """Raises ValueError where tf-CPU's gather/scatter_nd would (models/layers.py:106,78-82)."""
    ref = conn if conn is not None else (atom_ids if atom_ids is not None else bond_ids)
    require_gpu(ref)
    B = ref.shape[0]
    E = conn.shape[1] if conn is not None else (bond_ids.shape[1] if bond_ids is not None else 0)
    Nn = N if N is not None else (atom_ids.shape[1] if atom_ids is not None else 1)
    counts = torch.zeros(3, dtype=torch.int32, device=ref.device)
    with torch.cuda.device(ref.device):
        check(_lib.load().impnn_validate_indices(
            ptr(i32c(conn)) if conn is not None else None,
            ptr(i32c(atom_ids)) if atom_ids is not None else None,
            ptr(i32c(bond_ids)) if bond_ids is not None else None,
            ptr(counts), B, Nn, E, Va, Vb, stream_ptr()))
    c = counts.tolist()
    if any(c):
        raise ValueError(f"out-of-range indices: connectivity={c[0]} atom_ids={c[1]} bond_ids={c[2]}")


def batch_assemble(sample_idx, ions, max_atoms, slots, id_shift=1, t_flat=None):
    """train_viscosity.py:291-314 build_inputs(idx) on the GPU (impnn_batch_assemble).

    ions: per ion a dict of resident int32 device tensors atom_flat, atom_off (M+1), edge_flat (n,2),
    bond_flat, edge_off (M+1).  Returns per ion (atom_ids (B,N), bond_ids (B,slots), conn (B,slots,2))
    and the gathered t (B,1) or None."""
    require_gpu(sample_idx, *[t for ion in ions for t in ion.values()])
    sample_idx = i32c(sample_idx)
    dev = sample_idx.device
    B, n = int(sample_idx.numel()), len(ions)
    M = int(ions[0]["atom_off"].numel()) - 1
    outs = [(torch.empty(B, max_atoms, dtype=torch.int32, device=dev),
             torch.empty(B, slots, dtype=torch.int32, device=dev),
             torch.empty(B, slots, 2, dtype=torch.int32, device=dev)) for _ in range(n)]
    t_out = torch.empty(B, 1, dtype=torch.float32, device=dev) if t_flat is not None else None
    arr = C.c_void_p * n
    mk = lambda ts: arr(*[t.data_ptr() for t in ts])
    for ion in ions:
        for k in ("atom_flat", "atom_off", "edge_flat", "bond_flat", "edge_off"):
            if ion[k].dtype != torch.int32 or not ion[k].is_contiguous():
                raise ValueError(f"{k} must be a contiguous int32 tensor")
        if ion["atom_off"].numel() != M + 1 or ion["edge_off"].numel() != M + 1:
            raise ValueError("offset tables must have M+1 entries")
    with torch.cuda.device(dev):
        check(_lib.load().impnn_batch_assemble(
            n, ptr(sample_idx), B, M, mk([i["atom_flat"] for i in ions]), mk([i["atom_off"] for i in ions]),
            mk([i["edge_flat"] for i in ions]), mk([i["bond_flat"] for i in ions]), mk([i["edge_off"] for i in ions]),
            int(id_shift), int(max_atoms), int(slots), mk([o[0] for o in outs]), mk([o[1] for o in outs]),
            mk([o[2] for o in outs]), ptr(f32c(t_flat)) if t_flat is not None else None,
            ptr(t_out) if t_out is not None else None, stream_ptr()))
    return outs, t_out


def bmm_message(h, bond_state, conn, W):
    """BondMatrixMessage.call, models/layers.py:100-117 -> messages (B,E,D)."""
    if _wants_grad(h, bond_state, W):
        raise NoBackward("gradients of BondMatrixMessage are implemented for bond states that come from an "
                         "Embedding(lazy=True) (per-bond-type schedule), as the reference wires it")
    require_gpu(h, bond_state, conn, W)
    _check_bmm_shapes(h, conn)
    h, bond_state, W, conn = f32c(h), f32c(bond_state), f32c(W), i32c(conn)
    B, N, D = h.shape
    E, K = conn.shape[1], W.shape[0]
    if tuple(bond_state.shape) != (B, E, K) or tuple(W.shape) != (K, D, D):
        raise ValueError(f"bond_state {tuple(bond_state.shape)} / bond_transform {tuple(W.shape)} do not match "
                         f"(B,E,K)=({B},{E},{K}), (K,D,D)=({K},{D},{D})")
    if DEBUG_VALIDATE:
        validate_indices(conn=conn, N=N)
    m = torch.empty(B, E, D, dtype=torch.float32, device=h.device)
    with torch.cuda.device(h.device):
        check(_lib.load().impnn_bmm_message(ptr(h), ptr(bond_state), ptr(conn), ptr(W), ptr(m), B, N, E, D, K,
                                            stream_ptr()))
    return m


def bond_type_matrices(bond_table, W):
    """A[v] = sum_k bond_table[v,k] W[k]  (models/layers.py:108 once per vocabulary entry)."""
    if _wants_grad(bond_table, W):
        from . import autograd
        return autograd.BondTypeMatrices.apply(bond_table, W)
    require_gpu(bond_table, W)
    bond_table, W = f32c(bond_table), f32c(W)
    Vb, K = bond_table.shape
    D = W.shape[-1]
    if W.numel() != K * D * D:
        raise ValueError("bond_transform does not match bond_table")
    out = torch.empty(Vb, D, D, dtype=torch.float32, device=W.device)
    with torch.cuda.device(W.device):
        check(_lib.load().impnn_bond_type_matrices(ptr(bond_table), ptr(W), ptr(out), Vb, K, D, stream_ptr()))
    return out


class IonGraph:
    """atom_ids (B,N), bond_ids (B,E), conn (B,E,2) of one ion for one encode pass, and the device work that depends on
    them alone, shared by the message calls of all layers of the ion, forward and backward.  Kernels may refill these
    tensors in place without torch seeing it (the graphed training step's gather_rows): whoever does makes a new
    IonGraph."""

    def __init__(self, atom_ids, bond_ids, conn, bond_vocab_size):
        self.atom_ids, self.bond_ids, self.conn = atom_ids, bond_ids, conn
        self.bond_vocab_size = int(bond_vocab_size)
        self._sort = None
        self._messages = None

    def edge_sort(self):
        """(workspace, sorted_ready) of the edge sort by bond type.  The first call allocates the workspace and returns
        False: the message kernel it is handed to sorts into it.  Later calls return it with True."""
        if self._sort is not None:
            return self._sort, True
        B, E = self.conn.shape[0], self.conn.shape[1]
        wsb = int(_lib.load().impnn_bmm_message_typed_bwd_workspace_bytes(B, E, self.bond_vocab_size))
        self._sort = torch.empty(max(wsb, 4), dtype=torch.uint8, device=self.conn.device)
        return self._sort, False

    def message_buffer(self, D):
        """(buffer, zero_rows_written) of the (B,E,D) messages: the layers of the ion write theirs into one buffer, one
        after the other (each is consumed by the Reduce right behind it).  The first call allocates it and returns
        False: the message kernel it is handed to writes the zero rows of masked edges.  Later calls return True."""
        if self._messages is not None and self._messages.shape[-1] == D:
            return self._messages, True
        B, E = self.conn.shape[0], self.conn.shape[1]
        self._messages = torch.empty(B, E, D, dtype=torch.float32, device=self.conn.device)
        return self._messages, False

    def written_message_buffer(self, D):
        """The message buffer if a forward already wrote its zero rows, else None (never allocates)."""
        m = self._messages
        return m if m is not None and m.shape[-1] == D else None


def bmm_message_typed(h, bond_ids, conn, type_mats, graph=None, out=None):
    """BondMatrixMessage.call in the per-bond-type schedule (models/layers.py:100-117) -> messages (B,E,D).
    ``graph``: the IonGraph of (bond_ids, conn) in this pass, whose edge sort the call shares; without one the call
    sorts on its own.  ``out``: graph.message_buffer's pair (model-internal: the training step's message buffer)."""
    if _wants_grad(h, type_mats):
        from . import autograd
        return autograd.BmmMessageTyped.apply(h, bond_ids, conn, type_mats, graph)
    require_gpu(h, bond_ids, conn, type_mats)
    _check_bmm_shapes(h, conn)
    h, type_mats, conn, bond_ids = f32c(h), f32c(type_mats), i32c(conn), i32c(bond_ids)
    B, N, D = h.shape
    E, Vb = conn.shape[1], type_mats.shape[0]
    if graph is not None and graph.bond_vocab_size != Vb:
        raise ValueError(f"type matrices for {Vb} bond types, the ion graph has {graph.bond_vocab_size}")
    if DEBUG_VALIDATE:
        validate_indices(conn=conn, bond_ids=bond_ids, N=N, Vb=Vb)
    m, zero_rows = out if out is not None else (torch.empty(B, E, D, dtype=torch.float32, device=h.device), False)
    lib = _lib.load()
    with torch.cuda.device(h.device):
        if D != 32 and D <= 128 and E > 0 and B > 0:
            # any other width: type-sorted segments with A[type] in LDS (the D = 32 kernel sorts inside its workgroups)
            ws, ready = (graph or IonGraph(None, bond_ids, conn, Vb)).edge_sort()
            flags = (1 if ready else 0) | (2 if zero_rows else 0)
            check(lib.impnn_bmm_message_typed_sorted(ptr(h), ptr(bond_ids), ptr(conn), ptr(type_mats), ptr(m), ptr(ws),
                                                     ws.numel(), B, N, E, D, Vb, flags, stream_ptr()))
        else:
            check(lib.impnn_bmm_message_typed(ptr(h), ptr(bond_ids), ptr(conn), ptr(type_mats), ptr(m), B, N,
                                              E, D, Vb, stream_ptr()))
    return m


def reduce_scatter_add(messages, tgt_idx, num_atoms):
    """Reduce.call, models/layers.py:57-83.  `tgt_idx` may be the strided view conn[:, :, 1]
    (train_viscosity.py:182); it is then read in place."""
    if _wants_grad(messages):
        from . import autograd
        return autograd.ReduceScatterAdd.apply(messages, tgt_idx, num_atoms)
    require_gpu(messages, tgt_idx)
    messages = f32c(messages)
    B, E, D = messages.shape
    if tgt_idx.dtype != torch.int32:
        tgt_idx = i32c(tgt_idx)
    if tuple(tgt_idx.shape) != (B, E):
        raise ValueError(f"tgt_idx must be (B,E)=({B},{E}), got {tuple(tgt_idx.shape)}")
    stride = 1
    if not tgt_idx.is_contiguous():
        if B * E > 0 and tgt_idx.stride(1) == 2 and (tgt_idx.stride(0) == 2 * E or B == 1):
            stride = 2  # a conn[:, :, 1] view
        else:
            tgt_idx = tgt_idx.contiguous()
    if DEBUG_VALIDATE:
        validate_indices(conn=tgt_idx.contiguous().unsqueeze(-1).expand(B, E, 2), N=num_atoms)
    agg = torch.empty(B, num_atoms, D, dtype=torch.float32, device=messages.device)
    with torch.cuda.device(messages.device):
        check(_lib.load().impnn_reduce_scatter_add(ptr(messages), ptr(tgt_idx), stride, ptr(agg), B, num_atoms,
                                                   E, D, stream_ptr()))
    return agg


def bmm_fused(h, bond_state, conn, W):
    """Orphan models/bond_matrix_message.py:37-65 signature: -> aggregated (B,N,D)."""
    if _wants_grad(h, bond_state, W):
        raise NoBackward("the fused message+reduce entry is forward-only; train with fused=False")
    require_gpu(h, bond_state, conn, W)
    _check_bmm_shapes(h, conn)
    h, bond_state, W, conn = f32c(h), f32c(bond_state), f32c(W), i32c(conn)
    B, N, D = h.shape
    E, K = conn.shape[1], bond_state.shape[-1]
    if W.numel() != K * D * D:
        raise ValueError("bond_transform must hold K*D*D values")
    agg = torch.empty(B, N, D, dtype=torch.float32, device=h.device)
    if E == 0:
        return agg.zero_()
    with torch.cuda.device(h.device):
        check(_lib.load().impnn_bmm_fused(ptr(h), ptr(bond_state), ptr(conn), ptr(W), ptr(agg), B, N, E, D, K,
                                          stream_ptr()))
    return agg


def kept_row_index(atom_ids, bond_ids, conn, Vb):
    """(row_index (B*N,) int32, n_rows (1,) int32) of the rows an encode() loop has to carry: molecule b's rows
    [0, r_b) as flat indices b*N + n (impnn_kept_rows + impnn_row_index_fill; the prefix sum in between is
    torch.cumsum).  Everything stays on the device."""
    require_gpu(atom_ids, bond_ids, conn)
    atom_ids, bond_ids, conn = i32c(atom_ids), i32c(bond_ids), i32c(conn)
    B, N = atom_ids.shape
    E = conn.shape[1]
    dev = atom_ids.device
    r = torch.empty(B, dtype=torch.int32, device=dev)
    idx = torch.empty(max(B * N, 1), dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        check(lib.impnn_kept_rows(ptr(atom_ids), ptr(bond_ids), ptr(conn), ptr(r), B, N, E, int(Vb), stream_ptr()))
        incl = torch.cumsum(r, 0, dtype=torch.int32)
        check(lib.impnn_row_index_fill(ptr(r), ptr(incl), ptr(idx), ptr(cnt), B, N, stream_ptr()))
    return idx, cnt


def check_dropout_rate(rate):
    """-> rate as a float; ValueError unless 0 <= rate < 1 (also after rounding to float32, as the kernels see it)."""
    r = float(rate)
    if not (0.0 <= r < 1.0) or not float(torch.tensor(r, dtype=torch.float32)) < 1.0:
        raise ValueError(f"dropout rate must satisfy 0 <= rate < 1, got {rate!r}")
    return r


def dropout_layer_word(layer_id, rank=0):
    """The mask's layer counter word: layer_id | (rank << 16) (a model's cation step i is layer i, anion step i S + i)."""
    layer_id, rank = int(layer_id), int(rank)
    if not (0 <= layer_id < 1 << 16 and 0 <= rank < 1 << 15):
        raise ValueError(f"dropout layer id {layer_id} / rank {rank} out of range")
    return layer_id | (rank << 16)


class Dropout:
    """GatedUpdate's dropout in one training pass (include/impnn.h, impnn_*_dropout): rate, the 64-bit seed, the layer
    word and ``step`` - a device int64 tensor of one element, the pass's snapshot of a dropout counter
    (dropout_step).  The backward regenerates the mask from the same four values."""

    __slots__ = ("rate", "seed", "layer_word", "step")

    def __init__(self, rate, seed, layer_word, step):
        self.rate = check_dropout_rate(rate)
        self.seed = int(seed) & ((1 << 64) - 1)
        self.layer_word = int(layer_word)
        if not isinstance(step, torch.Tensor) or step.dtype != torch.int64 or step.numel() != 1:
            raise TypeError("Dropout.step must be a one-element int64 device tensor (ops.dropout_step)")
        self.step = step

    def args(self):
        return (float(self.rate), C.c_uint64(self.seed), ptr(self.step), int(self.layer_word))


def dropout_step(counter):
    """One launch: a fresh snapshot slot <- *counter, *counter += 1 (both device int64).  Returns the snapshot."""
    require_gpu(counter)
    if counter.dtype != torch.int64 or counter.numel() != 1:
        raise TypeError("the dropout counter must be a one-element int64 tensor")
    snap = torch.empty(1, dtype=torch.int64, device=counter.device)
    with torch.cuda.device(counter.device):
        check(_lib.load().impnn_dropout_step(ptr(counter), ptr(snap), stream_ptr()))
    return snap


def dropout_mask(dropout, rows, D, row_list=None):
    """The (rows, D) float32 mask the GatedUpdate kernels apply for ``dropout`` (impnn_dropout_mask): scale where kept,
    0 where dropped; with ``row_list`` = (row_index, n_rows) only the listed rows (zeros elsewhere)."""
    out = torch.zeros(int(rows), int(D), dtype=torch.float32, device=dropout.step.device)
    ri, rn = (ptr(row_list[0]), ptr(row_list[1])) if row_list is not None else (None, None)
    rate, seed, step, lw = dropout.args()
    with torch.cuda.device(out.device):
        check(_lib.load().impnn_dropout_mask(seed, step, lw, rate, ri, rn, int(rows), int(D), ptr(out), stream_ptr()))
    return out


def gated_update(h, agg, Wz, bz, Wr, br, Wh, bh, gamma, beta, eps=LN_EPS, rows=None, save=False, dropout=None):
    """GatedUpdate.call, models/layers.py:142-156.  ``rows`` = (row_index, n_rows) of kept_row_index: only those rows
    of the output are computed (model-internal use: padding atoms; the rest of ``out`` is undefined).
    ``save`` (atom_dim 32 / 64 / 128; the training forward): returns (out, saved) - the gates, the candidate
    and r * h of the listed rows for impnn_gated_update_rows_bwd_saved.
    ``dropout`` (an ops.Dropout; training): the output goes through its mask, fused into the kernel's final store.
    None or rate 0 is the plain forward, bit for bit."""
    if dropout is not None and dropout.rate == 0.0:
        dropout = None
    if _wants_grad(h, agg, Wz, bz, Wr, br, Wh, bh, gamma, beta):
        from . import autograd
        if dropout is not None:
            return autograd.GatedUpdate.apply(h, agg, Wz, bz, Wr, br, Wh, bh, gamma, beta, eps, dropout)
        return autograd.GatedUpdate.apply(h, agg, Wz, bz, Wr, br, Wh, bh, gamma, beta, eps)
    require_gpu(h, agg, Wz, bz, Wr, br, Wh, bh, gamma, beta)
    if h.shape != agg.shape:
        raise ValueError(f"atom_state {tuple(h.shape)} and agg {tuple(agg.shape)} differ")
    D = h.shape[-1]
    for name, w in (("dense_z", Wz), ("dense_r", Wr), ("dense_h", Wh)):
        if tuple(w.shape) != (2 * D, D):
            raise ValueError(f"{name} kernel must be (2D,D)=({2 * D},{D}), got {tuple(w.shape)}")
    ts = [f32c(t) for t in (h, agg, Wz, bz, Wr, br, Wh, bh, gamma, beta)]
    out = torch.empty_like(ts[0])
    nrows = ts[0].numel() // D
    if rows is not None and not save and dropout is None and D not in (32, 64, 128):
        rows = None  # the plain forward has no row list at other widths: every row is computed
    with torch.cuda.device(h.device):
        lib = _lib.load()
        saved = None
        if save:
            saved = torch.empty(int(lib.impnn_gated_update_rows_saved_floats(nrows, D)), dtype=torch.float32,
                                device=h.device)
        entry, tail = _gated_update_entry(lib, rows, saved, dropout, nrows, D)
        check(entry(*[ptr(t) for t in ts], float(eps), ptr(out), *tail, stream_ptr()))
    return (out, saved) if save else out


def _gated_update_entry(lib, rows, saved, dropout, max_rows, D):
    """(row list?, saved?, dropout?) -> the forward entry and its arguments between ``out`` and the stream.
    ``dropout``: rate > 0; with it, a row list or a saved buffer takes impnn_gated_update_rows_train_dropout."""
    ri, rn = (ptr(rows[0]), ptr(rows[1])) if rows is not None else (None, None)
    sv = ptr(saved) if saved is not None else None
    if dropout is not None:
        if rows is None and saved is None:
            return lib.impnn_gated_update_dropout, (max_rows, D, *dropout.args())
        return lib.impnn_gated_update_rows_train_dropout, (ri, rn, max_rows, D, sv, *dropout.args())
    if saved is not None:
        return lib.impnn_gated_update_rows_train, (ri, rn, max_rows, D, sv)
    if rows is not None:
        return lib.impnn_gated_update_rows, (ri, rn, max_rows, D)
    return lib.impnn_gated_update, (max_rows, D)


def global_sum_pool(h, atom_ids):
    """GlobalSumPool.call, models/layers.py:161-164."""
    if _wants_grad(h):
        from . import autograd
        return autograd.GlobalSumPool.apply(h, atom_ids)
    require_gpu(h, atom_ids)
    h, atom_ids = f32c(h), i32c(atom_ids)
    B, N, D = h.shape
    if tuple(atom_ids.shape) != (B, N):
        raise ValueError(f"atom_ids must be (B,N)=({B},{N}), got {tuple(atom_ids.shape)}")
    out = torch.empty(B, D, dtype=torch.float32, device=h.device)
    with torch.cuda.device(h.device):
        check(_lib.load().impnn_global_sum_pool(ptr(h), ptr(atom_ids), ptr(out), B, N, D, stream_ptr()))
    return out


def encoder_step_floats(D, K):
    return int(_lib.load().impnn_encoder_step_floats(D, K))


def pack_step_weights(steps):
    """steps: list of dicts with bond_transform,Wz,bz,Wr,br,Wh,bh,gamma,beta (torch tensors) ->
    one float32 tensor in the canonical layout of include/impnn.h."""
    parts = []
    for s in steps:
        for k in ("bond_transform", "Wz", "bz", "Wr", "br", "Wh", "bh", "gamma", "beta"):
            parts.append(f32c(s[k]).reshape(-1))
    return torch.cat(parts) if parts else None


_workspaces = {}


def _workspace(device, nbytes):
    """Encoder workspace of the CURRENT stream of `device`: calls on one stream reuse it in stream order; calls in
    flight on different streams (a caller overlapping consecutive batches) must not share one."""
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


ENCODER_MODES = {"f32": 0, "f16x2": 1, "f32t": 2, "f32x3": 3}
FP16_MAX = 65504.0
SPLIT_SX, SPLIT_SW = 16.0, 256.0  # kSX / kSW of encoder_fused.hip


def encoder_fused_supported(N, E, D, K, S, Vb, mode="f32t"):
    """Does the fused encoder cover this shape in this mode (impnn_encoder_workspace_bytes says so)?"""
    out = C.c_size_t(0)
    rc = _lib.load().impnn_encoder_workspace_bytes(1, 1, N, E, D, K, S, Vb, ENCODER_MODES[mode], 0, C.byref(out))
    return rc == 0


def encoder_overflow_possible(N, E, D, mode):
    """Can a batch of this padded shape hold a molecule that does not fit one chunk of the typed D = 32 encoder (more than
    256 kept rows, more than 512 valid edges, an in-degree above 255)?  Only then is the plan's overflow word read back
    (one 4-byte device-to-host copy per call)."""
    return D == 32 and mode in ("f32t", "f32x3") and (N > 256 or E > 255)


def _raise_on_overflow(ws):
    off = int(_lib.load().impnn_encoder_plan_overflow_offset())
    if int(ws[off:off + 4].view(torch.int32).item()) != 0:
        raise EncoderOverflow("a molecule of this batch does not fit one chunk of the fused encoder "
                              "(> 256 kept rows, > 512 valid edges or an in-degree > 255)")


PlanLayout = collections.namedtuple("PlanLayout", "nwg max_sub rows_off vr_off nsub_off desc_off ecap plan_vmin")
Plan = collections.namedtuple("Plan", "rows vr nsub desc ion")


def encoder_plan_layout(n_ions, B, N, E, D, K, S, Vb, mode="f32t", workgroups=0):
    """Where the chunk plan of such a call lies in its workspace (impnn_encoder_plan_layout; atom_dim 32 only): the
    resolved workgroup count, the chunk slots per workgroup, byte offsets of the plan's tables, the valid edges a typed
    chunk holds (0: pull-form records) and the least virtual rows a molecule counts.  No device call."""
    out = (C.c_int64 * 8)()
    lib = _lib.load()
    rc = lib.impnn_encoder_plan_layout(n_ions, B, N, E, D, K, S, Vb, ENCODER_MODES[mode], int(workgroups), out)
    if rc == _lib.IMPNN_E_UNSUPPORTED:
        raise EncoderUnsupported(lib.impnn_last_error_string().decode())
    check(rc)
    return PlanLayout(*[int(v) for v in out])


def read_plan(ws, layout, n_ions, B):
    """Copies a finished plan out of its workspace `ws` (a uint8 tensor; the caller has waited for the plan) -> host
    numpy arrays: rows, vr [n_ions][B]; nsub [nwg]; desc [nwg][max_sub][4] = first molecule, molecules, valid edges,
    virtual rows; ion [nwg][max_sub] (out of the descriptor's last word).  Slots at and beyond nsub[j] hold whatever the
    workspace held before."""
    def table(off, count):
        return ws[off:off + 4 * count].view(torch.int32).cpu().numpy().copy()
    rows = table(layout.rows_off, n_ions * B).reshape(n_ions, B)
    vr = table(layout.vr_off, n_ions * B).reshape(n_ions, B)
    nsub = table(layout.nsub_off, layout.nwg)
    desc = table(layout.desc_off, layout.nwg * layout.max_sub * 4).reshape(layout.nwg, layout.max_sub, 4)
    ion = desc[:, :, 3] >> 16
    desc[:, :, 3] &= 0xffff
    return Plan(rows, vr, nsub, desc, ion)


PlanRecords = collections.namedtuple("PlanRecords", "rec_off rec_stride grp_off runs_off nrun_off")
ChunkTables = collections.namedtuple("ChunkTables", "nrun runs grp_type grp_edges grp")


def encoder_plan_records(n_ions, B, N, E, D, K, S, Vb, mode="f32t", workgroups=0):
    """Where the chunk records of such a call lie in its workspace (impnn_encoder_plan_records; typed modes, atom_dim 32):
    byte offset and stride of the records, and inside a record the offsets of the group table, the run table and the run
    count.  No device call."""
    out = (C.c_int64 * 5)()
    lib = _lib.load()
    rc = lib.impnn_encoder_plan_records(n_ions, B, N, E, D, K, S, Vb, ENCODER_MODES[mode], int(workgroups), out)
    if rc == _lib.IMPNN_E_UNSUPPORTED:
        raise EncoderUnsupported(lib.impnn_last_error_string().decode())
    check(rc)
    return PlanRecords(*[int(v) for v in out])


def read_plan_records(ws, layout, chunk):
    """Copies the run and group tables of one chunk out of a finished plan's workspace `ws` (a uint8 tensor; the caller
    has waited for the plan).  `layout`: encoder_plan_records(...) of the call; `chunk`: the record's index, j * max_sub
    + sl for chunk sl of workgroup j.  -> nrun; runs [nrun + 1] (first group of every run, then the group count);
    per group its bond type and edge count; grp [groups][4], the groups' four words."""
    off = layout.rec_off + int(chunk) * layout.rec_stride
    rec = ws[off:off + layout.rec_stride].cpu().numpy().copy()
    nrun = int(rec[layout.nrun_off:layout.nrun_off + 2].view("<u2")[0])
    runs = rec[layout.runs_off:layout.runs_off + 2 * (nrun + 1)].view("<u2").astype("int64")
    ngrp = int(runs[nrun])
    grp = rec[layout.grp_off:layout.grp_off + 16 * ngrp].view("<u4").reshape(ngrp, 4)
    return ChunkTables(nrun, runs, (grp[:, 0] & 0xff).astype("int64"), ((grp[:, 0] >> 8) & 0xff).astype("int64"), grp)


class EncoderUnsupported(RuntimeError):
    pass


class EncoderOverflow(EncoderUnsupported):
    """The shape is covered, this BATCH is not (PlanHeader::overflow): the caller takes the layer-at-a-time path."""


def split_mode_degree_limit(atom_table, bond_table, steps, D):
    """Largest in-degree for which the encoder's "f16x2" mode provably stays inside fp16 range.

    With LayerNorm, |h_s| <= Hmax = max|atom_table| + S*(sqrt(D-1)*max|gamma| + max|beta|)
    (models/layers.py:154-155), |G| <= deg*max|bond_table|*Hmax and |agg_i| <= L1max(W)*|G|max, where
    L1max = max_i sum_{k,j}|W[k,i,j]|.  Mode 1 needs 16*max(|h|,|G|,|agg|) < 65504 and
    256*max|weights| < 65504.  Returns 0.0 when no degree is safe.  (One device sync: call when
    weights change, not per batch.)"""
    if not steps:
        return float("inf")
    gmax = max(float(s["gamma"].abs().max()) for s in steps)
    bmax = max(float(s["beta"].abs().max()) for s in steps)
    wmax = max(float(s[k].abs().max()) for s in steps for k in ("bond_transform", "Wz", "Wr", "Wh"))
    l1 = max(float(s["bond_transform"].abs().sum(dim=(0, 2)).max()) for s in steps)
    hmax = float(atom_table.abs().max()) + len(steps) * ((D - 1) ** 0.5 * gmax + bmax)
    cmax = float(bond_table.abs().max())
    if wmax * SPLIT_SW >= FP16_MAX or hmax * SPLIT_SX >= FP16_MAX:
        return 0.0
    per_deg = SPLIT_SX * cmax * hmax * max(1.0, l1)
    return float("inf") if per_deg == 0.0 else 0.999 * FP16_MAX / per_deg


def prepare_encoder_weights(packed, bond_table, D, K, num_steps, mode="f32t", atom_table=None, gates=True):
    """Builds the encoder's kernel-side weight image once (impnn_encoder_prepare_weights); pass the
    result as `prepared` to encoder_fused while the weights stay unchanged.  Mode "f32t" folds the bond
    embedding table into the image (the per-bond-type matrices), so it must be rebuilt when that table changes.
    With `atom_table` (the atom embedding, (Va, D)) the typed modes also fold it in: the image then carries the table of
    step-0 messages the encoder gathers from and, behind it, the table of step 0's gate accumulators after their h half
    (impnn_encoder_prepare_weights_gates; gates=False: the message table alone, impnn_encoder_prepare_weights_atoms),
    and must be rebuilt when the atom embedding changes too.  The results are the same bits every way."""
    require_gpu(packed, bond_table, atom_table)
    packed, bond_table = f32c(packed), f32c(bond_table)
    S, Vb = int(num_steps), int(bond_table.shape[0])
    lib = _lib.load()
    if atom_table is None:
        nbytes = int(lib.impnn_encoder_prepared_bytes(D, S, Vb, ENCODER_MODES[mode]))
    else:
        atom_table = f32c(atom_table)
        Va = int(atom_table.shape[0])
        size_of = lib.impnn_encoder_prepared_bytes_gates if gates else lib.impnn_encoder_prepared_bytes_atoms
        build = lib.impnn_encoder_prepare_weights_gates if gates else lib.impnn_encoder_prepare_weights_atoms
        nbytes = int(size_of(D, S, Va, Vb, ENCODER_MODES[mode]))
    out = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=packed.device)
    with torch.cuda.device(packed.device):
        if atom_table is None:
            rc = lib.impnn_encoder_prepare_weights(ptr(packed), ptr(bond_table), D, K, S, Vb, ENCODER_MODES[mode],
                                                   ptr(out), nbytes, stream_ptr())
        else:
            rc = build(ptr(packed), ptr(bond_table), ptr(atom_table), Va, D, K, S, Vb, ENCODER_MODES[mode], ptr(out),
                       nbytes, stream_ptr())
    if rc == _lib.IMPNN_E_UNSUPPORTED:
        raise EncoderUnsupported(lib.impnn_last_error_string().decode())
    check(rc)
    return out


def encoder_fused(ions, atom_table, bond_table, packed_weights, num_steps, eps=LN_EPS, mode="f32t", prepared=None,
                  workgroups=0):
    """encode() up to GlobalSumPool for 1 or 2 ion branches in one launch.

    ions: list of (atom_ids (B,N), bond_ids (B,E), conn (B,E,2)); packed_weights: list of packed
    step-weight tensors (pack_step_weights), or None when `prepared` (list of
    prepare_encoder_weights outputs built for the same `mode`) is given.  Returns a list of pooled
    (B,D) tensors.
    mode: "f32t" (per-bond-type messages, exact f32 MFMA, any bond_dim), "f32x3" (the same with the GatedUpdate GEMMs
    as exact three-term bf16 products on the bf16 matrix pipe; opt-in), "f32" (pull form, exact f32 MFMA,
    bond_dim <= 8) or "f16x2" (pull form, split-fp16 MFMA, f32 accumulate; the caller vouches for
    the range condition of include/impnn.h - ionic_mpnn_amd.model does via split_mode_degree_limit).
    workgroups: persistent workgroups of the launch (0: library default, one per CU).
    """
    n = len(ions)
    if n not in (1, 2):
        raise ValueError("1 or 2 ion branches")
    if mode not in ENCODER_MODES:
        raise ValueError(f"mode must be one of {sorted(ENCODER_MODES)}")
    atom_table, bond_table = f32c(atom_table), f32c(bond_table)
    require_gpu(atom_table, bond_table)
    dev = atom_table.device
    prepared_in = []
    for (a, b, c) in ions:
        require_gpu(a, b, c)
        prepared_in.append((i32c(a), i32c(b), i32c(c)))
    B, N = prepared_in[0][0].shape
    E = prepared_in[0][1].shape[1]
    for (a, b, c) in prepared_in:
        if tuple(a.shape) != (B, N) or tuple(b.shape) != (B, E) or tuple(c.shape) != (B, E, 2):
            raise ValueError("ion branches must share (B,N,E)")
    Va, D = atom_table.shape
    Vb, K = bond_table.shape
    S = int(num_steps)
    mode_i, wgs = ENCODER_MODES[mode], int(workgroups)
    lib = _lib.load()
    need = C.c_size_t(0)
    rc = lib.impnn_encoder_workspace_bytes(n, B, N, E, D, K, S, Vb, mode_i, wgs, C.byref(need))
    if rc == _lib.IMPNN_E_UNSUPPORTED:
        raise EncoderUnsupported(lib.impnn_last_error_string().decode())
    check(rc)
    if DEBUG_VALIDATE:
        for (a, b, c) in prepared_in:
            validate_indices(conn=c, atom_ids=a, bond_ids=b, N=N, Va=Va, Vb=Vb)
    ws = _workspace(dev, need.value)
    pooled = [torch.empty(B, D, dtype=torch.float32, device=dev) for _ in range(n)]
    arr = C.c_void_p * n
    mk = lambda ts: arr(*[t.data_ptr() if t is not None else 0 for t in ts])
    common = (mk([p[0] for p in prepared_in]), mk([p[1] for p in prepared_in]), mk([p[2] for p in prepared_in]),
              ptr(atom_table), Va, ptr(bond_table), Vb)
    with torch.cuda.device(dev):
        if prepared is not None:
            if len(prepared) != n or any(int(t.numel()) < int(lib.impnn_encoder_prepared_bytes(D, S, Vb, mode_i))
                                         for t in prepared):
                raise ValueError("prepared weight images do not match (n_ions, num_steps, bond vocabulary, mode)")
            check(lib.impnn_encoder_fused_prepared(n, *common, mk(prepared), mode_i, mk(pooled), B, N, E,
                                                   D, K, S, float(eps), wgs, ptr(ws), ws.numel(), stream_ptr()))
        else:
            ws_w = [f32c(w) if w is not None else None for w in packed_weights]
            step_f = encoder_step_floats(D, K)
            for w in ws_w:
                if S > 0 and (w is None or w.numel() != S * step_f):
                    raise ValueError(f"packed step weights must hold S*{step_f} floats")
            check(lib.impnn_encoder_fused(n, *common, mk(ws_w), mode_i, mk(pooled), B, N, E, D, K, S, float(eps), wgs,
                                          ptr(ws), ws.numel(), stream_ptr()))
    if B > 0 and encoder_overflow_possible(N, E, D, mode):
        _raise_on_overflow(ws)
    return pooled


# ---------------------------------------------------------------------------------------------
# pipelined use: plan of batch i+1 on a side stream while batch i is being encoded
# ---------------------------------------------------------------------------------------------
class EncoderPlan:
    """A planned batch: its workspace, the event that marks the plan complete, and the shapes."""
    __slots__ = ("slot", "ready", "ions", "shape", "n_ions", "info", "mode")


class EncoderPipeline:
    """Two (or more) plan workspaces and a side stream.  ``plan()`` enqueues the graph-only plan
    kernels of a batch on the side stream; ``run()`` enqueues the encoder kernel on torch's current
    stream after the plan's event.  A workspace is reused only after the run that read it is done
    (event-ordered, no host synchronisation)."""

    def __init__(self, device, depth=2):
        self.device = torch.device(device)
        self.side = torch.cuda.Stream(device=self.device)
        self.slots = [{"ws": None, "done": None} for _ in range(depth)]
        self.next = 0

    def plan(self, ions, D, K, S, Va, Vb, mode="f32t", workgroups=0):
        """mode: the mode the batch will be run in (modes "f32"/"f16x2" share one record kind, "f32t" has its own)."""
        n = len(ions)
        prep = []
        for (a, b, c) in ions:
            require_gpu(a, b, c)
            prep.append((i32c(a), i32c(b), i32c(c)))
        B, N = prep[0][0].shape
        E = prep[0][1].shape[1]
        lib = _lib.load()
        need = C.c_size_t(0)
        mode_i, wgs = ENCODER_MODES[mode], int(workgroups)
        rc = lib.impnn_encoder_workspace_bytes(n, B, N, E, D, K, S, Vb, mode_i, wgs, C.byref(need))
        if rc == _lib.IMPNN_E_UNSUPPORTED:
            raise EncoderUnsupported(lib.impnn_last_error_string().decode())
        check(rc)
        slot = self.slots[self.next]
        self.next = (self.next + 1) % len(self.slots)
        if slot["ws"] is None or slot["ws"].numel() < need.value:
            slot["ws"] = torch.empty(max(need.value, 1 << 20), dtype=torch.uint8, device=self.device)
        arr = C.c_void_p * n
        mk = lambda ts: arr(*[t.data_ptr() for t in ts])
        cur = torch.cuda.current_stream(self.device)
        self.side.wait_stream(cur)  # the inputs were produced on the current stream
        if slot["done"] is not None:
            self.side.wait_event(slot["done"])  # the encoder that last read this workspace
        with torch.cuda.device(self.device), torch.cuda.stream(self.side):
            info = _lib.PlanInfo()
            check(lib.impnn_encoder_plan(n, mk([p[0] for p in prep]), mk([p[1] for p in prep]), mk([p[2] for p in prep]),
                                         B, N, E, D, K, S, Va, Vb, mode_i, wgs, ptr(slot["ws"]), slot["ws"].numel(),
                                         C.c_void_p(self.side.cuda_stream), C.byref(info)))
            ready = torch.cuda.Event()
            ready.record(self.side)
        for trio in prep:
            for t in trio:
                t.record_stream(self.side)
        h = EncoderPlan()
        h.slot, h.ready, h.ions, h.shape, h.n_ions = slot, ready, prep, (B, N, E, D, K, S, Vb), n
        h.info, h.mode = info, mode
        return h

    def run(self, plan, atom_table, bond_table, prepared, mode=None, eps=LN_EPS):
        mode = plan.mode if mode is None else mode
        B, N, E, D, K, S, Vb = plan.shape
        n = plan.n_ions
        atom_table, bond_table = f32c(atom_table), f32c(bond_table)
        lib = _lib.load()
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(plan.ready)
        pooled = [torch.empty(B, D, dtype=torch.float32, device=self.device) for _ in range(n)]
        arr = C.c_void_p * n
        mk = lambda ts: arr(*[t.data_ptr() for t in ts])
        ws = plan.slot["ws"]
        with torch.cuda.device(self.device):
            check(lib.impnn_encoder_run(n, mk([p[0] for p in plan.ions]), ptr(atom_table), atom_table.shape[0],
                                        ptr(bond_table), Vb, mk(prepared), ENCODER_MODES[mode], mk(pooled), B, N, E, D,
                                        K, S, float(eps), C.byref(plan.info), ptr(ws), ws.numel(), stream_ptr()))
            done = torch.cuda.Event()
            done.record(cur)
        plan.slot["done"] = done
        if B > 0 and encoder_overflow_possible(N, E, D, mode):
            _raise_on_overflow(ws)
        return pooled


def gather_rows(srcs, dsts, rows):
    """dsts[t][r] = srcs[t][rows[r]] for up to 8 tensors in one launch (impnn_gather_rows): the mini-batch gather
    of model.fit from a device-resident data set.  rows: device int64; tensors: contiguous, 4-byte elements."""
    require_gpu(rows, *srcs, *dsts)
    if rows.dtype != torch.int64 or not rows.is_contiguous():
        raise TypeError("rows must be a contiguous int64 tensor")
    n_rows = rows.numel()
    rb = []
    for sx, dx in zip(srcs, dsts):
        if not (sx.is_contiguous() and dx.is_contiguous()) or sx.dtype != dx.dtype or sx.element_size() != 4:
            raise TypeError("gather_rows needs contiguous tensors of one 4-byte dtype per pair")
        if tuple(sx.shape[1:]) != tuple(dx.shape[1:]) or dx.shape[0] != n_rows:
            raise ValueError(f"gather_rows: shapes {tuple(sx.shape)} -> {tuple(dx.shape)} for {n_rows} rows")
        rb.append(sx[0].numel() * 4 if sx.shape[0] else 4)
    n = len(rb)
    st = (C.c_void_p * n)(*[t.data_ptr() for t in srcs])
    dt = (C.c_void_p * n)(*[t.data_ptr() for t in dsts])
    bt = (C.c_int64 * n)(*rb)
    with torch.cuda.device(rows.device):
        check(_lib.load().impnn_gather_rows(n, st, dt, bt, ptr(rows), n_rows, stream_ptr()))


def state_rows(tables, rows, out=None):
    """out[t][b] = tables[t][rows[t][b]] for one or two ions in one launch (impnn_state_rows): the batch's rows of
    data.FrozenStates, where a resumed training pass starts.  tables[t]: contiguous float32 (R_t, ...) whose row holds
    a multiple of 4 floats; rows[t]: contiguous device int32, B indices (one outside its table yields a row of zeros);
    out[t]: (B, ...) buffers to fill (a captured step's static ones), made here when None.  -> the list of outputs."""
    n = len(tables)
    if n not in (1, 2) or len(rows) != n or (out is not None and len(out) != n):
        raise ValueError("state_rows takes one or two tables, each with its index (and its output)")
    B = int(rows[0].numel())
    if out is None:
        out = [torch.empty((B,) + tuple(t.shape[1:]), dtype=torch.float32, device=t.device) for t in tables]
    require_gpu(*tables, *rows, *out)
    rf = []
    for tb, r, o in zip(tables, rows, out):
        if tb.dtype != torch.float32 or o.dtype != torch.float32 or not (tb.is_contiguous() and o.is_contiguous()):
            raise TypeError("state_rows needs contiguous float32 tables and outputs")
        if r.dtype != torch.int32 or not r.is_contiguous() or r.dim() != 1 or r.numel() != B:
            raise TypeError("state_rows needs one contiguous int32 index of B rows per table")
        if tb.dim() < 2 or tuple(o.shape) != (B,) + tuple(tb.shape[1:]):
            raise ValueError(f"state_rows: shapes {tuple(tb.shape)} -> {tuple(o.shape)} for {B} rows")
        rf.append(int(np.prod(tb.shape[1:])))
    if B == 0:
        return out
    with torch.cuda.device(out[0].device):
        check(_lib.load().impnn_state_rows(
            n, C.cast((C.c_void_p * n)(*[t.data_ptr() for t in tables]), _lib.PP),
            C.cast((C.c_void_p * n)(*[t.data_ptr() for t in rows]), _lib.PP),
            C.cast((C.c_void_p * n)(*[t.data_ptr() for t in out]), _lib.PP), (C.c_int64 * n)(*rf),
            (C.c_int64 * n)(*[int(t.shape[0]) for t in tables]), B, stream_ptr()))
    return out


REGRESSION_SUM_WORDS = 8   # impnn_regression_sums_words()


def regression_sums(pred, y, sample_weight=None, order=None, seg_offsets=None, offset=0.0, scale=1.0, out=None,
                    accumulate=False):
    """Segmented regression sums (impnn_regression_sums; train.regression_sums_reference is the definition) -> the
    (n_seg, 8) float64 device tensor of the records: samples, sum w, sum w e, sum w |e|, sum w e^2, sum w yr,
    sum w yr^2, max |e| over w > 0, with e = scale * (pred - y) and yr = offset + scale * y in fp64.

    ``pred`` / ``y`` / ``sample_weight`` (optional: w = 1): float32, one value per sample.  ``seg_offsets`` (device
    int64, n_seg + 1 ascending values in [0, n]) cuts the positions 0 .. n-1 into segments, ``order`` (device int32,
    optional) names the sample at each position; without ``seg_offsets`` all samples are one segment.  ``out``: the
    records' tensor to write, or with ``accumulate`` to add to (word 7 takes the maximum); stream-ordered, one launch,
    the same bits at every call."""
    require_gpu(pred, y, sample_weight, order, seg_offsets, out)
    for t, what in ((pred, "pred"), (y, "y"), (sample_weight, "sample_weight")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise TypeError(f"{what} must be a contiguous float32 tensor")
    n = pred.numel()
    if y.numel() != n or (sample_weight is not None and sample_weight.numel() != n):
        raise ValueError("pred, y and sample_weight must hold one value per sample")
    if order is not None and (order.dtype != torch.int32 or not order.is_contiguous() or order.numel() != n):
        raise TypeError("order must be a contiguous int32 tensor of one index per sample")
    n_seg = 1
    if seg_offsets is not None:
        if seg_offsets.dtype != torch.int64 or not seg_offsets.is_contiguous() or seg_offsets.numel() < 2:
            raise TypeError("seg_offsets must be a contiguous int64 tensor of n_seg + 1 values")
        n_seg = seg_offsets.numel() - 1
    if out is None:
        if accumulate:
            raise ValueError("accumulate adds to the records in `out`")
        out = torch.empty(n_seg, REGRESSION_SUM_WORDS, dtype=torch.float64, device=pred.device)
    elif out.dtype != torch.float64 or not out.is_contiguous() or tuple(out.shape) != (n_seg, REGRESSION_SUM_WORDS):
        raise TypeError(f"out must be a contiguous float64 tensor of shape ({n_seg}, {REGRESSION_SUM_WORDS})")
    if any(t is not None and t.device != pred.device for t in (y, sample_weight, order, seg_offsets, out)):
        raise ValueError("regression_sums: all tensors must live on one device")
    if n == 0:  # (an empty tensor has no address to hand over) every segment is empty: zeros, or nothing to add
        return out if accumulate else out.zero_()
    with torch.cuda.device(pred.device):
        check(_lib.load().impnn_regression_sums(
            ptr(pred), ptr(y), None if sample_weight is None else ptr(sample_weight),
            None if order is None else ptr(order), None if seg_offsets is None else ptr(seg_offsets), n, n_seg,
            float(offset), float(scale), 1 if accumulate else 0, ptr(out), stream_ptr()))
    return out


# the widths every head kernel covers: kHeadMaxX / kHeadMaxDim of csrc/common.h (tests/test_cabi.py holds them equal)
HEAD_MAX_X = 128    # pooled width (atom_dim)
HEAD_MAX_DIM = 64   # fp_size, mixing_size
# the most packed head floats (rounded up to 4) impnn_model_head_bwd holds in LDS next to their gradient sums: the
# library's impnn_model_head_bwd_max_floats() (tests/test_head_fuzz_host.py holds them equal)
HEAD_BWD_MAX_FLOATS = 15360


def model_head_bwd_fits(kind, D, fp_size, mixing_size):
    """Whether impnn_model_head_bwd / impnn_model_head_loss_bwd take a head of these widths (``kind`` 0 / 1): the
    launcher's LDS fit, which is narrower than the width limits."""
    n = int(_lib.load().impnn_model_head_floats(kind, D, fp_size, mixing_size))
    return n > 0 and (n + 3) // 4 * 4 <= HEAD_BWD_MAX_FLOATS


def _require_packed_head(head_weights, k, D, fp_size, mixing_size):
    if D < 1 or head_weights.numel() != _lib.load().impnn_model_head_floats(k, D, fp_size, mixing_size):
        raise ValueError("packed head weights have the wrong length")


def model_head(kind, pooled_cat, pooled_an, temperature, head_weights, fp_size, mixing_size):
    """Everything after GlobalSumPool in one launch (impnn_model_head): kind "viscosity" or "melting_point"."""
    require_gpu(pooled_cat, pooled_an, head_weights)
    pooled_cat, pooled_an, head_weights = f32c(pooled_cat), f32c(pooled_an), f32c(head_weights)
    B, D = pooled_cat.shape
    k = {"viscosity": 0, "melting_point": 1}[kind]
    lib = _lib.load()
    _require_packed_head(head_weights, k, D, fp_size, mixing_size)
    T = None
    if k == 0:
        require_gpu(temperature)
        T = f32c(temperature).reshape(-1)
        if T.numel() != B:
            raise ValueError("temperature must hold one value per sample")
    out = torch.empty(B, 1, dtype=torch.float32, device=pooled_cat.device)
    with torch.cuda.device(pooled_cat.device):
        check(lib.impnn_model_head(k, ptr(pooled_cat), ptr(pooled_an), ptr(T) if T is not None else None,
                                   ptr(head_weights), ptr(out), B, D, fp_size, mixing_size, stream_ptr()))
    return out


HEAD_KINDS = {"viscosity": 0, "melting_point": 1}


def head_ion_mix(kind, ion, pooled, head_weights, fp_size, mixing_size):
    """The per-ion half of the head (impnn_head_ion_mix): ``ion`` "cat" / 0 or "an" / 1, pooled (M,D) ->
    relu(relu(pooled Wfp + bfp) Wp + bp) (M,Mx), from the packed head weights of ``model_head``."""
    require_gpu(pooled, head_weights)
    pooled, head_weights = f32c(pooled), f32c(head_weights)
    if pooled.dim() != 2:
        raise ValueError(f"pooled must be (M,D), got {tuple(pooled.shape)}")
    M, D = pooled.shape
    k = HEAD_KINDS[kind]
    g = {"cat": 0, "an": 1, 0: 0, 1: 1}[ion]
    lib = _lib.load()
    _require_packed_head(head_weights, k, D, fp_size, mixing_size)
    mix = torch.empty(M, mixing_size, dtype=torch.float32, device=pooled.device)
    with torch.cuda.device(pooled.device):
        check(lib.impnn_head_ion_mix(k, g, ptr(pooled), ptr(head_weights), ptr(mix), M, D, fp_size, mixing_size,
                                     stream_ptr()))
    return mix


# ---- the screening family over a cation x anion grid: the operands are validated once (GridOperands), the six
# operations (grid_values, grid_topk, grid_partners, grid_rank, grid_mask, grid_summary) take any family's, and the named wrappers
# below them are "build the operands, call the operation"
class GridOperands:
    """The validated operands of the screening family's launches over one cation x anion grid, built by
    ``head_grid_operands`` (family 0), ``transfer_grid_operands`` (family 1), ``ensemble_grid_operands`` (family 2) or
    ``transfer_mc_grid_operands`` (family 3: family 1's tensors, ``multipliers`` (S,128) - ``samples`` = S - and ``kappa``):
    the contiguous float32 tensors (``cat`` and ``an`` rows, ``T`` or None, ``w``: the packed head, the prepared image or
    the members' tails), ``kind`` as the C entries take it (0 viscosity, 1 melting point and transfer) and ``widths``: (D,
    fp_size, mixing_size) for the head family, (fp_size, mixing_size) for the ensemble family, whose rows are
    three-dimensional - (M,C,Mx) and (M,A,Mx), ``members`` = M - and which carries ``kappa`` of its score.  ``lead`` and
    ``trail`` are the arguments every C entry of the family opens and closes with; the operation's own go between.
    ``rows`` and ``temperatures`` narrow it without validating again (the host tiling of screening.py)."""
    __slots__ = ("family", "kind", "cat", "an", "T", "w", "widths", "kappa", "multipliers")

    def __init__(self, family, kind, cat, an, T, w, widths=(), kappa=0.0, multipliers=None):
        self.family, self.kind, self.cat, self.an, self.T, self.w, self.widths = family, kind, cat, an, T, w, widths
        self.kappa, self.multipliers = kappa, multipliers

    C = property(lambda self: int(self.cat.shape[-2]))
    A = property(lambda self: int(self.an.shape[-2]))
    nT = property(lambda self: int(self.T.numel()) if self.T is not None else 0)
    D = property(lambda self: self.widths[0] if self.family == 0 else None)
    members = property(lambda self: int(self.cat.shape[0]) if self.family == 2 else 1)
    samples = property(lambda self: int(self.multipliers.shape[0]) if self.family == 3 else 1)
    device = property(lambda self: self.cat.device)

    @property
    def lead(self):
        T = ptr(self.T) if self.T is not None else None
        if self.family == 0:
            return self.kind, ptr(self.cat), ptr(self.an), T, ptr(self.w)
        if self.family == 2:
            return self.kind, self.members, ptr(self.cat), ptr(self.an), T, ptr(self.w), self.kappa
        image = ptr(self.cat), ptr(self.an), ptr(self.w), self.w.numel()
        return image if self.family == 1 else (*image, ptr(self.multipliers), self.samples, self.kappa)

    @property
    def trail(self):
        return (self.C, self.A, self.nT, *self.widths) if self.family in (0, 2) else (self.C, self.A)

    def _narrowed(self, cat, T):
        return GridOperands(self.family, self.kind, cat, self.an, T, self.w, self.widths, self.kappa, self.multipliers)

    def rows(self, lo, hi):
        """Cations lo .. hi of the grid (of every member: a copy, the C entries take contiguous rows)."""
        return self._narrowed(self.cat[lo:hi] if self.family != 2 else self.cat[:, lo:hi].contiguous(), self.T)

    def temperatures(self, t0, t1):
        """Temperatures t0 .. t1 of a viscosity grid; any other grid as it is."""
        return self if self.T is None else self._narrowed(self.cat, self.T[t0:t1])


def _require_params_kind(return_params, k):
    if return_params and k != 0:
        raise ValueError("return_params: only the viscosity head has VFT parameters")


def head_grid_operands(kind, mix_cat, mix_an, temperatures, head_weights, fp_size, mixing_size, return_params=False):
    """The arguments of ``head_grid`` and of every screening operation over its product, checked once -> GridOperands.
    ``return_params``: ``head_grid``'s own argument, checked where it always was, between the rows and the packed head."""
    require_gpu(mix_cat, mix_an, head_weights)
    mix_cat, mix_an, head_weights = f32c(mix_cat), f32c(mix_an), f32c(head_weights)
    k = HEAD_KINDS[kind]
    if mix_cat.dim() != 2 or mix_an.dim() != 2 or mix_cat.shape[1] != mixing_size or mix_an.shape[1] != mixing_size:
        raise ValueError(f"mixing rows must be (C,{mixing_size}) and (A,{mixing_size}), got {tuple(mix_cat.shape)} "
                         f"and {tuple(mix_an.shape)}")
    _require_params_kind(return_params, k)
    lib = _lib.load()
    # the packed length depends on D through the per-ion part only: recover D from it
    per_d = 2 * fp_size
    rest = lib.impnn_model_head_floats(k, 1, fp_size, mixing_size) - per_d
    D = (head_weights.numel() - rest) // per_d if head_weights.numel() > rest else 0
    _require_packed_head(head_weights, k, D, fp_size, mixing_size)
    T = None
    if k == 0:
        if temperatures is None:
            raise ValueError("the viscosity grid needs temperatures")
        require_gpu(temperatures)
        T = f32c(temperatures).reshape(-1)
    elif temperatures is not None:
        raise ValueError("the melting-point grid takes no temperatures")
    return GridOperands(0, k, mix_cat, mix_an, T, head_weights, (D, fp_size, mixing_size))


def transfer_grid_operands(u_cat, u_an, image):
    """The arguments of ``transfer_head_grid`` and of every screening operation over its product, checked once ->
    GridOperands."""
    require_gpu(u_cat, u_an, image)
    u_cat, u_an, image = f32c(u_cat), f32c(u_an), f32c(image)
    W = TRANSFER_GRID_WIDTH
    if u_cat.dim() != 2 or u_an.dim() != 2 or u_cat.shape[1] != W or u_an.shape[1] != W:
        raise ValueError(f"u rows must be (C,{W}) and (A,{W}), got {tuple(u_cat.shape)} and {tuple(u_an.shape)}")
    if image.dim() != 1 or image.numel() != _lib.load().impnn_transfer_grid_image_floats():
        raise ValueError("the prepared image has the wrong length")
    return GridOperands(1, 1, u_cat, u_an, None, image)


def ensemble_grid_operands(kind, mix_cat, mix_an, temperatures, tails, fp_size, mixing_size, kappa=0.0):
    """The operands of a deep ensemble's grid (impnn_ensemble_grid*): M members of ``kind`` -> GridOperands, family 2.
    ``mix_cat`` (M,C,Mx) and ``mix_an`` (M,A,Mx): member m's ``head_ion_mix`` rows; ``tails`` (M, tail floats): member
    m's tail of the packed head (impnn_ensemble_grid_tail_floats: ``packed[-tail_floats:]``); ``kappa``: the score is
    mean + kappa * std, any finite float."""
    require_gpu(mix_cat, mix_an, tails)
    mix_cat, mix_an, tails = f32c(mix_cat), f32c(mix_an), f32c(tails)
    k = HEAD_KINDS[kind]
    lib = _lib.load()
    if mix_cat.dim() != 3 or mix_an.dim() != 3 or mix_cat.shape[2] != mixing_size or mix_an.shape[2] != mixing_size \
            or mix_cat.shape[0] != mix_an.shape[0]:
        raise ValueError(f"mixing rows must be (M,C,{mixing_size}) and (M,A,{mixing_size}), got {tuple(mix_cat.shape)} "
                         f"and {tuple(mix_an.shape)}")
    M = int(mix_cat.shape[0])
    if not 1 <= M <= lib.impnn_ensemble_grid_max_members():
        raise ValueError(f"an ensemble grid takes 1 to {lib.impnn_ensemble_grid_max_members()} members, got {M}")
    if tuple(tails.shape) != (M, lib.impnn_ensemble_grid_tail_floats(k, fp_size, mixing_size)):
        raise ValueError("the members' tails have the wrong shape")
    kappa = C.c_float(kappa).value  # as the kernels see it: float32
    if kappa != kappa or kappa in (float("inf"), float("-inf")):
        raise ValueError("kappa must be finite")
    T = None
    if k == 0:
        if temperatures is None:
            raise ValueError("the viscosity grid needs temperatures")
        require_gpu(temperatures)
        T = f32c(temperatures).reshape(-1)
    elif temperatures is not None:
        raise ValueError("the melting-point grid takes no temperatures")
    return GridOperands(2, k, mix_cat, mix_an, T, tails, (fp_size, mixing_size), kappa)


def transfer_mc_grid_operands(u_cat, u_an, image, multipliers, kappa=0.0):
    """The operands of Monte-Carlo dropout over the transfer head's grid (impnn_transfer_mc_grid*) -> GridOperands,
    family 3.  ``u_cat``, ``u_an``, ``image`` as ``transfer_grid_operands``; ``multipliers`` (S,128) float32: sample s
    multiplies feature j of relu(Dense 128) by ``multipliers[s, j]`` (0: the feature is dropped) - for a Dropout,
    ``dropout_mask(dropout, rows=S, D=128)``, whose row s is the mask a training pass at that step gives batch row s.
    The table is the same for every pair (the "fixed set of masks" form of MC dropout): a pair's S values, and so its
    mean, spread and score, depend only on its two u rows, the image and the table - not on the tile, the launch, the
    host tiling or the grid's size.  ``kappa``: the score is mean + kappa * std, any finite float."""
    g = transfer_grid_operands(u_cat, u_an, image)
    require_gpu(multipliers)
    multipliers = f32c(multipliers)
    most = int(_lib.load().impnn_transfer_mc_grid_max_samples())
    if multipliers.dim() != 2 or multipliers.shape[1] != TRANSFER_MC_WIDTH or not 1 <= multipliers.shape[0] <= most:
        raise ValueError(f"multipliers must be (S,{TRANSFER_MC_WIDTH}) with 1 <= S <= {most}, got {tuple(multipliers.shape)}")
    kappa = C.c_float(kappa).value  # as the kernels see it: float32
    if kappa != kappa or kappa in (float("inf"), float("-inf")):
        raise ValueError("kappa must be finite")
    return GridOperands(3, 1, g.cat, g.an, None, g.w, (), kappa, multipliers)


def transfer_mc_grid(g, return_samples=False):
    """The materialised statistic of a family-3 ``g`` (impnn_transfer_mc_grid) -> (mean, std, score), each (C,A); with
    ``return_samples`` also the S sample planes (S,C,A), whose statistic in ``data.ensemble_grid_stats``'s order the
    three are."""
    if g.family != 3:
        raise ValueError("transfer_mc_grid takes the operands of transfer_mc_grid_operands")
    dev = g.device
    outs = [torch.empty(g.C, g.A, dtype=torch.float32, device=dev) for _ in range(3)]
    samples = torch.empty(g.samples, g.C, g.A, dtype=torch.float32, device=dev) if return_samples else None
    with torch.cuda.device(dev):
        check(_lib.load().impnn_transfer_mc_grid(*g.lead, *[ptr(o) for o in outs],
                                                 ptr(samples) if samples is not None else None, *g.trail, stream_ptr()))
    return (*outs, samples) if return_samples else tuple(outs)


def grid_values(g, return_params=False):
    """The materialised grid of ``g`` (impnn_head_grid / impnn_transfer_head_grid): what ``head_grid`` /
    ``transfer_head_grid`` return for the same operands.  An ensemble grid (impnn_ensemble_grid) and a transfer MC grid
    (impnn_transfer_mc_grid): (mean, std, score)."""
    _require_params_kind(return_params, g.kind)
    dev = g.device
    if g.family == 3:
        return transfer_mc_grid(g)
    if g.family == 2:
        if return_params:
            raise ValueError("return_params: an ensemble grid has no VFT parameters of its own")
        outs = [torch.empty((g.C, g.A, g.nT) if g.kind == 0 else (g.C, g.A), dtype=torch.float32, device=dev) for _ in range(3)]
        with torch.cuda.device(dev):
            check(_lib.load().impnn_ensemble_grid(*g.lead, *[ptr(o) for o in outs], *g.trail, stream_ptr()))
        return tuple(outs)
    out = torch.empty((g.C, g.A, g.nT) if g.kind == 0 else (g.C, g.A), dtype=torch.float32, device=dev)
    params = torch.empty(g.C, g.A, 3, dtype=torch.float32, device=dev) if return_params else None
    lib = _lib.load()
    with torch.cuda.device(dev):
        if g.family == 0:
            check(lib.impnn_head_grid(*g.lead, ptr(out), ptr(params) if params is not None else None, *g.trail,
                                      stream_ptr()))
        else:
            check(lib.impnn_transfer_head_grid(*g.lead, ptr(out), *g.trail, stream_ptr()))
    return (out, params) if return_params else out


def _grid_entry(g, name):
    """The C entry ``name`` of g's family: impnn_head_grid_<name>, impnn_transfer_head_grid_<name>,
    impnn_ensemble_grid_<name> or impnn_transfer_mc_grid_<name>."""
    if g.family == 2 and name == "summary":  # (named apart from impnn_ensemble_grid*, the list of that family's first entries)
        return _lib.load().impnn_deep_ensemble_grid_summary
    return getattr(_lib.load(), ("impnn_head_grid_", "impnn_transfer_head_grid_", "impnn_ensemble_grid_",
                                 "impnn_transfer_mc_grid_")[g.family] + name)


def _refuse_ensemble(g):
    if g.family == 2:
        raise NotImplementedError("ensemble grids: partners / rank are not built")
    if g.family == 3:
        raise NotImplementedError("transfer MC grids: partners / rank are not built")


def grid_topk(g, k, largest=False, workgroups=0, where=None):
    """The k best pairs of ``g``'s grid (impnn_*_grid_topk, with ``where`` impnn_*_grid_topk_where): what
    ``head_grid_topk`` / ``transfer_head_grid_topk`` return for the same operands."""
    k, workgroups = int(k), int(workgroups)
    if where is not None:
        where = _mask_words(where, g.C, g.A, g.device)
    with torch.cuda.device(g.device):
        values, cation, anion, ws, nbytes = _grid_topk_outputs(_lib.load(), g.family, g.C, g.A, g.nT, k, workgroups, g.device,
                                                               g.members if g.family != 3 else g.samples)
        mask = () if where is None else (ptr(where),)
        check(_grid_entry(g, "topk" if where is None else "topk_where")(
            *g.lead, *mask, k, int(bool(largest)), ptr(values), ptr(cation), ptr(anion), ptr(ws), nbytes, *g.trail,
            workgroups, stream_ptr()))
    return values, cation, anion


def grid_partners(g, m=1, largest=False, where=None):
    """Each ion's m best partners over ``g``'s grid (impnn_*_grid_partners): what ``head_grid_partners`` /
    ``transfer_head_grid_partners`` return for the same operands."""
    _refuse_ensemble(g)
    m = int(m)
    if where is not None:
        where = _mask_words(where, g.C, g.A, g.device)
    with torch.cuda.device(g.device):
        out, ws, nbytes = _grid_partners_outputs(_lib.load(), g.family, g.C, g.A, g.nT, m, g.device)
        check(_grid_entry(g, "partners")(*g.lead, ptr(where) if where is not None else None, m, int(bool(largest)),
                                         *[ptr(o) for o in out], ptr(ws), nbytes, *g.trail, stream_ptr()))
    return tuple(out)


def grid_rank(g, k, largest=False, where=None, mask=False, workgroups=0):
    """The k-th best pair of ``g``'s grid and, with ``mask``, the k best as mask words (impnn_*_grid_rank): what
    ``head_grid_rank`` / ``transfer_head_grid_rank`` return for the same operands."""
    _refuse_ensemble(g)
    k, workgroups = int(k), int(workgroups)
    if where is not None:
        where = _mask_words(where, g.C, g.A, g.device)
    with torch.cuda.device(g.device):
        out, ws, nbytes = _grid_rank_outputs(_lib.load(), g.family, g.C, g.A, g.nT, workgroups, mask, g.device)
        check(_grid_entry(g, "rank")(*g.lead, k, int(bool(largest)), ptr(where) if where is not None else None,
                                     *[ptr(o) if o is not None else None for o in out], ptr(ws), nbytes, *g.trail,
                                     workgroups, stream_ptr()))
    return out


# (cations, anions) of the blocks the summary's sums run over: the kernel tile of each family (csrc/grid_device.h)
SUMMARY_BLOCKS = {0: (16, 64), 1: (8, 32), 2: (16, 64), 3: (8, 32)}


def grid_summary(g, where=None, carry=None):
    """Per-ion records of ``g``'s grid without the grid (impnn_*_grid_summary; every family, the ensemble and MC grids
    on their score) -> (cat_count int32 (P,C) - the uint32 counts' bits -, cat_sums float64 (P,C,2) = (s, q), cat_range
    float32 (P,C,2) = (lo, hi), an_count (P,A), an_sums (P,A,2), an_range (P,A,2)) on the device, P = max(nT, 1): the
    bits of ``data.grid_ion_records(grid_values(g), where, SUMMARY_BLOCKS[g.family])``.  ``where``: the (C,W) words of
    a pair mask, only its pairs compete.  ``carry``: the three anion tensors an earlier range of cations returned (a
    range ends at a multiple of 16 cations); the anion records continue from them, and the result has the bits of one
    call over both ranges.  ``data.IonSummary.from_records`` finishes the records."""
    require_gpu(g.cat, g.an, g.w)
    if where is not None:
        where = _mask_words(where, g.C, g.A, g.device)
    C_, A_, planes, dev = g.C, g.A, max(g.nT, 1), g.device
    shapes = ((torch.int32, ()), (torch.float64, (2,)), (torch.float32, (2,)))
    if carry is not None:
        carry = tuple(carry)
        require_gpu(*carry)
        if len(carry) != 3 or any(c.dtype != dt or tuple(c.shape) != (planes, A_, *tail) or c.device != dev
                                  for c, (dt, tail) in zip(carry, shapes)):
            raise ValueError(f"carry must be the three anion tensors of an earlier grid_summary over {planes} planes and "
                             f"{A_} anions on {dev}")
    with torch.cuda.device(dev):
        cat = [torch.empty((planes, C_, *tail), dtype=dt, device=dev) for dt, tail in shapes]
        an = [c.clone().contiguous() for c in carry] if carry is not None else \
            [torch.empty((planes, A_, *tail), dtype=dt, device=dev) for dt, tail in shapes]
        if C_ == 0 or A_ == 0:  # zero work touches nothing: no pair competes
            for count, sums, rng in (cat, an) if carry is None else (cat,):
                count.zero_(), sums.zero_(), rng.fill_(float("nan"))
            return (*cat, *an)
        need = int(_lib.load().impnn_grid_summary_workspace_bytes(g.family, C_, A_, planes))
        if need == 0:
            raise ValueError(f"grid_summary: {planes} temperature planes are more than one launch takes; split the sweep")
        ws = _workspace(dev, need)
        table = (C.c_void_p * 7)(*[t.data_ptr() for t in (*cat, *an)], ws.data_ptr())
        check(_grid_entry(g, "summary")(*g.lead, ptr(where) if where is not None else None, int(carry is not None), need,
                                        table, *g.trail, stream_ptr()))
    return (*cat, *an)


def grid_mask(g, lo, hi):
    """``g``'s grid as a packed pair mask (impnn_*_grid_mask): what ``head_grid_mask`` / ``transfer_head_grid_mask``
    return for the same operands."""
    lo, hi = C.c_float(lo).value, C.c_float(hi).value  # as the kernels see them: float32
    if lo != lo or hi != hi:
        raise ValueError("a mask bound is NaN (an infinity means no limit)")
    lib = _lib.load()
    W = int(lib.impnn_grid_mask_row_words(g.A))
    words = torch.empty((g.nT, g.C, W) if g.kind == 0 else (g.C, W), dtype=torch.int32, device=g.device)
    with torch.cuda.device(g.device):
        check(_grid_entry(g, "mask")(*g.lead, lo, hi, ptr(words), *g.trail, stream_ptr()))
    return words


def head_grid(kind, mix_cat, mix_an, temperatures, head_weights, fp_size, mixing_size, return_params=False):
    """The head on every cation x anion pair in one launch (impnn_head_grid), from ``head_ion_mix`` rows.
    "viscosity": temperatures (nT) in kelvin -> (C,A,nT), with return_params also the VFT parameters (C,A,3);
    "melting_point": temperatures None -> (C,A).  Element (i,j,t) has the bits of ``model_head`` on that sample."""
    return grid_values(head_grid_operands(kind, mix_cat, mix_an, temperatures, head_weights, fp_size, mixing_size, return_params),
                       return_params)


TRANSFER_GRID_WIDTH = 256  # mp_dense_1's units: the width of a ``transfer_ion_half`` row
TRANSFER_MC_WIDTH = 128    # mp_dense_2's units: the features mp_dropout thins, the width of a multiplier row


def _transfer_weight_table(weights):
    if len(weights) != 18:
        raise ValueError(f"the transfer head has 18 weight tensors, got {len(weights)}")
    require_gpu(*weights)
    weights = [f32c(w) for w in weights]
    return weights, (C.c_void_p * len(weights))(*[w.data_ptr() for w in weights])


def transfer_grid_prepare(weights, cfg):
    """The weight image of ``transfer_head_grid`` (impnn_transfer_grid_prepare): mp_dense_2 / mp_dense_3 in MFMA operand
    order, BatchNormalization's moving statistics as scale and shift, the last biases and kernel.  ``weights`` the 18
    tensors in the order of include/impnn.h, ``cfg`` MPNNModel._transfer_cfg.  Build it once per weight version."""
    weights, table = _transfer_weight_table(weights)
    mean, var = cfg["moving_mean"], cfg["moving_variance"]
    require_gpu(mean, var)
    mean, var = f32c(mean), f32c(var)
    if weights[12].shape != (256, 128) or weights[14].shape != (128, 64) or mean.numel() != 256 or var.numel() != 256:
        raise ValueError("transfer_grid_prepare: the head is Dense 256 - BatchNormalization - Dense 128 - Dense 64 - Dense 1")
    lib = _lib.load()
    n = lib.impnn_transfer_grid_image_floats()
    image = torch.empty(n, dtype=torch.float32, device=mean.device)
    with torch.cuda.device(mean.device):
        check(lib.impnn_transfer_grid_prepare(table, ptr(mean), ptr(var), cfg["epsilon"], ptr(image), n, stream_ptr()))
    return image


def transfer_ion_half(ion, pooled, weights, fp_size, mixing_size):
    """The per-ion half of the transfer head (impnn_transfer_ion_half): ``ion`` "cat" / 0 or "an" / 1, pooled (M,D) ->
    relu(relu(pooled Wfp + bfp) Wp + bp) W1 (+ b1 for the anion) (M,256), from the 18 weight tensors."""
    require_gpu(pooled)
    pooled = f32c(pooled)
    if pooled.dim() != 2:
        raise ValueError(f"pooled must be (M,D), got {tuple(pooled.shape)}")
    weights, table = _transfer_weight_table(weights)
    M, D = pooled.shape
    g = {"cat": 0, "an": 1, 0: 0, 1: 1}[ion]
    if weights[2 * g].shape != (D, fp_size) or weights[4 + 2 * g].shape != (fp_size, mixing_size) \
            or weights[8].shape != (mixing_size, TRANSFER_GRID_WIDTH):
        raise ValueError(f"transfer_ion_half: weight shapes do not match D={D}, fp_size={fp_size}, mixing_size={mixing_size}")
    u = torch.empty(M, TRANSFER_GRID_WIDTH, dtype=torch.float32, device=pooled.device)
    with torch.cuda.device(pooled.device):
        check(_lib.load().impnn_transfer_ion_half(g, ptr(pooled), table, ptr(u), M, D, fp_size, mixing_size, stream_ptr()))
    return u


def transfer_head_grid(u_cat, u_an, image):
    """The transfer head on every cation x anion pair in one launch (impnn_transfer_head_grid), on the matrix cores in
    exact f32: ``transfer_ion_half`` rows (C,256) and (A,256), the image of ``transfer_grid_prepare`` -> (C,A)."""
    return grid_values(transfer_grid_operands(u_cat, u_an, image))


# the limits of one selecting launch: kSelectMaxK / kSelectMaxT of csrc/common.h (tests/test_screen_host.py holds them equal)
SELECT_MAX_K = 1024
SELECT_MAX_T = 4


def _grid_topk_outputs(lib, family, C_, A_, nT, k, workgroups, dev, members=1):
    rows = max(nT, 1)
    need = C.c_size_t(0)
    if family == 2:  # the ensemble grid has its own query: its temperature limit depends on the members
        check(lib.impnn_ensemble_grid_topk_workspace_bytes(members, C_, A_, nT, k, workgroups, C.byref(need)))
    elif family == 3:  # the transfer MC grid's: ``members`` is its sample count
        check(lib.impnn_transfer_mc_grid_topk_workspace_bytes(members, C_, A_, k, workgroups, C.byref(need)))
    else:
        check(lib.impnn_grid_topk_workspace_bytes(family, C_, A_, nT, k, workgroups, C.byref(need)))
    values = torch.empty(rows, k, dtype=torch.float32, device=dev)
    cation = torch.empty(rows, k, dtype=torch.int32, device=dev)
    anion = torch.empty(rows, k, dtype=torch.int32, device=dev)
    if C_ == 0 or A_ == 0:  # zero work touches nothing: no pair in any slot
        values.fill_(float("nan")), cation.fill_(-1), anion.fill_(-1)
    return values, cation, anion, _workspace(dev, need.value), need.value


def _mask_words(where, C_, A_, dev):
    """``where`` of the top-k wrappers: a (C,W) int32 tensor of mask words, or an object with such ``words``."""
    where = getattr(where, "words", where)
    require_gpu(where)
    want = (C_, (A_ + 31) // 32)
    if where.dtype != torch.int32 or tuple(where.shape) != want or where.device != dev:
        raise ValueError(f"where must be int32 mask words of shape {want} on {dev}, got {where.dtype} "
                         f"{tuple(where.shape)} on {where.device}")
    return where.contiguous()


def head_grid_topk(kind, mix_cat, mix_an, temperatures, head_weights, fp_size, mixing_size, k, largest=False,
                   workgroups=0, where=None):
    """The k best pairs of ``head_grid``'s product without the product (impnn_head_grid_topk): the same arguments, ->
    values (nT,k) float32, cation (nT,k), anion (nT,k) int32 on the device, a row per temperature (one row for
    "melting_point"), sorted under the order of ``data.grid_top_k``; slots past C*A hold NaN / -1.  A value has the
    bits ``head_grid`` gives for its pair.  k <= SELECT_MAX_K, at most SELECT_MAX_T temperatures, C*A < 2^32.
    ``where``: the (C,W) words of a pair mask (``head_grid_mask``, ``data.PairMask``): only its pairs compete
    (impnn_head_grid_topk_where), slots past their count hold NaN / -1."""
    return grid_topk(head_grid_operands(kind, mix_cat, mix_an, temperatures, head_weights, fp_size, mixing_size), k, largest, workgroups, where)


def transfer_head_grid_topk(u_cat, u_an, image, k, largest=False, workgroups=0, where=None):
    """The k best pairs of ``transfer_head_grid``'s product without the product (impnn_transfer_head_grid_topk) ->
    values (1,k) float32, cation (1,k), anion (1,k) int32 on the device, as ``head_grid_topk``; ``where`` as there
    (impnn_transfer_head_grid_topk_where)."""
    return grid_topk(transfer_grid_operands(u_cat, u_an, image), k, largest, workgroups, where)


# the limit of one partner-selecting launch: kPartnersMaxM of csrc/common.h (tests/test_partners_host.py holds them equal)
PARTNERS_MAX_M = 8
PARTNERS_TILE = {0: (16, 64), 1: (8, 32)}  # (cations, anions) of a kernel tile: head grid, transfer grid


def _grid_partners_outputs(lib, family, C_, A_, nT, m, dev):
    rows = max(nT, 1)
    need = C.c_size_t(0)
    check(lib.impnn_grid_partners_workspace_bytes(family, C_, A_, nT, m, C.byref(need)))
    out = [torch.empty(rows, n, m, dtype=dt, device=dev) for n in (C_, A_) for dt in (torch.float32, torch.int32)]
    if C_ == 0 or A_ == 0:  # zero work touches nothing: no ion has a partner
        for o in out:
            o.fill_(float("nan") if o.dtype == torch.float32 else -1)
    return out, _workspace(dev, need.value), need.value


def head_grid_partners(kind, mix_cat, mix_an, temperatures, head_weights, fp_size, mixing_size, m=1, largest=False,
                       where=None):
    """Each ion's m best partners over ``head_grid``'s product without the product (impnn_head_grid_partners): the same
    arguments -> (cat_values (nT,C,m) float32, cat_partner (nT,C,m) int32 of anion indices, an_values (nT,A,m),
    an_partner (nT,A,m) of cation indices) on the device, a plane per temperature (one for "melting_point"), ascending
    under the order of ``data.grid_best_partners``; slots past an ion's competing partners hold NaN / -1.  A value has
    the bits ``head_grid`` gives for its pair.  m <= PARTNERS_MAX_M, at most SELECT_MAX_T temperatures, C*A < 2^32.
    ``where``: the (C,W) words of a pair mask (``head_grid_mask``, ``data.PairMask``): only its pairs compete."""
    return grid_partners(head_grid_operands(kind, mix_cat, mix_an, temperatures, head_weights, fp_size, mixing_size), m, largest, where)


def transfer_head_grid_partners(u_cat, u_an, image, m=1, largest=False, where=None):
    """Each ion's m best partners over ``transfer_head_grid``'s product without the product
    (impnn_transfer_head_grid_partners) -> (cat_values (1,C,m), cat_partner, an_values (1,A,m), an_partner) on the
    device, as ``head_grid_partners``; ``where`` as there."""
    return grid_partners(transfer_grid_operands(u_cat, u_an, image), m, largest, where)


# the rank cut (csrc/grid_rank.hip): kRankDigitBits of csrc/common.h (tests/test_rank_host.py holds them equal)
RANK_DIGIT_BITS = 8
RANK_MAX_PAIRS = 2 ** 32 - 2   # the entry format: a pair index stays below 2^32 - 1


def rank_passes(C_, A_):
    """Launches over the grid one rank cut of a C x A grid takes (impnn_grid_rank_passes): a pass per digit of the key
    (32 bits) and per digit that holds C * A - 1."""
    passes, top = 32 // RANK_DIGIT_BITS, max(int(C_) * int(A_) - 1, 0)
    while top:
        passes, top = passes + 1, top >> RANK_DIGIT_BITS
    return passes


def _grid_rank_outputs(lib, family, C_, A_, nT, workgroups, mask, dev):
    planes = max(nT, 1)
    if C_ * A_ > RANK_MAX_PAIRS:
        raise ValueError(f"{C_ * A_} pairs: a rank cut takes at most 2^32 - 2")
    need = C.c_size_t(0)
    check(lib.impnn_grid_rank_workspace_bytes(family, C_, A_, nT, workgroups, C.byref(need)))
    values = torch.empty(planes, dtype=torch.float32, device=dev)
    cation = torch.empty(planes, dtype=torch.int32, device=dev)
    anion = torch.empty(planes, dtype=torch.int32, device=dev)
    count = torch.empty(planes, dtype=torch.int64, device=dev)
    words = None
    if mask:
        W = int(lib.impnn_grid_mask_row_words(A_))
        words = torch.empty((nT, C_, W) if nT > 0 else (C_, W), dtype=torch.int32, device=dev)
    if C_ == 0 or A_ == 0:  # zero work touches nothing: no pair competes
        values.fill_(float("nan")), cation.fill_(-1), anion.fill_(-1), count.zero_()
        if words is not None:
            words.zero_()
    return (values, cation, anion, count, words), _workspace(dev, need.value), need.value


def head_grid_rank(kind, mix_cat, mix_an, temperatures, head_weights, fp_size, mixing_size, k, largest=False, where=None,
                   mask=False, workgroups=0):
    """The k-th best pair of ``head_grid``'s product, and with ``mask`` the k best as a packed pair mask, without the
    product (impnn_head_grid_rank): the same arguments -> (values (nT,) float32, cation (nT,), anion (nT,) int32, count
    (nT,) int64, words) on the device, an element per temperature (one for "melting_point"): the k-th entry (1-based)
    under the order of ``data.grid_top_k`` and the number of competing pairs; more than count asked for: NaN / -1 / -1.
    ``words``: None, or the int32 words (C,W), "viscosity" (nT,C,W), of the first min(k, count) pairs - the ``words`` of
    a ``data.PairMask``.  A value has the bits ``head_grid`` gives for its pair; k is any integer >= 1.  At most
    SELECT_MAX_T temperatures, C*A <= RANK_MAX_PAIRS.  ``where``: the (C,W) words of a pair mask: only its pairs
    compete."""
    return grid_rank(head_grid_operands(kind, mix_cat, mix_an, temperatures, head_weights, fp_size, mixing_size), k, largest, where, mask, workgroups)


def transfer_head_grid_rank(u_cat, u_an, image, k, largest=False, where=None, mask=False, workgroups=0):
    """The k-th best pair of ``transfer_head_grid``'s product, and with ``mask`` the k best as a packed pair mask,
    without the product (impnn_transfer_head_grid_rank) -> (values (1,), cation (1,), anion (1,), count (1,), words
    (C,W) or None) on the device, as ``head_grid_rank``; ``where`` as there."""
    return grid_rank(transfer_grid_operands(u_cat, u_an, image), k, largest, where, mask, workgroups)


# ---- the Pareto front of two objectives (csrc/grid_pareto.hip, impnn_pareto_*): a filter over device planes, then the
# exact front of its few candidates on the host
PARETO_DEFAULT_CAPACITY = 4096


class ParetoFilter:
    """The staged Pareto filter over row-blocks of two (rows, A) float32 device planes: ``begin``, then ``range`` for
    every block, ``minima`` for every block, ``staircase``, ``collect`` for every block - a stage is complete before the
    next starts - and ``candidates``.  ``largest``: a flag per objective; ``capacity``: entries of the candidate arrays.
    Owns the workspace and the candidate arrays on ``device``; every call goes to the current stream."""

    def __init__(self, A, largest=(False, False), capacity=PARETO_DEFAULT_CAPACITY, device=None):
        if len(largest) != 2:
            raise ValueError("largest must hold one flag per objective")
        if int(capacity) < 1:
            raise ValueError("capacity must be >= 1")
        self.lib, self.A, self.device = _lib.load(), int(A), torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ionic_mpnn_amd runs on the MI355X HIP path only (there is no CPU fallback)")
        if self.device.index is None:  # as a tensor names its device
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.largest = (int(bool(largest[0])), int(bool(largest[1])))
        need = C.c_size_t(0)
        check(self.lib.impnn_pareto_workspace_bytes(C.byref(need)))
        self.nbytes = need.value
        self.ws = torch.empty(self.nbytes // 8, dtype=torch.int64, device=self.device)
        self.restart = False
        self._allocate(capacity)

    def _allocate(self, capacity):
        self.capacity = int(capacity)
        self.values = torch.empty(self.capacity, 2, dtype=torch.float32, device=self.device)
        self.cation = torch.empty(self.capacity, dtype=torch.int32, device=self.device)
        self.anion = torch.empty(self.capacity, dtype=torch.int32, device=self.device)

    def _block(self, f1, f2, where_words):
        require_gpu(f1, f2, where_words)
        if f1.dtype != torch.float32 or f2.dtype != torch.float32 or f1.dim() != 2 or f1.shape != f2.shape \
                or f1.shape[1] != self.A or not f1.is_contiguous() or not f2.is_contiguous() \
                or f1.device != self.device or f2.device != self.device:
            raise ValueError(f"a row-block is two contiguous float32 (rows,{self.A}) planes on {self.device}, got "
                             f"{f1.dtype} {tuple(f1.shape)} and {f2.dtype} {tuple(f2.shape)}")
        rows = int(f1.shape[0])
        if where_words is not None:
            where_words = _mask_words(where_words, rows, self.A, self.device)
        return (ptr(f1), ptr(f2), ptr(where_words) if where_words is not None else None, *self.largest), rows, where_words

    def begin(self):
        with torch.cuda.device(self.device):
            check(self.lib.impnn_pareto_begin(ptr(self.ws), self.nbytes, stream_ptr()))
        self.restart = False

    def range(self, f1, f2, where_words=None):
        lead, rows, keep = self._block(f1, f2, where_words)
        with torch.cuda.device(self.device):
            check(self.lib.impnn_pareto_range(*lead, ptr(self.ws), self.nbytes, rows, self.A, stream_ptr()))

    def minima(self, f1, f2, where_words=None):
        lead, rows, keep = self._block(f1, f2, where_words)
        with torch.cuda.device(self.device):
            check(self.lib.impnn_pareto_minima(*lead, ptr(self.ws), self.nbytes, rows, self.A, stream_ptr()))

    def staircase(self):
        with torch.cuda.device(self.device):
            check(self.lib.impnn_pareto_staircase(ptr(self.ws), self.nbytes, stream_ptr()))

    def collect(self, f1, f2, where_words=None, row0=0):
        lead, rows, keep = self._block(f1, f2, where_words)
        with torch.cuda.device(self.device):
            check(self.lib.impnn_pareto_collect(*lead, int(row0), int(self.restart), ptr(self.values), ptr(self.cation),
                                                ptr(self.anion), self.capacity, ptr(self.ws), self.nbytes, rows, self.A,
                                                stream_ptr()))
        if rows > 0 and self.A > 0:
            self.restart = False

    def header(self):
        """(key_min, key_max, competing, candidates) of the workspace's impnn_pareto_header: a device-to-host copy."""
        head = self.ws[:4].cpu().numpy()
        keys = head[:1].view(np.uint32)
        return int(keys[0]), int(keys[1]), int(head[1]), int(head[2])

    def grow(self, capacity):
        """Larger candidate arrays for a repeated collect stage; the next ``collect`` restarts the count."""
        self._allocate(capacity)
        self.restart = True

    def candidates(self):
        """-> (values (n,2) float32, cation (n,), anion (n,) int64 numpy, count, competing): the entries written, n =
        min(count, capacity), in no order; ``count`` above the capacity: ``grow`` and collect again."""
        _, _, competing, count = self.header()
        n = min(count, self.capacity)
        return (self.values[:n].cpu().numpy(), self.cation[:n].cpu().numpy().astype(np.int64),
                self.anion[:n].cpu().numpy().astype(np.int64), count, competing)


def pareto_run(filt, blocks):
    """The stages of ``filt`` over ``blocks``, a callable that yields (f1, f2, where_words, row0) for every row-block
    anew on each call, with ``collect`` repeated at a larger capacity while the count exceeds it -> ``data.ParetoFront``:
    the exact front of the candidates, finished on the host."""
    filt.begin()
    for stage in (filt.range, filt.minima):
        for f1, f2, wh, _ in blocks():
            stage(f1, f2, wh)
    filt.staircase()
    while True:
        for f1, f2, wh, row0 in blocks():
            filt.collect(f1, f2, wh, row0)
        values, cation, anion, count, competing = filt.candidates()
        if count <= filt.capacity:
            break
        filt.grow(count)
    flat = cation * filt.A + anion
    keep = data.pareto_front_of(data.select_keys(values[:, 0], bool(filt.largest[0])),
                                data.select_keys(values[:, 1], bool(filt.largest[1])), flat)
    return data.ParetoFront(values[keep].reshape(-1, 2), cation[keep], anion[keep], competing)


def pareto_front(f1, f2, largest=(False, False), where=None, capacity=None):
    """The Pareto front of two (C,A) float32 device planes (impnn_pareto_*): what ``data.pareto_front`` returns for
    their host copies.  ``where``: the (C,W) words of a pair mask; ``capacity``: entries of the first candidate arrays."""
    require_gpu(f1, f2)
    if f1.dim() != 2:
        raise ValueError(f"the two objectives must be (C,A) planes, got {tuple(f1.shape)}")
    filt = ParetoFilter(f1.shape[1], largest, PARETO_DEFAULT_CAPACITY if capacity is None else capacity, f1.device)
    if f1.shape[0] == 0 or f1.shape[1] == 0:
        return data.ParetoFront(np.empty((0, 2), np.float32), np.empty(0, np.int64), np.empty(0, np.int64), 0)
    return pareto_run(filt, lambda: [(f1, f2, where, 0)])


def head_grid_mask(kind, mix_cat, mix_an, temperatures, head_weights, fp_size, mixing_size, lo, hi):
    """``head_grid``'s product as a packed pair mask (impnn_head_grid_mask): bit (i,j[,t]) = lo <= v <= hi for the value
    v ``head_grid`` gives that element (a NaN fails; +-inf: no limit) -> int32 words (C,W), "viscosity" (nT,C,W), W =
    ceil(A / 32), pad bits 0: the ``words`` of a ``data.PairMask`` of shape (C,A) / (C,A,nT).  No (C,A) floats exist."""
    return grid_mask(head_grid_operands(kind, mix_cat, mix_an, temperatures, head_weights, fp_size, mixing_size), lo, hi)


def transfer_head_grid_mask(u_cat, u_an, image, lo, hi):
    """``transfer_head_grid``'s product as a packed pair mask (impnn_transfer_head_grid_mask) -> int32 words (C,W), as
    ``head_grid_mask``."""
    return grid_mask(transfer_grid_operands(u_cat, u_an, image), lo, hi)


# ---- the applicability domain (include/impnn.h, impnn_domain_*): the distance from a pair's latent vector mix_cat[i] +
# mix_an[j] - the head's `mixed` - to the nearest row of a reference set, the host reference is data.grid_domain
def domain_reference_chunk():
    """Reference rows per LDS chunk of the domain kernels (impnn_domain_reference_chunk): what a test sizes R by."""
    return int(_lib.load().impnn_domain_reference_chunk())


def _domain_operands(ref, exclude_self=False, **queries):
    """The rules of the ``domain_*`` calls, checked before any library call: every tensor float32 and 2-D, one width
    1 <= Mx <= HEAD_MAX_DIM, R >= 1, ``exclude_self`` with one query per reference row, everything on one GPU -> the
    contiguous tensors, the queries first."""
    named = list(queries.items()) + [("ref", ref)]
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
        if t.dim() != 2:
            raise ValueError(f"{name} must be 2-D (rows, Mx), got {tuple(t.shape)}")
    Mx = int(ref.shape[1])
    for name, t in named:
        if t.shape[1] != Mx:
            raise ValueError(f"{name} has width {t.shape[1]}, the reference rows have width {Mx}")
    if not 1 <= Mx <= HEAD_MAX_DIM:
        raise ValueError(f"Mx={Mx}: the domain kernels cover widths 1 to {HEAD_MAX_DIM}")
    if ref.shape[0] < 1:
        raise ValueError("the reference set is empty: R must be at least 1")
    if exclude_self and named[0][1].shape[0] != ref.shape[0]:
        raise ValueError(f"exclude_self needs one query per reference row, got {named[0][1].shape[0]} queries and "
                         f"{ref.shape[0]} rows")
    require_gpu(*[t for _, t in named])
    if any(t.device != ref.device for _, t in named):
        raise ValueError("the rows and the reference set must be on one device")
    return [t.contiguous() for _, t in named]


def domain_grid(mix_cat, mix_an, ref):
    """Every pair's distance to the reference set (impnn_domain_grid): ``mix_cat`` (C,Mx), ``mix_an`` (A,Mx) -
    ``head_ion_mix`` rows - and ``ref`` (R,Mx) -> (distance (C,A) float32, nearest (C,A) int32) on the device: the
    Euclidean distance from mix_cat[i] + mix_an[j] to its nearest reference row and that row's index (the lowest among
    equals); NaN / -1 where the pair's vector holds a NaN.  What ``data.grid_domain`` computes in float64."""
    mix_cat, mix_an, ref = _domain_operands(ref, mix_cat=mix_cat, mix_an=mix_an)
    C_, A_ = int(mix_cat.shape[0]), int(mix_an.shape[0])
    distance = torch.empty(C_, A_, dtype=torch.float32, device=ref.device)
    nearest = torch.empty(C_, A_, dtype=torch.int32, device=ref.device)
    with torch.cuda.device(ref.device):
        check(_lib.load().impnn_domain_grid(ptr(mix_cat), ptr(mix_an), ptr(ref), ptr(distance), ptr(nearest), C_, A_,
                                            int(ref.shape[0]), int(ref.shape[1]), stream_ptr()))
    return distance, nearest


def domain_grid_mask(mix_cat, mix_an, ref, lo, hi):
    """``domain_grid``'s distance as a packed pair mask (impnn_domain_grid_mask): bit (i,j) = lo <= distance <= hi as
    float32 for the distance ``domain_grid`` gives that pair (a NaN fails; +-inf: no limit) -> int32 words (C,W), W =
    ceil(A / 32), pad bits 0: the ``words`` of a ``data.PairMask`` of shape (C,A).  No (C,A) floats exist."""
    lo, hi = C.c_float(lo).value, C.c_float(hi).value  # as the kernels see them: float32
    if lo != lo or hi != hi:
        raise ValueError("a mask bound is NaN (an infinity means no limit)")
    mix_cat, mix_an, ref = _domain_operands(ref, mix_cat=mix_cat, mix_an=mix_an)
    C_, A_ = int(mix_cat.shape[0]), int(mix_an.shape[0])
    words = torch.empty(C_, data.mask_row_words(A_), dtype=torch.int32, device=ref.device)
    with torch.cuda.device(ref.device):
        check(_lib.load().impnn_domain_grid_mask(ptr(mix_cat), ptr(mix_an), ptr(ref), lo, hi, ptr(words), C_, A_,
                                                 int(ref.shape[0]), int(ref.shape[1]), stream_ptr()))
    return words


def domain_rows(z, ref, exclude_self=False):
    """The distance of explicit query rows ``z`` (Q,Mx) to the reference set (impnn_domain_rows) -> (distance (Q,)
    float32, nearest (Q,) int32) on the device; a row equal to mix_cat[i] + mix_an[j] gets the bits of ``domain_grid``'s
    element (i,j).  ``exclude_self``: query p skips reference row p (Q == R): with ``z`` the reference rows themselves,
    every reference row's distance to its nearest other row (NaN / -1 when R == 1)."""
    z, ref = _domain_operands(ref, bool(exclude_self), z=z)
    Q = int(z.shape[0])
    distance = torch.empty(Q, dtype=torch.float32, device=ref.device)
    nearest = torch.empty(Q, dtype=torch.int32, device=ref.device)
    with torch.cuda.device(ref.device):
        check(_lib.load().impnn_domain_rows(ptr(z), ptr(ref), int(bool(exclude_self)), ptr(distance), ptr(nearest), Q,
                                            int(ref.shape[0]), int(ref.shape[1]), stream_ptr()))
    return distance, nearest


# the limit of one diverse selection: kDiverseMaxK of csrc/common.h (tests/test_diverse_host.py holds them equal)
DIVERSE_MAX_K = 4096


def domain_diverse(mix_cat, mix_an, ref, k, where=None):
    """A diverse batch of ``k`` pairs by farthest-point selection (impnn_diverse_select): starting from every pair's
    ``domain_grid`` distance to ``ref``, k times the farthest pair that still competes is taken (the lowest i * A + j
    among equal float32 distances) and joins the reference set -> (cation (k,) int32, anion (k,) int32, distance (k,)
    float32, counts (2,) int64) on the device, without a host synchronisation: ``counts[0]`` = n picks were made (the
    slots from n on hold -1 / -1 / NaN), ``counts[1]`` pairs competed at the start.  ``distance[t]`` has the bits
    ``domain_grid`` gives pick t against ``ref`` plus the latent vectors of picks 0 .. t-1.  A pair competes while its
    distance is > 0 (not NaN, not a pair of the reference set, not chosen before) and its bit of ``where`` - the (C,W)
    words of a pair mask, or a ``data.PairMask`` - is set.  k <= DIVERSE_MAX_K, C*A < 2^32.  What ``data.grid_diverse``
    computes in float64."""
    mix_cat, mix_an, ref = _domain_operands(ref, mix_cat=mix_cat, mix_an=mix_an)
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1")
    if k > DIVERSE_MAX_K:
        raise ValueError(f"k={k}: one diverse selection takes at most {DIVERSE_MAX_K} picks")
    C_, A_, dev = int(mix_cat.shape[0]), int(mix_an.shape[0]), ref.device
    if where is not None:
        where = _mask_words(where, C_, A_, dev)
    lib = _lib.load()
    need = C.c_size_t(0)
    check(lib.impnn_diverse_workspace_bytes(C_, A_, k, C.byref(need)))
    cation = torch.empty(k, dtype=torch.int32, device=dev)
    anion = torch.empty(k, dtype=torch.int32, device=dev)
    distance = torch.empty(k, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    if C_ == 0 or A_ == 0:  # zero work touches nothing: no pair in any slot
        cation.fill_(-1), anion.fill_(-1), distance.fill_(float("nan")), counts.zero_()
        return cation, anion, distance, counts
    ws = _workspace(dev, need.value)
    with torch.cuda.device(dev):
        check(lib.impnn_diverse_select(ptr(mix_cat), ptr(mix_an), ptr(ref), None if where is None else ptr(where), k,
                                       ptr(cation), ptr(anion), ptr(distance), ptr(counts), ptr(ws), need.value, C_, A_,
                                       int(ref.shape[0]), int(ref.shape[1]), stream_ptr()))
    return cation, anion, distance, counts


def transfer_head(pooled_cat, pooled_an, weights, cfg):
    """The transfer model's head in inference, one launch (impnn_transfer_head): ``weights`` the 18 tensors in the
    order of include/impnn.h, ``cfg`` MPNNModel._transfer_cfg -> (B,1)."""
    require_gpu(pooled_cat, pooled_an, *weights)
    pooled_cat, pooled_an = f32c(pooled_cat), f32c(pooled_an)
    weights = [f32c(w) for w in weights]
    B, D = pooled_cat.shape
    out = torch.empty(B, 1, dtype=torch.float32, device=pooled_cat.device)
    table = (C.c_void_p * len(weights))(*[w.data_ptr() for w in weights])
    with torch.cuda.device(pooled_cat.device):
        check(_lib.load().impnn_transfer_head(ptr(pooled_cat), ptr(pooled_an), table, ptr(cfg["moving_mean"]),
                                              ptr(cfg["moving_variance"]), cfg["epsilon"], ptr(out), B, D,
                                              cfg["fp_size"], cfg["mixing_size"], stream_ptr()))
    return out


def _transfer_loss_operands(cat, an, cat_row, an_row, weights, y, sample_weight):
    """The operands of the transfer head's loss entries, checked once -> (cat, an, rows | None, weights, y, sw, B).
    With ``cat_row`` / ``an_row`` the first two are tables (C,D), (A,D) and the batch is the indices'; an index given
    as a host array is checked against its table here and uploaded, one that already lives on the GPU is checked for
    its dtype and length only (data.FrozenEncodings checked its values when it was built) - the rule of the sample
    weights."""
    require_gpu(cat, an, y, *weights)
    cat, an, y = f32c(cat), f32c(an), f32c(y).reshape(-1)
    weights = [f32c(w) for w in weights]
    if len(weights) != 18:
        raise ValueError("the transfer head takes 18 weight tensors (include/impnn.h)")
    if cat.dim() != 2 or an.dim() != 2 or cat.shape[1] != an.shape[1]:
        raise ValueError("the pooled operands must be (rows, D) matrices of one width")
    rows = None
    if (cat_row is None) != (an_row is None):
        raise ValueError("cat_row and an_row: both or neither")
    if cat_row is not None:
        rows = []
        for name, r, n in (("cat_row", cat_row, cat.shape[0]), ("an_row", an_row, an.shape[0])):
            if not (torch.is_tensor(r) and r.is_cuda):
                h = np.asarray(r.numpy() if torch.is_tensor(r) else r)
                if h.ndim != 1 or not np.issubdtype(h.dtype, np.integer):
                    raise ValueError(f"{name} must be a 1-d integer array")
                if h.size and (h.min() < 0 or h.max() >= n):
                    raise ValueError(f"{name} holds an index outside its table of {n} rows")
                r = torch.from_numpy(np.ascontiguousarray(h, dtype=np.int32)).to(cat.device)
            if r.dtype != torch.int32 or r.dim() != 1 or not r.is_contiguous() or r.device != cat.device:
                raise ValueError(f"{name} must be a contiguous 1-d int32 tensor on the tables' device")
            rows.append(r)
        if rows[0].numel() != rows[1].numel():
            raise ValueError("cat_row and an_row must hold one index per sample each")
        if cat.shape[0] < 1 or an.shape[0] < 1:
            raise ValueError("the tables need at least one row each")
    elif cat.shape != an.shape:
        raise ValueError("pooled_cat and pooled_an must hold one row per sample each")
    B = int(rows[0].numel()) if rows is not None else int(cat.shape[0])
    if y.numel() != B:
        raise ValueError("y must hold one value per sample")
    sw = None
    if sample_weight is not None:
        require_gpu(sample_weight)
        sw = f32c(sample_weight).reshape(-1)
        if sw.numel() != B:
            raise ValueError("sample_weight must hold one value per sample")
    return cat, an, rows, weights, y, sw, B


def _transfer_drop_args(cfg):
    drop = cfg.get("dropout")
    return drop.args() if drop is not None and drop.rate > 0.0 else (0.0, C.c_uint64(0), None, 0)


def transfer_head_loss_rows(cat_table, an_table, cat_row, an_row, weights, cfg, y, workspace, sample_weight=None,
                            keep=True):
    """The transfer head's loss over indexed rows, forward (impnn_transfer_head_loss_rows): sample b is
    (cat_table[cat_row[b]], an_table[an_row[b]]) -> (loss 0-d, pred (B), saved or None), no autograd (the training
    node is autograd.TransferHeadLoss with cfg["rows"]).  ``cfg``: MPNNModel._transfer_cfg; ``workspace``: a float
    tensor whose first word is zero; ``keep``: fill the buffer the backward reads.  With ``cat_row = an_row = None`` the
    first two arguments are the samples' own rows and the call is impnn_weighted_transfer_head_loss: the same code
    behind the load, the same bits on the gathered rows."""
    cat, an, rows, weights, y, sw, B = _transfer_loss_operands(cat_table, an_table, cat_row, an_row, weights, y,
                                                               sample_weight)
    lib = _lib.load()
    F, Mx, D = cfg["fp_size"], cfg["mixing_size"], int(cat.shape[1])
    keep = bool(keep) or bool(cfg["bn_batch"])
    n_saved = int(lib.impnn_transfer_head_saved_floats(B, F, Mx)) if keep and B else 0
    saved = torch.empty(n_saved, dtype=torch.float32, device=cat.device) if keep else None
    loss = torch.zeros((), dtype=torch.float32, device=cat.device)
    pred = torch.empty(B, dtype=torch.float32, device=cat.device)
    lam = (C.c_float * 18)(*[float(v) for v in cfg["l2"]])
    table = (C.c_void_p * 18)(*[w.data_ptr() for w in weights])
    head = (table, lam, ptr(cfg["moving_mean"]), ptr(cfg["moving_variance"]), cfg["momentum"], cfg["epsilon"],
            1 if cfg["bn_batch"] else 0, ptr(y), None if sw is None else ptr(sw), cfg["loss_kind"], cfg["delta"],
            *_transfer_drop_args(cfg), ptr(saved) if keep else None, n_saved, ptr(pred), ptr(loss), ptr(workspace),
            workspace.numel())
    with torch.cuda.device(cat.device):
        if rows is None:
            check(lib.impnn_weighted_transfer_head_loss(ptr(cat), ptr(an), *head, B, D, F, Mx, stream_ptr()))
        else:
            check(lib.impnn_transfer_head_loss_rows(ptr(cat), ptr(an), ptr(rows[0]), ptr(rows[1]), *head, B,
                                                    int(cat.shape[0]), int(an.shape[0]), D, F, Mx, stream_ptr()))
    return loss, pred, saved


def transfer_head_loss_rows_bwd(cat_table, an_table, cat_row, an_row, weights, dweights, cfg, y, dloss, saved,
                                sample_weight=None):
    """The backward of ``transfer_head_loss_rows`` (impnn_transfer_head_loss_rows_bwd): ADDS the parameter gradients
    into ``dweights[t]`` (18 entries; None: a frozen tensor, nothing is computed for it).  ``cfg`` and ``saved`` are
    the forward's.  ``cat_row = an_row = None``: impnn_weighted_transfer_head_loss_bwd on the samples' own rows,
    without dpooled."""
    cat, an, rows, weights, y, sw, B = _transfer_loss_operands(cat_table, an_table, cat_row, an_row, weights, y,
                                                               sample_weight)
    if len(dweights) != 18:
        raise ValueError("dweights: one entry (a tensor or None) per weight tensor")
    for g, w in zip(dweights, weights):
        if g is not None and (g.dtype != torch.float32 or not g.is_contiguous() or g.shape != w.shape
                              or g.device != w.device):
            raise ValueError("a gradient buffer must be a contiguous float32 tensor of its weight's shape and device")
    require_gpu(dloss, saved)
    lib = _lib.load()
    F, Mx, D = cfg["fp_size"], cfg["mixing_size"], int(cat.shape[1])
    dloss = f32c(dloss).reshape(1)
    wsn = int(lib.impnn_transfer_head_bwd_workspace_floats(B, F, Mx))
    ws = torch.empty(max(wsn, 1), dtype=torch.float32, device=cat.device)
    lam = (C.c_float * 18)(*[float(v) for v in cfg["l2"]])
    wt = (C.c_void_p * 18)(*[w.data_ptr() for w in weights])
    gt = (C.c_void_p * 18)(*[g.data_ptr() if g is not None else None for g in dweights])
    tail = (wt, gt, lam, 1 if cfg["bn_batch"] else 0, ptr(y), None if sw is None else ptr(sw), cfg["loss_kind"],
            cfg["delta"], ptr(dloss), *_transfer_drop_args(cfg), ptr(saved), saved.numel(), ptr(ws), wsn)
    with torch.cuda.device(cat.device):
        if rows is None:
            check(lib.impnn_weighted_transfer_head_loss_bwd(ptr(cat), ptr(an), *tail, None, None, B, D, F, Mx,
                                                            stream_ptr()))
        else:
            check(lib.impnn_transfer_head_loss_rows_bwd(ptr(cat), ptr(an), ptr(rows[0]), ptr(rows[1]), *tail, B,
                                                        int(cat.shape[0]), int(an.shape[0]), D, F, Mx, stream_ptr()))
