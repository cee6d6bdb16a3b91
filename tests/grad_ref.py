"""A differentiable torch-CPU reference of the training path that scales to the shapes the HIP kernels switch
branches on (tests/test_gpu_train_fuzz.py, tests/test_grad_ref_host.py).  oracle/torch_ref.py follows the reference's op
schedule and materialises the (B,E,D,D) bond matrices - 1 GiB per layer at D = 128 and 8192 edge slots before autograd
copies it.  Here the message step builds A = tensordot(bond_table, W) once, (Vb,D,D), and walks the bond types that
occur: source rows of the type's valid edges times A[v], index_add_ into the target rows - O(B E D) memory.
Everything else (GatedUpdate, GlobalSumPool, the head lines) is oracle/torch_ref.py's own code, imported, not restated;
tests/test_grad_ref_host.py holds the two equal in fp64 on small multigraphs.

An edge is valid when src > 0, tgt > 0 (indices, not ids: a hole inside a molecule still sends and receives) and
0 <= bond id < Vb - the library's documented rule for out-of-range ids.  Every function takes a dtype: fp64 is the
reference of the GPU tests, fp32 the "plain f32 implementation" whose distance from fp64 shows that a bound is
attainable."""
import contextlib

import torch
import torch.nn.functional as F

from oracle import torch_ref as TR


def type_matrices(bond_table, W):
    """A[v] = sum_k bond_table[v,k] W[k]: (Vb,K) x (K,D,D) -> (Vb,D,D)."""
    return torch.tensordot(bond_table, W, dims=([1], [0]))


def valid_edges(bond_ids, conn, Vb):
    """(B,E) bool of the edges that carry a message."""
    bond_ids, conn = torch.as_tensor(bond_ids).long(), torch.as_tensor(conn).long()
    return (conn[..., 0] > 0) & (conn[..., 1] > 0) & (bond_ids >= 0) & (bond_ids < Vb)


def _typed(h, A, bond_ids, conn, N, reduce):
    B, _, D = h.shape
    bond_ids, conn = torch.as_tensor(bond_ids).long(), torch.as_tensor(conn).long()
    E = conn.shape[1]
    src, tgt, bond = conn[..., 0].reshape(-1), conn[..., 1].reshape(-1), bond_ids.reshape(-1)
    valid = valid_edges(bond_ids, conn, A.shape[0]).reshape(-1)
    base = torch.arange(B).repeat_interleave(E) * N
    rows = h.reshape(B * N, D)
    out = torch.zeros(B * N if reduce else B * E, D, dtype=h.dtype)
    where = base + tgt if reduce else torch.arange(B * E)
    order = torch.argsort(torch.where(valid, bond, torch.full_like(bond, -1)), stable=True)
    order = order[int((~valid).sum()):]                      # the valid edges, by type
    types, counts = torch.unique_consecutive(bond[order], return_counts=True)
    mats = A.unbind(0)   # (one stack in the backward instead of a (Vb,D,D) zero fill per type)
    at = 0
    for v, c in zip(types.tolist(), counts.tolist()):
        sel = order[at:at + c]
        at += c
        out.index_add_(0, where[sel], rows[(base + src)[sel]] @ mats[v].T)   # m_e = A[v] h[src_e]
    return out.reshape(B, N if reduce else E, D)


def messages_from_matrices(h, A, bond_ids, conn):
    """BondMatrixMessage in the per-bond-type schedule: (B,E,D), zero rows at masked edges."""
    return _typed(h, A, bond_ids, conn, h.shape[1], reduce=False)


def message_reduce_from_matrices(h, A, bond_ids, conn, N):
    """Reduce o BondMatrixMessage from given type matrices: (B,N,D)."""
    return _typed(h, A, bond_ids, conn, N, reduce=True)


def message_reduce(h, bond_table, W, bond_ids, conn, N):
    """Reduce o BondMatrixMessage (models/layers.py:100-117 then :57-83) from the bond embedding table."""
    return message_reduce_from_matrices(h, type_matrices(bond_table, W), bond_ids, conn, N)


def encode(w, prefix, atom_ids, bond_ids, conn, dtype=torch.float64, pooled_only=False, gated_update=None):
    """oracle/torch_ref.py's encode() with the message step above.  ``gated_update``: a stand-in for
    TR.gated_update (the dropout tests multiply its output by the layer's mask)."""
    gu = gated_update or TR.gated_update
    atom_ids, bond_ids, conn = torch.as_tensor(atom_ids), torch.as_tensor(bond_ids), torch.as_tensor(conn)
    t = lambda a: TR._t(a, dtype)
    h = F.embedding(atom_ids.long(), t(w["atom_embedding"]))
    table = t(w["bond_embedding"])
    i = 0
    while f"{prefix}_bmm_{i}/bond_transform" in w:
        g = f"{prefix}_gu_{i}"
        p = {"Wz": t(w[f"{g}/dense_z/kernel"]), "bz": t(w[f"{g}/dense_z/bias"]),
             "Wr": t(w[f"{g}/dense_r/kernel"]), "br": t(w[f"{g}/dense_r/bias"]),
             "Wh": t(w[f"{g}/dense_h/kernel"]), "bh": t(w[f"{g}/dense_h/bias"]),
             "gamma": t(w[f"{g}/layernorm/gamma"]), "beta": t(w[f"{g}/layernorm/beta"])}
        agg = message_reduce(h, table, t(w[f"{prefix}_bmm_{i}/bond_transform"]), bond_ids, conn, h.shape[1])
        h = gu(h, agg, p)
        i += 1
    pooled = TR.global_sum_pool(h, atom_ids)
    if pooled_only:
        return pooled
    return torch.relu(pooled @ t(w[f"{prefix}_fp/kernel"]) + t(w[f"{prefix}_fp/bias"]))


@contextlib.contextmanager
def _encode_in_torch_ref(gated_update):
    """oracle/torch_ref.py's model functions look ``encode`` up in their module: while this holds they run with the
    scalable one, so their head lines are used as they stand."""
    saved = TR.encode
    TR.encode = lambda w, prefix, a, b, c, dtype=torch.float32, pooled_only=False: encode(
        w, prefix, a, b, c, dtype, pooled_only, gated_update)
    try:
        yield
    finally:
        TR.encode = saved


def viscosity_forward(w, inputs, dtype=torch.float64, gated_update=None):
    with _encode_in_torch_ref(gated_update):
        return TR.viscosity_forward(w, inputs, dtype)


def melting_point_forward(w, inputs, dtype=torch.float64, gated_update=None):
    with _encode_in_torch_ref(gated_update):
        return TR.melting_point_forward(w, inputs, dtype)


def model_loss(kind, w, inputs, y, fp_l2, dtype=torch.float64, gated_update=None):
    """keras "mse" + the l2 penalties of the fingerprint (and, melting point, the hidden) Dense kernels."""
    fwd = viscosity_forward if kind == "viscosity" else melting_point_forward
    pred = fwd(w, inputs, dtype, gated_update)
    names = ["cat_fp/kernel", "an_fp/kernel"] + (["mp_hidden/kernel"] if kind == "melting_point" else [])
    return torch.mean((pred.reshape(-1) - torch.as_tensor(y, dtype=dtype).reshape(-1)) ** 2) \
        + fp_l2 * sum((w[n] ** 2).sum() for n in names)
