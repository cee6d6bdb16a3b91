"""The numpy Philox4x32-10 of the dropout masks (include/impnn.h, impnn_dropout_mask), free of the library: the host
and GPU dropout tests and the reference trainer of tests/fit_ref.py share it."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Random123) on uint32 arrays: ctr (..., 4), key (..., 2) -> (..., 4)."""
    c = [np.asarray(ctr[..., i], np.uint64) for i in range(4)]
    k0, k1 = np.asarray(key[..., 0], np.uint64), np.asarray(key[..., 1], np.uint64)
    for i in range(10):
        if i:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M32, p0 & M32]
    return np.stack(c, -1).astype(np.uint32)


def reference_mask(seed, step, layer_word, rate, rows, D):
    """(rows, D) float32: scale where kept, 0 where dropped (include/impnn.h, impnn_dropout_mask)."""
    Q = (D + 3) // 4
    r, q = np.meshgrid(np.arange(rows, dtype=np.uint64), np.arange(Q, dtype=np.uint64), indexing="ij")
    ctr = np.stack([q, r & M32, np.full_like(r, layer_word & 0xFFFFFFFF), np.full_like(r, step & 0xFFFFFFFF)], -1)
    key = np.stack([np.full_like(r, seed & 0xFFFFFFFF), np.full_like(r, ((seed >> 32) ^ (step >> 32)) & 0xFFFFFFFF)], -1)
    words = philox4x32_10(ctr, key).reshape(rows, 4 * Q)[:, :D]
    u = (words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(rate))
    return np.where(u >= np.float32(rate), scale, np.float32(0.0)).astype(np.float32)
