"""The case of the Monte-Carlo dropout tests (tests/test_mc_dropout_host.py, tests/test_gpu_mc_dropout.py): one transfer
model with random weights and non-trivial moving statistics, 19 cations x 70 anions, the fp64 reference of its S
thinned heads and a plain float32 walk of the same, free of the library's kernels.

The model is test_gpu_transfer.make_transfer's (a perturbed viscosity model cut at mix_cat_an, head kernels x 1.5,
random biases, gamma, beta and moving statistics) with one change: the last kernel (melting_point, 64 -> 1) is made
non-negative.  A thinned head whose last sum cancels gives whole sample planes that are small against their own partial
sums (with the signed kernel: planes of max |value| 8 beside planes of 82), and 1e-5 RELATIVE TO SUCH A PLANE is a bound
a plain float32 walk misses (1.1e-5 on 2 of 64 planes, above half the bound on 8).  The project's rule for such inputs
(tests/test_transfer_grid_host.py): a bound that plain f32 misses marks a hard input, not a kernel defect, and cases are
chosen so that the f32 walk stays at or below half the bound.  With relu(a3) >= 0 and a non-negative kernel the last
sum does not cancel, a plane's scale is the scale of its partial sums, and the walk stays below 1e-6
(test_mc_dropout_host.py asserts 5e-6)."""
import numpy as np
import torch

from ionic_mpnn_amd import layers as L, model as MM, ops, synthetic, weights

import transfer_ref as R
from philox_ref import reference_mask

SEED = 0x5EED_0BAD_CAFE
GRIDS = [(1, 1), (8, 32), (9, 33), (19, 70)]  # one pair, one full tile (8 x 32), one past it both ways, 3 x 3 ragged tiles
CN, AN = 19, 70
CAT_SEED, AN_SEED = 50, 51
DRAW = 3
RATE = 0.3
HALF_BOUND = 5e-6


def make_transfer(tmp_path, device, S=1, seed=1):
    Va, Vb = synthetic.DEFAULT_VA, synthetic.DEFAULT_VB
    L.reset_uids()
    L.set_init_seed(seed)
    v = MM.build_model(Va, Vb, num_steps=S, device=device)
    v.load_weights(weights.init_weights("viscosity", Va, Vb, num_steps=S, seed=seed, perturb=True))
    path = tmp_path / "viscosity_final.keras"
    v.save(str(path))
    t = MM.build_transfer_model(str(path), device=device, dropout_seed=SEED)
    rng = np.random.default_rng(seed + 100)
    head = {n: a for n, a in t.state_dict().items() if n.startswith("mp_") or n.startswith("melting_point")}
    for n, a in head.items():
        if n.endswith("kernel"):
            head[n] = (a * 1.5).astype(np.float32)
        elif n.endswith("moving_variance"):
            head[n] = rng.uniform(0.5, 2.0, size=a.shape).astype(np.float32)
        elif n.endswith("gamma"):
            head[n] = rng.uniform(0.5, 1.5, size=a.shape).astype(np.float32)
        else:
            head[n] = rng.normal(0.0, 0.2, size=a.shape).astype(np.float32)
    head["melting_point/kernel"] = np.abs(head["melting_point/kernel"])  # (the module's docstring)
    t.load_weights({**t.state_dict(), **head})
    return t


def species():
    """-> (cations, anions): CN and AN ion graphs."""
    b = synthetic.make_batch(CN, max_atoms=40, max_edges=80, seed=CAT_SEED, with_temperature=False)
    cat = {k: b[f"cat_{k}"] for k in MM.ION_KEYS}
    b = synthetic.make_batch(AN, max_atoms=40, max_edges=80, seed=AN_SEED, with_temperature=False)
    return cat, {k: b[f"an_{k}"] for k in MM.ION_KEYS}


def corner(ions, n):
    return {k: v[:n] for k, v in ions.items()}


def pooled64(state, cat, an):
    """The encoder in fp64, once per species (transfer_ref.pooled) -> (pc (C,D), pa (A,D)) float64 tensors."""
    Cn, An = len(cat["atom"]), len(an["atom"])
    n = max(Cn, An)
    w = {k: torch.tensor(np.asarray(v), dtype=R.DT) for k, v in state.items()}
    pair = {f"cat_{k}": cat[k][np.arange(n) % Cn] for k in MM.ION_KEYS}
    pair.update({f"an_{k}": an[k][np.arange(n) % An] for k in MM.ION_KEYS})
    with torch.no_grad():
        pc, pa = R.pooled(w, pair)
    return pc[:Cn], pa[:An]


def masks(draw, S, seed=SEED):
    """The numpy Philox table (S,128): row s is the training mask of batch row s at dropout step ``draw``."""
    return reference_mask(seed, draw, ops.dropout_layer_word(L.Dropout.LAYER_ID, 0), RATE, S, 128)


def reference(state, cat, an, draw, S):
    """fp64, free of the code under test: transfer_ref.head in training mode on moving statistics with the mask of sample
    s, on the expanded pair list -> samples (S,C,A) float64."""
    Cn, An = len(cat["atom"]), len(an["atom"])
    w = {k: torch.tensor(np.asarray(v), dtype=R.DT) for k, v in state.items()}
    pc, pa = pooled64(state, cat, an)
    pcg, pag = pc.repeat_interleave(An, dim=0), pa.repeat(Cn, 1)
    table = masks(draw, S)
    with torch.no_grad():
        return np.stack([R.head(w, pcg, pag, training=True, mask=table[s], bn_batch=False)[0].numpy().reshape(Cn, An)
                         for s in range(S)])


def fp32_walk(state, cat, an, draw, S):
    """The S thinned heads in plain float32 numpy, in the kernels' factored order (u rows per ion, relu of their sum,
    BatchNormalization as scale and shift, the three Dense layers), from the fp64 pooled rows rounded to float32 ->
    samples (S,C,A) float32."""
    dt = np.float32
    c = lambda n: np.asarray(state[n], dt)
    relu = lambda x: np.maximum(x, dt(0))
    pc, pa = (p.numpy().astype(dt) for p in pooled64(state, cat, an))

    def half(ion, p):
        fp = relu(p @ c(f"{ion}_fp/kernel") + c(f"{ion}_fp/bias"))
        u = relu(fp @ c(f"{ion}_proj/kernel") + c(f"{ion}_proj/bias")) @ c("mp_dense_1/kernel")
        return u + c("mp_dense_1/bias") if ion == "an" else u

    scale = c("mp_bn_1/gamma") / np.sqrt(c("mp_bn_1/moving_variance") + dt(R.BN_EPS))
    shift = c("mp_bn_1/beta") - c("mp_bn_1/moving_mean") * scale
    bn = relu(half("cat", pc)[:, None, :] + half("an", pa)[None, :, :]) * scale + shift
    a2 = relu(bn @ c("mp_dense_2/kernel") + c("mp_dense_2/bias"))
    out = []
    for m in masks(draw, S):
        a3 = relu((a2 * m) @ c("mp_dense_3/kernel") + c("mp_dense_3/bias"))
        out.append((a3 @ c("melting_point/kernel") + c("melting_point/bias"))[..., 0])
    return np.stack(out)


def spread_fraction(samples):
    """The fraction of pairs whose std over the samples exceeds 1e-3 of max|mean|: a test of the spread must see one."""
    mean, std = samples.mean(0), samples.std(0)
    return float((std > 1e-3 * np.abs(mean).max()).mean())
