"""What tests/test_ensemble_host.py and tests/test_gpu_ensemble.py share: the members' seeds and weights, the species of a
grid, the temperatures, the cases, and a member's grid on the CPU (the oracle's encoder and head in float32), so that the
host test proves the statistic's bound attainable on the very member grids the GPU test produces."""
import numpy as np

from ionic_mpnn_amd import model as MM, synthetic, weights
from oracle import mpnn_oracle as O

VA, VB = synthetic.DEFAULT_VA, synthetic.DEFAULT_VB
KAPPA = 1.5
T_ALL = np.array([298.15, 273.15, 353.15, 323.15, 400.0], np.float32)
# name -> (kind, mixing_size, members, (C, A), temperatures); the viscosity cases with one temperature more than a
# selecting launch takes for that many members (4 up to M = 6, 2 at M = 8)
CASES = {"visc-M2-1x1": ("viscosity", 20, 2, (1, 1), 1),
         "visc-M3-16x64": ("viscosity", 20, 3, (16, 64), 3),
         "visc-M8-17x65": ("viscosity", 20, 8, (17, 65), 3),
         "visc-M3-33x130": ("viscosity", 20, 3, (33, 130), 5),
         "mp20-M2-17x65": ("melting_point", 20, 2, (17, 65), 0),
         "mp64-M8-33x130": ("melting_point", 64, 8, (33, 130), 0),
         "mp64-M3-16x64": ("melting_point", 64, 3, (16, 64), 0)}


def atom_dim_of(i, mixed_dims=False):
    return 64 if mixed_dims and i % 2 == 1 else 32


def member_weights(kind, i, mixing_size=20, mixed_dims=False):
    """Member i's weights: seed 11 + 7 i, one message-passing step, atom_dim 32 (``mixed_dims``: 64 for the odd members)."""
    d = atom_dim_of(i, mixed_dims)
    return weights.init_weights(kind, VA, VB, atom_dim=d, bond_dim=8 if kind == "viscosity" else d * d,
                                mixing_size=mixing_size, num_steps=1, seed=11 + 7 * i)


def build_members(kind, M, device, mixing_size=20, mixed_dims=False):
    out = []
    for i in range(M):
        d = atom_dim_of(i, mixed_dims)
        if kind == "viscosity":
            m = MM.build_model(VA, VB, atom_dim=d, mixing_size=mixing_size, num_steps=1, device=device)
        else:
            m = MM.build_melting_point_model(VA, VB, atom_dim=d, mixing_size=mixing_size, num_steps=1, device=device)
        m.load_weights(member_weights(kind, i, mixing_size, mixed_dims))
        out.append(m)
    return out


def species(C, A):
    """C cation and A anion species (dicts of int32 arrays), the same for every test."""
    b = synthetic.make_batch(max(C, A), max_atoms=24, max_edges=48, seed=5, with_temperature=False)
    return ({k: b[f"cat_{k}"][:C] for k in MM.ION_KEYS}, {k: b[f"an_{k}"][:A] for k in MM.ION_KEYS})


def temperatures(nT):
    return T_ALL[:nT] if nT else None


def cpu_member_grid(kind, w, cat, an, T):
    """One member's grid in float32 on the CPU: the oracle's encoder per species, then the head on every pair ->
    (C,A,nT) or (C,A)."""
    f = np.float32
    c = lambda a: np.asarray(a, dtype=f)
    mix = []
    for p, ion in (("cat", cat), ("an", an)):
        fp = O.encode(w, p, ion["atom"], ion["bond"], ion["connectivity"], f)
        mix.append(O.dense(fp, c(w[f"{p}_proj/kernel"]), c(w[f"{p}_proj/bias"]), "relu"))
    mixed = (mix[0][:, None, :] + mix[1][None, :, :]).astype(f)
    C, A, Mx = mixed.shape
    flat = mixed.reshape(C * A, Mx)
    if kind == "viscosity":
        vp = O.dense(flat, c(w["visc_params/kernel"]), c(w["visc_params/bias"])).reshape(C, A, 3)
        Bp = np.clip(O._softplus(vp[..., 1:2]), 0.0, 20.0).astype(f)
        Cp = np.clip(O._softplus(vp[..., 2:3]), 0.1, 50.0).astype(f)
        return (vp[..., 0:1] + Bp / (c(T)[None, None, :] / f(100.0) + Cp + f(1e-6))).astype(f)
    x = O.dense(flat, c(w["mp_hidden/kernel"]), c(w["mp_hidden/bias"]), "relu")
    return O.dense(x, c(w["mp_out/kernel"]), c(w["mp_out/bias"])).reshape(C, A).astype(f)


def cpu_member_grids(name):
    kind, mixing, M, (C, A), nT = CASES[name]
    cat, an = species(C, A)
    return np.stack([cpu_member_grid(kind, member_weights(kind, i, mixing), cat, an, temperatures(nT)) for i in range(M)])


def stats64(member_grids, kappa):
    """The reference: the statistic in float64 of the float32 member values."""
    v = np.asarray(member_grids, dtype=np.float64)
    mean, std = v.mean(axis=0), v.std(axis=0)
    return mean, std, mean + float(np.float32(kappa)) * std
