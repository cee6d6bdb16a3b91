"""Host reference of the typed chunk record's run and group tables (csrc/encoder_plan.hip, plan_chunks_typed, P3 / P4;
the layout: csrc/encoder_layout.h, kTRecGrp), and the batch compositions the run order is tested on.  Plain numpy; shared
by tests/test_run_order_host.py and tests/test_gpu_run_order.py.

A chunk's valid edges are grouped by bond type in groups of <= 4; the groups of a type are cut into pieces of <= gmax
groups (gmax = max(2, ceil(groups of the chunk / RUN_TARGET))), and one piece is one run of the encoder's message phase.
The run table lists the pieces by length descending, then type ascending, then piece index ascending, and the group table
lies in run order: run i covers groups [runs[i], runs[i + 1]).
"""
import collections
from functools import lru_cache

import numpy as np

import plan_cases as PC

RUN_TARGET = 32   # enc::kTRunTarget

RunTable = collections.namedtuple("RunTable", "hist gmax nrun runs run_type grp_type grp_edges")


def chunk_type_histogram(case, ion, first_mol, count):
    """Valid edges per bond type over molecules [first_mol, first_mol + count) of ion `ion` (0 / 1), by the rule
    plan_cases.valid_edges mirrors."""
    p = PC.IONS[ion]
    conn = case.inp[f"{p}_connectivity"][first_mol:first_mol + count]
    bond = case.inp[f"{p}_bond"][first_mol:first_mol + count]
    ok = PC.valid_edges(conn, bond, case.N, case.Vb)
    return np.bincount(bond[ok].astype(np.int64), minlength=case.Vb).astype(np.int64)


def pieces_of(hist, gmax):
    """[(length, type, piece index)] in table order: length descending, type ascending, piece ascending."""
    out = []
    for t, n in enumerate(hist):
        ng = (int(n) + 3) // 4
        full, rem = divmod(ng, gmax)
        out += [(gmax, t, i) for i in range(full)]
        if rem:
            out.append((rem, t, full))
    return sorted(out, key=lambda x: (-x[0], x[1], x[2]))


def run_table(hist):
    """The run table (+ end entry) and per group its type and edge count, from a chunk's per-type edge counts."""
    hist = np.asarray(hist, np.int64)
    ngrp = int(((hist + 3) // 4).sum())
    gmax = max(2, (ngrp + RUN_TARGET - 1) // RUN_TARGET)
    runs, run_type, grp_type, grp_edges = [], [], [], []
    for length, t, i in pieces_of(hist, gmax):
        runs.append(len(grp_type))
        run_type.append(t)
        for jg in range(i * gmax, i * gmax + length):   # the type's jg-th group holds its edges 4 jg .. 4 jg + 3
            grp_type.append(t)
            grp_edges.append(min(4, int(hist[t]) - 4 * jg))
    runs.append(len(grp_type))
    return RunTable(hist, gmax, len(run_type), np.array(runs, np.int64), np.array(run_type, np.int64),
                    np.array(grp_type, np.int64), np.array(grp_edges, np.int64))


def chunk_run_table(case, ion, first_mol, count):
    return run_table(chunk_type_histogram(case, ion, first_mol, count))


def check_run_table(hist, nrun, runs, grp_type, grp_edges, what="chunk"):
    """The properties a run table must hold whoever made it.  Raises AssertionError naming the first run that breaks one."""
    hist = np.asarray(hist, np.int64)
    runs, grp_type, grp_edges = (np.asarray(a, np.int64) for a in (runs, grp_type, grp_edges))
    ngrp = int(((hist + 3) // 4).sum())
    gmax = max(2, (ngrp + RUN_TARGET - 1) // RUN_TARGET)
    assert runs.shape == (nrun + 1,), f"{what}: {runs.size} run entries for {nrun} runs and the end"
    assert grp_type.shape == (ngrp,) and grp_edges.shape == (ngrp,), f"{what}: {grp_type.size} groups, the edges make {ngrp}"
    assert runs[0] == 0 and runs[nrun] == ngrp, f"{what}: the runs cover [{runs[0]}, {runs[nrun]}), the groups are [0, {ngrp})"
    lens = np.diff(runs)
    assert (lens >= 1).all(), f"{what}: run {int(np.argmax(lens < 1))} is empty or runs backwards: the runs do not tile"
    assert (lens <= gmax).all(), f"{what}: run {int(np.argmax(lens > gmax))} has {lens.max()} groups, gmax is {gmax}"
    up = np.nonzero(np.diff(lens) > 0)[0]
    assert up.size == 0, f"{what}: run {up[0] + 1 if up.size else 0} is longer than the run before it"
    seen_rem = {}
    order = []
    for i in range(nrun):
        g0, g1 = int(runs[i]), int(runs[i + 1])
        t = int(grp_type[g0])
        assert (grp_type[g0:g1] == t).all(), f"{what}: run {i} mixes bond types"
        assert (grp_edges[g0:g1 - 1] == 4).all(), f"{what}: run {i} (type {t}) has a partial group before its last"
        assert 1 <= grp_edges[g1 - 1] <= 4, f"{what}: run {i} (type {t}) ends in a group of {grp_edges[g1 - 1]} edges"
        assert t not in seen_rem, f"{what}: run {i} of type {t} lies behind the type's remainder (run {seen_rem.get(t)})"
        ng_t = (int(hist[t]) + 3) // 4
        if g1 - g0 < gmax or grp_edges[g1 - 1] < 4:
            seen_rem[t] = i   # the piece that ends the type: shorter than gmax, or with the type's partial group
        order.append((-(g1 - g0), t))
        assert ng_t >= 1, f"{what}: run {i} has type {t}, which has no edge"
    assert order == sorted(order), f"{what}: runs of one length are not in type order"
    for t in range(hist.size):
        got = int(grp_edges[grp_type == t].sum())
        assert got == hist[t], f"{what}: the groups of type {t} hold {got} edges, the chunk has {hist[t]}"
        mine = [i for i in range(nrun) if grp_type[runs[i]] == t]
        ng_t = (int(hist[t]) + 3) // 4
        assert len(mine) == (ng_t + gmax - 1) // gmax, f"{what}: type {t} with {ng_t} groups lies in {len(mine)} runs"


# ------------------------------------------------------------------------------------------------------------
# compositions: 96 molecules per ion (one: 144) of 40 atoms and <= 80 edge slots - shares of 12 molecules on 16 workgroups,
# chunks of up to 256 rows - each for a named property of the run order; one with the 640-edge record
# ------------------------------------------------------------------------------------------------------------
B_SMALL, N_SMALL, E_SMALL = 96, 40, 80


def _typed(name, seed, Vb, draw, B=B_SMALL, N=N_SMALL, E=E_SMALL, n_atoms=None, n_edges=None):
    """Every molecule: n_atoms atoms (default N), n_edges(rng, b) valid edges whose types come from draw(rng, b, n)."""
    rng = np.random.default_rng(seed)
    ions = []
    for _ in PC.IONS:
        ion = (np.zeros((B, N), np.int32), np.zeros((B, E), np.int32), np.zeros((B, E, 2), np.int32))
        for b in range(B):
            na = N if n_atoms is None else n_atoms
            ne = E if n_edges is None else int(n_edges(rng, b))
            PC._fill(rng, ion, b, na, ne, PC.VA, Vb)
            if ne:
                ion[1][b, :ne] = draw(rng, b, ne)
        ions.append(ion)
    return PC._case(name, ions, N, E, Vb=Vb, workgroups=16)


def uniform_71():
    """71 types drawn uniformly, 50 .. 80 edges per molecule: runs of one and two groups, many ties."""
    return _typed("uniform_71", 201, 71, lambda rng, b, n: rng.integers(0, 71, size=n),
                  n_edges=lambda rng, b: rng.integers(50, 81))


def three_long():
    """Three types, 70 .. 80 edges per molecule: six molecules make > 100 groups, gmax >= 3, every type is cut and has a
    remainder in most chunks."""
    return _typed("three_long", 202, 3, lambda rng, b, n: rng.choice(3, size=n, p=[0.55, 0.3, 0.15]),
                  n_edges=lambda rng, b: rng.integers(70, 81))


def one_type():
    """Type 2 of 5 only."""
    return _typed("one_type", 203, 5, lambda rng, b, n: np.full(n, 2), n_edges=lambda rng, b: rng.integers(60, 81))


def empty_between():
    """144 molecules per ion: shares of 18 molecules, three chunks of six.  Molecules 6 .. 11 of every share have atoms and
    no valid edge: a chunk with nrun = 0 between two chunks of the same workgroup that have edges."""
    return _typed("empty_between", 204, 7, lambda rng, b, n: rng.integers(0, 7, size=n), B=144,
                  n_edges=lambda rng, b: 0 if (b % 18) in range(6, 12) else 80)


def equal_counts():
    """Eight types, ten edges of each in every molecule: every type has the same pieces (ties by type)."""
    return _typed("equal_counts", 205, 8, lambda rng, b, n: rng.permutation(np.repeat(np.arange(8), 10)))


def last_lane_types():
    """A vocabulary of 256 with types 252 .. 255 (the last lane's four bins) and 0, 1, 130 in use."""
    used = np.array([0, 1, 130, 252, 253, 254, 255])
    return _typed("last_lane_types", 206, 256, lambda rng, b, n: rng.choice(used, size=n),
                  n_edges=lambda rng, b: rng.integers(60, 81))


def big_record():
    """Four molecules per ion of 160 atoms and 560 .. 640 valid edges of six types: the 640-edge record, gmax = 5 or 6."""
    return _typed("big_record", 207, 6, lambda rng, b, n: rng.choice(6, size=n, p=[0.4, 0.25, 0.15, 0.1, 0.06, 0.04]),
                  B=4, N=160, E=640, n_edges=lambda rng, b: rng.integers(560, 641))


COMPOSITIONS = {f.__name__: lru_cache(maxsize=None)(f) for f in (
    uniform_71, three_long, one_type, empty_between, equal_counts, last_lane_types, big_record)}


def relabelled(case, seed=77):
    """-> (the case with its bond ids permuted, perm): new id = perm[old id]; the caller permutes the bond table's rows
    with it (new_table[perm[v]] = table[v])."""
    perm = np.random.default_rng(seed).permutation(case.Vb).astype(np.int32)
    inp = dict(case.inp)
    for p in PC.IONS:
        inp[f"{p}_bond"] = perm[case.inp[f"{p}_bond"]]
    return case._replace(name=case.name + "_relabelled", inp=inp), perm


@lru_cache(maxsize=None)
def reference(name):
    """fp64 pooled pair of a composition (oracle/torch_ref.pooled_pair), computed once."""
    import torch
    from oracle import torch_ref as R
    case = COMPOSITIONS[name]()
    w = PC.case_weights(case.Va, case.Vb)
    B = case.inp["cat_atom"].shape[0]
    step = max(1, min(64, 8192 // max(case.E, 1)))
    parts = [R.pooled_pair(w, {k: v[i:i + step] for k, v in case.inp.items()}, dtype=torch.float64)
             for i in range(0, B, step)]
    return tuple(torch.cat([p[g] for p in parts]).numpy() for g in range(2))
