"""Deterministic batch compositions for the plan kernels of the fused encoder (csrc/encoder_plan.hip: plan_stats,
plan_chunks, plan_chunks_typed), shared by tests/test_plan_cases_host.py and tests/test_gpu_plan_fuzz.py.  Plain numpy.

The plan deals the virtual rows of a batch to `nwg` persistent workgroups in equal contiguous shares, per ion, and cuts
every share into chunks by next-fit.  Which of its branches a batch takes depends on how molecule sizes are DISTRIBUTED
along the batch, so every composition here is built for named branches, and a test asserts from the plan it reads back
(ops.encoder_plan_layout / ops.read_plan) that they were taken:

  * compositions: COMPOSITIONS[name]() -> Case (six input arrays, N, E, Va, Vb, workgroups);
  * host rules: kept_rows, valid_edges, virtual_rows - the documented contract (include/impnn.h, encoder_layout.h);
  * host_plan: a straightforward next-fit over equal shares (the same share arithmetic as the kernels);
  * check_plan: the invariants every plan must hold, whoever made it;
  * paths: the branch names a plan went through, from its descriptors.
"""
import collections
from functools import lru_cache

import numpy as np

RCAP = 256        # virtual rows of a chunk (enc::kRCap)
PULL_ECAP = 1024  # valid edges of a pull-form chunk: 4 per virtual row (enc::kECap)
VA, VB, K, S = 9, 5, 8, 2
PATHS = ("share_lt_64", "share_ge_64", "chunk_gt_64_molecules", "empty_share", "hops_ge_8", "edge_bound_chunk",
         "row_bound_chunk", "vmin_gt_1", "window_miss")

Case = collections.namedtuple("Case", "name inp N E Va Vb workgroups")
Plan = collections.namedtuple("Plan", "rows vr nsub desc ion")   # the fields of ops.read_plan
IONS = ("cat", "an")


# ------------------------------------------------------------------------------------------------------------
# molecules.  Atom row 0 never lies on an edge (index 0 in the connectivity marks a padding slot), so a molecule of n
# atoms has its bonds among rows 1 .. n-1.
# ------------------------------------------------------------------------------------------------------------
def _ion(B, N, E):
    return np.zeros((B, N), np.int32), np.zeros((B, E), np.int32), np.zeros((B, E, 2), np.int32)


def _fill(rng, ion, b, n_atoms, n_edges, Va, Vb, first_row=0):
    """Molecule b: atoms in rows first_row .. first_row + n_atoms - 1, n_edges valid edges in the first slots between
    its rows >= 1."""
    ids, bond, conn = ion
    ids[b, first_row:first_row + n_atoms] = rng.integers(1, Va, size=n_atoms)
    if n_edges:
        lo, hi = max(first_row, 1), first_row + n_atoms
        assert hi - lo >= 1
        conn[b, :n_edges, 0] = rng.integers(lo, hi, size=n_edges)
        conn[b, :n_edges, 1] = rng.integers(lo, hi, size=n_edges)
        bond[b, :n_edges] = rng.integers(0, Vb, size=n_edges)


def _case(name, ions, N, E, Va=VA, Vb=VB, workgroups=16):
    inp = {}
    for p, (ids, bond, conn) in zip(IONS, ions):
        inp[f"{p}_atom"], inp[f"{p}_bond"], inp[f"{p}_connectivity"] = ids, bond, conn
    return Case(name, inp, N, E, Va, Vb, workgroups)


def _sized(name, sizes_per_ion, N, E, seed, edges_of=lambda n: 2 * (n - 1) if n >= 2 else 0, **kw):
    rng = np.random.default_rng(seed)
    ions = []
    for sizes in sizes_per_ion:
        ion = _ion(len(sizes), N, E)
        for b, n in enumerate(sizes):
            if n > 0:
                _fill(rng, ion, b, int(n), min(E, int(edges_of(int(n)))), kw.get("Va", VA), kw.get("Vb", VB))
        ions.append(ion)
    return _case(name, ions, N, E, **kw)


def sorted_by_size():
    """Atoms per molecule ascending 1 .. 48 along the batch, both ions: equal shares of rows start near B sqrt(jj / nw),
    not at B jj / nw - the guessed window misses."""
    sizes = 1 + np.arange(1200) * 48 // 1200
    return _sized("sorted_by_size", [sizes, sizes], 48, 96, 101)


def sorted_descending():
    sizes = (1 + np.arange(1200) * 48 // 1200)[::-1]
    return _sized("sorted_descending", [sizes, sizes], 48, 96, 102)


def halves():
    """First half single atoms without edges, second half 40 atoms and 80 valid edge slots."""
    sizes = np.array([1] * 400 + [40] * 400)
    return _sized("halves", [sizes, sizes], 40, 80, 103, edges_of=lambda n: 80 if n > 1 else 0)


def one_giant_among_tiny():
    """Molecule 150 has 250 atoms and 500 valid edges; the others two atoms (rows 1, 2; row 0 is a hole) and one bond."""
    rng = np.random.default_rng(104)
    B, N, E = 300, 256, 512
    ions = []
    for _ in IONS:
        ion = _ion(B, N, E)
        for b in range(B):
            if b == 150:
                _fill(rng, ion, b, 250, 500, VA, VB)
            else:
                _fill(rng, ion, b, 2, 0, VA, VB, first_row=1)
                ion[2][b, :2] = [(1, 2), (2, 1)]
                ion[1][b, :2] = rng.integers(0, VB)
        ions.append(ion)
    return _case("one_giant_among_tiny", ions, N, E)


def tiny_many():
    """3000 single-atom molecules per ion, no edge slots at all: plan_vmin > 1, shares and chunks of many molecules."""
    sizes = np.ones(3000, np.int64)
    return _sized("tiny_many", [sizes, sizes], 4, 0, 105)


def unequal_ions():
    """Cations of 30 - 40 atoms, anions of one atom and no bond: the ions' workgroup counts differ from the even split the
    window guess assumes."""
    rng = np.random.default_rng(106)
    return _sized("unequal_ions", [rng.integers(30, 41, size=512), np.ones(512, np.int64)], 40, 80, 107)


def fewer_than_workgroups():
    """Three molecules per ion for one workgroup per compute unit: shares without molecules."""
    return _sized("fewer_than_workgroups", [np.array([5, 12, 8]), np.array([12, 3, 7])], 12, 24, 108, workgroups=0)


def edge_bound_512():
    """20 atoms and 160 valid edge slots per molecule: 80 virtual rows from edges against 20 kept rows (ecap 512)."""
    sizes = np.full(120, 20)
    return _sized("edge_bound_512", [sizes, sizes], 24, 200, 109, edges_of=lambda n: 160)


def edge_bound_640():
    """150 atoms and 600 valid edge slots of 640 per molecule: one molecule per chunk at ecap 640."""
    sizes = np.full(120, 150)
    return _sized("edge_bound_640", [sizes, sizes], 160, 640, 110, edges_of=lambda n: 600)


def padding_stretch():
    """Molecules 200 .. 399 are all padding (ids 0, no edges)."""
    rng = np.random.default_rng(111)
    sizes = rng.integers(3, 13, size=600)
    sizes[200:400] = 0
    return _sized("padding_stretch", [sizes, sizes], 12, 24, 112)


def few_types_long_runs():
    """480 valid edges of three bond types per molecule: 120 groups of four, so the runs of a type are cut
    (gmax = ceil(120 / 32) = 4 groups)."""
    sizes = np.full(64, 130)
    return _sized("few_types_long_runs", [sizes, sizes], 130, 512, 113, edges_of=lambda n: 480, Vb=3)


HUB_DEGREES = {3: 15, 4: 16, 5: 17, 6: 18, 7: 40}   # target row -> in-degree, around the plan's 16-entry ticket list


def _hub_ion(rng, B, N, E, top):
    """Every molecule: the in-degrees of HUB_DEGREES, edge slots interleaved; molecule B // 2: one more row (8) with
    in-degree `top`."""
    ion = _ion(B, N, E)
    ids, bond, conn = ion
    ids[:] = rng.integers(1, VA, size=(B, N))
    for b in range(B):
        tgt = np.concatenate([np.full(d, t) for t, d in HUB_DEGREES.items()])
        if b == B // 2:
            tgt = np.concatenate([tgt, np.full(top, 8)])
        tgt = np.concatenate([tgt, rng.integers(9, N, size=8)])
        rng.shuffle(tgt)
        n = tgt.size
        conn[b, :n, 1] = tgt
        conn[b, :n, 0] = rng.integers(1, N, size=n)
        bond[b, :n] = rng.integers(0, VB, size=n)
    return ion


def hubs(top=255):
    rng = np.random.default_rng(114)
    return _case("hubs" if top == 255 else f"hubs_{top}", [_hub_ion(rng, 24, 30, 400, top) for _ in IONS], 30, 400)


def hubs_overflow():
    """An in-degree of 256: one more than a typed record carries."""
    return hubs(256)


COMPOSITIONS = {f.__name__: lru_cache(maxsize=None)(f) for f in (
    sorted_by_size, sorted_descending, halves, one_giant_among_tiny, tiny_many, unequal_ions, fewer_than_workgroups,
    edge_bound_512, edge_bound_640, padding_stretch, few_types_long_runs, hubs)}

# the paths every composition was built for (asserted from the plan read back), per record kind where they differ
BUILT_FOR = {
    "sorted_by_size": {"window_miss", "row_bound_chunk", "hops_ge_8"},
    "sorted_descending": {"window_miss", "row_bound_chunk"},
    "halves": {"window_miss", "share_ge_64", "share_lt_64"},
    "one_giant_among_tiny": {"vmin_gt_1", "share_lt_64", "row_bound_chunk"},
    "tiny_many": {"share_ge_64", "chunk_gt_64_molecules", "vmin_gt_1"},
    "unequal_ions": {"window_miss", "share_ge_64"},
    "fewer_than_workgroups": {"empty_share", "share_lt_64"},
    "edge_bound_512": {"edge_bound_chunk"},
    "edge_bound_640": {"edge_bound_chunk"},
    "padding_stretch": {"share_lt_64", "row_bound_chunk"},
    "few_types_long_runs": {"edge_bound_chunk"},
    "hubs": {"edge_bound_chunk"},
}


def pull_form_covers(case):
    """The pull-form records' static limits (encoder_fused_supported: max(N, ceil(E / 4)) <= 128, bond_dim <= 8)."""
    return max(case.N, (case.E + 3) // 4) <= RCAP // 2 and K <= 8


# ------------------------------------------------------------------------------------------------------------
# host rules
# ------------------------------------------------------------------------------------------------------------
def valid_edges(conn, bond, N, Vb):
    """(B, E) bool: both endpoints in [1, N) and the bond id in [0, Vb) (edge_valid of encoder_layout.h; the reference
    masks src > 0 & tgt > 0, models/layers.py:114-115, and indices out of range behave as padding)."""
    s, t = conn[..., 0].astype(np.int64), conn[..., 1].astype(np.int64)
    b = bond.astype(np.int64)
    return (s >= 1) & (s < N) & (t >= 1) & (t < N) & (b >= 0) & (b < Vb)


def kept_rows(atom_ids, conn=None, bond=None, Vb=None):
    """Per molecule: 1 + the last row with an atom id > 0 or, with edges given, the largest row on a valid edge if that
    is further out (impnn_kept_rows in include/impnn.h); 0 for an all-padding molecule."""
    B, N = atom_ids.shape
    r = np.where((atom_ids > 0).any(axis=1), N - np.argmax((atom_ids > 0)[:, ::-1], axis=1), 0)
    if conn is not None and conn.shape[1] > 0:
        ok = valid_edges(conn, bond, N, Vb)
        far = np.where(ok, np.maximum(conn[..., 0], conn[..., 1]), -1).max(axis=1)
        r = np.maximum(r, far + 1)
    return r.astype(np.int64)


def virtual_rows(rows, edges, ecap, vmin):
    """max(vmin, rows, ceil(256 edges / ecap)) (typed plans, encoder_layout.h: tvr_of_edges); ecap 0: a pull-form plan,
    ceil(edges / 4)."""
    ev = (edges + 3) // 4 if ecap == 0 else (edges * RCAP + ecap - 1) // ecap
    return np.maximum(np.maximum(rows, ev), vmin).astype(np.int64)


def molecule_tables(case, layout):
    """-> rows, edges, vr, each [n_ions][B], by the host rules (a case may hold one ion only)."""
    rows, edges, vr = [], [], []
    for p in [p for p in IONS if f"{p}_atom" in case.inp]:
        ids, bond, conn = (case.inp[f"{p}_{k}"] for k in ("atom", "bond", "connectivity"))
        r = kept_rows(ids, conn, bond, case.Vb)
        e = valid_edges(conn, bond, case.N, case.Vb).sum(axis=1).astype(np.int64)
        rows.append(r)
        edges.append(e)
        vr.append(virtual_rows(r, e, layout.ecap, layout.plan_vmin))
    return np.stack(rows), np.stack(edges), np.stack(vr)


def in_degrees(case, p):
    """(B, N) in-degree of every row over the valid edges of ion p."""
    ids, bond, conn = (case.inp[f"{p}_{k}"] for k in ("atom", "bond", "connectivity"))
    ok = valid_edges(conn, bond, case.N, case.Vb)
    deg = np.zeros(ids.shape, np.int64)
    for b in range(ids.shape[0]):
        np.add.at(deg[b], conn[b, ok[b], 1], 1)
    return deg


# ------------------------------------------------------------------------------------------------------------
# the share arithmetic of the plan (resolve_share / resolve_chain), in the kernels' float32
# ------------------------------------------------------------------------------------------------------------
F = np.float32


def xcd_slot(j, nwg):
    """Workgroup j -> share number: the first half of the shares go to the workgroups with j % 8 < 4 (a bijection)."""
    lo = (nwg >> 3) * 4 + min(nwg & 7, 4)
    r, qd = j & 7, j >> 3
    return qd * 4 + r if r < 4 else lo + qd * 4 + (r - 4)


def share_bound(tg, jj, n):
    if jj <= 0:
        return 0
    if jj >= n:
        return int(tg)
    t = int(F(tg) * F(jj) * (F(1.0) / F(n)))
    return min(max(t, 0), int(tg))


def ion_split(t0, t1, nwg):
    n0 = int(F(nwg) * F(t0) * (F(1.0) / F(t0 + t1)) + F(0.5)) if t0 + t1 > 0 else nwg // 2
    if nwg >= 2:
        n0 = min(max(n0, 1), nwg - 1)
    return n0


def share_of(j, nwg, totals):
    """-> (ion, share index in the ion, shares of the ion) of workgroup j."""
    n0 = ion_split(int(totals[0]), int(totals[1]), nwg) if len(totals) == 2 else nwg
    jp = xcd_slot(j, nwg)
    g = 0 if jp < n0 else 1
    return g, jp - (n0 if g else 0), (nwg - n0) if g else n0


def window_guess(j, nwg, n_ions, B):
    """-> (ion, first molecule) of the 256 molecules resolve_chain parks in LDS before it knows the share."""
    half = max(nwg >> 1, 1) if n_ions == 2 else nwg
    jp = xcd_slot(j, nwg)
    gg = 1 if n_ions == 2 and jp >= half else 0
    jj = jp - (half if gg else 0)
    nw = max(nwg - half, 1) if gg else half
    w_lo = max(int(F(jj) * F(B) / F(nw)) - 64, 0)
    return gg, w_lo & ~15


def host_plan(case, layout):
    """A plan by the book: equal shares of virtual rows per ion, next-fit chunks of <= 256 virtual rows."""
    rows, edges, vr = molecule_tables(case, layout)
    n_ions, B = vr.shape
    nwg = layout.nwg
    totals = vr.sum(axis=1)
    start = np.concatenate([np.zeros((n_ions, 1), np.int64), np.cumsum(vr, axis=1)], axis=1)   # prefix, + end
    nsub = np.zeros(nwg, np.int32)
    desc = np.full((nwg, layout.max_sub, 4), -1, np.int32)
    ion = np.full((nwg, layout.max_sub), -1, np.int32)
    for j in range(nwg):
        g, jj, nw = share_of(j, nwg, totals)
        t_lo, t_hi = share_bound(totals[g], jj, nw), share_bound(totals[g], jj + 1, nw)
        mine = np.nonzero((start[g, :B] >= t_lo) & (start[g, :B] < t_hi))[0]
        if mine.size == 0:
            continue
        m, end, c = int(mine[0]), int(mine[-1]) + 1, 0
        while m < end:
            e = m + 1
            while e < end and start[g, e + 1] - start[g, m] <= RCAP:
                e += 1
            z = int(edges[g, m:e].sum()) if layout.ecap else 0
            desc[j, c] = (m, e - m, z, start[g, e] - start[g, m])
            ion[j, c] = g
            m, c = e, c + 1
        nsub[j] = c
    return Plan(rows.astype(np.int32), vr.astype(np.int32), nsub, desc, ion)


# ------------------------------------------------------------------------------------------------------------
# the invariants of a plan
# ------------------------------------------------------------------------------------------------------------
def chunks_of(plan, j):
    """[(first molecule, molecules, valid edges, virtual rows, ion)] of workgroup j."""
    return [tuple(int(v) for v in plan.desc[j, c]) + (int(plan.ion[j, c]),) for c in range(int(plan.nsub[j]))]


def check_plan(case, layout, plan):
    """Raises AssertionError naming the ion, workgroup and chunk unless the plan holds every invariant."""
    rows, edges, vr = molecule_tables(case, layout)
    n_ions, B = vr.shape
    typed = layout.ecap > 0
    for g in range(n_ions):
        for what, got, want in (("rows", plan.rows, rows), ("vr", plan.vr, vr)):
            bad = np.nonzero(got[g] != want[g])[0]
            assert bad.size == 0, (f"{case.name}: ion {g}: {what} of molecule {bad[0]} is {got[g][bad[0]]}, the host rule "
                                   f"says {want[g][bad[0]]} ({bad.size} molecules differ)")
    assert plan.nsub.shape == (layout.nwg,)
    tiles = [[] for _ in range(n_ions)]
    for j in range(layout.nwg):
        n = int(plan.nsub[j])
        assert 0 <= n <= layout.max_sub, f"{case.name}: workgroup {j}: nsub {n} outside [0, max_sub = {layout.max_sub}]"
        cs = chunks_of(plan, j)
        for c, (m0, M, z, R, g) in enumerate(cs):
            at = f"{case.name}: ion {g}, workgroup {j}, chunk {c} (molecules {m0} .. {m0 + M - 1})"
            assert 0 <= g < n_ions, f"{at}: no such ion"
            assert M >= 1, f"{at}: a chunk without molecules"
            assert 0 <= m0 and m0 + M <= B, f"{at}: molecules outside the batch of {B}"
            want_r = int(vr[g, m0:m0 + M].sum())
            assert R == want_r, f"{at}: R = {R}, its molecules hold {want_r} virtual rows"
            assert R <= RCAP or M == 1, f"{at}: {R} virtual rows in {M} molecules, a chunk holds {RCAP}"
            if typed:
                want_z = int(edges[g, m0:m0 + M].sum())
                assert z == want_z, f"{at}: z = {z}, its molecules hold {want_z} valid edges"
                assert z <= layout.ecap, f"{at}: {z} valid edges, a chunk holds {layout.ecap}"
            else:
                assert z == 0, f"{at}: z = {z} in a pull-form plan"
            if c > 0:
                pm0, pM, _, pR, pg = cs[c - 1]
                assert pg == g and pm0 + pM == m0, f"{at}: not consecutive with chunk {c - 1} of the workgroup"
                assert pR + R > RCAP, (f"{at}: fits the chunk before it ({pR} + {R} <= {RCAP} virtual rows): next-fit "
                                       f"had merged them, and max_sub counts on it")
            tiles[g].append((m0, M, j, c))
    for g in range(n_ions):
        at = 0
        for (m0, M, j, c) in sorted(tiles[g]):
            assert m0 >= at, f"{case.name}: ion {g}, workgroup {j}, chunk {c}: overlap, molecule {m0} is dealt twice"
            assert m0 == at, f"{case.name}: ion {g}, workgroup {j}, chunk {c}: gap, molecules {at} .. {m0 - 1} are in no chunk"
            at = m0 + M
        assert at == B, f"{case.name}: ion {g}: gap, molecules {at} .. {B - 1} are in no chunk"


def paths(case, layout, plan):
    """The set of path names (PATHS) the plan went through.  All from the descriptors, but window_miss, which mirrors
    the guess resolve_chain makes before it knows the share."""
    rows, edges, _ = molecule_tables(case, layout)
    n_ions, B = rows.shape
    ecap = layout.ecap if layout.ecap else PULL_ECAP
    out = set()
    if layout.plan_vmin > 1:
        out.add("vmin_gt_1")
    for j in range(layout.nwg):
        cs = chunks_of(plan, j)
        if not cs:
            out.add("empty_share")
            continue
        out.add("share_lt_64" if sum(c[1] for c in cs) < 64 else "share_ge_64")
        if len(cs) >= 8:
            out.add("hops_ge_8")
        for (m0, M, z, R, g) in cs:
            if M > 64:
                out.add("chunk_gt_64_molecules")
            e = z if layout.ecap else int(edges[g, m0:m0 + M].sum())   # (pull-form descriptors carry no edge count)
            out.add("edge_bound_chunk" if e * RCAP > ecap * int(rows[g, m0:m0 + M].sum()) else "row_bound_chunk")
        gg, w_lo = window_guess(j, layout.nwg, n_ions, B)
        first, g = cs[0][0], cs[0][4]
        if g != gg or not (w_lo <= first < w_lo + 256):
            out.add("window_miss")
    return out


def guessed_other_ion(layout, plan, n_ions, B):
    """The workgroups whose share lies on the other ion than resolve_chain guessed (g != gg): the ions' workgroup counts
    follow their rows, the guess assumes an even split."""
    return [j for j in range(layout.nwg)
            if plan.nsub[j] > 0 and int(plan.ion[j, 0]) != window_guess(j, layout.nwg, n_ions, B)[0]]


# ------------------------------------------------------------------------------------------------------------
# weights and the fp64 reference (computed once per composition)
# ------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def case_weights(Va, Vb):
    from ionic_mpnn_amd import weights
    return weights.init_weights("viscosity", Va, Vb, atom_dim=32, bond_dim=K, num_steps=S, seed=41, perturb=True)


@lru_cache(maxsize=None)
def reference(name):
    """fp64 pooled pair of a composition (oracle/torch_ref.pooled_pair), in slices of <= 64 molecules (fewer where the
    per-edge matrices of a slice would not fit a few hundred MB)."""
    import torch
    from oracle import torch_ref as R
    case = hubs_overflow() if name == "hubs_256" else COMPOSITIONS[name]()
    w = case_weights(case.Va, case.Vb)
    B = case.inp["cat_atom"].shape[0]
    step = max(1, min(64, 8192 // max(case.E, 1)))
    parts = [R.pooled_pair(w, {k: v[i:i + step] for k, v in case.inp.items()}, dtype=torch.float64)
             for i in range(0, B, step)]
    return tuple(torch.cat([p[g] for p in parts]).numpy() for g in range(2))
