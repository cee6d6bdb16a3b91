"""Deterministic adversarial batches for the wide encoder (csrc/encoder_wide.hip and csrc/wide_*.hip, atom_dim 64 /
128), shared by tests/test_gpu_wide_fuzz.py, tests/wide_child.py and tests/test_wide_cases_host.py.

A case is `build(name, D)`: shapes, inputs, weights (weights.init_weights(..., perturb=True)) and
  * its premises as a function of the CU count - the launcher's rules (choose_launch, csrc/encoder_wide.hip), so that a test
    can ASSERT which kernels the case reaches instead of assuming it;
  * a numpy restatement of the plan kernels (wide_count / wide_scan): valid edges by the valid_type rule, kept rows per
    molecule, ion bases aligned to 128 rows, valid-edge counts per (ion, bond type), in-degrees; and from it the
    molecules that sit where the update kernels change behaviour (last round of the 128-row kernel, ion tails, the gap
    in front of ion 1).

Every case mixes: id-0 holes, all-padding molecules (first and last of each ion, one inside, one with edges but no
atoms), self loops, a hub with in-degree E, 4x duplicated bonds (oracle.preprocess_edges_and_bonds), molecules of
1..N atoms, and one designed molecule whose rows have exactly 0, 1, 2 and 3 in-edges around the direct-source cut
(rows with <= 2 in-edges name their messages, the others are summed by wide_reduce)."""
from functools import lru_cache

import numpy as np

from ionic_mpnn_amd import weights
from oracle import mpnn_oracle as O

ROW_ALIGN = 128   # an ion's first compact row (wide::kRowAlign); the rows of wide_update_x3b_kernel's tiles
VA, K = 20, 8
DIMS = (64, 128)
MODES = ("f32t", "f32x3")

# name -> shape, and the kernels the launcher must choose for it (premises): tile16 - the 16-row update kernels;
# big128 - wide_update_x3b_kernel in mode f32x3; mpw4 - four molecules per wave in wide_count / wide_place; mini - a
# last, partial round of 128-row tiles cut into 16-row pieces
SHAPES = {
    "small":   dict(B=48, N=24, E=96, Vb=7, S=3, full=0.0, expect=dict(tile16=True, big128=False, mpw4=False)),
    "mid":     dict(B=70, N=64, E=128, Vb=7, S=2, full=0.0, expect=dict(tile16=False, big128=False, mpw4=False)),
    "many":    dict(B=520, N=16, E=24, Vb=7, S=2, full=0.0, expect=dict(tile16=False, big128=False, mpw4=True)),
    "big":     dict(B=520, N=64, E=128, Vb=7, S=2, full=0.75,
                    expect=dict(tile16=False, big128=True, mpw4=True, mini=True)),
    "runs":    dict(B=70, N=64, E=128, Vb=40, S=2, full=0.0, expect=dict(tile16=False, big128=False, mpw4=False)),
    "noanion": dict(B=70, N=64, E=128, Vb=7, S=2, full=0.0, expect=dict(tile16=False, big128=False, mpw4=False)),
}
CASES = tuple(SHAPES)
# the halves of a shard-concatenation check take other kernels than the whole batch
HALF_EXPECT = {"mid": dict(tile16=True), "noanion": dict(tile16=True), "big": dict(big128=False, mpw4=False, tile16=False)}
WHOLE_BATCH = ("small", "mid", "runs", "noanion")   # compared with the oracle molecule for molecule; the others by sample

# in-degrees of the designed molecule's rows (degree_molecule)
DESIGNED_DEGREES = {0: 0, 1: 0, 2: 1, 3: 2, 4: 3, 5: 2, 6: 1, 7: 1, 8: 0, 9: 2, 10: 2, 11: 3, 12: 1}


def tile_edges(D):
    """Edges of a message tile (wide::tile_edges): a type's run is padded to whole tiles."""
    return 64 if D >= 128 else 128


def run_counts(D):
    """The designed valid-edge counts of the `runs` case, in type order: 0, 1, te-1, te, an empty type between two full
    ones, te+1, 2te+3, and one more empty / full pair."""
    te = tile_edges(D)
    return [0, 1, te - 1, te, 0, te, te + 1, 2 * te + 3, 0, te]


# ------------------------------------------------------------------------------------------------------------
# molecules: (ids (N,), conn (E, 2), bond (E,))
# ------------------------------------------------------------------------------------------------------------
def _empty(N, E):
    return np.zeros(N, np.int32), np.zeros((E, 2), np.int32), np.zeros(E, np.int32)


def random_molecule(rng, N, E, Vb, full=False):
    """1..N atoms with id-0 holes, 0..E edges in scattered slots between atoms 0..n+1: an endpoint 0 makes the edge
    invalid, an endpoint >= n names a padding atom.  `full`: the last atom exists (N kept rows)."""
    ids, conn, bond = _empty(N, E)
    n = N if full else int(rng.integers(1, N + 1))
    ids[:n] = rng.integers(1, VA, size=n)
    ids[:n][rng.random(n) < 0.2] = 0
    if full:
        ids[N - 1] = 1 + int(rng.integers(0, VA - 1))
    ne = int(rng.integers(0, E + 1))
    slots = rng.choice(E, size=ne, replace=False)
    conn[slots] = rng.integers(0, min(N, n + 2), size=(ne, 2))
    bond[:] = rng.integers(0, Vb, size=E)
    return ids, conn, bond


def degree_molecule(rng, N, E, Vb):
    """Rows with exactly 0, 1, 2 and 3 in-edges (DESIGNED_DEGREES): degree 1 from a plain edge, from a self loop, from a
    hole (atom 8 has id 0) and from a padding atom behind the molecule (N-1); degree 2 from two edges, from a duplicated
    edge, from a self loop and an edge, and from two slots in different 64-slot groups of wide_place (slots 3 and 70
    where E > 64); degree 3 from three edges and from a duplicated edge and one more."""
    assert N >= 14 and E >= 20
    ids, conn, bond = _empty(N, E)
    ids[:13] = rng.integers(1, VA, size=13)
    ids[8] = 0
    far = (3, 70 if E > 64 else E - 1)
    conn[far[0]], conn[far[1]] = (2, 9), (4, 9)
    edges = [(1, 2), (1, 3), (2, 3), (1, 4), (2, 4), (3, 4), (1, 5), (1, 5), (6, 6), (8, 7), (10, 10), (3, 10),
             (5, 11), (5, 11), (2, 11), (N - 1, 12)]
    free = np.setdiff1d(np.arange(E), far)
    slots = rng.choice(free, size=len(edges), replace=False)   # any slot order: a row's sum follows the slots
    conn[slots] = np.asarray(edges, np.int32)
    bond[:] = rng.integers(0, Vb, size=E)
    return ids, conn, bond


def hub_molecule(rng, N, E, Vb):
    """Atom 3 receives every edge slot (in-degree E) - from itself, from holes and from padding atoms too."""
    ids, conn, bond = _empty(N, E)
    n = max(4, N // 2)
    ids[:n] = rng.integers(1, VA, size=n)
    ids[5 % n] = 0
    conn[:, 0] = rng.integers(1, N, size=E)
    conn[:, 1] = 3
    bond[:] = rng.integers(0, Vb, size=E)
    return ids, conn, bond


def dup4_molecule(rng, N, E, Vb):
    """Every bond four times: the trainer's expansion (a reverse edge per entry) of an edge list that already holds
    both directions, twice."""
    ids, _, _ = _empty(N, E)
    ids[:4] = rng.integers(1, VA, size=4)
    edges = [(1, 2), (2, 1), (2, 3), (3, 2)] * 2
    bonds = [1 % Vb, 1 % Vb, 2 % Vb, 2 % Vb] * 2
    conn, bond = O.preprocess_edges_and_bonds([edges], [bonds], E // 2)
    return ids, conn[0], bond[0]


def padding_with_edges(rng, N, E, Vb):
    """No atom (every id 0) but valid edges: rows are kept and updated, and pool to exactly 0."""
    ids, conn, bond = _empty(N, E)
    conn[:3] = [(1, 2), (2, 1), (2, 2)]
    bond[:] = rng.integers(0, Vb, size=E)
    return ids, conn, bond


DESIGNED = {"deg": degree_molecule, "hub": hub_molecule, "dup4": dup4_molecule, "pad_edges": padding_with_edges,
            "pad": lambda rng, N, E, Vb: _empty(N, E)}


def _ion(rng, B, N, E, Vb, full, where):
    """One ion's batch: designed molecules at `where` (kind -> indices), random molecules elsewhere."""
    ids, conn, bond = np.zeros((B, N), np.int32), np.zeros((B, E, 2), np.int32), np.zeros((B, E), np.int32)
    kind_at = {b: kind for kind, bs in where.items() for b in bs}
    for b in range(B):
        if b in kind_at:
            ids[b], conn[b], bond[b] = DESIGNED[kind_at[b]](rng, N, E, Vb)
        else:
            ids[b], conn[b], bond[b] = random_molecule(rng, N, E, Vb, full=bool(rng.random() < full))
    return ids, conn, bond


def _assign_runs(rng, conn, bond, counts, Vb, reverse):
    """The `runs` case: every edge gets valid endpoints or becomes padding, then bond ids are dealt so that the first
    len(counts) types (the last ones for `reverse`) hold exactly `counts` edges; the other edges go to the types in
    between, the type at the far end stays empty."""
    src, tgt = conn[:, :, 0], conn[:, :, 1]
    bad = (src <= 0) | (tgt <= 0)
    conn[bad] = 0
    bond[bad] = 0                                  # id 0 in a padding slot counts for no type
    where = np.argwhere(~bad)
    where = where[rng.permutation(len(where))]
    assert len(where) >= sum(counts) + 1, "too few valid edges for the designed runs"
    ty = np.empty(len(where), np.int32)
    at = 0
    for t, c in enumerate(counts):
        ty[at:at + c] = Vb - 1 - t if reverse else t
        at += c
    lo, hi = len(counts), Vb - 1                   # the other types, [lo, hi): one end of the vocabulary stays empty
    rest = rng.integers(lo, hi, size=len(where) - at)
    ty[at:] = Vb - 1 - rest if reverse else rest
    bond[where[:, 0], where[:, 1]] = ty


class Case:
    def __init__(self, name, D, B=None, seed=0):
        sh = SHAPES[name]
        self.name, self.D, self.K, self.S, self.Va, self.Vb = name, D, K, sh["S"], VA, sh["Vb"]
        self.B, self.N, self.E = int(B or sh["B"]), sh["N"], sh["E"]
        self.expect = sh["expect"]
        B, N, E, Vb = self.B, self.N, self.E, self.Vb
        assert B >= 16
        rng = np.random.default_rng(1000 * (CASES.index(name) + 1) + D + seed)
        # designed molecules: an all-padding molecule first and last in each ion; the others at the front of the
        # cation batch and at the back and in the middle of the anion batch
        self.where = [{"pad": [0, 5, B - 1], "deg": [1], "hub": [2], "dup4": [3], "pad_edges": [4]},
                      {"pad": [0, B - 6, B - 1], "deg": [B - 2, B // 2], "hub": [B - 3], "dup4": [B - 4],
                       "pad_edges": [B - 5]}]
        cat = _ion(rng, B, N, E, Vb, sh["full"], self.where[0])
        an = _ion(rng, B, N, E, Vb, sh["full"], self.where[1])
        if name == "noanion":                       # the whole anion is padding: ion 1 has no rows
            an = tuple(np.zeros_like(a) for a in an)
            self.where[1] = {"pad": list(range(B))}
        if name == "runs":
            _assign_runs(rng, cat[1], cat[2], run_counts(D), Vb, reverse=False)
            _assign_runs(rng, an[1], an[2], run_counts(D), Vb, reverse=True)
        self.inputs = {"cat_atom": cat[0], "cat_bond": cat[2], "cat_connectivity": cat[1],
                       "an_atom": an[0], "an_bond": an[2], "an_connectivity": an[1]}
        for v in self.inputs.values():
            v.setflags(write=False)
        self.weights = weights.init_weights("viscosity", self.Va, Vb, atom_dim=D, bond_dim=K, num_steps=self.S,
                                            seed=77 + CASES.index(name), perturb=True)
        self.plan = plan_of(self.inputs, Vb)

    def as_tuple(self):
        return self.D, self.K, self.S, self.Va, self.Vb, self.inputs, self.weights

    # -- premises ---------------------------------------------------------------------------------------------
    def premises(self, cus, B=None, kept_end=None):
        """What the launcher decides for this batch on a device of `cus` CUs (choose_launch, csrc/encoder_wide.hip)."""
        mols = 2 * (self.B if B is None else B)
        rows = mols * self.N                                    # the bound it goes by: the kept rows live on the device
        t_live = -(-(self.plan["kept_end"] if kept_end is None else kept_end) // ROW_ALIGN)
        return {"tile16": 4 * (-(-rows // 64)) <= 2 * cus, "big128": rows >= 2 * cus * ROW_ALIGN, "mpw4": mols > 1024,
                "mini": cus < t_live and t_live % cus != 0}

    def check_premises(self, cus):
        got = self.premises(cus)
        wrong = {k: got[k] for k, v in self.expect.items() if got[k] != v}
        assert not wrong, f"case {self.name} (B={self.B}, N={self.N}) on {cus} CUs does not reach its kernels: {wrong}"

    def half(self):
        """Where the shard-concatenation checks cut the batch (an uneven cut)."""
        return self.B // 2 - 3

    def check_half_premises(self, cus):
        for B in (self.half(), self.B - self.half()):
            got = self.premises(cus, B=B)
            wrong = {k: got[k] for k, v in HALF_EXPECT[self.name].items() if got[k] != v}
            assert not wrong, f"a half of case {self.name} (B={B}) on {cus} CUs takes the whole batch's kernels: {wrong}"

    # -- named molecules --------------------------------------------------------------------------------------
    def named(self, cus):
        """(ion, molecule) lists: `tail<g>` - molecules with rows in ion g's last 128-row tile; `gap` - the last molecule
        with rows of ion 0 and the first of ion 1 (either side of the aligned gap); `mini` - molecules with rows in the
        last, partial round of 128-row tiles (16-row pieces), empty where the case has none."""
        p, out = self.plan, {"gap": [], "mini": []}
        for g in (0, 1):
            kept, rb = p["kept"][g], p["rowbase"][g]
            have = np.flatnonzero(kept > 0)
            if not len(have):
                out[f"tail{g}"] = []
                continue
            end = p["base"][g] + p["rows"][g]
            tile0 = (end - 1) // ROW_ALIGN * ROW_ALIGN
            out[f"tail{g}"] = [(g, int(b)) for b in have if rb[b] + kept[b] > tile0]
            out["gap"].append((g, int(have[-1] if g == 0 else have[0])))
        t_live = -(-p["kept_end"] // ROW_ALIGN)
        if cus < t_live and t_live % cus != 0:
            first = t_live // cus * cus * ROW_ALIGN
            for g in (0, 1):
                kept, rb = p["kept"][g], p["rowbase"][g]
                out["mini"] += [(g, int(b)) for b in np.flatnonzero((kept > 0) & (rb + kept > first))]
        return out

    def sample(self, cus, extra=4):
        """Pair indices to compare with the oracle where the whole batch is too much for its (B, E, D, D) tensor: the
        designed molecules of both ions, the ends and the middle of every named set, a few random ones."""
        pick = set()
        for w in self.where:
            for kind, bs in w.items():
                pick.update(bs[:3])
        for mols in self.named(cus).values():
            bs = [b for _, b in mols]
            pick.update(bs[:2] + bs[len(bs) // 2:len(bs) // 2 + 1] + bs[-2:])
        rng = np.random.default_rng(5)
        pick.update(int(b) for b in rng.choice(self.B, size=extra, replace=False))
        return np.asarray(sorted(pick))


@lru_cache(maxsize=None)
def build(name, D, B=None):
    """The case `name` at atom_dim D (B: another batch size, for the premise checks).  Its arrays are read-only."""
    return Case(name, D, B)


# ------------------------------------------------------------------------------------------------------------
# the plan, restated (wide_count_kernel, wide_scan_kernel)
# ------------------------------------------------------------------------------------------------------------
def plan_of(inputs, Vb):
    kept, rowbase, counts, indeg, base, rows = [], [], [], [], [], []
    at = 0
    for p in ("cat", "an"):
        ids, bond, conn = inputs[f"{p}_atom"], inputs[f"{p}_bond"], inputs[f"{p}_connectivity"]
        B, N = ids.shape
        src, tgt = conn[:, :, 0].astype(np.int64), conn[:, :, 1].astype(np.int64)
        valid = (src > 0) & (tgt > 0) & (src < N) & (tgt < N) & (bond >= 0) & (bond < Vb)   # valid_type
        last = np.where(ids > 0, np.arange(N) + 1, 0).max(axis=1)
        emax = np.where(valid, np.maximum(src, tgt) + 1, 0).max(axis=1) if conn.shape[1] else np.zeros(B, np.int64)
        k = np.maximum(last, emax).astype(np.int64)          # rows that can send, receive or be pooled
        deg = np.zeros((B, N), np.int64)
        bb = np.repeat(np.arange(B)[:, None], conn.shape[1], axis=1)
        np.add.at(deg, (bb[valid], tgt[valid]), 1)
        kept.append(k)
        base.append(at)
        rows.append(int(k.sum()))
        rowbase.append(at + np.cumsum(k) - k)
        counts.append(np.bincount(bond[valid], minlength=Vb))
        indeg.append(deg)
        end = at + rows[-1]
        at = -(-end // ROW_ALIGN) * ROW_ALIGN                # the next ion starts at a multiple of 128 rows
    return {"kept": kept, "rowbase": rowbase, "counts": counts, "indeg": indeg, "base": base, "rows": rows,
            "kept_end": end}


def degree_census(case):
    """The set of in-degrees over the kept rows of both ions."""
    seen = set()
    for g in (0, 1):
        kept, deg = case.plan["kept"][g], case.plan["indeg"][g]
        live = np.arange(deg.shape[1])[None, :] < kept[:, None]
        seen.update(int(d) for d in np.unique(deg[live]))
    return seen


# ------------------------------------------------------------------------------------------------------------
# the fp64 oracle, in chunks
# ------------------------------------------------------------------------------------------------------------
def oracle_pooled(case, idx=None, chunk=8):
    """(cat, an) pooled states of the pairs `idx` (all of them by default) from oracle.mpnn_oracle.encode in fp64,
    `chunk` molecules at a time: its (chunk, E, D, D) tensor of edge matrices stays in the hundreds of MB."""
    idx = np.arange(case.B) if idx is None else np.asarray(idx)
    out = []
    for p in ("cat", "an"):
        parts = []
        for i in range(0, len(idx), chunk):
            sel = idx[i:i + chunk]
            parts.append(O.encode(case.weights, p, case.inputs[f"{p}_atom"][sel], case.inputs[f"{p}_bond"][sel],
                                  case.inputs[f"{p}_connectivity"][sel], pooled_only=True))
        out.append(np.concatenate(parts) if parts else np.zeros((0, case.D)))
    return out[0], out[1]
