"""The host layer of a screen over the cation x anion grid: the argument rules, the encoded rows, the host tiling of the
cation and the temperature axis, and the merges of the tiles' results - everything between a model's public ``screen_*`` /
``predict_grid`` methods (model.py, ensemble.py, mc_dropout.py, pareto.py: argument names, docstrings) and the
operations over ``ops.GridOperands`` (ops.py: the launches).

What a screen requires of its model, and nothing else:
  * ``kind`` ("viscosity", "melting_point", "transfer"), ``device``, ``grid_head_mode``;
  * ``encode_ions(cations, anions, batch_size)`` -> the pooled rows (C,D), (A,D) on ``device``;
  * ``_grid_kernels_cover()`` / ``_transfer_grid_covers()``: some grid kernel covers the widths;
  * ``_grid_operands(pc, pa, T, mfma)`` -> ``ops.GridOperands`` of the whole grid, where one does;
  * ``_grid_gathered(pc, pa, T)`` -> the head on a tile's explicit pairs (c,A[,nT]), where none does;
  * the domain functions also: ``_packed_head()``, ``fp_size``, ``mixing_size`` (and ``atom_dim`` in a refusal).
The fallback paths (no covering kernel) touch the device through ``_grid_gathered`` alone, so with a stand-in model
they run on the CPU: tests/test_screening_host.py holds the tiling and every merge against the ``data.*`` references."""
from __future__ import annotations

import numpy as np
import torch

from . import data, ops

ION_KEYS = ("atom", "bond", "connectivity")
# predict_grid: elements of `out` one launch may write (1 GiB of float32); above it the cation axis is tiled on the host
GRID_OUTPUT_BUDGET = 1 << 28
GRID_MAX_TEMPERATURES = 4096   # temperatures per impnn_head_grid launch (include/impnn.h)
GRID_GATHER_PAIRS = 1 << 18    # pairs per tile of the gathered path (widths above 64, the transfer head)
SCREEN_MAX_K = ops.SELECT_MAX_K       # screen_top_k: the largest k the selecting kernels keep (above it: the fallback)
SCREEN_MAX_PAIRS = (1 << 32) - 1      # pairs of one selecting launch: a pair's index has 32 bits
SUMMARY_RANGE = 16                    # screen_ion_summary cuts the cation axis at its multiples: every summary block's size divides it


def _ion_numpy(ion, what):
    """One species dict {"atom" (M,N), "bond" (M,E), "connectivity" (M,E,2)} as int32 numpy arrays."""
    if not isinstance(ion, dict) or any(k not in ion for k in ION_KEYS):
        raise KeyError(f"{what} must be a dict with the keys {ION_KEYS}")
    out = []
    for k in ION_KEYS:
        v = ion[k]
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        out.append(np.ascontiguousarray(np.asarray(v), dtype=np.int32))
    a, b, c = out
    if a.ndim != 2 or b.ndim != 2 or c.ndim != 3 or c.shape[2] != 2 or len({len(a), len(b), len(c)}) != 1 \
            or b.shape[1] != c.shape[1]:
        raise ValueError(f"{what}: atom (M,N), bond (M,E), connectivity (M,E,2) expected, got {a.shape}, {b.shape}, "
                         f"{c.shape}")
    return a, b, c


def ion_pair_batches(cations=None, anions=None, batch_size=4096):
    """The pair batches ``MPNNModel.encode_ions`` feeds to ``encode_pooled``: species lists -> (batches, C, A).

    Both sides are zero-padded to a common (N, E) - atom id 0, bond id 0 and [0, 0] edges are padding everywhere in
    the model - and to R = max(C, A) rows; the shorter or absent side is filled with all-padding molecules.  Row r of
    the batches holds cation r (r < C) and anion r (r < A); ``batches`` is a list of model input dicts (numpy int32,
    no temperature) of at most ``batch_size`` rows, in row order."""
    if cations is None and anions is None:
        raise ValueError("encode_ions needs cations, anions or both")
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    sides = [None if x is None else _ion_numpy(x, w) for x, w in ((cations, "cations"), (anions, "anions"))]
    given = [s for s in sides if s is not None]
    N = max(s[0].shape[1] for s in given)
    E = max(s[1].shape[1] for s in given)
    counts = [0 if s is None else len(s[0]) for s in sides]
    R = max(counts)
    padded = []
    for s in sides:
        atom, bond, conn = np.zeros((R, N), np.int32), np.zeros((R, E), np.int32), np.zeros((R, E, 2), np.int32)
        if s is not None:
            m = len(s[0])
            atom[:m, :s[0].shape[1]], bond[:m, :s[1].shape[1]], conn[:m, :s[2].shape[1]] = s
        padded.append((atom, bond, conn))
    batches = []
    for lo in range(0, R, batch_size):
        b = {}
        for p, arrs in zip(("cat", "an"), padded):
            for k, arr in zip(ION_KEYS, arrs):
                b[f"{p}_{k}"] = arr[lo:lo + batch_size]
        batches.append(b)
    return batches, counts[0], counts[1]


# ---------------------------------------------------------------------- the argument rules, one copy each
def mask_bounds(what, at_least, at_most, names="at_least, at_most"):
    """The bounds of a mask-writing screen as the kernels compare them -> (lo, hi) float32; a missing one is -inf /
    +inf.  ``what``: the screen's name in the messages, ``names``: the two bounds in the order of its signature."""
    if at_least is None and at_most is None:
        raise ValueError(f"{what} needs a bound: {names} or both")
    lo_b = np.float32(-np.inf if at_least is None else at_least)
    hi_b = np.float32(np.inf if at_most is None else at_most)
    if np.isnan(lo_b) or np.isnan(hi_b):
        raise ValueError(f"a {what} bound is NaN")
    return lo_b, hi_b


def at_least_one(name, v):
    """``k`` / ``m`` of a selecting screen as an int >= 1."""
    v = int(v)
    if v < 1:
        raise ValueError(f"{name} must be >= 1")
    return v


def score_kappa(kappa):
    """``kappa`` of a score mean + kappa * std as the kernels see it: the float32 value, finite."""
    with np.errstate(over="ignore"):  # (a float too large for float32 is refused below, not warned about)
        kappa = np.float32(kappa)
    if not np.isfinite(kappa):
        raise ValueError("kappa must be finite")
    return float(kappa)


def _screen_request(kind, what, cations, anions, temperatures, where, max_pairs_per_launch):
    """The argument rules the screens of a model of ``kind`` share (``what``: the screen's name in the messages) -> the
    temperatures as a float32 host tensor (nT), or None for a model without them."""
    if kind == "viscosity" and temperatures is None:
        raise KeyError("the viscosity model needs a 'temperature' input (train_viscosity.py:160)")
    if cations is None or anions is None:
        raise ValueError(f"{what} needs both cations and anions")
    if where is not None:
        if not isinstance(where, data.PairMask):
            raise TypeError(f"where must be a data.PairMask, got {type(where).__name__}")
        if len(where.shape) != 2:
            raise ValueError("where must be a 2-D mask over (cation, anion): take temperature(t) of a viscosity mask "
                             "and call per temperature")
        given = (len(cations["atom"]), len(anions["atom"]))
        if where.shape != given:
            raise ValueError(f"where has shape {where.shape}, the screen is {given[0]} cations x {given[1]} anions")
    if max_pairs_per_launch is not None:
        at_least_one("max_pairs_per_launch", max_pairs_per_launch)
    if kind != "viscosity":
        return None
    T = temperatures if isinstance(temperatures, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(np.asarray(temperatures, dtype=np.float32)))
    T = T.to(torch.float32).reshape(-1)
    if T.numel() == 0:
        raise ValueError("temperatures must hold at least one value")
    return T


def _rank_request(kind, what, cations, anions, temperatures, k, where):
    """``_screen_request`` and the two rules of a rank cut, which does not tile the cation axis -> (T, k)."""
    T = _screen_request(kind, what, cations, anions, temperatures, where, None)
    k = at_least_one("k", k)
    pairs = len(cations["atom"]) * len(anions["atom"])
    if pairs > ops.RANK_MAX_PAIRS:
        raise ValueError(f"{what}: {pairs} pairs, a rank cut takes at most 2^32 - 2")
    return T, k


# ---------------------------------------------------------------------- the host tiling, one generator per axis
def ranges(n, step):
    """(lo, hi) over 0 .. n, ``step`` at a time, in order: the temperature rows of one launch after another."""
    for lo in range(0, n, step):
        yield lo, min(n, lo + step)


def cation_ranges(C, A, pairs, most=1 << 62, multiple=1):
    """The host tiling of the cation axis of a C x A grid: (lo, hi) in order, each of at most ``pairs`` pairs (and never
    more than ``most``, a kernel's own limit) but at least ``multiple`` cations, cut at multiples of ``multiple`` only.
    Nothing for an empty grid."""
    if A > 0:
        yield from ranges(C, max(multiple, min(int(pairs), most) // A // multiple * multiple))


class _Screen:
    """The one object behind every screen: the pooled rows of ``encode_ions`` (``pc``, ``pa``), ``C``, ``A``, ``nT`` and
    ``planes`` (temperature rows: nT, or 1 for a model without temperatures), ``T`` and ``where`` on the device,
    ``mfma`` (the transfer head's matrix-core grid), ``covered`` (some grid kernel covers the model) and ``operands``:
    the ``ops.GridOperands`` of the whole grid, or None where the gathered fallback runs or the grid is empty.  Built
    after the argument check (``_screen_request``); its methods are the screens."""

    select_max_t, grid_max_t = ops.SELECT_MAX_T, GRID_MAX_TEMPERATURES  # temperature rows of one launch
    n_values = 1    # the planes of a materialised tile: ``tile_values``
    extra_axis = 0  # the cation axis of ``extra_out``

    def __init__(self, model, cations, anions, T, where, batch_size):
        self.model, self.visc = model, model.kind == "viscosity"
        self.pc, self.pa = model.encode_ions(cations, anions, batch_size)
        self.C, self.A = self._counts()
        self.nT = int(T.numel()) if self.visc else 0
        self.planes = self.nT if self.visc else 1
        self.mfma, self.covered = self._coverage()
        if where is not None and where.words.device != model.device:
            where = data.PairMask(where.words.to(model.device), where.shape)
        self.where, self.T, self.operands = where, None, None
        if self.C > 0 and self.A > 0:
            self.T = T.to(model.device) if self.visc else None
            if self.covered:
                self.operands = self._operands()

    def _operands(self):
        return self.model._grid_operands(self.pc, self.pa, self.T, self.mfma)

    def _counts(self):
        return int(self.pc.shape[0]), int(self.pa.shape[0])

    def _coverage(self):
        """(mfma, covered) of the model."""
        mfma = self.model._transfer_grid_covers() and self.model.grid_head_mode == "auto"
        return mfma, self.model._grid_kernels_cover() or mfma

    def default_pairs(self, select, workspace_per_pair=None):
        """``max_pairs_per_launch`` where the caller gives none.  A selecting launch: the most its pair index takes,
        or what keeps its workspace (``workspace_per_pair`` bytes) within 4 bytes per element of GRID_OUTPUT_BUDGET; a
        materialising one: GRID_OUTPUT_BUDGET elements of output, a gathered one GRID_GATHER_PAIRS at the most."""
        if select:
            return SCREEN_MAX_PAIRS if workspace_per_pair is None else min(
                SCREEN_MAX_PAIRS, max(1, int(4 * GRID_OUTPUT_BUDGET / workspace_per_pair)))
        pairs = max(1, GRID_OUTPUT_BUDGET // max(min(self.nT, self.grid_max_t), 1))
        return pairs if self.covered else min(pairs, GRID_GATHER_PAIRS)

    def tiles(self, max_pairs_per_launch, select, workspace_per_pair=None):
        """The host tiling: (lo, hi, t0, t1, operands, where) for every range of cations lo .. hi and of temperature
        rows t0 .. t1 of one launch - ``select``: a selecting launch (fewer than 2^32 pairs, ``select_max_t``
        temperatures), else a materialising one (``grid_max_t``) - with the operands narrowed to the tile (None: the gathered fallback)
        and the mask's rows lo .. hi (None: no mask).  Nothing for an empty grid."""
        if max_pairs_per_launch is None:
            max_pairs_per_launch = self.default_pairs(select, workspace_per_pair)
        t_step = self.select_max_t if select else self.grid_max_t
        for lo, hi in cation_ranges(self.C, self.A, max_pairs_per_launch, SCREEN_MAX_PAIRS if select else 1 << 62):
            rows = self.operands.rows(lo, hi) if self.operands is not None else None
            wh = self.where.rows(lo, hi) if self.where is not None else None
            for t0, t1 in ranges(self.planes, t_step):
                yield lo, hi, t0, t1, rows.temperatures(t0, t1) if rows is not None else None, wh

    def tile_values(self, lo, hi, t0, t1, operands, extra):
        """The tile (lo, hi, t0, t1, operands) of ``tiles``, materialised on the device -> (its ``n_values`` planes
        (hi - lo, A[, t1 - t0]), its part of ``extra_out`` or None): the head's values and, with ``extra``, from a
        covered tile's first temperature range the VFT parameters."""
        if operands is None:
            with torch.no_grad():
                return (self.model._grid_gathered(self.pc[lo:hi], self.pa, self.T[t0:t1] if self.visc else None),), None
        if extra and t0 == 0:
            tile, params = ops.grid_values(operands, return_params=True)
            return (tile,), params
        return (ops.grid_values(operands),), None

    def grid_tile(self, lo, hi, t0, t1, operands):
        """The plane of the tile the screens select from: the last of ``tile_values`` (a statistic's score)."""
        return self.tile_values(lo, hi, t0, t1, operands, False)[0][-1]

    def extra_out(self):
        """The output ``values`` fills beside the planes: the VFT parameters of every pair."""
        return np.empty((self.C, self.A, 3), np.float32)

    def values(self, max_pairs_per_launch, return_params=False):
        """The materialised grid (``MPNNModel.predict_grid``): numpy (C,A[,nT]), a tuple of them where a tile has more
        than one plane; with ``return_params`` -> (that, ``extra_out`` filled from the tiles)."""
        s = self
        out = [np.empty((s.C, s.A, s.nT) if s.visc else (s.C, s.A), np.float32) for _ in range(s.n_values)]
        extra = s.extra_out() if return_params else None
        for lo, hi, t0, t1, g, _ in s.tiles(max_pairs_per_launch, False):
            planes, part = s.tile_values(lo, hi, t0, t1, g, return_params)
            for o, tile in zip(out, planes):
                (o[lo:hi, :, t0:t1] if s.visc else o[lo:hi])[...] = tile.cpu().numpy()
            if part is not None:
                np.moveaxis(extra, s.extra_axis, 0)[lo:hi] = np.moveaxis(part.cpu().numpy(), s.extra_axis, 0)
        res = out[0] if s.n_values == 1 else tuple(out)
        return (res, extra) if return_params else res

    def pair_mask(self, lo_b, hi_b, max_pairs_per_launch):
        """The screen's values within the float32 bounds as a ``data.PairMask`` (``MPNNModel.screen_mask``)."""
        s, dev = self, self.model.device
        W = data.mask_row_words(s.A)
        words = torch.zeros((s.nT, s.C, W) if s.visc else (s.C, W), dtype=torch.int32, device=dev)
        for lo, hi, t0, t1, g, _ in s.tiles(max_pairs_per_launch, False):
            if g is not None:
                got = ops.grid_mask(g, lo_b, hi_b)
            else:
                tile = s.grid_tile(lo, hi, t0, t1, g).cpu().numpy()
                got = data.PairMask.from_bool((tile >= lo_b) & (tile <= hi_b), device=dev).words
            (words[t0:t1, lo:hi] if s.visc else words[lo:hi])[...] = got
        return data.PairMask(words, (s.C, s.A, s.nT) if s.visc else (s.C, s.A))

    def top_k(self, k, largest, max_pairs_per_launch):
        """The screen's k best pairs as a ``data.TopK`` (``MPNNModel.screen_top_k``): the selecting launches' results, or
        above SCREEN_MAX_K and without a covering kernel the materialised tiles', merged under the selection's order."""
        s = self
        A, select = s.A, s.covered and k <= SCREEN_MAX_K
        # the running best of every row: (values, flat index i * A + j as int64), at most k each
        best = [(np.empty(0, np.float32), np.empty(0, np.int64)) for _ in range(s.planes)]

        def offer(row, values, flat):
            v, f = np.concatenate([best[row][0], values]), np.concatenate([best[row][1], flat])
            order = data.top_k_order(v, f, k, largest)
            best[row] = (v[order], f[order])

        for lo, hi, t0, t1, g, wh in s.tiles(max_pairs_per_launch, select):
            if select:
                v, ci, ai = (x.cpu().numpy() for x in ops.grid_topk(g, k, largest, where=wh.words if wh is not None else None))
                for r in range(t1 - t0):
                    used = ci[r] >= 0
                    offer(t0 + r, v[r][used], (ci[r][used].astype(np.int64) + lo) * A + ai[r][used])
            else:
                tile = s.grid_tile(lo, hi, t0, t1, g).cpu().numpy().reshape((hi - lo) * A, -1)
                flat = np.arange(lo * A, hi * A, dtype=np.int64)
                if wh is not None:  # only the mask's pairs reach the order
                    keep = np.flatnonzero(wh.to_bool().reshape(-1))
                    tile, flat = tile[keep], flat[keep]
                for r in range(t1 - t0):
                    order = data.top_k_order(tile[:, r], flat, k, largest)
                    offer(t0 + r, tile[order, r], flat[order])
        m = min(k, s.C * A if s.where is None else s.where.count())
        values = np.empty((s.planes, m), np.float32)
        cation, anion = np.empty((s.planes, m), np.int64), np.empty((s.planes, m), np.int64)
        for r, (v, f) in enumerate(best):
            values[r], cation[r], anion[r] = v, f // max(A, 1), f % max(A, 1)
        values[np.isnan(values)] = data.QUIET_NAN
        if not s.visc:
            values, cation, anion = values[0], cation[0], anion[0]
        return data.TopK(values, cation, anion)

    def best_partners(self, m, largest, max_pairs_per_launch):
        """Every ion's m best partners as a ``data.BestPartners`` (``MPNNModel.screen_best_partners``): the selecting
        launches' results, or above ops.PARTNERS_MAX_M and without a covering kernel ``data.grid_best_partners`` of the
        materialised tiles; per-cation results side by side, per-anion results merged under the selection's order."""
        s = self
        select = s.covered and m <= ops.PARTNERS_MAX_M
        cat_v, cat_p = np.full((s.planes, s.C, m), data.QUIET_NAN, np.float32), np.full((s.planes, s.C, m), -1, np.int64)
        an_v, an_p = np.full((s.planes, s.A, m), data.QUIET_NAN, np.float32), np.full((s.planes, s.A, m), -1, np.int64)
        # a selecting launch's workspace: m entries of 8 bytes per plane for every tile row and tile column
        tc, ta = ops.PARTNERS_TILE[1 if s.mfma else 0]
        per_pair = 8 * m * min(s.planes, ops.SELECT_MAX_T) * (1.0 / tc + 1.0 / ta)
        for lo, hi, t0, t1, g, wh in s.tiles(max_pairs_per_launch, select, per_pair):
            if select:
                got = ops.grid_partners(g, m, largest, where=wh.words if wh is not None else None)
                cv, cp, av, ap = (x.cpu().numpy() for x in got)
                cp, ap = cp.astype(np.int64), ap.astype(np.int64)
            else:
                got = data.grid_best_partners(s.grid_tile(lo, hi, t0, t1, g).cpu().numpy(), m, largest, where=wh)
                (cv, cp), (av, ap) = ((x.reshape((t1 - t0, -1, m)) for x in side) for side in got)
            cat_v[t0:t1, lo:hi], cat_p[t0:t1, lo:hi] = cv, cp
            ap = np.where(ap >= 0, ap + lo, -1)      # the tile's cations are lo .. hi of the screen
            for r in range(t1 - t0):                 # an anion's best so far against this tile's, same order
                an_v[t0 + r], an_p[t0 + r] = data.best_of(np.concatenate([an_v[t0 + r], av[r]], axis=1),
                                                          np.concatenate([an_p[t0 + r], ap[r]], axis=1), m, largest)
        out = (cat_v, cat_p, an_v, an_p) if s.visc else (cat_v[0], cat_p[0], an_v[0], an_p[0])
        return data.BestPartners(data.Partners(*out[:2]), data.Partners(*out[2:]))

    def ion_summary(self, max_pairs_per_launch):
        """The screen's per-ion statistics as a ``data.IonSummary`` (``MPNNModel.screen_ion_summary``): the summary
        launches' records, or without a covering kernel those of the materialised tiles, over ranges of cations that end
        at multiples of SUMMARY_RANGE, the anion records carried from one range into the next."""
        s = self
        family = s.operands.family if s.operands is not None else (1 if s.model.kind == "transfer" else 0)
        blocks = ops.SUMMARY_BLOCKS[family]
        t_step = s.grid_max_t
        if max_pairs_per_launch is None and s.operands is None:
            max_pairs_per_launch = s.default_pairs(False)
        elif max_pairs_per_launch is None:  # a launch's workspace: one 32-byte record per plane, tile row and tile column
            max_pairs_per_launch = s.default_pairs(True, 32 * min(s.planes, t_step) * (1.0 / blocks[0] + 1.0 / blocks[1]))
        cations = list(cation_ranges(s.C, s.A, max_pairs_per_launch, multiple=SUMMARY_RANGE))
        parts = []  # per range of temperature rows: the records of all cations
        for t0, t1 in ranges(s.planes, t_step) if cations else ():
            cat, an = [], None
            for lo, hi in cations:
                wh = s.where.rows(lo, hi) if s.where is not None else None
                if s.operands is not None:
                    got = ops.grid_summary(s.operands.rows(lo, hi).temperatures(t0, t1),
                                           where=wh.words if wh is not None else None, carry=an)
                else:
                    tile = s.grid_tile(lo, hi, t0, t1, None).cpu().numpy()
                    got = data.grid_ion_records(tile, wh, blocks, carry=an)
                cat.append(got[:3])
                an = got[3:]
            host = lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else x
            parts.append([np.concatenate([host(c[f]) for c in cat], axis=1) for f in range(3)] + [host(x) for x in an])
        if parts:
            rec = [np.concatenate([p[f] for p in parts], axis=0) for f in range(6)]
        else:  # an empty grid: no pair competes
            rec = [x for n in (s.C, s.A) for x in (np.zeros((s.planes, n), np.uint32), np.zeros((s.planes, n, 2)),
                                                   np.full((s.planes, n, 2), data.QUIET_NAN, np.float32))]
        rec[0], rec[3] = rec[0].view(np.uint32), rec[3].view(np.uint32)  # (the device tensors are int32)
        return data.IonSummary.from_records(rec, planes=s.visc)

    def rank(self, k, largest, mask):
        """The rank cut of every plane and, with ``mask``, the best-k mask (``MPNNModel.screen_rank``,
        ``screen_best_mask``) -> (data.RankCut of arrays (planes,), int32 words (planes,C,W) on the model's device or
        None).  The cation axis is not tiled; without a covering kernel the host references run on ``values``."""
        s, dev = self, self.model.device
        C, A, planes = s.C, s.A, s.planes
        values, count = np.full(planes, data.QUIET_NAN, np.float32), np.zeros(planes, np.int64)
        cation, anion = np.full(planes, -1, np.int64), np.full(planes, -1, np.int64)
        words = torch.zeros((planes, C, data.mask_row_words(A)), dtype=torch.int32, device=dev) if mask else None
        if s.operands is not None:
            wh = s.where.words if s.where is not None else None
            for t0, t1 in ranges(planes, ops.SELECT_MAX_T):
                got = ops.grid_rank(s.operands.temperatures(t0, t1), k, largest, where=wh, mask=mask)
                values[t0:t1], cation[t0:t1], anion[t0:t1], count[t0:t1] = (x.cpu().numpy() for x in got[:4])
                if mask:
                    words[t0:t1] = got[4].reshape(t1 - t0, C, -1)
        elif C > 0 and A > 0:
            grid = s.values(None)
            values[:], cation[:], anion[:], count[:] = data.grid_rank(grid, k, largest, s.where)
            if mask:
                best = data.grid_best_mask(grid, k, largest, s.where)
                words = data.PairMask.from_bool(best, device=dev).words.reshape(planes, C, -1)
        return data.RankCut(values, cation, anion, count), words


# ---------------------------------------------------------------------- the applicability domain of a screen
def _domain_request(model, what, reference=None):
    """The refusals the domain methods share: the transfer model, widths the head kernels do not cover, and a
    reference set of another width."""
    if model.kind == "transfer":
        raise ValueError(f"{what}: the transfer model's head does not end the latent space at mix_cat_an; use the "
                         "base viscosity model it was built from")
    if not model._grid_kernels_cover():
        raise ValueError(f"{what}: the head kernels do not cover atom_dim {model.atom_dim}, fp_size {model.fp_size}, "
                         f"mixing_size {model.mixing_size} (<= {ops.HEAD_MAX_X}, {ops.HEAD_MAX_DIM}, {ops.HEAD_MAX_DIM})")
    if reference is not None:
        if not isinstance(reference, data.DomainReference):
            raise TypeError(f"reference must be a data.DomainReference, got {type(reference).__name__}")
        if reference.width != model.mixing_size:
            raise ValueError(f"{what}: the reference set has width {reference.width}, the model's mixing_size is "
                             f"{model.mixing_size}")


def _domain_mix(model, cations, anions, batch_size):
    """The per-ion halves of the latent space: ``encode_ions`` and ``ops.head_ion_mix`` -> (C,Mx), (A,Mx)."""
    if cations is None or anions is None:
        raise ValueError("the domain methods need both cations and anions")
    pc, pa = model.encode_ions(cations, anions, batch_size)
    w, fp, mx = model._packed_head(), model.fp_size, model.mixing_size
    return ops.head_ion_mix(model.kind, "cat", pc, w, fp, mx), ops.head_ion_mix(model.kind, "an", pa, w, fp, mx)


def domain_grid(model, cations, anions, reference, max_pairs_per_launch, batch_size):
    """``MPNNModel.domain_grid``: the two outputs of a pair count against GRID_OUTPUT_BUDGET."""
    _domain_request(model, "domain_grid", reference)
    mc, ma = _domain_mix(model, cations, anions, batch_size)
    C, A = int(mc.shape[0]), int(ma.shape[0])
    distance, nearest = np.empty((C, A), np.float32), np.empty((C, A), np.int32)
    pairs = GRID_OUTPUT_BUDGET // 2 if max_pairs_per_launch is None else at_least_one("max_pairs_per_launch", max_pairs_per_launch)
    for lo, hi in cation_ranges(C, A, pairs):
        d, n = ops.domain_grid(mc[lo:hi], ma, reference.rows)
        distance[lo:hi], nearest[lo:hi] = d.cpu().numpy(), n.cpu().numpy()
    return distance, nearest


def domain_mask(model, cations, anions, reference, lo_b, hi_b, max_pairs_per_launch, batch_size):
    """``MPNNModel.screen_domain_mask`` after its bounds: a launch holds fewer than 2^31 tiles of 16 x 64 pairs."""
    _domain_request(model, "screen_domain_mask", reference)
    mc, ma = _domain_mix(model, cations, anions, batch_size)
    C, A = int(mc.shape[0]), int(ma.shape[0])
    words = torch.zeros((C, data.mask_row_words(A)), dtype=torch.int32, device=model.device)
    pairs = 1 << 40 if max_pairs_per_launch is None else at_least_one("max_pairs_per_launch", max_pairs_per_launch)
    for lo, hi in cation_ranges(C, A, pairs):
        words[lo:hi] = ops.domain_grid_mask(mc[lo:hi], ma, reference.rows, lo_b, hi_b)
    return data.PairMask(words, (C, A))


def diverse(model, cations, anions, reference, k, where, batch_size):
    """``MPNNModel.screen_diverse``: one ``ops.domain_diverse`` call over the whole grid."""
    k = at_least_one("k", k)
    _domain_request(model, "screen_diverse", reference)
    if where is not None and not isinstance(where, data.PairMask):
        raise TypeError(f"where must be a data.PairMask, got {type(where).__name__}")
    mc, ma = _domain_mix(model, cations, anions, batch_size)
    C, A = int(mc.shape[0]), int(ma.shape[0])
    if where is not None and where.shape != (C, A):
        raise ValueError(f"where must be a PairMask of shape {(C, A)}, got {where.shape}")
    words = None if where is None else where.words.to(model.device)
    cation, anion, distance, counts = ops.domain_diverse(mc, ma, reference.rows, k, where=words)
    n, competing = (int(v) for v in counts.cpu().numpy())
    return data.DiverseSelection(cation[:n].cpu().numpy().astype(np.int64), anion[:n].cpu().numpy().astype(np.int64),
                                 distance[:n].cpu().numpy(), competing)
