"""The Pareto front of two objectives over the cation x anion grid: the pairs that no other pair beats on both
properties at once - the threshold-free way to screen by two properties.

Each objective is a model's prediction (or an ensemble's score) over the grid; both grids are evaluated tile by tile on
the device, a filter (impnn_pareto_*, csrc/grid_pareto.hip) leaves a short candidate list that holds the whole front,
and only the candidates reach the host, where the exact front is finished (``data.pareto_front`` is the definition)."""
from __future__ import annotations

import copy

import numpy as np
import torch

from . import data, ops
from .ensemble import ModelEnsemble, _EnsembleScreen
from .model import MPNNModel
from .screening import GRID_OUTPUT_BUDGET, _Screen, _screen_request, cation_ranges, score_kappa

MAX_BLOCK_PAIRS = (1 << 31) - 1   # pairs of one row-block of the filter (include/impnn.h)


class Objective:
    """One axis of a Pareto screen: ``model``, an ``MPNNModel`` of any kind or a ``ModelEnsemble``; ``temperature``:
    the one temperature in kelvin of a viscosity objective (the other kinds take none); ``largest``: the objective is
    maximised; ``kappa``: an ensemble's value is its score mean + kappa * std (default 0; a single model takes none)."""

    def __init__(self, model, temperature=None, largest=False, kappa=None):
        if not isinstance(model, (MPNNModel, ModelEnsemble)):
            raise TypeError(f"an objective's model is an MPNNModel or a ModelEnsemble, got {type(model).__name__}")
        self.model, self.largest = model, bool(largest)
        self.ensemble = isinstance(model, ModelEnsemble)
        if model.kind == "viscosity":
            T = None if temperature is None else np.asarray(temperature, dtype=np.float32).reshape(-1)
            if T is None or T.size != 1:
                raise ValueError("a viscosity objective needs exactly one temperature in kelvin")
            self.temperature = float(T[0])
        elif temperature is not None:
            raise ValueError(f"a {model.kind} objective takes no temperature")
        else:
            self.temperature = None
        if kappa is not None and not self.ensemble:
            raise ValueError("kappa applies to a ModelEnsemble objective only")
        self.kappa = score_kappa(0.0 if kappa is None else kappa)

    def _request(self, cations, anions, where, max_pairs_per_launch):
        T = None if self.temperature is None else [self.temperature]
        return _screen_request(self.model.kind, "screen_pareto", cations, anions, T, where, max_pairs_per_launch)

    def _screen(self, cations, anions, T, where, batch_size):
        if self.ensemble:
            return _EnsembleScreen(self.model, cations, anions, T, where, batch_size, self.kappa)
        return _Screen(self.model, cations, anions, T, where, batch_size)

    def _screen_like(self, other, T):
        """The screen of ``other``, an objective over the same model, with this objective's temperature and kappa:
        the encoder rows are shared."""
        s = copy.copy(other)
        if self.ensemble:
            s.kappa = self.kappa
        if s.T is not None:
            s.T = T.to(s.T.device)
        if s.operands is not None:
            s.operands = s._operands()
        return s


def _plane(screen, lo, hi):
    """Rows lo .. hi of a screen's grid as one contiguous float32 (hi - lo, A) device plane."""
    g = screen.operands.rows(lo, hi) if screen.operands is not None else None
    tile = screen.grid_tile(lo, hi, 0, 1, g)
    return tile.reshape(hi - lo, screen.A).to(torch.float32).contiguous()


def screen_pareto(objectives, cations, anions, where=None, max_pairs_per_launch=None, batch_size=4096, capacity=None):
    """The Pareto front of two objectives over every cation x anion pair -> ``data.ParetoFront`` of numpy arrays:
    ``values`` (n,2) float32, the raw predictions or scores in objective order with the bits ``predict_grid`` gives,
    ``cation`` and ``anion`` (n,) int64 (positions in the lists given) and ``competing``.  What
    ``data.pareto_front(grid_1, grid_2, (o1.largest, o2.largest), where)`` returns for the two materialised grids: the
    pairs that compete (``where``, neither value NaN) and that no competing pair dominates, by ascending first key.

        front = screen_pareto([Objective(visc_model, 298.15), Objective(mp_model)], cat, an)

    ``objectives``: exactly two ``Objective``s on one device.  ``where``: a 2-D ``data.PairMask`` as in
    ``screen_top_k``.  The encoders run once per model; the cation axis is cut into ranges (``max_pairs_per_launch``
    pairs at the most), each screen's tile of a range is evaluated on the device (the gathered fallback included) and
    the filter's stages stream over them: kept on the device between the stages if both whole planes fit
    GRID_OUTPUT_BUDGET elements, evaluated again per stage otherwise.  No tile is copied to the host.  ``capacity``:
    entries of the first candidate arrays; the collect stage is repeated with larger ones if more survive."""
    objectives = list(objectives)
    if len(objectives) != 2:
        raise ValueError(f"screen_pareto takes exactly two objectives, got {len(objectives)}: fronts of more objectives "
                         "are not built")
    for o in objectives:
        if not isinstance(o, Objective):
            raise TypeError(f"objectives are Objective instances, got {type(o).__name__}")
    o1, o2 = objectives
    if o1.model.device != o2.model.device:
        raise ValueError(f"both objectives must be on one device, got {o1.model.device} and {o2.model.device}")
    if capacity is not None and int(capacity) < 1:
        raise ValueError("capacity must be >= 1")
    T1, T2 = (o._request(cations, anions, where, max_pairs_per_launch) for o in objectives)
    s1 = o1._screen(cations, anions, T1, where, batch_size)
    s2 = o2._screen_like(s1, T2) if o2.model is o1.model else o2._screen(cations, anions, T2, where, batch_size)
    C, A = s1.C, s1.A
    if C == 0 or A == 0:
        return data.ParetoFront(np.empty((0, 2), np.float32), np.empty(0, np.int64), np.empty(0, np.int64), 0)
    pairs = min(s1.default_pairs(False), s2.default_pairs(False)) if max_pairs_per_launch is None else max_pairs_per_launch
    ranges = list(cation_ranges(C, A, pairs, MAX_BLOCK_PAIRS))

    def evaluate():
        for lo, hi in ranges:
            wh = s1.where.rows(lo, hi).words if s1.where is not None else None
            yield _plane(s1, lo, hi), _plane(s2, lo, hi), wh, lo

    blocks = evaluate
    if 2 * C * A <= GRID_OUTPUT_BUDGET:
        kept = list(evaluate())
        blocks = lambda: kept
    filt = ops.ParetoFilter(A, (o1.largest, o2.largest), ops.PARETO_DEFAULT_CAPACITY if capacity is None else capacity,
                            o1.model.device)
    return ops.pareto_run(filt, blocks)
