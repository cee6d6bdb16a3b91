"""A deep ensemble of MPNNModels over the cation x anion grid: mean, spread and a confidence-bound score per pair, and
the screens of ``MPNNModel`` on that score, evaluated inside one grid tile (impnn_ensemble_grid*, csrc/ensemble_grid.hip).

Point predictions of one model rank a screen by wherever that model happens to extrapolate low.  Train M copies from
different seeds or folds (``build_model(..., dropout_seed=...)`` / ``weights.init_weights(seed=...)``, ``fit``), then
rank by ``mean + kappa * std``: kappa > 0 prefers pairs the members agree on when the smallest values are sought."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, data, ops
from .model import MPNNModel
from .screening import _Screen, _screen_request, at_least_one, mask_bounds, score_kappa

ENSEMBLE_KINDS = ("viscosity", "melting_point")


class _EnsembleScreen(_Screen):
    """``_Screen`` over an ensemble: ``pc`` / ``pa`` are the members' pooled rows (lists), the operands are the ensemble
    grid's (always covered: ``ModelEnsemble`` refuses members the grid kernels do not cover), a launch takes the
    temperatures the library reports for this many members, and a materialised tile is the score; ``values`` assembles
    the three planes (mean, std, score)."""

    n_values = 3

    def __init__(self, ensemble, cations, anions, T, where, batch_size, kappa):
        lib, M = _lib.load(), len(ensemble.models)
        self.kappa = kappa
        self.select_max_t = int(lib.impnn_ensemble_grid_topk_max_temperatures(M))
        self.grid_max_t = max(int(lib.impnn_ensemble_grid_max_temperatures(ops.HEAD_KINDS[ensemble.kind], M)), 1)
        super().__init__(ensemble, cations, anions, T, where, batch_size)

    def _counts(self):
        return int(self.pc[0].shape[0]), int(self.pa[0].shape[0])

    def _coverage(self):
        return False, True

    def _operands(self):
        return self.model._grid_operands(self.pc, self.pa, self.T, self.kappa)

    def tile_values(self, lo, hi, t0, t1, operands, extra):
        return ops.grid_values(operands), None


class ModelEnsemble:
    """1 to 8 built ``MPNNModel``s of one kind ("viscosity" or "melting_point") as one screening model.  The members
    share ``fp_size``, ``mixing_size`` and the device and have head widths the grid kernels cover; ``atom_dim``,
    ``bond_dim`` and ``num_steps`` may differ, since only a member's mixing rows reach the grid.  Anything else is a
    ValueError that names the offending member."""

    def __init__(self, models):
        models = list(models)
        most = int(_lib.load().impnn_ensemble_grid_max_members())
        if not 1 <= len(models) <= most:
            raise ValueError(f"an ensemble takes 1 to {most} models, got {len(models)}")
        for i, m in enumerate(models):
            if not isinstance(m, MPNNModel):
                raise ValueError(f"member {i} is not an MPNNModel: {type(m).__name__}")
            if m.kind not in ENSEMBLE_KINDS:
                raise ValueError(f"member {i} is a {m.kind} model: an ensemble takes viscosity or melting_point models")
            first = models[0]
            if m.kind != first.kind:
                raise ValueError(f"member {i} is a {m.kind} model, member 0 a {first.kind} model")
            if (m.fp_size, m.mixing_size) != (first.fp_size, first.mixing_size):
                raise ValueError(f"member {i} has fp_size {m.fp_size} and mixing_size {m.mixing_size}, member 0 "
                                 f"{first.fp_size} and {first.mixing_size}")
            if m.device != first.device:
                raise ValueError(f"member {i} is on {m.device}, member 0 on {first.device}")
            if not m._grid_kernels_cover():
                raise ValueError(f"member {i}: the grid kernels do not cover atom_dim {m.atom_dim}, fp_size {m.fp_size}, "
                                 f"mixing_size {m.mixing_size} (<= {ops.HEAD_MAX_X}, {ops.HEAD_MAX_DIM}, {ops.HEAD_MAX_DIM})")
        self.models = tuple(models)
        self.kind, self.device = models[0].kind, models[0].device
        self.fp_size, self.mixing_size = models[0].fp_size, models[0].mixing_size

    def __len__(self):
        return len(self.models)

    def encode_ions(self, cations=None, anions=None, batch_size=4096):
        """Every member's ``encode_ions`` -> (list of pooled_cat, list of pooled_an)."""
        rows = [m.encode_ions(cations, anions, batch_size) for m in self.models]
        return [r[0] for r in rows], [r[1] for r in rows]

    def _grid_operands(self, pc, pa, T, kappa):
        """Each member's ``ops.head_ion_mix`` rows and the tail of its packed head as the ensemble grid's operands."""
        fp, mx, k = self.fp_size, self.mixing_size, ops.HEAD_KINDS[self.kind]
        n = int(_lib.load().impnn_ensemble_grid_tail_floats(k, fp, mx))
        cat, an, tails = [], [], []
        for m, c, a in zip(self.models, pc, pa):
            w = m._packed_head()
            cat.append(ops.head_ion_mix(self.kind, "cat", c, w, fp, mx))
            an.append(ops.head_ion_mix(self.kind, "an", a, w, fp, mx))
            tails.append(w[-n:])
        return ops.ensemble_grid_operands(self.kind, torch.stack(cat), torch.stack(an), T, torch.stack(tails), fp, mx, kappa)

    def _request(self, what, cations, anions, temperatures, where, max_pairs_per_launch, kappa):
        kappa = score_kappa(kappa)
        return _screen_request(self.kind, what, cations, anions, temperatures, where, max_pairs_per_launch), kappa

    def predict_grid(self, cations, anions, temperatures=None, kappa=None, max_pairs_per_launch=None, batch_size=4096):
        """Mean and population standard deviation of the members' ``predict_grid`` over every cation x anion pair (x
        temperature), from one impnn_ensemble_grid launch per host tile -> numpy (mean, std), with ``kappa`` also score
        = mean + kappa * std; (C,A,nT) for viscosity, (C,A) for melting point.  A member's value has the bits its own
        ``predict_grid`` gives; the statistic is float32 in a fixed order (``data.ensemble_grid_stats``), so an element's
        bits do not depend on the host tiling.  Arguments as ``MPNNModel.predict_grid``."""
        T, kp = self._request("predict_grid", cations, anions, temperatures, None, max_pairs_per_launch,
                              0.0 if kappa is None else kappa)
        out = _EnsembleScreen(self, cations, anions, T, None, batch_size, kp).values(max_pairs_per_launch)
        return out if kappa is not None else out[:2]

    def screen_mask(self, cations, anions, temperatures=None, at_least=None, at_most=None, kappa=0.0,
                    max_pairs_per_launch=None, batch_size=4096):
        """``at_least <= score <= at_most`` as a ``data.PairMask``, written on the GPU (impnn_ensemble_grid_mask), for
        the score ``predict_grid(..., kappa=kappa)`` gives.  Arguments as ``MPNNModel.screen_mask``."""
        lo_b, hi_b = mask_bounds("screen_mask", at_least, at_most)
        T, kp = self._request("screen_mask", cations, anions, temperatures, None, max_pairs_per_launch, kappa)
        return _EnsembleScreen(self, cations, anions, T, None, batch_size, kp).pair_mask(lo_b, hi_b, max_pairs_per_launch)

    def screen_top_k(self, cations, anions, temperatures=None, k=100, kappa=0.0, largest=False, where=None,
                     max_pairs_per_launch=None, batch_size=4096):
        """The k pairs with the smallest (``largest``: largest) score, selected on the GPU (impnn_ensemble_grid_topk,
        with ``where`` _topk_where): what ``data.grid_top_k(score, k, largest, where)`` returns for the score of
        ``predict_grid(..., kappa=kappa)``, without the grid -> ``data.TopK`` whose ``values`` are scores, in the order
        (value, cation, anion, NaN last).  Arguments, tiling and the merge as ``MPNNModel.screen_top_k``; read the mean
        and spread of the selected pairs with ``predict_pairs``."""
        T, kp = self._request("screen_top_k", cations, anions, temperatures, where, max_pairs_per_launch, kappa)
        k = at_least_one("k", k)
        return _EnsembleScreen(self, cations, anions, T, where, batch_size, kp).top_k(k, largest, max_pairs_per_launch)

    def screen_ion_summary(self, cations, anions, temperatures=None, where=None, kappa=0.0, max_pairs_per_launch=None,
                           batch_size=4096):
        """Per-ion statistics of the score, reduced on the GPU (impnn_deep_ensemble_grid_summary): what
        ``data.grid_ion_summary(score, where)`` returns for the score of ``predict_grid(..., kappa=kappa)``, bit for
        bit, without the grid -> ``data.IonSummary``.  Arguments, tiling and the carried anion records as
        ``MPNNModel.screen_ion_summary``."""
        T, kp = self._request("screen_ion_summary", cations, anions, temperatures, where, max_pairs_per_launch, kappa)
        return _EnsembleScreen(self, cations, anions, T, where, batch_size, kp).ion_summary(max_pairs_per_launch)

    def _no_domain(self, *args, **kwargs):
        """The applicability domain is a distance in one model's latent space; the members' spaces differ."""
        raise ValueError("an ensemble has no latent space of its own: fit and screen the applicability domain with one "
                         "member model (its masks constrain the ensemble's screens through where=)")

    fit_domain = domain_grid = screen_domain_mask = domain_distance = screen_diverse = _no_domain

    def predict_pairs(self, cations, anions, cation_index, anion_index, temperatures=None, batch_size=4096):
        """Mean and population standard deviation of listed pairs - pair p is (cations[cation_index[p]],
        anions[anion_index[p]]) - from the members' own ``head`` on gathered pooled rows -> numpy (mean, std) of shape
        (P,nT) for viscosity, (P,) for melting point.  How a caller reads the mean and spread behind the scores of
        ``screen_top_k``.  Not bitwise with the grid (another kernel evaluates the head): within 1e-5 of it."""
        T = _screen_request(self.kind, "predict_pairs", cations, anions, temperatures, None, None)
        ci = torch.as_tensor(np.asarray(cation_index, dtype=np.int64).reshape(-1), device=self.device)
        ai = torch.as_tensor(np.asarray(anion_index, dtype=np.int64).reshape(-1), device=self.device)
        P, nT = int(ci.numel()), int(T.numel()) if T is not None else 0
        values = []
        with torch.no_grad():
            for m in self.models:
                pc, pa = m.encode_ions(cations, anions, batch_size)
                pc, pa = pc[ci], pa[ai]
                if T is None:
                    values.append(m.head(pc, pa).reshape(P).cpu().numpy())
                else:
                    cols = [m.head(pc, pa, torch.full((P, 1), float(t), dtype=torch.float32, device=self.device)) for t in T]
                    values.append(torch.cat(cols, dim=1).reshape(P, nT).cpu().numpy())
        mean, std, _ = data.ensemble_grid_stats(np.stack(values), 0.0)
        return mean, std
