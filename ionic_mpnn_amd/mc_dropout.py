"""Monte-Carlo dropout of the transfer model over the cation x anion grid: mean, spread and a confidence-bound score per
pair from ONE trained model, and the screens of ``MPNNModel`` on that score, evaluated inside one grid tile
(impnn_transfer_mc_grid*, csrc/transfer_mc_grid.hip).

The transfer head has a Dropout between its 128- and 64-wide layers (``mp_dropout``).  S stochastic passes with that
dropout on and BatchNormalization on its moving statistics give S predictions per pair; their mean and population
standard deviation are the model's own estimate of where it is unsure, and ``mean + kappa * std`` ranks a screen as
``ModelEnsemble`` does.  The S masks are drawn once per (``samples``, ``draw``) and are the same for every pair of the
grid - the "fixed set of masks" form of MC dropout - so a pair's statistic is a deterministic function of its two ions,
the weights and the table: it does not depend on the tile, the launch, the host tiling or the grid's size, a screen's
ranking is reproducible, and ``predict_pairs`` returns the grid's bits.

Not built for this form: each ion's best partners, the rank cut, Pareto objectives (per-ion statistics are:
``screen_ion_summary``); dropout inside the encoder's
GatedUpdates stays off (the samples share one encoding of every ion)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, layers as L, ops
from .model import MPNNModel
from .screening import _Screen, _screen_request, at_least_one, mask_bounds, score_kappa


class _McScreen(_Screen):
    """``_Screen`` over the MC form: the operands are the transfer grid's with the multiplier table and ``kappa`` (always
    the matrix-core grid: ``McDropout`` refuses a model it does not cover), and a materialised tile is the score;
    ``values`` assembles the three planes (mean, std, score) and, for its extra output, the sample planes (S,C,A)."""

    n_values, extra_axis = 3, 1

    def __init__(self, mc, cations, anions, where, batch_size, kappa):
        self.mc, self.kappa = mc, kappa
        super().__init__(mc.model, cations, anions, None, where, batch_size)

    def _coverage(self):
        return True, True

    def _operands(self):
        g = self.model._grid_operands(self.pc, self.pa, None, True)
        return ops.transfer_mc_grid_operands(g.cat, g.an, g.w, self.mc.multipliers(), self.kappa)

    def tile_values(self, lo, hi, t0, t1, operands, extra):
        got = ops.transfer_mc_grid(operands, extra)
        return got[:3], got[3] if extra else None

    def extra_out(self):
        return np.empty((self.mc.samples, self.C, self.A), np.float32)


class McDropout:
    """``samples`` stochastic passes of a transfer model's head as one screening model (``MPNNModel.mc_dropout``).
    Sample s thins relu(mp_dense_2) with row s of the mask ``mp_dropout`` applies in a training pass at dropout step
    ``draw`` (``ops.dropout_mask`` with the layer's rate and seed): another ``draw`` is another set of S masks, the same
    ``draw`` the same bits.  The table is rebuilt when ``samples``, ``draw`` or the layer's rate / seed change; the
    weight image follows the weights as it does for ``MPNNModel.predict_grid``."""

    def __init__(self, model, samples=32, draw=0):
        if not isinstance(model, MPNNModel) or model.kind != "transfer":
            kind = model.kind if isinstance(model, MPNNModel) else type(model).__name__
            raise ValueError(f"mc_dropout: a {kind} model has no head Dropout to sample; only the transfer model's head "
                             "(mp_dropout between its 128- and 64-wide layers) has one")
        if not model._transfer_grid_covers():
            raise ValueError(f"mc_dropout: the transfer grid kernels do not cover atom_dim {model.atom_dim}, fp_size "
                             f"{model.fp_size}, mixing_size {model.mixing_size} (<= {ops.HEAD_MAX_X}, {ops.HEAD_MAX_DIM}, "
                             f"{ops.HEAD_MAX_DIM})")
        most = int(_lib.load().impnn_transfer_mc_grid_max_samples())
        if isinstance(samples, bool) or int(samples) != samples or not 1 <= int(samples) <= most:
            raise ValueError(f"mc_dropout: samples must be an integer from 1 to {most}, got {samples!r}")
        if isinstance(draw, bool) or int(draw) != draw or not 0 <= int(draw) < 1 << 63:
            raise ValueError(f"mc_dropout: draw must be a non-negative integer, got {draw!r}")
        self.model, self.samples, self.draw = model, int(samples), int(draw)
        self.device = model.device
        self._table, self._table_key = None, None

    def __len__(self):
        return self.samples

    def multipliers(self):
        """The (samples, 128) float32 table on the model's device: row s is ``ops.dropout_mask``'s row s for
        ``mp_dropout``'s rate and seed, the head's layer word and the dropout step ``draw``."""
        dp = self.model.mp_dropout
        key = (self.samples, self.draw, dp.rate, dp.seed)
        if self._table is None or self._table_key != key:
            step = torch.tensor([self.draw], dtype=torch.int64, device=self.device)
            drop = ops.Dropout(dp.rate, dp.seed or 0, ops.dropout_layer_word(L.Dropout.LAYER_ID, 0), step)
            self._table, self._table_key = ops.dropout_mask(drop, rows=self.samples, D=ops.TRANSFER_MC_WIDTH), key
        return self._table

    def _request(self, what, cations, anions, where, max_pairs_per_launch, kappa):
        kappa = score_kappa(kappa)
        _screen_request(self.model.kind, what, cations, anions, None, where, max_pairs_per_launch)
        return kappa

    def predict_grid(self, cations, anions, kappa=None, return_samples=False, max_pairs_per_launch=None, batch_size=4096):
        """Mean and population standard deviation of the S samples over every cation x anion pair, from one
        impnn_transfer_mc_grid launch per host tile -> numpy (mean, std), each (C,A); with ``kappa`` also score = mean +
        kappa * std; with ``return_samples`` the sample planes (S,C,A) last.  The statistic is float32 in a fixed order
        (``data.ensemble_grid_stats`` of the samples), and a pair's bits do not depend on the host tiling or the grid's
        size.  With dropout rate 0 every sample has the bits of ``MPNNModel.predict_grid``.  Arguments as
        ``MPNNModel.predict_grid``."""
        kp = self._request("predict_grid", cations, anions, None, max_pairs_per_launch, 0.0 if kappa is None else kappa)
        res = _McScreen(self, cations, anions, None, batch_size, kp).values(max_pairs_per_launch, return_samples)
        out, planes = res if return_samples else (res, None)
        out = out if kappa is not None else out[:2]
        return (*out, planes) if return_samples else out

    def screen_mask(self, cations, anions, at_least=None, at_most=None, kappa=0.0, max_pairs_per_launch=None,
                    batch_size=4096):
        """``at_least <= score <= at_most`` as a ``data.PairMask``, written on the GPU (impnn_transfer_mc_grid_mask),
        for the score ``predict_grid(..., kappa=kappa)`` gives.  Arguments as ``MPNNModel.screen_mask``."""
        lo_b, hi_b = mask_bounds("screen_mask", at_least, at_most)
        kp = self._request("screen_mask", cations, anions, None, max_pairs_per_launch, kappa)
        return _McScreen(self, cations, anions, None, batch_size, kp).pair_mask(lo_b, hi_b, max_pairs_per_launch)

    def screen_top_k(self, cations, anions, k=100, kappa=0.0, largest=False, where=None, max_pairs_per_launch=None,
                     batch_size=4096):
        """The k pairs with the smallest (``largest``: largest) score, selected on the GPU (impnn_transfer_mc_grid_topk,
        with ``where`` _topk_where): what ``data.grid_top_k(score, k, largest, where)`` returns for the score of
        ``predict_grid(..., kappa=kappa)``, without the grid -> ``data.TopK`` whose ``values`` are scores.  Arguments,
        tiling and the merge as ``MPNNModel.screen_top_k``; read the mean and spread of the selected pairs with
        ``predict_pairs``."""
        kp = self._request("screen_top_k", cations, anions, where, max_pairs_per_launch, kappa)
        k = at_least_one("k", k)
        return _McScreen(self, cations, anions, where, batch_size, kp).top_k(k, largest, max_pairs_per_launch)

    def screen_ion_summary(self, cations, anions, where=None, kappa=0.0, max_pairs_per_launch=None, batch_size=4096):
        """Per-ion statistics of the score, reduced on the GPU (impnn_transfer_mc_grid_summary): what
        ``data.grid_ion_summary(score, where, ops.SUMMARY_BLOCKS[3])`` returns for the score of ``predict_grid(...,
        kappa=kappa)``, bit for bit, without the grid -> ``data.IonSummary``.  Arguments, tiling and the carried anion
        records as ``MPNNModel.screen_ion_summary``."""
        kp = self._request("screen_ion_summary", cations, anions, where, max_pairs_per_launch, kappa)
        return _McScreen(self, cations, anions, where, batch_size, kp).ion_summary(max_pairs_per_launch)

    def predict_pairs(self, cations, anions, cation_index, anion_index, batch_size=4096):
        """Mean and population standard deviation of listed pairs - pair p is (cations[cation_index[p]],
        anions[anion_index[p]]) -> numpy (mean, std) of shape (P,), with the bits ``predict_grid`` gives those pairs:
        one 1 x n grid launch per distinct cation of the list.  Host plumbing for reading the mean and spread behind
        the scores of ``screen_top_k``, not a hot path."""
        self._request("predict_pairs", cations, anions, None, None, 0.0)
        ci = np.asarray(cation_index, dtype=np.int64).reshape(-1)
        ai = np.asarray(anion_index, dtype=np.int64).reshape(-1)
        if ci.shape != ai.shape:
            raise ValueError(f"cation_index and anion_index differ in length: {ci.size} and {ai.size}")
        s = _McScreen(self, cations, anions, None, batch_size, 0.0)
        if ci.size and (ci.min() < 0 or ci.max() >= s.C or ai.min() < 0 or ai.max() >= s.A):
            raise IndexError(f"a pair index is outside the {s.C} cations x {s.A} anions given")
        mean, std = np.empty(ci.size, np.float32), np.empty(ci.size, np.float32)
        g = s.operands
        for c in np.unique(ci):
            at = np.flatnonzero(ci == c)
            an = g.an[torch.as_tensor(ai[at], device=self.device)]
            one = ops.GridOperands(3, 1, g.cat[int(c):int(c) + 1], an, None, g.w, (), 0.0, g.multipliers)
            m, sd, _ = ops.transfer_mc_grid(one)
            mean[at], std[at] = m.cpu().numpy()[0], sd.cpu().numpy()[0]
        return mean, std
