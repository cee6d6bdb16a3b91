"""build_model() of the reference's trainers, wired from ionic_mpnn_amd.layers.

``build_model`` (viscosity, train_viscosity.py:139-231) and ``build_melting_point_model``
(train_melting_point.py:137-215) keep the reference's signatures/defaults and create the layers in
the reference's order, so Keras-style auto names (gated_update_2, dense_3, ...) line up.

Two execution schedules, both on the HIP library:
  * ``fused=True`` (default when the shape is covered): one impnn_encoder_fused launch computes
    both ions' encode() up to GlobalSumPool;
  * ``fused=False``: layer at a time through the drop-in layers (a1..a8), tensor boundaries
    identical to the reference's; the two ions' chains run on two HIP streams (batches up to 4096).
Everything after GlobalSumPool is one launch (impnn_model_head); training goes through the larger
autograd nodes of ionic_mpnn_amd.autograd (f4), the torch-op head remains for traces and widths the kernels do not cover.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import data
from . import layers as L
from . import ops
from . import screening
from .screening import ION_KEYS, SCREEN_MAX_K, _Screen, _ion_numpy, ion_pair_batches  # noqa: F401  (names users of this module take from it)

INPUT_NAMES = ["cat_atom", "cat_bond", "cat_connectivity", "an_atom", "an_bond", "an_connectivity", "temperature"]


# largest batch whose two ion chains run on two HIP streams in the layer-at-a-time path (MPNNModel._encode_two_streams).
# Measured on MI355X (training step, D=32): faster at every batch size, 0.47 -> 0.37 ms at 32 and 2.19 -> 1.88 ms at
# 4096; layered inference 7.7 -> 8.5 M pairs/s at 4096 and D=128 forward 9.8 -> 9.4 ms, but 1.12 -> 1.18 ms at batch
# 8192 (config 3), where every kernel already fills the chip.  IMPNN_TWO_STREAM_MAX_BATCH=0 switches it off.
TWO_STREAM_MAX_BATCH = 4096
TRAIN_ROW_LIST_MIN_ROWS = int(os.environ.get("IMPNN_TRAIN_ROW_LIST_MIN_ROWS", 4096))


class MPNNModel:
    def __init__(self, kind, atom_vocab_size, bond_vocab_size, atom_dim, bond_dim, fp_size, mixing_size,
                 num_steps, fp_l2, device=None, name=None, dropout_rate=0.0, dropout_seed=None,
                 head_dropout_rate=0.3, head_dropout_seed=None):
        """dropout_rate / dropout_seed: GatedUpdate's Dropout in every message-passing step of both ions, applied by
        training passes only (fit, train_on_batch, __call__(training=True)); the seed defaults to one draw from
        torch's CPU generator.  head_dropout_rate / head_dropout_seed (kind "transfer" only): the head's Dropout."""
        if kind not in ("viscosity", "melting_point", "transfer"):
            raise ValueError(f"unknown model kind {kind!r}")
        self.kind = kind
        self.name = name or {"melting_point": "MeltingPoint_MPNN", "transfer": "MeltingPoint_Transfer"}.get(kind, "model")
        self.atom_vocab_size, self.bond_vocab_size = int(atom_vocab_size), int(bond_vocab_size)
        self.atom_dim, self.bond_dim = int(atom_dim), int(bond_dim)
        self.fp_size, self.mixing_size, self.num_steps = int(fp_size), int(mixing_size), int(num_steps)
        self.fp_l2 = float(fp_l2)
        self.dropout_rate = ops.check_dropout_rate(dropout_rate)
        if dropout_seed is None and self.dropout_rate > 0.0:
            dropout_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self.dropout_seed = None if dropout_seed is None else int(dropout_seed)
        self._dropout_counter = None
        self.device = device or L.default_device()
        dev = dict(device=self.device)
        D, K, S = self.atom_dim, self.bond_dim, self.num_steps
        # shared embeddings (train_viscosity.py:163-164)
        self.atom_emb = L.Embedding(atom_vocab_size, D, mask_zero=False, **dev)
        self.bond_emb = L.Embedding(bond_vocab_size, K, mask_zero=False, lazy=True, **dev)
        self.branches = {}
        for p in ("cat", "an"):  # encode(), train_viscosity.py:166-190, called at :193-194
            br = {"bmm": [], "reduce": [], "update": []}
            for i in range(S):
                br["bmm"].append(L.BondMatrixMessage(D, K, name=f"{p}_bmm_{i}", **dev))
                br["reduce"].append(L.Reduce(name=f"{p}_reduce_{i}", **dev))
                br["update"].append(L.GatedUpdate(D, dropout_rate=self.dropout_rate, dropout_seed=self.dropout_seed, **dev))
            br["pool"] = L.GlobalSumPool(**dev)
            br["fp"] = L.Dense(fp_size, activation="relu", kernel_regularizer=("l2", fp_l2), **dev)
            self.branches[p] = br
        self.cat_proj = L.Dense(mixing_size, activation="relu", **dev)  # :197
        self.an_proj = L.Dense(mixing_size, activation="relu", **dev)   # :198
        if kind == "transfer":  # train_melting_point_transfer.py:95-103 on the viscosity model cut at mix_cat_an
            self.mix = L.AddTwoTensors(name="mix_cat_an", **dev)
            self.mp_dense_1 = L.Dense(256, activation="relu", name="mp_dense_1", **dev)
            self.mp_bn_1 = L.BatchNormalization(name="mp_bn_1", **dev)
            self.mp_dense_2 = L.Dense(128, activation="relu", name="mp_dense_2", **dev)
            self.mp_dropout = L.Dropout(head_dropout_rate, seed=head_dropout_seed, name="mp_dropout", **dev)
            self.mp_dense_3 = L.Dense(64, activation="relu", name="mp_dense_3", **dev)
            self.melting_point = L.Dense(1, name="melting_point", **dev)
        elif kind == "viscosity":
            self.mix = L.AddTwoTensors(name="mix_cat_an", **dev)        # :201
            self.visc_params = L.Dense(3, **dev)                        # :204
            self.param_A = L.SliceParamA(name="param_A", **dev)
            self.param_B = L.SliceParamB(name="param_B", **dev)
            self.param_C = L.SliceParamC(name="param_C", **dev)
            self.scale_T = L.ScaleTemperature(name="scale_T", **dev)
            self.log_eta = L.ComputeLogEta(name="log_eta", **dev)
        else:
            self.mix = L.AddTwoTensors(name="add", **dev)               # keras Add(), train_melting_point.py:191
            self.mp_hidden = L.Dense(fp_size, activation="relu", kernel_regularizer=("l2", fp_l2), **dev)  # :197
            self.mp_out = L.Dense(1, **dev)                             # :198
        self._build_all()
        self._packed = None
        self._prepared = {}
        self._split_deg_limit = None
        self.encoder_mode = "auto"  # "auto" | "f32t" | "f32x3" | "f32" | "f16x2" (ops.encoder_fused)
        self.encoder_workgroups = 0  # persistent workgroups per encoder launch (0: library default, one per CU)
        self._transfer_grid_image = None
        self._encoder_version = 0  # moves on whenever the encoder's packed weights are dropped (data.FrozenEncodings)
        self._frozen_state_version = 0  # moves on when weights are written from outside a step (data.FrozenStates)
        self._frozen_prefix_epoch = 0  # moves on when a compile() changes frozen_prefix() (data.FrozenStates)
        self.grid_head_mode = "auto"  # "auto" | "gathered": predict_grid's head for the transfer model

    # ------------------------------------------------------------------ construction
    def _build_all(self):
        D, K = self.atom_dim, self.bond_dim
        for lyr, shape in ((self.atom_emb, (None, None)), (self.bond_emb, (None, None))):
            lyr.build(shape); lyr.built = True
        for p in ("cat", "an"):
            br = self.branches[p]
            for i in range(self.num_steps):
                br["bmm"][i].build([(None, None, D), (None, None, K), (None, None, 2)]); br["bmm"][i].built = True
                br["update"][i].build([(None, None, D), (None, None, D)]); br["update"][i].built = True
                br["reduce"][i].built = True
            br["pool"].built = True
            br["fp"].build((None, D)); br["fp"].built = True
        for lyr in (self.cat_proj, self.an_proj):
            lyr.build((None, self.fp_size)); lyr.built = True
        if self.kind == "transfer":
            width = self.mixing_size
            for lyr in self._transfer_head_layers():
                lyr.build((None, width)); lyr.built = True
                width = getattr(lyr, "units", width)
        elif self.kind == "viscosity":
            self.visc_params.build((None, self.mixing_size)); self.visc_params.built = True
        else:
            self.mp_hidden.build((None, self.mixing_size)); self.mp_hidden.built = True
            self.mp_out.build((None, self.fp_size)); self.mp_out.built = True

    @property
    def layers(self):
        out = [self.atom_emb, self.bond_emb]
        for p in ("cat", "an"):
            br = self.branches[p]
            for i in range(self.num_steps):
                out += [br["bmm"][i], br["reduce"][i], br["update"][i]]
            out += [br["pool"], br["fp"]]
        out += [self.cat_proj, self.an_proj, self.mix]
        if self.kind == "transfer":
            out += self._transfer_head_layers()
        elif self.kind == "viscosity":
            out += [self.visc_params, self.param_A, self.param_B, self.param_C, self.scale_T, self.log_eta]
        else:
            out += [self.mp_hidden, self.mp_out]
        return out

    def _transfer_head_layers(self):
        return [self.mp_dense_1, self.mp_bn_1, self.mp_dense_2, self.mp_dropout, self.mp_dense_3, self.melting_point]

    def get_layer(self, name):
        for lyr in self.layers:
            if lyr.name == name:
                return lyr
        raise ValueError(f"No such layer: {name}")

    # ------------------------------------------------------------------ weights
    def _owned_tensors(self):
        """[(name, tensor, owning layer)] of every weight, in the fixed order of the weight files."""
        t = [("atom_embedding", self.atom_emb.embeddings, self.atom_emb),
             ("bond_embedding", self.bond_emb.embeddings, self.bond_emb)]
        dense = lambda prefix, lyr: [(f"{prefix}/kernel", lyr.kernel, lyr), (f"{prefix}/bias", lyr.bias, lyr)]
        for p in ("cat", "an"):
            br = self.branches[p]
            for i in range(self.num_steps):
                t.append((f"{p}_bmm_{i}/bond_transform", br["bmm"][i].bond_transform, br["bmm"][i]))
                for wn, w in br["update"][i]._weights.items():
                    t.append((f"{p}_gu_{i}/{wn}", w, br["update"][i]))
            t += dense(f"{p}_fp", br["fp"])
        t += dense("cat_proj", self.cat_proj) + dense("an_proj", self.an_proj)
        if self.kind == "transfer":
            bn = self.mp_bn_1
            t += dense("mp_dense_1", self.mp_dense_1) + [("mp_bn_1/gamma", bn.gamma, bn), ("mp_bn_1/beta", bn.beta, bn)]
            t += dense("mp_dense_2", self.mp_dense_2) + dense("mp_dense_3", self.mp_dense_3)
            t += dense("melting_point", self.melting_point)
        elif self.kind == "viscosity":
            t += dense("visc_params", self.visc_params)
        else:
            t += dense("mp_hidden", self.mp_hidden) + dense("mp_out", self.mp_out)
        return t

    def _named_tensors(self):
        return {n: w for n, w, _ in self._owned_tensors()}

    def _named_state(self):
        """What a training run changes besides the weights: BatchNormalization's moving statistics."""
        if self.kind != "transfer":
            return {}
        return {"mp_bn_1/moving_mean": self.mp_bn_1.moving_mean, "mp_bn_1/moving_variance": self.mp_bn_1.moving_variance}

    def variables(self):
        """[(name, tensor)] of everything a training run changes or a file must hold: all weights, trainable or
        frozen, then the moving statistics."""
        return list(self._named_tensors().items()) + list(self._named_state().items())

    def state_dict(self):
        return {k: v.detach().cpu().numpy().copy() for k, v in self.variables()}

    def load_weights(self, weights):
        """weights: dict name -> array in the naming of ionic_mpnn_amd.weights, or the path of a save_weights file."""
        if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
            weights = self.load_weight_file(weights)[1]
        named = dict(self.variables())
        missing = sorted(set(named) - set(weights))
        if missing:
            raise KeyError(f"missing weights: {missing[:5]}{'...' if len(missing) > 5 else ''}")
        for k, t in named.items():
            a = np.ascontiguousarray(np.asarray(weights[k], dtype=np.float32))
            if tuple(a.shape) != tuple(t.shape):
                raise ValueError(f"{k}: shape {a.shape} != {tuple(t.shape)}")
            with torch.no_grad():
                t.copy_(torch.from_numpy(a))
        self.invalidate_packed_weights()

    # ---- f3: configuration and weight files (the .keras archive itself needs an HDF5 reader: not here)
    def get_config(self):
        """Constructor arguments + per-layer configs (keras Model.get_config analogue, models/layers.py:119-125)."""
        return {"name": self.name, "kind": self.kind, "atom_vocab_size": self.atom_vocab_size,
                "bond_vocab_size": self.bond_vocab_size, "atom_dim": self.atom_dim, "bond_dim": self.bond_dim,
                "fp_size": self.fp_size, "mixing_size": self.mixing_size, "num_steps": self.num_steps,
                "fp_l2": self.fp_l2, "dropout_rate": self.dropout_rate, "dropout_seed": self.dropout_seed,
                **({"head_dropout_rate": self.mp_dropout.rate, "head_dropout_seed": self.mp_dropout.seed}
                   if self.kind == "transfer" else {}),
                "layer_trainable": {l.name: bool(l.trainable) for l in self.layers},
                "embedding_trainable_rows": {l.name: (None if l.trainable_rows is None else list(l.trainable_rows))
                                             for l in (self.atom_emb, self.bond_emb)},
                "layers": [{"class_name": type(l).__name__, "config": l.get_config()} for l in self.layers]}

    @classmethod
    def from_config(cls, config, device=None):
        L.reset_uids()  # keras auto-names (gated_update_3, ...) restart with a new model graph
        m = cls(config["kind"], config["atom_vocab_size"], config["bond_vocab_size"], config["atom_dim"],
                config["bond_dim"], config["fp_size"], config["mixing_size"], config["num_steps"],
                config.get("fp_l2", 1e-4), device=device, name=config.get("name"),
                dropout_rate=config.get("dropout_rate", 0.0), dropout_seed=config.get("dropout_seed"),
                head_dropout_rate=config.get("head_dropout_rate", 0.3),
                head_dropout_seed=config.get("head_dropout_seed"))
        flags = config.get("layer_trainable") or {}  # (absent in files written before layers could be frozen)
        for lyr in m.layers:
            lyr.trainable = bool(flags.get(lyr.name, True))
        rows = config.get("embedding_trainable_rows") or {}  # (absent in files written before rows could be listed)
        for lyr in (m.atom_emb, m.bond_emb):
            lyr.trainable_rows = rows.get(lyr.name)
        return m

    def save_weights(self, path):
        """All variables under their Keras-style names (ionic_mpnn_amd.weights) plus the config, as one .npz."""
        import json
        arrays = self.state_dict()  # every variable, frozen or not, and the moving statistics
        cfg = {k: v for k, v in self.get_config().items() if k != "layers"}  # (keeps each layer's trainable flag)
        # through a file handle: np.savez(path, ...) appends ".npz" to any other suffix, and the reference flow saves
        # to "models/viscosity_final.keras" and loads that very name (train_melting_point_transfer.py:78)
        with open(path, "wb") as f:
            np.savez(f, __config__=np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8), **arrays)

    def save(self, path):
        """model.save("models/viscosity_final.keras") (train_viscosity.py:354) - here the npz container of save_weights
        (config + variables) under exactly the name given; the Keras zip/HDF5 container is not written."""
        self.save_weights(path)

    @staticmethod
    def load_weight_file(path):
        """-> (config dict, weights dict) from a file written by save_weights (no pickle is involved)."""
        import json
        import os as _os
        if not _os.path.exists(path) and _os.path.exists(str(path) + ".npz"):
            path = str(path) + ".npz"  # files written before round 2 (np.savez appended the suffix then)
        with np.load(path, allow_pickle=False) as z:
            cfg = json.loads(bytes(z["__config__"].tobytes()).decode())
            return cfg, {k: z[k] for k in z.files if k != "__config__"}

    GRID_HEAD_MODES = ("auto", "gathered")

    @property
    def grid_head_mode(self):
        """How ``predict_grid`` evaluates the transfer head: "auto" takes the matrix-core grid kernel
        (impnn_transfer_head_grid) where it covers the model, "gathered" always runs ``self.head`` on gathered tiles of
        pairs.  The viscosity and melting-point models ignore it."""
        return self._grid_head_mode

    @grid_head_mode.setter
    def grid_head_mode(self, mode):
        if mode not in self.GRID_HEAD_MODES:
            raise ValueError(f"grid_head_mode must be one of {self.GRID_HEAD_MODES}, got {mode!r}")
        self._grid_head_mode = mode

    def invalidate_packed_weights(self):
        """Call after mutating layer weights in place; the fused encoder caches a packed copy."""
        self._transfer_grid_image = None
        self._packed = None
        self._prepared = {}
        self._split_deg_limit = None
        self._head_packed = None
        self._encoder_version += 1
        self._frozen_state_version += 1
        for p in ("cat", "an"):
            for lyr in self.branches[p]["bmm"]:
                lyr.invalidate_cache()

    def weights_updated(self):
        """After an optimizer step: drops the caches that hold copies of variables the step changed, and only those.
        The packed head, the packed encoder weights, an image and a frozen message layer's type matrices stay when
        nothing they were built from trains - a captured training step reads them on every replay."""
        if any(t.requires_grad for t in self._head_tensors()):
            self._head_packed = None
        if self.kind == "transfer" and (getattr(self, "_bn_training", self.mp_bn_1.trainable)
                                        or any(t.requires_grad for t in self._head_tensors()[10:])):
            self._transfer_grid_image = None  # (a frozen tail keeps its image, as a frozen encoder its prepared weights)
        steps = any(t.requires_grad for n, t in self._named_tensors().items() if "_bmm_" in n or "_gu_" in n)
        atom, table = self.atom_emb.embeddings.requires_grad, self.bond_emb.embeddings.requires_grad
        if steps:
            self._packed = None
        if steps or atom or table:
            # an image holds the step weights; the typed modes fold the bond table in as well and, at atom_dim 32, the
            # atom table (include/impnn.h, impnn_encoder_prepare_weights_gates); the degree limit reads both tables
            stale = lambda m: steps or (m in ("f32t", "f32x3") and (table or (atom and self.atom_dim == 32)))
            self._prepared = {m: image for m, image in self._prepared.items() if not stale(m)}
            self._split_deg_limit = None
            self._encoder_version += 1
        for p in ("cat", "an"):
            for lyr in self.branches[p]["bmm"]:
                if table or lyr.bond_transform.requires_grad:
                    lyr.invalidate_cache()

    @property
    def encoder_version(self):
        """The version of the encoder's weights: ``invalidate_packed_weights`` (so ``load_weights``) and every
        ``weights_updated`` of a model whose encoder trains move it on, with the packed weights they drop.  What was
        computed from the encoder at an older version (data.FrozenEncodings) is stale."""
        return self._encoder_version

    @property
    def frozen_state_version(self):
        """The version of the weights a step cannot change: ``invalidate_packed_weights`` (so ``load_weights``) moves
        it on, ``weights_updated`` does not - a training step writes trainable variables only, and what was computed
        from the frozen ones (data.FrozenStates) stays valid while ``frozen_prefix()`` stays what it was."""
        return self._frozen_state_version

    @property
    def frozen_prefix_epoch(self):
        """Counts the ``compile()`` calls that changed ``frozen_prefix()``.  A step under another prefix may have trained
        what lies below the old one, and ``weights_updated`` leaves ``frozen_state_version`` alone: states made before
        such a compile are stale even when a later compile brings their prefix back (data.FrozenStates)."""
        return self._frozen_prefix_epoch

    def frozen_prefix(self):
        """{"cat": s, "an": s}: per ion, what ``_first_trained_step`` returns inside a differentiated pass, read from
        the ``requires_grad`` flags that ``compile()`` set.  0: nothing is cacheable (an embedding or step 0 trains);
        1..num_steps-1: the atom embedding and steps 0..s-1 are frozen; None: the ion's whole encoder is."""
        with torch.enable_grad():
            return {p: self._first_trained_step(p) for p in ("cat", "an")}

    def _cache_refs(self):
        """The cached tensors a captured step may read (kept alive by train.GraphedTrainStep)."""
        return [dict(self._prepared), self._packed] + [getattr(l, "_mats_cache", None)
                                                       for p in ("cat", "an") for l in self.branches[p]["bmm"]]

    def _head_tensors(self):
        """Head weight tensors in the order of impnn_model_head's packed layout (include/impnn.h)."""
        parts = []
        for p in ("cat", "an"):
            parts += [self.branches[p]["fp"].kernel, self.branches[p]["fp"].bias]
        parts += [self.cat_proj.kernel, self.cat_proj.bias, self.an_proj.kernel, self.an_proj.bias]
        if self.kind == "transfer":  # the order of impnn_transfer_head's `weights`
            bn = self.mp_bn_1
            parts += [self.mp_dense_1.kernel, self.mp_dense_1.bias, bn.gamma, bn.beta, self.mp_dense_2.kernel,
                      self.mp_dense_2.bias, self.mp_dense_3.kernel, self.mp_dense_3.bias, self.melting_point.kernel,
                      self.melting_point.bias]
        elif self.kind == "viscosity":
            parts += [self.visc_params.kernel, self.visc_params.bias]
        else:
            parts += [self.mp_hidden.kernel, self.mp_hidden.bias, self.mp_out.kernel, self.mp_out.bias]
        return parts

    def _packed_head(self):
        """Head weights in the layout of impnn_model_head (include/impnn.h), cached per weight version."""
        if getattr(self, "_head_packed", None) is None:
            with torch.no_grad():
                self._head_packed = torch.cat([t.reshape(-1) for t in self._head_tensors()]).contiguous()
        return self._head_packed

    def _transfer_image(self):
        """The weight image of impnn_transfer_head_grid (ops.transfer_grid_prepare), cached per weight version."""
        if self._transfer_grid_image is None:
            with torch.no_grad():
                self._transfer_grid_image = ops.transfer_grid_prepare(self._head_tensors(), self._transfer_cfg(False))
        return self._transfer_grid_image

    def _prepared_weights(self, mode):
        """Kernel-side weight images (one per ion), built once per weight version and mode.  The typed modes fold the atom
        embedding in as well (the step-0 message table and, behind it, the step-0 gate table - both depend on the atom
        embedding and on step 0's weights): invalidate_packed_weights drops the images after an in-place change,
        weights_updated the images whose sources train (a typed image also when an embedding does)."""
        if mode not in self._prepared:
            self._prepared[mode] = [ops.prepare_encoder_weights(pk, self.bond_emb.embeddings, self.atom_dim,
                                                                self.bond_dim, self.num_steps, mode,
                                                                atom_table=self.atom_emb.embeddings)
                                    if pk is not None else None for pk in self._packed_weights()]
        return self._prepared[mode]

    def _packed_weights(self):
        if self._packed is None or self._split_deg_limit is None:
            # (the limit alone is missing after a step that trained an embedding and no step weight: weights_updated)
            packed, limit = [], None
            for p in ("cat", "an"):
                br = self.branches[p]
                steps = []
                for i in range(self.num_steps):
                    w = br["update"][i]._weights
                    steps.append({"bond_transform": br["bmm"][i].bond_transform,
                                  "Wz": w["dense_z/kernel"], "bz": w["dense_z/bias"],
                                  "Wr": w["dense_r/kernel"], "br": w["dense_r/bias"],
                                  "Wh": w["dense_h/kernel"], "bh": w["dense_h/bias"],
                                  "gamma": w["layernorm/gamma"], "beta": w["layernorm/beta"]})
                packed.append(ops.pack_step_weights(steps))
                lim = ops.split_mode_degree_limit(self.atom_emb.embeddings, self.bond_emb.embeddings, steps,
                                                  self.atom_dim)
                limit = lim if limit is None else min(limit, lim)
            if self._packed is None:
                self._packed = packed
            self._split_deg_limit = limit
        return self._packed

    def resolve_encoder_mode(self, N, E=None):
        """The fused encoder mode for (N, E)-shaped ion inputs, or None when no mode covers them.
        "auto" picks exact-f32 arithmetic only: "f32t" (per-bond-type messages, any bond_dim) first, then "f32"
        (pull form, bond_dim <= 8).  "f16x2" (split-fp16 products, narrower than f32) is used on request only, and
        then only while its static range bound holds for every possible in-degree (<= E edge slots); otherwise the
        request falls back to the exact modes.  "f32x3" (f32 as bf16x9: as exact as f32, another summation order) is used
        on request where the shape allows it and falls back to "f32t" where it does not."""
        if E is None:  # (older call sites passed E alone)
            N, E = 1, N
        sup = lambda m: ops.encoder_fused_supported(N, E, self.atom_dim, self.bond_dim, self.num_steps,
                                                    self.bond_vocab_size, m)
        want = self.encoder_mode
        if want == "f16x2":
            self._packed_weights()
            if sup("f16x2") and (self._split_deg_limit is None or E <= self._split_deg_limit):
                return "f16x2"
            want = "auto"
        if want == "f32x3" and not sup("f32x3") and sup("f32t"):
            return "f32t"  # a shape only the exact-f32 form of the same path takes
        if want in ("f32t", "f32", "f32x3"):
            return want if sup(want) else None
        for m in ("f32t", "f32"):
            if sup(m):
                return m
        return None

    # ------------------------------------------------------------------ forward
    def fused_supported(self, N, E):
        return self.resolve_encoder_mode(N, E) is not None

    def _builds_graph(self):
        """True when this call is differentiated: grad mode on and some variable asks for a gradient."""
        return torch.is_grad_enabled() and any(t.requires_grad for t in self._named_tensors().values())

    def _first_trained_step(self, prefix):
        """The lowest message-passing step of an ion below which a differentiated pass keeps nothing: the first whose
        BondMatrixMessage or GatedUpdate asks for a gradient; 0 when an embedding does (the atom embedding feeds step
        0, the bond embedding every step's type matrices); None when nothing in the ion's encoder does."""
        if not torch.is_grad_enabled():
            return None
        if self.atom_emb.embeddings.requires_grad or self.bond_emb.embeddings.requires_grad:
            return 0
        br = self.branches[prefix]
        for i in range(self.num_steps):
            if br["bmm"][i].bond_transform.requires_grad or any(w.requires_grad for w in br["update"][i].weights):
                return i
        return None

    def _encoder_trains(self):
        """True when a differentiated pass has to keep an encoder graph (some embedding or step asks for a gradient)."""
        return any(self._first_trained_step(p) is not None for p in ("cat", "an"))

    def _all_type_matrices(self):
        """Training: the type matrices of every message layer from one node (3 launches per step instead of 3 per
        layer) as {(ion, step): (matrices, their slice of the node's gradient pool)}; None where the per-layer entries
        are the better fit (bond_dim >= 64 is GEMM-shaped)."""
        if self.bond_dim >= 64 or self.num_steps == 0 or not self._encoder_trains():
            return None
        from . import autograd
        # (a frozen layer's matrices come from its cache and get no gradient; a trainable bond embedding needs every
        #  layer's)
        table = self.bond_emb.embeddings.requires_grad
        keys = [(p, i) for p in ("cat", "an") for i in range(self.num_steps)
                if table or self.branches[p]["bmm"][i].bond_transform.requires_grad]
        if not keys:
            return None
        *mats, pool = autograd.BondTypeMatricesAll.apply(
            self.bond_emb.embeddings, *[self.branches[p]["bmm"][i].bond_transform for p, i in keys])
        return {k: (mats[j], None if pool is None else pool[j]) for j, k in enumerate(keys)}

    def dropout_counter(self):
        """The model's device dropout step counter (None at rate 0): every training pass snapshots and advances it once
        (ops.dropout_step), before the two ions fork, and both ions' layers draw their masks from that snapshot."""
        if self.dropout_rate == 0.0 and self.kind != "transfer":  # (the transfer head's Dropout always owns one)
            return None
        if self._dropout_counter is None:
            self._dropout_counter = torch.zeros(1, dtype=torch.int64, device=self.device)
        return self._dropout_counter

    def _layer_dropout(self, prefix, i, step):
        """ops.Dropout of step i of an ion in the pass whose snapshot is ``step`` (layer id: cation i, anion S + i)."""
        from . import dist as idist
        lid = i + (self.num_steps if prefix == "an" else 0)
        return ops.Dropout(self.dropout_rate, self.dropout_seed, ops.dropout_layer_word(lid, idist.dropout_rank()), step)

    def encode_layered(self, prefix, atom_ids, bond_ids, conn, trace=None, typed=True, type_mats=None,
                       dropout_step=None, start=0, h0=None, atoms=None):
        """encode() layer at a time (train_viscosity.py:171-187) -> pooled (B,D); type_mats: _all_type_matrices().
        dropout_step: the pass's dropout snapshot (a training pass of a model with dropout_rate > 0), else None.
        ``start=s, h0=h`` (cached frozen steps, data.FrozenStates): the pass resumes at step s from the atom states
        ``h0`` (B,N,D) as they stand after step s-1 - no atom embedding launch, no step below s; every row of ``h0``,
        padding included, must be finite.  s may not lie above the ion's first trained step.
        ``atoms`` (a pass from step 0): the ion's embedded atoms (B,N,D), which the caller has looked up already."""
        br = self.branches[prefix]
        graph = ops.IonGraph(atom_ids, bond_ids, conn, self.bond_vocab_size)  # the message calls of all layers share it
        s0 = self._first_trained_step(prefix)
        if h0 is None:
            if start != 0:
                raise ValueError("encode_layered: start > 0 needs the atom states h0 to start from")
            h = self.atom_emb(atom_ids) if atoms is None else atoms
        else:
            if not 0 < start < self.num_steps or trace is not None or not typed:
                raise ValueError(f"encode_layered: a resumed pass starts at a step in 1..{self.num_steps - 1}, typed, "
                                 "without a trace")
            if s0 is not None and start > s0:
                raise ValueError(f"encode_layered: start={start} lies above the {prefix} ion's first trained step {s0}")
            if tuple(h0.shape) != tuple(atom_ids.shape) + (self.atom_dim,) or h0.dtype != torch.float32:
                raise ValueError(f"encode_layered: h0 must be float32 {tuple(atom_ids.shape) + (self.atom_dim,)}")
            h = h0
        bond = self.bond_emb(bond_ids)
        if not typed:
            bond = bond.dense()
        one_node = typed and trace is None and s0 is not None  # training: a whole step as one autograd node
        # inference through the layered path (what serves atom_dim 64 / 128): GatedUpdate only on the rows an
        # encode() loop has to carry - padding atoms can reach neither a message nor the pool (include/impnn.h,
        # impnn_gated_update_rows); their rows of h are left undefined and are never read
        rows = None
        # (atom_dim 32 has the entry too, but there the three small launches that build the list cost what the skipped
        #  rows save: measured 8.1 vs 8.5 M pairs/s at batch 4096)
        if typed and trace is None and self.atom_dim in (64, 128) and self.num_steps > 0 and (
                s0 is None or atom_ids.numel() >= TRAIN_ROW_LIST_MIN_ROWS):
            # (training too, from TRAIN_ROW_LIST_MIN_ROWS atom rows per ion: the one-node step runs GatedUpdate forward
            #  AND backward on the list, impnn_gated_update_rows_bwd - padding atoms carry no gradient; below that a
            #  step is bound by its launch count and the list's own launches cost more than the skipped rows save)
            rows = ops.kept_row_index(atom_ids, bond_ids, conn, self.bond_vocab_size)
        for i in range(start, self.num_steps):
            drop = self._layer_dropout(prefix, i, dropout_step) if dropout_step is not None else None
            if one_node and i >= s0:
                from . import autograd
                mats, dmats = (type_mats[(prefix, i)] if type_mats and (prefix, i) in type_mats
                               else (br["bmm"][i]._type_matrices(bond.table), None))
                u, w = br["update"][i], br["update"][i]._weights
                h = autograd.MessagePassingStep.apply(
                    h, bond.ids, conn, mats, w["dense_z/kernel"], w["dense_z/bias"], w["dense_r/kernel"],
                    w["dense_r/bias"], w["dense_h/kernel"], w["dense_h/bias"], u.gamma, u.beta, u.epsilon, graph, dmats,
                    *(rows if rows is not None else (None, None)), i > s0, drop)
                continue
            with torch.set_grad_enabled(torch.is_grad_enabled() and not one_node):  # (one_node: a step below s0)
                if typed:  # (the layer's own call would sort the edges again)
                    m = ops.bmm_message_typed(h, bond.ids, conn, br["bmm"][i]._type_matrices(bond.table), graph)
                else:
                    m = br["bmm"][i]([h, bond, conn])
                agg = br["reduce"][i]([m, conn[:, :, 1], h])
                if rows is not None or drop is not None:
                    u, w = br["update"][i], br["update"][i]._weights
                    h = ops.gated_update(h, agg, w["dense_z/kernel"], w["dense_z/bias"], w["dense_r/kernel"],
                                         w["dense_r/bias"], w["dense_h/kernel"], w["dense_h/bias"], u.gamma, u.beta,
                                         u.epsilon, rows=rows, dropout=drop)
                else:
                    h = br["update"][i]([h, agg])
            if trace is not None:
                trace[f"{prefix}/m{i}"], trace[f"{prefix}/agg{i}"], trace[f"{prefix}/h{i + 1}"] = m, agg, h
        pooled = br["pool"]([h, atom_ids])
        if trace is not None:
            trace[f"{prefix}/pooled"] = pooled
        return pooled

    def plan_batch(self, inputs):
        """Enqueues the graph-only plan of a batch on a side stream (ops.EncoderPipeline) and returns
        a handle for ``encode_pooled(inputs, plan=handle)``.  Call it for batch i+1 before encoding
        batch i: the plan then runs underneath the encoder of batch i."""
        if getattr(self, "_pipeline", None) is None:
            self._pipeline = ops.EncoderPipeline(self.device)
        ions = [(inputs["cat_atom"], inputs["cat_bond"], inputs["cat_connectivity"]),
                (inputs["an_atom"], inputs["an_bond"], inputs["an_connectivity"])]
        mode = self.resolve_encoder_mode(inputs["cat_atom"].shape[1], inputs["cat_bond"].shape[1])
        if mode is None:
            raise ops.EncoderUnsupported("no fused encoder mode covers this model / batch shape")
        return self._pipeline.plan(ions, self.atom_dim, self.bond_dim, self.num_steps, self.atom_vocab_size,
                                   self.bond_vocab_size, mode=mode, workgroups=self.encoder_workgroups)

    def encode_pooled(self, inputs, fused=None, trace=None, plan=None, training=False, dropout_step=None, states=None):
        """Both ions' GlobalSumPool outputs: the hot path.  ``training`` (layer at a time only):
        a training pass - GatedUpdate's dropout applies when the model has a rate above 0.
        ``states=(st, cat_row, an_row)`` (a training pass over data.FrozenStates; cat_row / an_row: the batch's (B)
        int32 rows of st's tables): one impnn_state_rows launch for both ions comes first; an ion with frozen steps
        resumes the layered pass behind them, an ion whose whole encoder is frozen takes its row as its pooled vector."""
        if states is not None:
            if plan is not None or fused or trace is not None or not training:
                raise ValueError("states go with a layered training pass (no plan, no fused encoder, no trace)")
            return self._encode_resumed(inputs, states)
        if plan is not None:
            mode = plan.mode
            pc, pa = self._pipeline.run(plan, self.atom_emb.embeddings, self.bond_emb.embeddings,
                                        self._prepared_weights(mode), mode=mode)
            if trace is not None:
                trace["cat/pooled"], trace["an/pooled"] = pc, pa
            return pc, pa
        ca, cb, cc = inputs["cat_atom"], inputs["cat_bond"], inputs["cat_connectivity"]
        aa, ab, ac = inputs["an_atom"], inputs["an_bond"], inputs["an_connectivity"]
        if fused is None:
            fused = (tuple(ca.shape) == tuple(aa.shape) and tuple(cb.shape) == tuple(ab.shape)
                     and self.fused_supported(ca.shape[1], cb.shape[1]))
        if fused:
            mode = self.resolve_encoder_mode(ca.shape[1], cb.shape[1])
            if mode is None:
                raise ops.EncoderUnsupported("no fused encoder mode covers this model / batch shape")
            prepared = self._prepared_weights(mode) if self.num_steps > 0 else None
            try:
                pc, pa = ops.encoder_fused([(ca, cb, cc), (aa, ab, ac)], self.atom_emb.embeddings,
                                           self.bond_emb.embeddings, None if prepared else self._packed_weights(),
                                           self.num_steps, mode=mode, prepared=prepared,
                                           workgroups=self.encoder_workgroups)
            except ops.EncoderOverflow:
                # a molecule of THIS batch exceeds a chunk (possible only for N > 256 or E > 255): layer at a time
                self.overflow_fallbacks = getattr(self, "overflow_fallbacks", 0) + 1
                return self.encode_pooled(inputs, fused=False, trace=trace)
            if trace is not None:
                trace["cat/pooled"], trace["an/pooled"] = pc, pa
            return pc, pa
        if training and fused:
            raise ValueError("a training pass runs layer at a time (fused=False)")
        # dropout: one snapshot of the step counter per pass, taken before the ions fork; it lives with the pass
        # (the autograd nodes of both ions hold it), so interleaved passes keep their own masks in the backward
        # (dropout_step: the caller took the pass's snapshot already - the transfer model, whose head shares it)
        ds = None
        if training and self.dropout_rate > 0.0:
            ds = dropout_step if dropout_step is not None else ops.dropout_step(self.dropout_counter())
        tm = self._all_type_matrices() if trace is None else None
        if trace is None and getattr(self, "two_streams", True) and ca.is_cuda \
                and ca.shape[0] <= int(os.environ.get("IMPNN_TWO_STREAM_MAX_BATCH", TWO_STREAM_MAX_BATCH)):
            return self._encode_two_streams((ca, cb, cc), (aa, ab, ac), tm, ds)
        return (self.encode_layered("cat", ca, cb, cc, trace, type_mats=tm, dropout_step=ds),
                self.encode_layered("an", aa, ab, ac, trace, type_mats=tm, dropout_step=ds))

    def _encode_resumed(self, inputs, states):
        """encode_pooled over cached frozen steps (DESIGN.md 6.1 "Cached frozen steps"; ``_loss`` has refused what
        ``_frozen_steps_check`` refuses, GatedUpdate dropout among it: the pass has no dropout snapshot)."""
        st, cat_row, an_row = states
        if st.stale(self):
            raise ValueError(f"the states were made at frozen-state version {st.version} for the prefix {st.steps}, the "
                             f"model is at {self.frozen_state_version} with {self.frozen_prefix()} (load_weights, or a "
                             "compile that moved the first trained step): build them again")
        pre = st.steps
        ions = {"cat": (inputs["cat_atom"], inputs["cat_bond"], inputs["cat_connectivity"]),
                "an": (inputs["an_atom"], inputs["an_bond"], inputs["an_connectivity"])}
        B = int(ions["cat"][0].shape[0])
        kept = [(p, t, r) for p, t, r in (("cat", st.cat, cat_row), ("an", st.an, an_row)) if pre[p] != 0]
        for p, t, r in kept:
            if r.numel() != B or (pre[p] is not None and t.shape[1] != ions[p][0].shape[1]):
                raise ValueError(f"the {p} states hold rows of {t.shape[1]} atoms for {r.numel()} samples; the batch has "
                                 f"{B} samples of {ions[p][0].shape[1]} atoms")
        got = dict(zip([p for p, _, _ in kept],
                       ops.state_rows([t for _, t, _ in kept], [r for _, _, r in kept])))  # one launch, both ions
        layered = [p for p in ("cat", "an") if pre[p] is not None]
        tm = self._all_type_matrices()
        resume = {p: (pre[p], got.get(p)) for p in layered}
        ca = ions["cat"][0]
        if len(layered) == 2 and getattr(self, "two_streams", True) and ca.is_cuda \
                and ca.shape[0] <= int(os.environ.get("IMPNN_TWO_STREAM_MAX_BATCH", TWO_STREAM_MAX_BATCH)):
            return self._encode_two_streams(ions["cat"], ions["an"], tm, None, resume)
        # (an ion whose whole encoder is frozen: its gathered (B,1,D) row IS its pooled vector)
        return tuple(self.encode_layered(p, *ions[p], None, type_mats=tm, start=resume[p][0], h0=resume[p][1])
                     if p in resume else got[p].reshape(B, self.atom_dim) for p in ("cat", "an"))

    def _encode_two_streams(self, cat, an, tm, dropout_step=None, resume=None):
        """Layer-at-a-time path: the two ions' chains are independent until the head, and most of their kernels
        leave part of the chip idle (a batch-32 kernel nearly all of it) - the anion chain runs on a second HIP stream
        (in training: a parallel branch of the captured hipGraph; autograd replays each node's backward on the stream
        of its forward).  Tensors allocated on
        the current stream and read by the side stream are recorded there, so the caching allocator does not reuse
        them before the side stream is done.  ``join_training_streams`` after backward() orders the gradient sinks
        written on the side stream before the optimizer step."""
        from . import autograd
        cur = torch.cuda.current_stream(self.device)
        side = getattr(self, "_side_stream", None)
        if side is None:
            side = self._side_stream = torch.cuda.Stream(device=self.device)
            # leaves reached from the side chain through AccumulateGrad (bond_dim >= 64 keeps per-layer type-matrix
            # nodes) see a producer on another stream than their own: intended here, torch syncs the two
            quiet = getattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch", None)
            if quiet is not None:
                quiet(False)
        for (p, _), (mats, dmats) in (tm or {}).items():
            if p == "an":
                mats.record_stream(side)
                if dmats is not None:
                    dmats.record_stream(side)
        for t in an:
            t.record_stream(side)
        if dropout_step is not None:
            dropout_step.record_stream(side)
        # (resume: {ion: (start, h0)} of a pass over cached frozen steps; the side stream reads the anion's gathered h0)
        kc, ka = ({} if resume is None else dict(zip(("start", "h0"), resume[p])) for p in ("cat", "an"))
        if ka.get("h0") is not None:
            ka["h0"].record_stream(side)
        elif torch.is_grad_enabled() and autograd._listed_rows(self.atom_emb.embeddings) is not None:
            # a row-restricted atom table: the row kernel adds into the gradient sink without atomics, so the two ions'
            # lookups, and with them their backward nodes, stay on ONE stream - the anion's atoms are looked up here
            ka["atoms"] = self.atom_emb(an[0])
            ka["atoms"].record_stream(side)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            pa = self.encode_layered("an", *an, None, type_mats=tm, dropout_step=dropout_step, **ka)
        pc = self.encode_layered("cat", *cat, None, type_mats=tm, dropout_step=dropout_step, **kc)
        cur.wait_stream(side)
        pa.record_stream(cur)
        self._side_stream_used = True
        if pa.requires_grad:
            # whoever calls backward(): when the gradient reaches the anion chain, queue the join for the end of that
            # backward pass (runs on the calling thread, so "current stream" is the caller's)
            def _queue_join(grad):
                torch.autograd.Variable._execution_engine.queue_callback(self.join_training_streams)
                return grad
            pa.register_hook(_queue_join)
        return pc, pa

    def join_training_streams(self):
        """After loss.backward(): the current stream waits for the side stream of _encode_two_streams (its backward
        kernels add into the gradient buffers in place, which torch's own end-of-backward sync does not see)."""
        if getattr(self, "_side_stream_used", False):
            torch.cuda.current_stream(self.device).wait_stream(self._side_stream)
            self._side_stream_used = False

    def _transfer_cfg(self, training, dropout_step=None):
        """The per-pass settings of the transfer head kernels (autograd.TransferHeadLoss, ops.transfer_head)."""
        from . import dist as idist
        bn, dp = self.mp_bn_1, self.mp_dropout
        drop = None
        if training and dp.rate > 0.0:
            drop = ops.Dropout(dp.rate, dp.seed, ops.dropout_layer_word(L.Dropout.LAYER_ID, idist.dropout_rank()),
                               dropout_step)
        # keras 2: a BatchNormalization frozen at compile() runs in inference mode inside a training pass
        return {"fp_size": self.fp_size, "mixing_size": self.mixing_size, "l2": self._head_l2(),
                "moving_mean": bn.moving_mean, "moving_variance": bn.moving_variance, "momentum": bn.momentum,
                "epsilon": bn.epsilon, "bn_batch": bool(training and getattr(self, "_bn_training", bn.trainable)),
                "dropout": drop, "loss_kind": 0 if self._loss_name() == "mse" else 1, "delta": self._loss_delta()}

    def _loss_name(self):
        return getattr(self, "loss", "mse") if isinstance(getattr(self, "loss", "mse"), str) else "huber"

    def _loss_delta(self):
        loss = getattr(self, "loss", "mse")
        return 1.0 if isinstance(loss, str) else float(loss.delta)

    def head(self, pooled_cat, pooled_an, temperature=None, trace=None, differentiable=False, training=False):
        if self.kind == "transfer":
            if trace is None and not differentiable and self._head_kernels_cover():
                return ops.transfer_head(pooled_cat, pooled_an, self._head_tensors(), self._transfer_cfg(False))
            # layer by layer (traces, model(x, training=True), widths the kernels do not cover)
            fp_cat, fp_an = self.branches["cat"]["fp"](pooled_cat), self.branches["an"]["fp"](pooled_an)
            x = self.mix([self.cat_proj(fp_cat), self.an_proj(fp_an)])
            if trace is not None:
                trace["cat/fp"], trace["an/fp"], trace["mixed"] = fp_cat, fp_an, x
            bn_batch = training and getattr(self, "_bn_training", True)
            if bn_batch and self.mp_bn_1.trainable:
                self._transfer_grid_image = None  # the layer moves its moving statistics, which the grid image holds
            x = self.mp_bn_1(self.mp_dense_1(x), training=bn_batch)
            x = self.mp_dropout(self.mp_dense_2(x), training=training, counter=self.dropout_counter())
            return self.melting_point(self.mp_dense_3(x))
        if trace is None and not differentiable and self._head_kernels_cover():
            return ops.model_head(self.kind, pooled_cat, pooled_an, temperature, self._packed_head(), self.fp_size,
                                  self.mixing_size)  # one launch
        if trace is None and differentiable and self._head_nodes_cover() and torch.is_grad_enabled():
            from . import autograd
            T = temperature if self.kind == "viscosity" else None
            return autograd.ModelHead.apply({"viscosity": 0, "melting_point": 1}[self.kind], self.fp_size,
                                            self.mixing_size, pooled_cat, pooled_an, T, *self._head_tensors())
        fp_cat = self.branches["cat"]["fp"](pooled_cat)   # Dense(fp_size, relu), :189
        fp_an = self.branches["an"]["fp"](pooled_an)
        mixed = self.mix([self.cat_proj(fp_cat), self.an_proj(fp_an)])
        if trace is not None:
            trace["cat/fp"], trace["an/fp"], trace["mixed"] = fp_cat, fp_an, mixed
        if self.kind == "viscosity":
            vp = self.visc_params(mixed)
            if trace is not None:
                trace["visc_params"] = vp
            T = self.scale_T(temperature.to(torch.float32).reshape(-1, 1))
            return self.log_eta([self.param_A(vp), self.param_B(vp), T, self.param_C(vp)])
        return self.mp_out(self.mp_hidden(mixed))

    def __call__(self, inputs, fused=None, trace=None, training=False):
        """Inference by default (no graph is kept, the fused encoder and the head kernel run).  With
        ``training=True`` the call is differentiable: layer-at-a-time path (ionic_mpnn_amd.autograd) and the
        head as one autograd node over impnn_model_head_tensors / impnn_model_head_bwd."""
        inputs = self._to_device(inputs)
        if training:
            pc, pa = self.encode_pooled(inputs, fused=False, training=True)
            return self.head(pc, pa, inputs.get("temperature"), differentiable=True, training=True)
        with torch.no_grad():
            pc, pa = self.encode_pooled(inputs, fused=fused, trace=trace)
            return self.head(pc, pa, inputs.get("temperature"), trace=trace)

    # ------------------------------------------------------------------ training
    def trainable_variables(self):
        """[(name, tensor)] of the weights whose layer is trainable (``layer.trainable``, all by default), in the
        fixed order of ``variables()``; an embedding whose layer is frozen but lists ``trainable_rows`` is among them
        (its listed rows train)."""
        return [(n, w) for n, w, lyr in self._owned_tensors()
                if lyr.trainable or getattr(lyr, "trainable_rows", None) is not None]

    def train_unseen_tokens(self, base_inputs, new_inputs):
        """Lists, as both embeddings' ``trainable_rows``, the tokens ``new_inputs`` uses and ``base_inputs`` (what the
        base model was trained on) never does: data.unseen_tokens, which is returned.  An empty list sets None.  Counts
        from the next ``compile()``, and only for an embedding whose layer is frozen."""
        from . import data
        unseen = data.unseen_tokens(base_inputs, new_inputs, self.atom_vocab_size, self.bond_vocab_size)
        self.atom_emb.trainable_rows = [int(v) for v in unseen.atom] or None
        self.bond_emb.trainable_rows = [int(v) for v in unseen.bond] or None
        return unseen

    def compile(self, optimizer=None, loss="mse", metrics=None, weighted_metrics=None):
        """model.compile(optimizer=Adam(1e-3, clipnorm=1.0), loss="mse") (train_viscosity.py:227-230) or
        loss=Huber(delta=1.0) / "huber" (train_melting_point_transfer.py:193-196).  Reads every ``layer.trainable``
        as Keras does: the optimizer (a fresh state per compile) holds the trainable variables only, the frozen ones
        ask for no gradient and no training step changes them; a flag changed later counts from the next compile.
        A frozen Embedding's ``trainable_rows`` are read the same way: the table asks for a gradient, the backward
        kernels hand the optimizer the listed rows' gradient and +0.0 everywhere else (autograd.restrict_rows), so
        every other row keeps its bits; the table counts as training for ``frozen_prefix()`` and the caches.
        ``metrics`` / ``weighted_metrics``: names ("mae", "mse", "rmse", "bias", "max_error", "r2") or train.Metric
        objects.  ``metrics`` ignore ``sample_weight`` and are logged as ``<name>``, ``weighted_metrics`` use it and are
        logged as ``weighted_<name>`` (``val_`` in front for the validation set); fit and evaluate add them up on the
        device (train.MetricSet).  With neither, fit, evaluate and the captured step are what they are without."""
        from . import train
        if not (loss in ("mse", "huber") or isinstance(loss, train.Huber)):
            raise ValueError("loss must be 'mse', 'huber' or a train.Huber object")
        metric_set = train.MetricSet(metrics, weighted_metrics)  # an unknown name raises before anything is touched
        tv = self.trainable_variables()
        if not tv:
            raise ValueError("no trainable variable: every layer of the model is frozen")
        self.loss = loss
        self._metric_set = metric_set if len(metric_set) else None
        self.optimizer = optimizer if optimizer is not None else train.Adam(1e-3, clipnorm=1.0)
        names = {n for n, _ in tv}
        before = self.frozen_prefix()
        for n, t in self._named_tensors().items():
            t.requires_grad_(n in names)
            if n not in names:
                t.grad = None
        from . import autograd
        for lyr in (self.atom_emb, self.bond_emb):  # (ahead of optimizer.build: a restricted table does not decay)
            autograd.restrict_rows(lyr.embeddings, None if lyr.trainable else lyr.trainable_rows)
        if self.frozen_prefix() != before:
            self._frozen_prefix_epoch += 1
        if self.kind == "transfer":
            self._bn_training = bool(self.mp_bn_1.trainable)
        if isinstance(self.optimizer, train.Adam):  # the names are what exclude_from_weight_decay matches
            self.optimizer.build([t for _, t in tv], names=[n for n, _ in tv])
        else:
            self.optimizer.build([t for _, t in tv])
        return self

    def regularization_loss(self):
        """keras l2(fp_l2) on the fingerprint Dense kernels (train_viscosity.py:189) and, for the melting-point
        model, on the hidden Dense (train_melting_point.py:173,197): fp_l2 * sum(w^2)."""
        ks = [self.branches["cat"]["fp"].kernel, self.branches["an"]["fp"].kernel]
        if self.kind == "melting_point":
            ks.append(self.mp_hidden.kernel)
        return self.fp_l2 * sum((k * k).sum() for k in ks)

    def _head_l2(self):
        """keras l2 lambda per head tensor, in the order of _head_tensors() (see regularization_loss)."""
        lam = [self.fp_l2, 0.0, self.fp_l2, 0.0, 0.0, 0.0, 0.0, 0.0]
        if self.kind == "transfer":
            return lam + [0.0] * 10
        return lam + ([0.0, 0.0] if self.kind == "viscosity" else [self.fp_l2, 0.0, 0.0, 0.0])

    def _metric_pred(self, B):
        """The first B floats of the persistent buffer a fused loss kernel writes its predictions to."""
        buf = getattr(self, "_metric_pred_buf", None)
        if buf is None or buf.numel() < B:
            if buf is not None:  # a captured step may hold its address: a buffer that was outgrown is kept, not freed
                self._metric_pred_kept = getattr(self, "_metric_pred_kept", []) + [buf]
            buf = self._metric_pred_buf = torch.zeros(max(B, 4096), dtype=torch.float32, device=self.device)
        return buf[:B]

    def _loss(self, inputs, y, training, sample_weight=None, metric_slot=None, states=None):
        """The batch loss.  ``sample_weight`` (one finite value >= 0 per sample, or None) makes it keras's weighted
        loss, (1/B) sum_b w_b L_b + penalties, B counting the samples of weight 0 too; it touches the loss only, never
        BatchNormalization's statistics or a dropout mask.  ``metric_slot`` ("train" / "eval"; a model compiled with
        metrics): the pass's predictions are kept and added to that slot's records behind the loss, one
        impnn_regression_sums launch per record; None leaves every call as it is without metrics.
        ``states=(st, cat_row, an_row)``: a training pass that resumes each ion's encoder from its rows of a
        data.FrozenStates (encode_pooled); refused where ``_frozen_steps_check`` refuses."""
        from . import train
        if states is not None:
            self._frozen_steps_check()
            if not training:
                raise ValueError("cache_frozen_steps: states serve a training pass; inference runs the fused encoder")
        y = torch.as_tensor(y, dtype=torch.float32).to(self.device).reshape(-1, 1)
        sw = train.checked_sample_weight(sample_weight, int(y.shape[0]), self.device)
        ms = getattr(self, "_metric_set", None) if metric_slot is not None else None
        if ms is None or y.shape[0] == 0:
            return self._loss_and_pred(inputs, y, training, sw, False, states)[0]
        loss, pred = self._loss_and_pred(inputs, y, training, sw, True, states)
        ms.accumulate(metric_slot, pred.detach().to(torch.float32).reshape(-1).contiguous(), y.reshape(-1), sw)
        return loss

    def _loss_and_pred(self, inputs, y, training, sw, keep_pred, states=None):
        """(loss, predictions or None) of _loss; ``keep_pred`` hands the fused loss kernels a buffer for them."""
        from . import train
        covered = y.shape[0] > 0 and self._head_kernels_cover()
        pbuf = self._metric_pred(int(y.shape[0])) if keep_pred else None
        if self.kind == "transfer" and covered:
            return self._transfer_loss(self._to_device(inputs), y, training, sw, pbuf, states), pbuf
        if training and torch.is_grad_enabled() and covered and self._head_nodes_cover() and self._loss_name() == "mse":
            # head, mse and the l2 penalties as ONE node (impnn_model_head_loss): ~25 launches fewer per step
            from . import autograd
            inputs = self._to_device(inputs)
            need = int(ops._lib.load().impnn_model_head_loss_workspace_floats(int(y.shape[0])))
            ws = getattr(self, "_loss_ws", None)
            if ws is None or ws.numel() < need:
                ws = self._loss_ws = torch.zeros(max(need, 1024), dtype=torch.float32, device=self.device)
            pc, pa = self.encode_pooled(inputs, fused=False, training=True, states=states)
            T = inputs.get("temperature") if self.kind == "viscosity" else None
            l2 = self._head_l2() if sw is None and pbuf is None else autograd.WeightedL2(self._head_l2(), sw, pbuf)
            return autograd.ModelHeadLoss.apply({"viscosity": 0, "melting_point": 1}[self.kind], self.fp_size,
                                                self.mixing_size, l2, ws, pc, pa, T, y, *self._head_tensors()), pbuf
        if states is not None:  # (_frozen_steps_check lets only the two fused loss nodes through)
            raise ValueError("cache_frozen_steps: an empty batch has no resumed pass")
        pred = self(inputs, training=True) if training else self(inputs)
        fn = train.mse if self._loss_name() == "mse" else train.Huber(self._loss_delta())
        if sw is not None:
            unweighted = fn
            fn = lambda y_true, y_pred: unweighted(y_true, y_pred, sw)
        if training:
            return fn(y, pred) + self.regularization_loss(), pred
        with torch.no_grad():
            return fn(y, pred) + self.regularization_loss(), pred

    def _overflow_check(self, inputs):
        """True where the fused encoder would end with its host-side overflow check (N > 256 or E > 255: a molecule
        may exceed a chunk) - a synchronisation a captured training step cannot contain, so training passes of such
        shapes run layer at a time, eager and captured alike."""
        N, E = inputs["cat_atom"].shape[1], inputs["cat_bond"].shape[1]
        mode = self.resolve_encoder_mode(N, E)
        return mode is not None and ops.encoder_overflow_possible(N, E, self.atom_dim, mode)

    def _transfer_loss(self, inputs, y, training, sample_weight=None, pred=None, states=None):
        """The transfer model's loss as one node (impnn_transfer_head_loss[_bwd], the weighted entries with a
        ``sample_weight``).  An encoder with nothing to train
        computes the pooled vectors as inference does - fused encoder where the shape allows, no graph, nothing saved -
        unless its GatedUpdate dropout has to apply; otherwise the layered pass keeps a graph from the first trained
        step up (_first_trained_step)."""
        from . import autograd
        B = int(y.shape[0])
        need = int(ops._lib.load().impnn_transfer_head_loss_workspace_floats(B))
        ws = getattr(self, "_loss_ws", None)
        if ws is None or ws.numel() < need:
            ws = self._loss_ws = torch.zeros(max(need, 1024), dtype=torch.float32, device=self.device)
        # one snapshot of the step counter per training pass, shared by the encoder's GatedUpdates and the head
        ds = ops.dropout_step(self.dropout_counter()) if training else None
        if training and self._encoder_trains():
            pc, pa = self.encode_pooled(inputs, fused=False, training=True, dropout_step=ds, states=states)
        else:
            with torch.no_grad():
                if training and self.dropout_rate > 0.0:
                    pc, pa = self.encode_pooled(inputs, fused=False, training=True, dropout_step=ds)
                else:
                    pc, pa = self.encode_pooled(inputs, fused=False if training and self._overflow_check(inputs) else None)
        with torch.set_grad_enabled(training and torch.is_grad_enabled()):
            cfg = self._transfer_cfg(training, ds)
            if sample_weight is not None:
                cfg = dict(cfg, sample_weight=sample_weight)
            if pred is not None:  # the head kernel writes the pass's predictions there (the metrics read them)
                cfg = dict(cfg, pred=pred)
            return autograd.TransferHeadLoss.apply(cfg, ws, pc, pa, y, *self._head_tensors())

    # ---- stage 1 of transfer learning over cached encodings (data.FrozenEncodings; DESIGN.md "Cached encodings")
    def _frozen_cache_check(self):
        """ValueError unless a training pass of this model needs the encoder for nothing but its pooled rows, and those
        cannot change: what ``cache_frozen_encoder=True`` and ``frozen_encodings`` require."""
        from . import dist as idist
        why = None
        if self.kind != "transfer":
            why = f"it is a {self.kind} model: only the transfer model's head reads indexed rows"
        elif self._encoder_trains():
            why = "an encoder layer is trainable (stage 2): its pooled rows change with every step"
        elif self.dropout_rate > 0.0:
            why = (f"the encoder's GatedUpdate dropout rate is {self.dropout_rate}: a training pass applies it to frozen "
                   "steps too, so the pooled rows differ from step to step")
        elif not self._head_kernels_cover():
            why = (f"the head kernels do not cover atom_dim {self.atom_dim}, fp_size {self.fp_size}, mixing_size "
                   f"{self.mixing_size} (<= {ops.HEAD_MAX_X}, {ops.HEAD_MAX_DIM}, {ops.HEAD_MAX_DIM})")
        elif idist.is_distributed():
            why = "torch.distributed is initialised: data-parallel fits encode per shard"
        if why is not None:
            raise ValueError(f"cache_frozen_encoder: the frozen encoder cannot be cached - {why}")

    def frozen_encodings(self, inputs, batch_size=4096):
        """data.FrozenEncodings of padded model inputs: every distinct ion through ``encode_ions`` once.  Refused
        (ValueError) where ``fit(cache_frozen_encoder=True)`` is."""
        self._frozen_cache_check()
        return data.FrozenEncodings.build(self, inputs, batch_size)

    def _loss_encoded(self, enc, cat_row, an_row, y, training, sample_weight=None, metric_slot=None):
        """``_loss`` of the samples (enc.cat[cat_row[b]], enc.an[an_row[b]]) without their inputs: the head's loss node
        over indexed rows (impnn_transfer_head_loss_rows[_bwd]) - no encoder launch, no gathered copy.  ``cat_row`` /
        ``an_row``: (B) int32 device tensors, rows of ``enc``'s index."""
        from . import autograd, train
        self._frozen_cache_check()
        if enc.stale(self):
            raise ValueError(f"the encodings were made at encoder version {enc.version}, the model is at "
                             f"{self.encoder_version} (load_weights, or a step that trained the encoder): build them again")
        y = torch.as_tensor(y, dtype=torch.float32).to(self.device).reshape(-1, 1)
        B = int(y.shape[0])
        if B == 0:
            raise ValueError("the indexed loss needs at least one sample")
        sw = train.checked_sample_weight(sample_weight, B, self.device)
        ms = getattr(self, "_metric_set", None) if metric_slot is not None else None
        pbuf = self._metric_pred(B) if ms is not None else None
        need = int(ops._lib.load().impnn_transfer_head_loss_workspace_floats(B))
        ws = getattr(self, "_loss_ws", None)
        if ws is None or ws.numel() < need:
            ws = self._loss_ws = torch.zeros(max(need, 1024), dtype=torch.float32, device=self.device)
        ds = ops.dropout_step(self.dropout_counter()) if training else None  # (the head's Dropout: one mask per pass)
        with torch.set_grad_enabled(training and torch.is_grad_enabled()):
            cfg = dict(self._transfer_cfg(training, ds), rows=(cat_row, an_row))
            if sw is not None:
                cfg["sample_weight"] = sw
            if pbuf is not None:
                cfg["pred"] = pbuf
            loss = autograd.TransferHeadLoss.apply(cfg, ws, enc.cat, enc.an, y, *self._head_tensors())
        if ms is not None:
            ms.accumulate(metric_slot, pbuf, y.reshape(-1), sw)
        return loss

    def train_on_encoded_batch(self, enc, rows, y, sample_weight=None, metric_slot=None):
        """``train_on_batch`` on the samples ``rows`` (device int64) of ``enc`` (data.FrozenEncodings): ``y`` and
        ``sample_weight`` hold one value per sample of the batch."""
        if getattr(self, "optimizer", None) is None:
            self.compile()
        kw = {} if metric_slot is None else {"metric_slot": metric_slot}
        loss = self._loss_encoded(enc, torch.index_select(enc.cat_row, 0, rows), torch.index_select(enc.an_row, 0, rows),
                                  y, True, sample_weight, **kw)
        loss.backward()
        self.optimizer.apply_gradients()
        self.optimizer.zero_grad()
        self.weights_updated()
        return loss.detach()

    def _evaluate_encoded(self, enc, y, batch_size, sw, return_dict):
        """``evaluate`` over cached encodings: the same sums, every batch through the indexed loss."""
        n = len(enc)
        ms = getattr(self, "_metric_set", None)
        kw = {}
        if ms is not None:
            records = ms.buffer("eval", self.device).zero_()
            kw = {"metric_slot": "eval"}
        tot = torch.zeros((), dtype=torch.float64, device=self.device)
        for lo in range(0, n, batch_size):
            sl = slice(lo, min(n, lo + batch_size))
            loss = self._loss_encoded(enc, enc.cat_row[sl], enc.an_row[sl], y[sl], False,
                                      None if sw is None else sw[sl], **kw)
            tot.add_(loss, alpha=sl.stop - sl.start)
        if ms is None:
            loss = float(tot) / max(n, 1)
            return {"loss": loss} if return_dict else loss
        host = torch.cat([tot.reshape(1), records.reshape(-1)]).cpu().numpy()
        out = {"loss": float(host[0]) / max(n, 1), **ms.results(host[1:])}
        return out if return_dict else list(out.values())

    # ---- fine-tuning over cached frozen steps (data.FrozenStates; DESIGN.md "Cached frozen steps")
    def _frozen_steps_check(self):
        """ValueError unless a training pass of this model can start each ion's layered encoder behind steps that
        cannot change: what ``cache_frozen_steps=True`` and ``frozen_states`` require.  Raised before the library is
        reached."""
        from . import dist as idist
        pre = self.frozen_prefix()
        why = None
        if pre["cat"] == 0 and pre["an"] == 0:
            why = "nothing below the first trained step is frozen (an embedding or step 0 of both ions trains)"
        elif pre["cat"] is None and pre["an"] is None:
            why = ("the whole encoder is frozen: no step is left to resume" +
                   (" - cache_frozen_encoder=True serves this case" if self.kind == "transfer" else ""))
        elif self.dropout_rate > 0.0:
            why = (f"the encoder's GatedUpdate dropout rate is {self.dropout_rate}: a training pass draws masks on frozen "
                   "steps too, so their atom states differ from step to step")
        elif idist.is_distributed():
            why = "torch.distributed is initialised: data-parallel fits keep no states"
        elif not self._head_kernels_cover():
            why = (f"the training pass is not one of the fused loss nodes: the head kernels do not cover atom_dim "
                   f"{self.atom_dim}, fp_size {self.fp_size}, mixing_size {self.mixing_size}")
        elif self.kind != "transfer" and self._loss_name() != "mse":
            why = (f"the training pass is not one of the fused loss nodes: a {self.kind} model compiled with "
                   f"{self._loss_name()} runs its head layer by layer")
        elif not self._head_nodes_cover():  # (asks the library for the head's size: the last question)
            why = (f"the training pass is not one of the fused loss nodes: the head's backward does not hold atom_dim "
                   f"{self.atom_dim}, fp_size {self.fp_size}, mixing_size {self.mixing_size} in LDS")
        if why is not None:
            raise ValueError(f"cache_frozen_steps: the frozen steps cannot be cached - {why}")

    def frozen_states(self, inputs, batch_size=4096):
        """data.FrozenStates of padded model inputs: every distinct ion once through its frozen steps.  Refused
        (ValueError) where ``fit(cache_frozen_steps=True)`` is."""
        self._frozen_steps_check()
        return data.FrozenStates.build(self, inputs, batch_size)

    def frozen_step_states(self, prefix, ions, steps, batch_size=4096):
        """The atom states (n, N, D) of the distinct ions ``ions`` ({"atom", "bond", "connectivity"}, padded int32
        arrays) after steps 0..steps-1 of the ``prefix`` ion's encoder: the table of data.FrozenStates.  Runs under
        no_grad on the layered kernels a training pass uses below its first trained step (typed message, Reduce,
        GatedUpdate over ALL rows: no kept-row list, so padding rows hold the finite values those kernels compute)."""
        br = self.branches[prefix]
        atom, bond, conn = (torch.from_numpy(a) for a in _ion_numpy(ions, f"{prefix} ions"))
        n, N = int(atom.shape[0]), int(atom.shape[1])
        out = torch.empty((n, N, self.atom_dim), dtype=torch.float32, device=self.device)
        with torch.no_grad():
            for lo in range(0, n, int(batch_size)):
                sl = slice(lo, min(n, lo + int(batch_size)))
                a, b, c = (t[sl].to(self.device).contiguous() for t in (atom, bond, conn))
                graph = ops.IonGraph(a, b, c, self.bond_vocab_size)
                h, bd = self.atom_emb(a), self.bond_emb(b)
                for i in range(steps):
                    m = ops.bmm_message_typed(h, bd.ids, c, br["bmm"][i]._type_matrices(bd.table), graph)
                    h = br["update"][i]([h, br["reduce"][i]([m, c[:, :, 1], h])])
                out[sl] = h
        return out

    def train_on_state_batch(self, states, x, rows, y, sample_weight=None, metric_slot=None):
        """``train_on_batch`` on the samples ``rows`` (device int64) of the device-resident padded inputs ``x``, each
        ion's encoder resumed from ``states`` (data.FrozenStates of ``x``): ``y`` and ``sample_weight`` hold one value
        per sample of the batch."""
        if getattr(self, "optimizer", None) is None:
            self.compile()
        self._frozen_steps_check()
        kw = {} if metric_slot is None else {"metric_slot": metric_slot}
        x = self._to_device(x)
        rows = torch.as_tensor(rows, dtype=torch.int64).to(self.device).reshape(-1)
        loss = self._loss({k: v[rows] for k, v in x.items()}, y, training=True, sample_weight=sample_weight,
                          states=(states, torch.index_select(states.cat_row, 0, rows),
                                  torch.index_select(states.an_row, 0, rows)), **kw)
        loss.backward()
        self.join_training_streams()
        self.optimizer.apply_gradients()
        self.optimizer.zero_grad()
        self.weights_updated()
        return loss.detach()

    def train_on_batch(self, inputs, y, sample_weight=None, group=None, n_global=None, metric_slot=None):
        """One optimizer step on one mini-batch -> the batch loss (MSE + penalties) as a 0-d tensor.
        ``sample_weight``: one finite value >= 0 per sample (of this rank's shard): the loss is keras's
        (1/B) sum_b w_b L_b + penalties, B counting the samples of weight 0 too.
        With torch.distributed initialised (or ``group`` given) every rank calls this with its shard of
        the global mini-batch: the gradients are averaged over ranks (weighted by shard size) with one
        all-reduce of the flat gradient buffer, then every rank applies the same step.  ``n_global``: size of the
        global mini-batch when the caller knows it (fit does) - saves the blocking all-reduce that counts it.
        ``metric_slot``: fit passes "train" for a model compiled with metrics (see _loss)."""
        from . import dist as idist
        if getattr(self, "optimizer", None) is None:
            self.compile()
        opt = self.optimizer
        n_local = len(inputs["cat_atom"])
        if sample_weight is not None and not n_local:
            from . import train
            train.checked_sample_weight(sample_weight, 0)
        kw = {} if metric_slot is None else {"metric_slot": metric_slot}
        loss = self._loss(inputs, y, training=True, sample_weight=sample_weight, **kw) if n_local else None
        if idist.is_distributed():
            if n_global is not None:
                weight = float(n_local) / float(n_global) if n_global > 0 else 0.0
            else:
                weight, _ = idist.shard_loss_weight(n_local, opt.flat_grad.device, group)
            if loss is not None:
                (loss * weight).backward()
            self.join_training_streams()
            idist.all_reduce_flat_gradients_(opt.flat_grad, group)
        elif loss is not None:
            loss.backward()
            self.join_training_streams()
        opt.apply_gradients()   # clips, updates, and leaves the gradients in place ...
        opt.zero_grad()         # ... so clear them for the next accumulation
        self.weights_updated()
        return loss.detach() if loss is not None else torch.zeros((), device=opt.flat_grad.device)

    def evaluate(self, inputs, y, batch_size=32, sample_weight=None, return_dict=False, cache_frozen_encoder=False):
        """model.evaluate: sample-count-weighted mean of the batch losses (MSE + penalties); with ``sample_weight`` a
        batch loss is the weighted one, (1/B) sum_b w_b L_b + penalties.  A model compiled with metrics returns
        ``[loss, *metrics]`` in compile order (``return_dict``: {"loss": ..., "<name>": ...}): every batch's inference
        predictions are added to the device records behind its loss, and the records come back with the loss sum in
        the one synchronisation.  ``cache_frozen_encoder`` (a transfer model with a frozen encoder; ``fit`` names the
        refusals): every distinct ion is encoded once and the batches run the indexed loss; ``inputs`` may then be a
        data.FrozenEncodings made earlier."""
        from . import train
        if cache_frozen_encoder or isinstance(inputs, data.FrozenEncodings):
            self._frozen_cache_check()
            n = len(inputs) if isinstance(inputs, data.FrozenEncodings) else len(inputs["cat_atom"])
            sw = train.checked_sample_weight(sample_weight, n, self.device)
            enc = inputs if isinstance(inputs, data.FrozenEncodings) else data.FrozenEncodings.build(self, inputs)
            y_dev = torch.as_tensor(np.asarray(y, np.float32) if not torch.is_tensor(y) else y).to(self.device)
            if y_dev.numel() != n:
                raise ValueError(f"y holds {y_dev.numel()} values for {n} samples")
            return self._evaluate_encoded(enc, y_dev.reshape(-1, 1), int(batch_size), sw, return_dict)
        n = len(inputs["cat_atom"])
        sw = train.checked_sample_weight(sample_weight, n, self.device)
        ms = getattr(self, "_metric_set", None)
        kw = {}
        if ms is not None:
            records = ms.buffer("eval", self.device).zero_()
            kw = {"metric_slot": "eval"}
        tot = torch.zeros((), dtype=torch.float64, device=self.device)
        for lo in range(0, n, batch_size):
            sl = slice(lo, min(n, lo + batch_size))
            loss = self._loss({k: v[sl] for k, v in inputs.items()}, y[sl], training=False,
                              sample_weight=None if sw is None else sw[sl], **kw)
            tot.add_(loss, alpha=sl.stop - sl.start)  # summed on the device: one host sync per evaluate()
        if ms is None:
            loss = float(tot) / max(n, 1)
            return {"loss": loss} if return_dict else loss
        host = torch.cat([tot.reshape(1), records.reshape(-1)]).cpu().numpy()
        out = {"loss": float(host[0]) / max(n, 1), **ms.results(host[1:])}
        return out if return_dict else list(out.values())

    def fit(self, x, y, validation_data=None, epochs=1, batch_size=32, callbacks=None, shuffle=True, verbose=0,
            seed=None, graph=True, sample_weight=None, cache_frozen_encoder=False, cache_frozen_steps=False):
        """model.fit as the trainers call it (train_viscosity.py:328-338): per epoch a fresh shuffle,
        mini-batches of ``batch_size``, `loss` = sample-weighted mean of the batch losses, `val_loss` from
        evaluate(); callbacks see on_train_begin / on_epoch_begin / on_epoch_end / on_train_end.  Returns a History.
        ``graph=True`` (single process): full-size mini-batches replay one captured hipGraph of the whole step
        (train.GraphedTrainStep); the last, smaller batch of an epoch runs eagerly.
        Under torch.distributed every rank passes the FULL (x, y): the shuffle seed is rank 0's (broadcast once), every
        global mini-batch is cut into contiguous shards (data.shard_bounds), so all ranks run the same number of steps
        with the same sample order, and the reported loss is the global sample-weighted mean.
        ``sample_weight``: one finite value >= 0 per training sample (data.balanced_weights, data.bootstrap_weights):
        every batch loss becomes (1/B) sum_b w_b L_b + penalties, B counting the samples of weight 0 too; the weights
        are uploaded once and cut like y.  ``validation_data`` may be ``(x, y)`` or ``(x, y, sample_weight)``.
        A model compiled with metrics logs them too: the training ones are keras's running metrics, added up on the
        device from every step's training-pass predictions (inside the captured step) and read with the loss at the
        end of the epoch; the validation ones come from evaluate() as ``val_<name>``.
        ``cache_frozen_encoder=True`` (stage 1 of transfer learning): every distinct ion of ``x`` and of the validation
        set is encoded once, before the first epoch (data.FrozenEncodings), and every step - the captured one and the
        eager last batch - and the validation run the head's loss over indexed rows: no encoder launch, no batch
        gather.  A ValueError names the reason where that is not possible: not a transfer model, a trainable encoder
        layer, GatedUpdate dropout above 0, widths the head kernels do not cover, torch.distributed.
        ``cache_frozen_steps=True`` (stage 2, or any fine-tuning with the lower steps frozen): every distinct ion of
        ``x`` runs once through the steps below its first trained one (data.FrozenStates), before the first epoch and
        again at the start of an epoch that finds the states stale; every training step - the captured one and the
        eager last batch - gathers the batch's rows with one impnn_state_rows launch and resumes the layered pass
        there.  Validation is unchanged (inference runs the fused encoder).  A ValueError names the reason where that
        is not possible: nothing frozen below the first trained step, the whole encoder frozen, GatedUpdate dropout
        above 0, torch.distributed, a training pass that is not one of the fused loss nodes, both cache flags."""
        from . import train
        if getattr(self, "optimizer", None) is None:
            self.compile()
        if cache_frozen_steps and cache_frozen_encoder:
            raise ValueError("cache_frozen_steps: given together with cache_frozen_encoder - a model has either a "
                             "frozen encoder (cache_frozen_encoder) or frozen lower steps (cache_frozen_steps)")
        if cache_frozen_steps:
            self._frozen_steps_check()
        if cache_frozen_encoder:
            self._frozen_cache_check()
        y = np.asarray(y, dtype=np.float32)
        n = len(y)
        w_host = train.checked_sample_weight(sample_weight, n)  # raises before anything reaches the device
        if validation_data is not None and len(validation_data) not in (2, 3):
            raise ValueError("validation_data must be (x, y) or (x, y, sample_weight)")
        val_w_host = None
        if validation_data is not None and len(validation_data) == 3:
            val_w_host = train.checked_sample_weight(validation_data[2], len(np.asarray(validation_data[1])))
        x = self._to_device(x)
        if n:  # once per data set (one device sync), not per batch: raise where tf-CPU's gather / scatter_nd would
            for pfx in ("cat", "an"):
                ops.validate_indices(conn=x[f"{pfx}_connectivity"], atom_ids=x[f"{pfx}_atom"], bond_ids=x[f"{pfx}_bond"],
                                     N=x[f"{pfx}_atom"].shape[1], Va=self.atom_vocab_size, Vb=self.bond_vocab_size)
        from . import dist as idist
        distributed = idist.is_distributed()
        if distributed:  # one shared permutation stream: rank 0's seed (drawn if none was given)
            import torch.distributed as tdist
            sd = torch.tensor([int(seed) if seed is not None else int(np.random.SeedSequence().entropy % (1 << 62))],
                              dtype=torch.int64, device=self.device if tdist.get_backend() == "nccl" else "cpu")
            tdist.broadcast(sd, src=0)
            seed = int(sd.item())
            rank, world = tdist.get_rank(), tdist.get_world_size()
        rng = np.random.default_rng(seed)
        hist = train.History()
        callbacks = list(callbacks or [])
        self.stop_training = False
        for cb in callbacks:
            if hasattr(cb, "set_model"):
                cb.set_model(self)
            if hasattr(cb, "on_train_begin"):
                cb.on_train_begin({})
        graphed = None
        use_graph = bool(graph) and not distributed and n >= batch_size
        y_dev = torch.from_numpy(y).to(self.device).reshape(-1, 1)
        w_dev = None if w_host is None else w_host.to(self.device)  # uploaded once, like y_dev
        val_dev = None
        ms = getattr(self, "_metric_set", None)
        mkw = {} if ms is None else {"metric_slot": "train"}
        enc = val_enc = None
        if cache_frozen_encoder and n:  # both sets' ions once, before the first epoch
            enc = data.FrozenEncodings.build(self, x)
            if validation_data is not None and len(validation_data[0]["cat_atom"]):
                val_enc = data.FrozenEncodings.build(self, validation_data[0])
        st = None
        if cache_frozen_steps and n:  # every distinct ion through its frozen steps once, before the first epoch
            x = {k: v.contiguous() for k, v in x.items()}
            st = data.FrozenStates.build(self, x)
        for epoch in range(int(epochs)):
            for cb in callbacks:
                if hasattr(cb, "on_epoch_begin"):
                    cb.on_epoch_begin(epoch, {})
            if st is not None and st.stale(self):  # (a callback loaded weights: the states again, capture again)
                st, graphed = data.FrozenStates.build(self, x), None
            if enc is not None and enc.stale(self):  # (a callback loaded weights: encode again, capture again)
                enc, graphed = data.FrozenEncodings.build(self, x), None
                val_enc = None if val_enc is None else data.FrozenEncodings.build(self, validation_data[0])
            order = rng.permutation(n) if shuffle else np.arange(n)
            order_dev = torch.from_numpy(order).to(self.device)  # one upload per epoch
            tot = torch.zeros((), dtype=torch.float64, device=self.device)
            if ms is not None:  # the epoch's running records: zeroed on the stream, outside any graph
                records = ms.buffer("train", self.device).zero_()
            for lo in range(0, n, batch_size):
                idx = order[lo:lo + batch_size]
                tidx = order_dev[lo:lo + batch_size]
                if enc is not None:
                    if use_graph and len(idx) == batch_size:
                        if graphed is None:
                            graphed = train.GraphedTrainStep(
                                self, tidx, y[idx], resident=(enc, y_dev) if w_dev is None else (enc, y_dev, w_dev),
                                sample_weight=None if w_dev is None else w_dev[tidx])
                        loss = graphed.step_on_rows(enc, y_dev, tidx, w_dev)
                    else:
                        loss = self.train_on_encoded_batch(enc, tidx, y_dev[tidx],
                                                           None if w_dev is None else w_dev[tidx], **mkw)
                elif use_graph and len(idx) == batch_size:
                    if graphed is None:
                        x = {k: v.contiguous() for k, v in x.items()}
                        skw = {} if st is None else {"states": st}
                        if w_dev is None:
                            graphed = train.GraphedTrainStep(self, {k: v[tidx] for k, v in x.items()}, y[idx],
                                                             resident=(x, y_dev), **skw)
                        else:
                            graphed = train.GraphedTrainStep(self, {k: v[tidx] for k, v in x.items()}, y[idx],
                                                             resident=(x, y_dev, w_dev), sample_weight=w_dev[tidx], **skw)
                    loss = graphed.step_on_rows(x, y_dev, tidx, w_dev)
                elif st is not None:
                    loss = self.train_on_state_batch(st, x, tidx, y_dev[tidx], None if w_dev is None else w_dev[tidx],
                                                     **mkw)
                elif distributed:
                    from .data import shard_bounds
                    s0, s1 = shard_bounds(len(idx), world, rank)
                    sidx = tidx[s0:s1]
                    loss = self.train_on_batch({k: v[sidx] for k, v in x.items()}, y_dev[sidx],
                                               None if w_dev is None else w_dev[sidx], n_global=len(idx), **mkw)
                    tot.add_(loss, alpha=s1 - s0)  # shard means, weighted by shard size; summed over ranks below
                    continue
                else:
                    loss = self.train_on_batch({k: v[tidx] for k, v in x.items()}, y_dev[tidx],
                                               None if w_dev is None else w_dev[tidx], **mkw)
                tot.add_(loss, alpha=len(idx))
            if distributed:  # every rank summed its shards' losses: one all-reduce per epoch for the logged mean
                if tdist.get_backend() == "nccl":
                    tdist.all_reduce(tot)
                else:
                    t_cpu = tot.cpu()
                    tdist.all_reduce(t_cpu)
                    tot = t_cpu.to(self.device)
                if ms is not None:
                    idist.all_reduce_metric_sums_(records)
            if ms is None:
                logs = {"loss": float(tot) / max(n, 1)}
            else:  # the records come back with the loss sum: still one synchronisation per epoch
                host = torch.cat([tot.reshape(1), records.reshape(-1)]).cpu().numpy()
                logs = {"loss": float(host[0]) / max(n, 1), **ms.results(host[1:])}
            if validation_data is not None:
                if val_dev is None:  # uploaded once, not per epoch
                    val_dev = (self._to_device(validation_data[0]),
                               torch.from_numpy(np.asarray(validation_data[1], np.float32)).to(self.device),
                               None if val_w_host is None else val_w_host.to(self.device))
                # the sample-weighted mean does not depend on how the set is cut: large forward-only batches
                val_x = val_dev[0] if val_enc is None else val_enc
                if ms is None:
                    logs["val_loss"] = self.evaluate(val_x, val_dev[1], max(batch_size, 4096), val_dev[2])
                else:
                    val = self.evaluate(val_x, val_dev[1], max(batch_size, 4096), val_dev[2], return_dict=True)
                    logs.update({"val_" + k: v for k, v in val.items()})
            hist._log(epoch, logs)
            if verbose:
                print(f"Epoch {epoch + 1}/{epochs} - " + " - ".join(f"{k}: {v:.4f}" for k, v in logs.items()), flush=True)
            for cb in callbacks:
                if hasattr(cb, "on_epoch_end"):
                    cb.on_epoch_end(epoch, logs)
            if self.stop_training:
                break
        for cb in callbacks:
            if hasattr(cb, "on_train_end"):
                cb.on_train_end({})
        self.history = hist
        return hist

    def error_table(self, x, y, groups, sample_weight=None, batch_size=4096, scale=1.0, offset=0.0):
        """Per-group errors of the model on (x, y) -> data.ErrorTable(group, count, weight, bias, mae, rmse,
        max_error), one row per distinct id of ``groups`` (an ion pair's ``pair_id``) in np.unique order;
        ``.worst(k, by="mae")`` names the groups the model gets worst.  The predictions of all batches stay in one
        device buffer, one segmented launch reduces them (data.error_table_on_device), and only the (G, 8) records reach
        the host.  ``scale`` / ``offset`` report in the target's unit.  data.error_table is the host reference."""
        from . import train
        n = len(x["cat_atom"])
        y_dev = torch.as_tensor(np.asarray(y, np.float32).reshape(-1)).to(self.device)
        if y_dev.numel() != n:
            raise ValueError(f"y holds {y_dev.numel()} values for {n} samples")
        sw = train.checked_sample_weight(sample_weight, n, self.device)
        pred = torch.empty(n, dtype=torch.float32, device=self.device)
        for lo in range(0, n, int(batch_size)):
            hi = min(n, lo + int(batch_size))
            pred[lo:hi] = self({k: v[lo:hi] for k, v in x.items()}).reshape(-1)
        return data.error_table_on_device(pred, y_dev, groups, sw, scale, offset)

    def predict(self, inputs, batch_size=None, fused=None):
        """model.predict(x) (train_viscosity.py:366): returns a numpy (n,1) array.  The reference's
        Keras default batch is 32; here the whole set is one batch unless batch_size is given."""
        n = len(inputs["cat_atom"])
        bs = n if not batch_size else int(batch_size)
        if n == 0:
            return np.zeros((0, 1), np.float32)
        if n <= bs:
            return self(inputs, fused=fused).detach().cpu().numpy()
        # several chunks: consecutive chunks on two HIP streams (their kernels overlap, see bench.py --streams), one
        # host synchronisation at the end instead of one per chunk
        cur = torch.cuda.current_stream(self.device)
        lanes = getattr(self, "_predict_lanes", None)
        if lanes is None:
            lanes = self._predict_lanes = [torch.cuda.Stream(device=self.device) for _ in range(2)]
        for ln in lanes:
            ln.wait_stream(cur)
        outs = []
        for i, lo in enumerate(range(0, n, bs)):
            chunk = {k: v[lo:lo + bs] for k, v in inputs.items()}
            with torch.cuda.stream(lanes[i % 2]):
                outs.append(self(chunk, fused=fused).detach())
        for ln in lanes:
            cur.wait_stream(ln)
        for o in outs:
            o.record_stream(cur)
        return torch.cat(outs, dim=0).cpu().numpy()

    # ------------------------------------------------------------------ screening: one encoder row per ion species
    def encode_ions(self, cations=None, anions=None, batch_size=4096):
        """GlobalSumPool rows of ion species on their own: ``cations`` / ``anions`` are dicts {"atom" (M,N), "bond"
        (M,E), "connectivity" (M,E,2)} of numpy arrays or torch tensors, or None -> (pooled_cat (C,D) | None,
        pooled_an (A,D) | None) on the model's device.  Goes through ``encode_pooled`` on the pair batches of
        ``ion_pair_batches`` (so: the resolved encoder mode, prepared weights, the overflow fallback, the wide and
        layered paths), ``batch_size`` rows at a time; the padding rows are dropped.  Inference only: no graph, no
        dropout."""
        batches, C, A = ion_pair_batches(cations, anions, batch_size)
        parts = []
        with torch.no_grad():
            for b in batches:
                inp = {k: torch.from_numpy(v).to(self.device, non_blocking=True) for k, v in b.items()}
                parts.append(self.encode_pooled(inp))
        out = []
        for g, (given, n) in enumerate(((cations, C), (anions, A))):
            if given is None:
                out.append(None)
            elif not parts:
                out.append(torch.zeros(0, self.atom_dim, dtype=torch.float32, device=self.device))
            else:
                out.append(torch.cat([p[g] for p in parts], dim=0)[:n].contiguous())
        return out[0], out[1]

    def _head_kernels_cover(self):
        """The head kernels (model head, transfer head and their grids) cover the model's widths."""
        return self.atom_dim <= ops.HEAD_MAX_X and max(self.fp_size, self.mixing_size) <= ops.HEAD_MAX_DIM

    def _head_nodes_cover(self):
        """The one rule of a training pass: it takes the fused head nodes (autograd.ModelHead, ModelHeadLoss,
        TransferHeadLoss) where the widths are covered AND the model head's backward holds the weights in LDS
        (ops.model_head_bwd_fits); otherwise the head runs layer by layer.  Inference and the grids need the widths alone."""
        if not self._head_kernels_cover():
            return False
        return self.kind == "transfer" or ops.model_head_bwd_fits(ops.HEAD_KINDS[self.kind], self.atom_dim, self.fp_size,
                                                                  self.mixing_size)

    def _grid_kernels_cover(self):
        return self.kind != "transfer" and self._head_kernels_cover()

    def _transfer_grid_covers(self):
        """The matrix-core grid of the transfer head (impnn_transfer_ion_half / impnn_transfer_head_grid) covers it."""
        return self.kind == "transfer" and self._head_kernels_cover()

    def predict_grid(self, cations, anions, temperatures=None, return_params=False, max_pairs_per_launch=None,
                     batch_size=4096):
        """Every cation x anion pair (x temperature) of a screen from C + A encoder rows: ``encode_ions``, the
        per-ion half of the head once per species (impnn_head_ion_mix), then one impnn_head_grid launch over the
        product.  Viscosity: ``temperatures`` (nT) in kelvin -> numpy (C,A,nT), with ``return_params`` also the VFT
        parameters (C,A,3) = (A, B, C) of every pair; melting point and transfer: numpy (C,A).  For the viscosity and
        melting-point models, and for the transfer model with ``grid_head_mode = "gathered"``, element [i,j,t] has the
        bits ``predict`` gives for the pair (cation i, anion j, T[t]) from the same pooled rows.  The transfer model in
        "auto" runs its head on the matrix cores from one ``impnn_transfer_ion_half`` row per species
        (impnn_transfer_head_grid): the order of the sums and the factored first layer differ from ``predict``'s
        kernel, the values agree within the project's 1e-5 bound, and an element's bits do not depend on the grid's
        size or the host tiling.
        ``max_pairs_per_launch`` tiles the cation axis on the host; the default keeps one launch's output within
        GRID_OUTPUT_BUDGET elements (1 GiB of float32); ``batch_size``: rows per encoder launch.  Widths the head kernels do not cover (fp_size or mixing_size
        above 64) and the transfer model in "gathered" mode evaluate ``self.head`` on gathered tiles of pairs instead."""
        if return_params and self.kind != "viscosity":
            raise ValueError(f"return_params: the {self.kind} model has no VFT parameters")
        T = self._screen_request("predict_grid", cations, anions, temperatures, None, max_pairs_per_launch)
        return _Screen(self, cations, anions, T, None, batch_size).values(max_pairs_per_launch, return_params)

    def screen_mask(self, cations, anions, temperatures=None, at_least=None, at_most=None, max_pairs_per_launch=None,
                    batch_size=4096):
        """A screen's constraint as a packed pair mask, written on the GPU: bit (i, j[, t]) is set where
        ``at_least <= prediction <= at_most`` for the value ``predict_grid`` gives that element -> ``data.PairMask`` of
        shape (C,A), viscosity (C,A,nT), its words on the model's device.  At least one bound is needed; a missing one is
        -inf / +inf; bounds are compared as float32, a NaN prediction fails.  ``encode_ions``, the per-ion halves and
        the host tiling of the cation axis are ``predict_grid``'s; the mask-writing kernels (impnn_head_grid_mask,
        impnn_transfer_head_grid_mask; the transfer model in "auto" on the matrix cores) evaluate every pair with the
        grid kernels' arithmetic, and no C x A float buffer exists.  Widths the head kernels do not cover and the
        transfer model with ``grid_head_mode = "gathered"`` evaluate ``predict_grid``'s tiles, compare and pack
        instead; more temperatures than one launch takes are split.  The result is the same.
        Masks compose (``&``, ``|``, ``~``) and constrain ``screen_top_k``: "of the pairs the melting-point model puts
        below a limit and nobody has made yet, the 100 least viscous at 298 K" is

            liquid = mp_model.screen_mask(cat, an, at_most=limit_scaled)
            known  = data.PairMask.from_bool(already_made, device=liquid.words.device)
            best   = visc_model.screen_top_k(cat, an, [298.15], k=100, where=liquid & ~known)

        (the melting-point model predicts the standardised target: convert a kelvin limit with the training set's
        ``y_mean`` / ``y_std`` first)."""
        lo_b, hi_b = screening.mask_bounds("screen_mask", at_least, at_most)
        T = self._screen_request("screen_mask", cations, anions, temperatures, None, max_pairs_per_launch)
        return _Screen(self, cations, anions, T, None, batch_size).pair_mask(lo_b, hi_b, max_pairs_per_launch)

    def _screen_request(self, what, cations, anions, temperatures, where, max_pairs_per_launch):
        """``screening._screen_request`` for this model's kind."""
        return screening._screen_request(self.kind, what, cations, anions, temperatures, where, max_pairs_per_launch)

    def screen_top_k(self, cations, anions, temperatures=None, k=100, largest=False, max_pairs_per_launch=None,
                     batch_size=4096, where=None):
        """The k pairs of a screen with the smallest (``largest``: largest) prediction, selected on the GPU: what
        ``data.grid_top_k(self.predict_grid(...), k, largest)`` returns, without the grid.  ``encode_ions`` and the
        per-ion halves are ``predict_grid``'s; the selecting kernels (impnn_head_grid_topk,
        impnn_transfer_head_grid_topk) evaluate every pair with the grid kernels' arithmetic and keep a running top k
        on the chip.  -> ``data.TopK`` of numpy ``values`` float32, ``cation``, ``anion`` int64 (positions in the lists
        given), sorted, of shape (nT, min(k, C*A)) for viscosity - a row per temperature - and (min(k, C*A),)
        otherwise.  Order: by value, ties by cation then anion index, NaN last.
        The cation axis is tiled on the host so that a launch has fewer than 2^32 pairs (``max_pairs_per_launch``
        overrides it), temperatures are split at ops.SELECT_MAX_T per launch, and the launches' results are merged
        under the same order.  Widths the head kernels do not cover, the transfer model with ``grid_head_mode =
        "gathered"`` and k above SCREEN_MAX_K walk ``predict_grid``'s tiles instead and select per tile: never more than
        one tile and k entries are held.
        ``where``: a 2-D ``data.PairMask`` of shape (C,A) (``screen_mask``, ``PairMask.from_bool``, and their ``&``,
        ``|``, ``~``); only its pairs compete, in every temperature row (for one plane of a viscosity mask take
        ``temperature(t)`` and call per row), and a row has min(k, where.count()) entries.  The selecting kernels read
        the mask (impnn_head_grid_topk_where, impnn_transfer_head_grid_topk_where) and pass over tiles without a set
        bit; it is tiled with the cation axis and honoured by every fallback too.  See ``screen_mask`` for the
        intended use."""
        T = self._screen_request("screen_top_k", cations, anions, temperatures, where, max_pairs_per_launch)
        k = screening.at_least_one("k", k)
        return _Screen(self, cations, anions, T, where, batch_size).top_k(k, largest, max_pairs_per_launch)

    def mc_dropout(self, samples=32, draw=0):
        """Monte-Carlo dropout of the transfer head as a screening model -> ``mc_dropout.McDropout``: ``samples``
        stochastic passes with ``mp_dropout`` on (the masks of dropout step ``draw``, the same for every pair) and
        BatchNormalization on its moving statistics, and ``predict_grid`` / ``screen_mask`` / ``screen_top_k`` /
        ``predict_pairs`` on their mean, spread and mean + kappa * std (impnn_transfer_mc_grid*).  Only the transfer
        model has a head Dropout: any other kind, and widths the transfer grid does not cover, raise a ValueError."""
        from .mc_dropout import McDropout
        return McDropout(self, samples, draw)

    def screen_best_partners(self, cations, anions, temperatures=None, m=1, largest=False, where=None,
                             max_pairs_per_launch=None, batch_size=4096):
        """For every cation of a screen its ``m`` best anions, and for every anion its ``m`` best cations, selected on
        the GPU: what ``data.grid_best_partners(self.predict_grid(...), m, largest, where)`` returns, without the grid.
        ``encode_ions``, the per-ion halves, the argument rules and the host tiling are ``screen_top_k``'s; the
        partner-selecting kernels (impnn_head_grid_partners, impnn_transfer_head_grid_partners) evaluate every pair
        with the grid kernels' arithmetic and answer both axes from one launch.  -> ``data.BestPartners(by_cation,
        by_anion)`` of ``data.Partners(values, partner)``, numpy float32 / int64 (positions in the lists given):
        (nT,C,m) and (nT,A,m) for viscosity - a plane per temperature - and (C,m), (A,m) otherwise.  An ion's partners
        are in order: by value, ties by the partner's index, NaN last; slots past the number of its competing partners
        hold NaN / -1.
        The cation axis is tiled on the host (``max_pairs_per_launch`` overrides the default, which bounds a launch's
        workspace): per-cation results are concatenated, per-anion results merged under the same order; temperatures
        are split at ops.SELECT_MAX_T per launch.  Widths the head kernels do not cover, the transfer model with
        ``grid_head_mode = "gathered"`` and m above ops.PARTNERS_MAX_M walk ``predict_grid``'s tiles instead and apply
        ``data.grid_best_partners`` per tile.  The result is the same.
        ``where``: a 2-D ``data.PairMask`` of shape (C,A), as in ``screen_top_k``; only its pairs compete."""
        T = self._screen_request("screen_best_partners", cations, anions, temperatures, where, max_pairs_per_launch)
        m = screening.at_least_one("m", m)
        return _Screen(self, cations, anions, T, where, batch_size).best_partners(m, largest, max_pairs_per_launch)

    def screen_ion_summary(self, cations, anions, temperatures=None, where=None, max_pairs_per_launch=None,
                           batch_size=4096):
        """The main-effects view of a screen, reduced on the GPU: for every cation over its anions, for every anion over
        its cations and for the whole plane, how many pairs compete and the mean, the population standard deviation,
        the least and the greatest prediction - what ``data.grid_ion_summary(self.predict_grid(...), where,
        ops.SUMMARY_BLOCKS[family])`` returns, bit for bit, without the grid.  "What does this cation do on average over
        the anions that may compete, how much does that depend on the partner, and what are its best and worst cases?"
        ``encode_ions``, the per-ion halves and the argument rules are ``screen_best_partners``'s; the summary kernels
        (impnn_head_grid_summary, impnn_transfer_head_grid_summary) evaluate every pair with the grid kernels'
        arithmetic and reduce both axes in one launch, in double, in one stated order (``data.grid_ion_records``).
        -> ``data.IonSummary(by_cation, by_anion, overall)`` of ``data.IonStats(count, mean, std, min, max)``: numpy
        int64 / float32 of shape (nT,C), (nT,A), (nT,) for viscosity - a row per temperature - and (C,), (A,), scalars
        otherwise; ``IonStats.order`` ranks the ions.  A pair competes when its ``where`` bit is set and its prediction
        is not NaN; an ion without a competing pair has count 0 and NaN statistics.
        The cation axis is tiled on the host at multiples of 16 only (``max_pairs_per_launch`` is rounded down to that,
        the least range is 16 cations; the default bounds a launch's workspace) and the anion records are carried from
        one range's launch into the next: the result's bits do not depend on the tiling.  Widths the head kernels do not
        cover and the transfer model with ``grid_head_mode = "gathered"`` apply ``data.grid_ion_records`` to
        ``predict_grid``'s tiles with the same blocks and the same carried records.
        ``where``: a 2-D ``data.PairMask`` of shape (C,A), as in ``screen_top_k``; only its pairs compete."""
        T = self._screen_request("screen_ion_summary", cations, anions, temperatures, where, max_pairs_per_launch)
        return _Screen(self, cations, anions, T, where, batch_size).ion_summary(max_pairs_per_launch)

    def screen_rank(self, cations, anions, temperatures=None, k=100, largest=False, where=None, batch_size=4096):
        """The rank cut of a screen: the ``k``-th pair (1-based) with the smallest (``largest``: largest) prediction,
        found on the GPU - what ``data.grid_rank(self.predict_grid(...), k, largest, where)`` returns, without the grid,
        for any k: "the value below which the best 1 % of the pairs lie".  ``encode_ions``, the per-ion halves and the
        argument rules are ``screen_top_k``'s; the rank-cut kernels (impnn_head_grid_rank,
        impnn_transfer_head_grid_rank) evaluate the grid once per 8-bit digit of the selection's 64-bit entry
        (``ops.rank_passes``) and keep only a histogram.  -> ``data.RankCut`` of numpy ``values`` float32, ``cation``,
        ``anion`` int64 (positions in the lists given) and ``count`` int64, the number of competing pairs: arrays (nT,)
        for viscosity, scalars otherwise.  Order: by value, ties by cation then anion index, NaN last; more than
        ``count`` asked for gives NaN / -1 / -1.  Temperatures are split at ops.SELECT_MAX_T per launch; the cation axis
        is not tiled: more than 2^32 - 2 pairs raise ValueError.  ``where``: a 2-D ``data.PairMask`` of shape (C,A), as
        in ``screen_top_k``; only its pairs compete.
        Widths the head kernels do not cover and the transfer model with ``grid_head_mode = "gathered"`` apply
        ``data.grid_rank`` to ``predict_grid``: that path holds the grid."""
        T, k = screening._rank_request(self.kind, "screen_rank", cations, anions, temperatures, k, where)
        cut, _ = _Screen(self, cations, anions, T, where, batch_size).rank(k, largest, False)
        return cut if self.kind == "viscosity" else data.RankCut(*[x[0] for x in cut])

    def screen_best_mask(self, cations, anions, temperatures=None, k=100, largest=False, where=None, batch_size=4096):
        """The ``k`` best pairs of a screen as a set to go on working with: a ``data.PairMask`` whose set bits are exactly
        the first min(k, competing) pairs under ``screen_top_k``'s order - ``PairMask.from_bool(data.grid_best_mask(
        self.predict_grid(...), k, largest, where))`` without the grid, for any k - of shape (C,A,nT) for viscosity, a
        plane per temperature, and (C,A) otherwise, its words on the model's device.  A run of equal predictions that
        straddles k is cut by index: a plane never holds more than k bits.  The rank cut of ``screen_rank`` gives the
        k-th entry, then one more launch over the grid sets every pair at or before it (impnn_head_grid_rank,
        impnn_transfer_head_grid_rank with mask words).  ``where`` and the limits as in ``screen_rank``.  "The best 1 %
        of the pairs that are liquid, then each cation's three best anions among them":

            liquid = mp_model.screen_mask(cat, an, at_most=limit_scaled)
            top1pc = visc_model.screen_best_mask(cat, an, [298.15], k=liquid.count() // 100, where=liquid).temperature(0)
            per_cation = visc_model.screen_best_partners(cat, an, [298.15], m=3, where=top1pc)

        Widths the head kernels do not cover and the transfer model with ``grid_head_mode = "gathered"`` apply
        ``data.grid_best_mask`` to ``predict_grid``: that path holds the grid."""
        T, k = screening._rank_request(self.kind, "screen_best_mask", cations, anions, temperatures, k, where)
        _, words = _Screen(self, cations, anions, T, where, batch_size).rank(k, largest, True)
        C, A = int(words.shape[1]), len(anions["atom"])
        if self.kind == "viscosity":
            return data.PairMask(words, (C, A, int(words.shape[0])))
        return data.PairMask(words[0], (C, A))

    # ------------------------------------------------------------------ the applicability domain of a screen
    def _domain_mix(self, cations, anions, batch_size):
        """The per-ion halves of the latent space: ``encode_ions`` and ``ops.head_ion_mix`` -> (C,Mx), (A,Mx)."""
        return screening._domain_mix(self, cations, anions, batch_size)

    def fit_domain(self, cations, anions, cation_index, anion_index, batch_size=4096):
        """The training pairs as a reference set in the model's latent space -> ``data.DomainReference``.  A pair's
        latent vector is the ``mix_cat_an`` layer, head_ion_mix(cat)[i] + head_ion_mix(an)[j] in float32 - where the
        reference's transfer script cuts the network; for a viscosity model it does not depend on temperature.
        ``cation_index`` / ``anion_index`` list the training pairs as indices into the species dicts
        (``data.unique_ions`` produces that form); repeated pairs are listed once, sorted by (cation, anion)
        (``data.unique_pairs``).  ``self_distance`` is every pair's distance to its nearest other pair
        (``ops.domain_rows(rows, rows, exclude_self=True)``), from which ``DomainReference.radius`` takes a threshold.
        The reference set is a snapshot of the weights at this moment: after further training fit it again - nothing
        checks that it is still current."""
        screening._domain_request(self, "fit_domain")
        ci, ai = data.unique_pairs(cation_index, anion_index, len(cations["atom"]), len(anions["atom"]))
        if len(ci) == 0:
            raise ValueError("fit_domain needs at least one training pair")
        mc, ma = self._domain_mix(cations, anions, batch_size)
        rows = mc[torch.from_numpy(ci.astype(np.int64)).to(self.device)] + ma[torch.from_numpy(ai.astype(np.int64)).to(self.device)]
        self_distance, _ = ops.domain_rows(rows, rows, exclude_self=True)
        return data.DomainReference(rows, ci, ai, self_distance.cpu().numpy())

    def domain_grid(self, cations, anions, reference, max_pairs_per_launch=None, batch_size=4096):
        """Every pair's distance to the reference set in the latent space, and the training pair it lies nearest to
        (impnn_domain_grid) -> numpy (distance (C,A) float32, nearest (C,A) int32): ``nearest[i,j]`` is a row of
        ``reference`` (``reference.cation`` / ``.anion`` name the pair), the lowest among equally near ones; a pair of
        the reference set has distance exactly 0.  What ``data.grid_domain`` computes in float64.  The cation axis is
        tiled on the host as in ``predict_grid``: the two outputs of a pair count against GRID_OUTPUT_BUDGET, and an
        element's bits do not depend on the tiling."""
        return screening.domain_grid(self, cations, anions, reference, max_pairs_per_launch, batch_size)

    def screen_domain_mask(self, cations, anions, reference, at_most=None, at_least=None, max_pairs_per_launch=None,
                           batch_size=4096):
        """The pairs whose distance to the reference set lies within the bounds, as a packed pair mask written on the
        GPU (impnn_domain_grid_mask): bit (i,j) is set where ``at_least <= distance <= at_most`` for the distance
        ``domain_grid`` gives that pair -> ``data.PairMask`` of shape (C,A) for either kind - it takes no temperatures -
        its words on the model's device.  At least one bound is needed; a missing one is -inf / +inf; bounds are
        compared as float32, a NaN distance fails.  No C x A float buffer exists.  It composes with every screen:

            dom    = visc_model.fit_domain(cat, an, train_cation_index, train_anion_index)
            inside = visc_model.screen_domain_mask(cat, an, dom, at_most=dom.radius(0.95))
            best   = visc_model.screen_top_k(cat, an, [298.15], k=100, where=liquid & inside & ~known)"""
        lo_b, hi_b = screening.mask_bounds("screen_domain_mask", at_least, at_most, "at_most, at_least")
        return screening.domain_mask(self, cations, anions, reference, lo_b, hi_b, max_pairs_per_launch, batch_size)

    def screen_diverse(self, cations, anions, reference, k=24, where=None, batch_size=4096):
        """Which ``k`` candidates to make next: a batch of pairs far from the reference set and from each other, by
        farthest-point (k-center greedy) selection in the latent space, on the GPU (impnn_diverse_select) ->
        ``data.DiverseSelection``: ``cation`` / ``anion`` (n,) int64 in the order of the picks, ``distance`` (n,) float32
        - each pick's distance to the training pairs and the earlier picks when it was chosen, non-increasing - and
        ``competing``, the number of candidates.  Every step takes the farthest pair that still competes - the lowest
        (cation, anion) among equal float32 distances - and adds it to the reference set; a pair competes while its
        distance is > 0, so a training pair, a pair that coincides with one, a chosen pair and a NaN never do.  n < k
        when the candidates run out.  ``where``: a ``data.PairMask`` of shape (C,A); only its pairs compete:

            dom   = visc_model.fit_domain(cat, an, train_cation_index, train_anion_index)
            cand  = visc_model.screen_best_mask(cat, an, [298.15], k=liquid.count() // 100, where=liquid & ~known).temperature(0)
            batch = visc_model.screen_diverse(cat, an, dom, k=24, where=cand)

        The C x A float32 state lives in the library's workspace for the call; the picks need C*A < 2^32."""
        return screening.diverse(self, cations, anions, reference, k, where, batch_size)

    def domain_distance(self, inputs, reference, batch_size=None):
        """The distance of listed pairs - a record list in ``predict``'s input format - to the reference set -> numpy
        (distance (n,) float32, nearest (n,) int32): ``encode_pooled``, the two ``ops.head_ion_mix`` halves, their
        float32 sum and ``ops.domain_rows``.  A record of a reference pair gets 0."""
        screening._domain_request(self, "domain_distance", reference)
        n = len(inputs["cat_atom"])
        bs = n if not batch_size else int(batch_size)
        distance, nearest = np.empty(n, np.float32), np.empty(n, np.int32)
        w, fp, mx = self._packed_head(), self.fp_size, self.mixing_size
        for lo in range(0, n, max(bs, 1)):
            chunk = {k: v[lo:lo + bs] for k, v in inputs.items() if k != "temperature"}
            with torch.no_grad():
                pc, pa = self.encode_pooled({k: self._as_device_tensor(k, v) for k, v in chunk.items()})
            z = ops.head_ion_mix(self.kind, "cat", pc, w, fp, mx) + ops.head_ion_mix(self.kind, "an", pa, w, fp, mx)
            d, p = ops.domain_rows(z, reference.rows)
            distance[lo:lo + bs], nearest[lo:lo + bs] = d.cpu().numpy(), p.cpu().numpy()
        return distance, nearest

    def _grid_operands(self, pc, pa, T, mfma):
        """The per-ion halves of the covered grid kernels as the operands of their launches (``ops.GridOperands``):
        ``impnn_transfer_ion_half`` rows and the prepared image on the matrix-core path, else ``impnn_head_ion_mix``
        rows, the packed head and the temperatures ``T`` (device, or None)."""
        fp, mx = self.fp_size, self.mixing_size
        if mfma:
            tensors = self._head_tensors()
            return ops.transfer_grid_operands(ops.transfer_ion_half("cat", pc, tensors, fp, mx),
                                              ops.transfer_ion_half("an", pa, tensors, fp, mx), self._transfer_image())
        w = self._packed_head()
        return ops.head_grid_operands(self.kind, ops.head_ion_mix(self.kind, "cat", pc, w, fp, mx),
                                      ops.head_ion_mix(self.kind, "an", pa, w, fp, mx), T, w, fp, mx)

    def _grid_gathered(self, pc, pa, T):
        """``self.head`` on the explicit pairs of a tile of cations x all anions (x T) -> (c, A[, nT])."""
        c, A, nT = int(pc.shape[0]), int(pa.shape[0]), (int(T.numel()) if T is not None else 1)
        D = pc.shape[1]
        pcg = pc[:, None, None, :].expand(c, A, nT, D).reshape(-1, D).contiguous()
        pag = pa[None, :, None, :].expand(c, A, nT, D).reshape(-1, D).contiguous()
        if T is None:
            return self.head(pcg, pag).reshape(c, A)
        return self.head(pcg, pag, T[None, None, :].expand(c, A, nT).reshape(-1, 1).contiguous()).reshape(c, A, nT)

    def _as_device_tensor(self, name, v):
        if isinstance(v, np.ndarray):
            v = torch.from_numpy(v)
        if not isinstance(v, torch.Tensor):
            raise TypeError(f"input {name!r} must be a numpy array or torch tensor")
        return v.to(self.device, non_blocking=True)

    def _to_device(self, inputs):
        out = {k: self._as_device_tensor(k, v) for k, v in inputs.items()}
        if self.kind == "viscosity" and "temperature" not in out:
            raise KeyError("the viscosity model needs a 'temperature' input (train_viscosity.py:160)")
        return out


def build_model(atom_vocab_size, bond_vocab_size, atom_dim=32, bond_dim=8, fp_size=32, mixing_size=20,
                num_steps=4, device=None, dropout_rate=0.0, dropout_seed=None):
    """train_viscosity.py:139-231 (same positional/keyword signature and defaults; dropout_rate / dropout_seed:
    GatedUpdate's Dropout in training, MPNNModel)."""
    return MPNNModel("viscosity", atom_vocab_size, bond_vocab_size, atom_dim, bond_dim, fp_size, mixing_size,
                     num_steps, fp_l2=1e-4, device=device, dropout_rate=dropout_rate, dropout_seed=dropout_seed)


def build_melting_point_model(atom_vocab_size, bond_vocab_size, atom_dim=32, fp_size=32, mixing_size=20,
                              num_steps=4, device=None, dropout_rate=0.0, dropout_seed=None):
    """train_melting_point.py:137-215: bond embedding width = atom_dim**2 (:146)."""
    return MPNNModel("melting_point", atom_vocab_size, bond_vocab_size, atom_dim, atom_dim * atom_dim, fp_size,
                     mixing_size, num_steps, fp_l2=1e-5, device=device, dropout_rate=dropout_rate,
                     dropout_seed=dropout_seed)


def build_transfer_model(viscosity_model_path, device=None, dropout_seed=None):
    """train_melting_point_transfer.py:73-106: the viscosity model of a file written by ``MPNNModel.save`` cut at
    ``mix_cat_an`` (layers, names and weights kept: cat_bmm_2, gated_update_6, ...), and on it the head Dense 256 relu
    "mp_dense_1", BatchNormalization "mp_bn_1", Dense 128 relu "mp_dense_2", Dropout 0.3 "mp_dropout", Dense 64 relu
    "mp_dense_3", Dense 1 "melting_point".  Inputs: the six graph tensors (a "temperature" key is ignored).
    dropout_seed: the seed of the head's Dropout mask (default: one draw from torch's CPU generator)."""
    cfg, w = MPNNModel.load_weight_file(viscosity_model_path)
    if cfg.get("kind") != "viscosity":
        raise ValueError(f"{viscosity_model_path}: a viscosity model is needed, this file holds kind {cfg.get('kind')!r}")
    L.reset_uids()
    m = MPNNModel("transfer", cfg["atom_vocab_size"], cfg["bond_vocab_size"], cfg["atom_dim"], cfg["bond_dim"],
                  cfg["fp_size"], cfg["mixing_size"], cfg["num_steps"], cfg.get("fp_l2", 1e-4), device=device,
                  dropout_rate=cfg.get("dropout_rate", 0.0), dropout_seed=cfg.get("dropout_seed"),
                  head_dropout_seed=dropout_seed)
    head = {n for lyr in m._transfer_head_layers() for n, _, o in m._owned_tensors() if o is lyr} | set(m._named_state())
    m.load_weights({**{n: t.detach().cpu().numpy() for n, t in m.variables() if n in head}, **w})
    return m


def load_model(path, custom_objects=None, device=None):
    """keras.models.load_model analogue for files written by MPNNModel.save / save_weights
    (train_melting_point_transfer.py:78-93 passes custom_objects: accepted and ignored - the layer classes are
    this package's own)."""
    cfg, w = MPNNModel.load_weight_file(path)
    m = MPNNModel.from_config(cfg, device=device)
    m.load_weights(w)
    return m
