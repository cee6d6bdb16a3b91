"""Stage 1 of transfer learning over cached encodings, on the GPU: (1) the indexed loss entries
(impnn_transfer_head_loss_rows[_bwd]) against the existing entries on the gathered rows, bit for bit; (2) their
gradients against the fp64 head reference at the bounds of tests/test_gpu_head_fuzz.py; (3) fit with
cache_frozen_encoder against the plain fit at the 2e-4 of tests/test_gpu_transfer.py's two training routes, with no
encoder or batch-assemble call once the first epoch has begun; (4) a captured step over encodings against eager indexed
steps, bit for bit; (5) load_weights and a stage-2 compile invalidate."""
import itertools

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, data, layers as L, ops, synthetic, train
from conftest import assert_close

import test_gpu_head_fuzz as FZ
import test_gpu_transfer as TT
import transfer_ref as R
from test_gpu_train import close

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, STEP = 0x5EED_0BAD_CAFE, 9
BATCHES = [1, 7, 8, 9, 33]                                 # around the 8-sample tile, and more than one workgroup
WIDTHS = [(32, 32, 20), (32, 64, 64), (128, 32, 20), (128, 64, 64)]   # D in {32, 128} x (F, Mx) in {(32,20), (64,64)}


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def head_tensors(rng, D, F, Mx):
    out = []
    for t, s in enumerate(FZ.transfer_shapes(D, F, Mx)):
        if len(s) == 2:
            out.append(_dev(rng.normal(0.0, 1.5 / np.sqrt(s[0]), s)))
        else:
            out.append(_dev(rng.uniform(0.5, 1.5, s) if t == 10 else rng.normal(0.0, 0.2, s)))
    return out


def run_pass(cat, an, rows, weights, cfg0, stats, y, sw, trainable_base, dloss):
    """One forward and backward through ops.transfer_head_loss_rows[_bwd] from fresh statistics -> everything the
    pass writes.  ``rows`` None: the existing weighted entries on the samples' own rows."""
    mm, mv = stats[0].clone(), stats[1].clone()
    cfg = dict(cfg0, moving_mean=mm, moving_variance=mv)
    ws = torch.zeros(int(_lib.load().impnn_transfer_head_loss_workspace_floats(len(y))), dtype=torch.float32, device=DEV)
    cr, ar = rows if rows is not None else (None, None)
    loss, pred, saved = ops.transfer_head_loss_rows(cat, an, cr, ar, weights, cfg, y, ws, sw)
    assert int(ws[:1].view(torch.int32).item()) == 0, "the arrival counter is back at zero"
    grads = [torch.zeros_like(w) if (t >= 8 or trainable_base) else None for t, w in enumerate(weights)]
    ops.transfer_head_loss_rows_bwd(cat, an, cr, ar, weights, grads, cfg, y, dloss, saved, sw)
    return dict(loss=loss, pred=pred, saved=saved, mm=mm, mv=mv, grads=grads)


@pytest.mark.parametrize("D,F,Mx", WIDTHS)
@pytest.mark.parametrize("B", BATCHES)
def test_indexed_entries_equal_the_existing_entries_bit_for_bit(B, D, F, Mx):
    rng = np.random.default_rng([B, D, F, Mx])
    weights = head_tensors(rng, D, F, Mx)
    stats = _dev(rng.uniform(0.0, 0.8, 256)), _dev(rng.uniform(0.5, 2.0, 256))
    y = _dev(rng.normal(0.0, 1.5, B))
    weight = _dev(np.where(np.arange(B) % 4 == 3, 0.0, rng.uniform(0.25, 3.0, B)))
    dloss = _dev([0.37])
    step = torch.tensor([STEP], dtype=torch.int64, device=DEV)
    lw = ops.dropout_layer_word(L.Dropout.LAYER_ID)
    l2 = [float(v) for v in FZ.KERAS_L2]
    tables = {}
    for name, (Cn, An) in (("one row", (1, 1)), ("more rows than samples", (B + 3, B + 5))):
        cat, an = _dev(rng.normal(0.0, 1.0, (Cn, D))), _dev(rng.normal(0.0, 1.0, (An, D)))
        cr, ar = _dev(rng.integers(0, Cn, B), torch.int32), _dev(rng.integers(0, An, B), torch.int32)
        if Cn > 1 and B > 1:
            cr[0], cr[-1], ar[0] = Cn - 1, 0, An - 1   # the tables' last and first rows are read
        tables[name] = (cat, an, cr, ar)
    seen = set()
    for (name, (cat, an, cr, ar)), bn, rate, loss, weighted, base in itertools.product(
            tables.items(), (True, False), (0.0, 0.3), (("mse", 1.0), ("huber", 1.0)), (False, True), (False, True)):
        cfg = {"fp_size": F, "mixing_size": Mx, "l2": l2, "momentum": R.BN_MOMENTUM, "epsilon": R.BN_EPS, "bn_batch": bn,
               "dropout": ops.Dropout(rate, SEED, lw, step) if rate else None,
               "loss_kind": 0 if loss[0] == "mse" else 1, "delta": loss[1]}
        sw = weight if weighted else None
        gathered = cat[cr.long()].contiguous(), an[ar.long()].contiguous()
        want = run_pass(*gathered, None, weights, cfg, stats, y, sw, base, dloss)
        got = run_pass(cat, an, (cr, ar), weights, cfg, stats, y, sw, base, dloss)
        what = f"{name} bn={bn} rate={rate} {loss[0]} weighted={weighted} base={base}"
        for k in ("loss", "pred", "saved", "mm", "mv"):
            assert torch.equal(got[k], want[k]), f"{what}: {k}"
        assert torch.isfinite(got["loss"]) and torch.isfinite(got["saved"]).all(), what
        assert bn == (not torch.equal(got["mm"], stats[0])), f"{what}: the moving statistics move with bn_batch only"
        for t, (g, e) in enumerate(zip(got["grads"], want["grads"])):
            assert (g is None) == (e is None) and (g is None or torch.equal(g, e)), f"{what}: gradient of tensor {t}"
        if base and (B > 1 or not bn):
            assert got["grads"][0].abs().max() > 0 and got["grads"][2].abs().max() > 0, f"{what}: the indexed job ran"
        seen.add(float(got["loss"]))
    assert len(seen) > 8, "the settings reach the loss"


def test_index_outside_its_table_reads_zeros_and_bad_indices_raise():
    rng = np.random.default_rng(3)
    B, D, F, Mx = 9, 32, 32, 20
    weights = head_tensors(rng, D, F, Mx)
    stats = _dev(rng.uniform(0.0, 0.8, 256)), _dev(rng.uniform(0.5, 2.0, 256))
    cat, an = _dev(rng.normal(0.0, 1.0, (4, D))), _dev(rng.normal(0.0, 1.0, (3, D)))
    y = _dev(rng.normal(0.0, 1.0, B))
    cfg = {"fp_size": F, "mixing_size": Mx, "l2": [0.0] * 18, "momentum": R.BN_MOMENTUM, "epsilon": R.BN_EPS,
           "bn_batch": True, "dropout": None, "loss_kind": 1, "delta": 1.0}
    cr, ar = rng.integers(0, 4, B), rng.integers(0, 3, B)
    for bad_c, bad_a in ((4, 0), (0, -1)):   # the host check of ops refuses what the kernel would read as zeros
        with pytest.raises(ValueError):
            ops.transfer_head_loss_rows(cat, an, np.r_[cr[:-1], bad_c], np.r_[ar[:-1], bad_a], weights,
                                        dict(cfg, moving_mean=stats[0], moving_variance=stats[1]), y,
                                        torch.zeros(64, device=DEV))
    # on the device the kernels never trust an index: a row outside the table is a row of zeros, nothing is read there
    cat0, an0 = torch.cat([cat, torch.zeros(1, D, device=DEV)]), torch.cat([an, torch.zeros(1, D, device=DEV)])
    out_c, out_a = _dev(np.r_[cr[:-1], 1 << 30], torch.int32), _dev(np.r_[ar[:-2], -7, 3], torch.int32)
    in_c, in_a = _dev(np.r_[cr[:-1], 4], torch.int32), _dev(np.r_[ar[:-2], 3, 3], torch.int32)
    got = run_pass(cat, an, (out_c, out_a), weights, cfg, stats, y, None, True, _dev([1.0]))
    want = run_pass(cat0, an0, (in_c, in_a), weights, cfg, stats, y, None, True, _dev([1.0]))
    assert torch.equal(got["loss"], want["loss"]) and torch.equal(got["saved"], want["saved"])
    assert all(torch.equal(g, e) for g, e in zip(got["grads"], want["grads"]))


def test_indexed_gradients_against_fp64():
    """The fuzz case "B=33" (batch statistics, Huber on both branches, all 18 tensors, 33 samples over 24 distinct
    rows per ion), its pooled rows scattered into tables: loss, moving statistics and every parameter gradient at the
    bounds tests/test_gpu_head_fuzz.py applies to the transfer loss (VALUE_TOL, GRAD_TOL)."""
    c = next(c for c in FZ.transfer_cases() if c.name == "B=33")
    inp = FZ.transfer_inputs(c)
    ref = FZ.transfer_reference(c, inp, torch.float64)
    rng = np.random.default_rng(5)
    tables, rows = [], []
    for k in ("pc", "pa"):   # the distinct rows in a shuffled order, between rows no sample reads
        uniq, inverse = np.unique(inp[k], axis=0, return_inverse=True)
        perm = rng.permutation(len(uniq) + 4)
        table = rng.normal(0.0, 1.0, (len(uniq) + 4, c.D)).astype(np.float32)
        table[perm[:len(uniq)]] = uniq
        tables.append(_dev(table))
        rows.append(_dev(perm[np.asarray(inverse).reshape(-1)], torch.int32))
        assert np.array_equal(table[perm[np.asarray(inverse).reshape(-1)]], inp[k])
    assert tables[0].shape[0] - 4 == FZ.TH_POOL_ROWS < c.B, "the case repeats rows"
    weights = [_dev(a) for a in inp["w"]]
    mm, mv = _dev(inp["mm"]), _dev(inp["mv"])
    step = torch.tensor([FZ.TH_STEP], dtype=torch.int64, device=DEV)
    cfg = {"fp_size": c.F, "mixing_size": c.Mx, "l2": inp["l2"], "momentum": R.BN_MOMENTUM, "epsilon": R.BN_EPS,
           "bn_batch": bool(c.bn), "loss_kind": 1, "delta": c.loss[1],
           "dropout": ops.Dropout(c.rate, FZ.TH_SEED, ops.dropout_layer_word(L.Dropout.LAYER_ID), step) if c.rate else None}
    assert c.bn and c.loss[0] == "huber"
    got = run_pass(tables[0], tables[1], rows, weights, cfg, (mm, mv), _dev(inp["y"]), None, True, _dev([FZ.DLOSS]))
    np_ = lambda t: t.detach().cpu().numpy()
    assert_close(np_(got["loss"]).reshape(1), ref["loss"], FZ.VALUE_TOL, "loss")
    assert_close(np_(got["mm"]), ref["mm"], FZ.VALUE_TOL, "moving mean")
    assert_close(np_(got["mv"]), ref["mv"], FZ.VALUE_TOL, "moving variance")
    assert set(ref["grads"]) == set(range(18))
    for t, e in ref["grads"].items():
        assert_close(np_(got["grads"][t]), e, FZ.GRAD_TOL, f"gradient of tensor {t} ({R.HEAD_TENSORS[t]})")


# ---------------------------------------------------------------------------------------------------- model level
def repeated_set(n, n_cat, n_an, seed):
    """n samples over n_cat cation and n_an anion graphs -> (inputs, y, weights)."""
    rng = np.random.default_rng(seed)
    pool = synthetic.make_batch(max(n_cat, n_an), seed=seed)
    ci, ai = rng.integers(0, n_cat, n), rng.integers(0, n_an, n)
    ci[:n_cat], ai[:n_an] = np.arange(n_cat), np.arange(n_an)
    x = {f"{p}_{k}": pool[f"{p}_{k}"][idx] for p, idx in (("cat", ci), ("an", ai)) for k in ("atom", "bond", "connectivity")}
    return x, rng.normal(0.0, 1.0, n).astype(np.float32), rng.uniform(0.2, 2.0, n).astype(np.float32)


ENCODER_ENTRIES = ("impnn_encoder", "impnn_batch_assemble", "impnn_embed_gather", "impnn_bmm_", "impnn_bond_type",
                   "impnn_reduce_scatter_add", "impnn_gated_update", "impnn_kept_rows", "impnn_row_index_fill",
                   "impnn_global_sum_pool", "impnn_edge_type", "impnn_message_reduce", "impnn_reduce_scatter_bwd")


class EncoderCalls:
    """Counts the library calls that belong to an encoder pass or a batch assemble, by wrapping the loaded entries."""

    def __init__(self, monkeypatch):
        self.count, self.names = 0, []
        lib = _lib.load()
        for name in _lib.SIGNATURES:
            if name.startswith(ENCODER_ENTRIES) and not name.endswith(("_bytes", "_floats", "_layout", "_offset")):
                monkeypatch.setattr(lib, name, self._wrap(name, getattr(lib, name)), raising=False)

    def _wrap(self, name, fn):
        def counted(*args):
            self.count += 1
            self.names.append(name)
            return fn(*args)
        return counted


def test_cached_fit_follows_the_plain_fit_without_an_encoder_call(tmp_path, monkeypatch):
    x, y, w = repeated_set(43, 6, 5, 21)       # 5 batches of 8 and a last one of 3
    vx, vy, vw = repeated_set(20, 6, 5, 22)
    hist, state, marks = {}, {}, {}
    calls = EncoderCalls(monkeypatch)

    class Mark(train.Callback):
        def on_epoch_begin(self, epoch, logs=None):
            if epoch == 0:
                marks["at first epoch"] = calls.count

    for cached in (False, True):
        t = TT.make_transfer(tmp_path, D=32, S=2)
        TT.stage1(t)
        t.compile(train.Adam(1e-3), loss=train.Huber(delta=1.0), metrics=["mae"])
        frozen = {n: a.copy() for n, a in t.state_dict().items() if not (n.startswith("mp_") or n.startswith("melting_point"))}
        before = calls.count
        h = t.fit(x, y, validation_data=(vx, vy, vw), epochs=3, batch_size=8, shuffle=False, sample_weight=w,
                  callbacks=[Mark()], cache_frozen_encoder=cached)
        hist[cached], state[cached] = h.history, t.state_dict()
        if cached:
            assert marks["at first epoch"] > before, "the ions were encoded before the first epoch"
            assert calls.count == marks["at first epoch"], calls.names[marks["at first epoch"] - before:]
        else:
            assert calls.count > marks["at first epoch"], "the counter sees the plain fit's encoder"
        for n, a in frozen.items():
            assert np.array_equal(state[cached][n], a), f"frozen {n} changed"
        assert int(t.dropout_counter().item()) == 18 and t.optimizer.iterations == 18
    print("plain", hist[False], "cached", hist[True])
    assert list(hist[True]) == list(hist[False]) == ["loss", "mae", "val_loss", "val_mae"]
    for k in hist[False]:
        close(np.array(hist[True][k]), np.array(hist[False][k]), 2e-4, k)
    for n in state[False]:
        if n.startswith("mp_") or n.startswith("melting_point"):
            close(state[True][n], state[False][n], 2e-4, n)
    assert len(set(hist[True]["loss"])) == 3
    exact = all(hist[True][k] == hist[False][k] for k in hist[False]) and all(
        np.array_equal(state[True][n], state[False][n]) for n in state[False])
    print("cached fit equals the plain fit bit for bit:", exact)


def test_cached_evaluate_equals_the_indexed_batches(tmp_path):
    x, y, w = repeated_set(21, 4, 3, 31)
    t = TT.make_transfer(tmp_path, D=32, S=2)
    TT.stage1(t)
    t.compile(train.Adam(1e-3), loss="huber", metrics=["mae"])
    plain = t.evaluate(x, y, batch_size=8, sample_weight=w, return_dict=True)
    cached = t.evaluate(x, y, batch_size=8, sample_weight=w, return_dict=True, cache_frozen_encoder=True)
    enc = t.frozen_encodings(x)
    again = t.evaluate(enc, y, batch_size=8, sample_weight=w, return_dict=True)
    assert cached == again and list(cached) == list(plain)
    for k in plain:
        close(np.array([cached[k]]), np.array([plain[k]]), 2e-4, k)
    assert enc.cat.shape == (4, 32) and enc.an.shape == (3, 32) and len(enc) == 21


def test_captured_step_over_encodings_equals_eager_indexed_steps(tmp_path):
    x, y, w = repeated_set(40, 6, 5, 41)
    B = 8
    row_sets = [np.arange(0, 8), np.arange(30, 38), np.array([39, 0, 17, 17, 5, 23, 8, 31])]
    out = {}
    for graphed in (False, True):
        t = TT.make_transfer(tmp_path, D=32, S=2)
        TT.stage1(t)
        t.compile(train.Adam(1e-3), loss=train.Huber(delta=1.0), metrics=["mae"])
        enc = t.frozen_encodings(x)
        y_dev, w_dev = _dev(y).reshape(-1, 1), _dev(w)
        rows = [_dev(r, torch.int64) for r in row_sets]
        records = t._metric_set.buffer("train", t.device).zero_()
        losses = []
        if graphed:
            step = train.GraphedTrainStep(t, rows[0], y[row_sets[0]], resident=(enc, y_dev, w_dev),
                                          sample_weight=w_dev[rows[0]])
            assert step.matches(enc) and not records.any(), "the warm-up steps left no trace in the records"
            for r in rows:
                losses.append(step.step_on_rows(enc, y_dev, r, w_dev).clone())
            with pytest.raises(ValueError):
                step(x, y[:B], w[:B])
        else:
            for r in rows:
                losses.append(t.train_on_encoded_batch(enc, r, y_dev[r], w_dev[r], metric_slot="train"))
        torch.cuda.synchronize()
        out[graphed] = (torch.stack(losses).cpu(), t.state_dict(), records.cpu().clone(), t.optimizer.state(),
                        int(t.dropout_counter().item()))
    assert torch.equal(out[True][0], out[False][0]), (out[True][0], out[False][0])
    assert len(set(out[True][0].tolist())) == 3
    for n, a in out[False][1].items():
        assert np.array_equal(out[True][1][n], a), n
    assert torch.equal(out[True][2], out[False][2]) and out[True][2][0, 0] == 3 * B
    for k in ("m", "v", "step"):
        assert torch.equal(out[True][3][k], out[False][3][k]), k
    assert out[True][4] == out[False][4] == 3


def test_load_weights_and_a_stage2_compile_invalidate(tmp_path):
    x, y, _ = repeated_set(16, 3, 3, 51)
    t = TT.make_transfer(tmp_path, D=32, S=2)
    TT.stage1(t)
    t.compile(train.Adam(1e-3), loss="huber")
    enc = t.frozen_encodings(x)
    rows = torch.arange(8, device=DEV)
    y_dev = _dev(y).reshape(-1, 1)
    step = train.GraphedTrainStep(t, rows, y[:8], resident=(enc, y_dev))
    step.step_on_rows(enc, y_dev, rows)
    t.train_on_encoded_batch(enc, rows, y_dev[rows])
    assert not enc.stale(t), "training the head leaves the encodings current"
    t.load_weights(t.state_dict())
    assert enc.stale(t)
    for call in (lambda: t.train_on_encoded_batch(enc, rows, y_dev[rows]), lambda: t.evaluate(enc, y),
                 lambda: step.step_on_rows(enc, y_dev, rows),
                 lambda: train.GraphedTrainStep(t, rows, y[:8], resident=(enc, y_dev))):
        with pytest.raises(ValueError):
            call()
    fresh = t.frozen_encodings(x)
    assert not fresh.stale(t) and torch.equal(fresh.cat, enc.cat) and torch.equal(fresh.an_row, enc.an_row)

    # inside fit: a callback that loads weights between epochs makes fit encode and capture again, and nothing else
    class Reload(train.Callback):
        def on_epoch_end(self, epoch, logs=None):
            if epoch == 0:
                self.model.load_weights(self.model.state_dict())

    hists = []
    for callbacks in ([], [Reload()]):
        t2 = TT.make_transfer(tmp_path, D=32, S=2)
        TT.stage1(t2)
        t2.compile(train.Adam(1e-3), loss="huber")
        v0 = t2.encoder_version
        hists.append(t2.fit(x, y, validation_data=(x, y), epochs=3, batch_size=8, shuffle=False, callbacks=callbacks,
                            cache_frozen_encoder=True).history)
        assert (t2.encoder_version > v0) == bool(callbacks)
    assert hists[0] == hists[1] and len(set(hists[0]["loss"])) == 3
    TT.stage2(t)
    t.compile(train.Adam(1e-4), loss="huber")
    for call in (lambda: t.fit(x, y, epochs=1, batch_size=8, cache_frozen_encoder=True),
                 lambda: t.evaluate(x, y, cache_frozen_encoder=True), lambda: t.frozen_encodings(x),
                 lambda: t.train_on_encoded_batch(fresh, rows, y_dev[rows])):
        with pytest.raises(ValueError, match="an encoder layer is trainable"):
            call()
    # a stage-2 step moves the version on: what stage 1 cached is stale from then on
    v = t.encoder_version
    t.train_on_batch({k: a[:8] for k, a in x.items()}, y[:8])
    assert t.encoder_version > v and fresh.stale(t)
