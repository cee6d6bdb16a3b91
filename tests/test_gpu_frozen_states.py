"""Cached frozen steps on the GPU: (1) impnn_state_rows against torch.index_select, bit for bit, with guard bytes;
(2) the resumed training pass against the fp64 references of tests/transfer_ref.py and tests/grad_ref.py at the
tolerances of tests/test_gpu_transfer.py::test_whole_model_gradients_against_fp64 (loss 1e-5, gradients 2e-4), and
against the plain pass of the same model at the same tolerances; (3) nothing frozen runs: no embedding launch, half the
step entries, one impnn_state_rows call; (4) a captured step over states against eager ones; (5) fit with
cache_frozen_steps against the plain fit, with a rebuild after load_weights; (6) the padding rule: below the row-list
threshold at atom_dim 128 every gradient is finite."""
import itertools

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, data, layers as L, model as MM, ops, synthetic, train, weights

import grad_ref as GR
import test_gpu_transfer as TT
import transfer_ref as R
from test_gpu_train import close

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64            # floats behind every output buffer
SENTINEL = -7.25


def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


# ------------------------------------------------------------------------------------------------- (1) the kernel
ROW_FLOATS = [8, 5 * 8, 40 * 32, 7 * 128, 160 * 32, 1028]   # R = 1 x D = 8 ... one 4 KB piece plus 4 floats
TABLE_ROWS = [1, 2, 50]


def _table_and_rows(rng, rf, n_rows, B, bad):
    """A table of n_rows rows of rf floats and B indices: repeats, the first and the last row; ``bad``: -1 and n_rows
    among them (a row of zeros each) -> (table, rows, the rows index_select takes from the table with a zero row)."""
    table = _dev(rng.normal(0.0, 1.0, (n_rows, rf)))
    idx = rng.integers(0, n_rows, B)
    idx[0] = n_rows - 1
    if B > 1:
        idx[-1] = 0
    if B > 2:
        idx[1] = idx[2]
    want = idx.copy()
    if bad:
        idx[B // 2] = -1 if B % 2 else n_rows
        want[B // 2] = n_rows
        if B > 4:
            idx[3], want[3] = n_rows, n_rows
            idx[4], want[4] = -1, n_rows
    return table, _dev(idx, torch.int32), _dev(want, torch.int64)


def _guarded(B, rf):
    flat = torch.full((B * rf + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    return flat, flat[:B * rf].view(B, rf)


def _check(table, want, flat, out, what):
    ref = torch.index_select(torch.cat([table, torch.zeros_like(table[:1])]), 0, want)
    assert torch.equal(out, ref), what
    assert bool((flat[out.numel():] == SENTINEL).all()), f"{what}: the guard behind out was written"


@pytest.mark.parametrize("B", [1, 3, 32, 257])
def test_state_rows_equals_index_select_bit_for_bit(B):
    rng = np.random.default_rng(B)
    # one ion alone: every row length with every table size
    for rf, n_rows, bad in itertools.product(ROW_FLOATS, TABLE_ROWS, (False, True)):
        table, rows, want = _table_and_rows(rng, rf, n_rows, B, bad)
        flat, out = _guarded(B, rf)
        got = ops.state_rows([table], [rows], out=[out])
        assert got[0] is out
        _check(table, want, flat, out, f"B={B} row_floats={rf} table_rows={n_rows} bad={bad}")
    # two ions of different row lengths in one call, both orders (the ion with fewer pieces idles some workgroups)
    pairs = [(160 * 32, 8), (8, 160 * 32), (1028, 40 * 32), (5 * 8, 7 * 128), (40 * 32, 40 * 32), (8, 8)]
    for (rf_c, rf_a), (n_c, n_a), bad in itertools.product(pairs, ((50, 2), (1, 50)), (False, True)):
        tc, rc, wc = _table_and_rows(rng, rf_c, n_c, B, bad)
        ta, ra, wa = _table_and_rows(rng, rf_a, n_a, B, bad)
        fc, oc = _guarded(B, rf_c)
        fa, oa = _guarded(B, rf_a)
        ops.state_rows([tc, ta], [rc, ra], out=[oc, oa])
        what = f"B={B} row_floats=({rf_c},{rf_a}) table_rows=({n_c},{n_a}) bad={bad}"
        _check(tc, wc, fc, oc, what + " cation")
        _check(ta, wa, fa, oa, what + " anion")
    # the wrapper makes the outputs where none are given, in the tables' shape, and refuses what the kernel cannot take
    table = _dev(rng.normal(0.0, 1.0, (5, 7, 8)))
    rows = _dev(rng.integers(0, 5, B), torch.int32)
    got, = ops.state_rows([table], [rows])
    assert got.shape == (B, 7, 8) and torch.equal(got, table[rows.long()])
    for bad_call in (lambda: ops.state_rows([table], [rows.long()]), lambda: ops.state_rows([table, table], [rows]),
                     lambda: ops.state_rows([table.double()], [rows]), lambda: ops.state_rows([], [])):
        with pytest.raises((TypeError, ValueError)):
            bad_call()
    with pytest.raises(RuntimeError):   # 6 floats per row: no 16-byte lanes (IMPNN_E_BADARG from the library)
        ops.state_rows([_dev(np.zeros((3, 6)))], [rows.clamp(max=2)])


def test_state_rows_offsets_past_2_31_floats():
    """A table of 420 000 rows x 5120 floats (N = 160, D = 32) holds 2.15e9 floats: the rows on both sides of float
    2^31 and the last one come back bit for bit (the table itself is never filled: 8.6 GB of it stay as allocated)."""
    rf, n_rows = 160 * 32, 420_000
    assert n_rows * rf > 2 ** 31
    split = 2 ** 31 // rf                       # the row that float 2^31 lies in
    idx = [split - 1, split, split + 1, n_rows - 1, 0, split]
    table = torch.empty((n_rows, rf), dtype=torch.float32, device=DEV)
    rng = np.random.default_rng(31)
    for r in set(idx):
        table[r] = _dev(rng.normal(0.0, 1.0, rf))
    rows = _dev(idx, torch.int32)
    flat, out = _guarded(len(idx), rf)
    ops.state_rows([table], [rows], out=[out])
    assert torch.equal(out, table[rows.long()]) and bool((flat[out.numel():] == SENTINEL).all())
    assert len({float(v) for v in out[:, 0]}) == len(set(idx)), "the rows differ from each other"


# ------------------------------------------------------------------------------------------------- (2) the resumed pass
def cation_only(t):
    TT.stage1(t)
    for layer in t.layers:
        if any(k in layer.name for k in ("cat_bmm_2", "cat_bmm_3", "gated_update_2", "gated_update_3")):
            layer.trainable = True


PATTERNS = {"stage2": TT.stage2, "mixed": TT.mixed, "cation_only": cation_only}
PREFIXES = {"stage2": {"cat": 2, "an": 2}, "mixed": {"cat": 3, "an": 1}, "cation_only": {"cat": 2, "an": None}}


def repeated_batch(B, n_cat, n_an, seed, temperature=False, **kw):
    """B samples drawn with repeats from n_cat cation and n_an anion graphs of one synthetic.make_batch, every graph
    used, not in graph order -> (inputs, cat_of, an_of)."""
    rng = np.random.default_rng(seed)
    pool = synthetic.make_batch(max(n_cat, n_an), seed=seed, **kw)
    ci, ai = rng.integers(0, n_cat, B), rng.integers(0, n_an, B)
    ci[:n_cat], ai[:n_an] = rng.permutation(n_cat), rng.permutation(n_an)
    x = {f"{p}_{k}": pool[f"{p}_{k}"][idx] for p, idx in (("cat", ci), ("an", ai)) for k in ("atom", "bond", "connectivity")}
    if temperature:
        x["temperature"] = rng.uniform(253.0, 393.0, size=(B, 1)).astype(np.float32)
    return x, ci, ai


def _grads(t):
    return {n: v.grad.detach().clone() for n, v in t.trainable_variables()}


def _transfer_pass_against_fp64(t, inp, pattern, D, tol_note, small=0.4):
    """One resumed pass of a compiled transfer model on ``inp`` against transfer_ref.loss and against the plain pass.
    Targets on both Huber branches, as test_whole_model_gradients_against_fp64 sets them; ``small``: the errors on the
    quadratic branch (per sample, so that a batch of 4 does not cancel the output bias's gradient to zero)."""
    B = len(inp["cat_atom"])
    w = R.leaves(t.state_dict())
    mask = TT.head_mask(9, B)
    with torch.no_grad():
        pred0, _, _ = R.head(w, *R.pooled(w, inp), True, mask)
    off = np.where(np.arange(B) % 2 == 0, small, 2.5) * np.where(np.arange(B) % 3 == 0, -1.0, 1.0)
    y = (pred0.numpy() - off).astype(np.float32)
    lo, e, _, _ = R.loss(w, inp, y, True, mask)
    ae = e.detach().abs().numpy()
    assert (ae <= 1.0).any() and (ae > 1.0).any() and np.all(np.abs(ae - 1.0) > 1e-3)
    lo.backward()
    assert abs(float(w["melting_point/bias"].grad)) > 1e-3, "the targets leave the output bias a gradient"
    x = t._to_device(inp)
    stats = t.mp_bn_1.moving_mean.clone(), t.mp_bn_1.moving_variance.clone()
    # the plain pass of the same model
    t.dropout_counter().fill_(9)
    plain = t._loss(x, y, training=True)
    plain.backward()
    t.join_training_streams()
    plain_grads = _grads(t)
    t.optimizer.zero_grad()
    with torch.no_grad():
        t.mp_bn_1.moving_mean.copy_(stats[0])
        t.mp_bn_1.moving_variance.copy_(stats[1])
    # the resumed one
    st = t.frozen_states(x)
    t.dropout_counter().fill_(9)
    before = {n: a.copy() for n, a in t.state_dict().items()}
    loss = t._loss(x, y, training=True, states=(st, st.cat_row, st.an_row))
    loss.backward()
    t.join_training_streams()
    close(loss, lo, 1e-5, "loss")
    close(loss, plain, 1e-5, "loss against the plain pass")
    trained = dict(t.trainable_variables())
    worst = 0.0
    for name, tensor in t._named_tensors().items():
        if name in trained:
            assert torch.isfinite(tensor.grad).all(), name
            close(tensor.grad, w[name].grad, 2e-4, f"{pattern} D={D}: grad {name}")
            close(tensor.grad, plain_grads[name], 2e-4, f"{pattern} D={D}: grad {name} against the plain pass")
            worst = max(worst, float((tensor.grad - plain_grads[name]).abs().max() / plain_grads[name].abs().max().clamp_min(1e-12)))
        else:
            assert tensor.grad is None and not tensor.requires_grad, name
            assert np.array_equal(tensor.detach().cpu().numpy(), before[name]), name
    print(f"{tol_note} {pattern} D={D}: resumed against plain: loss differs by {abs(float(loss.detach()) - float(plain.detach())):.3e}, "
          f"largest relative gradient difference {worst:.3e}, bit-equal: {worst == 0.0 and bool(loss == plain)}")
    return st


@pytest.mark.parametrize("D", [32, 128])
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_resumed_pass_against_fp64_and_the_plain_pass(tmp_path, pattern, D):
    B = 24
    t = TT.make_transfer(tmp_path, D=D, seed=3)
    PATTERNS[pattern](t)
    t.compile(train.Adam(1e-3), loss=train.Huber(delta=1.0))
    assert t.frozen_prefix() == PREFIXES[pattern]
    inp, ci, ai = repeated_batch(B, 10, 6, 7)
    st = _transfer_pass_against_fp64(t, inp, pattern, D, "resumed pass")
    assert st.steps == PREFIXES[pattern] and len(st) == B and not st.stale(t)
    N = inp["cat_atom"].shape[1]
    assert st.cat.shape == (10, N, D) and st.an.shape == (6, 1 if pattern == "cation_only" else N, D)
    assert torch.isfinite(st.cat).all() and torch.isfinite(st.an).all(), "every row of a table is finite, padding too"
    assert st.nbytes == 4 * (st.cat.numel() + st.an.numel() + 2 * B)
    for row, of in ((st.cat_row, ci), (st.an_row, ai)):   # not the identity: first-occurrence order with repeats
        order = list(dict.fromkeys(int(g) for g in of))
        assert row.cpu().tolist() == [order.index(int(g)) for g in of] and row.cpu().tolist() != list(range(B))


def test_padding_rows_hold_finite_states_below_the_row_list_threshold(tmp_path):
    """atom_dim 128, ions of 8 atoms padded to N = 40, B = 4: 160 atom rows per ion, below TRAIN_ROW_LIST_MIN_ROWS, so
    the trained steps run GatedUpdate forward and backward over ALL rows of the gathered states - padding rows times a
    zero incoming gradient must not be NaN: the tables are built without a kept-row list."""
    B, D, N = 4, 128, 40
    assert B * N < MM.TRAIN_ROW_LIST_MIN_ROWS
    t = TT.make_transfer(tmp_path, D=D, seed=3)
    TT.stage2(t)
    t.compile(train.Adam(1e-3), loss=train.Huber(delta=1.0))
    inp = synthetic.make_batch(B, max_atoms=8, max_edges=24, min_atoms=8, seed=13)
    assert all((inp[f"{p}_atom"] > 0).all() for p in ("cat", "an")), "ions of 8 atoms"
    for p in ("cat", "an"):
        inp[f"{p}_atom"] = np.pad(inp[f"{p}_atom"], ((0, 0), (0, N - 8)))
    st = _transfer_pass_against_fp64(t, inp, "stage2", D, "padding rule", small=0.4 + 0.1 * np.arange(B))
    assert st.cat.shape == (B, N, D) and torch.isfinite(st.cat).all() and torch.isfinite(st.an).all()
    assert float(st.cat[:, 8:].abs().max()) > 0, "the padding rows hold what the list-free pass computes, not a fill"


def test_viscosity_model_with_frozen_lower_steps_against_fp64():
    B, D, S = 24, 32, 4
    Va, Vb = synthetic.DEFAULT_VA, synthetic.DEFAULT_VB
    L.reset_uids()
    m = MM.build_model(Va, Vb, atom_dim=D, num_steps=S, device=DEV)
    m.load_weights(weights.init_weights("viscosity", Va, Vb, atom_dim=D, num_steps=S, seed=5, perturb=True))
    frozen = ("cat_bmm_0", "cat_bmm_1", "an_bmm_0", "an_bmm_1", "gated_update", "gated_update_1", "gated_update_4",
              "gated_update_5")
    for layer in m.layers:
        layer.trainable = not (layer.name.startswith("embedding") or layer.name in frozen)
    m.compile(train.Adam(1e-3), loss="mse")
    assert m.frozen_prefix() == {"cat": 2, "an": 2}
    inp, _, _ = repeated_batch(B, 10, 6, 17, temperature=True)
    y = np.random.default_rng(17).normal(0.0, 1.0, B).astype(np.float32)
    w = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in m.state_dict().items()}
    lo = GR.model_loss("viscosity", w, inp, y, m.fp_l2)
    lo.backward()
    x = m._to_device(inp)
    st = m.frozen_states(x)
    before = {n: a.copy() for n, a in m.state_dict().items()}
    loss = m._loss(x, y, training=True, states=(st, st.cat_row, st.an_row))
    loss.backward()
    m.join_training_streams()
    close(loss, lo, 1e-5, "loss")
    trained = dict(m.trainable_variables())
    assert 0 < len(trained) < len(m._named_tensors())
    for name, tensor in m._named_tensors().items():
        if name in trained:
            close(tensor.grad, w[name].grad, 2e-4, f"viscosity: grad {name}")
        else:
            assert tensor.grad is None and np.array_equal(tensor.detach().cpu().numpy(), before[name]), name


# ------------------------------------------------------------------------------------------------- (3) nothing frozen runs
class LibraryCalls:
    """Every call into the library, by wrapping the loaded entries: names and the integer value of each argument."""
    QUERIES = ("_bytes", "_floats", "_layout", "_offset", "_words", "_version", "_string", "_arch", "_chunk")

    def __init__(self, monkeypatch):
        self.calls = []
        lib = _lib.load()
        for name in _lib.SIGNATURES:
            if hasattr(lib, name) and not name.endswith(self.QUERIES):
                monkeypatch.setattr(lib, name, self._wrap(name, getattr(lib, name)), raising=False)

    def _wrap(self, name, fn):
        def counted(*args):
            self.calls.append((name, [getattr(a, "value", a) for a in args]))
            return fn(*args)
        return counted

    def names(self, since=0):
        return [n for n, _ in self.calls[since:]]

    def family(self, prefix, since=0):
        return sum(n.startswith(prefix) and not n.endswith("_bwd") for n in self.names(since))


STEP_FAMILIES = ("impnn_bmm_message", "impnn_reduce_scatter_add", "impnn_gated_update")


def test_nothing_frozen_runs_in_a_resumed_pass(tmp_path, monkeypatch):
    B = 24
    inp, _, _ = repeated_batch(B, 10, 6, 7)
    y = np.zeros(B, np.float32)
    calls = LibraryCalls(monkeypatch)
    counted = {}
    for pattern in ("stage2", "cation_only"):
        t = TT.make_transfer(tmp_path, D=32, S=4)
        PATTERNS[pattern](t)
        t.compile(train.Adam(1e-4), loss=train.Huber(delta=1.0))
        x = t._to_device(inp)
        st = t.frozen_states(x)
        rows = torch.arange(B, device=DEV)
        for resumed in (False, True):
            kw = {"states": (st, st.cat_row, st.an_row)} if resumed else {}
            at = len(calls.calls)
            loss = t._loss(x, y, training=True, **kw)   # the forward alone: every entry called here is a forward entry
            fwd = {f: calls.family(f, at) for f in STEP_FAMILIES + ("impnn_embed_gather", "impnn_state_rows")}
            loss.backward()
            t.join_training_streams()
            t.optimizer.zero_grad()
            at_step = len(calls.calls)
            if resumed:
                t.train_on_state_batch(st, x, rows, y)
            else:
                t.train_on_batch(x, y)
            counted[pattern, resumed] = (fwd, len(calls.calls) - at_step)
            if resumed and pattern == "cation_only":   # the anion's inputs reach no entry at all
                an = {x[f"an_{k}"].data_ptr() for k in ("atom", "bond", "connectivity")}
                for name, args in calls.calls[at:at_step]:
                    assert not an & {a for a in args if isinstance(a, int)}, f"{name} was handed an anion input"
        plain, res = counted[pattern, False][0], counted[pattern, True][0]
        print(f"{pattern}: forward entries plain {plain} resumed {res}; library calls of one eager step: plain "
              f"{counted[pattern, False][1]}, resumed {counted[pattern, True][1]}")
        assert plain["impnn_embed_gather"] >= 1 and res["impnn_embed_gather"] == 0
        assert plain["impnn_state_rows"] == 0 and res["impnn_state_rows"] == 1
        ions = 2 if pattern == "stage2" else 1   # (the plain pass of the cation-only pattern runs the anion's 4 steps too)
        for f in STEP_FAMILIES:
            assert plain[f] > 0 and plain[f] % 8 == 0, (f, plain[f])
            per_step = plain[f] // 8
            assert res[f] == 2 * ions * per_step, f"{f}: two steps per resumed ion, not four ({res[f]} of {plain[f]})"
        assert counted[pattern, True][1] < counted[pattern, False][1]


# ------------------------------------------------------------------------------------------------- (4) captured = eager
def repeated_set(n, n_cat, n_an, seed):
    x, _, _ = repeated_batch(n, n_cat, n_an, seed)
    return x, np.random.default_rng(seed).normal(0.0, 1.0, n).astype(np.float32)


STAGE2_RATE = 1e-4   # train_melting_point_transfer.py's lr_stage2


def test_captured_step_over_states_follows_eager_state_steps(tmp_path):
    B = 32
    x, y = repeated_set(100, 10, 6, 41)
    row_sets = [np.arange(0, 32), np.arange(60, 92), np.r_[np.arange(99, 70, -1), [0, 17, 17]], np.arange(32, 64),
                np.arange(5, 37)]
    out = {}
    for graphed in (False, True):
        t = TT.make_transfer(tmp_path, D=32, S=4)
        TT.stage2(t)
        t.compile(train.Adam(STAGE2_RATE), loss=train.Huber(delta=1.0))
        xd = {k: v.contiguous() for k, v in t._to_device(x).items()}
        y_dev = _dev(y).reshape(-1, 1)
        st = t.frozen_states(xd)
        before = t.state_dict()
        rows = [_dev(r, torch.int64) for r in row_sets]
        losses = []
        if graphed:
            step = train.GraphedTrainStep(t, {k: v[rows[0]] for k, v in xd.items()}, y[row_sets[0]],
                                          resident=(xd, y_dev), states=st)
            assert int(t.dropout_counter().item()) == 0 and t.optimizer.iterations == 0, "the warm-up left no trace"
            for r in rows:
                losses.append(step.step_on_rows(xd, y_dev, r).clone())
            with pytest.raises(ValueError):
                step({k: v[rows[0]] for k, v in xd.items()}, y[:B])
        else:
            for r in rows:
                losses.append(t.train_on_state_batch(st, xd, r, y_dev[r]))
        torch.cuda.synchronize()
        assert not st.stale(t), "training steps leave the states current"
        assert int(t.dropout_counter().item()) == 5 and t.optimizer.iterations == 5
        after = t.state_dict()
        trained = {n for n, _ in t.trainable_variables()}
        for n, a in before.items():
            if n in trained:
                assert not np.array_equal(after[n], a), f"{n} did not move"
            elif "moving" not in n:
                assert np.array_equal(after[n], a), f"frozen {n} changed"
        out[graphed] = (torch.stack(losses).cpu(), after, trained)
        if graphed:   # stale states are refused at replay and at capture
            t.load_weights(t.state_dict())
            assert st.stale(t)
            for call in (lambda: step.step_on_rows(xd, y_dev, rows[0]),
                         lambda: t.train_on_state_batch(st, xd, rows[0], y_dev[rows[0]]),
                         lambda: train.GraphedTrainStep(t, {k: v[rows[0]] for k, v in xd.items()}, y[row_sets[0]],
                                                        resident=(xd, y_dev), states=st)):
                with pytest.raises(ValueError):
                    call()
    close(out[True][0], out[False][0], 2e-4, "losses")
    assert len(set(out[True][0].tolist())) == 5
    for n in out[False][2]:
        close(out[True][1][n], out[False][1][n], 2e-4, n)


# ------------------------------------------------------------------------------------------------- (5) fit
@pytest.mark.parametrize("graph", [False, True])
def test_fit_over_cached_steps_follows_the_plain_fit(tmp_path, monkeypatch, graph):
    """At the reference's stage-2 rate.  (At 1e-3 two runs of the PLAIN fit on these 10 x 6 ions differ from each other
    by up to 1.6e-2 in the third epoch's loss: the backward's float atomics differ in the last bits from run to run
    and twelve Adam steps of that size amplify them; at 1e-4 four plain runs agreed to 1e-6.)"""
    x, y = repeated_set(100, 10, 6, 11)   # 3 full batches of 32 and a last one of 4
    vx, vy = repeated_set(40, 10, 6, 12)
    builds = []
    build = data.FrozenStates.build.__func__
    monkeypatch.setattr(data.FrozenStates, "build", classmethod(lambda cls, *a, **k: builds.append(1) or build(cls, *a, **k)))

    class Reload(train.Callback):
        def on_epoch_begin(self, epoch, logs=None):
            if epoch == 1:
                self.model.load_weights(self.model.state_dict())

    hist, state = {}, {}
    for what, cached, callbacks in (("plain", False, []), ("cached", True, []), ("reloaded", True, [Reload()])):
        t = TT.make_transfer(tmp_path)
        TT.stage2(t)
        t.compile(train.Adam(STAGE2_RATE), loss=train.Huber(delta=1.0))
        n0 = len(builds)
        h = t.fit(x, y, validation_data=(vx, vy), epochs=3, batch_size=32, seed=3, graph=graph, callbacks=callbacks,
                  cache_frozen_steps=cached)
        hist[what], state[what] = h.history, t.state_dict()
        assert len(builds) - n0 == {"plain": 0, "cached": 1, "reloaded": 2}[what], "the states are built once, and again when stale"
        assert int(t.dropout_counter().item()) == 12 and t.optimizer.iterations == 12
    print("graph", graph, hist)
    trained = {n for n, _ in t.trainable_variables()}
    for what in ("cached", "reloaded"):
        assert list(hist[what]) == list(hist["plain"]) == ["loss", "val_loss"]
        for k in ("loss", "val_loss"):
            close(np.array(hist[what][k]), np.array(hist["plain"][k]), 2e-4, f"{what} {k}")
        for n, a in state["plain"].items():
            if n not in trained and "moving" not in n:
                assert np.array_equal(state[what][n], a), f"frozen {n} differs"
    assert len(set(hist["cached"]["loss"])) == 3
