"""Row-restricted embedding training on the GPU ("Training listed embedding rows"):
  1. impnn_embed_rows_bwd against index_add in float64 at the wave and workgroup edges, twice for the same bits;
  2. its footprint: an exact-size guarded dtable that holds the guard pattern everywhere but in the listed rows;
  3. the autograd nodes and the whole model's gradient against tests/grad_ref.py in fp64: the listed rows match, every
     other element of the tables' gradient is exactly +0.0, with a sink and without one;
  4. the invariant: after eager and captured fits every unlisted row of both tables has the bits it had, and so has a
     listed row no sample uses; Adam's moments stay +0.0 there;
  5. captured against eager steps, save / load.
Tolerances: tests/test_gpu_train_fuzz.py's GRAD_TOL / MODEL_TOL with its FLOOR; tests/test_gpu_train.py's rule (close
at 1e-5 for losses, 1e-4 for weights) for captured against eager."""
import ctypes as C

import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, autograd, data, layers as L, model as MM, synthetic, train, weights
from conftest import assert_close

import grad_ref as GR
from footprint import FILL, Guarded
from test_gpu_train import close
from test_gpu_train_fuzz import FLOOR, GRAD_TOL, MODEL_TOL, _ion

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, N, E, B, VA, VB = 2, 6, 10, 8, 12, 6          # the whole-model shape


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rows_bwd(ids, dout, row_list, dtable_ptr, rows, vocab, dim, accumulate):
    """One call of the entry; dtable_ptr: a device address."""
    lib = _lib.load()
    table = (C.c_void_p * 1)(dtable_ptr)
    rc = lib.impnn_embed_rows_bwd(None if ids is None else C.c_void_p(ids.data_ptr()), C.c_void_p(dout.data_ptr()),
                                  C.c_void_p(row_list.data_ptr()), row_list.numel(), table, rows, vocab, dim, accumulate,
                                  _stream())
    assert rc == 0, (rc, lib.impnn_last_error_string().decode())


# ------------------------------------------------------------------------------------------------- 1. the kernel
ROWS = (1, 63, 64, 65, 255, 256, 257, 4097)      # the wave (64 rows a chunk) and workgroup (8 waves) edges
DIMS = (1, 8, 32, 130, 1024)
VOCABS = (1, 2, 40)


def reference(ids, dout64, listed, init64, vocab, accumulate):
    """index_add in float64 restricted to the listed rows; every other row keeps ``init``."""
    full = torch.zeros(vocab, dout64.shape[1], dtype=torch.float64, device=DEV)
    ok = (ids >= 0) & (ids < vocab)
    full.index_add_(0, ids[ok].long(), dout64[ok])
    want = init64.clone()
    want[listed] = (init64[listed] if accumulate else 0.0) + full[listed]
    return want


def id_cases(rng, rows, vocab):
    """{name: (ids, a row no id uses or None)}: every id equal (the longest sum); random ids that include -1 and vocab,
    with one token taken out (the row no id uses)."""
    hot = vocab - 1
    mixed = rng.integers(-1, vocab + 1, size=rows)
    unused = vocab // 2
    mixed[mixed == unused] = -1
    return {"all equal": (np.full(rows, hot), None), "mixed": (mixed, unused)}


def list_cases(vocab, unused):
    lists = {"one row": [vocab - 1], "every row": list(range(vocab)), "first and last": sorted({0, vocab - 1})}
    if unused is not None:
        lists["a row no id uses"] = [unused]
    return lists


@pytest.mark.parametrize("rows", ROWS)
def test_kernel_against_fp64_at_the_wave_and_workgroup_edges(rows):
    rng = np.random.default_rng(rows)
    calls = 0
    for dim in DIMS:
        dout = torch.tensor(rng.normal(size=(rows, dim)), dtype=torch.float32, device=DEV)
        dout64 = dout.double()
        for vocab in VOCABS:
            init = torch.tensor(rng.normal(size=(vocab, dim)), dtype=torch.float32, device=DEV)
            for id_name, (ids_np, unused) in id_cases(rng, rows, vocab).items():
                ids = torch.tensor(ids_np, dtype=torch.int32, device=DEV)
                for list_name, listed in list_cases(vocab, unused).items():
                    row_list = torch.tensor(listed, dtype=torch.int32, device=DEV)
                    for accumulate in (0, 1):
                        what = f"rows={rows} dim={dim} vocab={vocab} ids {id_name}, list {list_name}, acc={accumulate}"
                        got, again = init.clone(), init.clone()
                        rows_bwd(ids, dout, row_list, got.data_ptr(), rows, vocab, dim, accumulate)
                        rows_bwd(ids, dout, row_list, again.data_ptr(), rows, vocab, dim, accumulate)
                        want = reference(ids, dout64, listed, init.double(), vocab, accumulate)
                        assert torch.equal(_bits(got), _bits(again)), f"{what}: two calls, two results"
                        rest = np.setdiff1d(np.arange(vocab), listed)
                        assert torch.equal(_bits(got[rest]), _bits(init[rest])), f"{what}: an unlisted row was written"
                        assert_close(_np(got[listed]), _np(want[listed]), GRAD_TOL, what, FLOOR)
                        if list_name == "a row no id uses" and not accumulate:
                            assert not _bits(got[listed]).any(), f"{what}: an empty sum is +0.0"
                        calls += 1
    assert calls == len(DIMS) * len(VOCABS) * 2 * 7     # (3 lists for "all equal", 4 for "mixed")


@pytest.mark.parametrize("vocab,dim", [(1, 1), (2, 130), (40, 8), (40, 1024), (257, 32)])
def test_null_ids_are_the_identity(vocab, dim):
    """ids == NULL, rows == vocab: the listed rows of a full gradient are moved (accumulate 0) or added (1)."""
    rng = np.random.default_rng(vocab * dim)
    full = torch.tensor(rng.normal(size=(vocab, dim)), dtype=torch.float32, device=DEV)
    init = torch.tensor(rng.normal(size=(vocab, dim)), dtype=torch.float32, device=DEV)
    listed = sorted({0, vocab // 2, vocab - 1})
    row_list = torch.tensor(listed, dtype=torch.int32, device=DEV)
    rest = np.setdiff1d(np.arange(vocab), listed)
    for accumulate in (0, 1):
        got = init.clone()
        rows_bwd(None, full, row_list, got.data_ptr(), vocab, vocab, dim, accumulate)
        want = full[listed] + init[listed] if accumulate else full[listed]     # one float32 add: exact either way
        assert torch.equal(_bits(got[listed]), _bits(want)), (vocab, dim, accumulate)
        assert torch.equal(_bits(got[rest]), _bits(init[rest]))


# ------------------------------------------------------------------------------------------------- 2. the footprint
@pytest.mark.parametrize("offset", [0, 4])
def test_footprint_only_the_listed_rows_of_an_exact_size_table_are_written(offset):
    rows, vocab, dim = 257, 9, 130
    rng = np.random.default_rng(7)
    ids = torch.tensor(rng.integers(-1, vocab + 1, size=rows), dtype=torch.int32, device=DEV)
    dout = torch.tensor(rng.normal(size=(rows, dim)), dtype=torch.float32, device=DEV)
    # what the C entry itself promises of a list nobody checked: ids outside the vocabulary are skipped, an id that
    # comes twice counts once
    raw = [-1, 2, vocab, 5, 2, 8, 2 ** 31 - 1]
    listed = [2, 5, 8]
    row_list = torch.tensor(raw, dtype=torch.int32, device=DEV)
    snaps = [t.clone() for t in (ids, dout, row_list)]
    pattern = np.full(vocab * dim * 4, FILL, np.uint8).view(np.float32).reshape(vocab, dim)
    for accumulate in (0, 1):
        g = Guarded(vocab * dim * 4, FILL, offset)
        rows_bwd(ids, dout, row_list, g.ptr.value, rows, vocab, dim, accumulate)
        torch.cuda.synchronize()
        got = g.body(np.float32, "dtable").reshape(vocab, dim)             # (asserts both guards)
        rest = np.setdiff1d(np.arange(vocab), listed)
        assert (got[rest].view(np.uint8) == FILL).all(), "a row outside the list was written"
        want = reference(ids, dout.double(), listed, torch.tensor(pattern, device=DEV).double(), vocab, accumulate)
        assert_close(got[listed], _np(want[listed]), GRAD_TOL, f"listed rows, accumulate={accumulate}", FLOOR)
        assert (got[listed].view(np.uint8) != FILL).any()
    for t, snap in zip((ids, dout, row_list), snaps):
        assert torch.equal(_bits(t), _bits(snap)), "an input was modified"
    g = Guarded(vocab * dim * 4, FILL, offset)                               # only ids outside the vocabulary: nothing
    outside = torch.tensor([-5, vocab, vocab + 3], dtype=torch.int32, device=DEV)
    rows_bwd(ids, dout, outside, g.ptr.value, rows, vocab, dim, 0)
    torch.cuda.synchronize()
    g.unchanged(pattern, "dtable of a list outside the vocabulary")


# ------------------------------------------------------------------------------------------------- 3. gradients
def _masked_ok(what, got, ref, listed, tol=MODEL_TOL):
    """The listed rows against the reference's rows; every other element exactly +0.0."""
    rest = np.setdiff1d(np.arange(got.shape[0]), listed)
    assert not _bits(got[rest]).any(), f"{what}: an unlisted element is not +0.0"
    assert float(ref[listed].abs().max()) > 0.0, f"{what}: the reference's listed rows are dead"
    assert_close(_np(got[listed]), _np(ref[listed]), tol, f"{what}: listed rows", FLOOR)


@pytest.mark.parametrize("K,sinks", [(4, True), (4, False), (64, True), (64, False)])
def test_nodes_restrict_the_table_gradient_and_leave_dW_alone(K, sinks):
    """EmbedGather, BondTypeMatrices (K < 64: the adding form into the sinks; K >= 64; no sinks) and BondTypeMatricesAll
    with a row-restricted table against the same nodes on an unrestricted twin: the listed rows, +0.0 elsewhere, the
    same dW."""
    rng = np.random.default_rng(K)
    Vb, D, listed = 7, 8, [0, 3, 6]
    f = lambda *s: torch.tensor(rng.normal(size=s), dtype=torch.float32, device=DEV)
    table0, Ws0, douts = f(Vb, K), [f(K, D, D) for _ in range(2)], [f(Vb, D, D) for _ in range(3)]
    ids = torch.tensor(rng.integers(0, Vb, size=(5, 9)), dtype=torch.int32, device=DEV)
    gh = f(5, 9, K)

    def run(restricted, which):
        table = table0.clone().requires_grad_(True)
        Ws = [w.clone().requires_grad_(True) for w in Ws0]
        if restricted:
            autograd.restrict_rows(table, listed)
        if sinks:
            for t in (table, *Ws):
                t.grad = torch.zeros_like(t)
        if which == "gather":
            out = (autograd.EmbedGather.apply(ids, table) * gh).sum()
        elif which == "one":
            out = (autograd.BondTypeMatrices.apply(table, Ws[0]) * douts[0]).sum()
        else:
            *mats, _ = autograd.BondTypeMatricesAll.apply(table, *Ws)
            out = sum((m * d).sum() for m, d in zip(mats, douts[1:]))
        if sinks:
            out.backward()
            grads = [table.grad] + [w.grad for w in Ws]
        else:
            grads = torch.autograd.grad(out, [table] + Ws, allow_unused=True)
        torch.cuda.synchronize()
        return [None if g is None else g.clone() for g in grads]

    # (the model takes the all-layers node below bond_dim 64 only: MPNNModel._all_type_matrices)
    for which in ("gather", "one") + (("all",) if K < 64 else ()):
        got, full = run(True, which), run(False, which)
        _masked_ok(f"{which} K={K} sinks={sinks}", got[0], full[0].double(), listed, GRAD_TOL)
        for i, (a, b) in enumerate(zip(got[1:], full[1:])):
            assert (a is None) == (b is None)
            if b is not None:
                assert_close(_np(a), _np(b.double()), GRAD_TOL, f"{which}: dW {i}", FLOOR)


def _viscosity_case(D, K, seed):
    rng = np.random.default_rng(seed)
    ca, cb, cc = _ion(rng, B, N, E, VA, VB)
    aa, ab, ac = _ion(rng, B, N, E, VA, VB)
    inputs = {"cat_atom": ca, "cat_bond": cb, "cat_connectivity": cc, "an_atom": aa, "an_bond": ab, "an_connectivity": ac,
              "temperature": rng.uniform(280.0, 400.0, size=(B, 1)).astype(np.float32)}
    w = weights.init_weights("viscosity", VA, VB, atom_dim=D, bond_dim=K, fp_size=12, mixing_size=10, num_steps=S,
                             seed=seed, perturb=True)
    w["visc_params/kernel"] = (w["visc_params/kernel"] * np.float32(0.05)).astype(np.float32)
    y = rng.normal(1.0, 0.5, size=B).astype(np.float32)
    return inputs, w, y


def _freeze_encoder(m):
    for layer in m.layers:
        if layer in (m.atom_emb, m.bond_emb) or "bmm" in layer.name or "gated_update" in layer.name:
            layer.trainable = False


@pytest.mark.parametrize("D,K,row_list_path", [(32, 4, False), (64, 4, False), (64, 4, True), (8, 64, False)])
def test_whole_model_gradient_reaches_the_listed_rows_only(D, K, row_list_path, monkeypatch):
    """Both embeddings frozen with rows listed, the steps frozen, the head trainable, against tests/grad_ref.py in fp64.
    row_list_path: encode_layered's GatedUpdate row list, which a training pass takes from TRAIN_ROW_LIST_MIN_ROWS atom
    rows per ion on - lowered here, so that this shape's 48 rows take it.  K = 64: the per-layer type-matrix nodes, one
    per layer and ion on the two streams, instead of the all-layers node."""
    if row_list_path:
        monkeypatch.setattr(MM, "TRAIN_ROW_LIST_MIN_ROWS", 1)
    inputs, w, y = _viscosity_case(D, K, seed=D + int(row_list_path))
    atom_rows, bond_rows = [0, 3, 7, 11], [0, 2, 5]
    w64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in w.items()}
    ref_loss = GR.model_loss("viscosity", w64, inputs, y, 1e-4)
    ref_loss.backward()
    L.reset_uids()
    m = MM.build_model(VA, VB, atom_dim=D, bond_dim=K, fp_size=12, mixing_size=10, num_steps=S, device=DEV)
    m.load_weights(w)
    _freeze_encoder(m)
    m.atom_emb.trainable_rows, m.bond_emb.trainable_rows = atom_rows, bond_rows
    m.compile(train.Adam(1e-3, clipnorm=1.0))
    names = [n for n, _ in m.trainable_variables()]
    assert names[:2] == ["atom_embedding", "bond_embedding"] and not any("_bmm_" in n or "_gu_" in n for n in names)
    d = m._to_device(inputs)
    loss = m._loss(d, y, training=True)
    loss.backward()
    m.join_training_streams()
    torch.cuda.synchronize()
    what = f"D={D} K={K} row list {row_list_path}"
    assert_close(np.array([float(loss.detach())]), np.array([float(ref_loss.detach())]), 1e-5, f"{what}: loss", FLOOR)
    tables = {"atom_embedding": (m.atom_emb.embeddings, atom_rows), "bond_embedding": (m.bond_emb.embeddings, bond_rows)}
    flat = m.optimizer.flat_grad
    for n, (t, listed) in tables.items():
        assert flat.data_ptr() <= t.grad.data_ptr() < flat.data_ptr() + 4 * flat.numel()    # the sink path
        _masked_ok(f"{what}: {n} in flat_grad", t.grad, w64[n].grad, listed)
    for n, t in m.trainable_variables()[2:]:
        assert_close(_np(t.grad), _np(w64[n].grad), MODEL_TOL, f"{what}: grad {n}", FLOOR)
    # the dense-return path: no sink, torch.autograd.grad
    sink = {n: t.grad.clone() for n, (t, _) in tables.items()}
    for t, _ in tables.values():
        t.grad = None
    loss2 = m._loss(d, y, training=True)
    dense = torch.autograd.grad(loss2, [t for t, _ in tables.values()])
    m.join_training_streams()
    torch.cuda.synchronize()
    for (n, (t, listed)), g in zip(tables.items(), dense):
        assert g.shape == t.shape
        _masked_ok(f"{what}: {n} from torch.autograd.grad", g, w64[n].grad, listed)
        assert_close(_np(g), _np(sink[n].double()), MODEL_TOL, f"{what}: {n}, dense against the sink", FLOOR)


# ------------------------------------------------------------------------------------------------- 4. the invariant
ATOM_ROWS, BOND_ROWS = [2, 5, 11], [1, 3, 5]     # atom 11 and bond 5 occur in no sample of _fit_set


def _fit_set(n=8, seed=3):
    x = synthetic.make_batch(n, max_atoms=N, max_edges=E, atom_vocab_size=VA, bond_vocab_size=VB, min_atoms=3, seed=seed,
                             with_temperature=False)
    for p in ("cat", "an"):
        x[f"{p}_atom"][x[f"{p}_atom"] == 11] = 10
        x[f"{p}_bond"][x[f"{p}_bond"] == 5] = 4
    x["cat_atom"][0, :2], x["an_atom"][1, 0] = (2, 5), 5     # (every listed row but the two above is in use)
    y = np.random.default_rng(seed).normal(0.0, 1.0, size=n).astype(np.float32)
    use = data.token_usage(x, VA, VB)
    assert use.atom[11] == 0 and use.bond[5] == 0 and use.atom[[2, 5]].all() and use.bond[[1, 3]].all()
    return x, y


def _transfer(tmp_path, pattern, seed=1):
    """A transfer model on a synthetic base.  stage1: only the head trains; stage2: the upper step of both ions too.
    Both embeddings stay frozen and list their rows."""
    from test_gpu_transfer import make_transfer, stage1
    t = make_transfer(tmp_path, D=32, S=S, K=4, Va=VA, Vb=VB, seed=seed)
    stage1(t)
    if pattern == "stage2":
        for name in ("cat_bmm_1", "an_bmm_1", "gated_update_1", "gated_update_3"):
            t.get_layer(name).trainable = True
    t.atom_emb.trainable_rows, t.bond_emb.trainable_rows = ATOM_ROWS, BOND_ROWS
    return t


def _check_invariant(what, t, before, used_changed=True):
    """before: {name: table clone}.  Unlisted rows and listed rows nobody uses keep their bits; the used ones move."""
    for n, lyr, listed, unused in (("atom_embedding", t.atom_emb, ATOM_ROWS, [11]), ("bond_embedding", t.bond_emb, BOND_ROWS, [5])):
        now, then = lyr.embeddings, before[n]
        rest = np.setdiff1d(np.arange(now.shape[0]), listed)
        assert torch.equal(_bits(now[rest]), _bits(then[rest])), f"{what}: an unlisted row of {n} changed"
        assert torch.equal(_bits(now[unused]), _bits(then[unused])), f"{what}: a listed row of {n} that no sample uses changed"
        used = [v for v in listed if v not in unused]
        if used_changed:
            for v in used:
                assert not torch.equal(_bits(now[v]), _bits(then[v])), f"{what}: listed row {v} of {n} did not train"
        if getattr(t.optimizer, "m", None) is not None and lyr.embeddings.grad is not None:
            off = (lyr.embeddings.grad.data_ptr() - t.optimizer.flat_grad.data_ptr()) // 4
            for state in (t.optimizer.m, t.optimizer.v):
                rows_of = state[off:off + now.numel()].view_as(now)
                assert not _bits(rows_of[rest]).any(), f"{what}: a moment of an unlisted row of {n} is not +0.0"


OPTIMIZERS = {"clipnorm": lambda: train.Adam(1e-2, clipnorm=1.0),
              "global_clipnorm + weight_decay": lambda: train.Adam(1e-2, global_clipnorm=1.0, weight_decay=1e-2)}


@pytest.mark.parametrize("opt,graph,pattern", [("clipnorm", True, "stage1"), ("clipnorm", False, "stage1"),
                                               ("global_clipnorm + weight_decay", True, "stage2"),
                                               ("global_clipnorm + weight_decay", False, "stage1")])
def test_unlisted_rows_keep_their_bits_through_a_fit(tmp_path, opt, graph, pattern):
    x, y = _fit_set()
    t = _transfer(tmp_path, pattern)
    t.compile(OPTIMIZERS[opt](), loss=train.Huber(delta=1.0))
    assert t.frozen_prefix() == {"cat": 0, "an": 0}
    before = {n: a.clone() for n, a in t._named_tensors().items()}
    hist = t.fit(x, y, epochs=2, batch_size=4, seed=0, graph=graph)
    torch.cuda.synchronize()
    assert t.optimizer.iterations == 4 and np.isfinite(hist.history["loss"]).all()
    _check_invariant(f"{opt}, graph={graph}, {pattern}", t, before)
    trainable = {n for n, _ in t.trainable_variables()}
    for n, a in t._named_tensors().items():
        if n not in trainable:
            assert torch.equal(_bits(a), _bits(before[n])), f"frozen {n} changed"
        elif n not in ("atom_embedding", "bond_embedding"):
            assert not torch.equal(_bits(a), _bits(before[n])), f"{n} did not train"


# ------------------------------------------------------------------------------------------------- 5. graph, files
def test_captured_steps_follow_eager_steps(tmp_path):
    """Three steps each way from the same start, by the rule of test_gpu_train.py's graph-against-eager test: the
    losses at 1e-5, the weights at 1e-4 - and the unlisted rows bit for bit on both sides."""
    x, y = _fit_set(n=12, seed=4)
    ta, tb = _transfer(tmp_path, "stage2"), _transfer(tmp_path, "stage2")
    for t in (ta, tb):
        t.compile(train.Adam(1e-3, clipnorm=1.0), loss=train.Huber(delta=1.0))
    before = {n: a.clone() for n, a in ta._named_tensors().items()}
    d = ta._to_device(x)
    pick = lambda idx: ({k: v[torch.from_numpy(idx).to(DEV)] for k, v in d.items()}, y[idx])
    batches = [np.arange(0, 4), np.arange(4, 8), np.arange(8, 12)]
    g = train.GraphedTrainStep(tb, *pick(batches[0]))
    for (_, a), (_, b) in zip(ta.trainable_variables(), tb.trainable_variables()):
        assert torch.equal(a, b)                                   # the capture left the weights untouched
    for idx in batches:
        la = ta.train_on_batch(*pick(idx))
        lb = g(*pick(idx)).clone()
        close(lb, la, 1e-5, "loss")
    assert ta.optimizer.iterations == tb.optimizer.iterations == 3
    for (n, a), (_, b) in zip(ta.trainable_variables(), tb.trainable_variables()):
        close(b, a, 1e-4, f"weights {n}")
    for what, t in (("eager", ta), ("captured", tb)):
        _check_invariant(what, t, before)


def test_rows_and_weights_survive_save_and_load(tmp_path):
    x, y = _fit_set()
    t = _transfer(tmp_path, "stage1")
    t.compile(train.Adam(1e-2, clipnorm=1.0), loss=train.Huber(delta=1.0))
    t.fit(x, y, epochs=1, batch_size=4, seed=0, graph=False)
    path = tmp_path / "transfer.keras"
    t.save(str(path))
    back = MM.load_model(str(path), device=DEV)
    assert back.atom_emb.trainable_rows == tuple(ATOM_ROWS) and back.bond_emb.trainable_rows == tuple(BOND_ROWS)
    assert [(l.name, l.trainable) for l in back.layers] == [(l.name, l.trainable) for l in t.layers]
    for n, a in t.state_dict().items():
        assert np.array_equal(back.state_dict()[n], a), n
    back.compile(train.Adam(1e-2, clipnorm=1.0), loss=train.Huber(delta=1.0))
    assert [n for n, _ in back.trainable_variables()][:2] == ["atom_embedding", "bond_embedding"]
    before = {n: a.clone() for n, a in back._named_tensors().items()}
    d = back._to_device(x)
    back.train_on_batch({k: v[:4] for k, v in d.items()}, y[:4])
    torch.cuda.synchronize()
    _check_invariant("a step after load_model", back, before, used_changed=False)
    assert not torch.equal(back.atom_emb.embeddings, before["atom_embedding"])
