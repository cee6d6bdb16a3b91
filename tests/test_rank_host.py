"""CPU: the host side of the rank cut - the entries (declared, exported, bound), the digit width in common.h, ops.py and
the library, the pass count, the workspace query, the status and text of every argument rule of the two entries (every
failing call returns before a launch; the stand-in pointers are never dereferenced), the argument rules of
screen_rank / screen_best_mask, and the references data.grid_rank / data.grid_best_mask against data.grid_top_k on
hand-made grids: ties across k, signed zeros, NaNs, both directions, masks, k at and above the competing count."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import ROOT
from ionic_mpnn_amd import _lib, data, ops

_BAD, _UNS, _WS = -1, -2, -4
_P = 0x100000   # a stand-in pointer (16-byte aligned)
ENTRIES = ("impnn_grid_rank_digit_bits", "impnn_grid_rank_passes", "impnn_grid_rank_workspace_bytes", "impnn_head_grid_rank",
           "impnn_transfer_head_grid_rank")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_the_entries_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "impnn.h").read_text(), flags=re.S)
    raw = C.CDLL(str(_lib.lib_path()))
    for n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in impnn.h"
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} is not bound"
    assert _lib.load().impnn_abi_version() == 3  # additions only


def test_the_digit_width_in_common_h_ops_and_the_library_is_equal():
    text = (ROOT / "ionic_mpnn_amd" / "csrc" / "common.h").read_text()
    in_header = int(re.search(r"constexpr int kRankDigitBits = (\d+);", text).group(1))
    assert in_header == ops.RANK_DIGIT_BITS == _lib.load().impnn_grid_rank_digit_bits() == 8
    assert ops.RANK_MAX_PAIRS == 2 ** 32 - 2


def test_rank_passes():
    lib = _lib.load()
    # four digits of the key, then one per byte that holds C * A - 1
    for (Cn, An), want in (((1, 1), 4), ((0, 7), 4), ((1, 2), 5), ((16, 16), 5), ((1, 257), 6), ((257, 1), 6), ((256, 256), 6),
                           ((65537, 1), 7), ((4096, 4096), 7), ((4096, 4097), 8), ((65535, 65537), 8), ((2, 2 ** 31 - 1), 8)):
        assert ops.rank_passes(Cn, An) == want == lib.impnn_grid_rank_passes(Cn, An), (Cn, An)
    for pairs in (2, 255, 256, 257, 65535, 65536, 65537, 2 ** 24, 2 ** 24 + 1):
        assert ops.rank_passes(1, pairs) == lib.impnn_grid_rank_passes(1, pairs) == 4 + ((pairs - 1).bit_length() + 7) // 8


# ---------------------------------------------------------------- the workspace query
def _need(lib, family=0, C_=100, A=100, nT=2, workgroups=0):
    n = C.c_size_t(0)
    return lib.impnn_grid_rank_workspace_bytes(family, C_, A, nT, workgroups, C.byref(n)), n.value


def test_workspace_query():
    lib = _lib.load()
    # a 32-byte state per plane and [workgroups][planes][256] counters; tiles of 16 x 64 and 8 x 32 pairs cap the workgroups
    assert _need(lib, 0, 100, 100, 2, 0) == (0, 2 * 32 + 4 * 14 * 2 * 256)
    assert _need(lib, 0, 100, 100, 2, 3) == (0, 2 * 32 + 4 * 3 * 2 * 256)
    assert _need(lib, 1, 20, 70, 0, 0) == (0, 32 + 4 * 9 * 256)
    assert _need(lib, 0, 4096, 4096, 4, 0) == (0, 4 * 32 + 4 * 256 * 4 * 256)
    assert _need(lib, 0, 0, 5, 1, 0) == (0, 0)
    sizes = [_need(lib, 0, 400, 400, 2, g)[1] for g in (1, 2, 3, 50, 174, 175, 176, 1000)]
    assert sizes == sorted(sizes) and sizes[-1] == sizes[-2] == sizes[-3], "monotone in workgroups, capped by the tiles"
    sizes = [_need(lib, 0, 400, 400, nT, 7)[1] for nT in (1, 2, 3, 4)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4, "monotone in nT"
    for kw, code in ((dict(family=2), _BAD), (dict(C_=-1), _BAD), (dict(workgroups=-1), _BAD), (dict(nT=5), _UNS),
                     (dict(C_=1 << 16, A=1 << 16), _UNS), (dict(C_=(1 << 16) + 1, A=(1 << 16) - 1), _UNS)):
        assert _need(lib, **kw)[0] == code, kw
    assert _need(lib, C_=2, A=(1 << 31) - 1)[0] == 0    # 2^32 - 2 pairs: the most
    assert lib.impnn_grid_rank_workspace_bytes(0, 4, 4, 1, 0, None) == _BAD


# ---------------------------------------------------------------- the argument rules of the two entries
def _head(lib, **kw):
    a = dict(kind=0, mc=_P, ma=_P, T=_P, w=_P, k=5, largest=0, where=None, v=_P, ci=_P, ai=_P, n=_P, words=None, ws=_P,
             ws_bytes=1 << 40, C=3, A=4, nT=2, D=32, F=32, Mx=20, workgroups=0)
    a.update(kw)
    rc = lib.impnn_head_grid_rank(a["kind"], a["mc"], a["ma"], a["T"], a["w"], a["k"], a["largest"], a["where"], a["v"], a["ci"],
                                  a["ai"], a["n"], a["words"], a["ws"], a["ws_bytes"], a["C"], a["A"], a["nT"], a["D"], a["F"],
                                  a["Mx"], a["workgroups"], None)
    return rc, lib.impnn_last_error_string().decode()


def _transfer(lib, **kw):
    a = dict(uc=_P, ua=_P, image=_P, image_floats=lib.impnn_transfer_grid_image_floats(), k=5, largest=0, where=None, v=_P,
             ci=_P, ai=_P, n=_P, words=None, ws=_P, ws_bytes=1 << 40, C=3, A=4, workgroups=0)
    a.update(kw)
    rc = lib.impnn_transfer_head_grid_rank(a["uc"], a["ua"], a["image"], a["image_floats"], a["k"], a["largest"], a["where"],
                                           a["v"], a["ci"], a["ai"], a["n"], a["words"], a["ws"], a["ws_bytes"], a["C"], a["A"],
                                           a["workgroups"], None)
    return rc, lib.impnn_last_error_string().decode()


BIG = dict(C=1 << 16, A=1 << 16)
NAMES = {"_head": "impnn_head_grid_rank: ", "_transfer": "impnn_transfer_head_grid_rank: "}


def test_entries_refuse_bad_requests_before_a_launch():
    lib = _lib.load()
    for call in (_head, _transfer):
        for kw, code, text in ((dict(C=-1), _BAD, "bad shape"), (dict(workgroups=-1), _BAD, "bad shape"),
                               (dict(v=None), _BAD, "null pointer"), (dict(n=None), _BAD, "null pointer"),
                               (dict(ws=None), _BAD, "null pointer"), (dict(ws=_P + 4), _BAD, "8-byte aligned"),
                               (dict(n=_P + 4), _BAD, "8-byte aligned"), (dict(where=_P + 2), _BAD, "4-byte aligned"),
                               (dict(words=_P + 2), _BAD, "4-byte aligned"),
                               (dict(k=0), _BAD, "k=0 must be at least 1"), (dict(k=-3), _BAD, "k=-3 must be at least 1"),
                               (BIG, _UNS, "4294967296 pairs (<= 2^32 - 2 per call)"),
                               (dict(C=(1 << 16) + 1, A=(1 << 16) - 1), _UNS, "4294967295 pairs (<= 2^32 - 2 per call)"),
                               (dict(ws_bytes=8), _WS, "workspace of 8 bytes is too small")):
            rc, msg = call(lib, **kw)
            assert rc == code and text in msg and msg.startswith(NAMES[call.__name__]), (call.__name__, kw, rc, msg)
        assert call(lib, C=0)[0] == 0 and call(lib, A=0, v=None, ws=None, k=0)[0] == 0   # zero work: nothing touched
        # the order of the rules: a null pointer before k, k before the pair count, the pair count before the workspace
        assert "null pointer" in call(lib, v=None, k=0)[1]
        assert "must be at least 1" in call(lib, k=0, **BIG)[1]
        assert "pairs" in call(lib, ws_bytes=8, **BIG)[1]
        assert call(lib, k=1 << 40, ws_bytes=8)[0] == _WS     # k is a 64-bit integer and has no upper limit
    for kw, code, text in ((dict(kind=2), _BAD, "kind must be"), (dict(D=0), _BAD, "bad shape"), (dict(nT=0), _BAD, "needs nT >= 1"),
                           (dict(kind=1, nT=1), _BAD, "nT must be 0"), (dict(T=None), _BAD, "null pointer"),
                           (dict(kind=1, nT=0), _BAD, "takes no temperatures"),
                           (dict(nT=5), _UNS, "nT=5 temperatures (<= 4 per selecting call)"), (dict(Mx=65), _UNS, "Mx=65"),
                           (dict(D=129), _UNS, "D=129")):
        rc, msg = _head(lib, **kw)
        assert rc == code and text in msg, (kw, rc, msg)
    assert "kind must be" in _head(lib, kind=2, C=-1)[1] and "bad shape" in _head(lib, C=-1, v=None)[1]
    assert "pairs" in _head(lib, nT=5, **BIG)[1] and "nT=5" in _head(lib, nT=5, ws_bytes=8)[1]
    assert "too small" in _head(lib, ws_bytes=8, Mx=65)[1], "the workspace size before the widths"
    assert _transfer(lib, image_floats=16)[0] == _WS and _transfer(lib, uc=_P + 4)[0] == _BAD
    # the exact size is enough to pass the size rule (the next failure is none: it would launch, so stop at the query)
    assert _head(lib, ws_bytes=_need(lib, 0, 3, 4, 2, 0)[1] - 1)[0] == _WS
    assert _transfer(lib, ws_bytes=_need(lib, 1, 3, 4, 0, 0)[1] - 1)[0] == _WS


# ---------------------------------------------------------------- the references against grid_top_k
def tricky(shape, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(-3, 4, size=shape).astype(np.float32)      # few distinct values: runs of ties across every k
    g.reshape(-1)[rng.choice(g.size, g.size // 6, replace=False)] = np.nan
    flat = g.reshape(-1)
    zeros = np.flatnonzero(flat == 0)
    flat[zeros[::2]] = -0.0                                       # both zeros, in an order that is not the index order
    neg_nan = np.array([0xFFC00001], np.uint32).view(np.float32)[0]
    flat[np.flatnonzero(np.isnan(flat))[::3]] = neg_nan          # NaNs of another sign and payload
    return g


def check(g, k, largest, where_b=None, where=None):
    wh = where if where is not None else where_b
    top = data.grid_top_k(g, k, largest, where=wh)
    cut = data.grid_rank(g, k, largest, where=wh)
    best = data.grid_best_mask(g, k, largest, where=wh)
    competing = g.shape[0] * g.shape[1] if where_b is None else int(where_b.sum())
    planes = g.shape[2] if g.ndim == 3 else 1
    assert best.dtype == np.bool_ and best.shape == g.shape
    v, ci, ai, n = (np.asarray(x).reshape(planes) for x in cut)
    assert v.dtype == np.float32 and ci.dtype == ai.dtype == n.dtype == np.int64
    assert (np.ndim(cut.values) == 0) == (g.ndim == 2)
    assert (n == competing).all()
    tv, tc, ta = (np.asarray(x).reshape(planes, -1) for x in top)
    for t in range(planes):
        if k <= competing:      # element k - 1 of the top k
            assert bits(v[t]) == bits(tv[t, k - 1]) and ci[t] == tc[t, k - 1] and ai[t] == ta[t, k - 1], (k, largest, t)
        else:
            assert bits(v[t]) == 0x7FC00000 and ci[t] == -1 and ai[t] == -1, (k, largest, t)
        want = np.zeros(g.shape[:2], bool)
        want[tc[t], ta[t]] = True                                 # the scatter of the top k
        plane = best[:, :, t] if g.ndim == 3 else best
        assert np.array_equal(plane, want) and plane.sum() == min(k, competing), (k, largest, t)
        if where_b is not None:
            assert not (plane & ~where_b).any()


@pytest.mark.parametrize("shape", [(5, 7), (5, 7, 3), (1, 1), (6, 1, 2)], ids=str)
def test_references_are_the_order_on_hand_made_grids(shape):
    g = tricky(shape, 7)
    assert np.isnan(g).any() or g.size < 6
    n = shape[0] * shape[1]
    half = np.random.default_rng(3).random(shape[:2]) < 0.5
    for largest in (False, True):
        for k in sorted({1, 2, max(n // 2, 1), max(n - 1, 1), n, n + 5}):
            check(g, k, largest)
            check(g, k, largest, half)
            check(g, k, largest, half, where=data.PairMask.from_bool(half))
            check(g, k, largest, np.zeros(shape[:2], bool))       # an empty mask: count 0, nothing set, NaN / -1 / -1
            check(g, k, largest, np.ones(shape[:2], bool))


def test_ties_zeros_and_nans_by_hand():
    nan = np.float32(np.nan)
    g = np.array([[1.0, 0.0, -0.0, 1.0],
                  [nan, 2.0, 2.0, nan],
                  [1.0, 0.0, -0.0, 1.0]], np.float32)
    # ascending: -0.0 (0,2) (2,2) | +0.0 (0,1) (2,1) | 1.0 (0,0) (0,3) (2,0) (2,3) | 2.0 (1,1) (1,2) | NaN (1,0) (1,3)
    order = [(0, 2), (2, 2), (0, 1), (2, 1), (0, 0), (0, 3), (2, 0), (2, 3), (1, 1), (1, 2), (1, 0), (1, 3)]
    for k, (i, j) in enumerate(order, 1):
        cut = data.grid_rank(g, k)
        assert (cut.cation, cut.anion, cut.count) == (i, j, 12), k
        assert bits(cut.values) == (0x7FC00000 if k > 10 else bits(g[i, j])), k
        best = data.grid_best_mask(g, k)
        assert sorted(zip(*np.nonzero(best))) == sorted(order[:k]), "a run of equal values that straddles k is cut by index"
    cut = data.grid_rank(g, 13)
    assert (cut.cation, cut.anion, cut.count) == (-1, -1, 12) and bits(cut.values) == 0x7FC00000
    assert data.grid_best_mask(g, 13).all()
    down = [(1, 1), (1, 2), (0, 0), (0, 3), (2, 0), (2, 3), (0, 1), (2, 1), (0, 2), (2, 2), (1, 0), (1, 3)]   # NaN last here too
    for k, (i, j) in enumerate(down, 1):
        cut = data.grid_rank(g, k, largest=True)
        assert (cut.cation, cut.anion) == (i, j), k
    where = np.zeros((3, 4), bool)
    where[1] = True
    cut = data.grid_rank(g, 3, where=where)
    assert (cut.cation, cut.anion, cut.count) == (1, 0, 4) and bits(cut.values) == 0x7FC00000


def test_bad_arguments_of_the_references():
    g = np.zeros((3, 4), np.float32)
    for fn in (data.grid_rank, data.grid_best_mask):
        with pytest.raises(ValueError, match="grid must be"):
            fn(np.zeros(3, np.float32), 1)
        with pytest.raises(ValueError, match="k must be >= 1"):
            fn(g, 0)
        with pytest.raises(ValueError, match="where must be a bool array or PairMask of shape"):
            fn(g, 1, where=np.ones((4, 3), bool))
        with pytest.raises(ValueError, match="2-D PairMask"):
            fn(np.zeros((3, 4, 2), np.float32), 1, where=data.PairMask.from_bool(np.ones((3, 4, 2), bool)))
    assert data.grid_best_mask(np.zeros((0, 4), np.float32), 2).shape == (0, 4)
    assert data.grid_rank(np.zeros((0, 4, 2), np.float32), 2).count.tolist() == [0, 0]


# ---------------------------------------------------------------- the argument rules of the two screens
class _NoEncoder:
    """MPNNModel's argument rules run before the first use of the device: a model object without one."""

    def __new__(cls, kind):
        from ionic_mpnn_amd.model import MPNNModel
        m = object.__new__(MPNNModel)
        m.kind = kind
        return m


@pytest.mark.parametrize("screen", ["screen_rank", "screen_best_mask"])
def test_the_screens_refuse_bad_arguments_before_any_work(screen):
    ions = lambda n: {"atom": np.zeros((n, 4), np.int32), "bond": np.zeros((n, 6), np.int32),
                      "connectivity": np.zeros((n, 6, 2), np.int32)}
    cat, an = ions(3), ions(4)
    v = getattr(_NoEncoder("viscosity"), screen)
    mp = getattr(_NoEncoder("melting_point"), screen)
    with pytest.raises(KeyError, match="temperature"):
        v(cat, an, k=2)
    with pytest.raises(ValueError, match=f"{screen} needs both cations and anions"):
        mp(cat, None, k=2)
    with pytest.raises(ValueError, match="k must be >= 1"):
        mp(cat, an, k=0)
    with pytest.raises(ValueError, match="at least one value"):
        v(cat, an, temperatures=[], k=2)
    with pytest.raises(TypeError, match="data.PairMask"):
        mp(cat, an, k=2, where=np.ones((3, 4), bool))
    with pytest.raises(ValueError, match="2-D mask"):
        v(cat, an, temperatures=[300.0], k=2, where=data.PairMask.from_bool(np.ones((3, 4, 1), bool)))
    with pytest.raises(ValueError, match="where has shape"):
        mp(cat, an, k=2, where=data.PairMask.from_bool(np.ones((4, 3), bool)))

    class Many:   # more pairs than an entry's 32-bit pair index holds, without the arrays
        def __init__(self, n):
            self.n = n

        def __getitem__(self, key):
            return self

        def __len__(self):
            return self.n

    with pytest.raises(ValueError, match=r"at most 2\^32 - 2"):
        mp(Many(1 << 16), Many(1 << 16), k=2)
