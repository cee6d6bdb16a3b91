"""CPU: the host side of the applicability domain (include/impnn.h, impnn_domain_*): data.grid_domain on a grid worked
out by hand, DomainReference.radius, the de-duplication and order of fit_domain's pairs (data.unique_pairs), the
argument rules of ops.domain_* that fire before any library call, the status codes of the three C entries (every failing
call returns before a launch; no pointer is dereferenced), and the build list."""
import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, build, data, ops

_BAD, _UNS = -1, -2


def test_grid_domain_on_a_hand_written_grid():
    """2 cations x 3 anions, Mx = 2, R = 3.  z = [[(0,0), (1,0), (0,2)], [(1,1), (2,1), (1,3)]]; the reference rows are
    (1,1), (1,1) again and (0,2): two exact hits, and the lower index of the identical rows wherever (1,1) is nearest."""
    mc = np.array([[0, 0], [1, 1]], np.float32)
    ma = np.array([[0, 0], [1, 0], [0, 2]], np.float32)
    ref = np.array([[1, 1], [1, 1], [0, 2]], np.float32)
    distance, nearest = data.grid_domain(mc, ma, ref)
    assert distance.dtype == np.float64 and distance.shape == nearest.shape == (2, 3)
    r2 = np.sqrt(2.0)
    assert np.array_equal(distance, np.array([[r2, 1.0, 0.0], [0.0, 1.0, r2]]))
    assert np.array_equal(nearest, np.array([[0, 0, 2], [0, 0, 2]]))
    # z is the float32 sum: 1 + 2^-24 rounds to 1 before anything is widened, so the hit on (1, 1) stays exact
    tiny = np.array([[2.0 ** -24, 2.0 ** -24]], np.float32)
    d, n = data.grid_domain(np.array([[1, 1]], np.float32), tiny, ref)
    assert d[0, 0] == 0.0 and n[0, 0] == 0
    # a NaN row: no reference row ever wins
    d, n = data.grid_domain(np.array([[np.nan, 0]], np.float32), ma, ref)
    assert np.isnan(d).all() and (n == -1).all()
    with pytest.raises(ValueError, match="R must be at least 1"):
        data.grid_domain(mc, ma, np.zeros((0, 2), np.float32))
    with pytest.raises(ValueError, match="expected"):
        data.grid_domain(mc, ma, np.zeros((3, 3), np.float32))


def test_radius_is_the_quantile_of_the_self_distances():
    rows = torch.zeros(5, 3)
    ref = data.DomainReference(rows, np.arange(5), np.arange(5), np.array([4.0, 0.0, 2.0, 1.0, 3.0], np.float32))
    assert len(ref) == 5 and ref.width == 3 and ref.cation.dtype == np.int32 and ref.self_distance.dtype == np.float32
    assert ref.radius(0) == np.float32(0.0) and ref.radius(1) == np.float32(4.0)
    assert ref.radius(0.95) == np.float32(3.8) and ref.radius() == ref.radius(0.95)   # linear interpolation: 0.95 * 4
    assert isinstance(ref.radius(0.5), np.float32) and ref.radius(0.5) == np.float32(2.0)
    # NaNs do not count ...
    some = data.DomainReference(rows, np.arange(5), np.arange(5), np.array([np.nan, 1.0, np.nan, 3.0, 2.0], np.float32))
    assert some.radius(1) == np.float32(3.0) and some.radius(0.5) == np.float32(2.0)
    # ... and a set of one pair has none
    one = data.DomainReference(torch.zeros(1, 3), [0], [0], [np.nan])
    with pytest.raises(ValueError, match="no self distance"):
        one.radius()
    with pytest.raises(ValueError, match="one entry per reference row"):
        data.DomainReference(rows, np.arange(4), np.arange(5), np.zeros(5))
    with pytest.raises(ValueError, match="R >= 1"):
        data.DomainReference(torch.zeros(0, 3), [], [], [])


def test_unique_pairs_lists_a_pair_once_in_cation_anion_order():
    """What fit_domain does with the training pairs before anything runs on the GPU."""
    ci = np.array([3, 1, 3, 1, 0, 3, 1], np.int64)
    ai = np.array([2, 5, 2, 4, 0, 1, 5], np.int64)
    c, a = data.unique_pairs(ci, ai, 4, 6)
    assert c.dtype == a.dtype == np.int32
    assert list(zip(c.tolist(), a.tolist())) == [(0, 0), (1, 4), (1, 5), (3, 1), (3, 2)]
    # the form data.unique_ions produces: a pair at many temperatures is one pair
    rec = lambda x, y: {"cation": {"atom_ids": [x], "bond_ids": [], "edge_indices": []},
                        "anion": {"atom_ids": [y], "bond_ids": [], "edge_indices": []}}
    records = [rec(7, 9), rec(8, 9), rec(7, 9), rec(7, 9), rec(8, 5)]
    _, _, cat_index, an_index = data.unique_ions(records)
    c, a = data.unique_pairs(cat_index, an_index)
    assert list(zip(c.tolist(), a.tolist())) == [(0, 0), (1, 0), (1, 1)]
    c, a = data.unique_pairs([], [])
    assert c.shape == a.shape == (0,)
    with pytest.raises(ValueError, match="one length"):
        data.unique_pairs([1, 2], [1])
    with pytest.raises(ValueError, match="cation_index is out of range"):
        data.unique_pairs([4], [0], 4, 6)
    with pytest.raises(ValueError, match="anion_index is out of range"):
        data.unique_pairs([0], [-1], 4, 6)
    with pytest.raises(TypeError, match="integer"):
        data.unique_pairs([0.5], [1.0])


def test_ops_rules_fire_before_any_library_call():
    """Every rule but the last is met on CPU tensors: the device is judged after the shapes."""
    f = lambda *shape: torch.zeros(*shape)
    cases = [
        (lambda: ops.domain_grid(f(3, 20), f(4, 20), f(20)), ValueError, "ref must be 2-D"),
        (lambda: ops.domain_grid(f(3, 20, 1), f(4, 20), f(5, 20)), ValueError, "mix_cat must be 2-D"),
        (lambda: ops.domain_rows(f(20), f(5, 20)), ValueError, "z must be 2-D"),
        (lambda: ops.domain_grid(f(3, 20), f(4, 19), f(5, 20)), ValueError, "mix_an has width 19"),
        (lambda: ops.domain_grid_mask(f(3, 20), f(4, 20), f(5, 32), 0.0, 1.0), ValueError, "mix_cat has width 20"),
        (lambda: ops.domain_rows(f(3, 8), f(5, 20)), ValueError, "z has width 8"),
        (lambda: ops.domain_grid(f(3, 65), f(4, 65), f(5, 65)), ValueError, "Mx=65"),
        (lambda: ops.domain_rows(f(3, 65), f(5, 65)), ValueError, "Mx=65"),
        (lambda: ops.domain_grid(f(3, 0), f(4, 0), f(5, 0)), ValueError, "Mx=0"),
        (lambda: ops.domain_grid(f(3, 20), f(4, 20), f(0, 20)), ValueError, "R must be at least 1"),
        (lambda: ops.domain_rows(f(3, 20), f(0, 20)), ValueError, "R must be at least 1"),
        (lambda: ops.domain_grid_mask(f(3, 20), f(4, 20), f(5, 20), float("nan"), 1.0), ValueError, "bound is NaN"),
        (lambda: ops.domain_grid_mask(f(3, 20), f(4, 20), f(5, 20), 0.0, float("nan")), ValueError, "bound is NaN"),
        (lambda: ops.domain_rows(f(4, 20), f(5, 20), exclude_self=True), ValueError, "exclude_self"),
        (lambda: ops.domain_grid(f(3, 20).double(), f(4, 20), f(5, 20)), TypeError, "mix_cat must be float32"),
        (lambda: ops.domain_rows(np.zeros((3, 20), np.float32), f(5, 20)), TypeError, "expected torch.Tensor"),
        # CPU tensors that are otherwise in order
        (lambda: ops.domain_grid(f(3, 20), f(4, 20), f(5, 20)), RuntimeError, "no CPU fallback"),
        (lambda: ops.domain_grid_mask(f(3, 20), f(4, 20), f(5, 20), 0.0, float("inf")), RuntimeError, "no CPU fallback"),
        (lambda: ops.domain_rows(f(5, 20), f(5, 20), exclude_self=True), RuntimeError, "no CPU fallback"),
    ]
    for call, error, text in cases:
        with pytest.raises(error, match=text):
            call()


def test_c_entries_refuse_bad_arguments_in_order():
    """Shape (sizes, Mx >= 1, R >= 1, exclude_self with Q != R, a NaN bound), the width limit, zero work, null pointers."""
    lib = _lib.load()
    assert lib.impnn_domain_reference_chunk() >= 1
    P = 0x100000  # a stand-in that is never dereferenced
    nan, inf = float("nan"), float("inf")
    grid = lambda C=3, A=4, R=5, Mx=20, p=P, near=P: lib.impnn_domain_grid(p, p, p, p, near, C, A, R, Mx, None)
    mask = lambda lo=0.0, hi=inf, C=3, A=4, R=5, Mx=20, p=P: lib.impnn_domain_grid_mask(p, p, p, lo, hi, p, C, A, R, Mx, None)
    rows = lambda ex=0, Q=5, R=5, Mx=20, p=P: lib.impnn_domain_rows(p, p, ex, p, P, Q, R, Mx, None)
    msg = lib.impnn_last_error_string
    for call in (grid, mask):
        assert call(C=-1) == _BAD and b"bad shape" in msg()
        assert call(A=-1, p=None) == _BAD and b"bad shape" in msg()
        assert call(Mx=0) == _BAD and b"bad shape" in msg()
        assert call(R=0) == _BAD and b"R=0" in msg()
        assert call(R=0, Mx=65) == _BAD and b"R=0" in msg()           # shape before the width limit
        assert call(Mx=65) == _UNS and b"Mx=65 (<= 64)" in msg()
        assert call(Mx=65, C=0, p=None) == _UNS                        # ... which comes before zero work
        assert call(C=0, p=None) == 0 and call(A=0, p=None) == 0       # zero work: nothing looked at
        assert call(p=None) == _BAD and b"null pointer" in msg()
    assert mask(lo=nan) == _BAD and b"NaN" in msg()
    assert mask(hi=nan, C=0, p=None) == _BAD and b"NaN" in msg()       # a NaN bound is a shape rule
    assert mask(lo=nan, R=0) == _BAD and b"R=0" in msg()
    assert rows(Q=-1) == _BAD and b"bad shape" in msg()
    assert rows(Mx=0) == _BAD and rows(R=0) == _BAD and b"R=0" in msg()
    assert rows(ex=1, Q=4) == _BAD and b"Q == R" in msg()
    assert rows(ex=1, Q=0, p=None) == _BAD and b"Q == R" in msg()
    assert rows(Mx=65) == _UNS and b"Mx=65" in msg()
    assert rows(Q=0, p=None) == 0
    assert rows(p=None) == _BAD and b"null pointer" in msg()
    assert rows(ex=1, p=None) == _BAD and b"null pointer" in msg()


def test_the_kernels_are_in_the_build():
    assert "grid_domain.hip" in build.SOURCES and (build.CSRC / "grid_domain.hip").exists()
    assert {"impnn_domain_grid", "impnn_domain_grid_mask", "impnn_domain_rows"} <= set(_lib.SIGNATURES)
