"""The family-agnostic screening operations of ops.py (grid_values, grid_topk, grid_partners, grid_rank, grid_mask on a
GridOperands) through every branch of the one kernel launcher (csrc/grid_device.h, launch_grid_family): head family
viscosity <0,0>, melting point <1,32> and <1,64>, transfer family; the plain and the masked packs.

Everything is exact: a value is computed by the tile code of the materialising kernel, so values are compared by their
uint32 view, indices, counts and mask words for equality, against the host references of data.py on the materialised
grid of the same operands and against the named wrappers.  No tolerance appears.

Shapes: the smallest 2 x 2 tile grid with ragged edges, C = 17, A = 65 for the head family (tile 16 x 64), C = 9, A = 33
for the transfer family (tile 8 x 32); the ``where`` mask clears the whole first tile, which its workgroup passes over."""
import numpy as np
import pytest
import torch

from ionic_mpnn_amd import data, ops

from test_gpu_grid import bits
from test_gpu_screen import T_MAX, head_case, transfer_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
K, M = 5, 2
# name -> (family, kind, (atom_dim, fp_size, mixing_size), (C, A), (tile C, tile A))
CASES = {"viscosity-nT2": (0, "viscosity", (32, 32, 20), (17, 65), (16, 64)),
         "melting-Mx20": (0, "melting_point", (32, 32, 20), (17, 65), (16, 64)),
         "melting-Mx40": (0, "melting_point", (32, 32, 40), (17, 65), (16, 64)),
         "transfer": (1, None, (32, 32, 20), (9, 33), (8, 32))}
_cache = {}


def case(name):
    """-> (GridOperands, the named wrappers' leading arguments, the materialised grid on the host, the where mask as a
    bool array); built once per combination and left unchanged."""
    if name not in _cache:
        family, kind, dims, shape, tile = CASES[name]
        if family == 0:
            wp, mc, ma = head_case(kind, dims, shape)
            T = torch.from_numpy(T_MAX[:2]).to(DEV) if kind == "viscosity" else None
            args = (kind, mc, ma, T, wp, dims[1], dims[2])
            g = ops.head_grid_operands(*args)
            assert (g.family, g.kind, g.C, g.A, g.nT, g.D) == (0, ops.HEAD_KINDS[kind], *shape, 2 if T is not None else 0, dims[0])
        else:
            args = transfer_case(dims, shape)
            g = ops.transfer_grid_operands(*args)
            assert (g.family, g.kind, g.C, g.A, g.nT, g.D) == (1, 1, *shape, 0, None)
        where = np.ones(shape, np.bool_)
        where[:tile[0], :tile[1]] = False
        _cache[name] = g, args, ops.grid_values(g).cpu().numpy(), where
    return _cache[name]


def named(family, op):
    return getattr(ops, ("head_grid", "transfer_head_grid")[family] + op)


def same_tensors(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        if a is None or b is None:
            assert a is None and b is None, f"{what}: output {i}"
        else:
            assert a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                      b.view(torch.int32) if b.dtype == torch.float32 else b), f"{what}: output {i}"


@pytest.mark.parametrize("name", list(CASES))
def test_values_and_mask(name):
    g, args, grid, _ = case(name)
    family = g.family
    want = named(family, "")(*args)
    assert np.array_equal(bits(grid), bits(want.cpu().numpy())) and grid.shape == ((g.C, g.A, g.nT) if g.kind == 0 else (g.C, g.A))
    if g.kind == 0:
        out, params = ops.grid_values(g, return_params=True)
        w_out, w_params = named(family, "")(*args, return_params=True)
        same_tensors((out, params), (w_out, w_params), f"{name}: values with params")
        assert np.array_equal(bits(out.cpu().numpy()), bits(grid))
    else:
        with pytest.raises(ValueError, match="return_params: only the viscosity head has VFT parameters"):
            ops.grid_values(g, return_params=True)
    # narrowing without validating again: rows and temperatures of the same grid, the same bits
    rows = ops.grid_values(g.rows(3, g.C)).cpu().numpy()
    assert np.array_equal(bits(rows), bits(grid[3:]))
    if g.kind == 0:
        assert np.array_equal(bits(ops.grid_values(g.temperatures(1, 2)).cpu().numpy()), bits(grid[:, :, 1:2]))
    # the bound comparison, packed: bounds from the grid itself so that both sides of either bound occur
    lo, hi = np.sort(grid.reshape(-1))[[grid.size // 4, 3 * grid.size // 4]]
    words = ops.grid_mask(g, lo, hi)
    ref = data.PairMask.from_bool((grid >= lo) & (grid <= hi))
    assert words.dtype == torch.int32 and np.array_equal(words.cpu().numpy().view(np.uint32).reshape(-1), ref._host_words().reshape(-1))
    assert 0 < int(np.sum(ref.count())) < grid.size  # both outcomes of the comparison occur
    same_tensors((words,), (named(family, "_mask")(*args, lo, hi),), f"{name}: mask")


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "where"])
@pytest.mark.parametrize("name", list(CASES))
def test_selecting_operations(name, masked):
    g, args, grid, where_b = case(name)
    family, planes = g.family, max(g.nT, 1)
    where_b = where_b if masked else None
    where = data.PairMask.from_bool(where_b, device=DEV).words if masked else None
    rows = lambda x: np.asarray(x).reshape((planes,) + np.asarray(x).shape[(1 if g.kind == 0 else 0):])  # a plane axis in front

    # top-k
    got = ops.grid_topk(g, K, where=where)
    v, ci, ai = (x.cpu().numpy() for x in got)
    want = data.grid_top_k(grid, K, False, where=where_b)
    assert np.array_equal(bits(v), bits(rows(want.values))), f"{name}: top-k values"
    assert np.array_equal(ci, rows(want.cation)) and np.array_equal(ai, rows(want.anion)), f"{name}: top-k indices"
    same_tensors(got, named(family, "_topk")(*args, K, where=where), f"{name}: top-k")

    # partners
    got = ops.grid_partners(g, M, where=where)
    cv, cp, av, ap = (x.cpu().numpy() for x in got)
    by_c, by_a = data.grid_best_partners(grid, M, False, where=where_b)
    assert np.array_equal(bits(cv), bits(rows(by_c.values))) and np.array_equal(cp, rows(by_c.partner)), f"{name}: by cation"
    assert np.array_equal(bits(av), bits(rows(by_a.values))) and np.array_equal(ap, rows(by_a.partner)), f"{name}: by anion"
    if masked:  # a cation of the cleared tile keeps the partners of the ragged tile beside it alone
        ta = CASES[name][4][1]
        assert (cp[:, 0, :g.A - ta] >= ta).all() and (cp[:, 0, g.A - ta:] == -1).all()
    same_tensors(got, named(family, "_partners")(*args, M, where=where), f"{name}: partners")

    # the rank cut and the best-k mask
    got = ops.grid_rank(g, K, where=where, mask=True)
    v, ci, ai, n, words = (x.cpu().numpy() for x in got)
    want = data.grid_rank(grid, K, False, where=where_b)
    assert np.array_equal(bits(v), bits(np.atleast_1d(want.values))), f"{name}: rank value"
    assert np.array_equal(ci, np.atleast_1d(want.cation)) and np.array_equal(ai, np.atleast_1d(want.anion)), f"{name}: rank indices"
    assert np.array_equal(n, np.atleast_1d(want.count)), f"{name}: rank count"
    ref = data.PairMask.from_bool(data.grid_best_mask(grid, K, False, where=where_b))
    assert np.array_equal(words.view(np.uint32).reshape(-1), ref._host_words().reshape(-1)), f"{name}: best-k mask"
    assert np.asarray(ref.count()).tolist() in ([K] * planes, K)
    same_tensors(got, named(family, "_rank")(*args, K, where=where, mask=True), f"{name}: rank")
    assert ops.grid_rank(g, K, where=where)[4] is None


# the five named wrappers of a family, with the arguments that follow the operands
WRAPPERS = [("", ()), ("_topk", (K,)), ("_partners", (M,)), ("_rank", (K,)), ("_mask", (0.0, 1.0))]


@pytest.mark.parametrize("fault", ["rows", "length", "temperatures"])
def test_the_wrappers_of_a_family_share_their_operand_errors(fault):
    """A bad mixing-row width, a wrong packed or image length, temperatures on a melting-point head: one ValueError text
    from all five wrappers of a family, raised before any launch."""
    _, (kind, mc, ma, T, wp, F, Mx), _, _ = case("melting-Mx20")
    _, (uc, ua, image), _, _ = case("transfer")
    if fault == "rows":
        head, transfer = (kind, mc[:, :Mx - 1], ma, T, wp, F, Mx), (uc[:, :255], ua, image)
        texts = (f"mixing rows must be (C,{Mx}) and (A,{Mx}), got (17, {Mx - 1}) and (65, {Mx})",
                 "u rows must be (C,256) and (A,256), got (9, 255) and (33, 256)")
    elif fault == "length":
        head, transfer = (kind, mc, ma, T, wp[:-1], F, Mx), (uc, ua, image[:-1])
        texts = ("packed head weights have the wrong length", "the prepared image has the wrong length")
    else:
        head, transfer = (kind, mc, ma, torch.from_numpy(T_MAX[:1]).to(DEV), wp, F, Mx), None
        texts = ("the melting-point grid takes no temperatures", None)
    for family, args, text in ((0, head, texts[0]), (1, transfer, texts[1])):
        if args is None:
            continue
        seen = set()
        for op, extra in WRAPPERS:
            with pytest.raises(ValueError) as e:
                named(family, op)(*args, *extra)
            seen.add(str(e.value))
        assert seen == {text}
