"""The host reference of the chunk records' run order (tests/run_order_ref.py) against its own properties, on the
compositions the GPU test uses - and the property checker against mutated tables, which it must refuse: a checker that
passes everything is not a check.  No device."""
import numpy as np
import pytest

import plan_cases as PC
import run_order_ref as RO

NAMES = tuple(RO.COMPOSITIONS)


def _chunks(case):
    """Next-fit chunks of <= 256 virtual rows over each ion (one share: the cut differs from a plan's, the properties of a
    chunk's table do not depend on it)."""
    ecap = 640 if case.E > 512 else 512
    out = []
    for g, p in enumerate(PC.IONS):
        ids, bond, conn = (case.inp[f"{p}_{k}"] for k in ("atom", "bond", "connectivity"))
        rows = PC.kept_rows(ids, conn, bond, case.Vb)
        edges = PC.valid_edges(conn, bond, case.N, case.Vb).sum(axis=1)
        vr = PC.virtual_rows(rows, edges, ecap, 1)
        m = 0
        while m < vr.size:
            e = m + 1
            while e < vr.size and vr[m:e + 1].sum() <= PC.RCAP:
                e += 1
            out.append((g, m, e - m))
            m = e
    return out


@pytest.mark.parametrize("name", NAMES)
def test_reference_tables_hold_their_properties(name):
    case = RO.COMPOSITIONS[name]()
    lens, gmaxes, nruns = set(), set(), set()
    for (g, m0, M) in _chunks(case):
        t = RO.chunk_run_table(case, g, m0, M)
        RO.check_run_table(t.hist, t.nrun, t.runs, t.grp_type, t.grp_edges, what=f"{name}: ion {g}, molecules {m0} .. {m0 + M - 1}")
        assert t.nrun <= np.count_nonzero(t.hist) + RO.RUN_TARGET, "more runs than the record's run table holds"
        lens |= set(np.diff(t.runs).tolist())
        gmaxes.add(t.gmax)
        nruns.add(t.nrun)
    print(f"{name}: gmax {sorted(gmaxes)}, run lengths {sorted(lens)}, runs per chunk {min(nruns)} .. {max(nruns)}")
    # what each composition was built for
    if name in ("three_long", "big_record"):
        assert max(gmaxes) >= 3 and len(lens) >= 2, f"{name}: no type is cut with a remainder"
    if name == "big_record":
        assert min(gmaxes) >= 5
    if name == "empty_between":
        assert 0 in nruns and max(nruns) > 0
    if name == "one_type":
        assert all(np.count_nonzero(RO.chunk_type_histogram(case, g, m0, M)) == 1 for (g, m0, M) in _chunks(case))
    if name == "last_lane_types":
        assert all((RO.chunk_type_histogram(case, g, m0, M)[252:] > 0).all() for (g, m0, M) in _chunks(case))
    if name == "equal_counts":
        assert all(len(set(RO.chunk_type_histogram(case, g, m0, M).tolist())) == 1 for (g, m0, M) in _chunks(case))


def _cut_chunk():
    """A chunk in which a type is cut into full pieces and a remainder."""
    case = RO.COMPOSITIONS["three_long"]()
    t = RO.chunk_run_table(case, 0, 0, 6)
    assert t.gmax >= 3 and any(((int(n) + 3) // 4) % t.gmax and ((int(n) + 3) // 4) > t.gmax for n in t.hist)
    return t


def _rebuild(t, order):
    """The tables of `t` with its runs laid out in `order`."""
    runs, gt, ge = [0], [], []
    for i in order:
        g0, g1 = int(t.runs[i]), int(t.runs[i + 1])
        gt += t.grp_type[g0:g1].tolist()
        ge += t.grp_edges[g0:g1].tolist()
        runs.append(len(gt))
    return np.array(runs), np.array(gt), np.array(ge)


def test_checker_passes_the_unmutated_table():
    t = _cut_chunk()
    RO.check_run_table(t.hist, t.nrun, *_rebuild(t, range(t.nrun)))


def test_checker_refuses_two_runs_swapped():
    t = _cut_chunk()
    lens = np.diff(t.runs)
    # a long and a short run: the order of lengths breaks; two runs of one length and different types: the type order
    i = int(np.nonzero(np.diff(lens) < 0)[0][0])
    same = [k for k in range(t.nrun - 1) if lens[k] == lens[k + 1] and t.run_type[k] != t.run_type[k + 1]]
    for a in [i] + same[:1]:
        order = list(range(t.nrun))
        order[a], order[a + 1] = order[a + 1], order[a]
        with pytest.raises(AssertionError):
            RO.check_run_table(t.hist, t.nrun, *_rebuild(t, order))


def test_checker_refuses_a_run_one_group_short():
    t = _cut_chunk()
    runs = t.runs.copy()
    runs[2:] -= 1   # run 1 loses its last group; the tables behind it move up
    keep = np.ones(t.grp_type.size, bool)
    keep[t.runs[2] - 1] = False
    with pytest.raises(AssertionError):
        RO.check_run_table(t.hist, t.nrun, runs, t.grp_type[keep], t.grp_edges[keep])
    with pytest.raises(AssertionError):   # ... or the groups stay and the run table alone is short
        RO.check_run_table(t.hist, t.nrun, runs, t.grp_type, t.grp_edges)


def test_checker_refuses_a_remainder_ahead_of_its_full_pieces():
    t = _cut_chunk()
    typ = next(ty for ty in range(t.hist.size)
               if ((int(t.hist[ty]) + 3) // 4) > t.gmax and ((int(t.hist[ty]) + 3) // 4) % t.gmax)
    mine = [i for i in range(t.nrun) if t.run_type[i] == typ]
    order = list(range(t.nrun))
    order.remove(mine[-1])
    order.insert(mine[0], mine[-1])   # the type's remainder in front of its first full piece
    with pytest.raises(AssertionError):
        RO.check_run_table(t.hist, t.nrun, *_rebuild(t, order))
