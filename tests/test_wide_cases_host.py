"""tests/wide_cases.py without a device: on 256 CUs every case reaches the kernels it is built for, the designed
molecules and type runs are what they claim, the named molecules lie where the update kernels change behaviour, and
the fp64 oracle is finite and independent of its chunking on every sample."""
import numpy as np
import pytest

import wide_cases as WC

CUS = 256   # MI355X
ALL = [(name, D) for name in WC.CASES for D in WC.DIMS]


@pytest.mark.parametrize("name,D", ALL)
def test_every_case_meets_its_premises(name, D):
    case = WC.build(name, D)
    case.check_premises(CUS)
    got = case.premises(CUS)
    assert got["mini"] == case.expect.get("mini", False)       # no other case has a split last round
    if name in WC.HALF_EXPECT:
        case.check_half_premises(CUS)
    D_, K, S, Va, Vb, inputs, w = case.as_tuple()
    assert D_ == D and inputs["cat_atom"].shape == (case.B, case.N) and inputs["an_bond"].shape == (case.B, case.E)
    assert w["atom_embedding"].shape == (Va, D) and w["cat_bmm_0/bond_transform"].shape == (K, D, D)
    for p in ("cat", "an"):      # the oracle's contract: ids inside the vocabularies, endpoints inside the molecule
        assert 0 <= inputs[f"{p}_atom"].min() and inputs[f"{p}_atom"].max() < Va
        assert 0 <= inputs[f"{p}_bond"].min() and inputs[f"{p}_bond"].max() < Vb
        assert 0 <= inputs[f"{p}_connectivity"].min() and inputs[f"{p}_connectivity"].max() < case.N


@pytest.mark.parametrize("name,B", [("mid", 64), ("many", 512), ("big", 511), ("runs", 64), ("small", 171)])
def test_a_batch_on_the_wrong_side_of_its_threshold_fails_the_premise(name, B):
    WC.build(name, 128).check_premises(CUS)
    with pytest.raises(AssertionError, match="does not reach its kernels"):
        WC.build(name, 128, B).check_premises(CUS)


def test_premises_follow_the_cu_count():
    """The thresholds are the launcher's, not constants of the cases: on a smaller device `mid` would still take 64-row
    tiles, and `big` would fill it with whole rounds differently."""
    mid = WC.build("mid", 128)
    assert mid.premises(304)["tile16"] and not mid.premises(256)["tile16"]
    big = WC.build("big", 128)
    assert not big.premises(304)["big128"] and big.premises(256)["big128"]
    t_live = -(-big.plan["kept_end"] // 128)
    assert big.premises(256)["mini"] and not big.premises(t_live)["mini"]       # one partial round is not split


@pytest.mark.parametrize("D", WC.DIMS)
def test_runs_case_has_exactly_the_designed_type_counts(D):
    case = WC.build("runs", D)
    te, want = WC.tile_edges(D), WC.run_counts(D)
    assert want == [0, 1, te - 1, te, 0, te, te + 1, 2 * te + 3, 0, te]
    cat, an = case.plan["counts"]
    assert list(cat[:len(want)]) == want and cat[-1] == 0
    assert list(an[::-1][:len(want)]) == want and an[0] == 0
    assert (cat[len(want):-1] > 0).all() and (an[1:-len(want)] > 0).all()   # the types in between are all in use
    for p in ("cat", "an"):     # every edge has valid endpoints or is padding, so the counts are exact
        conn, bond = case.inputs[f"{p}_connectivity"], case.inputs[f"{p}_bond"]
        src, tgt = conn[:, :, 0], conn[:, :, 1]
        valid = (src > 0) & (tgt > 0)
        assert ((src == 0) & (tgt == 0))[~valid].all() and (bond[~valid] == 0).all()
        assert np.array_equal(np.bincount(bond[valid], minlength=case.Vb), case.plan["counts"][0 if p == "cat" else 1])


@pytest.mark.parametrize("name,D", ALL)
def test_degree_census_and_designed_molecules(name, D):
    case = WC.build(name, D)
    seen = WC.degree_census(case)
    assert {0, 1, 2, 3} <= seen and max(seen) >= 17, seen
    for g in (0, 1):
        where, p = case.where[g], case.plan
        for b in where.get("deg", []):
            assert [int(d) for d in p["indeg"][g][b, :13]] == [WC.DESIGNED_DEGREES[n] for n in range(13)]
            assert p["kept"][g][b] == case.N                        # the padding atom N-1 sends: every row is kept
            conn = case.inputs["cat_connectivity" if g == 0 else "an_connectivity"][b]
            slots = np.flatnonzero(conn[:, 1] == 9)
            assert len(slots) == 2 and (slots[0] // 64 != slots[1] // 64 or case.E <= 64)
        for b in where.get("hub", []):
            assert p["indeg"][g][b, 3] == case.E
        for b in where.get("dup4", []):
            assert list(p["indeg"][g][b, :4]) == [0, 4, 8, 4]
        for b in where.get("pad_edges", []):
            assert p["kept"][g][b] == 3 and not case.inputs["cat_atom" if g == 0 else "an_atom"][b].any()
        for b in where["pad"]:
            assert p["kept"][g][b] == 0
        assert p["kept"][g][0] == 0 and p["kept"][g][-1] == 0      # an all-padding molecule first and last
    kept = np.concatenate(case.plan["kept"])
    assert kept.min() == 0 and kept.max() == case.N and len(np.unique(kept)) >= min(case.N, 12)


@pytest.mark.parametrize("name,D", ALL)
def test_named_molecules_lie_where_the_case_says(name, D):
    case = WC.build(name, D)
    p, named = case.plan, case.named(CUS)
    assert p["base"][0] == 0 and p["base"][1] % 128 == 0 and 0 <= p["base"][1] - p["rows"][0] < 128
    assert p["kept_end"] == p["base"][1] + p["rows"][1]
    for g in (0, 1):
        if name == "noanion" and g == 1:
            assert p["rows"][1] == 0 and named["tail1"] == [] and not p["kept"][1].any()
            continue
        tail = named[f"tail{g}"]
        end = p["base"][g] + p["rows"][g]
        assert tail and p["rows"][g] % 128 != 0                    # the ion's last tile is a partial one
        for gg, b in tail:
            lo, hi = p["rowbase"][g][b], p["rowbase"][g][b] + p["kept"][g][b]
            assert gg == g and hi > lo and hi > (end - 1) // 128 * 128 and hi <= end
        assert max(p["rowbase"][g][b] + p["kept"][g][b] for _, b in tail) == end
    assert len(named["gap"]) == (1 if name == "noanion" else 2)
    if name != "noanion":
        (g0, b0), (g1, b1) = named["gap"]
        assert (g0, g1) == (0, 1) and p["rowbase"][0][b0] + p["kept"][0][b0] == p["rows"][0]
        assert p["rowbase"][1][b1] == p["base"][1]
    if case.expect.get("mini"):
        t_live = -(-p["kept_end"] // 128)
        first = t_live // CUS * CUS * 128
        assert named["mini"] and CUS < t_live
        for g, b in named["mini"]:
            assert p["rowbase"][g][b] + p["kept"][g][b] > first
        assert any(p["rowbase"][g][b] < first for g, b in named["mini"])   # a molecule cut by the round's first tile
    else:
        assert named["mini"] == []
    idx = case.sample(CUS)
    assert len(idx) == len(set(idx)) and 8 <= len(idx) <= 40
    for mols in named.values():
        for g, b in mols[:2] + mols[-2:]:
            assert b in idx
    for w in case.where:
        for bs in w.values():
            assert set(bs[:3]) <= set(idx)


@pytest.mark.parametrize("name,D", ALL)
def test_oracle_is_finite_and_independent_of_its_chunking(name, D):
    """The sample's reference does not depend on the chunk a molecule is evaluated in: alone or among seven others,
    the same value within fp64 round-off (the oracle treats molecules independently)."""
    case = WC.build(name, D)
    idx = case.sample(CUS)
    rc, ra = WC.oracle_pooled(case, idx)
    assert np.isfinite(rc).all() and np.isfinite(ra).all()
    scale = max(np.abs(rc).max(), np.abs(ra).max())
    for i in (1, 2, len(idx) - 1):
        c1, a1 = WC.oracle_pooled(case, idx[i:i + 1])
        assert np.abs(c1[0] - rc[i]).max() <= 1e-12 * scale and np.abs(a1[0] - ra[i]).max() <= 1e-12 * scale
    for g, (ref, p) in enumerate(((rc, "cat"), (ra, "an"))):      # all-padding molecules pool to exactly 0
        none = ~case.inputs[f"{p}_atom"][idx].any(axis=1)
        assert none.any() and not ref[none].any()
