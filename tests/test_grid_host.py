"""CPU: the host side of cation x anion screening - record deduplication, the argument rules of impnn_head_ion_mix /
impnn_head_grid (every failing call returns before a launch; the stand-in pointers are never dereferenced), the
Python-side errors of encode_ions / predict_grid, and the padding of ion_pair_batches."""
import numpy as np
import pytest
import torch

from ionic_mpnn_amd import _lib, data, model as MM, ops, synthetic

CPU = torch.device("cpu")
_BAD, _UNS = -1, -2
_P = 0x100000  # a stand-in pointer


# ---------------------------------------------------------------- unique_ions
def _same_ion(x, y):
    return (list(x["atom_ids"]) == list(y["atom_ids"]) and list(x["bond_ids"]) == list(y["bond_ids"])
            and [tuple(e) for e in x["edge_indices"]] == [tuple(e) for e in y["edge_indices"]])


def _records():
    recs, vocab = synthetic.make_id_records(6, seed=3)
    out = []
    # pairs (cation of a, anion of b) with repeats in both species, several temperatures per pair
    for k, (a, b) in enumerate([(0, 0), (1, 0), (0, 1), (2, 2), (1, 0), (0, 0), (3, 2), (2, 1)]):
        out.append({"pair_id": f"p{k}", "cation": recs[a]["cation"], "anion": recs[b]["anion"],
                    "T": 280.0 + 10.0 * k, "log_eta": 1.0})
    return out, vocab


def test_unique_ions_deduplicates_both_species_and_round_trips():
    recs, _ = _records()
    cats, ans, ci, ai = data.unique_ions(recs)
    assert len(cats) == 4 and len(ans) == 3
    assert ci.dtype == np.int64 and ai.dtype == np.int64 and ci.shape == ai.shape == (len(recs),)
    assert ci.tolist() == [0, 1, 0, 2, 1, 0, 3, 2] and ai.tolist() == [0, 0, 1, 2, 0, 0, 2, 1]  # first occurrence order
    for k, r in enumerate(recs):
        assert _same_ion(r["cation"], cats[ci[k]]) and _same_ion(r["anion"], ans[ai[k]])
    for group in (cats, ans):
        for i in range(len(group)):
            for j in range(i):
                assert not _same_ion(group[i], group[j])


def test_unique_ions_compares_element_for_element():
    recs, _ = _records()
    twin = {k: (list(v) if isinstance(v, list) else v) for k, v in recs[0]["cation"].items()}  # equal, another object
    other = dict(twin, bond_ids=[(b + 1) % 6 for b in twin["bond_ids"]])                        # differs in bond ids only
    extra = [dict(recs[0], cation=twin), dict(recs[0], cation=other)]
    cats, _, ci, _ = data.unique_ions(recs[:1] + extra)
    assert len(cats) == 2 and ci.tolist() == [0, 0, 1]


def test_a_cation_that_equals_an_anion_stays_two_entries():
    recs, _ = _records()
    ion = recs[0]["cation"]
    cats, ans, ci, ai = data.unique_ions([{"pair_id": "x", "cation": ion, "anion": ion, "T": 300.0}])
    assert len(cats) == 1 and len(ans) == 1 and ci.tolist() == [0] and ai.tolist() == [0]


def test_unique_ions_of_an_empty_list():
    cats, ans, ci, ai = data.unique_ions([])
    assert cats == [] and ans == [] and ci.shape == (0,) and ai.shape == (0,) and ci.dtype == np.int64


def test_dataset_unique_ions_matches_build_inputs():
    recs, vocab = _records()
    ds = data.IonPairDataset(recs, vocab)
    cats, ans, ci, ai = ds.unique_ions()
    _, _, ci0, ai0 = data.unique_ions(recs)
    assert np.array_equal(ci, ci0) and np.array_equal(ai, ai0)
    full = ds.build_inputs(range(len(ds)))
    for p, species, idx in (("cat", cats, ci), ("an", ans, ai)):
        for k in MM.ION_KEYS:
            assert species[k].dtype == np.int32
            assert np.array_equal(species[k][idx], full[f"{p}_{k}"]), (p, k)


# ---------------------------------------------------------------- status codes of the two entries
def _mix(lib, **kw):
    a = dict(kind=0, ion=0, pooled=_P, w=_P, mix=_P, M=5, D=32, F=32, Mx=20)
    a.update(kw)
    rc = lib.impnn_head_ion_mix(a["kind"], a["ion"], a["pooled"], a["w"], a["mix"], a["M"], a["D"], a["F"], a["Mx"], None)
    return rc, lib.impnn_last_error_string()


def _grid(lib, **kw):
    a = dict(kind=0, mc=_P, ma=_P, T=_P, w=_P, out=_P, params=None, C=3, A=4, nT=2, D=32, F=32, Mx=20)
    a.update(kw)
    rc = lib.impnn_head_grid(a["kind"], a["mc"], a["ma"], a["T"], a["w"], a["out"], a["params"], a["C"], a["A"], a["nT"],
                             a["D"], a["F"], a["Mx"], None)
    return rc, lib.impnn_last_error_string()


_MIX_NULLS = dict(pooled=None, w=None, mix=None)
_GRID_NULLS = dict(mc=None, ma=None, T=None, w=None, out=None, params=None)


def test_head_ion_mix_status_codes():
    lib = _lib.load()
    # 1. shape, before everything else (null pointers and zero rows included)
    for kw, code, what in ((dict(M=-1), _BAD, b"bad shape"), (dict(D=0), _BAD, b"bad shape"), (dict(F=-3), _BAD, b"bad shape"),
                           (dict(Mx=0), _BAD, b"bad shape"), (dict(D=129), _UNS, b"D=129"), (dict(Mx=65), _UNS, b"Mx=65"),
                           (dict(F=65), _UNS, b"F=65"), (dict(kind=2), _BAD, b"kind"), (dict(kind=-1), _BAD, b"kind"),
                           (dict(ion=2), _BAD, b"ion"), (dict(ion=-1), _BAD, b"ion")):
        for extra in ({}, _MIX_NULLS, dict(_MIX_NULLS, M=0)):
            args = dict(extra)
            args.update(kw)
            rc, msg = _mix(lib, **args)
            assert rc == code and what in msg and b"impnn_head_ion_mix" in msg, (kw, extra, rc, msg)
    # 2. zero work touches nothing
    assert _mix(lib, M=0, **_MIX_NULLS)[0] == 0
    assert _mix(lib, M=0, kind=1, ion=1, D=128, F=64, Mx=64, **_MIX_NULLS)[0] == 0
    # 3. null pointers: all, and each alone
    for kw in [_MIX_NULLS] + [{n: None} for n in _MIX_NULLS]:
        rc, msg = _mix(lib, **kw)
        assert rc == _BAD and b"null pointer" in msg, (kw, msg)


def test_head_grid_status_codes():
    lib = _lib.load()
    mp = dict(kind=1, nT=0, T=None)
    for kw, code, what in ((dict(C=-1), _BAD, b"bad shape"), (dict(A=-1), _BAD, b"bad shape"), (dict(nT=-1), _BAD, b"bad shape"),
                           (dict(D=0), _BAD, b"bad shape"), (dict(F=0), _BAD, b"bad shape"), (dict(Mx=-1), _BAD, b"bad shape"),
                           (dict(D=129), _UNS, b"D=129"), (dict(Mx=65), _UNS, b"Mx=65"), (dict(F=65), _UNS, b"F=65"),
                           (dict(mp, D=129), _UNS, b"D=129"),
                           (dict(kind=1, nT=3), _BAD, b"nT must be 0"), (dict(kind=0, nT=0), _BAD, b"nT >= 1"),
                           (dict(nT=4097), _UNS, b"nT=4097"),
                           (dict(kind=2), _BAD, b"kind"), (dict(kind=-1), _BAD, b"kind")):
        for extra in ({}, _GRID_NULLS, dict(_GRID_NULLS, C=0), dict(_GRID_NULLS, A=0)):
            args = dict(extra)
            args.update(kw)
            rc, msg = _grid(lib, **args)
            assert rc == code and what in msg and b"impnn_head_grid" in msg, (kw, extra, rc, msg)
    # 2. zero work: every pointer null
    for kw in (dict(C=0), dict(A=0), dict(C=0, A=0), dict(mp, C=0), dict(mp, A=0)):
        args = dict(_GRID_NULLS)
        args.update(kw)
        assert _grid(lib, **args)[0] == 0, kw
    # 3. null pointers (params is optional; the melting-point grid needs no temperatures)
    for kw in [_GRID_NULLS] + [{n: None} for n in ("mc", "ma", "T", "w", "out")]:
        rc, msg = _grid(lib, **kw)
        assert rc == _BAD and b"null pointer" in msg, (kw, msg)
    for n in ("mc", "ma", "w", "out"):
        rc, msg = _grid(lib, **dict(mp, **{n: None}))
        assert rc == _BAD and b"null pointer" in msg, (n, msg)
    # the melting-point grid takes neither temperatures nor params
    for kw in (dict(T=_P), dict(params=_P)):
        rc, msg = _grid(lib, **dict(mp, **kw))
        assert rc == _BAD and b"neither" in msg, (kw, msg)
    assert lib.impnn_abi_version() == 3


# ---------------------------------------------------------------- Python-side errors
def _species(n, seed, N=40, E=80):
    b = synthetic.make_batch(n, max_atoms=N, max_edges=E, seed=seed, with_temperature=False)
    return {k: b[f"cat_{k}"] for k in MM.ION_KEYS}, {k: b[f"an_{k}"] for k in MM.ION_KEYS}


def test_cpu_tensors_fail_loudly():
    cat, an = _species(3, 0)
    m = MM.build_model(synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, num_steps=1, device=CPU)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encode_ions(cat, an)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encode_ions(anions={k: torch.from_numpy(v) for k, v in an.items()})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict_grid(cat, an, temperatures=[300.0, 310.0])
    w = torch.zeros(_lib.load().impnn_model_head_floats(0, 32, 32, 20))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.head_ion_mix("viscosity", "cat", torch.zeros(2, 32), w, 32, 20)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.head_grid("viscosity", torch.zeros(2, 20), torch.zeros(3, 20), torch.zeros(2), w, 32, 20)


def test_predict_grid_argument_errors():
    cat, an = _species(2, 1)
    v = MM.build_model(synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, num_steps=1, device=CPU)
    with pytest.raises(KeyError, match="temperature"):
        v.predict_grid(cat, an)
    with pytest.raises(KeyError, match="temperature") as same:
        v.predict({f"{p}_{k}": s[k] for p, s in (("cat", cat), ("an", an)) for k in MM.ION_KEYS})
    assert same.type is KeyError
    mp = MM.build_melting_point_model(synthetic.DEFAULT_VA, synthetic.DEFAULT_VB, atom_dim=8, num_steps=1, device=CPU)
    with pytest.raises(ValueError, match="return_params"):
        mp.predict_grid(cat, an, return_params=True)
    with pytest.raises(ValueError, match="max_pairs_per_launch"):
        v.predict_grid(cat, an, temperatures=[300.0], max_pairs_per_launch=0)
    with pytest.raises(ValueError, match="both"):
        v.predict_grid(cat, None, temperatures=[300.0])
    with pytest.raises(ValueError):
        v.encode_ions()
    with pytest.raises(KeyError):
        v.encode_ions({"atom": cat["atom"]})


# ---------------------------------------------------------------- ion_pair_batches
def test_ion_pair_batches_pads_to_a_common_shape_and_chunks():
    cat, _ = _species(5, 2, N=40, E=80)
    _, an = _species(11, 3, N=12, E=16)
    batches, C, A = MM.ion_pair_batches(cat, an, batch_size=4)
    assert (C, A) == (5, 11) and [len(b["cat_atom"]) for b in batches] == [4, 4, 3]
    whole = {k: np.concatenate([b[k] for b in batches]) for k in batches[0]}
    assert set(whole) == {f"{p}_{k}" for p in ("cat", "an") for k in MM.ION_KEYS}
    for p in ("cat", "an"):
        assert whole[f"{p}_atom"].shape == (11, 40) and whole[f"{p}_bond"].shape == (11, 80)
        assert whole[f"{p}_connectivity"].shape == (11, 80, 2)
        assert all(v.dtype == np.int32 for v in whole.values())
    for k in MM.ION_KEYS:
        assert np.array_equal(whole[f"cat_{k}"][:5], cat[k])
        assert not whole[f"cat_{k}"][5:].any()          # the shorter side: all-padding molecules
    assert np.array_equal(whole["an_atom"][:, :12], an["atom"]) and not whole["an_atom"][:, 12:].any()
    assert np.array_equal(whole["an_bond"][:, :16], an["bond"]) and not whole["an_bond"][:, 16:].any()
    assert np.array_equal(whole["an_connectivity"][:, :16], an["connectivity"]) and not whole["an_connectivity"][:, 16:].any()


def test_ion_pair_batches_chunk_boundaries_and_absent_sides():
    cat, an = _species(8, 4)
    for bs, sizes in ((8, [8]), (9, [8]), (7, [7, 1]), (4, [4, 4]), (1, [1] * 8)):
        batches, C, A = MM.ion_pair_batches(cat, an, bs)
        assert [len(b["an_bond"]) for b in batches] == sizes and (C, A) == (8, 8)
    batches, C, A = MM.ion_pair_batches(None, an, 16)           # an absent side: all padding, same shape
    assert (C, A) == (0, 8) and len(batches) == 1
    assert batches[0]["cat_atom"].shape == an["atom"].shape and not batches[0]["cat_atom"].any()
    assert not batches[0]["cat_connectivity"].any() and np.array_equal(batches[0]["an_bond"], an["bond"])
    torch_side = {k: torch.from_numpy(v) for k, v in cat.items()}
    batches, C, A = MM.ion_pair_batches(torch_side, None, 16)
    assert (C, A) == (8, 0) and np.array_equal(batches[0]["cat_connectivity"], cat["connectivity"])
    empty = {k: v[:0] for k, v in cat.items()}
    batches, C, A = MM.ion_pair_batches(empty, empty, 16)
    assert batches == [] and (C, A) == (0, 0)
    with pytest.raises(ValueError):
        MM.ion_pair_batches(None, None)
    with pytest.raises(ValueError):
        MM.ion_pair_batches(cat, an, 0)
    with pytest.raises(ValueError):
        MM.ion_pair_batches({"atom": cat["atom"], "bond": cat["bond"], "connectivity": cat["connectivity"][:3]}, an)
