"""CPU: the host side of ensemble screening - the nine impnn_ensemble_grid* entries (declared, exported, bound), the
status code of every argument rule of the five launching entries and the workspace query (one table of (bad argument,
code, text); every failing call returns before a launch, the stand-in pointers are never dereferenced), the limits the
library reports, ModelEnsemble's construction errors, the partners / rank refusal, known answers of
data.ensemble_grid_stats, and - on the member grids tests/test_gpu_ensemble.py produces on the GPU, here from the
oracle in float32 - that the float32 statistic meets the project's bound against float64, while a statistic with M - 1
in the denominator or without the last member does not."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import ensemble_cases as E
from conftest import ROOT, assert_close
from ionic_mpnn_amd import ModelEnsemble, _lib, data, model as MM, ops

CPU = torch.device("cpu")
_BAD, _UNS, _WS = -1, -2, -4
_P = 0x100000   # a stand-in pointer (16-byte aligned)
ENTRIES = ("impnn_ensemble_grid_max_members", "impnn_ensemble_grid_max_temperatures",
           "impnn_ensemble_grid_topk_max_temperatures", "impnn_ensemble_grid_tail_floats", "impnn_ensemble_grid",
           "impnn_ensemble_grid_mask", "impnn_ensemble_grid_topk_workspace_bytes", "impnn_ensemble_grid_topk",
           "impnn_ensemble_grid_topk_where")


def test_the_entries_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "impnn.h").read_text(), flags=re.S)
    raw = C.CDLL(str(_lib.lib_path()))
    for n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in impnn.h"
        assert hasattr(raw, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} is not bound"
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("impnn_ensemble_grid")) == sorted(ENTRIES)
    assert _lib.load().impnn_abi_version() == 3  # additions only


def test_limits_the_library_reports():
    lib = _lib.load()
    assert lib.impnn_ensemble_grid_max_members() == 8
    for M in range(1, 9):
        assert lib.impnn_ensemble_grid_max_temperatures(0, M) == 4096 and lib.impnn_ensemble_grid_max_temperatures(1, M) == 0
        assert 1 <= lib.impnn_ensemble_grid_topk_max_temperatures(M) <= ops.SELECT_MAX_T
    # the members' kept results share the LDS with the lists: 12 KiB a member against 16 KiB a temperature
    assert [lib.impnn_ensemble_grid_topk_max_temperatures(M) for M in range(1, 9)] == [4, 4, 4, 4, 4, 4, 3, 2]
    for M in (0, 9, -1):
        assert lib.impnn_ensemble_grid_max_temperatures(0, M) == 0 and lib.impnn_ensemble_grid_topk_max_temperatures(M) == 0
    assert lib.impnn_ensemble_grid_tail_floats(0, 32, 20) == 20 * 3 + 3
    assert lib.impnn_ensemble_grid_tail_floats(1, 32, 20) == 20 * 32 + 32 + 32 + 1
    for kind, D in ((0, 32), (1, 64)):  # the tail is what the packed head holds behind its per-ion parts, whatever D
        assert lib.impnn_ensemble_grid_tail_floats(kind, 32, 20) == \
            lib.impnn_model_head_floats(kind, D, 32, 20) - 2 * (D * 32 + 32) - 2 * (32 * 20 + 20)
    assert lib.impnn_ensemble_grid_tail_floats(2, 32, 20) == -1 and lib.impnn_ensemble_grid_tail_floats(0, 0, 20) == -1


# ---------------------------------------------------------------- status codes
def _need(lib, M=3, C_=100, A=100, nT=2, k=100, workgroups=0):
    n = C.c_size_t(0)
    rc = lib.impnn_ensemble_grid_topk_workspace_bytes(M, C_, A, nT, k, workgroups, C.byref(n))
    return rc, n.value


_DEFAULT = dict(kind=0, M=3, mc=_P, ma=_P, T=_P, tails=_P, kappa=1.0, C=3, A=4, nT=2, F=32, Mx=20)


def _call(lib, entry, **kw):
    """One call of a launching entry with sound arguments except ``kw`` -> (status, message)."""
    a = dict(_DEFAULT, mean=_P, std=_P, score=_P, lo=0.0, hi=1.0, words=_P, where=_P, k=5, largest=0, values=_P,
             cation=_P, anion=_P, ws=_P, ws_bytes=None, workgroups=0)
    a.update(kw)
    lead = (a["kind"], a["M"], a["mc"], a["ma"], a["T"], a["tails"], a["kappa"])
    trail = (a["C"], a["A"], a["nT"], a["F"], a["Mx"])
    if entry == "impnn_ensemble_grid":
        rc = lib.impnn_ensemble_grid(*lead, a["mean"], a["std"], a["score"], *trail, None)
    elif entry == "impnn_ensemble_grid_mask":
        rc = lib.impnn_ensemble_grid_mask(*lead, a["lo"], a["hi"], a["words"], *trail, None)
    else:
        if a["ws_bytes"] is None:
            rc, a["ws_bytes"] = _need(lib, min(max(a["M"], 1), 8), max(a["C"], 0), max(a["A"], 0), min(max(a["nT"], 0), 2),
                                      min(max(a["k"], 1), 1024), max(a["workgroups"], 0))
            if rc != 0:  # (a shape the query refuses too: the entry must refuse it before it looks at the size)
                a["ws_bytes"] = 1 << 40
        mask = (a["where"],) if entry.endswith("_where") else ()
        rc = getattr(lib, entry)(*lead, *mask, a["k"], a["largest"], a["values"], a["cation"], a["anion"], a["ws"],
                                 a["ws_bytes"], *trail, a["workgroups"], None)
    return rc, lib.impnn_last_error_string()


_MP = dict(kind=1, nT=0, T=None)
_2_32 = dict(C=1 << 16, A=1 << 16)
# (bad argument, code, text): the rules every launching entry shares, in no particular order - each alone
_SHARED = ((dict(kind=2), _BAD, b"kind"), (dict(kind=-1), _BAD, b"kind"),
           (dict(C=-1), _BAD, b"bad shape"), (dict(A=-1), _BAD, b"bad shape"), (dict(nT=-1), _BAD, b"bad shape"),
           (dict(F=0), _BAD, b"bad shape"), (dict(Mx=-1), _BAD, b"bad shape"),
           (dict(kind=1, nT=3), _BAD, b"nT must be 0"), (dict(kind=0, nT=0), _BAD, b"nT >= 1"),
           (dict(M=0), _BAD, b"M=0"), (dict(M=-2), _BAD, b"M=-2"), (dict(M=9), _UNS, b"M=9"),
           (dict(kappa=float("nan")), _BAD, b"kappa"), (dict(kappa=float("inf")), _BAD, b"kappa"),
           (dict(kappa=float("-inf")), _BAD, b"kappa"),
           (dict(F=65), _UNS, b"F=65"), (dict(Mx=65), _UNS, b"Mx=65"), (dict(_MP, Mx=65), _UNS, b"Mx=65"),
           (dict(mc=None), _BAD, b"null pointer"), (dict(ma=None), _BAD, b"null pointer"),
           (dict(T=None), _BAD, b"null pointer"), (dict(tails=None), _BAD, b"null pointer"),
           (dict(_MP, T=_P), _BAD, b"takes no temperatures"))
# ... and each entry's own
_OWN = {"impnn_ensemble_grid": ((dict(mean=None, std=None, score=None), _BAD, b"null pointer"), (dict(nT=4097), _UNS, b"nT=4097")),
        "impnn_ensemble_grid_mask": ((dict(words=None), _BAD, b"null pointer"), (dict(lo=float("nan")), _BAD, b"NaN"),
                                     (dict(hi=float("nan")), _BAD, b"NaN"), (dict(words=_P + 2), _BAD, b"4-byte aligned"),
                                     (dict(nT=4097), _UNS, b"nT=4097")),
        "impnn_ensemble_grid_topk": ((dict(k=0), _BAD, b"k=0"), (dict(k=1025), _UNS, b"k=1025"), (dict(nT=5), _UNS, b"nT=5"),
                                     (dict(M=7, nT=4), _UNS, b"nT=4"), (dict(M=8, nT=3), _UNS, b"nT=3"),
                                     (dict(_2_32), _UNS, b"4294967296 pairs"), (dict(workgroups=-1), _BAD, b"bad shape"),
                                     (dict(values=None), _BAD, b"null pointer"), (dict(cation=None), _BAD, b"null pointer"),
                                     (dict(anion=None), _BAD, b"null pointer"), (dict(ws=None), _BAD, b"null pointer"),
                                     (dict(ws=_P + 4), _BAD, b"8-byte aligned"))}
_OWN["impnn_ensemble_grid_topk_where"] = _OWN["impnn_ensemble_grid_topk"] + (
    (dict(where=None), _BAD, b"null pointer"), (dict(where=_P + 2), _BAD, b"4-byte aligned"))


@pytest.mark.parametrize("entry", sorted(_OWN))
def test_status_codes(entry):
    lib = _lib.load()
    for kw, code, what in _SHARED + _OWN[entry]:
        rc, msg = _call(lib, entry, **kw)
        assert rc == code and what in msg and entry.encode() + b":" in msg, (entry, kw, rc, msg)
    # zero work comes before the null pointers: every pointer null, no workspace
    nulls = dict(mc=None, ma=None, T=None, tails=None, mean=None, std=None, score=None, words=None, where=None,
                 values=None, cation=None, anion=None, ws=None, ws_bytes=0)
    for kw in (dict(C=0), dict(A=0), dict(_MP, C=0)):
        assert _call(lib, entry, **dict(nulls, **kw))[0] == 0, (entry, kw)
    # ... and after the shape: a bad M with zero work is still refused
    assert _call(lib, entry, **dict(nulls, C=0, M=0))[0] == _BAD
    if "topk" in entry:  # the workspace, one byte short, after the null pointers
        for kw in ({}, _MP, dict(M=8, nT=2, k=1024, C=300, A=300, workgroups=7)):
            a = dict(M=3, C=3, A=4, nT=2, k=5, workgroups=0)
            a.update({k_: v for k_, v in kw.items() if k_ in a})
            rc, need = _need(lib, a["M"], a["C"], a["A"], a["nT"], a["k"], a["workgroups"])
            assert rc == 0 and need > 0
            rc, msg = _call(lib, entry, ws_bytes=need - 1, **kw)
            assert rc == _WS and b"workspace of %d bytes is too small (%d)" % (need - 1, need) in msg, (kw, msg)
        rc, msg = _call(lib, entry, ws_bytes=0, values=None)
        assert rc == _BAD and b"null pointer" in msg


def test_workspace_query():
    lib = _lib.load()
    # [workgroups][nT][k] entries of 8 bytes, one workgroup per 16 x 64 tile at most: the head grid's figures
    assert _need(lib, 3, 100, 100, 2, 100, 3) == (0, 3 * 2 * 100 * 8)
    assert _need(lib, 8, 17, 65, 0, 10, 9) == (0, 4 * 1 * 10 * 8)
    assert _need(lib, 1, 0, 5, 1, 10, 0) == (0, 0)
    for kw, code in ((dict(M=0), _BAD), (dict(M=9), _UNS), (dict(k=0), _BAD), (dict(k=1025), _UNS), (dict(nT=5), _UNS),
                     (dict(M=8, nT=3), _UNS), (dict(M=7, nT=4), _UNS), (dict(C_=1 << 16, A=1 << 16), _UNS),
                     (dict(workgroups=-1), _BAD), (dict(C_=-1), _BAD)):
        assert _need(lib, **kw)[0] == code and b"impnn_ensemble_grid_topk_workspace_bytes" in lib.impnn_last_error_string(), kw
    assert lib.impnn_ensemble_grid_topk_workspace_bytes(1, 1, 1, 1, 1, 0, None) == _BAD
    assert _need(lib, M=8, nT=2)[0] == 0 and _need(lib, M=7, nT=3)[0] == 0 and _need(lib, M=6, nT=4)[0] == 0
    # the families' shared queries do not serve this one
    n = C.c_size_t(0)
    assert lib.impnn_grid_topk_workspace_bytes(2, 3, 4, 1, 5, 0, C.byref(n)) == _BAD


# ---------------------------------------------------------------- Python-side errors
def _visc(**kw):
    return MM.build_model(E.VA, E.VB, **dict(dict(num_steps=1, device=CPU), **kw))


def test_model_ensemble_construction_errors():
    v, mp = _visc(), MM.build_melting_point_model(E.VA, E.VB, num_steps=1, device=CPU)
    assert len(ModelEnsemble([v])) == 1 and ModelEnsemble([v, _visc(atom_dim=64, num_steps=2)]).kind == "viscosity"
    assert ModelEnsemble([mp] * 8).kind == "melting_point"
    with pytest.raises(ValueError, match="1 to 8 models, got 0"):
        ModelEnsemble([])
    with pytest.raises(ValueError, match="1 to 8 models, got 9"):
        ModelEnsemble([v] * 9)
    with pytest.raises(ValueError, match="member 1 is not an MPNNModel"):
        ModelEnsemble([v, "model"])
    with pytest.raises(ValueError, match="member 1 is a melting_point model, member 0 a viscosity"):
        ModelEnsemble([v, mp])
    with pytest.raises(ValueError, match="member 2 has fp_size 16"):
        ModelEnsemble([v, v, _visc(fp_size=16)])
    with pytest.raises(ValueError, match="member 1 has fp_size 32 and mixing_size 24"):
        ModelEnsemble([v, _visc(mixing_size=24)])
    with pytest.raises(ValueError, match="member 0: the grid kernels do not cover"):
        ModelEnsemble([_visc(mixing_size=80)])
    with pytest.raises(ValueError, match="member 1 is on"):
        ModelEnsemble([v, _visc(device=torch.device("meta"))])
    transfer = MM.MPNNModel("transfer", E.VA, E.VB, 32, 8, 32, 20, 1, 1e-4, device=CPU)
    with pytest.raises(ValueError, match="member 0 is a transfer model"):
        ModelEnsemble([transfer])


def test_model_ensemble_argument_errors():
    cat, an = E.species(2, 3)
    ens = ModelEnsemble([_visc(), _visc()])
    with pytest.raises(KeyError, match="temperature"):
        ens.predict_grid(cat, an)
    with pytest.raises(ValueError, match="both"):
        ens.screen_top_k(cat, None, temperatures=[300.0])
    with pytest.raises(ValueError, match="kappa"):
        ens.predict_grid(cat, an, temperatures=[300.0], kappa=float("nan"))
    with pytest.raises(ValueError, match="k must be"):
        ens.screen_top_k(cat, an, temperatures=[300.0], k=0)
    with pytest.raises(ValueError, match="needs a bound"):
        ens.screen_mask(cat, an, temperatures=[300.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ens.predict_grid(cat, an, temperatures=[300.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ensemble_grid_operands("viscosity", torch.zeros(2, 2, 20), torch.zeros(2, 3, 20), torch.zeros(1), torch.zeros(2, 63), 32, 20)


def test_partners_and_rank_refuse_an_ensemble_grid_before_any_library_call():
    g = ops.GridOperands(2, 0, torch.zeros(2, 3, 20), torch.zeros(2, 4, 20), torch.zeros(1), torch.zeros(2, 63), (32, 20), 0.5)
    assert (g.family, g.members, g.C, g.A, g.nT, g.D, g.kappa) == (2, 2, 3, 4, 1, None, 0.5)
    assert g.trail == (3, 4, 1, 32, 20) and g.lead[:2] == (0, 2) and g.lead[-1] == 0.5
    assert g.rows(1, 3).C == 2 and g.rows(1, 3).cat.is_contiguous() and g.temperatures(0, 1).members == 2
    for call in (lambda: ops.grid_partners(g), lambda: ops.grid_rank(g, 3), lambda: ops.grid_rank(g, 3, mask=True)):
        with pytest.raises(NotImplementedError, match="ensemble grids: partners / rank are not built"):
            call()


# ---------------------------------------------------------------- the statistic
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_stats_of_one_member():
    v = np.array([[1.5, -2.25, 3e-39, 7e37, np.inf]], np.float32)
    for kappa in (0.0, 2.5, -1.0):
        mean, std, score = data.ensemble_grid_stats(v, kappa)
        assert np.array_equal(bits(mean), bits(v[0])) and np.array_equal(bits(mean[:4]), bits(score[:4]))
        assert np.array_equal(std[:4], np.zeros(4, np.float32)) and np.isnan(std[4]) and np.isnan(score[4])  # inf - inf


def test_stats_by_hand():
    # members 1, 2, 6: s = 9, mean = 3, d = -2, -1, 3, q = 14, std = sqrt(14 / 3), score = 3 + 2 * std
    v = np.array([1.0, 2.0, 6.0], np.float32).reshape(3, 1)
    mean, std, score = data.ensemble_grid_stats(v, 2.0)
    want = np.sqrt(np.float32(14.0) / np.float32(3.0))
    assert mean.dtype == std.dtype == score.dtype == np.float32 and mean.shape == (1,)
    assert mean[0] == 3.0 and bits(std)[0] == bits(want) and bits(score)[0] == bits(np.float32(3.0 + 2.0 * np.float64(want)))
    assert abs(float(std[0]) - np.std([1.0, 2.0, 6.0])) < 1e-6
    # the sum is ordered: (1e8 + 1) + -1e8 loses the 1 in float32, 1e8 + -1e8 + 1 does not
    a = data.ensemble_grid_stats(np.array([1e8, 1.0, -1e8], np.float32).reshape(3, 1), 0.0)[0]
    b = data.ensemble_grid_stats(np.array([1e8, -1e8, 1.0], np.float32).reshape(3, 1), 0.0)[0]
    assert a[0] == 0.0 and bits(b)[0] == bits(np.float32(1.0) / np.float32(3.0))
    with pytest.raises(ValueError, match="kappa"):
        data.ensemble_grid_stats(v, np.inf)
    with pytest.raises(ValueError, match="at least one member"):
        data.ensemble_grid_stats(np.empty((0, 3), np.float32), 0.0)


def test_stats_confine_a_nan():
    v = np.arange(24, dtype=np.float32).reshape(3, 2, 4)
    v[1, 0, 2] = np.nan
    out = data.ensemble_grid_stats(v, 1.0)
    clean = data.ensemble_grid_stats(np.nan_to_num(v, nan=1.0), 1.0)
    for o, c in zip(out, clean):
        nan = np.isnan(o)
        assert nan[0, 2] and nan.sum() == 1 and np.array_equal(bits(o[~nan]), bits(c[~nan]))


@pytest.fixture(scope="module", params=sorted(E.CASES))
def member_grids(request):
    return request.param, E.cpu_member_grids(request.param)


def test_the_float32_statistic_meets_the_bound(member_grids):
    name, v = member_grids
    for got, want, what in zip(data.ensemble_grid_stats(v, E.KAPPA), E.stats64(v, E.KAPPA), ("mean", "std", "score")):
        assert_close(got, want, rel=1e-5, what=f"{name} {what}", floor=0.3)


def test_the_bound_sees_a_wrong_denominator_and_a_skipped_member(member_grids):
    name, v = member_grids
    M = v.shape[0]
    mean, std, _ = E.stats64(v, E.KAPPA)
    sample = np.asarray(v, np.float64).std(axis=0, ddof=1)      # M - 1 in the denominator
    with pytest.raises(AssertionError):
        assert_close(sample.astype(np.float32), std, rel=1e-5, what=f"{name} std", floor=0.3)
    short = data.ensemble_grid_stats(v[:M - 1], E.KAPPA)         # the last member skipped
    with pytest.raises(AssertionError):
        assert_close(short[0], mean, rel=1e-5, what=f"{name} mean", floor=0.3)
    with pytest.raises(AssertionError):
        assert_close(short[1], std, rel=1e-5, what=f"{name} std", floor=0.3)
