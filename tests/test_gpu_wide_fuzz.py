"""Wide encoder fuzz (csrc/encoder_wide.hip, csrc/wide_*.hip): every update-kernel variant and both ways of feeding it aggregated
messages, on the adversarial batches of tests/wide_cases.py, against oracle.mpnn_oracle.encode in fp64.

In-process, the launcher's own choice: each case ASSERTS its premises from the device's CU count (which kernels the
batch reaches), then both wide modes against the oracle - exact f32 (f32t) within conftest.assert_close (1e-5,
BASELINE north_star), f32x3 by the rule of test_wide_f32x3_error_within_twice_f32t_and_bitwise_properties (max, rms
and elementwise error at most twice f32t's plus 1e-7, and max error at most 1e-5 for both).  Every output is taken
from a run on a workspace filled with 0xff bytes (wide_child.run_case), so a row that is read without having been
written in the same call shows as NaN instead of reading the zeros of fresh memory.

Forced paths: tests/wide_child.py in a fresh process per setting of IMPNN_WIDE_NO_DIRECT / IMPNN_WIDE_TILE_ROWS /
IMPNN_WIDE_X3_BIG (read once per process), compared BIT FOR BIT with the in-process outputs of the same mode - DESIGN
4.4: "a batch and its shards take different tile sizes and still agree bit for bit", "the value is the one
wide_reduce would have written".  The children's outputs thereby inherit the oracle comparison."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import wide_cases as WC
from conftest import assert_close
from wide_child import run_case
from ionic_mpnn_amd import model as MM

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ALL = [(name, D) for name in WC.CASES for D in WC.DIMS]
OVERRIDES = ("IMPNN_WIDE_NO_DIRECT", "IMPNN_WIDE_TILE_ROWS", "IMPNN_WIDE_X3_BIG")
SETTINGS = {
    "no_direct": {"IMPNN_WIDE_NO_DIRECT": "1"},
    "rows16": {"IMPNN_WIDE_TILE_ROWS": "16", "IMPNN_WIDE_X3_BIG": "0"},
    "rows64_big": {"IMPNN_WIDE_TILE_ROWS": "64", "IMPNN_WIDE_X3_BIG": "1"},
    "no_direct_rows32": {"IMPNN_WIDE_NO_DIRECT": "1", "IMPNN_WIDE_TILE_ROWS": "32", "IMPNN_WIDE_X3_BIG": "0"},
}
CHILD_TIMEOUT = 300   # seconds; a child takes well under a minute


def cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def to_dev(inputs):
    return {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in inputs.items()}


def make_model(case, mode):
    m = MM.build_model(case.Va, case.Vb, atom_dim=case.D, bond_dim=case.K, num_steps=case.S, device=DEV)
    m.load_weights(case.weights)
    m.encoder_mode = mode
    assert m.resolve_encoder_mode(case.N, case.E) == mode
    return m


@pytest.fixture(scope="module")
def natural():
    """(case, D) -> {mode: (cat, an)}: the in-process outputs with no override set, computed once."""
    for v in OVERRIDES:
        assert v not in os.environ, f"{v} is set: this module compares forced launches with the launcher's own choice"
    cache = {}

    def get(name, D):
        if (name, D) not in cache:
            case = WC.build(name, D)
            case.check_premises(cus())        # a case that runs another kernel than it claims is a failure
            cache[(name, D)] = {mode: run_case(case, mode, DEV) for mode in WC.MODES}
        return cache[(name, D)]
    return get


@pytest.fixture(scope="module")
def reference():
    """(case, D) -> (pair indices, cat, an): the fp64 oracle, once per case and shared by the modes."""
    cache = {}

    def get(name, D):
        if (name, D) not in cache:
            case = WC.build(name, D)
            idx = np.arange(case.B) if name in WC.WHOLE_BATCH else case.sample(cus())
            cache[(name, D)] = (idx,) + WC.oracle_pooled(case, idx, chunk=4)
        return cache[(name, D)]
    return get


def errors(got, ref):
    dd = np.abs(got.astype(np.float64) - ref)
    scale = np.abs(ref).max()
    return (float(dd.max() / scale), float(np.sqrt(np.mean(dd * dd)) / np.sqrt(np.mean(ref * ref))),
            float(np.max(dd / np.maximum(np.abs(ref), 1e-3 * scale))))


@pytest.mark.parametrize("name,D", ALL)
def test_wide_fuzz_against_the_oracle(name, D, natural, reference):
    case = WC.build(name, D)
    out = natural(name, D)
    idx, rc, ra = reference(name, D)
    ref = np.concatenate([rc, ra])
    err = {}
    for mode in WC.MODES:
        pc, pa = out[mode]
        assert np.isfinite(pc).all() and np.isfinite(pa).all(), mode
        err[mode] = errors(np.concatenate([pc[idx], pa[idx]]), ref)
        print(f"{name} D={D} {mode}: max {err[mode][0]:.3e} rms {err[mode][1]:.3e} elementwise {err[mode][2]:.3e}")
        for g, (got, p) in enumerate(((pc, "cat"), (pa, "an"))):     # no atom, nothing pooled: exactly 0
            none = ~case.inputs[f"{p}_atom"].any(axis=1)
            assert none[0] and none[-1] and not got[none].any(), (mode, p)
    assert_close(out["f32t"][0][idx], rc, what=f"{name} D={D} f32t cat pooled")
    assert_close(out["f32t"][1][idx], ra, what=f"{name} D={D} f32t an pooled")
    for i in range(3):
        assert err["f32x3"][i] <= 2.0 * err["f32t"][i] + 1e-7, err
    assert err["f32x3"][0] <= 1e-5 and err["f32t"][0] <= 1e-5, err


@pytest.mark.parametrize("mode", WC.MODES)
@pytest.mark.parametrize("name,D", [(n, D) for n in WC.HALF_EXPECT for D in WC.DIMS])
def test_wide_fuzz_shard_concat_bitwise(name, D, mode, natural):
    """The halves take other kernels than the whole batch (asserted) and agree with it bit for bit."""
    case = WC.build(name, D)
    case.check_half_premises(cus())
    pc, pa = natural(name, D)[mode]
    m, d, h = make_model(case, mode), to_dev(case.inputs), case.half()
    c0, a0 = m.encode_pooled({k: v[:h].contiguous() for k, v in d.items()}, fused=True)
    c1, a1 = m.encode_pooled({k: v[h:].contiguous() for k, v in d.items()}, fused=True)
    assert np.array_equal(torch.cat([c0, c1]).cpu().numpy(), pc) and np.array_equal(torch.cat([a0, a1]).cpu().numpy(), pa)


@pytest.mark.parametrize("mode", WC.MODES)
@pytest.mark.parametrize("name,D", ALL)
def test_wide_fuzz_plan_then_run_equals_one_call(name, D, mode, natural):
    case = WC.build(name, D)
    pc, pa = natural(name, D)[mode]
    m, d = make_model(case, mode), to_dev(case.inputs)
    for _ in range(2):                       # both workspaces of the pipeline exist ...
        m.encode_pooled(d, plan=m.plan_batch(d))
    torch.cuda.synchronize()
    for slot in m._pipeline.slots:           # ... and hold 0xff bytes: nothing may be read that this plan did not write
        slot["ws"].fill_(0xFF)
    plan = m.plan_batch(d)
    assert plan.mode == mode
    c, a = m.encode_pooled(d, plan=plan)
    assert np.array_equal(c.cpu().numpy(), pc) and np.array_equal(a.cpu().numpy(), pa)


# ------------------------------------------------------------------------------------------------------------
# forced paths: one fresh process per setting
# ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def children(tmp_path_factory, natural):
    """setting -> (npz path or None, what went wrong).  One child at a time, each a new process.  A child that ends by
    a signal, by exit 134 / 139, by a GPU fault or by its time limit is a finding: no further child is started, and
    every test that depends on one fails with the child's stderr."""
    for v in OVERRIDES:
        assert v not in os.environ, f"{v} is set in the parent's environment"
    out_dir = tmp_path_factory.mktemp("wide_children")
    child = str(Path(__file__).resolve().parent / "wide_child.py")
    specs = [f"{name}:{D}" for name, D in ALL]
    res, stop = {}, None
    try:                                   # nothing is started on a device that the in-process tests have faulted
        torch.cuda.synchronize()
    except RuntimeError as e:
        stop = ("in-process", str(e))
    for key, env in SETTINGS.items():
        if stop is not None:
            res[key] = (None, f"not started: {stop[0]!r} ended abnormally\n{stop[1]}")
            continue
        out = out_dir / f"{key}.npz"
        try:
            r = subprocess.run([sys.executable, child, str(out), *specs], env={**os.environ, **env},
                               timeout=CHILD_TIMEOUT, capture_output=True, text=True)
        except subprocess.TimeoutExpired as e:
            stop = (key, f"time limit of {CHILD_TIMEOUT} s\n{e.stderr or ''}")
            res[key] = (None, stop[1])
            continue
        fault = "illegal memory access" in r.stderr or "HSA_STATUS_ERROR" in r.stderr
        if r.returncode < 0 or r.returncode in (134, 139) or fault:
            stop = (key, f"exit status {r.returncode}\n{r.stderr[-4000:]}")
            res[key] = (None, stop[1])
        elif r.returncode != 0 or not out.exists():
            res[key] = (None, f"exit status {r.returncode}\n{r.stderr[-4000:]}")
        else:
            res[key] = (out, "")
    return res


def bits(x):
    """The uint32 image of a float32 array with -0 mapped to +0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return np.where(x == 0, np.float32(0), x).view(np.uint32)


@pytest.mark.parametrize("name,D", ALL)
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_wide_fuzz_forced_paths_agree_bitwise(setting, name, D, natural, children):
    out, why = children[setting]
    assert out is not None, f"child {setting} {SETTINGS[setting]}: {why}"
    z = np.load(out)
    for mode in WC.MODES:
        pc, pa = natural(name, D)[mode]
        for got, want, p in ((z[f"{name}/{D}/{mode}/cat"], pc, "cat"), (z[f"{name}/{D}/{mode}/an"], pa, "an")):
            same = bits(got) == bits(want)
            assert same.all(), (f"{setting} {SETTINGS[setting]}: {name} D={D} {mode} {p}: {int((~same).sum())} of "
                                f"{same.size} values differ, in molecules {np.flatnonzero(~same.all(axis=1))[:12]}, "
                                f"max |diff| {np.abs(got.astype(np.float64) - want).max():.3e}")
