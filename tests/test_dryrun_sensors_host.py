"""CPU-only checks of the dry run of candidate schedules (include/ssa_hip.h: ssa_dryrun_sensors_envs_f64; device.dryrun_rows;
SSA_Tasker_Env.evaluate_schedules; agents.refine_plan_sensors): the export, the parameter block's layout against the header, every
refusal before any launch, the env's and the planner's guards without device state, the host-side row builder, the planner on a stubbed
evaluator, and the new kernels' resource budget in the shipped code object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from support.codeobj import _kernels, assert_family_budget, header
from support.dryrun import ENTRY, StubEnv, refused
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.refusals import LOOK_PTRS, bad_rk4, nan_mask
from support.sensors import _bare_env


def test_the_entry_is_exported_declared_and_bound(lib):
    from ssa_gym_amd import _lib
    hdr = header()
    assert re.search(r"\bint %s\s*\(" % ENTRY, hdr) and re.search(r"\}\s*ssa_dryrun_sensors_params\s*;", hdr)
    assert ENTRY in _lib.SIGNATURES and hasattr(lib, ENTRY)
    res, args = _lib.SIGNATURES[ENTRY]
    assert res is C.c_int and len(args) == 5 and args[3] is C.POINTER(_lib.ssa_dryrun_sensors_params)
    assert lib.ssa_abi_version() == _lib.ABI_VERSION == 23          # (additive: the ABI version stays)
    assert re.search(r"#define\s+SSA_ABI_VERSION\s+23\b", hdr)
    for name in ("STRIDE", "ACTION", "VISIBLE", "TAKEN", "STATUS", "SCORE", "SPARE"):
        assert int(re.search(r"#define\s+SSA_DRY_%s\s+(\d+)" % name, hdr).group(1)) == getattr(_lib, "DRY_" + name), name
    assert _lib.DRY_SCORE + _lib.LOOK_NSCORE == _lib.DRY_SPARE == _lib.DRY_STRIDE - 1


def test_params_layout_matches_the_header(tmp_path):
    from ssa_gym_amd import _lib
    st = _lib.ssa_dryrun_sensors_params
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssa_hip.h"', 'int main(void){',
           'printf("%zu\\n", sizeof(ssa_dryrun_sensors_params));']
    want = [C.sizeof(st)]
    for f, _ in st._fields_:
        src.append('printf("%%zu\\n", offsetof(ssa_dryrun_sensors_params, %s));' % f)
        want.append(getattr(st, f).offset)
    src.append('return 0;}')
    c = tmp_path / "dry.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "dry"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).decode().split()] == want


def test_dry_run_refuses_bad_arguments_before_any_launch(lib):
    """every refusal the header lists, each from otherwise complete blocks and with its code; nothing is launched (no device is
    touched: this runs without a GPU)"""
    from ssa_gym_amd import _lib
    fn = getattr(lib, ENTRY)
    for k in range(4):                                                     # NULL blocks, `d` among them
        assert refused(fn, null=k) == _lib.E_INVALID, k
    invalid = [("d", "n_steps", 0), ("d", "n_steps", -2), ("d", "actions", 0), ("d", "actions", 0x1004), ("d", "actions", 0x1010),
               ("d", "out", 0), ("d", "n_obj_caller", 0), ("d", "n_obj_caller", -7),
               ("p", "n_obj", 0), ("p", "n_obj", -4), ("p", "n_env", 0), ("p", "n_env", -1),
               ("c", "propagator", 7), ("c", "obs_type", 5), ("sp", "n_sensor", 0), ("sp", "n_sensor", -1), ("sp", "n_sensor", 9)]
    invalid += [("p", nm, 0) for nm in LOOK_PTRS]                          # a NULL input
    for case in invalid:
        assert refused(fn, case) == _lib.E_INVALID, case
    assert refused(fn, spoil=nan_mask) == _lib.E_INVALID
    assert refused(fn, spoil=bad_rk4) == _lib.E_INVALID
    # the rows and the records are 32-bit counts: n_env * n_obj, n_env * n_sensor * n_obj and n_env * n_sensor * n_steps below 2^31
    assert refused(fn, ("p", "n_obj", 1 << 30)) == _lib.E_INVALID
    assert refused(fn, ("p", "n_obj", 1 << 28), ("sp", "n_sensor", 4)) == _lib.E_INVALID
    assert refused(fn, ("d", "n_steps", 1 << 29)) == _lib.E_INVALID       # 2 x 2 x 2^29 records
    assert refused(fn, ("d", "n_steps", (1 << 29) - 1), ("d", "out", 0)) == _lib.E_INVALID      # (in range: refused for the NULL output)
    # whole tiles per pseudo-env
    assert refused(fn, ("p", "n_obj", 6)) == _lib.E_UNSUPPORTED
    assert refused(fn, n_env=3, n_obj=7) == _lib.E_UNSUPPORTED
    assert refused(fn, ("p", "obj_ids", 0x1000), n_obj=6) == _lib.E_UNSUPPORTED
    # n_env == 1 takes any n_obj (the full-catalogue form): what is refused for these blocks is one of the dry run's own checks
    assert refused(fn, ("d", "n_steps", 0), n_env=1, n_obj=7) == _lib.E_INVALID
    assert refused(fn, ("d", "out", 0), n_env=1, n_obj=7) == _lib.E_INVALID
    assert refused(fn, ("d", "actions", 0x1008), n_env=1, n_obj=403) == _lib.E_INVALID


def test_totals_entry_is_exported_and_refuses_bad_arguments(lib):
    """ssa_dryrun_totals_f64: declared, bound, and every refusal of its header comment before any launch"""
    from ssa_gym_amd import _lib
    assert re.search(r"\bint ssa_dryrun_totals_f64\s*\(", header()) and "ssa_dryrun_totals_f64" in _lib.SIGNATURES
    fn = lib.ssa_dryrun_totals_f64
    good = dict(records=0x1000, n_env=2, n_steps=3, n_sensor=2, total=0x2000)
    order = ("records", "n_env", "n_steps", "n_sensor", "total")
    for name, value in (("records", 0), ("total", 0), ("n_env", 0), ("n_env", -1), ("n_steps", 0), ("n_sensor", 0), ("n_sensor", 9),
                        ("n_steps", 1 << 29)):
        args = dict(good, **{name: value})
        assert fn(*[args[k] for k in order], None) == _lib.E_INVALID, (name, value)


def test_env_and_planner_raise_without_device_state():
    from ssa_gym_amd import _lib, agents
    for S in (1, 3):
        env = _bare_env(S)
        sched = np.zeros((2, S), dtype=np.int64)
        with pytest.raises(_lib.SsaHipError, match="no device state"):
            env.evaluate_schedules(sched)
        with pytest.raises(_lib.SsaHipError, match="no device state"):
            env.evaluate_schedules(sched[None])
        with pytest.raises(_lib.SsaHipError, match="no device state"):
            agents.refine_plan_sensors(env, sched)
    eng_cls = __import__("ssa_gym_amd.engine", fromlist=["HotPathEngine"]).HotPathEngine
    eng = eng_cls.__new__(eng_cls)
    eng.E, eng.m = 3, 8
    with pytest.raises(_lib.SsaHipError, match="one env"):                 # (before anything of the engine is read)
        eng.launch_dryrun_sensors(0, 1, None, sched[None])


def test_row_builder_on_hand_made_candidates():
    """the distinct valid objects of each candidate, ascending, padded with -1 to whole tiles; the action words [K, B, 8], an idle entry as -1"""
    from ssa_gym_amd import _lib, device
    m = 20
    cand = np.array([[[7, 3], [3, 7], [7, -1]],                  # duplicates across steps: two objects
                     [[-1, -4], [20, 999], [-1, -1]],            # all idle: negative and out of range
                     [[0, 1], [2, 3], [4, 19]],                  # six objects: W rounds up to 8
                     [[5, 5], [5, 5], [5, 5]]])                  # a duplicate within every row: one object
    ids, words = device.dryrun_rows(cand, m)
    assert ids.dtype == np.int32 and words.dtype == np.int32
    assert ids.shape == (4, 8) and words.shape == (3, 4, _lib.MAX_SENSORS)
    assert ids[0].tolist() == [3, 7] + [-1] * 6
    assert ids[1].tolist() == [-1] * 8
    assert ids[2].tolist() == [0, 1, 2, 3, 4, 19, -1, -1]
    assert ids[3].tolist() == [5] + [-1] * 7
    assert np.array_equal(words[:, :, :2], np.maximum(cand, -1).transpose(1, 0, 2)) and (words[:, :, 2:] == -1).all()      # (idle is -1)
    for n, W in ((1, 4), (4, 4), (5, 8), (8, 8), (9, 12)):       # W = 4 ceil(distinct / 4)
        one = np.arange(n).reshape(1, n, 1)
        assert device.dryrun_rows(one, m)[0].shape == (1, W), n
    assert device.dryrun_rows(np.full((2, 3, 1), -1), m)[0].shape == (2, 4)      # an all-idle batch keeps one tile per candidate
    big = np.array([[[2 ** 40, 1]]])                             # (beyond int32: idle, not wrapped into range)
    ids, words = device.dryrun_rows(big, m)
    assert ids[0].tolist() == [1, -1, -1, -1] and words[0, 0, 0] >= m
    for bad in (cand[0], cand.astype(float), np.zeros((1, 2, 9), int), np.zeros((1, 0, 2), int)):
        with pytest.raises(ValueError):
            device.dryrun_rows(bad, m)
    with pytest.raises(ValueError):
        device.dryrun_rows(cand, m, n_sensor=3)


def test_refine_with_one_candidate_returns_its_plan_unchanged():
    """candidates=1: the incumbent alone -- no forecast, no draw, one evaluation of the plan as given, its total returned"""
    from ssa_gym_amd import agents
    env = StubEnv()
    plan = np.array([[4, 7], [1, 4], [9, 0]])
    out, total = agents.refine_plan_sensors(env, plan, rounds=3, candidates=1)
    assert np.array_equal(out, plan) and out is not plan and out.dtype == np.int64
    assert env.forecasts == 0 and len(env.calls) == 1 and np.array_equal(env.calls[0][0], plan)
    assert total.tolist() == [-25.0, 50.0, 25.0]


def test_refine_keeps_the_first_best_candidate_and_its_own_generator():
    """on the stub a schedule is worth the sum of its entries: every round's winner is the first candidate with the largest total, the
    incumbent is candidate 0, a redrawn slot never repeats an object of its row, the same seed gives the same plan, and the global numpy
    generator is not drawn from"""
    from ssa_gym_amd import _lib, agents
    plan = np.array([[0, 1], [1, 0], [2, 3]])
    state = np.random.get_state()[1].copy()
    env = StubEnv()
    out, total = agents.refine_plan_sensors(env, plan, kind='info', rounds=3, candidates=8, seed=4)
    assert np.array_equal(np.random.get_state()[1], state)
    assert env.forecasts == 1 and len(env.calls) == 3
    inc = plan
    for cand in env.calls:
        assert cand.shape == (8, 3, 2) and np.array_equal(cand[0], inc)
        assert all(len(set(r.tolist())) == 2 for c in cand for r in c)
        assert all((c != inc).sum() <= 1 for c in cand)
        tot = cand.reshape(8, -1).sum(axis=1)
        inc = cand[int(np.argmax(tot))]
    assert np.array_equal(out, inc) and total[_lib.LOOK_INFO_GAIN] == out.sum() >= plan.sum()
    again, _ = agents.refine_plan_sensors(StubEnv(), plan, rounds=3, candidates=8, seed=4)
    assert np.array_equal(again, out)
    worst, _ = agents.refine_plan_sensors(StubEnv(), plan, kind='trace', rounds=2, candidates=8, seed=4)   # (column 0 = -sum)
    assert worst.sum() <= plan.sum()
    with pytest.raises(ValueError):
        agents.refine_plan_sensors(StubEnv(), plan, kind='gain')
    with pytest.raises(ValueError):
        agents.refine_plan_sensors(StubEnv(), plan[:, :1])


def test_new_kernels_keep_the_rollout_kernels_budget(tmp_path):
    """exactly four dryrun_sensors_kernel instances; each fits 96 VGPRs, uses the LDS of rollout_sensor_envs_kernel's instance of the
    same propagator and no more scratch or VGPR spills than it, and touches scratch only around the out-of-line calls
    (SSA_PROP_ELEMENTS / SSA_PROP_HYBRID) -- FG and J2 none at all"""
    kern, ins_of = _kernels(tmp_path)
    assert_family_budget(kern, ins_of, "dryrun_sensors_kernel", "rollout_sensor_envs_kernel", 4)
