"""CPU-only checks of a sensor network's tasking forecast (include/ssa_hip.h: ssa_forecast_sensors_f64; SSA_Tasker_Env.forecast_sensors;
agents.plan_info_gain_sensors / plan_trace_gain_sensors): the export, the parameter block's layout against the header, refusal of bad
arguments before any launch, the env's and the planners' guards without device state, the planner's host fill-in, and the new kernels'
resource budget in the shipped code object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from support.codeobj import KERNEL_FAMILIES, _kernels, assert_family_budget, header
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.refusals import LOOK_PTRS, OUT_PTRS, bad_rk4, nan_mask, refused
from support.sensors import _bare_env


def test_forecast_is_exported_and_declared(lib):
    from ssa_gym_amd import _lib
    hdr = header()
    assert re.search(r"\bint ssa_forecast_sensors_f64\s*\(", hdr)
    assert re.search(r"\}\s*ssa_forecast_params\s*;", hdr)
    assert "ssa_forecast_sensors_f64" in _lib.SIGNATURES
    assert hasattr(lib, "ssa_forecast_sensors_f64")
    assert lib.ssa_abi_version() == _lib.ABI_VERSION == 23          # (additive: the ABI version stays)


def test_forecast_params_layout_matches_the_header(lib, tmp_path):
    from ssa_gym_amd import _lib
    st, lo = _lib.ssa_forecast_params, _lib.ssa_lookahead_out
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssa_hip.h"', 'int main(void){',
           'printf("%zu\\n", sizeof(ssa_forecast_params));']
    want = [C.sizeof(st)]
    for f, _ in st._fields_:
        src.append('printf("%%zu\\n", offsetof(ssa_forecast_params, %s));' % f)
        want.append(getattr(st, f).offset)
    for f, _ in lo._fields_:                                         # (the nested output block, member by member)
        src.append('printf("%%zu\\n", offsetof(ssa_forecast_params, out.%s));' % f)
        want.append(st.out.offset + getattr(lo, f).offset)
    src.append('return 0;}')
    c = tmp_path / "fc.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "fc"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).decode().split()] == want


def test_forecast_refuses_bad_arguments_before_any_launch(lib):
    """every refusal of ssa_lookahead_sensors_f64, n_steps < 1 and a NULL required output: each with its code and nothing launched (no
    device is touched: this runs without a GPU).  Every case spoils ONE field of blocks that are otherwise complete."""
    from ssa_gym_amd import _lib
    fn = lib.ssa_forecast_sensors_f64
    for k in range(4):                                                     # NULL blocks
        assert refused(fn, None, null=k) == _lib.E_INVALID, k
    invalid = [("f", "n_steps", 0), ("f", "n_steps", -2), ("p", "n_obj", 0), ("p", "n_obj", -4),
               ("c", "propagator", 7), ("c", "obs_type", 5), ("sp", "n_sensor", 0), ("sp", "n_sensor", -1), ("sp", "n_sensor", 9),
               ("p", "n_obj", (1 << 31) // 2)]                             # (S * m = 2^31 rows)
    invalid += [("o", nm, 0) for nm in OUT_PTRS] + [("p", nm, 0) for nm in LOOK_PTRS]
    for case in invalid:
        assert refused(fn, None, case) == _lib.E_INVALID, case
    assert refused(fn, None, spoil=nan_mask) == _lib.E_INVALID
    assert refused(fn, None, spoil=bad_rk4) == _lib.E_INVALID
    assert refused(fn, None, ("p", "n_env", 2)) == _lib.E_UNSUPPORTED


def test_env_and_planners_raise_without_device_state():
    from ssa_gym_amd import _lib, agents
    for S in (1, 3):
        env = _bare_env(S)
        with pytest.raises(_lib.SsaHipError):
            env.forecast_sensors(3)
        with pytest.raises(_lib.SsaHipError):
            env.forecast_sensors(3, covariances=True)
        with pytest.raises(_lib.SsaHipError):
            agents.plan_info_gain_sensors(env, 3)
        with pytest.raises(_lib.SsaHipError):
            agents.plan_trace_gain_sensors(env, 3)


def test_planner_fills_unassigned_entries_on_the_host():
    """-1 entries of a hand-made plan: each becomes an object in range that no sensor of its row holds, drawn from the action space's
    generator; assigned entries stay; env.np_random is not touched; the same seed gives the same plan"""
    from ssa_gym_amd import agents
    raw = np.array([[4, -1, 7], [-1, -1, -1], [0, 1, 2], [9, -1, -1], [-1, 3, -1]])

    def fill(seed):
        env = _bare_env(3, m=10)
        env.action_space.seed(seed)
        draws = env.np_random.get_state()[2]
        plan = agents._fill_plan(env, raw)
        assert env.np_random.get_state()[2] == draws
        return plan
    plan = fill(1)
    assert plan.dtype == np.int64 and plan.shape == raw.shape
    assert np.array_equal(plan[raw >= 0], raw[raw >= 0])
    assert ((plan >= 0) & (plan < 10)).all()
    assert all(len(set(row.tolist())) == 3 for row in plan)
    assert (raw[1] == -1).all()                                             # (the caller's array is not written)
    assert np.array_equal(plan, fill(1))
    one = agents._fill_plan(_bare_env(1, m=10), np.array([[-1], [5]]))      # (one site: a Discrete action space)
    assert one.shape == (2, 1) and 0 <= one[0, 0] < 10 and one[1, 0] == 5
    with pytest.raises(ValueError):                                         # more sensors than objects: nothing left to draw
        agents._fill_plan(_bare_env(3, m=2), np.array([[0, 1, -1]]))


def test_forecast_kernels_keep_the_lookahead_kernels_budget(tmp_path):
    """the four forecast_sensors_kernel instances fit 96 VGPRs (5 wavefronts per SIMD), use the LDS of lookahead_sensors_kernel's
    one-tile instance of the same propagator and no more scratch or VGPR spills than it, and touch scratch only around the out-of-line
    calls (SSA_PROP_ELEMENTS / SSA_PROP_HYBRID) -- FG and J2 none at all"""
    kern, ins_of = _kernels(tmp_path)
    assert_family_budget(kern, ins_of, "forecast_sensors_kernel", "lookahead_sensors_kernel", KERNEL_FAMILIES["forecast_sensors_kernel"])
