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
from support.codeobj import _kernels, header, stray_scratch
from support.gpu import lib  # noqa: F401  (the module fixture)
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


def _valid_blocks():
    """blocks that pass every check (the pointers are never dereferenced on the host: a refusal comes before any launch) -- each case
    below spoils exactly one field"""
    from ssa_gym_amd import _lib, host
    c = host.make_consts(np.eye(6), np.eye(3), 1e-4, 2.0, -3, 20.0, -np.pi / 2, np.array([0.6, -1.3, 20.0]))
    p, sp, f = _lib.ssa_step_params(), _lib.ssa_sensor_params(), _lib.ssa_forecast_params()
    p.n_obj, p.n_env = 8, 1
    p.x_true_in = p.x_in = p.P_in = p.status = p.trans = p.env_time = 0x1000
    sp.n_sensor = 2
    f.n_steps = 3
    f.out.score = f.out.status = f.out.visible = 0x1000
    return c, p, sp, f


def test_forecast_refuses_bad_arguments_before_any_launch(lib):
    """every refusal of ssa_lookahead_sensors_f64, n_steps < 1 and a NULL required output: each with its code and nothing launched (no
    device is touched: this runs without a GPU).  Every case spoils ONE field of blocks that are otherwise complete."""
    from ssa_gym_amd import _lib
    fn = lib.ssa_forecast_sensors_f64

    def call(spoil=None, null=None):
        c, p, sp, f = _valid_blocks()
        if spoil:
            spoil(c, p, sp, f)
        args = [C.byref(c), C.byref(p), C.byref(sp), C.byref(f)]
        if null is not None:
            args[null] = None
        return fn(*args, None)

    def setter(which, name, value):
        def spoil(c, p, sp, f):
            setattr(dict(c=c, p=p, sp=sp, f=f, o=f.out)[which], name, value)
        return spoil
    for k in range(4):                                                     # NULL blocks
        assert call(null=k) == _lib.E_INVALID, k
    invalid = [("f", "n_steps", 0), ("f", "n_steps", -2), ("p", "n_obj", 0), ("p", "n_obj", -4),
               ("c", "propagator", 7), ("c", "obs_type", 5), ("sp", "n_sensor", 0), ("sp", "n_sensor", -1), ("sp", "n_sensor", 9),
               ("p", "n_obj", (1 << 31) // 2)]                             # (S * m = 2^31 rows)
    invalid += [("o", nm, 0) for nm in ("score", "status", "visible")]
    invalid += [("p", nm, 0) for nm in ("x_true_in", "x_in", "P_in", "status", "trans", "env_time")]
    for which, name, value in invalid:
        assert call(setter(which, name, value)) == _lib.E_INVALID, (which, name, value)

    def nan_mask(c, p, sp, f):
        sp.obs_limit[1] = float("nan")
    assert call(nan_mask) == _lib.E_INVALID

    def bad_rk4(c, p, sp, f):
        c.propagator, c.rk4_substeps = _lib.PROP_J2_RK4, 0
    assert call(bad_rk4) == _lib.E_INVALID
    assert call(setter("p", "n_env", 2)) == _lib.E_UNSUPPORTED


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
    new = [k for k in kern if "forecast_sensors_kernel" in k]
    assert len(new) == 4, new
    checked = 0
    for name, ins in ins_of.items():
        if "forecast_sensors_kernel" not in name:
            continue
        prop = re.search(r"ILi(\d)E", name).group(1)
        ref = [k for k in kern if "lookahead_sensors_kernel" in k and "ILi%sELb0E" % prop in k]
        assert len(ref) == 1, (name, ref)
        k, b = kern[name], kern[ref[0]]
        assert k["vgpr_count"] <= 96 and k["group_segment_fixed_size"] == b["group_segment_fixed_size"], (name, k, b)
        assert k["private_segment_fixed_size"] <= b["private_segment_fixed_size"], (name, k, b)
        assert k["vgpr_spill_count"] <= b["vgpr_spill_count"], (name, k, b)
        calls = [i for i, op in enumerate(ins) if op == "s_swappc_b64"]
        assert not stray_scratch(ins), (name, stray_scratch(ins)[:8])
        if prop not in "03":
            assert not calls and k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        checked += 1
    assert checked == 4
