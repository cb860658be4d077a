"""CPU-only checks of the lookahead of a sensor network (include/ssa_hip.h: ssa_lookahead_sensors_f64; SSA_Tasker_Env.lookahead_sensors):
the export, refusal of bad arguments before any launch, no CPU fallback, and the new kernels' resource budget in the shipped code object
against the single-sensor lookahead's."""
import ctypes as C
import re

import pytest

from support.codeobj import _kernels, header, stray_scratch
from support.gpu import lib  # noqa: F401  (the module fixture)


def test_lookahead_sensors_is_exported_and_declared(lib):
    from ssa_gym_amd import _lib
    hdr = header()
    assert re.search(r"\bint\s+ssa_lookahead_sensors_f64\s*\(\s*const ssa_consts\s*\*\s*\w+\s*,\s*const ssa_step_params\s*\*\s*\w+\s*,"
                     r"\s*const ssa_sensor_params\s*\*\s*\w+\s*,\s*const ssa_lookahead_out\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)", hdr)
    assert "ssa_lookahead_sensors_f64" in _lib.SIGNATURES
    assert hasattr(lib, "ssa_lookahead_sensors_f64")


def _valid_blocks():
    """argument blocks that pass every check but the one a case breaks (the pointers are never dereferenced: each case is refused)"""
    from ssa_gym_amd import _lib
    c, p, sp, o = _lib.ssa_consts(), _lib.ssa_step_params(), _lib.ssa_sensor_params(), _lib.ssa_lookahead_out()
    c.obs_type, c.propagator, c.rk4_substeps = _lib.OBS_AER, _lib.PROP_FG, 4
    p.n_obj, p.n_env = 8, 1
    p.x_true_in = p.x_in = p.P_in = p.status = p.trans = p.env_time = 16
    o.score = o.status = o.visible = 16
    sp.n_sensor = 2
    return c, p, sp, o


def test_lookahead_sensors_refuses_bad_arguments_before_any_launch(lib):
    """NULL blocks or required outputs, 0 or more than 8 sensors, a NaN elevation mask, an unknown observation type or propagator, a bad
    RK4 substep count, too many objects -> SSA_E_INVALID; several envs -> SSA_E_UNSUPPORTED.  No case reaches a launch (no device is
    touched: this runs without a GPU)."""
    from ssa_gym_amd import _lib
    f = lib.ssa_lookahead_sensors_f64
    c, p, sp, o = _valid_blocks()
    r = C.byref
    assert f(None, r(p), r(sp), r(o), None) == _lib.E_INVALID
    assert f(r(c), None, r(sp), r(o), None) == _lib.E_INVALID
    assert f(r(c), r(p), None, r(o), None) == _lib.E_INVALID
    assert f(r(c), r(p), r(sp), None, None) == _lib.E_INVALID

    def refused(code, **change):
        c, p, sp, o = _valid_blocks()
        for k, v in change.items():
            blk, field = k.split("_", 1)
            setattr({"c": c, "p": p, "s": sp, "o": o}[blk], field, v)
        assert f(r(c), r(p), r(sp), r(o), None) == code, change

    for bad in (0, -1, 9):
        refused(_lib.E_INVALID, s_n_sensor=bad)
    refused(_lib.E_UNSUPPORTED, p_n_env=2)
    for out in ("score", "status", "visible"):
        refused(_lib.E_INVALID, **{"o_" + out: 0})
    for ptr in ("x_true_in", "x_in", "P_in", "status", "trans", "env_time"):
        refused(_lib.E_INVALID, **{"p_" + ptr: 0})
    refused(_lib.E_INVALID, p_n_obj=0)
    refused(_lib.E_INVALID, p_n_obj=1 << 31)
    refused(_lib.E_INVALID, c_obs_type=99)
    refused(_lib.E_INVALID, c_propagator=99)
    c, p, sp, o = _valid_blocks()
    c.propagator, c.rk4_substeps = _lib.PROP_J2_RK4, 0
    assert f(r(c), r(p), r(sp), r(o), None) == _lib.E_INVALID
    c, p, sp, o = _valid_blocks()
    sp.obs_limit[1] = float("nan")
    assert f(r(c), r(p), r(sp), r(o), None) == _lib.E_INVALID


def test_env_lookahead_sensors_has_no_cpu_fallback(lib):
    from ssa_gym_amd import _lib
    from ssa_gym_amd.envs.ssa_tasker_simple_2 import SSA_Tasker_Env
    env = SSA_Tasker_Env.__new__(SSA_Tasker_Env)     # (an env without device state: what a machine without a GPU has)
    env._engine, env.i, env.n = None, 0, 480
    with pytest.raises(_lib.SsaHipError):
        env.lookahead_sensors()
    with pytest.raises(_lib.SsaHipError):
        env.lookahead_sensors(covariances=True)


def test_lookahead_sensors_kernels_keep_the_lookahead_kernels_budget(tmp_path):
    """each of the eight instances (4 propagators x {one tile, multi tile}) within lookahead_kernel of the same propagator and launch
    form: at most 96 VGPRs, the same LDS, no more scratch and no more VGPR spills; scratch touched only around the out-of-line calls of
    SSA_PROP_ELEMENTS / SSA_PROP_HYBRID; FG and J2 without calls or scratch"""
    kern, ins_of = _kernels(tmp_path)
    new = sorted(k for k in kern if "lookahead_sensors_kernel" in k)
    assert len(new) == 8, new
    checked = 0
    for name, ins in ins_of.items():
        if "lookahead_sensors_kernel" not in name:
            continue
        form = re.search(r"ILi(\d)ELb(\d)E", name).group(0)
        ref = [k for k in kern if "lookahead_kernel" in k and "lookahead_sensors" not in k and form in k]
        assert len(ref) == 1, (name, ref)
        k, b = kern[name], kern[ref[0]]
        assert k["vgpr_count"] <= 96, (name, k)
        assert k["group_segment_fixed_size"] == b["group_segment_fixed_size"], (name, k, b)
        assert k["private_segment_fixed_size"] <= b["private_segment_fixed_size"], (name, k, b)
        assert k["vgpr_spill_count"] <= b["vgpr_spill_count"], (name, k, b)
        calls = [i for i, op in enumerate(ins) if op == "s_swappc_b64"]
        stray = stray_scratch(ins)
        assert not stray, (name, stray[:8])
        if form.startswith(("ILi1", "ILi2")):     # FG / J2: no call, no scratch at all
            assert not calls and k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        checked += 1
    assert checked == 8
