"""CPU-only checks of the lookahead of a sensor network (include/ssa_hip.h: ssa_lookahead_sensors_f64; SSA_Tasker_Env.lookahead_sensors):
the export, refusal of bad arguments before any launch, no CPU fallback, and the new kernels' resource budget in the shipped code object
against the single-sensor lookahead's."""
import re

import pytest

from support.codeobj import KERNEL_FAMILIES, _kernels, assert_family_budget, header
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.refusals import LOOK_PTRS, OUT_PTRS, bad_rk4, nan_mask, refused


def test_lookahead_sensors_is_exported_and_declared(lib):
    from ssa_gym_amd import _lib
    hdr = header()
    assert re.search(r"\bint\s+ssa_lookahead_sensors_f64\s*\(\s*const ssa_consts\s*\*\s*\w+\s*,\s*const ssa_step_params\s*\*\s*\w+\s*,"
                     r"\s*const ssa_sensor_params\s*\*\s*\w+\s*,\s*const ssa_lookahead_out\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)", hdr)
    assert "ssa_lookahead_sensors_f64" in _lib.SIGNATURES
    assert hasattr(lib, "ssa_lookahead_sensors_f64")


def test_lookahead_sensors_refuses_bad_arguments_before_any_launch(lib):
    """NULL blocks or required outputs, 0 or more than 8 sensors, a NaN elevation mask, an unknown observation type or propagator, a bad
    RK4 substep count, too many objects -> SSA_E_INVALID; several envs -> SSA_E_UNSUPPORTED.  No case reaches a launch (no device is
    touched: this runs without a GPU)."""
    from ssa_gym_amd import _lib
    f = lib.ssa_lookahead_sensors_f64
    for k in range(4):                                                     # NULL blocks
        assert refused(f, None, null=k) == _lib.E_INVALID, k
    invalid = [("sp", "n_sensor", 0), ("sp", "n_sensor", -1), ("sp", "n_sensor", 9), ("p", "n_obj", 0), ("p", "n_obj", 1 << 31),
               ("c", "obs_type", 99), ("c", "propagator", 99)]
    invalid += [("o", nm, 0) for nm in OUT_PTRS] + [("p", nm, 0) for nm in LOOK_PTRS]
    for case in invalid:
        assert refused(f, None, case) == _lib.E_INVALID, case
    assert refused(f, None, ("p", "n_env", 2)) == _lib.E_UNSUPPORTED
    assert refused(f, None, spoil=bad_rk4) == _lib.E_INVALID
    assert refused(f, None, spoil=nan_mask) == _lib.E_INVALID


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
    assert_family_budget(kern, ins_of, "lookahead_sensors_kernel", "lookahead_kernel", KERNEL_FAMILIES["lookahead_sensors_kernel"])
