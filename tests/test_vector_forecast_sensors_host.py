"""CPU-only checks of a sensor network's H-step forecast in each of several envs (include/ssa_hip.h: ssa_forecast_sensors_envs_f64;
HotPathEngine.launch_forecast_sensors_envs; SSA_Tasker_VecEnv.forecast_sensors; agents.plan_info_gain_sensors / plan_trace_gain_sensors
on a vector env): the export, refusal of bad arguments before any launch, the vector env's and the planners' guards without device
state, the planners' host fill-in per env, and the new kernels' resource budget in the shipped code object."""
import ctypes as C
import re

import numpy as np
import pytest

from support.codeobj import KERNEL_FAMILIES, _kernels, assert_family_budget, header
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.refusals import LOOK_PTRS, OUT_PTRS, bad_rk4, nan_mask, refused, valid_blocks
from support.vector_dryrun import StubVecEnv
from support.vector_forecast import bare_vec


def test_the_entry_is_exported_declared_and_bound(lib):
    from ssa_gym_amd import _lib
    hdr = header()
    assert re.search(r"\bint ssa_forecast_sensors_envs_f64\s*\(", hdr)
    assert "ssa_forecast_sensors_envs_f64" in _lib.SIGNATURES and hasattr(lib, "ssa_forecast_sensors_envs_f64")
    res, args = _lib.SIGNATURES["ssa_forecast_sensors_envs_f64"]
    assert res is C.c_int and len(args) == 5 and args[3] is C.POINTER(_lib.ssa_forecast_params)      # (ssa_forecast_params reused)
    assert _lib.SIGNATURES["ssa_forecast_sensors_envs_f64"] == _lib.SIGNATURES["ssa_forecast_sensors_f64"]
    assert lib.ssa_abi_version() == _lib.ABI_VERSION == 23          # (additive: the ABI version stays)
    assert re.search(r"#define\s+SSA_ABI_VERSION\s+23\b", hdr)


def test_vector_forecast_refuses_bad_arguments_before_any_launch(lib):
    """every refusal of ssa_forecast_sensors_f64 but its n_env one, and those of ssa_lookahead_sensors_envs_f64: each with its code and
    nothing launched (no device is touched: this runs without a GPU).  Every case spoils ONE field of blocks that are otherwise
    complete."""
    from ssa_gym_amd import _lib
    fn = lib.ssa_forecast_sensors_envs_f64
    for k in range(4):                                                     # NULL blocks
        assert refused(fn, None, null=k) == _lib.E_INVALID, k
    invalid = [("f", "n_steps", 0), ("f", "n_steps", -2), ("p", "n_obj", 0), ("p", "n_obj", -4), ("p", "n_env", 0), ("p", "n_env", -1),
               ("c", "propagator", 7), ("c", "obs_type", 5), ("sp", "n_sensor", 0), ("sp", "n_sensor", -1), ("sp", "n_sensor", 9)]
    invalid += [("o", nm, 0) for nm in OUT_PTRS] + [("p", nm, 0) for nm in LOOK_PTRS]      # a NULL required output, a NULL input
    for case in invalid:
        assert refused(fn, None, case) == _lib.E_INVALID, case
    assert refused(fn, None, spoil=nan_mask) == _lib.E_INVALID
    assert refused(fn, None, spoil=bad_rk4) == _lib.E_INVALID
    # inline envs: at most SSA_INLINE_ENVS travel by value
    assert _lib.INLINE_ENVS == 8
    assert refused(fn, None, ("p", "n_env", 9), ("p", "n_obj", 8), ("p", "launch_mask", _lib.LAUNCH_INLINE_ENVS)) == _lib.E_INVALID
    # a step's rows are 32-bit: n_env * n_obj and n_env * n_sensor * n_obj below 2^31 (whole tiles per env in all three)
    assert refused(fn, None, ("p", "n_obj", 1 << 30)) == _lib.E_INVALID                                      # 2 x 2^30 objects
    assert refused(fn, None, ("p", "n_obj", 1 << 28), ("sp", "n_sensor", 4)) == _lib.E_INVALID               # 2 x 4 x 2^28 rows
    assert refused(fn, None, ("p", "n_env", 1), ("p", "n_obj", 1 << 28), ("sp", "n_sensor", 8)) == _lib.E_INVALID
    # whole tiles per env
    assert refused(fn, None, ("p", "n_obj", 6)) == _lib.E_UNSUPPORTED                                        # n_env = 2, n_obj = 6
    assert refused(fn, None, ("p", "n_env", 3), ("p", "n_obj", 7)) == _lib.E_UNSUPPORTED
    assert refused(fn, None, ("p", "n_obj", 6), ("p", "obj_ids", 0x1000)) == _lib.E_UNSUPPORTED
    # n_env == 1 takes any n_obj: what is refused for these blocks is one of the forecast's own checks
    assert refused(fn, None, ("p", "n_env", 1), ("p", "n_obj", 7), ("f", "n_steps", 0)) == _lib.E_INVALID
    assert refused(fn, None, ("p", "n_env", 1), ("p", "n_obj", 7), ("o", "score", 0)) == _lib.E_INVALID


def test_one_env_forecast_still_refuses_several_envs(lib):
    from ssa_gym_amd import _lib
    fn = lib.ssa_forecast_sensors_f64
    assert refused(fn, valid_blocks(fn.__name__, n_env=2)) == _lib.E_UNSUPPORTED


def test_engine_keeps_the_one_env_refusal_and_checks_the_horizon():
    """HotPathEngine.launch_forecast_sensors still covers one env; launch_forecast_sensors_envs refuses n_steps < 1 -- both before
    anything of the engine is read (an engine object without device state)"""
    from ssa_gym_amd import _lib, engine
    eng = engine.HotPathEngine.__new__(engine.HotPathEngine)
    eng.E, eng.m = 3, 8
    with pytest.raises(_lib.SsaHipError, match="one env"):
        eng.launch_forecast_sensors(0, 1, None, 3)
    for bad in (0, -1):
        with pytest.raises(_lib.SsaHipError, match="n_steps"):
            eng.launch_forecast_sensors_envs(0, 1, None, bad)


def test_vector_forecast_guards_need_no_device_state():
    for S in (1, 3):
        vec = bare_vec(S)
        for bad in (0, -3):
            with pytest.raises(ValueError, match="horizon"):
                vec.forecast_sensors(bad)
        vec.i[1] = vec.n - 1
        with pytest.raises(ValueError, match="no next step"):
            vec.forecast_sensors(4)
        with pytest.raises(ValueError, match="no next step"):
            vec.forecast_sensors(4, covariances=True)
        assert vec.tick == 0 and vec.i.tolist() == [0, vec.n - 1, 0]      # (nothing counted)


def test_planners_take_a_vector_env_and_raise_without_device_state():
    from ssa_gym_amd import _lib, agents
    for S in (1, 3):
        vec = bare_vec(S)
        for planner in (agents.plan_info_gain_sensors, agents.plan_trace_gain_sensors):
            with pytest.raises(_lib.SsaHipError, match="no device state"):      # (detected by num_envs: not the single env's _engine)
                planner(vec, 3)


def test_planner_fills_unassigned_entries_per_env_on_the_host():
    """a hand-made [E, H', S] plan: every -1 becomes an object in range that no sensor of its row holds; assigned entries stay; envs
    ascending, rows ascending, sensors ascending -- the draws of _fill_plan env by env from a space seeded alike; the envs' own
    generators are not touched"""
    from ssa_gym_amd import agents
    raw = np.array([[[4, -1, 7], [-1, -1, -1], [0, 1, 2]],
                    [[9, -1, -1], [-1, 3, -1], [5, 6, 8]],
                    [[-1, -1, -1], [1, -1, 0], [-1, 2, -1]]])
    vec = bare_vec(3, E=3, m=10, seed=1)
    vec._rng = [np.random.RandomState(7 + e) for e in range(3)]
    states = [r.get_state()[2] for r in vec._rng]
    plan = agents._fill_plan(vec, raw)
    assert states == [r.get_state()[2] for r in vec._rng]
    assert plan.dtype == np.int64 and plan.shape == raw.shape
    assert np.array_equal(plan[raw >= 0], raw[raw >= 0]) and (raw[0, 1] == -1).all()      # (the caller's array is not written)
    assert ((plan >= 0) & (plan < 10)).all()
    assert all(len(set(row.tolist())) == 3 for env in plan for row in env)
    twin = bare_vec(3, E=3, m=10, seed=1)
    want = np.stack([agents._fill_plan(twin, raw[e]) for e in range(3)])
    assert np.array_equal(plan, want)
    for bad in (raw[:2], raw.reshape(-1), raw[None]):                                     # neither [E, H', S] nor one env's [H', S]
        with pytest.raises(ValueError):
            agents._fill_plan(vec, bad)
    with pytest.raises(ValueError, match="a plan"):                                       # (one env's rows where every env's plan enters)
        agents.refine_plan_sensors(StubVecEnv(E=3, m=10, S=3), raw[0])
    with pytest.raises(ValueError):                                                       # more sensors than objects
        agents._fill_plan(bare_vec(3, E=1, m=2), np.array([[[0, 1, -1]]]))


def test_new_kernels_keep_the_forecast_kernels_budget(tmp_path):
    """exactly four forecast_sensor_envs_kernel instances, none under a name another host test counts kernels by; each fits 96 VGPRs,
    uses the LDS of forecast_sensors_kernel's instance of the same propagator and no more scratch or VGPR spills than it, has its
    argument layout (ForeSensK's), and touches scratch only around the out-of-line calls (SSA_PROP_ELEMENTS / SSA_PROP_HYBRID) -- FG and
    J2 none at all"""
    kern, ins_of = _kernels(tmp_path)
    assert_family_budget(kern, ins_of, "forecast_sensor_envs_kernel", "forecast_sensors_kernel",
                         KERNEL_FAMILIES["forecast_sensor_envs_kernel"], same_args=True)
