"""CPU-only checks of a sensor network's lookahead and assignment in each of several envs (include/ssa_hip.h:
ssa_lookahead_sensors_envs_f64, ssa_assign_sensors_envs_f64; SSA_Tasker_VecEnv.lookahead_sensors / step_agent; the sensor agents on a
vector env): the exports, refusal of bad arguments before any launch, the workspace query, the vector env's and the agents' guards
without device state, and the new kernels' resource budgets in the shipped code object."""
import ctypes as C
import re

import numpy as np
import pytest

from support.codeobj import KERNEL_FAMILIES, _kernels, assert_family_budget, family, header
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.refusals import LOOK_PTRS, OUT_PTRS, bad_rk4, nan_mask, refused, valid_blocks
from support.vector_forecast import bare_vec as _bare_vec

NEW = ("ssa_lookahead_sensors_envs_f64", "ssa_assign_sensors_envs_f64", "ssa_assign_sensors_envs_workspace_bytes")


def test_the_three_entries_are_exported_declared_and_bound(lib):
    from ssa_gym_amd import _lib
    hdr = header()
    assert re.search(r"\bint ssa_lookahead_sensors_envs_f64\s*\(", hdr)
    assert re.search(r"\bint ssa_assign_sensors_envs_f64\s*\(", hdr)
    assert re.search(r"\bint64_t ssa_assign_sensors_envs_workspace_bytes\s*\(", hdr)
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.SIGNATURES["ssa_assign_sensors_envs_workspace_bytes"][0] is C.c_int64
    assert len(_lib.SIGNATURES["ssa_assign_sensors_envs_f64"][1]) == 11 and len(_lib.SIGNATURES["ssa_lookahead_sensors_envs_f64"][1]) == 5
    assert lib.ssa_abi_version() == _lib.ABI_VERSION == 23          # (additive: the ABI version stays)
    assert re.search(r"#define\s+SSA_ABI_VERSION\s+23\b", hdr)


def test_vector_lookahead_refuses_bad_arguments_before_any_launch(lib):
    """everything ssa_lookahead_sensors_f64 refuses but its n_env rule, and the entry's own: each with its code and nothing launched (no
    device is touched: this runs without a GPU).  Every case spoils ONE field of blocks that are otherwise complete."""
    from ssa_gym_amd import _lib
    fn = lib.ssa_lookahead_sensors_envs_f64
    for k in range(4):                                                     # NULL blocks
        assert refused(fn, None, null=k) == _lib.E_INVALID, k
    invalid = [("p", "n_obj", 0), ("p", "n_obj", -4), ("p", "n_env", 0), ("p", "n_env", -1), ("c", "propagator", 7), ("c", "obs_type", 5),
               ("sp", "n_sensor", 0), ("sp", "n_sensor", -1), ("sp", "n_sensor", 9)]
    invalid += [("o", nm, 0) for nm in OUT_PTRS] + [("p", nm, 0) for nm in LOOK_PTRS]
    for case in invalid:
        assert refused(fn, None, case) == _lib.E_INVALID, case
    assert refused(fn, None, ("p", "n_env", 9), ("p", "launch_mask", _lib.LAUNCH_INLINE_ENVS)) == _lib.E_INVALID      # more envs than travel by value
    assert refused(fn, None, spoil=nan_mask) == _lib.E_INVALID
    assert refused(fn, None, spoil=bad_rk4) == _lib.E_INVALID
    # the output rows are 32-bit: n_env * n_obj and n_env * n_sensor * n_obj below 2^31 (whole tiles per env in both)
    assert refused(fn, None, ("p", "n_obj", 1 << 30)) == _lib.E_INVALID                                      # 2 x 2^30 objects
    assert refused(fn, None, ("p", "n_obj", 1 << 28), ("sp", "n_sensor", 4)) == _lib.E_INVALID               # 2 x 4 x 2^28 rows
    assert refused(fn, None, ("p", "n_env", 1), ("p", "n_obj", 1 << 28), ("sp", "n_sensor", 8)) == _lib.E_INVALID
    # whole tiles per env
    assert refused(fn, None, ("p", "n_obj", 6)) == _lib.E_UNSUPPORTED                                        # n_env = 2, n_obj = 6
    assert refused(fn, None, ("p", "n_env", 3), ("p", "n_obj", 7)) == _lib.E_UNSUPPORTED
    assert refused(fn, None, ("p", "n_obj", 6), ("p", "obj_ids", 0x1000)) == _lib.E_UNSUPPORTED
    # n_env == 1 takes any n_obj: what is refused for these blocks is one of the lookahead's own checks
    assert refused(fn, None, ("p", "n_env", 1), ("p", "n_obj", 7), ("o", "score", 0)) == _lib.E_INVALID


def test_one_env_lookahead_still_refuses_several_envs(lib):
    from ssa_gym_amd import _lib
    fn = lib.ssa_lookahead_sensors_f64
    assert refused(fn, valid_blocks(fn.__name__, n_env=2)) == _lib.E_UNSUPPORTED


def test_envs_workspace_query_is_the_one_env_query_rounded_per_env(lib):
    from ssa_gym_amd import _lib
    one, envs = lib.ssa_assign_sensors_workspace_bytes, lib.ssa_assign_sensors_envs_workspace_bytes
    for m in (1, 8, 512, 513, 1100, 20000, 33000):
        for S in (1, 3, 8):
            per = (one(m, S) + 63) // 64 * 64
            assert per >= one(m, S) > 0 and per % 64 == 0
            for E in (1, 2, 3, 9):
                assert envs(m, S, E) == E * per, (m, S, E)
    for bad in ((0, 3, 2), (8, 0, 2), (8, 9, 2), (8, 3, 0), (8, 3, -1), (1 << 31, 3, 1)):
        assert envs(*bad) == _lib.E_INVALID, bad


def test_envs_assignment_refuses_bad_arguments_before_any_launch(lib):
    """the refusals of ssa_assign_sensors_f64, n_env < 1, n_env * n_sensor * n_obj >= 2^31 and a workspace one byte short -- each from
    otherwise complete arguments, nothing launched"""
    from ssa_gym_amd import _lib
    fn = lib.ssa_assign_sensors_envs_f64
    m, S, E = 1100, 3, 2
    need = lib.ssa_assign_sensors_envs_workspace_bytes(m, S, E)
    ok = dict(score=0x10000, n_obj=m, n_sensor=S, n_env=E, column=_lib.LOOK_INFO_GAIN, fallback=None, action_out=0x20000, pick_out=None,
              workspace=0x30000, workspace_bytes=need)

    def call(**over):
        a = dict(ok, **over)
        return fn(a["score"], a["n_obj"], a["n_sensor"], a["n_env"], a["column"], a["fallback"], a["action_out"], a["pick_out"],
                  a["workspace"], a["workspace_bytes"], None)

    cases = [dict(score=None), dict(action_out=None), dict(action_out=0x20004), dict(action_out=0x20010), dict(column=-1), dict(column=3),
             dict(n_obj=0), dict(n_obj=-5), dict(n_obj=1 << 31), dict(n_sensor=0), dict(n_sensor=9), dict(n_env=0), dict(n_env=-2),
             dict(workspace=None), dict(workspace=0x30008), dict(workspace_bytes=need - 1), dict(workspace_bytes=0)]
    for over in cases:
        assert call(**over) == _lib.E_INVALID, over
    # 2^31 score rows: refused even with a workspace that large
    big = dict(n_obj=1 << 28, n_sensor=4, n_env=2)
    assert call(workspace_bytes=lib.ssa_assign_sensors_envs_workspace_bytes(1 << 28, 4, 2), **big) == _lib.E_INVALID
    assert call(n_obj=1 << 28, n_sensor=8, n_env=1, workspace_bytes=lib.ssa_assign_sensors_envs_workspace_bytes(1 << 28, 8, 1)) == _lib.E_INVALID


def test_step_agent_guards_come_before_the_gpu_is_touched():
    from ssa_gym_amd import agents
    from ssa_gym_amd.envs.vector_env import check_fallback_actions, sensor_agent_column
    from ssa_gym_amd import _lib
    assert sensor_agent_column(agents.agent_info_gain_sensors) == sensor_agent_column("agent_info_gain_sensors") == _lib.LOOK_INFO_GAIN
    assert sensor_agent_column(agents.agent_trace_gain_sensors) == sensor_agent_column("agent_trace_gain_sensors") == _lib.LOOK_TRACE_GAIN
    vec = _bare_vec(3)
    for bad in (agents.agent_info_gain, "agent_visible_greedy", agents.agent_shannon, None, 3):
        with pytest.raises(NotImplementedError, match="agent_info_gain_sensors and agent_trace_gain_sensors"):
            vec.step_agent(bad)
    with pytest.raises(NotImplementedError, match="observers"):
        _bare_vec(1).step_agent("agent_info_gain_sensors")
    ok = np.array([[0, 1, 2], [7, 7, -1], [8, 100, -5]])              # (any integer is taken as given)
    for bad in (ok[:2], ok[:, :2], ok.reshape(-1), ok[None]):
        with pytest.raises(ValueError, match=re.escape(str(np.asarray(bad).shape))):
            vec.step_agent("agent_trace_gain_sensors", fallback_actions=bad)
    with pytest.raises(ValueError, match="integer"):
        vec.step_agent("agent_trace_gain_sensors", fallback_actions=ok.astype(np.float64))
    assert np.all(vec.i == 0) and vec.tick == 0                       # (refused before anything was launched or counted)
    rows = check_fallback_actions(ok, 3, 3)
    assert rows.dtype == np.int32 and rows.shape == (3, _lib.MAX_SENSORS)
    assert np.array_equal(rows[:, :3], [[0, 1, 2], [7, 7, -1], [8, 100, -1]]) and np.all(rows[:, 3:] == -1)
    assert check_fallback_actions(np.array([[2 ** 40]]), 1, 1)[0, 0] == 2 ** 31 - 1      # (an int32 word: still out of range)


def test_vector_lookahead_guards_need_no_device_state():
    vec = _bare_vec(3)
    with pytest.raises(NotImplementedError, match="lookahead_sensors"):
        vec.lookahead()                                                # (a network: the message names the method that does it)
    vec.i[1] = vec.n - 1
    with pytest.raises(ValueError, match="no next step"):
        vec.lookahead_sensors()
    with pytest.raises(ValueError, match="no next step"):
        vec.lookahead_sensors(covariances=True)


def test_agents_fill_idle_sensors_of_a_vector_env_by_the_single_env_rule():
    """the rule the vector agents apply to the rows the device leaves at -1 (no device involved): envs ascending, sensors ascending, an
    object the env has not assigned, drawn from single_action_space"""
    from ssa_gym_amd import agents
    vec = _bare_vec(3, E=3, m=5)
    raw = np.array([[4, -1, 0], [-1, -1, -1], [1, 2, 3]], dtype=np.int64)
    vec.assign_sensors = lambda k: raw.copy()
    got = agents.agent_info_gain_sensors(None, vec)
    assert got.shape == (3, 3) and got.dtype == np.int64
    assert np.array_equal(got[2], raw[2]) and got[0, 0] == 4 and got[0, 2] == 0
    for row in got:
        assert len(set(row.tolist())) == 3 and row.min() >= 0 and row.max() < 5
    # the same draws as the rule applied by hand to a space seeded alike
    twin = _bare_vec(3, E=3, m=5)
    want = raw.copy()
    for row in want:
        taken = set(row[row >= 0].tolist())
        for s in np.flatnonzero(row < 0):
            row[s] = agents._draw_unassigned(twin, taken)
            taken.add(int(row[s]))
    assert np.array_equal(got, want)
    with pytest.raises(ValueError):                                    # more sensors than objects: nothing left to draw
        v2 = _bare_vec(3, E=1, m=2)
        v2.assign_sensors = lambda k: np.array([[0, 1, -1]])
        agents.agent_trace_gain_sensors(None, v2)


def test_new_kernels_keep_their_budgets(tmp_path):
    """the eight lookahead_sensor_envs_kernel instances fit 96 VGPRs, use the LDS of lookahead_sensors_kernel's instance of the same
    propagator and launch form and no more scratch or VGPR spills than it, and touch scratch only around the out-of-line calls
    (SSA_PROP_ELEMENTS / SSA_PROP_HYBRID) -- FG and J2 none at all; assign_sensors_envs_kernel meets assign_sensors_kernel's budget: no
    scratch, no spills, at most 128 VGPRs, LDS for the table and the flag only"""
    kern, ins_of = _kernels(tmp_path)
    assert_family_budget(kern, ins_of, "lookahead_sensor_envs_kernel", "lookahead_sensors_kernel",
                         KERNEL_FAMILIES["lookahead_sensor_envs_kernel"], same_args=True)      # (LookSensK's layout)
    from ssa_gym_amd import _lib
    for name in family(kern, "assign_sensors_envs_kernel") + family(kern, "assign_sensors_kernel"):
        k = kern[name]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["vgpr_count"] <= 128, (name, k)
        assert k["group_segment_fixed_size"] == 16 * (_lib.MAX_SENSORS ** 2 + 1), (name, k)
        assert not any(op.startswith("scratch_") for op in ins_of[name]), name
