"""CPU-only checks of a sensor network's OPTIMAL assignment (include/ssa_hip.h: ssa_match_sensors_f64, ssa_match_sensors_envs_f64;
DESIGN.md section 8n): the exports, every refusal against the greedy sibling's code for the same spoiled arguments, the `rule`
argument of the Python layers, the guards of the new agents and planners without device state, and the two new kernels' budget in the
shipped code object."""
import re

import numpy as np
import pytest

from support.codeobj import KERNEL_FAMILIES, _kernels, family, header
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.sensors import _bare_env
from support.vector_forecast import bare_vec

NEW_AGENTS = ("agent_info_gain_sensors_optimal", "agent_trace_gain_sensors_optimal")


def test_the_two_entries_are_exported_declared_and_bound(lib):
    from ssa_gym_amd import _lib
    hdr = header()
    for name in ("ssa_match_sensors_f64", "ssa_match_sensors_envs_f64"):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # the argument lists are the greedy siblings'
    assert _lib.SIGNATURES["ssa_match_sensors_f64"] == _lib.SIGNATURES["ssa_assign_sensors_f64"]
    assert _lib.SIGNATURES["ssa_match_sensors_envs_f64"] == _lib.SIGNATURES["ssa_assign_sensors_envs_f64"]
    assert re.search(r"#define SSA_ABI_VERSION 23\b", hdr)
    assert lib.ssa_abi_version() == _lib.ABI_VERSION == 23          # (additive: the ABI version stays)
    # the header states what differs from the greedy rule
    assert "2^1020" in hdr and "pure function of the input bits" in hdr


def _one_env_cases(lib, L):
    m, S = 2003, 3
    need = lib.ssa_assign_sensors_workspace_bytes(m, S)
    valid = dict(score=0x10000, n_obj=m, n_sensor=S, column=L.LOOK_INFO_GAIN, fallback=0x20000, action_out=0x30000, pick_out=0x40000,
                 workspace=0x50000, workspace_bytes=need, stream=None)
    spoiled = [("score", 0), ("action_out", 0), ("action_out", 0x30004), ("action_out", 0x30010), ("n_sensor", 0), ("n_sensor", -1),
               ("n_sensor", L.MAX_SENSORS + 1), ("column", -1), ("column", L.LOOK_NSCORE), ("n_obj", 0), ("n_obj", -5), ("n_obj", 1 << 31),
               ("workspace", 0), ("workspace_bytes", need - 1), ("workspace_bytes", 0), ("workspace", 0x50008),
               ("workspace_bytes", lib.ssa_assign_sensors_workspace_bytes(m, S - 1)),
               ("workspace_bytes", lib.ssa_assign_sensors_workspace_bytes(m - 512, S))]
    return valid, [{k: v} for k, v in spoiled]


def _envs_cases(lib, L):
    m, S, E = 1100, 3, 2
    need = lib.ssa_assign_sensors_envs_workspace_bytes(m, S, E)
    valid = dict(score=0x10000, n_obj=m, n_sensor=S, n_env=E, column=L.LOOK_INFO_GAIN, fallback=None, action_out=0x20000, pick_out=None,
                 workspace=0x30000, workspace_bytes=need, stream=None)
    q = lib.ssa_assign_sensors_envs_workspace_bytes
    cases = [dict(score=None), dict(action_out=None), dict(action_out=0x20004), dict(action_out=0x20010), dict(column=-1), dict(column=3),
             dict(n_obj=0), dict(n_obj=-5), dict(n_obj=1 << 31), dict(n_sensor=0), dict(n_sensor=9), dict(n_env=0), dict(n_env=-2),
             dict(n_env=65536, workspace_bytes=q(m, S, 65536)), dict(workspace=None), dict(workspace=0x30008), dict(workspace=0x30020),
             dict(workspace_bytes=need - 1), dict(workspace_bytes=0),
             dict(n_obj=1 << 28, n_sensor=4, n_env=2, workspace_bytes=q(1 << 28, 4, 2)),               # 2^31 score rows
             dict(n_obj=1 << 28, n_sensor=8, n_env=1, workspace_bytes=q(1 << 28, 8, 1)),
             dict(score=None, n_env=0), dict(column=7, workspace=None), dict(action_out=0x20004, n_obj=1 << 28, n_sensor=8)]   # two rules at once
    return valid, cases


@pytest.mark.parametrize("envs", [False, True])
def test_every_refusal_equals_the_greedy_siblings(lib, envs):
    """each refusal from otherwise valid arguments, nothing launched (the pointers are never dereferenced on the host: this runs
    without a GPU): SSA_E_INVALID, and the code the greedy entry answers for the same arguments"""
    from ssa_gym_amd import _lib
    valid, cases = (_envs_cases if envs else _one_env_cases)(lib, _lib)
    new = getattr(lib, "ssa_match_sensors_envs_f64" if envs else "ssa_match_sensors_f64")
    old = getattr(lib, "ssa_assign_sensors_envs_f64" if envs else "ssa_assign_sensors_f64")
    assert len(cases) >= 18
    for over in cases:
        args = list(dict(valid, **over).values())
        got = new(*args)
        assert got == old(*args) == _lib.E_INVALID, (over, got)


def test_an_unknown_rule_names_both_rules():
    """rule='bogus' is a ValueError that names 'greedy' and 'optimal', raised before the library, a tensor or an engine is looked at"""
    from ssa_gym_amd import agents, device, engine
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    both = r"(?s)(?=.*greedy)(?=.*optimal)"
    assert device.assign_entry("greedy") == "ssa_assign_sensors_f64" and device.assign_entry("greedy", envs=True) == "ssa_assign_sensors_envs_f64"
    assert device.assign_entry("optimal") == "ssa_match_sensors_f64" and device.assign_entry("optimal", envs=True) == "ssa_match_sensors_envs_f64"
    eng = engine.HotPathEngine.__new__(engine.HotPathEngine)
    vec = bare_vec(3)
    calls = [lambda: device.assign_entry("bogus"), lambda: device.assign_sensors(None, 0, rule="bogus"),
             lambda: device.assign_sensors_envs(None, 0, rule="bogus"), lambda: eng.launch_assign_sensors({}, 0, None, rule="bogus"),
             lambda: eng.launch_assign_sensors_envs({}, 0, rule="bogus"), lambda: SSA_Tasker_VecEnv.assign_sensors(vec, 0, rule="bogus"),
             lambda: agents.plan_info_gain_sensors(_bare_env(3), 4, rule="bogus"), lambda: agents.plan_trace_gain_sensors(vec, 4, rule=None)]
    for call in calls:
        with pytest.raises(ValueError, match=both):
            call()


def test_new_agents_and_planners_need_device_state():
    from ssa_gym_amd import _lib, agents
    for S in (3, 1):
        env = _bare_env(S)
        for name in NEW_AGENTS:
            with pytest.raises(_lib.SsaHipError, match="no CPU fallback"):
                getattr(agents, name)(None, env)
            with pytest.raises(_lib.SsaHipError, match="no CPU fallback"):
                env.run_agent_sensors(name, 3)
        for plan in (agents.plan_info_gain_sensors, agents.plan_trace_gain_sensors):
            with pytest.raises(_lib.SsaHipError, match="no CPU fallback"):
                plan(env, 4, rule="optimal")
    vec = bare_vec(3)
    for name in NEW_AGENTS:
        with pytest.raises(_lib.SsaHipError, match="no CPU fallback"):
            getattr(agents, name)(None, vec)
    for plan in (agents.plan_info_gain_sensors, agents.plan_trace_gain_sensors):
        with pytest.raises(_lib.SsaHipError, match="no CPU fallback"):
            plan(vec, 4, rule="optimal")
    assert np.all(vec.i == 0) and vec.tick == 0 and env.i == 0


def test_new_agent_names_resolve_before_the_engine_is_touched():
    """the function or its name, for a single env and a vector env; the tables the existing tests index keep their keys and values, and
    the refusals keep their texts, with the new agents named after them"""
    from ssa_gym_amd import _lib, agents
    from ssa_gym_amd.envs import vector_env as V
    from ssa_gym_amd.envs.ssa_tasker_simple_2 import SSA_Tasker_Env
    old = {'agent_info_gain_sensors': _lib.LOOK_INFO_GAIN, 'agent_trace_gain_sensors': _lib.LOOK_TRACE_GAIN}
    assert SSA_Tasker_Env.SENSOR_AGENT_COLUMNS == old and V.SENSOR_AGENTS is SSA_Tasker_Env.SENSOR_AGENT_COLUMNS      # (one table, two names)
    want = {'agent_info_gain_sensors': (_lib.LOOK_INFO_GAIN, 'greedy'), 'agent_trace_gain_sensors': (_lib.LOOK_TRACE_GAIN, 'greedy'),
            'agent_info_gain_sensors_optimal': (_lib.LOOK_INFO_GAIN, 'optimal'),
            'agent_trace_gain_sensors_optimal': (_lib.LOOK_TRACE_GAIN, 'optimal')}
    assert SSA_Tasker_Env.SENSOR_AGENT_RULES == want and V.SENSOR_AGENT_RULES is SSA_Tasker_Env.SENSOR_AGENT_RULES
    for name, (col, rule) in want.items():
        fn = getattr(agents, name)
        assert V.sensor_agent_rule(fn) == V.sensor_agent_rule(name) == (col, rule)
        assert V.sensor_agent_column(fn) == V.sensor_agent_column(name) == col and isinstance(V.sensor_agent_column(name), int)
    # a vector env: the name resolves, the next guard (a network is needed) answers -- nothing touched the engine (there is none)
    for name in NEW_AGENTS:
        with pytest.raises(NotImplementedError, match="observers"):
            bare_vec(1).step_agent(name)
        with pytest.raises(NotImplementedError, match="observers"):
            bare_vec(1).step_agent(getattr(agents, name))
    with pytest.raises(NotImplementedError, match="agent_info_gain_sensors and agent_trace_gain_sensors.*"
                                                  "agent_info_gain_sensors_optimal and agent_trace_gain_sensors_optimal"):
        bare_vec(3).step_agent("agent_visible_greedy")
    # a single env: with an engine that is no engine, a new name passes the agent check and fails only where the engine is first used
    env = _bare_env(3)
    env._engine = object()
    for bad in (agents.agent_info_gain, "agent_visible_greedy", None):
        with pytest.raises(NotImplementedError, match="agent_info_gain_sensors.*agent_trace_gain_sensors.*"
                                                      "agent_info_gain_sensors_optimal.*agent_trace_gain_sensors_optimal"):
            env.run_agent_sensors(bad, 3)
    for name in NEW_AGENTS:
        for agent in (name, getattr(agents, name)):
            with pytest.raises(Exception) as err:
                env.run_agent_sensors(agent, 3)
            assert not isinstance(err.value, NotImplementedError), agent


def test_match_kernel_budget(tmp_path):
    """match_sensors_kernel and match_sensors_envs_kernel from the notes of the shipped code object: one instance each, and the greedy
    kernels still one each; no scratch, no spills, no out-of-line call.  Registers: the grid and the block are assign_sensors_kernel's
    (ceil(m / 512) workgroups of four wavefronts, 40 at 20 000 objects on 256 CUs), so its reasoning holds: occupancy never limits the
    launch, and the bound is the 128 VGPRs at which a SIMD still holds four wavefronts.  LDS: exactly the objects the layout declares --
        the S x S table and the last-arrival flag   65 x 16 = 1 040
        dp, two buffers of 256 doubles               2 x 256 x 8 = 4 096
        w, 64 columns x 8 sensors                    64 x 8 x 8 = 4 096
        choice, a byte per column and mask           64 x 256 = 16 384
        the columns' objects, their count, padding   68 x 4 = 272
        the eight results                            8 x 16 = 128"""
    kern, ins_of = _kernels(tmp_path)
    lds = 65 * 16 + 2 * 256 * 8 + 64 * 8 * 8 + 64 * 256 + 68 * 4 + 8 * 16
    assert lds == 26016
    for name in ("match_sensors_kernel", "match_sensors_envs_kernel"):
        names = family(kern, name)
        assert len(names) == 1 and [k for k in kern if name in k] == names, (name, names)
        k, ins = kern[names[0]], ins_of[names[0]]
        print("[%s]" % name, k)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
        assert k["vgpr_count"] <= 128, k
        assert k["group_segment_fixed_size"] == lds, k
        assert not [op for op in ins if op.startswith("scratch_")]
        assert "s_swappc_b64" not in ins
    for new, old in (("match_sensors_kernel", "assign_sensors_kernel"), ("match_sensors_envs_kernel", "assign_sensors_envs_kernel")):
        a, b = kern[family(kern, new)[0]], kern[family(kern, old)[0]]                          # (the greedy sibling's arguments)
        assert a["arg_kinds"] == b["arg_kinds"] and a["by_value_offsets"] == b["by_value_offsets"], new
    # the greedy kernels did not become templates or gain instances
    for name in ("assign_sensors_kernel", "assign_sensors_envs_kernel"):
        assert len(family(kern, name)) == KERNEL_FAMILIES[name] == 1 and kern[family(kern, name)[0]]["group_segment_fixed_size"] == 1040
