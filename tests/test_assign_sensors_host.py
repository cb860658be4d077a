"""CPU-only checks of a sensor network's device-side assignment (include/ssa_hip.h: ssa_assign_sensors_f64;
SSA_Tasker_Env.run_agent_sensors): the exports, refusal of bad arguments before any launch, the env's guards without device state, and
the new kernel's resource budget in the shipped code object."""
import re

import pytest

from support.codeobj import _kernels, header
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.sensors import _bare_env


def test_assignment_is_exported_and_declared(lib):
    from ssa_gym_amd import _lib
    hdr = header()
    assert re.search(r"\bint ssa_assign_sensors_f64\s*\(", hdr)
    assert re.search(r"\bint64_t ssa_assign_sensors_workspace_bytes\s*\(", hdr)
    for name in ("ssa_assign_sensors_f64", "ssa_assign_sensors_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define SSA_ABI_VERSION 23\b", hdr)
    assert lib.ssa_abi_version() == _lib.ABI_VERSION == 23          # (additive: the ABI version stays)


def test_workspace_size_covers_every_chunks_lists(lib):
    """64 bytes of ticket + per chunk of 512 objects S lists of S (value, index) pairs; out-of-range sizes are refused"""
    from ssa_gym_amd import _lib
    f = lib.ssa_assign_sensors_workspace_bytes
    for m, S in ((1, 1), (5, 3), (512, 8), (513, 8), (2003, 3), (20000, 8), (30001, 8)):
        assert f(m, S) == 64 + ((m + 511) // 512) * S * S * 16, (m, S)
    for m, S in ((0, 3), (-1, 3), (2 ** 31, 3), (10, 0), (10, -1), (10, 9)):
        assert f(m, S) == _lib.E_INVALID, (m, S)


def test_assignment_refuses_bad_arguments_before_any_launch(lib):
    """every refusal, each from otherwise valid arguments (the pointers are never dereferenced on the host and no device is touched:
    this runs without a GPU)"""
    from ssa_gym_amd import _lib
    f = lib.ssa_assign_sensors_f64
    m, S = 2003, 3
    need = lib.ssa_assign_sensors_workspace_bytes(m, S)
    valid = dict(score=0x10000, n_obj=m, n_sensor=S, column=_lib.LOOK_INFO_GAIN, fallback=0x20000, action_out=0x30000, pick_out=0x40000,
                 workspace=0x50000, workspace_bytes=need, stream=None)
    spoiled = [("score", 0), ("action_out", 0), ("action_out", 0x30004), ("action_out", 0x30010), ("n_sensor", 0), ("n_sensor", -1),
               ("n_sensor", _lib.MAX_SENSORS + 1), ("column", -1), ("column", _lib.LOOK_NSCORE), ("n_obj", 0), ("n_obj", -5),
               ("workspace", 0), ("workspace_bytes", need - 1), ("workspace_bytes", 0), ("workspace", 0x50008)]
    for name, value in spoiled:
        args = dict(valid)
        args[name] = value
        assert f(*args.values()) == _lib.E_INVALID, (name, value)
    # (the workspace must cover the sizes of THIS call: one sized for fewer sensors or objects is too small)
    assert f(*dict(valid, workspace_bytes=lib.ssa_assign_sensors_workspace_bytes(m, S - 1)).values()) == _lib.E_INVALID
    assert f(*dict(valid, workspace_bytes=lib.ssa_assign_sensors_workspace_bytes(m - 512, S)).values()) == _lib.E_INVALID


def test_env_guards_come_before_anything_is_launched():
    from ssa_gym_amd import _lib, agents
    for S in (3, 1):
        env = _bare_env(S)
        with pytest.raises(_lib.SsaHipError, match="no CPU fallback"):
            env.run_agent_sensors(agents.agent_info_gain_sensors, 3)          # no device state: no CPU fallback
        env._engine = object()                                                # (the checks below come before anything touches the engine)
        for agent in (agents.agent_info_gain, "agent_visible_greedy", agents.agent_naive_random, None):
            with pytest.raises(NotImplementedError, match="agent_info_gain_sensors.*agent_trace_gain_sensors"):
                env.run_agent_sensors(agent, 3)
    env = _bare_env(3)
    env._engine = object()
    with pytest.raises(NotImplementedError, match="run_agent: not implemented for a sensor network"):   # run_agent keeps refusing a network
        env.run_agent(agents.agent_visible_greedy, 3)
    with pytest.raises(NotImplementedError, match="rollout: not implemented for a sensor network"):
        env.rollout([0, 1])
    with pytest.raises(NotImplementedError, match="sensor network"):
        env.run_policy(None, 3)


def test_assign_kernel_budget(tmp_path):
    """assign_sensors_kernel from the notes of the shipped code object: one instance; no scratch and no spills (the kernel is a chain of
    short dependent rounds: a spill would put memory round trips into every one of them); the S x S candidate table and the last-arrival
    flag in LDS and nothing else.  Registers: the launch is ceil(m / 512) workgroups of four wavefronts -- 40 at 20 000 objects, on 256
    CUs -- so occupancy never limits it; the bound is the 128 VGPRs at which a SIMD still holds four wavefronts, i.e. a CU four whole
    workgroups, more than the grid puts on one CU below half a million objects.  (Forcing 64 VGPRs -- eight wavefronts per SIMD, which
    nothing here needs -- made the compiler spill.)"""
    kern, ins_of = _kernels(tmp_path)
    names = [k for k in kern if "assign_sensors_kernel" in k]
    assert len(names) == 1, names
    k = kern[names[0]]
    print("[assign_sensors_kernel]", k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
    assert k["vgpr_count"] <= 128 and k["sgpr_count"] <= 104, k
    assert k["group_segment_fixed_size"] <= 8 * 8 * 16 + 16, k
    ins = ins_of[names[0]]
    assert not [op for op in ins if op.startswith("scratch_")]
    assert "s_swappc_b64" not in ins                                           # (no out-of-line call)
