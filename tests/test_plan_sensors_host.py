"""CPU-only checks of a sensor network's horizon-wide optimal plan (include/ssa_hip.h: ssa_plan_sensors_f64,
ssa_plan_sensors_workspace_bytes): the exports, every refusal from otherwise complete arguments, the size query,
the cap on H' S in the Python layers, the guards of the planners without device state, the host's fill of the idle slots, and the
kernel's budget in the shipped code object."""
import re

import numpy as np
import pytest

from support.codeobj import _kernels, family, header
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.sensors import _bare_env
from support.vector_forecast import bare_vec

PLANNERS = ("plan_info_gain_sensors_horizon", "plan_trace_gain_sensors_horizon")


def test_the_two_entries_are_exported_declared_and_bound(lib):
    import ctypes as C
    from ssa_gym_amd import _lib
    hdr = header()
    assert re.search(r"\bint ssa_plan_sensors_f64\s*\(", hdr) and re.search(r"\bint64_t ssa_plan_sensors_workspace_bytes\s*\(", hdr)
    for name in ("ssa_plan_sensors_f64", "ssa_plan_sensors_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    res, args = _lib.SIGNATURES["ssa_plan_sensors_f64"]
    assert res is C.c_int and args == [_lib.c_dp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _lib.c_dp, _lib.c_dp, _lib.c_dp,
                                       C.c_int64, _lib.c_dp]
    assert _lib.SIGNATURES["ssa_plan_sensors_workspace_bytes"] == (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32])
    assert re.search(r"#define SSA_MAX_PLAN_SLOTS 64\b", hdr) and _lib.MAX_PLAN_SLOTS == 64
    assert re.search(r"#define SSA_ABI_VERSION 23\b", hdr)
    assert lib.ssa_abi_version() == _lib.ABI_VERSION == 23          # (additive: the ABI version stays)
    # the header states the rule's promises
    for text in ("2^1020", "pure function of the input bits", "4 N 2^-53 max|candidate score|", "no large constant", "no fallback argument"):
        assert text in hdr, text


def _valid(lib, L, **over):
    m, S, H, E = 2003, 3, 8, 2
    v = dict(score=0x10000, n_obj=m, n_sensor=S, n_step=H, n_env=E, column=L.LOOK_INFO_GAIN, plan_out=0x20000, pick_out=0x40000,
             workspace=0x80000, workspace_bytes=None, stream=None)
    v.update(over)
    if v["workspace_bytes"] is None:
        v["workspace_bytes"] = max(lib.ssa_plan_sensors_workspace_bytes(v["n_obj"], v["n_sensor"], v["n_step"], v["n_env"]), 0)
    return v


def test_every_refusal_before_any_launch(lib):
    """each refusal from otherwise complete, valid arguments (the pointers are never dereferenced on the host: a refusal comes before
    any launch, so this runs without a GPU), in the header's order, then two rules broken at once"""
    from ssa_gym_amd import _lib
    q = lib.ssa_plan_sensors_workspace_bytes
    need = q(2003, 3, 8, 2)
    assert need == 2 * (64 + 4 * 24 * 24 * 16) and need % 64 == 0
    cases = [dict(score=None), dict(plan_out=None),
             dict(plan_out=0x20004), dict(plan_out=0x20010),
             dict(n_sensor=0), dict(n_sensor=-1), dict(n_sensor=_lib.MAX_SENSORS + 1),
             dict(n_step=0), dict(n_step=-3),
             dict(n_step=22), dict(n_step=65, n_sensor=1), dict(n_step=9, n_sensor=8),                      # 66, 65 and 72 slots
             dict(n_env=0), dict(n_env=-2), dict(n_env=65536),
             dict(column=-1), dict(column=_lib.LOOK_NSCORE),
             dict(n_obj=0), dict(n_obj=-5),
             dict(n_obj=1 << 31, n_step=1, n_sensor=1, n_env=1), dict(n_obj=1 << 26, n_step=8, n_sensor=2, n_env=2),   # 2^31 score rows
             dict(n_obj=1 << 62),
             dict(workspace=None), dict(workspace=0x80008), dict(workspace=0x80020), dict(workspace_bytes=need - 1), dict(workspace_bytes=0),
             dict(workspace_bytes=q(2003, 3, 7, 2)), dict(workspace_bytes=q(2003 - 512, 3, 8, 2)), dict(workspace_bytes=q(2003, 3, 8, 1)),
             dict(score=None, n_env=0), dict(column=7, workspace=None), dict(plan_out=0x20004, n_step=65)]
    assert len(cases) >= 30
    ok = _valid(lib, _lib)
    assert ok["workspace_bytes"] == need
    for over in cases:
        args = list(_valid(lib, _lib, **over).values())
        assert lib.ssa_plan_sensors_f64(*args) == _lib.E_INVALID, over
    # the largest shapes the rule admits are not refused by the size query
    assert q(1, 1, 1, 1) == 64 + 16 and q(20000, 8, 8, 1) == 64 + 40 * 64 * 64 * 16 and q(511, 1, 64, 65535) > 0


def test_the_size_query_refuses_the_same_ranges(lib):
    from ssa_gym_amd import _lib
    q = lib.ssa_plan_sensors_workspace_bytes
    for args in ((0, 3, 8, 2), (-1, 3, 8, 2), (2003, 0, 8, 2), (2003, 9, 8, 2), (2003, 3, 0, 2), (2003, 3, -1, 2), (2003, 3, 22, 2),
                 (2003, 1, 65, 1), (2003, 3, 8, 0), (2003, 3, 8, 65536), (1 << 31, 1, 1, 1), (1 << 26, 2, 8, 2), (1 << 62, 8, 8, 65535)):
        assert q(*args) == _lib.E_INVALID, args
    assert q((1 << 31) - 1, 1, 1, 1) > 0 and q((1 << 26) - 1, 2, 8, 2) > 0


def test_more_than_64_slots_is_a_value_error_that_names_the_cap():
    """H' S = 65 (13 steps x 5 sensors, 65 x 1): a ValueError before the library, a tensor or an engine is looked at"""
    from ssa_gym_amd import agents, device, engine
    cap = r"64.*SSA_MAX_PLAN_SLOTS"
    with pytest.raises(ValueError, match=cap):
        device.check_plan_slots(13, 5)
    with pytest.raises(ValueError, match=cap):
        device.plan_sensors_workspace(100, 1, 65, 1, "cpu")
    device.check_plan_slots(8, 8)
    device.check_plan_slots(64, 1)
    for name in PLANNERS:
        with pytest.raises(ValueError, match=cap):
            getattr(agents, name)(_bare_env(5, n=20), 13)             # (13 of the 19 steps left)
        with pytest.raises(ValueError, match=cap):
            getattr(agents, name)(bare_vec(1, n=70), 65)
        with pytest.raises(_lib_error(), match="no CPU fallback"):
            getattr(agents, name)(_bare_env(5, n=13), 13)             # (12 steps left: 60 slots pass the cap, then no device state)
    eng = engine.HotPathEngine.__new__(engine.HotPathEngine)
    eng.m, eng.E = 10, 1
    with pytest.raises(_lib_error(), match="forecast"):
        eng.launch_plan_sensors({"score": None}, 0)                   # (anything but a forecast's CUDA scores is refused)
    with pytest.raises(_lib_error(), match="score must be"):
        device.plan_sensors(np.zeros((2, 1, 4, 3)), 0)


def _lib_error():
    from ssa_gym_amd import _lib
    return _lib.SsaHipError


def test_planners_need_device_state():
    from ssa_gym_amd import _lib, agents
    for S in (3, 1):
        env = _bare_env(S)
        for name in PLANNERS:
            with pytest.raises(_lib.SsaHipError, match="no device state.*no CPU fallback"):
                getattr(agents, name)(env, 4)
        assert env.i == 0
    vec = bare_vec(3)
    for name in PLANNERS:
        with pytest.raises(_lib.SsaHipError, match="no device state.*no CPU fallback"):
            getattr(agents, name)(vec, 4)
        with pytest.raises(ValueError, match="horizon"):
            getattr(agents, name)(vec, 0)
    assert np.all(vec.i == 0) and vec.tick == 0


def test_the_host_fill_never_tasks_an_object_planned_later():
    """a hand-made plan: slot (0, 1) is idle while object 4 is planned at step 1 -- the fill never draws 4 (or any object of the plan),
    whatever the generator gives; _fill_plan's row rule would allow it.  np_random is untouched; planned entries stay."""
    from ssa_gym_amd import agents
    plan = np.array([[2, -1, 7], [4, 5, -1], [-1, -1, 9]])
    for seed in range(40):
        env = _bare_env(3, m=10, seed=seed)
        env.action_space.seed(seed)
        draws = env.np_random.get_state()[2]
        got = agents._fill_plan_horizon(env, plan)
        assert got.dtype == np.int64 and got.shape == plan.shape and np.array_equal(got[plan >= 0], plan[plan >= 0])
        flat = got.reshape(-1).tolist()
        assert len(set(flat)) == len(flat) and min(flat) >= 0 and max(flat) < 10, got      # nothing twice in the WHOLE plan
        assert set(got[plan < 0].tolist()) <= {0, 1, 3, 6, 8}, got
        assert not set(got[plan < 0].tolist()) & {2, 7, 4, 5, 9}
        assert env.np_random.get_state()[2] == draws
        assert (plan == np.array([[2, -1, 7], [4, 5, -1], [-1, -1, 9]])).all()              # (the argument is not written)
    # the row rule does allow it: the old fill is a different rule (and stays as it is)
    hit = False
    for seed in range(40):
        env = _bare_env(3, m=10, seed=seed)
        env.action_space.seed(seed)
        hit |= int(agents._fill_plan(env, plan)[0, 1]) in (4, 5, 9)
    assert hit


def test_the_host_fill_falls_back_to_the_row_rule_when_every_object_is_planned():
    """4 objects, 6 slots: once every object appears in the plan, an idle slot gets an object no sensor of its ROW holds"""
    from ssa_gym_amd import agents
    plan = np.array([[0, 1], [2, -1], [-1, -1]])
    for seed in range(20):
        env = _bare_env(2, m=4, seed=seed)
        env.action_space.seed(seed)
        got = agents._fill_plan_horizon(env, plan)
        assert np.array_equal(got[plan >= 0], plan[plan >= 0]) and got[1, 1] == 3          # (the one object the plan does not hold)
        assert ((got >= 0) & (got < 4)).all() and all(len(set(r.tolist())) == 2 for r in got), got
    vec = bare_vec(2, E=2, m=4)
    both = np.stack([agents._fill_plan_horizon(vec, p) for p in np.stack([plan, plan[::-1]])])
    assert both.shape == (2, 3, 2) and ((both >= 0) & (both < 4)).all() and all(len(set(r.tolist())) == 2 for p in both for r in p)


def test_plan_kernel_budget(tmp_path):
    """plan_sensors_kernel from the notes of the shipped code object: one instance; no scratch, no vector spills, no out-of-line call.
    Registers: workgroups of 1 024 threads put four wavefronts on every SIMD, which allows 128 VGPRs.  LDS: exactly the objects the
    layout declares (one workgroup per CU, by the 160 KB of a gfx950 CU) --
        q, 64 slots x 64 entries of int64                          64 x 64 x 8 = 32 768
        the entries' objects                                       64 x 64 x 4 = 16 384
        the entries' column numbers                                64 x 64 x 2 =  8 192
        the hash table (8 192 keys, 8 192 numbers), then the
        columns' duals (4 096 int64, 4 096 int32)          8 192 x 4 + 8 192 x 2 = 49 152
        the slot a column is matched to                                  4 096 =  4 096
        one scan's relaxations: distance (8 + 4), entry, stamp    64 x 20 =  1 280
        the result                                                     64 x 4 =    256
        the scan's wavefront totals                                    16 x 4 =     64
        the largest magnitude, the last-arrival flag, padding        8 + 4 + 4 =     16"""
    kern, ins_of = _kernels(tmp_path)
    lds = 64 * 64 * 8 + 64 * 64 * 4 + 64 * 64 * 2 + (8192 * 4 + 8192 * 2) + 4096 + 64 * 20 + 64 * 4 + 16 * 4 + 16
    assert lds == 112208 and lds <= 160 * 1024
    names = family(kern, "plan_sensors_kernel")
    assert len(names) == 1 and [k for k in kern if "plan_sensors_kernel" in k] == names, names
    k, ins = kern[names[0]], ins_of[names[0]]
    print("[plan_sensors_kernel]", k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
    assert k["vgpr_count"] <= 128, k
    assert k["group_segment_fixed_size"] == lds, k
    assert not [op for op in ins if op.startswith("scratch_")]
    assert "s_swappc_b64" not in ins
    assert k["arg_kinds"][:9] == ["global_buffer", "by_value", "by_value", "by_value", "by_value", "global_buffer", "global_buffer",
                                  "global_buffer", "by_value"], k["arg_kinds"]
    # the assignment kernels are what they were
    for name, size in (("assign_sensors_kernel", 1040), ("match_sensors_kernel", 26016)):
        assert len(family(kern, name)) == 1 and kern[family(kern, name)[0]]["group_segment_fixed_size"] == size
