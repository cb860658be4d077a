"""CPU-only table of HotPathEngine's refusals (ssa-gym_amd/engine.py): every one that can be reached before anything is launched and
without device state, on an engine made with `__new__` that has E, m and the few attributes the rule reads -- the method, the
arguments, the exception class and the words the other tests already match.  What needs a device to be reached has no row: the
constructor's own refusals, whatever comes after a schedule or a score has been accepted as a CUDA tensor (the z_noise extent in
launch_rollout_sensors, `% 4`, z_noise and argmax_spos in launch_rollout_sensors_envs, MAX_PLAN_SLOTS and `picks` in
launch_plan_sensors, the later arguments of launch_closed_loop) and the return codes of the library."""
import types

import numpy as np
import pytest

S = 2
N_TIME = 2


def _sites(m):
    return types.SimpleNamespace(n_sensor=S, zn_stride_sensor=N_TIME * m * 3)


def _noise(m, n):
    """what _check_sensor_noise reads, with a noise table of n values"""
    import torch
    from ssa_gym_amd import _lib
    p = _lib.ssa_step_params()
    p.zn_stride_obj = 3
    return dict(z_noise=torch.zeros(n), n_time=N_TIME, zn_stride_time=m * 3, zn_stride_env=S * N_TIME * m * 3, _p=p)


def _look_state():
    """what a lookahead reads before it looks at env_times: its buffers (on the CPU here) and the input block of a history slot"""
    import torch
    from ssa_gym_amd import _lib
    st = dict(dev=torch.device("cpu"), H=2, _p=_lib.ssa_step_params(), _look=None, _look_s=None, _look_se=None, _fore=None, _fore_e=None)
    st.update({k: 0 for k in ("_bx_t", "_bx", "_bP", "_sx", "_sP")})
    return st


def _step_state():
    """what launch_step reads on the way to its refusals (no statistics by atomics: no shard set is touched)"""
    st = _look_state()
    st.update({k: 0 for k in ("_bo", "_bm", "_bs", "_bu", "_so", "_sm", "_ss", "_su", "_shard_cur", "_actions_ptr")})
    # (_bm: the metrics base is read back as an integer, so no null pointer)
    st.update(_bm=64, _fold_pending=None, stats_from_metrics=False, supports_argmax=False, force_generic=False, _pcache={})
    return st


def _cpu(shape, dtype="int32"):
    import torch
    return torch.zeros(shape, dtype=getattr(torch, dtype))


def _err():
    from ssa_gym_amd import _lib
    return _lib.SsaHipError


def _cases():
    """(id, method, E, m, attributes, args, kwargs, exception, words)"""
    HIP = _err()
    i64 = np.int64
    rows = []

    def row(ident, method, E, m, attrs, args, kw, exc, words):
        rows.append(pytest.param(method, E, m, attrs, args, kw, exc, words, id=ident))

    # ---- a one-env launch on several envs: before anything else is read
    for m in (6, 8):
        row("step_sensors-one_env-m%d" % m, "launch_step_sensors", 3, m, {}, (0, 1, 0, _sites(m), [0, 1], 0), {}, HIP, "one env")
        row("lookahead_sensors-one_env-m%d" % m, "launch_lookahead_sensors", 3, m, {}, (0, 1, None), {}, HIP, "one env")
        row("forecast_sensors-one_env-m%d" % m, "launch_forecast_sensors", 3, m, {}, (0, 1, None, 3), {}, HIP, "one env")
        row("dryrun_sensors-one_env-m%d" % m, "launch_dryrun_sensors", 3, m, {}, (0, 1, None, np.zeros((1, 2, S), dtype=i64)), {}, HIP, "one env")
        row("rollout_sensors-one_env-m%d" % m, "launch_rollout_sensors", 3, m, {}, (0, 1, None, None), {}, HIP, "one env")
    # ---- several envs need whole tiles
    row("step_sensors_envs-tiles", "launch_step_sensors_envs", 3, 6, {}, (0, 1, 0, _sites(6), np.zeros((3, S), dtype=i64)), {}, HIP, "% 4")
    row("set_layout-tiles", "set_layout", 3, 6, dict(_order=None), (np.tile(np.arange(6), (3, 1)),), {}, HIP, "% 4")
    # ---- schedules and action rows
    for E, m in ((1, 6), (3, 8)):
        for bad in (None, _cpu((2, E)), np.zeros((2, E), dtype=np.int32)):
            row("rollout-actions-E%d-%s" % (E, type(bad).__name__), "launch_rollout", E, m, {}, (0, 1, bad), {}, HIP, "actions")
        for bad in (None, _cpu((2, E, S)), np.zeros((4, E, S), dtype=np.int32)):
            row("rollout_sensors_envs-actions-E%d-%s" % (E, type(bad).__name__), "launch_rollout_sensors_envs", E, m, {},
                (0, 1, _sites(m), bad), {}, HIP, "actions")
    for bad in (None, _cpu((2, S)), _cpu((2, 8))):
        row("rollout_sensors-actions-%s" % (bad if bad is None else tuple(bad.shape),), "launch_rollout_sensors", 1, 6, {},
            (0, 1, _sites(6), bad), {}, HIP, "actions")
    row("step_sensors-count", "launch_step_sensors", 1, 6, {}, (0, 1, 0, _sites(6), [0], 0), {}, HIP, "1 actions for 2 sensors")
    row("step_sensors_envs-shape", "launch_step_sensors_envs", 3, 8, {}, (0, 1, 0, _sites(8), np.zeros((2, S), dtype=i64)), {}, HIP, "actions must be")
    row("step_sensors_envs-no_rows_no_words", "launch_step_sensors_envs", 3, 8, {}, (0, 1, 0, _sites(8)), dict(env_words=[1, 2, 3]), HIP, "env_words")
    # ---- the noise tables a network indexes
    row("step_sensors-z_noise", "launch_step_sensors", 1, 6, _noise(6, 4), (0, 1, 0, _sites(6), [0, 1], 0), {}, HIP, "z_noise")
    row("step_sensors_envs-z_noise", "launch_step_sensors_envs", 3, 8, _noise(8, 4), (0, 1, 0, _sites(8), np.zeros((3, S), dtype=i64)), {}, HIP, "z_noise")
    # ---- the dry runs' own
    row("dryrun_sensors-one_candidate", "launch_dryrun_sensors", 1, 6, {}, (0, 1, _sites(6), np.zeros((2, 2, S), dtype=i64)), dict(gather=False),
        HIP, "one candidate")
    for E, m in ((1, 6), (3, 8)):
        row("dryrun_sensors_envs-ndim-E%d" % E, "launch_dryrun_sensors_envs", E, m, {}, (0, 1, _sites(m), np.zeros((E, 2, S), dtype=i64)), {},
            ValueError, "actions must be")
        row("dryrun_sensors_envs-envs-E%d" % E, "launch_dryrun_sensors_envs", E, m, {}, (0, 1, _sites(m), np.zeros((E + 1, 1, 2, S), dtype=i64)), {},
            ValueError, "actions must be")
        row("dryrun_sensors_envs-env_times-E%d" % E, "launch_dryrun_sensors_envs", E, m, {}, (0, 1, _sites(m), np.zeros((E, 1, 2, S), dtype=i64)),
            dict(env_times=[0] * (E + 1)), ValueError, "env_times")
    # ---- the forecast's horizon: before buffers are touched
    for bad in (0, -1):
        row("forecast_sensors-n_steps%d" % bad, "launch_forecast_sensors", 1, 6, {}, (0, 1, _sites(6), bad), {}, HIP, "n_steps")
        row("forecast_sensors_envs-n_steps%d" % bad, "launch_forecast_sensors_envs", 3, 8, {}, (0, 1, _sites(8), bad), {}, HIP, "n_steps")
    # ---- unknown outputs of the lookahead family
    for E, m in ((1, 6), (3, 8)):
        row("lookahead-out-E%d" % E, "launch_lookahead", E, m, {}, (0, 1), dict(out=("P_post", "bogus")), ValueError, "unknown output")
        row("lookahead_sensors_envs-out-E%d" % E, "launch_lookahead_sensors_envs", E, m, {}, (0, 1, _sites(m)), dict(out=("bogus",)), ValueError,
            "unknown output")
        row("forecast_sensors_envs-out-E%d" % E, "launch_forecast_sensors_envs", E, m, {}, (0, 1, _sites(m), 2), dict(out=("bogus",)), ValueError,
            "unknown output")
    row("lookahead_sensors-out", "launch_lookahead_sensors", 1, 6, {}, (0, 1, _sites(6)), dict(out=("bogus",)), ValueError, "unknown output")
    row("forecast_sensors-out", "launch_forecast_sensors", 1, 6, {}, (0, 1, _sites(6), 2), dict(out=("bogus",)), ValueError, "unknown output")
    # ---- time words by value: at most INLINE_ENVS envs
    words = list(range(9))
    row("lookahead-env_times", "launch_lookahead", 9, 8, _look_state(), (0, 1), dict(stream=0, env_times=words), HIP, "at most 8 envs")
    row("lookahead_sensors_envs-env_times", "launch_lookahead_sensors_envs", 9, 8, _look_state(), (0, 1, _sites(8)), dict(stream=0, env_times=words),
        HIP, "at most 8 envs")
    row("forecast_sensors_envs-env_times", "launch_forecast_sensors_envs", 9, 8, _look_state(), (0, 1, _sites(8), 2), dict(stream=0, env_times=words),
        HIP, "at most 8 envs")
    from ssa_gym_amd import _lib
    row("step_sensors_envs-env_words", "launch_step_sensors_envs", 9, 8, dict(_noise(8, 10 ** 4), _sensor_envs=(_lib.ssa_sensor_envs_params(), None, None)),
        (0, 1, 0, _sites(8), np.zeros((9, S), dtype=i64)), dict(env_words=words), HIP, "at most 8 envs")
    row("step-env_words", "launch_step", 9, 8, _step_state(), (0, 1, 0), dict(stream=0, env_words=(words, words)), HIP, "at most 8 envs")
    # ---- launch_step's own
    row("step-argmax", "launch_step", 3, 6, _step_state(), (0, 1, 0), dict(stream=0, fast_stats=True, argmax_spos=True), HIP, "whole tiles")
    row("step-profile_slot", "launch_step", 1, 6, _step_state(), (0, 1, 0), dict(stream=0, sensors=_sites(6), profile_slot=0), HIP, "profile_slot")
    # ---- assignment and plan: the rule, the tensors, the scores
    for E, m in ((1, 6), (3, 8)):
        row("assign-rule-E%d" % E, "launch_assign_sensors", E, m, {}, ({}, 0, None), dict(rule="bogus"), ValueError, "rule must be 'greedy' or 'optimal'")
        row("assign_envs-rule-E%d" % E, "launch_assign_sensors_envs", E, m, {}, ({}, 0), dict(rule="bogus"), ValueError,
            "rule must be 'greedy' or 'optimal'")
        row("assign_envs-fallback-E%d" % E, "launch_assign_sensors_envs", E, m, {}, ({"score": None}, 0), dict(fallback=_cpu((E, 8))), HIP, "contiguous CUDA")
        row("assign_envs-picks-E%d" % E, "launch_assign_sensors_envs", E, m, {}, ({"score": None}, 0), dict(picks=_cpu((E, 8, 2), "int64")), HIP,
            "contiguous CUDA")
        for bad in (None, _cpu((E, S, m, 3), "float64"), np.zeros((E, S, m, 3))):
            row("assign_envs-score-E%d-%s" % (E, type(bad).__name__), "launch_assign_sensors_envs", E, m, {}, ({"score": bad}, 0), {}, HIP,
                "contiguous CUDA float64")
        for bad in (None, _cpu((2, S, m, 3), "float64"), _cpu((2, E, S, m, 3), "float64")):
            row("plan-score-E%d-%s" % (E, bad if bad is None else bad.dim()), "launch_plan_sensors", E, m, {}, ({"score": bad}, 0), {}, HIP, "forecast")
    row("assign-action_row", "launch_assign_sensors", 1, 6, {}, ({"score": None}, 0, _cpu(8)), {}, HIP, "contiguous CUDA")
    row("assign-fallback_row", "launch_assign_sensors", 1, 6, {}, ({"score": None}, 0, None), dict(fallback_row=_cpu(8)), HIP, "contiguous CUDA")
    row("assign-picks", "launch_assign_sensors", 1, 8, {}, ({"score": None}, 0, None), dict(picks=_cpu((8, 2), "int64")), HIP, "contiguous CUDA")
    for bad in (None, _cpu((S, 6, 3), "float64")):
        row("assign-score-%s" % type(bad).__name__, "launch_assign_sensors", 1, 6, {}, ({"score": bad}, 0, None), {}, HIP, "contiguous CUDA float64")
    # ---- the closed loop's arguments
    row("closed_loop-K", "launch_closed_loop", 1, 6, {}, (0, 1, 0, _cpu(1), None), {}, HIP, "K + 1 >= 2")
    row("closed_loop-actions", "launch_closed_loop", 1, 6, {}, (0, 1, 0, _cpu(3), None), {}, HIP, "contiguous CUDA")
    # ---- storage layouts
    row("set_layout-permutation", "set_layout", 1, 6, dict(_order=None), ([0, 1, 2, 3, 4, 4],), {}, HIP, "permutation")
    row("set_layout-rows", "set_layout", 3, 8, dict(_order=None), (np.arange(8),), {}, HIP, "permutation")
    row("set_env_layout-no_layout", "set_env_layout", 3, 8, dict(_order=None), (0, np.arange(8)), {}, HIP, "set_layout")
    row("set_env_layout-one_env", "set_env_layout", 1, 6, dict(_order=np.arange(6)), (0, np.arange(6)), {}, HIP, "set_layout")
    row("set_env_layout-permutation", "set_env_layout", 3, 8, dict(_order=np.tile(np.arange(8), (3, 1))), (0, np.zeros(8, dtype=i64)), {}, HIP, "permutation")
    return rows


def _bare(E, m, attrs):
    from ssa_gym_amd import engine
    eng = engine.HotPathEngine.__new__(engine.HotPathEngine)
    eng.E, eng.m = E, m
    for k, v in attrs.items():
        setattr(eng, k, v)
    return eng


@pytest.mark.parametrize("method,E,m,attrs,args,kw,exc,words", _cases())
def test_refusal(method, E, m, attrs, args, kw, exc, words):
    import re
    eng = _bare(E, m, attrs)
    with pytest.raises(exc, match=re.escape(words)) as info:
        getattr(eng, method)(*args, **kw)
    assert info.type is exc      # (the class itself: SsaHipError is no ValueError, and the other way round)


def test_closed_loop_declines_several_envs_before_anything_is_read():
    for m in (6, 8):
        assert _bare(3, m, {}).launch_closed_loop(0, 1, 0, None, None) is False


def test_a_refused_layout_leaves_the_one_in_force():
    order = np.tile(np.arange(8), (3, 1))
    eng = _bare(3, 8, dict(_order=order))
    with pytest.raises(_err(), match="permutation"):
        eng.set_layout(np.zeros((3, 8), dtype=np.int64))
    assert eng._order is order
