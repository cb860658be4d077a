"""The lookahead of a sensor network on the MI355X (include/ssa_hip.h: ssa_lookahead_sensors_f64; SSA_Tasker_Env.lookahead_sensors,
agents.agent_info_gain_sensors / agent_trace_gain_sensors).

Two ground truths.  Sensor s's slice of the one launch must be bit-identical to the single-sensor lookahead (ssa_lookahead_f64) launched
with sensor s's kernel constants -- every output, every object, NaN bit patterns included.  And for sampled (s, j) it must equal what
the sensor step with sensor s on j and every other sensor idle leaves for j (P_filter, status, the record's visibility)."""
import ctypes as C

import numpy as np
import pytest

from support.gpu import envs  # noqa: F401  (the module fixture)
from support.sensors import _advance, _distinct, _Relaunch, cfg8, xyz_net

pytestmark = pytest.mark.gpu


def _np(r):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in r.items()}


def _i64(a):
    return np.ascontiguousarray(a).view(np.int64)


def _single(env, s):
    """ssa_lookahead_f64 with sensor s's kernel constants, every part"""
    from ssa_gym_amd import engine
    e = env._engine
    c0, r0 = e.consts, e._cref
    try:
        e.consts = env._sensor_consts[s]
        e._cref = C.byref(e.consts)
        return _np(e.launch_lookahead(env.i % e.H, env.i + 1, out=engine.HotPathEngine.LOOKAHEAD_PARTS))
    finally:
        e.consts, e._cref = c0, r0


def check_slices(env):
    """every sensor's slice of lookahead_sensors() against the single-sensor lookahead with its constants, bit for bit"""
    net = _np(env.lookahead_sensors(covariances=True))
    S, m = env.n_sensor, env.m
    assert net["score"].shape == (S, 3, m) and net["status"].shape == (S, m) and net["visible"].shape == (S, m)
    assert net["x_prior"].shape == (m, 6) and net["P_prior"].shape == (m, 6, 6) and net["P_post"].shape == (S, m, 6, 6)
    for s in range(S):
        one = _single(env, s)
        assert np.array_equal(_i64(net["score"][s]), _i64(one["score"].T)), s
        assert np.array_equal(net["status"][s], one["status"]), s
        assert np.array_equal(net["visible"][s], one["visible"]), s
        assert np.array_equal(_i64(net["P_post"][s]), _i64(one["P_post"])), s
        assert np.array_equal(_i64(net["x_prior"]), _i64(one["x_prior"])), s
        assert np.array_equal(_i64(net["P_prior"]), _i64(one["P_prior"])), s
    return net


def check_against_step(env, net, rs, n=24):
    """sampled (s, j): the sensor step with only sensor s on j leaves P_post[s, j], status[s, j] and visible[s, j]"""
    from ssa_gym_amd import _lib
    S, m = env.n_sensor, env.m
    st_in = env._engine.status.cpu().numpy()
    vis, st = net["visible"].astype(bool), net["status"]
    pairs = []
    # an object hidden from sensor 0 but visible to sensor 1; an already failed filter; one failing in this predict; a singular S
    cross = np.where(~vis[0] & vis[1] & (st[1] == 0))[0]
    assert len(cross), "no object hidden from sensor 0 and visible to sensor 1"
    pairs += [(0, int(j)) for j in rs.permutation(cross)[:2]] + [(1, int(j)) for j in rs.permutation(cross)[:2]]
    for grp in (np.where(st_in != 0)[0], np.where((st_in == 0) & ((st[0] == 1) | (st[0] == 2)))[0]):
        pairs += [(int(rs.randint(S)), int(j)) for j in rs.permutation(grp)[:3]]
    sing = np.argwhere(st == _lib.ST_UPDATE_LINALG)
    pairs += [(int(s), int(j)) for s, j in sing[:3]]
    pairs += [(int(rs.randint(S)), int(rs.randint(m))) for _ in range(max(0, n - len(pairs)))]
    rl = _Relaunch(env)
    seen = dict(visible=0, hidden=0, failed=0, failing=0, singular=len(sing) > 0)
    for s, j in pairs:
        acts = [-1] * S
        acts[s] = j
        got = rl.sensors(acts)
        st_j = int(got["st"][j])
        if st_j == _lib.ST_UPDATE_NAN:     # (depends on the drawn noise: not foreseen -- the lookahead says OK and visible)
            assert st[s, j] == _lib.ST_OK and vis[s, j], (s, j)
        else:
            assert st[s, j] == st_j, (s, j, st[s, j], st_j)
            assert np.array_equal(got["P"][j], _i64(net["P_post"][s, j]).reshape(36)), (s, j)
        assert vis[s, j] == (got["upd"][s][_lib.UPD_VISIBLE] == 1.0), (s, j)
        seen["visible"] += int(vis[s, j])
        seen["hidden"] += int(not vis[s, j] and st[s, j] == 0)
        seen["failed"] += int(st_in[j] != 0)
        seen["failing"] += int(st_in[j] == 0 and st[s, j] in (1, 2))
    print("[lookahead_sensors vs step] i=%d S=%d: %s" % (env.i, S, seen))
    return seen


@pytest.mark.parametrize("S", [3, 8])
def test_slices_and_step_at_20000_early_and_late(envs, S):
    """20 000 objects, 'hybrid': step 2, and a step past 300 with failed filters -- every slice against the single-sensor lookahead,
    sampled pairs against the sensor step"""
    env = envs.make('ssa_tasker_simple-v2', config=cfg8(envs, m=20000, sensors=S))
    rs = np.random.RandomState(S)
    _advance(env, rs, 2)
    net = check_slices(env)
    check_against_step(env, net, rs)
    _advance(env, rs, 305)
    assert env.i >= 300
    net = check_slices(env)
    seen = check_against_step(env, net, rs)
    assert seen["visible"] and seen["hidden"] and seen["failed"]


@pytest.mark.parametrize("variant", ["fg", "elements", "j2", "xyz"])
def test_slices_for_the_other_propagators_and_xyz(envs, variant):
    over = xyz_net() if variant == "xyz" else dict(propagator=variant)
    env = envs.make('ssa_tasker_simple-v2', config=cfg8(envs, **over))
    rs = np.random.RandomState(11)
    _advance(env, rs, 3)
    net = check_slices(env)
    check_against_step(env, net, rs, n=12)


def test_update_interval_on_an_update_step_and_a_skipped_step(envs):
    env = envs.make('ssa_tasker_simple-v2', config=cfg8(envs, update_interval=3))
    rs = np.random.RandomState(5)
    _advance(env, rs, 4)        # next step 5: skipped
    net = check_slices(env)
    assert not net["visible"].any() and np.isnan(net["score"]).all()
    assert all(np.array_equal(_i64(net["P_post"][s]), _i64(net["P_prior"])) for s in range(env.n_sensor))
    _advance(env, rs, 1)        # next step 6: an update step
    net = check_slices(env)
    assert net["visible"].any()
    check_against_step(env, net, rs, n=12)


def test_regime_layout_gives_the_same_bits(envs):
    a = envs.make('ssa_tasker_simple-v2', config=cfg8(envs))
    b = envs.make('ssa_tasker_simple-v2', config=cfg8(envs, storage_layout='regime'))
    assert b._engine._order is not None
    rs = np.random.RandomState(9)
    for k in range(40):
        acts = _distinct(rs, a.m, 3)
        a.step(acts)
        b.step(acts)
        if k in (1, 39):
            ra, rb = _np(a.lookahead_sensors(covariances=True)), _np(b.lookahead_sensors(covariances=True))
            for key in ra:
                assert np.array_equal(ra[key].view(np.uint8), rb[key].view(np.uint8)), (k, key)
    check_slices(b)


def test_multi_tile_instance_above_20480_objects(envs):
    env = envs.make('ssa_tasker_simple-v2', config=cfg8(envs, m=24000, sensors=2))
    rs = np.random.RandomState(13)
    _advance(env, rs, 2)
    net = check_slices(env)
    check_against_step(env, net, rs, n=12)


@pytest.mark.parametrize("m", [5, 7, 2003])
def test_slices_with_a_ragged_last_tile(envs, m):
    """object counts that are no multiple of a tile's four -- one whole tile and a partial one of one row, of three rows; a partial tile
    behind 500 whole ones -- at step 0 and after two steps: every slice against the single-sensor lookahead"""
    env = envs.make('ssa_tasker_simple-v2', config=cfg8(envs, m=m))
    check_slices(env)
    _advance(env, np.random.RandomState(m), 2)
    check_slices(env)


def test_one_sensor_equals_the_existing_lookahead(envs):
    """S = 1 -- an env without observers and a one-site network -- is env.lookahead() bit for bit"""
    base = cfg8(envs, sensors=0)
    one = dict(base, observers=[tuple(base['observer'])])
    for cfg in (base, one):
        env = envs.make('ssa_tasker_simple-v2', config=cfg)
        assert env.n_sensor == 1
        rs = np.random.RandomState(2)
        for k in range(3):
            _advance(env, rs, 1 + 60 * k)
            ref, net = _np(env.lookahead(covariances=True)), _np(env.lookahead_sensors(covariances=True))
            assert np.array_equal(_i64(net["score"][0]), _i64(ref["score"]))
            for key in ("status", "visible"):
                assert np.array_equal(net[key][0], ref[key]), key
            assert np.array_equal(_i64(net["P_post"][0]), _i64(ref["P_post"]))
            for key in ("x_prior", "P_prior"):
                assert np.array_equal(_i64(net[key]), _i64(ref[key])), key


def test_no_side_effects_on_an_episode(envs):
    """120 steps with lookahead_sensors() before every step and the same episode without: states, rewards and failures bit for bit"""
    import torch
    cfg = cfg8(envs, seed=21, steps=130)
    a, b = envs.make('ssa_tasker_simple-v2', config=cfg), envs.make('ssa_tasker_simple-v2', config=cfg)
    rs = np.random.RandomState(4)
    ra, rb = [], []
    for k in range(120):
        acts = _distinct(rs, a.m, 3)
        a.lookahead_sensors(covariances=bool(k % 2))
        oa = a.step(acts)
        ob = b.step(acts)
        ra.append(oa[1])
        rb.append(ob[1])
        assert np.array_equal(oa[0], ob[0])
    assert np.array_equal(np.asarray(ra), np.asarray(rb))
    ea, eb = a._engine, b._engine
    for x, y in ((ea.x_true, eb.x_true), (ea.x_filter, eb.x_filter), (ea.P_filter, eb.P_filter), (ea.obs, eb.obs)):
        assert torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64))
    assert torch.equal(ea.status, eb.status) and torch.equal(ea.fail_count, eb.fail_count)
    assert a.failed_filters_id == b.failed_filters_id
    assert np.array_equal(ea.fail_log, eb.fail_log)


def _greedy_np(score):
    """global greedy over [S, m]: the largest finite entry (ties: the lowest s * m + j), its row and column removed, repeated"""
    sc = np.array(score, dtype=np.float64)
    S, m = sc.shape
    act = np.full(S, -1)
    free_s, free_j = np.ones(S, bool), np.ones(m, bool)
    for _ in range(S):
        ok = ~np.isnan(sc) & free_s[:, None] & free_j[None, :]
        if not ok.any():
            break
        f = int(np.argmax(np.where(ok, sc, -np.inf).reshape(-1)))
        s, j = divmod(f, m)
        act[s] = j
        free_s[s], free_j[j] = False, False
    return act


def test_agents_assign_distinct_objects_greedily(envs):
    from ssa_gym_amd import _lib, agents
    env = envs.make('ssa_tasker_simple-v2', config=cfg8(envs, seed=5))
    env.action_space.seed(3)
    rs = np.random.RandomState(6)
    _advance(env, rs, 2)
    for k in range(20):
        for agent, col in ((agents.agent_info_gain_sensors, _lib.LOOK_INFO_GAIN), (agents.agent_trace_gain_sensors, _lib.LOOK_TRACE_GAIN)):
            act = agent(None, env)
            want = _greedy_np(_np(env.lookahead_sensors())["score"][:, col, :])
            assert act.dtype == np.int64 and act.shape == (3,) and len(set(act.tolist())) == 3
            assert ((act >= 0) & (act < env.m)).all()
            assert np.array_equal(act[want >= 0], want[want >= 0]), (k, act, want)
        env.step(act)


def test_a_sensor_without_a_reachable_object_gets_an_unused_one(envs):
    from ssa_gym_amd import agents
    env = envs.make('ssa_tasker_simple-v2', config=cfg8(envs, seed=7, sensor_obs_limit=[15, 10, 90]))   # (sensor 2 sees nothing)
    env.action_space.seed(1)
    rs = np.random.RandomState(8)
    _advance(env, rs, 2)
    draws = env.np_random.get_state()[2]
    for _ in range(5):
        net = _np(env.lookahead_sensors())
        assert np.isnan(net["score"][2]).all() and not net["visible"][2].any()
        act = agents.agent_info_gain_sensors(None, env)
        assert len(set(act.tolist())) == 3 and 0 <= act[2] < env.m
        want = _greedy_np(net["score"][:, 2, :])
        assert want[2] == -1 and np.array_equal(act[:2][want[:2] >= 0], want[:2][want[:2] >= 0])
    assert env.np_random.get_state()[2] == draws      # (the env's noise stream is not touched by the fallback)
    env.step(act)


def test_one_sensor_agents_match_the_single_sensor_agents(envs):
    from ssa_gym_amd import agents
    env = envs.make('ssa_tasker_simple-v2', config=cfg8(envs, sensors=0, seed=9))
    rs = np.random.RandomState(10)
    _advance(env, rs, 2)
    for _ in range(5):
        a = agents.agent_info_gain_sensors(None, env)
        if np.isfinite(_np(env.lookahead())["score"][2]).any():
            assert a == agents.agent_info_gain(None, env)
        b = agents.agent_trace_gain_sensors(None, env)
        if np.isfinite(_np(env.lookahead())["score"][0]).any():
            assert b == agents.agent_trace_gain(None, env)
        env.step(a)
