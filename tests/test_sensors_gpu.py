"""Sensor networks on the MI355X (include/ssa_hip.h: ssa_env_step_sensors_f64; SSA_Tasker_Env with config['observers']).

The ground truth is the project's own single-sensor step.  A step reads history slot i and writes slot i + 1, so the same step can be
launched again with the status words and the failure counter restored: the sensor step of actions a[0..S-1] must leave every object a[s]
bit-identical to a single-sensor step with action a[s] and sensor s's site, elevation mask, R and noise table, its update record s equal to
that step's record, and every other object bit-identical to a step with no update."""
import numpy as np
import pytest

from support.gpu import envs  # noqa: F401  (the module fixture)
from support.sensors import _advance, _distinct, _Relaunch, cfg3, xyz_net

pytestmark = pytest.mark.gpu


def check_decomposition(env, acts):
    """the sensor step of `acts` (C level: < 0 idle, duplicates allowed) against single-sensor steps and a step without update"""
    from ssa_gym_amd import _lib
    rl = _Relaunch(env)
    m = env.m
    got = rl.sensors(acts)
    none = rl.single(0, -1)
    winners = {}
    for s, a in enumerate(acts):
        if 0 <= a < m and a not in acts[:s]:
            winners[s] = int(a)
    assert np.array_equal(got["xt"], none["xt"])
    rest = np.setdiff1d(np.arange(m), list(winners.values()))
    for k in ("x", "P", "st"):
        assert np.array_equal(got[k][rest], none[k][rest]), k
    taken = 0
    for s in range(env.n_sensor):
        rec = got["upd"][s]
        if s not in winners:
            assert rec[_lib.UPD_ACTION] == -1 and rec[_lib.UPD_OBS_TAKEN] == 0 and rec[_lib.UPD_VISIBLE] == 0, (s, rec[:8])
            continue
        a = winners[s]
        one = rl.single(s, a)
        for k in ("x", "P", "st"):
            assert np.array_equal(got[k][a], one[k][a]), (s, a, k)
        assert np.array_equal(got["upd"][s].view(np.int64), one["upd"][0].view(np.int64)), (s, a)
        taken += int(rec[_lib.UPD_OBS_TAKEN] == 1.0)
    return got, taken


def _visibility_next(env):
    """per sensor: the update's visibility test at step i + 1 (elevation of the true state there, from site s)"""
    import torch
    from ssa_gym_amd import device
    rl = _Relaunch(env)
    rl.sensors([-1] * env.n_sensor)
    e = env._engine
    sl = (env.i + 1) % e.H
    M = e.trans[(env.i + 1) % e.n_time].reshape(3, 3)
    vis = [device.visible_mask(e.x_true[sl], M, env._sensor_consts[s]).cpu().numpy().astype(bool) for s in range(env.n_sensor)]
    torch.cuda.synchronize()
    return vis


def _scenarios(env, rs, failed=False):
    vis = _visibility_next(env)
    st = env._engine.status.cpu().numpy()
    m = env.m
    ok = st == 0
    # three objects of one tile (one wavefront), each preferably visible to the sensor that takes it
    score = np.array([vis[0][b] + vis[1][b + 1] + vis[2][b + 2] if ok[b:b + 3].all() else -1 for b in range(0, m - 3, 4)])
    b = 4 * int(rs.choice(np.where(score == score.max())[0]))
    cross = np.where(~vis[0] & vis[1] & ok)[0]
    assert len(cross), "no object hidden from sensor 0 and visible to sensor 1"
    j = int(rs.choice(cross))
    third = int(rs.choice(np.where(vis[2] & ok)[0]))
    out = [[b, b + 1, b + 2], [j, third, int(rs.randint(m))] if third != j else [j, -1, b], [b, -1, b]]
    if failed:
        bad = np.where(st != 0)[0]
        assert len(bad), "no failed filter yet"
        out.append([int(rs.choice(bad)), b, int(rs.choice(np.where(vis[2] & ok & (np.arange(m) != b))[0]))])
    return out


def test_one_site_network_is_the_default_env_bit_for_bit(envs):
    """observers=[observer]: 120 steps at 2 000 objects ('hybrid') -- states, covariances, observations, rewards, failures identical"""
    import torch
    base = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, sensors=0))
    cfg = cfg3(envs, sensors=0)
    cfg['observers'] = [tuple(cfg['observer'])]
    one = envs.make('ssa_tasker_simple-v2', config=cfg)
    assert one.n_sensor == 1 and np.allclose(one.sensor_lla[0], one.obs_lla) and one.action_space.n == one.m
    assert np.array_equal(base.z_noise, one.z_noise)
    rs = np.random.RandomState(1)
    for _ in range(120):
        a = int(rs.randint(base.m))
        ob, rb, db, _ = base.step(a)
        oo, ro, do, _ = one.step(a)
        assert np.array_equal(ob, oo) and (rb == ro or (np.isnan(rb) and np.isnan(ro))) and db == do
    torch.cuda.synchronize()
    for name in ("x_true", "x_filter", "P_filter", "obs"):
        assert np.array_equal(getattr(base._engine, name)[:121].cpu().numpy(), getattr(one._engine, name)[:121].cpu().numpy()), name
    assert np.array_equal(base._engine.status.cpu().numpy(), one._engine.status.cpu().numpy())
    assert base.failed_filters_id == one.failed_filters_id
    assert np.array_equal(base.obs_taken, one.obs_taken) and np.array_equal(base.sigmas_h, one.sigmas_h)


def test_one_sensor_kernel_equals_the_step_kernel(envs):
    """ssa_env_step_sensors_f64 with S = 1 leaves the same bits and the same record as ssa_env_step_f64, at every step of 120"""
    from ssa_gym_amd import host
    cfg = cfg3(envs, sensors=0)
    env = envs.make('ssa_tasker_simple-v2', config=cfg)
    sp = host.make_sensor_params([env.obs_lla], [env.obs_limit], [env.R], 0)
    env._sensors = sp
    rs = np.random.RandomState(2)
    for _ in range(120):
        a = int(rs.randint(env.m))
        rl = _Relaunch(env)
        got = rl.sensors([a], sp)
        ref = rl.single(0, a)
        for k in ("x", "P", "xt", "st"):
            assert np.array_equal(got[k], ref[k]), (env.i, k)
        assert np.array_equal(got["upd"][0].view(np.int64), ref["upd"][0].view(np.int64)), env.i
        env.step(a)


@pytest.mark.parametrize("late", [False, True])
def test_three_sensors_decompose_into_single_sensor_steps_at_20000(envs, late):
    """step 2 and step 310 (failed filters among the tasked) at 20 000 objects, 'hybrid': three objects in one tile, an object hidden from
    its sensor but visible to another, an idle sensor, two sensors on one object (the lower one updates it)"""
    env = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, m=20000))
    rs = np.random.RandomState(7)
    _advance(env, rs, 309 if late else 1)
    taken = 0
    for acts in _scenarios(env, rs, failed=late):
        taken += check_decomposition(env, acts)[1]
    assert taken >= 1          # (visible tasked objects were updated)
    _advance(env, rs, 1)


def test_xyz_and_the_other_propagators_decompose(envs):
    for over in (xyz_net(), dict(propagator='fg'), dict(propagator='elements'), dict(propagator='j2')):
        env = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, **over))
        rs = np.random.RandomState(11)
        _advance(env, rs, 3)
        for acts in _scenarios(env, rs):
            check_decomposition(env, acts)


def test_update_interval_on_an_update_step_and_a_skipped_step(envs):
    env = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, update_interval=3))
    rs = np.random.RandomState(5)
    _advance(env, rs, 4)        # next step 5: skipped
    got, taken = check_decomposition(env, [1, 2, 3])
    assert taken == 0 and (got["upd"][:, 56] == -1).all()
    _advance(env, rs, 1)        # next step 6: an update step
    for acts in _scenarios(env, rs):
        check_decomposition(env, acts)


def test_regime_layout_gives_the_same_bits(envs):
    a_env = envs.make('ssa_tasker_simple-v2', config=cfg3(envs))
    b_env = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, storage_layout='regime'))
    rs = np.random.RandomState(9)
    for _ in range(60):
        a = _distinct(rs, a_env.m, 3)
        oa, ra, _, _ = a_env.step(a)
        ob, rb, _, _ = b_env.step(a)
        assert np.array_equal(oa, ob) and ra == rb
        assert np.array_equal(a_env._upd_s_np.view(np.int64), b_env._upd_s_np.view(np.int64))
    assert np.array_equal(a_env.P_filter[60], b_env.P_filter[60]) and np.array_equal(a_env.x_filter[60], b_env.x_filter[60])
    assert np.array_equal(a_env.obs_taken, b_env.obs_taken) and a_env.failed_filters_id == b_env.failed_filters_id


def test_reward_types_and_the_any_sensor_shaped_rule(envs):
    from ssa_gym_amd import _lib
    for rt in ('jones', 'trinary', 'shaped'):
        env = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, reward_type=rt))
        rs = np.random.RandomState(4)
        hits = 0
        for k in range(40):
            prev = env._argmax_sigma
            a = _distinct(rs, env.m, 3)
            if rt == 'shaped' and k % 2 and 0 <= prev < env.m:
                a = np.asarray([x for x in a if x != prev][:1] + [prev] + [x for x in a if x != prev][1:2])   # sensor 1 takes it
            _, r, done, _ = env.step(a)
            assert np.isfinite(r)
            if rt == 'shaped':
                md = env._stats[_lib.STAT_MAX_DPOS]
                if 3e4 <= md <= 5e6:
                    want = 1 / env.n if prev in a else -1 / env.n
                    assert r == want, (k, a, prev, r)
                    hits += prev in a
            if done:
                break
        if rt == 'shaped':
            assert hits > 0


def test_480_step_episode_at_20000_with_three_sensors(envs):
    env = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, m=20000))
    rs = np.random.RandomState(3)
    done, steps = False, 0
    while not done:
        _, _, done, _ = env.step(_distinct(rs, env.m, 3))
        steps += 1
    assert steps == 479 and env.i == 479
    assert len(env.failed_filters_id) > 0 and env.failed_filters_msg[env.failed_filters_id[0]] != "None"
    nis = env.nis()
    assert nis.shape == (480, 3)
    n_upd = int(env.obs_taken[1:480].sum())
    assert n_upd > 479 and np.isfinite(nis[1:480][env.obs_taken[1:480]]).sum() >= n_upd - 5
    fit = env.fitness_chi2()
    assert fit['nis_valid'] == int(np.isfinite(nis).sum()) > 479
    assert env.y.shape == (480, 3, 3) and np.isfinite(env.y[env.obs_taken]).all()
    assert env.visible_objects(sensor=2).size >= 0 and env.object_visibility(sensor=1).shape == (env.m,)
