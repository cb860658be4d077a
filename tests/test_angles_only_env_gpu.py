"""Angles-only sensors through every entry point and both envs (config['sensor_measurement']), at the mixed kinds ('aer', 'ae', 'ae'):
one definition of the update -- the lookahead, the forecast, the rollout and the dry run equal the step bit for bit, the vector env
equals single envs --; no change without the key; and the env's NIS and chi-square bookkeeping.  8 objects, 3 sites, 16 steps; the
catalogue the envs draw from stands high above every site's mask for the whole episode."""
import numpy as np
import pytest

from support import angles_only as ao
from support.batches import c2t
from support.dryrun import forecast_entries, record_bits, result_bits, same_result, step_chain
from support.gpu import envs, hip  # noqa: F401  (the module fixtures)
from support.sensors import N_TIME, _assert_same_env, _Relaunch
from support.vector_lookahead import single_envs
from support.vector_rollout import run_pair

pytestmark = pytest.mark.gpu

M, S = 8, 3
_ORBITS = {}


def _orbits(oracle_ld):
    """32 states that all three sites (some 200 km apart) see 45 degrees or more above the horizon at step 4, 12 000 km or more away:
    they move a few degrees over the 16 steps"""
    if "o" not in _ORBITS:
        from ssa_gym_amd import envs as E
        from ssa_gym_amd.envs._config import resolve_config
        c = resolve_config(ao.mixed_cfg(E))
        rs = np.random.RandomState(21)
        itrs = oracle_ld.lla2ecef(c.net.lla[0])
        out = []
        for _ in range(32):
            t = ao.place(c.net.lla[0], itrs, c.trans[4], rs.uniform(0, 2 * np.pi), rs.uniform(np.radians(50.0), np.radians(75.0)),
                         rs.uniform(1.2e7, 3e7), rs)
            out.append(oracle_ld.propagate(t, -4 * c.dt)[0])
        _ORBITS["o"] = np.array(out)
    return _ORBITS["o"]


def _cfg(envs, oracle_ld, **over):
    return ao.mixed_cfg(envs, orbits=_orbits(oracle_ld), x_sigma=tuple(ao.X_SIGMA), P_0=np.diag(ao.X_SIGMA ** 2), **over)


def _np(r):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in r.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a.astype(np.int64)


def _distinct(rs, m=M):
    return rs.permutation(m)[:S]


# ---------------------------------------------------------------------------------------------------------------- 8. one definition
def test_lookahead_equals_the_step_for_every_sensor_and_object_and_slab_0_of_the_forecast(envs, oracle_ld):
    """lookahead_sensors(): P_post, status and visible of every (sensor, object) are the step's with that one action; the score is a
    number exactly where the step took the observation, and its trace gain is tr P- - tr P+ of those covariances.  forecast_sensors(3):
    slab 0 is the lookahead, every key."""
    from ssa_gym_amd import _lib as L
    env = envs.make(config=_cfg(envs, oracle_ld))
    assert env.sensor_angles_only.tolist() == [False, True, True] and env._sensors.angles_only == 0b110
    rs = np.random.RandomState(1)
    for _ in range(2):
        env.step(_distinct(rs))
    look = _np(env.lookahead_sensors(covariances=True))
    fc = _np(env.forecast_sensors(3, covariances=True))
    assert set(fc) == set(look)
    for k in look:
        assert np.array_equal(_bits(fc[k][0]), _bits(np.moveaxis(look[k], 1, 2) if k == "score" else look[k])), k
    rl = _Relaunch(env)
    taken = np.zeros(S, dtype=int)
    for s in range(S):
        for j in range(M):
            out = rl.sensors([j if q == s else -1 for q in range(S)])
            assert np.array_equal(out["P"][j], _bits(look["P_post"][s, j]).reshape(36)), (s, j)
            assert out["st"][j] == look["status"][s, j] == 0 and out["upd"][s, L.UPD_VISIBLE] == look["visible"][s, j], (s, j)
            got = out["upd"][s, L.UPD_OBS_TAKEN] == 1.0
            assert got == bool(np.isfinite(look["score"][s, :, j]).all()) == (not np.isnan(look["score"][s, :, j]).any()), (s, j)
            if got:
                gain = np.trace(look["P_prior"][j]) - np.trace(look["P_post"][s, j])
                assert abs(look["score"][s, L.LOOK_TRACE_GAIN, j] - gain) <= 1e-9 * np.trace(look["P_prior"][j]), (s, j)
                taken[s] += 1
    assert (taken == M).all(), taken      # (every object stands above every mask)
    # the kinds differ in kind: from the same prior an az-el update leaves the along-range variance where it was.  The range sensor's
    # sigma is 1 km; the prior's along-range sd is 1 km at first and 0.58 km or more after the two steps taken (two range updates at
    # most), so the range update takes a quarter of it or more, and the cross-range terms (150 m at 30 000 km) are small against either
    for j in range(M):
        p = [np.trace(look["P_post"][s, j][:3, :3]) for s in range(S)]
        assert p[1] > 1.2 * p[0] and p[2] > 1.2 * p[0], (j, p)


def test_rollout_equals_three_steps(envs, oracle_ld):
    a, b = envs.make(config=_cfg(envs, oracle_ld)), envs.make(config=_cfg(envs, oracle_ld))
    rs = np.random.RandomState(2)
    sched = np.stack([_distinct(rs) for _ in range(3)])
    obs_a = None
    for row in sched:
        obs_a, _, _, _ = a.step(row)
    obs_b, rew, don, _ = b.rollout_sensors(sched)
    assert np.array_equal(_bits(np.asarray(obs_a)), _bits(np.asarray(obs_b))) and np.array_equal(_bits(a.rewards[1:4]), _bits(rew))
    _assert_same_env(a, b, "rollout_sensors against three steps")
    assert a.obs_taken[1:4].all() and a.i == 3


def _dry_engine(hip, oracle, oracle_ld, tix):
    """an engine in the placed scene of tests/test_angles_only_gpu.py, zero noise, at time row tix - 1 (slot 0)"""
    import torch
    from support.batches import make_batch
    net = ao.Net(oracle)
    g = make_batch(1, seed=0)[3]
    consts = hip.host.make_consts(g["Q"], net.R[0], ao.ALPHA, 2.0, -3, ao.DT, net.lim[0], net.lla[0], propagator="hybrid")
    zn = torch.zeros((S, N_TIME, M, 3), dtype=torch.float64, device="cuda")
    eng = hip.engine.HotPathEngine(consts, M, 1, c2t()[:N_TIME], zn, history=2, zn_stride_env=0)
    eng.load_state(0, *ao.scene(net, oracle_ld, c2t()[tix], M, 7, high=True))
    return eng, net.params(N_TIME * M * 3)


def test_dry_run_equals_the_forecast_and_the_chain(hip, oracle, oracle_ld):
    """evaluate_schedules' launch: a once-per-object schedule is the forecast's entries; a revisit by an az-el sensor after the
    az-el-range one (and the other way round) is the step-by-step chain's -- gathered and full-catalogue form"""
    torch = hip.torch
    eng, sp = _dry_engine(hip, oracle, oracle_ld, 3)
    fc = _np(eng.launch_forecast_sensors(0, 3, sp, 3))
    once = np.array([[0, 1, 2], [3, 4, 5], [6, 7, -1]])
    want = forecast_entries(fc, once, M, 3)
    assert want["taken"].sum() == 8, want["taken"]
    for gather in (True, False):
        same_result(record_bits(eng.launch_dryrun_sensors(0, 3, sp, once[None], gather=gather)), want, ("once", gather))
    # object 0: the az-el-range sensor, then az-el sensor 1, then az-el sensor 2; object 4: az-el sensor 1, then the az-el-range one
    revisit = np.array([[0, 4, -1], [-1, 0, -1], [4, -1, 0]])
    twin, _ = _dry_engine(hip, oracle, oracle_ld, 3)
    chain, _ = step_chain(torch, twin, sp, revisit, 0, 3)
    slots = [(0, 0), (1, 1), (2, 2), (0, 1), (2, 0)]
    assert all(chain["taken"][0, k, s] for k, s in slots), chain["taken"]
    for k, s in slots[1:3] + slots[4:]:      # a later visit is worth less than the forecast's first-visit entry: not the same number
        assert not np.array_equal(chain["score"][0, k, s], fc["score"][k, s, revisit[k, s]].view(np.int64)), (k, s)
    for gather in (True, False):
        same_result(record_bits(eng.launch_dryrun_sensors(0, 3, sp, revisit[None], gather=gather)), chain, ("revisit", gather))


def test_vector_env_equals_two_single_envs(envs, oracle_ld):
    """E = 2, m = 8: step, lookahead_sensors, forecast_sensors, evaluate_schedules and rollout_sensors against two single envs"""
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    cfg = _cfg(envs, oracle_ld)
    E = 2
    vec = SSA_Tasker_VecEnv(cfg, E, seed=10)
    assert vec.sensor_angles_only.tolist() == [False, True, True] and vec._sensors.angles_only == 0b110
    singles = single_envs(envs, cfg, vec, 10)
    rs = np.random.RandomState(4)
    finite = 0
    for k in range(3):
        look = _np(vec.lookahead_sensors(covariances=True))
        fc = _np(vec.forecast_sensors(3, covariances=True))
        a = np.stack([[np.stack([_distinct(rs) for _ in range(3)]) for _ in range(2)] for _ in range(E)])      # [E, B, K, S]
        a[0, 1, 1, 2] = a[0, 1, 0, 0]      # (a revisit by an az-el sensor of what the az-el-range one took a step earlier)
        dry = result_bits(vec.evaluate_schedules(a))
        for e, one in enumerate(singles):
            for got, want in ((look, _np(one.lookahead_sensors(covariances=True))), (fc, _np(one.forecast_sensors(3, covariances=True)))):
                assert set(got) == set(want)
                for name in want:
                    assert np.array_equal(got[name][e].view(np.uint8), want[name].view(np.uint8)), (k, e, name)
            want = result_bits(one.evaluate_schedules(a[e]))
            same_result({key: v[e] for key, v in dry.items()}, want, (k, e), keys=tuple(want))
        finite += int(np.isfinite(look["score"]).sum())
        acts = np.stack([_distinct(rs) for _ in range(E)])
        vec.step(acts)
        for e, one in enumerate(singles):
            one.step(acts[e])
            for name in ("x_true", "x_filter", "P_filter"):
                assert np.array_equal(_bits(getattr(vec, name)(e)), _bits(getattr(one, name)[one.i])), (k, e, name)
    assert finite >= 3 * E * S * M * 3 // 2
    # rollout_sensors: K = 3 in one launch against step() on a twin (two fresh envs of one seed: the same episode)
    a, b = SSA_Tasker_VecEnv(cfg, E, seed=11), SSA_Tasker_VecEnv(cfg, E, seed=11)
    sched = np.stack([np.stack([_distinct(rs) for _ in range(3)]) for _ in range(E)])
    calls, dones = run_pair(a, b, sched)
    assert calls == 1 and not dones.any() and a.i.tolist() == [3] * E


# ---------------------------------------------------------------------------------------------------------------- 9. no change without the key
def test_all_aer_kinds_are_the_env_without_the_key(envs, oracle_ld):
    """config['sensor_measurement'] = ['aer'] * 3 against the key absent: a 6-step episode with random distinct actions, the device
    state and every host history identical"""
    a = envs.make(config=_cfg(envs, oracle_ld, kinds=['aer'] * S))
    b = envs.make(config=_cfg(envs, oracle_ld, kinds=None))
    assert 'sensor_measurement' not in _cfg(envs, oracle_ld, kinds=None)
    assert a._sensors.angles_only == b._sensors.angles_only == 0 and not a.sensor_angles_only.any() and not b.sensor_angles_only.any()
    rs = np.random.RandomState(6)
    for k in range(6):
        acts = _distinct(rs)
        oa, ra, da, _ = a.step(acts)
        ob, rb, db, _ = b.step(acts)
        assert np.array_equal(_bits(np.asarray(oa)), _bits(np.asarray(ob))) and ra == rb and da == db, k
        _assert_same_env(a, b, "step %d" % k)
    assert a.obs_taken[1:7].all()
    # ... and the mixed network is another episode
    c = envs.make(config=_cfg(envs, oracle_ld))
    rs = np.random.RandomState(6)
    for k in range(6):
        c.step(_distinct(rs))
    assert not np.array_equal(_bits(c.P_filter[6]), _bits(a.P_filter[6]))


# ---------------------------------------------------------------------------------------------------------------- 10. env level
def test_env_nis_and_fitness_counts_per_kind(envs, oracle_ld):
    """a 10-step episode: env.nis() of an az-el update is y2^T inv(S2) y2 of the booked record (the block form makes ssa_nis_f64 return
    it as it stands); fitness_chi2() counts the az-el updates against the 2-dof interval -2 ln(1 - alpha/2) .. -2 ln(alpha/2), the
    others against the 3-dof one, pooled"""
    env = envs.make(config=_cfg(envs, oracle_ld))
    rs = np.random.RandomState(8)
    for _ in range(10):
        env.step(_distinct(rs))
    assert env.obs_taken[1:11].all() and env.obs_taken[1:11].shape == (10, S)
    nis = env.nis()
    want = np.full((10, S), np.nan)
    for i in range(1, 11):
        for s in range(S):
            y, Sm = env._y[i, s], env._S_sel[i, s]
            if env.sensor_angles_only[s]:
                assert y[2] == 0.0 and np.array_equal(Sm[2], [0.0, 0.0, 1.0]) and np.array_equal(Sm[:, 2], [0.0, 0.0, 1.0]), (i, s)
                want[i - 1, s] = y[:2] @ np.linalg.solve(Sm[:2, :2], y[:2])
            else:
                want[i - 1, s] = y @ np.linalg.solve(Sm, y)
    np.testing.assert_allclose(nis[1:11], want, rtol=1e-9)
    assert np.isnan(nis[0]).all() and np.isnan(nis[11:]).all()
    alpha = 0.05
    lo2, hi2 = -2 * np.log(1 - alpha / 2), -2 * np.log(alpha / 2)
    lo3, hi3 = 0.21579528262389788, 9.348403604496145      # (chi2.ppf([0.025, 0.975], 3); other alphas need scipy for 3 dof, as before)
    assert abs(lo2 - 0.050635615968579795) < 1e-15 and abs(hi2 - 7.377758908227871) < 1e-14      # (chi2.ppf([0.025, 0.975], 2))
    np.testing.assert_allclose(env._chi2_points(alpha, 2), (lo2, hi2), rtol=1e-15)
    np.testing.assert_allclose(env._chi2_points(0.3, 2), (-2 * np.log(0.85), -2 * np.log(0.15)), rtol=1e-15)
    v = nis[1:11]
    ang = np.broadcast_to(env.sensor_angles_only, v.shape)
    inside = int(((v > lo2) & (v < hi2) & ang).sum() + ((v > lo3) & (v < hi3) & ~ang).sum())
    got = env.fitness_chi2(alpha)
    assert (got['nis_inside'], got['nis_valid']) == (inside, 10 * S), (got, inside)
    assert got['Test 2: NIS chi2'] == round(100.0 * inside / (10 * S), 2)
    # the rule per kind, on constructed values: 8.0 lies inside the 3-dof interval and outside the 2-dof one, 0.1 the other way round
    env._y[1:11] = 0.0
    env._y[1:11, :, 0] = np.sqrt(8.0)
    env._S_sel[1:11] = np.eye(3)
    assert env.fitness_chi2(alpha)['nis_inside'] == 10          # (the az-el-range sensor's ten)
    env._y[1:11, :, 0] = np.sqrt(0.1)
    assert env.fitness_chi2(alpha)['nis_inside'] == 20          # (the az-el sensors' twenty)
