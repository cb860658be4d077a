"""A sensor network in each of E envs, one launch per vector step (include/ssa_hip.h: ssa_env_step_sensors_envs_f64;
HotPathEngine.launch_step_sensors_envs; SSA_Tasker_VecEnv with config['observers']) on the MI355X.

The yardstick is the project's own one-env path, which this feature leaves untouched: E one-env engines stepped by launch_step_sensors
(E single envs stepped by step()), each holding env e's state slice, noise tables and time index.  Everything is compared bit for
bit; there is no tolerance anywhere."""
import numpy as np
import pytest

from conftest import golden
from support.batches import c2t, make_batch
from support.gpu import envs, hip  # noqa: F401  (the module fixtures)
from support.sensors import BAD, N_TIME, _defined_fields, cfg3, sites_rad, xyz_net

pytestmark = pytest.mark.gpu

MASKS_DEG = [15.0, -90.0, -80.0, 0.0, 5.0, -10.0, 20.0, -30.0]     # (sensor 1 sees everything: an object below sensor 0's mask is above its)
K = 3                  # consecutive steps: updated covariances feed the next step
INTERVAL = 3           # update_interval: with the time indices below, every launch updates some envs and skips others
T0 = [2, 5, 3, 1, 4, 6, 8, 7, 9]      # env e's time index before the first step (envs 0 and 1 update in the same launch)


def _bad(m):
    """the object whose filter state is NaN (support.sensors.BAD, folded into envs smaller than that)"""
    return BAD if m > BAD else BAD % m


def _net(host, S, obs_type, stride):
    lla = sites_rad()[:S]
    lim = np.radians(MASKS_DEG[:S])
    if obs_type == "aer":
        sig = [np.array([(1.0 + k) * host.arcsec2rad, (0.5 + 2.0 * k) * host.arcsec2rad, 1e3 / (1 + k)]) for k in range(S)]
    else:
        sig = [np.array([5e2 / (1 + 0.25 * k)] * 3) for k in range(S)]
    Rs = [np.diag(s ** 2) for s in sig]
    return lla, lim, Rs, sig, host.make_sensor_params(lla, lim, Rs, stride)


def _t0(E):
    return [2, 4] if E == 2 else T0[:E]


def _update_step(t0):
    ks = [k for k in range(K) if (t0 + 1 + k) % INTERVAL == 0]
    assert len(ks) == 1
    return ks[0]


def _one_env_engine(hip, consts, m, trans, zn_e, xt, x, P, e, order=None):
    eng = hip.engine.HotPathEngine(consts, m, 1, trans, zn_e, history=K + 1, zn_stride_env=0)
    if order is not None:
        eng.set_layout(order)
    sl = slice(e * m, (e + 1) * m)
    eng.load_state(0, xt[sl], x[sl], P[sl])
    return eng


def _tables(hip, rs, E, m, S, t0, consts_of, trans, zn, xt, x, P, sp):
    """the action tables [K, E, S] with every condition of the module's cases in them (asserted on the yardstick's outputs by
    _assert_conditions).  An idle pass of the one-env engines gives the visibility: the truth does not depend on the tasking."""
    bad = _bad(m)
    acts = np.stack([np.stack([rs.permutation(m)[:S] for _ in range(E)]) for _ in range(K)]).astype(np.int64)
    ku = [_update_step(t) for t in t0]
    eng = _one_env_engine(hip, consts_of[0], m, trans, zn[0], xt, x, P, 0)
    for k in range(K):
        eng.launch_step_sensors(k, k + 1, t0[0] + 1 + k, sp, [-1] * S, 0, fast_stats=True)
    hip.torch.cuda.synchronize()
    M = eng.trans[(t0[0] + 1 + ku[0]) % eng.n_time].reshape(3, 3)
    vis = [hip.dev.visible_mask(eng.x_true[ku[0] + 1], M, c).cpu().numpy().astype(bool) for c in consts_of]
    cross = [j for j in range(m) if j != bad and not vis[0][j] and vis[1][j]]
    assert cross, "no object of env 0 below sensor 0's mask and above sensor 1's"
    c = cross[0]
    spare = [j for j in range(m) if j not in (c, bad)]
    if S >= 3:
        spare = [j for j in spare if vis[2][j]] + [j for j in spare if not vis[2][j]]
        assert vis[2][spare[0]], "no object of env 0 that sensor 2 sees"
    # env 0, the step its update runs: sensors 0 and 1 on ONE object (the lower one attempts it and does not see it), sensor 2 on one it
    # sees; two steps on, the NaN filter tasked
    acts[ku[0], 0] = ([c, c] + spare)[:S]
    acts[(ku[0] + 2) % K, 0, 1] = bad
    if E >= 2:    # env 1: the NaN filter, the SAME index as env 0's (another object: sensor 1 sees and updates it), an idle sensor
        acts[ku[1], 1] = ([bad, c] + ([-1] if S >= 3 else []) + spare)[:S]
    for e in range(2, E):      # ... an index the next env does not task
        acts[ku[1], e] = [j for j in rs.permutation(m) if j != c][:S]
    if E == 2:                 # (two envs: env 1 does not task it in the launch env 0 does)
        acts[ku[0], 1] = [j for j in rs.permutation(m) if j != c][:S]
    for e in range(E):         # a step the interval skips: an idle sensor and an out-of-range action
        k = (ku[e] + 1) % K
        acts[k, e, 0], acts[k, e, S - 1] = -1, m
    return acts, c, ku


def _run_yardstick(hip, consts, E, m, S, trans, zn, xt, x, P, sp, acts, t0, argmax, fold_inside, orders=None):
    torch, L = hip.torch, hip.lib
    outs = []
    for e in range(E):
        eng = _one_env_engine(hip, consts, m, trans, zn[e], xt, x, P, e, None if orders is None else orders[e])
        upd = torch.zeros((K, S, L.UPD_STRIDE), dtype=torch.float64, device="cuda")
        for k in range(K):
            eng.launch_step_sensors(k, k + 1, t0[e] + 1 + k, sp, [int(a) for a in acts[k, e]], upd[k].data_ptr(), fast_stats=True,
                                    argmax_spos=argmax, fold_inside=fold_inside)
        if orders is not None:
            eng.to_caller_order()
        torch.cuda.synchronize()
        out = {k: getattr(eng, k).cpu().numpy() for k in ("x_true", "x_filter", "P_filter", "obs", "metrics", "status", "stats")}
        out["upd"] = upd.cpu().numpy()
        n = int(eng.fail_count.cpu().numpy()[0])
        log = eng.fail_log[:n].copy()
        assert (log[:, L.FAIL_ENV] == 0).all()
        log[:, L.FAIL_ENV] = e
        out["fail_log"] = log
        outs.append(out)
    return outs


def _run_vector(hip, consts, E, m, S, trans, zn, xt, x, P, sp, acts, t0, argmax, fold_inside, by_value, orders=None, mirror_f32=False):
    torch, L = hip.torch, hip.lib
    eng = hip.engine.HotPathEngine(consts, m, E, trans, zn, history=K + 1, zn_stride_env=S * N_TIME * m * 3)
    if orders is not None:
        eng.set_layout(np.stack(orders) if E > 1 else orders[0])
    eng.load_state(0, xt, x, P)
    upd = torch.zeros((K, E, S, L.UPD_STRIDE), dtype=torch.float64, device="cuda")
    mirror = torch.zeros((K, E * m, 12), dtype=torch.float32, device="cuda") if mirror_f32 else None
    if not by_value:
        eng.env_time0.copy_(torch.as_tensor(t0, dtype=torch.int32))
    for k in range(K):
        kw = dict(fast_stats=True, argmax_spos=argmax, fold_inside=fold_inside)
        if mirror_f32:
            kw.update(obs_mirror=mirror[k].data_ptr(), mirror_f32=True)
        if by_value:
            eng.launch_step_sensors_envs(k, k + 1, 0, sp, acts[k], upd[k].data_ptr(), env_words=[t + 1 + k for t in t0], **kw)
        else:
            eng.launch_step_sensors_envs(k, k + 1, 1 + k, sp, acts[k], upd[k].data_ptr(), **kw)
    if orders is not None:
        eng.to_caller_order()
    torch.cuda.synchronize()
    out = {k: getattr(eng, k).cpu().numpy() for k in ("x_true", "x_filter", "P_filter", "obs", "metrics", "status", "stats")}
    out["upd"] = upd.cpu().numpy()
    out["fail_log"] = eng.fail_log[:int(eng.fail_count.cpu().numpy()[0])].copy()
    out["mirror"] = mirror.cpu().numpy() if mirror_f32 else None
    return out


def _assert_conditions(L, yard, acts, E, m, S, c, ku, t0):
    """the conditions the tables were built for, found again in the tables and in the YARDSTICK's outputs"""
    bad = _bad(m)
    assert (acts == -1).any() and (acts == m).any()
    u0 = yard[0]["upd"][ku[0]]                                  # env 0's records of its update step
    assert list(acts[ku[0], 0, :2]) == [c, c]
    assert u0[0, L.UPD_ACTION] == c and u0[0, L.UPD_VISIBLE] == 0 and u0[0, L.UPD_OBS_TAKEN] == 0      # below sensor 0's mask
    assert u0[1, L.UPD_ACTION] == -1                            # the duplicate: the lower sensor holds the object
    for e in range(E):
        assert yard[e]["status"][bad] != 0                      # the NaN filter failed
        assert any(int(r[L.FAIL_OBJ]) == bad and r[L.FAIL_TIME] == t0[e] + 1 for r in yard[e]["fail_log"]), e
        k = (ku[e] + 1) % K                                     # a step the interval skips for env e: cleared records
        assert (yard[e]["upd"][k][:, L.UPD_ACTION] == -1).all(), e
    assert acts[(ku[0] + 2) % K, 0, 1] == bad                  # the NaN filter, tasked after it failed
    if S >= 3:
        assert u0[2, L.UPD_OBS_TAKEN] == 1
    if E >= 2:
        s_bad = list(acts[ku[1], 1]).index(bad)
        assert yard[1]["upd"][ku[1]][s_bad, L.UPD_ACTION] == -1    # tasked, and skipped as a failed filter
        u1 = yard[1]["upd"][ku[1]]
        assert acts[ku[1], 1, 1] == c and u1[1, L.UPD_ACTION] == c and u1[1, L.UPD_OBS_TAKEN] == 1      # the same index, seen by sensor 1
        if S >= 3:
            assert acts[ku[1], 1, 2] == -1 and u1[2, L.UPD_ACTION] == -1
        assert len(set(t0)) == E                                # envs at different time indices
        launches = [sorted(e for e in range(E) if ku[e] == k) for k in range(K)]
        assert any(0 < len(up) < E for up in launches), launches      # a launch that updates some envs and skips others
    if E >= 3:
        assert ku[0] == ku[1] and c not in acts[ku[1], 2]       # tasked in envs 0 and 1 (one launch), not in the next
    elif E == 2:
        assert c not in acts[ku[0], 1]
    assert any((y["upd"][..., L.UPD_OBS_TAKEN] == 1).any() and ku[e] < K - 1 for e, y in enumerate(yard))      # an update feeds a later step


def _assert_equal(L, yard, vec, E, m, argmax):
    words = [L.STAT_MAX_DPOS, L.STAT_CNT_LT_1E4, L.STAT_CNT_LT_1E7, L.STAT_N_FAILED] + ([L.STAT_ARGMAX_SPOS, L.STAT_MAX_SPOS] if argmax else [])
    for e in range(E):
        sl, y = slice(e * m, (e + 1) * m), yard[e]
        for nme in ("x_true", "x_filter", "P_filter", "obs"):
            assert np.array_equal(vec[nme][:, sl].view(np.int64), y[nme].view(np.int64)), (e, nme)
        assert np.array_equal(vec["metrics"][:, e].view(np.int64), y["metrics"][:, 0].view(np.int64)), (e, "metrics")
        assert np.array_equal(vec["status"][sl], y["status"]), (e, "status")
        for k in range(K):
            for w in words:
                assert np.array_equal(vec["stats"][k + 1, e, w], y["stats"][k + 1, 0, w], equal_nan=True), (e, k, w)
        a, b = _defined_fields(L, vec["upd"][:, e]), _defined_fields(L, y["upd"])
        assert np.array_equal(a, b, equal_nan=True), (e, "upd")
    key = lambda r: tuple(np.nan_to_num(r, nan=-1.0))      # noqa: E731
    want = sorted(np.concatenate([y["fail_log"] for y in yard]).tolist(), key=key)
    got = sorted(vec["fail_log"].tolist(), key=key)
    assert len(got) == len(want) and np.array_equal(np.array(got), np.array(want), equal_nan=True)


def _case(hip, E, m, S, propagator="hybrid", obs_type="aer", by_value=None, argmax=False, fold_inside=False, layout=False, mirror_f32=False):
    torch, L, host = hip.torch, hip.lib, hip.host
    by_value = (E <= L.INLINE_ENVS) if by_value is None else by_value
    xt, x, P, g = make_batch(E * m, seed=123)
    for e in range(E):
        x[e * m + _bad(m), 1] = np.nan
    trans = c2t()[:N_TIME]
    lla, lim, Rs, sig, sp = _net(host, S, obs_type, N_TIME * m * 3)
    consts_of = [host.make_consts(g["Q"], Rs[s], 1e-4, 2.0, -3, 20.0, lim[s], lla[s], propagator=propagator, obs_type=obs_type,
                                  update_interval=INTERVAL) for s in range(S)]
    gen = torch.Generator(device="cuda").manual_seed(8)
    zn = torch.randn((E, S, N_TIME, m, 3), dtype=torch.float64, device="cuda", generator=gen) * \
        torch.as_tensor(np.stack(sig), device="cuda").view(1, S, 1, 1, 3)
    t0 = _t0(E)
    rs = np.random.RandomState(17)
    acts, c, ku = _tables(hip, rs, E, m, S, t0, consts_of, trans, zn, xt, x, P, sp)
    orders = [np.random.RandomState(40 + e).permutation(m) for e in range(E)] if layout else None
    yard = _run_yardstick(hip, consts_of[0], E, m, S, trans, zn, xt, x, P, sp, acts, t0, argmax, fold_inside)
    _assert_conditions(L, yard, acts, E, m, S, c, ku, t0)
    vec = _run_vector(hip, consts_of[0], E, m, S, trans, zn, xt, x, P, sp, acts, t0, argmax, fold_inside, by_value, orders, mirror_f32)
    _assert_equal(L, yard, vec, E, m, argmax)
    return yard, vec


@pytest.mark.parametrize("E,m,S", [(3, 8, 3), (9, 12, 8), (2, 4, 2), (6, 4000, 2), (1, 7, 3)])
def test_vector_launch_equals_one_env_launches(hip, E, m, S):
    """(3, 8, 3): the one-tile instance, two tiles per env, rows by value; (9, 12, 8): the device table, more envs than travel by value,
    every sensor slot; (2, 4, 2): one tile per env; (6, 4000, 2): 24 000 objects, the grid-stride instance, tiles of several envs per
    wavefront; (1, 7, 3): one env with a ragged tile, against ssa_env_step_sensors_f64 directly"""
    _case(hip, E, m, S)


def test_vector_launch_rows_from_the_device_table_with_few_envs(hip):
    _case(hip, 2, 4, 2, by_value=False)
    _case(hip, 1, 7, 3, by_value=False)


@pytest.mark.parametrize("propagator,obs_type", [("fg", "aer"), ("j2", "aer"), ("elements", "aer"), ("hybrid", "xyz")])
def test_vector_launch_every_propagator_and_the_xyz_observation(hip, propagator, obs_type):
    _case(hip, 3, 8, 3, propagator=propagator, obs_type=obs_type)


def test_vector_launch_with_per_env_layouts(hip):
    """per-env obj_ids (set_layout with [E][m] permutations) against the caller's order: actions, records, failure records and the
    arg-max speak each env's own indices"""
    _case(hip, 3, 8, 3, layout=True, argmax=True)


def test_vector_launch_folds_inside_with_argmax(hip):
    _case(hip, 3, 8, 3, fold_inside=True, argmax=True)


def test_vector_launch_mirror_f32(hip):
    """SSA_LAUNCH_MIRROR_F32: the second copy of the observation rows is the float64 rows rounded to single precision"""
    _, vec = _case(hip, 3, 8, 3, mirror_f32=True)
    for k in range(K):
        assert np.array_equal(vec["mirror"][k].view(np.int32), vec["obs"][k + 1].astype(np.float32).view(np.int32)), k


# ---------------------------------------------------------------------------------------------------------------- env level
def _vec_cfg(envs, **over):
    return cfg3(envs, m=8, steps=12, update_interval=1, **over)


def _singles(envs, cfg, vec, seed):
    """E single envs with seeds seed + e, their engines' noise tables overwritten with the vector env's draws (e, s, i) for every object"""
    singles = []
    for e in range(vec.E):
        one = envs.make(config=dict(cfg, seed=seed + e))
        z = vec._eng.z_noise[e]                                  # [S, n, 1, 3]
        one._engine.z_noise.copy_(z.expand(vec.n_sensor, vec.n, vec.m, 3).reshape(one._engine.z_noise.shape))
        singles.append(one)
    return singles


@pytest.mark.parametrize("mode,reward", [("flatten", "trinary"), ("aer", "trinary"), ("flatten", "shaped"), ("aer", "shaped")])
def test_vector_env_equals_single_envs(envs, mode, reward):
    import torch
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    cfg = _vec_cfg(envs, obs_returned=mode, reward_type=reward)
    E, S, m = 3, 3, 8
    vec = SSA_Tasker_VecEnv(cfg, E, seed=10)
    assert vec.single_action_space.shape == (S,) and vec._eng.z_noise.shape == (E, S, 12, 1, 3)
    singles = _singles(envs, cfg, vec, 10)
    rs = np.random.RandomState(4)
    for e in range(E):
        assert np.array_equal(vec.x_true(e), singles[e].x_true[0]) and np.array_equal(vec.x_filter(e), singles[e].x_filter[0])
    seen, live = set(), list(range(E))
    for k in range(1, 11):
        acts = np.stack([rs.permutation(m)[:S] for _ in range(E)])
        assert tuple(acts.reshape(-1)) not in seen
        seen.add(tuple(acts.reshape(-1)))
        obs, rew, done, infos = vec.step(acts)
        assert obs.shape == (E, m * (12 if mode == "flatten" else 4))
        for e in list(live):
            o1, r1, d1, _ = singles[e].step(acts[e])
            assert rew[e] == r1 and bool(done[e]) == bool(d1), (k, e, rew[e], r1)
            got = obs[e]
            if done[e]:      # ('shaped' may end an episode early: the vector env has reset env e in place, the single env has not)
                got = infos[e]['terminal_observation']
                live.remove(e)
            assert np.array_equal(got.view(np.int64), np.asarray(o1).reshape(-1).view(np.int64)), (k, e)
            if not done[e]:
                for nme in ("x_true", "x_filter", "P_filter"):
                    u, v = getattr(vec, nme)(e), getattr(singles[e], nme)[k]
                    assert np.array_equal(u.view(np.int64), np.asarray(v).view(np.int64)), (k, e, nme)
        print(mode, reward, "step", k, "live envs", live)
    assert live, "every env ended early: nothing compared over the ten steps"
    torch.cuda.synchronize()


def test_vector_env_runs_through_done_and_auto_reset(envs):
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    vec = SSA_Tasker_VecEnv(_vec_cfg(envs), 3, seed=10)
    rs = np.random.RandomState(5)
    for k in range(1, 11):
        _, _, done, _ = vec.step(np.stack([rs.permutation(8)[:3] for _ in range(3)]))
        assert not done.any()
    obs, rew, done, infos = vec.step(np.array([[0, 1, 2], [1, 2, 3], [2, 3, 4]]))      # step 11 = n - 1: done for every env, auto-reset
    assert done.all() and all('terminal_observation' in i for i in infos)
    assert all(not np.array_equal(infos[e]['terminal_observation'], obs[e]) for e in range(3))
    assert np.all(vec.i == 0)
    obs2, _, done2, _ = vec.step(np.array([[1, 2, 3], [2, 3, 4], [3, 4, 5]]))
    assert not done2.any() and np.all(vec.i == 1) and np.isfinite(obs2).all()
    with pytest.raises(AssertionError):
        vec.step(np.array([[1, 2, 8], [2, 3, 4], [3, 4, 5]]))
    with pytest.raises(ValueError):
        vec.step(np.array([[1, 2, 3], [2, 3, 2], [3, 4, 5]]))
    assert np.all(vec.i == 1)                                     # (refused before anything was launched or counted)


@pytest.mark.parametrize("mode,reward", [("flatten", "trinary"), ("aer", "shaped")])
def test_vector_env_pinned_copy_path_equals_by_value_and_obs_device(envs, mode, reward):
    """E = 9 (rows through the device table, times through the pinned copy) equals E = 8 (by value) on the shared envs until the first
    reset; obs_device=True equals the host form"""
    import torch
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    cfg = _vec_cfg(envs, obs_returned=mode, reward_type=reward)
    a = SSA_Tasker_VecEnv(cfg, 8, seed=20)
    b = SSA_Tasker_VecEnv(cfg, 9, seed=20)
    c = SSA_Tasker_VecEnv(dict(cfg, obs_device=True), 8, seed=20)
    assert a._inline and not b._inline and c._inline
    b._eng.z_noise[:8].copy_(a._eng.z_noise)                      # (b draws for 9 envs from one generator: the shared envs take a's draws)
    rs = np.random.RandomState(6)
    for k in range(1, 11):
        acts = np.stack([rs.permutation(8)[:3] for _ in range(9)])
        oa, ra, da, _ = a.step(acts[:8])
        ob, rb, db, _ = b.step(acts)
        oc, rc, dc, _ = c.step(acts[:8])
        assert isinstance(oc, torch.Tensor) and oc.is_cuda
        assert np.array_equal(oa, oc.cpu().numpy()) and np.array_equal(ra, rc) and np.array_equal(da, dc), k
        assert np.array_equal(oa, ob[:8]) and np.array_equal(ra, rb[:8]) and np.array_equal(da, db[:8]), k
        if da.any():      # (b draws its reset noise for 9 envs from one generator: after a reset the streams differ)
            break
    assert k >= 3


def test_vector_env_without_observers_is_unchanged(envs):
    """a config without config['observers'] at (E, m) = (3, 8): ten steps' observations and rewards as recorded from the parent commit
    (tests/golden/vector_env_plain_m8_e3.npz; DESIGN.md section 8i says how)"""
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    want = golden("vector_env_plain_m8_e3.npz")
    for i, (mode, reward) in enumerate([("flatten", "trinary"), ("aer", "shaped")]):
        cfg = dict(envs.env_config)
        cfg.update(rso_count=8, steps=12, reward_type=reward, obs_returned=mode)
        vec = SSA_Tasker_VecEnv(cfg, 3, seed=10)
        for k in range(1, 11):
            obs, rew, done, _ = vec.step([(k + e) % 8 for e in range(3)])
            assert np.array_equal(obs.view(np.int64), want["obs%d" % i][k - 1].view(np.int64)), (mode, k)
            assert np.array_equal(rew, want["rew%d" % i][k - 1]) and np.array_equal(done, want["done%d" % i][k - 1]), (mode, k)
