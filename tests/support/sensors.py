"""Sensor networks: the site lists, env configs and bare env of the host and GPU tests, the relaunch harness of the step, and the
bit-for-bit comparisons of two engines / two envs."""
import ctypes as C

import numpy as np

SITES3 = [(38.8, -104.5, 1800.0), (28.4, -80.6, 3.0), (-31.9, 115.9, 20.0)]
SITES8_NETWORK = SITES3 + [(51.5, -0.1, 50.0), (35.7, 139.7, 40.0), (-33.9, 18.4, 10.0), (64.8, -147.7, 150.0), (19.8, -155.5, 4200.0)]
# (lat [deg], lon [deg], h [m]): the default observer, south-east, high altitude, the antimeridian, far north, far south, a pole, (0, 0)
SITES8_GEOMETRY = [(38.828198, -77.305352, 20.0), (-31.9, 115.9, 20.0), (19.8, -155.5, 4200.0), (-17.7, 179.95, 5.0),
                   (78.2, 15.6, 500.0), (-77.8, 166.7, 200.0), (89.9995, 45.0, 10.0), (0.0, 0.0, 0.0)]


def sites_rad(sites=SITES8_GEOMETRY):
    return [np.array([np.radians(la), np.radians(lo), h]) for la, lo, h in sites]


def cfg3(E, m=2000, sensors=3, **over):
    cfg = dict(E.env_config)
    cfg.update(rso_count=m, steps=480, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3)
    if sensors:
        cfg.update(observers=SITES3[:sensors], sensor_obs_limit=[15, 10, 20][:sensors],
                   sensor_z_sigma=[(1, 1, 1e3), (2, 2, 5e2), (0.5, 0.5, 2e3)][:sensors])
    cfg.update(over)
    return cfg


def cfg8(E, m=2000, sensors=3, **over):
    cfg = dict(E.env_config)
    cfg.update(rso_count=m, steps=480, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3)
    if sensors:
        cfg.update(observers=SITES8_NETWORK[:sensors], sensor_obs_limit=[15, 10, 20, 12, 18, 8, 25, 15][:sensors],
                   sensor_z_sigma=[(1 + 0.5 * k, 1 + 0.5 * k, 1e3 / (1 + k)) for k in range(sensors)])
    cfg.update(over)
    return cfg


def xyz_net():
    from ssa_gym_amd.envs import dynamics as D
    return dict(obs_type='xyz', z_sigma=(5e2,) * 3, R=np.diag([5e2 ** 2] * 3), hx=D.hx_xyz, mean_z=D.mean_xyz, residual_z=np.subtract,
                sensor_z_sigma=[(5e2,) * 3, (3e2,) * 3, (8e2,) * 3])


def _bits(t):
    return t.contiguous().view(__import__("torch").int64).cpu().numpy()


def _distinct(rs, m, S):
    return rs.permutation(m)[:S]


def _advance(env, rs, k):
    for _ in range(k):
        env.step(_distinct(rs, env.m, env.n_sensor) if env.n_sensor > 1 else int(rs.randint(env.m)))


class _Relaunch:
    """launches of the step from the env's current state (slot i -> slot i + 1), each from the same status words and failure counter"""

    def __init__(self, env):
        import torch
        self.env, self.e = env, env._engine
        torch.cuda.synchronize()
        self.st0, self.fc0 = self.e.status.clone(), self.e.fail_count.clone()
        self.upd = torch.zeros((env.n_sensor, 64), dtype=torch.float64, device="cuda")

    def _out(self):
        import torch
        torch.cuda.synchronize()
        e, sl = self.e, (self.env.i + 1) % self.e.H
        out = dict(x=_bits(e.x_filter[sl]), P=_bits(e.P_filter[sl]).reshape(-1, 36), xt=_bits(e.x_true[sl]), st=e.status.cpu().numpy().copy(),
                   upd=self.upd.cpu().numpy().copy())
        e.status.copy_(self.st0)
        e.fail_count.copy_(self.fc0)
        return out

    def sensors(self, acts, sp=None):
        env, e, i = self.env, self.e, self.env.i
        self.upd.zero_()
        e.launch_step_sensors(i % e.H, (i + 1) % e.H, i + 1, env._sensors if sp is None else sp, list(acts), self.upd.data_ptr(),
                              fast_stats=True, fold_inside=True)
        return self._out()

    def single(self, s, act):
        """the plain step with sensor s's site, mask and R (its kernel constants) and its noise table"""
        env, e, i = self.env, self.e, self.env.i
        self.upd.zero_()
        z0, c0, r0 = e._p.z_noise, e.consts, e._cref
        try:
            e._p.z_noise = e.z_noise.data_ptr() + s * int(env._sensors.zn_stride_sensor) * 8 if env.n_sensor > 1 else z0
            e._pcache.clear()
            e.consts = env._sensor_consts[s]
            e._cref = C.byref(e.consts)
            e.launch_step(i % e.H, (i + 1) % e.H, i + 1, action=int(act), upd_out=self.upd.data_ptr(), fast_stats=True, fold_inside=True)
            return self._out()
        finally:
            e._p.z_noise, e.consts, e._cref = z0, c0, r0
            e._pcache.clear()


def _bare_env(S, m=10, n=6, seed=5):
    """an env object without device state (what a machine without a GPU has), with just what the host-side paths read"""
    from ssa_gym_amd import host
    from ssa_gym_amd.envs._gymshim import np_random, spaces
    from ssa_gym_amd.envs.ssa_tasker_simple_2 import SSA_Tasker_Env
    env = SSA_Tasker_Env.__new__(SSA_Tasker_Env)
    env._engine, env.i, env.n, env.m, env.n_sensor = None, 0, n, m, S
    env.z_sigma = np.array([1.0, 1.0, 1e3]) * [host.arcsec2rad, host.arcsec2rad, 1]
    env.sensor_z_sigma = np.stack([env.z_sigma * (k + 1) for k in range(S)])
    env.np_random, _ = np_random(seed)
    env.action_space = spaces.MultiDiscrete([m] * S) if S > 1 else spaces.Discrete(m)
    return env


N_TIME = 16           # rows of the GCRS -> ITRS table and of the noise tables the engine tests use (time indices stay below it)
BAD = 9               # the object whose filter state is NaN: it fails in the first step's predict


def _defined_fields(L, u):
    """an update record defines its flags always, z_true when the update was attempted (the action word is the object), y / S / sigmas_h
    when the observation was taken; the other words of a slot are leftovers of whatever used it before"""
    u = u.copy()
    att, taken = u[..., L.UPD_ACTION] >= 0, u[..., L.UPD_OBS_TAKEN] == 1.0
    keep = np.zeros(u.shape, dtype=bool)
    keep[..., [L.UPD_OBS_TAKEN, L.UPD_VISIBLE, L.UPD_ACTION]] = True
    keep[..., L.UPD_Z_TRUE:L.UPD_Z_TRUE + 3] = att[..., None]
    keep[..., L.UPD_Y:L.UPD_SIGMAS_H + 39] = taken[..., None]
    u[~keep] = 0.0
    return u


def _compare(L, a, b, K, H, argmax):
    for nme in ("x_true", "x_filter", "P_filter", "obs", "metrics", "status"):
        u, v = a[nme], b[nme]
        if nme == "metrics" or u.ndim == 1 or K >= H:
            assert np.array_equal(u, v, equal_nan=True), nme
        else:   # slots never written keep their initial fill
            sl = [s_ % H for s_ in range(0, K + 1)]
            assert np.array_equal(u[sl], v[sl], equal_nan=True), nme
    words = [L.STAT_MAX_DPOS, L.STAT_CNT_LT_1E4, L.STAT_CNT_LT_1E7, L.STAT_N_FAILED] + ([L.STAT_ARGMAX_SPOS, L.STAT_MAX_SPOS] if argmax else [])
    ua, ub = _defined_fields(L, a["upd"]), _defined_fields(L, b["upd"])
    for k in range(max(0, K - H), K):                     # statistics and records of the steps whose slot survives
        so = (k + 1) % H
        for w in words:
            assert np.array_equal(a["stats"][so, :, w], b["stats"][so, :, w], equal_nan=True), (k, w)
        assert np.array_equal(ua[so], ub[so], equal_nan=True), ("upd", k)
    # the failure log: the same records (the order in which concurrent wavefronts append is not defined on either path)
    assert a["fail_count"] == b["fail_count"]
    key = lambda r: tuple(np.nan_to_num(r, nan=-1.0))      # noqa: E731
    assert np.array_equal(np.array(sorted(a["fail_log"].tolist(), key=key)), np.array(sorted(b["fail_log"].tolist(), key=key)), equal_nan=True)
    assert not b["shards"].any()                           # every per-step shard set of the rollout is folded and cleared


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _assert_same_env(a, b, what):
    """everything step() leaves: the device state (bit for bit) and every host-side history"""
    import torch
    from ssa_gym_amd import _lib
    torch.cuda.synchronize()
    assert a.i == b.i, what
    for name in ("x_true", "x_filter", "P_filter", "obs", "metrics", "status"):
        u, v = getattr(a._engine, name), getattr(b._engine, name)
        if name != "status":
            u, v = u.view(torch.int64), v.view(torch.int64)
        assert torch.equal(u, v), (what, name)
    for name in ("actions", "obs_taken", "sigmas_h", "S", "rewards", "_y", "_z_true", "_S_sel", "_upd_action"):
        u, v = getattr(a, name), getattr(b, name)
        assert (u is None and v is None) or _same(u, v), (what, name)
    # failures: the same filters, dated to the same steps, with the same messages.  (Filters that fail in ONE step are listed in the order
    # their wavefronts reached the failure log, which no path defines -- two step() twins differ there too: the ids are compared step by step.)
    def by_step(env):
        return sorted((env.failed_filters_msg._rec[j][0], j) for j in env.failed_filters_id)
    assert len(a.failed_filters_id) == len(set(a.failed_filters_id)) == len(b.failed_filters_id) and by_step(a) == by_step(b), what
    assert [env.failed_filters_msg._rec[j][0] for env in (a, b) for j in env.failed_filters_id] == \
        sorted(env.failed_filters_msg._rec[j][0] for env in (a,) for j in env.failed_filters_id) * 2, what      # (in step order, both)
    assert list(a.failed_filters_msg) == list(b.failed_filters_msg), what
    assert a._n_failed == b._n_failed and a._argmax_sigma == b._argmax_sigma, (what, a._argmax_sigma, b._argmax_sigma)
    words = [_lib.STAT_MAX_DPOS, _lib.STAT_CNT_LT_1E4, _lib.STAT_CNT_LT_1E7, _lib.STAT_N_FAILED]
    assert _same(a._stats[words], b._stats[words]), what
