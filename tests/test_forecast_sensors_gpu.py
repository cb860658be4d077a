"""A sensor network's H-step tasking forecast in one launch (include/ssa_hip.h: ssa_forecast_sensors_f64;
HotPathEngine.launch_forecast_sensors; SSA_Tasker_Env.forecast_sensors; agents.plan_info_gain_sensors / plan_trace_gain_sensors) on the
MI355X.

The yardstick is the forecast's definition in terms of launches this feature leaves untouched: slab h is what the sensor network's
lookahead (launch_lookahead_sensors) writes after h all-idle sensor steps (launch_step_sensors).  Everything is compared bit for bit;
there is no tolerance anywhere."""
import numpy as np
import pytest

from support.batches import c2t, make_batch
from support.gpu import envs, hip  # noqa: F401  (the module fixtures)
from support.sensors import BAD as BAD_AT, N_TIME, _assert_same_env, _distinct, cfg8, sites_rad

pytestmark = pytest.mark.gpu

MASKS_DEG = [15.0, 0.0, 30.0, 5.0, 20.0, -10.0, 10.0, 25.0]
FAILED_AT = 21        # the object whose filter had failed before the launch (BAD's state is NaN: it fails in the first predict)
KEYS = ("score", "status", "visible", "x_prior", "P_prior", "P_post")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _np(r):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in r.items()}


def _state(hip, eng):
    """every tensor the engine holds (device and host-mapped), as bytes"""
    hip.torch.cuda.synchronize()
    return {k: v.detach().cpu().contiguous().numpy().tobytes() for k, v in vars(eng).items() if isinstance(v, hip.torch.Tensor)}


def _engine_case(hip, m, H, S, propagator="hybrid", obs_type="aer", interval=1, layout=False):
    """the forecast from a prepared state against its definition on the same engine, and the engine's state around the forecast;
    returns the yardstick's slabs"""
    torch, L, host = hip.torch, hip.lib, hip.host
    xt, x, P, g = make_batch(m, seed=123)
    BAD, FAILED = BAD_AT % m, FAILED_AT % m     # (folded into a batch smaller than that)
    x[BAD, 1] = np.nan
    lla, lim = sites_rad()[:S], np.radians(MASKS_DEG[:S])
    if obs_type == "aer":
        sig = [np.array([(1.0 + k) * host.arcsec2rad, (0.5 + 2.0 * k) * host.arcsec2rad, 1e3 / (1 + k)]) for k in range(S)]
    else:
        sig = [np.array([5e2 / (1 + 0.25 * k)] * 3) for k in range(S)]
    Rs = [np.diag(s ** 2) for s in sig]
    sp = host.make_sensor_params(lla, lim, Rs, N_TIME * m * 3)
    consts = host.make_consts(g["Q"], Rs[0], 1e-4, 2.0, -3, 20.0, lim[0], lla[0], propagator=propagator, obs_type=obs_type,
                              update_interval=interval)
    zn = torch.zeros((S, N_TIME, m, 3), dtype=torch.float64, device="cuda")      # (never read: no sensor observes anything here)
    eng = hip.engine.HotPathEngine(consts, m, 1, c2t()[:N_TIME], zn, history=2, zn_stride_env=0)
    pos = np.arange(m)
    if layout:
        from ssa_gym_amd.catalogue import regime_order
        order = regime_order(xt)
        eng.set_layout(order)
        pos = np.argsort(order)
    eng.load_state(0, xt, x, P)
    eng.status[int(pos[FAILED])] = L.ST_UPDATE_NAN
    # ---- the forecast, every optional output on, and the engine's state around it
    before = _state(hip, eng)
    fc = _np(eng.launch_forecast_sensors(0, 1, sp, H, out=hip.engine.HotPathEngine.LOOKAHEAD_PARTS))
    after = _state(hip, eng)
    assert before.keys() == after.keys() and {"status", "stats", "fail_count", "fail_log_host", "x_filter", "upd", "_shard_sets"} <= before.keys()
    for k in before:
        assert before[k] == after[k], "the forecast wrote the engine's %s" % k
    assert fc["score"].shape == (H, S, m, 3) and fc["status"].shape == fc["visible"].shape == (H, S, m)
    assert fc["x_prior"].shape == (H, m, 6) and fc["P_prior"].shape == (H, m, 6, 6) and fc["P_post"].shape == (H, S, m, 6, 6)
    # ---- the definition: the lookahead after h all-idle steps, on the same engine
    yard = []
    for h in range(H):
        yard.append(_np(eng.launch_lookahead_sensors(h % 2, 1 + h, sp, out=hip.engine.HotPathEngine.LOOKAHEAD_PARTS)))
        eng.launch_step_sensors(h % 2, (h + 1) % 2, 1 + h, sp, [-1] * S, 0, fast_stats=True)
    torch.cuda.synchronize()
    for h in range(H):
        for key in KEYS:
            bad = _bits(fc[key][h]) != _bits(yard[h][key])
            print("[forecast m=%d H=%d S=%d %s/%s i=%d] h=%d %s: %d of %d words differ"
                  % (m, H, S, propagator, obs_type, interval, h, key, int(bad.sum()), bad.size))
            assert not bad.any(), (h, key, np.argwhere(bad)[:4])
    # ---- what the start state was prepared to hold, found in the YARDSTICK's outputs
    st = np.stack([y["status"] for y in yard])                  # [H, S, m]
    vis = np.stack([y["visible"] for y in yard]).astype(bool)
    xp = np.stack([y["x_prior"] for y in yard])
    Pp = np.stack([y["P_prior"] for y in yard])
    upd = np.array([interval <= 1 or (1 + h) % interval == 0 for h in range(H)])
    # a filter already failed at entry: its code and its input slot, at every step
    assert (st[:, :, FAILED] == L.ST_UPDATE_NAN).all() and not vis[:, :, FAILED].any()
    assert all(np.array_equal(_bits(xp[h, FAILED]), _bits(x[FAILED])) and np.array_equal(_bits(Pp[h, FAILED]), _bits(P[FAILED]))
               for h in range(H))
    # a NaN filter that fails at h = 0; the sentinel pass-through from h = 1 on
    assert (st[:, :, BAD] == L.ST_PREDICT_NAN).all() and not vis[:, :, BAD].any()
    sent = np.array([1e20] * 3 + [1e12] * 3)
    assert all(np.array_equal(xp[h, BAD], sent) and np.array_equal(Pp[h, BAD], np.diag(sent)) for h in range(H))
    healthy = (st == L.ST_OK).all(axis=(0, 1))
    if m <= FAILED_AT:     # (a handful of objects: a tile's shape is the case, the sky's situations are the larger batches')
        return fc
    # an object hidden from one site and visible from another, at a step that updates
    cross = [(h, s0, s1) for h in np.flatnonzero(upd) for s0 in range(S) for s1 in range(S)
             if (~vis[h, s0] & vis[h, s1] & healthy).any()]
    assert cross, "no object hidden from one site and visible from another"
    # an (s, j) whose visibility changes inside the horizon (between two steps that update)
    vu = vis[upd][:, :, healthy]
    changes = int((vu.any(axis=0) & ~vu.all(axis=0)).sum())
    print("[forecast m=%d H=%d S=%d] visible per step %s, (s, j) whose visibility changes: %d" % (m, H, S, vis.sum(axis=(1, 2)).tolist(), changes))
    assert changes >= 1, "no (s, j) whose visibility changes inside the horizon"
    # skipped steps (update_interval): no update is attempted, P_post is the prior for every sensor
    for h in np.flatnonzero(~upd):
        assert not vis[h].any() and np.isnan(yard[h]["score"]).all()
        assert all(np.array_equal(_bits(yard[h]["P_post"][s]), _bits(yard[h]["P_prior"])) for s in range(S))
    assert vis[upd].any() and np.isfinite(fc["score"][upd]).any()
    return fc


@pytest.mark.parametrize("m,H,S", [(403, 9, 3), (2003, 5, 8), (30001, 3, 2), (7, 4, 3)])
def test_forecast_equals_its_definition_hybrid(hip, m, H, S):
    """a partial last tile; eight sites; more than 20 480 objects (several tiles per wavefront); one whole tile and a partial one"""
    _engine_case(hip, m, H, S)


@pytest.mark.parametrize("variant", ["fg", "j2", "elements", "xyz"])
def test_forecast_equals_its_definition_for_the_other_propagators_and_xyz(hip, variant):
    if variant == "xyz":
        _engine_case(hip, 403, 4, 3, obs_type="xyz")
    else:
        _engine_case(hip, 403, 4, 3, propagator=variant)


def test_forecast_over_update_steps_and_skipped_steps(hip):
    """update_interval = 3 over seven steps: time indices 3 and 6 update, the others are skipped"""
    _engine_case(hip, 403, 7, 3, interval=3)


def test_forecast_under_the_regime_layout(hip):
    """the rows of every output are the caller's, whatever order the engine stores the objects in"""
    a = _engine_case(hip, 2000, 4, 3, layout=True)
    b = _engine_case(hip, 2000, 4, 3)
    for key in KEYS:
        assert np.array_equal(_bits(a[key]), _bits(b[key])), key


def test_no_side_effects_on_an_episode(envs):
    """60 steps with forecast_sensors() before every step and the same episode without: everything step() leaves, bit for bit"""
    cfg = cfg8(envs, m=403, seed=21, steps=70)
    a, b = envs.make('ssa_tasker_simple-v2', config=cfg), envs.make('ssa_tasker_simple-v2', config=cfg)
    rs = np.random.RandomState(4)
    for k in range(60):
        acts = _distinct(rs, a.m, 3)
        r = a.forecast_sensors(1 + k % 5, covariances=bool(k % 2))
        assert r["score"].shape == (1 + k % 5, 3, 403, 3)
        oa, ob = a.step(acts), b.step(acts)
        assert np.array_equal(oa[0], ob[0]) and np.array_equal(oa[1], ob[1], equal_nan=True)
    _assert_same_env(a, b, "forecast before every step")
    assert np.array_equal(a._engine.fail_log, b._engine.fail_log)
    # the horizon is cut at the episode's end; past it there is nothing to forecast
    for _ in range(7):
        a.step(_distinct(rs, a.m, 3))
    assert a.i == 67 and a.forecast_sensors(10)["status"].shape == (2, 3, 403)
    for _ in range(2):
        a.step(_distinct(rs, a.m, 3))
    with pytest.raises(ValueError):
        a.forecast_sensors(3)


def test_one_sensor_slab_0_equals_the_existing_lookahead(envs):
    """S = 1 -- an env without observers and a one-site network: slab 0 is env.lookahead() bit for bit"""
    base = cfg8(envs, m=403, sensors=0)
    one = dict(base, observers=[tuple(base['observer'])])
    for cfg in (base, one):
        env = envs.make('ssa_tasker_simple-v2', config=cfg)
        assert env.n_sensor == 1
        rs = np.random.RandomState(2)
        for k in range(3):
            for _ in range(1 + 40 * k):
                env.step(int(rs.randint(env.m)))
            ref, fc = _np(env.lookahead(covariances=True)), _np(env.forecast_sensors(3, covariances=True))
            assert fc["score"].shape == (3, 1, 403, 3)
            assert np.array_equal(_bits(fc["score"][0, 0]), _bits(ref["score"].T))
            for key in ("status", "visible"):
                assert np.array_equal(fc[key][0, 0], ref[key]), key
            assert np.array_equal(_bits(fc["P_post"][0, 0]), _bits(ref["P_post"]))
            for key in ("x_prior", "P_prior"):
                assert np.array_equal(_bits(fc[key][0]), _bits(ref[key])), key


def _greedy_np(score):
    """global greedy over [S, m]: the largest non-NaN entry (ties: the lowest s * m + j), its row and column removed, repeated"""
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


def _plan_np(score):
    """the planner's rule on a read-back forecast column [H', S, m]: step by step the greedy assignment, without the objects planned
    at an earlier step"""
    Hp, S, m = score.shape
    planned = np.zeros(m, bool)
    plan = np.full((Hp, S), -1)
    for h in range(Hp):
        sc = np.array(score[h])
        sc[:, planned] = np.nan
        plan[h] = _greedy_np(sc)
        planned[plan[h][plan[h] >= 0]] = True
    return plan


def test_forecast_against_execution(envs):
    """the plan executed: every planned update that was taken leaves the forecast's P_post, and every planned (h, s, j) the forecast's
    visibility -- an object's trajectory depends on no other object, and the plan observes each object once"""
    from ssa_gym_amd import _lib, agents
    env = envs.make('ssa_tasker_simple-v2', config=cfg8(envs, m=403, seed=5, history='full'))
    env.action_space.seed(3)
    rs = np.random.RandomState(6)
    for _ in range(2):
        env.step(_distinct(rs, env.m, 3))
    i = env.i
    fc = _np(env.forecast_sensors(6, covariances=True))
    raw = agents._plan_assigned(env, 6, _lib.LOOK_INFO_GAIN)
    plan = agents._fill_plan(env, raw)
    assert plan.shape == (6, 3) and np.array_equal(raw, _plan_np(fc["score"][..., _lib.LOOK_INFO_GAIN]))
    env.rollout_sensors(plan)
    assert env.i == i + 6
    e = env._engine
    recs = e.upd_sensors.cpu().numpy()
    status = e.status.cpu().numpy()
    taken = 0
    for h in range(6):
        for s in range(3):
            j, rec = int(plan[h, s]), recs[(i + h + 1) % e.H, s]
            if raw[h, s] < 0:                                        # (a fill-in: nothing the sensor could have observed)
                assert not env.obs_taken[i + h + 1, s], (h, s, j)
                continue
            assert rec[_lib.UPD_ACTION] == j and fc["status"][h, s, j] == _lib.ST_OK and fc["visible"][h, s, j] == 1, (h, s, j)
            assert rec[_lib.UPD_VISIBLE] == 1.0 and env.obs_taken[i + h + 1, s], (h, s, j)
            if status[j] == _lib.ST_UPDATE_NAN:                      # (depends on the drawn noise: not foreseen)
                continue
            assert np.array_equal(_bits(env.P_filter[i + h + 1][j]), _bits(fc["P_post"][h, s, j])), (h, s, j)
            taken += 1
    print("[forecast vs execution] %d planned updates taken and compared" % taken)
    assert taken >= 6                                                # (a third of the plan's 18 entries)
    # the booked visibility of every (h, s, j) the plan attempted, fill-ins included
    for h in range(6):
        for s in range(3):
            rec = recs[(i + h + 1) % e.H, s]
            if rec[_lib.UPD_ACTION] >= 0:
                assert fc["visible"][h, s, int(plan[h, s])] == int(rec[_lib.UPD_VISIBLE]), (h, s)


@pytest.mark.parametrize("case", ["network", "blind_sensor", "small_pool", "one_site"])
def test_planners_follow_the_rule(envs, case):
    from ssa_gym_amd import _lib, agents
    over = dict(network=dict(m=403), blind_sensor=dict(m=403, sensor_obs_limit=[15, 10, 90]), small_pool=dict(m=10),
                one_site=dict(m=403, sensors=0))[case]
    env = envs.make('ssa_tasker_simple-v2', config=cfg8(envs, seed=7, **over))
    env.action_space.seed(1)
    S = env.n_sensor
    rs = np.random.RandomState(8)
    for _ in range(2):
        env.step(_distinct(rs, env.m, S) if S > 1 else int(rs.randint(env.m)))
    draws = env.np_random.get_state()[2]
    fc = _np(env.forecast_sensors(6))
    if case == "blind_sensor":
        assert np.isnan(fc["score"][:, 2]).all() and not fc["visible"][:, 2].any()
    for planner, col in ((agents.plan_info_gain_sensors, _lib.LOOK_INFO_GAIN), (agents.plan_trace_gain_sensors, _lib.LOOK_TRACE_GAIN)):
        want = _plan_np(fc["score"][..., col])
        raw = agents._plan_assigned(env, 6, col)
        assert np.array_equal(raw, want), (case, raw, want)
        got = raw[raw >= 0]
        assert len(set(got.tolist())) == len(got)                    # no object twice in a plan
        plan = planner(env, 6)
        assert plan.dtype == np.int64 and plan.shape == (6, S)
        assert np.array_equal(plan[want >= 0], want[want >= 0])
        assert ((plan >= 0) & (plan < env.m)).all() and all(len(set(r.tolist())) == S for r in plan)
        if case == "blind_sensor":
            assert (want[:, 2] == -1).all()
        if case == "small_pool":
            assert (want == -1).any()                                # (18 entries, 10 objects)
    assert env.np_random.get_state()[2] == draws                     # (the env's noise stream is not touched)
    i = env.i
    env.rollout_sensors(plan)
    assert env.i == i + 6
