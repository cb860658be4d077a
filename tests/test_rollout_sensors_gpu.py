"""A sensor network's K-step tasking schedule in one launch (include/ssa_hip.h: ssa_env_rollout_sensors_f64;
HotPathEngine.launch_rollout_sensors; SSA_Tasker_Env.rollout_sensors) on the MI355X.

The yardstick is the project's own per-step path, which this feature leaves untouched: K launches of the sensor step
(launch_step_sensors / step()) from the same state.  Everything is compared bit for bit; there is no tolerance anywhere."""
import numpy as np
import pytest

from support.batches import c2t, make_batch
from support.gpu import envs, hip  # noqa: F401  (the module fixtures)
from support.sensors import BAD, N_TIME, _assert_same_env, _compare, _distinct, _same, cfg3, sites_rad

pytestmark = pytest.mark.gpu

MASKS_DEG = [15.0, -90.0, 30.0, 0.0, 5.0, -10.0, 20.0, -30.0]
ALL_ITEMS = {"tile", "idle", "dup", "oor", "cross", "failed", "taken"}


def _net(host, S, obs_type, stride):
    """S sites with distinct elevation masks and R (and per-sensor noise sigmas for the tables)"""
    lla = sites_rad()[:S]
    lim = np.radians(MASKS_DEG[:S])
    if obs_type == "aer":
        sig = [np.array([(1.0 + k) * host.arcsec2rad, (0.5 + 2.0 * k) * host.arcsec2rad, 1e3 / (1 + k)]) for k in range(S)]
    else:
        sig = [np.array([5e2 / (1 + 0.25 * k)] * 3) for k in range(S)]
    Rs = [np.diag(s ** 2) for s in sig]
    return lla, lim, Rs, sig, host.make_sensor_params(lla, lim, Rs, stride)


def _build_schedule(rs, m, S, K, H, interval, vis, order=None):
    """a schedule [K, S] that holds, as far as S sensors allow it: two or three tasked objects in one tile, an idle sensor, a duplicate,
    an out-of-range action, an object below its sensor's mask but above another's, the failed filter tasked after it failed, and -- in
    the last update step, whose records survive -- for every sensor an object it sees.  vis[k][s]: bool [m], the visibility of the
    objects (caller's indices) from sensor s at step k.  order: storage position -> the caller's index (a storage layout).
    Returns the schedule and the items it was built to contain."""
    pos2id = np.arange(m) if order is None else np.asarray(order)
    FREE = -2
    sched = np.full((K, S), FREE, dtype=np.int64)
    upd_rows = [k for k in range(K) if (1 + k) % interval == 0]
    vis_row = [k for k in upd_rows if k >= K - H][-1]
    others = [k for k in upd_rows if k != vis_row] + [k for k in range(K) if k not in upd_rows]
    used, planned, todo = {BAD}, set(), ["tile", "cross", "dup", "idle", "oor", "failed"]
    perm = [int(j) for j in rs.permutation(m)]

    def fresh(ok=lambda j: True):
        for j in perm:
            if j not in used and ok(j):
                used.add(j)
                return j
        return None
    bad_tile = int(np.where(pos2id == BAD)[0][0]) // 4
    for k in others:
        for item in list(todo):
            free = [s for s in range(S) if sched[k, s] == FREE]
            if item == "tile" and len(free) >= 2:
                n = min(3, len(free))
                for tb in rs.permutation((m - 4) // 4):
                    ids = [int(pos2id[4 * tb + q]) for q in range(n)]
                    if tb != bad_tile and not used.intersection(ids):
                        break
                used.update(ids)
                sched[k, free[:n]] = ids
            elif item == "cross" and S >= 2 and free:
                hit = None
                for s0 in free:
                    seen_else = np.any([vis[k][s1] for s1 in range(S) if s1 != s0], axis=0)
                    j = fresh(lambda j: not vis[k][s0][j] and seen_else[j])
                    if j is not None:
                        hit = (s0, j)
                        break
                if hit is None:
                    continue
                sched[k, hit[0]] = hit[1]
            elif item == "dup" and len(free) >= 2:
                sched[k, free[:2]] = fresh()
            elif item in ("idle", "oor") and free:
                sched[k, free[0]] = -1 if item == "idle" else m + 3
            elif item == "failed" and free and k >= 1:
                sched[k, free[0]] = BAD
            else:
                continue
            todo.remove(item)
            planned.add(item)
    for s in range(S):
        j = fresh(lambda j: vis[vis_row][s][j])
        assert j is not None, "no object visible from sensor %d at step %d" % (s, vis_row + 1)
        sched[vis_row, s] = j
    planned.add("taken")
    for k in range(K):
        for s in range(S):
            if sched[k, s] == FREE:
                sched[k, s] = fresh()
    return sched, planned


def _assert_schedule_seen(L, m, S, K, H, interval, sched, planned, vis, order, yard):
    """the conditions the schedule was built for, found again in the schedule, the visibility tables and the YARDSTICK's outputs"""
    id2pos = np.arange(m) if order is None else np.argsort(np.asarray(order))
    inr = (sched >= 0) & (sched < m)
    seen = set()
    for k in range(K):
        row, ok = sched[k], inr[k]
        tiles = [int(id2pos[a]) // 4 for a in set(row[ok])]
        if max([tiles.count(t) for t in tiles] + [0]) >= 2:
            seen.add("tile")
        if len(set(row[ok])) < len(row[ok]):
            seen.add("dup")
        for s in range(S):
            a = int(row[s])
            if ok[s] and a != BAD and not vis[k][s][a] and any(vis[k][s1][a] for s1 in range(S) if s1 != s):
                seen.add("cross")
                if k >= K - H and (1 + k) % interval == 0 and a not in row[:s] and yard["status"][id2pos[a]] == 0:
                    # (the yardstick attempted it and did not see it)
                    rec = yard["upd"][(k + 1) % H, s]
                    assert rec[L.UPD_ACTION] == a and rec[L.UPD_VISIBLE] == 0 and rec[L.UPD_OBS_TAKEN] == 0, (k, s, rec[:8])
    if (sched == -1).any():
        seen.add("idle")
    if (sched >= m).any():
        seen.add("oor")
    # the failed filter: failed in step 1 (its record says so), tasked in a later step
    log = yard["fail_log"][:int(yard["fail_count"])]
    first = [r for r in log if int(r[L.FAIL_OBJ]) == BAD]
    assert len(first) == 1 and first[0][L.FAIL_TIME] == 1 and yard["status"][id2pos[BAD]] != 0
    if (sched[1:] == BAD).any():
        seen.add("failed")
    surviving = [k for k in range(max(0, K - H), K)]
    if all(any(yard["upd"][(k + 1) % H, s, L.UPD_OBS_TAKEN] == 1.0 for k in surviving) for s in range(S)):
        seen.add("taken")
    assert seen >= planned, (planned - seen)
    assert planned == (ALL_ITEMS if S >= 3 else {"idle", "oor", "failed", "taken"}), planned


def _visibility(hip, consts_of, xt, x, P, m, K, trans, zn, sp):
    """vis[k][s] for the steps 1 .. K: the truth does not depend on the tasking, so K idle steps give it"""
    eng = hip.engine.HotPathEngine(consts_of[0], m, 1, trans, zn, history=K + 1, zn_stride_env=0)
    eng.load_state(0, xt, x, P)
    for k in range(K):
        eng.launch_step_sensors(k, k + 1, 1 + k, sp, [-1] * int(sp.n_sensor), 0, fast_stats=True)
    hip.torch.cuda.synchronize()
    vis = []
    for k in range(K):
        M = eng.trans[(1 + k) % eng.n_time].reshape(3, 3)
        vis.append([hip.dev.visible_mask(eng.x_true[k + 1], M, c).cpu().numpy().astype(bool) for c in consts_of])
    return vis


def _run_both(hip, consts, m, K, H, xt, x, P, trans, zn, sp, sched, argmax, layout=None):
    """the K steps by K launches of the sensor step (the yardstick) and by one launch of the rollout, from the same state"""
    torch, L = hip.torch, hip.lib
    S = int(sp.n_sensor)
    outs = []
    for mode in ("steps", "rollout"):
        eng = hip.engine.HotPathEngine(consts, m, 1, trans, zn, history=H, zn_stride_env=0)
        if layout is not None:
            eng.set_layout(layout)
        eng.load_state(0, xt, x, P)
        if mode == "steps":
            upd = torch.zeros((H, S, L.UPD_STRIDE), dtype=torch.float64, device="cuda")
            for k in range(K):
                eng.launch_step_sensors(k % H, (k + 1) % H, 1 + k, sp, [int(a) for a in sched[k]], upd[(k + 1) % H].data_ptr(),
                                        fast_stats=True, argmax_spos=argmax)
        else:
            eng.launch_rollout_sensors(0, 1, sp, torch.as_tensor(sched.astype(np.int32)).cuda(), argmax_spos=argmax)
            upd = eng.upd_sensors
        torch.cuda.synchronize()
        out = {k: getattr(eng, k).cpu().numpy() for k in ("x_true", "x_filter", "P_filter", "obs", "metrics", "status", "stats")}
        out["upd"] = upd.cpu().numpy()
        out["fail_count"] = int(eng.fail_count.cpu().numpy()[0])
        out["fail_log"] = eng.fail_log[:out["fail_count"]].copy()
        out["shards"] = eng._roll_shards.cpu().numpy() if mode == "rollout" else None
        outs.append(out)
    return outs


def _engine_case(hip, S, m, K, H, propagator, obs_type, resample, interval, argmax, layout=False):
    torch, L, host = hip.torch, hip.lib, hip.host
    xt, x, P, g = make_batch(m, seed=123)
    x[BAD, 1] = np.nan
    trans = c2t()[:N_TIME]
    lla, lim, Rs, sig, sp = _net(host, S, obs_type, N_TIME * m * 3)

    def consts(s):
        return host.make_consts(g["Q"], Rs[s], 1e-4, 2.0, -3, 20.0, lim[s], lla[s], propagator=propagator, obs_type=obs_type,
                                resample=resample, update_interval=interval)
    consts_of = [consts(s) for s in range(S)]
    gen = torch.Generator(device="cuda").manual_seed(8)
    zn = torch.randn((S, N_TIME, m, 3), dtype=torch.float64, device="cuda", generator=gen) * \
        torch.as_tensor(np.stack(sig), device="cuda").view(S, 1, 1, 3)
    vis = _visibility(hip, consts_of, xt, x, P, m, K, trans, zn, sp)
    order = None
    if layout:
        from ssa_gym_amd.catalogue import regime_order
        order = regime_order(xt)
    sched, planned = _build_schedule(np.random.RandomState(17), m, S, K, H, interval, vis, order)
    a, b = _run_both(hip, consts_of[0], m, K, H, xt, x, P, trans, zn, sp, sched, argmax, order)
    _assert_schedule_seen(L, m, S, K, H, interval, sched, planned, vis, order, a)
    _compare(L, a, b, K, H, argmax)


SIZES = [(2003, 7, 8), (403, 9, 4), (30001, 4, 3)]     # ragged last tiles; K < H, ring wrap; > 20 480 objects: several tiles per wavefront


@pytest.mark.parametrize("S", [1, 3, 8])
@pytest.mark.parametrize("m,K,H", SIZES)
def test_sensor_rollout_equals_single_sensor_steps(hip, S, m, K, H):
    """the core test ('hybrid', arg-max of sigma_pos in the statistics): one launch_rollout_sensors against K launch_step_sensors"""
    _engine_case(hip, S, m, K, H, "hybrid", "aer", False, 1, True)


@pytest.mark.parametrize("propagator,obs_type,resample,interval,argmax", [("fg", "aer", False, 1, False), ("j2", "aer", False, 1, False),
                                                                         ("elements", "aer", False, 1, True), ("fg", "xyz", True, 1, False),
                                                                         ("fg", "aer", True, 3, True), ("hybrid", "xyz", False, 3, False)])
@pytest.mark.parametrize("S,m,K,H", [(3, 2003, 7, 8), (8, 403, 9, 4)])
def test_sensor_rollout_propagators_observations_resampling_interval(hip, S, m, K, H, propagator, obs_type, resample, interval, argmax):
    _engine_case(hip, S, m, K, H, propagator, obs_type, resample, interval, argmax)


@pytest.mark.parametrize("S,K,H", [(3, 7, 8), (8, 9, 4)])
def test_sensor_rollout_under_a_storage_layout(hip, S, K, H):
    """the same comparison with the objects stored by orbit regime (set_layout(regime_order(...))) at 20 000 objects"""
    _engine_case(hip, S, 20000, K, H, "hybrid", "aer", False, 1, True, layout=True)


@pytest.mark.parametrize("m,K,H", [(2003, 7, 8), (403, 9, 4)])
def test_one_site_rollout_equals_the_plain_rollout(hip, m, K, H):
    """S = 1 with the engine's own observer: launch_rollout_sensors leaves what launch_rollout leaves, bit for bit"""
    torch, L, host = hip.torch, hip.lib, hip.host
    xt, x, P, g = make_batch(m, seed=123)
    x[BAD, 1] = np.nan
    lim = np.radians(15.0)
    consts = host.make_consts(g["Q"], g["R"], 1e-4, 2.0, -3, 20.0, lim, g["obs_lla"], propagator="hybrid")
    sp = host.make_sensor_params([g["obs_lla"]], [lim], [g["R"]], 0)
    trans = c2t()[:N_TIME]
    zn = torch.as_tensor(np.random.RandomState(8).normal(size=(N_TIME, m, 3)) * np.array([4.8e-6, 4.8e-6, 1e3])).cuda()
    acts = np.array([[(7 + 3 * k) % m] for k in range(K)], dtype=np.int32)
    acts[2, 0] = BAD
    outs = []
    for mode in ("rollout", "sensors"):
        eng = hip.engine.HotPathEngine(consts, m, 1, trans, zn, history=H, zn_stride_env=0)
        eng.load_state(0, xt, x, P)
        if mode == "rollout":
            eng.launch_rollout(0, 1, torch.as_tensor(acts).cuda(), argmax_spos=True)
            upd = eng.upd
        else:
            eng.launch_rollout_sensors(0, 1, sp, torch.as_tensor(acts).cuda(), argmax_spos=True)
            upd = eng.upd_sensors
        torch.cuda.synchronize()
        out = {k: getattr(eng, k).cpu().numpy() for k in ("x_true", "x_filter", "P_filter", "obs", "metrics", "status", "stats")}
        out.update(upd=upd.cpu().numpy(), fail_count=int(eng.fail_count.cpu().numpy()[0]), shards=eng._roll_shards.cpu().numpy())
        out["fail_log"] = eng.fail_log[:out["fail_count"]].copy()
        outs.append(out)
    _compare(L, outs[0], outs[1], K, H, True)
    assert outs[0]["fail_count"] >= 1 and np.any(outs[0]["upd"][..., L.UPD_OBS_TAKEN] == 1.0)


def test_engine_refuses_several_envs_a_short_noise_table_and_a_wrong_schedule(hip):
    """before anything is launched: n_env != 1, a noise table too short for the network (it would be read out of bounds), a schedule
    that is not [K, S] / [K, 8] int32 on the device"""
    torch, host = hip.torch, hip.host
    m = 64
    xt, x, P, g = make_batch(2 * m, seed=3)
    _, _, _, _, sp = _net(host, 3, "aer", N_TIME * m * 3)
    consts = host.make_consts(g["Q"], g["R"], 1e-4, 2.0, -3, 20.0, -np.pi / 2, g["obs_lla"])
    sched = torch.zeros((4, 3), dtype=torch.int32, device="cuda")
    zn3 = torch.zeros((3, N_TIME, m, 3), dtype=torch.float64, device="cuda")
    two = hip.engine.HotPathEngine(consts, m, 2, c2t()[:N_TIME], zn3, history=4, zn_stride_env=0)
    with pytest.raises(hip.lib.SsaHipError, match="one env"):
        two.launch_rollout_sensors(0, 1, sp, sched)
    short = hip.engine.HotPathEngine(consts, m, 1, c2t()[:N_TIME], zn3[:2].contiguous(), history=4, zn_stride_env=0)
    with pytest.raises(hip.lib.SsaHipError, match="z_noise"):
        short.launch_rollout_sensors(0, 1, sp, sched)
    eng = hip.engine.HotPathEngine(consts, m, 1, c2t()[:N_TIME], zn3, history=4, zn_stride_env=0)
    for bad in (sched.cpu(), sched.to(torch.int64), sched[:, :2].contiguous(), sched.t(), sched[:0]):
        with pytest.raises(hip.lib.SsaHipError, match="actions"):
            eng.launch_rollout_sensors(0, 1, sp, bad)


# ---------------------------------------------------------------- the env
def _steps(env, rows):
    """rows by step(), up to the first done: (last observation, rewards, dones)"""
    obs, rewards, dones = None, [], []
    for row in rows:
        obs, r, d, _ = env.step(row if env.n_sensor > 1 else int(row[0]))
        rewards.append(r)
        dones.append(d)
        if d:
            break
    return np.array(obs, copy=True), np.asarray(rewards), np.asarray(dones, dtype=bool)


@pytest.mark.parametrize("reward_type,obs_returned,regime", [("trinary", "flatten", False), ("jones", "aer", False),
                                                             ("shaped", "flatten", False), ("shaped", "aer", False),
                                                             ("trinary", "flatten", True)])
def test_env_rollout_sensors_equals_a_step_loop(envs, reward_type, obs_returned, regime):
    """env.rollout_sensors(schedule) against step() on a twin: a schedule with a chunk boundary inside (K > H - 1), one more step() on
    both, then a schedule longer than the episode.  'shaped': every other row tasks the previous arg-max of sigma_pos from sensor 2.
    regime: the rollout's env stores its objects by orbit regime until the rollout puts them back (as rollout() does)."""
    over = dict(steps=48, history=16, reward_type=reward_type, obs_returned=obs_returned)
    a = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, **over))
    b = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, storage_layout='regime' if regime else None, **over))
    assert a._engine.H == 16 and b.n_sensor == 3
    rs = np.random.RandomState(21)
    # 25 rows by step() on the yardstick, built as it goes ('shaped' needs its arg-max of the step before); then a few more rows, which a
    # rollout that has seen `done` must not execute
    rows, rewards, dones, obs_a, hits = [], [], [], None, 0
    for k in range(25):
        row = _distinct(rs, a.m, 3)
        prev = a._argmax_sigma
        if reward_type == 'shaped' and k % 2 and 0 <= prev < a.m:
            row = np.asarray([x for x in row if x != prev][:2] + [prev])      # sensor 2 takes it
            hits += 1
        obs_a, r, d, _ = a.step(row)
        rows.append(row)
        rewards.append(r)
        dones.append(d)
        if d:
            break
    assert reward_type != 'shaped' or hits > 0
    print("yardstick: %d steps by step(), done = %s, failed filters %d" % (len(rows), dones[-1], len(a.failed_filters_id)))
    extra = [_distinct(rs, a.m, 3) for _ in range(3)] if dones[-1] else []
    obs_b, rew_b, don_b, info = b.rollout_sensors(np.asarray(rows + extra))
    assert info == {} and _same(rew_b, np.asarray(rewards)) and _same(don_b, np.asarray(dones, dtype=bool))
    assert _same(obs_b, obs_a), "observation after the schedule"
    _assert_same_env(a, b, "after the schedule")
    if not dones[-1]:
        row = _distinct(rs, a.m, 3)      # the rollout leaves the env steppable
        oa, ra, da, _ = a.step(row)
        ob, rb, db, _ = b.step(row)
        assert _same(oa, ob) and _same(ra, rb) and da == db
        _assert_same_env(a, b, "one more step")
        if not da:                       # a schedule longer than the episode stops at `done`
            long_rows = np.asarray([_distinct(rs, a.m, 3) for _ in range(a.n - a.i + 5)])
            obs_a, rew_a, don_a = _steps(a, long_rows)
            obs_b, rew_b, don_b, _ = b.rollout_sensors(long_rows)
            assert don_a[-1] and len(rew_a) < len(long_rows)
            assert _same(rew_a, rew_b) and _same(don_a, don_b) and _same(obs_a, obs_b)
            _assert_same_env(a, b, "to the end of the episode")
            print("to the end: %d steps, i = %d, failed filters %d" % (len(rew_a), a.i, len(a.failed_filters_id)))
            if reward_type == 'trinary':
                assert a.i == a.n - 1
    with pytest.raises(ValueError, match="row 1"):
        b.rollout_sensors([[1, 2, 3], [4, 4, 5]])


def test_env_rollout_sensors_late_in_an_episode(envs):
    """20 000 objects, three sites, 'hybrid': both envs advanced by the same 300 step() calls; then 60 scheduled steps by step() on one
    and by rollout_sensors on the other -- with filters failing during those steps and an already-failed filter among the tasked
    (asserted on the step() twin, the yardstick)"""
    from ssa_gym_amd import _lib
    a = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, m=20000, history=64))
    b = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, m=20000, history=64))
    for env in (a, b):
        rs = np.random.RandomState(7)
        for _ in range(300):
            env.step(_distinct(rs, env.m, 3))
    _assert_same_env(a, b, "after 300 steps")
    failed_before = list(a.failed_filters_id)
    n_failed_before = int(a._stats[_lib.STAT_N_FAILED])
    assert failed_before, "no failed filter after 300 steps"
    sched = np.asarray([_distinct(rs, a.m, 3) for _ in range(60)])
    for k, j in ((5, failed_before[0]), (40, failed_before[-1])):      # sensor 1 is tasked to a filter that failed before the window
        sched[k, 1] = j
        assert len(set(sched[k])) == 3
    obs_a, rew_a, don_a = _steps(a, sched)
    print("failed filters: %d before the window, %d after it" % (n_failed_before, int(a._stats[_lib.STAT_N_FAILED])))
    assert len(rew_a) == 60 and int(a._stats[_lib.STAT_N_FAILED]) > n_failed_before      # filters failed during the window
    assert any(j in failed_before for j in sched.ravel())                                 # ... and a failed one was tasked
    assert (a._upd_action[301 + 5, 1] == -1) and a.obs_taken[301:361].any()
    obs_b, rew_b, don_b, _ = b.rollout_sensors(sched)
    assert _same(rew_a, rew_b) and _same(don_a, don_b) and _same(obs_a, obs_b)
    _assert_same_env(a, b, "after the 60 scheduled steps")
    row = _distinct(rs, a.m, 3)
    assert _same(a.step(row)[0], b.step(row)[0])
    _assert_same_env(a, b, "one more step")


@pytest.mark.parametrize("reward_type,obs_returned", [("trinary", "flatten"), ("shaped", "aer")])
def test_without_observers_rollout_sensors_is_rollout(envs, reward_type, obs_returned):
    """no config['observers']: rollout_sensors with [K, 1] runs the env's one observer as a one-site network and equals rollout with [K]"""
    over = dict(steps=48, history=16, reward_type=reward_type, obs_returned=obs_returned)
    a = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, sensors=0, **over))
    b = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, sensors=0, **over))
    assert b.n_sensor == 1
    acts = np.random.RandomState(2).randint(a.m, size=40)
    oa, ra, da, _ = a.rollout(acts)
    ob, rb, db, _ = b.rollout_sensors(acts[:, None])
    assert len(ra) >= 1 and _same(ra, rb) and _same(da, db) and _same(oa, ob)
    _assert_same_env(a, b, "rollout against rollout_sensors")
    if not da[-1]:
        assert _same(a.step(3)[0], b.step(3)[0])
        _assert_same_env(a, b, "one more step")
