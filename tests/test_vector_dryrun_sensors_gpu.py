"""The dry run of B candidate schedules of every env in one launch (include/ssa_hip.h: ssa_dryrun_gather_f64, then
ssa_dryrun_sensors_envs_f64 over E * B pseudo-envs; HotPathEngine.launch_dryrun_sensors_envs; SSA_Tasker_VecEnv.evaluate_schedules;
agents.refine_plan_sensors on a vector env) on the MI355X.

The gather kernel is held against torch's index_select through device.dryrun_gather_rows, the numpy statement of its rule.  Everything
above it is held against the project's own one-env path, which this feature leaves untouched: E one-env engines (E single envs), each
holding env e's state slice, asked by launch_dryrun_sensors (evaluate_schedules, refine_plan_sensors) at env e's time index.
Everything is compared bit for bit; there is no tolerance anywhere.  All time indices stay below the support tables' N_TIME = 16."""
import numpy as np
import pytest

from support.dryrun import KEYS, record_bits, result_bits, same_result, slot_total
from support.gpu import envs, hip  # noqa: F401  (the module fixtures)
from support.sensors import cfg3, cfg8
from support.vector_dryrun import guarded, guards_intact, random_bits, schedules
from support.vector_forecast import bits, state_bytes
from support.vector_lookahead import Engines, bad_of, single_envs

pytestmark = pytest.mark.gpu
ALL = KEYS + ("spare",)


# ---------------------------------------------------------------------------------------------------------------- the gather kernel
@pytest.mark.parametrize("E,B,W,m,tables", [(1, 1, 4, 4, False), (2, 3, 8, 8, True), (9, 7, 12, 403, False), (9, 7, 12, 403, True)])
def test_gather_kernel_equals_index_select(hip, E, B, W, m, tables):
    """random bit patterns (NaN payloads, infinities, signed zeros) gathered by the kernel and by index_select over
    device.dryrun_gather_rows; guard words around every output; every candidate's time word.  (1, 1, 4, 4): the smallest; (2, 3, 8, 8):
    one slot_of permutation per env; (9, 7, 12, 403): 756 rows -- more than one block, a last block of four rows --, all-idle and
    out-of-range candidates, without and with tables"""
    torch, dev = hip.torch, hip.dev
    rs = np.random.RandomState(E * 100 + B)
    N, R = E * m, E * B * W
    src = [torch.from_numpy(random_bits(rs, N * w)).cuda() for w in (6, 6, 36)]
    status = torch.from_numpy(rs.randint(-2 ** 31, 2 ** 31, size=N, dtype=np.int64).astype(np.int32)).cuda()
    ids = np.full((E * B, W), -1, dtype=np.int32)
    for c in range(E * B):
        n = int(rs.randint(1, min(W, m) + 1))
        ids[c, :n] = np.sort(rs.permutation(m)[:n])
    if E * B >= 6:
        ids[1] = -1                                                            # an all-idle candidate
        ids[2] = [m, m + 7, 2 ** 31 - 1, -5] + [-1] * (W - 4)                  # nothing in range: the first id clamped below m
        ids[3, 1] = m                                                          # an id >= m between valid ones
        ids[4, 0], ids[4, 1] = -3, 1                                           # a negative first id: object 0 for the rows after it
        ids[E * B - 1] = np.arange(m - W, m)                                   # the last candidate full, up to the last object
    slot_of = None
    if tables:
        slot_of = np.concatenate([e * m + np.random.RandomState(70 + e).permutation(m) for e in range(E)]).astype(np.int32)
    times = rs.randint(0, 1000, size=E).astype(np.int32)
    rows = dev.dryrun_gather_rows(ids, E, B, m, slot_of=slot_of)
    assert rows.shape == (R,) and rows.min() >= 0 and rows.max() < N
    idx = torch.from_numpy(rows).cuda()
    want = [s.view(N, -1).index_select(0, idx) for s in src] + [status.index_select(0, idx)]
    bufs = [guarded(torch, R * 6, torch.int64), guarded(torch, R * 6, torch.int64), guarded(torch, R * 36, torch.int64),
            guarded(torch, R, torch.int32), guarded(torch, E * B, torch.int32)]
    f64 = torch.float64
    out = (bufs[0][1].view(f64).view(R, 6), bufs[1][1].view(f64).view(R, 6), bufs[2][1].view(f64).view(R, 6, 6), bufs[3][1], bufs[4][1])
    before = [t.clone() for t in src + [status]]
    got = dev.dryrun_gather(torch.from_numpy(ids).cuda(), torch.from_numpy(times).cuda(), src[0].view(f64).view(N, 6), src[1].view(f64).view(N, 6),
                            src[2].view(f64).view(N, 6, 6), status, E, B, m,
                            slot_of=None if slot_of is None else torch.from_numpy(slot_of).cuda(), out=out)
    torch.cuda.synchronize()
    assert all(g is o for g, o in zip(got, out))
    for k in range(3):
        assert torch.equal(bufs[k][1].view(R, -1), want[k]), ("x_true", "x", "P")[k]
    assert torch.equal(bufs[3][1], want[3])
    assert np.array_equal(bufs[4][1].cpu().numpy(), np.repeat(times, B))
    assert all(guards_intact(whole) for whole, _ in bufs)
    assert all(torch.equal(a, b) for a, b in zip(before, src + [status]))        # (the source block is read only)
    nan_words = int((src[2].view(f64) != src[2].view(f64)).sum())
    assert nan_words >= N * 36 // 8                                              # NaN payloads were among what was compared


# ---------------------------------------------------------------------------------------------------------------- engine level
def _pools(g):
    """per env the objects its schedules draw from, the NaN filter among the first two"""
    rs = np.random.RandomState(17)
    pools = []
    for e in range(g.E):
        p = [int(j) for j in rs.permutation(g.m) if j != bad_of(g.m)]
        pools.append(p[:1] + [bad_of(g.m)] + p[1:])
    return pools


def _dry_case(hip, E, m, S, K, B, by_value=True, **kw):
    """the vector launch against E one-env launches, from the loaded state (slot 0: the NaN filter fails inside THIS launch) and after
    one vector step with every sensor idle (slot 1: it had failed before the launch); the engine's state as bytes around every call.
    Returns the engines, the one-env twins, the schedules and both runs' (vector, yardsticks) records"""
    torch = hip.torch
    g = Engines(hip, E, m, S, **kw)
    assert max(g.t0) + 2 + K <= 16                                              # every time index below N_TIME
    ones = [g.one(e) for e in range(E)]
    a = schedules(np.random.RandomState(5 + E), E, B, K, S, m, pool=_pools(g))
    runs = []
    for k in (0, 1):
        if k == 1:       # one step, nobody observed: the state moves on, the NaN filter's status word is set
            g.vec.launch_step_sensors_envs(0, 1, 1, g.sp, np.full((E, S), -1), fast_stats=True)
            for e in range(E):
                ones[e].launch_step_sensors(0, 1, g.t0[e] + 1, g.sp, [-1] * S, 0, fast_stats=True)
        before = state_bytes(torch, g.vec)
        if by_value:
            rec = g.vec.launch_dryrun_sensors_envs(k, 0, g.sp, a, env_times=[t + 1 + k for t in g.t0])
        else:
            rec = g.vec.launch_dryrun_sensors_envs(k, 1 + k, g.sp, a)
        assert tuple(rec.shape) == (E, B, K, S, hip.lib.DRY_STRIDE)
        vec = [record_bits(rec[e]) for e in range(E)]
        after = state_bytes(torch, g.vec)
        assert before.keys() == after.keys() and {"status", "stats", "fail_count", "x_filter", "P_filter", "time_actions"} <= before.keys()
        for name in before:      # nothing of the engine's state is written
            assert before[name] == after[name], "the dry run wrote the engine's %s" % name
        yard = [record_bits(ones[e].launch_dryrun_sensors(k, g.t0[e] + 1 + k, g.sp, a[e])) for e in range(E)]
        for e in range(E):
            same_result(vec[e], yard[e], "slot %d env %d" % (k, e), keys=ALL)
            assert not vec[e]["spare"].any()
        runs.append((vec, yard))
    return g, ones, a, runs


def _assert_dry_conditions(hip, g, a, runs, interval=1):
    """what the cases were built for, found again in the YARDSTICK's records"""
    L = hip.lib
    E, m = g.E, g.m
    bad = bad_of(m)
    assert E == 1 or len(set(g.t0)) == E                                        # envs at different time indices
    (_, y0), (_, y1) = runs
    valid = (a >= 0) & (a < m)
    assert (~valid).any() and (a < 0).any() and (a >= m).any()                  # idle and out-of-range entries
    assert any(len(np.unique(a[e, b][valid[e, b]])) < valid[e, b].sum() for e in range(E) for b in range(a.shape[1]))      # revisits
    if a.shape[3] > 1:      # two sensors on one object in one row
        assert any(len(set(r[(r >= 0) & (r < m)].tolist())) < ((r >= 0) & (r < m)).sum() for r in a.reshape(-1, a.shape[3]))
    if a.shape[1] > 1:      # candidates with different numbers of distinct objects share the launch
        assert len({len(np.unique(a[e, b][valid[e, b]])) for e in range(E) for b in range(a.shape[1])}) >= 2
    assert any(y["taken"].any() for y in y0) and any(y["taken"].any() for y in y1)
    named = [(a[e] == bad).any() for e in range(E)]
    assert any(named)
    for e in range(E):
        at = a[e] == bad
        if interval == 1 and at[:, 1:].any():       # tasked after the predict of k = 0 failed it: its failure status, nothing taken
            assert not y0[e]["taken"][at].any()
            assert np.isin(y0[e]["status"][:, 1:][at[:, 1:]], (0, L.ST_PREDICT_NAN, L.ST_PREDICT_LINALG)).all(), e
        assert not y1[e]["taken"][at].any(), e      # a filter that had failed before the launch


@pytest.mark.parametrize("E,m,S,K,B", [(2, 4, 2, 3, 2), (3, 8, 3, 5, 7), (9, 12, 8, 4, 3), (1, 7, 3, 4, 2)])
def test_vector_dry_run_equals_one_env_dry_runs(hip, E, m, S, K, B):
    """(2, 4, 2, 3, 2): one tile per env; (3, 8, 3, 5, 7): candidates with different numbers of distinct objects in one launch;
    (9, 12, 8, 4, 3): more envs than INLINE_ENVS -- the time words still travel by value, in the call's own upload --, every sensor
    slot; (1, 7, 3, 4, 2): one env with a partial tile -- also equal to launch_dryrun_sensors on the same engine"""
    g, ones, a, runs = _dry_case(hip, E, m, S, K, B)
    _assert_dry_conditions(hip, g, a, runs)
    if E == 1:
        own = record_bits(g.vec.launch_dryrun_sensors(1, 2, g.sp, a[0]))
        same_result(runs[1][0][0], own, "the engine's own one-env launch", keys=ALL)


def test_vector_dry_run_time_words_by_value_and_from_memory(hip):
    x = _dry_case(hip, 3, 8, 3, 5, 7, by_value=True)
    y = _dry_case(hip, 3, 8, 3, 5, 7, by_value=False)
    _assert_dry_conditions(hip, x[0], x[2], x[3])
    for k in (0, 1):
        for e in range(3):
            same_result(x[3][k][0][e], y[3][k][0][e], "by value against env_time0", keys=ALL)
    _dry_case(hip, 9, 12, 8, 4, 3, by_value=False)
    _dry_case(hip, 1, 7, 3, 4, 2, by_value=False)


def test_vector_dry_run_with_per_env_layouts(hip):
    """per-env storage layouts (set_layout with [E][m] permutations): the gather goes through the inverse table; 400 objects per env"""
    g, ones, a, runs = _dry_case(hip, 3, 400, 3, 5, 4, layout=True)
    _assert_dry_conditions(hip, g, a, runs)
    assert g.vec._order is not None and not np.array_equal(g.orders[0], g.orders[1])
    _, _, a2, plain = _dry_case(hip, 3, 400, 3, 5, 4)
    assert np.array_equal(a, a2)
    for e in range(3):      # (a storage layout never shows)
        same_result(runs[0][0][e], plain[0][0][e], "layout against plain", keys=ALL)
    g1, _, a1, runs1 = _dry_case(hip, 1, 7, 3, 4, 2, layout=True)       # one env, a partial tile, a layout
    assert g1.vec._order is not None


@pytest.mark.parametrize("propagator,obs_type,interval", [("fg", "aer", 1), ("j2", "aer", 1), ("elements", "aer", 1), ("hybrid", "xyz", 1),
                                                          ("hybrid", "aer", 3)])
def test_vector_dry_run_every_propagator_xyz_and_update_interval(hip, propagator, obs_type, interval):
    g, ones, a, runs = _dry_case(hip, 3, 8, 3, 5, 4, propagator=propagator, obs_type=obs_type, interval=interval)
    _assert_dry_conditions(hip, g, a, runs, interval=interval)
    if interval == 3:      # env e's step k is an update step when (t0[e] + 1 + k) % 3 == 0 -- at other steps in every env
        upd = np.array([[(t + 1 + k) % 3 == 0 for k in range(5)] for t in g.t0])
        assert len({tuple(u) for u in upd.tolist()}) >= 2
        for e in range(3):
            y = runs[0][1][e]
            assert not y["taken"][:, ~upd[e]].any() and (y["action"][:, ~upd[e]] == -1).all(), e


# ---------------------------------------------------------------------------------------------------------------- env level
def _vec_cfg(envs, **over):
    return cfg3(envs, **dict(dict(m=12, steps=12, update_interval=1), **over))


def _actions(rs, E, S, m):
    return np.stack([rs.permutation(m)[:S] for _ in range(E)])


def _pair(envs, cfg, E, seed=10):
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    vec = SSA_Tasker_VecEnv(cfg, E, seed=seed)
    return vec, single_envs(envs, cfg, vec, seed)


def _step_both(vec, singles, acts):
    vec.step(acts)
    for e, one in enumerate(singles):
        one.step(acts[e] if vec.n_sensor > 1 else int(acts[e]))


def _same_as_singles(vec, singles, a, what):
    got = result_bits(vec.evaluate_schedules(a))
    a4 = a if a.ndim == 4 else a[:, None]
    assert set(got) == set(KEYS) | {"total"}
    for e, one in enumerate(singles):
        want = result_bits(one.evaluate_schedules(a4[e]))
        assert set(want) == set(got)
        same_result({k: v[e] for k, v in got.items()}, want, (what, e), keys=tuple(got))
    return got


def test_vector_env_dry_run_equals_single_envs(envs, hip):
    """after 2 steps every key, `total` included, equals the single envs'; [E, K, S] gives B = 1; torch input; K is clipped near the
    episode's end; no dry run once an env has no next step"""
    torch = hip.torch
    E, S, m = 3, 3, 12
    vec, singles = _pair(envs, _vec_cfg(envs), E)
    rs = np.random.RandomState(4)
    for _ in range(2):
        _step_both(vec, singles, _actions(rs, E, S, m))
    a = schedules(np.random.RandomState(9), E, 4, 4, S, m)
    got = _same_as_singles(vec, singles, a, "[E, B, K, S]")
    assert got["score"].shape == (E, 4, 4, S, 3) and got["total"].shape == (E, 4, 3) and got["taken"].shape == (E, 4, 4, S)
    assert got["taken"].any() and (got["action"] >= 0).any()
    for e in range(E):      # the totals are the slot-order sums
        for b in range(4):
            rec = {k: v[e, b:b + 1] for k, v in got.items()}
            for c in range(3):
                assert np.array_equal(np.array([slot_total(rec, c)]).view(np.int64), got["total"][e, b, c:c + 1]), (e, b, c)
    r = vec.evaluate_schedules(a[:, 1])
    assert r["score"].shape == (E, 1, 4, S, 3) and r["total"].shape == (E, 1, 3) and r["taken"].dtype == torch.bool
    assert r["status"].dtype == torch.int32 and r["action"].dtype == torch.int64
    one_b = _same_as_singles(vec, singles, a[:, 1], "[E, K, S]")
    for k in one_b:
        assert np.array_equal(one_b[k][:, 0], got[k][:, 1]), k
    as_torch = result_bits(vec.evaluate_schedules(torch.from_numpy(a).cuda()))
    for k in got:
        assert np.array_equal(as_torch[k], got[k]), k
    for _ in range(7):
        _step_both(vec, singles, _actions(rs, E, S, m))
    assert np.all(vec.i == 9)
    cut = _same_as_singles(vec, singles, a, "K clipped")                        # (steps = 12: two steps left)
    assert cut["taken"].shape == (E, 4, 2, S)
    saved = vec.i.copy()
    vec.i[1] = vec.n - 2
    assert vec.evaluate_schedules(a)["taken"].shape == (E, 4, 1, S)             # (one K' for all envs: the shortest)
    vec.i[1] = vec.n - 1                                                        # (an env on its last index: no next step)
    with pytest.raises(ValueError, match="at least one step"):
        vec.evaluate_schedules(a)
    vec.i[:] = saved


def test_vector_env_without_observers_and_six_objects(envs, hip):
    """no network (S = 1: the envs' own observer as a one-site network), rso_count = 6 in 2 envs: the plain vector env takes
    m % 4 != 0, and so does its dry run -- the gathered block has whole tiles"""
    E, m = 2, 6
    vec, singles = _pair(envs, _vec_cfg(envs, m=m, sensors=0), E)
    assert vec.n_sensor == 1
    rs = np.random.RandomState(2)
    for _ in range(3):
        _step_both(vec, singles, rs.randint(0, m, size=E))
    a = schedules(np.random.RandomState(3), E, 5, 4, 1, m)
    got = _same_as_singles(vec, singles, a, "no network")
    assert got["score"].shape == (E, 5, 4, 1, 3) and got["taken"].any()


def test_dry_run_before_every_step_leaves_the_episode_alone(envs, hip):
    """a dry run before each of 10 vector steps against a twin vector env that ran none: observations, rewards, dones and the state
    identical; the engine's tensors, i, tick and the envs' generators identical around every call"""
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    cfg = _vec_cfg(envs)
    E, S, m = 3, 3, 12
    vec = SSA_Tasker_VecEnv(cfg, E, seed=10)
    twin = SSA_Tasker_VecEnv(cfg, E, seed=10)
    twin._eng.z_noise.copy_(vec._eng.z_noise)
    rs, rc = np.random.RandomState(4), np.random.RandomState(8)
    for k in range(10):
        states = [r.get_state()[2] for r in vec._rng]
        before = state_bytes(hip.torch, vec._eng)
        a = schedules(rc, E, 1 + k % 3, 1 + k % 4, S, m)
        r = vec.evaluate_schedules(a if k % 2 else a[:, 0])
        after = state_bytes(hip.torch, vec._eng)
        assert before.keys() == after.keys() and all(before[n] == after[n] for n in before), k
        assert r["taken"].shape == (E, a.shape[1] if k % 2 else 1, min(a.shape[2], 11 - k), S)
        assert states == [g.get_state()[2] for g in vec._rng] and np.all(vec.i == k) and vec.tick == k
        acts = _actions(rs, E, S, m)
        oa, ra, da, _ = vec.step(acts)
        ob, rb, db, _ = twin.step(acts)
        assert np.array_equal(oa.view(np.int64), ob.view(np.int64)) and np.array_equal(ra, rb) and np.array_equal(da, db), k
        for e in range(E):
            for nme in ("x_true", "x_filter", "P_filter"):
                assert np.array_equal(bits(getattr(vec, nme)(e)), bits(getattr(twin, nme)(e))), (k, e, nme)


# ---------------------------------------------------------------------------------------------------------------- the planner
def test_vector_refine_equals_single_envs(envs, hip):
    """refine_plan_sensors(vec, plan): env e's plan and total equal refine_plan_sensors(single_e, plan[e], seed=seed + e), bit for bit;
    the returned totals are the plans' own and no smaller than the incumbents'; the envs' generators are not touched;
    vec.rollout_sensors() takes the plan as it comes, and the dry run's taken flags are the ones the rollout books"""
    from ssa_gym_amd import _lib as L, agents
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    torch = hip.torch
    E, S, m, K = 3, 3, 12, 4
    cfg = _vec_cfg(envs)
    vec, singles = _pair(envs, cfg, E)
    twin = SSA_Tasker_VecEnv(cfg, E, seed=10)
    twin._eng.z_noise.copy_(vec._eng.z_noise)
    rs = np.random.RandomState(4)
    for _ in range(2):
        acts = _actions(rs, E, S, m)
        _step_both(vec, singles, acts)
        twin.step(acts)
    vec.single_action_space.seed(1)
    plan = agents.plan_info_gain_sensors_horizon(vec, K)
    assert plan.shape == (E, K, S)
    states = [r.get_state()[2] for r in vec._rng]
    base = vec.evaluate_schedules(plan)["total"].cpu().numpy()[:, 0]
    out, total = agents.refine_plan_sensors(vec, plan, kind='info', rounds=2, candidates=8, seed=5)
    assert states == [r.get_state()[2] for r in vec._rng]
    assert out.shape == (E, K, S) and out.dtype == np.int64 and total.shape == (E, 3) and total.dtype == np.float64
    for e in range(E):
        one, tot = agents.refine_plan_sensors(singles[e], plan[e], kind='info', rounds=2, candidates=8, seed=5 + e)
        assert np.array_equal(out[e], one), (e, out[e].tolist(), one.tolist())
        assert np.array_equal(total[e].view(np.int64), tot.view(np.int64)), e
    own = vec.evaluate_schedules(out)
    assert np.array_equal(bits(own["total"].cpu().numpy()[:, 0]), bits(total))
    print("[vector refine] incumbents %s refined %s (%d slots changed)" % (base[:, L.LOOK_INFO_GAIN].tolist(), total[:, L.LOOK_INFO_GAIN].tolist(),
                                                                          int((out != plan).sum())))
    assert (total[:, L.LOOK_INFO_GAIN] >= base[:, L.LOOK_INFO_GAIN]).all()
    taken = own["taken"].cpu().numpy()[:, 0]                                    # [E, K, S]
    # what the rollout books: the update records of the same schedule run on the twin, the launch vec.rollout_sensors() makes
    twin._eng.env_time0.copy_(torch.as_tensor(twin.i + 1, dtype=torch.int32))
    sched = torch.from_numpy(np.ascontiguousarray(out.transpose(1, 0, 2)).astype(np.int32)).cuda()
    _, upd = twin._eng.launch_rollout_sensors_envs(twin.tick % 2, 0, twin._sites(), sched, records=True)
    torch.cuda.synchronize()
    booked = upd.cpu().numpy()[..., L.UPD_OBS_TAKEN].transpose(1, 0, 2) == 1.0  # [E, K, S]
    print("[vector refine] taken %s booked %s" % (taken.astype(int).tolist(), booked.astype(int).tolist()))
    assert np.array_equal(taken, booked) and booked.any()
    i0 = vec.i.copy()
    _, rewards, dones, _ = vec.rollout_sensors(out)
    assert rewards.shape == (E, K) and np.all(vec.i == i0 + K)


def test_vector_refine_finds_the_revisit(envs, hip):
    """10 objects, one site that sees all of them, 15 slots (the single env's case): the refined plan revisits, and its information
    gain is at least the horizon plan's.  A vector env forecasts rso_count = 10 for one env only (several envs need whole tiles per
    env), so this is num_envs = 1 -- and its result equals the single env's with the same seed; 12 objects in 3 envs follow"""
    from ssa_gym_amd import _lib as L, agents
    cfg = cfg8(envs, m=10, sensors=0, seed=21, steps=60, obs_limit=-80)
    vec, singles = _pair(envs, cfg, 1, seed=21)
    rs = np.random.RandomState(3)
    for _ in range(2):
        _step_both(vec, singles, rs.randint(0, 10, size=1))
    vec.single_action_space.seed(2)
    plan = agents.plan_info_gain_sensors_horizon(vec, 15)
    assert plan.shape == (1, 15, 1)
    base = vec.evaluate_schedules(plan)["total"].cpu().numpy()[:, 0]
    out, total = agents.refine_plan_sensors(vec, plan, kind='info', rounds=4, candidates=32, seed=2)
    one, tot = agents.refine_plan_sensors(singles[0], plan[0], kind='info', rounds=4, candidates=32, seed=2)
    assert np.array_equal(out[0], one) and np.array_equal(total[0].view(np.int64), tot.view(np.int64))
    counts = np.bincount(out[0, :, 0], minlength=10)
    print("[vector refine revisit] horizon plan %s total %r\n  refined %s total %r visits %s"
          % (plan[0, :, 0].tolist(), base[0, L.LOOK_INFO_GAIN], out[0, :, 0].tolist(), total[0, L.LOOK_INFO_GAIN], counts.tolist()))
    assert counts.max() >= 2, "the refined plan has no revisit"
    assert total[0, L.LOOK_INFO_GAIN] >= base[0, L.LOOK_INFO_GAIN]
    # three envs, 12 objects, 15 slots each: every env's refined plan revisits (15 slots, 12 objects) and is worth at least its incumbent
    E = 3
    cfg = cfg8(envs, m=12, sensors=0, seed=21, steps=60, obs_limit=-80)
    vec, singles = _pair(envs, cfg, E, seed=21)
    for _ in range(2):
        _step_both(vec, singles, rs.randint(0, 12, size=E))
    plan = agents.plan_info_gain_sensors_horizon(vec, 15)
    base = vec.evaluate_schedules(plan)["total"].cpu().numpy()[:, 0]
    out, total = agents.refine_plan_sensors(vec, plan, kind='info', rounds=3, candidates=16, seed=2)
    for e in range(E):
        one, tot = agents.refine_plan_sensors(singles[e], plan[e], kind='info', rounds=3, candidates=16, seed=2 + e)
        assert np.array_equal(out[e], one) and np.array_equal(total[e].view(np.int64), tot.view(np.int64)), e
        assert np.bincount(out[e, :, 0], minlength=12).max() >= 2, e
    assert (total[:, L.LOOK_INFO_GAIN] >= base[:, L.LOOK_INFO_GAIN]).all()
    i0 = vec.i.copy()
    vec.rollout_sensors(out)
    assert np.all(vec.i == i0 + 15)
