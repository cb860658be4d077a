"""A sensor network's horizon-wide OPTIMAL tasking plan on the device (include/ssa_hip.h: ssa_plan_sensors_f64)
and the planners on top of it (agents.plan_info_gain_sensors_horizon / plan_trace_gain_sensors_horizon), on the MI355X.

The exact part feeds DYADIC tables (multiples of 2^-10: the kernel's fixed-point arithmetic is exact on them) and asks for the optimum
itself: the filled-slot count of scipy's maximum_bipartite_matching and the total of linear_sum_assignment, `math.fsum` against
`math.fsum`, no tolerance.  On a raw forecast the total may fall short of the yardstick's by the header's bound, 4 N 2^-53 max|score|
(support.planning.bound): the one rounding of the scores to the kernel's unit, derived in DESIGN.md section 8o, not measured."""
import math

import numpy as np
import pytest

from support import planning as P
from support.batches import c2t, make_batch
from support.gpu import envs, hip  # noqa: F401  (the module fixtures)
from support.sensors import BAD, N_TIME, _distinct, cfg3, cfg8, sites_rad
from support.vector_forecast import bits, state_bytes
from support.vector_lookahead import single_envs

pytestmark = pytest.mark.gpu

W, CH = P.W, P.CH
SHAPES = [(2, 1, 2), (8, 8, 5), (8, 8, 70), (5, 3, 403), (8, 8, 2003), (64, 1, 130), (3, 8, 30001)]
PVIS = {(2, 1, 2): 1.0, (8, 8, 5): 0.6, (8, 8, 70): 0.3, (5, 3, 403): 0.1, (8, 8, 2003): 0.05, (64, 1, 130): 0.3, (3, 8, 30001): 0.02}


def _dy(a):
    return np.round(np.asarray(a, dtype=np.float64) * 1024.0) / 1024.0


def _spread(m, n):
    """n distinct objects spread over the chunks of m objects, chunk boundaries first (511 | 512, ...)"""
    edge = [j for b in range(CH, m, CH) for j in (b - 1, b)]
    rest = [j for j in np.linspace(0, m - 1, 4 * n + 3).astype(int).tolist() if j not in edge]
    out = []
    for j in edge + rest + list(range(m)):
        if j not in out:
            out.append(int(j))
        if len(out) == n:
            break
    return out


def _tables(H, S, m, seed):
    """named dyadic tables [H, S, m] that hold the situations the test asserts it saw"""
    rs = np.random.RandomState(seed)
    N = H * S
    out = {}

    def noise(lo=-5.0, hi=5.0, nan=0.3):
        a = _dy(rs.uniform(lo, hi, size=(H, S, m)))
        a[rs.uniform(size=(H, S, m)) < nan] = np.nan
        return a
    if (H, S, m) == (2, 1, 2):
        out["ab"] = np.array([[[10.0, 9.5]], [[9.0, np.nan]]])      # the time-ordered plan takes A (10) and finds nothing left
    for k in range(3):
        out["windows%d" % k] = P.dyadic_table(np.random.default_rng(seed + k), H, S, m, PVIS[(H, S, m)])
    out["noise"] = noise()
    ob = _spread(m, min(m, 4))
    a = noise(nan=0.1)                                   # one object best for every slot
    a[:, :, ob[0]] = 100.0 + _dy(rs.uniform(size=(H, S)))
    out["one_best"] = a
    a = noise()
    a[H - 1, S - 1], a[0, 0] = np.nan, np.nan            # all-NaN slots
    out["nan_slot"] = a
    a = noise(0.0, 5.0)                                  # a slot whose only candidate is negative (and nobody else's)
    a[0, 0], a[:, :, ob[0]] = np.nan, np.nan
    a[0, 0, ob[0]] = -3.5
    out["neg_only"] = a
    a = np.where(rs.uniform(size=(H, S, m)) < 0.5, -0.0, 0.0)      # -0.0 against 0.0: one value
    a[rs.uniform(size=(H, S, m)) < 0.3] = -1.0
    a[:, :, 0] = -0.0
    out["signed_zeros"] = a
    a = noise()                                          # +inf, -inf and 2^1021: not candidates
    for k, j in enumerate(_spread(m, min(m, 3 * N))):
        a[(k % N) // S, (k % N) % S, j] = (np.inf, 2.0 ** 1021, -np.inf, -2.0 ** 1021)[k % 4]
    out["nonfinite"] = a
    a = rs.randint(0, 3, size=(H, S, m)).astype(np.float64)        # exact ties across slots and chunk boundaries
    a[rs.uniform(size=(H, S, m)) < 0.2] = np.nan
    for j in _spread(m, min(m, 6)):
        a[:, :, j] = 7.0
    out["ties"] = a
    if m > CH:                                           # the best objects on both sides of a chunk boundary
        a = noise()
        a[0, 0, CH - 1], a[H - 1, S - 1, CH] = 50.0, 60.0
        out["boundary"] = a
    if 2 <= N <= m:
        # the last slot's N - 1 best objects are each worth far more to another slot: the optimum gives it its N-th candidate
        a = noise(lo=0.0, hi=1.0, nan=0.1)
        f = a.reshape(N, m)
        obj = _spread(m, N)
        for t in range(N - 1):
            f[t, obj[t]] = 1000.0 - t
            f[N - 1, obj[t]] = 100.0 - 0.5 * t
        f[N - 1, obj[N - 1]] = 50.0
        out["deep"] = a
    return out


def _rank_of(row, ok, j):
    """position of object j in its slot's own order (value descending, index ascending) among the candidates"""
    v = row[j]
    return int(np.sum(ok & (row > v)) + np.sum(ok[:j] & (row[:j] == v)))


def _optimum_plan(sc):
    """linear_sum_assignment's own plan [N] of a dyadic table (object per slot, -1: none)"""
    from scipy.optimize import linear_sum_assignment
    f = P.flat(sc)
    ok = P.candidates(f)
    cols = np.flatnonzero(ok.any(axis=0))
    r, c = linear_sum_assignment(np.where(ok[:, cols], f[:, cols] + P.SHIFT, 0.0), maximize=True)
    plan = np.full(f.shape[0], -1, dtype=np.int64)
    plan[r[ok[:, cols][r, c]]] = cols[c[ok[:, cols][r, c]]]
    return plan


def _call(hip, score, col, ws):
    """device.plan_sensors on score (numpy [H, (E,) S, m, 3]) into rows / picks prefilled with -7"""
    torch = hip.torch
    t = torch.as_tensor(np.ascontiguousarray(score)).cuda()
    lead = tuple(score.shape[:-3])
    rows = torch.full(lead + (W,), -7, dtype=torch.int32, device="cuda")
    picks = torch.full(lead + (W, 2), -7, dtype=torch.int64, device="cuda")
    got = hip.dev.plan_sensors(t, col, out=rows, picks=picks, workspace=ws)
    assert got is rows
    torch.cuda.synchronize()
    return rows.cpu().numpy(), picks.cpu().numpy()


def _in_column(sc, col):
    """[H, S, m, 3] with the table in column `col` and decoys (the table reversed along the objects, its negative) in the others"""
    out = np.empty(sc.shape + (3,))
    out[..., col], out[..., (col + 1) % 3], out[..., (col + 2) % 3] = sc, sc[..., ::-1], -sc
    return out


def _situations(tabs, H, S, m):
    """what the tables hold, found before the device is asked: (the yardstick per table, the situations seen)"""
    N = H * S
    seen = set()
    yard = {}
    # ---- what the inputs hold, asserted before the device is asked
    for name, sc in tabs.items():
        ok = P.candidates(P.flat(sc))
        yard[name] = P.best_dyadic(sc)
        assert yard[name][0] == P.best_count(sc), name
        if np.isfinite(sc[~np.isnan(sc)]).all():         # (the time-ordered rule takes +-inf for values: compared where there are none)
            to = P.time_ordered(sc)
            if P.count(to) < yard[name][0]:
                seen.add("time_ordered_fewer")
            elif P.total(sc, to) < yard[name][1]:
                seen.add("time_ordered_smaller")
            assert P.count(to) <= yard[name][0], name
        if not ok.any(axis=1).all():
            seen.add("nan_slot")
        if ok.any(axis=0).sum() < N:
            seen.add("fewer_objects_than_slots")
        if (np.signbit(sc) & (sc == 0)).any() and (~np.signbit(sc) & (sc == 0)).any():
            seen.add("signed_zeros")
        if np.isinf(sc).any() and (np.abs(sc[~np.isnan(sc)]) == 2.0 ** 1021).any():
            seen.add("nonfinite")
        if m > CH and ok[:, CH - 1].any() and ok[:, CH].any():
            seen.add("boundary")
        f = P.flat(sc)
        vals = f[ok]
        if len(np.unique(vals)) < len(vals):
            seen.add("ties")
    if "one_best" in tabs:
        f, ok = P.flat(tabs["one_best"]), P.candidates(P.flat(tabs["one_best"]))
        assert all(_rank_of(f[i], ok[i], int(np.nanargmax(f[i]))) == 0 for i in range(N)) and len({int(np.nanargmax(f[i])) for i in range(N)}) == 1
        seen.add("one_best")
    if "neg_only" in tabs:
        f, ok = P.flat(tabs["neg_only"]), P.candidates(P.flat(tabs["neg_only"]))
        assert ok[0].sum() == 1 and f[0][ok[0]][0] < 0 and ok[:, ok[0]].sum() == 1
        assert _optimum_plan(tabs["neg_only"])[0] == np.flatnonzero(ok[0])[0]
        seen.add("neg_only")
    if "deep" in tabs:
        f, ok = P.flat(tabs["deep"]), P.candidates(P.flat(tabs["deep"]))
        j = int(_optimum_plan(tabs["deep"])[N - 1])
        assert j >= 0 and _rank_of(f[N - 1], ok[N - 1], j) == N - 1, (j, N)
        seen.add("deep")
    want = {"nan_slot", "signed_zeros", "nonfinite", "ties", "one_best", "neg_only"}
    want |= {(2, 1, 2): {"time_ordered_fewer"}, (8, 8, 5): {"fewer_objects_than_slots", "time_ordered_smaller"},
             (8, 8, 70): {"time_ordered_smaller", "time_ordered_fewer", "deep"}, (5, 3, 403): {"time_ordered_smaller", "deep"},
             (8, 8, 2003): {"time_ordered_smaller", "deep", "boundary"}, (64, 1, 130): {"time_ordered_smaller", "deep"},
             (3, 8, 30001): {"time_ordered_smaller", "deep", "boundary"}}[(H, S, m)]
    assert want <= seen, (want - seen, sorted(seen))
    return yard, seen


@pytest.mark.parametrize("H,S,m", SHAPES)
def test_synthetic_tables_are_planned_optimally(hip, H, S, m):
    """device.plan_sensors against scipy on dyadic tables, every column: a valid plan, the yardstick's count, its total exactly"""
    tabs = _tables(H, S, m, seed=100 + m)
    yard, _ = _situations(tabs, H, S, m)
    # ---- the device
    ws = hip.dev.plan_sensors_workspace(m, S, H, 1, "cuda")
    for name, sc in tabs.items():
        for col in range(3):
            rows, picks = _call(hip, _in_column(sc, col), col, ws)
            plan = P.check_plan(sc, rows, picks, S)
            got = (P.count(plan), P.total(sc, plan))
            print("[plan H=%d S=%d m=%d %s col=%d] device %s yardstick %s" % (H, S, m, name, col, got, yard[name]))
            assert got[0] == yard[name][0], (name, col, got, yard[name])
            assert got[1] == yard[name][1], (name, col, got, yard[name])
        # determinism: a second call on the same workspace gives the same bits
        again = _call(hip, _in_column(sc, col), col, ws)
        assert np.array_equal(rows, again[0]) and np.array_equal(picks, again[1]), name
    assert int(ws[0].item()) == 0                        # (the last workgroup to arrive left the ticket at zero)


@pytest.mark.parametrize("E,H,S,m", [(3, 4, 8, 513), (2, 8, 8, 1100)])
def test_every_env_is_planned_as_if_alone(hip, E, H, S, m):
    """each env's rows equal the n_env = 1 call on that env's strided slab copied contiguous; two envs given the same slab get the
    same rows"""
    rs = np.random.RandomState(E + m)
    sc = rs.randint(0, 40, size=(H, E, S, m, 3)).astype(np.float64) / 8.0          # (dyadic, with exact ties)
    sc[rs.uniform(size=sc.shape) < 0.6] = np.nan
    for same in (False, True):
        if same:
            sc[:, E - 1] = sc[:, 0]
        ws = hip.dev.plan_sensors_workspace(m, S, H, E, "cuda")
        ws1 = hip.dev.plan_sensors_workspace(m, S, H, 1, "cuda")
        for col in range(3):
            rows, picks = _call(hip, sc, col, ws)
            assert rows.shape == (H, E, W) and picks.shape == (H, E, W, 2)
            for e in range(E):
                one = _call(hip, sc[:, e], col, ws1)
                assert np.array_equal(rows[:, e], one[0]) and np.array_equal(picks[:, e], one[1]), (same, col, e)
                plan = P.check_plan(sc[:, e, :, :, col], rows[:, e], picks[:, e], S)
                assert (P.count(plan), P.total(sc[:, e, :, :, col], plan)) == P.best_dyadic(sc[:, e, :, :, col])
            if same:
                assert np.array_equal(rows[:, 0], rows[:, E - 1]) and np.array_equal(picks[:, 0], picks[:, E - 1])


@pytest.mark.parametrize("m", [5, 700, 2003])
def test_one_slot_is_the_first_maximum(hip, m):
    """N = 1 and finite scores: the first maximum (lowest j, -0.0 == 0.0), as for the greedy entry"""
    torch = hip.torch
    rs = np.random.RandomState(m)
    tabs = [rs.randint(-3, 4, size=m).astype(np.float64), np.where(rs.uniform(size=m) < 0.5, -0.0, 0.0), rs.normal(size=m), -np.abs(rs.normal(size=m)) - 1]
    tabs[1][0] = -0.0
    ws = hip.dev.plan_sensors_workspace(m, 1, 1, 1, "cuda")
    for v in tabs:
        sc = np.zeros((1, 1, m, 3))
        sc[0, 0, :, 2] = v
        rows, picks = _call(hip, sc, 2, ws)
        greedy = hip.dev.assign_sensors(torch.as_tensor(sc[0]).cuda(), 2).cpu().numpy()
        assert rows[0, 0] == int(np.argmax(v)) == greedy[0] and (rows[0, 1:] == -1).all(), (rows, int(np.argmax(v)), greedy)
        assert picks[0, 0, 0] == rows[0, 0] and picks[0, 0, 1] == v[rows[0, 0]:rows[0, 0] + 1].view(np.int64)[0]


# ---------------------------------------------------------------- real forecasts
MASKS_DEG = [15.0, 0.0, 30.0, 5.0, 20.0, -10.0, 10.0, 25.0]


def _forecast(hip, m, H, S, propagator):
    """the score tensor [H, S, m, 3] of a forecast from a prepared state (the state of tests/test_forecast_sensors_gpu.py)"""
    torch, host = hip.torch, hip.host
    xt, x, Pm, g = make_batch(m, seed=123)
    x[BAD, 1] = np.nan
    lla, lim = sites_rad()[:S], np.radians(MASKS_DEG[:S])
    sig = [np.array([(1.0 + k) * host.arcsec2rad, (0.5 + 2.0 * k) * host.arcsec2rad, 1e3 / (1 + k)]) for k in range(S)]
    Rs = [np.diag(s ** 2) for s in sig]
    sp = host.make_sensor_params(lla, lim, Rs, N_TIME * m * 3)
    consts = host.make_consts(g["Q"], Rs[0], 1e-4, 2.0, -3, 20.0, lim[0], lla[0], propagator=propagator)
    zn = torch.zeros((S, N_TIME, m, 3), dtype=torch.float64, device="cuda")
    eng = hip.engine.HotPathEngine(consts, m, 1, c2t()[:N_TIME], zn, history=2, zn_stride_env=0)
    eng.load_state(0, xt, x, Pm)
    fc = eng.launch_forecast_sensors(0, 1, sp, H)
    return eng, fc


def _best_rounded(sc):
    """(count, total) of the optimum of a table of multiples of 2^-10 of ANY magnitude below 2^36 (a forecast's trace gains reach
    3e10 m^2, where best_dyadic's shift of 2^30 no longer puts the count first and a larger one would push the sums past 2^43, the
    last power of two below which multiples of 2^-10 are exact): the count from maximum_bipartite_matching, and where every
    slot that has a candidate can be filled, linear_sum_assignment over those slots with the non-candidates at -inf
    (matching.best_full's form) IS the count-first optimum; its sums of at most 64 scores stay below 2^42: exact"""
    from scipy.optimize import linear_sum_assignment
    f = P.flat(sc)
    ok = P.candidates(f)
    rows, cols = np.flatnonzero(ok.any(axis=1)), np.flatnonzero(ok.any(axis=0))
    n = P.best_count(sc)
    if not n:
        return 0, 0.0
    if n != len(rows):                                   # (a slot that cannot be filled: the shift form, where it is exact)
        assert float(np.abs(f[ok]).max()) < 2.0 ** 10, "a slot stays empty and the scores are too large for best_dyadic"
        return P.best_dyadic(sc)
    sub, oks = f[np.ix_(rows, cols)], ok[np.ix_(rows, cols)]
    assert (sub[oks] * 1024 == np.round(sub[oks] * 1024)).all() and float(np.abs(sub[oks]).max()) < 2.0 ** 36
    r, c = linear_sum_assignment(np.where(oks, sub, -np.inf), maximize=True)
    assert oks[r, c].all() and len(r) == n
    return n, math.fsum(sub[r, c].tolist())


@pytest.mark.parametrize("propagator,S,m,H", [("hybrid", 3, 403, 8), ("fg", 8, 2003, 5), ("hybrid", 8, 2003, 5), ("fg", 3, 403, 8)])
def test_real_forecasts(hip, propagator, S, m, H):
    """on the forecast rounded to multiples of 2^-10 everything is exact; on the raw forecast the plan is valid, its count exact and its
    total within the header's bound of linear_sum_assignment's on the same doubles"""
    torch = hip.torch
    eng, fc = _forecast(hip, m, H, S, propagator)
    torch.cuda.synchronize()
    raw = fc["score"].cpu().numpy().copy()
    assert raw.shape == (H, S, m, 3) and np.isfinite(raw).any()
    rounded = np.round(raw * 1024.0) / 1024.0
    ws = hip.dev.plan_sensors_workspace(m, S, H, 1, "cuda")
    for col in range(3):
        # ---- rounded: exact
        sc = rounded[..., col]
        rows, picks = _call(hip, rounded, col, ws)
        plan = P.check_plan(sc, rows, picks, S)
        want = _best_rounded(sc)
        to = P.time_ordered(np.where(np.isfinite(sc), sc, np.nan))
        got = (P.count(plan), P.total(sc, plan))
        print("[plan %s S=%d m=%d H=%d col=%d rounded] device %s yardstick %s time-ordered %s"
              % (propagator, S, m, H, col, got, want, (P.count(to), P.total(sc, to))))
        assert got[0] == want[0] == P.best_count(sc) and got[1] == want[1], (col, got, want)
        assert got[0] >= P.count(to) and (got[0] > P.count(to) or got[1] >= P.total(sc, to)), (col, got)
        # ---- raw: valid, exact count, the total within the bound
        sc = raw[..., col]
        table = eng.launch_plan_sensors(fc, col)          # (the engine's own path on the forecast it holds)
        rows, picks = _call(hip, raw, col, ws)
        assert np.array_equal(table.cpu().numpy(), rows)
        plan = P.check_plan(sc, rows, picks, S)
        n = P.best_count(sc)
        assert P.count(plan) == n, (col, P.count(plan), n)
        yard, tol = P.best_total_doubles(sc, n), P.bound(sc)
        gap = yard - P.total(sc, plan)
        print("[plan %s S=%d m=%d H=%d col=%d raw] filled %d of %d, total %.17g, yardstick - total = %.3g, bound %.3g"
              % (propagator, S, m, H, col, n, H * S, P.total(sc, plan), gap, tol))
        assert gap <= tol, (col, gap, tol)


# ---------------------------------------------------------------- plumbing
def _np(r):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in r.items()}


def test_planners_against_the_device_entry_and_execution(hip, envs):
    """forecast -> plan -> rollout_sensors(plan) at 403 objects, 3 sites, H = 6: the planner's device part is the entry on the read-back
    forecast, the engine is untouched by planning, and every planned update that was taken leaves the forecast's P_post"""
    from ssa_gym_amd import _lib, agents
    torch = hip.torch
    env = envs.make('ssa_tasker_simple-v2', config=cfg8(envs, m=403, seed=5, history='full'))
    env.action_space.seed(3)
    rs = np.random.RandomState(6)
    for _ in range(2):
        env.step(_distinct(rs, env.m, 3))
    i, S = env.i, 3
    draws = env.np_random.get_state()[2]
    fc = _np(env.forecast_sensors(6, covariances=True))
    for planner, col in ((agents.plan_trace_gain_sensors_horizon, _lib.LOOK_TRACE_GAIN), (agents.plan_info_gain_sensors_horizon, _lib.LOOK_INFO_GAIN)):
        before = state_bytes(torch, env._engine)
        raw = agents._plan_horizon_assigned(env, 6, col)
        after = state_bytes(torch, env._engine)
        assert before.keys() == after.keys() and all(before[k] == after[k] for k in before), "planning wrote an engine tensor"
        rows = hip.dev.plan_sensors(torch.as_tensor(fc["score"]).cuda(), col).cpu().numpy()
        assert raw.shape == (6, S) and raw.dtype == np.int64 and np.array_equal(raw, rows[:, :S]) and (rows[:, S:] == -1).all()
        plan = planner(env, 6)
        assert plan.shape == (6, S) and plan.dtype == np.int64 and np.array_equal(plan[raw >= 0], raw[raw >= 0])
        assert len(set(plan.reshape(-1).tolist())) == plan.size and ((plan >= 0) & (plan < env.m)).all()      # (403 objects: nothing twice)
    assert env.np_random.get_state()[2] == draws
    env.rollout_sensors(plan)                                        # (the result as it comes)
    assert env.i == i + 6
    e = env._engine
    recs, status = e.upd_sensors.cpu().numpy(), e.status.cpu().numpy()
    taken = 0
    for h in range(6):
        for s in range(S):
            j, rec = int(plan[h, s]), recs[(i + h + 1) % e.H, s]
            assert rec[_lib.UPD_ACTION] == j and fc["visible"][h, s, j] == int(rec[_lib.UPD_VISIBLE]), (h, s, j)      # the booked visibility
            if raw[h, s] < 0:                                        # (a fill-in: nothing the sensor could have observed)
                assert not env.obs_taken[i + h + 1, s], (h, s, j)
                continue
            assert fc["status"][h, s, j] == _lib.ST_OK and rec[_lib.UPD_VISIBLE] == 1.0 and env.obs_taken[i + h + 1, s], (h, s, j)
            if status[j] == _lib.ST_UPDATE_NAN:                      # (depends on the drawn noise: not foreseen)
                continue
            assert np.array_equal(bits(env.P_filter[i + h + 1][j]), bits(fc["P_post"][h, s, j])), (h, s, j)
            taken += 1
    print("[horizon plan vs execution] %d planned updates taken and compared" % taken)
    assert taken >= 6


def test_vector_planners_equal_single_envs_and_execute(hip, envs):
    """E = 3: env e of a vector plan is a single env's plan from the same state; the plan runs with vec.rollout_sensors as it comes,
    and every planned update that was taken leaves the forecast's P_post"""
    from ssa_gym_amd import _lib, agents
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    torch = hip.torch
    cfg = cfg3(envs, m=16, steps=12, update_interval=1, sensor_obs_limit=[-89.0, -89.0, -89.0])
    E, S, m, H = 3, 3, 16, 4           # (16 objects for 12 slots: a fill-in is an object the plan does not hold, so it disturbs no forecast gain)
    vec, twin = SSA_Tasker_VecEnv(cfg, E, seed=10), SSA_Tasker_VecEnv(cfg, E, seed=10)
    twin._eng.z_noise.copy_(vec._eng.z_noise)
    singles = single_envs(envs, cfg, vec, 10)
    vec.single_action_space.seed(1)
    rs = np.random.RandomState(8)
    for _ in range(2):
        acts = np.stack([rs.permutation(m)[:S] for _ in range(E)])
        vec.step(acts)
        twin.step(acts)
        for e in range(E):
            singles[e].step(acts[e])
    states = [r.get_state()[2] for r in vec._rng]
    fc = _np({k: v for k, v in vec.forecast_sensors(H, covariances=True).items()})
    for planner, col in ((agents.plan_trace_gain_sensors_horizon, _lib.LOOK_TRACE_GAIN), (agents.plan_info_gain_sensors_horizon, _lib.LOOK_INFO_GAIN)):
        before = state_bytes(torch, vec._eng)
        raw = agents._plan_horizon_assigned(vec, H, col)
        after = state_bytes(torch, vec._eng)
        assert all(before[k] == after[k] for k in before), "planning wrote an engine tensor"
        assert raw.shape == (E, H, S) and raw.dtype == np.int64
        for e in range(E):
            one = agents._plan_horizon_assigned(singles[e], H, col)
            assert np.array_equal(raw[e], one), (col, e, raw[e], one)
            sc = fc["score"][e][..., col]
            got = raw[e][raw[e] >= 0]
            assert len(set(got.tolist())) == len(got) and P.count(raw[e]) == P.best_count(sc), (col, e, raw[e])
            assert all(np.isfinite(sc[h, s, raw[e, h, s]]) for h in range(H) for s in range(S) if raw[e, h, s] >= 0)
        plan = planner(vec, H)
        assert plan.shape == (E, H, S) and plan.dtype == np.int64 and np.array_equal(plan[raw >= 0], raw[raw >= 0])
        assert ((plan >= 0) & (plan < m)).all() and all(len(set(r.tolist())) == S for p in plan for r in p)
    assert states == [r.get_state()[2] for r in vec._rng]
    twin.rollout_sensors(plan)                                       # (the result as it comes)
    assert np.all(twin.i == 2 + H)
    taken = 0
    for h in range(H):
        _, _, done, _ = vec.step(plan[:, h])
        assert not done.any()
        status = vec._eng.status.cpu().numpy().reshape(E, m)
        for e in range(E):
            Pf = vec.P_filter(e)
            for s in range(S):
                j = int(raw[e, h, s])
                if j < 0:
                    continue
                assert fc["status"][e, h, s, j] == _lib.ST_OK and fc["visible"][e, h, s, j] == 1, (e, h, s, j)
                if status[e, j] != _lib.ST_OK:
                    continue
                assert np.array_equal(bits(Pf[j]), bits(fc["P_post"][e, h, s, j])), (e, h, s, j)
                taken += 1
    for e in range(E):
        assert np.array_equal(bits(vec.P_filter(e)), bits(twin.P_filter(e))), e
    print("[vector horizon plan vs execution] %d planned updates taken and compared" % taken)
    assert taken >= E * S
