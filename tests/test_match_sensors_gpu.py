"""A sensor network's OPTIMAL assignment on the device (include/ssa_hip.h: ssa_match_sensors_f64, ssa_match_sensors_envs_f64; DESIGN.md
section 8n) and everything that takes rule='optimal' on top of it, on the MI355X.

The exact part feeds DYADIC scores (multiples of 2^-10 below 2^10 in magnitude: every sum of eight is exact) and asks for the optimum
itself: the tasked-sensor count of scipy's maximum_bipartite_matching and the total of linear_sum_assignment, `math.fsum` against
`math.fsum`, no tolerance.  On real lookaheads the total may fall short of the yardstick's by the rounding of the sums the rule compares:
2 S (S - 1) u max|score| (support.matching.tolerance), derived, not measured.  The loops are compared bit for bit with the project's own
per-step paths fed the device's rows."""
import numpy as np
import pytest

from support import matching as M
from support.batches import c2t, make_batch
from support.gpu import envs, hip  # noqa: F401  (the module fixtures)
from support.sensors import BAD, N_TIME, _assert_same_env, _compare, _distinct, _same, cfg3, cfg8, sites_rad
from support.vector_lookahead import single_envs

pytestmark = pytest.mark.gpu

W, CH = M.W, M.CH
NEG0 = np.array(-0.0).view(np.int64).item()


# ---------------------------------------------------------------- synthetic, dyadic score tables
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


def _cases(S, m, seed):
    """named dyadic score columns [S, m] that hold the situations the tests assert they saw"""
    rs = np.random.RandomState(seed)
    out = {}

    def noise(lo=-5.0, hi=5.0, nan=0.3):
        a = _dy(rs.uniform(lo, hi, size=(S, m)))
        a[rs.uniform(size=(S, m)) < nan] = np.nan
        return a
    out["random"] = noise()
    ob = _spread(m, min(m, S + 2))
    if S > 1:
        a = noise(-5.0, -1.0)                            # sensor 0: 10, 9; sensor 1: 9.5, 0 -- greedy takes 10 + 0, the optimum 9 + 9.5
        a[:, ob[0]], a[:, ob[1]] = np.nan, np.nan
        a[0, ob[0]], a[0, ob[1]], a[1, ob[0]], a[1, ob[1]] = 10.0, 9.0, 9.5, 0.0
        out["greedy_smaller"] = a
        a = noise(-5.0, -1.0)                            # sensor 0: 5, 1; sensor 1: 4, nothing else -- greedy leaves sensor 1 idle
        a[:, ob[0]], a[:, ob[1]], a[1] = np.nan, np.nan, np.nan
        a[0, ob[0]], a[0, ob[1]], a[1, ob[0]] = 5.0, 1.0, 4.0
        out["greedy_fewer"] = a
    a = noise(nan=0.1)                                   # one object best for every sensor
    a[:, ob[0]] = 100.0 + _dy(rs.uniform(size=S))
    out["one_best"] = a
    a = noise()
    a[S - 1] = np.nan                                    # an all-NaN sensor
    out["nan_row"] = a
    if S >= 3:
        a = noise()
        a[0], a[S - 1] = np.nan, np.nan                  # two sensors left without an object: the fallback draws can collide
        out["two_nan_rows"] = a
    a = np.full((S, m), np.nan)                          # fewer candidates than sensors
    for j in (_spread(m, S - 1) if S > 1 else []):
        a[:, j] = _dy(rs.uniform(0, 1, size=S))
    out["few"] = a
    a = noise(0.0, 5.0)                                  # a sensor whose only candidate is negative (and nobody else's)
    a[0], a[:, ob[0]] = np.nan, np.nan
    a[0, ob[0]] = -3.5
    out["neg_only"] = a
    a = np.where(rs.uniform(size=(S, m)) < 0.5, -0.0, 0.0)      # -0.0 against 0.0: one value
    a[rs.uniform(size=(S, m)) < 0.3] = -1.0
    a[:, 0] = -0.0
    out["signed_zeros"] = a
    a = noise()                                          # +inf, -inf and 2^1021: values to the greedy rule, nothing to the optimal one
    for k, j in enumerate(_spread(m, min(m, 3 * S))):
        a[k % S, j] = (np.inf, 2.0 ** 1021, -np.inf, -2.0 ** 1021)[k % 4]
    out["nonfinite"] = a
    a = rs.randint(0, 3, size=(S, m)).astype(np.float64)       # exact ties across sensors and chunk boundaries
    a[rs.uniform(size=(S, m)) < 0.2] = np.nan
    for j in _spread(m, min(m, 6)):
        a[:, j] = 7.0
    out["ties"] = a
    if S >= 2 and m > CH:                                # the optimum's objects on both sides of a chunk boundary
        a = noise()
        a[0, CH - 1], a[1, CH] = 50.0, 60.0
        out["boundary"] = a
    if 2 <= S <= m:
        # sensor S-1's S-1 best objects are each worth far more to another sensor: the optimum gives it its S-th candidate
        a = noise(lo=0.0, hi=1.0, nan=0.1)
        obj = _spread(m, S)
        for t in range(S - 1):
            a[t, obj[t]] = 1000.0 - t
            a[S - 1, obj[t]] = 100.0 - t
        a[S - 1, obj[S - 1]] = 50.0
        out["deep"] = a
    return out


def _fallbacks(S, m, base, rs):
    """fallback rows for a column whose assignment is `base`: NULL, random draws, out of range, duplicated, colliding, usable"""
    free = [j for j in rs.permutation(m).tolist() if j not in base][:W]
    out = {"null": None, "random": rs.randint(0, m, size=W), "oor": np.array([-1, m, m + 7, -2 ** 31, 2 ** 31 - 1, -5, m, m + 1])}
    if free:
        out["dup"] = np.full(W, free[0])
    if (base >= 0).any():
        out["collide"] = np.resize(base[base >= 0], W)
    if len(free) >= S:
        out["distinct"] = np.resize(np.asarray(free), W)
    return {k: (None if v is None else np.asarray(v, dtype=np.int64).astype(np.int32)) for k, v in out.items()}


def _rank_of(row, ok, j):
    """position of object j in its sensor's own order (value descending, index ascending) among the candidates"""
    v = row[j]
    return int(np.sum(ok & (row > v)) + np.sum(ok[:j] & (row[:j] == v)))


def _call(dev, torch, score, col, fb, ws, rule="optimal"):
    row = torch.full((W,), -7, dtype=torch.int32, device="cuda")
    picks = torch.full((W, 2), -7, dtype=torch.int64, device="cuda")
    got = dev.assign_sensors(score, col, fallback=None if fb is None else torch.as_tensor(fb).cuda(), out=row, picks=picks, workspace=ws,
                             rule=rule)
    assert got is row
    return row.cpu().numpy(), picks.cpu().numpy()


@pytest.mark.parametrize("m", [5, 2003, 30001])
@pytest.mark.parametrize("S", [1, 3, 8])
def test_synthetic_scores_are_assigned_optimally(hip, S, m):
    """device.assign_sensors(rule='optimal') against scipy on dyadic tables: one chunk, many chunks, a ragged tail, more than the 32 768
    objects phase 2 holds in registers; every column; every fallback flavour; the picks; greedy calls in between -- all on ONE workspace,
    zeroed once"""
    torch, dev = hip.torch, hip.dev
    cases = [_cases(S, m, 100 * S + c) for c in range(3)]
    ws = dev.assign_sensors_workspace(m, S, "cuda")
    rs = np.random.RandomState(S + m)
    seen, n_calls = set(), 0
    for name in cases[0]:
        host = np.stack([cases[c][name] for c in range(3)], axis=2)      # [S, m, 3]
        score = torch.as_tensor(host).cuda()
        for col in range(3):
            sc = host[:, :, col]
            ok = M.candidates(sc)
            count, best = M.best_dyadic(sc)
            assert count == M.best_count(sc), (name, col)                # (the two yardsticks agree on the count)
            r0, p0 = _call(dev, torch, score, col, None, ws)
            base = M.check_row(sc, r0, p0, S, m)
            # ---- a greedy call on the same workspace in between, then the same optimal call again: the same row
            g_row, g_picks = _call(dev, torch, score, col, None, ws, rule="greedy")
            greedy = M.greedy_np(sc)
            assert np.array_equal(g_row[:S], greedy) and np.array_equal(g_picks[:S, 0], greedy), (name, col)
            r1, p1 = _call(dev, torch, score, col, None, ws)
            assert np.array_equal(r0, r1) and np.array_equal(p0, p1), (name, col)
            n_calls += 3
            if S == 1 and name != "nonfinite":                           # (finite scores: the greedy row, bit for bit)
                assert np.array_equal(r0, g_row) and np.array_equal(p0, g_picks), (name, col)
            # ---- what this input holds
            g_ok = np.array([j >= 0 and ok[s, j] for s, j in enumerate(greedy)])
            if (greedy >= 0).sum() < count:
                seen.add("greedy_fewer")
            elif g_ok.all() and (greedy >= 0).sum() == count and M.total(sc, greedy) < best:
                seen.add("greedy_smaller")
            if ((greedy >= 0) & ~g_ok).any():
                seen.add("greedy_takes_nonfinite")
                assert (np.isinf(sc) | (np.abs(np.nan_to_num(sc)) > M.BOUND)).any()
            if (~ok).all(axis=1).any():
                seen.add("nan_row")
            if ok.any(axis=0).sum() < S:
                seen.add("few")
            tops = [int(np.argmax(np.where(ok[s], sc[s], -np.inf))) for s in range(S) if ok[s].any()]
            if S > 1 and len(tops) == S and len(set(tops)) == 1:
                seen.add("one_best")
            for s in range(S):
                if base[s] >= 0 and ok[s].sum() == 1 and sc[s, base[s]] < 0:
                    seen.add("neg_only")
                if base[s] >= 0 and p0[s, 1] == NEG0:
                    seen.add("neg_zero")
                if S > 1 and base[s] >= 0 and _rank_of(sc[s], ok[s], base[s]) == S - 1:
                    seen.add("deep")
            if CH - 1 in base and CH in base:
                seen.add("boundary")
            vals = sc[ok]
            if len(vals) and (vals == vals.max()).sum() > 1 and len(set(np.where(ok & (sc == vals.max()))[0].tolist())) > 1:
                seen.add("ties")
            for fname, fb in _fallbacks(S, m, base, rs).items():
                r, p = _call(dev, torch, score, col, fb, ws)
                n_calls += 1
                assigned = M.check_row(sc, r, p, S, m, fb)               # valid, the picks' bits, the fallback outcome
                assert np.array_equal(assigned, base) and np.array_equal(p, p0), (name, col, fname)      # a pure function of the scores
                assert (assigned >= 0).sum() == count, (name, col, fname, assigned, count)
                assert M.total(sc, assigned) == best, (name, col, fname, assigned, M.total(sc, assigned), best)
                want = r[:S]
                idle = want < 0
                if fb is None:
                    seen.add("fb_null")
                    assert np.array_equal(want, base)
                elif fname == "oor" and (base < 0).any():
                    seen.add("fb_oor")
                    assert np.array_equal(want, base)
                elif fname == "dup" and (base < 0).sum() >= 2:
                    seen.add("fb_dup")
                    assert (want == fb[0]).sum() == 1 and idle.sum() == (base < 0).sum() - 1
                elif fname == "collide" and (base < 0).any():
                    seen.add("fb_collide")
                    assert np.array_equal(want, base)
                elif fname == "distinct" and (base < 0).any():
                    seen.add("fb_taken")
                    assert not idle.any()
    assert n_calls > 2 and int(ws[0].item()) == 0                        # the last arrival left the ticket at zero every time
    out = dev.assign_sensors(score, 0, rule="optimal")                   # the defaults: a fresh row, a fresh workspace, no fallback
    assert out.dtype == torch.int32 and tuple(out.shape) == (W,)
    need = {"nan_row", "few", "neg_only", "neg_zero", "greedy_takes_nonfinite", "fb_null", "fb_oor"}
    if S > 1:
        need |= {"one_best", "ties", "fb_collide"}
    if S > 1 and m >= 2 * S:        # (per S: where the objects outnumber the sensors, so that the built cases stand alone)
        need |= {"greedy_smaller", "greedy_fewer"}
    if 2 <= S <= m:
        need |= {"deep"}
    if m >= 2 * S:
        need |= {"fb_taken"} | ({"fb_dup"} if S >= 3 else set())
    if S >= 2 and m > CH:
        need |= {"boundary"}
    print("[match synthetic] S=%d m=%d: %d calls, seen %s" % (S, m, n_calls, sorted(seen)))
    assert seen >= need, need - seen


@pytest.mark.parametrize("E,S,m", [(1, 3, 8), (3, 8, 513), (9, 3, 1100), (2, 8, 33000)])
def test_envs_entry_equals_the_one_env_entry_on_each_slab(hip, E, S, m):
    """device.assign_sensors_envs(rule='optimal') against device.assign_sensors(rule='optimal') on every env's slab: rows and picks
    identical, with fallback rows; a greedy call on the same workspace in between"""
    torch, dev = hip.torch, hip.dev
    rs = np.random.RandomState(7 * E + S)
    host = _dy(rs.uniform(-5, 5, size=(E, S, m, 3)))
    host[rs.uniform(size=host.shape) < 0.4] = np.nan
    host[0, S - 1] = np.nan                                               # an idle sensor in env 0: its fallback word counts
    host[E - 1, :, :, 1] = np.where(rs.uniform(size=(S, m)) < 0.5, 1.0, np.nan)      # ties everywhere
    host[E - 1, 0, m - 1, 2] = np.inf
    score = torch.as_tensor(host).cuda()
    fb = rs.randint(-2, m + 2, size=(E, W)).astype(np.int32)
    ws = dev.assign_sensors_envs_workspace(m, S, E, "cuda")
    ws1 = dev.assign_sensors_workspace(m, S, "cuda")
    for col in range(3):
        for f in (None, fb):
            table = torch.full((E, W), -7, dtype=torch.int32, device="cuda")
            picks = torch.full((E, W, 2), -7, dtype=torch.int64, device="cuda")
            dev.assign_sensors_envs(score, col, fallback=None if f is None else torch.as_tensor(f).cuda(), out=table, picks=picks,
                                    workspace=ws, rule="optimal")
            dev.assign_sensors_envs(score, col, workspace=ws)             # (greedy, same workspace)
            t, p = table.cpu().numpy(), picks.cpu().numpy()
            for e in range(E):
                r1, p1 = _call(dev, torch, score[e], col, None if f is None else f[e], ws1)
                assert np.array_equal(t[e], r1) and np.array_equal(p[e], p1), (col, e, t[e], r1)
                M.check_row(host[e, :, :, col], t[e], p[e], S, m, None if f is None else f[e])
    assert not ws.view(-1)[::ws.numel() // E].cpu().numpy().any()          # every env's ticket is back at zero


# ---------------------------------------------------------------- real lookaheads
@pytest.mark.parametrize("propagator,sensors,regime", [("hybrid", 3, False), ("fg", 8, False), ("hybrid", 8, True)])
def test_real_lookaheads_within_the_derived_tolerance(envs, propagator, sensors, regime):
    """the engine advanced by step(); launch_assign_sensors(rule='optimal') on the scores launch_lookahead_sensors leaves, both agent
    columns -- also under a storage layout.  Every sensor has at least S candidates (asserted), so every sensor is tasked; the total is
    within 2 S (S - 1) u max|score| of linear_sum_assignment's on the full matrix, and not below the greedy row's by more than that."""
    import torch
    from ssa_gym_amd import _lib
    # (an open sky: with the masks of cfg8, and still with masks at the horizon, one site sees fewer than S of the 2 000 objects)
    over = dict(propagator=propagator, storage_layout='regime' if regime else None, sensor_obs_limit=[-89.0] * sensors)
    env = envs.make('ssa_tasker_simple-v2', config=cfg8(envs, sensors=sensors, **over))
    e, S = env._engine, env.n_sensor
    assert (e._order is not None) == regime and S == sensors
    rs = np.random.RandomState(31)
    gaps, beats = [], 0
    for k in range(12):
        env.step(_distinct(rs, env.m, S))
        if k % 3:
            continue
        i = env.i
        look = e.launch_lookahead_sensors(i % e.H, i + 1, env._sites())
        host = look["score"].cpu().numpy()
        for col in (_lib.LOOK_INFO_GAIN, _lib.LOOK_TRACE_GAIN):
            sc = host[:, :, col]
            assert (M.candidates(sc).sum(axis=1) >= S).all(), (k, col)
            fb = rs.randint(0, env.m, size=W).astype(np.int32)
            rows = {}
            for rule in ("optimal", "greedy"):
                row = torch.full((W,), -7, dtype=torch.int32, device="cuda")
                picks = torch.full((W, 2), -7, dtype=torch.int64, device="cuda")
                e.launch_assign_sensors(look, col, row, fallback_row=torch.as_tensor(fb).cuda(), picks=picks, rule=rule)
                rows[rule] = (row.cpu().numpy(), picks.cpu().numpy())
            assigned = M.check_row(sc, rows["optimal"][0], rows["optimal"][1], S, env.m, fb)
            assert (assigned >= 0).all(), (k, col, assigned)
            tol, best, got = M.tolerance(sc, S), M.best_full(sc), M.total(sc, assigned)
            greedy = M.total(sc, rows["greedy"][1][:S, 0])
            gaps.append((best - got) / max(tol, 1e-300))
            beats += got > greedy
            print("[match real] %s S=%d k=%d col=%d: optimal %.17g  yardstick %.17g  greedy %.17g  tol %.3g" % (propagator, S, k, col, got,
                                                                                                            best, greedy, tol))
            assert got >= best - tol, (k, col, got, best, tol)
            assert got >= greedy - tol, (k, col, got, greedy, tol)
    print("[match real] largest (yardstick - device) / tolerance: %.3g; beat greedy in %d of %d" % (max(gaps), beats, len(gaps)))
    assert e._assign_ws[0] == S and int(e._assign_ws[1][0].item()) == 0


# ---------------------------------------------------------------- the engine loop
TIGHT = 1         # the site whose elevation mask nothing clears: its sensor is idle at every step


def _net_tight(host, S, stride):
    lla = sites_rad()[:S]
    lim = np.radians([15.0, 89.9, 30.0, 0.0, 5.0, -10.0, 20.0, -30.0][:S])
    sig = [np.array([(1.0 + k) * host.arcsec2rad, (0.5 + 2.0 * k) * host.arcsec2rad, 1e3 / (1 + k)]) for k in range(S)]
    Rs = [np.diag(s ** 2) for s in sig]
    return lla, lim, Rs, sig, host.make_sensor_params(lla, lim, Rs, stride)


@pytest.mark.parametrize("S,m,K,H", [(3, 2003, 7, 8), (8, 403, 9, 4)])
def test_engine_loop_equals_the_host_loop(hip, S, m, K, H):
    """K steps of lookahead + launch_assign_sensors(rule='optimal') + a one-row launch_rollout_sensors with no host sync, against the
    loop that reads every row back and calls launch_step_sensors: the state bit for bit"""
    torch, L, host = hip.torch, hip.lib, hip.host
    xt, x, P, g = make_batch(m, seed=123)
    x[BAD, 1] = np.nan
    trans = c2t()[:N_TIME]
    lla, lim, Rs, sig, sp = _net_tight(host, S, N_TIME * m * 3)
    consts = host.make_consts(g["Q"], Rs[0], 1e-4, 2.0, -3, 20.0, lim[0], lla[0], propagator="hybrid")
    gen = torch.Generator(device="cuda").manual_seed(8)
    zn = torch.randn((S, N_TIME, m, 3), dtype=torch.float64, device="cuda", generator=gen) * \
        torch.as_tensor(np.stack(sig), device="cuda").view(S, 1, 1, 3)
    col = L.LOOK_INFO_GAIN
    outs, rows_of = [], []
    for mode in ("steps", "loop"):
        eng = hip.engine.HotPathEngine(consts, m, 1, trans, zn, history=H, zn_stride_env=0)
        eng.load_state(0, xt, x, P)
        log = torch.full((K, W), -7, dtype=torch.int32, device="cuda")
        if mode == "steps":
            upd = torch.zeros((H, S, L.UPD_STRIDE), dtype=torch.float64, device="cuda")
            for k in range(K):
                look = eng.launch_lookahead_sensors(k % H, 1 + k, sp)
                eng.launch_assign_sensors(look, col, log[k], rule="optimal")
                row = log[k].cpu().numpy()                                # the host in the loop
                sc = look["score"].cpu().numpy()[:, :, col]
                assert (row[S:] == -1).all() and (row[:S] >= 0).sum() == M.best_count(sc), (k, row)
                eng.launch_step_sensors(k % H, (k + 1) % H, 1 + k, sp, [int(a) for a in row[:S]], upd[(k + 1) % H].data_ptr(),
                                        fast_stats=True, argmax_spos=True)
        else:
            for k in range(K):
                look = eng.launch_lookahead_sensors(k % H, 1 + k, sp)
                eng.launch_assign_sensors(look, col, log[k], rule="optimal")
                eng.launch_rollout_sensors(k % H, 1 + k, sp, log[k:k + 1], argmax_spos=True)
            upd = eng.upd_sensors
        torch.cuda.synchronize()
        out = {k: getattr(eng, k).cpu().numpy() for k in ("x_true", "x_filter", "P_filter", "obs", "metrics", "status", "stats")}
        out["upd"] = upd.cpu().numpy()
        out["fail_count"] = int(eng.fail_count.cpu().numpy()[0])
        out["fail_log"] = eng.fail_log[:out["fail_count"]].copy()
        out["shards"] = eng._roll_shards.cpu().numpy() if mode == "loop" else None
        outs.append(out)
        rows_of.append(log.cpu().numpy())
    assert np.array_equal(rows_of[0], rows_of[1])
    rows = rows_of[0][:, :S]
    assert (rows[:, TIGHT] == -1).all() and (rows[:, 0] >= 0).all()        # an idle sensor at every step; the others work
    assert all(len(set(r[r >= 0].tolist())) == (r >= 0).sum() for r in rows)
    _compare(L, outs[0], outs[1], K, H, True)


# ---------------------------------------------------------------- the env
def _row_on_device(env, col, fb_row, rule="optimal"):
    """the device's row for the env's next step, from the env's own lookahead and the given fallback row"""
    import torch
    from ssa_gym_amd import _lib, device
    S = env.n_sensor
    sc = env.lookahead_sensors()["score"].permute(0, 2, 1).contiguous()
    fbd = torch.full((_lib.MAX_SENSORS,), -1, dtype=torch.int32, device="cuda")
    fbd[:S] = torch.as_tensor(np.asarray(fb_row).astype(np.int32))
    return device.assign_sensors(sc, col, fallback=fbd, rule=rule).cpu().numpy()[:S].astype(np.int64)


@pytest.mark.parametrize("reward_type,obs_returned", [("trinary", "flatten"), ("shaped", "aer")])
def test_env_run_agent_sensors_optimal_equals_a_step_loop(envs, reward_type, obs_returned):
    """env.run_agent_sensors('agent_info_gain_sensors_optimal') against a twin env that steps the device's optimal rows (the same
    fallback rows) through step(): a chunk boundary inside (K > H - 1)"""
    from ssa_gym_amd import _lib, agents
    over = dict(steps=48, history=16, reward_type=reward_type, obs_returned=obs_returned)
    a = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, **over))
    b = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, **over))
    S, col, n_steps = b.n_sensor, _lib.LOOK_INFO_GAIN, 25
    assert b._engine.H == 16 and type(b).SENSOR_AGENT_RULES["agent_info_gain_sensors_optimal"] == (col, "optimal")
    for env in (a, b):
        for row in (_distinct(np.random.RandomState(5), env.m, S) for _ in range(2)):
            env.step(row)
    rs = np.random.RandomState(41)
    fb = np.stack([_distinct(rs, a.m, S) for _ in range(n_steps + 1)])
    obs_a, acts, rewards, dones = None, [], [], []
    for k in range(n_steps):
        if a.i + 1 >= a.n:
            break
        row = _row_on_device(a, col, fb[k])
        assert (row >= 0).all() and len(set(row.tolist())) == S, (k, row)           # complete: step() can express it
        obs_a, r, d, _ = a.step(row)
        acts.append(row)
        rewards.append(r)
        dones.append(d)
        if d:
            break
    agent = agents.agent_info_gain_sensors_optimal if reward_type == "trinary" else "agent_info_gain_sensors_optimal"
    obs_b, act_b, rew_b, don_b = b.run_agent_sensors(agent, n_steps, fallback_actions=fb)
    assert act_b.shape == (len(rewards), S) and _same(np.asarray(acts), act_b), (acts, act_b)
    assert _same(np.asarray(rewards), rew_b) and _same(np.asarray(dones, dtype=bool), don_b) and _same(np.array(obs_a), obs_b)
    _assert_same_env(a, b, "run_agent_sensors, optimal")
    assert len(rewards) > b._engine.H - 1 or dones[-1]                              # (the chunk boundary lay inside the run)
    # the host agent of the same name decides the same row for the next step (no fallback needed: every sensor is tasked)
    if not dones[-1]:
        want = _row_on_device(a, col, [-1] * S)
        if (want >= 0).all():
            assert np.array_equal(np.asarray(agents.agent_info_gain_sensors_optimal(None, b)), want)


@pytest.mark.parametrize("agent,mode,reward", [("agent_info_gain_sensors_optimal", "flatten", "trinary"),
                                               ("agent_trace_gain_sensors_optimal", "aer", "shaped")])
def test_step_agent_optimal_equals_single_envs_stepped_with_the_device_rows(envs, agent, mode, reward):
    """vec.step_agent with the new agents, E = 3, m = 8, S = 3, ten steps, against single envs stepped with
    device.assign_sensors(rule='optimal') rows"""
    from ssa_gym_amd import agents
    from ssa_gym_amd.envs.vector_env import SENSOR_AGENT_RULES, SSA_Tasker_VecEnv
    cfg = cfg3(envs, m=8, steps=12, update_interval=1, obs_returned=mode, reward_type=reward,
               **(dict(sensor_obs_limit=[-89.0, -89.0, -89.0]) if reward == "trinary" else {}))
    E, S, m = 3, 3, 8
    vec = SSA_Tasker_VecEnv(cfg, E, seed=10)
    singles = single_envs(envs, cfg, vec, 10)
    col, rule = SENSOR_AGENT_RULES[agent]
    assert rule == "optimal"
    rs = np.random.RandomState(4)
    live, compared = list(range(E)), 0
    for k in range(1, 11):
        fb = np.stack([rs.permutation(m)[:S] for _ in range(E)])
        want = {}
        for e in live:      # the yardstick's rows, from the single envs' own lookaheads, before anything steps
            for _ in range(50):
                want[e] = _row_on_device(singles[e], col, fb[e])
                if (want[e] >= 0).all():
                    break
                fb[e] = rs.permutation(m)[:S]
            assert (want[e] >= 0).all() and len(set(want[e].tolist())) == S, (k, e, want[e])
        obs, rew, done, infos = vec.step_agent(getattr(agents, agent) if k % 2 else agent, fallback_actions=fb)
        for e in list(live):
            row = infos[e]['action']
            assert row.dtype == np.int64 and np.array_equal(row, want[e]), (k, e, row, want[e])
            compared += 1
            o1, r1, d1, _ = singles[e].step(row)
            assert rew[e] == r1 and bool(done[e]) == bool(d1), (k, e, rew[e], r1)
            got = obs[e]
            if done[e]:
                got = infos[e]['terminal_observation']
                live.remove(e)
            assert np.array_equal(got.view(np.int64), np.asarray(o1).reshape(-1).view(np.int64)), (k, e)
            if not done[e]:
                for nme in ("x_true", "x_filter", "P_filter"):
                    u, v = getattr(vec, nme)(e), getattr(singles[e], nme)[k]
                    assert np.array_equal(u.view(np.int64), np.asarray(v).view(np.int64)), (k, e, nme)
    assert compared >= (10 * E if reward == 'trinary' else E)
    if live:                # the host agents of a vector env: [E, S], every live env's row the device's
        rows = getattr(agents, agent)(None, vec)
        assert rows.shape == (E, S) and all(len(set(r.tolist())) == S for r in rows)


# ---------------------------------------------------------------- the planners
def _check_plan_step(dev, torch, slab, row, S, m):
    """one step of a plan: `row` [S] (-1: none) for the masked slab [S, m] -- the optimal count, the total within the tolerance; and the
    slab rounded to 2^-10 through the device, exactly optimal"""
    ok = M.candidates(slab)
    for s, j in enumerate(row):
        assert j < 0 or ok[s, j], (s, j)
    assert (row >= 0).sum() == M.best_count(slab), (row, M.best_count(slab))
    if (ok.sum(axis=1) >= S).all():
        assert M.total(slab, row) >= M.best_full(slab) - M.tolerance(slab, S), row
    if not ok.any():            # (everything visible is planned already: nothing to assign, and `row` says so)
        return
    dy = _dy(slab)
    assert np.nanmax(np.abs(dy)) < 2.0 ** 10
    three = np.repeat(dy[:, :, None], 3, axis=2)
    got = dev.assign_sensors(torch.as_tensor(three).cuda(), 1, rule="optimal").cpu().numpy()[:S].astype(np.int64)
    count, best = M.best_dyadic(dy)
    assert (got >= 0).sum() == count and M.total(dy, got) == best, (got, count, best)
    assert len(set(got[got >= 0].tolist())) == (got >= 0).sum()


def test_plans_with_the_optimal_rule(envs, hip):
    """plan_info_gain_sensors(env, 4, rule='optimal') for a single env and a vector env: no object twice per plan and env, each step's
    row optimal for the slab without the objects planned before it"""
    from ssa_gym_amd import _lib, agents
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    torch, dev = hip.torch, hip.dev
    col = _lib.LOOK_INFO_GAIN
    # ---- a single env
    env = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, steps=48, history=16))
    S, m = env.n_sensor, env.m
    rs = np.random.RandomState(3)
    for _ in range(3):
        env.step(_distinct(rs, m, S))
    raw = agents._plan_assigned(env, 4, col, "optimal")
    score = env.forecast_sensors(4)["score"].cpu().numpy()                # [H', S, m, 3]
    assert raw.shape == (4, S) and score.shape == (4, S, m, 3)
    planned = []
    for h in range(4):
        slab = score[h, :, :, col].copy()
        slab[:, planned] = np.nan
        _check_plan_step(dev, torch, slab, raw[h], S, m)
        planned += raw[h][raw[h] >= 0].tolist()
    assert len(planned) == len(set(planned)) and len(planned) >= S
    plan = agents.plan_info_gain_sensors(env, 4, rule="optimal")
    assert plan.shape == (4, S) and np.array_equal(plan[raw >= 0], raw[raw >= 0]) and (plan >= 0).all()
    assert all(len(set(r.tolist())) == S for r in plan)
    raw_g = agents._plan_assigned(env, 4, col)                            # (the default is the greedy plan, as before)
    assert np.array_equal(agents.plan_info_gain_sensors(env, 4)[raw_g >= 0], raw_g[raw_g >= 0])
    assert env.i == 3
    # ---- a vector env
    E, S, m = 3, 3, 8
    vec = SSA_Tasker_VecEnv(cfg3(envs, m=m, steps=12, update_interval=1, sensor_obs_limit=[-89.0, -89.0, -89.0]), E, seed=10)
    vec.step(np.stack([rs.permutation(m)[:S] for _ in range(E)]))
    raw = agents._plan_assigned(vec, 4, col, "optimal")              # [E, H', S]
    score = vec._launch_forecast_sensors(4)["score"]
    torch.cuda.synchronize()
    score = score.cpu().numpy()                                           # [H', E, S, m, 3]
    assert raw.shape == (E, 4, S)
    for e in range(E):
        planned = []
        for h in range(4):
            slab = score[h, e, :, :, col].copy()
            slab[:, planned] = np.nan
            _check_plan_step(dev, torch, slab, raw[e, h], S, m)
            planned += raw[e, h][raw[e, h] >= 0].tolist()
        assert len(planned) == len(set(planned))
    plan = agents.plan_info_gain_sensors(vec, 4, rule="optimal")
    assert plan.shape == (E, 4, S) and np.array_equal(plan[raw >= 0], raw[raw >= 0])
    assert all(len(set(r.tolist())) == S for p in plan for r in p)
    assert np.all(vec.i == 1)
