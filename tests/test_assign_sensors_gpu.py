"""A sensor network's tasking assignment on the device and the closed loop on top of it (include/ssa_hip.h: ssa_assign_sensors_f64;
device.assign_sensors, HotPathEngine.launch_assign_sensors, SSA_Tasker_Env.run_agent_sensors) on the MI355X.

Everything is exact: there is no tolerance anywhere.  The yardstick of the assignment is `_assign_np`, a numpy restatement of the rounds
of agents._assign_lookahead_sensors (the largest non-NaN score of the column assigns its object to its sensor, ties to the lowest
s * m + j, the sensor's row and the object's column leave) plus the fallback rule of the header; it is cross-checked against repeated
device.masked_argmax calls on the same tensor, the rounds the host agent used to make.  The yardstick of the loops is the project's own
per-step path: the row read back (or the yardstick's row) followed by launch_step_sensors / step()."""
import numpy as np
import pytest

from support.batches import c2t, make_batch
from support.gpu import envs, hip  # noqa: F401  (the module fixtures)
from support.sensors import BAD, N_TIME, _assert_same_env, _compare, _distinct, _same, cfg3, cfg8, sites_rad

pytestmark = pytest.mark.gpu

W = 8                 # SSA_MAX_SENSORS: the width of an action row
CH = 512              # objects per workgroup of the kernel: what "a chunk boundary" means below
NEG0 = np.array(-0.0).view(np.int64).item()


# ---------------------------------------------------------------- the yardstick
def _assign_np(sc, fallback=None):
    """(actions [S], assigned [S], bits [S]) for a score column sc [S, m]: the greedy rounds, then the fallback rule"""
    sc = np.asarray(sc, dtype=np.float64)
    S, m = sc.shape
    assigned, bits = np.full(S, -1, dtype=np.int64), np.zeros(S, dtype=np.int64)
    alive = ~np.isnan(sc)
    for _ in range(S):
        idx = np.flatnonzero(alive.reshape(-1))
        if not len(idx):
            break
        f = int(idx[np.argmax(sc.reshape(-1)[idx])])        # (np.argmax: the first maximum, compared by value)
        s, j = divmod(f, m)
        assigned[s], bits[s] = j, sc[s, j:j + 1].view(np.int64)[0]
        alive[s], alive[:, j] = False, False
    act = assigned.copy()
    if fallback is not None:
        for s in range(S):
            f = int(fallback[s])
            if act[s] < 0 and 0 <= f < m and f not in act[act >= 0]:
                act[s] = f
    return act, assigned, bits


def _assign_by_masked_argmax(dev, torch, score, col):
    """the rounds as agents._assign_lookahead_sensors made them: one device.masked_argmax per sensor over the [S][m][3] tensor itself"""
    S, m = score.shape[0], score.shape[1]
    flat = score.reshape(-1)
    mask = torch.zeros(flat.shape[0], dtype=torch.uint8, device="cuda")
    mask[col::3] = 1
    rows = mask.view(S, m, 3)
    act = np.full(S, -1, dtype=np.int64)
    for _ in range(S):
        f = dev.masked_argmax(flat, mask)
        if f < 0:
            break
        s, j = divmod(f // 3, m)
        act[s] = j
        rows[s] = 0
        rows[:, j] = 0
    return act


def _rank_of(row, j):
    """position of object j in its sensor's own order (value descending, index ascending) among the non-NaN entries"""
    v = row[j]
    ok = ~np.isnan(row)
    return int(np.sum(ok & (row > v)) + np.sum(ok[:j] & (row[:j] == v)))


# ---------------------------------------------------------------- synthetic score tensors
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
    """named score columns [S, m] that hold the situations the issue lists (each is asserted where it is built or in the test)"""
    rs = np.random.RandomState(seed)
    out = {}

    def noise(lo=-5.0, hi=5.0, nan=0.3):
        a = rs.uniform(lo, hi, size=(S, m))
        a[rs.uniform(size=(S, m)) < nan] = np.nan
        return a
    out["random"] = noise()
    a = noise()
    a[S - 1] = np.nan                                   # all-NaN rows for one sensor
    out["nan_row"] = a
    if S >= 3:
        a = noise()
        a[0], a[S - 1] = np.nan, np.nan                 # two sensors left without an object: the fallback draws can collide
        out["two_nan_rows"] = a
    a = np.full((S, m), np.nan)                         # fewer non-NaN objects than sensors
    for j in _spread(m, S - 1):
        a[:, j] = rs.uniform(0, 1, size=S)
    out["few"] = a
    a = noise(nan=0.1)                                  # one object best for every sensor
    jb = _spread(m, 1)[0]
    a[:, jb] = 100.0 + rs.uniform(size=S)
    assert (np.nanargmax(a, axis=1) == jb).all()
    out["one_best"] = a
    a = rs.randint(0, 3, size=(S, m)).astype(np.float64)      # exact ties across sensors and across chunk boundaries
    a[rs.uniform(size=(S, m)) < 0.2] = np.nan
    for j in _spread(m, min(m, 6)):
        a[:, j] = 7.0
    out["ties"] = a
    a = np.where(rs.uniform(size=(S, m)) < 0.5, -0.0, 0.0)    # -0.0 against 0.0 (the maximum of the column, by value one number)
    a[rs.uniform(size=(S, m)) < 0.3] = -1.0
    a[:, 0], a[:, 1:3] = -0.0, 0.0
    out["signed_zeros"] = a
    a = noise()
    for k, j in enumerate(_spread(m, min(m, S + 2))):         # +inf (several: they tie), -inf
        a[k % S, j] = np.inf
        a[(k + 1) % S, j] = -np.inf if k % 2 else np.inf
    out["inf"] = a
    a = np.full((S, m), np.nan)
    a[:, _spread(m, 1)[0]] = -np.inf                          # -inf alone is a score, not "nothing"
    out["neg_inf_only"] = a
    if 2 <= S <= m:
        # sensor S-1's S-1 best objects are each the best of another sensor, with larger values: it ends up with its S-th candidate
        a = noise(lo=0.0, hi=1.0, nan=0.1)
        obj = _spread(m, S)
        for t in range(S - 1):
            a[t, obj[t]] = 1000.0 + t
            a[S - 1, obj[t]] = 100.0 - t
        a[S - 1, obj[S - 1]] = 50.0
        out["deep"] = a
    return out


def _fallbacks(S, m, base, rs):
    """fallback rows for a column whose no-fallback assignment is `base`: NULL, valid random draws, out of range, duplicated, colliding
    with assigned objects"""
    free = [j for j in rs.permutation(m).tolist() if j not in base][:W]
    out = {"null": None, "random": rs.randint(0, m, size=W), "oor": np.array([-1, m, m + 7, -2 ** 31, 2 ** 31 - 1, -5, m, m + 1])}
    if free:
        out["dup"] = np.full(W, free[0])
    if (base >= 0).any():
        out["collide"] = np.resize(base[base >= 0], W)
    if len(free) >= S:
        out["distinct"] = np.resize(np.asarray(free), W)
    return {k: (None if v is None else np.asarray(v, dtype=np.int64).astype(np.int32)) for k, v in out.items()}


@pytest.mark.parametrize("m", [5, 2003, 30001])
@pytest.mark.parametrize("S", [1, 3, 8])
def test_synthetic_scores_every_column(hip, S, m):
    """device.assign_sensors against the yardstick: one chunk, many chunks, a ragged tail; every column; every fallback flavour; the
    picks; the row's tail; ONE workspace for all the calls of a size, never zeroed again"""
    torch, dev = hip.torch, hip.dev
    cases = [_cases(S, m, 100 * S + c) for c in range(3)]       # (the three columns hold different draws of every case)
    ws = dev.assign_sensors_workspace(m, S, "cuda")
    seen = set()
    rs = np.random.RandomState(S + m)
    n_calls = 0
    for name in cases[0]:
        host = np.stack([cases[c][name] for c in range(3)], axis=2)      # [S, m, 3]
        score = torch.as_tensor(host).cuda()
        for col in range(3):
            sc = host[:, :, col]
            base, _, bits0 = _assign_np(sc)
            assert np.array_equal(base, _assign_by_masked_argmax(dev, torch, score, col)), (name, col)     # the yardstick itself
            # ---- what this input holds
            nn = ~np.isnan(sc)
            if np.isnan(sc).all(axis=1).any():
                seen.add("nan_row")
            if nn.any(axis=0).sum() < S:
                seen.add("few")
            if len(set(np.where(nn.any(axis=1), np.nanargmax(np.where(nn, sc, -np.inf), axis=1), -1).tolist())) == 1 and S > 1 and nn.all(axis=1).any():
                seen.add("one_best")
            top = np.nanmax(np.where(nn, sc, -np.inf)) if nn.any() else None
            if top is not None:
                ss, jj = np.where(nn & (sc == top))
                if len(set(ss)) > 1:
                    seen.add("ties_sensors")
                if len(set((jj // CH).tolist())) > 1:
                    seen.add("ties_chunks")
            for s in range(S):
                if base[s] >= 0 and bits0[s] == NEG0 and (sc[s, base[s] + 1:] == 0.0).any() and \
                        (np.signbit(sc[s]) == False)[sc[s] == 0.0].any():      # noqa: E712  (a -0.0 won over a later +0.0)
                    seen.add("neg_zero")
                if base[s] >= 0 and np.isposinf(sc[s, base[s]]):
                    seen.add("inf")
                if base[s] >= 0 and _rank_of(sc[s], base[s]) == S - 1 and S > 1:
                    seen.add("deep")
            for fname, fb in _fallbacks(S, m, base, rs).items():
                want, assigned, bits = _assign_np(sc, fb)
                row = torch.full((W,), -7, dtype=torch.int32, device="cuda")
                picks = torch.full((W, 2), -7, dtype=torch.int64, device="cuda")
                got = dev.assign_sensors(score, col, fallback=None if fb is None else torch.as_tensor(fb).cuda(), out=row, picks=picks,
                                         workspace=ws)
                n_calls += 1
                assert got is row
                r, p = row.cpu().numpy(), picks.cpu().numpy()
                assert np.array_equal(r[:S], want), (name, col, fname, r, want)
                assert (r[S:] == -1).all() and (p[S:, 0] == -1).all() and (p[S:, 1] == 0).all(), (name, col, fname)
                assert np.array_equal(p[:S, 0], assigned) and np.array_equal(p[:S, 1], bits), (name, col, fname)
                held = r[:S][r[:S] >= 0]
                assert len(set(held.tolist())) == len(held) and (held < m).all(), (name, col, fname)      # no object named twice
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
    # two (and many more) consecutive calls on the one workspace: the last arrival left the ticket at zero every time
    assert n_calls > 2 and int(ws[0].item()) == 0
    out = dev.assign_sensors(score, 0)                                    # the defaults: a fresh row, a fresh workspace, no fallback
    assert out.dtype == torch.int32 and tuple(out.shape) == (W,) and np.array_equal(out.cpu().numpy()[:S], _assign_np(host[:, :, 0])[0])
    need = {"nan_row", "few", "neg_zero", "inf", "fb_null", "fb_oor"}
    if S > 1:       # (what takes two sensors: a common best, a tie between them, a draw another sensor's object spoils)
        need |= {"one_best", "ties_sensors", "fb_collide"}
    if 2 <= S <= m:         # (the S-th candidate: S objects)
        need |= {"deep"}
    if m >= 2 * S:          # (objects nobody holds are left for the draws; two idle sensors for a duplicated draw)
        need |= {"fb_taken"} | ({"fb_dup"} if S >= 3 else set())
    if m > CH:
        need |= {"ties_chunks"}
    print("[assign synthetic] S=%d m=%d: %d calls, seen %s" % (S, m, n_calls, sorted(seen)))
    assert seen >= need, need - seen


def test_device_front_end_refuses_what_the_kernel_cannot_take(hip):
    torch, dev, L = hip.torch, hip.dev, hip.lib
    score = torch.zeros((3, 40, 3), dtype=torch.float64, device="cuda")
    for bad in (score.cpu(), score[:, :, :2].contiguous(), score.to(torch.float32), score.permute(0, 2, 1)):
        with pytest.raises(L.SsaHipError):
            dev.assign_sensors(bad, 0)
    with pytest.raises(L.SsaHipError):
        dev.assign_sensors(score, 3)                                                               # no such column
    with pytest.raises(L.SsaHipError):
        dev.assign_sensors(score, 0, out=torch.zeros(3, dtype=torch.int32, device="cuda"))         # not a whole row
    with pytest.raises(L.SsaHipError):
        dev.assign_sensors(score, 0, out=torch.zeros(9, dtype=torch.int32, device="cuda")[1:])     # a misaligned row
    with pytest.raises(L.SsaHipError):
        dev.assign_sensors(score, 0, workspace=dev.assign_sensors_workspace(40, 2, "cuda"))        # sized for fewer sensors


# ---------------------------------------------------------------- real lookaheads
@pytest.mark.parametrize("propagator,sensors,regime", [("hybrid", 3, False), ("fg", 8, False), ("hybrid", 8, True)])
def test_real_lookaheads_equal_the_yardstick(envs, propagator, sensors, regime):
    """the engine advanced by step(); launch_assign_sensors on the scores launch_lookahead_sensors leaves, both agent columns, with and
    without fallback words -- also under a storage layout set at the engine (the scores are in the caller's numbering)"""
    import torch
    from ssa_gym_amd import _lib
    over = dict(propagator=propagator, storage_layout='regime' if regime else None)
    env = envs.make('ssa_tasker_simple-v2', config=cfg8(envs, sensors=sensors, **over))
    e, S = env._engine, env.n_sensor
    assert (e._order is not None) == regime and S == sensors
    rs = np.random.RandomState(31)
    for k in range(12):
        env.step(_distinct(rs, env.m, S))
        if k % 3:
            continue
        i = env.i
        look = e.launch_lookahead_sensors(i % e.H, i + 1, env._sites())
        host = look["score"].cpu().numpy()
        assert host.shape == (S, env.m, 3)
        for col in (_lib.LOOK_INFO_GAIN, _lib.LOOK_TRACE_GAIN):
            for fb in (None, rs.randint(0, env.m, size=W).astype(np.int32)):
                row = torch.full((W,), -7, dtype=torch.int32, device="cuda")
                picks = torch.full((W, 2), -7, dtype=torch.int64, device="cuda")
                e.launch_assign_sensors(look, col, row, fallback_row=None if fb is None else torch.as_tensor(fb).cuda(), picks=picks)
                want, assigned, bits = _assign_np(host[:, :, col], fb)
                r, p = row.cpu().numpy(), picks.cpu().numpy()
                assert np.array_equal(r[:S], want) and (r[S:] == -1).all(), (k, col, r, want)
                assert np.array_equal(p[:S, 0], assigned) and np.array_equal(p[:S, 1], bits), (k, col)
                assert (assigned >= 0).sum() >= 2                        # (a real assignment: most sensors see something)
    assert e._assign_ws[0] == S and int(e._assign_ws[1][0].item()) == 0


# ---------------------------------------------------------------- the engine loop
TIGHT = 1         # the site whose elevation mask nothing clears: its sensor is idle at every step (no fallback words)


def _net_tight(host, S, stride):
    lla = sites_rad()[:S]
    lim = np.radians([15.0, 89.9, 30.0, 0.0, 5.0, -10.0, 20.0, -30.0][:S])
    sig = [np.array([(1.0 + k) * host.arcsec2rad, (0.5 + 2.0 * k) * host.arcsec2rad, 1e3 / (1 + k)]) for k in range(S)]
    Rs = [np.diag(s ** 2) for s in sig]
    return lla, lim, Rs, sig, host.make_sensor_params(lla, lim, Rs, stride)


@pytest.mark.parametrize("S,m,K,H", [(3, 2003, 7, 8), (8, 403, 9, 4), (3, 30001, 4, 3)])
def test_engine_loop_equals_the_host_loop(hip, S, m, K, H):
    """K steps of lookahead + assign + launch_rollout_sensors (a one-row slice of the device log) with no host sync, against the host
    loop that reads every row back and calls launch_step_sensors: ring slots, status, statistics, per-sensor records bit for bit, the
    failure log as a set (test_rollout_sensors_gpu._compare).  One site's mask leaves its sensor idle (asserted)."""
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
                eng.launch_assign_sensors(look, col, log[k])
                row = log[k].cpu().numpy()                                # the host in the loop
                want = _assign_np(look["score"].cpu().numpy()[:, :, col])[0]
                assert np.array_equal(row[:S], want) and (row[S:] == -1).all(), (k, row, want)
                eng.launch_step_sensors(k % H, (k + 1) % H, 1 + k, sp, [int(a) for a in row[:S]], upd[(k + 1) % H].data_ptr(),
                                        fast_stats=True, argmax_spos=True)
        else:
            for k in range(K):
                look = eng.launch_lookahead_sensors(k % H, 1 + k, sp)
                eng.launch_assign_sensors(look, col, log[k])
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
    assert outs[0]["fail_count"] >= 1 and np.any(outs[0]["upd"][..., L.UPD_OBS_TAKEN] == 1.0)
    slots = [(k + 1) % H for k in range(max(0, K - H), K)]                  # (the record slots the K steps wrote)
    assert (outs[0]["upd"][slots, TIGHT, L.UPD_ACTION] < 0).all()           # the idle sensor has no record
    _compare(L, outs[0], outs[1], K, H, True)


# ---------------------------------------------------------------- the env
def _twin_loop(env, agent_col, fallback, n_steps):
    """the yardstick of run_agent_sensors: the yardstick's row from the env's own lookahead, then step(row) -- every row must be complete
    (step() takes one object per sensor).  Returns (last observation, actions, rewards, dones)."""
    S = env.n_sensor
    obs, acts, rewards, dones = None, [], [], []
    for k in range(n_steps):
        if env.i + 1 >= env.n:
            break
        sc = env.lookahead_sensors()["score"].cpu().numpy()[:, agent_col, :]
        row = _assign_np(sc, fallback[k])[0]
        assert (row >= 0).all() and len(set(row.tolist())) == S, (k, row)           # complete: step() can express it
        obs, r, d, _ = env.step(row if S > 1 else int(row[0]))
        acts.append(row)
        rewards.append(r)
        dones.append(d)
        if d:
            break
    return np.array(obs, copy=True), np.asarray(acts).reshape(len(acts), S), np.asarray(rewards), np.asarray(dones, dtype=bool)


def _check_run(a, b, agent, col, n_steps, rs, what):
    """n_steps on the twin `a` (host loop) and by b.run_agent_sensors, the same fallback rows"""
    S = a.n_sensor
    fb = np.stack([_distinct(rs, a.m, S) for _ in range(n_steps + 1)])
    obs_a, act_a, rew_a, don_a = _twin_loop(a, col, fb, n_steps)
    obs_b, act_b, rew_b, don_b = b.run_agent_sensors(agent, n_steps, fallback_actions=fb)
    assert act_b.shape == (len(rew_a), S) and _same(act_a, act_b), (what, act_a, act_b)
    assert _same(rew_a, rew_b) and _same(don_a, don_b) and _same(obs_a, obs_b), what
    _assert_same_env(a, b, what)
    return don_a


@pytest.mark.parametrize("reward_type,obs_returned,agent,sensors", [("trinary", "flatten", "agent_info_gain_sensors", 3),
                                                                    ("jones", "aer", "agent_trace_gain_sensors", 3),
                                                                    ("shaped", "flatten", "agent_info_gain_sensors", 3),
                                                                    ("shaped", "aer", "agent_trace_gain_sensors", 3),
                                                                    ("trinary", "aer", "agent_info_gain_sensors", 0),
                                                                    ("shaped", "flatten", "agent_trace_gain_sensors", 0)])
def test_env_run_agent_sensors_equals_a_step_loop(envs, reward_type, obs_returned, agent, sensors):
    """env.run_agent_sensors against a twin env that runs the yardstick's row through step(): a chunk boundary inside (K > H - 1), one more
    step() on both, then n_steps beyond the episode's end.  sensors = 0: no config['observers'], the env's one observer as a network."""
    from ssa_gym_amd import agents
    over = dict(steps=48, history=16, reward_type=reward_type, obs_returned=obs_returned, sensors=sensors)
    a = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, **over))
    b = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, **over))
    col = type(b).SENSOR_AGENT_COLUMNS[agent]
    S = b.n_sensor
    assert b._engine.H == 16 and S == max(sensors, 1)
    rs = np.random.RandomState(41)
    for env in (a, b):
        for row in (_distinct(np.random.RandomState(5), env.m, S) for _ in range(2)):
            env.step(row if S > 1 else int(row[0]))
    draws = b.np_random.get_state()[2]
    done = _check_run(a, b, getattr(agents, agent) if reward_type == "trinary" else agent, col, 25, rs, "25 steps")
    print("run_agent_sensors %s/%s S=%d: %d steps, done = %s, failed filters %d" % (reward_type, obs_returned, S, a.i - 2, done[-1],
                                                                                   len(a.failed_filters_id)))
    assert b.np_random.get_state()[2] == draws
    if not done[-1]:
        row = _distinct(rs, a.m, S)                      # the loop leaves the env steppable
        oa, ra, da, _ = a.step(row if S > 1 else int(row[0]))
        ob, rb, db, _ = b.step(row if S > 1 else int(row[0]))
        assert _same(oa, ob) and _same(ra, rb) and da == db
        _assert_same_env(a, b, "one more step")
        if not da:                                       # n_steps beyond the episode's end stops with the episode
            done = _check_run(a, b, agent, col, a.n - a.i + 5, rs, "to the end of the episode")
            assert done[-1]
            if reward_type == 'trinary':
                assert a.i == a.n - 1
            if a.i == a.n - 1:
                assert b.run_agent_sensors(agent, 3)[1].shape == (0, S)   # nothing left to run


def test_env_run_agent_sensors_default_fallback_and_idle_sensors(envs):
    """the default fallback rows (one action_space.sample() per row; env.np_random untouched) with a site that sees nothing: its sensor
    takes the draw unless another sensor holds that object, and is then booked idle (-1, no update record)"""
    a = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, steps=48, history=16, sensor_obs_limit=[15, 10, 90]))
    a.action_space.seed(11)
    draws = a.np_random.get_state()[2]
    fb = np.stack([_distinct(np.random.RandomState(k), a.m, 3) for k in range(13)])
    fb[3, 2], fb[7, 2] = -1, a.m + 4                          # out of range: sensor 2 stays idle at steps 4 and 8
    obs, acts, rewards, dones = a.run_agent_sensors("agent_info_gain_sensors", 12, fallback_actions=fb)
    assert acts.shape == (12, 3) and (acts[:, :2] >= 0).all()
    assert acts[3, 2] == -1 and acts[7, 2] == -1
    other = [k for k in range(12) if k not in (3, 7)]
    assert all(acts[k, 2] == fb[k, 2] or (acts[k, 2] == -1 and fb[k, 2] in acts[k, :2]) for k in other)
    assert np.array_equal(a.actions[1:13], acts) and (a._upd_action[[4, 8], 2] == -1).all() and not a.obs_taken[1:13, 2].any()
    obs, acts, rewards, dones = a.run_agent_sensors("agent_trace_gain_sensors", 5)         # the default draws
    assert acts.shape == (5, 3) and all(len(set(r[r >= 0].tolist())) == (r >= 0).sum() for r in acts)
    assert a.np_random.get_state()[2] == draws and a.i == 17


def test_engine_and_env_refuse_malformed_inputs(envs):
    """launch_assign_sensors takes the engine's [S][m][3] block and nothing that merely has its shape (a permuted view of a [S][3][m]
    block, float32); run_agent_sensors names the shape it wants when the fallback rows are too few or not rows of S; the env is untouched"""
    import torch
    from ssa_gym_amd import _lib
    env = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, steps=48, history=16))
    e, S = env._engine, env.n_sensor
    look = e.launch_lookahead_sensors(env.i % e.H, env.i + 1, env._sites())
    row = e.assign_row()
    assert row is e.assign_row() and tuple(row.shape) == (W,) and row.dtype == torch.int32
    e.launch_assign_sensors(look, _lib.LOOK_INFO_GAIN, row)
    good = look["score"]
    for bad in (good.permute(0, 2, 1).contiguous().permute(0, 2, 1), good.to(torch.float32), good.cpu(), good[:, :-1], good[0], None,
                good.cpu().numpy()):
        with pytest.raises(_lib.SsaHipError, match="contiguous CUDA float64"):
            e.launch_assign_sensors({"score": bad}, _lib.LOOK_INFO_GAIN, row)
    for bad in (np.zeros((4, S), dtype=int), np.zeros(5 * S + 1, dtype=int)):       # K + 1 = 5 rows of S wanted
        with pytest.raises(ValueError, match=r"\[K \+ 1, S\] = \[5, %d\]" % S):
            env.run_agent_sensors("agent_info_gain_sensors", 4, fallback_actions=bad)
    assert env.i == 0
    assert env.run_agent_sensors("agent_info_gain_sensors", 4, fallback_actions=np.zeros((7, S), dtype=int))[1].shape == (4, S)


def test_env_run_agent_sensors_late_in_an_episode(envs):
    """20 000 objects, three sites, 'hybrid': both envs advanced by the same 300 step() calls; then 60 steps of the closed loop against the
    twin's host loop, with filters failing inside the window (asserted on the twin)"""
    from ssa_gym_amd import _lib
    a = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, m=20000, history=64))
    b = envs.make('ssa_tasker_simple-v2', config=cfg3(envs, m=20000, history=64))
    for env in (a, b):
        rs = np.random.RandomState(7)
        for _ in range(300):
            env.step(_distinct(rs, env.m, 3))
    _assert_same_env(a, b, "after 300 steps")
    n_failed_before = int(a._stats[_lib.STAT_N_FAILED])
    assert a.failed_filters_id, "no failed filter after 300 steps"
    _check_run(a, b, "agent_info_gain_sensors", _lib.LOOK_INFO_GAIN, 60, rs, "60 steps from step 300")
    print("failed filters: %d before the window, %d after it" % (n_failed_before, int(a._stats[_lib.STAT_N_FAILED])))
    assert a.i == 360 and int(a._stats[_lib.STAT_N_FAILED]) > n_failed_before      # filters failed during the window
    assert a.obs_taken[301:361].any(axis=0).all()                                   # every sensor took observations
    row = _distinct(rs, a.m, 3)
    assert _same(a.step(row)[0], b.step(row)[0])
    _assert_same_env(a, b, "one more step")
