"""A sensor network's K-step schedule in each of several envs: the bare vector env of the host tests; for the GPU tests the schedules
built from the visibility tables, the yardstick (K vector steps on a twin engine), the conditions found again in its outputs, and the
bit-for-bit comparisons of two engines / two vector envs."""
import numpy as np

from support.batches import make_batch
from support.sensors import _defined_fields
from support.vector_forecast import bare_vec as _bare_vec
from support.vector_lookahead import Engines, bad_of

# (every sensor sees a fair share of the objects and misses a fair share: sensor 1 sees everything)
MASKS_DEG = [-30.0, -90.0, -20.0, -45.0, -25.0, -60.0, -35.0, -40.0]
ALL_ITEMS = {"tile", "same_index", "idle", "dup", "oor", "cross", "failed", "taken"}
SMALL_ITEMS = {"idle", "oor", "failed", "same_index"}      # what two sensors on a handful of objects always have room for
STATE = ("x_true", "x_filter", "P_filter", "obs", "metrics", "status")


def bare_vec(S, reward_type="trinary", **kw):
    """support.vector_forecast.bare_vec with what the rollout's guards and its booking read"""
    vec = _bare_vec(S, **kw)
    vec.reward_type = reward_type
    vec.rewards_sum, vec._argmax_prev = np.zeros(vec.E), np.zeros(vec.E, dtype=np.int64)
    return vec


def engines(hip, E, m, S, history=2, **kw):
    return Engines(hip, E, m, S, history=history, masks=MASKS_DEG, **kw)


def visibility(hip, E, m, S, K, **kw):
    """vis [K, E, S, m] (the caller's indices) and upd_step [K, E]: the visibility of every object from every site at every step, and
    whether the update_interval lets env e update at step k.  The truth does not depend on the tasking: K idle vector steps give it."""
    X = engines(hip, E, m, S, history=K + 1, **kw)
    torch, host = hip.torch, hip.host
    g = make_batch(4, seed=123)[3]
    prop = kw.get("propagator", "hybrid")
    consts_of = [host.make_consts(g["Q"], X.Rs[s], 1e-4, 2.0, -3, 20.0, X.lim[s], X.lla[s], propagator=prop,
                                  obs_type=kw.get("obs_type", "aer")) for s in range(S)]
    idle = np.full((E, S), -1)
    for k in range(K):
        X.vec.launch_step_sensors_envs(k, k + 1, 1 + k, X.sp, idle, 0, fast_stats=True)
        torch.cuda.synchronize()      # (the rows travel through the engine's table: one launch at a time)
    vis = np.zeros((K, E, S, m), dtype=bool)
    for k in range(K):
        for e in range(E):
            M = X.vec.trans[(X.t0[e] + 1 + k) % X.vec.n_time].reshape(3, 3)
            for s in range(S):
                vis[k, e, s] = hip.dev.visible_mask(X.vec.x_true[k + 1, e * m:(e + 1) * m], M, consts_of[s]).cpu().numpy().astype(bool)
    iv = int(kw.get("interval", 1))
    upd_step = np.array([[(X.t0[e] + 1 + k) % iv == 0 for e in range(E)] for k in range(K)])
    return vis, upd_step


def build_schedule(rs, E, m, S, K, vis, upd_step, pos_of=None):
    """a schedule [K, E, S] (each env's own numbering) that holds, as far as the slots allow it: every env's NaN filter tasked after
    step 1, for every sensor an object it sees, an object below its sensor's mask and above another's, two tasked objects of one env
    in one tile with one of them tasked in another env at the same step, a duplicate in a row, an idle sensor and an out-of-range
    action -- the records-bearing ones in rows whose update runs.  pos_of [E][m]: the storage position of env e's object j (a layout).
    Returns the schedule and the set of items it holds."""
    FREE = -2
    bad = bad_of(m)
    pos_of = np.tile(np.arange(m), (E, 1)) if pos_of is None else np.asarray(pos_of)
    sched = np.full((K, E, S), FREE, dtype=np.int64)
    planned = set()

    def free(k, e):
        return [s for s in range(S) if sched[k, e, s] == FREE]

    def pick(k, e, ok=lambda j: True):
        for j in rs.permutation(m):
            if j != bad and j not in sched[k, e] and ok(int(j)):
                return int(j)
        return None

    rows = [(k, e) for k in range(K) for e in range(E)]
    upd_rows = [(k, e) for k, e in rows if upd_step[k, e]]
    # every env's NaN filter, tasked after the step it failed in
    if K >= 2:
        for e in range(E):
            k = 1 + e % (K - 1)
            sched[k, e, S - 1] = bad
        planned.add("failed")
    # an idle sensor and an out-of-range action (in the last rows: the first ones are left to what needs a row whose update runs)
    for item, word in (("idle", -1), ("oor", m + 3)):
        for k, e in rows[::-1]:
            f = free(k, e)
            if f:
                sched[k, e, f[-1]] = word
                planned.add(item)
                break
    # one object index in two envs at one step
    for k in range(K):
        es = [e for e in range(E) if free(k, e)]
        if len(es) >= 2:
            j = pick(k, es[0], lambda j: j not in sched[k, es[1]])
            if j is None:
                continue
            sched[k, es[0], free(k, es[0])[0]] = sched[k, es[1], free(k, es[1])[0]] = j
            planned.add("same_index")
            break
    # every sensor takes an observation
    got = 0
    for s in range(S):
        for k, e in upd_rows:
            if sched[k, e, s] != FREE:
                continue
            j = pick(k, e, lambda j: vis[k, e, s, j])
            if j is not None:
                sched[k, e, s] = j
                got += 1
                break
    if got == S:
        planned.add("taken")
    # below its sensor's mask, above another's
    for k, e in upd_rows:
        hit = None
        for s in free(k, e):
            j = pick(k, e, lambda j: not vis[k, e, s, j] and vis[k, e, :, j].any())
            if j is not None:
                hit = (s, j)
                break
        if hit and S >= 2:
            sched[k, e, hit[0]] = hit[1]
            planned.add("cross")
            break
    # two objects of one env in one tile; one of them in another env at the same step
    for k, e in rows:
        f = free(k, e)
        others = [e2 for e2 in range(E) if e2 != e and free(k, e2)]
        if len(f) < 2:
            continue
        pair = None
        for j in rs.permutation(m):
            mates = [int(q) for q in range(m) if q != j and pos_of[e, q] // 4 == pos_of[e, j] // 4 and q != bad and q not in sched[k, e]]
            if j != bad and j not in sched[k, e] and mates:
                pair = (int(j), mates[0])
                break
        if pair is None:
            continue
        sched[k, e, f[0]], sched[k, e, f[1]] = pair
        planned.add("tile")
        for e2 in others:      # (... and one of the two in another env at the same step)
            if pair[0] not in sched[k, e2]:
                sched[k, e2, free(k, e2)[0]] = pair[0]
                break
        break
    # a duplicate (in a row whose update runs: the higher sensor's record says so)
    for k, e in upd_rows:
        f = free(k, e)
        if len(f) >= 2:
            sched[k, e, f[0]] = sched[k, e, f[1]] = pick(k, e)
            planned.add("dup")
            break
    for k, e in rows:
        for s in free(k, e):
            sched[k, e, s] = pick(k, e)
    assert (sched != FREE).all()
    return sched, planned


def outputs(hip, eng, stats, upd):
    """what a run left: the engine's rings, status words and failure log, the per-step statistics [K, E, STAT_STRIDE] and records"""
    hip.torch.cuda.synchronize()
    out = {k: getattr(eng, k).cpu().numpy().copy() for k in STATE + ("stats",)}
    out["stats_k"], out["upd"] = stats.cpu().numpy().copy(), None if upd is None else upd.cpu().numpy().copy()
    out["fail_count"] = int(eng.fail_count.cpu().numpy()[0])
    out["fail_log"] = eng.fail_log[:out["fail_count"]].copy()
    return out


def run_steps(hip, X, sched, argmax=False):
    """the yardstick: K launch_step_sensors_envs on X's vector engine -- rows and time words by value up to 8 envs, through the engine's
    table and env_time0 beyond -- every step's statistics and records kept"""
    torch, L = hip.torch, hip.lib
    K, E, S = sched.shape
    eng, H = X.vec, X.H
    stats = torch.zeros((K, E, L.STAT_STRIDE), dtype=torch.float64, device="cuda")
    upd = torch.zeros((K, E, S, L.UPD_STRIDE), dtype=torch.float64, device="cuda")
    for k in range(K):
        kw = dict(fast_stats=True, argmax_spos=argmax, stats_out=stats[k].data_ptr())
        if E <= L.INLINE_ENVS:
            eng.launch_step_sensors_envs(k % H, (k + 1) % H, 0, X.sp, sched[k], upd[k].data_ptr(), env_words=[t + 1 + k for t in X.t0], **kw)
        else:
            eng.launch_step_sensors_envs(k % H, (k + 1) % H, 1 + k, X.sp, sched[k], upd[k].data_ptr(), **kw)
            torch.cuda.synchronize()
    return outputs(hip, eng, stats, upd)


def run_rollout(hip, X, sched, argmax=False, records=True):
    """the K steps by ONE launch_rollout_sensors_envs on X's vector engine (time words from env_time0)"""
    torch = hip.torch
    rows = torch.as_tensor(np.clip(sched, -1, 2 ** 31 - 1).astype(np.int32)).cuda()
    stats, upd = X.vec.launch_rollout_sensors_envs(0, 1, X.sp, rows, argmax_spos=argmax, records=records)
    out = outputs(hip, X.vec, stats, upd)
    out["shards"] = X.vec._roll_shards.cpu().numpy()
    return out


def log_set(log):
    return sorted(tuple(np.nan_to_num(np.asarray(r, dtype=np.float64), nan=-1.0).tolist()) for r in log)


def i64(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_equal_runs(L, a, b, K, H):
    """two runs bit for bit: the rings, the status words, every step's statistics and defined record fields, the statistics ring where
    step k owns its slot (against the yardstick's statistics of step k), the failure count, and the failure log as a set of records"""
    for nme in STATE:
        assert np.array_equal(i64(a[nme]), i64(b[nme])), nme
    assert np.array_equal(i64(a["stats_k"]), i64(b["stats_k"])), "stats of every step"
    for k in range(max(0, K - H), K):
        assert np.array_equal(i64(b["stats"][(k + 1) % H]), i64(a["stats_k"][k])), ("statistics ring", k)
    ua, ub = _defined_fields(L, a["upd"]), _defined_fields(L, b["upd"])
    for k in range(K):
        assert np.array_equal(i64(ua[k]), i64(ub[k])), ("upd", k)
    assert a["fail_count"] == b["fail_count"]
    assert log_set(a["fail_log"]) == log_set(b["fail_log"])
    assert not b["shards"].any()      # every per-step shard set of the rollout is folded and cleared


def assert_schedule_seen(L, X, sched, planned, vis, upd_step, yard, pos_of=None, required=ALL_ITEMS):
    """the conditions the schedule was built for, found again in the schedule, the visibility tables and the YARDSTICK's outputs"""
    K, E, S = sched.shape
    m, bad = X.m, bad_of(X.m)
    pos_of = np.tile(np.arange(m), (E, 1)) if pos_of is None else np.asarray(pos_of)
    upd, seen = yard["upd"], set()
    inr = (sched >= 0) & (sched < m)
    for k in range(K):
        for e in range(E):
            row, ok = sched[k, e], inr[k, e]
            tiles = [int(pos_of[e, a]) // 4 for a in set(row[ok].tolist())]
            if max([tiles.count(t) for t in tiles] + [0]) >= 2:
                seen.add("tile")
            for s in range(S):
                a = int(row[s])
                if a == -1:
                    assert upd[k, e, s, L.UPD_ACTION] == -1
                    seen.add("idle")
                elif a >= m:
                    assert upd[k, e, s, L.UPD_ACTION] == -1
                    seen.add("oor")
                elif a in row[:s]:
                    if upd_step[k, e]:
                        assert upd[k, e, s, L.UPD_ACTION] == -1      # the lower sensor holds the object
                        seen.add("dup")
                elif a != bad and upd_step[k, e] and not vis[k, e, s, a] and vis[k, e, :, a].any():
                    rec = upd[k, e, s]
                    if rec[L.UPD_ACTION] == a:                        # (attempted: the filter was healthy) ... and not seen
                        assert rec[L.UPD_VISIBLE] == 0 and rec[L.UPD_OBS_TAKEN] == 0, (k, e, s, rec[:8])
                        seen.add("cross")
        for e1 in range(E):
            for e2 in range(e1 + 1, E):
                for c in set(sched[k, e1][inr[k, e1]].tolist()) & set(sched[k, e2][inr[k, e2]].tolist()):
                    s1, s2 = list(sched[k, e1]).index(c), list(sched[k, e2]).index(c)
                    z1 = X.zn[e1, s1, (X.t0[e1] + 1 + k) % X.zn.shape[2], c].cpu().numpy()
                    z2 = X.zn[e2, s2, (X.t0[e2] + 1 + k) % X.zn.shape[2], c].cpu().numpy()
                    if not np.array_equal(z1, z2):
                        seen.add("same_index")
    # every env's NaN filter: failed in step 1 (its record says so), tasked in a later step and skipped there
    log = yard["fail_log"]
    ok = K >= 2
    for e in range(E):
        first = [r for r in log if int(r[L.FAIL_ENV]) == e and int(r[L.FAIL_OBJ]) == bad]
        assert len(first) == 1 and first[0][L.FAIL_TIME] == X.t0[e] + 1, (e, first)
        later = [(k, s) for k in range(1, K) for s in range(S) if sched[k, e, s] == bad]
        ok = ok and bool(later)
        for k, s in later:
            assert upd[k, e, s, L.UPD_ACTION] == -1, (e, k, s)
    if ok:
        seen.add("failed")
    if all((upd[:, :, s, L.UPD_OBS_TAKEN] == 1.0).any() for s in range(S)):
        seen.add("taken")
    assert len(set(X.t0)) == E                                  # envs at different time words
    assert seen >= planned, (planned - seen)
    assert planned >= required, (required - planned)


# ---------------------------------------------------------------------------------------------------------------- env level
def force_reset(vec, e):
    """env e reset in place as step() resets an env that is done (its arg-max refreshed): the envs then stand at different i"""
    slot = vec.tick % 2
    vec._reset_env(e, slot)
    st = vec._eng.stats[slot].cpu().numpy()
    vec._argmax_prev[e] = int(st[e, 3])


def host_obs(o):
    return o.cpu().numpy() if hasattr(o, "cpu") else np.asarray(o)


def assert_same_vec(a, b, what):
    """everything a vector step leaves: the envs' state (bit for bit), their step indices, what the episodes have paid, the arg-max
    the 'shaped' reward compares with, the status words and the failure count"""
    import torch
    torch.cuda.synchronize()
    assert a.tick % 2 == b.tick % 2 and np.array_equal(a.i, b.i), (what, a.i, b.i)
    assert np.array_equal(i64(a.rewards_sum), i64(b.rewards_sum)), (what, a.rewards_sum, b.rewards_sum)
    if a.reward_type == 'shaped':
        assert np.array_equal(a._argmax_prev, b._argmax_prev), what
    for e in range(a.E):
        for nme in ("x_true", "x_filter", "P_filter"):
            assert np.array_equal(i64(getattr(a, nme)(e)), i64(getattr(b, nme)(e))), (what, e, nme)
    assert torch.equal(a._eng.status, b._eng.status), what
    assert int(a._eng.fail_count.cpu()[0]) == int(b._eng.fail_count.cpu()[0]), what
    n = int(a._eng.fail_count.cpu()[0])
    assert log_set(a._eng.fail_log[:n]) == log_set(b._eng.fail_log[:n]), what


def run_pair(a, b, sched, rollout=None):
    """the schedule [E, K, S] by step() on `a` and by rollout_sensors() on `b` (rollout(): the [E, K] form), called again after each
    stop; every call compared: observations, rewards, dones, terminal observations, and the envs behind it.  Returns the number of
    calls and the dones [E, K]."""
    E, K, S = sched.shape
    k0, calls, all_d = 0, 0, []
    while k0 < K:
        rew, don, obs_a, info_a = [], [], None, None
        for k in range(k0, K):
            obs_a, r, d, info_a = a.step(sched[:, k] if S > 1 or a.n_sensor > 1 else sched[:, k, 0])
            rew.append(np.array(r, copy=True))
            don.append(np.array(d, copy=True))
            if d.any():
                break
        obs_a = np.array(host_obs(obs_a), copy=True)
        if rollout is None:
            obs_b, rew_b, don_b, info_b = b.rollout_sensors(sched[:, k0:])
        else:
            obs_b, rew_b, don_b, info_b = rollout(b, sched[:, k0:, 0])
        n = len(rew)
        what = "call %d, steps %d .. %d" % (calls, k0, k0 + n - 1)
        assert rew_b.shape == (E, n) and don_b.shape == (E, n) and don_b.dtype == bool, (what, rew_b.shape)
        assert np.array_equal(i64(rew_b), i64(np.stack(rew, axis=1))), (what, rew_b, rew)
        assert np.array_equal(don_b, np.stack(don, axis=1)), what
        oa, ob = obs_a, host_obs(obs_b)
        assert oa.dtype == ob.dtype and oa.shape == ob.shape and np.array_equal(oa.view(np.uint8), ob.view(np.uint8)), (what, "observation")
        assert len(info_b) == E
        for e in range(E):
            assert set(info_a[e]) == set(info_b[e]), (what, e, info_a[e].keys(), info_b[e].keys())
            assert ('terminal_observation' in info_b[e]) == bool(don_b[e, -1]), (what, e)
            if 'terminal_observation' in info_a[e]:
                ta, tb = host_obs(info_a[e]['terminal_observation']), host_obs(info_b[e]['terminal_observation'])
                assert ta.dtype == tb.dtype and np.array_equal(ta.view(np.uint8), tb.view(np.uint8)), (what, e, "terminal observation")
        assert_same_vec(a, b, what)
        all_d.append(don_b)
        k0 += n
        calls += 1
    return calls, np.concatenate(all_d, axis=1)
