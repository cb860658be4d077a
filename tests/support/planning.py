"""The horizon-wide optimal plan of a sensor network (include/ssa_hip.h: ssa_plan_sensors_f64): what a
candidate is, the time-ordered greedy rule restated in numpy, the yardsticks from scipy -- the optimum of a dyadic table
(linear_sum_assignment with the count put first), the largest number of filled slots of any table (maximum_bipartite_matching) -- and
the checker of a device plan's fixed parts.  A table here is sc [H, S, m]: one column of one env's forecast."""
import math

import numpy as np

from support.matching import BOUND, SHIFT, U, W, candidates      # noqa: F401  (the candidate test is the one-step rule's)

CH = 512                    # objects per workgroup of the kernel: what "a chunk boundary" means
MAX_SLOTS = 64              # SSA_MAX_PLAN_SLOTS


def flat(sc):
    """the slots as rows: [H * S, m], slot h * S + s"""
    sc = np.asarray(sc, dtype=np.float64)
    return sc.reshape(sc.shape[0] * sc.shape[1], sc.shape[2])


def time_ordered(sc):
    """the planners of section 8h in numpy: steps in time order, per step the greedy rounds of ssa_assign_sensors_f64 (not NaN: a
    candidate; ties: the lowest s * m + j) with the objects planned at earlier steps removed.  plan [H, S], -1: none"""
    sc = np.asarray(sc, dtype=np.float64)
    H, S, m = sc.shape
    plan = np.full((H, S), -1, dtype=np.int64)
    planned = np.zeros(m, dtype=bool)
    for h in range(H):
        sl = sc[h].copy()
        sl[:, planned] = np.nan
        alive = ~np.isnan(sl)
        for _ in range(S):
            idx = np.flatnonzero(alive.reshape(-1))
            if not len(idx):
                break
            s, j = divmod(int(idx[np.argmax(sl.reshape(-1)[idx])]), m)
            plan[h, s] = j
            planned[j] = True
            alive[s], alive[:, j] = False, False
    return plan


def count(plan):
    return int((np.asarray(plan) >= 0).sum())


def total(sc, plan):
    """math.fsum of the scores a plan [H, S] picks: exact"""
    sc, plan = np.asarray(sc), np.asarray(plan)
    return math.fsum(float(sc[h, s, plan[h, s]]) for h in range(plan.shape[0]) for s in range(plan.shape[1]) if plan[h, s] >= 0)


def _columns(ok):
    return np.flatnonzero(ok.any(axis=0))


def best_count(sc):
    """the largest number of slots that can be filled with distinct candidate objects, for any table"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    ok = candidates(flat(sc))
    cols = _columns(ok)
    if not len(cols):
        return 0
    match = maximum_bipartite_matching(csr_matrix(ok[:, cols].astype(np.int8)), perm_type="column")
    return int((match >= 0).sum())


def best_dyadic(sc):
    """(count, total) of the plan-wide optimum of a DYADIC table (multiples of 2^-10 below 2^10 in magnitude: every sum is exact), as
    matching.best_dyadic reads them: linear_sum_assignment(maximize=True) on score + 2^30 for candidates and 0 elsewhere"""
    from scipy.optimize import linear_sum_assignment
    f = flat(sc)
    ok = candidates(f)
    cols = _columns(ok)
    if not len(cols):
        return 0, 0.0
    sub, oks = f[:, cols], ok[:, cols]
    assert (np.abs(sub[oks]) < 2.0 ** 10).all() and (sub[oks] * 1024 == np.round(sub[oks] * 1024)).all(), "not a dyadic table"
    r, c = linear_sum_assignment(np.where(oks, sub + SHIFT, 0.0), maximize=True)
    used = oks[r, c]
    return int(used.sum()), math.fsum(sub[r, c][used].tolist())


def best_total_doubles(sc, n_filled):
    """the math.fsum of the scores linear_sum_assignment picks on the table's own doubles, for a table whose optimum fills n_filled
    slots (the caller's exact count).  Where every slot that has a candidate can be filled -- a forecast with many visible objects --
    the slots without one are left out and the non-candidates are -inf (matching.best_full's form): scipy then works on the scores
    alone.  Otherwise the non-candidates cost -B, B a power of two above every sum of magnitudes, which puts the count first; B's
    rounding can only make this yardstick smaller, never the check unfair to the device."""
    from scipy.optimize import linear_sum_assignment
    f = flat(sc)
    ok = candidates(f)
    rows, cols = np.flatnonzero(ok.any(axis=1)), _columns(ok)
    if not len(cols):
        return 0.0
    sub, oks = f[np.ix_(rows, cols)], ok[np.ix_(rows, cols)]
    if n_filled == len(rows):
        r, c = linear_sum_assignment(np.where(oks, sub, -np.inf), maximize=True)
    else:
        big = 2.0 ** math.ceil(math.log2(max(float(np.abs(sub[oks]).max()), 2.0 ** -1000))) * 4 * MAX_SLOTS
        r, c = linear_sum_assignment(np.where(oks, sub, -big), maximize=True)
    used = oks[r, c]
    assert int(used.sum()) == n_filled, (int(used.sum()), n_filled)
    return math.fsum(sub[r, c][used].tolist())


def bound(sc):
    """the header's bound for a table that is not dyadic: 4 N 2^-53 max|candidate score|"""
    f = flat(sc)
    ok = candidates(f)
    return 4.0 * f.shape[0] * U * float(np.abs(f[ok]).max()) if ok.any() else 0.0


def check_plan(sc, rows, picks, S):
    """a device plan of ONE env -- rows [H, W] and picks [H, W, 2] -- against the rule's fixed parts: candidates only, no object twice
    across the whole plan, -1 beyond S, the picks' objects and bits.  Returns plan [H, S]."""
    sc = np.asarray(sc, dtype=np.float64)
    H, _, m = sc.shape
    ok = candidates(flat(sc)).reshape(sc.shape)
    rows, picks = np.asarray(rows), np.asarray(picks)
    assert rows.shape == (H, W) and picks.shape == (H, W, 2), (rows.shape, picks.shape)
    assert (rows[:, S:] == -1).all() and (picks[:, S:, 0] == -1).all() and (picks[:, S:, 1] == 0).all(), (rows, picks)
    plan = rows[:, :S].astype(np.int64)
    assert np.array_equal(plan, picks[:, :S, 0]), (plan, picks[:, :S, 0])
    for h in range(H):
        for s in range(S):
            j = plan[h, s]
            assert -1 <= j < m, (h, s, j)
            if j >= 0:
                assert ok[h, s, j], (h, s, j, sc[h, s, j])
                assert picks[h, s, 1] == sc[h, s, j:j + 1].view(np.int64)[0], (h, s, j)
            else:
                assert picks[h, s, 1] == 0, (h, s, picks[h, s])
    held = plan[plan >= 0]
    assert len(set(held.tolist())) == len(held), plan
    return plan


def dyadic_table(rng, H, S, m, pvis):
    """a dyadic random table with pass windows: gains that grow with h, every (sensor, object) visible in one window of steps"""
    base = np.round(rng.random(m) * 8 * 1024) / 1024
    sc = np.empty((H, S, m))
    for h in range(H):
        for s in range(S):
            sc[h, s] = base * (1 + h / 8.0) + np.round(rng.random(m) * 1024) / 1024
    sc = np.round(sc * 1024) / 1024
    start, ln = rng.integers(-H, H, size=(S, m)), rng.integers(1, H + 1, size=(S, m))
    for h in range(H):
        vis = (h >= start) & (h < start + ln)
        if pvis < 1:
            vis &= rng.random((S, m)) < max(pvis, 0.5)
        sc[h][~vis] = np.nan
    if pvis < 1:
        sc[:, :, rng.random(m) > pvis * 4] = np.nan
    return sc
