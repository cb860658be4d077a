"""The optimal assignment of a sensor network (include/ssa_hip.h: ssa_match_sensors_f64): what a candidate is, the fallback rule
restated in numpy, the greedy rounds for comparison, and the yardsticks from scipy -- the largest number of tasked sensors
(maximum_bipartite_matching on the candidate pattern) and the largest total (linear_sum_assignment)."""
import math

import numpy as np

W = 8                       # SSA_MAX_SENSORS: the width of an action row
CH = 512                    # objects per workgroup of the kernel: what "a chunk boundary" means
BOUND = 2.0 ** 1020         # a candidate's magnitude is at most this
SHIFT = 2.0 ** 30           # added to every candidate of a dyadic table: tasking one more sensor beats every sum of scores
U = 2.0 ** -53              # the unit roundoff of a double


def candidates(sc):
    """[S, m] bool: finite and of magnitude <= 2^1020"""
    sc = np.asarray(sc, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(sc) & (np.abs(sc) <= BOUND)


def apply_fallback(assigned, fallback, m):
    """the header's fallback rule on an assigned row [S] (-1: none): ascending s, the caller's draw if in range and held by nobody"""
    act = np.array(assigned, dtype=np.int64)
    if fallback is not None:
        for s in range(len(act)):
            f = int(fallback[s])
            if act[s] < 0 and 0 <= f < m and f not in act[act >= 0]:
                act[s] = f
    return act


def greedy_np(sc):
    """the greedy rounds of ssa_assign_sensors_f64 over sc [S, m] (not NaN: a candidate; ties: the lowest s * m + j): assigned [S]"""
    sc = np.asarray(sc, dtype=np.float64)
    S, m = sc.shape
    assigned = np.full(S, -1, dtype=np.int64)
    alive = ~np.isnan(sc)
    for _ in range(S):
        idx = np.flatnonzero(alive.reshape(-1))
        if not len(idx):
            break
        s, j = divmod(int(idx[np.argmax(sc.reshape(-1)[idx])]), m)
        assigned[s] = j
        alive[s], alive[:, j] = False, False
    return assigned


def total(sc, assigned):
    """math.fsum of the scores a row picks: exact"""
    return math.fsum(float(sc[s, j]) for s, j in enumerate(assigned) if j >= 0)


def _columns(ok):
    """the objects any sensor has as a candidate (the only ones that matter), ascending"""
    return np.flatnonzero(ok.any(axis=0))


def best_count(sc):
    """the largest number of sensors that can be tasked with distinct candidates"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    ok = candidates(sc)
    cols = _columns(ok)
    if not len(cols):
        return 0
    match = maximum_bipartite_matching(csr_matrix(ok[:, cols].astype(np.int8)), perm_type="column")
    return int((match >= 0).sum())


def best_dyadic(sc):
    """(count, total) of the optimum of a DYADIC table (multiples of 2^-10 below 2^10 in magnitude: every sum is exact):
    linear_sum_assignment(maximize=True) on score + 2^30 for candidates and 0 elsewhere, which puts the count first"""
    from scipy.optimize import linear_sum_assignment
    sc = np.asarray(sc, dtype=np.float64)
    ok = candidates(sc)
    cols = _columns(ok)
    if not len(cols):
        return 0, 0.0
    sub, oks = sc[:, cols], ok[:, cols]
    assert (np.abs(sub[oks]) < 2.0 ** 10).all() and (sub[oks] * 1024 == np.round(sub[oks] * 1024)).all(), "not a dyadic table"
    cost = np.where(oks, sub + SHIFT, 0.0)
    r, c = linear_sum_assignment(cost, maximize=True)
    used = oks[r, c]
    return int(used.sum()), math.fsum(sub[r, c][used].tolist())


def best_full(sc):
    """the optimum's total for a table in which every sensor can be tasked (asserted by the caller): linear_sum_assignment on the
    candidates' objects with non-candidates at -inf"""
    from scipy.optimize import linear_sum_assignment
    sc = np.asarray(sc, dtype=np.float64)
    ok = candidates(sc)
    cols = _columns(ok)
    sub = np.where(ok[:, cols], sc[:, cols], -np.inf)
    r, c = linear_sum_assignment(sub, maximize=True)
    return math.fsum(sub[r, c].tolist())


def tolerance(sc, S):
    """2 S (S - 1) u max|score|: each compared sum of at most S terms is off by at most (S - 1) u S max|score|, on both sides"""
    ok = candidates(sc)
    return 2.0 * S * (S - 1) * U * float(np.abs(np.asarray(sc)[ok]).max()) if ok.any() else 0.0


def check_row(sc, row, picks, S, m, fallback=None):
    """a device row [W] and picks [W, 2] against the rule's fixed parts: candidates only, no object twice, -1 beyond S, the picks' bits,
    the fallback outcome.  Returns assigned [S]."""
    sc = np.asarray(sc, dtype=np.float64)
    ok = candidates(sc)
    row, picks = np.asarray(row), np.asarray(picks)
    assigned = picks[:S, 0].astype(np.int64)
    assert (row[S:] == -1).all() and (picks[S:, 0] == -1).all() and (picks[S:, 1] == 0).all(), (row, picks)
    for s in range(S):
        j = assigned[s]
        assert -1 <= j < m, (s, j)
        if j >= 0:
            assert ok[s, j], (s, j, sc[s, j])
            assert picks[s, 1] == sc[s, j:j + 1].view(np.int64)[0], (s, j)
        else:
            assert picks[s, 1] == 0, (s, picks[s])
    held = assigned[assigned >= 0]
    assert len(set(held.tolist())) == len(held), assigned
    want = apply_fallback(assigned, fallback, m)
    assert np.array_equal(row[:S], want), (row, want)
    out = row[:S][row[:S] >= 0]
    assert len(set(out.tolist())) == len(out), row
    return assigned
