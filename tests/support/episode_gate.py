"""The episode failure gate of tests/test_episode_failures.py, stated once: what "the same failure behaviour over five 479-step episodes"
means between two evaluations of the reference's arithmetic (a HIP variant and the oracle; a HIP variant and the reference composite;
the oracle and the reference composite).  The runs are the dictionaries of episode_workload.run_oracle / run_hip, or what json made of
them (window keys as strings)."""
import numpy as np

import episode_workload as ew


def band(a, b):
    """two failure counts are 'the same statistics' when they differ by no more than three standard deviations of a
    Poisson count of their size (+3): the oracle's own two summation orders differ by 52 vs 64 at step 479"""
    return abs(a - b) <= 3.0 * np.sqrt(max(a, b)) + 3.0


def ks_distance(a, b):
    """two-sample Kolmogorov-Smirnov statistic of two samples of first-failure steps"""
    a, b = np.sort(np.asarray(a, dtype=float)), np.sort(np.asarray(b, dtype=float))
    grid = np.concatenate([a, b])
    return float(np.max(np.abs(np.searchsorted(a, grid, side="right") / len(a) - np.searchsorted(b, grid, side="right") / len(b))))


def late_in_population(run, population, after=ew.DIVERGED_STEP):
    """(failures after step `after` that lie in `population`, failures after step `after`)"""
    late = [j for j, s in zip(run["failed_ids"], run["failed_first_step"]) if s > after]
    return len(set(late) & set(population)), len(late)


def failed_at(run, w):
    """run["failed_at"][w], whether the run comes from a kernel (integer keys) or from a json fixture (string keys)"""
    f = run["failed_at"]
    return f[w] if w in f else f[str(w)]


def yardstick(fixture):
    """the oracle's own: per-seed overlap of the failed sets of its two summation orders of the SAME arithmetic"""
    return [ew.jaccard(fixture["seed%d" % s]["reference_order"]["failed_ids"], fixture["seed%d" % s]["centred_means"]["failed_ids"])
            for s in ew.SEEDS]


def hold_to(name, r, ref, yard, other_name="the oracle", also=None):
    """Holds the runs r[seed] to the runs ref[seed] (`other_name`); `yard` is the oracle's own yardstick, `also` a second set of runs whose
    overlap is printed only.  Returns the figures it printed.
    (1) pooled counts per window inside band(); at least 150 failures pooled
    (2) the ladder, not Kepler: at least 80 % of the failures are ST_PREDICT_LINALG; nothing from the update
    (3) a 'jones' episode ends where the other side's does, to one step, per seed
    (4) WHICH filters: mean overlap of the failed sets at least half the oracle's own yardstick, and >= 0.03 (chance: 0.014)
    (5) the population: at least 40 % of the late failures inside the OTHER side's diverged-by-step-300 filters (a random 13 %: 0.13)
    (6) WHEN: the median first-failure step within 25 steps, the KS distance of the two distributions <= 0.25; the first failure of
        every seed between steps 150 and 400"""
    orc = ew.orc
    for wdw in ew.WINDOWS:
        a, b = sum(failed_at(r[s], wdw) for s in ew.SEEDS), sum(failed_at(ref[s], wdw) for s in ew.SEEDS)
        assert band(a, b), (name, other_name, wdw, a, b)
    tot, tot_ref = (sum(failed_at(q[s], 479) for s in ew.SEEDS) for q in (r, ref))
    assert tot >= 150
    mix = np.sum([r[s]["status_mix"] for s in ew.SEEDS], axis=0)
    assert mix[orc.ST_PREDICT_LINALG] >= 0.8 * tot and mix[orc.ST_UPDATE_NAN] == 0 and mix[orc.ST_UPDATE_LINALG] == 0, (name, mix)
    for s in ew.SEEDS:
        assert abs(r[s]["jones_done_step"] - ref[s]["jones_done_step"]) <= 1, (name, other_name, s)
    J = [ew.jaccard(r[s]["failed_ids"], ref[s]["failed_ids"]) for s in ew.SEEDS]
    k = n = 0
    for s in ew.SEEDS:
        kk, nn = late_in_population(r[s], ref[s]["diverged_at_%d" % ew.DIVERGED_STEP])
        k, n = k + kk, n + nn
    first = sum((list(r[s]["failed_first_step"]) for s in ew.SEEDS), [])
    ref_first = sum((list(ref[s]["failed_first_step"]) for s in ew.SEEDS), [])
    ks = ks_distance(first, ref_first)
    extra = "" if also is None else "; with %s %.3f" % (also[0], np.mean([ew.jaccard(r[s]["failed_ids"], also[1][s]["failed_ids"]) for s in ew.SEEDS]))
    print("[%s against %s] pooled failed @479: %d (%s: %d); per seed %s; status mix %s; overlap per seed %s (mean %.3f%s; the oracle's own "
          "yardstick %.3f); late failures inside the other side's diverged population: %d of %d; first-failure step median %d (%s: %d), KS %.3f"
          % (name, other_name, tot, other_name, tot_ref, [failed_at(r[s], 479) for s in ew.SEEDS], mix.tolist(), np.round(J, 3).tolist(),
             np.mean(J), extra, np.mean(yard), k, n, np.median(first), other_name, np.median(ref_first), ks))
    assert np.mean(J) >= 0.5 * np.mean(yard) and np.mean(J) >= 0.03, (name, other_name, J, yard)
    assert k >= 0.4 * n, (name, other_name, k, n)
    assert abs(np.median(first) - np.median(ref_first)) <= 25 and ks <= 0.25, (name, other_name, np.median(first), np.median(ref_first), ks)
    assert all(150 <= r[s]["first_failure_step"] <= 400 for s in ew.SEEDS)
    return dict(total=tot, total_ref=tot_ref, mix=mix.tolist(), overlap=float(np.mean(J)), population=(k, n), median=float(np.median(first)),
                median_ref=float(np.median(ref_first)), ks=ks)
