"""Episode-level failure behaviour (parity of what a whole episode DOES, not of one step).

In the reference a filter fails when predict() raises LinAlgError (robust_cholesky's ladder exhausted, dynamics.py:402-417) or
returns NaN (newton() gave up, farnocchia.py:337-353); filter_error() then overwrites it with the 1e20 sentinels
(ssa_tasker_simple_2.py:271-285, 369-382) and the next np.max(delta_pos) ends a 'jones' / 'shaped' episode (:325-343).  With the
env defaults (alpha = 1e-4) the reference loses 2-3 % of its filters over a 480-step round-robin episode: the prior covariance
sum_i Wc_i y_i y_i^T carries Wc_0 ~ -2e8, and for a diverged (hyperbolic) prior its cancellation noise makes P indefinite.

Measured on the oracle (reference order of operations) and on the HIP path, same inputs, FIVE workloads (seeds):
  * SSA_PROP_HYBRID + SSA_FLAG_REFERENCE_COV (the env default: what `fx_xyz_farnocchia` resolves to): the series solver on strong-elliptic
    states, the reference's formulas (fast primitives) on every other state -- the BEHAVIOUR-FAITHFUL variant at speed;
  * SSA_PROP_ELEMENTS + SSA_FLAG_REFERENCE_COV ('elements'): the reference's operation order throughout;
  * SSA_PROP_FG ('fg'): more accurate than the reference on diverged states, its filters survive -- zero failures, asserted as exactly
    that: a documented behavioural difference.
What "the same behaviour" can mean is bounded by the oracle itself: its two summation orders of the SAME arithmetic (reference order /
centred means) lose 52 vs 64 filters on seed 7 and agree on WHICH filters only to a Jaccard overlap of 0.07-0.12 -- which filter of the
susceptible population goes first is decided by rounding noise.  The gate therefore is: pooled counts per window (~270 failures: a
three-sigma band of +-6 %), the status-code mix, the 'jones' step, the overlap of the failed sets with the oracle's at the level of the
oracle's own yardstick, the POPULATION the failures come from (filters the oracle sees diverged by step 300: 13 % of the objects, 57 %
of the oracle's late failures) and the distribution of first-failure steps.  A variant that reproduced the count with the wrong filters
(random ones: 13 % from that population, overlap 0.01) fails it.

The oracle is our own restatement, so the gate (tests/support/episode_gate.py::hold_to, stated once) is also applied against the REFERENCE
COMPOSITE -- tests/golden/episode_failures_reference.json: the same five episodes run by the reference's own fx_xyz_farnocchia,
robust_cholesky, hx_aer_erfa, mean_z_uvw and residual_z_aer driving oracle/ukf_numpy.py (gen_episode_failures_reference.py): the oracle
is held to it on the CPU, fixture against fixture, and the HIP variants on the GPU from the same runs.  Measured: composite 264 failures
pooled (248 LinAlgError, 13 AssertionError, 3 NaN), oracle 273, hybrid 277, elements 263; overlaps with the composite 0.086 / 0.111 /
0.095 against the yardstick's 0.092; first-failure medians 370 / 365 / 374 / 375, KS <= 0.076.
"""
import json
import os

import numpy as np
import pytest

import episode_workload as ew
from conftest import GOLDEN
from support.episode_gate import band, hold_to, ks_distance, late_in_population, yardstick

FIXTURE = os.path.join(GOLDEN, "episode_failures_oracle.json")
REFERENCE_FIXTURE = os.path.join(GOLDEN, "episode_failures_reference.json")


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(FIXTURE))


@pytest.fixture(scope="module")
def reference_fixture():
    """the same five episodes run by the reference's own callbacks (tests/golden/gen_episode_failures_reference.py)"""
    f = json.load(open(REFERENCE_FIXTURE))
    return {seed: f["seed%d" % seed]["reference_composite"] for seed in ew.SEEDS}


@pytest.fixture(scope="module")
def workload():
    return ew.workload(m=2000, seed=7)


@pytest.fixture(scope="module")
def oracle_runs(workload):
    import oracle as orc
    orc.build()
    return {"reference_order": ew.run_oracle(workload), "centred_means": ew.run_oracle(workload, centred=True)}


def test_oracle_episode_matches_the_committed_fixture(oracle_runs, fixture):
    """the fixture (tests/golden/gen_episode_failures.py, generated in the build container) pins the oracle's episode: same
    libm, same summation order -> same counts; a different host libm may move single filters across the ladder's edge"""
    fx = fixture["seed7"]
    for name in ("reference_order", "centred_means"):
        got, want = oracle_runs[name], fx[name]
        print(name, {k: got[k] for k in ("failed_at", "status_mix", "jones_done_step")})
        assert got["jones_done_step"] == want["jones_done_step"]
        for w in ew.WINDOWS:
            assert band(got["failed_at"][w], want["failed_at"][str(w)]), (name, w, got, want)
        assert ew.jaccard(got["failed_ids"], want["failed_ids"]) >= 0.8          # (same arithmetic, same machine class: the same filters)
    # the headline fact: the reference arithmetic loses filters late in the episode, almost all to LinAlgError
    ro = oracle_runs["reference_order"]
    assert ro["failed_at"][240] <= 2 and 30 <= ro["failed_at"][479] <= 90
    assert ro["status_mix"][ew.orc.ST_PREDICT_LINALG] >= 0.8 * ro["failed_at"][479]


def test_the_oracles_own_yardstick(fixture):
    """what two faithful evaluations of the SAME arithmetic agree on (fixture only, no GPU): the oracle in the reference's summation order
    against the oracle with centred means, five seeds -- pooled counts inside the band, WHICH filters: overlap 0.07-0.12 (chance, for
    ~55 of 2 000: 0.014), the population: more than half of the late failures from the 13 % of filters diverged by step 300."""
    J, cnt_a, cnt_b, pop_in, pop_n, div_n = [], 0, 0, 0, 0, 0
    for seed in ew.SEEDS:
        a, b = fixture["seed%d" % seed]["reference_order"], fixture["seed%d" % seed]["centred_means"]
        J.append(ew.jaccard(a["failed_ids"], b["failed_ids"]))
        cnt_a += a["failed_at"]["479"]
        cnt_b += b["failed_at"]["479"]
        k, n = late_in_population(b, a["diverged_at_%d" % ew.DIVERGED_STEP])
        pop_in, pop_n, div_n = pop_in + k, pop_n + n, div_n + len(a["diverged_at_%d" % ew.DIVERGED_STEP])
    print("[yardstick] pooled failures %d vs %d; overlap per seed %s; late failures of one order inside the other's diverged population: %d of %d "
          "(population = %.3f of the objects)" % (cnt_a, cnt_b, np.round(J, 3).tolist(), pop_in, pop_n, div_n / (2000.0 * len(ew.SEEDS))))
    assert band(cnt_a, cnt_b) and 200 <= cnt_a <= 350
    assert 0.04 <= np.mean(J) <= 0.3
    assert pop_in >= 0.4 * pop_n and div_n <= 0.2 * 2000 * len(ew.SEEDS)


def test_oracle_episode_statistics_match_the_reference_composite(fixture, reference_fixture):
    """fixture against fixture (no GPU, no oracle run): the oracle's reference-order episodes are held to the REFERENCE COMPOSITE -- the
    reference's own fx_xyz_farnocchia, robust_cholesky, hx_aer_erfa, mean_z_uvw and residual_z_aer driving oracle/ukf_numpy.py over the
    same inputs -- with the gate the HIP variants face against the oracle (support.episode_gate.hold_to), and no looser one.  Without
    this the gate below is circular: our kernels against our own restatement."""
    ref = {seed: fixture["seed%d" % seed]["reference_order"] for seed in ew.SEEDS}
    exc = sum((reference_fixture[s]["failed_exception"] for s in ew.SEEDS), [])
    print("[reference composite] first-failure exceptions: %s" % {e: exc.count(e) for e in sorted(set(exc))})
    hold_to("oracle, reference order", ref, reference_fixture, yardstick(fixture), "the reference composite")


@pytest.mark.gpu
def test_faithful_variants_reproduce_the_reference_failures_fg_does_not(fixture, reference_fixture):
    import torch
    import ssa_gym_amd
    from ssa_gym_amd import _lib, device, host, engine
    ssa_gym_amd.build()
    _lib.load()

    class H:
        pass
    hip = H()
    hip.torch, hip.lib, hip.dev, hip.host, hip.engine = torch, _lib, device, host, engine
    runs = {name: {} for name in ("hybrid", "elements", "fg")}
    extra = {}
    for seed in ew.SEEDS:
        w = ew.workload(m=2000, seed=seed)
        for name in runs:
            runs[name][seed] = ew.run_hip(hip, w, name)
        if seed == 7:      # what each ingredient contributes
            extra = {"elements + centred covariance": ew.run_hip(hip, w, "elements", covariance="centred"),
                     "fg + reference covariance": ew.run_hip(hip, w, "fg", covariance="reference")}
    ref = {seed: fixture["seed%d" % seed]["reference_order"] for seed in ew.SEEDS}
    cen = {seed: fixture["seed%d" % seed]["centred_means"] for seed in ew.SEEDS}
    yard = yardstick(fixture)
    ref_first = sum((ref[s]["failed_first_step"] for s in ew.SEEDS), [])
    cen_first = sum((cen[s]["failed_first_step"] for s in ew.SEEDS), [])
    print("[oracle] pooled failed @479: %d (reference order) / %d (centred means); overlap of the two per seed %s; first-failure step median %d / %d, "
          "KS distance between them %.3f" % (sum(ref[s]["failed_at"]["479"] for s in ew.SEEDS), sum(cen[s]["failed_at"]["479"] for s in ew.SEEDS),
                                          np.round(yard, 3).tolist(), np.median(ref_first), np.median(cen_first), ks_distance(ref_first, cen_first)))
    # ---- the behaviour-faithful variants: against the oracle, and against the reference's own code (the same gate, the same runs)
    for name in ("hybrid", "elements"):
        hold_to(name, runs[name], ref, yard, "the oracle", also=("its centred-means run", cen))
        hold_to(name, runs[name], reference_fixture, yard, "the reference composite")
    # ---- fg: NOT the reference's failure behaviour (more accurate on diverged states; nothing fails), stated as such
    for s in ew.SEEDS:
        fg = runs["fg"][s]
        assert all(v == 0 for v in fg["failed_at"].values()), (s, fg["failed_at"])
        assert abs(fg["jones_done_step"] - ref[s]["jones_done_step"]) <= 1        # a 'jones' episode still ends at the same step
        assert abs(fg["jones_done_step"] - reference_fixture[s]["jones_done_step"]) <= 1      # ... as the reference's own code ends it
    # what each ingredient contributes: the reference's covariance arithmetic alone (with the accurate propagator) fails nothing,
    # its propagator alone (with the cancellation-free covariance) a tenth of the reference's count
    assert all(v == 0 for v in extra["fg + reference covariance"]["failed_at"].values())
    assert extra["elements + centred covariance"]["failed_at"][479] <= 0.4 * ref[7]["failed_at"]["479"]
