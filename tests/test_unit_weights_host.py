"""The unit-weight pins of the fused step's UKF arithmetic without a GPU (tests/support/unit_weights.py): that every
case tests/test_unit_weights_gpu.py judges is a case -- no filter fails, every update is taken, in both oracles; that the float64
oracle's own distance from the 80-bit one at alpha = 1 is where the criterion assumes it is; that the criterion rejects a step with one
constant slightly off or one term of the transform missing, which the bounds at the reference's alpha = 1e-3 accept; and which solver
the hybrid's sigma points reach at alpha = 1."""
import numpy as np
import pytest

import oracle as orc
from conftest import golden
from support import unit_weights as uw
from support.devmath import build_hostmath

UPDATE_CASES = ("aer", "xyz", "aer resample", "xyz resample")
MU = 3.986004418e14


def _rows(d, rows):
    return {k: d[k][rows] for k in ("x", "P")}


def _figures(got, f64, ld, c):
    """the criterion's figures on the updated rows (with y and S) and on the predict-only rows of case c"""
    figs = uw.state_figures(_rows(got, c.updated), _rows(f64, c.updated), _rows(ld, c.updated))
    figs += uw.innovation_figures(uw.updates(got, c), uw.updates(f64, c), uw.updates(ld, c))
    return figs + [("predict-only " + n_, s_, g_, r_, b) for n_, s_, g_, r_, b in
                   uw.state_figures(_rows(got, c.predicted), _rows(f64, c.predicted), _rows(ld, c.predicted))]


# ---------------------------------------------------------------------------------------------------------------- 1. the conditions
@pytest.mark.parametrize("name", uw.CASES)
def test_every_case_is_one_on_the_oracle_side(oracle, oracle_ld, name):
    """status 0 on every row, the update taken in every env that is handed an action, in the float64 and in the 80-bit oracle: a change
    of seed or size that silently drops an update fails here, without a GPU"""
    c, f64, ld = uw.references(oracle, oracle_ld, name)
    assert c.E * c.m <= 768
    uw.assert_oracle_conditions(c, f64, ld)
    want = {"predict": (0, 256), "anisotropic": (0, 256), "tight": (0, 256), "ragged 1": (1, 0), "ragged 3": (1, 2), "ragged 5": (1, 4),
            "ragged 63": (1, 62)}.get(name, (48, 48 * 15))
    assert (len(c.updated), len(c.predicted)) == want
    # the criterion judges the float64 oracle itself as passing, and the references are handed out read-only
    uw.assert_criterion(name + ", the float64 oracle as the result", f64, f64, ld)
    with pytest.raises(ValueError):
        f64["x"][0, 0] = 0.0


def test_the_lookahead_case_on_the_oracle_side(oracle, oracle_ld):
    c = uw.case("lookahead")
    assert (c.E, c.m) == (1, 16)
    for o, centred in ((oracle, False), (oracle_ld, True)):
        r = uw.lookahead_references(o, c, uw.ALPHA, centred)
        assert not r["status"].any() and r["obs_taken"].all()
        assert np.isfinite(r["gain"].astype(np.float64)).all() and (r["gain"] > 0).all()


def test_the_network_scene_on_the_oracle_side(oracle, oracle_ld):
    """every (sensor, object) of every launch: visible 5 degrees or more above the mask, the update taken by both references (asserted
    where they are formed); each sensor tasks an object placed for it, a different one from launch to launch"""
    net, g, launches, refs = uw.network_references(oracle, oracle_ld)
    assert len(launches) == len(refs) == uw.NET_LAUNCHES and net.ang.tolist() == [False, True]
    for (tix, state, acts), r in zip(launches, refs):
        assert 0 < tix < uw.NET_TIME_ROWS and [a % 2 for a in acts] == [0, 1] and len(r) == 2
        assert r[0][1]["y"].shape == (3,) and r[1][1]["y"].shape == (2,)
    assert len({tuple(acts) for _, _, acts in launches}) >= uw.NET_M // 2


# ---------------------------------------------------------------------------------------------------------------- 2. the floor
def test_the_criterion_is_the_projects():
    """factor 3 and the slacks of tests/test_sensors_oracle_gpu.py / tests/support/j2.py; 1e-9 innovation sd for y and S"""
    from support import j2
    assert uw.FACTOR == 3.0 and uw.SLACK == (1e-12, 1e-12, 1e-9) == j2.SLACK and uw.INNOVATION_SLACK == 1e-9 and uw.ALPHA == 1.0
    Wm, Wc, scale = orc.merwe_weights(uw.ALPHA, uw.BETA, uw.KAPPA)
    assert (Wm[0], Wc[0], scale) == (-1.0, 1.0, 3.0) and np.all(Wm[1:] == 1 / 6) and np.all(Wc[1:] == 1 / 6)


@pytest.mark.parametrize("name", UPDATE_CASES)
def test_the_float64_floor_at_unit_weights(oracle, oracle_ld, name):
    """the float64 oracle against the 80-bit one on the updated rows: below 1e-13 / 1e-12 / 1e-8 and y, S below 1e-9 sd (loose caps on
    what DESIGN.md section 4 records), so that a change of the oracle cannot quietly turn the GPU criterion into a loose one"""
    c, f64, ld = uw.references(oracle, oracle_ld, name)
    figs = {(n_, s_): r_ for n_, s_, g_, r_, b in _figures(f64, f64, ld, c)}
    print("[unit weights floor] %s: float64 oracle vs 80-bit, updated rows max (pos, vel, cov) %.2e %.2e %.2e median %.2e %.2e %.2e; "
          "y %.2e S %.2e sd" % ((name,) + tuple(figs[(q, s)] for s in ("max", "median") for q in uw.QUANTITIES) + (figs[("y", "max")], figs[("S", "max")])))
    assert figs[("position", "max")] < 1e-13 and figs[("velocity", "max")] < 1e-12 and figs[("covariance", "max")] < 1e-8
    assert figs[("y", "max")] < 1e-9 and figs[("S", "max")] < 1e-9


# ---------------------------------------------------------------------------------------------------------------- 3. power
@pytest.mark.parametrize("wrong", list(uw.WRONG_CONSTANTS))
def test_a_wrong_constant_fails_at_unit_weights(oracle, oracle_ld, wrong):
    """the 80-bit oracle with one constant off as the result under test, on the 'aer' update case: at alpha = 1 at least one figure lies
    3 x beyond its bound.  For the record the same at alpha = 1e-3 against what test_update_parity_every_object asserts: R, the
    weights and the site are accepted there -- the gap this module closes"""
    ratio = {}
    for alpha in (uw.ALPHA, 1e-3):
        c, f64, ld = uw.references(oracle, oracle_ld, "aer", alpha)
        got = uw.oracle_run(oracle_ld, c, alpha, True, **uw.WRONG_CONSTANTS[wrong])
        assert not got["status"].any() and got["obs_taken"].all()
        figs = _figures(got, f64, ld, c)
        uw.report("%s at alpha = %g" % (wrong, alpha), figs)
        ratio[alpha] = uw.worst(figs)
        accepted = uw.accepted_by_the_update_parity_test(got, f64, ld, c)
    print("[unit weights power] %s: at alpha = 1 %s %s is %.1f x its bound; at alpha = 1e-3 %s %s is %.2g x the same criterion's bound, "
          "and test_update_parity_every_object's bounds %s it" % ((wrong,) + ratio[uw.ALPHA][1:] + ratio[uw.ALPHA][:1] + ratio[1e-3][1:] + ratio[1e-3][:1]
                                                                   + ("ACCEPT" if accepted else "reject",)))
    assert ratio[uw.ALPHA][0] >= 3.0, (wrong, ratio[uw.ALPHA])
    if wrong.startswith(("R ", "Wc_i", "site")):
        assert accepted, wrong


@pytest.mark.parametrize("mistake", ["no sum_wc term", "mean of the angles"])
def test_a_structural_mistake_fails_at_unit_weights(oracle, oracle_ld, mistake):
    """two mistakes written in long double on top of the 80-bit oracle's propagated points and sigmas_h: the prior covariance of the
    centred form without sum(Wc) m' m'^T (judged on the 'anisotropic' predict case: with the golden P0, isotropic in position, the mean
    shift m' vanishes to second order -- the gravity field is harmonic -- and the term is 1e-11 of the covariance, below any bound),
    and the predicted measurement as the weighted mean of the angles (the 'aer' update case).  The restatement without the mistake
    passes; with it at least one figure lies 3 x beyond its bound"""
    name, kw = {"no sum_wc term": ("anisotropic", dict(sum_wc_term=False)), "mean of the angles": ("aer", dict(angle_mean=True))}[mistake]
    for alpha in (uw.ALPHA, 1e-3):
        c, f64, ld = uw.references(oracle, oracle_ld, name, alpha)
        judge = (lambda r: _figures(r, f64, ld, c)) if len(c.updated) else (lambda r: uw.state_figures(_rows(r, c.predicted), f64, ld))
        right, wrong = judge(uw.restated(oracle_ld, c, alpha)), judge(uw.restated(oracle_ld, c, alpha, **kw))
        uw.report("%s at alpha = %g" % (mistake, alpha), wrong)
        print("[unit weights power] %s on '%s' at alpha = %g: %s %s is %.3g x its bound (the restatement without the mistake: %.2g x)"
              % ((mistake, name, alpha) + uw.worst(wrong)[1:] + uw.worst(wrong)[:1] + uw.worst(right)[:1]))
        if alpha == uw.ALPHA:
            assert uw.worst(right)[0] <= 1.0 and uw.worst(wrong)[0] >= 3.0, (mistake, uw.worst(right), uw.worst(wrong))
    if mistake == "no sum_wc term":      # the statement above about the golden P0
        c, f64, ld = uw.references(oracle, oracle_ld, "predict")
        iso = uw.worst(uw.state_figures(uw.restated(oracle_ld, c, uw.ALPHA, **kw), f64, ld))
        print("[unit weights power] %s on 'predict' (the golden P0): %s %s is %.2g x its bound" % ((mistake,) + iso[1:] + iso[:1]))
        assert iso[0] < 1.0


# ---------------------------------------------------------------------------------------------------------------- 4. hybrid routing
@pytest.fixture(scope="module")
def mm(tmp_path_factory):
    return build_hostmath(str(tmp_path_factory.mktemp("hostmath_unit_weights")))


def _series_lanes(mm, points):
    """which of the states [n, 6] the hybrid step leaves to the series solver (csrc/ssa_kernels.hip: kepler_hybrid_fast): handled by it
    and eccentricity below 0.99"""
    r, v = points[:, :3], points[:, 3:]
    rn = np.linalg.norm(r, axis=1, keepdims=True)
    e = np.linalg.norm(((v * v).sum(1, keepdims=True) - MU / rn) * r - (r * v).sum(1, keepdims=True) * v, axis=1) / MU
    _, handled = mm.uv_fast(points, uw.DT)
    return handled & (e < 0.99), e


def test_hybrid_routing_of_the_sigma_points_at_unit_weights(oracle, mm):
    """the sigma points of the predict case at alpha = 1 stand sqrt(3) sigma from the mean (170 km, 170 m/s): how many of them the hybrid
    step's lane-level choice hands to the series solver, and how many objects have points on both sides.  Recorded: all of them, and
    none -- and the same for every row of the catalogue under make_batch's filter offsets (its largest eccentricity is 0.737, its lowest
    perigee 6 673 km; no sigma point passes 0.89), so no choice of rows gives an object whose thirteen points take different solvers
    (DESIGN.md section 4).  Pinned so that a change of the series' domain or of the catalogue that makes mixed objects possible
    shows here -- the place to add them to the predict case"""
    c = uw.case("predict")
    sig = np.stack([oracle.sigma_points(c.x[j], c.P[j], 3.0) for j in range(c.m)])
    assert np.allclose(np.abs(sig[:, 1:7, :3] - sig[:, :1, :3]).max(axis=(1, 2)), np.sqrt(3.0) * 1e5)
    series, e = _series_lanes(mm, sig.reshape(-1, 6))
    per_obj = series.reshape(c.m, 13).sum(axis=1)
    mixed = int(((per_obj > 0) & (per_obj < 13)).sum())
    print("[unit weights routing] predict case: the series solver takes %d of %d sigma points; objects with points on both sides: %d; largest "
          "eccentricity of a point %.3f" % (series.sum(), series.size, mixed, e.max()))
    cat = golden("catalogue_subset.npy")
    xc = cat + np.random.RandomState(7).normal(size=cat.shape) * np.array([1e5] * 3 + [1e2] * 3)
    sc = np.stack([oracle.sigma_points(xj, c.g["P0"], 3.0) for xj in xc])
    series_c, ec = _series_lanes(mm, sc.reshape(-1, 6))
    per_row = series_c.reshape(len(cat), 13).sum(axis=1)
    print("[unit weights routing] all %d catalogue rows: the series solver takes %d of %d sigma points; rows with points on both sides: %d; "
          "largest eccentricity of a point %.3f" % (len(cat), series_c.sum(), series_c.size, ((per_row > 0) & (per_row < 13)).sum(), ec.max()))
    assert series.all() and mixed == 0
    assert series_c.all() and ec.max() < 0.99
