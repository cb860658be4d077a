"""SSA_PROP_J2_RK4 without a GPU: the pins of the 80-bit yardstick (oracle/j2_reference.py rk4_j2 / ukf_predict_j2) to what the suite
already trusts -- the 80-bit oracle's sigma points and predict, the DOP853 integration --, and the POWER of the two criteria the J2
tests use: the operator criterion of support/devmath.py (run on the host build by tests/test_device_math_host.py, on the device by
tests/test_device_math_gpu.py and tests/test_j2_step_gpu.py) must reject a propagator with one sub-step more or fewer, the equatorial
radius of WGS84 instead of the IERS one, a J2 off by 1e-6 and no J2 at all; the filter criterion of support/j2.py must reject a filter
whose J2 is 1 % off."""
import numpy as np
import pytest

import j2_reference as J
import oracle as orc
from conftest import golden
from support import j2 as sj
from support.batches import relnorm
from support.devmath import J2_CASES, assert_j2_criterion, build_hostmath

ALPHAS = (1e-3, 1e-4)


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return build_hostmath(str(tmp_path_factory.mktemp("hostmath_j2")))


# ---------------------------------------------------------------------------------------------------------------- pins of the yardstick
@pytest.mark.parametrize("alpha", ALPHAS)
def test_yardstick_sigma_points_are_the_80bit_oracles(oracle_ld, alpha):
    """drawn in 80 bits from the plain upper Cholesky factor and rounded: oracle_ld.sigma_points to one ulp (both round an 80-bit value;
    the oracle multiplies P by a scale that arrives as a double, as the yardstick does)"""
    g = golden("ukf_step_golden.npz")
    _, _, scale = orc.merwe_weights(alpha, 2.0, -3)
    worst = 0.0
    for x in g["x0"][:16]:
        mine = J.sigma_points(x, g["P0"], scale, np.longdouble).astype(np.float64)
        ref = oracle_ld.sigma_points(x, g["P0"], scale)
        worst = max(worst, (np.abs(mine - ref) / np.spacing(np.abs(ref))).max())
    print("[j2 yardstick] alpha %.0e: sigma points against the 80-bit oracle's, largest difference %.1f ulp" % (alpha, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("alpha", ALPHAS)
def test_yardstick_predict_with_the_oracles_propagation_is_the_oracles_predict(oracle_ld, alpha, centred):
    """ukf_predict_j2 with its propagation replaced by oracle_ld.propagate against oracle_ld.ukf_predict.  One difference remains:
    the hook takes the points as doubles, the oracle keeps them in 80 bits.  A point's rounding error is at most eps |x| / 2 per
    component (eps = 2^-52); twelve points enter the mean with weight Wm[1], so the mean moves by at most 12 Wm[1] eps / 2 of |x|,
    component by component -- in units of the prior sd that is 6 Wm[1] eps |x| / sd; a covariance entry moves by at most
    2 . 12 Wc[1] |dy| eps |x| / 2 with |dy| = sqrt(scale) sd the points' distance from the mean (plus the mean's own movement, second
    order), in units of sd^2: 12 Wc[1] sqrt(scale) eps |x| / sd.  The bounds below are those (with |x| the state's largest
    component per block, x 2 for the propagation's conditioning over 20 s) -- a few ulps of the sd-normalised covariance at the
    catalogue's sd of 100 km, and of the size of the float64 floor of the predict itself (1e-10 relative in the mean at alpha =
    1e-3): which is why the yardstick draws its points in 80 bits and does not round them."""
    g = golden("ukf_step_golden.npz")
    Wm, Wc, scale = orc.merwe_weights(alpha, 2.0, -3)
    eps = 2.0 ** -52
    worst = np.zeros(2)
    bound = np.zeros(2)
    for x in g["x0"][:16]:
        xm, Pm, _ = J.ukf_predict_j2(x, g["P0"], g["Q"], 20.0, Wm, Wc, scale, 4, dtype=np.longdouble, centred=centred,
                                     fx=lambda p: oracle_ld.propagate(p.astype(np.float64), 20.0))
        rc, xo, Po, _ = oracle_ld.ukf_predict(x, g["P0"], g["Q"], 20.0, Wm, Wc, scale, centred=centred)
        assert rc == 0
        sd = np.sqrt(np.diag(Po))
        big = np.repeat([np.abs(x[:3]).max(), np.abs(x[3:]).max()], 3)
        d_x = (np.abs(xm.astype(np.float64) - xo) / sd).max()
        d_P = (np.abs(Pm.astype(np.float64) - Po) / np.outer(sd, sd)).max()
        b_x = 2 * (6 * Wm[1] * eps * big / sd).max() + eps
        b_P = 2 * (12 * Wc[1] * np.sqrt(scale) * eps * big / sd).max() + 4 * eps
        worst = np.maximum(worst, [d_x, d_P])
        bound = np.maximum(bound, [b_x, b_P])
        assert d_x <= b_x and d_P <= b_P, (alpha, centred, d_x, b_x, d_P, b_P)
    print("[j2 yardstick] alpha %.0e centred %s: predict against the 80-bit oracle's, mean %.2e sd (bound %.2e), covariance %.2e sd^2 "
          "(bound %.2e)" % (alpha, centred, worst[0], bound[0], worst[1], bound[1]))


def test_yardstick_rk4_against_dop853_is_the_truncation():
    """the 80-bit RK4 against scipy's DOP853 at rtol 1e-11 on the rows of tests/test_j2_extension.py: what h = 5 s costs (2.2e-13 measured
    at 20 s); the bounds are that test's, and hold for this comparison only"""
    x = golden("catalogue_subset.npy")[::7][:64]
    for dt, nsub in ((20.0, 4), (150.0, 30)):
        y = J.rk4_j2(x, dt, nsub, dtype=np.longdouble).astype(np.float64)
        ref = np.array([J.fx_xyz_cowell_j2(xi, dt) for xi in x])
        ep, ev = relnorm(y, ref, slice(0, 3)).max(), relnorm(y, ref, slice(3, 6)).max()
        print("[j2 yardstick] 80-bit RK4 against DOP853 at dt %.0f, %d sub-steps: position %.2e velocity %.2e" % (dt, nsub, ep, ev))
        assert ep < 1e-10 and ev < 1e-9


def test_yardstick_runs_in_both_types_and_over_leading_axes():
    x = golden("catalogue_subset.npy")[:24].reshape(2, 3, 4, 6)
    for T in (np.float64, np.longdouble):
        y = J.rk4_j2(x, 30.0, 6, dtype=T)
        assert y.dtype == T and y.shape == x.shape
        assert np.array_equal(y[1, 2, 3], J.rk4_j2(x[1, 2, 3], 30.0, 6, dtype=T))


# ---------------------------------------------------------------------------------------------------------------- the criteria's power
MUTANTS = {
    "one sub-step more": lambda hm, x, dt, n: hm.propagate_j2(x, dt, n + 1, J.J2_EARTH, J.R_EQ_EARTH),
    "one sub-step fewer (two for one)": lambda hm, x, dt, n: hm.propagate_j2(x, dt, n - 1 if n > 1 else 2, J.J2_EARTH, J.R_EQ_EARTH),
    "r_eq of WGS84": lambda hm, x, dt, n: hm.propagate_j2(x, dt, n, J.J2_EARTH, 6378137.0),
    "j2 off by 1e-6": lambda hm, x, dt, n: hm.propagate_j2(x, dt, n, J.J2_EARTH * (1 + 1e-6), J.R_EQ_EARTH),
    "no j2": lambda hm, x, dt, n: hm.propagate_j2(x, dt, n, 0.0, J.R_EQ_EARTH),
}


@pytest.mark.parametrize("case", J2_CASES, ids=lambda c: "dt%g-n%d" % c)
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_operator_criterion_rejects_a_wrong_propagator(hm, mutant, case):
    """the host build of propagate_j2_rk4 run with the wrong sub-step count or constant: the body that passes on the right one
    (test_device_math_host.py::test_j2_rk4_vs_80bit) fails, at every (dt, nsub) of its cases.  (The smallest of these moves a state by
    1e-13 in position and 8.7e-12 in velocity against a bound near 5e-15.)"""
    with pytest.raises(AssertionError):
        assert_j2_criterion(lambda x, dt, n: MUTANTS[mutant](hm, x, dt, n)[0], mutant, cases=(case,))
    assert_j2_criterion(lambda x, dt, n: hm.propagate_j2(x, dt, n, J.J2_EARTH, J.R_EQ_EARTH)[0], "right", cases=(case,))


def _golden_predicts(oracle, alpha, j2, ld, rows=slice(None)):
    g = golden("ukf_step_golden.npz")
    return [sj.predict_reference(oracle, x, g["P0"], g["Q"], 20.0, alpha, 4, j2=j2, ld=ld) for x in g["x0"][rows]]


def test_filter_criterion_rejects_a_j2_off_by_one_per_cent(oracle):
    """the rows of ukf_step_golden.npz at alpha = 1e-3: the float64 yardstick run with 0.99 J2 fails the criterion of the GPU tests
    (its velocity moves by 2.9e-7 against a floor of 5e-10); run in the centred form instead of index order -- another rounding of
    the same mathematics, as a kernel is -- it passes"""
    ld = _golden_predicts(oracle, 1e-3, J.J2_EARTH, True)
    f64 = _golden_predicts(oracle, 1e-3, J.J2_EARTH, False)
    Rf = [sj.distances(a, b) for a, b in zip(f64, ld)]
    wrong = _golden_predicts(oracle, 1e-3, 0.99 * J.J2_EARTH, False)
    G = np.array([sj.distances(a, b) for a, b in zip(wrong, ld)])
    assert G[:, 1].max() > 1e-7
    with pytest.raises(AssertionError):
        sj.assert_filter_criterion(G, Rf, "0.99 J2")
    g = golden("ukf_step_golden.npz")
    Wm, Wc, scale = orc.merwe_weights(1e-3, 2.0, -3)
    other = []
    for x in g["x0"]:
        xp, Pp, _ = J.ukf_predict_j2(x, g["P0"], g["Q"], 20.0, Wm, Wc, scale, 4, centred=True)
        other.append(dict(x=xp, P=Pp))
    sj.assert_filter_criterion([sj.distances(a, b) for a, b in zip(other, ld)], Rf, "float64, centred")
