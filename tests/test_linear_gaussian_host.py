"""The linear-Gaussian pin of the UKF without a GPU (tests/support/linear_gaussian.py): with dt = 0 and obs_type
'xyz' one step is P- = P + Q, S = H B H^T + R, K = B H^T S^-1, P+ = P- - K S K^T with B = P (the default) or B = P- (resample) -- no
sigma point in it.  Here the oracle's env_step in float64 and 80-bit and oracle/ukf_numpy.py are held to both forms, the conditions the
GPU tests rely on are asserted, and the criterion is shown to reject the other form and a slightly wrong R, Q or measurement noise.

This family does NOT pin Wc0: in the linear case the zeroth point sits on the mean, so its covariance weight multiplies zero and beta
never enters (test_parameter_independence shows it); tests/test_unit_weights_*.py pin Wc0."""
import numpy as np
import pytest

from support import linear_gaussian as lg

VARIANTS = [False, True]


def _name(resample):
    return "resample" if resample else "keep"


# ---------------------------------------------------------------------------------------------------------------- the oracle's step
@pytest.mark.parametrize("alpha", lg.ALPHAS)
@pytest.mark.parametrize("resample", VARIANTS)
def test_oracle_step_against_the_closed_form(oracle, oracle_ld, alpha, resample):
    """env_step in both arithmetics on the one-step launches of m = 9 and m = 1, updated and predict-only rows: the 80-bit oracle meets
    the criterion and is closer to the closed form than the float64 one; every update was taken (asserted where the references are
    formed); the two closed forms lie 1e3 bounds apart or more on every judged update"""
    for m in (9, 1):
        cf, f64, ld = lg.step_family(oracle, oracle_ld, m, alpha, resample)
        label = "oracle, %s, alpha %g, m %d" % (_name(resample), alpha, m)
        figs = lg.assert_criterion(label + ", updated rows, 80-bit", ld, f64, cf, innovation=True)
        lg.assert_criterion(label + ", updated rows, float64", f64, f64, cf, innovation=True)
        for n_, s_, g_, r_, b in figs:      # (both hand their result out in float64 words: on a lone row they can tie at that rounding)
            assert g_ < r_ or g_ <= 1e-10, (label, n_, "the 80-bit oracle is no closer to the closed form than the float64 one", g_, r_)
        assert len(cf["x"]) == len(lg.STEP_LAUNCHES[m])
        other = lg.step_family(oracle, oracle_ld, m, alpha, not resample)[0]
        for k in range(len(cf["x"])):      # every judged update on its own
            one = lambda d: {q: d[q][k:k + 1] for q in ("x", "P")}      # noqa: E731
            d = lg.apart(one(cf), one(other), one(f64))
            print("[linear gaussian] %s, update %d: the other form lies %s bounds away" % (label, k, ", ".join("%s %.3g" % (n_, g_ / b) for n_, g_, b in d)))
            assert max(g_ / b for n_, g_, b in d) >= 1e3, (label, k, d)
            if alpha == 1.0:
                assert all(g_ / b >= 1e3 for n_, g_, b in d), (label, k, d)
        if m > 1:
            pc, pf, pl = lg.step_family(oracle, oracle_ld, m, alpha, resample, predicted=True)
            assert len(pc["x"]) == len(lg.STEP_LAUNCHES[m]) * (m - 1)
            lg.assert_criterion(label + ", predict-only rows, 80-bit", pl, pf, pc)
            # a predict-only row of the closed form: the mean's bits, P + Q
            sc = lg.scene(m)
            j0 = lg.STEP_LAUNCHES[m][0][1]
            keep = [j for j in range(m) if j != j0]
            assert np.array_equal(pc["x"][:m - 1].astype(np.float64), sc.x[keep])
            assert np.array_equal(pc["P"][:m - 1], sc.P[keep].astype(lg.L) + lg.Q.astype(lg.L))


def test_oracle_step_uncentred_80_bit(oracle, oracle_ld):
    """centred=False (the reference's own order of the weighted sums) in 80-bit at alpha = 1, both variants"""
    for resample in VARIANTS:
        got = lg.step_runs(lambda: lg.OracleStep(oracle_ld, 1.0, resample, False), 9)
        cf, f64, _ = lg.step_family(oracle, oracle_ld, 9, 1.0, resample)
        lg.assert_criterion("oracle, %s, alpha 1, 80-bit uncentred" % _name(resample), got, f64, cf, innovation=True)


def test_covariance_at_the_smallest_alpha(oracle, oracle_ld):
    """alpha = 1e-4: the covariance is judged, the state printed (the float64 reference algorithm's mean is 0.1 sd off there)"""
    for resample in VARIANTS:
        cf, f64, ld = lg.step_family(oracle, oracle_ld, 9, 1e-4, resample)
        lg.assert_criterion("oracle, %s, alpha 1e-4, 80-bit" % _name(resample), ld, f64, cf, only=("covariance",))


@pytest.mark.parametrize("resample", VARIANTS)
def test_oracle_chain_against_the_closed_chain(oracle, oracle_ld, resample):
    """K = 6 steps of one observer with a revisit and an idle step, and H = 3 steps of three sensors with their own R: every step's rows"""
    for name, (sched, tix0), m in [("rollout %d" % i, r, 9) for i, r in enumerate(lg.ROLLOUTS)] + [("network", lg.NETWORK, 9)]:
        cf, f64, ld = lg.references(oracle, oracle_ld, lg.scene(m), 0, sched, tix0, 1.0, resample)
        assert len(cf["tasked"]) == sum(1 for r in sched for j in r if j >= 0) == len(ld["tasked"])
        label = "oracle chain, %s, %s" % (name, _name(resample))
        lg.assert_criterion(label + ", updated rows", lg.rows(ld), lg.rows(f64), lg.rows(cf), innovation=True)
        lg.assert_criterion(label + ", other rows", *(lg.rows(r, predicted=True) for r in (ld, f64, cf)))


def test_update_interval_and_hidden_objects_leave_predict_only_rows(oracle, oracle_ld):
    """the closed chain under update_interval = 2 takes the updates of the even time indices alone; hidden: none"""
    sched, tix0 = lg.ROLLOUT
    cf = lg.chain(lg.ClosedForm(False), lg.scene(9), 0, sched, tix0, update_interval=2)
    assert [(k, j) for k, s, j in cf["tasked"]] == [(k, r[0]) for k, r in enumerate(sched) if r[0] >= 0 and (tix0 + k) % 2 == 0] and cf["tasked"]
    assert not lg.chain(lg.ClosedForm(False), lg.scene(9), 0, sched, tix0, hidden=True)["tasked"]


def test_covariance_reads_the_noise_only_through_the_mean(oracle):
    """the float64 oracle's rollout under two noise tables: every object's covariance is the same bits up to and including its first
    update; the means of the updated objects differ -- the property tests/test_linear_gaussian_gpu.py asserts of the kernel.  After
    the revisit object 2's covariance is NOT the same bits (its sigma points were drawn around a mean that carries the noise): the
    bit-for-bit statement cannot be made of the whole rollout"""
    import copy
    sched, tix0 = lg.ROLLOUT
    sc = lg.scene(9)
    other = copy.copy(sc)
    other.noise = np.random.RandomState(5).normal(size=sc.noise.shape) * 50.0
    a, b = (lg.chain(lg.OracleStep(oracle, 1.0, False, False), s_, 0, sched, tix0) for s_ in (sc, other))
    first = lg.first_updates(sched, 9)
    assert first.tolist() == [6, 6, 0, 6, 6, 5, 6, 1, 4]
    for j in range(9):
        k = min(int(first[j]), len(sched) - 1) + 1
        assert np.array_equal(a["P"][:k, j], b["P"][:k, j]), j
    assert not np.array_equal(a["x"][0, 2], b["x"][0, 2])
    assert not np.array_equal(a["P"][-1, 2], b["P"][-1, 2])


# ---------------------------------------------------------------------------------------------------------------- power
@pytest.mark.parametrize("alpha", lg.ALPHAS)
@pytest.mark.parametrize("resample", VARIANTS)
def test_the_swapped_form_fails(oracle, oracle_ld, alpha, resample):
    """the oracle's run of one variant judged against the OTHER variant's closed form: the covariance lies beyond its bound, in both
    arithmetics"""
    cf_other = lg.step_family(oracle, oracle_ld, 9, alpha, not resample)[0]
    cf, f64, ld = lg.step_family(oracle, oracle_ld, 9, alpha, resample)
    for what, got in (("80-bit", ld), ("float64", f64)):
        bad = dict(lg.fails(got, f64, cf_other, yard=cf))
        print("[linear gaussian] %s run (%s, alpha %g) against the %s form: beyond the bound by %s" % (_name(resample), what, alpha, _name(not resample), bad))
        assert bad.get("covariance", 0.0) >= 1e3, (what, bad)


WRONG = {"R (1 + 1e-6)": (dict(R_scale=1 + 1e-6), "covariance"), "measurement noise (1 + 1e-6)": (dict(noise_scale=1 + 1e-6), "position"),
         "Q (1 + 1e-3)": (dict(Q_scale=1 + 1e-3), "covariance")}


@pytest.mark.parametrize("wrong", list(WRONG))
@pytest.mark.parametrize("resample", VARIANTS)
def test_a_wrong_oracle_step_fails(oracle, oracle_ld, wrong, resample):
    """the 80-bit oracle with one input slightly off, at alpha = 1: the quantity the input reaches lies beyond its bound on the updated
    rows (Q: on the predict-only rows too)"""
    kw, quantity = WRONG[wrong]
    wrong_step = lambda: lg.OracleStep(oracle_ld, 1.0, resample, True, **kw)      # noqa: E731
    cf, f64, ld = lg.step_family(oracle, oracle_ld, 9, 1.0, resample)
    bad = dict(lg.fails(lg.step_runs(wrong_step, 9), f64, cf))
    print("[linear gaussian] %s, %s: beyond the bound by %s" % (wrong, _name(resample), bad))
    assert bad.get(quantity, 0.0) > 3.0, (wrong, bad)
    if wrong.startswith("Q"):
        pc, pf, _ = lg.step_family(oracle, oracle_ld, 9, 1.0, resample, predicted=True)
        badp = dict(lg.fails(lg.step_runs(wrong_step, 9, predicted=True), pf, pc))
        assert badp.get("covariance", 0.0) > 3.0, (wrong, badp)


# ---------------------------------------------------------------------------------------------------------------- beta and kappa
@pytest.mark.parametrize("resample", VARIANTS)
def test_parameter_independence(oracle, oracle_ld, resample):
    """the unscented transform of a linear map is exact for every beta and kappa: the 80-bit oracle's step under four (beta, kappa)
    meets the criterion against the ONE closed form, at alpha = 1 and 1e-3.  beta enters through Wc0 alone and Wc0 multiplies the zeroth
    point's deviation from the mean, which is zero here: a wrong Wc0 passes this family (the unit-weight tests pin it)"""
    for alpha in lg.ALPHAS:
        cf, f64, _ = lg.step_family(oracle, oracle_ld, 9, alpha, resample)
        for beta, kappa in ((2.0, -3), (0.0, -3), (2.0, 0), (5.0, 3)):
            got = lg.step_runs(lambda: lg.OracleStep(oracle_ld, alpha, resample, True, beta=beta, kappa=kappa), 9)
            lg.assert_criterion("beta %g kappa %g, %s, alpha %g" % (beta, kappa, _name(resample), alpha), got, f64, cf, innovation=True)


# ---------------------------------------------------------------------------------------------------------------- oracle/ukf_numpy.py
class _Numpy:
    """oracle/ukf_numpy.py's filter with fx the identity and hx = x[:3], as a stepper of lg.chain()"""
    dtype = np.float64

    def __init__(self, alpha, resample):
        self.alpha, self.resample = alpha, resample

    def step(self, xt, x, P, tasks):
        import ukf_numpy as un
        xo, Po, rec = np.array(x, dtype=np.float64), np.array(P, dtype=np.float64), {}
        for j in range(len(xo)):
            pts = un.MerweScaledSigmaPoints(6, self.alpha, lg.BETA, lg.KAPPA, sqrt_method=lambda A: np.linalg.cholesky(A).T)
            f = un.UnscentedKalmanFilter(6, 3, lg.DT, hx=lambda s: s[:3], fx=lambda s, dt: s, points=pts, resample_after_predict=self.resample)
            f.x, f.P, f.Q = xo[j].copy(), Po[j].copy(), lg.Q
            f.predict()
            if j in tasks:
                R_, zn = tasks[j]
                f.update(lg.measurement(xt[j], zn), R=R_)
                rec[j] = dict(y=f.y.copy(), S=f.S.copy())
            xo[j], Po[j] = f.x, f.P
        return xo, Po, rec


@pytest.mark.parametrize("resample", VARIANTS)
def test_ukf_numpy_against_the_closed_forms(oracle, oracle_ld, resample):
    """the NumPy restatement of the filter library under its resample_after_predict switch.  At alpha = 1 it meets the criterion against
    its own form and misses the other by 1e3 bounds.  At alpha = 1e-3 its weighted mean is np.dot's sum of terms of |Wm0| |x| = 8e13 m in
    BLAS order, not the oracle's: the same algorithm, the same number format, 2.6e-4 sd / 2.6e-7 sd^2 from the closed form where the
    float64 oracle's order gives 3.0e-5 / 3.0e-8 (measured; 'keep') -- it is no kernel and is not held to 3 x the oracle's order there.
    What is asserted at 1e-3 is the choice of form: 1e3 times closer to its own than to the other in the covariance"""
    for alpha in lg.ALPHAS:
        got = lg.step_runs(lambda: _Numpy(alpha, resample), 9)
        cf, f64, _ = lg.step_family(oracle, oracle_ld, 9, alpha, resample)
        other = lg.step_family(oracle, oracle_ld, 9, alpha, not resample)[0]
        label = "ukf_numpy, %s, alpha %g" % (_name(resample), alpha)
        if alpha == 1.0:
            lg.assert_criterion(label, got, f64, cf, innovation=True)
            assert dict(lg.fails(got, f64, other, yard=cf)).get("covariance", 0.0) >= 1e3
        else:
            lg.report(label, lg.figures(got, f64, cf, innovation=True))
            own, far = lg.errs_sd(got, cf)[2], lg.errs_sd(got, other)[2]
            assert np.all(1e3 * own <= far), (label, own.max(), far.min())
