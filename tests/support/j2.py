"""The fused step with SSA_PROP_J2_RK4 against the 80-bit yardstick (oracle/j2_reference.py): the references of a predict and of an
update in float64 and in np.longdouble, the criterion that compares a filter with them, and the small scene of the GPU tests.  Shared by
tests/test_j2_host.py (the criterion's power, without a GPU), tests/test_j2_step_gpu.py and tests/test_j2_extension.py."""
import numpy as np

import j2_reference as J
import oracle as orc
from support import angles_only as ao
from support.batches import errs

DT = 20.0
SLACK = (1e-12, 1e-12, 1e-9)      # position, velocity, sd-normalised covariance: the slacks of tests/test_sensors_oracle_gpu.py


def predict_reference(o, x, P, Q, dt, alpha, nsub, j2=J.J2_EARTH, r_eq=J.R_EQ_EARTH, ld=False):
    """one filter's predict by the yardstick: float64 in index order, or 80-bit centred (the forms the fp64 and the 80-bit oracle take
    in every oracle test); `o`: the fp64 oracle, which must factorise (n + lambda) P on the ladder's first rung -- the plain attempt.
    Returns dict(x, P, sf) as float64 arrays plus the weights."""
    Wm, Wc, scale = orc.merwe_weights(alpha, 2.0, -3)
    assert o.robust_cholesky(scale * np.asarray(P))[1] == -1      # (the yardstick has no ladder)
    xp, Pp, sf = J.ukf_predict_j2(x, P, Q, dt, Wm, Wc, scale, nsub, j2, r_eq, np.longdouble if ld else np.float64, centred=ld)
    assert np.isfinite(xp.astype(np.float64)).all()
    return dict(x=xp.astype(np.float64), P=Pp.astype(np.float64), sf=sf.astype(np.float64), w=(Wm, Wc, scale))


def update_reference(o, pred, z, R, M, lla, itrs, resample, ld):
    """the oracle's own ukf_update on the yardstick's prediction and points: dict(x, P, y, S)"""
    Wm, Wc, scale = pred["w"]
    rc, xu, Pu, y, S, _ = o.ukf_update(pred["x"], pred["P"], pred["sf"], z, R, Wm, Wc, scale, M, lla, itrs, centred=ld, resample=resample)
    assert rc == 0
    return dict(x=xu, P=Pu, y=y, S=S)


def distances(a, b):
    """(position, velocity, sd-normalised covariance) distance of one filter dict(x [6], P [6, 6]) from another"""
    one = lambda r: {"x": np.asarray(r["x"])[None], "P": np.asarray(r["P"])[None]}      # noqa: E731
    return np.array(errs(one(a), one(b)))[:, 0]


def assert_filter_criterion(G, Rf, label):
    """G [n, 3]: the filter under test against the 80-bit yardstick, Rf [n, 3]: the float64 yardstick against it -- (position, velocity,
    sd-normalised covariance) per filter.  Median and maximum of G at most 3 x those of Rf plus SLACK.  Prints both sides."""
    G, Rf = np.asarray(G), np.asarray(Rf)
    assert G.shape == Rf.shape and len(G) > 0, (label, G.shape, Rf.shape)
    print("[j2 step vs yardstick] %s: %d filters; vs 80-bit (pos, vel, cov) under test median %s max %s, float64 yardstick median %s max %s"
          % (label, len(G), np.median(G, 0), G.max(0), np.median(Rf, 0), Rf.max(0)))
    for c, slack in enumerate(SLACK):
        assert np.median(G[:, c]) <= 3 * np.median(Rf[:, c]) + slack, (label, c, "median", np.median(G[:, c]), np.median(Rf[:, c]))
        assert G[:, c].max() <= 3 * Rf[:, c].max() + slack, (label, c, "max", G[:, c].max(), Rf[:, c].max())


def assert_truth_criterion(xt_out, xt_in, dt, nsub, j2, r_eq, label):
    """the truth rows of a step (or any batch of states through the kernel's RK4) under the operator criterion of support/devmath.py:
    distance from the 80-bit rk4_j2, maximum and median, at most 3 x the float64 restatement's plus 1e-15.  Returns the 80-bit value."""
    from support.devmath import J2_SLACK, _relnorm_ld
    ld = J.rk4_j2(xt_in, dt, nsub, j2, r_eq, np.longdouble)
    f64 = J.rk4_j2(xt_in, dt, nsub, j2, r_eq, np.float64)
    for what, sl in (("position", slice(0, 3)), ("velocity", slice(3, 6))):
        b, r = _relnorm_ld(xt_out, ld, sl), _relnorm_ld(f64, ld, sl)
        print("[j2 step truth] %s %s: %d rows; kernel vs 80-bit max %.2e median %.2e, float64 restatement max %.2e median %.2e"
              % (label, what, len(b), b.max(), np.median(b), r.max(), np.median(r)))
        assert b.max() <= 3 * r.max() + J2_SLACK, (label, what, "max", b.max(), r.max())
        assert np.median(b) <= 3 * np.median(r) + J2_SLACK, (label, what, "median", np.median(b), np.median(r))
    return ld


def scene(site_lla, site_itrs, mask, M, m, seed, dt=DT, nsub=4, j2=J.J2_EARTH, r_eq=J.R_EQ_EARTH, far=(1e7, 3e7)):
    """m objects at the step before the one under M, every one 10 degrees or more above the mask of the site (and below 80), the even
    ones 800 .. 2 200 km away -- below 9 000 km from the centre, where J2 moves a state by metres per step -- the odd ones `far`
    away (10 000 .. 30 000 km; None: 800 .. 2 200 km as the even ones); propagated dt BACK with the 80-bit rk4_j2 so that the step's
    own prediction brings them there.  Filters as support/angles_only.scene: 1 km / 1 m/s off the truth, and a covariance that says so."""
    rs = np.random.RandomState(seed)
    xt, x = np.empty((m, 6)), np.empty((m, 6))
    for j in range(m):
        leo = j % 2 == 0 or far is None
        t = ao.place(site_lla, site_itrs, M, rs.uniform(0, 2 * np.pi), rs.uniform(mask + np.radians(10.0), np.radians(80.0)),
                     rs.uniform(8e5, 2.2e6) if leo else rs.uniform(*far), rs)
        assert not leo or np.linalg.norm(t[:3]) < 9e6
        xt[j] = J.rk4_j2(t, -dt, nsub, j2, r_eq, np.longdouble).astype(np.float64)
        x[j] = xt[j] + rs.normal(size=6) * ao.X_SIGMA
    return xt, x, np.tile(np.diag(ao.X_SIGMA ** 2), (m, 1, 1))
