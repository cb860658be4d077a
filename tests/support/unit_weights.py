"""The fused step's UKF arithmetic at unit sigma-point weights (alpha = 1: Wm0 = -1, Wc0 = 1, Wi = 1 / 6, n + lambda = 3), where the float64
result of the reference algorithm is defined six to nine orders of magnitude more tightly than at the reference's alpha = 1e-3 / 1e-4
(DESIGN.md section 4): the criterion that judges a result against the float64 and the 80-bit oracle, the cases (inputs and both oracles'
results, computed once and read-only), the wrong constants and structural mistakes that show the criterion's power, and the long-double
restatements they need.  Shared by tests/test_unit_weights_host.py and tests/test_unit_weights_gpu.py."""
import numpy as np

import oracle as orc
from support.batches import c2t, errs, make_batch
from support.fused_step import run_oracle

ALPHA, BETA, KAPPA, DT = 1.0, 2.0, -3, 20.0
FACTOR = 3.0                      # the project's: "no further from the exact value than 3 x the reference arithmetic is"
SLACK = (1e-12, 1e-12, 1e-9)      # position, velocity, sd-normalised covariance: tests/test_sensors_oracle_gpu.py, tests/support/j2.py
INNOVATION_SLACK = 1e-9           # y and S, in 80-bit innovation standard deviations
ANISOTROPY = np.array([1.0, 0.5, 0.2, 1.0, 1.0, 1.0])
NOISE_SIGMA = np.array([4.8e-6, 4.8e-6, 1e3])
QUANTITIES = ("position", "velocity", "covariance")
L = np.longdouble


# ---------------------------------------------------------------------------------------------------------------- the criterion
def state_figures(got, f64, ld, slack=SLACK):
    """[(quantity, statistic, got, float64 oracle, bound)]: maximum and median of errs(got, ld) per quantity over ALL rows handed in,
    the same statistic of errs(f64, ld), and FACTOR x that plus the quantity's slack"""
    out = []
    for name, g_, r_, s in zip(QUANTITIES, errs(got, ld), errs(f64, ld), slack):
        assert g_.shape == r_.shape and len(g_) > 0
        for stat, fn in (("max", np.max), ("median", np.median)):
            out.append((name, stat, float(fn(g_)), float(fn(r_)), FACTOR * float(fn(r_)) + s))
    return out


def innovation_sd(y, S, ld):
    """(|y - y_ld| / sd, |S - S_ld| / (sd sd^T)), the largest component per update, sd the 80-bit innovation's standard deviations"""
    Sd = np.sqrt(np.einsum('kii->ki', ld["S"]))
    ey = np.max(np.abs(np.asarray(y) - ld["y"]) / Sd, axis=1)
    eS = np.max(np.abs(np.asarray(S) - ld["S"]) / (Sd[:, :, None] * Sd[:, None, :]), axis=(1, 2))
    return ey, eS


def innovation_figures(got, f64, ld, slack=INNOVATION_SLACK):
    """y and S of every update: the largest figure at most FACTOR x the float64 oracle's largest plus the slack"""
    (gy, gS), (ry, rS) = innovation_sd(got["y"], got["S"], ld), innovation_sd(f64["y"], f64["S"], ld)
    return [("y", "max", float(gy.max()), float(ry.max()), FACTOR * float(ry.max()) + slack),
            ("S", "max", float(gS.max()), float(rS.max()), FACTOR * float(rS.max()) + slack)]


def report(label, figs):
    for name, stat, g_, r_, b in figs:
        print("[unit weights] %s: %s %s under test %.3e, float64 oracle %.3e, bound %.3e%s"
              % (label, name, stat, g_, r_, b, "" if g_ <= b else "   <-- %.1f x the bound" % (g_ / b)))


def worst(figs):
    """the figure furthest beyond its bound, as (ratio, quantity, statistic)"""
    return max((g_ / b, name, stat) for name, stat, g_, r_, b in figs)


def assert_criterion(label, got, f64, ld, rows=None, innovation=False):
    """the criterion on rows `rows` (None: all) of got / f64 / ld (dicts with x [n, 6], P [n, 6, 6]; innovation: y [k, 3], S [k, 3, 3] of
    every update too).  Prints every figure with its bound, then asserts all of them; returns the figures."""
    sub = (lambda d: {k: d[k] for k in ("x", "P")}) if rows is None else (lambda d: {k: d[k][rows] for k in ("x", "P")})
    figs = state_figures(sub(got), sub(f64), sub(ld))
    if innovation:
        figs += innovation_figures(got, f64, ld)
    report(label, figs)
    bad = [(n_, s_, g_, b) for n_, s_, g_, r_, b in figs if not g_ <= b]
    assert not bad, (label, bad)
    return figs


# ---------------------------------------------------------------------------------------------------------------- the cases
def noise(E, m):
    """the noise table of support/fused_step.run_gpu (its default, spelled out so that the oracle side needs no device)"""
    return np.random.RandomState(99).normal(size=(E, 480, m, 3)) * NOISE_SIGMA


class Case:
    """inputs of one launch: E envs of m rows, one action per env (-1: predict only), the time row, the measurement"""

    def __init__(self, name, batch, E, actions, tix, obs_type='aer', resample=False):
        self.name, self.E, self.tix, self.obs_type, self.resample = name, E, tix, obs_type, resample
        self.xt, self.x, self.P, self.g = batch
        self.m = len(self.x) // E
        self.actions = list(actions)
        self.R = self.g["R"] if obs_type == 'aer' else self.g["xyz_R"]
        self.z_noise = noise(E, self.m)
        self.updated = np.array([e * self.m + a for e, a in enumerate(self.actions) if a >= 0], dtype=np.int64)
        self.predicted = np.setdiff1d(np.arange(E * self.m), self.updated)

    def env(self, e):
        return slice(e * self.m, (e + 1) * self.m)


def case(name):
    """the cases of tests/test_unit_weights_gpu.py by name; every one a single launch of at most 768 rows"""
    upd = {"aer": ('aer', False), "xyz": ('xyz', False), "aer resample": ('aer', True), "xyz resample": ('xyz', True)}
    if name == "predict":
        return Case(name, make_batch(256, seed=1), 1, [-1], 1)
    if name in upd:      # the layout of tests/test_hip_step.py: test_update_parity_every_object
        return Case(name, make_batch(16 * 48, seed=3), 48, [(7 * e) % 16 for e in range(48)], 5, *upd[name])
    if name == "anisotropic":      # position variances 1 : 1 / 4 : 1 / 25 of the golden P0's (why: DESIGN.md section 4)
        xt, x, P, g = make_batch(256, seed=1)
        return Case(name, (xt, x, P * np.outer(ANISOTROPY, ANISOTROPY), g), 1, [-1], 1)
    if name == "tight":
        return Case(name, make_batch(256, seed=4, tight_fraction=1.0), 1, [-1], 2)
    if name.startswith("ragged "):
        m = int(name.split()[1])
        return Case(name, make_batch(m, seed=10 + m), 1, [m - 1], 3)
    if name == "lookahead":
        return Case(name, make_batch(16, seed=21), 1, [-1], 4)
    raise KeyError(name)


CASES = ("predict", "anisotropic", "aer", "xyz", "aer resample", "xyz resample", "tight", "ragged 1", "ragged 3", "ragged 5", "ragged 63")
_REFERENCES = {}


def _freeze(d):
    for v in d.values():
        v.setflags(write=False)
    return d


def oracle_run(o, c, alpha, centred, **wrong):
    """the oracle's step on every env of case c, stacked: x, P, x_true [E m, ...], status [E m], and per env obs_taken, z_true, y, S,
    sigmas_h (NaN where the env takes no update).  `wrong`: constants the step is handed in place of the right ones (wrong_step)"""
    out = {k: [] for k in ("x", "P", "x_true", "status", "obs_taken", "z_true", "y", "S", "sigmas_h")}
    ot = 0 if c.obs_type == 'aer' else 1
    for e in range(c.E):
        sl, a = c.env(e), c.actions[e]
        zn = c.z_noise[e, c.tix, a] if a >= 0 else np.zeros(3)
        if wrong:
            r = wrong_step(o, c, sl, a, zn, alpha, centred, **wrong)
        else:
            r = run_oracle(o, c.xt[sl], c.x[sl], c.P[sl], c.g, a, c.tix, alpha, obs_type=ot, centred=centred, resample=c.resample, R=c.R,
                           z_noise3=zn)
        for k in out:
            out[k].append(np.asarray(r[k]))
    cat = ("x", "P", "x_true", "status")
    return {k: (np.concatenate(v) if k in cat else np.stack(v)) for k, v in out.items()}


def references(oracle, oracle_ld, name, alpha=ALPHA):
    """(case, float64 oracle's result, 80-bit centred oracle's result) -- computed once per (case, alpha), shared, read-only"""
    key = (name, alpha)
    if key not in _REFERENCES:
        c = case(name)
        _REFERENCES[key] = (c, _freeze(oracle_run(oracle, c, alpha, False)), _freeze(oracle_run(oracle_ld, c, alpha, True)))
    return _REFERENCES[key]


def assert_oracle_conditions(c, f64, ld):
    """the conditions of a case on the oracle side: no filter fails in either arithmetic, every env that is handed an action takes its
    update in both"""
    tasked = np.array(c.actions) >= 0
    for what, r in (("float64", f64), ("80-bit", ld)):
        assert not r["status"].any(), (c.name, what, np.where(r["status"])[0])
        assert np.array_equal(r["obs_taken"].astype(bool), tasked), (c.name, what, np.where(r["obs_taken"].astype(bool) != tasked)[0])
        assert np.isfinite(r["x"]).all() and np.isfinite(r["P"]).all(), (c.name, what)
    assert len(c.updated) == tasked.sum() and len(c.updated) + len(c.predicted) == c.E * c.m


def updates(r, c):
    """the envs of r that were handed an action: dict(y [k, 3], S [k, 3, 3]) next to the states"""
    k = np.array(c.actions) >= 0
    return dict(x=r["x"], P=r["P"], y=r["y"][k], S=r["S"][k])


# ---------------------------------------------------------------------------------------------------------------- wrong constants
def _rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


# name -> (the constants handed to the step, the magnitude as the table of DESIGN.md section 4 states it)
WRONG_CONSTANTS = {
    "R (1 + 1e-7)": dict(R_scale=1 + 1e-7),
    "measurement noise (1 + 1e-6)": dict(noise_scale=1 + 1e-6),
    "dt (1 + 1e-9)": dict(dt_scale=1 + 1e-9),
    "c2t row rotated 1e-10 rad": dict(M_rot=1e-10),
    "site moved 1 cm": dict(site_shift=np.array([0.01, 0.0, 0.0])),
    "Wc_i (1 + 1e-8), i >= 1": dict(Wc_scale=1 + 1e-8),
}


def wrong_step(o, c, sl, a, zn, alpha, centred, R_scale=1.0, noise_scale=1.0, dt_scale=1.0, M_rot=0.0, site_shift=0.0, Wc_scale=1.0):
    """run_oracle's call with one constant off: what a kernel with that constant wrong computes, in the oracle's arithmetic"""
    Wm, Wc, scale = orc.merwe_weights(alpha, BETA, KAPPA)
    Wc = Wc.copy()
    Wc[1:] *= Wc_scale
    M = c2t()[c.tix]
    if M_rot:
        M = (_rot_z(M_rot) @ np.asarray(M).reshape(3, 3)).reshape(np.shape(M))
    st = np.zeros(sl.stop - sl.start, dtype=np.int32)
    r = o.env_step(c.xt[sl], c.x[sl], c.P[sl], st, DT * dt_scale, c.g["Q"], c.R * R_scale, Wm, Wc, scale, a, M, c.g["obs_lla"],
                   c.g["obs_itrs"] + site_shift, -np.pi / 2, zn * noise_scale, obs_type=0 if c.obs_type == 'aer' else 1, centred=centred,
                   resample=c.resample)
    r["status"] = st
    return r


# ---------------------------------------------------------------------------------------------------------------- structural mistakes
def _aer2uvw(aer):
    az, el, r = aer[..., 0], aer[..., 1], aer[..., 2]
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], axis=-1)


def _residual_aer(a, b):
    d = a[..., 0] - b[..., 0]
    return np.stack([np.arctan2(np.sin(d), np.cos(d)), a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]], axis=-1)


def inv3_ld(S):
    """the 3 x 3 inverse by cofactors (np.linalg has no long double)"""
    c = np.array([[S[1, 1] * S[2, 2] - S[1, 2] * S[2, 1], S[0, 2] * S[2, 1] - S[0, 1] * S[2, 2], S[0, 1] * S[1, 2] - S[0, 2] * S[1, 1]],
                  [S[1, 2] * S[2, 0] - S[1, 0] * S[2, 2], S[0, 0] * S[2, 2] - S[0, 2] * S[2, 0], S[0, 2] * S[1, 0] - S[0, 0] * S[1, 2]],
                  [S[1, 0] * S[2, 1] - S[1, 1] * S[2, 0], S[0, 1] * S[2, 0] - S[0, 0] * S[2, 1], S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]]], dtype=L)
    return c / (S[0, 0] * c[0, 0] + S[0, 1] * c[1, 0] + S[0, 2] * c[2, 0])


def prior_ld(sf, Q, Wm, Wc, sum_wc_term=True):
    """mean and covariance of propagated points sf [13, 6] in long double, in the kernel's form (csrc/ssa_kernels.hip: covariance_entry):
    with d_i = sf_i - sf_0 and s = m' = Wi sum d_i:  x = sf_0 + m',  P = Wi sum d_i d_i^T - m' s^T - s m'^T + sum(Wc) m' m'^T + Q.
    sum_wc_term=False: the mistake -- the last correction left out"""
    sf, Q, Wm, Wc = (np.asarray(a).astype(L) for a in (sf, Q, Wm, Wc))
    Wi = Wc[1]
    d = sf[1:] - sf[0]
    mp = Wi * d.sum(axis=0)
    P = Wi * np.einsum('ia,ib->ab', d, d) - 2 * np.outer(mp, mp) + Q
    if sum_wc_term:
        P = P + Wc.sum() * np.outer(mp, mp)
    return sf[0] + mp, P


def update_aer_ld(x, P, sf, sh, z, R, Wm, Wc, angle_mean=False):
    """the 'aer' update (oracle/ssa_oracle.c: ukf_update) in long double on the prior x, P, the points sf [13, 6] and their measurements
    sh [13, 3].  angle_mean=True: the mistake -- the predicted measurement as the plain weighted mean of (az, el, range), not mean_z_uvw's
    mean of the local vectors.  Returns dict(x, P, y, S)"""
    x, P, sf, sh, z, R, Wm, Wc = (np.asarray(a).astype(L) for a in (x, P, sf, sh, z, R, Wm, Wc))
    if angle_mean:
        zp = sh[0] + (Wm[1:, None] * (sh[1:] - sh[0])).sum(axis=0)
    else:
        uvw = _aer2uvw(sh)
        mu = uvw[0] + (Wm[1:, None] * (uvw[1:] - uvw[0])).sum(axis=0)
        r = np.sqrt((mu * mu).sum())
        az = np.arctan2(mu[1], mu[0])
        zp = np.array([az + (L(8) * np.arctan(L(1)) if az < 0 else L(0)), np.arcsin(mu[2] / r), r], dtype=L)
    rz = _residual_aer(sh, zp)
    S = np.einsum('i,ia,ib->ab', Wc, rz, rz) + R
    K = np.einsum('i,ia,ib->ab', Wc, sf - x, rz) @ inv3_ld(S)
    y = _residual_aer(z, zp)
    return dict(x=x + K @ y, P=P - K @ (S @ K.T), y=y, S=S)


def restated(oracle_ld, c, alpha, sum_wc_term=True, angle_mean=False):
    """case c ('aer', no resampling) in the long-double restatement on top of the 80-bit oracle's propagated points and sigmas_h: the
    result in the layout of oracle_run (states, and y / S per env).  With both flags at their defaults this is the step itself."""
    assert c.obs_type == 'aer' and not c.resample
    Wm, Wc, scale = orc.merwe_weights(alpha, BETA, KAPPA)
    M, g = c2t()[c.tix], c.g
    n = c.E * c.m
    out = dict(x=np.empty((n, 6)), P=np.empty((n, 6, 6)), y=np.full((c.E, 3), np.nan), S=np.full((c.E, 3, 3), np.nan))
    for j in range(n):
        rc, _, _, sf = oracle_ld.ukf_predict(c.x[j], c.P[j], g["Q"], DT, Wm, Wc, scale, centred=True)
        assert rc == 0
        x, P = prior_ld(sf, g["Q"], Wm, Wc, sum_wc_term)
        e, a = divmod(j, c.m)
        if a == c.actions[e]:
            z = oracle_ld.hx_aer(oracle_ld.propagate(c.xt[j], DT), M, g["obs_lla"], g["obs_itrs"])[0] + c.z_noise[e, c.tix, a]
            u = update_aer_ld(x, P, sf, oracle_ld.hx_aer(sf, M, g["obs_lla"], g["obs_itrs"]), z, c.R, Wm, Wc, angle_mean)
            x, P = u["x"], u["P"]
            out["y"][e], out["S"][e] = u["y"].astype(np.float64), u["S"].astype(np.float64)
        out["x"][j], out["P"][j] = x.astype(np.float64), P.astype(np.float64)
    return out


# ---------------------------------------------------------------------------------------------------------------- lookahead gains
def logdet6_ld(A):
    """log det of a symmetric positive definite 6 x 6 matrix by its Cholesky factor, in long double"""
    A = np.asarray(A).astype(L)
    U = np.zeros((6, 6), dtype=L)
    for j in range(6):
        d = A[j, j] - (U[:j, j] * U[:j, j]).sum()
        assert d > 0, (j, d)
        U[j, j] = np.sqrt(d)
        for k in range(j + 1, 6):
            U[j, k] = (A[j, k] - (U[:j, j] * U[:j, k]).sum()) / U[j, j]
    return 2 * np.log(np.diagonal(U)).sum()


def gains_ld(P_prior, P_post):
    """(trace gain, position trace gain, information gain) of one object from its prior and posterior covariance, in long double, in the
    order of the lookahead's score rows LOOK_TRACE_GAIN, LOOK_POS_TRACE_GAIN, LOOK_INFO_GAIN"""
    Pm, Pp = np.asarray(P_prior).astype(L), np.asarray(P_post).astype(L)
    return np.array([np.trace(Pm) - np.trace(Pp), np.trace(Pm[:3, :3]) - np.trace(Pp[:3, :3]), (logdet6_ld(Pm) - logdet6_ld(Pp)) / 2], dtype=L)


def lookahead_references(o, c, alpha, centred):
    """every object of the one-env case c tasked in turn with zero noise: dict(x [m, 6] prior mean, P_prior, P [m, 6, 6] the posterior of
    the object's own update, gain [m, 3] from that oracle's P- / P+ in long double) and the statuses / obs_taken of all m steps"""
    m = c.m
    out = dict(x=np.empty((m, 6)), P_prior=np.empty((m, 6, 6)), P=np.empty((m, 6, 6)), gain=np.empty((m, 3), dtype=L),
               status=np.empty((m, m), dtype=np.int32), obs_taken=np.empty(m, dtype=bool))
    prior = run_oracle(o, c.xt, c.x, c.P, c.g, -1, c.tix, alpha, centred=centred, z_noise3=np.zeros(3))
    out["x"][:], out["P_prior"][:] = prior["x"], prior["P"]
    for j in range(m):
        r = run_oracle(o, c.xt, c.x, c.P, c.g, j, c.tix, alpha, centred=centred, z_noise3=np.zeros(3))
        out["P"][j], out["status"][j], out["obs_taken"][j] = r["P"][j], r["status"], r["obs_taken"]
        out["gain"][j] = gains_ld(prior["P"][j], r["P"][j])
    return out


# ---------------------------------------------------------------------------------------------------------------- today's bounds
def accepted_by_the_update_parity_test(got, f64, ld, c):
    """whether the updated rows of `got` pass what tests/test_hip_step.py: test_update_parity_every_object asserts of them (the bounds the
    suite had at alpha = 1e-3 / 1e-4 before this module): position and velocity within 1e-5 of the 80-bit value, the median position
    and the median and maximum covariance distance at most 3 x the float64 oracle's plus 1e-12 / 1e-9, y within 1e-3 and S within 1e-2
    innovation sd"""
    sub = lambda d: {k: d[k][c.updated] for k in ("x", "P")}      # noqa: E731
    (gp, gv, gP), (rp, rv, rP) = errs(sub(got), sub(ld)), errs(sub(f64), sub(ld))
    ey, eS = innovation_sd(updates(got, c)["y"], updates(got, c)["S"], updates(ld, c))
    return bool(gp.max() < 1e-5 and gv.max() < 1e-5 and np.median(gP) <= 3 * np.median(rP) + 1e-9 and gP.max() <= 3 * rP.max() + 1e-9
                and np.median(gp) <= 3 * np.median(rp) + 1e-12 and ey.max() < 1e-3 and eS.max() < 1e-2)


# ---------------------------------------------------------------------------------------------------------------- the network scene
NET_M, NET_LAUNCHES, NET_TIME_ROWS = 8, 8, 16
ARCSEC = np.pi / 648000.0


class Net:
    """two sensors as the oracle sees them (its own lla2ecef): an az-el-range one at the default observer, an az-el one at the first
    site of support/sensors.SITES3; masks and sigmas of their own"""
    kinds = ('aer', 'ae')

    def __init__(self, oracle):
        from support.sensors import SITES3
        sites = [(38.828198, -77.305352, 20.0), SITES3[0]]
        self.lla = [np.array([np.radians(la), np.radians(lo), h]) for la, lo, h in sites]
        self.itrs = [oracle.lla2ecef(s) for s in self.lla]
        self.lim = np.radians([15.0, 10.0])
        self.sig = np.array([[(1.0 + k) * ARCSEC, (0.5 + 2.0 * k) * ARCSEC, 1e3 / (1 + k)] for k in range(2)])
        self.R = [np.diag(s ** 2) for s in self.sig]
        self.ang = np.array([k == 'ae' for k in self.kinds])
        self.S = 2
        self.z_noise = np.random.RandomState(77).normal(size=(2, NET_TIME_ROWS, NET_M, 3)) * self.sig[:, None, None, :]

    def params(self):
        from ssa_gym_amd import host
        return host.make_sensor_params(self.lla, self.lim, self.R, NET_TIME_ROWS * NET_M * 3, angles_only=self.ang)


def network_launches(net, oracle_ld):
    """[(time row, (x_true, x, P), [object of sensor 0, object of sensor 1])]: per launch NET_M objects at the step before the one under
    the time row's matrix -- object j placed for sensor j % 2, 10 degrees or more above its mask (below 80), 5 000 .. 30 000 km away,
    propagated DT back with the 80-bit oracle -- with make_batch's filters: 100 km / 100 m/s off the truth, the golden P0"""
    from support.angles_only import place
    g = make_batch(1, seed=0)[3]
    out = []
    for k in range(NET_LAUNCHES):
        tix = 1 + 2 * k
        rs = np.random.RandomState(500 + k)
        xt = np.empty((NET_M, 6))
        for j in range(NET_M):
            s = j % 2
            t = place(net.lla[s], net.itrs[s], c2t()[tix], rs.uniform(0, 2 * np.pi), rs.uniform(net.lim[s] + np.radians(10.0), np.radians(80.0)),
                      rs.uniform(5e6, 3e7), rs)
            xt[j] = oracle_ld.propagate(t, -DT)[0]
        x = xt + rs.normal(size=(NET_M, 6)) * np.array([1e5] * 3 + [1e2] * 3)
        out.append((tix, (xt, x, np.tile(g["P0"], (NET_M, 1, 1))), [2 * ((k + s) % (NET_M // 2)) + s for s in range(2)]))
    return g, out


def network_reference(o, net, g, state, tix, j, s, alpha, ld):
    """sensor s's update of object j: the oracle's env_step from the sensor's site for the az-el-range sensor; its ukf_predict and the
    yardstick of dim_z = 2 (support/angles_only.update_2d: float64, or long double on the 80-bit oracle's points) for the az-el one.
    dict(x, P, y, S) -- y [2], S [2, 2] for the az-el sensor"""
    from support.angles_only import update_2d
    Wm, Wc, scale = orc.merwe_weights(alpha, BETA, KAPPA)
    xt, x, P = state
    M, zn3 = c2t()[tix], net.z_noise[s, tix, j]
    zt = o.hx_aer(o.propagate(xt[j], DT), M, net.lla[s], net.itrs[s])[0]
    assert zt[1] >= net.lim[s] + np.radians(5.0), (j, s, zt)       # (visible, far from the mask)
    if not net.ang[s]:
        st = np.zeros(1, dtype=np.int32)
        r = o.env_step(xt[j:j + 1], x[j:j + 1], P[j:j + 1], st, DT, g["Q"], net.R[s], Wm, Wc, scale, 0, M, net.lla[s], net.itrs[s], net.lim[s],
                       zn3, centred=ld)
        assert st[0] == 0 and r["obs_taken"], (j, s, st)
        return dict(x=r["x"][0], P=r["P"][0], y=r["y"], S=r["S"])
    rc, xp, Pp, sf = o.ukf_predict(x[j], P[j], g["Q"], DT, Wm, Wc, scale, centred=ld)
    assert rc == 0
    r = update_2d(xp, Pp, sf, o.hx_aer(sf, M, net.lla[s], net.itrs[s]), (zt + zn3)[:2], net.R[s][:2, :2], Wm, Wc,
                  dtype=np.longdouble if ld else np.float64, centred=ld)
    assert r is not None
    return {k: np.asarray(r[k], dtype=np.float64) for k in ("x", "P", "y", "S")}


def network_references(oracle, oracle_ld, alpha=ALPHA):
    """(net, g, launches, refs): refs[k][s] = (float64, 80-bit) reference of sensor s's update in launch k; computed once"""
    key = ("network", alpha)
    if key not in _REFERENCES:
        net = Net(oracle)
        g, launches = network_launches(net, oracle_ld)
        refs = [[(network_reference(oracle, net, g, state, tix, acts[s], s, alpha, False),
                  network_reference(oracle_ld, net, g, state, tix, acts[s], s, alpha, True)) for s in range(net.S)]
                for tix, state, acts in launches]
        _REFERENCES[key] = (net, g, launches, refs)
    return _REFERENCES[key]
