"""CPU reference for the J2 EXTENSION propagator (test infrastructure only).

The reference repo has no perturbed propagator on its hot path; its only numerical integrator is
fx_xyz_cowell (envs/dynamics.py:168-201): scipy DOP853, rtol 1e-11, atol 1e-12, with the perturbing
acceleration passed as `ad`.  This module configures exactly that integrator with the J2 acceleration of
poliastro.core.perturbations.J2_perturbation (the function the reference's ecosystem would pass as `ad`),
so the device RK4 stepper is validated against an independent high-order integration.  Parity with the
reference is "unpinned" by construction.
"""
import numpy as np
from scipy.integrate import DOP853, solve_ivp

MU = 398600441800000.0
J2_EARTH = 0.00108263
R_EQ_EARTH = 6378136.6


def j2_accel(r, j2=J2_EARTH, r_eq=R_EQ_EARTH, k=MU):
    rn = np.linalg.norm(r)
    factor = 1.5 * k * j2 * r_eq ** 2 / rn ** 5
    zz = 5.0 * r[2] ** 2 / rn ** 2
    return np.array([zz - 1, zz - 1, zz - 3]) * r * factor


def fx_xyz_cowell_j2(x, dt, j2=J2_EARTH, r_eq=R_EQ_EARTH, rtol=1e-11):
    def f(t, u):
        r = u[:3]
        a = -MU * r / np.linalg.norm(r) ** 3 + j2_accel(r, j2, r_eq)
        return np.concatenate([u[3:], a])
    res = solve_ivp(f, (0, dt), np.asarray(x, dtype=float), rtol=rtol, atol=1e-12, method=DOP853, dense_output=True)
    if not res.success:
        raise RuntimeError("Integration failed")
    return res.sol(dt)


# ---------------------------------------------------------------------------------------------------------------- the RK4 yardstick
# The device's own scheme (csrc/ssa_math.hpp accel_j2 / propagate_j2_rk4) restated in numpy, stage for stage, so that it runs in
# np.float64 (the float64 restatement: what the scheme's rounding costs) and in np.longdouble (the 80-bit yardstick: the scheme's value).
# Against fx_xyz_cowell_j2 it differs by the truncation of RK4 at h = dt / nsub; against the kernels by rounding alone.
def accel_j2(r, j2=J2_EARTH, r_eq=R_EQ_EARTH, dtype=np.float64):
    """r[..., 3] -> a[..., 3] in `dtype`, in accel_j2's order of operations"""
    T = np.dtype(dtype).type
    r = np.asarray(r, dtype=T)
    r2 = r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1] + r[..., 2] * r[..., 2]
    inv_r = T(1) / np.sqrt(r2)
    inv_r2 = inv_r * inv_r
    inv_r3 = inv_r2 * inv_r
    zz = T(5) * r[..., 2] * r[..., 2] * inv_r2
    fj = T(1.5) * T(j2) * T(r_eq) * T(r_eq) * inv_r2
    k0 = -T(MU) * inv_r3
    return np.stack([k0 * r[..., 0] * (T(1) - fj * (zz - T(1))), k0 * r[..., 1] * (T(1) - fj * (zz - T(1))),
                     k0 * r[..., 2] * (T(1) - fj * (zz - T(3)))], axis=-1)


def rk4_j2(x, dt, nsub, j2=J2_EARTH, r_eq=R_EQ_EARTH, dtype=np.float64):
    """x[..., 6] through `nsub` equal classical RK4 sub-steps of dt / nsub, in `dtype` (the result stays in `dtype`)"""
    T = np.dtype(dtype).type
    x = np.asarray(x, dtype=T)
    r, v = x[..., :3], x[..., 3:]
    h = T(dt) / T(int(nsub))
    hh, h6 = T(0.5) * h, h / T(6)
    with np.errstate(all="ignore"):
        for _ in range(int(nsub)):
            k1 = accel_j2(r, j2, r_eq, T)
            v2 = v + hh * k1
            k2 = accel_j2(r + hh * v, j2, r_eq, T)
            v3 = v + hh * k2
            k3 = accel_j2(r + hh * v2, j2, r_eq, T)
            v4 = v + h * k3
            k4 = accel_j2(r + h * v3, j2, r_eq, T)
            r, v = r + h6 * (v + T(2) * v2 + T(2) * v3 + v4), v + h6 * (k1 + T(2) * k2 + T(2) * k3 + k4)
    return np.concatenate([r, v], axis=-1)


def cholesky_upper(A, dtype=np.float64):
    """the plain upper Cholesky factor of A [6, 6] in `dtype`, column by column as LAPACK's dpotf2('U') (oracle/ssa_oracle.c
    cholesky_upper); raises LinAlgError where a pivot is not positive -- no jitter ladder"""
    T = np.dtype(dtype).type
    A = np.asarray(A, dtype=T)
    n = len(A)
    U = np.zeros((n, n), dtype=T)
    for j in range(n):
        ajj = A[j, j]
        for i in range(j):
            ajj = ajj - U[i, j] * U[i, j]
        if not ajj > 0:
            raise np.linalg.LinAlgError("cholesky_upper: pivot %d" % j)
        ajj = np.sqrt(ajj)
        U[j, j] = ajj
        for c in range(j + 1, n):
            s = A[j, c]
            for i in range(j):
                s = s - U[i, j] * U[i, c]
            U[j, c] = s / ajj
    return U


def sigma_points(x, P, scale, dtype=np.float64):
    """filterpy's MerweScaledSigmaPoints.sigma_points in `dtype`: x, x + U[k], x - U[k] (rows of the upper factor of scale * P)"""
    T = np.dtype(dtype).type
    x, P = np.asarray(x, dtype=T), np.asarray(P, dtype=T)
    U = cholesky_upper(T(scale) * P, T)
    return np.concatenate([x[None], x[None] + U, x[None] - U])


def ukf_predict_j2(x, P, Q, dt, Wm, Wc, scale, nsub, j2=J2_EARTH, r_eq=R_EQ_EARTH, dtype=np.float64, centred=False, fx=None):
    """The UKF predict of one filter in `dtype`: sigma points DRAWN in `dtype` (the first rung of the ladder only), each through
    rk4_j2, the weighted mean (centred: about point 0, as oracle/ssa_oracle.c weighted_mean) and covariance in index order, plus Q.
    fx(points[13, 6]) -> [13, 6] replaces the propagation (the pins of this function against the oracle's two-body predict).
    Returns (x-, P-, propagated points), all in `dtype`."""
    T = np.dtype(dtype).type
    Q, Wm, Wc = (np.asarray(a, dtype=T) for a in (Q, Wm, Wc))
    pts = sigma_points(x, P, scale, T)
    sf = rk4_j2(pts, dt, nsub, j2, r_eq, T) if fx is None else np.asarray(fx(pts), dtype=T)
    xm = np.zeros(6, dtype=T)
    if centred:
        for i in range(1, len(sf)):
            xm = xm + Wm[i] * (sf[i] - sf[0])
        xm = sf[0] + xm
    else:
        for i in range(len(sf)):
            xm = xm + Wm[i] * sf[i]
    Pm = np.zeros((6, 6), dtype=T)
    for i in range(len(sf)):
        y = sf[i] - xm
        Pm = Pm + np.outer(y, Wc[i] * y)
    return xm, Pm + Q, sf
