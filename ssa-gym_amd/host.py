"""Host-side (init-time) logic of the hot path: everything the reference computes ONCE
per environment in SSA_Tasker_Env.__init__ -- filter weights, process noise, observer
geometry -- packed into the `ssa_consts` block the kernels take by value.

None of this is per-step work; it runs in numpy.  Citations: file:line under the
reference root.
"""
from fractions import Fraction

import numpy as np

from . import _lib

arcsec2rad = np.pi / 648000   # envs/transformations.py:14
deg2rad = np.pi / 180         # envs/transformations.py:15
# WGS84 (envs/transformations.py:11-13: a, f = erfa.eform(1))
WGS84_A = 6378137.0
WGS84_F = 0.0033528106647474805

X_FAILED = np.array([1e20, 1e20, 1e20, 1e12, 1e12, 1e12])   # ssa_tasker_simple_2.py:157
P_FAILED = np.diag([1e20, 1e20, 1e20, 1e12, 1e12, 1e12])    # ssa_tasker_simple_2.py:158


def merwe_weights(alpha, beta, kappa, n=6):
    """filterpy MerweScaledSigmaPoints._compute_weights as used at
    ssa_tasker_simple_2.py:211-214.  Returns Wm[2n+1], Wc[2n+1], (n + lambda)."""
    lambda_ = alpha ** 2 * (n + kappa) - n
    c = .5 / (n + lambda_)
    Wc = np.full(2 * n + 1, c)
    Wm = np.full(2 * n + 1, c)
    Wc[0] = lambda_ / (n + lambda_) + (1 - alpha ** 2 + beta)
    Wm[0] = lambda_ / (n + lambda_)
    return Wm, Wc, lambda_ + n


def exact_weight_sums(Wm, Wc):
    """sum(Wm) - 1 and sum(Wc) of the DOUBLE weights, evaluated exactly.  At alpha=1e-4 the
    doubles Wm0 ~ -2e8 and 12*Wi ~ 2e8+1 do not sum to exactly 1 (ulp(2e8) = 3e-8): the
    reference's np.dot(Wm, sigmas) therefore carries the factor sum(Wm) on sigma_0, and the
    centred form used on the device reproduces it."""
    sm = sum(Fraction(float(w)) for w in Wm) - 1
    sc = sum(Fraction(float(w)) for w in Wc)
    return float(sm), float(sc)


def Q_discrete_white_noise(dim, dt=1., var=1., block_size=1, order_by_dim=True):
    """filterpy.common.Q_discrete_white_noise, dim == 2 (call: ssa_tasker_simple_2.py:110)."""
    if dim != 2:
        raise ValueError("the reference only uses dim=2")
    q = np.array([[.25 * dt ** 4, .5 * dt ** 3], [.5 * dt ** 3, dt ** 2]])
    if order_by_dim:
        return np.kron(np.eye(block_size), q) * var
    return np.kron(q, np.eye(block_size)) * var


def lla2ecef(obs_lla):
    """envs/transformations.py:217-235 (observer position, init-time)."""
    a, f = WGS84_A, WGS84_F
    e = np.sqrt(f * (2 - f))
    lat, lon, alt = obs_lla
    N = a / np.sqrt(1 - e ** 2 * np.sin(lat) ** 2)
    x = (N + alt) * np.cos(lat) * np.cos(lon)
    y = (N + alt) * np.cos(lat) * np.sin(lon)
    z = (N * (1 - e ** 2) + alt) * np.sin(lat)
    return np.array([x, y, z])


def enu_matrix(obs_lla):
    """trans_uvw_ecef of ecef2aer (envs/transformations.py:341-343); constant per observer."""
    lat, lon = obs_lla[0], obs_lla[1]
    return np.array([[-np.sin(lat) * np.cos(lon), -np.sin(lon), np.cos(lat) * np.cos(lon)],
                     [-np.sin(lat) * np.sin(lon), np.cos(lon), np.cos(lat) * np.sin(lon)],
                     [np.cos(lat), 0, np.sin(lat)]])


J2_EARTH = 0.00108263      # poliastro Earth.J2 (what the reference's ecosystem would plug into ad=J2_perturbation)
R_EQ_EARTH = 6378136.6     # poliastro Earth.R [m]


def make_consts(Q, R, alpha, beta, kappa, dt, obs_limit_rad, obs_lla, obs_type='aer', propagator='fg',
                resample=False, update_interval=1, j2=J2_EARTH, r_eq=R_EQ_EARTH, rk4_substeps=None, covariance=None):
    """pack the per-environment constants for the kernels (include/ssa_hip.h: ssa_consts).

    covariance: 'reference' = the prior covariance in the reference's own arithmetic (SSA_FLAG_REFERENCE_COV: reproduces the
    reference's episode-level filter failures), 'centred' = the cancellation-free expansion; None = 'reference' with the
    'elements' and 'hybrid' propagators (the behaviour-faithful variants), 'centred' otherwise."""
    Wm, Wc, scale = merwe_weights(alpha, beta, kappa)
    sm, sc = exact_weight_sums(Wm, Wc)
    c = _lib.ssa_consts()
    c.Q[:] = np.asarray(Q, dtype=np.float64).reshape(36)
    c.R[:] = np.asarray(R, dtype=np.float64).reshape(9)
    c.Wm0, c.Wc0, c.Wi = float(Wm[0]), float(Wc[0]), float(Wm[1])
    c.sum_wm_m1, c.sum_wc, c.scale = sm, sc, float(scale)
    c.dt, c.obs_limit = float(dt), float(obs_limit_rad)
    obs_lla = np.asarray(obs_lla, dtype=np.float64)
    c.enu[:] = enu_matrix(obs_lla).reshape(9)
    c.obs_itrs[:] = lla2ecef(obs_lla)
    c.obs_type = {'aer': _lib.OBS_AER, 'xyz': _lib.OBS_XYZ}[obs_type]
    c.propagator = {'elements': _lib.PROP_ELEMENTS, 'fg': _lib.PROP_FG, 'j2': _lib.PROP_J2_RK4, 'hybrid': _lib.PROP_HYBRID}[propagator]
    c.j2, c.r_eq = float(j2), float(r_eq)
    # RK4 sub-step <= 5 s: local error (n h)^5/120 |r| < 1e-6 m even in LEO
    c.rk4_substeps = int(rk4_substeps) if rk4_substeps else max(1, int(np.ceil(abs(dt) / 5.0)))
    if covariance is None:
        covariance = 'reference' if propagator in ('elements', 'hybrid') else 'centred'
    if covariance not in ('reference', 'centred'):
        raise ValueError("covariance must be 'reference' or 'centred', got %r" % (covariance,))
    c.flags = (_lib.FLAG_RESAMPLE if resample else 0) | (_lib.FLAG_REFERENCE_COV if covariance == 'reference' else 0)
    c.update_interval = int(update_interval)
    return c


def pack_sun_rows(sun, dark):
    """the rows of ssa_sensor_params.sun as one float64 array [n, 4]: sun [n, 3] unit vectors from the geocentre to the Sun (the frame
    of x_true), dark [n] integers whose bit s says that site s is dark at that row (envs/sun.py: dark_sites) -- the word's BITS travel in
    the fourth column"""
    sun = np.asarray(sun, dtype=np.float64)
    dark = np.asarray(dark, dtype=np.int64)
    if sun.ndim != 2 or sun.shape[1] != 3 or dark.shape != (sun.shape[0],):
        raise ValueError("a Sun table is [n, 3] vectors and [n] dark words, got %s and %s" % (sun.shape, dark.shape))
    rows = np.empty((sun.shape[0], 4), dtype=np.float64)
    rows[:, :3] = sun
    rows[:, 3] = dark.view(np.float64)
    return rows


SITE_ROW = 16      # doubles per (time row, sensor) of ssa_step_params.site_rows: enu[9], obs_itrs[3], 4 zeros -- 128 bytes


def pack_site_rows(enu, obs):
    """the rows of ssa_step_params.site_rows as one float64 array [n_time, S, 16]: enu [n_time, S, 9] (or [n_time, S, 3, 3]) in the
    element layout of enu_matrix / ssa_sensor_params.enu[s], obs [n_time, S, 3] the sensor's position in the frame `trans` maps into;
    the last 4 words of every row are 0.  Rows of the sensors that do not move are never read: leave them 0."""
    enu = np.asarray(enu, dtype=np.float64)
    obs = np.asarray(obs, dtype=np.float64)
    if enu.ndim == 4 and enu.shape[2:] == (3, 3):
        enu = enu.reshape(enu.shape[0], enu.shape[1], 9)
    if enu.ndim != 3 or enu.shape[2] != 9 or obs.shape != enu.shape[:2] + (3,):
        raise ValueError("site rows are enu [n_time, S, 9] and obs [n_time, S, 3], got %s and %s" % (enu.shape, obs.shape))
    if not 1 <= enu.shape[1] <= _lib.MAX_SENSORS or enu.shape[0] < 1:
        raise ValueError("site rows need n_time >= 1 and 1 .. %d sensors, got %s" % (_lib.MAX_SENSORS, enu.shape[:2]))
    rows = np.zeros(enu.shape[:2] + (SITE_ROW,), dtype=np.float64)
    rows[:, :, :9] = enu
    rows[:, :, 9:12] = obs
    return rows


def orbit_site_rows(trans, r_inertial):
    """the site words of ONE orbiting sensor, (enu [n_time, 9], obs [n_time, 3]) for pack_site_rows: trans [n_time, 9] (or [n_time, 3, 3])
    the matrices of ssa_step_params.trans, r_inertial [n_time, 3] the sensor's position at the same epochs in the frame of x_true.
        obs_t = trans_t . r_t
        enu_t = trans_t        (enu_matrix's element layout; the kernel applies it transposed: uvw[j] = sum_i enu[i][j] d[i])
    so that the kernel's local vector uvw = enu_t^T (trans_t x - obs_t) is x - r_t itself, in INERTIAL axes: with hx_aer_enu's own
    reading of it -- uvw = (north, east, up), az = atan2(east, north) -- east is y, north is x, up is z, the azimuth is the topocentric
    right ascension, the elevation the topocentric declination and the range the slant range."""
    trans = np.asarray(trans, dtype=np.float64)
    r = np.asarray(r_inertial, dtype=np.float64)
    if trans.ndim == 3 and trans.shape[1:] == (3, 3):
        trans = trans.reshape(-1, 9)
    if trans.ndim != 2 or trans.shape[1] != 9 or r.shape != (trans.shape[0], 3):
        raise ValueError("an orbit's site rows need trans [n_time, 9] and r_inertial [n_time, 3], got %s and %s" % (trans.shape, r.shape))
    obs = np.einsum('tij,tj->ti', trans.reshape(-1, 3, 3), r)
    return trans.copy(), obs


def make_sensor_params(sites_lla, obs_limits_rad, Rs, zn_stride_sensor, angles_only=None, sunlit_only=None, shadow_radius=R_EQ_EARTH):
    """pack a sensor network (include/ssa_hip.h: ssa_sensor_params): site s at sites_lla[s] = (lat [rad], lon [rad], h [m]) with elevation
    mask obs_limits_rad[s] and measurement noise covariance Rs[s] (3 x 3); sensor s's noise table starts zn_stride_sensor doubles after
    sensor s - 1's.  angles_only: S booleans, True where sensor s measures azimuth and elevation only (None: every sensor measures
    az, el and range).  sunlit_only: S booleans, True where sensor s sees only sunlit objects, and only while its site is dark (None: no
    sensor tests the illumination); shadow_radius: the radius [m] of the Earth's cylindrical shadow.  The Sun table itself lives on the
    device: engine.set_sun_table points the block at it (`sun` stays NULL here).  Every sensor idle (action -1) and no record destination: the caller sets `action` and `upd` per step."""
    S = len(sites_lla)
    if not 1 <= S <= _lib.MAX_SENSORS or len(obs_limits_rad) != S or len(Rs) != S:
        raise ValueError("a sensor network has 1 .. %d sites, each with one elevation mask and one R" % _lib.MAX_SENSORS)
    sp = _lib.ssa_sensor_params()
    sp.n_sensor = S
    kinds = [False] * S if angles_only is None else [bool(k) for k in angles_only]
    if len(kinds) != S:
        raise ValueError("angles_only has %d entries for %d sensors" % (len(kinds), S))
    sp.angles_only = sum(1 << k for k in range(S) if kinds[k])
    for k in range(_lib.MAX_SENSORS):
        sp.action[k] = -1
    for k in range(S):
        lla = np.asarray(sites_lla[k], dtype=np.float64)
        sp.enu[k][:] = enu_matrix(lla).reshape(9)
        sp.obs_itrs[k][:] = lla2ecef(lla)
        sp.obs_limit[k] = float(obs_limits_rad[k])
        sp.R[k][:] = np.asarray(Rs[k], dtype=np.float64).reshape(9)
    sp.zn_stride_sensor = int(zn_stride_sensor)
    sp.upd = 0
    lit = [False] * S if sunlit_only is None else [bool(k) for k in sunlit_only]
    if len(lit) != S:
        raise ValueError("sunlit_only has %d entries for %d sensors" % (len(lit), S))
    sp.sunlit_only = sum(1 << k for k in range(S) if lit[k])
    sp.shadow_radius = float(shadow_radius) if any(lit) else 0.0
    sp.sun, sp.reserved2 = 0, 0
    return sp

