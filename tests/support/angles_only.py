"""Angles-only sensors (ssa_sensor_params.angles_only; config['sensor_measurement']): the numpy yardstick of the update with dim_z = 2,
written so that it runs in float64 and in np.longdouble; the refusal harness of all nine entries that take the sensor block; and the
small scene of the GPU tests -- objects placed at a chosen (az, el, range) from the site that tasks them."""
import numpy as np

from support.refusals import ENTRIES

KINDS = ('aer', 'ae', 'ae')          # the mixed network of the tests: sensor 0 a radar, sensors 1 and 2 telescopes
MASKS_DEG = [15.0, 5.0, 25.0]
SITES = [(38.828198, -77.305352, 20.0), (39.6, -76.1, 150.0), (38.1, -78.6, 400.0)]      # three sites that share passes
MU = 3.986004418e14
ARCSEC = np.pi / 648000.0
ALPHA, DT = 1e-3, 20.0
SENSOR_ENTRIES = [e for e in ENTRIES if "sensors" in e] + ["ssa_dryrun_sensors_envs_f64"]


# ---------------------------------------------------------------------------------------------------------------- the yardstick
def _aer2uvw(aer):
    az, el, r = aer[..., 0], aer[..., 1], aer[..., 2]
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], axis=-1)


def predicted_ae(sigmas_h, Wm, centred=False):
    """the first two components of uvw2aer(mean_z_uvw(sigmas_h, Wm)) in sigmas_h's dtype: the weighted mean of the points' local
    vectors in index order (centred: about point 0, the same mathematics since sum(Wm) = 1), then azimuth in [0, 2 pi) and elevation"""
    T = sigmas_h.dtype.type
    uvw = _aer2uvw(sigmas_h)
    m = np.zeros(3, dtype=T)
    if centred:
        for i in range(1, len(uvw)):
            m = m + Wm[i] * (uvw[i] - uvw[0])
        m = uvw[0] + m
    else:
        for i in range(len(uvw)):
            m = m + Wm[i] * uvw[i]
    az = np.arctan2(m[1], m[0])
    if az < 0:
        az = az + T(8) * np.arctan(T(1))
    return np.array([az, np.arcsin(m[2] / np.sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]))], dtype=T)


def residual_ae(a, b):
    """residual_z_aer's first two components: the azimuth difference wrapped into (-pi, pi], the elevation difference"""
    d = a[..., 0] - b[..., 0]
    return np.stack([np.arctan2(np.sin(d), np.cos(d)), a[..., 1] - b[..., 1]], axis=-1)


def inv2(S):
    """the 2 x 2 inverse written out (np.linalg.inv has no longdouble); None for a singular or non-finite S"""
    det = S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]
    if det == 0 or not np.isfinite(det):
        return None
    return np.array([[S[1, 1], -S[0, 1]], [-S[1, 0], S[0, 0]]], dtype=S.dtype) / det


def update_2d(x, P, sigmas_f, sigmas_h, z, R2, Wm, Wc, dtype=np.float64, centred=False):
    """The UKF update with dim_z = 2 (filterpy's, as oracle/ukf_numpy restates it) of an az-el sensor, in `dtype`: x-, P- [6], [6, 6];
    sigmas_f [13, 6] the points handed to update(); sigmas_h [13, 3] the sensor's hx (az, el, range) of them -- the range enters the
    predicted measurement through mean_z_uvw and nothing else; z [2] the measurement; R2 the upper-left 2 x 2 block of the sensor's R.
    Returns dict(x, P, y, S, K, zp) in `dtype`, or None where S is singular."""
    T = np.dtype(dtype).type
    x, P, sf, sh, z, R2, Wm, Wc = (np.asarray(a).astype(T) for a in (x, P, sigmas_f, sigmas_h, z, R2, Wm, Wc))
    zp = predicted_ae(sh, Wm, centred)
    rz = residual_ae(sh[:, :2], zp)
    S = np.zeros((2, 2), dtype=T)
    for k in range(len(rz)):
        S = S + Wc[k] * np.outer(rz[k], rz[k])
    S = S + R2
    SI = inv2(S)
    if SI is None:
        return None
    Pxz = np.zeros((6, 2), dtype=T)
    for k in range(len(rz)):
        Pxz = Pxz + Wc[k] * np.outer(sf[k] - x, rz[k])
    K = np.dot(Pxz, SI)
    y = residual_ae(z, zp)
    return dict(x=x + np.dot(K, y), P=P - np.dot(K, np.dot(S, K.T)), y=y, S=S, K=K, zp=zp, Pxz=Pxz)


# ---------------------------------------------------------------------------------------------------------------- refusals
def sensor_blocks(entry, n_env=None):
    """complete, valid blocks of any of the nine entries that take the sensor block (support/refusals.py; the dry run: support/dryrun.py)"""
    if entry == "ssa_dryrun_sensors_envs_f64":
        from support import dryrun
        return dryrun.valid_blocks() if n_env is None else dryrun.valid_blocks(n_env=n_env)
    from support.refusals import valid_blocks
    return valid_blocks(entry, n_env)


def answer(lib, entry, *fields, n_env=None, spoil=None):
    """the code `entry` answers its valid blocks (2 sensors) with the (block, field, value) fields spoiled; nothing is launched, so every
    call must break at least one rule"""
    from ssa_gym_amd import _lib
    from support.refusals import refused
    # (a binding without the word would leave a block spoiled only there complete -- and a complete block is launched)
    assert any(name == "angles_only" for name, _ in _lib.ssa_sensor_params._fields_), "ssa_sensor_params has no angles_only word"
    return refused(getattr(lib, entry), sensor_blocks(entry, n_env), *fields, spoil=spoil)


# ---------------------------------------------------------------------------------------------------------------- the GPU scene
def _frame(site):
    lat, lon = site[0], site[1]
    e = np.array([-np.sin(lon), np.cos(lon), 0.0])
    n = np.array([-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)])
    u = np.array([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])
    return e, n, u


def place(site, itrs, M, az, el, rng, rs):
    """a GCRS state whose ITRS position is seen from `site` at (az, el, range) under M; velocity: circular, in a random plane"""
    e, n, u = _frame(site)
    p = np.asarray(M).reshape(3, 3).T @ (itrs + rng * (np.cos(el) * np.cos(az) * n + np.cos(el) * np.sin(az) * e + np.sin(el) * u))
    w = np.cross(p, rs.normal(size=3))
    v = np.sqrt(MU / np.linalg.norm(p)) * w / np.linalg.norm(w)
    return np.concatenate([p, v])


class Net:
    """the three sensors as the oracle sees them (its own lla2ecef), their kinds, and the network packed for the kernels"""

    def __init__(self, oracle, kinds=KINDS):
        self.lla = [np.array([np.radians(la), np.radians(lo), h]) for la, lo, h in SITES]
        self.itrs = [oracle.lla2ecef(s) for s in self.lla]
        self.lim = np.radians(MASKS_DEG)
        self.sig = np.array([[(1.0 + k) * ARCSEC, (0.5 + 2.0 * k) * ARCSEC, 1e3 / (1 + k)] for k in range(3)])
        self.R = [np.diag(s ** 2) for s in self.sig]
        self.ang = np.array([k == 'ae' for k in kinds])
        self.S = 3

    def params(self, zn_stride_sensor, R=None, kinds=True):
        from ssa_gym_amd import host
        return host.make_sensor_params(self.lla, self.lim, self.R if R is None else R, zn_stride_sensor,
                                       angles_only=self.ang if kinds else None)


def owner_of(j):
    """the sensor object j is placed for (and tasked by)"""
    return j % 3


X_SIGMA = np.array([1e3] * 3 + [1.0] * 3)      # the filter's offset from the truth, 1 sigma: 1 km, 1 m/s -- and the covariance that says so


def scene(net, oracle_ld, M, m, seed, high=False):
    """m objects at the step before the one under M: object j above the mask of sensor owner_of(j) by 10 degrees at least and below
    80 degrees, 1 000 .. 30 000 km away, propagated DT back with the 80-bit oracle so that the step's own prediction brings it there;
    the filter X_SIGMA off the truth, its covariance diag(X_SIGMA^2): a consistent filter, as a tasked object's is.  (With the
    catalogue's initial covariance of (100 km)^2 against a range sigma of 1 km, P+ = P- - K S K^T is the difference of numbers 10^4
    times its size, the float64 reference's own P+ is off by up to 1e-2 standard deviations, and the maximum over 32 samples of such a
    tail says little about either side.)  high: 50 degrees or more above the horizon and 12 000 km or more away instead -- every
    site of the network (some 200 km apart) then sees every object, for several steps."""
    rs = np.random.RandomState(seed)
    xt, x = np.empty((m, 6)), np.empty((m, 6))
    for j in range(m):
        s = owner_of(j)
        t = place(net.lla[s], net.itrs[s], M, rs.uniform(0, 2 * np.pi),
                  rs.uniform(np.radians(50.0) if high else net.lim[s] + np.radians(10.0), np.radians(80.0)), rs.uniform(1.2e7 if high else 1e6, 3e7), rs)
        xt[j] = oracle_ld.propagate(t, -DT)[0]
        x[j] = xt[j] + rs.normal(size=6) * X_SIGMA
    return xt, x, np.tile(np.diag(X_SIGMA ** 2), (m, 1, 1))


def mixed_cfg(E, m=8, kinds=KINDS, **over):
    """an env config with the three sites, the tests' masks and sigmas, and the mixed kinds"""
    cfg = dict(E.env_config)
    cfg.update(rso_count=m, steps=16, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3, observers=SITES,
               sensor_obs_limit=MASKS_DEG, sensor_z_sigma=[(1, 1, 1e3), (2, 2, 5e2), (0.5, 0.5, 2e3)])
    if kinds is not None:
        cfg.update(sensor_measurement=list(kinds))
    cfg.update(over)
    return cfg
