"""The Sun for the illumination test of a sensor network (EXTENSION, no reference counterpart): its direction in the
env's inertial frame and the rows at which a site is dark.  Init-time work in numpy, as everything in host.py: the kernels take the
result as a table (include/ssa_hip.h: ssa_sensor_params.sun) and never compute an ephemeris.

The direction is the Astronomical Almanac's low-precision series ("Low precision formulas for the Sun", section C; stated accuracy
0.01 degrees between 1950 and 2050):
    n = days of TT from J2000.0
    L = 280.460 + 0.9856474 n       mean longitude, corrected for aberration          [degrees]
    g = 357.528 + 0.9856003 n       mean anomaly
    lambda = L + 1.915 sin g + 0.020 sin 2g,  beta = 0                               ecliptic longitude and latitude
The series refers to the mean equinox and ecliptic OF DATE; x_true and `trans` refer to the GCRS, whose axes are those of J2000 to
17 mas (the frame bias, ignored).  In 2020 the equinox of date lies 0.28 degrees of longitude from that of J2000 -- 28 times the series'
own error -- so the longitude is brought to J2000 by taking the general precession in longitude off (IAU 2006: p_A = 5028.796195" T +
1.1054348" T^2, T in Julian centuries of TT from J2000) and the vector is formed with the J2000 obliquity 84381.406".  What is left
out: the motion of the ecliptic itself (47" per century in obliquity: 0.003 degrees by 2020), nutation (the GCRS has none) and the
Sun's latitude (< 1.2")."""
from datetime import timedelta

import numpy as np

from . import earth_orientation as eo

DEG = np.pi / 180
AS2R = np.pi / 648000
EPS_J2000 = 84381.406 * AS2R          # IAU 2006 obliquity of the ecliptic at J2000.0
MJD_J2000 = 51544.5


def tt_days_j2000(t):
    """days of TT from J2000.0 (2000-01-01 12:00 TT) of the UTC datetime `t`: the calendar day by earth_orientation.cal2jd, the leap
    seconds by earth_orientation.dat, TT - TAI = 32.184 s"""
    _, djm = eo.cal2jd(t.year, t.month, t.day)
    fd = (60.0 * (60.0 * t.hour + t.minute) + t.second + t.microsecond * 1e-6) / 86400.0
    return (djm - MJD_J2000) + fd + (eo.dat(t.year, t.month, t.day, fd) + 32.184) / 86400.0


def sun_gcrs(t):
    """the unit vector from the geocentre to the Sun in the GCRS at the UTC datetime `t` (or a sequence of them: [n, 3])"""
    single = not hasattr(t, '__len__')
    n = np.array([tt_days_j2000(ti) for ti in ([t] if single else t)], dtype=np.float64)
    L = 280.460 + 0.9856474 * n
    g = (357.528 + 0.9856003 * n) * DEG
    lam_date = (L + 1.915 * np.sin(g) + 0.020 * np.sin(2 * g)) * DEG
    T = n / 36525.0
    lam = lam_date - (5028.796195 * T + 1.1054348 * T * T) * AS2R      # (the mean equinox of J2000)
    v = np.stack([np.cos(lam), np.cos(EPS_J2000) * np.sin(lam), np.sin(EPS_J2000) * np.sin(lam)], axis=-1)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    return v[0] if single else v


def sun_table(t_0, dt, n):
    """[n, 3]: sun_gcrs at t_0 + i * dt, i < n -- the rows of transformations.trans_matrix_table(t_0, dt, n)"""
    return sun_gcrs([t_0 + timedelta(seconds=dt) * i for i in range(n)])


def site_up(sites_lla):
    """[S, 3]: the geodetic up vector of every site (lat [rad], lon [rad], h) in the ITRS"""
    lla = np.asarray(sites_lla, dtype=np.float64).reshape(-1, 3)
    lat, lon = lla[:, 0], lla[:, 1]
    return np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], axis=-1)


def dark_sites(trans, sun, sites_lla, limits_rad):
    """[n] int64 words: bit s of word t set where site s is dark at time row t -- the Sun's elevation there, sin(el) = up_s . (trans[t]
    . sun[t]), strictly below limits_rad[s].  trans [n, 3, 3] GCRS->ITRS, sun [n, 3] unit vectors in the GCRS, sites_lla [S, 3] (lat
    [rad], lon [rad], h [m]).  The Sun is taken at infinity (its parallax, at most 4.3e-5 rad, is ignored).  A NaN anywhere: not dark."""
    trans = np.asarray(trans, dtype=np.float64).reshape(-1, 3, 3)
    sun = np.asarray(sun, dtype=np.float64).reshape(-1, 3)
    lim = np.asarray(limits_rad, dtype=np.float64).reshape(-1)
    up = site_up(sites_lla)
    if sun.shape[0] != trans.shape[0] or lim.shape[0] != up.shape[0] or up.shape[0] > 63:
        raise ValueError("dark_sites: one Sun vector per matrix and one limit per site (at most 63 sites)")
    s_itrs = np.einsum('nij,nj->ni', trans, sun)
    el = np.arcsin(np.clip(np.einsum('sk,nk->ns', up, s_itrs), -1.0, 1.0))      # [n, S]
    dark = el < lim[None, :]
    return (dark.astype(np.int64) << np.arange(up.shape[0], dtype=np.int64)[None, :]).sum(axis=1).astype(np.int64)
