"""Synthetic orbit catalogue by the reference's own recipe.

The reference ships `envs/1.5_hour_viz_20000_of_20000_sample_orbits_seed_0.npy` (20000x6, m and m/s, GCRS), produced by
envs/orbit_gen.py:30-70: per row a regime is drawn -- LEO / MEO / GEO / Tundra / Molniya with probabilities 1/3, 1/3, 1/9, 1/9, 1/9
(:53) -- and `init_state_vec` (dynamics.py:357-399) candidates of that regime are drawn until one is ACCEPTED (:55-70): propagated over
4 h in 150 s steps it must stay above 300 km altitude and, seen from the observer (38.83 N, 77.31 W) above 15 deg elevation, either be
visible all the time or be visible within the first 45 min and never out of sight for 1.5 h or longer.  Regime shares are therefore
exactly the draw probabilities (6 755 LEO rows in the reference file), every GEO row is equatorial (inc = 0: 2 231 rows) and half of
them circular (1 135: `stationary * ecc`, :383-385), eccentricities reach 0.737 (Molniya); WITHIN a regime the rule shapes the
distribution of inclination, node and phase (a LEO object has to pass over the site on consecutive revolutions).  That file is an
input of the reference repo and does not travel with this package; `synthetic_catalogue` draws rows by the same recipe (vectorised:
not the same random stream), including the exactly circular / equatorial rows that take rv2coe's special branches
(farnocchia.py:278-309).  Workload synthesis for bench.py and the tests -- numpy, no device needed: Kepler's equation in closed
elliptic form for the 96 sample times, the elevation of envs/transformations.py:330-352.
"""
from datetime import datetime

import numpy as np

MU = 398600441800000.0
RE_EQ = 6378136.6   # poliastro Earth.R used by the reference sampler


def coe2rv_host(p, ecc, inc, raan, argp, nu):
    cn, sn = np.cos(nu), np.sin(nu)
    fr, fv = p / (1 + ecc * cn), np.sqrt(MU / p)
    px, py, vx, vy = cn * fr, sn * fr, -sn * fv, (ecc + cn) * fv
    cO, sO, ci, si, cw, sw = np.cos(raan), np.sin(raan), np.cos(inc), np.sin(inc), np.cos(argp), np.sin(argp)
    r00, r01 = cO * cw - sO * ci * sw, -cO * sw - sO * ci * cw
    r10, r11 = sO * cw + cO * ci * sw, -sO * sw + cO * ci * cw
    r20, r21 = si * sw, si * cw
    return np.stack([px * r00 + py * r01, px * r10 + py * r11, px * r20 + py * r21,
                     vx * r00 + vy * r01, vx * r10 + vy * r11, vx * r20 + vy * r21], axis=-1)


def _draw_elements(rs, regime, k):
    """k candidates of one regime, as init_state_vec (dynamics.py:357-399): (a, ecc, inc, raan, argp, nu)"""
    inc = np.radians(rs.uniform(0, 180, k))
    raan = np.radians(rs.uniform(0, 360, k))
    argp = np.radians(rs.uniform(0, 360, k))
    nu = np.radians(rs.uniform(0, 360, k))
    if regime in (0, 1):      # LEO / MEO: exo-atmospheric rejection on the semi-minor axis (:369-382)
        lo, hi = [(RE_EQ + 300e3, RE_EQ + 2000e3), (RE_EQ + 2000e3, RE_EQ + 35786e3)][regime]
        a, ecc = rs.uniform(lo, hi, k), rs.uniform(0, .25, k)
        bad = a * np.sqrt(1 - ecc ** 2) <= RE_EQ + 300e3
        while bad.any():
            a[bad], ecc[bad] = rs.uniform(lo, hi, bad.sum()), rs.uniform(0, .25, bad.sum())
            bad = a * np.sqrt(1 - ecc ** 2) <= RE_EQ + 300e3
    elif regime == 2:         # GEO: inc = 0 always, ecc = 0 for half of them (:383-386)
        stationary = rs.randint(0, 2, k)
        a, ecc, inc = np.full(k, 42164e3), stationary * rs.uniform(0, .25, k), np.zeros(k)
    elif regime == 3:         # Tundra
        a, inc, ecc, argp = np.full(k, 42164e3), np.full(k, np.radians(63.4)), np.full(k, 0.2), np.full(k, np.radians(270))
    else:                     # Molniya
        a, inc, ecc, argp = np.full(k, 26600e3), np.full(k, np.radians(63.4)), np.full(k, 0.737), np.full(k, np.radians(270))
    return a, ecc, inc, raan, argp, nu


def _accepted(a, ecc, inc, raan, argp, nu, M_t, times, enu, obs_itrs, el_min, first, max_gap):
    """orbit_gen.py:55-70 for a batch of candidates: bool[k]"""
    k = len(a)
    cO, sO, ci, si, cw, sw = np.cos(raan), np.sin(raan), np.cos(inc), np.sin(inc), np.cos(argp), np.sin(argp)
    P = np.stack([cO * cw - sO * ci * sw, sO * cw + cO * ci * sw, si * sw], axis=1)          # perifocal unit vectors in GCRS
    Q = np.stack([-cO * sw - sO * ci * cw, -sO * sw + cO * ci * cw, si * cw], axis=1)
    E0 = 2.0 * np.arctan2(np.sqrt(1 - ecc) * np.sin(nu / 2), np.sqrt(1 + ecc) * np.cos(nu / 2))
    M0 = E0 - ecc * np.sin(E0)
    n = np.sqrt(MU / a ** 3)
    b = a * np.sqrt(1 - ecc ** 2)
    ok_alt = np.ones(k, dtype=bool)
    vis = np.empty((len(times), k), dtype=bool)
    for i, t in enumerate(times):
        M = M0 + n * t
        E = M + ecc * np.sin(M)
        for _ in range(12):       # Newton on Kepler's equation (ecc <= 0.737: converged to 1e-14 long before)
            E = E - (E - ecc * np.sin(E) - M) / (1 - ecc * np.cos(E))
        r = (a * (np.cos(E) - ecc))[:, None] * P + (b * np.sin(E))[:, None] * Q
        x = r @ M_t[i].T                                                                        # GCRS -> ITRS
        rn = np.linalg.norm(x, axis=1)
        lat = np.arcsin(x[:, 2] / rn)
        ok_alt &= rn - WGS84_A * (1 - WGS84_F * np.sin(lat) ** 2) > 300e3                      # (geodetic height to ~1 km)
        d = x - obs_itrs
        up = d @ enu[:, 2]
        vis[i] = np.arcsin(up / np.linalg.norm(d, axis=1)) >= el_min
    run = np.zeros(k, dtype=np.int64)
    worst = np.zeros(k, dtype=np.int64)
    for i in range(len(times)):
        run = np.where(vis[i], 0, run + 1)
        worst = np.maximum(worst, run)
    always = vis.all(axis=0)
    return ok_alt & (always | (vis[:first].any(axis=0) & (worst < max_gap)))


WGS84_A, WGS84_F = 6378137.0, 0.0033528106647474805
_CACHE = {}


def synthetic_catalogue(n=20000, seed=0, visibility=True):
    """n rows by orbit_gen.py's recipe (module docstring).  visibility=False: the regime mix and element distributions alone (every
    candidate accepted) -- the catalogue of rounds 1-3 up to its regime probabilities."""
    key = (int(n), int(seed), bool(visibility))
    if key in _CACHE:
        return _CACHE[key].copy()
    if visibility:      # the benchmark's catalogue ships as data (eleven minutes of numpy to draw: LEO candidates pass the rule about
        import os       # once in 1 250; visible_catalogue draws the same rows with the screen on the GPU)
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "synthetic_catalogue_n%d_seed%d.npy" % key[:2])
        if os.path.exists(path):
            _CACHE[key] = np.load(path)
            return _CACHE[key].copy()
    from .envs.transformations import trans_matrix_table
    from . import host
    step, duration = 150.0, 4 * 3600.0
    T = int(np.ceil(duration / step))
    times = step * np.arange(T)
    M_t = trans_matrix_table(datetime(2020, 5, 4, 0, 0, 0), step, T)
    obs_lla = np.array((38.828198, -77.305352, 20.0)) * [host.deg2rad, host.deg2rad, 1]
    enu, obs_itrs = host.enu_matrix(obs_lla), host.lla2ecef(obs_lla)

    def screen(cand):
        if not visibility:
            return np.ones(len(cand[0]), dtype=bool)
        return _accepted(*cand, M_t, times, enu, obs_itrs, np.radians(15.0), int(45 * 60 / step), int(1.5 * 3600 / step))
    out = _draw(n, seed, screen)
    _CACHE[key] = out
    return out.copy()


def _draw(n, seed, screen):
    """orbit_gen.py's draw loop: a regime per row from RandomState(seed), then per regime batches of max(4096, 4 * missing) candidates
    (_draw_elements) of which the first ones `screen(cand) -> bool[batch]` accepts fill the regime's rows, in order.  GCRS states [n, 6]."""
    rs = np.random.RandomState(seed)
    regime = rs.choice(5, size=n, p=[1 / 3, 1 / 3, 1 / 9, 1 / 9, 1 / 9])   # LEO MEO GEO Tundra Molniya (orbit_gen.py:53)
    el = np.empty((n, 6))
    for k in range(5):
        idx = np.where(regime == k)[0]
        got = 0
        while got < idx.size:
            batch = max(4096, 4 * (idx.size - got))
            cand = _draw_elements(rs, k, batch)
            ok = screen(cand)
            sel = np.where(ok)[0][:idx.size - got]
            el[idx[got:got + sel.size]] = np.stack([c[sel] for c in cand], axis=1)
            got += sel.size
    a, ecc, inc, raan, argp, nu = el.T
    return np.ascontiguousarray(coe2rv_host(a * (1 - ecc ** 2), ecc, inc, raan, argp, nu))


DEFAULT_SITE = (38.828198, -77.305352, 20.0)    # orbit_gen.py's observer (env_config['observer'])
MAX_SITES = 8


def _site_table(sites, el_min_deg):
    """[S, 13] rows of ssa_screen_params.sites for 1 .. 8 sites (lat, lon, h) in degrees, degrees, metres, and one elevation mask
    (degrees) for all of them or one per site.  Anything else raises ValueError."""
    from . import host
    try:
        arr = np.asarray(sites, dtype=np.float64)
        lim = np.asarray(el_min_deg, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("sites must be a list of (lat, lon, h) and el_min_deg a number or one per site") from None
    if arr.ndim != 2 or arr.shape[1] != 3 or not 1 <= arr.shape[0] <= MAX_SITES or not np.all(np.isfinite(arr)):
        raise ValueError("sites must list 1 .. %d finite sites (lat, lon, h), got %r" % (MAX_SITES, sites))
    S = arr.shape[0]
    if lim.ndim == 0:
        lim = np.full(S, float(lim))
    if lim.shape != (S,) or not np.all(np.isfinite(lim)):
        raise ValueError("el_min_deg must be one finite elevation mask (degrees) or one per site: %d" % S)
    tab = np.empty((S, 13))
    for s in range(S):
        lla = arr[s] * [host.deg2rad, host.deg2rad, 1]
        tab[s, :9] = host.enu_matrix(lla).reshape(9)
        tab[s, 9:12] = host.lla2ecef(lla)
        tab[s, 12] = np.radians(lim[s])
    return tab


def visible_catalogue(n, seed=0, *, sites=(DEFAULT_SITE,), el_min_deg=15.0, t_0=datetime(2020, 5, 4), step=150.0,
                      duration=4 * 3600.0, first_window=45 * 60.0, max_gap=1.5 * 3600.0, min_altitude=300e3):
    """n rows by orbit_gen.py's recipe, screened on the GPU for a network of 1 .. 8 sites (lat, lon, h; deg, deg, m) with elevation
    masks el_min_deg (one for all or one per site), from epoch t_0: the draw loop of synthetic_catalogue (same RandomState(seed), same
    regimes, batches and element draws) with _accepted replaced by the device screen (ssa_catalogue_screen_f64), so that with the
    defaults the rows are those of synthetic_catalogue(n, seed).  A candidate is kept if over `duration`, sampled every `step` seconds,
    it stays above min_altitude and is either always visible from some site, or visible within first_window and never out of sight
    of every site for max_gap or longer.  Always draws (no shipped file, no cache); needs the library and a GPU."""
    n, step, duration = int(n), float(step), float(duration)
    if n < 0:
        raise ValueError("n must be >= 0, got %d" % n)
    if not np.isfinite(step) or step <= 0:
        raise ValueError("step must be a positive number of seconds, got %r" % step)
    if not np.isfinite(duration) or duration < step:
        raise ValueError("duration must be at least one step (%r s), got %r" % (step, duration))
    for name, v in (("first_window", first_window), ("max_gap", max_gap), ("min_altitude", min_altitude)):
        if not np.isfinite(float(v)) or (name != "min_altitude" and float(v) < 0):
            raise ValueError("%s must be a finite%s number, got %r" % (name, "" if name == "min_altitude" else " non-negative", v))
    tab = _site_table(sites, el_min_deg)
    T = int(np.ceil(duration / step))
    first, gap = int(first_window / step), int(max_gap / step)
    from .envs.transformations import trans_matrix_table
    from . import _lib, device
    import torch
    M_t = trans_matrix_table(t_0, step, T)
    _lib.load()
    if not torch.cuda.is_available():
        raise _lib.SsaHipError("visible_catalogue screens on the GPU (there is no CPU fallback): no device")
    trans, site_tab = device.as_dev(M_t), device.as_dev(tab)

    def screen(cand):
        acc = device.catalogue_screen(device.as_dev(np.stack(cand, axis=1)), trans, site_tab, step, min_altitude, first, gap)
        return acc.cpu().numpy().astype(bool)
    return _draw(n, seed, screen)


def catalogue_for_config(config, n=20000, seed=0, **kw):
    """visible_catalogue for the sensors of an env_config dict: the sites of config['observers'] (else config['observer']), the masks of
    config['sensor_obs_limit'] (else el_min_deg, default 15 deg -- not the env's obs_limit, -90 by default, which accepts everything)
    and config['t_0'].  Keyword arguments override these and pass through to visible_catalogue.
    The screen is on the GROUND sites only: a space-based sensor of config['observers'] ({'orbit': ...}) and its
    sensor_obs_limit entry (None) are left out -- nothing is screened from orbit, so an object only such a sensor could see is dropped.
    catalogue_for_network screens by the network's own rule instead: from orbit, and with a telescope's night and the Earth's shadow."""
    args = {}
    if config.get('observers') is not None:
        orbiting = [isinstance(s, dict) for s in config['observers']]
        args['sites'] = [tuple(s) for s, o in zip(config['observers'], orbiting) if not o]
        if config.get('sensor_obs_limit') is not None:
            lim = list(config['sensor_obs_limit'])
            args['el_min_deg'] = [v for v, o in zip(lim, orbiting) if not o] if any(orbiting) and len(lim) == len(orbiting) else lim
    elif config.get('observer') is not None:
        args['sites'] = [tuple(config['observer'])]
    if config.get('t_0') is not None:
        args['t_0'] = config['t_0']
    args.update(kw)
    return visible_catalogue(n, seed, **args)


def _network_sensors(sensors, el_min_deg, illumination):
    """the sensors of visible_catalogue_network, checked (no GPU): (sites [S] of (lat, lon, h) with (0, 0, 0) in an orbit's place, masks
    [S] in degrees with 0 in an orbit's place, orbits [S] of a state [6] or None, sun limits [S] in degrees or None, sunlit_only word).
    Anything else raises ValueError."""
    if isinstance(sensors, (str, dict)) or not hasattr(sensors, '__len__') or not 1 <= len(sensors) <= MAX_SITES:
        raise ValueError("sensors must list 1 .. %d entries, (lat, lon, h) or {'orbit': [x, y, z, vx, vy, vz]}, got %r" % (MAX_SITES, sensors))
    S = len(sensors)
    sites, orbits = [], []
    for k, ent in enumerate(sensors):
        if isinstance(ent, dict):
            if set(ent) != {'orbit'}:
                raise ValueError("sensors[%d]: a space-based sensor is {'orbit': [x, y, z, vx, vy, vz]}, got %r" % (k, ent))
            try:
                st = np.asarray(ent['orbit'], dtype=np.float64)
            except (TypeError, ValueError):
                st = np.empty(0)
            if st.shape != (6,) or not np.all(np.isfinite(st)):
                raise ValueError("sensors[%d]['orbit'] must be six finite values (x, y, z [m], vx, vy, vz [m/s]), got %r" % (k, ent['orbit']))
            orbits.append(st)
            sites.append((0.0, 0.0, 0.0))
        else:
            orbits.append(None)
            sites.append(ent)
    moving = [o is not None for o in orbits]
    if np.ndim(el_min_deg) == 0 and el_min_deg is not None:
        masks = [0.0 if m else el_min_deg for m in moving]
    else:
        if isinstance(el_min_deg, str) or not hasattr(el_min_deg, '__len__') or len(el_min_deg) != S:
            raise ValueError("el_min_deg must be one elevation mask (degrees) or one entry per sensor (None for an orbit): %d" % S)
        for k, v in enumerate(el_min_deg):
            if moving[k] != (v is None):
                raise ValueError("el_min_deg[%d]: a space-based sensor takes None (its line of sight clears limb_radius instead), a ground "
                                 "site an elevation mask in degrees, got %r" % (k, v))
        masks = [0.0 if m else v for m, v in zip(moving, el_min_deg)]
    _site_table(sites, masks)      # (the sites and masks themselves: finite numbers, three per site)
    if illumination is None:
        illumination = [None] * S
    if isinstance(illumination, str) or not hasattr(illumination, '__len__') or len(illumination) != S:
        raise ValueError("illumination must be None or one entry per sensor: %d" % S)
    limits, word = [], 0
    for k, v in enumerate(illumination):
        if v is None:
            limits.append(None)
            continue
        if moving[k]:
            if not (isinstance(v, str) and v == 'sunlit'):
                raise ValueError("illumination[%d]: a space-based sensor takes None or 'sunlit', got %r" % (k, v))
            limits.append(0.0)      # (no site, no night: the dark bit of a moving sensor is never read)
        else:
            if isinstance(v, (bool, str)) or not np.isscalar(v) or not np.isreal(v) or not -90.0 <= float(v) <= 90.0:
                raise ValueError("illumination[%d]: a ground site takes None or a Sun elevation limit in [-90, 90] degrees, got %r" % (k, v))
            limits.append(float(v))
        word |= 1 << k
    return sites, masks, orbits, limits, word


def _orbit_positions(orbits, step, T, limb_radius):
    """[T, S, 3]: every orbiting sensor's inertial position at the samples i * step, by repeated two-body steps of `step` on the device
    (device.propagate, as _config.orbit_site_table); zeros for a ground site.  ValueError for an orbit that fails or dips below limb_radius."""
    import torch
    from . import device
    idx = [k for k, o in enumerate(orbits) if o is not None]
    x = device.as_dev(np.stack([orbits[k] for k in idx]))
    dev_pos = torch.empty((T, len(idx), 3), dtype=torch.float64, device=x.device)
    dev_pos[0] = x[:, :3]
    for t in range(1, T):
        x = device.propagate(x, step)
        dev_pos[t] = x[:, :3]
    dev_pos = dev_pos.cpu().numpy()
    pos = np.zeros((T, len(orbits), 3))
    for q, k in enumerate(idx):
        if not np.all(np.isfinite(dev_pos[:, q])):
            raise ValueError("sensors[%d]: the orbit's propagation fails at sample %d" % (k, int(np.argmax(~np.isfinite(dev_pos[:, q]).all(axis=1)))))
        r = np.linalg.norm(dev_pos[:, q], axis=1)
        if not np.all(r >= limb_radius):
            raise ValueError("sensors[%d]: the orbit dips to %.0f m from the geocentre at sample %d, below limb_radius = %.0f m"
                             % (k, r.min(), int(np.argmin(r)), limb_radius))
        pos[:, k] = dev_pos[:, q]
    return pos


def visible_catalogue_network(n, seed=0, *, sensors, el_min_deg=15.0, illumination=None, t_0=datetime(2020, 5, 4), step=150.0,
                              duration=4 * 3600.0, first_window=45 * 60.0, max_gap=1.5 * 3600.0, min_altitude=300e3,
                              limb_radius=RE_EQ + 100e3, shadow_radius=RE_EQ, sun_table=None):
    """visible_catalogue by the network's OWN visibility rule (ssa_catalogue_screen_network_f64): the same draw loop
    (_draw: same RandomState(seed), regimes, batches and element draws), the same altitude floor, first window and gap rule, but
    sensor s sees a sample as the env's kernels would let it.
      sensors: 1 .. 8 entries, each a ground site (lat, lon, h; deg, deg, m) or a space-based sensor {'orbit': [x, y, z, vx, vy, vz]},
        its state at t_0 in the frame of x_true -- at any position of the list, position 0 included (the screen has no primary observer).
      el_min_deg: one elevation mask for every ground site, or one entry per sensor with None for an orbit, whose line of sight must
        clear the sphere of limb_radius (host.R_EQ_EARTH + 100 km) instead.
      illumination: None, or one entry per sensor as config['sensor_illumination']: for a ground site None or the Sun elevation limit in
        degrees below which the site is dark; for an orbit None or 'sunlit'.  A sensor with an entry sees only candidates outside the
        Earth's cylindrical shadow of shadow_radius (host.R_EQ_EARTH), a ground site only while it is dark.
    The tables stand at the screen's own samples t_0 + i * step: trans_matrix_table, the Sun (envs.sun.sun_table, or sun_table [T, 3]
    unit vectors in the frame of x_true), the sites' dark words (envs.sun.dark_sites) and every orbit's positions.  An orbit is
    propagated on the device by repeated steps of `step` (device.propagate): TWO-BODY, whatever propagator an env will use later -- the
    screen's candidates are two-body too.  An orbit that fails or dips below limb_radius at any sample raises ValueError, as every bad
    shape does.  With ground sites only and no illumination the rows are visible_catalogue's exactly.  Always draws; needs the
    library and a GPU."""
    n, step, duration = int(n), float(step), float(duration)
    if n < 0:
        raise ValueError("n must be >= 0, got %d" % n)
    if not np.isfinite(step) or step <= 0:
        raise ValueError("step must be a positive number of seconds, got %r" % step)
    if not np.isfinite(duration) or duration < step:
        raise ValueError("duration must be at least one step (%r s), got %r" % (step, duration))
    for name, v in (("first_window", first_window), ("max_gap", max_gap), ("min_altitude", min_altitude)):
        if not np.isfinite(float(v)) or (name != "min_altitude" and float(v) < 0):
            raise ValueError("%s must be a finite%s number, got %r" % (name, "" if name == "min_altitude" else " non-negative", v))
    sites, masks, orbits, limits, sunlit_only = _network_sensors(sensors, el_min_deg, illumination)
    S = len(sites)
    site_moving = sum(1 << k for k, o in enumerate(orbits) if o is not None)
    T = int(np.ceil(duration / step))
    first, gap = int(first_window / step), int(max_gap / step)
    if site_moving:
        if not float(limb_radius) >= 0.0:
            raise ValueError("limb_radius must be a number >= 0, got %r" % (limb_radius,))
        for k, o in enumerate(orbits):
            if o is not None and not np.linalg.norm(o[:3]) >= limb_radius:
                raise ValueError("sensors[%d]: the orbit starts %.0f m from the geocentre, inside limb_radius = %.0f m"
                                 % (k, np.linalg.norm(o[:3]), limb_radius))
    sun_vec = None
    if sunlit_only:
        if not float(shadow_radius) >= 0.0:
            raise ValueError("shadow_radius must be a number >= 0, got %r" % (shadow_radius,))
        if sun_table is not None:
            sun_vec = np.array(sun_table, dtype=np.float64)
            if sun_vec.shape != (T, 3):
                raise ValueError("sun_table must be %s unit vectors, one per sample t_0 + i * step, got %s" % ((T, 3), sun_vec.shape))
    from .envs.transformations import trans_matrix_table
    from .envs import sun as sun_mod
    from . import _lib, device, host
    import torch
    tab = _site_table(sites, masks)
    M_t = trans_matrix_table(t_0, step, T)
    sun_rows = None
    if sunlit_only:
        if sun_vec is None:
            sun_vec = sun_mod.sun_table(t_0, step, T)
        lla = np.array(sites, dtype=np.float64) * [host.deg2rad, host.deg2rad, 1]
        dark = sun_mod.dark_sites(M_t, sun_vec, lla, np.radians([0.0 if v is None else v for v in limits]))
        sun_rows = host.pack_sun_rows(sun_vec, dark)
    _lib.load()
    if not torch.cuda.is_available():
        raise _lib.SsaHipError("visible_catalogue_network screens on the GPU (there is no CPU fallback): no device")
    rows = None
    if site_moving:
        pos = _orbit_positions(orbits, step, T, float(limb_radius))
        enu, obs = np.zeros((T, S, 9)), np.zeros((T, S, 3))
        for k, o in enumerate(orbits):
            if o is not None:
                enu[:, k], obs[:, k] = host.orbit_site_rows(M_t.reshape(-1, 9), pos[:, k])
        rows = device.as_dev(host.pack_site_rows(enu, obs))
    trans, site_tab = device.as_dev(M_t), device.as_dev(tab)
    sun_dev = None if sun_rows is None else device.as_dev(sun_rows)

    def screen(cand):
        acc = device.catalogue_screen_network(device.as_dev(np.stack(cand, axis=1)), trans, site_tab, step, min_altitude, first, gap,
                                              site_rows=rows, site_moving=site_moving, limb_radius=limb_radius, sun=sun_dev,
                                              sunlit_only=sunlit_only, shadow_radius=shadow_radius)
        return acc.cpu().numpy().astype(bool)
    return _draw(n, seed, screen)


def catalogue_for_network(config, n=20000, seed=0, **kw):
    """visible_catalogue_network for the sensors of an env_config dict: config['observers'] (else config['observer']) with the
    space-based ones kept, config['sensor_obs_limit'], config['sensor_illumination'], config['limb_radius'], config['shadow_radius'] and
    config['t_0'].  Keyword arguments override these and pass through.  A config['sun_table'] stands on the ENV's time rows (t_0 + i *
    time_step), not on the screen's samples: a config that has one raises ValueError unless the caller passes sun_table= for the
    screen's own samples."""
    args = {}
    if config.get('observers') is not None:
        args['sensors'] = [dict(s) if isinstance(s, dict) else tuple(s) for s in config['observers']]
    elif config.get('observer') is not None:
        args['sensors'] = [tuple(config['observer'])]
    if config.get('observers') is not None and config.get('sensor_obs_limit') is not None:
        args['el_min_deg'] = list(config['sensor_obs_limit'])
    for key, name in (('sensor_illumination', 'illumination'), ('limb_radius', 'limb_radius'), ('shadow_radius', 'shadow_radius'),
                      ('t_0', 't_0')):
        if config.get(key) is not None:
            args[name] = list(config[key]) if key == 'sensor_illumination' else config[key]
    if config.get('sun_table') is not None and kw.get('sun_table') is None:
        raise ValueError("config['sun_table'] is on the env's time rows, not the screen's samples: pass sun_table= [T, 3] for t_0 + i * step")
    args.update(kw)
    return visible_catalogue_network(n, seed, **args)


def regime_order(x, tile=4, n_xcd=8, one_tile_limit=20480):
    """a permutation of the objects (rows of x: GCRS states) that puts objects of the same regime into the same wavefronts: ascending
    semi-major axis, the sorted list dealt in chunks of one tile (4 objects = one wavefront) round-robin over the 8 XCDs' runs of tiles, so
    that every XCD gets the same share of every regime.  Why it matters (round 4, profiles/r04_sorted_tiles_experiment.txt): with the
    behaviour-faithful propagator the filters that leave the strong-elliptic regime late in an episode are the LEO objects (6 795 of 6 806;
    0 of the 13 194 others); in catalogue order they are spread over 76 % of the wavefronts, each of which then runs the conic chain
    and the jitter ladder for one or two of its four objects.  Returns order[m]: new position -> original row (m a multiple of tile * n_xcd;
    otherwise -- and beyond 20 480 objects, where a wavefront walks several tiles -- the plain sort)."""
    x = np.asarray(x)
    a = 1.0 / (2.0 / np.linalg.norm(x[:, :3], axis=1) - np.sum(x[:, 3:] ** 2, axis=1) / MU)
    L = np.argsort(a, kind="stable")
    m = len(L)
    nt = m // tile
    if m % (tile * n_xcd) or m > one_tile_limit:
        # (more than 20 480 objects: a wavefront walks several tiles, stride = the number of wavefronts -- in plain sorted order every wavefront's
        # walk then runs from the slowest regime to the fastest, the same mix for all of them)
        return L
    q = nt // n_xcd
    order = np.empty(m, dtype=np.int64)
    for c in range(nt):
        t = (c % n_xcd) * q + c // n_xcd
        order[tile * t:tile * t + tile] = L[tile * c:tile * c + tile]
    return order


def regime_order_env(x, e, n_env, tile=4):
    """the layout of env e of a vector env's batch (HotPathEngine.set_layout with several envs): the plain sort by semi-major axis, ROTATED
    by e / n_env of the env's tiles.  The batch is one launch in which a wavefront walks one tile of every env at the same position (8 envs
    x 20 000 objects: wavefront w takes tile w of each); sorted alike, a wavefront would meet the slow regime in all of its tiles or in none
    -- rotated, every walk runs through the same mix (the single env's rule beyond 20 480 objects, regime_order).  Returns order[m]."""
    x = np.asarray(x)
    a = 1.0 / (2.0 / np.linalg.norm(x[:, :3], axis=1) - np.sum(x[:, 3:] ** 2, axis=1) / MU)
    L = np.argsort(a, kind="stable")
    nt = len(L) // tile
    if nt < n_env or len(L) % tile:
        return L
    return np.roll(L, -tile * ((e * nt) // n_env))
