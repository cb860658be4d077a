"""What SSA_Tasker_Env and SSA_Tasker_VecEnv derive from an env_config dict, in one place so that both accept -- and refuse --
exactly the same configurations and resolve them to the same values: the operator plug points (envs/__init__.py:23-28 of the
reference) as the fused-kernel variant, the sensor network, the filter and site values, the kernel constants and the observation
options (resolve_config); and the two rules both envs apply per episode and per step: the initial-state draw and the reward."""
from types import SimpleNamespace

import numpy as np

from .. import _lib, host
from . import dynamics, sun, transformations
from ._gymshim import spaces

_MODELS = {(("hx", "aer"), ("mean_z", "uvw"), ("residual_z", "aer")): 'aer',
           (("hx", "xyz"), ("mean_z", "xyz"), ("residual_z", "xyz")): 'xyz'}


def resolve_kernel_variant(config):
    """(measurement model 'aer' | 'xyz', propagator 'hybrid' | 'fg' | 'elements' | 'j2') of a config dict.

    The propagator comes from config['propagator'] when given, else from the `fx` token (dynamics.fx_xyz_farnocchia
    -> 'hybrid', the behaviour-faithful variant; fx_xyz_farnocchia_fg -> 'fg', fx_xyz_farnocchia_elements -> 'elements',
    fx_xyz_j2_rk4 -> 'j2'); the reference's own function object of that name maps to 'hybrid'.  Foreign callables and
    hx / mean_z / residual_z combinations without a fused kernel raise NotImplementedError (there is no CPU fallback)."""
    fx_id = dynamics.kernel_id_of(config['fx'], "fx")
    ids = tuple(dynamics.kernel_id_of(config[k], k) for k in ("hx", "mean_z", "residual_z"))
    dynamics.kernel_id_of(config['msqrt'], "msqrt")
    model = _MODELS.get(ids)
    if model is None:
        raise NotImplementedError("hx/mean_z/residual_z combination %s has no fused kernel" % (ids,))
    if fx_id != ("fx", "farnocchia"):
        raise NotImplementedError("fx %r has no fused kernel" % (config['fx'],))
    propagator = config.get('propagator', getattr(dynamics.unwrap_partial(config['fx']), 'propagator', 'hybrid'))
    if propagator not in ('fg', 'elements', 'j2', 'hybrid'):
        raise NotImplementedError("unknown propagator %r" % (propagator,))
    return model, propagator


def resolve_perturbation(config):
    """(J2, R_eq) of the device integrator for this config, or None for the defaults: the acceleration bound to an
    fx_xyz_cowell token (`ad` / ad_kwargs, envs/dynamics.py:168-201 of the reference), or config['ad'] / config['ad_kwargs']
    next to a Cowell / J2 propagator."""
    fx = dynamics.unwrap_partial(config['fx'])
    if config.get('ad') is not None:
        fx = dynamics.fx_xyz_cowell.with_ad(config['ad'], **dict(config.get('ad_kwargs') or {}))
    if hasattr(fx, 'perturbation'):
        return fx.perturbation()
    return None


def kernel_consts(config, Q, R, dt, obs_limit_rad, obs_lla):
    """(ssa_consts, measurement model) for a config dict: the ONE place where SSA_Tasker_Env and SSA_Tasker_VecEnv turn the
    operator tokens and the optional keys `propagator`, `resample_sigmas`, `covariance_form` ('reference' | 'centred';
    default: 'reference' with the 'hybrid' and 'elements' propagators -- the behaviour-faithful variants -- else 'centred'),
    `ad` / `ad_kwargs` into kernel constants."""
    model, propagator = resolve_kernel_variant(config)
    kw = {}
    pert = resolve_perturbation(config)
    if pert is not None:
        if propagator != 'j2':
            raise NotImplementedError("an acceleration (ad) needs the Cowell / J2 propagator, got %r" % (propagator,))
        kw.update(j2=pert[0], r_eq=pert[1])
    consts = host.make_consts(Q, R, config['alpha'], config['beta'], config['kappa'], dt, obs_limit_rad, obs_lla, obs_type=model,
                              propagator=propagator, resample=bool(config.get('resample_sigmas', False)),
                              update_interval=config['update_interval'], covariance=config.get('covariance_form'), **kw)
    return consts, model


MAX_SENSORS = 8


def resolve_sensors(config):
    """the sensor network of a config dict (EXTENSION, no reference counterpart), or None without config['observers']:
    {'sites': [(lat, lon, h)] * S (degrees, degrees, metres), 'obs_limit': [S] degrees or None, 'z_sigma': [S] or None,
    'angles_only': [S] booleans, 'illumination': [S] of None or a limit in degrees, 'orbit': [S] of None or a state of six}.
    config['observers'] lists 1 <= S <= 8 sites; the optional config['sensor_obs_limit'] / config['sensor_z_sigma'] give per-sensor
    values (S of them; default: the scalar obs_limit / z_sigma / R).  The optional config['sensor_measurement'] gives each sensor's
    measurement kind, S strings: 'aer' (azimuth, elevation, range: the default) or 'ae' (azimuth and elevation only, a telescope:
    the update of dim_z = 2); it needs obs_type 'aer' and, for an 'ae' entry, more than one site (a one-site env runs the
    one-observer kernels, which measure az, el and range).  The optional config['sensor_illumination'] gives each sensor None (no
    illumination test: a radar, the default) or a number: the sensor sees only sunlit objects, and only while the Sun is below that
    elevation (degrees, -90 .. 90; -12 is nautical twilight) at its site.  It is independent of the measurement kind and of obs_type
    (a laser ranger needs sunlight too) and needs at least two sites, for the reason 'ae' does.
    A space-based sensor: an entry of config['observers'] may be {'orbit': [x, y, z, vx, vy, vz]} instead of a site -- the
    sensor's state at t_0 in the frame of x_true, metres and m/s; the env propagates it to every row of the trans table on the device
    (orbit_site_table).  Never entry 0: the primary sensor is a ground site.  Such a sensor has no elevation mask -- its line of sight
    must clear the sphere of config['limb_radius'] instead --, so its config['sensor_obs_limit'] entry is None (the one place a None
    may stand in that list), and no night: its config['sensor_illumination'] entry is None or the string 'sunlit' (the object outside
    the Earth's shadow, no test of a site), never a number.  It needs obs_type 'aer'.  Its 'sites' entry is (0, 0, 0), a placeholder
    no kernel reads.  Anything else raises ValueError."""
    sites = config.get('observers')
    orbits = None
    if sites is not None and not isinstance(sites, (str, dict)) and hasattr(sites, '__len__'):
        orbits = [None] * len(sites)
        ground = []
        for k, ent in enumerate(sites):
            if isinstance(ent, dict):
                if set(ent) != {'orbit'}:
                    raise ValueError("config['observers'][%d]: a space-based sensor is {'orbit': [x, y, z, vx, vy, vz]}, got %r" % (k, ent))
                try:
                    st = np.asarray(ent['orbit'], dtype=np.float64)
                except (TypeError, ValueError):
                    st = np.empty(0)
                if st.shape != (6,) or not np.all(np.isfinite(st)):
                    raise ValueError("config['observers'][%d]['orbit'] must be six finite values (x, y, z [m], vx, vy, vz [m/s]), got %r"
                                     % (k, ent['orbit']))
                if k == 0:
                    raise ValueError("config['observers'][0] must be a ground site: the primary sensor (the env's own observer) cannot orbit")
                if config.get('obs_type') != 'aer':
                    raise ValueError("a space-based sensor needs obs_type 'aer', got %r" % (config.get('obs_type'),))
                orbits[k] = st
                ground.append((0.0, 0.0, 0.0))
            else:
                ground.append(ent)
        if any(o is not None for o in orbits):
            sites = ground
    illum = config.get('sensor_illumination')
    if sites is None and illum is not None:
        raise ValueError("config['sensor_illumination'] needs config['observers']")
    lim, zs = config.get('sensor_obs_limit'), config.get('sensor_z_sigma')
    kinds = config.get('sensor_measurement')
    if sites is None and kinds is not None:
        raise ValueError("config['sensor_measurement'] needs config['observers']")
    if sites is None:
        if lim is not None or zs is not None:
            raise ValueError("config['sensor_obs_limit'] / config['sensor_z_sigma'] need config['observers']")
        return None
    try:
        arr = np.asarray(sites, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("config['observers'] must be a list of (lat, lon, h) sites") from None
    if arr.ndim != 2 or arr.shape[1] != 3 or not 1 <= arr.shape[0] <= MAX_SENSORS or not np.all(np.isfinite(arr)):
        raise ValueError("config['observers'] must list 1 .. %d sites (lat, lon, h), got %r" % (MAX_SENSORS, sites))
    S = arr.shape[0]
    orbits = [None] * S if orbits is None else orbits
    moving = [o is not None for o in orbits]
    if lim is not None and any(moving):
        # (an orbiting sensor's entry is None -- there is no elevation mask to give it -- and stands for the placeholder 0 below)
        if isinstance(lim, str) or not hasattr(lim, '__len__') or len(lim) != S:
            raise ValueError("config['sensor_obs_limit'] must give one elevation mask (degrees) per sensor: %d" % S)
        lim = list(lim)
        for k in range(S):
            if moving[k] and lim[k] is not None:
                raise ValueError("config['sensor_obs_limit'][%d] must be None: a space-based sensor has no elevation mask (its line of "
                                 "sight clears config['limb_radius'] instead)" % k)
            if not moving[k] and lim[k] is None:
                raise ValueError("config['sensor_obs_limit'][%d]: a ground site needs an elevation mask (degrees)" % k)
        lim = [0.0 if moving[k] else lim[k] for k in range(S)]
    if lim is not None:
        lim = np.asarray(lim, dtype=np.float64)
        if lim.shape != (S,) or not np.all(np.isfinite(lim)):
            raise ValueError("config['sensor_obs_limit'] must give one elevation mask (degrees) per sensor: %d" % S)
        lim = [float(v) for v in lim]
    if zs is not None:
        if len(zs) != S:
            raise ValueError("config['sensor_z_sigma'] must give one z_sigma per sensor: %d" % S)
        zs = [np.asarray(z, dtype=np.float64) for z in zs]
        if any(z.shape != (3,) or not np.all(np.isfinite(z)) or np.any(z < 0) for z in zs):
            raise ValueError("config['sensor_z_sigma']: every entry is a z_sigma of three non-negative values")
    if kinds is None:
        kinds = ['aer'] * S
    else:
        if isinstance(kinds, str) or not hasattr(kinds, '__len__') or len(kinds) != S:
            raise ValueError("config['sensor_measurement'] must give one measurement kind per sensor: %d" % S)
        kinds = list(kinds)
        if any(not isinstance(k, str) or k not in ('aer', 'ae') for k in kinds):
            raise ValueError("config['sensor_measurement']: every entry is 'aer' or 'ae', got %r" % (kinds,))
        if config.get('obs_type') != 'aer':
            raise ValueError("config['sensor_measurement'] needs obs_type 'aer', got %r" % (config.get('obs_type'),))
        if S == 1 and kinds[0] == 'ae':
            raise ValueError("config['sensor_measurement']: a one-site network cannot be 'ae' -- with one site step(), rollout, "
                             "run_agent, run_policy and lookahead() run the one-observer kernels, which measure az, el and range")
    if illum is None:
        illum = [None] * S
    else:
        if isinstance(illum, str) or not hasattr(illum, '__len__') or len(illum) != S:
            raise ValueError("config['sensor_illumination'] must give one entry per sensor (None or a Sun elevation limit in degrees): %d" % S)
        illum = list(illum)
        for k, v in enumerate(illum):
            if v is None:
                continue
            if moving[k]:      # (no site, no night: the object's own illumination or nothing)
                if not (isinstance(v, str) and v == 'sunlit'):
                    raise ValueError("config['sensor_illumination'][%d]: a space-based sensor takes None or 'sunlit' (the object outside "
                                     "the Earth's shadow; there is no site whose Sun elevation a number could limit), got %r" % (k, v))
                continue
            if isinstance(v, (bool, str)) or not np.isscalar(v) or not np.isreal(v) or not -90.0 <= float(v) <= 90.0:
                raise ValueError("config['sensor_illumination']: every entry is None or a Sun elevation limit in [-90, 90] degrees, "
                                 "got %r" % (illum,))
        illum = [None if v is None else 0.0 if moving[k] else float(v) for k, v in enumerate(illum)]
        if S == 1 and illum[0] is not None:
            raise ValueError("config['sensor_illumination'] needs at least two sites -- with one site step(), rollout, run_agent, "
                             "run_policy and lookahead() run the one-observer kernels, whose visibility is the elevation mask alone")
    return {'sites': [tuple(float(v) for v in row) for row in arr], 'obs_limit': lim, 'z_sigma': zs,
            'angles_only': [k == 'ae' for k in kinds], 'illumination': illum, 'orbit': orbits}


def resolve_config(config):
    """everything SSA_Tasker_Env and SSA_Tasker_VecEnv derive from a config dict, in one place (no GPU needed): the filter and site
    values (z_sigma, R, P_0, x_sigma, Q, obs_lla / obs_itrs / obs_limit of the primary sensor), the sensor network (`net`: None
    without config['observers']; else per-sensor lla, obs_limit, z_sigma, R and ssa_consts), the primary ssa_consts, the
    measurement model, the trans table and the validated observation options.  Sensor 0 of a network is the PRIMARY sensor: its
    site, elevation mask, z_sigma and R are the env's observer."""
    c = SimpleNamespace(obs_type=config['obs_type'], dt=config['time_step'], n=config['steps'], m=config['rso_count'])
    unit = np.array([host.arcsec2rad, host.arcsec2rad, 1])
    if c.obs_type == 'aer':
        c.z_sigma = config['z_sigma'] * unit
    elif c.obs_type == 'xyz':
        c.z_sigma = np.asarray(config['z_sigma'], dtype=np.float64)
    else:
        print('Invalid Observation Type: ' + str(config['obs_type']))
        raise SystemExit
    c.x_sigma = np.array(config['x_sigma'])
    c.Q = host.Q_discrete_white_noise(dim=2, dt=c.dt, var=config['q_sigma'] ** 2, block_size=3, order_by_dim=False)
    c.model, _ = resolve_kernel_variant(config)      # (operator plug points -> fused kernel variant; no CPU fallback)
    c.P_0 = np.copy(np.diag(c.x_sigma ** 2)) if config['P_0'] is None else np.copy(config['P_0'])
    c.R = np.diag(c.z_sigma ** 2) if config['R'] is None else np.copy(config['R'])
    c.obs_lla = np.array(config['observer']) * [host.deg2rad, host.deg2rad, 1]
    c.obs_limit = np.radians(config['obs_limit'])
    net = resolve_sensors(config)
    c.n_sensor = 1 if net is None else len(net['sites'])
    c.net = None
    if net is not None:
        S = c.n_sensor
        lla = np.array(net['sites']) * [host.deg2rad, host.deg2rad, 1]
        lim = np.radians(net['obs_limit']) if net['obs_limit'] is not None else np.full(S, c.obs_limit)
        if net['z_sigma'] is not None:
            zs = np.array([z * (unit if c.obs_type == 'aer' else 1.0) for z in net['z_sigma']])
            R = np.array([np.diag(z ** 2) for z in zs])
        else:
            zs, R = np.tile(c.z_sigma, (S, 1)), np.tile(c.R, (S, 1, 1))
        c.net = SimpleNamespace(lla=lla, obs_limit=lim, z_sigma=zs, R=R, angles_only=np.array(net['angles_only'], dtype=bool),
                                sunlit_only=np.array([v is not None for v in net['illumination']], dtype=bool),
                                sun_limit=np.radians([0.0 if v is None else v for v in net['illumination']]),
                                moving=np.array([o is not None for o in net['orbit']], dtype=bool),
                                orbit=[None if o is None else np.copy(o) for o in net['orbit']])
        c.obs_lla, c.obs_limit = lla[0], lim[0]
        c.z_sigma, c.R = zs[0], np.copy(R[0])
    c.obs_itrs = host.lla2ecef(c.obs_lla)
    # config['obs_dtype'] = 'float64' (default, the reference's) | 'float32' (EXTENSION): the observation handed to the host in single
    # precision -- the step kernel writes its host-facing copy that way (SSA_LAUNCH_MIRROR_F32).  The device state stays float64
    dt = np.dtype(config.get('obs_dtype', np.float64))
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("config['obs_dtype'] must be float64 or float32")
    c.obs_f32 = dt == np.float32
    # config['obs_device'] = True (opt-in, for policies that live on the GPU): step() returns CUDA tensors the kernel wrote, nothing but
    # the statistics crosses PCIe.  config['obs_zero_copy'] = True (opt-in): a view of the host-mapped ring the kernel writes instead of
    # a fresh array per step
    c.obs_device = bool(config.get('obs_device', False))
    c.obs_zero_copy = bool(config.get('obs_zero_copy', False))
    shape = {'flatten': (c.m * 12,), 'aer': (c.m * 4,)}.get(config['obs_returned'], (c.m, 12))
    c.obs_space = spaces.Box(low=np.full(shape, -np.inf), high=np.full(shape, np.inf), dtype=np.float32 if c.obs_f32 else np.float64)
    # config['storage_layout'] = None (default) | 'regime': how the engine STORES the objects; invisible but for speed
    c.storage_layout = config.get('storage_layout', None)
    if c.storage_layout not in (None, 'regime'):
        raise ValueError("config['storage_layout'] must be None or 'regime', not %r" % (c.storage_layout,))
    c.consts, _ = kernel_consts(config, c.Q, c.R, c.dt, c.obs_limit, c.obs_lla)
    # (every sensor's site as kernel constants: their visibility helpers)
    c.sensor_consts = [c.consts] + [kernel_consts(config, c.Q, c.net.R[k], c.dt, c.net.obs_limit[k], c.net.lla[k])[0]
                                    for k in range(1, c.n_sensor)]
    if config.get('trans_matrix') is not None:
        c.trans = np.asarray(config['trans_matrix'], dtype=np.float64).reshape(-1, 3, 3)
    else:
        c.trans = transformations.trans_matrix_table(config['t_0'], c.dt, c.n)
    # the Sun of the illumination test (config['sensor_illumination']): config['sun_table'], [n, 3] unit vectors in the frame
    # of x_true, overrides the ephemeris as config['trans_matrix'] overrides the rotation; the sites' dark words always come from the
    # `trans` and the vectors in force.  Without a sensor that asks for it nothing is computed
    c.sun = c.sun_dark = None
    c.shadow_radius = float(config.get('shadow_radius', host.R_EQ_EARTH))
    if c.net is not None and c.net.sunlit_only.any():
        if not c.shadow_radius >= 0.0:
            raise ValueError("config['shadow_radius'] must be a number >= 0, got %r" % (config.get('shadow_radius'),))
        if config.get('sun_table') is not None:
            c.sun = np.array(config['sun_table'], dtype=np.float64)
            if c.sun.shape != (c.trans.shape[0], 3):
                raise ValueError("config['sun_table'] must be %s unit vectors, one per row of the trans table, got %s"
                                 % ((c.trans.shape[0], 3), c.sun.shape))
        else:
            c.sun = sun.sun_table(config['t_0'], c.dt, c.trans.shape[0])
        c.sun_dark = sun.dark_sites(c.trans, c.sun, c.net.lla, c.net.sun_limit)      # (a bit of a sensor without the test: not read)
    # the space-based sensors (config['observers'] entries {'orbit': ...}): the sphere their line of sight must clear.  What
    # needs no GPU is refused here -- the radius, a sensor that starts inside the sphere --, the rest by orbit_site_table at construction
    c.limb_radius = float(config.get('limb_radius', host.R_EQ_EARTH + 100e3))
    if c.net is not None and c.net.moving.any():
        if not c.limb_radius >= 0.0:
            raise ValueError("config['limb_radius'] must be a number >= 0, got %r" % (config.get('limb_radius'),))
        for k in np.nonzero(c.net.moving)[0]:
            if not np.linalg.norm(c.net.orbit[k][:3]) >= c.limb_radius:
                raise ValueError("config['observers'][%d]: the orbit starts %.0f m from the geocentre, inside config['limb_radius'] = %.0f m"
                                 % (k, np.linalg.norm(c.net.orbit[k][:3]), c.limb_radius))
    return c


def orbit_site_table(c, config):
    """the site rows of the space-based sensors of a resolved config `c` (resolve_config; `config` the dict it came from), float64
    [n_time, S, 16] as host.pack_site_rows packs them, or None without one.  Needs the GPU: every orbit is propagated from its state at
    t_0 to the epoch of every row of the trans table ON THE DEVICE, by the propagator the env's truth uses -- device.propagate (the
    two-body solver of the kernel variant), or device.propagate_j2 for a J2 env --, one step of time_step after another exactly as the
    truth of the objects it watches advances: a sensor is an object.  Row t of sensor s: host.orbit_site_rows of trans[t] and the
    position at row t.  Raises ValueError for an orbit whose propagation fails (a NaN position) or that dips below config['limb_radius']
    at any row."""
    if c.net is None or not c.net.moving.any():
        return None
    import torch
    from .. import device
    idx = [int(k) for k in np.nonzero(c.net.moving)[0]]
    n_time = c.trans.shape[0]
    x = device.as_dev(np.stack([c.net.orbit[k] for k in idx]))
    pos = torch.empty((n_time, len(idx), 3), dtype=torch.float64, device=x.device)
    pos[0] = x[:, :3]
    for t in range(1, n_time):
        if c.consts.propagator == _lib.PROP_J2_RK4:
            x = device.propagate_j2(x, c.dt, c.consts.j2, c.consts.r_eq, c.consts.rk4_substeps)
        else:
            x = device.propagate(x, c.dt, c.consts.propagator)
        pos[t] = x[:, :3]
    pos = pos.cpu().numpy()
    S = c.n_sensor
    enu, obs = np.zeros((n_time, S, 9)), np.zeros((n_time, S, 3))
    for q, k in enumerate(idx):
        r = np.linalg.norm(pos[:, q], axis=1)
        if not np.all(np.isfinite(pos[:, q])):
            raise ValueError("config['observers'][%d]: the orbit's propagation fails at time row %d"
                             % (k, int(np.argmax(~np.isfinite(pos[:, q]).all(axis=1)))))
        if not np.all(r >= c.limb_radius):
            raise ValueError("config['observers'][%d]: the orbit dips to %.0f m from the geocentre at time row %d, below "
                             "config['limb_radius'] = %.0f m" % (k, r.min(), int(np.argmin(r)), c.limb_radius))
        enu[:, k], obs[:, k] = host.orbit_site_rows(c.trans.reshape(-1, 9), pos[:, q])
    return host.pack_site_rows(enu, obs)


def reward_done(reward_type, st, hit, paid, last, m, n):
    """(rewards, dones) of a step from its statistics rows st [E, STAT_STRIDE], for SSA_Tasker_Env and SSA_Tasker_VecEnv alike
    (ssa_tasker_simple_2.py:324-354 of the reference): 'jones' pays 1 and ends the episode when every filter is within 30 km
    (max_dpos < 3e4), ends it unpaid when one is 5000 km off; 'trinary' pays the mean of the two threshold counts (results.py:432);
    'shaped' ends as 'jones' but pays 1 - `paid` (what the episode has paid so far) on the win, else +1/n on a `hit` (the action was
    np.argmax(sigma_pos[i - 1])) and -1/n otherwise; any other reward type pays 0.  `last`: the step is the episode's last, which ends
    it whatever the reward type.  A NaN max_dpos neither wins nor loses.
    One row st [STAT_STRIDE] (a single env's step): scalars in, scalars out with the same bits, at a scalar's cost -- `last` is returned as
    given, and `paid` may be a function, called on a win only (the env sums its reward history for it)."""
    if st.ndim == 1:
        if reward_type == 'trinary':          # (Python floats: the same IEEE double arithmetic, without numpy's scalar overhead)
            return (st.item(_lib.STAT_CNT_LT_1E4) + st.item(_lib.STAT_CNT_LT_1E7)) / m / 2, last
        mx = st.item(_lib.STAT_MAX_DPOS)
        if reward_type == 'jones':
            return (0.0, True) if mx > 5e6 else (1.0, True) if mx < 3e4 else (0.0, last)
        if reward_type == 'shaped':
            if mx > 5e6:
                return 0.0, True
            if mx < 3e4:
                return 1.0 - (paid() if callable(paid) else paid), True
            return (1.0 / n if hit else -1.0 / n), last
        return 0.0, last
    if reward_type == 'trinary':
        return (st[:, _lib.STAT_CNT_LT_1E4] + st[:, _lib.STAT_CNT_LT_1E7]) / m / 2, last
    mx = st[:, _lib.STAT_MAX_DPOS]
    if reward_type not in ('jones', 'shaped'):
        return np.zeros_like(mx), last
    lost, won = mx > 5e6, mx < 3e4
    done = lost | won | last
    if reward_type == 'jones':
        return np.where(won, 1.0, 0.0), done
    return np.where(lost, 0.0, np.where(won, 1.0 - paid, np.where(hit, 1.0 / n, -1.0 / n))), done


def draw_initial_state(rs, orbits, m, x_sigma, bulk, x_noise=None):
    """(x_true, x_filter) of a reset from RandomState `rs`: per object a catalogue row, then six normals scaled by x_sigma -- the
    reference's draw order (ssa_tasker_simple_2.py:206-209) -- or with `bulk` (config['device_rng']) all rows, then all normals: 1 ms
    instead of 40 at m = 20 000.  The noise goes into `x_noise` when given."""
    N = orbits.shape[0]
    x_true = np.empty((m, 6))
    noise = np.empty((m, 6)) if x_noise is None else x_noise
    if bulk:
        x_true[:] = orbits[rs.randint(low=0, high=N, size=m)]
        noise[:] = rs.normal(size=(m, 6)) * x_sigma
    else:
        for j in range(m):
            x_true[j] = orbits[rs.randint(low=0, high=N), :]
            noise[j] = rs.normal(size=6) * x_sigma
    return x_true, x_true + noise
