"""Resolution of the operator plug points of an env_config dict (envs/__init__.py:23-28 of the reference) into
the fused-kernel variant, shared by SSA_Tasker_Env and SSA_Tasker_VecEnv so that both accept -- and refuse --
exactly the same configurations."""
import numpy as np

from . import dynamics

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
    from .. import host
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
    {'sites': [(lat, lon, h)] * S (degrees, degrees, metres), 'obs_limit': [S] degrees or None, 'z_sigma': [S] or None}.
    config['observers'] lists 1 <= S <= 8 sites; the optional config['sensor_obs_limit'] / config['sensor_z_sigma'] give per-sensor
    values (S of them; default: the scalar obs_limit / z_sigma / R).  Anything else raises ValueError."""
    sites = config.get('observers')
    lim, zs = config.get('sensor_obs_limit'), config.get('sensor_z_sigma')
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
    return {'sites': [tuple(float(v) for v in row) for row in arr], 'obs_limit': lim, 'z_sigma': zs}
