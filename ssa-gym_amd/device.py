"""Thin torch front-end over the C ABI: PyTorch only owns device memory and streams here.

Every function takes/returns CUDA (ROCm) float64 tensors laid out exactly like the
reference's numpy arrays and launches on torch's current stream (the sensor-network
launchers: on the `stream` they are given, see _stream).  There is no CPU path:
a CPU tensor or a missing library raises.
"""
import ctypes as C

import torch

from . import _lib

f64 = torch.float64


def _chk(t, name, dtype=f64):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.SsaHipError("%s must be a CUDA tensor (the hot path has no CPU fallback)" % name)
    if t.dtype != dtype or not t.is_contiguous():
        raise _lib.SsaHipError("%s must be contiguous %s" % (name, dtype))
    return t.data_ptr()


def _chk_n(t, name, dtype, n):
    """_chk of an optional tensor that holds exactly n elements: its pointer, None for None"""
    if t is None:
        return None
    ptr = _chk(t, name, dtype)
    if t.numel() != n:
        raise _lib.SsaHipError("%s must hold %d %s words" % (name, n, dtype))
    return ptr


def _stream(stream=None):
    """the raw handle of `stream`: None (torch's current stream), a torch.cuda.Stream, or the handle itself"""
    if stream is None:
        return torch.cuda.current_stream().cuda_stream
    return stream.cuda_stream if isinstance(stream, torch.cuda.Stream) else stream


def as_dev(a, device="cuda", dtype=f64):
    if not isinstance(a, torch.Tensor):
        import numpy as np
        a = np.asarray(a)
        if not a.flags.writeable or not a.flags.c_contiguous:
            a = np.array(a, order="C")   # torch refuses read-only / strided numpy views
    return torch.as_tensor(a, dtype=dtype).contiguous().to(device)


def propagate(x, dt, propagator=_lib.PROP_FG, out=None):
    """P1-P5: fx_xyz_farnocchia for every row of x[n,6]."""
    lib = _lib.load()
    n = x.shape[0]
    out = torch.empty_like(x) if out is None else out
    _lib.check(lib.ssa_propagate_f64(_chk(x, "x"), _chk(out, "out"), n, float(dt), int(propagator), _stream()),
               "ssa_propagate_f64")
    return out


def propagate_j2(x, dt, j2, r_eq, substeps, out=None):
    """extension: two-body + J2, RK4 with `substeps` steps per dt."""
    lib = _lib.load()
    n = x.shape[0]
    out = torch.empty_like(x) if out is None else out
    _lib.check(lib.ssa_propagate_j2_f64(_chk(x, "x"), _chk(out, "out"), n, float(dt), float(j2), float(r_eq),
                                        int(substeps), _stream()), "ssa_propagate_j2_f64")
    return out


def kepler_elements(x, dt):
    lib = _lib.load()
    n = x.shape[0]
    coe = torch.empty((n, 8), dtype=f64, device=x.device)
    _lib.check(lib.ssa_kepler_elements_f64(_chk(x, "x"), _chk(coe, "coe"), n, float(dt), _stream()),
               "ssa_kepler_elements_f64")
    return coe


def robust_cholesky(A):
    """U2: returns (U[n,6,6] upper, rung[n])."""
    lib = _lib.load()
    n = A.shape[0]
    U = torch.empty_like(A)
    rung = torch.empty(n, dtype=torch.int32, device=A.device)
    _lib.check(lib.ssa_robust_cholesky6_f64(_chk(A, "A"), _chk(U, "U"), _chk(rung, "rung", torch.int32), n, _stream()),
               "ssa_robust_cholesky6_f64")
    return U, rung


def ladder_probe(A, scale):
    """U2 as the fused step kernels run it (ssa_ladder_probe_f64): returns (rung[n], mask[n], U[n,6,6]) -- the rung of the kernels' one-pass
    ladder on scale * A, and which of the sixteen rungs factorise in that arithmetic (bit i; bit 16 = the plain attempt)."""
    lib = _lib.load()
    n = A.shape[0]
    U = torch.empty_like(A)
    rung = torch.empty(n, dtype=torch.int32, device=A.device)
    mask = torch.empty(n, dtype=torch.int32, device=A.device)
    _lib.check(lib.ssa_ladder_probe_f64(_chk(A, "A"), float(scale), _chk(rung, "rung", torch.int32), _chk(mask, "mask", torch.int32),
                                        _chk(U, "U"), n, _stream()), "ssa_ladder_probe_f64")
    return rung, mask, U


def sigma_points(x, P, scale):
    """U1: returns (sigmas[n,13,6], fail[n])."""
    lib = _lib.load()
    n = x.shape[0]
    sig = torch.empty((n, 13, 6), dtype=f64, device=x.device)
    fail = torch.empty(n, dtype=torch.int32, device=x.device)
    _lib.check(lib.ssa_sigma_points_f64(_chk(x, "x"), _chk(P, "P"), float(scale), _chk(sig, "sig"),
                                        _chk(fail, "fail", torch.int32), n, _stream()), "ssa_sigma_points_f64")
    return sig, fail


def hx_aer(x, M, consts):
    """H1: az/el/range of x[n,>=3] seen through GCRS->ITRS matrix M[3,3]."""
    lib = _lib.load()
    n = x.shape[0]
    z = torch.empty((n, 3), dtype=f64, device=x.device)
    _lib.check(lib.ssa_hx_aer_f64(_chk(x, "x"), x.shape[1], _chk(M, "M"), C.byref(consts), _chk(z, "z"), n, _stream()),
               "ssa_hx_aer_f64")
    return z


def mean_z_uvw(sigmas, consts):
    lib = _lib.load()
    n = sigmas.shape[0]
    zp = torch.empty((n, 3), dtype=f64, device=sigmas.device)
    _lib.check(lib.ssa_mean_z_uvw_f64(_chk(sigmas, "sigmas"), C.byref(consts), _chk(zp, "zp"), n, _stream()),
               "ssa_mean_z_uvw_f64")
    return zp


def residual_z_aer(a, b):
    lib = _lib.load()
    n = a.shape[0]
    c = torch.empty_like(a)
    _lib.check(lib.ssa_residual_z_aer_f64(_chk(a, "a"), _chk(b, "b"), _chk(c, "c"), n, _stream()),
               "ssa_residual_z_aer_f64")
    return c


def visible_mask(x_true, M, consts, want_el=False):
    """V1: object_visibility() for every row of x_true[n,6]."""
    lib = _lib.load()
    n = x_true.shape[0]
    mask = torch.empty(n, dtype=torch.uint8, device=x_true.device)
    el = torch.empty(n, dtype=f64, device=x_true.device) if want_el else None
    _lib.check(lib.ssa_visible_mask_f64(_chk(x_true, "x_true"), _chk(M, "M"), C.byref(consts),
                                        _chk(mask, "mask", torch.uint8), _chk(el, "el") if want_el else None, n,
                                        _stream()), "ssa_visible_mask_f64")
    return (mask, el) if want_el else mask


def sunlit_mask(x_true, sun_row, shadow_radius):
    """the sensor kernels' sunlit rule (ssa_sunlit_mask_f64) for every row of x_true[n,6] against one row of a Sun table, sun_row[>=3] =
    (sx, sy, sz, ...) on the device: uint8 mask[n], 1 where the object is outside the Earth's cylindrical shadow of that radius."""
    lib = _lib.load()
    n = x_true.shape[0]
    mask = torch.empty(n, dtype=torch.uint8, device=x_true.device)
    if sun_row.numel() < 3:
        raise _lib.SsaHipError("sun_row must hold the three components of the Sun's direction")
    _lib.check(lib.ssa_sunlit_mask_f64(_chk(x_true, "x_true"), _chk(sun_row, "sun_row"), float(shadow_radius),
                                       _chk(mask, "mask", torch.uint8), n, _stream()), "ssa_sunlit_mask_f64")
    return mask


def los_mask(x_true, trans_row, site_row, limb_radius):
    """the sensor kernels' line-of-sight rule of a moving sensor (ssa_los_mask_f64) for every row of x_true[n,6] against one row of the
    trans table, trans_row[9], and one row of a site table, site_row[16] = (enu[9], obs_itrs[3], 4 unread words), all on the device:
    uint8 mask[n], 1 where the segment from the sensor to the object stays outside the sphere of radius limb_radius."""
    lib = _lib.load()
    n = x_true.shape[0]
    mask = torch.empty(n, dtype=torch.uint8, device=x_true.device)
    if trans_row.numel() < 9 or site_row.numel() < 12:
        raise _lib.SsaHipError("trans_row must hold 9 words and site_row the 12 site words")
    _lib.check(lib.ssa_los_mask_f64(_chk(x_true, "x_true"), _chk(trans_row, "trans_row"), _chk(site_row, "site_row"), float(limb_radius),
                                    _chk(mask, "mask", torch.uint8), n, _stream()), "ssa_los_mask_f64")
    return mask


def catalogue_screen(elements, trans, sites, step, min_alt, first, max_gap, want_gap=False, want_flags=False):
    """catalogue._accepted for every candidate row of elements[n,6] (a, ecc, inc, raan, argp, nu), seen from a network of sites[S,13]
    (enu 9 as host.enu_matrix, obs_itrs 3, el_min [rad]) through trans[T,3,3]: accept[n] uint8, plus worst_gap[n] int32 and flags[n]
    uint8 (bit 0 altitude ok, bit 1 visible in the first window, bit 2 always visible) on request."""
    lib = _lib.load()
    n, dev = elements.shape[0], elements.device
    accept = torch.empty(n, dtype=torch.uint8, device=dev)
    gap = torch.empty(n, dtype=torch.int32, device=dev) if want_gap else None
    flags = torch.empty(n, dtype=torch.uint8, device=dev) if want_flags else None
    p = _lib.ssa_screen_params(n=n, n_time=trans.shape[0], n_site=sites.shape[0], step=float(step), min_alt=float(min_alt),
                               first=int(first), max_gap=int(max_gap), elements=_chk(elements, "elements"), trans=_chk(trans, "trans"),
                               sites=_chk(sites, "sites"), accept=_chk(accept, "accept", torch.uint8),
                               worst_gap=_chk(gap, "worst_gap", torch.int32) if want_gap else None,
                               flags=_chk(flags, "flags", torch.uint8) if want_flags else None)
    _lib.check(lib.ssa_catalogue_screen_f64(C.byref(p), _stream()), "ssa_catalogue_screen_f64")
    if not (want_gap or want_flags):
        return accept
    return (accept,) + ((gap,) if want_gap else ()) + ((flags,) if want_flags else ())


def catalogue_screen_network(elements, trans, sites, step, min_alt, first, max_gap, *, site_rows=None, site_moving=0, limb_radius=0.0,
                             sun=None, sunlit_only=0, shadow_radius=0.0, want_gap=False, want_flags=False, want_seen_by=False):
    """catalogue_screen by the network's own visibility rule (ssa_catalogue_screen_network_f64): sensor s with bit s of site_moving is
    screened by line of sight from its rows of site_rows[T,S,16] (host.pack_site_rows) past the sphere of limb_radius -- sites[s] is
    not read --, sensor s with bit s of sunlit_only additionally needs the candidate outside the Earth's cylindrical shadow of
    shadow_radius and, on the ground, bit s of the dark word of sun[T,4] (host.pack_sun_rows).  Returns accept[n] uint8, plus
    worst_gap[n] int32, flags[n] uint8 and seen_by[n] uint8 (bit s: sensor s sees the candidate at some sample) on request, in that
    order.  With both words 0 the outputs are catalogue_screen's."""
    lib = _lib.load()
    n, dev = elements.shape[0], elements.device
    T, S = trans.shape[0], sites.shape[0]
    accept = torch.empty(n, dtype=torch.uint8, device=dev)
    gap = torch.empty(n, dtype=torch.int32, device=dev) if want_gap else None
    flags = torch.empty(n, dtype=torch.uint8, device=dev) if want_flags else None
    seen = torch.empty(n, dtype=torch.uint8, device=dev) if want_seen_by else None
    p = _lib.ssa_screen_network_params(
        site_rows=_chk_n(site_rows, "site_rows", f64, T * S * 16), sun=_chk_n(sun, "sun", f64, T * 4),
        limb_radius=float(limb_radius), shadow_radius=float(shadow_radius), site_moving=int(site_moving), sunlit_only=int(sunlit_only),
        seen_by=_chk(seen, "seen_by", torch.uint8) if want_seen_by else None, reserved=0)
    p.base = _lib.ssa_screen_params(n=n, n_time=T, n_site=S, step=float(step), min_alt=float(min_alt),
                                    first=int(first), max_gap=int(max_gap), elements=_chk(elements, "elements"), trans=_chk(trans, "trans"),
                                    sites=_chk(sites, "sites"), accept=_chk(accept, "accept", torch.uint8),
                                    worst_gap=_chk(gap, "worst_gap", torch.int32) if want_gap else None,
                                    flags=_chk(flags, "flags", torch.uint8) if want_flags else None)
    _lib.check(lib.ssa_catalogue_screen_network_f64(C.byref(p), _stream()), "ssa_catalogue_screen_network_f64")
    if not (want_gap or want_flags or want_seen_by):
        return accept
    return (accept,) + ((gap,) if want_gap else ()) + ((flags,) if want_flags else ()) + ((seen,) if want_seen_by else ())


def observe(x_true, x, P, obs=None, metrics=None):
    """O1/O2: observations() + error() -> obs[n,12], metrics[4,n]."""
    lib = _lib.load()
    n = x.shape[0]
    obs = torch.empty((n, 12), dtype=f64, device=x.device) if obs is None else obs
    metrics = torch.empty((4, n), dtype=f64, device=x.device) if metrics is None else metrics
    _lib.check(lib.ssa_observe_f64(_chk(x_true, "x_true"), _chk(x, "x"), _chk(P, "P"), _chk(obs, "obs"),
                                   _chk(metrics, "metrics"), n, _stream()), "ssa_observe_f64")
    return obs, metrics


def aer_obs(x, P, M, consts, out=None):
    """O4: aer_obs() -> out[n,4]."""
    lib = _lib.load()
    n = x.shape[0]
    out = torch.empty((n, 4), dtype=f64, device=x.device) if out is None else out
    _lib.check(lib.ssa_aer_obs_f64(_chk(x, "x"), _chk(P, "P"), _chk(M, "M"), C.byref(consts), _chk(out, "out"), n,
                                   _stream()), "ssa_aer_obs_f64")
    return out


_stats_ws = {}


def stats_workspace(n_env, dev):
    """device scratch of the two-launch statistics reduction (cached per (device, n_env))."""
    key = (str(dev), int(n_env))
    if key not in _stats_ws:
        nbytes = _lib.load().ssa_reward_stats_workspace_bytes(int(n_env))
        _stats_ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return _stats_ws[key]


def reward_stats(metrics, status, n_obj, n_env=1, out=None):
    """O3: per-env reductions -> stats[E, STAT_STRIDE]."""
    lib = _lib.load()
    out = torch.empty((n_env, _lib.STAT_STRIDE), dtype=f64, device=metrics.device) if out is None else out
    ws = stats_workspace(n_env, metrics.device)
    _lib.check(lib.ssa_reward_stats_f64(_chk(metrics, "metrics"), _chk(status, "status", torch.int32),
                                        _chk(out, "stats"), ws.data_ptr(), int(n_obj), int(n_env), _stream()),
               "ssa_reward_stats_f64")
    return out


def agent_scores(x_true, x_cur, P_cur, P_prev, M, consts, want_mask=True):
    """agents.py primitives: scores[4, n] (trace P | log det ratio | delta_pos | delta_vel) and the visibility mask."""
    lib = _lib.load()
    n = x_cur.shape[0]
    scores = torch.empty((4, n), dtype=f64, device=x_cur.device)
    mask = torch.empty(n, dtype=torch.uint8, device=x_cur.device) if want_mask else None
    _lib.check(lib.ssa_agent_scores_f64(_chk(x_true, "x_true"), _chk(x_cur, "x_cur"), _chk(P_cur, "P_cur"),
                                        _chk(P_prev, "P_prev") if P_prev is not None else None,
                                        _chk(M, "M") if want_mask else None, C.byref(consts), _chk(scores, "scores"),
                                        _chk(mask, "mask", torch.uint8) if want_mask else None, n, _stream()),
               "ssa_agent_scores_f64")
    return scores, mask


def agent_scores_at(x_true, x_cur, P_cur, P_prev, trans, env_time, time_offset, consts):
    """agent_scores() with the GCRS -> ITRS matrix picked ON THE DEVICE: row (env_time[0] + time_offset) % n_time of the table `trans`
    (callers inside a captured graph, whose time index the graph advances between replays)."""
    lib = _lib.load()
    n = x_cur.shape[0]
    scores = torch.empty((4, n), dtype=f64, device=x_cur.device)
    mask = torch.empty(n, dtype=torch.uint8, device=x_cur.device)
    _lib.check(lib.ssa_agent_scores_at_f64(_chk(x_true, "x_true"), _chk(x_cur, "x_cur"), _chk(P_cur, "P_cur"),
                                           _chk(P_prev, "P_prev") if P_prev is not None else None, _chk(trans, "trans"),
                                           _chk(env_time, "env_time", torch.int32), int(time_offset), int(trans.shape[0]), C.byref(consts),
                                           _chk(scores, "scores"), _chk(mask, "mask", torch.uint8), n, _stream()), "ssa_agent_scores_at_f64")
    return scores, mask


def visible_mask_at(x_true, trans, env_time, time_offset, consts):
    """visible_mask() with the matrix picked on the device (see agent_scores_at)"""
    lib = _lib.load()
    n = x_true.shape[0]
    mask = torch.empty(n, dtype=torch.uint8, device=x_true.device)
    _lib.check(lib.ssa_visible_mask_at_f64(_chk(x_true, "x_true"), _chk(trans, "trans"), _chk(env_time, "env_time", torch.int32), int(time_offset),
                                           int(trans.shape[0]), C.byref(consts), _chk(mask, "mask", torch.uint8), None, n, _stream()),
               "ssa_visible_mask_at_f64")
    return mask


def agent_select_workspace(n_obj, n_env, device):
    """device scratch of ssa_agent_select_f64 for n_env envs of n_obj objects (one call at a time)"""
    nbytes = int(_lib.load().ssa_agent_select_workspace_bytes(int(n_obj), int(n_env)))
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)


def agent_select(consts, kind, x_true, x_cur, P_cur, P_prev, trans, env_time, time_offset, fallback=None, workspace=None, obj_ids=None):
    """ssa_agent_select_f64 (ssa_agent_select_ids_f64 with obj_ids, one env): for every env e -- objects e*n_obj .. +n_obj of the
    [n_env * n_obj] state, n_env = env_time.shape[0] -- the first maximum of agent `kind`'s score (_lib.AGENT_*) over the objects it
    considers, NaN skipped, or fallback[e] when none qualifies (-1 without fallback).  Returns (action int32 [n_env], pick int64
    [n_env, 2]: the arg-max, -1 = none, and the winning score's bit pattern)."""
    lib = _lib.load()
    n_env = env_time.shape[0]
    n_obj = x_cur.shape[0] // n_env
    dev = x_cur.device
    ws = agent_select_workspace(n_obj, n_env, dev) if workspace is None else workspace
    action = torch.empty(n_env, dtype=torch.int32, device=dev)
    pick = torch.empty((n_env, 2), dtype=torch.int64, device=dev)
    args = (C.byref(consts), int(kind), _chk(x_true, "x_true"), _chk(x_cur, "x_cur"), _chk(P_cur, "P_cur"),
            _chk(P_prev, "P_prev") if P_prev is not None else None, _chk(trans, "trans"), _chk(env_time, "env_time", torch.int32),
            int(time_offset), int(trans.shape[0]), _chk(fallback, "fallback", torch.int32) if fallback is not None else None,
            _chk(ws, "workspace", torch.uint8), _chk(action, "action", torch.int32), _chk(pick, "pick", torch.int64), n_obj, n_env)
    if obj_ids is None:
        _lib.check(lib.ssa_agent_select_f64(*args, _stream()), "ssa_agent_select_f64")
    else:
        _lib.check(lib.ssa_agent_select_ids_f64(*args, _chk(obj_ids, "obj_ids", torch.int32), _stream()), "ssa_agent_select_ids_f64")
    return action, pick


def masked_argmax(score, mask=None):
    """index of the first maximum of score[mask != 0] (NaN skipped), -1 if nothing is selected."""
    lib = _lib.load()
    out = torch.empty(2, dtype=torch.int64, device=score.device)
    _lib.check(lib.ssa_masked_argmax_f64(_chk(score, "score"), _chk(mask, "mask", torch.uint8) if mask is not None else None,
                                         score.shape[0], out.data_ptr(), _stream()), "ssa_masked_argmax_f64")
    return int(out[0].item())


def masked_argmax_workspace(n, device):
    """zeroed workspace of ssa_masked_argmax_ws_f64 for up to n entries (one call at a time: keep it with the stream that uses it)"""
    lib = _lib.load()
    return torch.zeros(int(lib.ssa_masked_argmax_workspace_bytes(int(n))) // 8, dtype=torch.int64, device=device)


def masked_argmax_action(score, mask=None, workspace=None):
    """the arg-max head of a device-side policy: np.argmax of `score` over the entries with mask != 0 (first maximum; NaN skipped; -1 when
    nothing is selected) as an int32 CUDA tensor [1] -- the action word the next step launch reads.  ONE launch, nothing leaves the device
    (the kernel writes an int64 pair; its low word IS the int32 action: little endian).  workspace (masked_argmax_workspace): the fold
    spread over the chip instead of one workgroup (3 us instead of 8.6 at 20 000 entries)."""
    lib = _lib.load()
    out = torch.empty(2, dtype=torch.int64, device=score.device)
    m = _chk(mask, "mask", torch.uint8) if mask is not None else None
    if workspace is not None:
        _lib.check(lib.ssa_masked_argmax_ws_f64(_chk(score, "score"), m, score.shape[0], out.data_ptr(), workspace.data_ptr(),
                                                workspace.numel() * 8, _stream()), "ssa_masked_argmax_ws_f64")
    else:
        _lib.check(lib.ssa_masked_argmax_f64(_chk(score, "score"), m, score.shape[0], out.data_ptr(), _stream()), "ssa_masked_argmax_f64")
    return out.view(torch.int32)[:1]


# the assignment rules of a sensor network: rule -> (the one-env entry, its *_envs sibling).  Same arguments, same workspace.
ASSIGN_RULES = {'greedy': ("ssa_assign_sensors_f64", "ssa_assign_sensors_envs_f64"),
                'optimal': ("ssa_match_sensors_f64", "ssa_match_sensors_envs_f64")}


def assign_entry(rule, envs=False):
    """the name of the C entry that assigns by `rule` ('greedy': the global greedy rounds; 'optimal': most sensors tasked, then the
    largest sum of scores -- include/ssa_hip.h: ssa_match_sensors_f64)"""
    if rule not in ASSIGN_RULES:
        raise ValueError("rule must be 'greedy' or 'optimal', not %r" % (rule,))
    return ASSIGN_RULES[rule][bool(envs)]


def assign_sensors_workspace(n_obj, n_sensor, device):
    """zeroed workspace of ssa_assign_sensors_f64 for n_sensor sensors over n_obj objects (one call at a time: keep it with the stream
    that uses it; the kernel leaves it ready for the next call)"""
    nbytes = int(_lib.load().ssa_assign_sensors_workspace_bytes(int(n_obj), int(n_sensor)))
    if nbytes < 0:
        raise _lib.SsaHipError("ssa_assign_sensors_workspace_bytes(%d, %d) failed with code %d" % (n_obj, n_sensor, nbytes))
    return torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=device)


def assign_sensors(score, column, fallback=None, out=None, picks=None, workspace=None, rule='greedy', stream=None):
    """the tasking assignment of a sensor network on the device (ssa_assign_sensors_f64): the global greedy assignment of
    agents._assign_lookahead_sensors over column `column` (_lib.LOOK_*) of score [S, m, 3] -- the rows launch_lookahead_sensors leaves --
    in ONE launch.  fallback: int32 [MAX_SENSORS] draws for the sensors left without an object (taken in ascending s when in range and held
    by nobody; None: they stay idle, -1).  Returns the int32 CUDA row [MAX_SENSORS] (`out`: a 32-byte aligned row to write, e.g. one row
    of launch_rollout_sensors' schedule; entries s >= S are -1); picks: int64 [MAX_SENSORS, 2] to receive the assigned objects and their
    scores' bit patterns.  workspace: assign_sensors_workspace (default: a fresh one).  rule='optimal': the exact optimum instead
    (ssa_match_sensors_f64: most sensors tasked, then the largest sum; finite scores only), same arguments, same workspace.
    stream: as every launcher's here (None: torch's current stream, a torch.cuda.Stream or a raw handle).  No host sync."""
    entry = assign_entry(rule)
    _chk(score, "score")
    if score.dim() != 3 or score.shape[2] != _lib.LOOK_NSCORE:
        raise _lib.SsaHipError("score must be [S, m, %d]" % _lib.LOOK_NSCORE)
    S, m = int(score.shape[0]), int(score.shape[1])
    W = _lib.MAX_SENSORS
    out = torch.empty(W, dtype=torch.int32, device=score.device) if out is None else out
    ws = assign_sensors_workspace(m, S, score.device) if workspace is None else workspace
    _assign_check(W, fallback, out, picks, ws)
    _assign_launch(entry, score, (m, S), column, fallback, out, picks, ws, stream)
    return out


def _assign_check(n, fallback, out, picks, ws):
    """the row arguments of assign_sensors (n = MAX_SENSORS words) and assign_sensors_envs (n = E * MAX_SENSORS)"""
    _chk_n(out, "out", torch.int32, n)
    _chk_n(fallback, "fallback", torch.int32, n)
    _chk_n(picks, "picks", torch.int64, 2 * n)
    _chk(ws, "workspace", torch.int64)


def _assign_launch(entry, score, dims, column, fallback, out, picks, ws, stream=None):
    """the launch half of assign_sensors and assign_sensors_envs, nothing checked: entry(score, *dims, column, fallback, out, picks,
    workspace, stream) with dims = (m, S) or (m, S, E).  The engine's launches, which have checked the same arguments against their
    own state, call it as it is: a second pass over them costs a quarter of the call's host time."""
    _lib.check(getattr(_lib.load(), entry)(score.data_ptr(), *dims, int(column), None if fallback is None else fallback.data_ptr(), out.data_ptr(),
                                           None if picks is None else picks.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream(stream)), entry)


def assign_sensors_envs_workspace(n_obj, n_sensor, n_env, device):
    """zeroed workspace of ssa_assign_sensors_envs_f64 for n_env envs of n_sensor sensors over n_obj objects each (one call at a time:
    keep it with the stream that uses it; the kernel leaves it ready for the next call)"""
    nbytes = int(_lib.load().ssa_assign_sensors_envs_workspace_bytes(int(n_obj), int(n_sensor), int(n_env)))
    if nbytes < 0:
        raise _lib.SsaHipError("ssa_assign_sensors_envs_workspace_bytes(%d, %d, %d) failed with code %d" % (n_obj, n_sensor, n_env, nbytes))
    return torch.zeros(nbytes // 8, dtype=torch.int64, device=device)


def assign_sensors_envs(score, column, fallback=None, out=None, picks=None, workspace=None, rule='greedy', stream=None):
    """the tasking assignment of a sensor network in each of E envs (ssa_assign_sensors_envs_f64): assign_sensors for every env's slab of
    score [E, S, m, 3] -- the rows launch_lookahead_sensors_envs leaves -- in ONE launch.  fallback: int32 [E, MAX_SENSORS] draws per env
    (None: a sensor left without an object stays idle, -1).  Returns the int32 CUDA table [E, MAX_SENSORS] (`out`: a 32-byte aligned
    table to write, e.g. the action table the next launch_step_sensors_envs reads; entries s >= S are -1); picks: int64
    [E, MAX_SENSORS, 2] to receive the assigned objects and their scores' bit patterns.  workspace: assign_sensors_envs_workspace
    (default: a fresh one).  rule: as assign_sensors ('optimal': ssa_match_sensors_envs_f64).  No host sync."""
    entry = assign_entry(rule, envs=True)
    _chk(score, "score")
    if score.dim() != 4 or score.shape[3] != _lib.LOOK_NSCORE:
        raise _lib.SsaHipError("score must be [E, S, m, %d]" % _lib.LOOK_NSCORE)
    E, S, m = (int(v) for v in score.shape[:3])
    W = _lib.MAX_SENSORS
    out = torch.empty((E, W), dtype=torch.int32, device=score.device) if out is None else out
    ws = assign_sensors_envs_workspace(m, S, E, score.device) if workspace is None else workspace
    _assign_check(E * W, fallback, out, picks, ws)
    _assign_launch(entry, score, (m, S, E), column, fallback, out, picks, ws, stream)
    return out


def check_plan_slots(n_step, n_sensor):
    """a plan has at most MAX_PLAN_SLOTS (step, sensor) slots: a ValueError that names the cap, before any launch"""
    if int(n_step) * int(n_sensor) > _lib.MAX_PLAN_SLOTS:
        raise ValueError("a horizon-wide plan has at most %d (step, sensor) slots (SSA_MAX_PLAN_SLOTS), got %d steps x %d sensors = %d"
                         % (_lib.MAX_PLAN_SLOTS, n_step, n_sensor, int(n_step) * int(n_sensor)))


def plan_sensors_workspace(n_obj, n_sensor, n_step, n_env, device):
    """zeroed workspace of ssa_plan_sensors_f64 for n_env envs of n_step x n_sensor slots over n_obj objects each (one call at a time:
    keep it with the stream that uses it; the kernel leaves it ready for the next call)"""
    check_plan_slots(n_step, n_sensor)
    nbytes = int(_lib.load().ssa_plan_sensors_workspace_bytes(int(n_obj), int(n_sensor), int(n_step), int(n_env)))
    if nbytes < 0:
        raise _lib.SsaHipError("ssa_plan_sensors_workspace_bytes(%d, %d, %d, %d) failed with code %d" % (n_obj, n_sensor, n_step, n_env, nbytes))
    return torch.zeros(nbytes // 8, dtype=torch.int64, device=device)


def plan_sensors(score, column, out=None, picks=None, workspace=None, stream=None):
    """the horizon-wide optimal tasking plan of a sensor network on the device (ssa_plan_sensors_f64): ONE assignment problem over all
    H' * S (step, sensor) slots of column `column` (_lib.LOOK_*) of a forecast's scores -- [H', S, m, 3] (one env: what
    launch_forecast_sensors leaves) or [H', E, S, m, 3] (what launch_forecast_sensors_envs leaves) -- in ONE launch: the most slots
    filled, then the largest sum of scores, no object twice in an env's plan; finite scores of magnitude <= 2^1020 only.  Returns the
    int32 CUDA table [H', MAX_SENSORS] or [H', E, MAX_SENSORS] (`out`: a 32-byte aligned table to write; -1 beyond S and in unfilled
    slots): the schedule launch_rollout_sensors / launch_rollout_sensors_envs takes.  picks: int64 [H', (E,) MAX_SENSORS, 2] to receive
    the objects and their scores' bit patterns.  workspace: plan_sensors_workspace (default: a fresh one).  H' * S > MAX_PLAN_SLOTS is a
    ValueError.  No host sync."""
    if not (isinstance(score, torch.Tensor) and score.is_cuda and score.dtype == f64 and score.is_contiguous() and score.dim() in (4, 5)
            and score.shape[-1] == _lib.LOOK_NSCORE):
        raise _lib.SsaHipError("score must be a contiguous CUDA float64 tensor [H', S, m, %d] or [H', E, S, m, %d]" % ((_lib.LOOK_NSCORE,) * 2))
    Hp, S, m = int(score.shape[0]), int(score.shape[-3]), int(score.shape[-2])
    E = int(score.shape[1]) if score.dim() == 5 else 1
    check_plan_slots(Hp, S)
    lib = _lib.load()
    W = _lib.MAX_SENSORS
    out = torch.empty(tuple(score.shape[:-3]) + (W,), dtype=torch.int32, device=score.device) if out is None else out
    ws = plan_sensors_workspace(m, S, Hp, E, score.device) if workspace is None else workspace
    _lib.check(lib.ssa_plan_sensors_f64(score.data_ptr(), m, S, Hp, E, int(column), _chk_n(out, "out", torch.int32, Hp * E * W),
                                        _chk_n(picks, "picks", torch.int64, 2 * Hp * E * W), _chk(ws, "workspace", torch.int64),
                                        ws.numel() * 8, _stream(stream)), "ssa_plan_sensors_f64")
    return out


def dryrun_rows(actions, n_obj, n_sensor=None):
    """the host side of a gathered dry run (engine.launch_dryrun_sensors): for candidates `actions` [B, K, S] over a catalogue of n_obj
    objects, (ids [B, W] int32, words [K, B, MAX_SENSORS] int32).  ids[b] = the distinct valid objects (0 <= a < n_obj) candidate b names,
    ascending, padded with -1 to W = 4 * ceil(max_b distinct / 4) (at least one tile: an all-idle batch still has its first row, which
    clears the records); words = the action rows as ssa_dryrun_sensors_params.actions takes them, -1 beyond S."""
    import numpy as np
    a = np.asarray(actions)
    if a.ndim != 3 or a.shape[1] < 1 or a.shape[0] < 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("dry run: actions must be an integer array [B, K, S], got %s %s" % (a.dtype, a.shape))
    B, K, S = a.shape
    if not 1 <= S <= _lib.MAX_SENSORS or (n_sensor is not None and S != int(n_sensor)):
        raise ValueError("dry run: actions [B, K, S] must have S = %s sensors, got %d" % (n_sensor or "1 .. %d" % _lib.MAX_SENSORS, S))
    a = a.astype(np.int64)
    # per candidate: its entries sorted with the idle ones last, the first of every run of equal objects kept (no loop over B)
    idle = np.iinfo(np.int64).max
    v = np.sort(np.where((a >= 0) & (a < int(n_obj)), a, idle).reshape(B, K * S), axis=1)
    keep = v < idle
    keep[:, 1:] &= v[:, 1:] != v[:, :-1]
    W = 4 * max(1, -(-int(keep.sum(axis=1).max()) // 4))
    ids = np.full((B, W), -1, dtype=np.int32)
    ids[np.nonzero(keep)[0], (np.cumsum(keep, axis=1) - 1)[keep]] = v[keep]
    words = np.full((K, B, _lib.MAX_SENSORS), -1, dtype=np.int32)
    words[:, :, :S] = np.clip(a, -1, np.iinfo(np.int32).max).transpose(1, 0, 2)
    return ids, words


def dryrun_sensors(consts, params, sensors, actions, n_steps, n_obj_caller, out=None, stream=None):
    """the dry run of candidate schedules on the device (ssa_dryrun_sensors_envs_f64), stateless: `params` a filled _lib.ssa_step_params
    (its INPUT fields: n_env pseudo-envs of n_obj rows each, obj_ids per env), `sensors` host.make_sensor_params(), `actions` a contiguous
    32-byte aligned CUDA int32 tensor [K, n_env, MAX_SENSORS].  Returns the records [K, n_env, S, DRY_STRIDE] (CUDA float64; `out`: the
    tensor to write).  Nothing else is written.  No host sync."""
    K, E, S = int(n_steps), int(params.n_env), int(sensors.n_sensor)
    if not (isinstance(actions, torch.Tensor) and actions.is_cuda and actions.dtype == torch.int32 and actions.is_contiguous()
            and tuple(actions.shape) == (K, E, _lib.MAX_SENSORS)):
        raise _lib.SsaHipError("dry run: actions must be a contiguous CUDA int32 tensor [%d, %d, %d]" % (K, E, _lib.MAX_SENSORS))
    if out is None:
        out = torch.empty((K, E, S, _lib.DRY_STRIDE), dtype=f64, device=actions.device)
    elif _chk(out, "out") and out.numel() != K * E * S * _lib.DRY_STRIDE:
        raise _lib.SsaHipError("out must hold %d doubles" % (K * E * S * _lib.DRY_STRIDE))
    d = _lib.ssa_dryrun_sensors_params()
    d.n_steps, d.n_obj_caller, d.actions, d.out = K, int(n_obj_caller), actions.data_ptr(), out.data_ptr()
    _lib.check(_lib.load().ssa_dryrun_sensors_envs_f64(C.byref(consts), C.byref(params), C.byref(sensors), C.byref(d), _stream(stream)),
               "ssa_dryrun_sensors_envs_f64")
    return out


def access_words(n_steps):
    """W: the 64-bit words per row of a pass table over n_steps steps"""
    return (int(n_steps) + 63) // 64


def access_sensors(consts, params, sensors, n_steps, bits=None, summary=None, n_left=None, env_sel=None, stream=None):
    """the pass table of a sensor network on the device (ssa_access_sensors_f64), stateless: `params` a filled _lib.ssa_step_params (its
    INPUT fields: x_true_in, trans, env_time, time_offset, n_time, n_obj, n_env, obj_ids and the moving sensors' tail), `sensors`
    host.make_sensor_params().  bits: a contiguous CUDA int64 tensor of n_env * S * n_obj * W words to write (None: a new [n_env, S,
    n_obj, W] one), W = access_words(n_steps); summary: a contiguous CUDA int32 tensor of n_env * S * n_obj * 4 words for (first, length,
    count, passes), True for a new one, None / False for none; n_left: CUDA int32 [n_env] or None; env_sel: CUDA int32 words, the envs to
    compute (every other env's slab of bits / summary is left as it is), or None for all.  Returns (bits, summary).  Nothing else is
    written; no host sync."""
    T, E, S, m = int(n_steps), int(params.n_env), int(sensors.n_sensor), int(params.n_obj)
    W = access_words(T)
    dev = torch.device("cuda")
    if bits is None:
        bits = torch.empty((E, S, m, W), dtype=torch.int64, device=dev)
    if summary is True:
        summary = torch.empty((E, S, m, 4), dtype=torch.int32, device=dev)
    elif summary is False:
        summary = None
    a = _lib.ssa_access_params()
    a.n_steps = T
    a.bits = _chk_n(bits, "bits", torch.int64, E * S * m * W)
    a.pass_ = _chk_n(summary, "summary", torch.int32, E * S * m * 4) or 0
    a.n_left = _chk_n(n_left, "n_left", torch.int32, E) or 0
    if env_sel is not None:
        a.env_sel, a.n_sel = _chk(env_sel, "env_sel", torch.int32), int(env_sel.numel())
    _lib.check(_lib.load().ssa_access_sensors_f64(C.byref(consts), C.byref(params), C.byref(sensors), C.byref(a), _stream(stream)),
               "ssa_access_sensors_f64")
    return bits, summary


def access_mask(bits, k):
    """the bool mask [..., S, m] of step k of a pass table `bits` [..., S, m, W] (int64 words, bit h mod 64 of word h div 64 = step h):
    one shift-and-mask, no kernel of the library.  k: one step for the whole table, or one per entry of its LEADING axis (the envs of a
    vector table [E, S, m, W], each at its own step: the words are gathered first)"""
    import numpy as np
    ks = np.asarray(k, dtype=np.int64)
    if ks.size == 0 or ks.min() < 0 or ks.max() >= 64 * bits.shape[-1]:
        raise _lib.SsaHipError("access_mask: step %r outside the table's %d words" % (k, bits.shape[-1]))
    if ks.ndim == 0:
        return ((bits[..., int(ks) >> 6] >> (int(ks) & 63)) & 1).to(torch.bool)
    if ks.shape != (bits.shape[0],) or bits.dim() < 2:
        raise _lib.SsaHipError("access_mask: one step per entry of the table's leading axis (%d), got %r" % (bits.shape[0], ks.shape))
    lead = (-1,) + (1,) * (bits.dim() - 1)
    at = torch.as_tensor(ks, device=bits.device)
    words = bits.gather(-1, (at >> 6).view(lead).expand(bits.shape[:-1] + (1,))).squeeze(-1)
    return ((words >> (at & 63).view(lead[:-1])) & 1).to(torch.bool)


def access_unpack(bits, n_steps):
    """a pass table `bits` [..., S, m, W] as the bool array [..., S, m, n_steps] (for small cases: one byte per cell)"""
    T = int(n_steps)
    if T < 0 or T > 64 * bits.shape[-1]:
        raise _lib.SsaHipError("access_unpack: %d steps in %d words" % (T, bits.shape[-1]))
    sh = torch.arange(64, dtype=torch.int64, device=bits.device)
    cells = (bits.unsqueeze(-1) >> sh) & 1      # [..., W, 64]; an arithmetic shift: bit 63 comes out as -1 & 1 = 1
    return cells.reshape(bits.shape[:-1] + (64 * bits.shape[-1],))[..., :T].to(torch.bool)


def dryrun_totals(records, out=None):
    """the totals of a dry run's records [K, E, S, DRY_STRIDE] (contiguous CUDA float64, as dryrun_sensors leaves them) on the device
    (ssa_dryrun_totals_f64): [E, LOOK_NSCORE], per candidate and score column the sum of the taken slots' scores in slot order (k outer,
    s inner) -- one defined fp64 sum; 0 for none.  No host sync."""
    _chk(records, "records")
    if records.dim() != 4 or records.shape[3] != _lib.DRY_STRIDE:
        raise _lib.SsaHipError("records must be [K, E, S, %d]" % _lib.DRY_STRIDE)
    K, E, S = (int(v) for v in records.shape[:3])
    if out is None:
        out = torch.empty((E, _lib.LOOK_NSCORE), dtype=f64, device=records.device)
    elif _chk(out, "out") and out.numel() != E * _lib.LOOK_NSCORE:
        raise _lib.SsaHipError("out must hold %d doubles" % (E * _lib.LOOK_NSCORE))
    _lib.check(_lib.load().ssa_dryrun_totals_f64(records.data_ptr(), E, K, S, out.data_ptr(), _stream()), "ssa_dryrun_totals_f64")
    return out


def dryrun_gather_rows(ids, n_env, n_cand, n_obj, slot_of=None):
    """the rule of ssa_dryrun_gather_f64 in numpy: for `ids` (integers, E * B * W of them: per env and candidate the W object indices
    dryrun_rows leaves, -1 = padding) the source row of every output row, int64 [E * B * W].  Row (e, b, w): j = ids[e, b, w]; an id
    < 0 or >= n_obj is replaced by the candidate's first id, taken as 0 when negative and as n_obj - 1 beyond the end (a padding row
    carries the state of the candidate's first object; object 0 in an all-idle candidate); the row is e * n_obj + j, and with
    `slot_of` (the storage row of every caller's global row, [E * n_obj]) slot_of[e * n_obj + j].  Needs no device."""
    import numpy as np
    E, B, m = int(n_env), int(n_cand), int(n_obj)
    a = np.asarray(ids)
    if E < 1 or B < 1 or m < 1 or a.size < E * B or a.size % (E * B) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("dry-run gather: integer ids [%d * %d, W] with W >= 1 and n_obj >= 1, got %s of %d" % (E, B, a.dtype, a.size))
    j = a.astype(np.int64).reshape(E, B, -1)
    first = np.clip(j[:, :, :1], 0, m - 1)
    rows = np.where((j >= 0) & (j < m), j, first) + (np.arange(E, dtype=np.int64) * m)[:, None, None]
    if slot_of is not None:
        t = np.asarray(slot_of).astype(np.int64).reshape(-1)
        if t.size != E * m:
            raise ValueError("dry-run gather: slot_of must hold %d rows, got %d" % (E * m, t.size))
        rows = np.clip(t[rows], 0, E * m - 1)
    return rows.reshape(-1)


def dryrun_gather(ids, env_time, x_true, x_filter, P_filter, status, n_env, n_cand, n_obj, slot_of=None, out=None, stream=None):
    """the gathered block of a vector dry run on the device (ssa_dryrun_gather_f64; the rule: dryrun_gather_rows), stateless: `ids`
    contiguous CUDA int32 [E * B, W] (W % 4 == 0), `env_time` int32 [E], the source block x_true / x_filter [E * n_obj, 6], P_filter
    [E * n_obj, 6, 6] float64 and status int32 [E * n_obj], slot_of int32 [E * n_obj] or None.  Returns (x_true, x_filter, P_filter,
    status, time) of the E * B pseudo-envs of W rows -- [E * B * W, 6], [.., 6], [.., 6, 6] float64, [E * B * W] and [E * B] int32; `out`:
    the five tensors to write, none of them a part of the inputs.  One launch, no host sync."""
    E, B, m = int(n_env), int(n_cand), int(n_obj)
    i32 = torch.int32
    _chk(ids, "ids", i32)
    if ids.dim() != 2 or ids.shape[0] != E * B:
        raise _lib.SsaHipError("ids must be [%d, W]" % (E * B))
    W = int(ids.shape[1])
    R = E * B * W
    g = _lib.ssa_dryrun_gather_params()
    g.n_obj, g.n_env, g.n_cand, g.n_rows, g.reserved = m, E, B, W, 0
    g.ids, g.env_time = ids.data_ptr(), _chk(env_time, "env_time", i32)
    g.slot_of = _chk(slot_of, "slot_of", i32) if slot_of is not None else 0
    g.x_true_in, g.x_in, g.P_in, g.status_in = _chk(x_true, "x_true"), _chk(x_filter, "x_filter"), _chk(P_filter, "P_filter"), _chk(status, "status", i32)
    for t, n, nm in ((env_time, E, "env_time"), (x_true, 6 * E * m, "x_true"), (x_filter, 6 * E * m, "x_filter"), (P_filter, 36 * E * m, "P_filter"),
                     (status, E * m, "status")) + (((slot_of, E * m, "slot_of"),) if slot_of is not None else ()):
        if t.numel() != n:
            raise _lib.SsaHipError("%s must hold %d elements, got %d" % (nm, n, t.numel()))
    if out is None:
        dev = ids.device
        out = (torch.empty((R, 6), dtype=f64, device=dev), torch.empty((R, 6), dtype=f64, device=dev), torch.empty((R, 6, 6), dtype=f64, device=dev),
               torch.empty(R, dtype=i32, device=dev), torch.empty(E * B, dtype=i32, device=dev))
    for t, n, dt, nm in zip(out, (6 * R, 6 * R, 36 * R, R, E * B), (f64, f64, f64, i32, i32), ("x_true", "x_filter", "P_filter", "status", "time")):
        if _chk(t, "out: " + nm, dt) and t.numel() != n:
            raise _lib.SsaHipError("out: %s must hold %d elements, got %d" % (nm, n, t.numel()))
    g.x_true_out, g.x_out, g.P_out, g.status_out, g.time_out = (t.data_ptr() for t in out)
    _lib.check(_lib.load().ssa_dryrun_gather_f64(C.byref(g), _stream(stream)), "ssa_dryrun_gather_f64")
    return tuple(out)


def env_step(consts, params):
    """E1: the fused step.  `params` is a filled _lib.ssa_step_params."""
    lib = _lib.load()
    _lib.check(lib.ssa_env_step_f64(C.byref(consts), C.byref(params), _stream()), "ssa_env_step_f64")


def nees(x_true, x, P):
    """d^T inv(P) d for every row (anees() / fitness_test() of the reference)."""
    lib = _lib.load()
    n = x.shape[0]
    out = torch.empty(n, dtype=f64, device=x.device)
    _lib.check(lib.ssa_nees_f64(_chk(x_true, "x_true"), _chk(x, "x"), _chk(P, "P"), _chk(out, "nees"), n, _stream()), "ssa_nees_f64")
    return out


def nis(y, S):
    """y^T inv(S) y for every row (fitness_test() of the reference)."""
    lib = _lib.load()
    n = y.shape[0]
    out = torch.empty(n, dtype=f64, device=y.device)
    _lib.check(lib.ssa_nis_f64(_chk(y, "y"), _chk(S, "S"), _chk(out, "nis"), n, _stream()), "ssa_nis_f64")
    return out


def chi2_contained(values, lo, hi):
    """(inside, valid) = number of entries strictly inside (lo, hi) and number of non-NaN entries of a float64 device tensor
    (fitness_test()'s chi-square containment, ssa_tasker_simple_2.py:757-760, 770-771)."""
    lib = _lib.load()
    v = values.reshape(-1)
    out = torch.empty(2, dtype=torch.int64, device=v.device)
    _lib.check(lib.ssa_chi2_contained_f64(_chk(v, "values"), v.numel(), float(lo), float(hi), out.data_ptr(), _stream()),
               "ssa_chi2_contained_f64")
    c = out.cpu()
    return int(c[0]), int(c[1])
