"""Making the UKF update fail inside a step, and comparing a poisoned launch with its clean twin as 64-bit patterns.

Two recipes, both pinned to the fp64 oracle by tests/test_update_failures_host.py:

  SSA_ST_UPDATE_NAN     one component of the updated object's measurement noise is NaN: S and K stay finite, the innovation y and with it
                        x + K y are NaN.  The reference books the update (obs_taken, y, S, sigmas_h; ssa_tasker_simple_2.py:300-305) and then
                        calls filter_error (:306-311).
  SSA_ST_UPDATE_LINALG  R = diag(1e103): the cofactor determinant of S is ~1e309, infinite in fp64, and both oracle.inv3 and the device
                        inv3 refuse a non-finite determinant.  Nothing is booked (:312-315).
                        (np.eye(3) * np.inf is NOT this recipe: its off-diagonal entries are 0 * inf = NaN.  In 80-bit arithmetic 1e309 is
                        finite, so the long-double oracle does not flag this R: for the failing object the fp64 oracle is the authority and
                        the 80-bit witness is not used.)
"""
import ctypes as C

import numpy as np

import oracle as orc
from support.batches import c2t, make_batch

ALPHA = 1e-4
NOISE_SD = np.array([4.8e-6, 4.8e-6, 1e3])
R_OVERFLOW = np.diag([1e103, 1e103, 1e103])
STAT_COLS = ("STAT_MAX_DPOS", "STAT_CNT_LT_1E4", "STAT_CNT_LT_1E7", "STAT_N_FAILED")      # what every launch form computes
STAT_COLS_ARGMAX = STAT_COLS + ("STAT_ARGMAX_SPOS", "STAT_MAX_SPOS")                    # ... and the forms that carry np.argmax(sigma_pos)


# the components of the innovation y that are NaN when component `comp` of the noise is: the poisoned one alone, for 'xyz' (y = z - zp) and
# for 'aer' alike (the oracle's residual_z_aer wraps each angle on its own and subtracts the range).  Recorded from the fp64 oracle and
# asserted by tests/test_update_failures_host.py; the GPU tests read it.
Y_NAN = {(ot, comp): (comp,) for ot in ('aer', 'xyz') for comp in range(3)}

# the batch the recipes are pinned on: make_batch(HOST_M, seed=HOST_SEED), action HOST_ACTION at time index HOST_TIX, no elevation mask
HOST_M, HOST_SEED, HOST_ACTION, HOST_TIX = 12, 8, 5, 1


def nan_noise(z_noise, e, i, a, comp):
    """a copy of the noise table z_noise[E][n_time][m][3] whose component `comp` of env e, time index i, object a is NaN"""
    z = np.array(z_noise, dtype=np.float64, copy=True)
    z[e, i, a, comp] = np.nan
    return z


def noise_table(E, n_time, m, seed=99):
    return np.random.RandomState(seed).normal(size=(E, n_time, m, 3)) * NOISE_SD


def golden_R(g, obs_type):
    return g["R"] if obs_type == 'aer' else g["xyz_R"]


def b64(a):
    """a float64 array as its 64-bit patterns (NaN payloads and signed zeros compare as bits); anything else as it is"""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return np.array_equal(b64(a), b64(b))


def twin(hip, launch, z_noise, R, poison):
    """the same launch twice from one state: launch(z_noise, R) clean -- finite noise, the golden R -- and launch(*poison(z_noise, R)).
    `launch` builds its engine itself, so the two runs share nothing on the device.  Returns (clean, poisoned)."""
    assert np.isfinite(z_noise).all() and np.isfinite(R).all() and np.abs(R).max() < 1e12
    clean = launch(z_noise, R)
    zp, Rp = poison(np.array(z_noise, copy=True), np.array(R, copy=True))
    assert not (same_bits(zp, z_noise) and same_bits(Rp, R)), "poison() changed nothing"
    return clean, launch(zp, Rp)


def error_failed(xt, x, P):
    """error_failed() of ssa_tasker_simple_2.py:376-378 on one object's slot: delta_pos, delta_vel, sigma_pos, sigma_vel"""
    d = np.asarray(x) - np.asarray(xt)
    v = np.diag(np.asarray(P))
    return np.array([np.sqrt(np.sum(d[:3] ** 2)), np.sqrt(np.sum(d[3:] ** 2)), np.sqrt(np.sum(v[:3])), np.sqrt(np.sum(v[3:]))])


def oracle_step(o, xt, x, P, g, action, tix, obs_type, resample, R, z_noise3, obs_limit=-np.pi / 2, status=None, centred=False):
    """one reference step of the oracle `o`; returns its dict with the status vector under "status" """
    Wm, Wc, scale = orc.merwe_weights(ALPHA, 2.0, -3)
    st = np.zeros(x.shape[0], dtype=np.int32) if status is None else status.copy()
    r = o.env_step(xt, x, P, st, 20.0, g["Q"], R, Wm, Wc, scale, action, c2t()[tix], g["obs_lla"], g["obs_itrs"], obs_limit, z_noise3,
                   obs_type=0 if obs_type == 'aer' else 1, centred=centred, resample=resample)
    r["status"] = st
    return r


# ---------------------------------------------------------------- engines and what a launch leaves

def engine(hip, xt, x, P, g, z_noise, R, obs_type='aer', propagator='fg', resample=False, obs_limit=-np.pi / 2, E=1, history=2,
           layout=None, generic=False):
    """a HotPathEngine over the batch (E envs of m = len(x) / E objects), state in slot 0"""
    m = x.shape[0] // E
    consts = hip.host.make_consts(g["Q"], R, ALPHA, 2.0, -3, 20.0, obs_limit, g["obs_lla"], obs_type=obs_type, propagator=propagator,
                                  resample=resample)
    eng = hip.engine.HotPathEngine(consts, m, E, c2t()[:z_noise.shape[1]], z_noise, history=history)
    eng.force_generic = generic
    if layout is not None:
        eng.set_layout(layout)
    eng.load_state(0, xt, x, P)
    return eng


def read_slot(eng, s, caller_order=True):
    """history slot s and the status words as numpy arrays, rows as the caller numbers the objects (a storage layout does not show)"""
    rows = (lambda t: eng.caller_rows(t)) if (caller_order and eng.E == 1) else (lambda t: t)
    met = eng.metrics[s]                                            # [E][4][m]
    if caller_order and eng.E == 1 and eng._order is not None:
        met = met.index_select(2, eng._slot_of)
    return dict(x_true=rows(eng.x_true[s]).cpu().numpy(), x=rows(eng.x_filter[s]).cpu().numpy(), P=rows(eng.P_filter[s]).cpu().numpy(),
                obs=rows(eng.obs[s]).cpu().numpy(), metrics=met.cpu().numpy(), status=rows(eng.status).cpu().numpy(),
                upd=eng.upd[s].cpu().numpy())


def fail_log(hip, eng):
    """the failure records written so far, sorted by (step, env, object) -- they land in the order the failing wavefronts reach the counter"""
    L = hip.lib
    hip.torch.cuda.synchronize()
    nf = int(eng.fail_count.cpu().numpy()[0])
    recs = sorted(map(tuple, eng.fail_log[:nf]), key=lambda r: (r[L.FAIL_TIME], r[L.FAIL_ENV], r[L.FAIL_OBJ]))
    return np.array(recs, dtype=np.float64).reshape(nf, L.FAIL_STRIDE)


def instances(hip, eng):
    """ssa_env_step_instance() of every parameter block the engine has launched: 0 the generic step kernel, 1 the plain instance"""
    lib = hip.lib.load()
    return {int(lib.ssa_env_step_instance(eng._cref, C.byref(ent[0]))) for ent in eng._pcache.values()}


def assert_records_equal(L, want, got, what):
    """update records [..., UPD_STRIDE]: the words the step defines (support.sensors._defined_fields: the flags always, z_true once the
    update was attempted, y / S / sigmas_h once it was taken), bit-identical.  The reference leaves y, S and sigmas_h unwritten on a
    LinAlgError (ssa_tasker_simple_2.py:312) and for a hidden object, and so does the kernel: those words hold whatever the record's memory
    held before, which differs between a ring of two slots and a slot per step -- they are not compared."""
    from support.sensors import _defined_fields
    want, got = np.asarray(want).reshape(-1, L.UPD_STRIDE), np.asarray(got).reshape(-1, L.UPD_STRIDE)
    assert want.shape == got.shape, what
    a, b = _defined_fields(L, want), _defined_fields(L, got)
    for k in range(a.shape[0]):
        assert same_bits(a[k], b[k]), (what, "record", k, a[k][[L.UPD_OBS_TAKEN, L.UPD_VISIBLE, L.UPD_ACTION]], b[k][[L.UPD_OBS_TAKEN, L.UPD_VISIBLE, L.UPD_ACTION]])


# ---------------------------------------------------------------- a schedule of steps through every form of the step

N_STEPS = 6
N_TIME = N_STEPS + 1
SCHED_LIMIT = np.radians(20.0)


def schedule_batch(m):
    """the batch of the schedule runs (m = 7 or 12) and its six actions: a healthy visible object, an object whose noise is NaN at that
    step, the same object again, a hidden object, the last object (NaN noise again), object 0.  Elevations of this batch over the six
    steps (oracle.hx_aer of the propagated truth, degrees): m = 7: [10..17, 35, 39, -55, 45, -30, 21]; m = 12: [30, 87, -61, -30, 34, -34,
    -56, 45, 69, 84, -74, 44] -- against the 20 degree mask object 0 is hidden at m = 7 and visible at m = 12."""
    xt, x, P, g = make_batch(m, seed=1200 + m)
    sched = {7: [1, 2, 2, 3, 6, 0], 12: [1, 4, 4, 2, 11, 0]}[m]
    return xt, x, P, g, sched


def poison_schedule_nan(sched, e=0):
    """NaN noise at steps 2 and 5 of the schedule (time indices = step numbers), on the objects scheduled there"""
    def poison(z, R):
        z = nan_noise(z, e, 2, sched[1], 1)
        return nan_noise(z, e, 5, sched[4], 2), R
    return poison


def poison_overflow(z, R):
    return z, R_OVERFLOW.copy()


def run_schedule(hip, m, z_noise, R, form="generic", argmax=False, layout=None, propagator='hybrid'):
    """the six steps of schedule_batch(m) through one form of the one-env step, a history slot per step.  Returns what
    assert_same_schedule compares: per step the slot it wrote (rows in the caller's order) and its statistics row, the sorted failure
    log, and the instances the launches took.
      generic      step + post + final, the action a word in memory (the form of run A)
      fold_kernel  fast_stats, the fold kernel behind every step
      deferred     fast_stats + defer_fold with the action by value: folded by the next launch, the last by flush_stats()
      inside       fast_stats + fold_inside
      rollout      launch_rollout, the six actions in one launch
    (the plain instance runs through support.plain_step.run: see from_plain_step)"""
    torch = hip.torch
    xt, x, P, g, sched = schedule_batch(m)
    eng = engine(hip, xt, x, P, g, z_noise, R, propagator=propagator, obs_limit=SCHED_LIMIT, history=N_STEPS + 2, layout=layout)
    staged = torch.as_tensor(np.asarray(sched, dtype=np.int32)).cuda()
    if form == "rollout":
        eng.launch_rollout(0, 1, staged.view(N_STEPS, 1).contiguous(), argmax_spos=argmax)
    else:
        for k, a in enumerate(sched):
            if form == "generic":
                eng.set_actions([a])
                eng.launch_step(k, k + 1, k + 1)
                torch.cuda.synchronize()      # (the action word is rewritten for the next step)
            elif form == "fold_kernel":
                eng.launch_step(k, k + 1, k + 1, action=a, fast_stats=True, argmax_spos=argmax)
            elif form == "deferred":
                eng.launch_step(k, k + 1, k + 1, action=a, fast_stats=True, defer_fold=True, argmax_spos=argmax)
            elif form == "inside":
                eng.launch_step(k, k + 1, k + 1, action=a, fast_stats=True, fold_inside=True, argmax_spos=argmax)
            else:
                raise ValueError(form)
        eng.flush_stats()
    torch.cuda.synchronize()
    steps = []
    for k in range(1, N_STEPS + 1):
        s = read_slot(eng, k)
        del s["status"]                    # (one status vector per engine: the final one, below)
        s["stats"] = eng.stats[k].cpu().numpy()
        steps.append(s)
    return dict(steps=steps, status=read_slot(eng, N_STEPS)["status"], fail_log=fail_log(hip, eng), instances=instances(hip, eng), sched=sched)


def run_schedule_envs(hip, m, E, z_noise, R, inline, propagator='hybrid'):
    """the schedule in each of E envs that start from the same state (z_noise [E][N_TIME][m][3]), one launch per step: the actions
    device words (inline=False) or by value in the parameter block (SSA_LAUNCH_INLINE_ENVS).  Returns one run_schedule-shaped dict per
    env -- env e's rows of every slot, its record, its statistics row, its failure records (FAIL_ENV = e) -- so that each compares with
    the one-env run of that env's noise table."""
    torch, L = hip.torch, hip.lib
    xt, x, P, g, sched = schedule_batch(m)
    eng = engine(hip, np.tile(xt, (E, 1)), np.tile(x, (E, 1)), np.tile(P, (E, 1, 1)), g, z_noise, R, propagator=propagator,
                 obs_limit=SCHED_LIMIT, E=E, history=N_STEPS + 2)
    for k, a in enumerate(sched):
        if inline:
            eng.launch_step(k, k + 1, k + 1, env_words=([0] * E, [a] * E))
        else:
            eng.set_actions([a] * E)
            eng.launch_step(k, k + 1, k + 1)
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    log = fail_log(hip, eng)
    slots = [read_slot(eng, k) for k in range(1, N_STEPS + 1)]
    stats = [eng.stats[k].cpu().numpy() for k in range(1, N_STEPS + 1)]
    out = []
    for e in range(E):
        sl = slice(e * m, (e + 1) * m)
        steps = [dict(x_true=s["x_true"][sl], x=s["x"][sl], P=s["P"][sl], obs=s["obs"][sl], metrics=s["metrics"][e:e + 1], upd=s["upd"][e:e + 1],
                      stats=st[e:e + 1]) for s, st in zip(slots, stats)]
        out.append(dict(steps=steps, status=slots[-1]["status"][sl], fail_log=log[log[:, L.FAIL_ENV] == e], instances=instances(hip, eng),
                        sched=sched))
    return out


def from_plain_step(hip, res):
    """what support.plain_step.run returns (bit patterns on the device, a ring of two slots, no layout) in run_schedule's form"""
    f64 = hip.torch.float64
    val = lambda t: t.view(f64).cpu().numpy() if t.dtype == hip.torch.int64 else t.cpu().numpy()      # noqa: E731
    steps = []
    for t, s in res["steps"]:
        steps.append(dict(x_true=val(s["xt"]), x=val(s["x"]), P=val(s["P"]), obs=val(s["obs"]), metrics=val(s["metrics"]), upd=val(s["upd"]),
                          stats=val(res["rows"][t])))
    log = res["fail_log"].reshape(-1, hip.lib.FAIL_STRIDE)
    return dict(steps=steps, status=val(res["steps"][-1][1]["status"]), fail_log=log, instances=res["instances"])


def assert_same_schedule(L, want, got, what, stat_cols=STAT_COLS):
    """every slot (x_true, x, P, obs, metrics, upd), the statistics columns `stat_cols` of every step, the status words and the sorted
    failure log: bit-identical"""
    for k, (a, b) in enumerate(zip(want["steps"], got["steps"])):
        for key in ("x_true", "x", "P", "obs", "metrics"):
            assert same_bits(a[key], b[key]), (what, "step", k + 1, key)
        assert_records_equal(L, a["upd"], b["upd"], (what, "step", k + 1))
        cols = [getattr(L, c) for c in stat_cols]
        assert same_bits(a["stats"][:, cols], b["stats"][:, cols]), (what, "statistics of step", k + 1, a["stats"], b["stats"])
    assert np.array_equal(want["status"], got["status"]), what
    assert want["fail_log"].shape == got["fail_log"].shape and same_bits(want["fail_log"], got["fail_log"]), (what, want["fail_log"], got["fail_log"])


# ---------------------------------------------------------------- sensor networks: one step of S sensors

SENSOR_M, SENSOR_S, SENSOR_TIME = 12, 3, 4


def sensor_inputs():
    """the batch of the sensor cases, the golden R for each of three sites that see everything (mask -90 degrees), and the noise tables
    [S][SENSOR_TIME][m][3]"""
    from support.sensors import sites_rad
    xt, x, P, g = make_batch(SENSOR_M, seed=8)
    zn = np.stack([noise_table(1, SENSOR_TIME, SENSOR_M, seed=50 + s)[0] for s in range(SENSOR_S)])
    return xt, x, P, g, sites_rad()[:SENSOR_S], [g["R"].copy() for _ in range(SENSOR_S)], zn


def sensor_step(hip, Rs, zn, acts, form, propagator='hybrid'):
    """step 1 of the network (sensor s on object acts[s], R = Rs[s], noise zn[s]) from the batch of sensor_inputs():
      step     launch_step_sensors
      rollout  launch_rollout_sensors with a schedule of one row
      envs     launch_step_sensors_envs in E = 2 envs that hold the same state and noise; returns env 0's and env 1's results
    Returns (a list of, for 'envs') dict(x_true, x, P, obs, metrics, status, upd [S][UPD_STRIDE], stats, fail_log)."""
    torch, L, host = hip.torch, hip.lib, hip.host
    xt, x, P, g, lla, _, _ = sensor_inputs()
    m, S, T = SENSOR_M, SENSOR_S, SENSOR_TIME
    E = 2 if form == "envs" else 1
    lim = [-np.pi / 2] * S
    sp = host.make_sensor_params(lla, lim, Rs, T * m * 3)
    consts = host.make_consts(g["Q"], Rs[0], ALPHA, 2.0, -3, 20.0, lim[0], lla[0], propagator=propagator)
    table = np.ascontiguousarray(np.tile(zn[None], (E, 1, 1, 1, 1)))
    eng = hip.engine.HotPathEngine(consts, m, E, c2t()[:T], table, history=2, zn_stride_env=(S * T * m * 3 if E > 1 else 0))
    eng.load_state(0, np.tile(xt, (E, 1)), np.tile(x, (E, 1)), np.tile(P, (E, 1, 1)))
    upd = torch.zeros((E, S, L.UPD_STRIDE), dtype=torch.float64, device="cuda")
    if form == "step":
        eng.launch_step_sensors(0, 1, 1, sp, [int(a) for a in acts], upd.data_ptr(), fast_stats=True)
    elif form == "rollout":
        eng.launch_rollout_sensors(0, 1, sp, torch.as_tensor(np.asarray([acts], dtype=np.int32)).cuda())
    elif form == "envs":
        eng.launch_step_sensors_envs(0, 1, 1, sp, [list(acts)] * E, upd.data_ptr(), fast_stats=True)
    else:
        raise ValueError(form)
    torch.cuda.synchronize()
    if form == "rollout":
        upd = eng.upd_sensors[1][None]
    s, log, stats, rec = read_slot(eng, 1), fail_log(hip, eng), eng.stats[1].cpu().numpy(), upd.cpu().numpy()
    outs = []
    for e in range(E):
        sl = slice(e * m, (e + 1) * m)
        le = log[log[:, L.FAIL_ENV] == e].copy()
        le[:, L.FAIL_ENV] = 0.0
        outs.append(dict(x_true=s["x_true"][sl], x=s["x"][sl], P=s["P"][sl], obs=s["obs"][sl], metrics=s["metrics"][e], status=s["status"][sl],
                         upd=rec[e], stats=stats[e], fail_log=le))
    assert len(log) == sum(len(o["fail_log"]) for o in outs)
    return outs if form == "envs" else outs[0]


def assert_same_step(L, want, got, what, objects=None, records=None):
    """two sensor_step results: the rows of `objects` (default all) in every tensor, the records `records` (default all), and -- when
    nothing is left out -- the statistics and the failure log, bit for bit"""
    rows = slice(None) if objects is None else objects
    for k in ("x_true", "x", "P", "obs", "status"):
        assert same_bits(want[k][rows], got[k][rows]), (what, k)
    assert same_bits(want["metrics"][:, rows], got["metrics"][:, rows]), (what, "metrics")
    recs = range(want["upd"].shape[0]) if records is None else records
    assert_records_equal(L, want["upd"][list(recs)], got["upd"][list(recs)], what)
    if objects is None and records is None:
        cols = [getattr(L, c) for c in STAT_COLS]
        assert same_bits(want["stats"][cols], got["stats"][cols]), (what, want["stats"], got["stats"])
        assert want["fail_log"].shape == got["fail_log"].shape and same_bits(want["fail_log"], got["fail_log"]), (what, want["fail_log"], got["fail_log"])
