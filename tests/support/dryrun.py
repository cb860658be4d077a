"""The dry run of candidate schedules (ssa_dryrun_sensors_envs_f64): the refusal harness of its host test -- complete blocks and a
refused() of its own, as support/refusals.py has for the other entries -- and the GPU tests' shared pieces: envs, the record of a call
as bits, the step-by-step yardstick chain and the forecast's entries of a once-per-object schedule."""
import ctypes as C

import numpy as np

from support.refusals import LOOK_PTRS, PTR, _fill

ENTRY = "ssa_dryrun_sensors_envs_f64"
ALIGNED = 0x1000     # a 32-byte aligned address (never dereferenced on the host)


def valid_blocks(n_env=2, n_obj=8):
    """{short name: block} in argument order: blocks that pass every check of the entry -- 2 pseudo-envs of 8 rows, 2 sensors, 3 steps"""
    from ssa_gym_amd import _lib, host
    d = _lib.ssa_dryrun_sensors_params()
    d.n_steps, d.n_obj_caller, d.actions, d.out = 3, 100, ALIGNED, PTR
    return {"c": host.make_consts(np.eye(6), np.eye(3), 1e-4, 2.0, -3, 20.0, -np.pi / 2, np.array([0.6, -1.3, 20.0])),
            "p": _fill(_lib.ssa_step_params(), LOOK_PTRS, n_obj=n_obj, n_env=n_env),
            "sp": _fill(_lib.ssa_sensor_params(), (), n_sensor=2, zn_stride_sensor=384),
            "d": d}


def refused(fn, *fields, null=None, spoil=None, **shape):
    """the code the entry answers complete blocks with the named (block, field, value) spoiled; null: an argument passed as NULL"""
    b = valid_blocks(**shape)
    for which, name, value in fields:
        setattr(b[which], name, value)
    if spoil:
        spoil(b)
    args = [C.byref(blk) for blk in b.values()]
    if null is not None:
        args[null] = None
    return fn(*args, None)


class StubEnv:
    """what agents.refine_plan_sensors reads of an env, with an evaluator that counts its calls and values a schedule by the sum of its entries (the info-gain column; trace gain: minus that)"""

    def __init__(self, m=10, S=2, n=20):
        self._engine, self.i, self.n, self.m, self.n_sensor = object(), 0, n, m, S
        self.calls, self.forecasts = [], 0

    def forecast_sensors(self, horizon):
        import torch
        self.forecasts += 1
        return {"visible": torch.ones((horizon, self.n_sensor, self.m), dtype=torch.uint8),
                "status": torch.zeros((horizon, self.n_sensor, self.m), dtype=torch.int32)}

    def evaluate_schedules(self, actions):
        import torch
        a = np.asarray(actions)
        a = a[None] if a.ndim == 2 else a
        self.calls.append(a.copy())
        tot = a.reshape(a.shape[0], -1).sum(axis=1).astype(np.float64)
        return {"total": torch.as_tensor(np.stack([-tot, 2 * tot, tot], axis=1))}


# ---------------------------------------------------------------------------------------------------------------- GPU side
KEYS = ("score", "taken", "visible", "status", "action")
SITES = [(38.828198, -77.305352, 20.0), (39.6, -76.1, 150.0), (38.1, -78.6, 400.0)]      # three sites that share passes
MASKS_DEG = [15.0, 5.0, 25.0]
BAD, FAILED = 9, 21      # BAD's filter state is NaN (it fails in the first predict of a launch); FAILED's filter had failed before
WARM = ([5, 6, 7], [8, 5, 30])      # the two steps every engine case has run: the launches start at step 2


def record_bits(rec):
    """a record tensor [B, K, S, DRY_STRIDE] as the fields of evaluate_schedules(), integers (the scores as their bit patterns)"""
    import torch
    from ssa_gym_amd import _lib as L
    torch.cuda.synchronize()
    r = rec.cpu().numpy().copy()
    return {"score": np.ascontiguousarray(r[..., L.DRY_SCORE:L.DRY_SCORE + 3]).view(np.int64), "taken": r[..., L.DRY_TAKEN].astype(np.int64),
            "visible": r[..., L.DRY_VISIBLE].astype(np.int64), "status": r[..., L.DRY_STATUS].astype(np.int64),
            "action": r[..., L.DRY_ACTION].astype(np.int64), "spare": np.ascontiguousarray(r[..., L.DRY_SPARE]).view(np.int64)}


def result_bits(res):
    """an evaluate_schedules() result as integer arrays (the doubles as their bit patterns), copied off the engine's buffers"""
    import torch
    torch.cuda.synchronize()
    return {k: (v.contiguous().view(torch.int64) if v.dtype == torch.float64 else v.to(torch.int64)).cpu().numpy() for k, v in res.items()}


def same_result(a, b, what="", keys=KEYS):
    for k in keys:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k, np.argwhere(a[k] != b[k])[:4].tolist())


def make_case(hip, m=403, propagator="hybrid", obs_type="aer", interval=1, layout=False, special=True):
    """(engine, sites, slot, time index of the next step, storage row of every object): m objects, three sites, two steps run (WARM),
    then -- special -- BAD's filter state made NaN and FAILED's status a failure, written into the engine's tensors"""
    from support.batches import c2t, make_batch
    from support.sensors import N_TIME
    torch, L, host = hip.torch, hip.lib, hip.host
    S = len(SITES)
    xt, x, P, g = make_batch(m, seed=123)
    lla = [np.array([np.radians(la), np.radians(lo), h]) for la, lo, h in SITES]
    lim = np.radians(MASKS_DEG)
    if obs_type == "aer":
        sig = [np.array([(1.0 + k) * host.arcsec2rad, (0.5 + 2.0 * k) * host.arcsec2rad, 1e3 / (1 + k)]) for k in range(S)]
    else:
        sig = [np.array([5e2 / (1 + 0.25 * k)] * 3) for k in range(S)]
    Rs = [np.diag(v ** 2) for v in sig]
    sp = host.make_sensor_params(lla, lim, Rs, N_TIME * m * 3)
    consts = host.make_consts(g["Q"], Rs[0], 1e-4, 2.0, -3, 20.0, lim[0], lla[0], propagator=propagator, obs_type=obs_type,
                              update_interval=interval)
    zn = torch.zeros((S, N_TIME, m, 3), dtype=torch.float64, device="cuda")      # (zero noise: the warm-up's innovations are the model's)
    eng = hip.engine.HotPathEngine(consts, m, 1, c2t()[:N_TIME], zn, history=2, zn_stride_env=0)
    pos = np.arange(m)
    if layout:
        from ssa_gym_amd.catalogue import regime_order
        order = regime_order(xt)
        eng.set_layout(order)
        pos = np.argsort(order)
    eng.load_state(0, xt, x, P)
    for k, acts in enumerate(WARM):
        eng.launch_step_sensors(k % 2, (k + 1) % 2, 1 + k, sp, list(acts), 0, fast_stats=True)
    eng.flush_stats()
    torch.cuda.synchronize()
    if special:
        eng.x_filter[0, int(pos[BAD]), 1] = float("nan")
        eng.status[int(pos[FAILED])] = L.ST_UPDATE_NAN
    torch.cuda.synchronize()
    return eng, sp, 0, 1 + len(WARM), pos


def cleared(K, S):
    return {"score": np.full((1, K, S, 3), np.nan), "taken": np.zeros((1, K, S), np.int64), "visible": np.zeros((1, K, S), np.int64),
            "status": np.zeros((1, K, S), np.int64), "action": np.full((1, K, S), -1, np.int64)}


def owners_of(row, m):
    """{object: the sensor that updates it} of one action row: valid entries, the lowest-numbered sensor of several on one object"""
    own = {}
    for s, j in enumerate(int(v) for v in row):
        if 0 <= j < m and j not in own:
            own[j] = s
    return own


def forecast_entries(fc, sched, m, t0, interval=1):
    """the entries (k, s, sched[k, s]) of a read-back forecast as the records of one candidate whose valid entries name each object at
    most once: score bits, status, visible, taken (= the score is a number), and the action by the step's rule (the object, unless its
    filter has failed by then).  An idle or out-of-range slot and a step the interval skips: the cleared record."""
    from ssa_gym_amd import _lib as L
    K, S = sched.shape
    out = cleared(K, S)
    for k in range(K):
        if interval > 1 and (t0 + k) % interval:
            continue
        for j, s in owners_of(sched[k], m).items():
            out["score"][0, k, s] = fc["score"][k, s, j]
            out["status"][0, k, s] = fc["status"][k, s, j]
            out["visible"][0, k, s] = fc["visible"][k, s, j]
            out["taken"][0, k, s] = int(not np.isnan(fc["score"][k, s, j, 0]))
            out["action"][0, k, s] = j if fc["status"][k, s, j] in (L.ST_OK, L.ST_UPDATE_LINALG) else -1
    out["score"] = out["score"].view(np.int64)
    return out


def step_chain(torch, eng, sp, sched, slot0, t0):
    """The yardstick of a schedule with revisits, on `eng` (a twin, spent by it): for k = 0 .. K-1 the network's lookahead with
    covariances -- the expected record of every slot of row k --, then an all-idle sensor step, then for every taken slot P_post[s, j]
    written into object j's row of the new P_filter slot.  Returns the records of the one candidate as record_bits() would, and the
    lookahead's read-back scores per step ([K, S, m, 3]) for the tests' own assertions."""
    from ssa_gym_amd import _lib as L
    K, S = sched.shape
    m, H = eng.m, eng.H
    interval = int(eng.consts.update_interval)
    out = cleared(K, S)
    looks = []
    for k in range(K):
        si, so, t = (slot0 + k) % H, (slot0 + k + 1) % H, t0 + k
        look = eng.launch_lookahead_sensors(si, t, sp, out=("P_post",))
        torch.cuda.synchronize()
        score, status, visible = (look[key].cpu().numpy().copy() for key in ("score", "status", "visible"))
        P_post = look["P_post"].clone()
        looks.append(score)
        eng.launch_step_sensors(si, so, t, sp, [-1] * S, 0, fast_stats=True)
        eng.flush_stats()
        torch.cuda.synchronize()
        if interval > 1 and t % interval:
            continue
        for j, s in owners_of(sched[k], m).items():
            st = int(status[s, j])
            assert st != L.ST_UPDATE_LINALG, "the chain does not model a singular S (slot %d, %d)" % (k, s)
            out["status"][0, k, s] = st
            if st == L.ST_OK:
                out["action"][0, k, s] = j
                out["visible"][0, k, s] = int(visible[s, j])
                if not np.isnan(score[s, j, 0]):
                    out["taken"][0, k, s] = 1
                    out["score"][0, k, s] = score[s, j]
                    row = int(eng._slot_of[j]) if eng._order is not None else j
                    eng.P_filter[so, row].copy_(P_post[s, j])
    torch.cuda.synchronize()
    out["score"] = out["score"].view(np.int64)
    return out, np.stack(looks)


def slot_total(rec, column):
    """the sum of the taken slots' scores of one candidate's records (bits) in slot order, k outer and s inner, as fp64; 0 for none"""
    tot = np.float64(0.0)
    score = rec["score"].view(np.float64)
    for k in range(score.shape[1]):
        for s in range(score.shape[2]):
            if rec["taken"][0, k, s]:
                tot = tot + score[0, k, s, column]
    return tot
