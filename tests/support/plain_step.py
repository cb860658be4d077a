"""The plain one-env step form run twice from one state -- once through step_plain_kernel, once with HotPathEngine.force_generic -- and
the whole-slot comparison of the two runs, bit for bit: what the tests of the plain family's store stage share."""
import ctypes as C

import numpy as np

from support.batches import c2t, make_batch

H = 2               # slots of the ring
N_STEPS = 6
N_TIME = N_STEPS + 1      # rows of the time table: ticks 0 .. N_STEPS, nothing wraps (the noise table is n_time x m x 3 doubles)


def planted(m):
    """the objects a case plants where its size allows it: (a NaN filter state, a filter that has failed at entry)"""
    return (1, 2) if m < 8 else (m - 3, 2)


def make_engine(hip, m, propagator, layout, generic, z_noise=None, R=None, plant=True):
    """z_noise ([1][N_TIME][m][3]) / R: another noise table / measurement covariance than the module's own; plant=False: the batch as
    make_batch gives it, nothing planted (callers that make filters fail INSIDE a step bring their own trouble)"""
    g = make_batch(8, seed=1)[3]
    consts = hip.host.make_consts(g["Q"], g["R"] if R is None else R, 1e-4, 2.0, -3, 20.0, np.radians(20.0), g["obs_lla"], obs_type='aer',
                                  propagator=propagator)
    xt, x, P, _ = make_batch(m, seed=1200 + m)
    nan_obj, failed_obj = planted(m)
    if plant:
        x[nan_obj, 1] = np.nan
    trans = c2t()[:N_TIME]
    zn = np.random.RandomState(3).normal(size=(1, N_TIME, m, 3)) * np.array([4.8e-6, 4.8e-6, 1e3]) if z_noise is None else z_noise
    eng = hip.engine.HotPathEngine(consts, m, 1, trans, zn, history=H)
    eng.force_generic = generic
    if layout:
        eng.set_layout(np.random.RandomState(m).permutation(m))
    eng.load_state(0, xt, x, P)
    if plant:
        pos = int(eng._slot_of[failed_obj]) if layout else failed_obj
        eng.status[pos] = hip.lib.ST_UPDATE_LINALG      # failed before the first step: its state passes through
    return eng, consts


def bits(t):
    """a copy of the tensor, doubles as their 64-bit patterns (NaN payloads and signed zeros compare as bits)"""
    import torch
    return t.clone().view(torch.int64) if t.dtype == torch.float64 else t.clone()


def slot_of(eng, s):
    return dict(xt=bits(eng.x_true[s]), x=bits(eng.x_filter[s]), P=bits(eng.P_filter[s]), obs=bits(eng.obs[s]), metrics=bits(eng.metrics[s]),
                status=bits(eng.status), upd=bits(eng.upd[s]))


def schedule(m):
    """object 0, the NaN one, the failed one, the last object, object 0 again, the object next to it"""
    nan_obj, failed_obj = planted(m)
    return [0, nan_obj, failed_obj, m - 1, 0, 1 % m]


def run(hip, m, propagator, layout, generic, z_noise=None, R=None, actions=None, plant=True):
    """N_STEPS deferred-fold steps through HipLocalStepper on the two-slot ring: the slot each step wrote, each step's statistics row
    (cloned once the next launch -- or flush() -- has folded it), the failure log, and the instance every launch took.  z_noise / R / plant: make_engine's; actions: another schedule of N_STEPS actions than schedule(m)"""
    from ssa_gym_amd import parallel
    eng, consts = make_engine(hip, m, propagator, layout, generic, z_noise=z_noise, R=R, plant=plant)
    assert eng.stats_from_metrics
    local = parallel.HipLocalStepper(eng, consts, fast_stats=True, defer_fold=True)
    local.load_schedule(schedule(m) if actions is None else list(actions))
    steps, rows = [], {}
    for _ in range(N_STEPS):
        local.step(-1)
        steps.append((local.tick, slot_of(eng, local.tick % H)))
        if local.tick > 1:
            rows[local.tick - 1] = bits(eng.stats[(local.tick - 1) % H])      # folded by the launch just enqueued
    local.flush()
    rows[local.tick] = bits(eng.stats[local.tick % H])
    hip.torch.cuda.synchronize()
    nf = int(eng.fail_count.cpu().numpy()[0])
    log = np.array(sorted(map(tuple, eng.fail_log[:nf]), key=lambda r: (r[hip.lib.FAIL_TIME], r[hip.lib.FAIL_OBJ])), dtype=np.float64)
    log = log.reshape(nf, -1) if nf else np.zeros((0, hip.lib.FAIL_STRIDE))
    lib = hip.lib.load()
    inst = {int(lib.ssa_env_step_instance(eng._cref, C.byref(ent[0]))) for ent in eng._pcache.values()}
    return dict(steps=steps, rows=rows, nfail=nf, fail_log=log, instances=inst)


def assert_same_bits(hip, want, got, what):
    eq = hip.torch.equal
    assert [t for t, _ in want["steps"]] == [t for t, _ in got["steps"]] == list(range(1, N_STEPS + 1)) == sorted(want["rows"]) == sorted(got["rows"])
    for (t, a), (_, b) in zip(want["steps"], got["steps"]):
        for k in a:
            assert eq(a[k], b[k]), (what, "step", t, k)
    for t in want["rows"]:
        assert eq(want["rows"][t], got["rows"][t]), (what, "statistics row of step", t)
    assert want["nfail"] == got["nfail"], what
    assert np.array_equal(want["fail_log"].view(np.int64), got["fail_log"].view(np.int64)), what
