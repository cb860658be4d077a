"""step_plain_kernel against the generic step kernel: a launch of the plain one-env form goes to the instance compiled for that form
(ssa_env_step_instance() == 1), and must compute what the generic instance computes, bit for bit -- the arithmetic is the same, only the
per-wavefront decisions are constants.  Two engines start from the same state, one with HotPathEngine.force_generic (SSA_LAUNCH_GENERIC),
and run the benchmark's form: 14 deferred-fold steps through HipLocalStepper on a ring of two slots, with an episode reset after step 9.
After EVERY step the slot just written is compared whole -- truth, state, covariance, observation rows, metrics, status words and the
update record -- then every step's statistics row (each cloned as soon as its fold is enqueued; the last by flush()), the failure log and
its count.  No tolerance, no object left out.

Object counts as tests/test_stats_from_metrics_gpu.py: 64 (16 whole tiles), 66 (a ragged last tile), 260, 4 100.  Planted: a filter that
has failed at entry (its state passes through), a NaN filter state, the recorded ill-conditioned wavefront of
tests/golden/ladder_illconditioned_tile.npz and a scaled copy of its worst matrix (the jitter ladder), an object at the observer's zenith
(visible: its update is taken) and one at the nadir (selected, never visible).  The schedule selects object 0, the visible one, the
invisible one, the failed ones and the ladder's."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
from support.batches import c2t, make_batch
from support.gpu import hip  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

SIZES = (64, 66, 260, 4100)
EP, N1, N2, H = 24, 9, 5, 2
FAILED_AT_ENTRY, NAN_STATE, LADDER_COPY, ZENITH, NADIR = 5, 42, 20, 30, 31
MU = 3.986004418e14


def planted_batch(m, consts):
    xt, x, P, g = make_batch(m, seed=700 + m)
    tile = golden("ladder_illconditioned_tile.npz")
    x[8:12] = tile["x_tile"]                     # one whole wavefront (objects 8 .. 11), as recorded
    xt[8:12] = tile["x_tile"] + np.array([3e3, -2e3, 1e3, 1.0, -1.0, 0.5])
    P[8:12] = tile["P_tile"]
    j = int(tile["obj"]) % 4
    x[LADDER_COPY], xt[LADDER_COPY], P[LADDER_COPY] = tile["x_tile"][j], xt[8 + j], 0.5 * tile["P_tile"][j]
    x[NAN_STATE, 1] = np.nan
    # a circular orbit 800 km above the observer at time index 3 (and its antipode): GCRS = M^T ITRS
    M = c2t()[3].reshape(3, 3)
    site = np.array(list(consts.obs_itrs))
    up = site / np.linalg.norm(site)
    r = np.linalg.norm(site) + 800e3
    east = np.cross([0.0, 0.0, 1.0], up)
    east /= np.linalg.norm(east)
    v = M.T @ east * np.sqrt(MU / r)
    for k, sign in ((ZENITH, 1.0), (NADIR, -1.0)):
        xt[k] = np.concatenate([sign * (M.T @ up) * r - 3 * 20.0 * v, v])     # (three steps of 20 s before the pass overhead)
        x[k] = xt[k] + np.array([2e3, -1e3, 1.5e3, 1.0, 0.5, -1.0])
    return xt, x, P, g


def schedule(m):
    """tick -> action: the first episode's nine steps, then the five behind the reset (ticks EP + 1 ..)"""
    first = [0, ZENITH, NADIR, FAILED_AT_ENTRY, NAN_STATE, 9, ZENITH, LADDER_COPY, m - 1]
    second = [0, ZENITH, NADIR, 10, 3]
    sched = np.full(EP + N2 + 1, 1, dtype=np.int32)
    sched[:N1] = first
    sched[EP:EP + N2] = second
    return sched


def make_engine(hip, m, propagator, layout, generic, E=1):
    g = make_batch(8, seed=1)[3]
    consts = hip.host.make_consts(g["Q"], g["R"], 1e-4, 2.0, -3, 20.0, np.radians(20.0), g["obs_lla"], obs_type='aer', propagator=propagator)
    xt, x, P, _ = planted_batch(m, consts)
    zn = np.random.RandomState(1).normal(size=(E, c2t().shape[0], m, 3)) * np.array([4.8e-6, 4.8e-6, 1e3])
    eng = hip.engine.HotPathEngine(consts, m, E, c2t(), zn, history=H)
    assert eng.force_generic is False
    eng.force_generic = generic
    if layout:
        eng.set_layout(np.random.RandomState(m).permutation(m))
    eng.load_state(0, np.tile(xt, (E, 1)), np.tile(x, (E, 1)), np.tile(P, (E, 1, 1)))
    pos = int(eng._slot_of[FAILED_AT_ENTRY]) if layout else FAILED_AT_ENTRY
    eng.status[pos] = hip.lib.ST_UPDATE_LINALG      # failed before the first step: skipped, its state passes through
    return eng, consts


def bits(t):
    """a copy of the tensor, doubles as their 64-bit patterns (NaN payloads and signed zeros compare as bits)"""
    import torch
    return t.clone().view(torch.int64) if t.dtype == torch.float64 else t.clone()


def equal(a, b):
    import torch
    return torch.equal(a, b)


def slot_of(eng, s):
    return dict(xt=bits(eng.x_true[s]), x=bits(eng.x_filter[s]), P=bits(eng.P_filter[s]), obs=bits(eng.obs[s]), metrics=bits(eng.metrics[s]),
                status=bits(eng.status), upd=bits(eng.upd[s]))


def instances(hip, eng):
    """what the query answers for every parameter block the engine has launched"""
    lib = hip.lib.load()
    return {int(lib.ssa_env_step_instance(eng._cref, C.byref(ent[0]))) for ent in eng._pcache.values()}


def run(hip, m, propagator, layout, generic):
    from ssa_gym_amd import parallel
    eng, consts = make_engine(hip, m, propagator, layout, generic)
    assert eng.stats_from_metrics
    snap = eng.snapshot(0)
    local = parallel.HipLocalStepper(eng, consts, fast_stats=True, defer_fold=True)
    local.load_schedule(schedule(m).tolist())
    steps, rows, prev = [], {}, [None]

    def step():
        local.step(-1)
        steps.append((local.tick, slot_of(eng, local.tick % H)))
        if prev[0] is not None:
            rows[prev[0]] = bits(eng.stats[prev[0] % H])      # folded by the launch just enqueued
        prev[0] = local.tick
    for _ in range(N1):
        step()
    local.reset_episode(snap, EP)
    rows[prev[0]], prev[0] = bits(eng.stats[prev[0] % H]), None
    for _ in range(N2):
        step()
    local.flush()
    rows[prev[0]] = bits(eng.stats[prev[0] % H])
    hip.torch.cuda.synchronize()
    nf = int(eng.fail_count.cpu().numpy()[0])
    assert [t for t, _ in steps] == list(range(1, N1 + 1)) + list(range(EP + 1, EP + N2 + 1)) == sorted(rows)
    # (the records land in the order the failing wavefronts reach the counter: sorted by step and object, which name a record)
    log = np.array(sorted(map(tuple, eng.fail_log[:nf]), key=lambda r: (r[hip.lib.FAIL_TIME], r[hip.lib.FAIL_OBJ]))).reshape(nf, -1)
    return dict(steps=steps, rows=rows, nfail=nf, fail_log=log, instances=instances(hip, eng))


def assert_same_bits(want, got, what):
    for (t, a), (_, b) in zip(want["steps"], got["steps"]):
        for k in a:
            assert equal(a[k], b[k]), (what, "step", t, k)
    for t in want["rows"]:
        assert equal(want["rows"][t], got["rows"][t]), (what, "statistics row of step", t)
    assert want["nfail"] == got["nfail"], what
    assert np.array_equal(want["fail_log"].view(np.int64), got["fail_log"].view(np.int64)), what


@pytest.mark.parametrize("layout", [False, True])
@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("propagator", ["hybrid", "fg"])
def test_plain_instance_equals_the_generic_one_bit_for_bit(hip, propagator, m, layout):
    L = hip.lib
    want = run(hip, m, propagator, layout, generic=True)
    got = run(hip, m, propagator, layout, generic=False)
    assert want["instances"] == {0} and got["instances"] == {1}      # the forced engine ran generic launches only, the other plain ones only
    assert_same_bits(want, got, (propagator, m, layout))
    # the schedule and the planted state did their work in the generic run
    rec = {t: s["upd"].view(hip.torch.float64)[0].cpu().numpy() for t, s in want["steps"]}
    assert rec[1][L.UPD_ACTION] == 0
    assert rec[2][L.UPD_ACTION] == ZENITH and rec[2][L.UPD_VISIBLE] == 1 and rec[2][L.UPD_OBS_TAKEN] == 1
    assert rec[3][L.UPD_ACTION] == NADIR and rec[3][L.UPD_VISIBLE] == 0 and rec[3][L.UPD_OBS_TAKEN] == 0
    assert rec[4][L.UPD_ACTION] == -1 and rec[5][L.UPD_ACTION] == -1          # failed filters are skipped: no attempt
    assert rec[EP + 2][L.UPD_ACTION] == ZENITH and rec[EP + 3][L.UPD_ACTION] == NADIR
    first = want["steps"][0][1]
    order = np.random.RandomState(m).permutation(m) if layout else np.arange(m)
    at = {int(o): i for i, o in enumerate(order)}
    st = first["status"].cpu().numpy()
    assert st[at[FAILED_AT_ENTRY]] == L.ST_UPDATE_LINALG and st[at[NAN_STATE]] != 0 and want["nfail"] >= 1
    stats_last = want["rows"][N1].view(hip.torch.float64)[0].cpu().numpy()
    assert stats_last[L.STAT_N_FAILED] >= 2


def one_launch(hip, generic, kind):
    m = 8 if kind == "two envs" else 66
    E = 2 if kind == "two envs" else 1
    eng, _ = make_engine_small(hip, m, E, generic)
    sched = hip.torch.as_tensor(np.array([3] * E, dtype=np.int32)).cuda()
    mirror = hip.torch.zeros((E * m, 12), dtype=hip.torch.float64, device="cuda")
    kw = dict(fast_stats=True, actions_ptr=sched.data_ptr())
    if kind == "fold inside":
        kw.update(fold_inside=True)
    elif kind == "obs mirror":
        kw.update(defer_fold=True, obs_mirror=mirror.data_ptr())
    else:
        kw.update(defer_fold=True)
    eng.launch_step(0, 1, 1, **kw)
    eng.flush_stats()
    hip.torch.cuda.synchronize()
    out = slot_of(eng, 1)
    out.update(stats=bits(eng.stats[1]), mirror=bits(mirror))
    return out, instances(hip, eng)


def make_engine_small(hip, m, E, generic):
    g = make_batch(8, seed=1)[3]
    consts = hip.host.make_consts(g["Q"], g["R"], 1e-4, 2.0, -3, 20.0, np.radians(20.0), g["obs_lla"], obs_type='aer', propagator="hybrid")
    xt, x, P, _ = make_batch(m, seed=900 + m)
    zn = np.random.RandomState(2).normal(size=(E, c2t().shape[0], m, 3)) * np.array([4.8e-6, 4.8e-6, 1e3])
    eng = hip.engine.HotPathEngine(consts, m, E, c2t(), zn, history=H)
    eng.force_generic = generic
    eng.load_state(0, np.tile(xt, (E, 1)), np.tile(x, (E, 1)), np.tile(P, (E, 1, 1)))
    return eng, consts


@pytest.mark.parametrize("kind", ["two envs", "fold inside", "obs mirror"])
def test_launches_outside_the_plain_form_stay_generic(hip, kind):
    want, wi = one_launch(hip, True, kind)
    got, gi = one_launch(hip, False, kind)
    assert wi == {0} and gi == {0}, (kind, wi, gi)
    for k in want:
        assert equal(want[k], got[k]), (kind, k)
    if kind == "obs mirror":
        assert equal(got["mirror"], got["obs"])
