"""The plain family's unscented transform with SSA_FLAG_REFERENCE_COV (sigma_rows_write / moment_sums_rows / covariance_reference_rows,
ssa_kernels.hip): both matrix passes are fed from ONE tile of the propagated sigma points, the differences formed in the matrix unit's
operand layout.  The yardstick is the generic instance (HotPathEngine.force_generic), which keeps the two tiles of differences.

Everything a step writes -- truth, state, covariance, status, observation rows, metrics, the update record, the statistics rows once
flushed, the failure records and their count -- must be the same BITS in both instances at

  3 objects     a ragged tile only
  4, 8          one and two whole tiles
  66, 260       whole tiles and a ragged one; more than one block

in these cases: `hybrid` with and without a storage layout; `fg` with the flag forced on (its default covariance is the centred one);
a planted NaN state and a filter failed at entry in every one of them; ten consecutive steps from a DIVERGED prior.

The diverged prior (tests/golden/transform_tile_diverged.npz) is the CPU oracle's state of tests/episode_workload.py's seed-7 episode
after step 300, the healthy filters whose propagated sigma_0' lies >= 1e8 m from the prior mean x (26 of 2 000).  There the reference's
y_i = sigma_i' - x (one rounding) and the two-rounding (sigma_i' - sigma_0') - m' differ -- the error that once withdrew a tile-less second
pass: the fixture's test checks with numpy that they do, so the comparison on the GPU can see it.  `python tests/test_transform_tile_gpu.py`
writes the fixture again."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

if __name__ != "__main__":
    from conftest import golden
    from support.batches import c2t, make_batch
    from support.gpu import hip  # noqa: F401  (the module fixture)
    from support.plain_step import H, bits, planted, slot_of

pytestmark = pytest.mark.gpu

SIZES = [3, 4, 8, 66, 260]
FIXTURE = "transform_tile_diverged.npz"
FIXTURE_STEP, FIXTURE_DIST = 300, 1e8


def _run(hip, m, propagator, layout, generic, n_steps=6, force_flag=False, state=None):
    """n_steps deferred-fold steps on the two-slot ring: what every step wrote, every statistics row once folded, the failure log, the
    instances the launches took.  state: (x_true, x, P) instead of the planted batch"""
    from ssa_gym_amd import parallel
    L = hip.lib
    g = make_batch(8, seed=1)[3]
    consts = hip.host.make_consts(g["Q"], g["R"], 1e-4, 2.0, -3, 20.0, np.radians(20.0), g["obs_lla"], obs_type='aer', propagator=propagator)
    if force_flag:
        consts.flags |= L.FLAG_REFERENCE_COV
    assert consts.flags & L.FLAG_REFERENCE_COV
    n_time = n_steps + 1
    if state is None:
        xt, x, P, _ = make_batch(m, seed=1200 + m)
        nan_obj, failed_obj = planted(m)
        x[nan_obj, 1] = np.nan
        sched = [0, nan_obj, failed_obj, m - 1, 0, 1 % m]
    else:
        xt, x, P = state
        sched = [k % m for k in range(n_steps)]
    zn = np.random.RandomState(3).normal(size=(1, n_time, m, 3)) * np.array([4.8e-6, 4.8e-6, 1e3])
    eng = hip.engine.HotPathEngine(consts, m, 1, c2t()[:n_time], zn, history=H)
    eng.force_generic = generic
    if layout:
        eng.set_layout(np.random.RandomState(m).permutation(m))
    eng.load_state(0, xt, x, P)
    if state is None:
        eng.status[int(eng._slot_of[failed_obj]) if layout else failed_obj] = L.ST_UPDATE_LINALG
    assert eng.stats_from_metrics
    local = parallel.HipLocalStepper(eng, consts, fast_stats=True, defer_fold=True)
    local.load_schedule(sched[:n_steps])
    steps, rows = [], {}
    for _ in range(n_steps):
        local.step(-1)
        steps.append(slot_of(eng, local.tick % H))
        if local.tick > 1:
            rows[local.tick - 1] = bits(eng.stats[(local.tick - 1) % H])      # folded by the launch just enqueued
    local.flush()
    rows[local.tick] = bits(eng.stats[local.tick % H])
    hip.torch.cuda.synchronize()
    nf = int(eng.fail_count.cpu().numpy()[0])
    log = np.array(sorted(map(tuple, eng.fail_log[:nf]), key=lambda r: (r[L.FAIL_TIME], r[L.FAIL_OBJ])), dtype=np.float64)
    log = log.reshape(nf, -1) if nf else np.zeros((0, L.FAIL_STRIDE))
    lib = L.load()
    inst = {int(lib.ssa_env_step_instance(eng._cref, C.byref(ent[0]))) for ent in eng._pcache.values()}
    return dict(steps=steps, rows=rows, nfail=nf, fail_log=log, instances=inst)


def _assert_same_bits(hip, want, got, what):
    eq = hip.torch.equal
    assert want["instances"] == {0} and got["instances"] == {1}, what      # generic launches only | plain ones only
    assert len(want["steps"]) == len(got["steps"]) and sorted(want["rows"]) == sorted(got["rows"]) == list(range(1, len(want["steps"]) + 1))
    for t, (a, b) in enumerate(zip(want["steps"], got["steps"])):
        for k in a:
            assert eq(a[k], b[k]), (what, "step", t + 1, k)
    for t in want["rows"]:
        assert eq(want["rows"][t], got["rows"][t]), (what, "statistics row of step", t)
    assert want["nfail"] == got["nfail"], what
    assert np.array_equal(want["fail_log"].view(np.int64), got["fail_log"].view(np.int64)), what


@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("case", ["hybrid", "hybrid-layout", "fg-flag"])
def test_one_tile_of_sigma_points_gives_the_generic_instances_bits(hip, case, m):
    L = hip.lib
    propagator, layout, force = ("fg", False, True) if case == "fg-flag" else ("hybrid", case == "hybrid-layout", False)
    want = _run(hip, m, propagator, layout, generic=True, force_flag=force)
    got = _run(hip, m, propagator, layout, generic=False, force_flag=force)
    _assert_same_bits(hip, want, got, (case, m))
    # the planted state did its work in the generic run: the failed filter kept its status, the NaN state failed in the first step,
    # both are counted -- and the other filters are alive with a finite covariance (the comparison is not one of sentinels)
    nan_obj, failed_obj = planted(m)
    order = np.random.RandomState(m).permutation(m) if layout else np.arange(m)
    at = {int(o): i for i, o in enumerate(order)}
    st = want["steps"][0]["status"].cpu().numpy()
    assert st[at[failed_obj]] == L.ST_UPDATE_LINALG and st[at[nan_obj]] != 0 and want["nfail"] >= 1
    last = want["rows"][len(want["steps"])].view(hip.torch.float64)[0].cpu().numpy()
    assert last[L.STAT_N_FAILED] >= 2
    st_end = want["steps"][-1]["status"].cpu().numpy()
    alive = st_end == 0
    assert alive.sum() >= m - 2
    P_end = want["steps"][-1]["P"].view(hip.torch.float64).cpu().numpy().reshape(m, 36)
    assert np.isfinite(P_end[alive]).all()


def _diverged():
    f = golden(FIXTURE)
    return f["x_true"], f["x"], f["P"]


def _transform_operands(x, P):
    """(sigma_i', sigma_0' - x, the rows y_i in the reference's one rounding, the rows in two roundings) of one filter, the mean in the
    kernel's centred form -- all on the CPU: the oracle's sigma points and propagator, numpy's IEEE doubles"""
    import oracle as orc
    from ssa_gym_amd import host
    Wm, Wc, scale = orc.merwe_weights(1e-4, 2.0, -3)
    o = orc.Oracle()
    sp = o.propagate(o.sigma_points(x, P, scale), 20.0)
    mp = host.exact_weight_sums(Wm, Wc)[0] * sp[0] + Wm[1] * (sp[1:] - sp[0]).sum(axis=0)
    xb = sp[0] + mp
    return sp, sp[0] - xb, sp - xb, (sp - sp[0]) - mp


@pytest.fixture(scope="module")
def diverged():
    """the fixture's filters, checked on the CPU before any use: every one of them >= 1e8 m from its sigma_0', and the two-rounding rows
    differ from the reference's in at least one bit for every one of them"""
    xt, x, P = _diverged()
    assert len(x) >= 8
    for j in range(len(x)):
        sp, off, one, two = _transform_operands(x[j], P[j])
        assert np.isfinite(sp).all() and np.linalg.norm(off[:3]) >= FIXTURE_DIST, j
        assert (one.view(np.int64) != two.view(np.int64)).any(), j
    return xt, x, P


@pytest.mark.parametrize("m", SIZES)
def test_ten_steps_from_a_diverged_prior_give_the_generic_instances_bits(hip, diverged, m):
    xt, x, P = diverged
    pick = np.arange(m) % len(x)      # (the same filter in several rows and tiles: every row computes for itself)
    state = (xt[pick].copy(), x[pick].copy(), P[pick].copy())
    want = _run(hip, m, "hybrid", m >= 8, generic=True, n_steps=10, state=state)
    got = _run(hip, m, "hybrid", m >= 8, generic=False, n_steps=10, state=state)
    _assert_same_bits(hip, want, got, ("diverged", m))
    # the comparison is one of live filters at the start, and the reference's covariance arithmetic then fails some of them -- the
    # behaviour the flag exists for -- which both instances record alike
    st0 = want["steps"][0]["status"].cpu().numpy()
    assert (st0 == 0).sum() >= (m + 1) // 2
    P1 = want["steps"][0]["P"].view(hip.torch.float64).cpu().numpy().reshape(m, 36)
    assert np.isfinite(P1[st0 == 0]).all()


def _regenerate():
    """the oracle's seed-7 episode to FIXTURE_STEP, the healthy filters that lie >= FIXTURE_DIST from their propagated sigma_0'"""
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here), os.path.join(os.path.dirname(here), "oracle")):
        sys.path.insert(0, p)
    import oracle as orc
    import episode_workload as ew
    w = ew.workload(seed=7)
    o = orc.Oracle(omp=True)
    g, m = w["g"], w["m"]
    Wm, Wc, scale = orc.merwe_weights(1e-4, 2.0, -3)
    xt, x, P, st = w["x_true"], w["x"], w["P"], np.zeros(m, dtype=np.int32)
    for i in range(1, FIXTURE_STEP + 1):
        a = (i - 1) % m
        r = o.env_step(xt, x, P, st, 20.0, g["Q"], g["R"], Wm, Wc, scale, a, w["c2t"][i], g["obs_lla"], g["obs_itrs"], -np.pi / 2, w["z_noise"][i, a])
        xt, x, P = r["x_true"], r["x"], r["P"]
    keep = []
    for j in np.where(st == 0)[0]:
        try:
            sp, off, one, two = _transform_operands(x[j], P[j])
        except np.linalg.LinAlgError:
            continue
        if np.isfinite(sp).all() and np.linalg.norm(off[:3]) >= FIXTURE_DIST and (one.view(np.int64) != two.view(np.int64)).any():
            keep.append(int(j))
    out = os.path.join(here, "golden", FIXTURE)
    np.savez(out, ids=np.array(keep), x_true=xt[keep], x=x[keep], P=P[keep])
    print(out, len(keep), "filters")


if __name__ == "__main__":
    _regenerate()
