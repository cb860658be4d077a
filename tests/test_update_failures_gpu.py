"""UKF update failures forced INSIDE a step, on every launch form of the step family.

A filter can fail in two ways during the update (ssa_tasker_simple_2.py:300-315, 369-382; ssa_kernels.hip, Phase 2 of the update):
SSA_ST_UPDATE_NAN (x + K y has a NaN: the update is booked, then filter_error) and SSA_ST_UPDATE_LINALG (inv(S) refused: nothing is
booked, then filter_error).  tests/support/update_failures.py has the two recipes, tests/test_update_failures_host.py pins them to the
fp64 oracle.  Here:

  A  one generic step (step + post + final) against the oracle and against its clean twin;
  B  a six-step schedule with both failures through every one-env form, several envs and a storage layout, bit-identical to A's form;
  C  sensor networks: a singular S is per sensor;
  D  the lookahead's status 4 and sentinel P_post against the step;
  E  the gym surface: failed_filters_id / failed_filters_msg / obs_taken.

Every test asserts the number of status 3 and status 4 words it expects: a recipe that stops failing fails the test.  For the failing
object the fp64 oracle is the authority -- the 80-bit oracle does not flag R_OVERFLOW (1e309 is finite there) and is not used."""
import numpy as np
import pytest

from support import plain_step
from support import update_failures as uf
from support.batches import make_batch
from support.gpu import envs, hip  # noqa: F401  (the module fixtures)

pytestmark = pytest.mark.gpu

EPS = 2.220446049250313e-16
CODE = {"nan": 3, "linalg": 4}


# ================================================================ A. one generic step against the oracle

# (m, a): the failing object in every row of a wavefront's four-object tile, and in a ragged last tile
PAIRS = ((1, 0), (4, 0), (4, 3), (5, 4), (12, 5), (12, 6))
TIX, NAN_COMP = 1, 1


def _two_steps(hip, xt, x, P, g, a, obs_type, propagator, resample):
    """launch(z_noise, R) of twin(): the generic three-launch step with action a, then a second one with the same action"""
    def launch(z, R):
        eng = uf.engine(hip, xt, x, P, g, z, R, obs_type=obs_type, propagator=propagator, resample=resample, history=3)
        out = []
        for k in (0, 1):
            eng.set_actions([a])
            eng.launch_step(k, k + 1, TIX + k)
            hip.torch.cuda.synchronize()
            s = uf.read_slot(eng, k + 1)
            s.update(stats=eng.stats[k + 1, 0].cpu().numpy(), fail_log=uf.fail_log(hip, eng))
            out.append(s)
        assert uf.instances(hip, eng) == {0}
        return out
    return launch


@pytest.mark.parametrize("resample", [False, True])
@pytest.mark.parametrize("propagator", ["fg", "hybrid"])
@pytest.mark.parametrize("obs_type", ["aer", "xyz"])
@pytest.mark.parametrize("failure", ["nan", "linalg"])
def test_one_generic_step_against_the_oracle(hip, oracle, failure, obs_type, propagator, resample):
    L = hip.lib
    n3 = n4 = 0
    for m, a in PAIRS:
        xt, x, P, g = make_batch(m, seed=8)
        R = uf.golden_R(g, obs_type)
        zn = uf.noise_table(1, 8, m)
        if failure == "nan":
            poison = lambda z, R_: (uf.nan_noise(z, 0, TIX, a, NAN_COMP), R_)      # noqa: E731
        else:
            poison = uf.poison_overflow
        (clean, clean2), (bad, bad2) = uf.twin(hip, _two_steps(hip, xt, x, P, g, a, obs_type, propagator, resample), zn, R, poison)
        zp, Rp = poison(zn, R)
        f64 = uf.oracle_step(oracle, xt, x, P, g, a, TIX, obs_type, resample, Rp, zp[0, TIX, a])
        what = (failure, obs_type, propagator, resample, m, a)
        # ---- status, sentinels
        assert np.array_equal(bad["status"], f64["status"]), (what, bad["status"], f64["status"])
        assert bad["status"][a] == CODE[failure] and np.count_nonzero(bad["status"]) == 1, (what, bad["status"])
        assert np.all(clean["status"] == 0), what
        n3 += int(np.sum(bad["status"] == 3))
        n4 += int(np.sum(bad["status"] == 4))
        assert np.array_equal(bad["x"][a], hip.host.X_FAILED) and np.array_equal(bad["P"][a], hip.host.P_FAILED), what
        # ---- the update record
        rec, crec = bad["upd"][0], clean["upd"][0]
        assert rec[L.UPD_ACTION] == a and rec[L.UPD_VISIBLE] == 1.0, (what, rec[[L.UPD_ACTION, L.UPD_VISIBLE]])
        assert crec[L.UPD_ACTION] == a and crec[L.UPD_OBS_TAKEN] == 1.0, what
        zt = slice(L.UPD_Z_TRUE, L.UPD_Z_TRUE + 3)
        assert uf.same_bits(rec[zt], crec[zt]), what                         # hx(x_true): recorded before anything can fail (:298)
        if failure == "nan":
            assert rec[L.UPD_OBS_TAKEN] == 1.0 and f64["obs_taken"], what    # booked, then filter_error (:305-311)
            # S and sigmas_h do not depend on the noise
            assert uf.same_bits(rec[L.UPD_S:L.UPD_S + 9], crec[L.UPD_S:L.UPD_S + 9]), what
            assert np.isfinite(rec[L.UPD_S:L.UPD_S + 9]).all()
            assert uf.same_bits(rec[L.UPD_SIGMAS_H:L.UPD_SIGMAS_H + 39], crec[L.UPD_SIGMAS_H:L.UPD_SIGMAS_H + 39]), what
            y, cy = rec[L.UPD_Y:L.UPD_Y + 3], crec[L.UPD_Y:L.UPD_Y + 3]
            assert tuple(np.where(np.isnan(y))[0]) == uf.Y_NAN[(obs_type, NAN_COMP)], (what, y)
            keep = ~np.isnan(y)
            assert uf.same_bits(y[keep], cy[keep]), (what, y, cy)
        else:
            # UPD_Y / UPD_S are not compared: the reference leaves y and S unwritten when inv(S) raises (:312), and so does the kernel
            assert rec[L.UPD_OBS_TAKEN] == 0.0 and not f64["obs_taken"], what
        # ---- nothing leaks into the tile's neighbours
        others = np.arange(m) != a
        for k in ("x_true", "x", "P", "obs", "status"):
            assert uf.same_bits(bad[k][others], clean[k][others]), (what, k)
        assert uf.same_bits(bad["metrics"][0][:, others], clean["metrics"][0][:, others]), what
        assert uf.same_bits(bad["x_true"][a], clean["x_true"][a]), what
        # ---- obs / metrics of the failed object: oracle.observe of the sentinel state (tolerances of tests/test_hip_ops.py's observe test)
        o_obs, o_met = oracle.observe(bad["x_true"][a:a + 1], bad["x"][a:a + 1], bad["P"][a:a + 1])
        assert np.array_equal(bad["obs"][a], o_obs[0]), what
        np.testing.assert_allclose(bad["metrics"][0][:, a], o_met[:, 0], rtol=1e-15)
        # ---- statistics
        dpos = bad["metrics"][0][0]
        st = bad["stats"]
        assert st[L.STAT_N_FAILED] == 1 and clean["stats"][L.STAT_N_FAILED] == 0, (what, st)
        assert st[L.STAT_MAX_DPOS] == np.max(dpos) and st[L.STAT_MAX_DPOS] > 1e19, (what, st)
        assert st[L.STAT_CNT_LT_1E4] == np.sum(dpos < 1e4) and st[L.STAT_CNT_LT_1E7] == np.sum(dpos < 1e7), (what, st)
        # ---- filter_error()'s record
        log = bad["fail_log"]
        assert log.shape[0] == 1 and clean["fail_log"].shape[0] == 0, (what, log)
        assert log[0, L.FAIL_ENV] == 0 and log[0, L.FAIL_OBJ] == a and log[0, L.FAIL_STATUS] == CODE[failure] and log[0, L.FAIL_TIME] == TIX, (what, log)
        # error_failed() of the step's inputs (:376-378): four to six roundings and a square root, the kernel may contract to fma
        want = uf.error_failed(xt[a], x[a], P[a])
        got = log[0, L.FAIL_ERR:L.FAIL_ERR + 4]
        assert np.all(np.abs(got - want) <= 16 * EPS * np.abs(want)), (what, got, want)
        # ---- a second step with the same action: the record cleared, the state passed through, nothing counted twice
        rec2 = bad2["upd"][0]
        assert rec2[L.UPD_ACTION] == -1.0 and rec2[L.UPD_OBS_TAKEN] == 0.0, (what, rec2[[L.UPD_ACTION, L.UPD_OBS_TAKEN]])
        assert bad2["status"][a] == CODE[failure] and np.count_nonzero(bad2["status"]) == 1, what
        assert uf.same_bits(bad2["x"][a], bad["x"][a]) and uf.same_bits(bad2["P"][a], bad["P"][a]), what
        assert bad2["fail_log"].shape[0] == 1 and uf.same_bits(bad2["fail_log"], log), what
        assert bad2["stats"][L.STAT_N_FAILED] == 1, (what, bad2["stats"])
        assert clean2["upd"][0][L.UPD_ACTION] == a and clean2["upd"][0][L.UPD_OBS_TAKEN] == 1.0, what
    assert (n3, n4) == ((len(PAIRS), 0) if failure == "nan" else (0, len(PAIRS)))


# ================================================================ B. every form of the step, bit-identical to A's form

SIZES = (12, 7)                      # 7: a ragged last tile, and no arg-max slots with several envs
# (status 3 words, status 4 words) at the end of the schedule.  NaN noise fails the object of step 2 and the last object (step 5); with
# R_OVERFLOW every visible scheduled object fails at its first update -- m = 12: objects 1, 4, 11, 0; m = 7: 1, 2, 6 (object 0 is hidden
# there) -- and the hidden ones stay at 0.
EXPECT = {(12, "nan"): (2, 0), (7, "nan"): (2, 0), (12, "linalg"): (0, 4), (7, "linalg"): (0, 3), (12, "clean"): (0, 0), (7, "clean"): (0, 0)}
_REF = {}


def _sched_inputs(m, failure, E=1, env=0):
    """(z_noise, R) of a schedule run: the clean table and the golden R, poisoned as `failure` says (NaN noise in env `env` only)"""
    _, _, _, g, sched = uf.schedule_batch(m)
    zn = np.tile(uf.noise_table(1, uf.N_TIME, m, seed=3), (E, 1, 1, 1))
    if failure == "nan":
        return uf.poison_schedule_nan(sched, e=env)(zn, g["R"])
    if failure == "linalg":
        return uf.poison_overflow(zn, g["R"])
    return zn, g["R"]


def _reference(hip, m, failure):
    """six launches of the generic three-launch form, computed once per (m, failure) and shared; checked for what the schedule is
    meant to do before anything is compared with it"""
    key = (m, failure)
    if key not in _REF:
        L = hip.lib
        ref = uf.run_schedule(hip, m, *_sched_inputs(m, failure), form="generic")
        assert ref["instances"] == {0}
        sched, st = ref["sched"], ref["status"]
        assert (int(np.sum(st == 3)), int(np.sum(st == 4))) == EXPECT[key], (key, st)
        assert not np.any((st == 1) | (st == 2)), (key, st)
        rec = [s["upd"][0] for s in ref["steps"]]
        assert rec[0][L.UPD_ACTION] == sched[0] and rec[0][L.UPD_VISIBLE] == 1
        assert rec[3][L.UPD_ACTION] == sched[3] and rec[3][L.UPD_VISIBLE] == 0 and rec[3][L.UPD_OBS_TAKEN] == 0 and st[sched[3]] == 0      # hidden
        assert rec[2][L.UPD_ACTION] == (sched[2] if failure == "clean" else -1)              # the same object again: failed, not attempted
        log = ref["fail_log"]
        if failure == "clean":
            assert log.shape[0] == 0 and all(r[L.UPD_OBS_TAKEN] == r[L.UPD_VISIBLE] for r in rec)
        elif failure == "nan":
            assert st[sched[1]] == 3 and st[sched[4]] == 3 and rec[0][L.UPD_OBS_TAKEN] == 1
            assert rec[1][L.UPD_OBS_TAKEN] == 1 and rec[4][L.UPD_OBS_TAKEN] == 1             # booked, then failed
            assert log[:, [L.FAIL_OBJ, L.FAIL_STATUS, L.FAIL_TIME]].tolist() == [[sched[1], 3, 2], [sched[4], 3, 5]], log
        else:
            vis = [k for k in range(uf.N_STEPS) if rec[k][L.UPD_VISIBLE] == 1]
            assert all(rec[k][L.UPD_OBS_TAKEN] == 0 for k in range(uf.N_STEPS))               # nothing is ever booked
            assert log[:, [L.FAIL_OBJ, L.FAIL_STATUS, L.FAIL_TIME]].tolist() == [[sched[k], 4, k + 1] for k in vis], log
            nf = [s["stats"][0, L.STAT_N_FAILED] for s in ref["steps"]]
            assert nf == list(np.cumsum([int(k in vis) for k in range(uf.N_STEPS)])), nf    # one more per visible scheduled object
        for k in np.where(st != 0)[0]:
            assert np.array_equal(ref["steps"][-1]["x"][k], hip.host.X_FAILED) and np.array_equal(ref["steps"][-1]["P"][k], hip.host.P_FAILED)
        _REF[key] = ref
    return _REF[key]


FAILURES = ("nan", "linalg", "clean")


@pytest.mark.parametrize("failure", FAILURES)
@pytest.mark.parametrize("m", SIZES)
def test_schedule_failures_are_local_to_the_failing_objects(hip, m, failure):
    """the reference run itself against its clean twin: objects that did not fail are bit-identical in every slot"""
    ref, clean = _reference(hip, m, failure), _reference(hip, m, "clean")
    ok = ref["status"] == 0
    for k, (a, b) in enumerate(zip(ref["steps"], clean["steps"])):
        for key in ("x_true", "x", "P", "obs"):
            assert uf.same_bits(a[key][ok], b[key][ok]), (m, failure, k + 1, key)
        assert uf.same_bits(a["metrics"][0][:, ok], b["metrics"][0][:, ok]), (m, failure, k + 1)
        assert uf.same_bits(a["x_true"], b["x_true"])


@pytest.mark.parametrize("form", ["fold_kernel", "deferred", "inside", "rollout"])
@pytest.mark.parametrize("failure", FAILURES)
@pytest.mark.parametrize("m,argmax", [(12, False), (12, True), (7, False)])      # (argmax_spos where m % 4 == 0)
def test_one_launch_forms_equal_the_three_launch_form(hip, m, argmax, failure, form):
    ref = _reference(hip, m, failure)
    got = uf.run_schedule(hip, m, *_sched_inputs(m, failure), form=form, argmax=argmax)
    st = got["status"]
    assert (int(np.sum(st == 3)), int(np.sum(st == 4))) == EXPECT[(m, failure)]
    uf.assert_same_schedule(hip.lib, ref, got, (m, failure, form, argmax), uf.STAT_COLS_ARGMAX if argmax else uf.STAT_COLS)


@pytest.mark.parametrize("failure", FAILURES)
@pytest.mark.parametrize("m", SIZES)
def test_plain_instance_and_forced_generic(hip, m, failure):
    ref = _reference(hip, m, failure)
    zn, R = _sched_inputs(m, failure)
    for generic, inst in ((False, {1}), (True, {0})):
        res = plain_step.run(hip, m, "hybrid", False, generic, z_noise=zn, R=R, actions=ref["sched"], plant=False)
        assert res["instances"] == inst, (m, failure, generic, res["instances"])      # the instance really taken (ssa_env_step_instance)
        got = uf.from_plain_step(hip, res)
        st = got["status"]
        assert (int(np.sum(st == 3)), int(np.sum(st == 4))) == EXPECT[(m, failure)]
        uf.assert_same_schedule(hip.lib, ref, got, (m, failure, "plain", generic))


@pytest.mark.parametrize("failure", FAILURES)
@pytest.mark.parametrize("m", SIZES)
def test_storage_layout_speaks_the_callers_indices(hip, m, failure):
    """set_layout with a permutation: failure records, UPD_ACTION and STAT_ARGMAX_SPOS carry the caller's indices, and every row read
    back in the caller's order is the row of the run without a layout"""
    ref = _reference(hip, m, failure)
    perm = np.random.RandomState(40 + m).permutation(m)
    assert not np.array_equal(perm, np.arange(m))
    # (one env: a layout goes with the launches that carry stat_shards and with the rollout -- include/ssa_hip.h, obj_ids -- so the
    # three-launch form has none; it is the reference, without a layout)
    for form, argmax in (("fold_kernel", m % 4 == 0), ("deferred", False), ("inside", False), ("rollout", m % 4 == 0)):
        got = uf.run_schedule(hip, m, *_sched_inputs(m, failure), form=form, argmax=argmax, layout=perm)
        st = got["status"]
        assert (int(np.sum(st == 3)), int(np.sum(st == 4))) == EXPECT[(m, failure)]
        cols = uf.STAT_COLS_ARGMAX if argmax else uf.STAT_COLS
        uf.assert_same_schedule(hip.lib, ref, got, (m, failure, form, "layout"), cols)


@pytest.mark.parametrize("inline", [False, True])
@pytest.mark.parametrize("failure", ["nan", "linalg"])
@pytest.mark.parametrize("m", SIZES)
def test_three_envs_the_failure_stays_in_its_env(hip, m, failure, inline):
    """E = 3 envs from one state.  NaN noise in env 1 only: envs 0 and 2 are their clean twins, env 1 the one-env NaN run, its failure
    records carry FAIL_ENV == 1.  R is the launch's (one ssa_consts for all envs): with R_OVERFLOW every env is the one-env overflow run."""
    L, E = hip.lib, 3
    got = uf.run_schedule_envs(hip, m, E, *_sched_inputs(m, failure, E=E, env=1), inline=inline)
    n3 = n4 = 0
    for e in range(E):
        kind = failure if (failure == "linalg" or e == 1) else "clean"
        ref = _reference(hip, m, kind)
        assert got[e]["instances"] == {0}
        log = got[e]["fail_log"].copy()
        assert log.shape[0] == ref["fail_log"].shape[0] and np.all(log[:, L.FAIL_ENV] == e), (e, log)
        log[:, L.FAIL_ENV] = 0.0
        uf.assert_same_schedule(L, ref, dict(got[e], fail_log=log), (m, failure, inline, "env", e))
        n3 += int(np.sum(got[e]["status"] == 3))
        n4 += int(np.sum(got[e]["status"] == 4))
    want = EXPECT[(m, failure)]
    assert (n3, n4) == (want[0], want[1] * E)


# ================================================================ C. sensor networks: a singular S is per sensor

SENSOR_FORMS = ("step", "rollout", "envs")


def _sensor_case(case):
    """(Rs, noise tables, actions, the run the untouched sensors are compared with: its Rs / tables / actions)"""
    _, _, _, g, _, Rs, zn = uf.sensor_inputs()
    if case.startswith("overflow"):                 # sensor 1's R overflows; every sensor on an object of its own
        acts = [4, 5, 6] if case == "overflow_one_tile" else [1, 6, 10]
        bad = [Rs[0], uf.R_OVERFLOW.copy(), Rs[2]]
        return bad, zn, acts, (bad, zn, [acts[0], -1, acts[2]])
    if case == "nan":                               # NaN in sensor 2's table row only
        acts = [4, 9, 6]
        z = zn.copy()
        z[2] = uf.nan_noise(zn[2][None], 0, 1, acts[2], 0)[0]
        assert np.isfinite(z[:2]).all() and np.isnan(z[2]).sum() == 1
        return Rs, z, acts, (Rs, z, [acts[0], acts[1], -1])
    if case == "shared_lower_overflows":            # sensors 0 and 1 on one object, the lower sensor's R overflows
        acts = [5, 5, 9]
        bad = [uf.R_OVERFLOW.copy(), Rs[1], Rs[2]]
        return bad, zn, acts, (bad, zn, [-1, -1, 9])
    if case == "shared_higher_overflows":           # ... the higher one's: the lower sensor updates, the overflowing R is never used
        acts = [5, 5, 9]
        bad = [Rs[0], uf.R_OVERFLOW.copy(), Rs[2]]
        return bad, zn, acts, (Rs, zn, [5, -1, 9])
    raise ValueError(case)


@pytest.mark.parametrize("case", ["overflow_one_tile", "overflow_three_tiles", "nan", "shared_lower_overflows", "shared_higher_overflows"])
def test_sensor_network_failure_is_the_failing_sensors_alone(hip, case):
    L = hip.lib
    Rs, zn, acts, (Rs0, zn0, acts0) = _sensor_case(case)
    got = uf.sensor_step(hip, Rs, zn, acts, "step")
    base = uf.sensor_step(hip, Rs0, zn0, acts0, "step")
    st, rec = got["status"], got["upd"]
    flags = lambda r: (r[L.UPD_ACTION], r[L.UPD_VISIBLE], r[L.UPD_OBS_TAKEN])      # noqa: E731
    assert np.all(base["status"] == 0) and base["fail_log"].shape[0] == 0
    if case == "shared_higher_overflows":
        # the object is the lower sensor's: updated with its R; sensor 1's record is cleared and its R never enters
        assert np.all(st == 0) and got["fail_log"].shape[0] == 0
        assert flags(rec[0]) == (5, 1, 1) and flags(rec[1]) == (-1, 0, 0) and flags(rec[2]) == (9, 1, 1)
        uf.assert_same_step(L, base, got, case)
        return
    s_bad = {"overflow_one_tile": 1, "overflow_three_tiles": 1, "nan": 2, "shared_lower_overflows": 0}[case]
    code = 3 if case == "nan" else 4
    j = acts[s_bad]
    assert st[j] == code and np.count_nonzero(st) == 1, (case, st)
    assert (int(np.sum(st == 3)), int(np.sum(st == 4))) == ((1, 0) if case == "nan" else (0, 1))
    assert np.array_equal(got["x"][j], hip.host.X_FAILED) and np.array_equal(got["P"][j], hip.host.P_FAILED)
    assert flags(rec[s_bad]) == (j, 1, 1 if case == "nan" else 0), (case, flags(rec[s_bad]))
    log = got["fail_log"]
    assert log.shape[0] == 1 and log[0, L.FAIL_OBJ] == j and log[0, L.FAIL_STATUS] == code and log[0, L.FAIL_TIME] == 1, log
    assert got["stats"][L.STAT_N_FAILED] == 1 and base["stats"][L.STAT_N_FAILED] == 0
    if case == "nan":      # booked: y is NaN where the noise is, S is the clean S of that sensor (the run with finite noise)
        clean = uf.sensor_step(hip, Rs, uf.sensor_inputs()[6], acts, "step")
        assert np.all(clean["status"] == 0)
        y = rec[2][L.UPD_Y:L.UPD_Y + 3]
        assert tuple(np.where(np.isnan(y))[0]) == uf.Y_NAN[('aer', 0)], y
        for sl in (slice(L.UPD_Z_TRUE, L.UPD_Z_TRUE + 3), slice(L.UPD_Y + 1, L.UPD_Y + 3), slice(L.UPD_S, L.UPD_VISIBLE)):
            assert uf.same_bits(rec[2][sl], clean["upd"][2][sl]), (case, sl)
    if case == "shared_lower_overflows":
        assert flags(rec[1]) == (-1, 0, 0), flags(rec[1])      # "a lower sensor's object": the higher sensor's record is cleared
    # everything the failing sensor did not touch: the run in which it idles
    others = np.arange(uf.SENSOR_M) != j
    keep = [s for s in range(uf.SENSOR_S) if acts0[s] >= 0]
    assert all(flags(rec[s]) == (acts[s], 1, 1) for s in keep), [flags(r) for r in rec]
    uf.assert_same_step(L, base, got, case, objects=others, records=keep)


@pytest.mark.parametrize("form", ["rollout", "envs"])
@pytest.mark.parametrize("case", ["overflow_one_tile", "overflow_three_tiles", "nan", "shared_lower_overflows", "shared_higher_overflows"])
def test_sensor_rollout_and_envs_equal_the_sensor_step(hip, case, form):
    """launch_rollout_sensors and launch_step_sensors_envs (E = 2) on the same inputs: bit-identical to the one-env launch_step_sensors"""
    Rs, zn, acts, _ = _sensor_case(case)
    want = uf.sensor_step(hip, Rs, zn, acts, "step")
    n_bad = 0 if case == "shared_higher_overflows" else 1
    assert np.count_nonzero(want["status"]) == n_bad and np.sum(want["status"] == (3 if case == "nan" else 4)) == n_bad
    got = uf.sensor_step(hip, Rs, zn, acts, form)
    for e, g_ in enumerate(got if form == "envs" else [got]):
        uf.assert_same_step(hip.lib, want, g_, (case, form, e))


# ================================================================ D. lookahead

def _i64(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("variant", ["aer", "xyz"])
def test_lookahead_foresees_the_singular_S(envs, variant):
    """R_OVERFLOW in the config: the lookahead says SSA_ST_UPDATE_LINALG for every object an update would reach, with the sentinel
    covariance the step leaves, and OK for the hidden ones -- against the step launched with every object in turn"""
    from ssa_gym_amd import host
    from support.lookahead import cfg1, check_against_step, xyz1
    over = dict(R=uf.R_OVERFLOW.copy()) if variant == "aer" else dict(xyz1(envs), R=uf.R_OVERFLOW.copy())
    env = envs.make(config=cfg1(envs, rso_count=64, seed=11, **over))
    st_in = env._engine.status.cpu().numpy().copy()
    assert not st_in.any()
    look, seen = check_against_step(env, n=64, seed=3)      # (64 objects sampled of 64: every one)
    vis, st = look["visible"] == 1, look["status"]
    assert vis.sum() >= 4 and (~vis).sum() >= 4, vis.sum()
    assert np.all(st[vis] == 4) and np.all(st[~vis] == 0), st           # the "singular S" group: every visible object, no hidden one
    assert (int(np.sum(st == 3)), int(np.sum(st == 4))) == (0, int(vis.sum()))
    assert seen["visible"] == vis.sum() and seen["hidden"] == (~vis).sum()
    assert np.array_equal(_i64(look["P_post"][vis]), _i64(np.broadcast_to(host.P_FAILED, (vis.sum(), 6, 6))))
    assert np.isnan(look["score"][:, vis]).all()
    # a filter the step has failed: the env's next lookahead passes it through as failed at entry
    a = int(np.where(vis)[0][0])
    env.step(a)
    assert env._engine.status.cpu().numpy()[a] == 4 and env.failed_filters_id == [a] and not env.obs_taken[1]


def test_lookahead_sensors_singular_S_in_one_sensors_slice(envs):
    """only sensor 1's R overflows (its z_sigma squared): status 4 in that sensor's slice of lookahead_sensors() and in no other, and the
    sensor step with that sensor alone on the object leaves the same status and covariance"""
    from ssa_gym_amd import host
    from support.sensors import _Relaunch, cfg3
    # (the third site sees none of these 64 objects above cfg3's 20 degree mask: it gets none)
    cfg = cfg3(envs, m=64, sensors=3, sensor_z_sigma=[(1, 1, 1e3), (1e60, 1e60, 1e52), (0.5, 0.5, 2e3)], sensor_obs_limit=[15, 10, -90])
    env = envs.make('ssa_tasker_simple-v2', config=cfg)
    with np.errstate(over='ignore'):
        assert np.isinf(np.prod(np.diag(env.sensor_R[1]))) and np.isfinite(env.sensor_R).all()
    r = env.lookahead_sensors(covariances=True)
    import torch
    torch.cuda.synchronize()
    net = {k: v.cpu().numpy().copy() for k, v in r.items()}
    vis, st = net["visible"] == 1, net["status"]
    assert all(vis[s].sum() >= 2 for s in range(3)) and (~vis[1]).sum() >= 2, vis.sum(axis=1)
    assert np.all(st[1][vis[1]] == 4) and np.all(st[1][~vis[1]] == 0)
    assert not st[0].any() and not st[2].any()
    assert (int(np.sum(st == 3)), int(np.sum(st == 4))) == (0, int(vis[1].sum()))
    assert np.array_equal(_i64(net["P_post"][1][vis[1]]), _i64(np.broadcast_to(host.P_FAILED, (vis[1].sum(), 6, 6))))
    L = __import__("ssa_gym_amd")._lib
    rl = _Relaunch(env)
    for s in range(3):
        for j in np.where(vis[s])[0][:3]:
            acts = [-1] * 3
            acts[s] = int(j)
            got = rl.sensors(acts)
            assert got["st"][j] == st[s, j] == (4 if s == 1 else 0), (s, j, got["st"][j])
            assert np.array_equal(got["P"][j], _i64(net["P_post"][s, j]).reshape(36)), (s, j)
            assert got["upd"][s][L.UPD_OBS_TAKEN] == (0.0 if s == 1 else 1.0) and got["upd"][s][L.UPD_VISIBLE] == 1.0


# ================================================================ E. the gym surface

def _gym_env(envs, **over):
    cfg = dict(envs.env_config)
    cfg.update(rso_count=20, steps=48, reward_type='trinary', obs_returned='flatten', seed=0, obs_limit=-90)
    cfg.update(over)
    env = envs.make('ssa_tasker_simple-v2', config=cfg)
    env.reset()
    return env


def _message(env, a, i, kind):
    """the reference's filter_error message (ssa_tasker_simple_2.py:375-378): error_failed of slot i - 1, rounded to two decimals"""
    from ssa_gym_amd.envs.results import error_failed
    err = error_failed(state=np.asarray(env.x_true[i - 1])[a], x=np.asarray(env.x_filter[i - 1])[a], P=np.diag(np.asarray(env.P_filter[i - 1])[a]))
    return "".join(['Object ', str(a), ' failed on update step ', str(i), kind, str(np.round(err, 2))])


def test_gym_step_reports_update_nan(envs):
    env = _gym_env(envs)
    env.step(0)
    env.step(3)
    a, i = 7, env.i + 1
    zn = env._engine.z_noise
    assert zn.numel() == env.n * env.m * 3
    zn.view(env.n, env.m, 3)[i, a, 2] = float("nan")      # the noise of the next step's action
    env.step(a)
    assert env.i == i and env.failed_filters_id == [a]
    assert bool(env.obs_taken[i]) is True                  # booked before filter_error (:305)
    assert env.failed_filters_msg[a] == [_message(env, a, i, ', update returned nan. ')]
    st = env._engine.status.cpu().numpy()
    assert (int(np.sum(st == 3)), int(np.sum(st == 4))) == (1, 0) and st[a] == 3
    assert np.array_equal(np.asarray(env.x_filter[i])[a], __import__("ssa_gym_amd").host.X_FAILED)


def test_gym_step_reports_update_linalg(envs):
    env = _gym_env(envs, R=uf.R_OVERFLOW.copy())
    a, i = 7, 1
    env.step(a)
    assert env.i == i and env.failed_filters_id == [a]
    assert bool(env.obs_taken[i]) is False                 # nothing is booked (:310-311)
    assert env.failed_filters_msg[a] == [_message(env, a, i, ', LinAlgError. ')]
    st = env._engine.status.cpu().numpy()
    assert (int(np.sum(st == 3)), int(np.sum(st == 4))) == (0, 1) and st[a] == 4
