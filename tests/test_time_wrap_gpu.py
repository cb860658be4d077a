"""The time row every fused kernel reads once the index wraps (include/ssa_hip.h: "index = i % n_time"), pinned to a table that never
wraps (tests/support/time_wrap.py): every entry runs on a SHORT engine of T = 16 rows, where the index wraps, and on a LONG engine
whose trans, z_noise, Sun and site tables have 4 T rows chosen by numpy (long[r] = short[r % T]), where it does not -- the same consts,
state, actions, sensor block and launch arguments, so everything the launch leaves is the same bits.  The control of every
comparison: the long tables with ONE table's rows from T on shifted by one -- the result must differ, for every table the entry reads.
Two absolute anchors at wrapped indices, on the CPU oracle and numpy at row tix % T of the short tables: z_true and the aer_out payload
(oracle.hx_aer, the bounds of tests/test_sensors_oracle_gpu.py), and the visibility words (support.illumination.expected_visible,
support.orbiting's line of sight).  Indices T - 1, T, T + 1, 2 T, 3 T + 5; time words [T - 2, T + 3, 3 T - 1] and [T - 1, 2 T + 1]; 8
objects and a ragged 7.  The scenes' margins and non-vacuity are asserted here and, on the CPU, in tests/test_time_wrap_host.py.
Negative indices are out of scope: the fused entries require i >= 0."""
import numpy as np
import pytest

from support import illumination as il
from support import time_wrap as tw
from support.gpu import hip  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

T = tw.T
PLAIN = ("trans", "z_noise")                 # what an entry without a network reads
GEOMETRY = ("trans", "sun", "site_rows")     # ... a lookahead, a forecast, a dry run of a network: no measurement is drawn
SEVERAL = [tw.WORDS3, tw.WORDS2]


def case(oracle, oracle_ld, kind, m, words, K=1, reads=tw.TABLES):
    """(scene, the tables of `reads` its network has -- none where no index of the case wraps: a control cannot differ there)"""
    sc = tw.scene(oracle, oracle_ld, kind, m, len(words), tw.phase_of(words, K))
    wrapped = sc.check(words, K)
    return sc, tuple(t for t in reads if t in sc.tables()) if wrapped else ()


def want_visible(sc, words, k=0):
    """[E, S, m] of numpy's: env e's truth at step k under row (words[e] + k) % T of the short tables"""
    return np.array([sc.visible(k, (int(w) + k) % T)[0][:, sc.src] for w in words])


# ---------------------------------------------------------------------------------------------------------------- 1. ssa_env_step_f64
@pytest.mark.parametrize("tix", tw.SINGLE)
@pytest.mark.parametrize("m", [8, 7])
@pytest.mark.parametrize("propagator", ["hybrid", "fg"])
def test_step(hip, oracle, oracle_ld, propagator, m, tix):
    """one env: the action by pointer (payload of 4 columns), by action= (the trace only) and by env_words= (no payload), and the
    two-launch statistics path, whose post kernel forms the payload with its own %.  An update is taken at every index; at the wrapped
    ones z_true and the payload are the oracle's at row tix % T"""
    L = hip.lib
    sc, tables = case(oracle, oracle_ld, "moving", m, (tix,), reads=PLAIN)
    got = {}
    for delivery, aer, two in (("ptr", 4, False), ("inline", 1, False), ("words", 0, False), ("ptr", 4, True)):
        def run(tabs):
            return tw.run_step(hip, sc, tabs, (tix,), propagator, delivery, aer, two)
        r = got[(delivery, two)] = tw.pin(run, sc, tables, ("step", propagator, m, tix, delivery, aer, two))
        rec = r["upd_ring"][1, 0]
        assert rec[L.UPD_OBS_TAKEN] == 1.0 and rec[L.UPD_ACTION] == 0.0 and not r["status"].any() and r["fail_count"][0] == 0
        tw.anchor_z_true(sc, oracle, rec, r["x_true"][1, 0], tix, L)
        if aer == 4:
            tw.anchor_aer(sc, oracle, oracle_ld, r["aer"].reshape(m, 4), r["x_filter"][1], tix)
    keys = ("x_true", "x_filter", "P_filter", "obs", "metrics", "status", "upd_ring")
    for k in (("inline", False), ("words", False), ("ptr", True)):
        il.same_bits(got[("ptr", False)], got[k], ("deliveries", k), keys=keys)
    il.same_bits(got[("ptr", False)], got[("ptr", True)], "payload of the epilogue and of the post kernel", keys=("aer",))


@pytest.mark.parametrize("delivery", ["ptr", "words"])
@pytest.mark.parametrize("words", SEVERAL)
@pytest.mark.parametrize("propagator", ["hybrid", "fg"])
def test_step_of_several_envs(hip, oracle, oracle_ld, propagator, words, delivery):
    """in one launch an env below the table's end and envs wrapped differently: every env's update, z_true and payload at its own row"""
    L = hip.lib
    sc, tables = case(oracle, oracle_ld, "moving", 8, words, reads=PLAIN)
    r = tw.pin(lambda tabs: tw.run_step(hip, sc, tabs, words, propagator, delivery, aer=4), sc, tables, ("step", propagator, words, delivery))
    aer = r["aer"].reshape(len(words), 8, 4)
    for e, w in enumerate(words):
        rec = r["upd_ring"][1, e]
        assert rec[L.UPD_OBS_TAKEN] == 1.0 and rec[L.UPD_ACTION] == 0.0
        tw.anchor_z_true(sc, oracle, rec, r["x_true"][1, 8 * e], w, L)
        tw.anchor_aer(sc, oracle, oracle_ld, aer[e], r["x_filter"][1, 8 * e:8 * e + 8], w)


def test_steps_whose_wavefronts_walk_tiles_of_two_envs(hip, oracle, oracle_ld):
    """2 x 10 244 objects, time words [T - 1, 2 T + 1]: the grid-stride instance, wavefront 0 walks the tile env 0 tasks and the tile env 1
    tasks -- the row is read again per tile.  The plain step and the network's (site_moving = 0b110: the first lane's row)"""
    L = hip.lib
    m, words = tw.M_TILES, tw.WORDS2
    sc, tables = case(oracle, oracle_ld, "moving", m, words)
    r = tw.pin(lambda tabs: tw.run_step(hip, sc, tabs, words), sc, PLAIN, ("step", m))
    for e, w in enumerate(words):
        rec = r["upd_ring"][1, e]
        assert rec[L.UPD_OBS_TAKEN] == 1.0 and rec[L.UPD_ACTION] == sc.acts[e, 0]
        tw.anchor_z_true(sc, oracle, rec, r["x_true"][1, e * m + sc.acts[e, 0]], w, L)
    r = tw.pin(lambda tabs: tw.run_step_sensors(hip, sc, tabs, words, entry="envs"), sc, tables, ("sensor step", m))
    want = want_visible(sc, words)
    for e in range(2):
        cells = [float(want[e, s, sc.acts[e, s]]) for s in range(3)]
        assert r["upd"][e, :, L.UPD_VISIBLE].tolist() == cells and r["upd"][e, :, L.UPD_OBS_TAKEN].tolist() == cells, (e, cells)


# ---------------------------------------------------------------------------------------------------------------- 2. ssa_env_rollout_f64
@pytest.mark.parametrize("m", [8, 7])
@pytest.mark.parametrize("propagator", ["hybrid", "fg"])
def test_rollout_across_the_wrap(hip, oracle, oracle_ld, propagator, m):
    """K = 5 from T - 2: the wrap falls inside the launch; every step's ring slot and record (history 6: all of them survive)"""
    L = hip.lib
    sc, tables = case(oracle, oracle_ld, "moving", m, (T - 2,), K=5, reads=PLAIN)
    r = tw.pin(lambda tabs: tw.run_rollout(hip, sc, tabs, (T - 2,), 5, propagator), sc, tables, ("rollout", propagator, m))
    taken = r["upd_ring"][1:6, 0, L.UPD_OBS_TAKEN].tolist()
    assert taken == [1.0, 0.0, 1.0, 0.0, 1.0] and not r["status"].any(), taken      # (time indices T and T + 2 update)
    tw.anchor_z_true(sc, oracle, r["upd_ring"][3, 0], r["x_true"][3, 0], T, L)
    tw.anchor_z_true(sc, oracle, r["upd_ring"][5, 0], r["x_true"][5, 0], T + 2, L)


@pytest.mark.parametrize("words", SEVERAL)
def test_rollout_of_several_envs(hip, oracle, oracle_ld, words):
    sc, tables = case(oracle, oracle_ld, "moving", 8, words, K=4, reads=PLAIN)
    r = tw.pin(lambda tabs: tw.run_rollout(hip, sc, tabs, words, 4), sc, tables, ("rollout", words))
    assert (r["upd_ring"][[1, 3], :, hip.lib.UPD_OBS_TAKEN] == 1.0).all()


# ---------------------------------------------------------------------------------------------------------------- 3. ssa_lookahead_f64
@pytest.mark.parametrize("m", [8, 7])
def test_lookahead(hip, oracle, oracle_ld, m):
    """at T + 1; its visibility is the ground radar's at row 1"""
    sc, tables = case(oracle, oracle_ld, "moving", m, (T + 1,), reads=("trans",))
    r = tw.pin(lambda tabs: tw.run_lookahead(hip, sc, tabs, (T + 1,)), sc, tables, ("lookahead", m))
    assert np.array_equal(r["visible"].astype(bool), want_visible(sc, (T + 1,))[0, 0]) and r["visible"].all() and not r["status"].any()


@pytest.mark.parametrize("by_value", [False, True])
@pytest.mark.parametrize("words", SEVERAL)
def test_lookahead_of_several_envs(hip, oracle, oracle_ld, words, by_value):
    sc, tables = case(oracle, oracle_ld, "moving", 8, words, reads=("trans",))
    r = tw.pin(lambda tabs: tw.run_lookahead(hip, sc, tabs, words, by_value=by_value), sc, tables, ("lookahead", words, by_value))
    assert r["visible"].all() and not np.isnan(r["score"]).any()


# ---------------------------------------------------------------------------------------------------------------- 4. ssa_env_closed_loop_f64
@pytest.mark.parametrize("persistent", [True, False])
@pytest.mark.parametrize("m", [8, 7])
def test_closed_loop_across_the_wrap(hip, oracle, oracle_ld, m, persistent):
    """one greedy agent from the state of step T - 2: the steps T - 1 .. T + 2 and their decisions in ONE persistent launch, and as step +
    decision launches.  The agent's visibility mask reads the row through the closed loop's own expression (the per-step form: through
    the decision kernel's %): object 3 stands on the radar's mask and has the largest covariance -- below the mask at the decisions of
    rows T - 2 and T - 1, above it at step T under row 0 and below it under row 1 -- so the decision after step T is object 3, and with
    the trans rows shifted it is not"""
    L = hip.lib
    sc = tw.scene(oracle, oracle_ld, "moving", m, 1, 0, edge=True)
    tw.check_edge(sc)

    def run(tabs):
        return tw.run_closed_loop(hip, sc, tabs, tw.LOOP_I0, 4, persistent)
    r = tw.pin(run, sc, PLAIN, ("closed loop", m, persistent))
    log = r["log"].tolist()
    assert min(log[:4]) >= 0 and not r["status"].any()
    assert log[0] != tw.EDGE and log[1] != tw.EDGE and log[2] == tw.EDGE, log
    rec = r["upd"] if persistent else r["upd_ring"][[(T - 1 + k) % tw.H for k in range(4)], 0]
    assert (rec[:, L.UPD_OBS_TAKEN] == 1.0).all() and rec[:, L.UPD_ACTION].tolist() == log[:4]
    tw.anchor_z_true(sc, oracle, rec[1], r["x_true"][T % tw.H, log[1]], T, L)
    wrong = run(tw.variant(sc.tabs, "trans"))["log"].tolist()
    assert wrong[:2] == log[:2] and wrong[2] != tw.EDGE, (log, wrong)


# ---------------------------------------------------------------------------------------------------------------- 5. a network
def _cells(sc, want, e=0):
    """the tasked cells (sensor s, its object) of env e of a visibility table [E, S, m], as the update records show them"""
    return [float(want[e, s, sc.acts[e, s]]) for s in range(3)]


@pytest.mark.parametrize("tix", tw.SINGLE)
@pytest.mark.parametrize("m", [8, 7])
@pytest.mark.parametrize("kind,propagator", [("moving", "hybrid"), ("moving", "fg"), ("ground", "hybrid")])
def test_sensor_step(hip, oracle, oracle_ld, kind, propagator, m, tix):
    """ssa_env_step_sensors_f64 (and, m % 4 == 0, ssa_env_step_sensors_envs_f64 of one env) with per-sensor noise tables, an 'ae' sensor
    and the Sun table; 'moving': sensors 1 and 2 from site_rows.  The records' visibility words are numpy's at row tix % T --
    'ground': support.illumination.expected_visible (sunlit object, dark site), 'moving': the line of sight and the sunlit rule --
    and sensor 0's z_true the oracle's"""
    L = hip.lib
    sc, tables = case(oracle, oracle_ld, kind, m, (tix,))
    assert int(sc.net.ang.sum()) == 1 and tw.strides(sc.tabs)["sensor"] != 0
    want = _cells(sc, want_visible(sc, (tix,)))
    assert want[0] == 1.0 and (tix < T or want == [1.0, 1.0, 1.0])      # (the right row of a wrapped index shows every cell)
    for entry in ("sensors",) + (("envs",) if m % 4 == 0 else ()):
        r = tw.pin(lambda tabs: tw.run_step_sensors(hip, sc, tabs, (tix,), propagator, entry), sc, tables, (entry, kind, propagator, m, tix))
        upd = r["upd"][0]
        assert upd[:, L.UPD_VISIBLE].tolist() == want and upd[:, L.UPD_OBS_TAKEN].tolist() == want, (entry, upd[:, :2], want)
        assert upd[:, L.UPD_ACTION].tolist() == [0.0, 1.0, 2.0] and not r["status"].any()
        tw.anchor_z_true(sc, oracle, upd[0], r["x_true"][1, 0], tix, L)


@pytest.mark.parametrize("by_value", [False, True])
@pytest.mark.parametrize("words", SEVERAL)
@pytest.mark.parametrize("kind", ["moving", "ground"])
def test_sensor_step_of_several_envs(hip, oracle, oracle_ld, kind, words, by_value):
    """ssa_env_step_sensors_envs_f64: the rows and time words through device memory and by value; every env's records at its own row"""
    L = hip.lib
    sc, tables = case(oracle, oracle_ld, kind, 8, words)
    r = tw.pin(lambda tabs: tw.run_step_sensors(hip, sc, tabs, words, entry="envs", by_value=by_value), sc, tables, (kind, words, by_value))
    want = want_visible(sc, words)
    for e, w in enumerate(words):
        cells = _cells(sc, want, e)
        assert r["upd"][e, :, L.UPD_VISIBLE].tolist() == cells and r["upd"][e, :, L.UPD_OBS_TAKEN].tolist() == cells, (e, cells)
        tw.anchor_z_true(sc, oracle, r["upd"][e, 0], r["x_true"][1, 8 * e], w, L)


@pytest.mark.parametrize("tix", tw.SINGLE)
@pytest.mark.parametrize("m", [8, 7])
def test_sensor_lookahead(hip, oracle, oracle_ld, m, tix):
    """ssa_lookahead_sensors_f64 (and ssa_lookahead_sensors_envs_f64 of one env): the whole [S, m] visibility table is numpy's at row
    tix % T, NaN scores exactly in the other cells"""
    sc, tables = case(oracle, oracle_ld, "moving", m, (tix,), reads=GEOMETRY)
    want = want_visible(sc, (tix,))[0]
    for entry in ("sensors",) + (("envs",) if m % 4 == 0 else ()):
        r = tw.pin(lambda tabs: tw.run_lookahead(hip, sc, tabs, (tix,), entry), sc, tables, ("lookahead", entry, m, tix))
        vis = r["visible"].astype(bool).reshape(3, m)
        assert np.array_equal(vis, want), np.argwhere(vis != want).tolist()
        assert np.array_equal(np.isnan(r["score"][..., 0]).reshape(3, m), ~want) and not r["status"].any()


@pytest.mark.parametrize("by_value", [False, True])
@pytest.mark.parametrize("words", SEVERAL)
def test_sensor_lookahead_and_forecast_of_several_envs(hip, oracle, oracle_ld, words, by_value):
    """ssa_lookahead_sensors_envs_f64 at the words, ssa_forecast_sensors_envs_f64 with H = 4 from them: each env's visibility tables at
    its own rows, step by step"""
    sc, tables = case(oracle, oracle_ld, "moving", 8, words, K=4, reads=GEOMETRY)
    r = tw.pin(lambda tabs: tw.run_lookahead(hip, sc, tabs, words, "envs", by_value), sc, tables, ("lookahead", words, by_value))
    assert np.array_equal(r["visible"].astype(bool), want_visible(sc, words))
    r = tw.pin(lambda tabs: tw.run_lookahead(hip, sc, tabs, words, "envs", by_value, n_steps=4), sc, tables, ("forecast", words, by_value))
    for h in range(4):
        assert np.array_equal(r["visible"][h].astype(bool), want_visible(sc, words, h)), h


@pytest.mark.parametrize("m", [8, 7])
def test_sensor_forecast_across_the_wrap(hip, oracle, oracle_ld, m):
    """ssa_forecast_sensors_f64 (and the envs entry of one env), H = 4 from T - 2: steps T and T + 1 read rows 0 and 1"""
    sc, tables = case(oracle, oracle_ld, "moving", m, (T - 2,), K=4, reads=GEOMETRY)
    for entry in ("sensors",) + (("envs",) if m % 4 == 0 else ()):
        r = tw.pin(lambda tabs: tw.run_lookahead(hip, sc, tabs, (T - 2,), entry, n_steps=4), sc, tables, ("forecast", entry, m))
        for h in range(4):
            vis = r["visible"][h].astype(bool).reshape(3, m)
            assert np.array_equal(vis, want_visible(sc, (T - 2,), h)[0]), h
        assert len({r["visible"][h].tobytes() for h in range(4)}) > 1


@pytest.mark.parametrize("m", [8, 7])
def test_sensor_rollout_across_the_wrap(hip, oracle, oracle_ld, m):
    """ssa_env_rollout_sensors_f64 (and the envs entry of one env), K = 4 from T - 2: every step's slot and records"""
    L = hip.lib
    sc, tables = case(oracle, oracle_ld, "moving", m, (T - 2,), K=4)
    sched = tw.schedule(sc, 4)
    for entry in ("sensors",) + (("envs",) if m % 4 == 0 else ()):
        r = tw.pin(lambda tabs: tw.run_rollout_sensors(hip, sc, tabs, (T - 2,), 4, entry), sc, tables, ("rollout", entry, m))
        rec = r["upd_sensors"][1:5] if entry == "sensors" else r["upd"][:, 0]
        for k in range(4):
            want = want_visible(sc, (T - 2,), k)[0]
            cells = [float(j >= 0 and want[s, j]) for s, j in enumerate(sched[k, 0])]
            assert rec[k, :, L.UPD_OBS_TAKEN].tolist() == cells, (entry, k, cells)
        assert not r["status"].any()


@pytest.mark.parametrize("words", SEVERAL)
def test_sensor_rollout_of_several_envs(hip, oracle, oracle_ld, words):
    """ssa_env_rollout_sensors_envs_f64, K = 4 from the words"""
    L = hip.lib
    sc, tables = case(oracle, oracle_ld, "moving", 8, words, K=4)
    sched = tw.schedule(sc, 4)
    r = tw.pin(lambda tabs: tw.run_rollout_sensors(hip, sc, tabs, words, 4, "envs"), sc, tables, ("rollout", words))
    for k in range(4):
        want = want_visible(sc, words, k)
        for e in range(len(words)):
            cells = [float(j >= 0 and want[e, s, j]) for s, j in enumerate(sched[k, e])]
            assert r["upd"][k, e, :, L.UPD_OBS_TAKEN].tolist() == cells, (k, e, cells)


@pytest.mark.parametrize("form", ["gather", "full"])
@pytest.mark.parametrize("m", [8, 7])
def test_dry_run_across_the_wrap(hip, oracle, oracle_ld, m, form):
    """ssa_dryrun_sensors_envs_f64 from the engine's one-env call, K = 4 from T - 2, with the gathered block (two candidates) and on the
    slot itself (one)"""
    sc, tables = case(oracle, oracle_ld, "moving", m, (T - 2,), K=4, reads=GEOMETRY)
    r = tw.pin(lambda tabs: tw.run_dryrun(hip, sc, tabs, (T - 2,), 4, form), sc, tables, ("dry run", m, form))
    cand = tw.candidates(sc, 4)[0]
    for b in range(r["visible"].shape[0]):
        for k in range(4):
            want = want_visible(sc, (T - 2,), k)[0]
            cells = [int(j >= 0 and want[s, j]) for s, j in enumerate(cand[b, k])]
            assert r["visible"][b, k].tolist() == cells and r["taken"][b, k].tolist() == cells, (b, k, cells)


@pytest.mark.parametrize("form", ["envs", "envs_by_value"])
@pytest.mark.parametrize("words", SEVERAL)
def test_dry_run_of_several_envs(hip, oracle, oracle_ld, words, form):
    """launch_dryrun_sensors_envs with per-env time words: ssa_dryrun_gather_f64 hands each pseudo-env its env's word"""
    sc, tables = case(oracle, oracle_ld, "moving", 8, words, K=4, reads=GEOMETRY)
    r = tw.pin(lambda tabs: tw.run_dryrun(hip, sc, tabs, words, 4, form), sc, tables, ("dry run", words, form))
    cand = tw.candidates(sc, 4)
    for e in range(len(words)):
        for b in range(2):
            for k in range(4):
                want = want_visible(sc, words, k)[e]
                cells = [int(j >= 0 and want[s, j]) for s, j in enumerate(cand[e, b, k])]
                assert r["visible"][e, b, k].tolist() == cells, (e, b, k, cells)


@pytest.mark.parametrize("words", SEVERAL)
def test_decision_chain(hip, oracle, oracle_ld, words):
    """step_agent's chain at the wrapped words: lookahead, ssa_assign_sensors_envs_f64 into the action table, and the step that reads
    table and time words from device memory.  Every tasked cell is one numpy calls visible at the env's own row, and is observed"""
    L = hip.lib
    sc, tables = case(oracle, oracle_ld, "moving", 8, words)
    r = tw.pin(lambda tabs: tw.run_chain(hip, sc, tabs, words), sc, tables, ("chain", words))
    want = want_visible(sc, words)
    assert np.array_equal(r["visible"].astype(bool), want)
    for e in range(len(words)):
        acts = r["table"][e, :3].tolist()
        assert acts[0] >= 0 and all(want[e, s, j] for s, j in enumerate(acts) if j >= 0), (e, acts)
        assert r["upd"][e, :, L.UPD_OBS_TAKEN].tolist() == [float(j >= 0) for j in acts], (e, acts)


# ---------------------------------------------------------------------------------------------------------------- 6. update_interval
@pytest.mark.parametrize("tix", [T + 1, T + 2, 2 * T + 1])
@pytest.mark.parametrize("m", [8, 7])
def test_update_interval_is_tested_on_the_unwrapped_index(hip, oracle, oracle_ld, m, tix):
    """update_interval = 3, which does not divide T = 16: 18 and 33 update, 17 does not -- whatever 17 % 16, 18 % 16 and 33 % 16 are"""
    L = hip.lib
    due = tix % 3 == 0
    assert [t % 3 == 0 for t in (T + 1, T + 2, 2 * T + 1)] == [False, True, True] and (tix % T) % 3 != 0
    sc, tables = case(oracle, oracle_ld, "moving", m, (tix,))
    if not due:
        tables = ()      # (nothing is read at a skipped step: no table's row can matter)
    r = tw.pin(lambda tabs: tw.run_step(hip, sc, tabs, (tix,), interval=3), sc, tuple(t for t in tables if t in PLAIN), ("interval", m, tix))
    assert (r["upd_ring"][1, 0, L.UPD_ACTION] >= 0) == due and r["upd_ring"][1, 0, L.UPD_OBS_TAKEN] == float(due)
    r = tw.pin(lambda tabs: tw.run_step_sensors(hip, sc, tabs, (tix,), interval=3), sc, tables, ("interval, sensors", m, tix))
    assert ((r["upd"][0, :, L.UPD_ACTION] >= 0) == due).all() and (r["upd"][0, :, L.UPD_OBS_TAKEN] == float(due)).all()
