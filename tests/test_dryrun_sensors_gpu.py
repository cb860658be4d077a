"""The dry run of B candidate tasking schedules in one launch (include/ssa_hip.h: ssa_dryrun_sensors_envs_f64;
HotPathEngine.launch_dryrun_sensors; SSA_Tasker_Env.evaluate_schedules; agents.refine_plan_sensors) on the MI355X.

Two yardsticks, both made of launches this feature leaves untouched.  A schedule that names every object at most once is valued by the
forecast: slot (k, s) equals entry (k, s, a[k, s]) of launch_forecast_sensors.  A schedule with revisits is valued by the step-by-step
chain: the network's lookahead with covariances, an all-idle step, and P_post written into the next slot for every slot taken
(support.dryrun.step_chain).  Everything is compared bit for bit; there is no tolerance anywhere.  Shapes: 403 objects (a ragged last
tile in the full-catalogue form), three sites that share passes, K = 5, launched at step 2."""
import numpy as np
import pytest

from support.dryrun import (BAD, FAILED, KEYS, WARM, forecast_entries, make_case, record_bits, result_bits, same_result, slot_total,
                            step_chain)
from support.gpu import envs, hip  # noqa: F401  (the module fixtures)
from support.sensors import _assert_same_env, _distinct, cfg8
from support.vector_forecast import state_bytes

pytestmark = pytest.mark.gpu
M, K, S = 403, 5, 3


def _read(hip, r):
    hip.torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in r.items()}


def _both_forms(eng, sp, slot, t0, cand):
    """the records of one candidate from the gathered launch and from the full-catalogue one"""
    a = record_bits(eng.launch_dryrun_sensors(slot, t0, sp, cand[None]))
    b = record_bits(eng.launch_dryrun_sensors(slot, t0, sp, cand[None], gather=False))
    assert not a["spare"].any() and not b["spare"].any()
    return a, b


def _once_schedule(fc, m, Kk, specials=True):
    """a schedule [K, S] whose valid entries name each object at most once: per slot the first unused healthy object the forecast shows
    visible there (else the first unused one), with -- specials -- FAILED, BAD (tasked at k = 1: it fails in the predict of k = 0), an
    idle and an out-of-range entry in fixed slots"""
    sched = np.full((Kk, S), -1, dtype=np.int64)
    fixed = {(0, 1): FAILED, (1, 2): BAD, (2, 0): -1, (Kk - 1, 1): m + 5} if specials else {}
    used = {FAILED, BAD}
    for k in range(Kk):
        for s in range(S):
            if (k, s) in fixed:
                sched[k, s] = fixed[(k, s)]
                continue
            vis = [j for j in np.flatnonzero(~np.isnan(fc["score"][k, s, :, 0])) if j not in used]
            j = int(vis[0]) if vis else min(set(range(m)) - used)
            sched[k, s] = j
            used.add(j)
    return sched


def _once_case(hip, Kk=K, m=M, **kw):
    eng, sp, slot, t0, _ = make_case(hip, m=m, **kw)
    interval = int(eng.consts.update_interval)
    fc = _read(hip, eng.launch_forecast_sensors(slot, t0, sp, Kk))
    sched = _once_schedule(fc, m, Kk)
    want = forecast_entries(fc, sched, m, t0, interval)
    before = state_bytes(hip.torch, eng)
    gathered, full = _both_forms(eng, sp, slot, t0, sched)
    after = state_bytes(hip.torch, eng)
    assert before.keys() == after.keys() and all(before[k] == after[k] for k in before), "the dry run wrote the engine's state"
    print("[dry run m=%d K=%d %s] schedule %s taken %s status %s" % (m, Kk, kw, sched.tolist(), want["taken"][0].tolist(), want["status"][0].tolist()))
    assert want["taken"].sum() >= 3, "the schedule takes too few observations to show anything"
    same_result(gathered, want, "gathered against the forecast")
    same_result(full, want, "full catalogue against the forecast")
    return want, sched


def test_once_per_object_schedule_equals_the_forecast(hip):
    """every slot of a candidate that names each object at most once is the forecast's entry (k, s, a[k, s]) -- scores, status,
    visibility, taken -- in the gathered form and in the full-catalogue one; the engine's tensors are byte-identical around the calls.
    Among the slots: a filter failed before the launch (ACTION -1, its status), a NaN filter tasked one step after its predict failed,
    an idle and an out-of-range entry (the cleared record)."""
    from ssa_gym_amd import _lib as L
    want, sched = _once_case(hip)
    assert want["status"][0, 0, 1] == L.ST_UPDATE_NAN and want["action"][0, 0, 1] == -1          # FAILED
    assert want["status"][0, 1, 2] == L.ST_PREDICT_NAN and want["action"][0, 1, 2] == -1         # BAD
    assert want["action"][0, 2, 0] == want["action"][0, K - 1, 1] == -1 and want["status"][0, 2, 0] == 0


@pytest.mark.parametrize("variant", ["fg", "j2", "elements", "xyz"])
def test_once_per_object_schedule_for_the_other_propagators_and_xyz(hip, variant):
    _once_case(hip, Kk=4, **({"obs_type": "xyz"} if variant == "xyz" else {"propagator": variant}))


def test_once_per_object_schedule_over_update_steps_and_skipped_steps(hip):
    """update_interval = 3 over seven steps from time index 3: indices 3, 6 and 9 update, the others are skipped -- a skipped step's
    slots are cleared records, whoever they name"""
    want, _ = _once_case(hip, Kk=7, interval=3)
    skipped = [k for k in range(7) if (3 + k) % 3]
    assert not want["taken"][0, skipped].any() and (want["action"][0, skipped] == -1).all() and want["taken"][0, [0, 3, 6]].any()


def test_once_per_object_schedule_under_the_regime_layout(hip):
    """2 000 objects stored by orbit regime: the gather goes through the layout's inverse table, the full form through its obj_ids"""
    a, sa = _once_case(hip, Kk=4, m=2000, layout=True)
    b, sb = _once_case(hip, Kk=4, m=2000)
    assert np.array_equal(sa, sb)
    same_result(a, b, "layout against caller order")


def _revisit_schedule(fc, m):
    """object A tasked at steps 0, 2 and 3 by sensors 0, 1, 2; object B at steps 1 and 4; a duplicate within row 1; an idle and an
    out-of-range entry; the rest once-per-object fill.  A and B: healthy objects the forecast shows taken at those slots, if any."""
    ok = ~np.isnan(fc["score"][..., 0])      # [K, S, m]
    a_slots, b_slots = ((0, 0), (2, 1), (3, 2)), ((1, 0), (4, 2))
    score = lambda slots: np.sum([ok[k, s] for k, s in slots], axis=0)      # noqa: E731
    A = int(np.argmax(score(a_slots)))
    sb = score(b_slots)
    sb[A] = -1
    B = int(np.argmax(sb))
    sched = np.full((K, S), -1, dtype=np.int64)
    for k, s in a_slots:
        sched[k, s] = A
    for k, s in b_slots:
        sched[k, s] = B
    sched[1, 1] = B              # the duplicate within a row: sensor 0 takes B, sensor 1's slot is cleared
    sched[0, 1] = -1             # idle
    sched[0, 2] = m + 17         # out of range
    used = {A, B, BAD, FAILED}
    for k in range(K):
        for s in range(S):
            if sched[k, s] == -1 and (k, s) != (0, 1):
                vis = [j for j in np.flatnonzero(ok[k, s]) if j not in used]
                sched[k, s] = int(vis[0]) if vis else min(set(range(m)) - used)
                used.add(int(sched[k, s]))
    return sched, A, B, a_slots, b_slots


def test_revisits_equal_the_step_by_step_chain(hip):
    """a candidate with an object tasked three times, another twice, a duplicate within a row, an idle and an out-of-range entry:
    every record equals the chain's on a second engine from the same state, in both forms.  Asserted on the yardstick's own outputs:
    a revisited object is taken at two or more steps, and its later gain is NOT the forecast's entry for that slot -- what the first
    test cannot show."""
    eng, sp, slot, t0, _ = make_case(hip)
    fc = _read(hip, eng.launch_forecast_sensors(slot, t0, sp, K))
    sched, A, B, a_slots, b_slots = _revisit_schedule(fc, M)
    twin = make_case(hip)[0]
    want, _ = step_chain(hip.torch, twin, sp, sched, slot, t0)
    print("[dry run revisits] schedule %s A=%d B=%d taken %s" % (sched.tolist(), A, B, want["taken"][0].tolist()))
    shown = 0
    for slots in (a_slots, b_slots):
        took = [(k, s) for k, s in slots if want["taken"][0, k, s]]
        for k, s in took[1:]:
            j = int(sched[k, s])
            later, first = want["score"][0, k, s], fc["score"][k, s, j].view(np.int64)
            print("[dry run revisits] object %d slot (%d, %d): chain gain %s, forecast's %s" % (j, k, s, later.view(np.float64), fc["score"][k, s, j]))
            shown += int(not np.array_equal(later, first))
    assert shown >= 1, "no revisited slot whose gain differs from the forecast's entry: the test shows nothing"
    assert want["action"][0, 1, 1] == -1 and want["action"][0, 0, 1] == -1 and want["action"][0, 0, 2] == -1      # duplicate, idle, out of range
    gathered, full = _both_forms(eng, sp, slot, t0, sched)
    same_result(gathered, want, "gathered against the chain")
    same_result(full, want, "full catalogue against the chain")


def test_special_rows(hip):
    """each found on the yardstick (the chain), then compared: a filter failed before the launch and tasked (twice); a NaN filter that
    fails in the predict of k = 0 and is tasked at k = 1 and k = 3; an object hidden from its sensor but visible from another; an (s, j)
    whose visibility changes inside the horizon, tasked at every step"""
    from ssa_gym_amd import _lib as L
    eng, sp, slot, t0, _ = make_case(hip)
    fc = _read(hip, eng.launch_forecast_sensors(slot, t0, sp, K))
    vis, healthy = fc["visible"].astype(bool), (fc["status"] == L.ST_OK).all(axis=(0, 1))
    changing = [(s, int(j)) for s in range(S) for j in np.flatnonzero(vis[:, s].any(axis=0) & ~vis[:, s].all(axis=0) & healthy)]
    assert changing, "no (s, j) whose visibility changes inside the horizon"
    sc, jc = changing[0]
    others = [s for s in range(S) if s != sc]
    # hidden from a sensor that is not the changing pair's, visible from another, at a step where that sensor's column is free (k = 4)
    hidden = [(4, s0, int(j)) for s0 in others for s1 in range(S) for j in np.flatnonzero(~vis[4, s0] & vis[4, s1] & healthy) if j != jc]
    assert hidden, "no object hidden from one site and visible from another"
    kh, sh, jh = hidden[0]
    sched = np.full((K, S), -1, dtype=np.int64)
    sched[:, sc] = jc                                   # the changing (s, j), every step: a revisit wherever it is visible twice
    sched[0, others[0]], sched[2, others[0]] = FAILED, FAILED
    sched[1, others[1]], sched[3, others[1]] = BAD, BAD
    sched[kh, sh] = jh
    twin = make_case(hip)[0]
    want, _ = step_chain(hip.torch, twin, sp, sched, slot, t0)
    print("[dry run special rows] schedule %s\n  taken %s visible %s status %s" % (sched.tolist(), want["taken"][0].tolist(),
                                                                                    want["visible"][0].tolist(), want["status"][0].tolist()))
    fs = [(k, s) for k in range(K) for s in range(S) if sched[k, s] == FAILED]
    bs = [(k, s) for k in range(K) for s in range(S) if sched[k, s] == BAD]
    assert fs and all(want["status"][0, k, s] == L.ST_UPDATE_NAN and want["action"][0, k, s] == -1 for k, s in fs)
    assert bs and all(want["status"][0, k, s] == L.ST_PREDICT_NAN and want["action"][0, k, s] == -1 for k, s in bs) and min(bs)[0] >= 1
    col = want["visible"][0, :, sc]
    assert col.any() and not col.all(), "the changing (s, j) did not change on the chain"
    assert want["action"][0, kh, sh] == jh and not want["visible"][0, kh, sh] and not want["taken"][0, kh, sh]      # attempted, hidden
    gathered, full = _both_forms(eng, sp, slot, t0, sched)
    same_result(gathered, want, "gathered against the chain")
    same_result(full, want, "full catalogue against the chain")


def test_candidates_do_not_see_each_other(hip):
    """seven candidates of 1, 4, 5 and 15 distinct objects, an all-idle one and an identical pair in ONE launch: each one's records
    equal the same candidate evaluated alone and in the full-catalogue form; the pair is byte-identical"""
    eng, sp, slot, t0, _ = make_case(hip)
    fc = _read(hip, eng.launch_forecast_sensors(slot, t0, sp, K))
    seen = np.flatnonzero((~np.isnan(fc["score"][..., 0])).any(axis=(0, 1)))      # objects some sensor could take at some step
    assert len(seen) >= 15
    pool = [int(j) for j in seen[:15]]
    one = np.full((K, S), pool[0], dtype=np.int64)                       # 1 object: every slot, duplicates in every row
    four = np.array(pool[:4] * 4)[:K * S].reshape(K, S)                  # 4 objects, each revisited
    five = np.array(pool[3:8] * 3).reshape(K, S)                         # 5 objects: W = 8
    fifteen = np.array(pool).reshape(K, S)                               # 15 objects: W = 16
    idle = np.array([[-1, M, -7]] * K)
    pair = np.array([[pool[2], pool[9], BAD]] * K)
    cands = np.stack([one, four, five, fifteen, idle, pair, pair])
    got = record_bits(eng.launch_dryrun_sensors(slot, t0, sp, cands))
    assert got["score"].shape == (7, K, S, 3) and not got["spare"].any()
    assert got["taken"][:4].any(axis=(1, 2)).all() and not got["taken"][4].any()
    for b in range(7):
        alone, full = _both_forms(eng, sp, slot, t0, cands[b])
        for k in KEYS:
            assert np.array_equal(got[k][b:b + 1], alone[k]), (b, k)
            assert np.array_equal(got[k][b:b + 1], full[k]), (b, k, "full")
    for k in KEYS:
        assert np.array_equal(got[k][5], got[k][6]), k


def test_env_is_untouched_and_an_episode_does_not_notice(envs, hip):
    """evaluate_schedules() before every step of a 30-step episode: the engine's tensors, env.i and np_random around each call, and at
    the end everything step() leaves equals the twin's without, bit for bit"""
    cfg = cfg8(envs, m=M, seed=21, steps=40)
    a, b = envs.make('ssa_tasker_simple-v2', config=cfg), envs.make('ssa_tasker_simple-v2', config=cfg)
    rs, rc = np.random.RandomState(4), np.random.RandomState(8)
    for k in range(30):
        cand = rc.randint(-2, M + 2, size=(1 + k % 4, 1 + k % 5, 3))
        before, draws, i0 = state_bytes(hip.torch, a._engine), a.np_random.get_state()[1].copy(), a.i
        r = a.evaluate_schedules(cand if k % 2 else cand[0])
        after = state_bytes(hip.torch, a._engine)
        assert before.keys() == after.keys() and all(before[n] == after[n] for n in before), k
        assert a.i == i0 and np.array_equal(a.np_random.get_state()[1], draws)
        B = cand.shape[0] if k % 2 else 1
        assert r["score"].shape == (B, cand.shape[1], 3, 3) and r["total"].shape == (B, 3) and r["taken"].dtype == hip.torch.bool
        acts = _distinct(rs, a.m, 3)
        oa, ob = a.step(acts), b.step(acts)
        assert np.array_equal(oa[0], ob[0]) and np.array_equal(oa[1], ob[1], equal_nan=True)
    _assert_same_env(a, b, "evaluate_schedules before every step")
    # K is cut at the episode's end; past it there is nothing to evaluate
    for _ in range(7):
        a.step(_distinct(rs, a.m, 3))
    assert a.i == 37 and a.evaluate_schedules(np.zeros((6, 3), dtype=np.int64))["taken"].shape == (1, 2, 3)
    for _ in range(2):
        a.step(_distinct(rs, a.m, 3))
    with pytest.raises(ValueError):
        a.evaluate_schedules(np.zeros((6, 3), dtype=np.int64))


def test_dry_run_against_execution(envs, hip):
    """a horizon-wide plan, dry-run and then executed by rollout_sensors(): the dry run's taken / visible flags are the ones the
    execution books (visibility is the truth's, a singular S does not depend on the noise), and its totals are the slot-order sums"""
    from ssa_gym_amd import _lib as L, agents
    env = envs.make('ssa_tasker_simple-v2', config=cfg8(envs, m=M, seed=21, steps=40))
    rs = np.random.RandomState(3)
    for _ in range(2):
        env.step(_distinct(rs, env.m, 3))
    plan = agents.plan_info_gain_sensors_horizon(env, K)
    res = result_bits(env.evaluate_schedules(plan))
    for c in range(3):
        assert np.array_equal(np.array([slot_total(res, c)]).view(np.int64), res["total"][0, c:c + 1]), c
    i0 = env.i
    env.rollout_sensors(plan)
    assert env.i == i0 + K
    booked = np.array([[bool(env.obs_taken[i0 + 1 + k, s]) for s in range(3)] for k in range(K)])
    print("[dry run against execution] plan %s taken %s booked %s" % (plan.tolist(), res["taken"][0].tolist(), booked.astype(int).tolist()))
    assert np.array_equal(res["taken"][0].astype(bool), booked) and booked.any()
    e = env._engine
    hip.torch.cuda.synchronize()
    upd = e.upd_sensors.cpu().numpy()
    for k in range(max(0, K - e.H), K):                  # the records that survive in the ring
        rec = upd[(i0 + 1 + k) % e.H]
        assert np.array_equal(rec[:, L.UPD_VISIBLE].astype(np.int64), res["visible"][0, k]), k
        assert np.array_equal(rec[:, L.UPD_ACTION].astype(np.int64), res["action"][0, k]), k


def test_refine_plan_sensors(envs, hip):
    """2 rounds x 16 candidates on 403 objects: the returned total is the plan's own, bit for bit, and no smaller than the incumbent's;
    rollout_sensors() accepts the plan; the same seed gives the same plan; env.np_random is not touched"""
    from ssa_gym_amd import _lib as L, agents
    env = envs.make('ssa_tasker_simple-v2', config=cfg8(envs, m=M, seed=21, steps=40))
    rs = np.random.RandomState(3)
    for _ in range(2):
        env.step(_distinct(rs, env.m, 3))
    plan = agents.plan_info_gain_sensors_horizon(env, K)
    draws = env.np_random.get_state()[1].copy()
    base = env.evaluate_schedules(plan)["total"].cpu().numpy()[0]
    out, total = agents.refine_plan_sensors(env, plan, kind='info', rounds=2, candidates=16, seed=5)
    again, total2 = agents.refine_plan_sensors(env, plan, kind='info', rounds=2, candidates=16, seed=5)
    assert np.array_equal(env.np_random.get_state()[1], draws)
    assert np.array_equal(out, again) and np.array_equal(total.view(np.int64), total2.view(np.int64))
    own = env.evaluate_schedules(out)["total"].cpu().numpy()[0]
    print("[refine] incumbent %s refined %s (%d slots changed)" % (base.tolist(), total.tolist(), int((out != plan).sum())))
    assert np.array_equal(total.view(np.int64), own.view(np.int64)) and total[L.LOOK_INFO_GAIN] >= base[L.LOOK_INFO_GAIN]
    assert out.shape == plan.shape and out.dtype == np.int64
    i0 = env.i
    env.rollout_sensors(out)
    assert env.i == i0 + K


def test_refine_finds_the_revisit_the_horizon_plan_cannot_express(envs, hip):
    """10 objects, one site that sees all of them, 15 slots: the horizon-wide plan names every object once and has nothing to value the
    other five slots by; the refined plan revisits, and its information gain is strictly larger -- first on the yardstick chain (twin
    envs spent by it), then by the dry run, whose totals equal the chain's bit for bit"""
    from ssa_gym_amd import _lib as L, agents
    cfg = cfg8(envs, m=10, sensors=0, seed=21, steps=60, obs_limit=-80)
    env = envs.make('ssa_tasker_simple-v2', config=cfg)
    rs = np.random.RandomState(3)
    acts = [int(rs.randint(10)) for _ in range(2)]
    for a in acts:
        env.step(a)
    plan = agents.plan_info_gain_sensors_horizon(env, 15)
    out, total = agents.refine_plan_sensors(env, plan, kind='info', rounds=4, candidates=32, seed=2)
    chain = []
    for sched in (plan, out):
        twin = envs.make('ssa_tasker_simple-v2', config=cfg)
        for a in acts:
            twin.step(a)
        want, _ = step_chain(hip.torch, twin._engine, twin._sites(), sched, twin.i % twin._engine.H, twin.i + 1)
        same_result(result_bits(env.evaluate_schedules(sched)), want, "the dry run against the chain")
        chain.append(slot_total(want, L.LOOK_INFO_GAIN))
    counts = np.bincount(out[:, 0], minlength=10)
    print("[refine revisit] horizon plan %s chain total %r\n  refined %s chain total %r visits %s"
          % (plan[:, 0].tolist(), chain[0], out[:, 0].tolist(), chain[1], counts.tolist()))
    assert chain[1] > chain[0], "no better schedule with a revisit exists on the chain for this seed"
    assert counts.max() >= 2, "the refined plan has no revisit"
    assert total[L.LOOK_INFO_GAIN] == chain[1]
