"""Space-based sensors of a network on the GPU, engine level (ssa_step_params.site_rows / limb_radius / site_moving): the line-of-sight
rule itself through ssa_los_mask_f64, the sensor step against the ground step that is given the row's site words and a mask that says
what the rule says, the lookahead's visibility table, every composite entry against its defining chain with the site table changing
along the chain (two sensors on LEO arcs from device.propagate), the *_envs forms with different time words per env, and the feature
off.  8 objects (two tiles; 6: a ragged one), 3 sensors -- a ground radar, a moving 'ae' telescope, a moving 'aer' sensor that needs
its object sunlit: site_moving = 0b110 --, 16 time rows.  Every yardstick is bit-exact: paths that exist without the feature, and
the numpy rule on cells with margin (tests/support/orbiting.py)."""
import numpy as np
import pytest

from support import angles_only as ao
from support import illumination as il
from support import orbiting as ob
from support.batches import c2t
from support.gpu import hip  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

ACTS = [0, 1, 2]     # sensor s is tasked with object s


def _propagate(hip):
    """device.propagate as support.orbiting.leo_arc takes it: the arcs of the tests' sensors come from the device"""
    torch = hip.torch
    return lambda x, dt: hip.dev.propagate(torch.as_tensor(np.ascontiguousarray(x), device="cuda"), dt).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- 1. the rule
def test_the_rule_against_numpy(hip):
    """ssa_los_mask_f64 from sensors at three radii, under a real trans row: objects on the sensor's side of the Earth, directly behind
    it, 1e-6 R_b inside and outside the limb, with the closest point of the line beyond either end of the segment, a NaN row -- and
    against a NaN site row: nothing is visible.  Every judged row keeps | closest approach - R_b | >= 1e-6 R_b and | p |, | p - dd | >=
    1e3 | d |, asserted on the inputs"""
    torch = hip.torch
    R = ob.R_LIMB
    M = c2t()[3]
    for k, radius in enumerate((ob.LEO, 2.6e7, 4.2e7)):
        u = il.unit([0.3 + k, -0.8, 0.52])
        w = il.unit(np.cross(u, [0.0, 0.2 * k, 1.0]))
        o_in = radius * u                      # (the sensor in the frame of x_true; the site row holds M o)

        def along(q, L):                       # a point L along the line from the sensor that passes the geocentre at distance q
            a = np.arcsin(q / radius)
            return o_in + L * (-np.cos(a) * u + np.sin(a) * w)
        reach = np.sqrt(radius ** 2 - (0.5 * R) ** 2)
        far = radius + 4e7
        rows = [o_in + 3e7 * u + 1e6 * w, o_in + 2e7 * w + 1e4 * u,                      # on the sensor's side
                along(0.0, far) + 10.0 * w, along(1e3, far),                             # directly behind the Earth (10 m, 1 km off the axis)
                along(R * (1 - 1.001e-6), far), along(R * (1 + 1.001e-6), far),      # just inside, just outside the limb (1e-6 R_b, and the
                #                                                                          construction's own rounding on top)
                along(0.5 * R, 0.2 * reach), along(0.5 * R, 0.6 * reach),                # the line cuts the sphere, the object stops short of it
                along(0.5 * R, far), along(2.0 * R if radius > 2 * R else 1.05 * R, far),   # ... carried through; and a line that misses
                np.array([np.nan, 1e7, 1e7])]
        x = np.concatenate([np.array(rows), np.ones((len(rows), 3))], axis=1)
        enu, obs = ob.site_words(M, o_in)
        ob.assert_margins(x[:-1, :3], M, obs)
        want = ob.los_clear(x[:, :3], M, obs)
        assert want.tolist() == [True, True, False, False, False, True, True, True, False, True, False], (k, want.tolist())
        xd = torch.as_tensor(x, device="cuda")
        Md = torch.as_tensor(np.ascontiguousarray(M).reshape(9), device="cuda")
        row = np.zeros(16)
        row[:9], row[9:12] = enu, obs
        got = hip.dev.los_mask(xd, Md, torch.as_tensor(row, device="cuda"), R).cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got.astype(bool), want), (k, np.flatnonzero(got.astype(bool) != want))
        for bad in (9, 10, 11):                # (a NaN in the sensor's position: nothing is visible; the enu words are not read)
            nan_row = row.copy()
            nan_row[bad] = np.nan
            assert not hip.dev.los_mask(xd, Md, torch.as_tensor(nan_row, device="cuda"), R).cpu().numpy().any()
        nan_row = row.copy()
        nan_row[:9] = np.nan
        assert np.array_equal(hip.dev.los_mask(xd, Md, torch.as_tensor(nan_row, device="cuda"), R).cpu().numpy(), got)
        # (the radius is the argument: a sphere that holds the sensor itself blocks every object whose line of sight has its closest point inside the segment)
        big = hip.dev.los_mask(xd, Md, torch.as_tensor(row, device="cuda"), 1e9).cpu().numpy().astype(bool)
        assert np.array_equal(big, ob.los_clear(x[:, :3], M, obs, R=1e9))


# ---------------------------------------------------------------------------------------------------------------- 2. the step
def _step_case(hip, oracle, oracle_ld, propagator, m, tix, seed, place, sun_of, dark_word):
    """one step at row tix, sensors 1 and 2 at place(s, truth of object s at the step), site_moving = 0b110; and the same call with
    site_moving = 0, the block's enu[s] / obs_itrs[s] set to row (tix, s) and obs_limit[s] = -2.0 where the rule says clear, 2.0 where it
    says blocked (the Sun table the same vectors, every site dark: a ground sensor reads the bit).  Byte-equal; returns (the rule's
    verdicts, the result, the truth, the row's Sun)"""
    net = ob.Net(oracle)
    state = ao.scene(net, oracle_ld, c2t()[tix], m, seed, high=True)
    tr = il.truths(oracle, state[0], 1)[0]
    pos = {s: np.tile(place(s, tr[s, :3]), (ob.N_TIME, 1)) for s in (1, 2)}
    for s in (1, 2):                # (the other rows hold another position: a wrong row is a wrong answer)
        pos[s][np.arange(ob.N_TIME) != tix] = ob.below(tr[s, :3], tilt=0.9, seed=77 + s)
    rows, obs = ob.table(c2t()[:ob.N_TIME], pos)
    sun, dark = il.table({tix: (sun_of(tr), dark_word)}, il.zenith(net, c2t()[tix]), default_dark=0)
    clear = {s: bool(ob.los_clear(tr[s, :3], c2t()[tix], obs[tix, s])) for s in (1, 2)}
    for s in (1, 2):
        ob.assert_margins(tr[s:s + 1, :3], c2t()[tix], obs[tix, s])
    gap = np.abs(oracle.hx_aer(tr[:1], c2t()[tix], net.lla[0], net.itrs[0])[:, 1] - net.lim[0])
    il.assert_margins(tr[ACTS], sun[tix], gap)
    eng, sp, zn = ob.make_engine(hip, net, m, rows, sun, dark, propagator)
    assert eng._site_moving == 0b110 and sp.sunlit_only == 0b100 and sp.angles_only == 0b010
    on = il.step(hip, eng, sp, state, tix, ACTS)
    lim = net.lim.copy()
    for s in (1, 2):
        lim[s] = ob.BELOW_ANY if clear[s] else ob.ABOVE_ANY
    ref_eng, _, _ = ob.make_engine(hip, net, m, rows, sun, np.full(ob.N_TIME, il.ALL_DARK, dtype=np.int64), propagator, zn=zn, on=False)
    assert ref_eng._site_moving == 0 and ref_eng.site_rows is None
    ref_sp = net.params(ob.N_TIME * m * 3, sun_ptr=ref_eng.sun.data_ptr(), lim=lim,
                        sites={s: (rows[tix, s, :9], rows[tix, s, 9:12]) for s in (1, 2)})
    ref = il.step(hip, ref_eng, ref_sp, state, tix, ACTS)
    il.same_bits(on, ref, (propagator, m, tix, clear))
    L = hip.lib
    lit = bool(il.sunlit(tr[2, :3], sun[tix]))
    want = [1.0, float(clear[1]), float(clear[2] and lit)]
    assert on["upd"][:, L.UPD_OBS_TAKEN].tolist() == want and on["upd"][:, L.UPD_VISIBLE].tolist() == want, on["upd"][:, :2]
    assert on["upd"][:, L.UPD_ACTION].tolist() == ACTS and on["fails"] == 0 and not on["st"].any()
    return clear, on, tr, sun[tix]


@pytest.mark.parametrize("m", [8, 6])
@pytest.mark.parametrize("propagator", ["fg", "hybrid"])
def test_step_is_the_ground_step_with_the_rows_words(hip, oracle, oracle_ld, propagator, m):
    """all clear; sensor 1's object behind the Earth; sensor 2 clear but its object in the Earth's shadow; sensor 2's 'site' not dark in
    the Sun table while its object is lit and clear -- the observation is taken: the dark bit is not read for a moving sensor"""
    net = ob.Net(oracle)

    def under(s, r):
        return ob.below(r, seed=s)
    clear, on, tr, s = _step_case(hip, oracle, oracle_ld, propagator, m, 5, 11, under, lambda tr: il.zenith(net, c2t()[5]), il.ALL_DARK)
    assert clear == {1: True, 2: True} and il.sunlit(tr[ACTS, :3], s).all()
    clear, on, tr, s = _step_case(hip, oracle, oracle_ld, propagator, m, 7, 12, lambda s, r: ob.behind(r, seed=s) if s == 1 else ob.below(r, seed=s),
                                  lambda tr: il.zenith(net, c2t()[7]), il.ALL_DARK)
    assert clear == {1: False, 2: True}
    clear, on, tr, s = _step_case(hip, oracle, oracle_ld, propagator, m, 3, 13, under, lambda tr: il.sun_lighting(tr[2, :3], -1.0), il.ALL_DARK)
    assert clear == {1: True, 2: True} and not il.sunlit(tr[2, :3], s) and on["upd"][2, hip.lib.UPD_OBS_TAKEN] == 0.0
    clear, on, tr, s = _step_case(hip, oracle, oracle_ld, propagator, m, 9, 14, under, lambda tr: il.zenith(net, c2t()[9]), 0b001)
    assert clear == {1: True, 2: True} and il.sunlit(tr[2, :3], s) and on["upd"][2, hip.lib.UPD_OBS_TAKEN] == 1.0


# ---------------------------------------------------------------------------------------------------------------- 3. the lookahead
@pytest.mark.parametrize("m", [8, 6])
def test_lookahead_visibility_is_mask_and_rule(hip, oracle, oracle_ld, m):
    """visible[S, m] of ssa_lookahead_sensors_f64 for all S m cells at a row where sensor 1 sees some objects and not others; the three
    score columns of every visible cell bit for bit against the ground lookahead on the row's words (NaN in every other cell); status
    and P_post of every cell against the sensor step that tasks that cell alone: its P+ where the observation is taken, the prior where
    it is not, and the step's status"""
    torch, L = hip.torch, hip.lib
    net = ob.Net(oracle)
    t1 = ob.CHAIN_T1
    state, rows, obs, sun, dark, exp, _ = ob.chain_scene(net, oracle, oracle_ld, _propagate(hip), m)
    want = exp[0]
    assert want[1].any() and not want[1].all() and want[2].all()
    eng, sp, zn = ob.make_engine(hip, net, m, rows, sun, dark)
    eng.load_state(0, *state)
    eng.status.zero_()
    look = il.read(torch, eng.launch_lookahead_sensors(0, t1, sp, out=("P_prior", "P_post")))
    assert np.array_equal(look["visible"].astype(bool), want), np.argwhere(look["visible"].astype(bool) != want).tolist()
    assert np.array_equal(np.isnan(look["score"][..., 0]), ~want) and not look["status"].any()
    # the score VALUES: the ground lookahead (site_moving = 0) given row t1's words for sensors 1 and 2 and a mask every elevation clears
    # sees every cell; where the rule says clear the moving pass's three score columns and P+ are its bits
    ref_eng, _, _ = ob.make_engine(hip, net, m, rows, sun, np.full(ob.N_TIME, il.ALL_DARK, dtype=np.int64), zn=zn, on=False)
    lim = net.lim.copy()
    lim[1:] = ob.BELOW_ANY
    ref_sp = net.params(ob.N_TIME * m * 3, sun_ptr=ref_eng.sun.data_ptr(), lim=lim, sites={s: (rows[t1, s, :9], rows[t1, s, 9:12]) for s in (1, 2)})
    ref_eng.load_state(0, *state)
    ref_eng.status.zero_()
    ref = il.read(torch, ref_eng.launch_lookahead_sensors(0, t1, ref_sp, out=("P_prior", "P_post")))
    assert ref["visible"][1:].all() and not np.isnan(ref["score"][1:]).any()
    il.same_bits({"score": look["score"][want], "P_post": look["P_post"][want], "P_prior": look["P_prior"], "row0": look["score"][0]},
                 {"score": ref["score"][want], "P_post": ref["P_post"][want], "P_prior": ref["P_prior"], "row0": ref["score"][0]}, "scores")
    assert np.isnan(look["score"][~want]).all()
    for s in range(3):
        for j in range(m):
            one = il.step(hip, eng, sp, state, t1, [j if q == s else -1 for q in range(3)])
            assert one["upd"][s, L.UPD_OBS_TAKEN] == float(want[s, j]) and one["st"][j] == look["status"][s, j]
            il.same_bits({"P": one["P"][j]}, {"P": look["P_post"][s, j] if want[s, j] else look["P_prior"][j]}, (s, j))


# ---------------------------------------------------------------------------------------------------------------- 4. the composite entries
@pytest.mark.parametrize("m", [8, 6])
def test_forecast_is_lookahead_and_idle_step_with_the_table_changing(hip, oracle, oracle_ld, m):
    """ssa_forecast_sensors_f64, H = 3, byte for byte against lookahead + idle step at each row; its visible[H, S, m] is the numpy
    table, with cells that flip each way between the rows (asserted by the scene)"""
    torch = hip.torch
    t1 = ob.CHAIN_T1
    net = ob.Net(oracle)
    state, rows, obs, sun, dark, exp, _ = ob.chain_scene(net, oracle, oracle_ld, _propagate(hip), m)
    eng, sp, zn = ob.make_engine(hip, net, m, rows, sun, dark)
    eng.load_state(0, *state)
    eng.status.zero_()
    fc = il.read(torch, eng.launch_forecast_sensors(0, t1, sp, 3, out=("P_post",)))
    assert np.array_equal(fc["visible"].astype(bool), exp), np.argwhere(fc["visible"].astype(bool) != exp).tolist()
    for h in range(3):
        look = il.read(torch, eng.launch_lookahead_sensors(h % 2, t1 + h, sp, out=("P_post",)))
        il.same_bits({k: fc[k][h] for k in look}, look, ("forecast step", h))
        il.step(hip, eng, sp, None, t1 + h, [-1] * 3, slot=h % 2)


@pytest.mark.parametrize("m", [8, 6])
def test_rollout_is_k_steps_with_the_table_changing(hip, oracle, oracle_ld, m):
    """ssa_env_rollout_sensors_f64, K = 3, against three sensor steps: sensor 1 keeps object 3 while the limb passes over it"""
    torch, L = hip.torch, hip.lib
    t1 = ob.CHAIN_T1
    net = ob.Net(oracle)
    state, rows, obs, sun, dark, exp, _ = ob.chain_scene(net, oracle, oracle_ld, _propagate(hip), m)
    sched = ob.SCHEDULES[0]
    eng, sp, zn = ob.make_engine(hip, net, m, rows, sun, dark)
    taken = []
    for k in range(3):
        r = il.step(hip, eng, sp, state if k == 0 else None, t1 + k, sched[k], slot=k % 2)
        taken.append(r["upd"][:, L.UPD_OBS_TAKEN].tolist())
    assert taken == [[float(exp[k, s, sched[k, s]]) for s in range(3)] for k in range(3)]
    assert len({tuple(t) for t in taken}) > 1      # (the table was at work: the steps do not all take the same observations)
    twin, sp2, _ = ob.make_engine(hip, net, m, rows, sun, dark, zn=zn)
    twin.load_state(0, *state)
    twin.status.zero_()
    twin.launch_rollout_sensors(0, t1, sp2, torch.as_tensor(sched, dtype=torch.int32, device="cuda").contiguous())
    twin.flush_stats()
    torch.cuda.synchronize()
    got = dict(x=twin.x_filter[1].cpu().numpy(), P=twin.P_filter[1].cpu().numpy(), xt=twin.x_true[1].cpu().numpy(),
               obs=twin.obs[1].cpu().numpy(), metrics=twin.metrics[1].cpu().numpy(), st=twin.status.cpu().numpy())
    il.same_bits(got, r, "rollout", keys=list(got))
    flags = twin.upd_sensors.cpu().numpy()[:, :, L.UPD_OBS_TAKEN]
    assert sorted(flags.tolist()) == sorted(taken[1:])


@pytest.mark.parametrize("m", [8, 6])
def test_dry_run_is_its_step_chain_with_the_table_changing(hip, oracle, oracle_ld, m):
    """ssa_dryrun_sensors_envs_f64 on B = 2 candidates of K = 3 steps (the first revisits its objects at every step) against
    support.dryrun.step_chain, candidate by candidate"""
    from support import dryrun
    torch = hip.torch
    t1 = ob.CHAIN_T1
    net = ob.Net(oracle)
    state, rows, obs, sun, dark, exp, _ = ob.chain_scene(net, oracle, oracle_ld, _propagate(hip), m)
    eng, sp, zn = ob.make_engine(hip, net, m, rows, sun, dark)
    eng.load_state(0, *state)
    eng.status.zero_()
    got = dryrun.record_bits(eng.launch_dryrun_sensors(0, t1, sp, ob.SCHEDULES))
    for b in range(2):
        twin, sp2, _ = ob.make_engine(hip, net, m, rows, sun, dark, zn=zn)
        twin.load_state(0, *state)
        twin.status.zero_()
        want, _ = dryrun.step_chain(torch, twin, sp2, ob.SCHEDULES[b], 0, t1)
        dryrun.same_result({k: got[k][b:b + 1] for k in dryrun.KEYS}, want, ("dry run", b))
    for b in range(2):
        assert got["visible"][b].tolist() == [[int(exp[k, s, ob.SCHEDULES[b, k, s]]) for s in range(3)] for k in range(3)], b


def test_the_envs_forms_are_e_single_envs(hip, oracle, oracle_ld):
    """E = 3 envs of 8 objects with different time words (rows 2.., 9.., 5..), ONE site table: the step, the lookahead, the forecast,
    the rollout and the dry run of the *_envs entries against the one-env entries on each env's slice -- an entry that indexed
    site_rows by another env's row would fail: each env's scene flips at its own rows"""
    from support import dryrun
    from support.sensors import _defined_fields
    torch, L = hip.torch, hip.lib
    m, E, t0 = 8, 3, [1, 8, 4]
    net = ob.Net(oracle)
    scenes, shared = [], None
    for e in range(E):
        sc = ob.chain_scene(net, oracle, oracle_ld, _propagate(hip), m, t1=t0[e] + 1, seed=4 + e, shared=shared)
        shared = sc[6]
        scenes.append(sc)
    rows, sun, dark = scenes[0][1], scenes[0][3], scenes[0][4]
    exp = [sc[5] for sc in scenes]
    state = tuple(np.concatenate([sc[0][k] for sc in scenes]) for k in range(3))
    vec, spv, zn = ob.make_engine(hip, net, m, rows, sun, dark, E=E)
    words = torch.as_tensor(t0, dtype=torch.int32)

    def fresh():
        vec.load_state(0, *state)
        vec.status.zero_()
        vec.env_time0.copy_(words)

    def single(e):
        eng, sp, _ = ob.make_engine(hip, net, m, rows, sun, dark, zn=zn[e])
        eng.load_state(0, *(a[e * m:(e + 1) * m] for a in state))
        eng.status.zero_()
        return eng, sp
    sched = ob.SCHEDULES[0]
    cands = [ob.SCHEDULES, ob.SCHEDULES[::-1], ob.SCHEDULES]
    fresh()
    look = il.read(torch, vec.launch_lookahead_sensors_envs(0, 1, spv, out=("P_post",)))
    fc = il.read(torch, vec.launch_forecast_sensors_envs(0, 1, spv, 3, out=("P_post",)))
    dry = dryrun.record_bits(vec.launch_dryrun_sensors_envs(0, 1, spv, np.stack(cands)))
    for e in range(E):
        eng, sp = single(e)
        one = il.read(torch, eng.launch_lookahead_sensors(0, t0[e] + 1, sp, out=("P_post",)))
        il.same_bits({k: look[k][e] for k in one}, one, ("lookahead", e))
        one = il.read(torch, eng.launch_forecast_sensors(0, t0[e] + 1, sp, 3, out=("P_post",)))
        il.same_bits({k: fc[k][:, e] for k in one}, one, ("forecast", e))
        assert np.array_equal(one["visible"].astype(bool), exp[e]), e
        one = dryrun.record_bits(eng.launch_dryrun_sensors(0, t0[e] + 1, sp, cands[e]))
        dryrun.same_result({k: dry[k][e] for k in dryrun.KEYS}, one, ("dry run", e))
    fresh()
    outs = []
    for k in range(3):
        upd = torch.zeros((E, 3, L.UPD_STRIDE), dtype=torch.float64, device="cuda")
        vec.launch_step_sensors_envs(k % 2, (k + 1) % 2, 1 + k, spv, np.tile(sched[k], (E, 1)), upd.data_ptr(), fast_stats=True)
        vec.flush_stats()
        torch.cuda.synchronize()
        outs.append(upd.cpu().numpy())
    final = dict(x=vec.x_filter[1].cpu().numpy(), P=vec.P_filter[1].cpu().numpy(), xt=vec.x_true[1].cpu().numpy(), st=vec.status.cpu().numpy())
    for e in range(E):
        eng, sp = single(e)
        for k in range(3):
            r = il.step(hip, eng, sp, None, t0[e] + 1 + k, sched[k], slot=k % 2)
            il.same_bits({"upd": _defined_fields(L, outs[k][e])}, {"upd": r["upd"]}, ("step", e, k))
            assert r["upd"][:, L.UPD_OBS_TAKEN].tolist() == [float(exp[e][k, s, sched[k, s]]) for s in range(3)], (e, k)
        il.same_bits({k_: v[e * m:(e + 1) * m] for k_, v in final.items()}, {k_: r[k_] for k_ in final}, ("steps", e))
    fresh()
    vec.launch_rollout_sensors_envs(0, 1, spv, torch.as_tensor(np.tile(sched[:, None, :], (1, E, 1)), dtype=torch.int32, device="cuda").contiguous())
    vec.flush_stats()
    torch.cuda.synchronize()
    roll = dict(x=vec.x_filter[1].cpu().numpy(), P=vec.P_filter[1].cpu().numpy(), xt=vec.x_true[1].cpu().numpy(), st=vec.status.cpu().numpy())
    il.same_bits(roll, final, "rollout of the envs")


def _envs_case(hip, oracle, oracle_ld):
    """the E = 3 scene of the *_envs tests: (net, vec engine, its block, noise, state, time words, fresh(), single(e))"""
    torch = hip.torch
    m, E, t0 = 8, 3, [1, 8, 4]
    net = ob.Net(oracle)
    scenes, shared = [], None
    for e in range(E):
        sc = ob.chain_scene(net, oracle, oracle_ld, _propagate(hip), m, t1=t0[e] + 1, seed=4 + e, shared=shared)
        shared = sc[6]
        scenes.append(sc)
    rows, sun, dark = scenes[0][1], scenes[0][3], scenes[0][4]
    state = tuple(np.concatenate([sc[0][k] for sc in scenes]) for k in range(3))
    vec, spv, zn = ob.make_engine(hip, net, m, rows, sun, dark, E=E)
    words = torch.as_tensor(t0, dtype=torch.int32)

    def fresh():
        vec.load_state(0, *state)
        vec.status.zero_()
        vec.env_time0.copy_(words)

    def single(e):
        eng, sp, _ = ob.make_engine(hip, net, m, rows, sun, dark, zn=zn[e])
        eng.load_state(0, *(a[e * m:(e + 1) * m] for a in state))
        eng.status.zero_()
        return eng, sp
    return m, E, t0, [sc[5] for sc in scenes], vec, spv, fresh, single


@pytest.mark.parametrize("rule", ["greedy", "optimal"])
def test_the_envs_decision_chain_reads_each_envs_own_row(hip, oracle, oracle_ld, rule):
    """what SSA_Tasker_VecEnv.step_agent enqueues, at E = 3 with different time words: every env's lookahead, every env's assignment
    (greedy, optimal) into the engine's action table, and the step that reads that table and the time words from device memory
    (launch_step_sensors_envs(actions=None)) -- against lookahead + assignment + step of the one-env entries on each env's slice.
    And the horizon plan on the envs' forecast against the plan on each env's own.  Each env's scene flips at its own rows, so a
    launch that took site_rows at another env's row would task, or observe, other cells"""
    from support.sensors import _defined_fields
    torch, L = hip.torch, hip.lib
    m, E, t0, exp, vec, spv, fresh, single = _envs_case(hip, oracle, oracle_ld)
    fresh()
    plan = vec.launch_plan_sensors(vec.launch_forecast_sensors_envs(0, 1, spv, 3), L.LOOK_INFO_GAIN)
    torch.cuda.synchronize()
    plan = plan.cpu().numpy().copy()
    look = vec.launch_lookahead_sensors_envs(0, 1, spv)
    table = vec.launch_assign_sensors_envs(look, L.LOOK_INFO_GAIN, rule=rule)
    upd = torch.zeros((E, 3, L.UPD_STRIDE), dtype=torch.float64, device="cuda")
    vec.launch_step_sensors_envs(0, 1, 1, spv, None, upd.data_ptr(), fast_stats=True)
    vec.flush_stats()
    torch.cuda.synchronize()
    table, upd = table.cpu().numpy().copy(), upd.cpu().numpy()
    final = dict(x=vec.x_filter[1].cpu().numpy(), P=vec.P_filter[1].cpu().numpy(), xt=vec.x_true[1].cpu().numpy(), st=vec.status.cpu().numpy())
    rows_seen = set()
    for e in range(E):
        eng, sp = single(e)
        one_plan = eng.launch_plan_sensors(eng.launch_forecast_sensors(0, t0[e] + 1, sp, 3), L.LOOK_INFO_GAIN)
        torch.cuda.synchronize()
        assert np.array_equal(plan[:, e], one_plan.cpu().numpy()), (e, plan[:, e].tolist(), one_plan.cpu().numpy().tolist())
        assert all(exp[e][h, s, j] for h in range(3) for s, j in enumerate(plan[h, e, :3]) if j >= 0), e
        row = eng.assign_row()
        eng.launch_assign_sensors(eng.launch_lookahead_sensors(0, t0[e] + 1, sp), L.LOOK_INFO_GAIN, row, rule=rule)
        torch.cuda.synchronize()
        acts = row.cpu().numpy()[:3].tolist()
        assert table[e, :3].tolist() == acts and all(exp[e][0, s, j] for s, j in enumerate(acts) if j >= 0), (e, table[e].tolist(), acts)
        rows_seen.add(tuple(acts))
        r = il.step(hip, eng, sp, None, t0[e] + 1, acts)
        il.same_bits({"upd": _defined_fields(L, upd[e])}, {"upd": r["upd"]}, ("step", e))
        il.same_bits({k_: v[e * m:(e + 1) * m] for k_, v in final.items()}, {k_: r[k_] for k_ in final}, ("state", e))
        assert r["upd"][:, L.UPD_OBS_TAKEN].tolist() == [float(j >= 0) for j in acts], (e, acts)


# ---------------------------------------------------------------------------------------------------------------- 5. off means off
def test_off_means_off(hip, oracle, oracle_ld):
    """site_moving = 0 with site_rows a constant that is never dereferenced (the refusal harness's kind) and limb_radius = NaN:
    byte-equal to the zero tail at the step and the lookahead -- neither is read"""
    torch = hip.torch
    m, t1 = 8, 4
    net = ob.Net(oracle)
    state = ao.scene(net, oracle_ld, c2t()[t1], m, 21, high=True)
    sun, dark = il.table({}, il.zenith(net, c2t()[t1]))
    eng, sp, zn = ob.make_engine(hip, net, m, None, sun, dark, on=False)
    junk, _, _ = ob.make_engine(hip, net, m, None, sun, dark, on=False, zn=zn)
    seen = []

    def never_read(p, sensors):
        p.site_rows, p.limb_radius, p.site_moving = ob.SITE_PTR, float("nan"), 0
        seen.append(sensors is not None)
    junk._set_sites = never_read
    spj = net.params(ob.N_TIME * m * 3, sun_ptr=junk.sun.data_ptr())
    a, b = il.step(hip, eng, sp, state, t1, ACTS), il.step(hip, junk, spj, state, t1, ACTS)
    il.same_bits(a, b, "step")
    assert a["upd"][:, hip.lib.UPD_OBS_TAKEN].tolist() == [1.0, 1.0, 1.0]
    for e_, s_ in ((eng, sp), (junk, spj)):
        e_.load_state(0, *state)
        e_.status.zero_()
    a = il.read(torch, eng.launch_lookahead_sensors(0, t1, sp, out=("P_post",)))
    b = il.read(torch, junk.launch_lookahead_sensors(0, t1, spj, out=("P_post",)))
    il.same_bits(a, b, "lookahead")
    assert a["visible"].all() and seen == [True, True]


# ---------------------------------------------------------------------------------------------------------------- 6. the closed loop's refusal
def test_the_closed_loop_cannot_honour_a_moving_sensor(hip, oracle, oracle_ld):
    """ssa_env_closed_loop_f64 reads the one observer of ssa_consts: a complete block (the one HotPathEngine.launch_closed_loop builds,
    which the entry would launch) with any site_moving bit is SSA_E_UNSUPPORTED, however good the table; behind every other rule of
    the entry -- the same block with a negative wait_ticks keeps SSA_E_INVALID, with the bit and without.  The entry asks the device
    for its occupancy before these rules, so the case needs a GPU; nothing is launched: every call breaks a rule"""
    import ctypes as C
    torch, L = hip.torch, hip.lib
    m, K = 8, 3
    net = ob.Net(oracle)
    sun, dark = il.table({}, il.zenith(net, c2t()[4]))
    eng, sp, zn = ob.make_engine(hip, net, m, None, sun, dark, on=False)
    eng.load_state(0, *ao.scene(net, oracle_ld, c2t()[4], m, 21, high=True))
    ws = torch.zeros(int(eng._lib.ssa_closed_loop_workspace_bytes(m, 1)) // 8, dtype=torch.int64, device="cuda")
    assert ws.numel() > 0
    actions = torch.zeros(K + 1, dtype=torch.int32, device="cuda")
    stats = torch.zeros((K, L.STAT_STRIDE), dtype=torch.float64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32).pin_memory()
    before = (eng.x_filter.clone(), eng.status.clone())

    def answer(bits, wait_ticks, table=ob.SITE_PTR, radius=ob.R_LIMB):
        r = L.ssa_closed_loop_params()
        r.n_steps, r.history, r.slot_out, r.agent = K, eng.H, 1, L.AGENT_NAIVE_GREEDY
        r.x_true_ring, r.x_ring, r.P_ring, r.obs_ring, r.metrics_ring = eng._bx_t, eng._bx, eng._bP, eng._bo, eng._bm
        r.stats_out, r.actions, r.error = stats.data_ptr(), actions.data_ptr(), err.data_ptr()
        r.workspace, r.workspace_bytes, r.wait_ticks = ws.data_ptr(), ws.numel() * 8, wait_ticks
        eng._first_step_block(4)
        p = L.ssa_step_params()
        C.memmove(C.byref(p), C.byref(eng._p), C.sizeof(p))
        p.site_moving, p.site_rows, p.limb_radius = bits, table, radius
        return eng._lib.ssa_env_closed_loop_f64(eng._cref, C.byref(p), C.byref(r), None)
    for bits in (0b10, 0b01, 0b100, -1):
        assert answer(bits, 0) == L.E_UNSUPPORTED, bits
        assert answer(bits, 0, table=0, radius=float("nan")) == L.E_UNSUPPORTED, bits
        assert answer(bits, -1) == L.E_INVALID, bits
    assert answer(0, -1) == L.E_INVALID
    torch.cuda.synchronize()
    assert torch.equal(eng.status, before[1]) and torch.equal(eng.x_filter.view(torch.int64), before[0].view(torch.int64))
    assert not actions.any() and err[0] == 0
