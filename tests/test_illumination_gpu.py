"""The illumination test of a sensor network on the GPU, engine level (ssa_sensor_params.sun / shadow_radius / sunlit_only): the rule
itself through ssa_sunlit_mask_f64, the sensor step lit, dark and blocked, the lookahead's visibility table, every composite entry
against its defining chain with the feature on and the Sun table changing along the chain, and the feature off.  8 objects (two
tiles; 6: a ragged one), 3 sites with sunlit_only = 0b110 and the kinds aer / ae / aer, 16 time rows; the Sun table is the tests' own
(tests/support/illumination.py).  Every yardstick is bit-exact: the existing invisible path, the numpy rule on cells with margin."""
import numpy as np
import pytest

from support import angles_only as ao
from support import illumination as il
from support.batches import c2t
from support.gpu import hip  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

ABOVE_ANY = 2.0      # an elevation mask [rad] no elevation reaches: the existing, tested way to make a sensor see nothing
ACTS = [0, 1, 2]     # object j is placed for sensor j % 3


# ---------------------------------------------------------------------------------------------------------------- 1. the rule
def test_the_rule_against_numpy(hip):
    """ssa_sunlit_mask_f64 on sunward objects, objects on the antisolar axis, just inside and just outside the cylinder (1e-6 R either
    side), behind the terminator plane but outside the cylinder, a NaN row -- and against a NaN Sun: nothing is sunlit"""
    torch = hip.torch
    R = il.R_SHADOW
    s = il.unit([0.3, -0.8, 0.52])
    a = il.unit(np.cross(s, [0.0, 0.0, 1.0]))
    b = np.cross(s, a)
    rows = []
    for k, h in enumerate((7e6, 2.6e7, 4.2e7)):
        w = np.cos(k) * a + np.sin(k) * b
        rows += [h * s + 3e6 * w, h * s, 1e3 * s + h * w,                     # sunward (the last barely: p = 1 km)
                 -h * s, -h * s + 1e4 * w,                                    # on the antisolar axis and next to it
                 -h * s + R * (1 - 1e-6) * w, -h * s + R * (1 + 1e-6) * w,    # just inside, just outside
                 -1e3 * s + R * (1 - 1e-6) * w,                               # 1 km behind the terminator plane, inside
                 -h * s + 2 * R * w, -1e3 * s + h * w]                        # behind the plane, outside the cylinder
    rows.append(np.array([np.nan, 1e7, 1e7]))
    x = np.concatenate([np.array(rows), np.ones((len(rows), 3))], axis=1)
    rel, p, inside = il.margins(x[:-1, :3], s)
    assert np.all(rel >= 0.99e-6) and np.all(p[inside] >= 0.99e3)
    want = il.sunlit(x[:, :3], s)
    assert want.sum() == 18 and not want[-1] and len(want) == 31
    xd = torch.as_tensor(x, device="cuda")
    got = hip.dev.sunlit_mask(xd, torch.as_tensor(np.append(s, 0.0), device="cuda"), R).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got.astype(bool), want), np.flatnonzero(got.astype(bool) != want)
    nan_sun = hip.dev.sunlit_mask(xd, torch.as_tensor([np.nan, s[1], s[2], 0.0], dtype=torch.float64, device="cuda"), R).cpu().numpy()
    assert not nan_sun.any()
    # (the shadow's radius is the argument: every object behind the terminator plane is in a shadow of 1e9 m)
    assert np.array_equal(hip.dev.sunlit_mask(xd, torch.as_tensor(s, device="cuda"), 1e9).cpu().numpy().astype(bool), x[:, :3] @ s >= 0)


# ---------------------------------------------------------------------------------------------------------------- 2, 3. the step
def _step_case(hip, oracle, oracle_ld, propagator, m, tix, seed, sun_of, dark_word):
    """one step at row tix with the row's Sun sun_of(truth at the step) and dark word, feature on; the same call with sunlit_only = 0
    and the mask of every blocked sensor raised above any elevation.  Byte-equal; returns (blocked sensors, the result, the truth)"""
    net = il.Net(oracle)
    state = ao.scene(net, oracle_ld, c2t()[tix], m, seed)
    tr = il.truths(oracle, state[0], 1)[0]
    sun, dark = il.table({tix: (sun_of(tr), dark_word)}, il.zenith(net, c2t()[tix]), default_dark=0)
    vis, gap = il.expected_visible(net, oracle, tr, c2t()[tix], sun[tix], dark[tix])
    il.assert_margins(tr[ACTS], sun[tix], np.array([gap[s, j] for s, j in enumerate(ACTS)]))
    blocked = [s for s, j in enumerate(ACTS) if not vis[s, j]]
    eng, sp, zn = il.make_engine(hip, net, m, sun, dark, propagator)
    assert sp.sunlit_only == 0b110 and sp.angles_only == 0b010
    on = il.step(hip, eng, sp, state, tix, ACTS)
    lim = net.lim.copy()
    lim[blocked] = ABOVE_ANY
    ref = il.step(hip, eng, net.params(il.N_TIME * m * 3, on=False, lim=lim), state, tix, ACTS)
    il.same_bits(on, ref, (propagator, m, tix, blocked))
    L = hip.lib
    for s in range(3):
        assert on["upd"][s, L.UPD_OBS_TAKEN] == on["upd"][s, L.UPD_VISIBLE] == (0.0 if s in blocked else 1.0), (s, on["upd"][s, :4])
        assert on["upd"][s, L.UPD_ACTION] == ACTS[s]
    assert on["fails"] == 0 and not on["st"].any()
    return blocked, on, tr, sun[tix]


@pytest.mark.parametrize("m", [8, 6])
@pytest.mark.parametrize("propagator", ["fg", "hybrid"])
def test_step_lit_and_dark_is_the_step_without_the_test(hip, oracle, oracle_ld, propagator, m):
    """every tasked object lit, every site dark: every output byte equals the same call with sunlit_only = 0"""
    net = il.Net(oracle)
    blocked, on, tr, s = _step_case(hip, oracle, oracle_ld, propagator, m, 5, 11, lambda tr: il.zenith(net, c2t()[5]), il.ALL_DARK)
    assert blocked == [] and il.sunlit(tr[ACTS, :3], s).all()


@pytest.mark.parametrize("m", [8, 6])
@pytest.mark.parametrize("propagator", ["fg", "hybrid"])
def test_step_blocked_is_the_invisible_path(hip, oracle, oracle_ld, propagator, m):
    """sensor 1's object in the Earth's shadow; sensor 2's site not dark at the row; and sensor 0, whose bit is clear, updating an
    object in shadow from a site that is not dark -- each byte-equal to the call with sunlit_only = 0 and the blocked sensors' masks
    raised above any elevation"""
    net = il.Net(oracle)
    blocked, on, tr, s = _step_case(hip, oracle, oracle_ld, propagator, m, 7, 12, lambda tr: il.sun_lighting(tr[1, :3], -1.0), il.ALL_DARK)
    assert 1 in blocked and not il.sunlit(tr[1, :3], s)
    blocked, on, tr, s = _step_case(hip, oracle, oracle_ld, propagator, m, 3, 13, lambda tr: il.zenith(net, c2t()[3]), 0b011)
    assert blocked == [2] and il.sunlit(tr[ACTS, :3], s).all()
    blocked, on, tr, s = _step_case(hip, oracle, oracle_ld, propagator, m, 9, 14, lambda tr: il.sun_lighting(tr[0, :3], -1.0), 0b110)
    assert 0 not in blocked and not il.sunlit(tr[0, :3], s) and on["upd"][0, hip.lib.UPD_OBS_TAKEN] == 1.0


# ---------------------------------------------------------------------------------------------------------------- 4. the lookahead
@pytest.mark.parametrize("m", [8, 6])
def test_lookahead_visibility_is_mask_and_rule_and_dark_bit(hip, oracle, oracle_ld, m):
    """visible[S, m] of ssa_lookahead_sensors_f64 for all S m cells, at a row where object JSTAR is in shadow and site 2 is not dark;
    score, status and P_post of every cell against the sensor step that tasks that cell alone: its P+ where the observation is taken,
    the prior where it is not (score NaN), and the step's status"""
    torch, L = hip.torch, hip.lib
    net = il.Net(oracle)
    t1 = 6
    state = ao.scene(net, oracle_ld, c2t()[t1], m, 4, high=True)
    tr = il.truths(oracle, state[0], 1)[0]
    sun, dark = il.table({t1: (il.sun_lighting(tr[il.JSTAR, :3], -1.0), 0b011)}, il.zenith(net, c2t()[t1]))
    want, gap = il.expected_visible(net, oracle, tr, c2t()[t1], sun[t1], dark[t1])
    il.assert_margins(tr, sun[t1], gap)
    assert want[0].all() and not want[2].any() and not want[1, il.JSTAR] and want[1].any()
    eng, sp, zn = il.make_engine(hip, net, m, sun, dark)
    eng.load_state(0, *state)
    eng.status.zero_()
    look = il.read(torch, eng.launch_lookahead_sensors(0, t1, sp, out=("P_prior", "P_post")))
    assert np.array_equal(look["visible"].astype(bool), want), np.argwhere(look["visible"].astype(bool) != want).tolist()
    assert np.array_equal(np.isnan(look["score"][..., 0]), ~want) and not look["status"].any()
    for s in range(3):
        for j in range(m):
            one = il.step(hip, eng, sp, state, t1, [j if q == s else -1 for q in range(3)])
            assert one["upd"][s, L.UPD_OBS_TAKEN] == float(want[s, j]) and one["st"][j] == look["status"][s, j]
            il.same_bits({"P": one["P"][j]}, {"P": look["P_post"][s, j] if want[s, j] else look["P_prior"][j]}, (s, j))


# ---------------------------------------------------------------------------------------------------------------- 5. the composite entries
def _chain(hip, oracle, oracle_ld, m, t1=2, seed=4):
    net = il.Net(oracle)
    state, sun, dark, exp = il.chain_scene(net, oracle, oracle_ld, t1, m, seed)
    return net, state, sun, dark, exp


@pytest.mark.parametrize("m", [8, 6])
def test_forecast_is_lookahead_and_idle_step_with_the_table_changing(hip, oracle, oracle_ld, m):
    """ssa_forecast_sensors_f64, H = 3, byte for byte against lookahead + idle step at each row; its visible[H, S, m] is the numpy
    table, with cells that flip each way between the rows (asserted by the scene)"""
    torch = hip.torch
    t1 = 2
    net, state, sun, dark, exp = _chain(hip, oracle, oracle_ld, m, t1)
    eng, sp, zn = il.make_engine(hip, net, m, sun, dark)
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
    """ssa_env_rollout_sensors_f64, K = 3, against three sensor steps: sensor 1 keeps object JSTAR (taken, then in shadow, then its
    site not dark), sensor 2 object 2 (site not dark, then taken twice)"""
    torch, L = hip.torch, hip.lib
    t1 = 2
    net, state, sun, dark, exp = _chain(hip, oracle, oracle_ld, m, t1)
    sched = il.SCHEDULES[0]
    eng, sp, zn = il.make_engine(hip, net, m, sun, dark)
    taken = []
    for k in range(3):
        r = il.step(hip, eng, sp, state if k == 0 else None, t1 + k, sched[k], slot=k % 2)
        taken.append(r["upd"][:, L.UPD_OBS_TAKEN].tolist())
    assert taken == [[float(exp[k, s, sched[k, s]]) for s in range(3)] for k in range(3)]
    assert taken == [[1.0, 1.0, 0.0], [1.0, 0.0, 1.0], [1.0, 0.0, 1.0]]
    twin, sp2, _ = il.make_engine(hip, net, m, sun, dark, zn=zn)
    twin.load_state(0, *state)
    twin.status.zero_()
    twin.launch_rollout_sensors(0, t1, sp2, torch.as_tensor(sched, dtype=torch.int32, device="cuda").contiguous())
    twin.flush_stats()
    torch.cuda.synchronize()
    got = dict(x=twin.x_filter[1].cpu().numpy(), P=twin.P_filter[1].cpu().numpy(), xt=twin.x_true[1].cpu().numpy(),
               obs=twin.obs[1].cpu().numpy(), metrics=twin.metrics[1].cpu().numpy(), st=twin.status.cpu().numpy())
    il.same_bits(got, r, "rollout", keys=list(got))
    # (the records of the last two steps: their flags say what the chain's said)
    flags = twin.upd_sensors.cpu().numpy()[:, :, L.UPD_OBS_TAKEN]
    assert sorted(flags.tolist()) == sorted(taken[1:])


@pytest.mark.parametrize("m", [8, 6])
def test_dry_run_is_its_step_chain_with_the_table_changing(hip, oracle, oracle_ld, m):
    """ssa_dryrun_sensors_envs_f64 on B = 2 candidates of K = 3 steps against support.dryrun.step_chain, candidate by candidate"""
    from support import dryrun
    torch = hip.torch
    t1 = 2
    net, state, sun, dark, exp = _chain(hip, oracle, oracle_ld, m, t1)
    eng, sp, zn = il.make_engine(hip, net, m, sun, dark)
    eng.load_state(0, *state)
    eng.status.zero_()
    got = dryrun.record_bits(eng.launch_dryrun_sensors(0, t1, sp, il.SCHEDULES))
    for b in range(2):
        twin, sp2, _ = il.make_engine(hip, net, m, sun, dark, zn=zn)
        twin.load_state(0, *state)
        twin.status.zero_()
        want, _ = dryrun.step_chain(torch, twin, sp2, il.SCHEDULES[b], 0, t1)
        dryrun.same_result({k: got[k][b:b + 1] for k in dryrun.KEYS}, want, ("dry run", b))
    assert got["taken"][0].tolist() == [[1, 1, 0], [1, 0, 1], [1, 0, 1]] and got["visible"][0].tolist() == got["taken"][0].tolist()


def test_the_envs_forms_are_e_single_envs(hip, oracle, oracle_ld):
    """E = 2 envs of 8 objects with different time words (rows 2.. and 9..), one Sun table: the step, the lookahead, the forecast, the
    rollout and the dry run of the *_envs entries against the one-env entries on each env's slice"""
    from support import dryrun
    torch, L = hip.torch, hip.lib
    m, E, t0 = 8, 2, [1, 8]
    net = il.Net(oracle)
    st0, sun, dark, exp0 = il.chain_scene(net, oracle, oracle_ld, t0[0] + 1, m, 4)
    st1, sun, dark, exp1 = il.chain_scene(net, oracle, oracle_ld, t0[1] + 1, m, 5, sun=sun, dark=dark)
    exp = [exp0, exp1]
    state = tuple(np.concatenate([a, b]) for a, b in zip(st0, st1))
    vec, spv, zn = il.make_engine(hip, net, m, sun, dark, E=E)
    words = torch.as_tensor(t0, dtype=torch.int32)

    def fresh():
        vec.load_state(0, *state)
        vec.status.zero_()
        vec.env_time0.copy_(words)

    def single(e):
        eng, sp, _ = il.make_engine(hip, net, m, sun, dark, zn=zn[e])
        eng.load_state(0, *(a[e * m:(e + 1) * m] for a in state))
        eng.status.zero_()
        return eng, sp
    sched = il.SCHEDULES[0]
    # the lookahead and the forecast (nothing is written)
    fresh()
    look = il.read(torch, vec.launch_lookahead_sensors_envs(0, 1, spv, out=("P_post",)))
    fc = il.read(torch, vec.launch_forecast_sensors_envs(0, 1, spv, 3, out=("P_post",)))
    dry = dryrun.record_bits(vec.launch_dryrun_sensors_envs(0, 1, spv, np.stack([il.SCHEDULES, il.SCHEDULES[::-1]])))
    for e in range(E):
        eng, sp = single(e)
        one = il.read(torch, eng.launch_lookahead_sensors(0, t0[e] + 1, sp, out=("P_post",)))
        il.same_bits({k: look[k][e] for k in one}, one, ("lookahead", e))
        one = il.read(torch, eng.launch_forecast_sensors(0, t0[e] + 1, sp, 3, out=("P_post",)))
        il.same_bits({k: fc[k][:, e] for k in one}, one, ("forecast", e))
        assert np.array_equal(one["visible"].astype(bool), exp[e]), e
        cand = il.SCHEDULES if e == 0 else il.SCHEDULES[::-1]
        one = dryrun.record_bits(eng.launch_dryrun_sensors(0, t0[e] + 1, sp, cand))
        dryrun.same_result({k: dry[k][e] for k in dryrun.KEYS}, one, ("dry run", e))
    # the step, three times, and the rollout
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
            from support.sensors import _defined_fields
            il.same_bits({"upd": _defined_fields(L, outs[k][e])}, {"upd": r["upd"]}, ("step", e, k))
            assert r["upd"][:, L.UPD_OBS_TAKEN].tolist() == [float(exp[e][k, s, sched[k, s]]) for s in range(3)], (e, k)
        il.same_bits({k_: v[e * m:(e + 1) * m] for k_, v in final.items()}, {k_: r[k_] for k_ in final}, ("steps", e))
    fresh()
    vec.launch_rollout_sensors_envs(0, 1, spv, torch.as_tensor(np.tile(sched[:, None, :], (1, E, 1)), dtype=torch.int32, device="cuda").contiguous())
    vec.flush_stats()
    torch.cuda.synchronize()
    roll = dict(x=vec.x_filter[1].cpu().numpy(), P=vec.P_filter[1].cpu().numpy(), xt=vec.x_true[1].cpu().numpy(), st=vec.status.cpu().numpy())
    il.same_bits(roll, final, "rollout of the envs")


# ---------------------------------------------------------------------------------------------------------------- 6. off means off
def test_off_means_off(hip, oracle, oracle_ld):
    """sunlit_only = 0 with `sun` pointing at NaNs and shadow_radius = NaN: byte-equal to the zero tail at the step, the lookahead and
    the forecast -- neither is read"""
    torch = hip.torch
    m, t1 = 8, 4
    net = il.Net(oracle)
    state = ao.scene(net, oracle_ld, c2t()[t1], m, 21, high=True)
    eng, _, zn = il.make_engine(hip, net, m, np.full((il.N_TIME, 3), np.nan), np.full(il.N_TIME, -1, dtype=np.int64))
    assert torch.isnan(eng.sun).all()
    zero = net.params(il.N_TIME * m * 3, on=False)
    assert (zero.sunlit_only, zero.sun, zero.shadow_radius) == (0, None, 0.0)
    nans = net.params(il.N_TIME * m * 3, on=False)
    nans.sun, nans.shadow_radius = eng.sun.data_ptr(), float("nan")
    a, b = il.step(hip, eng, zero, state, t1, ACTS), il.step(hip, eng, nans, state, t1, ACTS)
    il.same_bits(a, b, "step")
    assert a["upd"][:, hip.lib.UPD_OBS_TAKEN].tolist() == [1.0, 1.0, 1.0]
    eng.load_state(0, *state)
    eng.status.zero_()
    for launch in (lambda sp: eng.launch_lookahead_sensors(0, t1, sp, out=("P_post",)),
                   lambda sp: eng.launch_forecast_sensors(0, t1, sp, 3, out=("P_post",))):
        a = il.read(torch, launch(zero))
        b = il.read(torch, launch(nans))
        il.same_bits(a, b, "lookahead / forecast")
        assert a["visible"].all()
