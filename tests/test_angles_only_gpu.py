"""Angles-only sensors on the GPU, engine level (ssa_sensor_params.angles_only): the sensor step of a mixed network -- one az-el-range
sensor, two az-el ones -- against the numpy yardstick of the update with dim_z = 2 (tests/support/angles_only.py; pinned to the
project's filterpy restatement by tests/test_angles_only_host.py) in float64 and in 80-bit arithmetic; what such a sensor must not
read; and the rows of one wavefront taking turns through the shared scratch area.  8 objects (two tiles; 6: a ragged one), 3 sites, 16
time rows; every object stands above the mask of the sensor that tasks it, and every judged update is taken."""
import numpy as np
import pytest

import oracle as orc
from support import angles_only as ao
from support.batches import c2t, errs, make_batch
from support.gpu import hip  # noqa: F401  (the module fixture)
from support.sensors import N_TIME, _defined_fields

pytestmark = pytest.mark.gpu

LAUNCHES = 32      # per case: 32 updates of the az-el-range sensor, 64 of the az-el ones


def _engine(hip, net, m, propagator, resample, zn=None, kinds=True, R=None):
    torch = hip.torch
    g = make_batch(1, seed=0)[3]
    consts = hip.host.make_consts(g["Q"], net.R[0], ao.ALPHA, 2.0, -3, ao.DT, net.lim[0], net.lla[0], propagator=propagator, resample=resample)
    if zn is None:
        gen = torch.Generator(device="cuda").manual_seed(77 + m)
        zn = torch.randn((net.S, N_TIME, m, 3), dtype=torch.float64, device="cuda", generator=gen) * \
            torch.as_tensor(net.sig, dtype=torch.float64, device="cuda").view(net.S, 1, 1, 3)
    eng = hip.engine.HotPathEngine(consts, m, 1, c2t()[:N_TIME], zn, history=2)
    return eng, zn, net.params(N_TIME * m * 3, R=R, kinds=kinds), g


def _launch(hip, eng, sp, state, tix, acts):
    """one sensor step from `state` (slot 0 -> slot 1) at time row tix; everything it leaves, as numpy"""
    torch, L = hip.torch, hip.lib
    eng.load_state(0, *state)
    eng.status.zero_()
    eng.fail_count.zero_()
    eng.stats.zero_()
    upd = torch.zeros((len(acts), L.UPD_STRIDE), dtype=torch.float64, device="cuda")
    eng.launch_step_sensors(0, 1, tix, sp, [int(a) for a in acts], upd.data_ptr(), fast_stats=True, fold_inside=True)
    torch.cuda.synchronize()
    words = [L.STAT_MAX_DPOS, L.STAT_CNT_LT_1E4, L.STAT_CNT_LT_1E7, L.STAT_N_FAILED]
    return dict(x=eng.x_filter[1].cpu().numpy(), P=eng.P_filter[1].cpu().numpy(), xt=eng.x_true[1].cpu().numpy(),
                obs=eng.obs[1].cpu().numpy(), metrics=eng.metrics[1].cpu().numpy(), st=eng.status.cpu().numpy(),
                upd=_defined_fields(L, upd.cpu().numpy()), stats=eng.stats[1].cpu().numpy()[:, words],
                fails=int(eng.fail_count.cpu()[0]))


def _same_bits(a, b, what, keys=None):
    for k in keys or a:
        u, v = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if u.dtype == np.float64:
            u, v = u.view(np.int64), v.view(np.int64)
        assert np.array_equal(u, v), (what, k, np.argwhere(u != v)[:4].tolist())


def _acts(k, m):
    """launch k's objects: sensor s tasks one of the objects placed for it (object j: sensor j % 3), a different one from launch to launch"""
    return [[j for j in range(m) if ao.owner_of(j) == s][(k + s) % len([j for j in range(m) if ao.owner_of(j) == s])] for s in range(3)]


def _reference(o, net, g, state, tix, j, s, zn3, resample, ld):
    """sensor s's update of object j by the oracle `o` (its ukf_predict, sigma points, propagate and hx_aer): the 3-dimensional
    ukf_update for an az-el-range sensor, the yardstick of dim_z = 2 for an az-el one -- in float64 on the fp64 oracle, in longdouble
    on the 80-bit one"""
    Wm, Wc, scale = orc.merwe_weights(ao.ALPHA, 2.0, -3)
    xt, x, P = state
    M = c2t()[tix]
    rc, xp, Pp, sf = o.ukf_predict(x[j], P[j], g["Q"], ao.DT, Wm, Wc, scale, centred=ld)
    assert rc == 0
    zt = o.hx_aer(o.propagate(xt[j], ao.DT), M, net.lla[s], net.itrs[s])[0]
    assert zt[1] >= net.lim[s] + np.radians(5.0), (j, s, zt)       # (visible in the restatement too, far from the mask)
    z = zt + zn3
    if not net.ang[s]:
        rc, xu, Pu, y, S, _ = o.ukf_update(xp, Pp, sf, z, net.R[s], Wm, Wc, scale, M, net.lla[s], net.itrs[s], centred=ld, resample=resample)
        assert rc == 0
        return dict(x=xu, P=Pu, y=y, S=S)
    if resample:
        sf = o.sigma_points(xp, Pp, scale)
    r = ao.update_2d(xp, Pp, sf, o.hx_aer(sf, M, net.lla[s], net.itrs[s]), z[:2], net.R[s][:2, :2], Wm, Wc,
                     dtype=np.longdouble if ld else np.float64, centred=ld)
    assert r is not None
    return {k: np.asarray(r[k], dtype=np.float64) for k in ("x", "P", "y", "S")}


# ---------------------------------------------------------------------------------------------------------------- 5. against the yardstick
@pytest.mark.parametrize("m", [8, 6])
@pytest.mark.parametrize("resample", [False, True])
@pytest.mark.parametrize("propagator", ["fg", "hybrid"])
def test_mixed_network_step_against_the_yardstick(hip, oracle, oracle_ld, propagator, resample, m):
    """x+, P+, y and S of every sensor's update, 32 launches at different time rows.  Criterion of tests/test_sensors_oracle_gpu.py: the
    kernel's distance from the 80-bit value (position, velocity, sd-normalised covariance), median and maximum, at most 3 x the float64
    restatement's own distance plus 1e-12, 1e-12, 1e-9 -- per kind; y within 1e-3 and S within 1e-2 of the 80-bit ones in units of the
    innovation's standard deviations.  The records of the az-el sensors hold y[2] = 0 and S in block form, exactly."""
    L = hip.lib
    net = ao.Net(oracle)
    eng, zn, sp, g = _engine(hip, net, m, propagator, resample)
    assert sp.angles_only == 0b110
    zn_host = zn.cpu().numpy()
    G, Rf = {False: [], True: []}, {False: [], True: []}
    for k in range(LAUNCHES):
        tix = 1 + k % (N_TIME - 1)
        state = ao.scene(net, oracle_ld, c2t()[tix], m, 1000 * m + k)
        acts = _acts(k, m)
        dev = _launch(hip, eng, sp, state, tix, acts)
        assert dev["fails"] == 0 and not dev["st"].any()
        for s, j in enumerate(acts):
            rec = dev["upd"][s]
            assert rec[L.UPD_ACTION] == j and rec[L.UPD_VISIBLE] == 1 and rec[L.UPD_OBS_TAKEN] == 1, (k, s, j, rec[:4])
            f = _reference(oracle, net, g, state, tix, j, s, zn_host[s, tix, j], resample, False)
            ld = _reference(oracle_ld, net, g, state, tix, j, s, zn_host[s, tix, j], resample, True)
            y, S = rec[L.UPD_Y:L.UPD_Y + 3], rec[L.UPD_S:L.UPD_S + 9].reshape(3, 3)
            d = 2 if net.ang[s] else 3
            if net.ang[s]:      # the record's conventions, exactly
                assert y[2] == 0.0 and np.array_equal(S[2], [0.0, 0.0, 1.0]) and np.array_equal(S[:, 2], [0.0, 0.0, 1.0]), (k, s, y, S)
            Sd = np.sqrt(np.diag(ld["S"]))
            e_y = np.max(np.abs(y[:d] - ld["y"]) / Sd)
            e_S = np.max(np.abs(S[:d, :d] - ld["S"]) / np.outer(Sd, Sd))
            assert e_y < 1e-3 and e_S < 1e-2, (k, s, j, e_y, e_S)
            one = lambda r: {"x": r["x"][None], "P": r["P"][None]}      # noqa: E731
            G[bool(net.ang[s])].append(np.array(errs({"x": dev["x"][j:j + 1], "P": dev["P"][j:j + 1]}, one(ld)))[:, 0])
            Rf[bool(net.ang[s])].append(np.array(errs(one(f), one(ld)))[:, 0])
    for ang, need in ((False, LAUNCHES), (True, 2 * LAUNCHES)):
        g_, r_ = np.array(G[ang]), np.array(Rf[ang])
        assert len(g_) == need and need >= 32, (ang, len(g_))
        print("[angles-only step vs yardstick] %s resample=%s m=%d %s: %d updates; vs 80-bit (pos, vel, cov) gpu median %s max %s, "
              "float64 restatement median %s max %s" % (propagator, resample, m, "az-el" if ang else "az-el-range", len(g_),
                                                         np.median(g_, 0), g_.max(0), np.median(r_, 0), r_.max(0)))
        for c, slack in ((0, 1e-12), (1, 1e-12), (2, 1e-9)):
            assert np.median(g_[:, c]) <= 3 * np.median(r_[:, c]) + slack, (ang, c, np.median(g_[:, c]), np.median(r_[:, c]))
            assert g_[:, c].max() <= 3 * r_[:, c].max() + slack, (ang, c, g_[:, c].max(), r_[:, c].max())


def test_an_angles_only_update_is_not_the_range_update(hip, oracle, oracle_ld):
    """the same launch with the kinds set and without: the az-el-range sensor's object is bit-identical, the az-el sensors' objects
    keep more variance than the 3-dimensional update leaves them (the along-range uncertainty stays)"""
    net = ao.Net(oracle)
    eng, zn, sp, g = _engine(hip, net, 8, "fg", False)
    state = ao.scene(net, oracle_ld, c2t()[3], 8, 5)
    acts = _acts(0, 8)
    a = _launch(hip, eng, sp, state, 3, acts)
    b = _launch(hip, eng, net.params(N_TIME * 8 * 3, kinds=False), state, 3, acts)
    assert np.array_equal(a["P"][acts[0]].view(np.int64), b["P"][acts[0]].view(np.int64))
    for s in (1, 2):
        assert np.trace(a["P"][acts[s]][:3, :3]) > 2 * np.trace(b["P"][acts[s]][:3, :3]), s


# ---------------------------------------------------------------------------------------------------------------- 6. what it must not read
@pytest.mark.parametrize("resample", [False, True])
@pytest.mark.parametrize("propagator", ["fg", "hybrid"])
def test_an_angles_only_sensor_reads_neither_the_range_noise_nor_r_beyond_its_block(hip, oracle, oracle_ld, propagator, resample):
    """the same launches twice: R[s][2][*], R[s][*][2] and the third noise word of the az-el sensors' draws ordinary, then NaN.  State,
    records, status, statistics, observation and metrics: bit-identical"""
    torch = hip.torch
    net = ao.Net(oracle)
    m = 8
    eng, zn, sp, g = _engine(hip, net, m, propagator, resample)
    R_nan = [r.copy() for r in net.R]
    zn_nan = zn.clone()
    for s in np.where(net.ang)[0]:
        R_nan[s][2, :] = np.nan
        R_nan[s][:, 2] = np.nan
        zn_nan[s, :, :, 2] = float("nan")
    eng_n, _, sp_n, _ = _engine(hip, net, m, propagator, resample, zn=zn_nan, R=R_nan)
    assert np.isnan(np.array(sp_n.R[1][:])).sum() == 5 and not np.isnan(np.array(sp_n.R[0][:])).any()
    taken = 0
    for k in range(4):
        tix = 2 + 3 * k
        state = ao.scene(net, oracle_ld, c2t()[tix], m, 50 + k)
        acts = _acts(k, m)
        a, b = _launch(hip, eng, sp, state, tix, acts), _launch(hip, eng_n, sp_n, state, tix, acts)
        _same_bits(a, b, (propagator, resample, k))
        taken += int(a["upd"][:, hip.lib.UPD_OBS_TAKEN].sum())
        assert not a["st"].any() and not np.isnan(a["x"]).any() and not np.isnan(a["P"]).any()
    assert taken == 12


# ---------------------------------------------------------------------------------------------------------------- 7. rows taking turns
@pytest.mark.parametrize("resample", [False, True])
@pytest.mark.parametrize("propagator", ["fg", "hybrid"])
def test_rows_of_one_wavefront_take_turns_with_their_own_kind(hip, oracle, oracle_ld, propagator, resample):
    """all three sensors task objects of ONE tile (objects 0, 1, 2 -- and 3, 1, 2: the az-el-range row behind the az-el ones): every
    row's object and record are bit-identical to a launch in which the other two sensors are idle"""
    L = hip.lib
    net = ao.Net(oracle)
    m = 8
    eng, zn, sp, g = _engine(hip, net, m, propagator, resample)
    for tix, acts in ((4, [0, 1, 2]), (9, [3, 1, 2])):
        state = ao.scene(net, oracle_ld, c2t()[tix], m, 90 + tix)
        both = _launch(hip, eng, sp, state, tix, acts)
        assert both["upd"][:, L.UPD_OBS_TAKEN].tolist() == [1.0, 1.0, 1.0], both["upd"][:, :4]
        for s in range(3):
            alone = _launch(hip, eng, sp, state, tix, [a if q == s else -1 for q, a in enumerate(acts)])
            j = acts[s]
            assert alone["upd"][s, L.UPD_OBS_TAKEN] == 1.0
            for key in ("x", "P", "obs"):
                assert np.array_equal(both[key][j].view(np.int64), alone[key][j].view(np.int64)), (propagator, resample, tix, s, key)
            assert np.array_equal(both["upd"][s].view(np.int64), alone["upd"][s].view(np.int64)), (propagator, resample, tix, s)
            assert both["st"][j] == alone["st"][j] == 0
