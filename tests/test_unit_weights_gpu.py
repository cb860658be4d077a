"""The fused step's UKF arithmetic on the GPU at unit sigma-point weights (alpha = 1), against the 80-bit oracle under the criterion of
tests/support/unit_weights.py: no further from the 80-bit value than 3 x the float64 oracle is, plus 1e-12 / 1e-12 / 1e-9 (position,
velocity, sd-normalised covariance) and 1e-9 innovation sd for y and S -- six to nine orders of magnitude tighter than the reference's
alpha = 1e-3 / 1e-4 allow (tests/test_hip_step.py), where a slightly wrong weight, R, site or time step passes (shown without a GPU by
tests/test_unit_weights_host.py, which also asserts that every case here is one on the oracle side).  Every row and every env of a case is
judged; every figure is printed with its bound before it is asserted.  One launch per case, 768 rows at the most."""
import numpy as np
import pytest

from support import unit_weights as uw
from support.batches import c2t, relnorm
from support.fused_step import run_gpu
from support.gpu import hip  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

PROPAGATORS = ("fg", "hybrid", "elements")


def _step(hip, oracle, oracle_ld, name, propagator):
    """case `name` in one launch, judged: the device's statuses and records, the truth rows (1e-9 parity with the float64 oracle, as
    tests/test_hip_step.py), z_true, sigmas_h, and under the criterion the updated rows with y and S and the predict-only rows"""
    L = hip.lib
    c, f64, ld = uw.references(oracle, oracle_ld, name)
    uw.assert_oracle_conditions(c, f64, ld)
    label = "%s, %s" % (name, propagator)
    gpu = run_gpu(hip, c.xt, c.x, c.P, c.g, c.actions, c.tix, uw.ALPHA, obs_type=c.obs_type, propagator=propagator, resample=c.resample,
                  E=c.E, R=c.R, z_noise=c.z_noise)
    assert not gpu["status"].any(), (label, np.where(gpu["status"])[0])
    for sl in (slice(0, 3), slice(3, 6)):
        assert relnorm(gpu["x_true"], f64["x_true"], sl).max() < 1e-9, (label, "truth")
    y, S = [], []
    for e, a in enumerate(c.actions):
        rec = gpu["upd"][e]
        if a < 0:
            assert rec[L.UPD_ACTION] == -1.0 and rec[L.UPD_OBS_TAKEN] == 0.0, (label, e, rec[:4])
            continue
        assert rec[L.UPD_OBS_TAKEN] == 1.0 and rec[L.UPD_ACTION] == a and rec[L.UPD_VISIBLE] == 1.0, (label, e, rec[:4])
        zt = f64["z_true"][e]
        assert np.linalg.norm(rec[L.UPD_Z_TRUE:L.UPD_Z_TRUE + 3] - zt) <= 1e-12 * np.linalg.norm(zt) + 1e-12, (label, e)
        sh = rec[L.UPD_SIGMAS_H:L.UPD_SIGMAS_H + 39].reshape(13, 3)
        if not c.resample:     # propagated sigma points: identical inputs -> identical measurements
            np.testing.assert_allclose(sh, f64["sigmas_h"][e], rtol=1e-12, atol=1e-7, err_msg="%s env %d" % (label, e))
        else:                  # redrawn around a prior mean that is good to 1e-14 x 4e7 m now
            np.testing.assert_allclose(sh, ld["sigmas_h"][e], rtol=1e-12, atol=1e-6, err_msg="%s env %d" % (label, e))
        y.append(rec[L.UPD_Y:L.UPD_Y + 3])
        S.append(rec[L.UPD_S:L.UPD_S + 9].reshape(3, 3))
    got = dict(x=gpu["x"], P=gpu["P"])
    if len(c.updated):
        got.update(y=np.array(y), S=np.array(S))
        uw.assert_criterion(label + ", updated rows", got, uw.updates(f64, c), uw.updates(ld, c), rows=c.updated, innovation=True)
    if len(c.predicted):
        uw.assert_criterion(label + ", predict-only rows", got, f64, ld, rows=c.predicted)
    Pp = gpu["P"][c.predicted]      # (a prior covariance leaves the kernel exactly symmetric; P - K S K^T is symmetric to rounding, as the reference's)
    assert np.array_equal(Pp, np.swapaxes(Pp, 1, 2))


# ---------------------------------------------------------------------------------------------------------------- B. the one-observer step
@pytest.mark.parametrize("propagator", PROPAGATORS)
@pytest.mark.parametrize("name", ["predict", "anisotropic"])
def test_predict_only(hip, oracle, oracle_ld, name, propagator):
    """256 objects, no update.  'hybrid' and 'elements' form the covariance in the reference's order: at alpha = 1 there is no
    cancellation to excuse them, and they are held to the same criterion.  'anisotropic': position variances 1 : 1/4 : 1/25 -- the case
    on which a missing sum(Wc) m' m'^T shows (with the golden P0 the mean shift m' vanishes to second order)"""
    _step(hip, oracle, oracle_ld, name, propagator)


@pytest.mark.parametrize("propagator", PROPAGATORS)
@pytest.mark.parametrize("resample", [False, True])
@pytest.mark.parametrize("obs_type", ["aer", "xyz"])
def test_update_of_every_env(hip, oracle, oracle_ld, obs_type, resample, propagator):
    """48 envs of 16 objects in one launch, one update each (the layout of tests/test_hip_step.py: test_update_parity_every_object)"""
    _step(hip, oracle, oracle_ld, obs_type + (" resample" if resample else ""), propagator)


@pytest.mark.parametrize("propagator", PROPAGATORS)
def test_second_step_from_tight_covariances(hip, oracle, oracle_ld, propagator):
    """256 objects with posterior-like covariances (sigma points centimetres to tens of metres apart around |r| ~ 4e7 m).  The float64
    oracle itself has outliers here (max 1.6e-10 / 2.4e-6 in position / covariance against medians of 7.8e-16 / 4.9e-12): the factor 3
    on maximum and median carries them, no row is left out"""
    _step(hip, oracle, oracle_ld, "tight", propagator)


@pytest.mark.parametrize("propagator", ["fg", "hybrid"])
@pytest.mark.parametrize("m", [1, 3, 5, 63])
def test_ragged_sizes(hip, oracle, oracle_ld, m, propagator):
    """a lone object, ragged tiles, a ragged last tile of sixteen: the update on the last row"""
    _step(hip, oracle, oracle_ld, "ragged %d" % m, propagator)


# ---------------------------------------------------------------------------------------------------------------- C. the lookahead
@pytest.mark.parametrize("propagator", PROPAGATORS)
def test_lookahead(hip, oracle, oracle_ld, propagator):
    """the lookahead launch on one env of 16 objects: the prior and P_post[j] against the 80-bit oracle's step with action j and zero
    noise under the criterion; the three gains against values formed in long double from the 80-bit P- / P+ -- within 3 x the float64
    oracle's own gain error plus 1e-9 max(1, |gain|), every object"""
    L, torch = hip.lib, hip.torch
    c = uw.case("lookahead")
    f64, ld = uw.lookahead_references(oracle, c, uw.ALPHA, False), uw.lookahead_references(oracle_ld, c, uw.ALPHA, True)
    for r in (f64, ld):
        assert not r["status"].any() and r["obs_taken"].all()
    consts = hip.host.make_consts(c.g["Q"], c.R, uw.ALPHA, uw.BETA, uw.KAPPA, uw.DT, -np.pi / 2, c.g["obs_lla"], propagator=propagator)
    eng = hip.engine.HotPathEngine(consts, c.m, 1, c2t(), np.zeros((1, 480, c.m, 3)), history=2)
    eng.load_state(0, c.xt, c.x, c.P)
    r = eng.launch_lookahead(0, c.tix, out=hip.engine.HotPathEngine.LOOKAHEAD_PARTS)
    torch.cuda.synchronize()
    look = {k: v.cpu().numpy() for k, v in r.items()}
    assert not look["status"].any() and look["visible"].all() and look["score"].shape == (c.m, L.LOOK_NSCORE)
    label = "lookahead, %s" % propagator
    for what, key in (("prior", "P_prior"), ("P_post", "P")):
        uw.assert_criterion("%s, %s" % (label, what), dict(x=look["x_prior"], P=look["P_prior" if what == "prior" else "P_post"]),
                            dict(x=f64["x"], P=f64[key]), dict(x=ld["x"], P=ld[key]))
    rows = [L.LOOK_TRACE_GAIN, L.LOOK_POS_TRACE_GAIN, L.LOOK_INFO_GAIN]
    err = np.abs(look["score"][:, rows].astype(np.longdouble) - ld["gain"]).astype(np.float64)
    ref = np.abs(f64["gain"] - ld["gain"]).astype(np.float64)
    bound = uw.FACTOR * ref + 1e-9 * np.maximum(1.0, np.abs(ld["gain"].astype(np.float64)))
    for k, nm in enumerate(("trace gain", "position trace gain", "information gain")):
        j = int(np.argmax(err[:, k] / bound[:, k]))
        print("[unit weights] %s: %s, object %d (the closest to its bound): under test %.3e, float64 oracle %.3e, bound %.3e; |gain| %.3e"
              % (label, nm, j, err[j, k], ref[j, k], bound[j, k], abs(float(ld["gain"][j, k]))))
    assert np.all(err <= bound), (label, np.argwhere(err > bound).tolist(), (err / bound).max())


# ---------------------------------------------------------------------------------------------------------------- D. 'aer' next to 'ae'
@pytest.mark.parametrize("propagator", ["fg", "hybrid"])
def test_sensor_network_aer_next_to_ae(hip, oracle, oracle_ld, propagator):
    """two sites, an az-el-range sensor and an az-el one, 8 objects with the golden P0, 8 launches at different time rows: each sensor's
    updated row, y and S against the 80-bit oracle -- env_step from the sensor's site for the az-el-range sensor, the yardstick of
    dim_z = 2 (tests/support/angles_only.py) for the az-el one -- under the criterion, per kind"""
    L, torch = hip.lib, hip.torch
    net, g, launches, refs = uw.network_references(oracle, oracle_ld)
    consts = hip.host.make_consts(g["Q"], net.R[0], uw.ALPHA, uw.BETA, uw.KAPPA, uw.DT, net.lim[0], net.lla[0], propagator=propagator)
    eng = hip.engine.HotPathEngine(consts, uw.NET_M, 1, c2t()[:uw.NET_TIME_ROWS], net.z_noise, history=2)
    sp = net.params()
    assert sp.angles_only == 0b10
    got = [dict(x=[], P=[], y=[], S=[]) for _ in range(net.S)]
    for (tix, state, acts), ref in zip(launches, refs):
        eng.load_state(0, *state)
        eng.status.zero_()
        eng.fail_count.zero_()
        eng.stats.zero_()
        upd = torch.zeros((net.S, L.UPD_STRIDE), dtype=torch.float64, device="cuda")
        eng.launch_step_sensors(0, 1, tix, sp, [int(a) for a in acts], upd.data_ptr(), fast_stats=True, fold_inside=True)
        torch.cuda.synchronize()
        assert int(eng.fail_count.cpu()[0]) == 0 and not eng.status.cpu().numpy().any()
        x, P, rec = eng.x_filter[1].cpu().numpy(), eng.P_filter[1].cpu().numpy(), upd.cpu().numpy()
        for s, j in enumerate(acts):
            assert rec[s, L.UPD_ACTION] == j and rec[s, L.UPD_VISIBLE] == 1 and rec[s, L.UPD_OBS_TAKEN] == 1, (tix, s, j, rec[s, :4])
            d = 2 if net.ang[s] else 3
            y, S = rec[s, L.UPD_Y:L.UPD_Y + 3], rec[s, L.UPD_S:L.UPD_S + 9].reshape(3, 3)
            if net.ang[s]:      # the record's conventions, exactly
                assert y[2] == 0.0 and np.array_equal(S[2], [0.0, 0.0, 1.0]) and np.array_equal(S[:, 2], [0.0, 0.0, 1.0]), (tix, s, y, S)
            for k, v in (("x", x[j]), ("P", P[j]), ("y", y[:d]), ("S", S[:d, :d])):
                got[s][k].append(v)
    for s in range(net.S):
        stack = lambda i: {k: np.array([r[s][i][k] for r in refs]) for k in ("x", "P", "y", "S")}      # noqa: E731
        uw.assert_criterion("network, %s, the %s sensor" % (propagator, "az-el" if net.ang[s] else "az-el-range"),
                            {k: np.array(v) for k, v in got[s].items()}, stack(0), stack(1), innovation=True)
