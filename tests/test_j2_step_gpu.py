"""SSA_PROP_J2_RK4 on the GPU against the 80-bit RK4 yardstick (oracle/j2_reference.py; pinned without a GPU by tests/test_j2_host.py,
which also shows that the criteria used here reject a propagator that is subtly wrong): the operator ssa_propagate_j2_f64 under the
shared body of support/devmath.py at ragged sizes and with constants of its own, its refusals; the fused step (launch_step,
propagator='j2') -- truth row, predict-only rows, the updated row, y and S -- at 8 objects (two tiles; 6: a ragged one); the constants
of ssa_consts reaching the kernel; and the 'predict returned nan' path of the PROP == 2 instance next to the fg instance's."""
import numpy as np
import pytest

import j2_reference as J
from support import j2 as sj
from support.batches import c2t, make_batch
from support.devmath import J2_CASES, assert_j2_criterion, j2_nonfinite_rows, j2_pool
from support.gpu import hip  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

N_TIME = 17          # rows of the GCRS -> ITRS table and of the noise table: launches at rows 1 .. 16
LAUNCHES = 16
MASK = np.radians(15.0)
SIG = np.array([4.8e-6, 4.8e-6, 1e3])


# ---------------------------------------------------------------------------------------------------------------- a) the operator
def _operator(hip, j2=J.J2_EARTH, r_eq=J.R_EQ_EARTH):
    return lambda x, dt, nsub: hip.dev.propagate_j2(hip.dev.as_dev(np.array(x, order="C")), dt, j2, r_eq, nsub).cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 65, 476])
def test_propagate_j2_operator_vs_80bit(hip, n):
    """ssa_propagate_j2_f64 on the first n rows of the pool -- one lane, a block less one, a block and one, and the whole pool with its
    ragged last block (the polar, equatorial, GEO, on-axis, high-e and hyperbolic rows are its last 28) -- at every (dt, nsub)"""
    assert_j2_criterion(_operator(hip), "ssa_propagate_j2_f64", rows=slice(0, n))
    x = j2_pool()[:n]
    y = _operator(hip)(x, 0.0, 4)
    assert np.array_equal(y.view(np.uint64), np.ascontiguousarray(x).view(np.uint64))      # dt = 0: the input's bits


def test_propagate_j2_operator_takes_its_own_constants(hip):
    """2 x J2 and r_eq = 6.0e6 against the yardstick with the same values; the two sets of constants do not give the same states"""
    assert_j2_criterion(_operator(hip, 2 * J.J2_EARTH, 6.0e6), "2 J2, r_eq 6.0e6", cases=J2_CASES[:4], j2=2 * J.J2_EARTH, r_eq=6.0e6)
    with pytest.raises(AssertionError):
        assert_j2_criterion(_operator(hip), "default constants", cases=J2_CASES[:1], j2=2 * J.J2_EARTH, r_eq=6.0e6)


def test_propagate_j2_operator_nonfinite_rows(hip):
    """a NaN velocity component, r = 0, an infinite coordinate: NaN in every component, the neighbours' bits their own"""
    xb, bad = j2_nonfinite_rows()
    for dt, nsub in ((20.0, 4), (20.0, 1), (-20.0, 4)):
        y = _operator(hip)(xb, dt, nsub)
        assert np.isnan(y[bad]).all() and np.isfinite(y[~bad]).all(), (dt, nsub, y)
        assert np.array_equal(y[~bad].view(np.uint64), _operator(hip)(xb[~bad], dt, nsub).view(np.uint64)), (dt, nsub)


def test_propagate_j2_operator_refusals(hip):
    lib, L, torch = hip.lib.load(), hip.lib, hip.torch
    x = hip.dev.as_dev(np.array(j2_pool()[:4], order="C"))
    out = torch.full_like(x, -1.0)
    call = lambda xi, xo, n, nsub: lib.ssa_propagate_j2_f64(xi, xo, n, 20.0, J.J2_EARTH, J.R_EQ_EARTH, nsub, None)      # noqa: E731
    px, po = x.data_ptr(), out.data_ptr()
    for args in ((px, po, 4, 0), (px, po, 4, 4097), (px, po, 4, -1), (None, po, 4, 4), (px, None, 4, 4), (px, po, -1, 4)):
        assert call(*args) == L.E_INVALID, args
    assert call(px, po, 0, 4) == 0 and call(None, None, 0, 0) == 0
    torch.cuda.synchronize()
    assert (out == -1.0).all()                      # nothing was launched
    assert call(px, po, 4, 4096) == 0            # the largest count the entry takes
    torch.cuda.synchronize()
    assert np.isfinite(out.cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------------------------- b) the fused step
def _engine(hip, m, alpha, resample, dt=sj.DT, **consts_kw):
    g = make_batch(1, seed=0)[3]
    consts = hip.host.make_consts(g["Q"], g["R"], alpha, 2.0, -3, dt, MASK, g["obs_lla"], propagator='j2', resample=resample, **consts_kw)
    zn = np.random.RandomState(77 + m).normal(size=(1, N_TIME, m, 3)) * SIG
    return hip.engine.HotPathEngine(consts, m, 1, c2t()[:N_TIME], zn, history=2), consts, zn, g


def _launch(hip, eng, state, tix, action):
    """one step from `state` (slot 0 -> slot 1) at time row tix; everything it leaves, as numpy"""
    eng.load_state(0, *state)
    eng.status.zero_()
    eng.fail_count.zero_()
    eng.set_actions([action])
    eng.launch_step(0, 1, tix)
    hip.torch.cuda.synchronize()
    return dict(x=eng.x_filter[1].cpu().numpy(), P=eng.P_filter[1].cpu().numpy(), xt=eng.x_true[1].cpu().numpy(), obs=eng.obs[1].cpu().numpy(),
                metrics=eng.metrics[1].cpu().numpy(), st=eng.status.cpu().numpy(), upd=eng.upd[1].cpu().numpy()[0],
                n_failed=eng.stats[1].cpu().numpy()[0, hip.lib.STAT_N_FAILED], fails=int(eng.fail_count.cpu()[0]))


def _judge(hip, oracle, oracle_ld, label, m, alpha, resample, launches, dt=sj.DT, judge=("state", "innovation"), far=(1e7, 3e7), **consts_kw):
    """`launches` steps, each from a fresh scene at its own time row, object k % m tasked.  judge 'state': the truth rows under the
    operator criterion, the m - 1 predict-only rows and the updated row under the filter criterion; 'innovation': y and S of every
    update within 1e-3 / 1e-2 innovation sd of the 80-bit ones.  Either way: status 0 everywhere, every update taken, no filter
    failing in either arithmetic; no object is left out; both sides' figures are printed before anything is judged"""
    L = hip.lib
    eng, consts, zn, g = _engine(hip, m, alpha, resample, dt, **consts_kw)
    nsub, j2, r_eq = consts.rk4_substeps, consts.j2, consts.r_eq
    lla, itrs = g["obs_lla"], g["obs_itrs"]
    G, Rf = {"predict": [], "update": []}, {"predict": [], "update": []}
    xt_in, xt_out, inn = [], [], []
    for k in range(launches):
        tix = 1 + k
        M = c2t()[tix]
        state = sj.scene(lla, itrs, MASK, M, m, 7000 * m + 31 * k + int(round(alpha * 1e5)), dt, nsub, j2, r_eq, far=far)
        act = k % m
        dev = _launch(hip, eng, state, tix, act)
        assert dev["fails"] == 0 and not dev["st"].any() and dev["n_failed"] == 0, (label, k, dev["st"])
        assert dev["upd"][L.UPD_OBS_TAKEN] == 1 and dev["upd"][L.UPD_ACTION] == act and dev["upd"][L.UPD_VISIBLE] == 1, (label, k, dev["upd"][:4])
        xt_in.append(state[0])
        xt_out.append(dev["xt"])
        xt, x, P = state
        for j in range(m):
            pf = sj.predict_reference(oracle, x[j], P[j], g["Q"], dt, alpha, nsub, j2, r_eq, ld=False)
            pl = sj.predict_reference(oracle, x[j], P[j], g["Q"], dt, alpha, nsub, j2, r_eq, ld=True)
            kind = "predict"
            if j == act:
                kind = "update"
                refs = []
                for o, p, ld in ((oracle, pf, False), (oracle_ld, pl, True)):
                    T = np.longdouble if ld else np.float64
                    zt = o.hx_aer(J.rk4_j2(xt[j], dt, nsub, j2, r_eq, T).astype(np.float64), M, lla, itrs)[0]
                    assert zt[1] >= MASK + np.radians(5.0), (label, k, zt)      # (visible in the restatement too, far from the mask)
                    refs.append(sj.update_reference(o, p, zt + zn[0, tix, j], g["R"], M, lla, itrs, resample, ld))
                pf, pl = refs
                y, S = dev["upd"][L.UPD_Y:L.UPD_Y + 3], dev["upd"][L.UPD_S:L.UPD_S + 9].reshape(3, 3)
                Sd = np.sqrt(np.diag(pl["S"]))
                inn.append([np.max(np.abs(y - pl["y"]) / Sd), np.max(np.abs(S - pl["S"]) / np.outer(Sd, Sd)),
                            np.max(np.abs(pf["y"] - pl["y"]) / Sd), np.max(np.abs(pf["S"] - pl["S"]) / np.outer(Sd, Sd))])
            G[kind].append(sj.distances({"x": dev["x"][j], "P": dev["P"][j]}, pl))
            Rf[kind].append(sj.distances(pf, pl))
    inn = np.array(inn)
    assert len(inn) == len(G["update"]) == launches and len(G["predict"]) == launches * (m - 1)
    print("[j2 step innovation] %s: %d updates; vs 80-bit in innovation sd, kernel y max %.2e median %.2e S max %.2e; float64 oracle y max "
          "%.2e median %.2e S max %.2e" % (label, launches, inn[:, 0].max(), np.median(inn[:, 0]), inn[:, 1].max(), inn[:, 2].max(),
                                           np.median(inn[:, 2]), inn[:, 3].max()))
    if "state" in judge:
        sj.assert_truth_criterion(np.concatenate(xt_out), np.concatenate(xt_in), dt, nsub, j2, r_eq, label)
        for kind in ("predict", "update"):
            sj.assert_filter_criterion(G[kind], Rf[kind], "%s, %s rows" % (label, kind))
    if "innovation" in judge:
        # (a condition of the test: the reference arithmetic itself resolves the bound on this scene)
        assert inn[:, 2].max() < 1e-3 and inn[:, 3].max() < 1e-2, (label, "the float64 oracle", inn[:, 2].max(), inn[:, 3].max())
        assert inn[:, 0].max() < 1e-3 and inn[:, 1].max() < 1e-2, (label, int(np.argmax(inn[:, 0])), inn[:, 0].max(), inn[:, 1].max())
    return np.concatenate(xt_in), consts


@pytest.mark.parametrize("m", [8, 6])
@pytest.mark.parametrize("resample", [False, True])
@pytest.mark.parametrize("alpha", [1e-3, 1e-4])
def test_j2_step_against_the_yardstick(hip, oracle, oracle_ld, alpha, resample, m):
    """truth, x-, P- of the predict-only rows, x+, P+ of the updated row: 16 launches at time rows 1 .. 16"""
    _judge(hip, oracle, oracle_ld, "alpha %.0e resample=%s m=%d" % (alpha, resample, m), m, alpha, resample, LAUNCHES, judge=("state",))


@pytest.mark.parametrize("m", [8, 6])
@pytest.mark.parametrize("resample", [False, True])
@pytest.mark.parametrize("alpha", [1e-3, 1e-4])
def test_j2_step_innovation_against_the_80bit_values(hip, oracle, oracle_ld, alpha, resample, m):
    """y and S of 16 updates within 1e-3 / 1e-2 innovation sd of the 80-bit ones, the bounds of tests/test_angles_only_gpu.py (which
    runs at alpha = 1e-3 only).  The scene: at alpha = 1e-3 the one of test_j2_step_against_the_yardstick; at alpha = 1e-4 every object
    800 .. 2 200 km from the site (below 9 000 km from the centre).  Why: the prior mean and the predicted measurement are sums of
    thirteen vectors with weights Wm[i] = 1 / (6 alpha^2) = 1.7e7 at alpha = 1e-4, so a few ulps of one term are |x| . 2e-16 . 1.7e7 .
    sqrt(12) in the sum -- 0.1 m at |x| = 8e6 m, 0.4 m at 3.5e7 m, per ulp -- against an innovation sd of 1.4 km in range and 1 km /
    range in angle: the floor of float64 in y grows with |x| / alpha^2 whatever the order of summation.  Measured on the CPU, the
    float64 oracle's own y against the 80-bit one, largest of 48 updates at alpha = 1e-4: 3.9e-4 sd at 800 .. 2 200 km, 1.2e-3 at
    2 500 .. 10 000 km, 3.7e-3 at 10 000 .. 30 000 km.  Beyond 2 200 km the bound lies inside the noise of the number format and
    judges no kernel (there the MI355X's y is 1.29e-3, the float64 oracle's 2.38e-3); the test asserts that the float64 oracle itself
    meets the bound on every update it judges.  x+ and P+ of the far objects at alpha = 1e-4 stay judged, relative to the float64
    floor, by test_j2_step_against_the_yardstick."""
    far = (1e7, 3e7) if alpha >= 1e-3 else None
    _judge(hip, oracle, oracle_ld, "alpha %.0e resample=%s m=%d" % (alpha, resample, m), m, alpha, resample, LAUNCHES, judge=("innovation",), far=far)


# ---------------------------------------------------------------------------------------------------------------- c) the constants
@pytest.mark.parametrize("case", ["rk4_substeps=2", "dt=30", "2 J2, r_eq 6.0e6"])
def test_j2_step_constants_reach_the_kernel(hip, oracle, oracle_ld, case):
    """ssa_consts.rk4_substeps, .dt (and the default count that follows from it) and .j2 / .r_eq: each against the yardstick with its
    own values, under the criteria of the test above.  The comparison cannot pass by ignoring the field: on the rows below 9 000 km the
    80-bit truths with 2 and with 4 sub-steps (with 6 and with 4 over 30 s; with the two sets of constants) differ by more than 100 x
    the bound."""
    kw, dt = {"rk4_substeps=2": (dict(rk4_substeps=2), 20.0), "dt=30": ({}, 30.0),
              "2 J2, r_eq 6.0e6": (dict(j2=2 * J.J2_EARTH, r_eq=6.0e6), 20.0)}[case]
    xt, consts = _judge(hip, oracle, oracle_ld, case, 8, 1e-3, False, 4, dt=dt, **kw)
    assert (consts.rk4_substeps, consts.dt) == {"rk4_substeps=2": (2, 20.0), "dt=30": (6, 30.0), "2 J2, r_eq 6.0e6": (4, 20.0)}[case]
    from support.devmath import J2_SLACK, _relnorm_ld
    leo = np.linalg.norm(xt[:, :3], axis=1) < 9e6
    assert leo.sum() >= len(xt) // 2
    mine = J.rk4_j2(xt[leo], dt, consts.rk4_substeps, consts.j2, consts.r_eq, np.longdouble)
    other = J.rk4_j2(xt[leo], dt, 4, J.J2_EARTH, J.R_EQ_EARTH, np.longdouble)      # what a kernel that ignores the field computes
    f64 = J.rk4_j2(xt[leo], dt, consts.rk4_substeps, consts.j2, consts.r_eq, np.float64)
    bound = 3 * _relnorm_ld(f64, mine, slice(0, 3)).max() + J2_SLACK
    gap = _relnorm_ld(other.astype(np.float64), mine, slice(0, 3))
    print("[j2 step constants] %s: the defaults' truth is %.2e .. %.2e away on the rows below 9 000 km, the bound is %.2e" % (case, gap.min(), gap.max(), bound))
    assert gap.min() > 100 * bound, (case, gap.min(), bound)


# ---------------------------------------------------------------------------------------------------------------- d) the failure path
@pytest.mark.parametrize("tasked", ["another object", "the object itself"])
@pytest.mark.parametrize("what", ["filter", "truth"])
def test_j2_step_nan_input_fails_one_object_alone(hip, oracle, what, tasked):
    """one NaN component in a filter state (object 1, velocity) or in a true state (object 5, position), ordinary inputs: the object's
    status, sentinels, record, failure count and statistics word are those the fg instance gives from the same inputs; every other
    object of its tile and of the batch is bit-identical to the clean run"""
    L, m = hip.lib, 8
    bad = 1 if what == "filter" else 5
    act = bad if tasked == "the object itself" else (2 if what == "filter" else 6)      # (the other one: in the bad object's tile)
    g = make_batch(1, seed=0)[3]
    tix = 3
    clean = sj.scene(g["obs_lla"], g["obs_itrs"], MASK, c2t()[tix], m, 4242)
    state = tuple(a.copy() for a in clean)
    state[1 if what == "filter" else 0][bad, 4 if what == "filter" else 1] = np.nan
    out = {}
    for prop in ("j2", "fg"):
        consts = hip.host.make_consts(g["Q"], g["R"], 1e-3, 2.0, -3, sj.DT, MASK, g["obs_lla"], propagator=prop)
        zn = np.random.RandomState(5).normal(size=(1, N_TIME, m, 3)) * SIG
        eng = hip.engine.HotPathEngine(consts, m, 1, c2t()[:N_TIME], zn, history=2)
        out[prop] = _launch(hip, eng, state, tix, act)
        if prop == "j2":
            ref = _launch(hip, eng, clean, tix, act)
    a, b = out["j2"], out["fg"]
    assert np.array_equal(a["st"], b["st"]) and a["fails"] == b["fails"] and a["n_failed"] == b["n_failed"], (a["st"], b["st"], a["fails"], b["fails"])
    for k in ("x", "P", "xt"):      # the bad object: sentinels and NaN where the fg instance has them, and the same ones
        assert np.array_equal(np.isnan(a[k][bad]), np.isnan(b[k][bad])), k
        s = (a[k][bad] == b[k][bad]) & (np.abs(b[k][bad]) >= 1e12)
        assert np.array_equal(s, np.abs(b[k][bad]) >= 1e12), k
    assert np.array_equal(a["upd"][[L.UPD_OBS_TAKEN, L.UPD_VISIBLE, L.UPD_ACTION]], b["upd"][[L.UPD_OBS_TAKEN, L.UPD_VISIBLE, L.UPD_ACTION]])
    if what == "filter":
        assert a["st"][bad] == L.ST_PREDICT_NAN and a["fails"] == 1 and a["n_failed"] == 1
        assert np.array_equal(a["x"][bad], hip.host.X_FAILED) and np.array_equal(a["P"][bad], hip.host.P_FAILED)
        assert np.isfinite(a["xt"][bad]).all()
    else:
        assert np.isnan(a["xt"][bad]).all()
    others = np.arange(m) != bad
    assert not a["st"][others].any() and not ref["st"].any()
    for k in ("x", "P", "xt", "obs"):
        assert np.array_equal(a[k][others].view(np.int64), ref[k][others].view(np.int64)), (what, tasked, k)
    assert np.array_equal(a["metrics"][..., others].view(np.int64), ref["metrics"][..., others].view(np.int64))
    if tasked == "another object":
        assert np.array_equal(a["upd"].view(np.int64), ref["upd"].view(np.int64)) and a["upd"][L.UPD_OBS_TAKEN] == 1
