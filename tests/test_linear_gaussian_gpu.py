"""The fused UKF kernels against closed-form Kalman algebra (tests/support/linear_gaussian.py): with dt = 0 every
propagator is the identity and obs_type 'xyz' measures H x, H = [I 0], so one step is P- = P + Q, S = H B H^T + R, K = B H^T S^-1,
x+ = x + K (z - H x), P+ = P- - K S K^T with B = P (default) or B = P- (SSA_FLAG_RESAMPLE) -- an answer that restates nothing of the
filter.  Every entry that runs the filter is judged against it under the criterion of that module: no further from the closed form than
3 x the float64 oracle is on the same rows, plus 1e-9 sd / sd^2; every figure is printed with its bound before it is asserted.  The
conditions (every update taken, the two forms 1e3 bounds apart, the oracle side) are asserted without a GPU by
tests/test_linear_gaussian_host.py.  Every launch has at most 16 rows."""
import numpy as np
import pytest

from support import linear_gaussian as lg
from support.batches import relnorm
from support.gpu import hip  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

PROPAGATORS = ("fg", "hybrid", "j2", "elements")
VARIANTS = [False, True]
S3 = len(lg.R)


def _name(resample):
    return "resample" if resample else "keep"


def _engine(hip, sc, alpha, propagator="fg", resample=False, covariance="centred", interval=1, obs_limit=lg.OBS_LIMIT, R=lg.R[0], Q=lg.Q,
            noise=None, network=False, history=2, obs_type="xyz", dt=lg.DT):
    """an engine on scene sc with the state in slot 0: one observer (sensor 0's noise table) or, network, the three sensors' tables"""
    consts = hip.host.make_consts(Q, R, alpha, lg.BETA, lg.KAPPA, dt, obs_limit, lg.sites()[0], obs_type=obs_type, propagator=propagator,
                                  resample=resample, update_interval=interval, covariance=covariance)
    if network:
        noise = sc.noise if noise is None else noise
        eng = hip.engine.HotPathEngine(consts, sc.m, sc.E, sc.trans, np.ascontiguousarray(noise), history=history,
                                       zn_stride_env=S3 * lg.N_TIME * sc.m * 3)
    else:
        eng = hip.engine.HotPathEngine(consts, sc.m, sc.E, sc.trans, sc.noise_one(0) if noise is None else noise, history=history)
    eng.load_state(0, sc.xt, sc.x, sc.P)
    return eng


def _sensors(hip, sc, Rs=lg.R, limits=None):
    return hip.host.make_sensor_params(lg.sites(), [lg.OBS_LIMIT] * S3 if limits is None else limits, Rs, lg.N_TIME * sc.m * 3)


def _np(hip, t):
    hip.torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _healthy(hip, eng):
    assert not _np(hip, eng.status).any() and int(_np(hip, eng.fail_count)[0]) == 0


def _record(L, rec, j):
    """y and S of an update record that says the update of object j was taken"""
    assert rec[L.UPD_OBS_TAKEN] == 1.0 and rec[L.UPD_VISIBLE] == 1.0 and rec[L.UPD_ACTION] == j, (j, rec[:4])
    return rec[L.UPD_Y:L.UPD_Y + 3].copy(), rec[L.UPD_S:L.UPD_S + 9].reshape(3, 3).copy()


def _one_step(hip, eng, j, tix, form):
    """one launch of ssa_env_step_f64 from slot 0 to slot 1, the action by the pointer, by value (action=) or in the env words"""
    eng.status.zero_()
    if form == "pointer":
        eng.set_actions([j])
        eng.launch_step(0, 1, tix)
    elif form == "action":
        eng.launch_step(0, 1, tix, action=j)
    else:
        eng.launch_step(0, 1, 0, env_words=([tix], [j]))
    x, P, rec = _np(hip, eng.x_filter[1]), _np(hip, eng.P_filter[1]), _np(hip, eng.upd[1])[0]
    _healthy(hip, eng)
    return x, P, rec


def _step_family(hip, m, alpha, **kw):
    """the launches of lg.STEP_LAUNCHES[m] on the device: (updated rows with y and S, predict-only rows), pooled, and the truth untouched"""
    L = hip.lib
    upd, rest, engines = dict(x=[], P=[], y=[], S=[]), dict(x=[], P=[]), {}
    for n, (k, j) in enumerate(lg.STEP_LAUNCHES[m]):
        sc = lg.scene(m, seed=k)
        if k not in engines:
            engines[k] = _engine(hip, sc, alpha, **kw)
        eng = engines[k]
        x, P, rec = _one_step(hip, eng, j, lg.step_tix(j, k), ("pointer", "action", "words")[n % 3])
        xt = _np(hip, eng.x_true[1])      # (dt = 0: the propagated truth is the truth's bits; through the element chain, 2.8e-14 of |r|, |v|)
        if kw.get("propagator", "fg") != "elements":
            assert np.array_equal(xt, sc.xt)
        else:
            assert max(relnorm(xt, sc.xt, slice(0, 3)).max(), relnorm(xt, sc.xt, slice(3, 6)).max()) < 1e-12
        y, S = _record(L, rec, j)
        for key, v in (("x", x[j]), ("P", P[j]), ("y", y), ("S", S)):
            upd[key].append(v)
        keep = [i for i in range(m) if i != j]
        rest["x"].append(x[keep])
        rest["P"].append(P[keep])
    return {k: np.array(v) for k, v in upd.items()}, ({k: np.concatenate(v) for k, v in rest.items()} if m > 1 else None)


def _judge_steps(hip, oracle, oracle_ld, m, alpha, resample, label, only=None, **kw):
    got, rest = _step_family(hip, m, alpha, resample=resample, **kw)
    cf, f64, _ = lg.step_family(oracle, oracle_ld, m, alpha, resample)
    lg.assert_criterion(label + ", updated rows", got, f64, cf, innovation=only is None, only=only)
    if rest is not None:
        pc, pf, _ = lg.step_family(oracle, oracle_ld, m, alpha, resample, predicted=True)
        lg.assert_criterion(label + ", predict-only rows", rest, pf, pc, only=only)


# ---------------------------------------------------------------------------------------------------------------- ssa_env_step_f64
@pytest.mark.parametrize("propagator", PROPAGATORS)
@pytest.mark.parametrize("resample", VARIANTS)
def test_step(hip, oracle, oracle_ld, resample, propagator):
    """the generic step (xyz never takes the plain form), m = 9 (every object updated in turn, the other eight rows P + Q and x) and
    m = 1, the three ways an action reaches the kernel in rotation; y and S of the record against z - H x- and H B H^T + R.
    alpha = 1 and 1e-3 under the whole criterion; at 1e-4 the covariance (the state printed)"""
    for alpha in lg.ALPHAS + (1e-4,):
        for m in (9, 1):
            _judge_steps(hip, oracle, oracle_ld, m, alpha, resample, "step, %s, %s, alpha %g, m %d" % (propagator, _name(resample), alpha, m),
                         only=("covariance",) if alpha == 1e-4 else None, propagator=propagator)


@pytest.mark.parametrize("propagator", ["hybrid", "elements", "fg"])
@pytest.mark.parametrize("resample", VARIANTS)
def test_step_reference_covariance(hip, oracle, oracle_ld, resample, propagator):
    """SSA_FLAG_REFERENCE_COV, the prior covariance in the reference's own arithmetic, at alpha = 1 (at the small alphas that arithmetic
    is the float64 oracle's cancellation itself and is judged by tests/test_hip_step.py)"""
    _judge_steps(hip, oracle, oracle_ld, 9, 1.0, resample, "step, reference covariance, %s, %s" % (propagator, _name(resample)),
                 propagator=propagator, covariance="reference")


@pytest.mark.parametrize("resample", VARIANTS)
def test_step_skipped_by_the_update_interval_and_hidden_object(hip, oracle, oracle_ld, resample):
    """update_interval = 2: the step at an odd time index updates nobody, the one at an even index does; an object below a control
    obs_limit (+90 degrees: nothing is visible) is not updated either.  Every row of the skipped launches is P + Q, x"""
    L, sc, j = hip.lib, lg.scene(9), 4
    for what, kw, tix in (("interval skips", dict(interval=2), 3), ("interval takes", dict(interval=2), 6), ("hidden", dict(obs_limit=np.pi / 2), 3)):
        eng = _engine(hip, sc, 1.0, resample=resample, **kw)
        x, P, rec = _one_step(hip, eng, j, tix, "pointer")
        hidden = what == "hidden"
        cf, f64, _ = lg.references(oracle, oracle_ld, sc, 0, [[j]], tix, 1.0, resample, update_interval=kw.get("interval", 1), hidden=hidden)
        label = "step, %s, %s" % (what, _name(resample))
        if what == "interval takes":
            assert cf["tasked"] == [(0, 0, j)]
            y, S = _record(L, rec, j)
            lg.assert_criterion(label, dict(x=x[j:j + 1], P=P[j:j + 1], y=y[None], S=S[None]), lg.rows(f64), lg.rows(cf), innovation=True)
        else:
            assert not cf["tasked"] and rec[L.UPD_OBS_TAKEN] == 0.0 and not (hidden and rec[L.UPD_VISIBLE] != 0.0), (label, rec[:4])
            lg.assert_criterion(label, dict(x=x, P=P), lg.rows(f64, predicted=True), lg.rows(cf, predicted=True))


# ---------------------------------------------------------------------------------------------------------------- ssa_env_rollout_f64
def _rollout(hip, sc, alpha, resample, propagator="fg", noise=None, which=lg.ROLLOUT, **kw):
    """a K-step schedule (lg.ROLLOUT) in one launch: (x [K, m, 6], P [K, m, 6, 6] after every step, the K update records)"""
    sched, tix0 = which
    K = len(sched)
    eng = _engine(hip, sc, alpha, propagator=propagator, resample=resample, history=K + 2, noise=noise, **kw)
    eng.launch_rollout(0, tix0, hip.torch.as_tensor(np.array(sched, dtype=np.int32)).cuda())
    x, P, upd = _np(hip, eng.x_filter), _np(hip, eng.P_filter), _np(hip, eng.upd)
    _healthy(hip, eng)
    return x[1:K + 1], P[1:K + 1], upd[1:K + 1, 0]


@pytest.mark.parametrize("propagator", ["fg", "elements"])
@pytest.mark.parametrize("resample", VARIANTS)
def test_rollout(hip, oracle, oracle_ld, resample, propagator):
    """K = 6 steps in one launch, an object revisited and one idle step in each of the three schedules of lg.ROLLOUTS: every step's rows
    against the closed chain (the state carried in long double from step to step), the updated rows with their records; the rows of
    the three launches are judged together; alpha = 1 and 1e-3.  (The first schedule alone, five updated rows: 'elements', keep, alpha
    = 1e-3 gave a velocity figure of 1.4795e-4 sd on the MI355X against 3 x the oracle's 4.909e-5 -- two realisations of the same
    rounding noise; over the fifteen rows the figures are 1.48e-4 and 1.89e-4: DESIGN.md section 4b)"""
    L, sc = hip.lib, lg.scene(9)
    for alpha in lg.ALPHAS:
        parts = []
        for sched, tix0 in lg.ROLLOUTS:
            x, P, upd = _rollout(hip, sc, alpha, resample, propagator, which=(sched, tix0))
            cf, f64, _ = lg.references(oracle, oracle_ld, sc, 0, sched, tix0, alpha, resample)
            got = dict(x=x, P=P, tasked=cf["tasked"], rec={(k, j): dict(zip(("y", "S"), _record(L, upd[k], j))) for k, s, j in cf["tasked"]})
            assert [k for k, r in enumerate(sched) if r[0] < 0] == [k for k in range(len(sched)) if upd[k, L.UPD_OBS_TAKEN] == 0.0]
            parts.append((got, f64, cf))
        label = "rollout, %s, %s, alpha %g" % (propagator, _name(resample), alpha)
        lg.assert_criterion(label + ", updated rows", *(lg.pool([lg.rows(p[i]) for p in parts]) for i in range(3)), innovation=True)
        lg.assert_criterion(label + ", other rows", *(lg.pool([lg.rows(p[i], predicted=True) for p in parts]) for i in range(3)))


@pytest.mark.parametrize("obs_type", ["xyz", "aer"])
def test_covariance_never_reads_the_noise(hip, obs_type):
    """P+ = P- - K S K^T has no innovation in it: under two different noise tables the covariance of every object is the same BITS at
    every step of the rollout up to and including the object's first update, while the updated means are not.  (Past its first update
    an object's sigma points are drawn around a mean that carries the noise: its later covariances depend on it -- through hx and fx
    for 'aer', through the rounding of (x + u) - x in the linear case; lg.first_updates.)  General, not linear: run for 'xyz' at
    dt = 0 and for 'aer' at dt = 20 s"""
    sc = lg.scene(9)
    kw = {} if obs_type == "xyz" else dict(obs_type="aer", dt=20.0, R=np.diag(np.array([4.8e-6, 4.8e-6, 1e3]) ** 2))
    sig = np.array([50.0, 80.0, 20.0]) if obs_type == "xyz" else np.array([4.8e-6, 4.8e-6, 1e3])
    runs = [_rollout(hip, sc, 1.0, False, "fg", noise=np.random.RandomState(seed).normal(size=(1, lg.N_TIME, 9, 3)) * sig, **kw) for seed in (5, 6)]
    (xa, Pa, ua), (xb, Pb, ub) = runs
    first = lg.first_updates(lg.ROLLOUT[0], 9)
    assert sorted(first[first < len(Pa)].tolist()) == [0, 1, 4, 5]
    for j in range(9):
        k = min(int(first[j]), len(Pa) - 1) + 1
        assert np.array_equal(Pa[:k, j].view(np.int64), Pb[:k, j].view(np.int64)), j
    for k, row in enumerate(lg.ROLLOUT[0]):
        if row[0] >= 0:
            assert ua[k, hip.lib.UPD_OBS_TAKEN] == 1.0 and ub[k, hip.lib.UPD_OBS_TAKEN] == 1.0
            assert not np.array_equal(xa[k, row[0]], xb[k, row[0]]), k


# ---------------------------------------------------------------------------------------------------------------- ssa_lookahead_f64
def _gain_err(score, ref):
    """per score column the largest |score - ref| / max(1, |ref|) over the objects"""
    ref = np.asarray(ref).astype(lg.L)
    return (np.abs(np.asarray(score).astype(lg.L) - ref) / np.maximum(1, np.abs(ref))).max(axis=0).astype(np.float64)


def _lookahead_refs(stepper_of, sc, e, h=0, Rs=lg.R[:1]):
    """every object of env e updated hypothetically by each sensor of Rs after h idle steps: dict(x [m, 6], P_prior [m, 6, 6], P_post
    [S, m, 6, 6], gain [S, m, 3] -- formed in long double from that stepper's own P- and P+)"""
    st = stepper_of()
    sl = sc.env(e)
    xt, x, P = sc.xt[sl], sc.x[sl].astype(st.dtype), sc.P[sl].astype(st.dtype)
    for _ in range(h):
        x, P, _r = st.step(xt, x, P, {})
    xp, Pp, _r = st.step(xt, x, P, {})
    out = dict(x=xp, P_prior=Pp, P_post=np.empty((len(Rs), sc.m, 6, 6), dtype=st.dtype), gain=np.empty((len(Rs), sc.m, 3), dtype=lg.L))
    for s, R_ in enumerate(Rs):
        for j in range(sc.m):
            u = stepper_of().step(xt[j:j + 1], x[j:j + 1], P[j:j + 1], {0: (R_, np.zeros(3))})
            out["P_post"][s, j] = u[1][0]
            out["gain"][s, j] = lg.uw.gains_ld(Pp[j], u[1][0])
    return out


def _judge_look(label, got, f64, cf):
    """one lookahead result (x_prior [m, 6], P_prior [m, 6, 6], P_post [S, m, 6, 6], score [S, m, 3]) under the criterion: the prior, every
    sensor's posteriors, and the scores -- within 3 x the float64 oracle's own score error plus 1e-9 max(1, |score|)"""
    lg.assert_criterion(label + ", prior", dict(x=got["x_prior"], P=got["P_prior"]), dict(x=f64["x"], P=f64["P_prior"]), dict(x=cf["x"], P=cf["P_prior"]))
    flat = lambda a: np.asarray(a).reshape(-1, 6, 6)      # noqa: E731
    xs = lambda d, k: np.tile(np.asarray(d[k]), (len(cf["P_post"]), 1))      # noqa: E731
    lg.assert_criterion(label + ", P_post", dict(x=xs(got, "x_prior"), P=flat(got["P_post"])), dict(x=xs(f64, "x"), P=flat(f64["P_post"])),
                        dict(x=xs(cf, "x"), P=flat(cf["P_post"])), only=("covariance",))
    err, ref = _gain_err(got["score"].reshape(-1, 3), cf["gain"].reshape(-1, 3)), _gain_err(f64["gain"].reshape(-1, 3), cf["gain"].reshape(-1, 3))
    bound = lg.FACTOR * ref + 1e-9
    for k, nm in enumerate(("trace gain", "position trace gain", "information gain")):
        print("[linear gaussian] %s: %s under test %.3e, float64 oracle %.3e, bound %.3e" % (label, nm, err[k], ref[k], bound[k]))
    assert np.all(err <= bound), (label, err, bound)
    return bound


@pytest.mark.parametrize("resample", VARIANTS)
def test_lookahead(hip, oracle, oracle_ld, resample):
    """P_prior, P_post and the three scores of every object of m = 9 in one launch against the closed form; the scores at alpha = 1 and
    at alpha = 1e-3 agree with each other to the sum of their bounds (the linear case has one answer for every alpha)"""
    sc, scores, bounds = lg.scene(9), [], []
    cf = _lookahead_refs(lambda: lg.ClosedForm(resample), sc, 0)
    for alpha in lg.ALPHAS:
        eng = _engine(hip, sc, alpha, resample=resample)
        r = eng.launch_lookahead(0, 2, out=hip.engine.HotPathEngine.LOOKAHEAD_PARTS)
        look = {k: _np(hip, v) for k, v in r.items()}
        assert not look["status"].any() and look["visible"].all()
        f64 = _lookahead_refs(lambda: lg.OracleStep(oracle, alpha, resample, False), sc, 0)
        got = dict(x_prior=look["x_prior"], P_prior=look["P_prior"], P_post=look["P_post"][None], score=look["score"][None])
        bounds.append(_judge_look("lookahead, %s, alpha %g" % (_name(resample), alpha), got, f64, cf))
        scores.append(look["score"])
    assert np.all(_gain_err(scores[0], scores[1]) <= bounds[0] + bounds[1]), (_gain_err(scores[0], scores[1]), bounds)


# ---------------------------------------------------------------------------------------------------------------- sensor networks
def _env_rows(sc, e, row):
    """env e's version of a schedule row: env 0 as it stands, env e with every object moved on by e (mod m)"""
    return [int((j + e) % sc.m) if j >= 0 else -1 for j in row]


@pytest.mark.parametrize("entry", ["sensors", "envs"])
@pytest.mark.parametrize("resample", VARIANTS)
def test_step_of_a_sensor_network(hip, oracle, oracle_ld, resample, entry):
    """ssa_env_step_sensors_f64 (one env of 9) and ssa_env_step_sensors_envs_f64 (two envs of 8, the rows by the table and by value):
    three ground sensors with their own R, the three rows of lg.NETWORK as three launches from the same state -- each tasked object
    follows ITS sensor's closed form, the idle sensor's record says so and every other row is P + Q, x"""
    L, torch = hip.lib, hip.torch
    sc = lg.scene(9) if entry == "sensors" else lg.scene(8, E=2)
    sched, tix0 = lg.NETWORK
    for alpha in lg.ALPHAS:
        eng, sp = _engine(hip, sc, alpha, resample=resample, network=True), _sensors(hip, sc)
        got_u, got_p, ref_u, ref_p = [], [], [], []
        for k, row0 in enumerate(sched):
            rows_e = [_env_rows(sc, e, row0) for e in range(sc.E)]
            upd = torch.zeros((sc.E, S3, L.UPD_STRIDE), dtype=torch.float64, device="cuda")
            eng.status.zero_()
            if entry == "sensors":
                eng.launch_step_sensors(0, 1, tix0 + k, sp, rows_e[0], upd.data_ptr(), fast_stats=True, fold_inside=True)
            elif k % 2:
                eng.launch_step_sensors_envs(0, 1, 0, sp, rows_e, upd.data_ptr(), env_words=[tix0 + k] * sc.E, fast_stats=True)
            else:
                eng.launch_step_sensors_envs(0, 1, tix0 + k, sp, rows_e, upd.data_ptr(), fast_stats=True)
            x, P, rec = _np(hip, eng.x_filter[1]), _np(hip, eng.P_filter[1]), _np(hip, upd)
            _healthy(hip, eng)
            for e in range(sc.E):
                refs = lg.references(oracle, oracle_ld, sc, e, [rows_e[e]], tix0 + k, alpha, resample)
                xe, Pe = x[sc.env(e)], P[sc.env(e)]
                got = dict(x=xe[None], P=Pe[None], tasked=refs[0]["tasked"], rec={})
                for s, j in enumerate(rows_e[e]):
                    if j < 0:
                        assert rec[e, s, L.UPD_OBS_TAKEN] == 0.0, (k, e, s, rec[e, s, :4])
                    else:
                        got["rec"][(0, j)] = dict(zip(("y", "S"), _record(L, rec[e, s], j)))
                assert sorted(j for _, _, j in refs[0]["tasked"]) == sorted(j for j in rows_e[e] if j >= 0)
                got_u.append(lg.rows(got))
                got_p.append(lg.rows(got, predicted=True))
                ref_u.append([lg.rows(r) for r in refs])
                ref_p.append([lg.rows(r, predicted=True) for r in refs])
        label = "network step (%s), %s, alpha %g" % (entry, _name(resample), alpha)
        cf, f64 = (lg.pool([r[i] for r in ref_u]) for i in (0, 1))
        lg.assert_criterion(label + ", tasked rows", lg.pool(got_u), f64, cf, innovation=True)
        cf, f64 = (lg.pool([r[i] for r in ref_p]) for i in (0, 1))
        lg.assert_criterion(label + ", other rows", lg.pool(got_p), f64, cf)


@pytest.mark.parametrize("resample", VARIANTS)
def test_lookahead_and_forecast_of_a_sensor_network(hip, oracle, oracle_ld, resample):
    """ssa_lookahead_sensors_f64 and ssa_forecast_sensors_f64 (H = 3) on one env of 9, three sensors: the prior, every sensor's P_post
    and scores of every object at every step of the horizon against the closed chain of idle steps -- a forecast is exact in the linear
    case -- and the forecast's P_post against what REAL steps of lg.NETWORK's rows after h idle steps leave (to the criterion: the
    two launches order their sums differently)"""
    L, torch = hip.lib, hip.torch
    sc, H = lg.scene(9), 3
    sched, tix0 = lg.NETWORK
    idle = [-1] * S3
    for alpha in lg.ALPHAS:
        eng, sp = _engine(hip, sc, alpha, resample=resample, network=True, history=H + 2), _sensors(hip, sc)
        parts = hip.engine.HotPathEngine.LOOKAHEAD_PARTS
        look = {k: _np(hip, v) for k, v in eng.launch_lookahead_sensors(0, tix0, sp, out=parts).items()}
        fore = {k: _np(hip, v) for k, v in eng.launch_forecast_sensors(0, tix0, sp, H, out=parts).items()}
        assert not look["status"].any() and look["visible"].all() and not fore["status"].any() and fore["visible"].all()
        for h in range(H):
            cf = _lookahead_refs(lambda: lg.ClosedForm(resample), sc, 0, h, lg.R)
            f64 = _lookahead_refs(lambda: lg.OracleStep(oracle, alpha, resample, False), sc, 0, h, lg.R)
            label = "%s, alpha %g" % (_name(resample), alpha)
            if h == 0:
                _judge_look("network lookahead, " + label, dict(x_prior=look["x_prior"], P_prior=look["P_prior"], P_post=look["P_post"], score=look["score"]), f64, cf)
            _judge_look("network forecast, step %d, %s" % (h, label),
                        dict(x_prior=fore["x_prior"][h], P_prior=fore["P_prior"][h], P_post=fore["P_post"][h], score=fore["score"][h]), f64, cf)
            # real steps: h idle ones, then row h of the schedule
            real = np.array([idle] * h + [sched[h]], dtype=np.int32)
            eng.status.zero_()
            eng.launch_rollout_sensors(0, tix0, sp, torch.as_tensor(real).cuda())
            P_real = _np(hip, eng.P_filter[h + 1])
            _healthy(hip, eng)
            for s, j in enumerate(sched[h]):
                if j >= 0:
                    sd = np.sqrt(np.diag(cf["P_post"][s, j]).astype(np.float64))
                    d = np.abs(P_real[j] - fore["P_post"][h, s, j]) / np.outer(sd, sd)
                    own = lg.errs_sd(dict(x=sc.x[j:j + 1], P=f64["P_post"][s, j][None]), dict(x=sc.x[j:j + 1].astype(lg.L), P=cf["P_post"][s, j][None]))[2][0]
                    assert d.max() <= 2 * (lg.FACTOR * own + lg.SLACK[2]), (label, h, s, j, d.max(), own)


# ---------------------------------------------------------------------------------------------------------------- controls
CONTROLS = {"R (1 + 1e-6)": (dict(R=lg.R[0] * (1 + 1e-6)), "covariance"), "Q (1 + 1e-3)": (dict(Q=lg.Q * (1 + 1e-3)), "covariance"),
            "noise (1 + 1e-6)": (dict(noise_scale=1 + 1e-6), "position"), "the other variant": (dict(flip=True), "covariance")}


@pytest.mark.parametrize("control", list(CONTROLS))
@pytest.mark.parametrize("resample", VARIANTS)
def test_a_wrong_input_fails_on_the_device(hip, oracle, oracle_ld, resample, control):
    """the m = 9 launches of test_step at alpha = 1 with ONE input of the launch wrong -- R or the noise table off by 1e-6, Q by 1e-3,
    the resample flag flipped -- judged against the unaltered closed form: the quantity that input reaches lies beyond its bound (Q
    and the flag: on the predict-only rows or the updated ones by a wide margin).  No rebuild, no altered kernel"""
    kw, quantity = CONTROLS[control]
    kw = dict(kw)
    flip, scale = kw.pop("flip", False), kw.pop("noise_scale", None)
    if scale is not None:
        kw["noise"] = lg.scene(9).noise_one(0) * scale
    got, rest = _step_family(hip, 9, 1.0, resample=resample != flip, **kw)
    cf, f64, _ = lg.step_family(oracle, oracle_ld, 9, 1.0, resample)
    bad = dict(lg.fails(got, f64, cf))
    print("[linear gaussian] control %s, %s: beyond the bound by %s" % (control, _name(resample), bad))
    assert bad.get(quantity, 0.0) > (1e3 if flip else 3.0), (control, bad)
    with pytest.raises(AssertionError):
        lg.assert_criterion("control " + control, got, f64, cf, innovation=True)
    if control.startswith("Q"):
        pc, pf, _ = lg.step_family(oracle, oracle_ld, 9, 1.0, resample, predicted=True)
        assert dict(lg.fails(rest, pf, pc)).get("covariance", 0.0) > 3.0
