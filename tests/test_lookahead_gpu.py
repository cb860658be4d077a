"""One-step tasking lookahead on the MI355X (include/ssa_hip.h: ssa_lookahead_f64; SSA_Tasker_Env.lookahead, the vector env's,
agents.agent_info_gain / agent_trace_gain).

The ground truth is the project's own step: a step reads history slot i and writes slot i + 1, so re-launching it with another action
only needs the status words (and the failure counter) saved and restored.  For every sampled object j, P_post[j] must be
bit-identical to P_filter[i + 1, j] after the step with action j, x_prior / P_prior bit-identical to what that step leaves for every
OTHER object, and status / visible equal to the step's status word and update record."""
import numpy as np
import pytest

from support.batches import c2t, errs, make_batch
from support.gpu import envs  # noqa: F401  (the module fixture)
from support.lookahead import _bits, _look_np, cfg1, check_against_step, xyz1

pytestmark = pytest.mark.gpu


def test_bit_identical_to_step_hybrid_20000_early_and_late(envs):
    """the default 'hybrid' env at 20 000 objects: an early step, and a late one (>= 300) where filters are diverging"""
    env = envs.make(config=cfg1(envs, rso_count=20000, seed=1))
    env.step(5)
    env.step(17)
    check_against_step(env, n=64, seed=1)
    env.run_agent('agent_visible_greedy', 310 - env.i)
    assert env.i >= 300
    _, seen = check_against_step(env, n=96, seed=2)
    assert seen["visible"] and seen["hidden"]
    assert seen["failed"], "late in the episode some filters have failed"


@pytest.mark.parametrize("variant", ["fg", "elements", "j2", "xyz", "resample"])
def test_bit_identical_to_step_variants(envs, variant):
    from ssa_gym_amd.envs import dynamics as D
    over = {"fg": dict(fx=D.fx_xyz_farnocchia_fg), "elements": dict(fx=D.fx_xyz_farnocchia_elements), "j2": dict(fx=D.fx_xyz_j2_rk4),
            "xyz": xyz1(envs), "resample": dict(resample_sigmas=True)}[variant]
    env = envs.make(config=cfg1(envs, seed=11, **over))
    env.step(3)
    check_against_step(env, n=64, seed=3)
    env.run_agent('agent_visible_greedy', 200)
    check_against_step(env, n=64, seed=4)


def test_update_interval_update_and_skipped_step(envs):
    from ssa_gym_amd import _lib
    env = envs.make(config=cfg1(envs, seed=12, update_interval=3))
    env.step(1)                                   # i = 1: the next step (2) is skipped by the interval
    look, _ = check_against_step(env, n=64, seed=5)
    assert not look["visible"].any() and np.isnan(look["score"]).all()
    assert np.array_equal(look["P_post"].view(np.int64), look["P_prior"].view(np.int64))
    env.step(2)                                   # i = 2: the next step (3) updates
    look, seen = check_against_step(env, n=64, seed=6)
    assert seen["visible"] > 0 and np.isfinite(look["score"][_lib.LOOK_INFO_GAIN]).any()


def test_no_side_effects_on_an_episode(envs):
    """one episode of 120 steps with lookahead() before every step and the same episode without: bit-identical"""
    import torch
    cfg = cfg1(envs, seed=21, steps=130)
    a, b = envs.make(config=cfg), envs.make(config=cfg)
    rs = np.random.RandomState(4)
    acts = rs.randint(0, cfg['rso_count'], 120)
    ra, rb = [], []
    for k in range(120):
        a.lookahead(covariances=bool(k % 2))
        a.lookahead()
        oa = a.step(int(acts[k]))
        ob = b.step(int(acts[k]))
        ra.append(oa[1])
        rb.append(ob[1])
        assert np.array_equal(oa[0], ob[0])
    assert np.array_equal(np.asarray(ra), np.asarray(rb))
    ea, eb = a._engine, b._engine
    for x, y in ((ea.x_true, eb.x_true), (ea.x_filter, eb.x_filter), (ea.P_filter, eb.P_filter), (ea.obs, eb.obs)):
        assert torch.equal(_bits(x), _bits(y))
    assert torch.equal(ea.status, eb.status) and torch.equal(ea.fail_count, eb.fail_count)
    assert a.failed_filters_id == b.failed_filters_id
    assert np.array_equal(ea.fail_log, eb.fail_log)


def test_against_the_oracle(envs, oracle, oracle_ld):
    """P+ of every object against oracle.ukf_predict + ukf_update on the update parity tests' batch and arguments (tests/test_hip_step.py:
    make_batch, SSA_PROP_FG, alpha = 1e-3), with the criteria of that module's check_parity.  The prior mean is held to criterion (1)
    (within 1e-6 of the reference value).  P+ = P- - K S K^T is a cancellation whose fp64 rounding noise is amplified far beyond 1e-5
    (the reference arithmetic's own P+ is within 0.5 x 1e-5 of the exact value on 1.7 % of this batch, measured oracle-only), so the
    strict criterion (1) does not apply to it: every rounding of the chain shows.  It is held to criterion (2) -- as close to the exact
    value as the reference arithmetic, on every object (factor 3 on median and maximum), as check_parity applies it."""
    import torch
    import oracle as orc
    from ssa_gym_amd import engine, host
    m, alpha, tix = 2000, 1e-3, 1
    xt, x, P, g = make_batch(m, seed=1)
    consts = host.make_consts(g["Q"], g["R"], alpha, 2.0, -3, 20.0, -np.pi / 2, g["obs_lla"], propagator='fg')
    eng = engine.HotPathEngine(consts, m, 1, c2t(), np.zeros((1, 480, m, 3)), history=2)
    eng.load_state(0, xt, x, P)
    r = eng.launch_lookahead(0, tix, out=engine.HotPathEngine.LOOKAHEAD_PARTS)
    torch.cuda.synchronize()
    look = {k: v.cpu().numpy() for k, v in r.items()}
    assert np.all(look["status"] == 0) and np.all(look["visible"] == 1)
    Wm, Wc, scale = orc.merwe_weights(alpha, 2.0, -3)
    res = {}
    for name, o, centred in (("f64", oracle, False), ("ld", oracle_ld, True)):
        xs, Ps = np.empty((m, 6)), np.empty((m, 6, 6))
        for j in range(m):
            rc, xp, Pp, sf = o.ukf_predict(x[j], P[j], g["Q"], 20.0, Wm, Wc, scale, centred=centred)
            rc2, _, Pu, _, _, _ = o.ukf_update(xp, Pp, sf, np.zeros(3), g["R"], Wm, Wc, scale, c2t()[tix], g["obs_lla"], g["obs_itrs"],
                                               obs_type=0, centred=centred)
            assert rc == 0 and rc2 == 0
            xs[j], Ps[j] = xp, Pu
        res[name] = {"x": xs, "P": Ps}
    gpu = {"x": look["x_prior"], "P": look["P_post"]}
    ep, ev, _ = errs(gpu, res["f64"])
    rp, rv, rP = errs(res["f64"], res["ld"])
    gp, gv, gP = errs(gpu, res["ld"])
    well = (rp < 0.5e-6) & (rv < 0.5e-6)
    print("[lookahead vs oracle] prior mean: %.4f of objects compared strictly, max |gpu-ref| pos %.2e vel %.2e; P+ vs exact: gpu median "
          "%.2e max %.2e, reference arithmetic median %.2e max %.2e" % (well.mean(), ep[well].max(), ev[well].max(), np.median(gP), gP.max(),
                                                                     np.median(rP), rP.max()))
    assert well.mean() >= 0.99 and (ep[well] < 1e-6).all() and (ev[well] < 1e-6).all()
    for g_, r_ in ((gp, rp), (gv, rv), (gP, rP)):
        assert np.median(g_) <= 3 * np.median(r_) + 1e-13
        assert g_.max() <= 3 * r_.max() + 1e-12


def test_scores_from_the_returned_covariances(envs):
    """the three scores recomputed from the returned P_prior / P_post (numpy, slogdet) late in an episode; NaN where the update would not
    run.  The information gain is also NaN where the plain Cholesky factorisation of P- or P+ fails (a covariance that is not positive
    definite in fp64 -- diverged filters), as agent_shannon's log-det ratio is"""
    from ssa_gym_amd import _lib
    env = envs.make(config=cfg1(envs, rso_count=20000, seed=41))
    env.run_agent('agent_visible_greedy', 320)
    look = _look_np(env)
    ok = (look["status"] == 0) & (look["visible"] == 1)
    assert ok.any() and (~ok).any()
    sc = look["score"]
    assert np.isnan(sc[:, ~ok]).all()
    assert np.isfinite(sc[_lib.LOOK_TRACE_GAIN, ok]).all() and np.isfinite(sc[_lib.LOOK_POS_TRACE_GAIN, ok]).all()
    Pm, Pp = look["P_prior"][ok], look["P_post"][ok]
    tr = np.trace(Pm, axis1=1, axis2=2) - np.trace(Pp, axis1=1, axis2=2)
    trp = np.trace(Pm[:, :3, :3], axis1=1, axis2=2) - np.trace(Pp[:, :3, :3], axis1=1, axis2=2)
    scale = np.trace(Pm, axis1=1, axis2=2)       # (a trace difference is a cancellation: relative to the traces it came from)
    assert np.all(np.abs(sc[_lib.LOOK_TRACE_GAIN, ok] - tr) <= 1e-9 * scale)
    assert np.all(np.abs(sc[_lib.LOOK_POS_TRACE_GAIN, ok] - trp) <= 1e-9 * scale)
    ig_dev = sc[_lib.LOOK_INFO_GAIN, ok]
    fin = np.isfinite(ig_dev)
    print("[lookahead scores] %d objects an update would reach, information gain finite on %d" % (ok.sum(), fin.sum()))
    assert fin.mean() > 0.5
    sm, sp = np.linalg.slogdet(Pm[fin]), np.linalg.slogdet(Pp[fin])
    assert (sm[0] > 0).all() and (sp[0] > 0).all()
    ig = 0.5 * (sm[1] - sp[1])
    ld = np.abs(sm[1]) + np.abs(sp[1])
    err = np.abs(ig_dev[fin] - ig) / np.maximum(np.abs(ig), ld)
    # (a log-det is defined to ~cond(P) eps, and late in an episode the posterior covariances of diverged filters are ill-conditioned:
    # 1e-9 relative where both matrices are conditioned better than 1e8, the rounding level of the factorisation elsewhere)
    cond = np.maximum(np.linalg.cond(Pm[fin]), np.linalg.cond(Pp[fin]))
    well = cond < 1e8
    print("[lookahead scores] info gain vs slogdet: max rel %.2e over %d objects; %.2e over the %d with cond < 1e8"
          % (err.max(), fin.sum(), err[well].max() if well.any() else 0.0, well.sum()))
    assert np.all(err[well] <= 1e-9)
    assert np.all(err <= 1e-9 + 1e-16 * cond)
    # where it is NaN, one of the two matrices has no Cholesky factor in fp64 (numpy's LAPACK agrees on all but rounding-level cases)
    nf = 0
    for a_, b_ in zip(Pm[~fin], Pp[~fin]):
        try:
            np.linalg.cholesky(a_), np.linalg.cholesky(b_)
        except np.linalg.LinAlgError:
            nf += 1
    print("[lookahead scores] NaN information gains: %d, of them numpy's Cholesky fails too on %d" % ((~fin).sum(), nf))


def test_layout_and_vector_env(envs):
    """a storage layout never shows; each env of a vector env equals a single env with the same state"""
    import torch
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    cfg = cfg1(envs, seed=51)
    plain, lay = envs.make(config=cfg), envs.make(config=dict(cfg, storage_layout='regime'))
    acts = np.random.RandomState(5).randint(0, cfg['rso_count'], 40)
    for a in acts:
        plain.step(int(a))
        lay.step(int(a))
    assert lay._engine._order is not None
    lp, ll = _look_np(plain), _look_np(lay)
    for k in lp:
        assert np.array_equal(lp[k].view(np.uint8), ll[k].view(np.uint8)), k
    for layout in (None, 'regime'):
        vcfg = dict(cfg, storage_layout=layout)
        vec = SSA_Tasker_VecEnv(vcfg, 8, seed=7)
        rs = np.random.RandomState(9)
        for _ in range(30):
            vec.step(rs.randint(0, vcfg['rso_count'], 8))
        lv = {k: v.cpu().numpy().copy() for k, v in vec.lookahead(covariances=True).items()}
        for ev in range(8):
            # a single env holding env ev's state and time index
            one = envs.make(config=dict(cfg, storage_layout=None))
            eng = one._engine
            i = int(vec.i[ev])
            one.i = i
            sl = i % eng.H
            eng.x_true[sl].copy_(torch.as_tensor(vec.x_true(ev)))
            eng.x_filter[sl].copy_(torch.as_tensor(vec.x_filter(ev)))
            eng.P_filter[sl].copy_(torch.as_tensor(vec.P_filter(ev)))
            st = vec._eng.status[ev * vec.m:(ev + 1) * vec.m]
            eng.status.copy_(vec._eng.env_caller_rows(ev, st))
            l1 = _look_np(one)
            for k in l1:
                assert np.array_equal(lv[k][ev].view(np.uint8), l1[k].view(np.uint8)), (layout, ev, k)


def test_agents(envs):
    from ssa_gym_amd import _lib, agents
    env = envs.make(config=cfg1(envs, seed=61))
    env.step(2)
    for agent, row in ((agents.agent_info_gain, _lib.LOOK_INFO_GAIN), (agents.agent_trace_gain, _lib.LOOK_TRACE_GAIN)):
        a = agent(None, env)
        s = env.lookahead()["score"][row].cpu().numpy()
        assert np.isfinite(s).any()
        assert a == int(np.argmax(np.where(np.isfinite(s), s, -np.inf)))
    with pytest.raises(NotImplementedError):
        env.run_agent(agents.agent_info_gain, 5)
    # nothing finite: nothing visible -> action_space.sample()
    blind = envs.make(config=cfg1(envs, seed=62, obs_limit=90))
    blind.action_space.seed(123)
    want = blind.action_space.sample()
    blind.action_space.seed(123)
    assert not np.isfinite(blind.lookahead()["score"].cpu().numpy()).any()
    assert agents.agent_info_gain(None, blind) == want
    # whole episodes
    results = {}
    for agent in (agents.agent_info_gain, agents.agent_trace_gain, agents.agent_visible_greedy):
        ep = envs.make(config=cfg1(envs, seed=63))
        obs, done, k = None, False, 0
        while not done:
            obs, r, done, _ = ep.step(agent(obs, ep))
            k += 1
        assert k == 479
        results[agent.__name__] = (float(np.nanmean(np.asarray(ep.delta_pos[ep.i]))), len(ep.failed_filters_id))
    print("[lookahead agents] end of episode (mean delta_pos, failed filters):", results)
    with pytest.raises(ValueError):
        ep.lookahead()
