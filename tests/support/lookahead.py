"""The single-sensor lookahead against the project's own step: the env configs of the lookahead tests and the central check, shared by
tests/test_lookahead_gpu.py and tests/test_update_failures_gpu.py."""
import numpy as np


def cfg1(E, **over):
    cfg = dict(E.env_config)
    cfg.update(rso_count=2000, steps=480, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3)
    cfg.update(over)
    return cfg


def xyz1(E):
    from ssa_gym_amd.envs import dynamics as D
    return dict(obs_type='xyz', z_sigma=(5e2,) * 3, R=np.diag([5e2 ** 2] * 3), hx=D.hx_xyz, mean_z=D.mean_xyz, residual_z=np.subtract)


def _bits(t):
    """float64 tensor -> its bit patterns (NaN == NaN, -0 != +0)"""
    return t.contiguous().view(__import__("torch").int64)


def _look_np(env):
    r = env.lookahead(covariances=True)
    return {k: v.cpu().numpy().copy() for k, v in r.items()}


def _sample(look, st_in, rs, n=64):
    """visible, not visible, already failed, failing in this predict, singular S -- then random objects up to n"""
    m = st_in.shape[0]
    vis, stl = look["visible"].astype(bool), look["status"]
    groups = [np.where(vis)[0], np.where(~vis & (stl == 0))[0], np.where(st_in != 0)[0],
              np.where((st_in == 0) & ((stl == 1) | (stl == 2)))[0], np.where(stl == 4)[0]]
    pick = []
    for g in groups:      # (the groups overlap once S is singular -- those objects are visible too: an object is picked once, so that the
        #                   fill-up below still reaches n distinct objects)
        pick.extend(j for j in rs.permutation(g)[:16].tolist() if j not in pick)
    rest = rs.permutation(np.setdiff1d(np.arange(m), pick))
    pick.extend(rest[:max(0, n - len(pick))].tolist())
    return np.unique(np.asarray(pick, dtype=np.int64))


def check_against_step(env, n=64, seed=0):
    """the central check: lookahead of the env's current state vs. the step launched with every sampled action in turn"""
    import torch
    from ssa_gym_amd import _lib
    e = env._engine
    assert e._order is None       # (engine rows = the env's indices)
    i = env.i
    sin, sout = i % e.H, (i + 1) % e.H
    look = _look_np(env)
    torch.cuda.synchronize()
    st0, fc0 = e.status.clone(), e.fail_count.clone()
    st_in = st0.cpu().numpy()
    objs = _sample(look, st_in, np.random.RandomState(seed), n)
    assert len(objs) >= n
    xp_bits = _bits(torch.as_tensor(look["x_prior"]).cuda())
    Pp_bits = _bits(torch.as_tensor(look["P_prior"]).cuda()).view(-1, 36)
    m = env.m
    seen = {"visible": 0, "hidden": 0, "failed": 0, "failing": 0}
    for j in objs:
        e.status.copy_(st0)
        e.launch_step(sin, sout, i + 1, action=int(j))
        torch.cuda.synchronize()
        st_j = int(e.status[j])
        upd = e.upd[sout, 0].cpu().numpy()
        # status / visible as the step produced them
        if st_j == _lib.ST_UPDATE_NAN:      # (depends on the drawn noise: not foreseen -- the lookahead says OK and visible)
            assert look["status"][j] == _lib.ST_OK and look["visible"][j] == 1
        else:
            assert look["status"][j] == st_j, (j, look["status"][j], st_j)
            assert np.array_equal(e.P_filter[sout, j].cpu().numpy().view(np.int64), look["P_post"][j].view(np.int64)), j
        assert look["visible"][j] == int(upd[_lib.UPD_VISIBLE]), (j, look["visible"][j], upd[_lib.UPD_VISIBLE])
        # every other object: the prior, bit for bit
        other = torch.ones(m, dtype=torch.bool, device="cuda")
        other[int(j)] = False
        assert torch.equal(_bits(e.x_filter[sout])[other], xp_bits[other]), j
        assert torch.equal(_bits(e.P_filter[sout]).view(-1, 36)[other], Pp_bits[other]), j
        seen["visible"] += int(look["visible"][j] == 1)
        seen["hidden"] += int(look["visible"][j] == 0 and look["status"][j] == 0)
        seen["failed"] += int(st_in[j] != 0)
        seen["failing"] += int(st_in[j] == 0 and look["status"][j] in (1, 2))
    e.status.copy_(st0)
    e.fail_count.copy_(fc0)
    torch.cuda.synchronize()
    # every object's status after a step that did not choose it: the predict's outcome (= the lookahead's where no update runs)
    e.launch_step(sin, sout, i + 1, action=int(objs[0]))
    torch.cuda.synchronize()
    st_after = e.status.cpu().numpy()
    no_upd = look["visible"] == 0
    no_upd[objs[0]] = False
    assert np.array_equal(st_after[no_upd], look["status"][no_upd])
    e.status.copy_(st0)
    e.fail_count.copy_(fc0)
    torch.cuda.synchronize()
    print("[lookahead vs step] i=%d, %d objects: %s" % (i, len(objs), seen))
    return look, seen
