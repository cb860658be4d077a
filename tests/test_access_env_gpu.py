"""The pass table behind the envs: SSA_Tasker_Env.action_masks() against lookahead_sensors()['visible'] at every
step of an episode under arbitrary actions, from ONE launch of the library's entry; access_sensors()' summary against its own bits;
SSA_Tasker_VecEnv.action_masks() against single envs across two auto-resets, with exactly one refresh launch per reset; and the same
episodes with the new methods never called: byte-equal to the run that calls them, and to the digests recorded from the commit before
the feature (tests/golden/access_unused_episode.json).
support.illumination.illum_cfg: 3 ground sites (one a radar, two that need a sunlit object and a dark site), 8 objects."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from support import illumination as il
from support.gpu import envs  # noqa: F401  (the module fixture)
from support.vector_lookahead import single_envs

pytestmark = pytest.mark.gpu


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _counted(engine):
    """the engine's launch_access_sensors wrapped: calls[0] counts the launches of the library's entry"""
    calls, inner = [0], engine.launch_access_sensors

    def wrapped(*a, **kw):
        calls[0] += 1
        return inner(*a, **kw)
    engine.launch_access_sensors = wrapped
    return calls


def _actions(rs, m=8, S=3):
    return rs.permutation(m)[:S]


# ---------------------------------------------------------------------------------------------------------------- the single env
def test_action_masks_are_the_lookaheads_visibility_from_one_launch(envs):
    from ssa_gym_amd import _lib
    env = envs.make(config=il.illum_cfg(envs))
    calls = _counted(env._engine)
    rs = np.random.RandomState(8)
    seen = judged = 0
    for k in range(12):
        mask = _np(env.action_masks())
        assert mask.shape == (3, 8) and mask.dtype == np.bool_
        look = env.lookahead_sensors()
        vis, ok = _np(look["visible"]).astype(bool), _np(look["status"]) == _lib.ST_OK
        assert np.array_equal(mask[ok], vis[ok]), (k, np.argwhere(mask != vis).tolist())
        seen += int(mask.sum())
        judged += int(ok.sum())
        assert np.array_equal(_np(env.action_masks()), mask)          # (asked twice: the same mask, no launch)
        env.step(_actions(rs))
    assert calls[0] == 1, calls
    assert 0 < seen < judged and judged >= 12 * 3 * 8 - 24, (seen, judged)
    # a reset is a new truth: a new table, anchored there
    env.reset()
    mask = _np(env.action_masks())
    assert calls[0] == 2 and np.array_equal(mask, _np(env.lookahead_sensors()["visible"]).astype(bool))


def test_access_sensors_summary_agrees_with_its_bits(envs):
    from ssa_gym_amd import device
    env = envs.make(config=il.illum_cfg(envs))
    rs = np.random.RandomState(9)
    for _ in range(2):
        env.step(_actions(rs))
    r = env.access_sensors()
    T = r["n_steps"]
    assert T == env.n - 1 - env.i == 13 and tuple(r["bits"].shape) == (3, 8, 1)
    acc = _np(device.access_unpack(r["bits"], T))                    # [S, m, T]
    first, length, count, passes = (_np(r[k]) for k in ("first", "length", "count", "passes"))
    for s in range(3):
        for j in range(8):
            col = acc[s, j].tolist()
            f = col.index(True) if True in col else -1
            n = 0
            while f >= 0 and f + n < T and col[f + n]:
                n += 1
            runs = sum(1 for h in range(T) if col[h] and (h == 0 or not col[h - 1]))
            assert (first[s, j], length[s, j], count[s, j], passes[s, j]) == (f, n, sum(col), runs), (s, j, col)
    assert acc.any() and not acc.all()
    # the table IS the episode's visibility: the forecast's, step by step, while no filter fails
    fc = env.forecast_sensors(T)
    assert not _np(fc["status"]).any() and np.array_equal(np.moveaxis(_np(fc["visible"]).astype(bool), 0, -1), acc)
    # a shorter horizon: the same first steps; action_masks() reads the table the last call left
    short = env.access_sensors(horizon=5)
    assert short["n_steps"] == 5 and np.array_equal(_np(device.access_unpack(short["bits"], 5)), acc[..., :5])
    assert np.array_equal(_np(env.action_masks()), acc[..., 0])
    with pytest.raises(ValueError):
        env.access_sensors(horizon=0)


# ---------------------------------------------------------------------------------------------------------------- the vector env
def _follow(one, vec, e):
    """the single env `one` put where env e of `vec` stands after its auto-reset: a reset of its own, then e's truth and filters"""
    one.reset()
    one._engine.load_state(0, vec.x_true(e), vec.x_filter(e), vec.P_filter(e))


def test_vector_masks_are_the_single_envs_across_auto_resets(envs):
    from ssa_gym_amd import _lib
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    cfg = il.illum_cfg(envs, steps=6)
    E = 2
    vec = SSA_Tasker_VecEnv(cfg, E, seed=10)
    singles = single_envs(envs, cfg, vec, 10)
    calls = _counted(vec._eng)
    rs = np.random.RandomState(3)
    resets = 0
    for k in range(12):
        masks = _np(vec.action_masks())
        assert masks.shape == (E, 3, 8) and masks.dtype == np.bool_
        look = vec.lookahead_sensors()
        vis, ok = _np(look["visible"]).astype(bool), _np(look["status"]) == _lib.ST_OK
        assert np.array_equal(masks[ok], vis[ok]), k
        for e in range(E):
            assert np.array_equal(_np(singles[e].action_masks()), masks[e]), (k, e)
        assert calls[0] == 1 + resets, (k, calls, resets)
        acts = np.stack([_actions(rs) for _ in range(E)])
        _, _, dones, _ = vec.step(acts)
        assert dones.all() or not dones.any()
        if dones.any():
            resets += 1
            for e in range(E):
                _follow(singles[e], vec, e)
        else:
            for e in range(E):
                singles[e].step(acts[e])
    assert resets == 2 and calls[0] == 1 + resets - 0, (resets, calls)
    # the table of all envs and each env's own steps
    r = vec.access_sensors()
    assert tuple(r["bits"].shape) == (E, 3, 8, 1) and r["n_steps"].tolist() == (vec.n - 1 - vec.i).tolist()


def test_a_vector_env_refreshes_only_the_env_that_was_reset(envs):
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    cfg = il.illum_cfg(envs, steps=8)
    vec = SSA_Tasker_VecEnv(cfg, 2, seed=10)
    rs = np.random.RandomState(4)
    vec.action_masks()
    for _ in range(3):
        vec.step(np.stack([_actions(rs) for _ in range(2)]))
    before = _np(vec._eng._access["bits"])
    seen = []
    inner = vec._eng.launch_access_sensors

    def spy(*a, **kw):
        seen.append(None if kw.get("envs") is None else np.asarray(kw["envs"]).tolist())
        return inner(*a, **kw)
    vec._eng.launch_access_sensors = spy
    vec._reset_env(1, vec.tick % 2)                                   # env 1 starts a new episode; env 0 is at its step 3
    masks = _np(vec.action_masks())
    assert seen == [[1]], seen
    after = _np(vec._eng._access["bits"])
    assert np.array_equal(after[0], before[0])                        # env 0's slab: not a byte written
    assert np.array_equal(masks, _np(vec.lookahead_sensors()["visible"]).astype(bool))
    vec.action_masks()
    assert seen == [[1]]


# ---------------------------------------------------------------------------------------------------------------- unused: what it was
def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _episode(envs, ask):
    """15 steps of the single env under fixed actions; ask: action_masks() and access_sensors() called along the way.  The digests of
    every observation, every reward, and the final truth, estimates, covariances and status"""
    env = envs.make(config=il.illum_cfg(envs))
    rs = np.random.RandomState(12)
    obs, rew = [env.reset()], []
    for k in range(15):
        if ask:
            env.action_masks()
            if k % 4 == 0:
                env.access_sensors(horizon=3)
        o, r, done, _ = env.step(_actions(rs))
        obs.append(np.array(o, copy=True))
        rew.append(r)
    e = env._engine
    sl = env.i % e.H
    state = [_np(t) for t in (e.x_true[sl], e.x_filter[sl], e.P_filter[sl], e.status)]
    return {"observations": _digest(*obs), "rewards": _digest(np.array(rew, dtype=np.float64)), "state": _digest(*state)}


def test_the_episode_is_what_it_was_when_the_methods_are_never_called(envs):
    """the digests of an episode that never calls the new methods: those of the same episode run on the commit before the feature, and
    those of the episode that does call them (the table reads the truth and writes nothing of the env)"""
    plain = _episode(envs, ask=False)
    assert plain == _episode(envs, ask=True)
    recorded = json.load(open(os.path.join(GOLDEN, "access_unused_episode.json")))
    assert plain == recorded["digests"], (plain, recorded)
