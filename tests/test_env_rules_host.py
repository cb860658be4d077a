"""CPU-only checks of what SSA_Tasker_Env and SSA_Tasker_VecEnv share (envs/_config.py): the reward rule, against the reference's
per-step rule (ssa_tasker_simple_2.py:324-354) for every reward type (an unknown one pays 0), threshold, NaN statistic, last step,
any-sensor hit and both forms of `paid`, in its rows form and its one-row form; and the config rules the vector env takes from the env."""
import numpy as np
import pytest

M, N = 7, 12
# max_dpos around both thresholds, at them, NaN and inf
MAX_DPOS = [np.nan, 1e3, 2.9999e4, 3e4, 3.0001e4, 1e6, 5e6, 5.0001e6, np.inf]


def _stats(rng, E):
    from ssa_gym_amd import _lib
    st = np.zeros((E, _lib.STAT_STRIDE))
    st[:, _lib.STAT_MAX_DPOS] = [MAX_DPOS[k % len(MAX_DPOS)] for k in range(E)]
    st[:, _lib.STAT_CNT_LT_1E4] = rng.integers(0, M + 1, E)
    st[:, _lib.STAT_CNT_LT_1E7] = rng.integers(0, M + 1, E)
    return st


def _reference(reward_type, st, hit, paid, last):
    """the reference's rule for one step, as a scalar: (reward, done)"""
    from ssa_gym_amd import _lib
    max_dpos, r, done = st[_lib.STAT_MAX_DPOS], 0.0, False
    if reward_type == 'jones':
        if max_dpos > 5e6:
            done, r = True, 0
        elif max_dpos < 3e4:
            done, r = True, 1
    elif reward_type == 'trinary':
        r = (st[_lib.STAT_CNT_LT_1E4] + st[_lib.STAT_CNT_LT_1E7]) / M / 2
    elif reward_type == 'shaped':
        if max_dpos > 5e6:
            done, r = True, 0
        elif max_dpos < 3e4:
            done, r = True, 1 - paid
        elif hit:
            r = 1 / N
        else:
            r = -1 / N
    return np.float64(r), bool(done or last)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


REWARD_TYPES = ['jones', 'trinary', 'shaped', 'none']     # ('none': a type the rule does not know -- no reward, done at the last step)


@pytest.mark.parametrize("reward_type", REWARD_TYPES)
def test_reward_rule_rows_match_the_reference_rule(reward_type):
    """the vector env's form: statistics rows [E, STAT_STRIDE], hit / paid / last per env"""
    from ssa_gym_amd import _lib
    from ssa_gym_amd.envs._config import reward_done
    rng = np.random.default_rng(1)
    E = 4 * len(MAX_DPOS)
    st = _stats(rng, E)
    hit = np.arange(E) % 2 == 0
    last = (np.arange(E) // 2) % 2 == 0
    paid = rng.normal(size=E) * 0.1
    r, d = reward_done(reward_type, st, hit, paid, last, M, N)
    assert r.shape == (E,) and d.shape == (E,)
    want = [_reference(reward_type, st[e], hit[e], paid[e], last[e]) for e in range(E)]
    assert np.array_equal(_bits(r), _bits([w[0] for w in want]))
    assert np.array_equal(d, [w[1] for w in want])
    for e in range(E):          # the one-row form: the same bits, `paid` as a value or as a function called on a win only
        calls = []
        r1, d1 = reward_done(reward_type, st[e], hit[e], lambda: calls.append(e) or paid[e], bool(last[e]), M, N)
        assert _bits(r1) == _bits(want[e][0]) and d1 is want[e][1]
        assert len(calls) == (reward_type == 'shaped' and st[e, _lib.STAT_MAX_DPOS] < 3e4)
        r2, d2 = reward_done(reward_type, st[e], hit[e], paid[e], bool(last[e]), M, N)
        assert _bits(r2) == _bits(want[e][0]) and d2 is want[e][1]
    # every branch was taken: both ends, neither, NaN
    mx = st[:, _lib.STAT_MAX_DPOS]
    assert (mx > 5e6).any() and (mx < 3e4).any() and np.isnan(mx).any() and ((mx >= 3e4) & (mx <= 5e6)).any()


def _bare_env(S, reward_type):
    from ssa_gym_amd.envs.ssa_tasker_simple_2 import SSA_Tasker_Env
    env = SSA_Tasker_Env.__new__(SSA_Tasker_Env)
    env.n, env.m, env.n_sensor, env.reward_type = N, M, S, reward_type
    env.rewards = np.zeros(N)
    return env


@pytest.mark.parametrize("reward_type", REWARD_TYPES)
def test_env_reward_is_the_reference_rule_with_the_episodes_sum(reward_type):
    """the env's form: one statistics row per step, `paid` = np.sum(self.rewards[:i]) (which rounds differently from the vector env's
    running sum: the rewards keep their bits), the last step ends the episode"""
    rng = np.random.default_rng(2)
    env = _bare_env(1, reward_type)
    st = _stats(rng, N)
    for i in range(1, N):
        a, prev = int(rng.integers(0, M)), int(rng.integers(0, M))
        want = _reference(reward_type, st[i], a == prev, np.sum(env.rewards[:i]), i + 1 >= N)
        done = env._reward_done(i, a, st[i], prev)
        assert done is want[1] and _bits(env.rewards[i]) == _bits(want[0])
        if i % 3 == 0:
            env.rewards[i] = 1.0 / 3.0          # (a history whose sum has rounding in it)
    assert done is True                         # (the last step)


def test_shaped_pays_a_sensor_network_if_any_sensor_took_the_argmax():
    from ssa_gym_amd import _lib
    env = _bare_env(3, 'shaped')
    st = np.zeros(_lib.STAT_STRIDE)
    st[_lib.STAT_MAX_DPOS] = 1e5
    assert env._reward_done(1, np.array([1, 5, 6]), st, 5) is False and env.rewards[1] == 1 / N
    assert env._reward_done(2, np.array([1, 4, 6]), st, 5) is False and env.rewards[2] == -1 / N


def test_vector_env_takes_the_envs_config_rules():
    """the three rules the vector env used to apply differently: obs_dtype other than float64 / float32 is refused, an obs_type other than
    'aer' / 'xyz' ends the program as the env does (the reference's behaviour), and the observation space says float32 when the
    observations are (the vector env's space itself: tests/test_env_gpu.py::test_float32_observations_are_the_float64_ones_rounded).
    The refusals come before anything touches the GPU."""
    from ssa_gym_amd.envs import env_config
    from ssa_gym_amd.envs._config import resolve_config
    from ssa_gym_amd.envs.ssa_tasker_simple_2 import SSA_Tasker_Env
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    cfg = dict(env_config, rso_count=8, steps=6)
    for make in (lambda c: SSA_Tasker_Env(c), lambda c: SSA_Tasker_VecEnv(c, 2)):
        with pytest.raises(ValueError, match="obs_dtype"):
            make(dict(cfg, obs_dtype=np.float16))
        with pytest.raises(SystemExit):
            make(dict(cfg, obs_type='uvw'))
    assert resolve_config(dict(cfg, obs_dtype=np.float32)).obs_space.dtype == np.float32
    assert resolve_config(dict(cfg, obs_dtype=np.float32, obs_returned='aer')).obs_space.shape == (8 * 4,)
    assert resolve_config(dict(cfg)).obs_space.dtype == np.float64
