"""Which library entries the sensor-tasking layer of ssa-gym_amd/agents.py issues, in which order and how often, on the MI355X: every
entry's return code passes through _lib.check with the entry's name, so a recorder in its place sees the exact sequence.  A single env
keeps its one-env entries and a vector env its *_envs entries, whether its time words travel by value (up to INLINE_ENVS envs) or
through device memory: the lists below are written out, not derived from the code under test."""
import numpy as np
import pytest

from support.gpu import envs  # noqa: F401  (the module fixture)
from support.sensors import cfg3, cfg8

pytestmark = pytest.mark.gpu

H = 3                   # the planners' horizon
ROUNDS, CANDIDATES = 2, 4

# a single env: the one-env entries; its dry run gathers with torch index ops and runs the envs entry over B pseudo-envs
SINGLE = {
    "agent_info_gain_sensors": ["ssa_lookahead_sensors_f64", "ssa_assign_sensors_f64"],
    "agent_info_gain_sensors_optimal": ["ssa_lookahead_sensors_f64", "ssa_match_sensors_f64"],
    "plan_info_gain_sensors-greedy": ["ssa_forecast_sensors_f64"] + ["ssa_assign_sensors_f64"] * H,
    "plan_info_gain_sensors-optimal": ["ssa_forecast_sensors_f64"] + ["ssa_match_sensors_f64"] * H,
    "plan_info_gain_sensors_horizon": ["ssa_forecast_sensors_f64", "ssa_plan_sensors_f64"],
    "refine_plan_sensors": ["ssa_forecast_sensors_f64"] + ["ssa_dryrun_sensors_envs_f64", "ssa_dryrun_totals_f64"] * ROUNDS,
}
# a vector env, time words by value or not: the same entries in the same order
VECTOR = {
    "agent_info_gain_sensors": ["ssa_lookahead_sensors_envs_f64", "ssa_assign_sensors_envs_f64"],
    "agent_info_gain_sensors_optimal": ["ssa_lookahead_sensors_envs_f64", "ssa_match_sensors_envs_f64"],
    "plan_info_gain_sensors-greedy": ["ssa_forecast_sensors_envs_f64"] + ["ssa_assign_sensors_envs_f64"] * H,
    "plan_info_gain_sensors-optimal": ["ssa_forecast_sensors_envs_f64"] + ["ssa_match_sensors_envs_f64"] * H,
    "plan_info_gain_sensors_horizon": ["ssa_forecast_sensors_envs_f64", "ssa_plan_sensors_f64"],
    "refine_plan_sensors": ["ssa_forecast_sensors_envs_f64"] + ["ssa_dryrun_gather_f64", "ssa_dryrun_sensors_envs_f64", "ssa_dryrun_totals_f64"] * ROUNDS,
}


def _cfg(envs, m, S):
    make = cfg8 if S > 3 else cfg3
    return make(envs, m=m, steps=12, update_interval=1, sensors=S if S > 1 else 0)


def _calls(agents, env, plan):
    """name -> the call, in the order the test makes them"""
    return {
        "agent_info_gain_sensors": lambda: agents.agent_info_gain_sensors(None, env),
        "agent_info_gain_sensors_optimal": lambda: agents.agent_info_gain_sensors_optimal(None, env),
        "plan_info_gain_sensors-greedy": lambda: agents.plan_info_gain_sensors(env, H),
        "plan_info_gain_sensors-optimal": lambda: agents.plan_info_gain_sensors(env, H, rule="optimal"),
        "plan_info_gain_sensors_horizon": lambda: agents.plan_info_gain_sensors_horizon(env, H),
        "refine_plan_sensors": lambda: agents.refine_plan_sensors(env, plan, rounds=ROUNDS, candidates=CANDIDATES),
    }


def _assert_sequences(monkeypatch, env, plan, expected, what):
    from ssa_gym_amd import _lib, agents
    names = []

    def recorder(rc, entry):
        names.append(entry)
        if rc != 0:
            raise _lib.SsaHipError("%s failed with code %d" % (entry, rc))

    seen = {}
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "check", recorder)
        for name, call in _calls(agents, env, plan).items():
            del names[:]
            call()
            seen[name] = list(names)
            print("[tasking launches] %s %s: %s" % (what, name, seen[name]))
    assert seen == expected, what


@pytest.mark.parametrize("m,S", [(7, 3), (8, 1)])
def test_a_single_env_issues_its_one_env_entries(envs, monkeypatch, m, S):
    """(7, 3): a partial tile; (8, 1): no config['observers'] -- the env's own observer as a one-site network"""
    env = envs.make(config=_cfg(envs, m, S))
    env.action_space.seed(2)
    env.step(np.arange(S) if S > 1 else 0)
    plan = np.stack([(np.arange(S) + k) % m for k in range(H)])
    _assert_sequences(monkeypatch, env, plan, SINGLE, "single env m = %d, S = %d" % (m, S))


@pytest.mark.parametrize("E,m,S", [(3, 8, 3), (9, 12, 8), (1, 7, 3)])
def test_a_vector_env_issues_its_envs_entries(envs, monkeypatch, E, m, S):
    """(3, 8, 3): time words by value; (9, 12, 8): more envs than travel by value, every sensor slot; (1, 7, 3): one env with a
    partial tile"""
    from ssa_gym_amd import _lib
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    vec = SSA_Tasker_VecEnv(_cfg(envs, m, S), E, seed=10)
    assert vec._inline == (E <= _lib.INLINE_ENVS)
    vec.single_action_space.seed(2)
    vec.step(np.tile(np.arange(S), (E, 1)))
    plan = np.tile(np.stack([(np.arange(S) + k) % m for k in range(H)]), (E, 1, 1))
    _assert_sequences(monkeypatch, vec, plan, VECTOR, "vector env E = %d, m = %d, S = %d" % (E, m, S))
