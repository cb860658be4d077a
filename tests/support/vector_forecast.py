"""A sensor network's H-step forecast in each of several envs: the bare vector env of the host tests, and for the GPU tests the
engine's state as bytes and the numpy restatement of the vector planner's rule."""
import numpy as np

from support.vector_lookahead import greedy_rows

KEYS = ("score", "status", "visible", "x_prior", "P_prior", "P_post")
SENTINEL = np.array([1e20] * 3 + [1e12] * 3)      # what a filter that failed carries: x, and the diagonal of P


def bare_vec(S, E=3, m=8, n=12, seed=5):
    """a vector env object without device state (what a machine without a GPU has), with just what the guards and the fill-in read"""
    from ssa_gym_amd.envs._gymshim import spaces
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    vec = SSA_Tasker_VecEnv.__new__(SSA_Tasker_VecEnv)
    vec.E, vec.num_envs, vec.m, vec.n, vec.n_sensor = E, E, m, n, S
    vec.i, vec.tick, vec._eng = np.zeros(E, dtype=np.int64), 0, None
    vec.single_action_space = spaces.MultiDiscrete([m] * S) if S > 1 else spaces.Discrete(m)
    vec.single_action_space.seed(seed)
    return vec


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def state_bytes(torch, eng):
    """every tensor the engine holds (device and host-mapped), as bytes"""
    torch.cuda.synchronize()
    return {k: v.detach().cpu().contiguous().numpy().tobytes() for k, v in vars(eng).items() if isinstance(v, torch.Tensor)}


def plan_np(score):
    """the vector planner's rule on a read-back forecast column [E, H', S, m]: per env, step by step, the global greedy assignment
    (support.vector_lookahead.greedy_rows) without the objects that env planned at an earlier step; int64 [E, H', S], -1 for none"""
    E, Hp, S, m = score.shape
    plan = np.full((E, Hp, S), -1, dtype=np.int64)
    for e in range(E):
        planned = np.zeros(m, bool)
        for h in range(Hp):
            sc = np.array(score[e, h], dtype=np.float64)
            sc[:, planned] = np.nan
            plan[e, h] = greedy_rows(sc)[0]
            planned[plan[e, h][plan[e, h] >= 0]] = True
    return plan
