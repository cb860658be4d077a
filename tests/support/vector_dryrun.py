"""The dry run of candidate schedules in every env of a vector env (ssa_dryrun_gather_f64; HotPathEngine.launch_dryrun_sensors_envs;
SSA_Tasker_VecEnv.evaluate_schedules; agents.refine_plan_sensors on a vector env): complete blocks for the gather's refusals, the stub
vector env of the planner's host tests, and the GPU tests' shared pieces -- guarded buffers, random bit patterns and schedules."""
import ctypes as C

import numpy as np

from support.dryrun import StubEnv

ENTRY = "ssa_dryrun_gather_f64"
PTR_FIELDS = ("ids", "slot_of", "env_time", "x_true_in", "x_in", "P_in", "status_in", "x_true_out", "x_out", "P_out", "status_out", "time_out")
ALIGNED16 = ("x_true_in", "x_in", "P_in", "x_true_out", "x_out", "P_out")      # the pointers whose rows move as 16-byte pieces


def gather_block(**over):
    """a block that passes every check of the entry (2 envs of 8 objects, 3 candidates of 4 rows, a table; addresses never
    dereferenced on the host), with the named fields replaced"""
    from ssa_gym_amd import _lib
    g = _lib.ssa_dryrun_gather_params()
    g.n_obj, g.n_env, g.n_cand, g.n_rows, g.reserved = 8, 2, 3, 4, 0
    for k, name in enumerate(PTR_FIELDS):
        setattr(g, name, 0x10000 * (k + 1))
    for name, value in over.items():
        setattr(g, name, value)
    return g


def gather_refused(fn, **over):
    return fn(C.byref(gather_block(**over)), None)


class StubVecEnv(StubEnv):
    """StubEnv as a vector env of E envs: what agents.refine_plan_sensors reads of one, the forecast and the evaluator with a leading
    [E] axis, a schedule again worth the sum of its entries"""

    def __init__(self, E=3, m=10, S=2, n=20):
        StubEnv.__init__(self, m=m, S=S, n=n)
        self.num_envs = self.E = E
        self._eng, self.i = object(), np.zeros(E, dtype=np.int64)

    def forecast_sensors(self, horizon):
        import torch
        self.forecasts += 1
        return {"visible": torch.ones((self.E, horizon, self.n_sensor, self.m), dtype=torch.uint8),
                "status": torch.zeros((self.E, horizon, self.n_sensor, self.m), dtype=torch.int32)}

    def evaluate_schedules(self, actions):
        import torch
        a = np.asarray(actions)
        a = a[:, None] if a.ndim == 3 else a
        assert a.ndim == 4 and a.shape[0] == self.E
        self.calls.append(a.copy())
        tot = a.reshape(a.shape[0], a.shape[1], -1).sum(axis=2).astype(np.float64)
        return {"total": torch.as_tensor(np.stack([-tot, 2 * tot, tot], axis=2))}


# ---------------------------------------------------------------------------------------------------------------- GPU side
GUARD = 16          # elements in front of and behind every guarded buffer (64 or 128 bytes: the payload stays 16-byte aligned)
GUARD_WORD = 0x5A5A5A5A


def guarded(torch, n, dtype):
    """(whole buffer, payload view) of n int32 / int64 elements with GUARD elements of GUARD_WORD on either side"""
    whole = torch.full((n + 2 * GUARD,), GUARD_WORD, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole):
    w = whole.cpu().numpy()
    return bool((w[:GUARD] == GUARD_WORD).all() and (w[-GUARD:] == GUARD_WORD).all())


def random_bits(rs, n_words):
    """n_words random 64-bit patterns, every eighth a NaN with a random payload, every sixteenth an infinity or a signed zero"""
    w = rs.randint(0, 2 ** 63, size=n_words, dtype=np.int64) ^ (rs.randint(0, 2, size=n_words).astype(np.int64) << 63)
    w[::8] |= 0x7FF0000000000001
    w[5::16] = np.array([0x7FF0000000000000, -0x8000000000000000], dtype=np.int64)[rs.randint(0, 2, size=len(w[5::16]))]
    return w


def schedules(rs, E, B, K, S, m, pool=None):
    """[E, B, K, S] schedules out of a small pool of objects per env -- so that steps revisit an object and two sensors meet on one --,
    candidates with different numbers of distinct objects (b + 1 of them at most), idle and out-of-range entries sprinkled in, and in
    env 0 the last candidate all idle"""
    a = np.empty((E, B, K, S), dtype=np.int64)
    for e in range(E):
        objs = rs.permutation(m) if pool is None else np.asarray(pool[e])
        for b in range(B):
            use = objs[:max(1, min(len(objs), (b + 1) * 2))]
            a[e, b] = use[rs.randint(0, len(use), size=(K, S))]
    spoil = rs.rand(E, B, K, S)
    a[spoil < 0.08] = -1
    a[(spoil >= 0.08) & (spoil < 0.12)] = m + 3
    a[(spoil >= 0.12) & (spoil < 0.14)] = -9
    a[E - 1, 0, K - 1, S - 1] = m + 3
    if B > 1:
        a[0, B - 1] = -1
    else:
        a[0, 0, K - 1, 0] = -1
    return a
