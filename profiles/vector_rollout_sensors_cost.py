"""cost of a sensor network's K-step schedule in E envs, 8 x 20 000 objects, hybrid, caller order, K = 32:
  (a) HotPathEngine.launch_rollout_sensors_envs, one call (the rollout and the fold of its statistics), against
  (b) what a vector env had before it: K launch_step_sensors_envs with rows and time words by value, in one stream, one
      synchronisation at the end, and
  (c) E one-env launch_rollout_sensors on E one-env engines holding the envs' state slices (history K + 2), in one stream.
All three spend the envs: the slot, the status words and the failure counter are restored (outside the timed region) after every
run.  The forms alternate repetition by repetition, each from the same restored state; before any timing the script checks that the
three forms leave the same state bits.
usage (from the repository root): python profiles/vector_rollout_sensors_cost.py S[,S...] early|late|both [reps]
  wall clock around the synchronised call, profiler off"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import ssa_gym_amd  # noqa: E402,F401
from ssa_gym_amd import engine, envs as E  # noqa: E402
from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv  # noqa: E402
from support.sensors import SITES8_GEOMETRY  # noqa: E402

sensors = [int(v) for v in sys.argv[1].split(",")]
phases = ["early", "late"] if sys.argv[2] == "both" else [sys.argv[2]]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
warm, m, NE, K = 3, 20000, 8, 32


def config(S):
    cfg = dict(E.env_config)
    cfg.update(rso_count=m, steps=480, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3, obs_device=True, device_rng=True)
    if S > 1:
        cfg.update(observers=SITES8_GEOMETRY[:S], sensor_obs_limit=[15, 10, 20, 0, 5, 10, 20, 15][:S],
                   sensor_z_sigma=[(1 + 0.5 * k, 1 + 0.5 * k, 1e3) for k in range(S)])
    return cfg


def advance(vec, S, rs, to):
    while vec.tick < to:
        vec.step(np.stack([rs.permutation(m)[:S] for _ in range(NE)]) if S > 1 else rs.randint(m, size=NE))


def measure(vec, S, phase, rs):
    e, i = vec._eng, vec.tick
    sin = i % 2
    sp = vec._sites()
    torch.cuda.synchronize()
    times = [int(t) + 1 for t in vec.i]
    e.env_time0.copy_(torch.as_tensor(times, dtype=torch.int32))
    rows = np.stack([np.stack([rs.permutation(m)[:S] for _ in range(NE)]) for _ in range(K)])      # [K, E, S]
    sched = torch.as_tensor(rows.astype(np.int32)).cuda()
    per_env = [sched[:, k].contiguous() for k in range(NE)]
    trans = e.trans.cpu().numpy()
    HC = K + 2
    ones = []       # (c): one-env engines on the envs' slices of the same state
    for k in range(NE):
        one = engine.HotPathEngine(vec._consts, m, 1, trans, e.z_noise[k], history=HC, zn_stride_env=0, zn_stride_time=3, zn_stride_obj=0)
        sl = slice(k * m, (k + 1) * m)
        for nme in ("x_true", "x_filter", "P_filter", "obs", "metrics"):
            getattr(one, nme)[sin].copy_(getattr(e, nme)[sin, sl] if nme != "metrics" else getattr(e, nme)[sin, k:k + 1])
        one.status.copy_(e.status[sl])
        ones.append((one, one.snapshot_state(sin)))
    snap = e.snapshot_state(sin)

    def a():
        e.launch_rollout_sensors_envs(sin, 0, sp, sched)

    def b():
        for k in range(K):
            e.launch_step_sensors_envs((sin + k) % 2, (sin + k + 1) % 2, 0, sp, rows[k], env_words=[t + k for t in times], fast_stats=True,
                                       fold_inside=True)

    def c():
        for k, (one, _) in enumerate(ones):
            one.launch_rollout_sensors(sin, times[k], sp, per_env[k])

    def restore():
        e.restore_state(sin, snap)
        torch.cuda.synchronize()

    def restore_ones():
        for one, s in ones:
            one.restore_state(sin, s)
        torch.cuda.synchronize()

    def state():
        torch.cuda.synchronize()
        sl = (sin + K) % 2
        return [getattr(e, nme)[sl].view(torch.int64).clone() for nme in ("x_true", "x_filter", "P_filter")] + [e.status.clone()]

    # the three forms leave the same state bits
    a()
    sa = state()
    restore()
    b()
    sb = state()
    restore()
    assert all(torch.equal(u, v) for u, v in zip(sa, sb)), "a / b leave different state"
    c()
    torch.cuda.synchronize()
    for k, (one, _) in enumerate(ones):
        sl, so = slice(k * m, (k + 1) * m), (sin + K) % HC
        for q, nme in enumerate(("x_true", "x_filter", "P_filter")):
            assert torch.equal(sa[q][sl], getattr(one, nme)[so].view(torch.int64)), ("a / c leave different state", k, nme)
        assert torch.equal(sa[3][sl], one.status), ("a / c leave different status words", k)
    restore_ones()
    order = [("a_vector_rollout_one_call", a, restore), ("b_%d_vector_steps_by_value" % K, b, restore),
             ("c_%d_one_env_rollouts" % NE, c, restore_ones)]
    took = {k: [] for k, _, _ in order}
    for r in range(warm + reps):
        for name, fn, after in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e6
            after()
            if r >= warm:
                took[name].append(dt)
    med = {}
    for name, _, _ in order:
        v = np.array(took[name])
        med[name] = np.median(v)
        print("S=%d %-5s step %3d  %-32s [us]: median %9.2f  [min %9.2f .. max %9.2f]  (%d reps, %d x %d objects, K = %d, hybrid)"
              % (S, phase, i, name, np.median(v), v.min(), v.max(), reps, NE, m, K))
    print("S=%d %-5s step %3d  a / b = %.3f   a / c = %.3f" % (S, phase, i, med[order[0][0]] / med[order[1][0]], med[order[0][0]] / med[order[2][0]]))
    del ones
    torch.cuda.empty_cache()


for S in sensors:
    vec, rs = SSA_Tasker_VecEnv(config(S), NE, seed=3), np.random.RandomState(7)
    for phase in phases:
        advance(vec, S, rs, 2 if phase == "early" else 300)
        measure(vec, S, phase, rs)
