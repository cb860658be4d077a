"""cost of a sensor network's lookahead and assignment in E envs:
  (a) HotPathEngine.launch_lookahead_sensors_envs, one launch, against (b) the only way to ask the same envs without it: E
      launch_lookahead_sensors on E one-env engines holding the envs' state slices, in one stream;
  (c) launch_assign_sensors_envs, one launch, against (d) E launch_assign_sensors on those engines' scores;
  (e) SSA_Tasker_VecEnv.step_agent end to end against (f) the same three launches with the rows passed through the host: the
      lookahead and the assignment, a synchronisation and the read-back, then the step with the rows as an array (S >= 2).
Nothing in (a) .. (d) changes the state; (e) and (f) start from the same state -- the engine's slot, status words and failure counter
and the env's counters are restored (outside the timed region) after every run.  The forms alternate repetition by repetition.
usage (from the repository root): python profiles/vector_lookahead_sensors_cost.py S[,S...] early|late|both [reps]
  wall clock around the synchronised call, profiler off"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import ssa_gym_amd  # noqa: E402,F401
from ssa_gym_amd import _lib, engine, envs as E  # noqa: E402
from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv  # noqa: E402
from support.sensors import SITES8_GEOMETRY  # noqa: E402

sensors = [int(v) for v in sys.argv[1].split(",")]
phases = ["early", "late"] if sys.argv[2] == "both" else [sys.argv[2]]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
warm, m, NE = 3, 20000, 8
COL = _lib.LOOK_INFO_GAIN


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


def report(S, phase, i, order, took):
    med = {}
    for name, _ in order:
        v = np.array(took[name])
        med[name] = np.median(v)
        print("S=%d %-5s step %3d  %-34s [us]: median %8.2f  [min %8.2f .. max %8.2f]  (%d reps, %d x %d objects, hybrid)"
              % (S, phase, i, name, np.median(v), v.min(), v.max(), reps, NE, m))
    return med


def timed(order, restore=None):
    took = {k: [] for k, _ in order}
    for r in range(warm + reps):
        for name, fn in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e6
            if restore is not None:
                restore()
            if r >= warm:
                took[name].append(dt)
    return took


def measure(vec, S, phase):
    e, i = vec._eng, vec.tick
    sin = i % 2
    sp = vec._sites()
    torch.cuda.synchronize()
    times = [int(t) + 1 for t in vec.i]
    trans = e.trans.cpu().numpy()
    ones = []       # (b), (d): one-env engines on the envs' slices of the same state
    for k in range(NE):
        one = engine.HotPathEngine(vec._consts, m, 1, trans, e.z_noise[k], history=2, zn_stride_env=0, zn_stride_time=3, zn_stride_obj=0)
        sl = slice(k * m, (k + 1) * m)
        for nme in ("x_true", "x_filter", "P_filter", "obs"):
            getattr(one, nme)[sin].copy_(getattr(e, nme)[sin, sl])
        one.status.copy_(e.status[sl])
        ones.append(one)
    look = e.launch_lookahead_sensors_envs(sin, 0, sp, env_times=times)
    looks = [one.launch_lookahead_sensors(sin, times[k], sp) for k, one in enumerate(ones)]
    rows = [one.assign_row() for one in ones]
    torch.cuda.synchronize()
    assert all(torch.equal(look["score"][k].view(torch.int64), looks[k]["score"].view(torch.int64)) for k in range(NE))

    def a():
        e.launch_lookahead_sensors_envs(sin, 0, sp, env_times=times)

    def b():
        for k, one in enumerate(ones):
            one.launch_lookahead_sensors(sin, times[k], sp)

    def c():
        e.launch_assign_sensors_envs(look, COL)

    def d():
        for k, one in enumerate(ones):
            one.launch_assign_sensors(looks[k], COL, rows[k])
    order = [("a_vector_lookahead_one_launch", a), ("b_%d_one_env_lookaheads" % NE, b)]
    med = report(S, phase, i, order, timed(order))
    print("S=%d %-5s step %3d  a / b = %.3f" % (S, phase, i, med[order[0][0]] / med[order[1][0]]))
    order = [("c_vector_assignment_one_launch", c), ("d_%d_one_env_assignments" % NE, d)]
    med = report(S, phase, i, order, timed(order))
    print("S=%d %-5s step %3d  c / d = %.3f" % (S, phase, i, med[order[0][0]] / med[order[1][0]]))
    torch.cuda.synchronize()
    assert all(torch.equal(e.action_table()[k], rows[k]) for k in range(NE))
    if S < 2:
        return
    snap = e.snapshot_state(sin)
    keep = (vec.i.copy(), vec.tick, vec.rewards_sum.copy(), vec._argmax_prev.copy())
    idle = np.full((NE, S), -1)

    def restore():
        e.restore_state(sin, snap)
        vec.i[:], vec.tick, vec.rewards_sum[:], vec._argmax_prev = keep[0], keep[1], keep[2], keep[3].copy()
        torch.cuda.synchronize()

    def on_device():
        vec.step_agent("agent_info_gain_sensors", fallback_actions=idle)

    def through_host():
        vec._step(vec.assign_sensors(COL))
    order = [("e_step_agent_rows_on_the_device", on_device), ("f_same_launches_rows_through_host", through_host)]
    med = report(S, phase, i, order, timed(order, restore))
    print("S=%d %-5s step %3d  e / f = %.3f" % (S, phase, i, med[order[0][0]] / med[order[1][0]]))


for S in sensors:
    vec, rs = SSA_Tasker_VecEnv(config(S), NE, seed=3), np.random.RandomState(7)
    for phase in phases:
        advance(vec, S, rs, 2 if phase == "early" else 300)
        measure(vec, S, phase)
