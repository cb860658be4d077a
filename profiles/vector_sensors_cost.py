"""cost of a sensor network's step in E envs: (a) HotPathEngine.launch_step_sensors_envs, one launch, against (b) the only way to step
the same envs without it: E launch_step_sensors on E one-env engines holding the envs' state slices, in one stream, and (c) the plain
vector step without a network (one action per env), the floor.  All three start from the same state -- the status words and the
failure counter are restored (outside the timed region) after every run -- and alternate repetition by repetition.
usage (from the repository root): python profiles/vector_sensors_cost.py S[,S...] early|late|both [reps]
  wall clock around the synchronised call, profiler off"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import ssa_gym_amd  # noqa: E402,F401
from ssa_gym_amd import engine, envs as E, host  # noqa: E402
from ssa_gym_amd.envs._config import resolve_config  # noqa: E402
from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv  # noqa: E402
from support.sensors import SITES8_GEOMETRY  # noqa: E402

sensors = [int(v) for v in sys.argv[1].split(",")]
phases = ["early", "late"] if sys.argv[2] == "both" else [sys.argv[2]]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
warm, m, NE = 3, 20000, 8


def config(S):
    cfg = dict(E.env_config)
    cfg.update(rso_count=m, steps=480, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3, obs_device=True, device_rng=True,
               observers=SITES8_GEOMETRY[:S], sensor_obs_limit=[15, 10, 20, 0, 5, 10, 20, 15][:S],
               sensor_z_sigma=[(1 + 0.5 * k, 1 + 0.5 * k, 1e3) for k in range(S)])
    return cfg


def advance(vec, S, rs, to):
    while vec.tick < to:
        vec.step(np.stack([rs.permutation(m)[:S] for _ in range(NE)]) if S > 1 else rs.randint(m, size=NE))


def measure(vec, S, phase, sp, rs):
    e, i = vec._eng, vec.tick
    sin, sout = i % 2, (i + 1) % 2
    torch.cuda.synchronize()
    snap = e.snapshot_state(sin)
    times = [int(t) + 1 for t in vec.i]
    acts = np.stack([rs.permutation(m)[:S] for _ in range(NE)])
    trans = e.trans.cpu().numpy()
    ones = []       # (b): one-env engines on the envs' slices of the same state and noise
    for k in range(NE):
        one = engine.HotPathEngine(vec._consts, m, 1, trans, e.z_noise[k], history=2, zn_stride_env=0, zn_stride_time=3, zn_stride_obj=0)
        sl = slice(k * m, (k + 1) * m)
        for nme in ("x_true", "x_filter", "P_filter", "obs"):
            getattr(one, nme)[sin].copy_(getattr(e, nme)[sin, sl])
        one.status.copy_(e.status[sl])
        ones.append((one, one.status.clone()))

    def vector():
        e.launch_step_sensors_envs(sin, sout, 0, sp, acts, env_words=times, fast_stats=True, fold_inside=True)

    def parent():
        for k, (one, _) in enumerate(ones):
            one.launch_step_sensors(sin, sout, times[k], sp, acts[k].tolist(), 0, fast_stats=True, fold_inside=True)

    def plain():
        e.launch_step(sin, sout, 0, env_words=(times, acts[:, 0].tolist()), fast_stats=True, fold_inside=True)

    def restore():
        e.restore_state(sin, snap)
        for one, st in ones:
            one.status.copy_(st)
            one.fail_count.zero_()
        torch.cuda.synchronize()
    order = [("a_vector_sensors_one_launch", vector), ("b_%d_one_env_sensor_steps" % NE, parent), ("c_plain_vector_step", plain)]
    took = {k: [] for k, _ in order}
    for r in range(warm + reps):
        for name, fn in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e6
            restore()
            if r >= warm:
                took[name].append(dt)
    med = {}
    for name, _ in order:
        v = np.array(took[name])
        med[name] = np.median(v)
        print("S=%d %-5s step %3d  %-30s per vector step [us]: median %8.2f  [min %8.2f .. max %8.2f]  (%d reps, %d x %d objects, hybrid)"
              % (S, phase, i, name, np.median(v), v.min(), v.max(), reps, NE, m))
    a, b, c = (med[k] for k, _ in order)
    print("S=%d %-5s step %3d  a / b = %.3f   a - c = %.2f us" % (S, phase, i, a / b, a - c))


for S in sensors:
    cfg = config(S)
    vec, rs = SSA_Tasker_VecEnv(cfg, NE, seed=3), np.random.RandomState(7)
    net = resolve_config(cfg).net
    sp = vec._sensors if S > 1 else host.make_sensor_params(net.lla, net.obs_limit, net.R, 0)
    for phase in phases:
        advance(vec, S, rs, 2 if phase == "early" else 300)
        measure(vec, S, phase, sp, rs)
