"""cost of a sensor network's H-step tasking forecast: (a) HotPathEngine.launch_forecast_sensors, one launch, against (b) the only way
to get the same numbers without it: H x (launch_lookahead_sensors + an all-idle launch_step_sensors, one launch each: statistics by
the step kernel's atomics, fold deferred) on the same engine.  Both start from the same state -- history slot and status words are
restored (outside the timed region) after every run of (b), which spends the env -- and alternate repetition by repetition.
usage (from the repository root): python profiles/forecast_sensors_cost.py S[,S...] early|late|both [reps] [kernels]
  wall clock around the synchronised call; `kernels`: a few untimed repetitions of each, (b) last -- run that under
  rocprofv3 --kernel-trace for the kernels' own time (the trace's last reps x H lookahead / step dispatches are (b)'s)"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import ssa_gym_amd  # noqa: E402,F401
from ssa_gym_amd import envs as E  # noqa: E402
from support.sensors import SITES8_GEOMETRY  # noqa: E402

sensors = [int(v) for v in sys.argv[1].split(",")]
phases = ["early", "late"] if sys.argv[2] == "both" else [sys.argv[2]]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
kernels_only = len(sys.argv) > 4 and sys.argv[4] == "kernels"
warm, m, H, HOR = 3, 20000, 16, 8


def make_env(S):
    cfg = dict(E.env_config)
    cfg.update(rso_count=m, steps=480, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3, history=H)
    if S > 1:
        cfg.update(observers=SITES8_GEOMETRY[:S], sensor_obs_limit=[15, 10, 20, 0, 5, 10, 20, 15][:S],
                   sensor_z_sigma=[(1 + 0.5 * k, 1 + 0.5 * k, 1e3) for k in range(S)])
    return E.make('ssa_tasker_simple-v2', config=cfg)


def advance(env, S, rs, to):
    while env.i < to:
        env.step(rs.permutation(m)[:S] if S > 1 else int(rs.randint(m)))


def measure(env, S, phase):
    e, sites, i = env._engine, env._sites(), env.i
    slot = i % H
    torch.cuda.synchronize()
    snap = e.snapshot_state(slot)

    def forecast():
        e.launch_forecast_sensors(slot, i + 1, sites, HOR)

    def parent():
        for h in range(HOR):
            e.launch_lookahead_sensors((i + h) % H, i + 1 + h, sites)
            e.launch_step_sensors((i + h) % H, (i + h + 1) % H, i + 1 + h, sites, [-1] * S, 0, fast_stats=True, defer_fold=True)

    def restore():
        e.flush_stats()
        e.restore_state(slot, snap)
        torch.cuda.synchronize()
    order = [("a_forecast_one_launch", forecast), ("b_lookahead_plus_idle_step_x%d" % HOR, parent)]
    if kernels_only:
        for _ in range(1 + reps):
            forecast()
        torch.cuda.synchronize()
        for _ in range(reps):      # (last: the trace's final reps x HOR lookahead / step dispatches)
            parent()
            restore()
        print("S=%d %-5s step %d: %d + 1 forecasts, then %d x %d (lookahead + idle step)" % (S, phase, i, reps, reps, HOR))
        return
    times = {k: [] for k, _ in order}
    for r in range(warm + reps):
        for name, fn in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e6
            restore()
            if r >= warm:
                times[name].append(dt)
    med = {}
    for name, _ in order:
        v = np.array(times[name])
        med[name] = np.median(v)
        print("S=%d %-5s step %3d  %-32s per %d-step horizon [us]: median %8.2f  min %8.2f  max %8.2f  (%d reps, %d objects, hybrid)"
              % (S, phase, i, name, HOR, np.median(v), v.min(), v.max(), reps, m))
    print("S=%d %-5s step %3d  forecast / parent = %.3f" % (S, phase, i, med[order[0][0]] / med[order[1][0]]))
    assert env.i == i


for S in sensors:
    env, rs = make_env(S), np.random.RandomState(7)
    for phase in phases:
        advance(env, S, rs, 2 if phase == "early" else 300)
        measure(env, S, phase)
