"""cost and worth of a sensor network's horizon-wide optimal plan (ssa_plan_sensors_f64) against the time-ordered
planners of section 8h (agents._plan_assigned, both rules), on the same engine and state, at 20 000 objects, hybrid, H = 8.
usage (from the repository root):
  python profiles/plan_sensors_cost.py S early|late [reps] [kernels]
      an env advanced to step 2 / 300; wall clock around the synchronised device part of each planner -- the forecast launch, the plan
      or assignment launches, the read-back --, the three alternating, 3 warm-ups, then `reps` (20) repetitions: median [min .. max].
      Also each plan's filled slots and total on that forecast.  `kernels`: three rounds only -- run that under
      rocprofv3 --kernel-trace --stats for the kernels' own time
  python profiles/plan_sensors_cost.py 8 gain
      one 480-step episode with 8 sites per planner from the same seed, replanned every 8 steps and executed with rollout_sensors:
      the realised information gain (the forecast's gain of every planned update that was taken: the forecast's P_post IS the filter's
      covariance after such an update), the (step, sensor) pairs that observed, and how often the plans differ on the same forecast"""
import math
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import ssa_gym_amd  # noqa: E402,F401
from ssa_gym_amd import _lib, agents  # noqa: E402
from ssa_gym_amd import envs as E  # noqa: E402
from support.sensors import SITES8_GEOMETRY  # noqa: E402

S, phase = int(sys.argv[1]), sys.argv[2]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
kernels_only = len(sys.argv) > 4 and sys.argv[4] == "kernels"
warm = 3
m, HIST, HOR = 20000, 64, 8
col = _lib.LOOK_INFO_GAIN


def make_env():
    cfg = dict(E.env_config)
    cfg.update(rso_count=m, steps=480, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3, history=HIST)
    if S > 1:
        cfg.update(observers=SITES8_GEOMETRY[:S], sensor_obs_limit=[15, 10, 20, 0, 5, 10, 20, 15][:S],
                   sensor_z_sigma=[(1 + 0.5 * k, 1 + 0.5 * k, 1e3) for k in range(S)])
    env = E.make('ssa_tasker_simple-v2', config=cfg)
    env.action_space.seed(11)
    return env


PLANNERS = {"time-ordered greedy": lambda env: agents._plan_assigned(env, HOR, col, 'greedy'),
            "time-ordered optimal": lambda env: agents._plan_assigned(env, HOR, col, 'optimal'),
            "horizon-wide optimal": lambda env: agents._plan_horizon_assigned(env, HOR, col)}


def worth(sc, plan):
    """(filled slots, math.fsum of the forecast's gains) of a raw plan [H', S] on the read-back column sc [H', S, m]"""
    hs = [(h, s) for h in range(plan.shape[0]) for s in range(plan.shape[1]) if plan[h, s] >= 0]
    return len(hs), math.fsum(float(sc[h, s, plan[h, s]]) for h, s in hs)


if phase == "gain":
    for name, planner in PLANNERS.items():
        env = make_env()
        gain, observed, tasked_steps, replans, differ, fc_tot = 0.0, 0, 0, 0, 0, {k: 0.0 for k in PLANNERS}
        while env.i + 1 < env.n:
            i = env.i
            raws = {k: p(env) for k, p in PLANNERS.items()}             # (all three on the same state: planning changes nothing)
            sc = env.forecast_sensors(HOR)["score"][..., col].cpu().numpy()
            for k in PLANNERS:
                fc_tot[k] += worth(sc, raws[k])[1]
            replans += 1
            differ += not np.array_equal(raws["horizon-wide optimal"], raws["time-ordered greedy"])
            raw = raws[name]
            plan = agents._fill_plan_horizon(env, raw) if name.startswith("horizon") else agents._fill_plan(env, raw)
            _, _, dones, _ = env.rollout_sensors(plan if S > 1 else plan.reshape(-1, 1))
            took = env.obs_taken[i + 1:i + 1 + len(dones)].reshape(len(dones), -1)
            for h in range(len(dones)):
                tasked_steps += bool(took[h].any())
                for s in range(S):
                    if raw[h, s] >= 0 and took[h, s]:
                        observed += 1
                        gain += float(sc[h, s, raw[h, s]])
            if np.any(dones):
                break
        print("S=%d gain [%s]: %d steps, %d replans; realised information gain %.6f nat over %d observing (step, sensor) pairs, %d steps "
              "with a tasked sensor that observed; the horizon-wide plan differed from the time-ordered greedy one at %d replans"
              % (S, name, env.i, replans, gain, observed, tasked_steps, differ))
        print("S=%d gain [%s]: on this episode's forecasts, the sum of the plans' forecast totals [nat]: %s"
              % (S, name, "  ".join("%s %.6f" % kv for kv in fc_tot.items())))
    sys.exit(0)

env = make_env()
rs = np.random.RandomState(7)
for _ in range(2 if phase == "early" else 300):
    env.step(rs.permutation(m)[:S] if S > 1 else int(rs.randint(m)))
sc = env.forecast_sensors(HOR)["score"][..., col].cpu().numpy()
for name, planner in PLANNERS.items():
    n, tot = worth(sc, planner(env))
    print("S=%d %-5s step %d [%s]: %d of %d slots filled, forecast total %.9g nat; %d finite scores of %d"
          % (S, phase, env.i, name, n, sc.shape[0] * S, tot, int(np.isfinite(sc).sum()), sc.size))
t = {k: [] for k in PLANNERS}
for k in range(warm + (reps if not kernels_only else 0)):
    for name, planner in PLANNERS.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        planner(env)
        torch.cuda.synchronize()
        if k >= warm:
            t[name].append((time.perf_counter() - t0) * 1e6)
for name in PLANNERS:
    if t[name]:
        v = np.array(t[name])
        print("S=%d %-5s device part of the planner, forecast to read-back, wall clock [us]: %-22s median %8.1f  [%8.1f .. %8.1f]  (%d reps)"
              % (S, phase, name, np.median(v), v.min(), v.max(), len(v)))
