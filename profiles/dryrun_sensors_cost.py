"""cost and worth of the dry run of candidate schedules (ssa_dryrun_sensors_envs_f64) at 20 000 objects, hybrid,
K = 8.
usage (from the repository root):
  python profiles/dryrun_sensors_cost.py S[,S...] early|late|both [reps] [kernels]
      an env advanced to step 2 / 300; B = 1, 64, 512 candidates (the horizon-wide plan with, per candidate, one to three slots redrawn
      from the objects visible there -- what a search planner evaluates); wall clock around the synchronised env.evaluate_schedules,
      alternating with launch_forecast_sensors at H = 8 on the same state (the reference point) and, at B = 1, with the full-catalogue
      form (gather=False): 3 warm-ups, then `reps` (20) repetitions, median [min .. max].  The call's parts, each timed on its own in
      the same way: the host's row builder, the engine call (upload, gather, launch) and the whole call (the records' split and the
      slot-order totals on top).  `kernels`: a few untimed repetitions of each -- run that under rocprofv3 --kernel-trace --stats
  python profiles/dryrun_sensors_cost.py 8 gain
      one 480-step episode with 8 sites per planner from the same seed, replanned every 8 steps and executed with rollout_sensors: the
      horizon-wide plan against the same plan refined (agents.refine_plan_sensors, 4 rounds x 64 candidates).  Realised information gain:
      the dry run's gain of every slot the execution booked as taken (the flags agree by construction: visibility is the truth's)"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import ssa_gym_amd  # noqa: E402,F401
from ssa_gym_amd import _lib, agents, device  # noqa: E402
from ssa_gym_amd import envs as E  # noqa: E402
from support.sensors import SITES8_GEOMETRY  # noqa: E402

sensors = [int(v) for v in sys.argv[1].split(",")]
mode = sys.argv[2]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
kernels_only = len(sys.argv) > 4 and sys.argv[4] == "kernels"
warm, m, HIST, HOR = 3, 20000, 64, 8
col = _lib.LOOK_INFO_GAIN


def make_env(S):
    cfg = dict(E.env_config)
    cfg.update(rso_count=m, steps=480, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3, history=HIST)
    if S > 1:
        cfg.update(observers=SITES8_GEOMETRY[:S], sensor_obs_limit=[15, 10, 20, 0, 5, 10, 20, 15][:S],
                   sensor_z_sigma=[(1 + 0.5 * k, 1 + 0.5 * k, 1e3) for k in range(S)])
    env = E.make('ssa_tasker_simple-v2', config=cfg)
    env.action_space.seed(11)
    return env


def candidates(env, B, rs):
    """the horizon-wide plan, and B - 1 copies of it with one to three slots redrawn from the objects visible there"""
    S = env.n_sensor
    plan = agents.plan_info_gain_sensors_horizon(env, HOR)
    ok = ~torch.isnan(env.forecast_sensors(HOR)["score"][..., col]).cpu().numpy()
    cand = np.repeat(plan[None], B, axis=0)
    for b in range(1, B):
        for _ in range(1 + b % 3):
            k, s = divmod(int(rs.randint(HOR * S)), S)
            pool = np.flatnonzero(ok[k, s])
            if len(pool):
                cand[b, k, s] = pool[rs.randint(len(pool))]
    return cand


def timed(fns, label):
    t = {k: [] for k in fns}
    for r in range(warm + reps):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warm:
                t[name].append((time.perf_counter() - t0) * 1e6)
    med = {}
    for name in fns:
        v = np.array(t[name])
        med[name] = np.median(v)
        print("%s  %-34s wall clock [us]: median %8.1f  [%8.1f .. %8.1f]  (%d reps)" % (label, name, np.median(v), v.min(), v.max(), len(v)))
    return med


if mode == "gain":
    S = sensors[0]
    for name in ("horizon-wide plan", "the same plan refined (4 x 64)"):
        env = make_env(S)
        gain, observed, undefined, revisits, changed, replans, nan_totals = 0.0, 0, 0, 0, 0, 0, 0
        while env.i + 1 < env.n:
            i = env.i
            plan = agents.plan_info_gain_sensors_horizon(env, HOR)
            if name.startswith("the same"):
                out, _ = agents.refine_plan_sensors(env, plan, kind='info', rounds=4, candidates=64, seed=replans)
                changed += int((out != plan).sum())
                plan = out
            ids, counts = np.unique(plan, return_counts=True)
            revisits += int((counts - 1).sum())
            r = env.evaluate_schedules(plan)
            score, taken = r["score"][0, ..., col].cpu().numpy(), r["taken"][0].cpu().numpy()
            nan_totals += int(torch.isnan(r["total"][0, col]))
            replans += 1
            _, _, dones, _ = env.rollout_sensors(plan)
            took = env.obs_taken[i + 1:i + 1 + len(dones)].reshape(len(dones), -1)
            assert np.array_equal(took, taken[:len(dones)]), "the execution booked other observations than the dry run foresaw"
            for h in range(len(dones)):
                for s in range(S):
                    if took[h, s]:
                        observed += 1
                        if np.isnan(score[h, s]):      # (an update of a covariance without a log-determinant: a diverged filter)
                            undefined += 1
                        else:
                            gain += float(score[h, s])
            if np.any(dones):
                break
        print("S=%d gain [%s]: %d steps, %d replans; realised information gain %.6f nat over %d observing (step, sensor) pairs (%d more "
              "observed with an undefined gain: no log-determinant; %d plans' totals are NaN for it); %d revisits chosen (an object named "
              "again inside one plan), %d slots changed by the refinement"
              % (S, name, env.i, replans, gain, observed - undefined, undefined, nan_totals, revisits, changed))
    sys.exit(0)

for S in sensors:
    env, rs = make_env(S), np.random.RandomState(7)
    for phase in (["early", "late"] if mode == "both" else [mode]):
        while env.i < (2 if phase == "early" else 300):
            env.step(rs.permutation(m)[:S] if S > 1 else int(rs.randint(m)))
        e, sites, i = env._engine, env._sites(), env.i
        for B in (1, 64, 512):
            cand = candidates(env, B, np.random.RandomState(B))
            ids, _ = device.dryrun_rows(cand, m, S)
            label = "S=%d %-5s step %3d B=%3d" % (S, phase, i, B)
            r = env.evaluate_schedules(cand)
            print("%s  K=%d: W = %d rows per candidate (%d wavefronts), %d of %d slots taken in candidate 0, its total %.6f nat"
                  % (label, HOR, ids.shape[1], B * ids.shape[1] // 4, int(r["taken"][0].sum()), HOR * S, float(r["total"][0, col])))
            fns = {"a_evaluate_schedules": lambda: env.evaluate_schedules(cand),
                   "b_forecast_H8_one_launch": lambda: e.launch_forecast_sensors(i % HIST, i + 1, sites, HOR),
                   "c_engine_call_alone": lambda: e.launch_dryrun_sensors(i % HIST, i + 1, sites, cand),
                   "d_host_row_builder_alone": lambda: device.dryrun_rows(cand, m, S)}
            if B == 1:
                fns["e_full_catalogue_form"] = lambda: env.evaluate_schedules(cand, gather=False)
            if kernels_only:
                for fn in fns.values():
                    for _ in range(reps):
                        fn()
                torch.cuda.synchronize()
                print("%s  %d untimed repetitions of each of %s" % (label, reps, sorted(fns)))
                continue
            med = timed(fns, label)
            print("%s  evaluate_schedules / forecast = %.3f; of the call: row builder %.0f %%, engine call %.0f %% (upload, gather, launch), "
                  "records and totals %.0f %%" % (label, med["a_evaluate_schedules"] / med["b_forecast_H8_one_launch"],
                                                  100 * med["d_host_row_builder_alone"] / med["a_evaluate_schedules"],
                                                  100 * med["c_engine_call_alone"] / med["a_evaluate_schedules"],
                                                  100 * (1 - med["c_engine_call_alone"] / med["a_evaluate_schedules"])))
        assert env.i == i
