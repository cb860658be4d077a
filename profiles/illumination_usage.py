"""one episode with the illumination test in use ("In use"): 2 000 objects, the 8 sites of
tests/support/sensors.SITES8_NETWORK, sensors 4 .. 7 'ae' with a Sun limit of -12 degrees, 480 steps, tasked by plan_info_gain_sensors over
8-step horizons, next to the same episode without the key.  Prints the share of dark (step, sensor) slots, the share of mask-visible
cells the test removed, and what each run observed.  usage (from the repository root): python profiles/illumination_usage.py"""
import sys
import numpy as np
import torch
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import ssa_gym_amd
from ssa_gym_amd import envs as E, agents
from support.sensors import SITES8_NETWORK
S, m, H = 8, 2000, 8
cfg = dict(E.env_config)
cfg.update(rso_count=m, steps=480, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3,
           observers=SITES8_NETWORK, sensor_measurement=['aer'] * 4 + ['ae'] * 4)
on = E.make('ssa_tasker_simple-v2', config=dict(cfg, sensor_illumination=[None] * 4 + [-12.0] * 4))
off = E.make('ssa_tasker_simple-v2', config=cfg)
print("t_0", cfg['t_0'], "dt", cfg['time_step'], "sites", SITES8_NETWORK)
dark = np.array([[(int(w) >> s) & 1 for s in range(4, 8)] for w in on.sun_dark[1:480]])
print("dark share of (step, sensor) slots, sensors 4..7:", dark.mean(), "per sensor", dark.mean(axis=0))
vis_on = vis_off = 0
while on.i + 1 < on.n:
    h = min(H, on.n - 1 - on.i)
    f_on = on.forecast_sensors(h)["visible"].cpu().numpy()[:, 4:]
    f_off = off.forecast_sensors(h)["visible"].cpu().numpy()[:, 4:]
    vis_on += int(f_on.sum()); vis_off += int(f_off.sum())
    for env in (on, off):
        plan = np.asarray(agents.plan_info_gain_sensors(env, h))
        for row in plan:
            env.step(row)
print("visible cells of sensors 4..7 over the episode's forecasts: mask alone %d, with the test %d, removed share %.4f" % (vis_off, vis_on, 1 - vis_on / max(vis_off, 1)))
for name, env in (("on", on), ("off", off)):
    t = env.obs_taken[1:env.i + 1]
    a = env.actions[1:env.i + 1]
    print(name, "updates taken per sensor", t.sum(axis=0).tolist(), "distinct objects observed", len(set(a[t].tolist())),
          "mean trace P at the end %.4e" % float(np.nanmean(np.trace(env.P_filter[env.i], axis1=1, axis2=2))), "steps", env.i)
