"""time of the pass table of a sensor network (ssa_access_sensors_f64) next to the lookahead whose `visible` was the
only source of an action mask before: 20 000 objects, 8 sites (tests/support/sensors.py: SITES8_NETWORK), the default propagator
(hybrid), a 480-step episode -- T = 479 steps from the reset.
usage (from the repository root):
  python profiles/access_sensors_cost.py one|vec [launches]
      one: SSA_Tasker_Env; vec: SSA_Tasker_VecEnv with E = 8.  `launches` (default 12; the first 2 are warm-up) launches of the access
      kernel over the whole episode and as many of the lookahead from the same state, every one between two events of its own: the
      median and the minimum of device time between the events in microseconds (a launch's own overhead included).  Then the wall clock
      of action_masks(): the first call (which makes the table) and the median of 200 later calls, each ended by a synchronisation.
  python profiles/access_sensors_cost.py reduce TRACE_DIR
      the kernels' own time of such a run made under `rocprofv3 --kernel-trace --output-format csv -d TRACE_DIR -- python
      profiles/access_sensors_cost.py one|vec [launches]`: per kernel family the dispatches of the trace but the first 2 (End_Timestamp -
      Start_Timestamp: no launch overhead), and the figure of merit: access time / (479 x lookahead time)."""
import sys
import time

import numpy as np

T, WARM = 479, 2

if sys.argv[1] == "reduce":
    import csv
    import glob
    f = glob.glob(sys.argv[2] + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f)))
    med = {}
    for label, key in (("access", "access_sensors_kernel"), ("lookahead", "lookahead_sens")):
        # (the first call of action_masks() is one more access dispatch, the last of the trace: the same launch, kept)
        t = np.array([(b - a) * 1e-3 for a, b, name in rows if key in name][WARM:])
        med[label] = np.median(t)
        print("kernel %-9s median %10.2f us  min %10.2f  max %10.2f  (%d dispatches)" % (label, np.median(t), t.min(), t.max(), len(t)))
    print("access / (%d x lookahead) = %.4f" % (T, med["access"] / (T * med["lookahead"])))
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import ssa_gym_amd  # noqa: E402,F401
from ssa_gym_amd import envs as E  # noqa: E402
from support.sensors import SITES8_NETWORK  # noqa: E402

mode, n = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 12
S, m = 8, 20000
cfg = dict(E.env_config)
cfg.update(rso_count=m, steps=T + 1, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3, history=4,
           observers=SITES8_NETWORK, sensor_obs_limit=[15, 10, 20, 12, 18, 8, 25, 15],
           sensor_z_sigma=[(1 + 0.5 * k, 1 + 0.5 * k, 1e3 / (1 + k)) for k in range(S)])
if mode == "one":
    env = E.make('ssa_tasker_simple-v2', config=cfg)
    eng, n_env = env._engine, 1
    access = lambda: eng.launch_access_sensors(env.i % eng.H, env.i + 1, env._sites(), T)                  # noqa: E731
    look = lambda: eng.launch_lookahead_sensors(env.i % eng.H, env.i + 1, env._sites())                   # noqa: E731
else:
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    n_env = 8
    env = SSA_Tasker_VecEnv(cfg, n_env, seed=3)
    eng = env._eng
    times = [int(v) + 1 for v in env.i]
    access = lambda: eng.launch_access_sensors(env.tick % 2, 0, env._sites(), T, env_times=times)          # noqa: E731
    look = lambda: eng.launch_lookahead_sensors_envs(env.tick % 2, 0, env._sites(), env_times=times)      # noqa: E731
torch.cuda.synchronize()


def timed(launch):
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    t = np.array(out[WARM:])
    return np.median(t), "median %10.2f us  min %10.2f  max %10.2f  (%d launches)" % (np.median(t), t.min(), t.max(), len(t))


ta, sa = timed(access)
tl, sl = timed(look)
bits = eng._access["bits"]
seen = int(sum(bin(int(w) & (2 ** 64 - 1)).count("1") for w in bits[0, :, ::97].cpu().numpy().reshape(-1)))
print("%s: %d env(s) x %d objects, %d sites, %d steps, table %.1f MB, set bits in every 97th row of env 0: %d"
      % (mode, n_env, m, S, T, bits.numel() * 8 / 1e6, seen))
print("%s access    %s" % (mode, sa))
print("%s lookahead %s" % (mode, sl))
print("%s access / (%d x lookahead) = %.4f (between events)" % (mode, T, ta / (T * tl)))
t0 = time.perf_counter()
env.action_masks()
torch.cuda.synchronize()
first = time.perf_counter() - t0
wall = []
for _ in range(200):
    t0 = time.perf_counter()
    mask = env.action_masks()
    torch.cuda.synchronize()
    wall.append(time.perf_counter() - t0)
print("%s action_masks(): first call %.1f us, later calls median %.1f us  min %.1f us (wall clock, synchronised), %d of %d cells set"
      % (mode, first * 1e6, np.median(wall) * 1e6, min(wall) * 1e6, int(mask.sum()), mask.numel()))
