"""cost of one env through a sensor network's two entry points: (a) HotPathEngine.launch_lookahead_sensors /
launch_forecast_sensors (ssa_lookahead_sensors_f64 / ssa_forecast_sensors_f64, one env) against (b) launch_lookahead_sensors_envs /
launch_forecast_sensors_envs on the same E = 1 engine, from the same history slot, alternating A B A B.  Neither changes the state.
Cells: the lookahead at 20 000 objects (one tile per wavefront) and 40 000 (grid-stride instance), the forecast (H = 8) at 20 000;
S in {1, 8}; step 2 and step 302; `hybrid`.  The margin of a cell is (a)'s own spread: |median of the first half - median of the second
half| of (a)'s alternations; (b) - (a) inside it cannot be told from the shared machine's noise.
usage (from the repository root):
  python profiles/one_env_sensors_cost.py [reps]                 wall clock around the synchronised call, profiler off
  python profiles/one_env_sensors_cost.py [reps] kernels         the same alternations untimed -- run under rocprofv3 --kernel-trace --stats
  python profiles/one_env_sensors_cost.py [reps] reduce TRACE    the kernels' own time from that trace, cell by cell in dispatch order"""
import csv
import glob
import sys
import time

import numpy as np

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
mode = sys.argv[2] if len(sys.argv) > 2 else "wall"
warm, H, HOR = 5, 16, 8
SIZES = ((20000, ("lookahead", "forecast")), (40000, ("lookahead",)))
CELLS = [(family, m, S, step) for m, families in SIZES for S in (1, 8) for step in (2, 302) for family in families]   # (in dispatch order)
PER_CELL = 2 * (1 + warm + reps)   # (one checked pair, then the alternations)


def report(cell, a, b, names=""):
    a, b = np.array(a), np.array(b)
    half = len(a) // 2
    ma, mb, spread = np.median(a), np.median(b), abs(np.median(a[:half]) - np.median(a[half:]))
    print("%-9s m=%5d S=%d step %3d  a_one_env median %8.2f us [min %8.2f] halves %8.2f / %8.2f  b_envs median %8.2f us [min %8.2f]  "
          "b - a %+7.2f  spread %6.2f  %s  (%d each)%s" % (cell + (ma, a.min(), np.median(a[:half]), np.median(a[half:]), mb, b.min(), mb - ma,
                                                         spread, "inside" if mb - ma <= spread else "SLOWER", len(a), names)))


if mode == "reduce":
    f = glob.glob(sys.argv[3] + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f)))
    rows = [r for r in rows if "lookahead_sensor" in r[2] or "forecast_sensor" in r[2]][-len(CELLS) * PER_CELL:]
    assert len(rows) == len(CELLS) * PER_CELL, len(rows)
    for k, cell in enumerate(CELLS):
        mine = rows[k * PER_CELL:(k + 1) * PER_CELL][2 * (1 + warm):]
        assert all(cell[0] in r[2] for r in mine)
        short = [sorted({r[2].split("<")[0].split("(")[0].replace("void ", "").replace("ssa::", "") for r in mine[j::2]}) for j in (0, 1)]
        report(cell, [(r[1] - r[0]) / 1e3 for r in mine[0::2]], [(r[1] - r[0]) / 1e3 for r in mine[1::2]], "  a: %s  b: %s" % tuple(short))
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import ssa_gym_amd  # noqa: E402,F401
from ssa_gym_amd import envs as E  # noqa: E402
from support.sensors import SITES8_GEOMETRY  # noqa: E402


def make_env(m, S):
    cfg = dict(E.env_config)
    cfg.update(rso_count=m, steps=480, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3, history=H)
    if S > 1:
        cfg.update(observers=SITES8_GEOMETRY[:S], sensor_obs_limit=[15, 10, 20, 0, 5, 10, 20, 15][:S],
                   sensor_z_sigma=[(1 + 0.5 * k, 1 + 0.5 * k, 1e3) for k in range(S)])
    return E.make('ssa_tasker_simple-v2', config=cfg)


def measure(env, cell):
    family, m, S, _ = cell
    e, sites, i = env._engine, env._sites(), env.i
    slot = i % H
    if family == "lookahead":
        pair = (lambda: e.launch_lookahead_sensors(slot, i + 1, sites), lambda: e.launch_lookahead_sensors_envs(slot, i + 1, sites))
    else:
        pair = (lambda: e.launch_forecast_sensors(slot, i + 1, sites, HOR), lambda: e.launch_forecast_sensors_envs(slot, i + 1, sites, HOR))
    one, envs = pair[0](), pair[1]()
    torch.cuda.synchronize()
    assert all(torch.equal(one[k].view(-1).view(torch.uint8), envs[k].view(-1).view(torch.uint8)) for k in ("score", "status", "visible"))
    took = ([], [])
    for r in range(warm + reps):
        for j, fn in enumerate(pair):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warm:
                took[j].append((time.perf_counter() - t0) * 1e6)
    assert env.i == i
    if mode == "kernels":
        print("%-9s m=%5d S=%d step %3d: one checked pair, then %d + %d alternations a b" % (cell + (warm, reps)))
    else:
        report(cell, took[0], took[1])


env = None
for cell in CELLS:
    _, m, S, step = cell
    if env is None or (env.m, env_S) != (m, S):
        env, env_S, rs = make_env(m, S), S, np.random.RandomState(7)
    while env.i < step:
        env.step(rs.permutation(m)[:S] if S > 1 else int(rs.randint(m)))
    measure(env, cell)
