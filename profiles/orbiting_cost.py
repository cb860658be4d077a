"""time of a sensor network's step, lookahead and forecast (H = 8) with and without moving sensors (ssa_step_params.site_moving;
DESIGN.md section 8v): 20 000 objects, 8 sites, the default propagator, from the state after 5 steps of an episode.
usage (from the repository root):
  python profiles/orbiting_cost.py off|on [launches]
      off: eight ground sites (runs on any commit that has sensor networks); on: sensors 4 .. 7 ride LEO arcs (the engine's site table
      set by set_site_table: each starts 800 km above a ground site of the network and is propagated by device.propagate), screened by
      line of sight.  Each sensor is tasked to an object it sees, so that all eight updates run.  `launches` (default 60) launches of
      each kernel from the same slot, every one between two events of its own; the first 10 are warm-up.  Quoted: the median, the
      minimum and the two half-medians of the rest (their difference is the run's own drift), in microseconds of device time between
      the events -- a launch's own overhead included, the same on every commit.
  python profiles/orbiting_cost.py reduce TRACE_DIR [launches]
      the kernels' own time of such a run made under `rocprofv3 --kernel-trace --output-format csv -d TRACE_DIR -- python
      profiles/orbiting_cost.py off|on [launches]`: per kernel family the last `launches` dispatches of the trace, the first 10 of them
      dropped, the same four figures (End_Timestamp - Start_Timestamp: no launch overhead)."""
import sys

import numpy as np

if sys.argv[1] == "reduce":
    import csv
    import glob
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 60
    f = glob.glob(sys.argv[2] + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f)))
    for label, key in (("step", "step_sensors_kernel"), ("lookahead", "lookahead_sensors_kernel"), ("forecast", "forecast_sensors_kernel")):
        t = np.array([(b - a) * 1e-3 for a, b, name in rows if key in name][-n:][10:])
        half = len(t) // 2
        print("kernel %-9s median %8.2f us  min %8.2f  halves %8.2f / %8.2f  (%d dispatches)"
              % (label, np.median(t), t.min(), np.median(t[:half]), np.median(t[half:]), len(t)))
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import ssa_gym_amd  # noqa: E402,F401
from ssa_gym_amd import device  # noqa: E402
from ssa_gym_amd import envs as E  # noqa: E402
from support.sensors import SITES8_NETWORK  # noqa: E402

mode, n = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 60
S, m, H, HOR, WARM = 8, 20000, 4, 8, 10
cfg = dict(E.env_config)
cfg.update(rso_count=m, steps=480, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3, history=H,
           observers=SITES8_NETWORK, sensor_obs_limit=[15, 10, 20, 12, 18, 8, 25, 15],
           sensor_z_sigma=[(1 + 0.5 * k, 1 + 0.5 * k, 1e3 / (1 + k)) for k in range(S)])
env = E.make('ssa_tasker_simple-v2', config=cfg)
e = env._engine
if mode == "on":      # (by the engine's table, not by config['observers']: the same script runs on the parent commit for `off`)
    from ssa_gym_amd import host
    MU, radius = 3.986004418e14, host.R_EQ_EARTH + 800e3
    n_time = env.trans_matrix.shape[0]
    enu, obs = np.zeros((n_time, S, 9)), np.zeros((n_time, S, 3))
    for s in range(4, S):
        u = env.trans_matrix[0].T @ host.lla2ecef(env.sensor_lla[s])
        u /= np.linalg.norm(u)
        v = np.cross([0.0, 0.0, 1.0], u)
        x = torch.as_tensor(np.concatenate([radius * u, np.sqrt(MU / radius) * v / np.linalg.norm(v)])[None], device="cuda")
        pos = [x[0, :3].cpu().numpy()]
        for _ in range(n_time - 1):
            x = device.propagate(x, env.dt, env._consts.propagator)
            pos.append(x[0, :3].cpu().numpy())
        enu[:, s], obs[:, s] = host.orbit_site_rows(env.trans_matrix.reshape(-1, 9), np.array(pos))
    e.set_site_table(host.pack_site_rows(enu, obs), [s >= 4 for s in range(S)], host.R_EQ_EARTH + 100e3)
rs = np.random.RandomState(7)
for _ in range(5):
    env.step(rs.permutation(m)[:S])
i = env.i
vis = e.launch_lookahead_sensors(i % H, i + 1, env._sites())["visible"].cpu().numpy().astype(bool)
acts, used = [], set()
for s in range(S):
    j = next(int(j) for j in np.flatnonzero(vis[s]) if int(j) not in used)
    used.add(j)
    acts.append(j)
torch.cuda.synchronize()
st0 = e.status.clone()
upd = torch.zeros((S, 64), dtype=torch.float64, device="cuda")


def timed(launch, after=None):
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        if after:
            after()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    t = np.array(out[WARM:])
    half = len(t) // 2
    return "median %8.2f us  min %8.2f  halves %8.2f / %8.2f  (%d launches)" % (np.median(t), t.min(), np.median(t[:half]), np.median(t[half:]), len(t))


step = timed(lambda: e.launch_step_sensors(i % H, (i + 1) % H, i + 1, env._sensors, acts, upd.data_ptr(), fast_stats=True, fold_inside=True),
             lambda: e.status.copy_(st0))
taken = int((upd.cpu().numpy()[:, 0] == 1.0).sum())
look = timed(lambda: e.launch_lookahead_sensors(i % H, i + 1, env._sites()))
fore = timed(lambda: e.launch_forecast_sensors(i % H, i + 1, env._sites(), HOR))
print("%s: %d objects, %d sites, step %d, actions %s, %d of %d updates taken, visible cells per sensor %s, site_moving %#x"
      % (mode, m, S, i + 1, acts, taken, S, vis.sum(axis=1).tolist(), int(getattr(e, "_site_moving", 0))))
print("%s step      %s" % (mode, step))
print("%s lookahead %s" % (mode, look))
print("%s forecast  %s" % (mode, fore))
