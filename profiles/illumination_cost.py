"""kernel time of a sensor network's step and lookahead with and without the illumination test (ssa_sensor_params.sunlit_only; DESIGN.md
section 8t): 20 000 objects, 8 sites, the default propagator, from the state after 5 steps of an episode.
usage (from the repository root, under rocprofv3 --kernel-trace --stats; reduce the trace with profiles/angles_only_reduce.py):
  python profiles/illumination_cost.py off|on [launches]
      off: no sensor tests the illumination, all radars (runs on any commit that has sensor networks); on: sensors 4 .. 7 see sunlit
      objects only, from dark sites, against a twilight Sun (20 degrees below site 0's horizon: every site dark, the objects lit but for
      those the Earth's shadow holds).  Each sensor is tasked to an object it sees, so that all eight updates run; `launches` (default
      40) launches of step_sensors_kernel, then as many of lookahead_sensors_kernel, each from the same slot."""
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import ssa_gym_amd  # noqa: E402,F401
from ssa_gym_amd import envs as E  # noqa: E402
from support.sensors import SITES8_NETWORK  # noqa: E402

mode, n = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 40
S, m, H = 8, 20000, 4
cfg = dict(E.env_config)
cfg.update(rso_count=m, steps=480, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3, history=H,
           observers=SITES8_NETWORK, sensor_obs_limit=[15, 10, 20, 12, 18, 8, 25, 15],
           sensor_z_sigma=[(1 + 0.5 * k, 1 + 0.5 * k, 1e3 / (1 + k)) for k in range(S)])
env = E.make('ssa_tasker_simple-v2', config=cfg)
e = env._engine
if mode == "on":      # (by the block's words, not by config['sensor_illumination']: the same script runs on the parent commit for `off`)
    from ssa_gym_amd import host
    lat, lon = env.sensor_lla[0][0], env.sensor_lla[0][1]
    up = np.array([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])
    east = np.array([-np.sin(lon), np.cos(lon), 0.0])
    sun = np.array([M.T @ (np.cos(np.radians(110.0)) * up + np.sin(np.radians(110.0)) * east) for M in env.trans_matrix])
    e.set_sun_table(sun, np.full(len(sun), 0xFF, dtype=np.int64), [env._sensors])
    env._sensors.sunlit_only, env._sensors.shadow_radius = 0xF0, host.R_EQ_EARTH
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
for _ in range(n):
    e.launch_step_sensors(i % H, (i + 1) % H, i + 1, env._sensors, acts, upd.data_ptr(), fast_stats=True, fold_inside=True)
    e.status.copy_(st0)
torch.cuda.synchronize()
taken = int((upd.cpu().numpy()[:, 0] == 1.0).sum())
for _ in range(n):
    e.launch_lookahead_sensors(i % H, i + 1, env._sites())
torch.cuda.synchronize()
print("%s: %d objects, %d sites, step %d, actions %s, %d of %d updates taken, visible cells per sensor %s, sunlit_only word %#x, "
      "%d launches of each kernel" % (mode, m, S, i + 1, acts, taken, S, vis.sum(axis=1).tolist(), int(getattr(env._sensors, "sunlit_only", 0)), n))
