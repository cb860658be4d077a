"""per-step cost of a sensor network's K-step schedule: (a) launch_rollout_sensors in chunks of H - 1, (b) the loop of launch_step_sensors
(one launch per step: deferred fold, no host synchronisation between steps), (c) launch_rollout with one observer.
usage (from the repository root): python profiles/rollout_sensors_cost.py S early|late [reps]   -- wall clock around the synchronised chunk; run under rocprofv3 for the kernels' own time"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import ssa_gym_amd  # noqa: E402
from ssa_gym_amd import _lib, host  # noqa: E402
from ssa_gym_amd import envs as E  # noqa: E402
from support.sensors import SITES8_GEOMETRY, sites_rad  # noqa: E402

S, phase = int(sys.argv[1]), sys.argv[2]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 24
warm = 3
m, H = 20000, 64
cfg = dict(E.env_config)
cfg.update(rso_count=m, steps=480, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3, history=H,
           observers=SITES8_GEOMETRY, sensor_obs_limit=[15, 10, 20, 0, 5, 10, 20, 15],
           sensor_z_sigma=[(1 + 0.5 * k, 1 + 0.5 * k, 1e3) for k in range(8)])
env = E.make('ssa_tasker_simple-v2', config=cfg)
rs = np.random.RandomState(7)
i0 = 0 if phase == "early" else 299
for _ in range(i0):
    env.step(rs.permutation(m)[:8])
e = env._engine
torch.cuda.synchronize()
sp = host.make_sensor_params(env.sensor_lla[:S], env.sensor_obs_limit[:S], env.sensor_R[:S], env.n * m * 3)
K = H - 1
sched = np.stack([rs.permutation(m)[:S] for _ in range(K)]).astype(np.int32)
sched_d = torch.as_tensor(sched).cuda()
one_d = sched_d[:, :1].contiguous()
upd = torch.zeros((H, S, _lib.UPD_STRIDE), dtype=torch.float64, device="cuda")
snap = e.snapshot_state(i0 % H)
rows = [[int(a) for a in r] for r in sched]


def run_a():
    e.launch_rollout_sensors(i0 % H, i0 + 1, sp, sched_d)


def run_b():
    for k in range(K):
        i = i0 + k + 1
        e.launch_step_sensors((i - 1) % H, i % H, i, sp, rows[k], upd[i % H].data_ptr(), fast_stats=True, defer_fold=True)
    e.flush_stats()


def run_c():
    e.launch_rollout(i0 % H, i0 + 1, one_d)


res = {}
order = [("a_rollout_sensors", run_a), ("b_step_sensors_loop", run_b), ("c_rollout_one_observer", run_c)]
times = {k: [] for k, _ in order}
for r in range(warm + reps):          # the three alternate: whatever else the machine does hits them alike
    for name, fn in order:
        e.restore_state(i0 % H, snap)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if r >= warm:
            times[name].append(dt / K * 1e6)
for name, _ in order:
    v = np.array(times[name])
    print("S=%d %-5s %-24s per step [us]: median %7.2f  min %7.2f  max %7.2f  (%d reps of %d steps, %d objects, hybrid)"
          % (S, phase, name, np.median(v), v.min(), v.max(), reps, K, m))
