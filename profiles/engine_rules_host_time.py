"""Host time per call of HotPathEngine.launch_step_sensors_envs and launch_assign_sensors_envs, which bench.py does not time, on one
engine (E = 8, m = 2000, S = 3): time.perf_counter around 2000 enqueues between two synchronisations, three times each (`enqueue_us`;
`with_sync_us` includes the wait for the last kernel).  The numbers of engine_rules_bench_parent_change.txt.

    python profiles/engine_rules_host_time.py ROOT OUT.json

ROOT: the checkout whose package is measured (`.`, or a built worktree of another commit: the test helpers are this checkout's)."""
import json
import os
import sys
import time

root, out = os.path.abspath(sys.argv[1]), sys.argv[2]
here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import ssa_gym_amd  # noqa: E402  (first: the support modules below then find THIS package)
assert os.path.dirname(os.path.dirname(ssa_gym_amd.__file__)) == root, ssa_gym_amd.__file__
sys.path.append(os.path.join(here, "tests"))
import numpy as np  # noqa: E402
from support.gpu import namespace  # noqa: E402
from support.vector_lookahead import Engines  # noqa: E402

hip = namespace()
assert os.path.dirname(os.path.dirname(hip.engine.__file__)) == root, hip.engine.__file__
torch, L = hip.torch, hip.lib
E, m, S, N = 8, 2000, 3, 2000
X = Engines(hip, E, m, S, history=2, nan=False)
eng = X.vec
acts = np.random.RandomState(3).randint(0, m, size=(E, S))
res = {"root": root}


def timed(fn):
    for k in range(200):
        fn(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(N):
        fn(k)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t1 - t0) / N * 1e6, (t2 - t0) / N * 1e6


def step(k):
    eng.launch_step_sensors_envs(k % 2, (k + 1) % 2, 0, X.sp, acts, 0, env_words=[t + 1 + k % 8 for t in X.t0], fast_stats=True)


look = eng.launch_lookahead_sensors_envs(0, 1, X.sp)
torch.cuda.synchronize()


def assign(k):
    eng.launch_assign_sensors_envs(look, L.LOOK_INFO_GAIN)


for rep in range(3):
    for name, fn in (("launch_step_sensors_envs", step), ("launch_assign_sensors_envs", assign)):
        enq, tot = timed(fn)
        res.setdefault(name, []).append({"enqueue_us": round(enq, 3), "with_sync_us": round(tot, 3)})
print(json.dumps(res))
with open(out, "w") as f:
    json.dump(res, f)
