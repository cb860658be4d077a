"""cost and worth of a sensor network's OPTIMAL assignment (ssa_match_sensors_f64) against the greedy one of
the same commit, on the same lookahead scores at 20 000 objects, by the method of profiles/assign_sensors_cost.py.
usage (from the repository root):
  python profiles/match_sensors_cost.py S early|late [reps] [kernels]
      an env advanced to step 0 / 299; on the scores of its next lookahead, 200 launches of each kernel back to back in one stream, wall
      clock around the synchronised batch; also the number of columns (distinct objects of the S x S table) the dynamic programme walks.
      `kernels`: one round only -- run that under rocprofv3 --kernel-trace for the kernels' own time (profiles/match_sensors_reduce.py)
  python profiles/match_sensors_cost.py 8 gain
      one 480-step episode with 8 sites, stepped with the optimal rows: per step both rules' total information gain on the same
      lookahead (math.fsum of the picks), how often and by how much the optimal rule beats the greedy one"""
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
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 8
kernels_only = len(sys.argv) > 4 and sys.argv[4] == "kernels"
warm, n_alone = 2, 200
m, H = 20000, 64
cfg = dict(E.env_config)
cfg.update(rso_count=m, steps=480, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3, history=H)
if S > 1:
    cfg.update(observers=SITES8_GEOMETRY[:S], sensor_obs_limit=[15, 10, 20, 0, 5, 10, 20, 15][:S],
               sensor_z_sigma=[(1 + 0.5 * k, 1 + 0.5 * k, 1e3) for k in range(S)])
col = _lib.LOOK_INFO_GAIN
env = E.make('ssa_tasker_simple-v2', config=cfg)
e = env._engine
W = _lib.MAX_SENSORS


def rows_of(look):
    """both rules' rows and picks on one lookahead, read back"""
    out = {}
    for rule in ("greedy", "optimal"):
        row = torch.empty(W, dtype=torch.int32, device="cuda")
        picks = torch.empty((W, 2), dtype=torch.int64, device="cuda")
        e.launch_assign_sensors(look, col, row, picks=picks, rule=rule)
        p = picks.cpu().numpy()
        out[rule] = (row.cpu().numpy()[:S].astype(np.int64), math.fsum(p[:S, 1][p[:S, 0] >= 0].copy().view(np.float64).tolist()),
                     int((p[:S, 0] >= 0).sum()))
    return out


if phase == "gain":
    better, more, worse, rel, abs_gain, tot_g, tot_o = 0, 0, 0, [], [], 0.0, 0.0
    n = 0
    while env.i + 1 < env.n:
        look = e.launch_lookahead_sensors(env.i % H, env.i + 1, env._sites())
        r = rows_of(look)
        (g_row, g_tot, g_n), (o_row, o_tot, o_n) = r["greedy"], r["optimal"]
        n += 1
        more += o_n > g_n
        if o_n == g_n and o_tot > g_tot:
            better += 1
            rel.append((o_tot - g_tot) / g_tot)
            abs_gain.append(o_tot - g_tot)
        worse += o_n < g_n or (o_n == g_n and o_tot < g_tot)
        tot_g += g_tot
        tot_o += o_tot
        act = o_row.copy()
        taken = set(act[act >= 0].tolist())
        for s in np.flatnonzero(act < 0):
            act[s] = agents._draw_unassigned(env, taken)
            taken.add(int(act[s]))
        _, _, done, _ = env.step(act)
        if done:
            break
    rel, abs_gain = np.array(rel), np.array(abs_gain)
    print("S=%d gain: %d steps of one episode (%d objects, hybrid), stepped with the optimal rows" % (S, n, m))
    print("S=%d gain: the optimal rule tasked more sensors at %d steps; same count and a strictly larger total at %d steps (%.1f %%); "
          "fewer sensors or a smaller total at %d" % (S, more, better, 100.0 * better / n, worse))
    if len(rel):
        print("S=%d gain: where larger, by [nat] median %.4g  mean %.4g  max %.4g; relative to the greedy total: median %.3g %%  max %.3g %%"
              % (S, np.median(abs_gain), abs_gain.mean(), abs_gain.max(), 100 * np.median(rel), 100 * rel.max()))
    print("S=%d gain: sum over the episode of the per-step totals [nat]: greedy %.6f  optimal %.6f  (+%.4f %%)"
          % (S, tot_g, tot_o, 100.0 * (tot_o - tot_g) / tot_g))
    sys.exit(0)

rs = np.random.RandomState(7)
for _ in range(0 if phase == "early" else 299):
    env.step(rs.permutation(m)[:S] if S > 1 else int(rs.randint(m)))
look = e.launch_lookahead_sensors(env.i % H, env.i + 1, env._sites())
sc = look["score"].cpu().numpy()[:, :, col]
top = set()
for s in range(S):                                   # the S x S table's distinct objects: the columns of the dynamic programme
    ok = np.flatnonzero(np.isfinite(sc[s]))
    top |= set(ok[np.argsort(-sc[s, ok], kind="stable")[:S]].tolist())
r = rows_of(look)
print("S=%d %-5s step %d: %d columns; greedy row %s total %.9g; optimal row %s total %.9g"
      % (S, phase, env.i + 1, len(top), r["greedy"][0].tolist(), r["greedy"][1], r["optimal"][0].tolist(), r["optimal"][1]))
row = torch.empty(W, dtype=torch.int32, device="cuda")


def alone(rule):
    for _ in range(n_alone):
        e.launch_assign_sensors(look, col, row, rule=rule)


names = [("assign_sensors_kernel", "greedy"), ("match_sensors_kernel", "optimal")]
t = {k: [] for k, _ in names}
for k in range(warm + (reps if not kernels_only else 1)):
    for name, rule in names:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        alone(rule)
        torch.cuda.synchronize()
        if k >= warm:
            t[name].append((time.perf_counter() - t0) / n_alone * 1e6)
med = {}
for name, _ in names:
    v = np.array(t[name])
    med[name] = np.median(v)
    print("S=%d %-5s alone, %d back to back, per assignment [us]: %-24s median %8.2f  min %8.2f  max %8.2f"
          % (S, phase, n_alone, name, np.median(v), v.min(), v.max()))
print("S=%d %-5s match / assign (wall clock, back to back): %.2f" % (S, phase, med["match_sensors_kernel"] / med["assign_sensors_kernel"]))
