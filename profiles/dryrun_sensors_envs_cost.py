"""cost of the dry run of candidate schedules in a vector env (ssa_dryrun_gather_f64 + ssa_dryrun_sensors_envs_f64; DESIGN.md section
8q) at 8 x 20 000 objects, hybrid, K = 8.
usage (from the repository root):
  python profiles/dryrun_sensors_envs_cost.py S[,S...] early|late|both [reps] [kernels]
      a vector env of 8 envs and 8 single envs in the same states (the vector env's noise draws), advanced to step 2 / 300; B = 1, 64
      candidates per env (each env's horizon-wide plan with, per candidate, one to three slots redrawn from the objects visible there).
      Wall clock around the synchronised call, alternating, 3 warm-ups, then `reps` (20) repetitions, median [min .. max]:
        a  vec.evaluate_schedules(cand[E, B, K, S])
        b  the 8 single envs each calling evaluate_schedules(cand[e]) -- the only way before this change
        c  a, with the gathered block made by torch index ops as the single env's launch makes it (below; in this script only):
           what the gather kernel saves
      `kernels`: a few untimed repetitions of a -- run that under rocprofv3 --kernel-trace"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import ssa_gym_amd  # noqa: E402,F401
from ssa_gym_amd import _lib, agents, device  # noqa: E402
from ssa_gym_amd import envs as E  # noqa: E402
from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv  # noqa: E402
from support.sensors import SITES8_GEOMETRY  # noqa: E402
from support.vector_lookahead import single_envs  # noqa: E402

sensors = [int(v) for v in sys.argv[1].split(",")]
mode = sys.argv[2]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
kernels_only = len(sys.argv) > 4 and sys.argv[4] == "kernels"
warm, m, NE, HOR = 3, 20000, 8, 8
col = _lib.LOOK_INFO_GAIN


def config(S):
    cfg = dict(E.env_config)
    cfg.update(rso_count=m, steps=480, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3)
    if S > 1:
        cfg.update(observers=SITES8_GEOMETRY[:S], sensor_obs_limit=[15, 10, 20, 0, 5, 10, 20, 15][:S],
                   sensor_z_sigma=[(1 + 0.5 * k, 1 + 0.5 * k, 1e3) for k in range(S)])
    return cfg


def candidates(vec, B, rs):
    """every env's horizon-wide plan, and B - 1 copies of it with one to three slots redrawn from the objects visible there"""
    S = vec.n_sensor
    plan = agents.plan_info_gain_sensors_horizon(vec, HOR)                                   # [E, K, S]
    ok = ~torch.isnan(vec.forecast_sensors(HOR)["score"][..., col]).cpu().numpy()            # [E, K, S, m]
    cand = np.repeat(plan[:, None], B, axis=1)
    for e in range(NE):
        for b in range(1, B):
            for _ in range(1 + b % 3):
                k, s = divmod(int(rs.randint(HOR * S)), S)
                pool = np.flatnonzero(ok[e, k, s])
                if len(pool):
                    cand[e, b, k, s] = pool[rs.randint(len(pool))]
    return cand


def torch_gather_call(vec, a):
    """vec.evaluate_schedules with HotPathEngine.launch_dryrun_sensors' torch index ops in the gather kernel's place: the same upload,
    the same dry-run launch, the same totals"""
    e, S = vec._eng, vec.n_sensor
    EB = a.shape[0] * a.shape[1]
    ids, words = device.dryrun_rows(a.reshape((EB,) + a.shape[2:]), e.m, S)
    K, W, B = int(words.shape[0]), int(ids.shape[1]), a.shape[1]
    key = ("torch", EB, K, S, W)
    buf = e._dry_envs.get(key)
    if buf is None:
        buf = e._dry_envs[key] = {"dev": torch.empty(K * EB * _lib.MAX_SENSORS + EB * W + e.E, dtype=torch.int32, device=e.dev),
                                  "out": torch.empty((K, EB, S, _lib.DRY_STRIDE), dtype=torch.float64, device=e.dev),
                                  "base": (torch.arange(e.E, device=e.dev) * e.m).repeat_interleave(B).view(EB, 1)}
    nw, ni = K * EB * _lib.MAX_SENSORS, EB * W
    up = np.concatenate((words.reshape(-1), ids.reshape(-1), (vec.i + 1).astype(np.int32)))
    with torch.cuda.stream(vec._stream):
        buf["dev"].copy_(torch.from_numpy(up))
        dev_ids = buf["dev"][nw:nw + ni].view(EB, W)
        rows = (torch.where(dev_ids >= 0, dev_ids, dev_ids[:, :1].clamp(min=0).expand(EB, W)).to(torch.int64) + buf["base"]).reshape(-1)
        if e._order is not None:
            rows = e._slot_of.index_select(0, rows)
        sl = vec.tick % e.H
        g = (e.x_true[sl].index_select(0, rows), e.x_filter[sl].index_select(0, rows), e.P_filter[sl].index_select(0, rows),
             e.status.index_select(0, rows), buf["dev"][nw + ni:].repeat_interleave(B))
        p = e._lookahead_params(sl, 0)
        p.n_obj, p.n_env = W, EB
        p.x_true_in, p.x_in, p.P_in, p.status = (t.data_ptr() for t in g[:4])
        p.env_time, p.obj_ids = g[4].data_ptr(), dev_ids.data_ptr()
        device.dryrun_sensors(e.consts, p, vec._sites(), buf["dev"][:nw].view(K, EB, _lib.MAX_SENSORS), K, e.m, out=buf["out"])
        total = device.dryrun_totals(buf["out"])
        rec = buf["out"].view(K, e.E, B, S, _lib.DRY_STRIDE).permute(1, 2, 0, 3, 4)
        return {"score": rec[..., _lib.DRY_SCORE:_lib.DRY_SCORE + 3], "taken": rec[..., _lib.DRY_TAKEN] != 0, "visible": rec[..., _lib.DRY_VISIBLE] != 0,
                "status": rec[..., _lib.DRY_STATUS].to(torch.int32), "action": rec[..., _lib.DRY_ACTION].to(torch.int64),
                "total": total.view(e.E, B, 3), "keep": g}


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
        print("%s  %-36s wall clock [us]: median %8.1f  [%8.1f .. %8.1f]  (%d reps)" % (label, name, np.median(v), v.min(), v.max(), len(v)))
    return med


for S in sensors:
    cfg = config(S)
    vec = SSA_Tasker_VecEnv(dict(cfg, obs_device=True), NE, seed=10)      # (the vector env's observations stay on the device)
    vec.single_action_space.seed(11)
    singles = [] if kernels_only else single_envs(E, cfg, vec, 10)
    rs = np.random.RandomState(7)
    for phase in (["early", "late"] if mode == "both" else [mode]):
        while vec.i[0] < (2 if phase == "early" else 300):
            acts = np.stack([rs.permutation(m)[:S] for _ in range(NE)]) if S > 1 else rs.randint(m, size=NE)
            vec.step(acts)
            for e, one in enumerate(singles):
                one.step(acts[e] if S > 1 else int(acts[e]))
        i = vec.i.copy()
        for B in (1, 64):
            cand = candidates(vec, B, np.random.RandomState(B))
            ids, _ = device.dryrun_rows(cand.reshape(NE * B, HOR, S), m, S)
            label = "S=%d %-5s step %3d B=%2d" % (S, phase, i[0], B)
            if kernels_only:
                for _ in range(reps):
                    vec.evaluate_schedules(cand)
                torch.cuda.synchronize()
                print("%s  K=%d: W = %d rows per candidate, %d candidates (%d wavefronts of the dry run, %d workgroups of the gather): %d "
                      "untimed repetitions of vec.evaluate_schedules" % (label, HOR, ids.shape[1], NE * B, NE * B * ids.shape[1] // 4,
                                                                         -(-NE * B * ids.shape[1] // 8), reps))
                continue
            r = vec.evaluate_schedules(cand)
            t = torch_gather_call(vec, cand)
            one = [singles[e].evaluate_schedules(cand[e]) for e in range(NE)]
            torch.cuda.synchronize()
            same = all(torch.equal(r[k].contiguous().view(torch.uint8 if r[k].dtype == torch.bool else r[k].dtype).view(-1),
                                   t[k].contiguous().view(torch.uint8 if t[k].dtype == torch.bool else t[k].dtype).view(-1)) for k in ("taken", "action", "status"))
            same = same and torch.equal(r["total"].view(torch.int64), t["total"].contiguous().view(torch.int64))
            same1 = all(torch.equal(r["total"][e].view(torch.int64), one[e]["total"].view(torch.int64)) for e in range(NE))
            print("%s  K=%d: W = %d rows per candidate, %d candidates (%d wavefronts), %d of %d slots taken in env 0's candidate 0, its total "
                  "%.6f nat; equal to the torch-gather form: %s; totals equal to the single envs': %s"
                  % (label, HOR, ids.shape[1], NE * B, NE * B * ids.shape[1] // 4, int(r["taken"][0, 0].sum()), HOR * S,
                     float(r["total"][0, 0, col]), same, same1))
            fns = {"a_vec_evaluate_schedules": lambda: vec.evaluate_schedules(cand),
                   "b_eight_single_envs": lambda: [singles[e].evaluate_schedules(cand[e]) for e in range(NE)],
                   "c_vec_with_torch_index_gather": lambda: torch_gather_call(vec, cand)}
            med = timed(fns, label)
            print("%s  a / b = %.3f   a / c = %.3f   (c - a = %.1f us: what the gather kernel saves)"
                  % (label, med["a_vec_evaluate_schedules"] / med["b_eight_single_envs"],
                     med["a_vec_evaluate_schedules"] / med["c_vec_with_torch_index_gather"],
                     med["c_vec_with_torch_index_gather"] - med["a_vec_evaluate_schedules"]))
        assert np.array_equal(vec.i, i)
