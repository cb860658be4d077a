"""cost of a sensor network's closed loop per env step: (a) env.run_agent_sensors (lookahead, device assignment and step in-stream, one
read-back per chunk), (b) the host loop agent_info_gain_sensors + step() with the assignment as it was before ssa_assign_sensors_f64 (one
masked arg-max launch and one read-back per sensor), (c) the same host loop with the assignment on the device (one launch, one read-back).
Three twin envs advanced to the same step run the same window of the episode, alternating chunk by chunk.  Then the assignment alone on
the last lookahead's scores: the assign kernel against the S masked arg-max launches it replaces, back to back in one stream.
usage (from the repository root): python profiles/assign_sensors_cost.py S early|late [reps] [kernels]
  wall clock around synchronised chunks; `kernels`: only the assignment alone -- run that under rocprofv3 --kernel-trace for the kernels'
  own time (profiles/assign_sensors_reduce.py)"""
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

S, phase = int(sys.argv[1]), sys.argv[2]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 8
kernels_only = len(sys.argv) > 4 and sys.argv[4] == "kernels"
warm, n_chunk, n_alone = 2, 12, 200
m, H = 20000, 64
cfg = dict(E.env_config)
cfg.update(rso_count=m, steps=480, obs_limit=15, reward_type='trinary', obs_returned='flatten', seed=3, history=H)
if S > 1:
    cfg.update(observers=SITES8_GEOMETRY[:S], sensor_obs_limit=[15, 10, 20, 0, 5, 10, 20, 15][:S],
               sensor_z_sigma=[(1 + 0.5 * k, 1 + 0.5 * k, 1e3) for k in range(S)])
i0 = 0 if phase == "early" else 299


def parent_agent(obs, env, k=_lib.LOOK_INFO_GAIN):
    """agents._assign_lookahead_sensors as it was: S masked arg-max launches, S read-backs, the mask edited on the host in between"""
    score = env.lookahead_sensors()["score"]
    S_, m_ = score.shape[0], score.shape[2]
    flat = score.permute(0, 2, 1).reshape(-1)
    mask = agents._column_mask(env, k, flat.shape[0]).clone()
    rows = mask.view(S_, m_, _lib.LOOK_NSCORE)
    act = np.full(S_, -1, dtype=np.int64)
    for _ in range(S_):
        f = device.masked_argmax(flat, mask)
        if f < 0:
            break
        s, j = divmod(f // _lib.LOOK_NSCORE, m_)
        act[s] = j
        rows[s] = 0
        rows[:, j] = 0
    taken = set(act[act >= 0].tolist())
    for s in np.flatnonzero(act < 0):
        act[s] = agents._draw_unassigned(env, taken)
        taken.add(int(act[s]))
    return act if env.n_sensor > 1 else int(act[0])


def make_env():
    env = E.make('ssa_tasker_simple-v2', config=cfg)
    rs = np.random.RandomState(7)
    for _ in range(i0):
        env.step(rs.permutation(m)[:S] if S > 1 else int(rs.randint(m)))
    return env


def host_loop(env, agent, n):
    for _ in range(n):
        env.step(agent(None, env))


same = True
if not kernels_only:
    envs3 = [make_env() for _ in range(3)]
    order = [("a_run_agent_sensors", lambda env: env.run_agent_sensors("agent_info_gain_sensors", n_chunk)),
             ("b_host_loop_masked_argmax_per_sensor", lambda env: host_loop(env, parent_agent, n_chunk)),
             ("c_host_loop_device_assignment", lambda env: host_loop(env, agents.agent_info_gain_sensors, n_chunk))]
    times = {k: [] for k, _ in order}
    for r in range(warm + reps):          # the three alternate over the same window of the episode
        for (name, fn), env in zip(order, envs3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(env)
            torch.cuda.synchronize()
            if r >= warm:
                times[name].append((time.perf_counter() - t0) / n_chunk * 1e6)
    same = len({env.i for env in envs3}) == 1 and np.array_equal(envs3[0].actions, envs3[1].actions) and \
        np.array_equal(envs3[1].actions, envs3[2].actions)
    print("S=%d %-5s the three variants ran the same episode (same actions at every step): %s" % (S, phase, same))
    for (na, _), ea in zip(order, envs3):       # where two variants part, and with which rows
        for (nb_, _), eb in zip(order, envs3):
            if na < nb_ and not np.array_equal(ea.actions, eb.actions):
                n = min(ea.i, eb.i) + 1
                d = np.flatnonzero((np.asarray(ea.actions[:n]) != np.asarray(eb.actions[:n])).reshape(n, -1).any(axis=1))
                print("S=%d %-5s   %s and %s differ at %d steps (at step i, not yet %d); first at step %d: %s against %s"
                      % (S, phase, na, nb_, len(d), ea.i, d[0], np.asarray(ea.actions[d[0]]).ravel(), np.asarray(eb.actions[d[0]]).ravel()))
    for name, _ in order:
        v = np.array(times[name])
        print("S=%d %-5s %-38s per env step [us]: median %8.2f  min %8.2f  max %8.2f  (%d chunks of %d steps, steps %d..%d, %d objects, hybrid)"
              % (S, phase, name, np.median(v), v.min(), v.max(), reps, n_chunk, i0 + 1 + warm * n_chunk, envs3[0].i, m))
    env = envs3[0]
else:
    env = make_env()

# ---- the assignment alone, on the scores of the lookahead from the state reached
e = env._engine
look = e.launch_lookahead_sensors(env.i % H, env.i + 1, env._sites())
score = look["score"]
flat = score.reshape(-1)
mask = agents._column_mask(env, _lib.LOOK_INFO_GAIN, flat.shape[0])
one = flat[:m].contiguous()
row = torch.empty(_lib.MAX_SENSORS, dtype=torch.int32, device="cuda")


def alone_assign():
    for _ in range(n_alone):
        e.launch_assign_sensors(look, _lib.LOOK_INFO_GAIN, row)


def alone_argmax():        # (the S launches of one assignment, without the read-backs and mask edits between them)
    for _ in range(n_alone * S):
        device.masked_argmax_action(flat, mask)


def alone_argmax_20000():  # (the single-workgroup arg-max over 20 000 entries: the figure include/ssa_hip.h quotes)
    for _ in range(n_alone):
        device.masked_argmax_action(one)


alone = [("assign_sensors_kernel", alone_assign, 1), ("masked_argmax_kernel x S over S*m*3 entries", alone_argmax, 1),
         ("masked_argmax_kernel over 20000 entries", alone_argmax_20000, 1)]
t_alone = {k: [] for k, _, _ in alone}
for r in range(warm + (reps if not kernels_only else 1)):
    for name, fn, _ in alone:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warm:
            t_alone[name].append((time.perf_counter() - t0) / n_alone * 1e6)
for name, _, _ in alone:
    v = np.array(t_alone[name])
    print("S=%d %-5s alone, %d back to back, per assignment [us]: %-46s median %8.2f  min %8.2f  max %8.2f"
          % (S, phase, n_alone, name, np.median(v), v.min(), v.max()))
if not same:        # (exit status 3; the lines above say where two variants part.  With every sensor assigned from its scores the three take
    # the same actions -- which keeps parent_agent, the restated assignment, honest; a sensor without a score takes a draw, each env its own)
    print("the three variants did not take the same actions at every step: see the lines above", file=sys.stderr)
    sys.exit(3)
