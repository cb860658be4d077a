"""Device-side versions of the reference's heuristic agents (agents.py:7-81), same names and
`agent(obs, env)` signature.  The reference evaluates them with Python loops over all objects
(`visible_objects()` + list comprehensions over `env.P_filter[env.i]`), which at 20 000 objects costs
as much as the env step itself; here one kernel produces the visibility mask and
the per-object scores from the HBM-resident state and a second one does the masked arg-max, so an
agent call moves 16 bytes to the host.

Deviations: objects whose score is NaN are skipped by the arg-max; numpy's argmax would return the first NaN's index.  The
Shannon score log(det P / det P_prev) comes from plain Cholesky factors (ssa_hip.h, ssa_agent_scores_f64) and is NaN whenever
either factorisation fails, not only where the ratio of determinants is <= 0.  A matrix with two negative eigenvalues (det > 0)
therefore gets no score here but a finite one in the reference; in a filter's own covariances this happens late in an episode
(1-3 objects per step of the seed-7 test episode from step 300 on), on matrices whose negative eigenvalue is at rounding level
(at most 3e-16 of the largest, diagonal entries 1e18 .. 1e21), where the reference's score is set by rounding, not by the
filter.  On those steps the two agents may pick different objects.

The lookahead agents of a sensor network (agent_info_gain_sensors, agent_trace_gain_sensors) also take a vector env
(SSA_Tasker_VecEnv) and then return [E, S]: one lookahead launch and one assignment launch for all envs and one read-back of
E x 32 bytes; vec.step_agent(agent) is the vector step that takes their rows without the host in between.
The planners (plan_info_gain_sensors, plan_trace_gain_sensors) take a vector env too and then return [E, H', S] (section 8k); so do
the horizon-wide optimal planners (plan_info_gain_sensors_horizon, plan_trace_gain_sensors_horizon; section 8o)."""
import numpy as np

from . import _lib


def _scores(env):
    """(scores[4, m], mask[m]) on the device for the env's current step."""
    return env.agent_scores()


def _pick(env, row, masked=True):
    from . import device
    scores, mask = _scores(env)
    j = device.masked_argmax(scores[row], mask if masked else None)
    return j if j >= 0 else env.action_space.sample()


def agent_naive_greedy(obs, env=None):          # agents.py:7  argmax trace(P)
    return _pick(env, 0, masked=False)


def agent_naive_random(obs=None, env=None):     # agents.py:12
    return env.action_space.sample()


def agent_shannon(obs, env):                    # agents.py:15  argmax log(det P_i / det P_{i-1}) over visible
    return _pick(env, 1)


def agent_visible_random(obs, env):             # agents.py:29
    visible = env.visible_objects()
    if not np.any(visible):
        return env.action_space.sample()
    return int(np.random.choice(visible))


def agent_visible_greedy(obs, env):             # agents.py:36  argmax trace(P) over visible
    return _pick(env, 0)


def agent_visible_greedy_spoiled(obs, env, p=0.25):   # agents.py:46
    greedy = _pick(env, 0)
    rand = env.action_space.sample()
    return int(np.random.choice(a=[greedy, rand], p=[1 - p, p]))


def agent_visible_greedy_aer(obs, env):         # agents.py:58  (trace P is the 4th aer-obs column)
    return _pick(env, 0)


def agent_pos_error_greedy(obs, env):           # agents.py:66
    return _pick(env, 2)


def agent_vel_error_greedy(obs, env):           # agents.py:75
    return _pick(env, 3)


# ---- one-step lookahead agents (no reference counterpart): the standard SSA tasking baseline -- task the object whose observation
# would shrink its uncertainty most -- from env.lookahead(): every object's hypothetical update in one launch, then ONE masked arg-max
# over the score column (NaN = not visible / failed, skipped), 16 bytes to the host.  run_agent has no persistent form of these.
def _column_mask(env, k, n):
    """uint8 mask over the [m][3] score rows that selects column k (built once per env)"""
    import torch
    cache = env.__dict__.setdefault("_look_cols", {})
    if (k, n) not in cache:
        msk = torch.zeros(n, dtype=torch.uint8, device="cuda")
        msk[k::3] = 1
        cache[(k, n)] = msk
    return cache[(k, n)]


def _pick_lookahead(env, k):
    from . import device
    flat = env.lookahead()["score"].t().reshape(-1)      # (the engine's [m][3] rows: a view, no copy)
    j = device.masked_argmax(flat, _column_mask(env, k, flat.shape[0]))
    return j // _lib.LOOK_NSCORE if j >= 0 else env.action_space.sample()


def agent_info_gain(obs, env):                  # argmax 1/2 ln(det P- / det P+) over the objects an update would reach
    return _pick_lookahead(env, _lib.LOOK_INFO_GAIN)


def agent_trace_gain(obs, env):                 # argmax tr P- - tr P+ over the objects an update would reach
    return _pick_lookahead(env, _lib.LOOK_TRACE_GAIN)


# ---- the same baselines for a sensor network (config['observers']): every sensor's lookahead in one launch
# (env.lookahead_sensors), then a global greedy assignment over the [S, m] score column -- the largest finite score (ties: the lowest
# s * m + j, the masked arg-max's first maximum) assigns its object to its sensor, that sensor's row and that object's column leave,
# and so on: ONE launch for all the rounds (ssa_assign_sensors_f64) and one 32-byte read-back.  A sensor left
# without a finite score gets an object nobody has, drawn from the action space's generator as _pick's fallback (env.np_random, the
# env's noise stream, is not touched).  env.run_agent_sensors runs the same agents without the host in the loop.
# On a vector env (SSA_Tasker_VecEnv) the same two agents return [E, S]: ONE lookahead launch and ONE assignment
# launch for all envs (ssa_lookahead_sensors_envs_f64, ssa_assign_sensors_envs_f64) and one read-back of E x 32 bytes; a sensor left
# without an object draws by the same rule from single_action_space, envs in ascending order (the envs' own generators are not touched).
# vec.step_agent(agent) is the step that takes the rows without the host in between.
#
# Every rule below is written ONCE, over arrays with a leading env axis: a single env is the batch of one, the
# axis added on the way in (_lift) and taken off on the way out (_strip).  Where the two kinds of env differ, both classes answer the same
# methods -- assign_sensors, _tasking_stream, _forecast_scores, _slab_assigner, _plan_table -- so this module asks the env, never the
# env's engine, and every launch stays the env's own: a single env's the one-env entries, a vector env's the *_envs ones.
def _num_envs(env):
    """E of a vector env (SSA_Tasker_VecEnv), None for a single env: the one place in this module that tells the two apart"""
    return getattr(env, "num_envs", None)


def _lift(env, x):
    """x with the env axis in front: a vector env's own, a single env's as the batch of one (a view)"""
    return x[None] if _num_envs(env) is None else x


def _strip(env, x):
    return x[0] if _num_envs(env) is None else x


def _steps_left(env):
    """the steps every env still has in its episode: one horizon for all envs"""
    return int(env.n - 1 - np.max(env.i))


def _need_device_state(env, why):
    if (env._engine if _num_envs(env) is None else env._eng) is None:
        raise _lib.SsaHipError("no device state: %s (no CPU fallback)" % why)


def _draw_unassigned(env, taken):
    if len(taken) >= env.m:
        raise ValueError("%d sensors but %d objects: no object left to assign" % (len(taken) + 1, env.m))
    space = env.action_space if _num_envs(env) is None else env.single_action_space
    while True:
        for j in np.atleast_1d(space.sample()):
            if int(j) not in taken:
                return int(j)


def _plan_copy(env, plan):
    """an int64 C-order copy of a plan: [H', S], one env's rows, or [E, H', S], every env's -- the rank decides, not the env's kind"""
    plan = np.array(plan, dtype=np.int64, order='C')
    E = _num_envs(env) or 1
    if plan.ndim not in (2, 3) or (plan.ndim == 3 and plan.shape[0] != E):
        raise ValueError("a plan is [H', S], one env's, or every env's, [%d, H', S]: got shape %s" % (E, plan.shape))
    return plan


def _fill_plan(env, plan):
    """the -1 entries of a plan [H', S] filled row by row, sensors ascending: an object no sensor of that row holds, drawn from the
    action space's generator (env.np_random and a vector env's _rng are not touched).  Such a sensor has no healthy visible object left
    at that step, so its draw updates nothing the forecast counted on.  A plan [E, H', S] is filled env by env, envs ascending, from
    the one generator (a vector env's single_action_space); the rows of one assignment, [S] per env, are a plan of one step."""
    plan = _plan_copy(env, plan)
    for row in plan.reshape(-1, plan.shape[-1]):            # (a view: envs ascending, rows ascending)
        taken = set(row[row >= 0].tolist())
        for s in np.flatnonzero(row < 0):
            row[s] = _draw_unassigned(env, taken)
            taken.add(int(row[s]))
    return plan


def _assign_lookahead_sensors(env, k, rule='greedy'):
    # the rounds above on the device (env.assign_sensors: no fallback words, int64 [S] or [E, S], -1 where the scores leave a sensor
    # without an object), the -1 entries filled as a plan of one step per env: envs ascending, sensors ascending
    acts = env.assign_sensors(k) if rule == 'greedy' else env.assign_sensors(k, rule=rule)
    acts = _strip(env, _fill_plan(env, _lift(env, acts)))
    return acts if env.n_sensor > 1 or _num_envs(env) is not None else int(acts[0])      # (one sensor: a Discrete action, as agent_info_gain's)


def agent_info_gain_sensors(obs, env):          # one object per sensor, greedy over 1/2 ln(det P- / det P+) from every site
    return _assign_lookahead_sensors(env, _lib.LOOK_INFO_GAIN)


def agent_trace_gain_sensors(obs, env):         # one object per sensor, greedy over tr P- - tr P+ from every site
    return _assign_lookahead_sensors(env, _lib.LOOK_TRACE_GAIN)


# ... and with the exact one-step optimum where the greedy rounds were (ssa_match_sensors_f64 / ssa_match_sensors_envs_f64; DESIGN.md
# section 8n): as many sensors tasked as the finite scores allow, then the largest sum of gains -- the upper bound of every myopic rule.
# The launches, the read-back and the host's fill of the -1 entries are those of the greedy twins.
def agent_info_gain_sensors_optimal(obs, env):  # one object per sensor, the largest total 1/2 ln(det P- / det P+)
    return _assign_lookahead_sensors(env, _lib.LOOK_INFO_GAIN, 'optimal')


def agent_trace_gain_sensors_optimal(obs, env):  # one object per sensor, the largest total tr P- - tr P+
    return _assign_lookahead_sensors(env, _lib.LOOK_TRACE_GAIN, 'optimal')


# ---- non-myopic planning for a sensor network: the schedules env.rollout_sensors() executes.  ONE forecast
# launch (env.forecast_sensors: every sensor's lookahead at each of the next H' steps, nobody observed in between), then the global
# greedy assignment above on slab h for h = 0 .. H'-1 in order (ssa_assign_sensors_f64 on the slab's base address), with the objects
# planned at an earlier step of this plan removed from the slab first: the forecast's gains assume no update before h, so an object
# is planned at most once per plan.  Everything in-stream, one read-back at the end.  No device fallback row: a sensor the scores leave
# without an object comes back -1 and is filled here by _assign_lookahead_sensors' rule.
# On a vector env (SSA_Tasker_VecEnv) the same two planners return [E, H', S] -- plan[:, h] is what vec.step()
# takes at step h, and the whole plan is what vec.rollout_sensors() takes (section 8l): ONE forecast launch for all envs (ssa_forecast_sensors_envs_f64), then per step ONE assignment launch for all envs
# on the contiguous slab h, each env's earlier picks removed from its own part of the slab; one read-back, the -1 entries filled per
# env, envs ascending, from single_action_space.
def _plan_rows(env, table):
    """an int32 device table [H', E, MAX_SENSORS] of a planner as the plan it stands for: int64 [H', S] ([E, H', S] of a vector env)"""
    return _strip(env, np.ascontiguousarray(table.cpu().numpy()[:, :, :env.n_sensor].astype(np.int64).transpose(1, 0, 2)))


def _plan_assigned(env, horizon, k, rule='greedy'):
    """the device's part of a plan: int64 [H', S] ([E, H', S] of a vector env), -1 where the scores leave a sensor without an object.
    ONE forecast launch for all envs, then per step ONE assignment launch for all envs on the contiguous slab score[h] = [E, S, m, 3],
    into row h of a table of the planner's own (not the engine's action table); what an env planned at an earlier step is NaN in a copy
    of its part of the slab."""
    import torch
    cur = env._tasking_stream()
    with torch.cuda.stream(cur):
        score = env._forecast_scores(horizon)                      # [H', E, S, m, 3]
        Hp, E, S, m = score.shape[:4]
        assign = env._slab_assigner(score)
        rows = torch.full((Hp, E, _lib.MAX_SENSORS), -1, dtype=torch.int32, device=score.device)
        planned = torch.zeros((E, m + 1), dtype=torch.bool, device=score.device)     # (slot m: where the -1 entries of a row land)
        for h in range(Hp):
            slab = score[h] if h == 0 else score[h].masked_fill(planned[:, :m].view(E, 1, m, 1), float("nan"))
            assign(slab, k, rows[h], rule)
            r = rows[h].long()
            planned.scatter_(1, torch.where(r >= 0, r, torch.full_like(r, m)), True)      # (env e's picks into env e's row)
    cur.synchronize()
    return _plan_rows(env, rows)


def _plan_lookahead_sensors(env, horizon, k, rule='greedy'):
    from . import device
    device.assign_entry(rule)                              # (an unknown rule: refused before anything else)
    _need_device_state(env, "a plan comes from the forecast, which runs on the GPU only")
    return _fill_plan(env, _plan_assigned(env, horizon, k, rule))


def plan_info_gain_sensors(env, horizon, rule='greedy'):       # a schedule [H', S] for env.rollout_sensors() ([E, H', S] of a vector
                                                               # env): greedy over 1/2 ln(det P- / det P+) per step
    """rule='optimal': each step's row is the exact optimum of its masked slab (ssa_match_sensors_f64) instead of the greedy rounds.
    A single env runs the plan with env.rollout_sensors(plan); a vector env's plan [E, H', S] runs with vec.rollout_sensors(plan)
    (DESIGN.md section 8l): one launch per chunk, stopping after the first step at which any env is done."""
    return _plan_lookahead_sensors(env, horizon, _lib.LOOK_INFO_GAIN, rule)


def plan_trace_gain_sensors(env, horizon, rule='greedy'):      # ... over tr P- - tr P+
    return _plan_lookahead_sensors(env, horizon, _lib.LOOK_TRACE_GAIN, rule)


# ---- the horizon-wide optimal plan: the forecast's gains are gains of a FIRST observation, so an object is
# planned at most once per plan, and that makes the whole plan ONE assignment problem over its H' * S (step, sensor) slots -- the most
# slots filled, then the largest total gain (ssa_plan_sensors_f64).  The planners above commit step 0 before they look at step 1 (an
# object that is best now and almost as good later is taken now, and the object that sets before the next step is lost); these do not.
# ONE forecast launch, ONE plan launch, ONE read-back.  H' * S is at most _lib.MAX_PLAN_SLOTS.
def _fill_plan_horizon(env, plan):
    """the -1 entries of a horizon-wide plan [H', S] filled, steps ascending, sensors ascending, from the action space's generator as
    _draw_unassigned draws (env.np_random is not touched).  _fill_plan's rule would be wrong here: an idle slot can coexist with an
    object that is visible now and planned LATER, and tasking it now would make its later forecast gain false.  So a filled slot gets an
    object that appears NOWHERE in this env's plan (planned or filled, at any step).  Such an object cannot be a candidate of that slot
    -- the plan would have filled the slot with it --, so its draw updates nothing the plan counts on.  If every object appears in the
    plan already (fewer objects than slots can make it so), the row rule of _fill_plan is all that is left: an object no sensor of that
    row holds.  A plan [E, H', S] is filled env by env, envs ascending, each env with its own set of objects in use."""
    plan = _plan_copy(env, plan)
    for one in plan.reshape((-1,) + plan.shape[-2:]):       # (views: envs ascending)
        used = set(one[one >= 0].tolist())
        for row in one:
            for s in np.flatnonzero(row < 0):
                taken = used if len(used) < env.m else set(row[row >= 0].tolist())
                row[s] = _draw_unassigned(env, taken)
                used.add(int(row[s]))
    return plan


def _plan_horizon_steps(env, horizon):
    """H' of the forecast a plan would come from, with the cap on H' * S checked: before any launch, before the device state is asked for"""
    from . import device
    if int(horizon) < 1:
        raise ValueError("forecast_sensors: a horizon of at least one step, got %r" % (horizon,))
    Hp = min(int(horizon), _steps_left(env))
    device.check_plan_slots(Hp, env.n_sensor)
    return Hp


def _plan_horizon_assigned(env, horizon, k):
    """the device's part of a horizon-wide plan: int64 [H', S] ([E, H', S] of a vector env), -1 in the slots the plan leaves idle"""
    import torch
    cur = env._tasking_stream()
    with torch.cuda.stream(cur):
        table = env._plan_table(horizon, k)                 # [H', E, MAX_SENSORS]: the forecast's launch, then the plan's
    cur.synchronize()
    return _plan_rows(env, table)


def _plan_horizon(env, horizon, k):
    _plan_horizon_steps(env, horizon)
    _need_device_state(env, "a plan comes from the forecast, which runs on the GPU only")
    return _fill_plan_horizon(env, _plan_horizon_assigned(env, horizon, k))


def plan_info_gain_sensors_horizon(env, horizon):              # a schedule [H', S] for env.rollout_sensors() ([E, H', S] of a vector
                                                               # env, for vec.rollout_sensors()): the plan-wide optimum of 1/2 ln(det P- / det P+)
    """the most (step, sensor) slots filled, then the largest total gain over the whole horizon, no object twice (ssa_plan_sensors_f64;
    DESIGN.md section 8o).  H' * S > MAX_PLAN_SLOTS is a ValueError."""
    return _plan_horizon(env, horizon, _lib.LOOK_INFO_GAIN)


def plan_trace_gain_sensors_horizon(env, horizon):             # ... of tr P- - tr P+
    return _plan_horizon(env, horizon, _lib.LOOK_TRACE_GAIN)


# ---- search on top of the dry run: env.evaluate_schedules() values whole schedules -- revisits included, which
# no forecast can value -- so a planner can compare candidates from one state.  The smallest such planner: local search around a plan.
REFINE_KINDS = {'info': _lib.LOOK_INFO_GAIN, 'trace': _lib.LOOK_TRACE_GAIN, 'pos_trace': _lib.LOOK_POS_TRACE_GAIN}


def refine_plan_sensors(env, plan, kind='info', rounds=4, candidates=64, seed=0):
    """a schedule [K', S] for env.rollout_sensors(), no worse than `plan` under the dry run: `rounds` rounds of `candidates` schedules,
    each scored by ONE env.evaluate_schedules() launch.  Candidate 0 is the incumbent; every other one is the incumbent with one slot
    (k, s) redrawn from the objects the forecast shows visible to s at step k with status OK and not already in row k -- an object
    planned at another step is allowed: the revisit the forecast planners cannot express.  The incumbent becomes the first candidate
    with the largest total in column `kind` ('info', 'trace', 'pos_trace').  ONE forecast launch for the masks.  The draws come from
    RandomState(seed): env.np_random and the action space's generator are not touched.  Returns (plan, total [3] float64 of it).
    A vector env (SSA_Tasker_VecEnv; section 8q): `plan` [E, K, S]; env e searches with RandomState(seed + e) exactly as a single env
    in its state would with that seed -- it is the same loop, a single env being the batch of one --, drawn from in the single env's
    order; ONE forecast and ONE evaluate_schedules() launch per round ([E, candidates, K', S]) serve all envs, with one horizon for
    all, K' = min(K, min_e(steps - 1 - i_e)); returns (plan [E, K', S] as vec.rollout_sensors() takes it, total [E, 3]).
    Of an env this reads forecast_sensors(), evaluate_schedules(), i, n, m, n_sensor and num_envs, and for the device-state guard
    _engine / _eng: nothing else."""
    if kind not in REFINE_KINDS:
        raise ValueError("refine_plan_sensors: kind must be one of %s, got %r" % (sorted(REFINE_KINDS), kind))
    if int(rounds) < 0 or int(candidates) < 1:
        raise ValueError("refine_plan_sensors: rounds >= 0 and candidates >= 1, got %r and %r" % (rounds, candidates))
    _need_device_state(env, "a plan is refined by dry runs, which run on the GPU only")
    col, rounds, candidates = REFINE_KINDS[kind], int(rounds), int(candidates)
    E, S = _num_envs(env), int(env.n_sensor)
    lead = () if E is None else (int(E),)
    plan = np.array(plan, dtype=np.int64)
    if plan.ndim != len(lead) + 2 or plan.shape[:-2] != lead or plan.shape[-1] != S:
        raise ValueError("refine_plan_sensors: a plan [%sK, %d], got shape %s" % ("".join("%d, " % v for v in lead), S, plan.shape))
    plan = _lift(env, plan)                                                                       # [E, K, S]
    E = plan.shape[0]
    K = min(plan.shape[1], _steps_left(env))
    if K < 1:
        raise ValueError("refine_plan_sensors: at least one step inside %s episode" % ("every env's" if lead else "the"))
    plan = plan[:, :K]
    rngs = [np.random.RandomState(seed + e if e else seed) for e in range(E)]
    ok = None
    if candidates > 1 and rounds > 0:
        f = env.forecast_sensors(K)
        ok = _lift(env, (f["visible"].cpu().numpy() != 0) & (f["status"].cpu().numpy() == _lib.ST_OK))      # [E, K', S, m]
    total = None
    for _ in range(rounds if candidates > 1 else 0):
        cand = np.repeat(plan[:, None], candidates, axis=1)
        for e in range(E):
            for c in range(1, candidates):
                k, s = divmod(int(rngs[e].randint(K * S)), S)
                free = ok[e, k, s].copy()
                row = plan[e, k]
                free[row[(row >= 0) & (row < free.shape[0])]] = False
                pool = np.flatnonzero(free)
                if len(pool):
                    cand[e, c, k, s] = pool[rngs[e].randint(len(pool))]
        totals = _lift(env, env.evaluate_schedules(_strip(env, cand))["total"].cpu().numpy())    # [E, candidates, 3]
        # (per env the first of equal maxima: the incumbent stays unless something is strictly better.  A NaN total -- a taken update
        # of a covariance that has no log-determinant left, late in an episode -- never wins)
        best = np.argmax(np.where(np.isnan(totals[:, :, col]), -np.inf, totals[:, :, col]), axis=1)
        plan, total = cand[np.arange(E), best], totals[np.arange(E), best]
    if total is None:
        total = _lift(env, env.evaluate_schedules(_strip(env, plan))["total"].cpu().numpy())[:, 0]
    return _strip(env, plan), np.asarray(_strip(env, total), dtype=np.float64)
