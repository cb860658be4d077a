"""What SSA_Tasker_Env and SSA_Tasker_VecEnv share around a sensor network's tasking queries: the agent table,
the one-site network of an env without config['observers'], the shaping of the engine's results into what the envs hand out -- the
vector env's with a leading [n_env] axis -- and a vector env's time words.  The launches themselves stay with the env classes."""
import numpy as np

from .. import _lib

# every agent of a sensor network that decides on the device (SSA_Tasker_Env.run_agent_sensors, SSA_Tasker_VecEnv.step_agent):
# name -> (score column, assignment rule of device.ASSIGN_RULES); the greedy ones also name -> score column
SENSOR_AGENT_RULES = {'agent_info_gain_sensors': (_lib.LOOK_INFO_GAIN, 'greedy'), 'agent_trace_gain_sensors': (_lib.LOOK_TRACE_GAIN, 'greedy'),
                      'agent_info_gain_sensors_optimal': (_lib.LOOK_INFO_GAIN, 'optimal'),
                      'agent_trace_gain_sensors_optimal': (_lib.LOOK_TRACE_GAIN, 'optimal')}
SENSOR_AGENT_COLUMNS = {name: column for name, (column, rule) in SENSOR_AGENT_RULES.items() if rule == 'greedy'}


def sensor_agent_rule(agent, what='step_agent'):
    """(score column, assignment rule) of a lookahead agent of a sensor network, given as the function of agents.py or its name;
    anything else has no device form (NotImplementedError naming the caller `what`).  Needs no device state."""
    name = agent if isinstance(agent, str) else getattr(agent, '__name__', None)
    if name not in SENSOR_AGENT_RULES:
        raise NotImplementedError("%s: %r is not implemented; the agents of a sensor network that decide on the device are %s, "
                                  "and with the optimal assignment %s"
                                  % (what, agent, " and ".join(sorted(SENSOR_AGENT_COLUMNS)),
                                     " and ".join(sorted(set(SENSOR_AGENT_RULES) - set(SENSOR_AGENT_COLUMNS)))))
    return SENSOR_AGENT_RULES[name]


def sensor_agent_column(agent):
    """the score column of sensor_agent_rule(agent)"""
    return sensor_agent_rule(agent)[0]


def network_sites(env, lla, limit, R):
    """the sites of the env(s) as a network: their own; without config['observers'] the one observer as a one-site block, built once"""
    if env._look_sites is None:
        from .. import host
        env._look_sites = env._sensors if env.n_sensor > 1 else host.make_sensor_params([lla], [limit], [R], 0)
    return env._look_sites


def lookahead_result(r, want, envs=None):
    """the engine's lookahead dict `r` as lookahead() and lookahead_sensors() hand it out: the score rows [..., m, 3] as [..., 3, m] (a
    view, no copy), visible, status and the covariance parts `want` as they are.  envs: E for a vector env's plain lookahead, whose
    rows [E * m, ...] get their env axis."""
    def lead(v):
        return v if envs is None else v.view((envs, -1) + tuple(v.shape[1:]))
    res = {"score": lead(r["score"]).transpose(-1, -2), "visible": lead(r["visible"]), "status": lead(r["status"])}
    for k in want:
        res[k] = lead(r[k])
    return res


def check_schedules(actions, n_sensor, envs=None):
    """the candidates of evaluate_schedules() as a numpy array with its candidate axis: integers [K, S] (one candidate) or [B, K, S],
    numpy or torch; with envs = E, a vector env's [E, K, S] or [E, B, K, S].  Anything else is a ValueError naming the shape.  Needs no
    device state."""
    import torch
    a = actions.detach().cpu().numpy() if isinstance(actions, torch.Tensor) else np.asarray(actions)
    lead = () if envs is None else (int(envs),)
    if a.ndim == len(lead) + 2:
        a = np.expand_dims(a, len(lead))
    if a.ndim != len(lead) + 3 or a.shape[:len(lead)] != lead or a.shape[-3] < 1 or a.shape[-1] != n_sensor or a.dtype.kind not in "iu":
        pre = "".join("%d, " % v for v in lead)
        raise ValueError("evaluate_schedules: integer schedules [%sK, %d] or [%sB, K, %d], got %s %s" % (pre, n_sensor, pre, n_sensor, a.dtype, a.shape))
    return a


def schedules_result(rec, stream):
    """a dry run's record tensor [B, K', S, DRY_STRIDE] ([E, B, K', S, DRY_STRIDE] of a vector env) as the dict evaluate_schedules()
    returns, its torch work and the totals' launch (ssa_dryrun_totals_f64) enqueued in `stream`"""
    import torch
    from .. import device
    K, S = int(rec.shape[-3]), int(rec.shape[-2])
    with torch.cuda.stream(stream):
        # (the engine's own [K', candidates, S, 8] block, a view again; slot order: one defined fp64 sum per candidate)
        total = device.dryrun_totals(rec.movedim(-3, 0).reshape(K, -1, S, _lib.DRY_STRIDE)).view(tuple(rec.shape[:-3]) + (_lib.LOOK_NSCORE,))
        return {"score": rec[..., _lib.DRY_SCORE:_lib.DRY_SCORE + _lib.LOOK_NSCORE], "taken": rec[..., _lib.DRY_TAKEN] != 0,
                "visible": rec[..., _lib.DRY_VISIBLE] != 0, "status": rec[..., _lib.DRY_STATUS].to(torch.int32),
                "action": rec[..., _lib.DRY_ACTION].to(torch.int64), "total": total}


def env_time_words(vec, what):
    """the keyword arguments that give a query launch of a vector env (lookahead, lookahead_sensors, forecast_sensors) the step each
    env takes next: up to INLINE_ENVS envs the time words travel by value, in the vector env's own stream; beyond, through the
    engine's env_time0 words as a step reads them (a synchronous copy: the pinned staging is the step's), in torch's current stream.
    ValueError naming `what` if an env has no next step."""
    import torch
    if np.any(vec.i + 1 >= vec.n):
        raise ValueError("%s: an env has no next step" % what)
    times = [int(v) + 1 for v in vec.i]
    if vec._inline:
        return dict(stream=vec._stream.cuda_stream, env_times=times)
    vec._eng.env_time0.copy_(torch.as_tensor(times, dtype=torch.int32))
    return {}
