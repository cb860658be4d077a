"""SSA_Tasker_VecEnv: E independent copies of SSA_Tasker_Env advanced by ONE kernel launch per step
(BASELINE config 5: "20 000 objects x 64 parallel env instances (RLlib vectorised rollout)").

The reference reaches env-level parallelism with one Python process per env (RLlib `num_workers`,
RLLib_training.py:40-56).  Here the E environments are one batch of E*m objects in HBM; the step
kernel takes per-env actions and per-env time indices, so envs that terminated are reset in place
while the others continue (the usual vector-env auto-reset).  Semantics per env are those of
SSA_Tasker_Env (same reward / done logic, same RNG draw order for reset, seed = base seed + env index);
measurement noise is drawn on the device per (env, time step) -- only the object the action selects
consumes noise in a step (ssa_tasker_simple_2.py:301).

A sensor network (config['observers'] with S > 1 sites, EXTENSION): every env tasks the same S sites, each sensor to its own object;
`step(actions)` takes [E, S] and is still ONE launch (ssa_env_step_sensors_envs_f64).  Noise is then drawn per
(env, sensor, time step).

Around the step: `lookahead_sensors()` is every sensor's lookahead in every env from ONE launch
(ssa_lookahead_sensors_envs_f64) -- the action mask and the gains an RL user trains against; `step_agent(agent)` is a vector step whose
actions a lookahead agent decides ON THE DEVICE: lookahead, every env's greedy assignment (ssa_assign_sensors_envs_f64) into the
engine's action table, and the step reading that table -- three launches in one stream, one synchronisation, the actions never on the
host in between.  agents.agent_info_gain_sensors / agent_trace_gain_sensors take a vector env and return [E, S].

Ahead of the step: `forecast_sensors(horizon)` is every sensor's lookahead at each of the next H' steps of every
env from ONE launch (ssa_forecast_sensors_envs_f64) -- the action masks, the covariance growth and the gains of the steps to come, read
only; agents.plan_info_gain_sensors / plan_trace_gain_sensors take a vector env and return the greedy plan [E, H', S].

A schedule: `rollout_sensors(actions [E, K, S])` runs such a plan -- or any fixed tasking schedule -- as the K
step() calls would, in one launch per chunk with the envs' state resident on chip (ssa_env_rollout_sensors_envs_f64); `rollout([E, K])`
is the same without a network.
"""
import numpy as np

from .. import _lib
from ._config import draw_initial_state, orbit_site_table, resolve_config, reward_done
from ._gymshim import np_random, spaces
# (the agent table is one object: SENSOR_AGENTS is SSA_Tasker_Env.SENSOR_AGENT_COLUMNS, SENSOR_AGENT_RULES the env's of that name)
from ._tasking import SENSOR_AGENT_COLUMNS as SENSOR_AGENTS, SENSOR_AGENT_RULES, sensor_agent_column, sensor_agent_rule  # noqa: F401
from ._tasking import check_schedules, env_time_words, lookahead_result, network_sites, schedules_result


def check_sensor_actions(actions, E, S, m):
    """the [E, S] action table of a vector step of a sensor network, checked as SSA_Tasker_Env.step checks one env's row -- every entry
    an object in 0 .. m-1 (AssertionError), no two sensors of ONE env on one object (ValueError; the same index in two envs is two
    objects) -- and returned as int64.  Needs no device state."""
    a = np.asarray(actions)
    if a.shape != (E, S) or a.dtype.kind not in "iu" or not (np.all(a >= 0) and np.all(a < m)):
        raise AssertionError("%r (%s) invalid: one object in 0 .. %d per sensor (%d envs x %d sensors)" % (actions, type(actions), m - 1, E, S))
    a = a.astype(np.int64)
    for e in range(E):
        if len(np.unique(a[e])) != S:
            raise ValueError("step: two sensors tasked to the same object (%s) in env %d" % (a[e], e))
    return a


def check_fallback_actions(fallback, E, S):
    """the [E, S] fallback rows of step_agent as int32 [E, MAX_SENSORS] words (-1 beyond S): any integer is taken as given -- an entry
    outside 0 .. m-1 leaves its sensor idle when it gets no object -- any other shape or dtype is a ValueError naming the shape.  Needs
    no device state."""
    a = np.asarray(fallback)
    if a.shape != (E, S) or a.dtype.kind not in "iu":
        raise ValueError("step_agent: fallback_actions must be an integer array of shape (%d, %d) (envs x sensors), got shape %s (%s)"
                         % (E, S, a.shape, a.dtype))
    rows = np.full((E, _lib.MAX_SENSORS), -1, dtype=np.int32)
    rows[:, :S] = np.clip(a.astype(np.int64), -1, 2 ** 31 - 1)
    return rows


def shaped_hit(actions, argmax_prev):
    """per env: did its action -- with a sensor network ANY of its sensors' ([E, S]) -- task np.argmax(sigma_pos[i - 1])?  (the 'shaped'
    reward's +1/n, as SSA_Tasker_Env._reward_done)"""
    a = np.asarray(actions)
    prev = np.asarray(argmax_prev)
    return (a == prev) if a.ndim == 1 else np.any(a == prev[:, None], axis=1)


def book_rollout(reward_type, stats, actions, rewards_sum, argmax_prev, i, m, n):
    """The bookkeeping of a chunk of a vector rollout, as C consecutive step() calls would do it: stats [C, E, STAT_STRIDE] (every
    step's statistics), actions [C, E, S] (the rows the chunk ran), rewards_sum / argmax_prev / i [E] (what the episodes have paid,
    np.argmax(sigma_pos) of the step before, the envs' step indices -- all in front of the chunk), m objects, n steps per episode.
    Step k has the index i + k + 1 and is an episode's last when i + k + 2 >= n; the 'shaped' hit of step k is against the arg-max of
    step k - 1 (stats[k - 1], argmax_prev for k = 0) and its win pays 1 - (the rewards summed up to k - 1).  The chunk is kept up to
    and including the first step at which ANY env is done.  Returns (rewards [E, keep], dones [E, keep], rewards_sum, argmax_prev,
    keep), the sums and arg-maxes behind step keep - 1; the inputs are not written.  Needs no device."""
    st = np.asarray(stats)
    paid = np.array(rewards_sum, dtype=np.float64)
    prev = np.array(argmax_prev, dtype=np.int64)
    i = np.asarray(i, dtype=np.int64)
    shaped = reward_type == 'shaped'
    rewards, dones = [], []
    for k in range(st.shape[0]):
        hit = shaped_hit(actions[k], prev) if shaped else False
        r, d = reward_done(reward_type, st[k], hit, paid, i + k + 2 >= n, m, n)
        paid = paid + r
        if shaped:
            prev = st[k][:, _lib.STAT_ARGMAX_SPOS].astype(np.int64)
        rewards.append(np.asarray(r, dtype=np.float64))
        dones.append(np.asarray(d, dtype=bool))
        if dones[-1].any():
            break
    return np.stack(rewards, axis=1), np.stack(dones, axis=1), paid, prev, len(rewards)


def check_schedule(actions, E, S, m, name="rollout_sensors"):
    """the [E, K, S] schedule of a vector rollout as int64: any other shape or dtype is a ValueError naming the shape, and every
    actions[:, k] is checked as step() checks its table (check_sensor_actions), the error naming step k.  Needs no device state."""
    a = np.asarray(actions)
    if a.ndim != 3 or a.shape[0] != E or a.shape[2] != S or a.shape[1] < 1 or a.dtype.kind not in "iu":
        raise ValueError("%s: actions must be an integer array of shape (%d, K, %d) (envs x steps x sensors), K >= 1, got shape %s (%s)"
                         % (name, E, S, a.shape, a.dtype))
    for k in range(a.shape[1]):
        try:
            check_sensor_actions(a[:, k], E, S, m)
        except (AssertionError, ValueError) as err:
            raise type(err)("%s: step %d: %s" % (name, k, err)) from None
    return a.astype(np.int64)


class SSA_Tasker_VecEnv:
    ROLLOUT_CHUNK = 64      # rollout_sensors(): at most this many steps per launch

    def __init__(self, config, num_envs, seed=0):
        import torch
        from .. import engine
        from ._obspool import HostObs
        c = resolve_config(config)          # (as SSA_Tasker_Env: the same values, constants and options from the same config)
        self.E, self.m, self.n, self.dt = int(num_envs), c.m, c.n, c.dt
        # (a sensor network, S > 1 sites: sensor 0 is the primary sensor, the env's observer; one site takes the plain path, as SSA_Tasker_Env)
        self.n_sensor = S = c.n_sensor
        if S > 1 and self.E > 1 and self.m % 4:
            raise ValueError("a sensor network in several envs needs rso_count % 4 == 0 (whole tiles per env), got " + str(self.m))
        self._bulk_draws = bool(config.get('device_rng', False))
        self.obs_returned, self.reward_type = config['obs_returned'], config['reward_type']
        self.orbits = config['orbits']
        self.obs_type, self.x_sigma, self.z_sigma, self.P_0 = c.obs_type, c.x_sigma, c.z_sigma, c.P_0
        self._consts = c.consts
        self._gen = torch.Generator(device="cuda").manual_seed(int(seed))
        self._zs = torch.as_tensor(self.z_sigma, dtype=torch.float64, device="cuda")
        if S > 1:      # (noise per (env, sensor, time step): [E, S, n, 1, 3], sensor s scaled by its own z_sigma)
            from .. import host
            self._zs = torch.as_tensor(c.net.z_sigma, dtype=torch.float64, device="cuda").view(S, 1, 1, 3)
            self._sensors = host.make_sensor_params(c.net.lla, c.net.obs_limit, c.net.R, self.n * 3, angles_only=c.net.angles_only,
                                                    sunlit_only=c.net.sunlit_only, shadow_radius=c.shadow_radius)
        # (config['sensor_measurement']: True where a sensor measures az and el only; without a network: the one az-el-range observer)
        self.sensor_angles_only = np.zeros(S, dtype=bool) if c.net is None else c.net.angles_only
        # (config['sensor_illumination']: True where a sensor sees only sunlit objects, and only from a dark site; sun_table: the Sun's
        # direction per row of the trans table -- one epoch, one table for all envs --, None unless a sensor asks for it)
        self.sensor_sunlit_only = np.zeros(S, dtype=bool) if c.net is None else c.net.sunlit_only
        self.sun_table, self.sun_dark, self.shadow_radius = c.sun, c.sun_dark, c.shadow_radius
        # (config['observers'] entries {'orbit': ...}: True where a sensor is space-based; site_table: its site rows per row of the trans
        # table -- the orbit propagated on the device, one table for all envs --, None without one)
        self.sensor_moving = np.zeros(S, dtype=bool) if c.net is None else c.net.moving
        self.limb_radius = c.limb_radius
        self.site_table = orbit_site_table(c, config)
        self._site = (c.obs_lla, c.obs_limit, c.R)      # (the env's own observer: a one-site network for lookahead_sensors)
        self._look_sites = None
        self._rows_host = None                          # step_agent: pinned [E, MAX_SENSORS] read-back of the action table
        self._z_shape = (S, self.n, 1, 3) if S > 1 else (self.n, 1, 3)
        z = torch.randn((self.E,) + self._z_shape, dtype=torch.float64, device="cuda", generator=self._gen) * self._zs
        self._eng = engine.HotPathEngine(self._consts, self.m, self.E, c.trans, z, history=2,
                                         zn_stride_env=S * self.n * 3, zn_stride_time=3, zn_stride_obj=0)
        if self.sun_table is not None:
            self._eng.set_sun_table(self.sun_table, self.sun_dark, [self._sensors])
        if self.site_table is not None:
            self._eng.set_site_table(self.site_table, self.sensor_moving, self.limb_radius)
        self._rng = [np_random(seed + e)[0] for e in range(self.E)]
        self.single_action_space = spaces.MultiDiscrete([self.m] * S) if S > 1 else spaces.Discrete(self.m)
        self.single_observation_space = c.obs_space
        self.num_envs = self.E
        self._aer = torch.zeros((self.E * self.m, 4), dtype=torch.float64, device="cuda")
        # host side of a step: time indices and actions leave from pinned staging (asynchronous copies), the statistics and the
        # observation vectors arrive in host-mapped pinned memory written by the kernels themselves (the 'aer' block by the step
        # kernel's epilogue, the observation rows as its second destination): one stream synchronisation per vector step, no
        # device-to-host copy pass.
        self._ta_host = torch.zeros(2 * self.E, dtype=torch.int32).pin_memory()      # [time indices | actions]: one copy per step
        self._time_np, self._act_np = self._ta_host.numpy()[:self.E], self._ta_host.numpy()[self.E:]
        # up to 8 envs: time indices and actions travel BY VALUE in the launch's parameter block (no copy in front of the step, and
        # with no torch call left in step() the stream handle is looked up once); the statistics of every env are folded by the last
        # wavefront that adds to them (SSA_LAUNCH_FOLD_INSIDE): ONE launch per vector step
        self._inline = self.E <= _lib.INLINE_ENVS
        self._stream = torch.cuda.current_stream()
        # config['obs_device'] = True: step() returns the observations as ONE CUDA tensor [E, ...] -- a view of device memory the step
        # kernel wrote.  Otherwise a FRESH array (gym's vector envs copy their observation buffer by default, and so does the reference's
        # single env for 'flatten'), or with config['obs_zero_copy'] a view of the two-deep host-mapped ring the kernel writes, valid until
        # step k + 2 (envs/_obspool.py)
        self._obs_device = c.obs_device
        self._stats_host = torch.zeros((self.E, _lib.STAT_STRIDE), dtype=torch.float64).pin_memory()
        self._stats_np = self._stats_host.numpy()
        per = self.m * (4 if self.obs_returned == 'aer' else 12)
        # config['obs_dtype'] = 'float32': the host-facing observations in single precision, written that way by the step kernel
        # (SSA_LAUNCH_MIRROR_F32) -- half of the 5 MB a vector step sends over PCIe
        self._mirror_f32 = c.obs_f32 and not self._obs_device
        if self._mirror_f32 and self.reward_type == 'shaped' and not self._eng.supports_argmax:
            raise ValueError("obs_dtype float32 with the 'shaped' reward needs rso_count % 4 == 0 (the one-launch statistics path)")
        self._obs_host = HostObs(self.E * per, (self.E,) + c.obs_space.shape, self._mirror_f32, 2,
                                 None if (c.obs_zero_copy or self._obs_device) else config.get('obs_pool', 16))
        self._obs_pool = self._obs_host.pool
        # config['storage_layout'] = 'regime' (opt-in): every env's objects stored sorted by orbit regime (catalogue.regime_order_env;
        # HotPathEngine.set_layout with one permutation per env) -- actions, rewards and observations stay in the env's own numbering.  It pays
        # where the observations stay on the GPU (obs_device): host-facing rows would leave the kernel one by one instead of tile by tile
        self._layout = c.storage_layout
        if self._layout and self.m % 4:
            raise ValueError("storage_layout with several envs needs rso_count % 4 == 0")
        self._obs_dev_rows = None       # (layout + obs_device, 'flatten' / rows: the step kernel's second copy of the observation, at the caller's rows)
        self.i = np.zeros(self.E, dtype=np.int64)       # per-env step index
        self.tick = 0
        self.rewards_sum = np.zeros(self.E)
        self._argmax_prev = np.zeros(self.E, dtype=np.int64)
        self.reset()

    # ------------------------------------------------------------------
    def _draw(self, e):
        return draw_initial_state(self._rng[e], self.orbits, self.m, self.x_sigma, self._bulk_draws)

    def _reset_env(self, e, slot, draw=None):
        import torch
        xt, xf = self._draw(e) if draw is None else draw
        if self._layout and draw is None:        # (reset() of all envs has set the whole table already)
            from ..catalogue import regime_order_env
            self._eng.set_env_layout(e, regime_order_env(xt, e, self.E))
        self._eng.load_env_state(slot, e, xt, xf, self.P_0)
        self._eng.z_noise[e].copy_(torch.randn(self._z_shape, dtype=torch.float64, device="cuda", generator=self._gen) * self._zs)
        self.i[e] = 0
        self.rewards_sum[e] = 0.0
        if self._access_T is not None:      # (a new truth: action_masks() makes this env's slab of the pass table again)
            self._access_stale = set(self._access_stale) | {e}

    def reset(self):
        slot = self.tick % 2
        draws = [self._draw(e) for e in range(self.E)]
        if self._layout:
            from ..catalogue import regime_order_env
            self._eng.set_layout(np.stack([regime_order_env(draws[e][0], e, self.E) for e in range(self.E)]))
        for e in range(self.E):
            self._reset_env(e, slot, draw=draws[e])
        self._refresh_stats(slot)
        return self._obs(slot, reset=True)

    def _refresh_stats(self, slot):
        st = self._eng.stats[slot].cpu().numpy()
        self._argmax_prev = st[:, _lib.STAT_ARGMAX_SPOS].astype(np.int64)
        return st

    def _obs(self, slot, reset=False):
        e = self._eng
        if self._obs_device:
            if self.obs_returned == 'aer':
                if reset:
                    self._aer_reset_rows()
                return self._aer.view(self.E, self.m * 4)
            rows = e.obs[slot]
            if self._layout:       # the kernel's second copy, at the caller's rows (a reset: gathered from the state just loaded); one per
                if self._obs_dev_rows is None:      # history slot, so that what step k returned stays intact until step k + 2
                    import torch
                    self._obs_dev_rows = [torch.zeros_like(e.obs[0]) for _ in range(2)]
                if reset:
                    self._obs_dev_rows[slot].copy_(e.caller_rows(e.obs[slot]))
                rows = self._obs_dev_rows[slot]
            return rows.view(self.E, self.m * 12) if self.obs_returned == 'flatten' else rows.view(self.E, self.m, 12)
        cast = self._obs_host.cast
        if self.obs_returned == 'flatten':
            return cast(e.caller_rows(e.obs[slot]).cpu().numpy().reshape(self.E, self.m * 12))
        if self.obs_returned == 'aer':
            if reset:
                self._aer_reset_rows()
            return cast(self._aer.cpu().numpy().reshape(self.E, self.m * 4))
        return cast(e.caller_rows(e.obs[slot]).cpu().numpy().reshape(self.E, self.m, 12))

    def _aer_reset_rows(self):
        """the 'aer' block of the CURRENT state of every env (reset time only: a step's block is the step kernel's epilogue)"""
        from .. import device
        e, slot = self._eng, self.tick % 2
        for k in range(self.E):
            sl = slice(k * self.m, (k + 1) * self.m)
            M = e.trans[int(self.i[k]) % e.n_time].reshape(3, 3)
            device.aer_obs(e.x_filter[slot, sl], e.P_filter[slot, sl], M, self._consts, out=self._aer[sl])
            if self._layout:
                self._aer[sl].copy_(e.env_caller_rows(k, self._aer[sl]))

    def step(self, actions):
        S = self.n_sensor
        if S > 1:
            actions = check_sensor_actions(actions, self.E, S, self.m)
        else:
            actions = np.asarray(actions, dtype=np.int64).reshape(self.E)
            assert 0 <= int(actions.min()) and int(actions.max()) < self.m, "invalid action"
        return self._step(actions)

    def step_agent(self, agent, fallback_actions=None):
        """One vector step of a sensor network whose actions a lookahead agent decides ON THE DEVICE: every
        sensor's lookahead in every env, every env's greedy assignment into the engine's action table, and the step reading that
        table -- three launches in one stream, one synchronisation; the actions reach the host only afterwards, for the 'shaped' hit and
        for the caller.  `agent`: agents.agent_info_gain_sensors or agents.agent_trace_gain_sensors, or its name; their
        *_optimal forms decide by the exact one-step optimum instead of the greedy rounds (ssa_match_sensors_envs_f64).  fallback_actions:
        what a sensor the scores leave without an object gets -- None: one single_action_space.sample() row per env; an [E, S] integer
        array: taken as given, sensors ascending, unless out of 0 .. m-1 or held by another sensor of the env (the sensor then stays
        idle).  Returns step()'s 4-tuple -- rewards, dones, auto-reset and observations are step()'s -- with infos[e]['action'] the int64
        [S] row env e executed (-1: the sensor stayed idle)."""
        column, rule = sensor_agent_rule(agent)
        if self.n_sensor < 2:
            raise NotImplementedError("step_agent: not implemented without a sensor network (config['observers'])")
        if fallback_actions is None:
            fallback_actions = np.stack([np.atleast_1d(self.single_action_space.sample()) for _ in range(self.E)])
        return self._step(None, decide=(column, check_fallback_actions(fallback_actions, self.E, self.n_sensor), rule))

    def _step(self, actions, decide=None):
        """the vector step: `actions` as step() checked them, or -- decide = (score column, fallback words [E, MAX_SENSORS], rule) -- decided
        on the device in front of the step's launch (step_agent) and read back behind the one synchronisation"""
        import torch
        S = self.n_sensor
        e = self._eng
        argmax_prev = self._argmax_prev
        self.i += 1
        self.tick += 1
        sin, sout = (self.tick - 1) % 2, self.tick % 2
        aer = self.obs_returned == 'aer'
        shaped = self.reward_type == 'shaped'
        # 'shaped' needs np.argmax(sigma_pos[i - 1]) per env: from the arg-max slots of the one-launch path when every env is whole
        # tiles (rso_count % 4 == 0), through the three-launch exact statistics otherwise
        fast = (not shaped) or e.supports_argmax
        if self._obs_device:
            aer_out, mirror = (self._aer.data_ptr() if aer else 0), (self._obs_dev_rows[sout].data_ptr() if (self._layout and not aer) else 0)
        else:
            dst = self._obs_host.dest(self.tick)
            aer_out, mirror = (dst, 0) if aer else (0, dst)
        if S > 1:      # (a sensor network: the same single launch, a row of S actions per env; the update records stay on the device side)
            kw = dict(aer_out=aer_out, obs_mirror=mirror, stats_out=self._stats_host.data_ptr(), fast_stats=fast, fold_inside=True,
                      argmax_spos=shaped and fast, mirror_f32=self._mirror_f32 and fast)
            if decide is not None:     # (lookahead -> assignment -> step, all reading the time words and the rows from device memory)
                self._time_np[:] = self.i
                e.time_actions.copy_(self._ta_host, non_blocking=True)
                fb = torch.from_numpy(decide[1]).to("cuda")
                cur = torch.cuda.current_stream()
                look = e.launch_lookahead_sensors_envs(sin, 0, self._sensors, stream=cur.cuda_stream)
                table = e.launch_assign_sensors_envs(look, decide[0], fallback=fb, stream=cur.cuda_stream, rule=decide[2])
                e.launch_step_sensors_envs(sin, sout, 0, self._sensors, None, stream=cur.cuda_stream, **kw)
                if self._rows_host is None:
                    self._rows_host = torch.zeros((self.E, _lib.MAX_SENSORS), dtype=torch.int32).pin_memory()
                self._rows_host.copy_(table, non_blocking=True)
            elif self._inline:
                cur = self._stream
                e.launch_step_sensors_envs(sin, sout, 0, self._sensors, actions, stream=cur.cuda_stream, env_words=self.i.tolist(), **kw)
            else:
                self._time_np[:] = self.i
                e.time_actions.copy_(self._ta_host, non_blocking=True)
                cur = torch.cuda.current_stream()
                e.launch_step_sensors_envs(sin, sout, 0, self._sensors, actions, stream=cur.cuda_stream, **kw)
        elif self._inline:
            cur = self._stream
            e.launch_step(sin, sout, 0, aer_out=aer_out, obs_mirror=mirror, stats_out=self._stats_host.data_ptr(), stream=cur.cuda_stream,
                          fast_stats=fast, fold_inside=True, env_words=(self.i.tolist(), actions.tolist()), argmax_spos=shaped and fast,
                          mirror_f32=self._mirror_f32 and fast)
        else:
            self._time_np[:] = self.i
            self._act_np[:] = actions
            e.time_actions.copy_(self._ta_host, non_blocking=True)
            cur = torch.cuda.current_stream()     # (the stream the time / action copy above was enqueued in)
            e.launch_step(sin, sout, 0, aer_out=aer_out, obs_mirror=mirror, stats_out=self._stats_host.data_ptr(), stream=cur.cuda_stream,
                          fast_stats=fast, fold_inside=True, argmax_spos=shaped and fast, mirror_f32=self._mirror_f32 and fast)
        cur.synchronize()
        if decide is not None:
            actions = self._rows_host.numpy()[:, :S].astype(np.int64)
        st = self._stats_np            # (host-mapped: the step kernel's folds wrote it; stable until the next launch)
        if shaped:
            self._argmax_prev = st[:, _lib.STAT_ARGMAX_SPOS].astype(np.int64)
        hit = shaped_hit(actions, argmax_prev) if shaped else False
        rewards, dones = reward_done(self.reward_type, st, hit, self.rewards_sum, self.i + 1 >= self.n, self.m, self.n)
        self.rewards_sum += rewards
        obs = self._obs(sout) if self._obs_device else self._obs_host.hand_out()
        infos = [{'action': actions[k]} for k in range(self.E)] if decide is not None else [{} for _ in range(self.E)]
        if dones.any():   # auto-reset in place; the returned observation of a finished env is its new first one
            for d in np.where(dones)[0]:
                infos[d]['terminal_observation'] = obs[d].clone() if self._obs_device else obs[d].copy()
                self._reset_env(int(d), sout)
            st_dev = self._eng.stats[sout].cpu().numpy()          # (the reset wrote the new envs' statistics on the device)
            self._argmax_prev[dones] = st_dev[dones, _lib.STAT_ARGMAX_SPOS].astype(np.int64)
            obs = self._obs(sout, reset=(self.obs_returned == 'aer') or bool(self._layout))
        # (ssa_tasker_simple_2.py:365-367 passes the reward of the other modes through nan_to_num(nan=.5, inf=.5): the rewards formed above are
        # finite by construction -- counts of comparisons, constants -- so there is nothing for it to replace)
        return obs, rewards, dones, infos

    def rollout(self, actions):
        """rollout_sensors() for a vector env without config['observers']: `actions` integer [E, K], one object per env and step."""
        if self.n_sensor > 1:
            raise NotImplementedError("rollout: not implemented for a sensor network in a vector env (config['observers'] with %d "
                                      "sensors); use rollout_sensors" % self.n_sensor)
        a = np.asarray(actions)
        if a.ndim != 2:
            raise ValueError("rollout: actions must be an integer array of shape (%d, K) (envs x steps), got shape %s" % (self.E, a.shape))
        return self.rollout_sensors(a[..., None])

    def rollout_sensors(self, actions):
        """A K-step tasking schedule of every env in one launch per chunk (ssa_env_rollout_sensors_envs_f64):
        `actions` integer [E, K, S] -- a plan of agents.plan_info_gain_sensors as it comes; S = 1 without config['observers'], the
        envs' own observer as a one-site network -- applied as the consecutive step(actions[:, k]) calls would be, state, rewards and
        bookkeeping bit for bit.  Stops after the first step at which ANY env is done; the envs done there auto-reset as step() resets
        them, and the caller goes on with actions[:, K':] in a new call.  Returns (obs, rewards [E, K'], dones [E, K'], infos): obs and
        infos what the last executed step() would have returned.  ValueError: a schedule of the wrong shape or dtype, an env without
        a next step, several envs with rso_count % 4 != 0; a bad row raises what step() raises, naming its step.
        At most ROLLOUT_CHUNK steps per launch and never more than the fewest steps an env has left, so the time limit ends a chunk;
        one copy of the time words and one synchronisation per chunk.  'jones' and 'shaped' can end an episode inside a chunk: the chunk
        then starts from a snapshot, and is launched again up to that step (the launch is deterministic)."""
        import torch
        S, E = self.n_sensor, self.E
        a = check_schedule(actions, E, S, self.m)
        if np.any(self.i + 1 >= self.n):
            raise ValueError("rollout_sensors: an env has no next step")
        if E > 1 and self.m % 4:
            raise ValueError("rollout_sensors: several envs need rso_count % 4 == 0 (whole tiles per env), got " + str(self.m))
        e = self._eng
        if e is None:
            raise _lib.SsaHipError("no device state: a rollout runs on the GPU only (no CPU fallback)")
        shaped = self.reward_type == 'shaped'
        if shaped and not e.supports_argmax:
            raise ValueError("rollout_sensors: the 'shaped' reward needs rso_count % 4 == 0 (every step's arg-max of sigma_pos)")
        undo = self.reward_type in ('jones', 'shaped')      # (a win or a loss may turn up inside a chunk)
        rows = np.ascontiguousarray(a.transpose(1, 0, 2))   # [K, E, S]
        sched = torch.from_numpy(rows.astype(np.int32)).to("cuda")
        sites = self._sites()
        K, k0 = rows.shape[0], 0
        rewards, dones = [], []
        while k0 < K:
            C = min(int(self.ROLLOUT_CHUNK), K - k0, int((self.n - 1 - self.i).min()))
            sin = self.tick % 2
            snap = e.snapshot_state(sin) if (undo and C > 1) else None
            e.env_time0.copy_(torch.as_tensor(self.i + 1, dtype=torch.int32))      # (a synchronous copy: the pinned staging is the step's)
            st = e.launch_rollout_sensors_envs(sin, 0, sites, sched[k0:k0 + C], argmax_spos=shaped)[0].cpu().numpy()
            r, d, paid, prev, keep = book_rollout(self.reward_type, st, rows[k0:k0 + C], self.rewards_sum, self._argmax_prev, self.i,
                                                  self.m, self.n)
            if keep < C:      # the device ran past a done: the same rows again from the snapshot, up to that step -- the same bits
                e.restore_state(sin, snap)
                e.launch_rollout_sensors_envs(sin, 0, sites, sched[k0:k0 + keep], argmax_spos=shaped)
                torch.cuda.current_stream().synchronize()
            self.i += keep
            self.tick += keep
            self.rewards_sum[:] = paid
            self._argmax_prev = prev
            rewards.append(r)
            dones.append(d)
            k0 += keep
            if d[:, -1].any():
                break
        rewards, dones = np.concatenate(rewards, axis=1), np.concatenate(dones, axis=1)
        slot, last = self.tick % 2, dones[:, -1]
        obs = self._obs(slot, reset=True)      # (the path a reset's observation takes: the step kernel's host-mapped destinations are not used)
        infos = [{} for _ in range(E)]
        if last.any():
            for d in np.where(last)[0]:
                infos[d]['terminal_observation'] = obs[d].clone() if self._obs_device else obs[d].copy()
                self._reset_env(int(d), slot)
            st_dev = e.stats[slot].cpu().numpy()
            self._argmax_prev[last] = st_dev[last, _lib.STAT_ARGMAX_SPOS].astype(np.int64)
            obs = self._obs(slot, reset=True)
        return obs, rewards, dones, infos

    def lookahead(self, covariances=False):
        """SSA_Tasker_Env.lookahead() of every env from ONE launch: the same dict with a leading [n_env] axis -- score [E, 3, m],
        visible / status [E, m], and with covariances=True x_prior [E, m, 6], P_prior / P_post [E, m, 6, 6]; objects in each env's own
        order.  Nothing of the envs changes; the next call overwrites the tensors."""
        from .. import engine as _engine
        if self.n_sensor > 1:
            raise NotImplementedError("lookahead: not implemented for a sensor network in a vector env (config['observers'] with %d "
                                      "sensors); use lookahead_sensors" % self.n_sensor)
        words = env_time_words(self, "lookahead")
        want = _engine.HotPathEngine.LOOKAHEAD_PARTS if covariances else ()
        return lookahead_result(self._eng.launch_lookahead(self.tick % 2, 0, out=want, **words), want, envs=self.E)

    def _sites(self):
        """the sites of the envs as a network: their own; without config['observers'] the envs' one observer as a one-site block"""
        return network_sites(self, *self._site)

    def _launch_lookahead_sensors(self, want=()):
        """the network's lookahead of every env enqueued for the step each env takes next (_tasking.env_time_words); the engine's
        result dict"""
        words = env_time_words(self, "lookahead_sensors")
        return self._eng.launch_lookahead_sensors_envs(self.tick % 2, 0, self._sites(), out=want, **words)

    def lookahead_sensors(self, covariances=False):
        """SSA_Tasker_Env.lookahead_sensors() of every env from ONE launch (ssa_lookahead_sensors_envs_f64): the
        same dict with a leading [n_env] axis, S = n_sensor (1 without config['observers']: the envs' own observer, and then equal to
        lookahead() bit for bit) -- score [E, S, 3, m], visible / status [E, S, m], and with covariances=True x_prior [E, m, 6],
        P_prior [E, m, 6, 6] and P_post [E, S, m, 6, 6]; objects in each env's own order.  visible is the action mask of the next step,
        the scores are the greedy baselines' gains.  Nothing of the envs changes; the next call overwrites the tensors."""
        from .. import engine as _engine
        want = _engine.HotPathEngine.LOOKAHEAD_PARTS if covariances else ()
        return lookahead_result(self._launch_lookahead_sensors(want), want)

    def _launch_forecast_sensors(self, horizon, want=()):
        """the network's H'-step forecast of every env enqueued from the step each env takes next, H' = min(horizon, the fewest steps
        an env has left) (_tasking.env_time_words); the engine's result dict, [H', E, ...]"""
        if int(horizon) < 1:
            raise ValueError("forecast_sensors: a horizon of at least one step, got %r" % (horizon,))
        words = env_time_words(self, "forecast_sensors")
        H = min(int(horizon), int(self.n - 1 - self.i.max()))
        return self._eng.launch_forecast_sensors_envs(self.tick % 2, 0, self._sites(), H, out=want, **words)

    # ---- what agents.py asks of an env beside its public queries (SSA_Tasker_Env answers the same four)
    def _tasking_stream(self):
        """the torch stream the planners' launches go in: the query launches' own (_tasking.env_time_words)"""
        import torch
        return self._stream if self._inline else torch.cuda.current_stream()

    def _forecast_scores(self, horizon):
        """the forecast's scores as the engine leaves them, [H', E, S, m, 3] (contiguous; slab h of all envs is score[h])"""
        return self._launch_forecast_sensors(horizon)["score"]

    def _slab_assigner(self, score):
        """assign(slab [E, S, m, 3], column, row [E, MAX_SENSORS], rule): every env's assignment of one slab into a row of the planner's
        own, one launch in torch's current stream (device.assign_sensors_envs) with ONE workspace of the planner's own for all calls"""
        from .. import device
        E, S, m = (int(v) for v in score.shape[1:4])
        ws = device.assign_sensors_envs_workspace(m, S, E, score.device)
        return lambda slab, column, row, rule: device.assign_sensors_envs(slab, column, out=row, workspace=ws, rule=rule)

    def _plan_table(self, horizon, column):
        """the forecast's launch and the horizon-wide plan's (ssa_plan_sensors_f64) on it: the engine's int32 table [H', E, MAX_SENSORS]"""
        return self._eng.launch_plan_sensors(self._launch_forecast_sensors(horizon), column, stream=self._tasking_stream().cuda_stream)

    def forecast_sensors(self, horizon, covariances=False):
        """SSA_Tasker_Env.forecast_sensors() of every env from ONE launch (ssa_forecast_sensors_envs_f64): from
        env e's state at its step i_e, what lookahead_sensors() would return at each of the steps i_e + 1 .. i_e + H' if every sensor
        stayed idle until then, with ONE horizon for all envs, H' = min(horizon, min_e(steps - 1 - i_e)).  ValueError if an env has no
        next step (the rule of lookahead_sensors()) or horizon < 1.  The single env's dict with a leading [n_env] axis, S = n_sensor (1
        without config['observers']: the envs' own observer as a one-site network), objects in each env's own order:
            score   [E, H', S, m, 3]  float64: columns _lib.LOOK_*; NaN unless status == OK and visible from s at that step
            visible [E, H', S, m]     uint8: the action mask of each of the next H' steps
            status  [E, H', S, m]     int32
        and with covariances=True also x_prior [E, H', m, 6], P_prior [E, H', m, 6, 6] and P_post [E, H', S, m, 6, 6] -- views of the
        engine's [H', E, ...] tensors with the first two axes swapped (not contiguous).  Nothing of the envs changes: no step is spent,
        no auto-reset, no bookkeeping; the next call overwrites the tensors.  Memory: the scores are 24 * H' * E * S * m bytes and
        P_post is twelve times that -- at 8 x 20 000 objects, H' = 8 and S = 8 that is 245 MB and 2.9 GB: covariances are for short
        horizons."""
        from .. import engine as _engine
        want = _engine.HotPathEngine.LOOKAHEAD_PARTS if covariances else ()
        r = self._launch_forecast_sensors(horizon, want)
        return {k: v.transpose(0, 1) for k, v in r.items()}

    # the pass table of all envs: its steps, per env the step index it was made at and the steps it counts there,
    # and the envs that have been reset since (their slabs are made again before a mask is formed); None: no table
    _access_T, _access_anchor, _access_left, _access_stale = None, None, None, ()

    def access_sensors(self, horizon=None, envs=None):
        """SSA_Tasker_Env.access_sensors() of every env from ONE launch (ssa_access_sensors_f64): one table
        [E, S, m, W] over T = min(horizon, steps - 1) steps (the whole episode by default), env e anchored at ITS step i_e and counting
        min(T, steps - 1 - i_e) steps from there; later bits are 0.  envs: only these envs are made again (one launch, the others'
        slabs and anchors stay); a table of another T is made for all.  The single env's dict with a leading [n_env] axis -- bits
        [E, S, m, W] int64, first / length / count / passes [E, S, m] int32, CUDA, objects in each env's own order -- and n_steps, the
        int64 [E] steps each env counts.  Nothing of the envs changes; the tensors are the engine's, and action_masks() reads them."""
        import torch
        if self._eng is None:
            raise _lib.SsaHipError("no device state: the pass table is made on the GPU only (no CPU fallback)")
        T = self.n - 1 if horizon is None else min(int(horizon), self.n - 1)
        if T < 1:
            raise ValueError("access_sensors: a horizon of at least one step inside the episode, got %r (steps = %d)" % (horizon, self.n))
        if envs is None or self._access_T != T:
            sel = np.arange(self.E)
            self._access_T, self._access_anchor, self._access_left = T, np.zeros(self.E, dtype=np.int64), np.zeros(self.E, dtype=np.int64)
        else:
            sel = np.unique(np.asarray(envs, dtype=np.int64).reshape(-1))
            if len(sel) == 0 or sel[0] < 0 or sel[-1] >= self.E:
                raise ValueError("access_sensors: envs must name envs in 0 .. %d, got %r" % (self.E - 1, envs))
        self._access_anchor[sel] = self.i[sel]
        self._access_left[sel] = np.minimum(T, self.n - 1 - self.i[sel])
        words = env_time_words(self, "access_sensors")
        with torch.cuda.stream(self._tasking_stream()):
            left = torch.as_tensor(self._access_left.astype(np.int32)).to("cuda")
            r = self._eng.launch_access_sensors(self.tick % 2, 0, self._sites(), T, envs=None if len(sel) == self.E else sel, n_left=left, **words)
        self._access_stale = set(self._access_stale) - set(int(v) for v in sel)
        p = r["pass"]
        return {"bits": r["bits"], "first": p[..., _lib.PASS_FIRST], "length": p[..., _lib.PASS_LENGTH], "count": p[..., _lib.PASS_COUNT],
                "passes": p[..., _lib.PASS_PASSES], "n_steps": self._access_left.copy()}

    def action_masks(self):
        """The action masks of the NEXT step of every env: bool [E, S, m] on the device (SSA_Tasker_Env.action_masks() per env).  The
        table is made by the first call (access_sensors(): one launch over whole episodes); afterwards a call is one gather and one
        shift-and-mask of it, and launches a kernel of the library only when envs have auto-reset since the last call -- those envs'
        slabs are then made again, all in ONE launch.  A failed filter is not masked out."""
        from .. import device
        if np.any(self.i + 1 >= self.n):
            raise ValueError("action_masks: an env has no next step")
        if self._access_T is None:
            self.access_sensors()
        else:
            k = self.i - self._access_anchor
            stale = sorted(set(self._access_stale) | set(np.where((k < 0) | (k >= self._access_left))[0].tolist()))
            if stale:
                self.access_sensors(self._access_T, envs=stale)
        return device.access_mask(self._eng._access["bits"], self.i - self._access_anchor)

    def evaluate_schedules(self, actions):
        """SSA_Tasker_Env.evaluate_schedules() of every env from ONE dry-run launch (ssa_dryrun_gather_f64, then
        ssa_dryrun_sensors_envs_f64 over E * B pseudo-envs): what each of B candidate schedules per env would be
        worth if rollout_sensors() ran it from env e's state at its step i_e, without spending the envs.  `actions`: integers
        [E, K, S] (B = 1) or [E, B, K, S], numpy or torch, env e's candidates in e's own object numbering (S = n_sensor; 1 without
        config['observers']: the envs' own observer as a one-site network); an entry < 0 or >= m is an idle sensor, two sensors on one
        object in a row are not refused -- the lower one takes it.  ONE horizon for all envs, K' = min(K, min_e(steps - 1 - i_e)), as
        forecast_sensors().  ValueError: a wrong shape or dtype, K' < 1 (an env without a next step).  The single env's dict with a
        leading [n_env] axis, CUDA tensors:
            score   [E, B, K', S, 3] float64: columns _lib.LOOK_* from the step's P- and P+; NaN unless taken
            taken, visible [E, B, K', S] bool;  status [E, B, K', S] int32;  action [E, B, K', S] int64 (-1: no update attempted)
            total   [E, B, 3] float64: the sum of the taken slots' scores per column, in slot order (k outer, s inner); 0 for none
        Nothing of the envs changes: no engine tensor, not i, tick, the bookkeeping or a generator; any rso_count (the gathered block
        has whole tiles).  The next call with the same shapes overwrites the tensors."""
        if self._eng is None:
            raise _lib.SsaHipError("no device state: the dry run of a schedule runs on the GPU only (no CPU fallback)")
        a = check_schedules(actions, self.n_sensor, envs=self.E)
        K = min(int(a.shape[2]), int(self.n - 1 - self.i.max()))
        if K < 1:
            raise ValueError("evaluate_schedules: at least one step inside every env's episode (i = %s, steps = %d, K = %d)"
                             % (self.i.tolist(), self.n, a.shape[2]))
        rec = self._eng.launch_dryrun_sensors_envs(self.tick % 2, 0, self._sites(), a[:, :, :K], stream=self._stream,
                                                   env_times=[int(v) + 1 for v in self.i])
        return schedules_result(rec, self._stream)

    def assign_sensors(self, column, rule='greedy'):
        """the lookahead of every env and every env's assignment over score column `column` (_lib.LOOK_*) by `rule` ('greedy', or
        'optimal': most sensors tasked, then the largest sum): two launches and one read-back of E x 32 bytes.  int64 [E, S]; -1: the
        scores left that sensor without an object.  Nothing of the envs changes."""
        from .. import device
        device.assign_entry(rule)                     # (an unknown rule: refused before anything is launched)
        if self._eng is None:
            raise _lib.SsaHipError("no device state: the assignment comes from the lookahead, which runs on the GPU only (no CPU fallback)")
        look = self._launch_lookahead_sensors()
        cur = self._tasking_stream()
        table = self._eng.launch_assign_sensors_envs(look, column, stream=cur.cuda_stream, rule=rule)
        cur.synchronize()
        return table.cpu().numpy()[:, :self.n_sensor].astype(np.int64)

    # inspection helpers (per env)
    def P_filter(self, e):
        return self._eng.env_caller_rows(e, self._eng.P_filter[self.tick % 2, e * self.m:(e + 1) * self.m]).cpu().numpy()

    def x_filter(self, e):
        return self._eng.env_caller_rows(e, self._eng.x_filter[self.tick % 2, e * self.m:(e + 1) * self.m]).cpu().numpy()

    def x_true(self, e):
        return self._eng.env_caller_rows(e, self._eng.x_true[self.tick % 2, e * self.m:(e + 1) * self.m]).cpu().numpy()
