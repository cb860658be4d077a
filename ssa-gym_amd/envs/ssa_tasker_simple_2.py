"""SSA_Tasker_Env: drop-in for the reference's envs/ssa_tasker_simple_2.py::SSA_Tasker_Env.

Same constructor dict, env id, spaces, return shapes and inspectable attributes
(SURVEY 8b); the per-object arithmetic of reset()/step() runs in the fused HIP kernels
(engine.HotPathEngine).  Host code here is orchestration only: RNG draws in the reference's
order, one launch per step, one small device->host copy for reward/done, lazy numpy views of
the device-resident history.  Citations: ssa_tasker_simple_2.py:line in the reference.
"""
import math
import time
from datetime import timedelta

import numpy as np

from .. import _lib, host
from ._config import draw_initial_state, orbit_site_table, resolve_config, reward_done
from ._gymshim import Env, np_random, spaces
from ._policy import _PolicyLoop
from ._tasking import SENSOR_AGENT_COLUMNS, SENSOR_AGENT_RULES, check_schedules, lookahead_result, network_sites, schedules_result, sensor_agent_rule
from ._views import _FailureMessages, _History, _Sparse


class SSA_Tasker_Env(_PolicyLoop, Env):
    metadata = {'render.modes': ['live', 'none']}
    visualization = None
    n_sensor = 1      # sensors of the network (config['observers']); one observer without

    def __init__(self, config=None):
        s = time.time()
        if config is None:
            from . import env_config as config
        self.runtime = {'__init__': 0, 'reset': 0, 'step': 0, 'step prep': 0, 'propagate next true state': 0,
                        'perform predictions': 0, 'update with observation': 0, 'Observations and Reward': 0,
                        'filter_error': 0, 'visible_objects': 0, 'object_visibility': 0, 'anees': 0,
                        'failed_filters': 0, 'plot_sigma_delta': 0, 'plot_rewards': 0, 'plot_anees': 0,
                        'plot_actions': 0, 'all_true_obs': 0, 'plot_visibility': 0, 'predict method': 0}
        # ---- simulation and filter configuration (:81-118), the sensor network, the kernel constants and the observation options:
        # envs/_config.py resolves them for this env and SSA_Tasker_VecEnv alike
        c = resolve_config(config)
        self.t_0 = config['t_0']
        self.dt, self.n, self.m = c.dt, c.n, c.m
        self.obs_returned = config['obs_returned']
        self.reward_type = config['reward_type']
        self.orbits = config['orbits']
        self.update_interval = config['update_interval']
        self.i = 0
        self.obs_type = c.obs_type
        self.fx, self.hx = config['fx'], config['hx']
        self.mean_z, self.residual_z, self.msqrt = config['mean_z'], config['residual_z'], config['msqrt']
        self.alpha, self.beta, self.kappa = config['alpha'], config['beta'], config['kappa']
        self._model = c.model
        self.x_sigma, self.Q, self.P_0 = c.x_sigma, c.Q, c.P_0
        # (a sensor network, config['observers'] -- DESIGN.md section 8c: sensor 0 is the PRIMARY sensor, the env's observer (obs_lla,
        # obs_limit, z_sigma, R); the 'aer' observation, the visibility helpers and the agents' scores use its site)
        self.z_sigma, self.R = c.z_sigma, c.R
        self.obs_lla, self.obs_itrs, self.obs_limit = c.obs_lla, c.obs_itrs, c.obs_limit
        self.n_sensor = c.n_sensor
        # (config['sensor_measurement']: True where a sensor measures az and el only, section 8r; without a network: the one az-el-range observer)
        self.sensor_angles_only = np.zeros(c.n_sensor, dtype=bool) if c.net is None else c.net.angles_only
        # (config['sensor_illumination']: True where a sensor sees only sunlit objects, and only from a dark site, section 8t; sun_table: the
        # Sun's direction per row of trans_matrix, None unless a sensor asks for it; sun_dark: per row the word of the sites' dark bits)
        self.sensor_sunlit_only = np.zeros(c.n_sensor, dtype=bool) if c.net is None else c.net.sunlit_only
        self.sun_table, self.sun_dark, self.shadow_radius = c.sun, c.sun_dark, c.shadow_radius
        # (config['observers'] entries {'orbit': ...}: True where a sensor is space-based, section 8v; site_table: its [n, S, 16] site rows
        # per row of trans_matrix -- the orbit propagated on the device, here and now --, None without one; limb_radius: the sphere its
        # line of sight must clear)
        self.sensor_moving = np.zeros(c.n_sensor, dtype=bool) if c.net is None else c.net.moving
        self.limb_radius = c.limb_radius
        self.site_table = orbit_site_table(c, config)
        if c.net is not None:
            self.sensor_lla, self.sensor_obs_limit = c.net.lla, c.net.obs_limit
            self.sensor_z_sigma, self.sensor_R = c.net.z_sigma, c.net.R
        self.time = [self.t_0 + (timedelta(seconds=self.dt) * i) for i in range(self.n)]
        self.trans_matrix = c.trans
        self.x_noise = np.empty(shape=(self.m, 6))
        self.filters = []   # the reference keeps one filterpy object per RSO; state lives in HBM here
        self.rewards = np.empty(self.n)
        self.failed_filters_id = []
        self.failed_filters_msg = _FailureMessages(self.m)
        # (a sensor network: one column per sensor -- actions (n, S), obs_taken (n, S), sigmas_h (n, S, 13, 3), S (n, S, m, 3, 3))
        sens = (self.n_sensor,) if self.n_sensor > 1 else ()
        self.actions = np.empty((self.n,) + sens, dtype=int)
        self.obs_taken = np.empty((self.n,) + sens, dtype=bool)
        self.x_failed = np.copy(host.X_FAILED)
        self.P_failed = np.copy(host.P_FAILED)
        self.visibility = []
        self.sigmas_h = np.empty((self.n,) + sens + (13, 3))
        self.S = np.empty((self.n,) + sens + (self.m, 3, 3)) if self.n * self.m * self.n_sensor <= (1 << 22) else None
        # ---- spaces (:163-177)
        self.action_space = spaces.MultiDiscrete([self.m] * self.n_sensor) if self.n_sensor > 1 else spaces.Discrete(self.m)
        if self.obs_returned == 'aer':
            self.observation = np.zeros(self.m * 4)
        # (config['obs_dtype'] = 'float32': the observation reaches the host in single precision; the device-resident history and
        # everything computed stay float64)
        self._obs_f32 = c.obs_f32
        self.observation_space = c.obs_space
        # ---- device engine
        hist = config.get('history', 'auto')
        bytes_per_step = self.m * (6 + 6 + 36 + 12 + 4) * 8
        if hist == 'auto':
            hist = 'full' if self.n * bytes_per_step <= 64 * 2 ** 30 else 2
        self._H = self.n if hist == 'full' else max(2, int(hist))
        self._consts, self._sensor_consts = c.consts, c.sensor_consts
        self._engine = None
        self._device_rng = bool(config.get('device_rng', False))
        self._storage_layout = c.storage_layout      # (how the engine STORES the objects: reset())
        self._obs_buffers = config.get('obs_buffers', 2)
        # step() hands out a FRESH array per call for the 'flatten' and (m, 12) observations, as the reference does (:360-366: `.flatten()` /
        # a row of the history that no later step overwrites) -- a consumer may keep it as long as it likes (replay buffers, sample
        # collectors, GAE targets).  config['obs_zero_copy'] = True (opt-in): a VIEW of the host-mapped ring the kernel writes, valid until
        # `obs_buffers` (default 2) further steps have been taken -- no 1.9 MB host copy per step at 20 000 objects
        self._obs_zero_copy = c.obs_zero_copy
        self._obs_pool_cap = config.get('obs_pool', 64)      # (pinned buffers that may be out with the consumer at once; beyond: copies)
        # the persistent closed loop's bound on any wait inside the launch (100 MHz ticks; 0 = the library's 2 s)
        self._loop_wait_ticks = int(config.get('closed_loop_wait_ticks', 0))
        self._loop_debug_withhold = False
        # config['obs_device'] = True: step() returns the observation as a CUDA tensor -- a view of the device-resident history slot
        # ('aer': of the persistent (4 m,) block) -- and nothing crosses PCIe
        self._obs_device = c.obs_device
        # run_agent(): the persistent closed-loop kernel (one launch per chunk) unless config['closed_loop'] == 'per_step'
        self._closed_loop_persistent = config.get('closed_loop', 'persistent') != 'per_step'
        self.loop_gave_up = 0                  # persistent launches of run_agent that gave up and were re-run per step
        # run_policy's graphs by (id(policy), chunk length, history phase), None where the policy cannot be captured (policy_graph_error: why);
        self._policy_graphs, self._policy_refs, self.policy_graph_error = {}, {}, None      # _policy_refs: those policies, kept alive
        self.np_random = None
        self.init_seed = self.seed(config.get('seed'))[0]
        self.reset()
        self.runtime['__init__'] += time.time() - s

    # ------------------------------------------------------------------ gym API
    def seed(self, seed=None):
        self.np_random, seed = np_random(seed)   # old-gym hash_seed -> RandomState (:188-191)
        self.init_seed = seed
        return [seed]

    def _build_engine(self):
        from .. import engine
        self._engine = engine.HotPathEngine(self._consts, self.m, 1, self.trans_matrix, self._z_noise_dev, self._H)
        e = self._engine
        import torch
        self._aer_dev = torch.zeros(self.m * 4, dtype=torch.float64, device="cuda")
        self._stream = torch.cuda.current_stream()
        self._look_sites = None                # the sites of the env as a network (_sites); this and the next two: made on first use
        self._argmax_ws, self._argmax_ws_n = None, 0     # PolicyView.argmax's workspace (owned by the env: its launches share a stream)
        self._policy_streams = None            # capture / replay stream and the copy stream of the pipelined chunks: one pair per env
        # host-mapped mailboxes (pinned memory is addressable from the GPU): the kernels read the action
        # from / write statistics and the update record to host memory directly, so a step needs one
        # stream synchronisation and one observation copy instead of four blocking transfers
        self._stats_host = torch.zeros(_lib.STAT_STRIDE, dtype=torch.float64).pin_memory()
        if self.n_sensor > 1:     # the network's sites and one update record per sensor (host-mapped, as the single record)
            self._sensors = host.make_sensor_params(self.sensor_lla, self.sensor_obs_limit, self.sensor_R, self.n * self.m * 3,
                                                    angles_only=self.sensor_angles_only, sunlit_only=self.sensor_sunlit_only,
                                                    shadow_radius=self.shadow_radius)
            if self.sun_table is not None:      # (the packed table lives on the device next to trans; the block points at it)
                e.set_sun_table(self.sun_table, self.sun_dark, [self._sensors])
            if self.site_table is not None:     # (... and the moving sensors' site rows: every sensor launch of the engine carries them)
                e.set_site_table(self.site_table, self.sensor_moving, self.limb_radius)
            self._upd_s_host = torch.zeros((self.n_sensor, _lib.UPD_STRIDE), dtype=torch.float64).pin_memory()
            self._upd_s_np, self._upd_s_ptr = self._upd_s_host.numpy(), self._upd_s_host.data_ptr()
        self._upd_host = torch.zeros(_lib.UPD_STRIDE, dtype=torch.float64).pin_memory()
        # The observation reaches the host FROM INSIDE the step kernel: its epilogue writes the (az, el, range, trace P) block
        # ('aer') or a second copy of the observation rows (other modes) straight into host-mapped pinned memory, overlapped
        # with the other wavefronts' arithmetic -- no copy-engine pass behind the kernel (1.92 MB 'flatten' vector: 44 us).
        # 'aer' hands out ONE persistent array refreshed in place, as the reference does (:362-363); the other modes a buffer nobody
        # holds, returned as a fresh array (the reference returns a fresh array per step) unless config['obs_zero_copy'] asks for a
        # view of the ring the kernel writes, which stays intact until step i + `obs_buffers` (default 2) is taken (envs/_obspool.py)
        from ._obspool import HostObs
        aer = self.obs_returned == 'aer'
        self._mirror_f32 = self._obs_f32 and not self._obs_device      # (obs_device hands out the float64 device tensors themselves)
        self._obs_host = HostObs(self.m * (4 if aer else 12), self.observation_space.shape, self._mirror_f32,
                                 1 if aer else max(2, int(self._obs_buffers)),
                                 None if (aer or self._obs_zero_copy or self._obs_device) else self._obs_pool_cap)
        self._obs_pool = self._obs_host.pool
        # (numpy views and raw pointers of the mailboxes, taken once: each .numpy() / .data_ptr() costs the step a microsecond)
        self._upd_np, self._stats_np = self._upd_host.numpy(), self._stats_host.numpy()
        self._upd_ptr, self._stats_ptr = self._upd_host.data_ptr(), self._stats_host.data_ptr()
        if aer:
            self.observation = self._obs_host.ring_np[0]
        self.x_true = _History(self, e.x_true, self.m, (6,))
        self.x_filter = _History(self, e.x_filter, self.m, (6,))
        self.P_filter = _History(self, e.P_filter, self.m, (6, 6))
        self.obs = _History(self, e.obs, self.m, (12,))
        self._met = [_History(self, e.metrics[:, 0, k], self.m, ()) for k in range(4)]
        self.delta_pos, self.delta_vel, self.sigma_pos, self.sigma_vel = self._met

    def reset(self):
        s = time.time()
        import torch
        m, n = self.m, self.n
        x_true0, x_filter0 = draw_initial_state(self.np_random, self.orbits, m, self.x_sigma, self._device_rng, self.x_noise)
        # ... then n*m*3 normals (:219-221); RandomState.normal keeps its Box-Muller cache across
        # calls, so one bulk draw consumes the stream exactly like the reference's n*m size-3 draws
        if self._device_rng:
            gen = torch.Generator(device="cuda").manual_seed(int(self.np_random.randint(0, 2 ** 31 - 1)))
            zs = torch.as_tensor(self.z_sigma, dtype=torch.float64, device="cuda")
            if self.n_sensor > 1:     # (a leading sensor axis: sensor s draws z_noise[s][i][j])
                zs = torch.as_tensor(self.sensor_z_sigma, dtype=torch.float64, device="cuda").view(self.n_sensor, 1, 1, 3)
                self._z_noise_dev = torch.randn((self.n_sensor, n, m, 3), dtype=torch.float64, device="cuda", generator=gen) * zs
            else:
                self._z_noise_dev = torch.randn((1, n, m, 3), dtype=torch.float64, device="cuda", generator=gen) * zs
            self.z_noise = None
        else:
            self.z_noise = self._draw_z_noise()
            self._z_noise_dev = torch.as_tensor(self.z_noise, dtype=torch.float64).to("cuda")
        if self._engine is None:
            self._build_engine()
        else:
            self._engine.z_noise.copy_(self._z_noise_dev.reshape(self._engine.z_noise.shape))
        # STORAGE LAYOUT (round 4, config['storage_layout'] = 'regime'; default off): the engine keeps objects of one orbit regime in the same
        # wavefronts -- ascending semi-major axis, dealt tile by tile over the XCDs (catalogue.regime_order) -- because late in an episode
        # the diverged filters are the LEO objects, and packed they cost a launch 15 % less.  Nothing of it shows: the
        # step kernel speaks the env's own indices wherever an index enters or leaves it (actions, failure records, arg-max of sigma_pos, the
        # observation rows it writes for the host), an object's arithmetic does not depend on its position (bit-identical episodes,
        # build_ablate/layout_episode_ab.py), and whatever reads the device state as the env numbers it -- the history arrays, the device-side
        # agents' scores and policies' views, rollout -- puts the state back first (_caller_order(): the layout is then off until the next
        # reset(); run_agent keeps it: its kernels take the table).  OFF by default HERE: what step() gains in the kernel (2-5 us late in an episode) it loses on the way to the host -- the
        # observation rows leave the kernel row by row at the env's indices instead of tile by tile (1.9 MB over PCIe in 96-byte pieces: 'flatten'
        # 73 -> 84 us per step at 20 000 objects).  It pays for launch sequences that keep the observations on the device: the engine-level
        # loops (HotPathEngine.set_layout; bench.py's `value`), C-ABI callers (ssa_step_params.obj_ids).
        lay = self._storage_layout == 'regime' and m >= 64 and not self._obs_device
        if lay:
            from ..catalogue import regime_order
            self._engine.set_layout(regime_order(x_true0))
        else:
            self._engine.set_layout(None)
        self._engine.load_state(0, x_true0, x_filter0, np.broadcast_to(self.P_0, (m, 6, 6)))
        # tracking variables (:222-231)
        self.actions[:], self.obs_taken[:], self.failed_filters_id, self.visibility = -1, False, [], []
        self.failed_filters_msg = _FailureMessages(self.m)
        self.rewards[:] = 0
        self.sigmas_h[:] = 0
        if self.S is not None:
            self.S[:] = np.nan
        sens = (self.n_sensor,) if self.n_sensor > 1 else ()
        self._y = np.full((n,) + sens + (3,), np.nan)
        self._z_true = np.full((n,) + sens + (3,), np.nan)
        self._S_sel = np.full((n,) + sens + (3, 3), np.nan)
        self._upd_action = np.full((n,) + sens, -1, dtype=int)
        if sens:      # (a sensor network: per-sensor records (n, S, 3), NaN where the sensor updated nothing)
            self.y, self.z_true = self._y, self._z_true
        else:
            self.y = _Sparse(self, self._y, (3,))
            self.z_true = _Sparse(self, self._z_true, (3,))
        self._n_failed = 0
        self._fail_read, self._fail_pending, self._fail_chunk_total = 0, {}, 0      # records of the kernel's failure log consumed so far
        self._engine.fail_log[:] = 0.0             # (time index 0 = "not written": steps count from 1)
        self._ring_head = None
        self._argmax_sigma_prev = None
        self._access_anchor = None      # (a new truth: action_masks() makes its table again)
        self.i = 0
        self._fetch_small(0)
        self.runtime['reset'] += time.time() - s
        return self._obs_out()

    def _draw_z_noise(self):
        """the measurement noise of the episode from np_random (:219-221): (n, m, 3); a sensor network (S, n, m, 3) -- sensor 0's draws are
        the reference's stream, sensors 1 .. S-1 draw after it, in order"""
        z = self.np_random.normal(size=(self.n, self.m, 3)) * self.z_sigma
        if self.n_sensor > 1:
            z = np.stack([z] + [self.np_random.normal(size=(self.n, self.m, 3)) * self.sensor_z_sigma[k] for k in range(1, self.n_sensor)])
        return z

    def _fetch_small(self, i):
        e = self._engine
        slot = i % e.H
        self._stats = e.stats[slot, 0].cpu().numpy()     # synchronises the stream
        self._argmax_sigma = int(self._stats[_lib.STAT_ARGMAX_SPOS])

    def _caller_order(self):
        """the device state back in the env's own object order (drops the engine's storage layout until the next reset(); a no-op without)"""
        if self._engine is not None:
            self._engine.to_caller_order()

    def _obs_out(self, refresh_aer_dev=False):
        """the observation of the current step through the slow path (reset(), rollout(), run_agent()): a device-to-host copy (gathered into
        the env's object order while a storage layout is set: a reset does not cost the layout).  'aer' refreshes self.observation in
        place; with refresh_aer_dev (the multi-step drivers) it goes through self._aer_dev, the (4 m,) block an obs_device consumer may
        hold, which reset() leaves alone"""
        e, slot = self._engine, self.i % self._engine.H
        if self.obs_returned == 'aer':
            if not refresh_aer_dev:
                return self.aer_obs(self.observation)
            from .. import device
            M = e.trans[self.i % e.n_time].reshape(3, 3)
            device.aer_obs(e.x_filter[slot], e.P_filter[slot], M, self._consts, out=self._aer_dev.view(self.m, 4))
            self.observation[:] = e.caller_rows(self._aer_dev.view(self.m, 4)).cpu().numpy().reshape(-1)
            return self.observation
        obs = e.caller_rows(e.obs[slot]).cpu().numpy()
        return self._obs_host.cast(obs.reshape(-1) if self.obs_returned == 'flatten' else obs)

    def step(self, a):
        """step() of the reference (:265-367); with a sensor network (config['observers'] with S > 1 sites) `a` holds one object per
        sensor, all different, and sensor s updates object a[s] with its own site, elevation mask, R and noise (ssa_env_step_sensors_f64)
        in the same single launch"""
        step_s = time.time()
        S = self.n_sensor
        if S == 1:
            assert self.action_space.contains(a), "%r (%s) invalid" % (a, type(a))
        else:
            if self._engine is None:
                raise _lib.SsaHipError("no device state: a sensor network's step runs on the GPU only (no CPU fallback)")
            if not self.action_space.contains(a):
                raise AssertionError("%r (%s) invalid: one object in 0 .. %d per sensor (%d sensors)" % (a, type(a), self.m - 1, S))
            a = np.asarray(a, dtype=np.int64)
            if len(np.unique(a)) != len(a):
                raise ValueError("step: two sensors tasked to the same object (%s)" % (a,))
        self._argmax_sigma_prev = self._argmax_sigma
        self._ring_head = None
        self.i += 1
        i = self.i
        self.actions[i] = a
        e = self._engine
        s = time.time()
        self.runtime['step prep'] += s - step_s
        # propagate + predict + update + observations/metrics + statistics: ONE launch (:265-322; the step kernel's last wavefront folds
        # the statistics, SSA_LAUNCH_FOLD_INSIDE).  The action travels by value in the parameter block (a network's actions in its sensor
        # block); statistics, update records and the observation are written by the kernel straight into host-mapped pinned memory: ONE
        # stream synchronisation, no copy
        cur = self._stream                    # (the stream the engine was built in; torch.cuda.current_stream() costs 3 us per call,
        #                                        and every step ends with a synchronisation, so later work in any stream sees its results)
        aer = self.obs_returned == 'aer'
        shaped = self.reward_type == 'shaped'      # needs np.argmax(sigma_pos[i - 1]) (:346): the arg-max slots of the one-launch path
        if self._obs_device:
            aer_out, mirror = (self._aer_dev.data_ptr() if aer else 0), 0
        else:
            dst = self._obs_host.dest(i)
            aer_out, mirror = (dst, 0) if aer else (0, dst)
        if S == 1:
            e.launch_step((i - 1) % e.H, i % e.H, i, action=int(a), aer_out=aer_out, obs_mirror=mirror, stats_out=self._stats_ptr,
                          upd_out=self._upd_ptr, stream=cur.cuda_stream, fast_stats=True, fold_inside=True, argmax_spos=shaped,
                          mirror_f32=self._mirror_f32)
        else:
            e.launch_step_sensors((i - 1) % e.H, i % e.H, i, self._sensors, a, self._upd_s_ptr, aer_out=aer_out, obs_mirror=mirror,
                                  stats_out=self._stats_ptr, stream=cur.cuda_stream, fast_stats=True, fold_inside=True, argmax_spos=shaped,
                                  mirror_f32=self._mirror_f32)
        cur.synchronize()
        self._stats = self._stats_np.copy()
        self._argmax_sigma = int(self._stats[_lib.STAT_ARGMAX_SPOS])
        t_dev = time.time()
        self.runtime['perform predictions'] += t_dev - s
        if S == 1:
            self._book_update(i, a, self._upd_np)
        else:
            for k in range(S):
                self._book_update(i, a[k], self._upd_s_np[k], sensor=k)
        if int(self._stats[_lib.STAT_N_FAILED]) != self._n_failed:
            self._record_failures()
        done = self._reward_done(i, a, self._stats, self._argmax_sigma_prev)
        # 'aer' hands out its ONE persistent array refreshed in place, as the reference does (:362-363: self.observation); the other
        # modes a fresh array unless config['obs_zero_copy']
        if self._obs_device:
            obs = self._aer_dev if aer else (e.obs[i % e.H].reshape(-1) if self.obs_returned == 'flatten' else e.obs[i % e.H])
        else:
            obs = self._obs_host.hand_out()
        e_t = time.time()
        self.runtime['Observations and Reward'] += e_t - t_dev
        self.runtime['step'] += e_t - step_s
        return obs, self._returned_reward(self.rewards[i]), done, {}

    def _single_sensor(self, what):
        if self.n_sensor > 1:
            raise NotImplementedError("%s: not implemented for a sensor network (config['observers'] with %d sensors); "
                                      "use step()%s" % (what, self.n_sensor, " or rollout_sensors()" if what == 'rollout' else ""))

    # ------------------------------------------------------------------ per-step host bookkeeping
    def _book_update(self, i, a, rec, sensor=None):
        """update record of step i (:292-315) into the env's sparse histories (a sensor network: the record of `sensor`, into its column)"""
        if rec[_lib.UPD_ACTION] >= 0:
            a = int(a)
            at = i if sensor is None else (i, sensor)
            self._upd_action[at] = a
            self._z_true[at] = rec[_lib.UPD_Z_TRUE:_lib.UPD_Z_TRUE + 3]
            if rec[_lib.UPD_OBS_TAKEN] == 1.0:
                self._y[at] = rec[_lib.UPD_Y:_lib.UPD_Y + 3]
                self._S_sel[at] = rec[_lib.UPD_S:_lib.UPD_S + 9].reshape(3, 3)
                if self.S is not None:
                    self.S[(i, a) if sensor is None else (i, sensor, a)] = self._S_sel[at]
                self.sigmas_h[at] = rec[_lib.UPD_SIGMAS_H:_lib.UPD_SIGMAS_H + 39].reshape(13, 3)
                self.obs_taken[at] = True

    def _reward_done(self, i, a, st, argmax_sigma_prev):
        """reward / done of step i from its statistics (:324-354, envs/_config.py: reward_done); fills self.rewards[i].  The statistics
        are taken over all objects whatever the number of sensors; with a sensor network 'shaped' pays its +1/n if ANY sensor tasked
        np.argmax(sigma_pos[i - 1])"""
        if self.reward_type == 'shaped':     # (what the episode has paid: summed on a win only)
            hit = (a == argmax_sigma_prev) if self.n_sensor == 1 else bool(np.any(np.asarray(a) == argmax_sigma_prev))
            self.rewards[i], done = reward_done('shaped', st, hit, lambda: np.sum(self.rewards[:i]), i + 1 >= self.n, self.m, self.n)
        else:
            self.rewards[i], done = reward_done(self.reward_type, st, False, None, i + 1 >= self.n, self.m, self.n)
        return done

    def _returned_reward(self, r):
        """the reward as step() hands it out: np.nan_to_num(r, nan=0.5, posinf=0.5, neginf=0.5) of a scalar (:365-367), except in the
        'flatten' mode, which returns it as it is"""
        return r if (self.obs_returned == 'flatten' or np.isfinite(r)) else np.float64(0.5)

    def _ring_chunk(self, i0, kk, upd_ring):
        """(statistics, update records) of steps i0 + 1 .. i0 + kk from the engine's statistics ring and the record ring `upd_ring`
        [H, ...] (run_agent: the engine's own, e.upd[:, 0]); synchronises the stream"""
        e = self._engine
        slots = [(i0 + 1 + k) % e.H for k in range(kk)]
        return e.stats[slots, 0].cpu().numpy(), upd_ring[slots].cpu().numpy()

    def _book_steps(self, acts, stats, upd, ring_head, out, check_actions=False):
        """the bookkeeping of consecutive step() calls for steps self.i + 1, ... of a multi-step launch (rollout, run_agent, run_policy):
        actions, update records, failures, rewards, dones, arg-max of sigma_pos, in step order, up to the first `done`.  `ring_head`: the
        newest step the history rings hold; check_actions: a ValueError for an action outside 0 .. m-1 before its step is booked
        (run_policy).  A sensor network (rollout_sensors): acts[k] holds one object per sensor and upd[k] one record per sensor.
        Appends the booked steps to the caller's lists out = (actions, rewards, dones), rewards as step() hands them
        out; returns the `done` of the last booked step."""
        self._ring_head = ring_head
        self._fail_chunk_total = int(stats[-1][_lib.STAT_N_FAILED])      # (the chunk's last LAUNCHED step, even when booking stops early)
        actions, rewards, dones = out
        for k in range(len(acts)):
            self.i += 1
            i = self.i
            if self.n_sensor > 1:      # (a sensor network: acts[k] one object per sensor, upd[k] one record per sensor)
                a = np.asarray(acts[k], dtype=np.int64)
                self.actions[i] = a
                for q in range(self.n_sensor):
                    self._book_update(i, a[q], upd[k][q], sensor=q)
            else:
                a = int(acts[k])
                if check_actions and not (0 <= a < self.m):
                    raise ValueError("run_policy: the policy chose action %d at step %d (valid: 0 .. %d)" % (a, i, self.m - 1))
                self.actions[i] = a
                self._book_update(i, a, upd[k])
            self._stats = stats[k]
            if int(stats[k][_lib.STAT_N_FAILED]) != self._n_failed:
                self._record_failures(at_step=i)
            done = self._reward_done(i, a, stats[k], self._argmax_sigma)
            self._argmax_sigma = int(stats[k][_lib.STAT_ARGMAX_SPOS])      # (-1 unless 'shaped' asked for it)
            actions.append(a)
            rewards.append(self._returned_reward(self.rewards[i]))
            dones.append(done)
            if done:
                break
        return done

    def rollout(self, actions):
        """Open-loop extension (no reference counterpart as ONE call): apply `actions` as consecutive step()
        calls would -- the loop of the reference's agent_naive_random / round-robin drivers (agents.py,
        tests.py:584-603) -- with up to H-1 steps per kernel launch (ssa_env_rollout_f64: state resident on
        chip across the steps, results bit-identical to step()).  Stops at the first `done`.  Returns
        (observation after the last executed step, rewards[k], dones[k], info).  Every reward type ('shaped': the arg-max of
        sigma_pos of every step comes from the rollout's arg-max slots, ssa_rollout_params.spos_tiles)."""
        self._single_sensor('rollout')
        self._caller_order()
        actions = np.asarray(actions, dtype=np.int64).ravel()
        for a in actions:
            assert self.action_space.contains(int(a)), "%r invalid" % (a,)
        e = self._engine
        return self._run_schedule(actions, actions.reshape(-1, 1), e.launch_rollout, lambda: e.upd[:, 0])

    def rollout_sensors(self, actions):
        """rollout() for a sensor network (no reference counterpart; include/ssa_hip.h: ssa_env_rollout_sensors_f64):
        apply the tasking schedule `actions` [K, S] -- row k one object per sensor, all different, as step() takes them -- as consecutive
        step() calls would, with up to H-1 steps per kernel launch and results bit-identical to step()'s.  Stops at the first `done`.
        Returns what rollout() returns: (observation after the last executed step, rewards[k], dones[k], info); books per step and per
        sensor what step() books.  Without config['observers'] (S = 1: the env's own observer as a one-site network) it equals
        rollout(actions[:, 0]) bit for bit.  A row that step() would refuse is refused before anything is launched."""
        if self._engine is None:
            raise _lib.SsaHipError("no device state: a sensor network's rollout runs on the GPU only (no CPU fallback)")
        S = self.n_sensor
        actions = np.asarray(actions)
        if actions.ndim != 2 or actions.shape[1] != S or actions.dtype.kind not in "iu":
            raise AssertionError("rollout_sensors: an integer schedule [K, %d] (one object per sensor and step), got %s %s"
                                 % (S, actions.dtype, actions.shape))
        actions = actions.astype(np.int64)
        for k, row in enumerate(actions):
            if not (self.action_space.contains(row) if S > 1 else self.action_space.contains(int(row[0]))):
                raise AssertionError("rollout_sensors: row %d (%s) invalid: one object in 0 .. %d per sensor (%d sensors)"
                                     % (k, row, self.m - 1, S))
            if len(np.unique(row)) != S:
                raise ValueError("rollout_sensors: row %d tasks two sensors to the same object (%s)" % (k, row))
        self._caller_order()
        e, sites = self._engine, self._sites()
        return self._run_schedule(actions if S > 1 else actions[:, 0], actions,
                                  lambda slot, t, act, **kw: e.launch_rollout_sensors(slot, t, sites, act, **kw),
                                  lambda: e.upd_sensors if S > 1 else e.upd_sensors[:, 0])      # (allocated by the first launch)

    def _run_schedule(self, acts, sched, launch, upd_ring):
        """the chunk loop of rollout() and rollout_sensors(): the validated schedule -- acts[k] as _book_steps takes step k, sched[k] its
        row of the launch's device tensor -- in chunks of up to H-1 steps, each enqueued by launch(slot_in, time index, rows on the
        device, argmax_spos=) and booked from the statistics ring and the record ring upd_ring(), up to the first `done`.  Returns
        what both return."""
        import torch
        shaped = self.reward_type == 'shaped'     # (np.argmax(sigma_pos) of every step from the arg-max slots of the rollout)
        e = self._engine
        K = min(len(acts), self.n - 1 - self.i)
        rewards, dones = [], []
        pos, done = 0, False
        while pos < K and not done:
            kk = min(K - pos, e.H - 1)
            i0 = self.i
            launch(i0 % e.H, i0 + 1, torch.as_tensor(sched[pos:pos + kk].astype(np.int32)).to(e.dev), argmax_spos=shaped)
            stats, upd = self._ring_chunk(i0, kk, upd_ring())
            done = self._book_steps(acts[pos:pos + kk], stats, upd, i0 + kk, ([], rewards, dones))
            pos += kk
        return self._obs_out(refresh_aer_dev=True), np.asarray(rewards), np.asarray(dones, dtype=bool), {}

    def _sites(self):
        """the sites of the env as a network: its own; without config['observers'] the env's one observer as a one-site block, built once"""
        return network_sites(self, self.obs_lla, self.obs_limit, self.R)

    AGENT_KINDS = {'agent_naive_greedy': _lib.AGENT_NAIVE_GREEDY, 'agent_visible_greedy': _lib.AGENT_VISIBLE_GREEDY,
                   'agent_visible_greedy_aer': _lib.AGENT_VISIBLE_GREEDY, 'agent_shannon': _lib.AGENT_SHANNON,
                   'agent_pos_error_greedy': _lib.AGENT_POS_ERROR, 'agent_vel_error_greedy': _lib.AGENT_VEL_ERROR}

    def run_agent(self, agent, n_steps, fallback_actions=None):
        """Closed loop on the device (no reference counterpart as ONE call): the loop
            a = agent(obs, env); obs, r, done, _ = env.step(a)
        of the reference's drivers (run_environment.py, compare_agents.py) for one of its greedy agents (agents.py: `agent`
        is the function or its name), with the agent's arg-max computed on the GPU and handed to the next step's launch
        in-stream -- no host round trip per step.  `fallback_actions[k]` replaces the reference's action_space.sample()
        when no object is visible at decision k (default: draws from the env's action space, as the reference does).
        Stops at the first `done`.  Returns (observation after the last executed step, actions[k], rewards[k], dones[k]).
        Every reward type.  If the persistent launch gives up (a wavefront waited longer than config['closed_loop_wait_ticks'] for a
        decision: something else holds the GPU's wavefront slots) the env restores the state the chunk started from, takes the
        per-step launches for this and every later call, and warns once."""
        self._single_sensor('run_agent')
        import torch
        name = agent if isinstance(agent, str) else getattr(agent, "__name__", None)
        if name not in self.AGENT_KINDS:
            raise NotImplementedError("run_agent: %r has no device-side version (supported: %s)" % (agent, sorted(self.AGENT_KINDS)))
        shaped = self.reward_type == 'shaped'     # (np.argmax(sigma_pos) of every step travels with the decision / the arg-max slots)
        kind = self.AGENT_KINDS[name]
        e = self._engine
        K = min(int(n_steps), self.n - 1 - self.i)
        if fallback_actions is None:
            fallback_actions = [self.action_space.sample() for _ in range(K + 1)]
        fbh = np.asarray(fallback_actions, dtype=np.int32)[:K + 1]
        assert fbh.size >= K, "one fallback action per decision"
        if fbh.size < K + 1:      # (the decision AFTER the last step is computed too and nobody uses it)
            fbh = np.concatenate([fbh, np.full(K + 1 - fbh.size, -1, dtype=np.int32)])
        fb = torch.as_tensor(fbh).to(e.dev)
        log = torch.full((K + 1,), -1, dtype=torch.int32, device=e.dev)     # log[k] = action of step i0 + k + 1
        actions, rewards, dones = [], [], []
        pos, done = 0, False
        e.launch_agent_select(self.i, self.i, kind, log.data_ptr(), fallback_ptr=fb.data_ptr(), have_prev=self.i >= 1)
        persistent = bool(self._closed_loop_persistent)
        while pos < K and not done:
            # 'trinary' has no early `done`: the whole run is one chunk; otherwise every step of a chunk must stay resident
            # in the history ring, because the step that turns out to be the last one is the state this call returns
            kk = (K - pos) if (persistent and self.reward_type == 'trinary') else min(K - pos, e.H - 1)
            i0 = self.i
            used = False
            if persistent:
                # ONE launch for the kk steps and their kk decisions (ssa_env_closed_loop_f64)
                stats_d = torch.empty((kk, _lib.STAT_STRIDE), dtype=torch.float64, device=e.dev)
                upd_d = torch.empty((kk, _lib.UPD_STRIDE), dtype=torch.float64, device=e.dev)
                snap = e.snapshot_state(i0 % e.H)      # (what a launch that gives up is undone to: ~9 MB device-to-device at 20 000 objects)
                first = log[pos:pos + 1].clone()
                used = e.launch_closed_loop(i0 % e.H, i0 + 1, kind, log[pos:pos + kk + 1], stats_d, upd_d, fallback=fb[pos:pos + kk + 1],
                                            argmax_spos=shaped, wait_ticks=self._loop_wait_ticks, debug_withhold=self._loop_debug_withhold)
                if used:
                    stats = stats_d.cpu().numpy()                      # synchronises the stream
                    upd = upd_d.cpu().numpy()
                    if int(e.loop_error[0]) != 0:
                        # the launch gave up (every wait inside it is bounded): the rings hold a partial chunk.  Back to the state the
                        # chunk started from, and per-step launches from here on -- for this env: whatever took the wavefront slots
                        # (another stream's kernels, another process on the card) may well stay
                        import warnings
                        warnings.warn("ssa_env_closed_loop_f64 gave up (a wavefront waited longer than the bound for a decision); "
                                      "the chunk is re-run with per-step launches, which this env uses from now on", RuntimeWarning)
                        e.restore_state(i0 % e.H, snap)
                        log[pos:pos + 1].copy_(first)
                        log[pos + 1:pos + kk + 1].fill_(-1)
                        self.loop_gave_up += 1
                        self._closed_loop_persistent = False
                        used = False
                if not used:
                    persistent = False
                    kk = min(kk, e.H - 1)
                del snap
            if not used:
                for k in range(kk):
                    i = i0 + k + 1
                    e.launch_step((i - 1) % e.H, i % e.H, i, actions_ptr=log.data_ptr() + 4 * (pos + k), fast_stats=True, defer_fold=True,
                                  argmax_spos=shaped)
                    if pos + k + 1 < K:     # (the decision for the step after this one)
                        e.launch_agent_select(i, i, kind, log.data_ptr() + 4 * (pos + k + 1), fallback_ptr=fb.data_ptr() + 4 * (pos + k + 1))
                e.flush_stats()
                stats, upd = self._ring_chunk(i0, kk, e.upd[:, 0])
            done = self._book_steps(log[pos:pos + kk].cpu().numpy(), stats, upd, i0 + kk, (actions, rewards, dones))
            pos += kk
        return self._obs_out(refresh_aer_dev=True), np.asarray(actions, dtype=int), np.asarray(rewards), np.asarray(dones, dtype=bool)

    # (every agent run_agent_sensors takes: the one table of envs/_tasking.py under the names it has here)
    SENSOR_AGENT_COLUMNS, SENSOR_AGENT_RULES = SENSOR_AGENT_COLUMNS, SENSOR_AGENT_RULES

    def run_agent_sensors(self, agent, n_steps, fallback_actions=None):
        """run_agent() for a sensor network (no reference counterpart): the loop
            a = agent(obs, env); obs, r, done, _ = env.step(a)
        for agents.agent_info_gain_sensors / agent_trace_gain_sensors and their *_optimal forms (`agent`: the function or its name) with the
        assignment computed on the GPU (ssa_assign_sensors_f64; *_optimal: ssa_match_sensors_f64) and handed to the step in-stream.  Per step three launches in one stream -- every sensor's
        lookahead, the assignment into row k of a device log, the step that reads that row (ssa_env_rollout_sensors_f64 with a one-row
        schedule) -- and nothing is read back until a chunk of up to H-1 steps ends.  Stops at the first `done`.  Returns what run_agent
        returns: (observation after the last executed step, actions [k, S], rewards [k], dones [k]); books per step and per sensor what
        step() books.  Without config['observers'] (S = 1) the env's own observer runs as a one-site network.
        `fallback_actions` [K + 1, S]: row k holds the draws for the sensors the scores leave without an object at decision k (default:
        one action_space.sample() per row; env.np_random is not touched).  The device's rule differs from the host agents' redraw loop:
        sensor s, in ascending s, takes its draw if no sensor holds that object, and otherwise STAYS IDLE at that step -- booked as action
        -1 with no update record, a row step() itself cannot express (it wants one object per sensor)."""
        if self._engine is None:
            raise _lib.SsaHipError("no device state: a sensor network's closed loop runs on the GPU only (no CPU fallback)")
        import torch
        column, rule = sensor_agent_rule(agent, 'run_agent_sensors')
        self._caller_order()
        shaped = self.reward_type == 'shaped'
        e, sites, S, W = self._engine, self._sites(), self.n_sensor, _lib.MAX_SENSORS
        K = max(min(int(n_steps), self.n - 1 - self.i), 0)
        if fallback_actions is None:
            fallback_actions = [self.action_space.sample() for _ in range(K + 1)]
        fbh = np.full((K + 1, W), -1, dtype=np.int32)
        rows = np.asarray(fallback_actions, dtype=np.int32)
        if rows.size % S or rows.size < (K + 1) * S:
            raise ValueError("run_agent_sensors: fallback_actions must be [K + 1, S] = [%d, %d] (one row per decision and one to spare; "
                             "longer is fine), got shape %s" % (K + 1, S, rows.shape))
        fbh[:, :S] = rows.reshape(-1, S)[:K + 1]
        fb = torch.as_tensor(fbh).to(e.dev)                                      # (uploaded once)
        log = torch.full((K + 1, W), -1, dtype=torch.int32, device=e.dev)        # log[k] = the sensors' objects at step i0 + k + 1
        actions, rewards, dones = [], [], []
        pos, done = 0, False
        while pos < K and not done:
            kk = min(K - pos, e.H - 1)     # (every step of a chunk stays resident: the one that turns out to be the last is returned)
            i0 = self.i
            for k in range(kk):
                i = i0 + k + 1
                look = e.launch_lookahead_sensors((i - 1) % e.H, i, sites)
                e.launch_assign_sensors(look, column, log[pos + k], fallback_row=fb[pos + k], rule=rule)
                e.launch_rollout_sensors((i - 1) % e.H, i, sites, log[pos + k:pos + k + 1], argmax_spos=shaped)
            stats, upd = self._ring_chunk(i0, kk, e.upd_sensors if S > 1 else e.upd_sensors[:, 0])
            acts = log[pos:pos + kk, :S].cpu().numpy()
            done = self._book_steps(acts if S > 1 else acts[:, 0], stats, upd, i0 + kk, (actions, rewards, dones))
            pos += kk
        return (self._obs_out(refresh_aer_dev=True), np.asarray(actions, dtype=int).reshape(len(actions), S), np.asarray(rewards),
                np.asarray(dones, dtype=bool))

    # ------------------------------------------------------------------ failures (:369-382)
    def _record_failures(self, at_step=None):
        """filter_error() bookkeeping (:369-382) for the filters that failed in step self.i (at_step: the step being booked after a rollout
        / closed-loop / policy launch that ran several).  The KERNEL wrote the records -- object, status code, step, error_failed() of the
        state it failed from -- into host-mapped memory (ssa_step_params.fail_log) as the filters failed: nothing is copied here.  The
        reference loses 2-3 % of its filters over an episode (and so does this env's default, the behaviour-faithful variant): a few per
        step late in an episode."""
        s = time.time()
        e = self._engine
        step = self.i if at_step is None else at_step
        total = int(self._stats[_lib.STAT_N_FAILED])               # filters failed by the END of `step`
        # records appended since the last call (a multi-step launch appends in the order its wavefronts reach the failures, not by step)
        n_dev = max(total, self._fail_read) if at_step is None else self._fail_chunk_total
        while self._fail_read < n_dev:
            r = e.fail_log[self._fail_read]
            if r[_lib.FAIL_TIME] == 0.0:         # (not written: a status word set from outside the kernels is counted in the statistics but has no record)
                break
            self._fail_pending.setdefault(int(r[_lib.FAIL_TIME]), []).append(r.copy())
            self._fail_read += 1
        for t in sorted(k for k in self._fail_pending if k <= step):
            for r in self._fail_pending.pop(t):
                j = int(r[_lib.FAIL_OBJ])
                self.failed_filters_msg.record(j, t, int(r[_lib.FAIL_STATUS]), r[_lib.FAIL_ERR:_lib.FAIL_ERR + 4])
                self.failed_filters_id.append(j)
        self._n_failed = len(self.failed_filters_id)
        self.runtime['filter_error'] += time.time() - s

    def _latest_resident(self):
        """the newest step the device history holds (a rollout / closed-loop launch has advanced the rings beyond self.i while the
        host is still booking its steps one by one)"""
        return self.i if self._ring_head is None else self._ring_head

    def anees(self):
        """:436-446 -- average normalised estimation error squared over the episode so far: NEES on the device for every
        resident (step, object) of the history (the reference loops n * m numpy inversions); fills self.nees (n, m)."""
        self._caller_order()
        from .. import device
        s = time.time()
        e = self._engine
        self.nees = np.full((self.n, self.m), np.nan)
        lo = max(0, self.i - e.H + 1)
        for i in range(lo, self.i + 1):
            sl = i % e.H
            self.nees[i] = device.nees(e.x_true[sl], e.x_filter[sl], e.P_filter[sl]).cpu().numpy()
        self.runtime['anees'] += time.time() - s
        return float(np.mean(self.nees[lo:self.i + 1]))

    def nis(self):
        """normalised innovation squared of every update taken so far (fitness_test(), :750-754); NaN where no update ran.  A sensor
        network: (n, S), one value per (step, sensor) update"""
        import torch
        from .. import device
        out = np.full(self.obs_taken.shape, np.nan)     # ((n, S) for a sensor network: every (step, sensor) update)
        k = np.nonzero(self.obs_taken[:self.i + 1])
        if len(k[0]):
            out[k] = device.nis(torch.as_tensor(self._y[k]).to("cuda"), torch.as_tensor(self._S_sel[k]).to("cuda")).cpu().numpy()
        return out

    # two-sided chi-square critical points stats.chi2.ppf([alpha / 2, 1 - alpha / 2], df) for the reference's alpha = 0.05
    # (:756, :762); other alphas need scipy -- but for df = 2 (the updates of angles-only sensors), where the quantile is closed-form
    _CHI2_95 = {3: (0.21579528262389788, 9.348403604496145), 6: (1.2373442457912032, 14.449375335447922)}

    @classmethod
    def _chi2_points(cls, alpha, df):
        if df == 2:      # (chi2(2) is exponential with mean 2: ppf(q) = -2 ln(1 - q))
            return -2.0 * math.log(1.0 - alpha / 2), -2.0 * math.log(alpha / 2)
        if abs(alpha - 0.05) < 1e-15 and df in cls._CHI2_95:
            return cls._CHI2_95[df]
        from scipy import stats
        lo, hi = stats.chi2.ppf([alpha / 2, 1 - alpha / 2], df=df)
        return float(lo), float(hi)

    def fitness_chi2(self, alpha=0.05):
        """Tests 2 and 4 of fitness_test() (:750-775): the percentage of normalised innovations squared (NaN dropped, :757)
        and of normalised estimation errors squared (NaN kept in the mean, :771) inside the two-sided (1 - alpha) chi-square
        interval, counted ON THE DEVICE (ssa_nis_f64 / ssa_nees_f64 + ssa_chi2_contained_f64) over the steps simulated so
        far that are still resident.  The reference's Test 4 covers the WHOLE episode (its history arrays hold every step): build the
        env with config['history'] = 'full' for that -- with a short ring (history = 2, what 'auto' picks for very large envs) the NEES
        window is the last `history` steps only, and 'nees_steps' in the result says how many it was.  A sensor network: the updates
        of 'ae' sensors (config['sensor_measurement']) are counted against the 2-dof interval, the others against the 3-dof one, pooled.
        Returns {'Test 2: NIS chi2': pct, 'Test 4: NEES chi2': pct, counts...}."""
        self._caller_order()
        import torch
        from .. import device
        e = self._engine
        out = {}
        k = np.nonzero(self.obs_taken[:self.i + 1])      # (a sensor network: every (step, sensor) update, pooled)
        inside, valid = 0, 0
        if len(k[0]):
            nis = device.nis(torch.as_tensor(self._y[k]).to("cuda"), torch.as_tensor(self._S_sel[k]).to("cuda"))
            if self.sensor_angles_only.any():      # (k[1]: the update's sensor; each kind against the interval of its own dimension)
                ang = torch.as_tensor(self.sensor_angles_only[k[1]]).to("cuda")
                parts = ((nis[~ang], 3), (nis[ang], 2))
            else:
                parts = ((nis, 3),)
            for v, df in parts:
                if v.numel():
                    lo, hi = self._chi2_points(alpha, df)
                    a, b = device.chi2_contained(v.contiguous(), lo, hi)
                    inside, valid = inside + a, valid + b
        out['Test 2: NIS chi2'] = round(100.0 * inside / valid, 2) if valid else float('nan')
        out['nis_inside'], out['nis_valid'] = inside, valid
        first = max(0, self.i - e.H + 1)
        slots = [i % e.H for i in range(first, self.i + 1)]
        if slots == list(range(slots[0], slots[0] + len(slots))):     # contiguous in the history tensors: no gather
            sl = slice(slots[0], slots[0] + len(slots))
            xt, x, P = e.x_true[sl], e.x_filter[sl], e.P_filter[sl]
        else:
            xt, x, P = e.x_true[slots], e.x_filter[slots], e.P_filter[slots]
        nees = device.nees(xt.reshape(-1, 6), x.reshape(-1, 6), P.reshape(-1, 6, 6))
        lo, hi = self._chi2_points(alpha, 6)
        inside, _ = device.chi2_contained(nees, lo, hi)
        out['Test 4: NEES chi2'] = round(100.0 * inside / nees.numel(), 2)
        out['nees_inside'], out['nees_total'], out['nees_steps'] = inside, int(nees.numel()), len(slots)
        return out

    def failed_filters(self):
        if not self.failed_filters_id:
            print("No failed Objects")
        else:
            print("Failed Objects: ", self.failed_filters_id)
            for rso_id in self.failed_filters_id:
                print(self.failed_filters_msg[rso_id])

    # ------------------------------------------------------------------ visibility (:410-434)
    def _mask(self, sensor=0):
        from .. import device
        if not 0 <= int(sensor) < self.n_sensor:
            raise ValueError("sensor %r: the env has %d sensor(s)" % (sensor, self.n_sensor))
        self._caller_order()
        e = self._engine
        row = self.i % e.n_time
        M = e.trans[row].reshape(3, 3)
        if self.sensor_moving[int(sensor)]:           # (a space-based sensor: line of sight instead of an elevation mask, and no night)
            mask = device.los_mask(e.x_true[self.i % e.H], e.trans[row], e.site_rows[row, int(sensor)], self.limb_radius)
        else:
            mask = device.visible_mask(e.x_true[self.i % e.H], M, self._sensor_consts[int(sensor)])
        if self.sensor_sunlit_only[int(sensor)]:      # (the sensor kernels' rule at this time row, so that the helpers agree with step())
            if self.sensor_moving[int(sensor)] or (int(self.sun_dark[row]) >> int(sensor)) & 1:
                mask = mask & device.sunlit_mask(e.x_true[self.i % e.H], e.sun[row], self.shadow_radius)
            else:
                mask = mask & 0
        return mask.cpu().numpy().astype(bool)

    # (sensor=: a sensor network's site s; default the primary sensor, the only one without config['observers'])
    def visible_objects(self, sensor=0):
        s = time.time()
        viz = np.where(self._mask(sensor))[0]
        self.runtime['visible_objects'] += time.time() - s
        return viz

    def object_visible(self, RSO_ID=[], sensor=0):
        if len(RSO_ID) == 0:
            print('RSO ID expected, but not supplied')
            return RSO_ID
        return self._mask(sensor)[np.asarray(RSO_ID)]

    def object_visibility(self, sensor=0):
        s = time.time()
        viz = self._mask(sensor)
        self.runtime['object_visibility'] += time.time() - s
        return viz

    def agent_scores(self):
        """device tensors (scores[4, m], mask[m]) for the heuristic agents (ssa_gym_amd.agents)."""
        from .. import device
        self._caller_order()
        e = self._engine
        cur, prev = self.i % e.H, (self.i - 1) % e.H
        M = e.trans[self.i % e.n_time].reshape(3, 3)
        P_prev = e.P_filter[prev] if self.i >= 1 else None
        return device.agent_scores(e.x_true[cur], e.x_filter[cur], e.P_filter[cur], P_prev, M, self._consts)

    def _lookahead_parts(self, what, covariances):
        """the guards of lookahead() and lookahead_sensors(); the covariance parts to ask the launch for"""
        from .. import engine as _engine
        if self._engine is None:
            raise _lib.SsaHipError("no device state: the lookahead runs on the GPU only (no CPU fallback)")
        if self.i + 1 >= self.n:
            raise ValueError("%s: the episode has no next step (i = %d, steps = %d)" % (what, self.i, self.n))
        return _engine.HotPathEngine.LOOKAHEAD_PARTS if covariances else ()

    def lookahead(self, covariances=False):
        """One-step tasking lookahead (no reference counterpart; include/ssa_hip.h: ssa_lookahead_f64): for EVERY object j, what step(j)
        would produce for j at the next step, from the current state and in ONE launch -- nothing of the env changes, and nothing
        returned depends on the measurement noise still to be drawn.  A dict of CUDA tensors, objects in the env's own order:
            score   [3, m]  float64: rows _lib.LOOK_TRACE_GAIN (tr P- - tr P+), LOOK_POS_TRACE_GAIN (position block), LOOK_INFO_GAIN
                            (1/2 ln(det P- / det P+)); NaN unless status == OK and visible
            visible [m]     uint8: the update's visibility test at the next step (0 where the update would not be attempted)
            status  [m]     int32: the SSA_ST_* code step(j) would leave on j (a NaN update, which depends on the noise, is not foreseen)
        and with covariances=True also x_prior [m, 6], P_prior [m, 6, 6] (the prediction every object gets) and P_post [m, 6, 6] (P_filter
        of the next step after step(j)).  The tensors are the env's lookahead buffers: the next call overwrites them."""
        self._single_sensor('lookahead')
        e, want = self._engine, self._lookahead_parts('lookahead', covariances)
        return lookahead_result(e.launch_lookahead(self.i % e.H, self.i + 1, out=want, stream=self._stream.cuda_stream), want)

    def lookahead_sensors(self, covariances=False):
        """The lookahead of every sensor of the network (no reference counterpart; include/ssa_hip.h: ssa_lookahead_sensors_f64; DESIGN.md
        section 8d): for every sensor s and object j, what step() would produce for j at the next step if s were tasked to j and no other
        sensor were -- lookahead() from sensor s's site, with its elevation mask and R -- in ONE launch that predicts every object once.
        Nothing of the env changes.  A dict of CUDA tensors, objects in the env's own order, S = n_sensor (1 without config['observers']:
        the env's own observer):
            score   [S, 3, m]  float64: rows as lookahead()'s score (_lib.LOOK_*); NaN unless status == OK and visible from s
            visible [S, m]     uint8: the update's visibility test from site s at the next step
            status  [S, m]     int32: the SSA_ST_* code the step would leave on j (a singular S is per sensor)
        and with covariances=True also x_prior [m, 6], P_prior [m, 6, 6] (the prediction, the same for every sensor) and P_post
        [S, m, 6, 6].  The tensors are the env's buffers: the next call overwrites them."""
        e, want = self._engine, self._lookahead_parts('lookahead_sensors', covariances)
        return lookahead_result(e.launch_lookahead_sensors(self.i % e.H, self.i + 1, self._sites(), out=want, stream=self._stream.cuda_stream), want)

    def forecast_sensors(self, horizon, covariances=False):
        """The H-step tasking forecast of the network (no reference counterpart; include/ssa_hip.h: ssa_forecast_sensors_f64; DESIGN.md
        section 8h): from the state at step i, what lookahead_sensors() would return at each of the steps i+1 .. i+H' -- H' =
        min(horizon, steps - 1 - i) -- if every sensor stayed idle until then: when each object passes over each site, how far its
        covariance has grown by then, and what an observation from that site at that step would gain.  ONE launch, and nothing of the
        env changes: an env can be asked about its future without spending it.  A dict of CUDA tensors, objects in the env's own order,
        S = n_sensor (1 without config['observers']: the env's own observer as a one-site network):
            score   [H', S, m, 3]  float64: columns _lib.LOOK_*; NaN unless status == OK and visible from s at that step
            visible [H', S, m]     uint8
            status  [H', S, m]     int32
        and with covariances=True also x_prior [H', m, 6], P_prior [H', m, 6, 6] and P_post [H', S, m, 6, 6].  Slab h assumes no update
        before step i+1+h.  Memory: the scores are 24 * H' * S * m bytes (3.8 MB at 20 000 objects, 8 steps, one site), P_post twelve
        times that.  The tensors are the env's buffers: the next call overwrites them."""
        e, want = self._engine, self._lookahead_parts('forecast_sensors', covariances)
        H = min(int(horizon), self.n - 1 - self.i)
        if H < 1:
            raise ValueError("forecast_sensors: a horizon of at least one step, got %r" % (horizon,))
        return dict(e.launch_forecast_sensors(self.i % e.H, self.i + 1, self._sites(), H, out=want, stream=self._stream.cuda_stream))

    _access_anchor = None      # (step index at which the pass table the engine holds was made, its steps; None: none since the last reset())

    def access_sensors(self, horizon=None):
        """The pass table of the network (no reference counterpart; include/ssa_hip.h: ssa_access_sensors_f64):
        for each of the steps i+1 .. i+T -- T = min(horizon, steps - 1 - i), the whole rest of the episode by default -- which sensor
        sees which object, by the visibility rule step() applies (elevation mask, dark site, Earth shadow, line of sight from orbit).
        The truth does not depend on actions, noise or filters, so this is what step() WILL find, whatever is done until then; ONE
        launch, no filter arithmetic, and nothing of the env changes.  A dict, objects in the env's own order, S = n_sensor (1 without
        config['observers']: the env's own observer as a one-site network):
            bits    [S, m, W] int64 CUDA, W = ceil(T / 64): bit h mod 64 of word h div 64 = step i + 1 + h (device.access_mask(bits, h),
                    device.access_unpack(bits, T))
            first, length, count, passes  [S, m] int32 CUDA: the first step seen (h; -1: never), the length of that first pass, the
                    steps seen, the passes
            n_steps T
        A failed filter is NOT masked out (the table knows no filter): AND with the status where that is wanted --
        lookahead_sensors()['visible'] == the mask AND (the update would be attempted).  The tensors are the engine's: the next call
        overwrites them, and action_masks() reads them from now on."""
        if self._engine is None:
            raise _lib.SsaHipError("no device state: the pass table is made on the GPU only (no CPU fallback)")
        T = self.n - 1 - self.i if horizon is None else min(int(horizon), self.n - 1 - self.i)
        if T < 1:
            raise ValueError("access_sensors: at least one step inside the episode (i = %d, steps = %d, horizon = %r)" % (self.i, self.n, horizon))
        e = self._engine
        r = e.launch_access_sensors(self.i % e.H, self.i + 1, self._sites(), T, stream=self._stream.cuda_stream)
        self._access_anchor = (self.i, T)
        p = r["pass"][0]
        return {"bits": r["bits"][0], "first": p[..., _lib.PASS_FIRST], "length": p[..., _lib.PASS_LENGTH], "count": p[..., _lib.PASS_COUNT],
                "passes": p[..., _lib.PASS_PASSES], "n_steps": T}

    def action_masks(self):
        """The action mask of the NEXT step: bool [S, m] on the device, True where sensor s will see object j at step i + 1 -- what
        lookahead_sensors()['visible'] reports for every filter that has not failed, without the lookahead's UKF updates.  The pass
        table is made by the first call after a reset() (access_sensors(): one launch over the rest of the episode); every later call
        is one shift-and-mask of it (device.access_mask) and launches no kernel of the library.  It stays valid across step(),
        rollout*(), run_agent*() and run_policy(): the truth does not depend on them.  A failed filter is not masked out: AND with the
        status where wanted."""
        from .. import device
        if self.i + 1 >= self.n:
            raise ValueError("action_masks: the episode has no next step (i = %d, steps = %d)" % (self.i, self.n))
        a = self._access_anchor
        if a is None or not (0 <= self.i - a[0] < a[1]):
            self.access_sensors()
            a = self._access_anchor
        return device.access_mask(self._engine._access["bits"][0], self.i - a[0])

    def evaluate_schedules(self, actions, gather=True):
        """The dry run of B candidate tasking schedules (no reference counterpart; include/ssa_hip.h: ssa_dryrun_sensors_envs_f64;
        DESIGN.md section 8p): what each schedule would be worth if rollout_sensors() ran it from the state at step i, in ONE launch and
        without spending the env.  The covariance update does not depend on the measurement drawn and the expected innovation is zero,
        so a schedule is run with P+ = P- - K S K^T committed and x+ = x-: deterministic, read-only, and -- unlike forecast_sensors() --
        a revisit is valued from the covariance the earlier visit left.  `actions`: integers [K, S] or [B, K, S] (S = n_sensor; 1 without
        config['observers']: the env's own observer as a one-site network), K clipped to steps - 1 - i; an entry < 0 or >= m is an idle
        sensor; two sensors on one object in a row are NOT refused -- the lower one takes it and the record shows who did.  A dict of
        CUDA tensors, B = 1 for [K, S]:
            score   [B, K', S, 3] float64: columns _lib.LOOK_* from the step's P- and P+; NaN unless taken
            taken, visible [B, K', S] bool;  status [B, K', S] int32 (the SSA_ST_* the object carries after the step; 0: nobody updated)
            action  [B, K', S] int64: the object whose update was attempted, else -1
            total   [B, 3] float64: the sum of the taken slots' scores per column, in slot order (k outer, s inner); 0 for none
        Nothing of the env changes: no engine tensor, not i, the histories or np_random.  Only the objects a candidate names are run
        (gather=False, B == 1: the whole catalogue on the slot itself -- the cost of a rollout; the tests' yardstick)."""
        if self._engine is None:
            raise _lib.SsaHipError("no device state: the dry run of a schedule runs on the GPU only (no CPU fallback)")
        a = check_schedules(actions, self.n_sensor)
        K = min(int(a.shape[1]), self.n - 1 - self.i)
        if K < 1:
            raise ValueError("evaluate_schedules: at least one step inside the episode (i = %d, steps = %d, K = %d)" % (self.i, self.n, a.shape[1]))
        e = self._engine
        rec = e.launch_dryrun_sensors(self.i % e.H, self.i + 1, self._sites(), a[:, :K], stream=self._stream, gather=gather)
        return schedules_result(rec, self._stream)

    # ---- what agents.py asks of an env beside its public queries (SSA_Tasker_VecEnv answers the same for its E
    # envs): the planners' arrays carry a leading env axis, this env being the batch of one
    def assign_sensors(self, column, rule='greedy'):
        """the network's lookahead and its assignment over score column `column` (_lib.LOOK_*) by `rule` ('greedy', or 'optimal': most
        sensors tasked, then the largest sum): two launches and one 32-byte read-back (SSA_Tasker_VecEnv.assign_sensors for one env).
        int64 [S]; -1: the scores left that sensor without an object.  Nothing of the env changes."""
        score = self.lookahead_sensors()["score"]              # [S, 3, m]: a view of the engine's [S][m][3] rows
        S = score.shape[0]
        row = self._engine.assign_row()
        # the rounds of the agents on the device (ssa_assign_sensors_f64; no fallback words: a sensor without an object comes back -1): one
        # launch and one 32-byte read-back where S masked arg-max launches and S read-backs were
        # (permuted back, the view IS the engine's contiguous [S][m][3] block: launch_assign_sensors refuses anything else)
        self._engine.launch_assign_sensors({"score": score.permute(0, 2, 1)}, column, row, stream=self._stream.cuda_stream, rule=rule)
        self._stream.synchronize()
        return row.cpu().numpy()[:S].astype(np.int64)

    def _tasking_stream(self):
        return self._stream                 # (the torch stream the planners' launches go in)

    def _forecast_scores(self, horizon):
        """the forecast's scores as the engine leaves them, with the env axis: [H', 1, S, m, 3] (a view; slab h is score[h])"""
        return self.forecast_sensors(horizon)["score"].unsqueeze(1)

    def _slab_assigner(self, score):
        """assign(slab [1, S, m, 3], column, row [1, MAX_SENSORS], rule): one launch in the env's stream, the engine's workspace"""
        e, stream = self._engine, self._stream.cuda_stream
        return lambda slab, column, row, rule: e.launch_assign_sensors({"score": slab[0]}, column, row[0], stream=stream, rule=rule)

    def _plan_table(self, horizon, column):
        """the forecast's launch and the horizon-wide plan's (ssa_plan_sensors_f64) on it: the engine's int32 table as [H', 1, MAX_SENSORS]"""
        return self._engine.launch_plan_sensors(self.forecast_sensors(horizon), column, stream=self._stream.cuda_stream).unsqueeze(1)

    def aer_obs(self, obs):
        """:834-840 -- [az, el, range, trace(P)] per object, NaN/inf -> 0.001."""
        from .. import device
        e = self._engine
        slot = self.i % e.H
        M = e.trans[self.i % e.n_time].reshape(3, 3)
        out = e.caller_rows(device.aer_obs(e.x_filter[slot], e.P_filter[slot], M, self._consts).view(self.m, 4)).cpu().numpy().reshape(-1)
        obs[:] = out
        return obs

    def render(self, mode='live'):
        raise NotImplementedError("rendering/plots are outside the hot-path scope (SURVEY section 2, rows 1b/6b)")
