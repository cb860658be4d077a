"""HotPathEngine: device-resident state of E environments x m objects and the per-step
launch sequence (fused step kernel + reward statistics kernel).

Data layout in HBM (all float64, the reference's own array-of-structures shapes so a
history slot is byte-identical to the reference's `x_true[i]`, `x_filter[i]`, `P_filter[i]`,
`obs[i]` numpy slices -- ssa_tasker_simple_2.py:132-161):

    x_true  [H][E*m][6]        x_filter [H][E*m][6]       P_filter [H][E*m][6][6]
    obs     [H][E*m][12]       metrics  [H][E][4][m]      stats    [H][E][8]
    upd     [H][E][64]         status   [E*m] int32

H is the history depth: the reference keeps the whole episode (H = n steps); with 288 GB of
HBM that is affordable up to hundreds of thousands of objects, and the step kernel then
reads slot i-1 and writes slot i with no copy.  H = 2 is the ping-pong minimum (what
agents.py needs: P_filter[i] and P_filter[i-1]).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, device, host

f64 = torch.float64


class _Snapshot(tuple):
    """a snapshot's tensors + the storage layout (`order`) they were taken under"""
    order = None


def _dev_tensor(t, dtype, n=None, at_least=False):
    """is `t` what device._chk takes -- a contiguous CUDA tensor of `dtype` -- with n elements (at_least: n or more; None: any number)?"""
    try:
        device._chk(t, "", dtype)
    except _lib.SsaHipError:
        return False
    return n is None or (t.numel() >= n if at_least else t.numel() == n)


def _tensor_args(what, args, at_least=False):
    """the tensor arguments of launch `what`: every (tensor, dtype, n, name) of `args` that is not None must pass _dev_tensor"""
    for t, dt, n, nm in args:
        if t is not None and not _dev_tensor(t, dt, n, at_least):
            raise _lib.SsaHipError("%s: %s must be a contiguous CUDA %s tensor of %s%d elements" % (what, nm, dt, ">= " if at_least else "", n))


def _in_stream(stream):
    """the context in which torch's own ops go to `stream` (as device._stream takes it; None: no change), for the launches that run some
    next to the library's kernels: the dry runs' upload and gather"""
    return torch.cuda.stream(stream if stream is None or isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(stream))


def _dry_target(p, g, ids):
    """a _lookahead_params block `p` re-targeted at the gathered block of a dry run: g = (x_true, x_filter, P_filter, status, time words)
    of ids.shape[0] pseudo-envs of ids.shape[1] rows each, `ids` [n, W] the caller's object of every row (-1: padding)"""
    p.n_env, p.n_obj = ids.shape
    p.x_true_in, p.x_in, p.P_in, p.status, p.env_time = (t.data_ptr() for t in g)
    p.obj_ids = ids.data_ptr()


class HotPathEngine:
    site_rows, _site_moving, limb_radius = None, 0, 0.0      # (until set_site_table: no sensor moves)

    def __init__(self, consts, n_obj, n_env, trans, z_noise, history, device_name="cuda",
                 zn_stride_env=None, zn_stride_time=None, zn_stride_obj=3):
        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.SsaHipError("no GPU visible: the ssa-gym hot path runs on MI355X only (no CPU fallback)")
        self.consts = consts
        self.m, self.E, self.H = int(n_obj), int(n_env), int(history)
        if self.H < 2:
            raise ValueError("history depth must be >= 2")
        self.dev = torch.device(device_name)
        N = self.m * self.E
        d = self.dev
        self.x_true = torch.zeros((self.H, N, 6), dtype=f64, device=d)
        self.x_filter = torch.zeros((self.H, N, 6), dtype=f64, device=d)
        self.P_filter = torch.zeros((self.H, N, 6, 6), dtype=f64, device=d)
        self.obs = torch.zeros((self.H, N, 12), dtype=f64, device=d)
        self.metrics = torch.full((self.H, self.E, 4, self.m), float("nan"), dtype=f64, device=d)
        self.stats = torch.zeros((self.H, self.E, _lib.STAT_STRIDE), dtype=f64, device=d)
        self.upd = torch.zeros((self.H, self.E, _lib.UPD_STRIDE), dtype=f64, device=d)
        self.status = torch.zeros(N, dtype=torch.int32, device=d)
        self.trans = device.as_dev(np.asarray(trans, dtype=np.float64).reshape(-1, 9), d)
        self.n_time = self.trans.shape[0]
        self.sun = None      # set_sun_table: the [n_time, 4] rows (sx, sy, sz, the sites' dark word) of ssa_sensor_params.sun, next to `trans`
        self.z_noise = z_noise if isinstance(z_noise, torch.Tensor) else device.as_dev(z_noise, d)
        # default strides for z_noise[E][n_time][m][3]
        self.zn_stride_time = self.m * 3 if zn_stride_time is None else int(zn_stride_time)
        self.zn_stride_env = self.n_time * self.m * 3 if zn_stride_env is None else int(zn_stride_env)
        # per-env time origin and action words: two views of ONE device buffer, so that a caller that refreshes both every step
        # (the vector env) needs a single host-to-device copy
        self.time_actions = torch.zeros(2 * self.E, dtype=torch.int32, device=d)
        self.time_actions[self.E:] = -1
        self.env_time0 = self.time_actions[:self.E]
        self.actions = self.time_actions[self.E:]
        self._p = _lib.ssa_step_params()
        self._p.n_obj, self._p.n_env = self.m, self.E
        self._p.status = self.status.data_ptr()
        self._p.trans = self.trans.data_ptr()
        self._p.env_time = self.env_time0.data_ptr()
        # the kernel indexes z_noise[e*stride_env + (i % n_time)*stride_time + a*stride_obj + 0..2]: check the extent here
        need = (self.E - 1) * self.zn_stride_env + (self.n_time - 1) * self.zn_stride_time + (self.m - 1) * int(zn_stride_obj) + 3
        if min(self.zn_stride_env, self.zn_stride_time, int(zn_stride_obj)) < 0 or self.z_noise.numel() < need \
                or self.z_noise.dtype != torch.float64 or not self.z_noise.is_contiguous():
            raise _lib.SsaHipError("z_noise: %d contiguous float64 values needed for (n_env=%d, n_time=%d, n_obj=%d) with strides "
                                   "(%d, %d, %d), got %s of %d" % (need, self.E, self.n_time, self.m, self.zn_stride_env,
                                                                   self.zn_stride_time, int(zn_stride_obj), self.z_noise.dtype,
                                                                   self.z_noise.numel()))
        self._p.z_noise = self.z_noise.data_ptr()
        self._p.zn_stride_env, self._p.zn_stride_time = self.zn_stride_env, self.zn_stride_time
        self._p.zn_stride_obj = int(zn_stride_obj)
        self._p.n_time = self.n_time
        self._stats_ws = device.stats_workspace(self.E, d)
        self.work = torch.zeros(self._lib.ssa_env_step_work_bytes(self.m, self.E) // 4, dtype=torch.int32, device=d)
        self._p.work, self._p.stat_ws, self._p.launch_mask = self.work.data_ptr(), self._stats_ws.data_ptr(), 0
        # filter_error()'s records written by the kernels themselves into host-mapped pinned memory (ssa_step_params.fail_log): one record
        # per filter that fails, capacity = every filter once per episode; the counter is a device word, zeroed with the episode
        self.fail_log_host = torch.zeros((N, _lib.FAIL_STRIDE), dtype=f64).pin_memory()
        self.fail_log = self.fail_log_host.numpy()
        self.fail_count = torch.zeros(1, dtype=torch.int32, device=d)
        self._p.fail_log, self._p.fail_count, self._p.fail_cap = self.fail_log_host.data_ptr(), self.fail_count.data_ptr(), N
        # statistics accumulators of the atomics path; two sets, alternated when the fold is deferred
        self._shard_sets = torch.zeros((2, self.E, _lib.STAT_SHARDS, _lib.STAT_SHARD_WORDS), dtype=torch.int64, device=d)
        self.stat_shards = self._shard_sets[0]
        self._shard_cur = 0
        self.force_generic = False     # set: every launch_step carries SSA_LAUNCH_GENERIC (the generic step kernel; tests and A/B runs)
        self._fold_pending = None      # (shard set index, stats destination, arg-max slots?, metrics block or 0) of a step whose fold was deferred
        # SSA_LAUNCH_STATS_FROM_METRICS: a deferred step of ONE env (one tile per wavefront) leaves max delta_pos and the trinary counts
        # to service wavefronts of the next launch, which reduce them from the metrics rows it stored (0: the path does not apply)
        self.stats_from_metrics = int(self._lib.ssa_stats_from_metrics_waves(self.m, self.E)) > 0
        self._shard_ptr = [self._shard_sets[0].data_ptr(), self._shard_sets[1].data_ptr()]
        # arg-max slots of sigma_pos (ssa_step_params.spos_tiles: the 'shaped' reward on the one-launch paths), one set per shard set;
        # the step kernel needs whole tiles per env for them
        self.ntiles = (N + 3) // 4
        self.supports_argmax = self.E == 1 or self.m % 4 == 0
        self._spos_sets = None
        self._actions_ptr = self.actions.data_ptr()
        self._order = None             # storage layout (set_layout): position -> the caller's index, or None
        # allocated by the first launch that needs them:
        self._roll_shards = self._roll_spos = None      # per-step shard sets and arg-max slots of a rollout (_rollout_params)
        self._roll_sched = self.upd_sensors = None      # launch_rollout_sensors: its schedule (kept until the next launch), its record ring
        self._roll_envs_out = None      # launch_rollout_sensors_envs: its per-step statistics and records (grown as _roll_shards is)
        self._loop_ws = self._agent_ws = None           # workspaces of launch_closed_loop (with loop_error) and launch_agent_select
        self._look = self._look_s = None                # output buffers of launch_lookahead / launch_lookahead_sensors
        self._fore = None                               # ... and of launch_forecast_sensors
        self._assign_ws = None                          # (S, workspace) of launch_assign_sensors
        self._assign_row = None                         # assign_row()'s
        self._plan = None                               # (shape, table, workspace) of launch_plan_sensors
        self._sensor_envs = None                        # launch_step_sensors_envs: its block, the [E][8] action table and its staging
        self._look_se = None                            # output buffers of launch_lookahead_sensors_envs
        self._assign_envs_ws = None                     # (S, workspace) of launch_assign_sensors_envs
        self._fore_e = None                             # output buffers of launch_forecast_sensors_envs
        self._access = None                             # ... and of launch_access_sensors: the pass table and its summary
        self._dry = {}                                  # launch_dryrun_sensors: per (B, K, S, W) its upload, gathered block and records
        self._dry_envs = {}                             # launch_dryrun_sensors_envs: per (E * B, K, S, W) its upload, gathered block and records
        self._pcache = {}
        self._cref = C.byref(self.consts)
        self._pref = C.byref(self._p)
        # element strides of one history slot
        self._sx, self._sP, self._so = N * 6 * 8, N * 36 * 8, N * 12 * 8
        self._sm, self._ss, self._su = self.E * 4 * self.m * 8, self.E * _lib.STAT_STRIDE * 8, self.E * _lib.UPD_STRIDE * 8
        self._bx_t, self._bx, self._bP = self.x_true.data_ptr(), self.x_filter.data_ptr(), self.P_filter.data_ptr()
        self._bo, self._bm, self._bs, self._bu = (self.obs.data_ptr(), self.metrics.data_ptr(), self.stats.data_ptr(),
                                                  self.upd.data_ptr())

    # ------------------------------------------------------------------ layout (ssa_step_params.obj_ids)
    def set_layout(self, order):
        """Store the objects in another order than the caller numbers them: position i of every state tensor holds the object the
        caller calls order[i]; None: the caller's order.  Objects of one orbit regime then share wavefronts (catalogue.regime_order) --
        late in an episode the diverged filters are the LEO objects, and packed they cost a launch 10 % less.
        The per-step launches speak the caller's indices wherever an index enters or leaves (actions, failure records, arg-max of sigma_pos,
        the host-facing observation rows: include/ssa_hip.h); the state tensors of this engine (x_true, x_filter, P_filter, obs, metrics,
        status) are in STORAGE order while a layout is set -- `to_caller_order()` puts them back (the rollout and closed-loop launches keep the
        layout).  Call before load_state(); the state present is not moved.
        Several envs (the per-step launch only): `order` is [n_env][n_obj], one permutation per env (indices within the env, as the actions
        are), n_obj % 4 == 0; `set_env_layout(e, order)` replaces one env's row (a vector env's auto-reset)."""
        if order is None and self._order is None:
            return
        if order is not None:       # (checked before anything changes: a refused table leaves the layout in force as it was)
            order = np.asarray(order, dtype=np.int64)
            if self.E == 1:
                order = order.reshape(-1)
            if order.shape != ((self.m,) if self.E == 1 else (self.E, self.m)) or \
                    not np.array_equal(np.sort(order.reshape(self.E, self.m), axis=1), np.broadcast_to(np.arange(self.m), (self.E, self.m))):
                raise _lib.SsaHipError("set_layout: `order` must be a permutation of 0 .. n_obj - 1 (one per env)")
            self._whole_tiles("a storage layout with")
        self._order = None
        self._p.obj_ids = 0
        self._pcache.clear()
        if order is None:
            return
        self._order = order.copy()
        self._obj_ids = torch.full((4 * self.ntiles,), -1, dtype=torch.int32, device=self.dev)   # (whole tiles: the kernel reads a tile's four words at once)
        self._p.obj_ids = self._obj_ids.data_ptr()
        self._upload_layout()

    def _upload_layout(self):
        """the device tables of self._order (in place: the launch parameter blocks keep their pointers)"""
        N = self.m * self.E
        rows = (self._order.reshape(self.E, self.m) + (np.arange(self.E, dtype=np.int64) * self.m)[:, None]).reshape(-1)
        self._obj_ids[:N].copy_(torch.as_tensor(self._order.reshape(-1).astype(np.int32)))
        self._order_idx = torch.as_tensor(rows).to(self.dev)                      # storage position -> the caller's row
        self._slot_of = torch.as_tensor(np.argsort(rows)).to(self.dev)            # the caller's row -> storage position
        self._slot_of32 = self._slot_of.to(torch.int32)                           # (the closed loop's inverse table: ssa_closed_loop_params.slot_of)

    def set_env_layout(self, e, order):
        """one env's row of a several-env layout replaced (before load_env_state of that env: the state present is not moved)"""
        if self._order is None or self.E == 1:
            raise _lib.SsaHipError("set_env_layout: set_layout([n_env][n_obj]) first")
        order = np.asarray(order, dtype=np.int64).reshape(-1)
        if order.shape[0] != self.m or not np.array_equal(np.sort(order), np.arange(self.m)):
            raise _lib.SsaHipError("set_env_layout: `order` must be a permutation of 0 .. n_obj - 1")
        self._order[e] = order
        self._upload_layout()

    def _reorder(self, idx, slots):
        """every per-object tensor of the given history slots gathered through `idx` (new[i] = old[idx[i]], rows of all envs), and the status words"""
        N = self.m * self.E
        for sl in slots:
            for tns in (self.x_true, self.x_filter, self.P_filter, self.obs):
                tns[sl].copy_(tns[sl].index_select(0, idx))
            mt = self.metrics[sl].reshape(self.E, 4, self.m).permute(1, 0, 2).reshape(4, N).index_select(1, idx)      # [E][4][m]
            self.metrics[sl].copy_(mt.reshape(4, self.E, self.m).permute(1, 0, 2).reshape(self.metrics[sl].shape))
        self.status.copy_(self.status.index_select(0, idx))

    def caller_rows(self, tensor):
        """a per-object tensor of ONE history slot ([n_obj, ...]) as the caller numbers the objects: a gather while a layout is set, the
        tensor itself otherwise (for the occasional reader that should not cost the layout: the observation a reset returns)"""
        return tensor if self._order is None else tensor.index_select(0, self._slot_of)

    def to_caller_order(self):
        """put the state tensors back into the caller's order and drop the layout (asynchronous, in the current stream): for everything that
        reads them as the caller numbers them -- a policy's views of the state, the operator entry points, inspection"""
        if self._order is None:
            return
        self.flush_stats()
        self._reorder(self._slot_of, range(self.H))
        self.set_layout(None)

    # ------------------------------------------------------------------ state in
    def load_state(self, slot, x_true, x_filter, P_filter):
        """reset(): place the initial truth / estimates / covariances in history slot `slot`
        and compute obs + metrics + stats for it (ssa_tasker_simple_2.py:228-229)."""
        N = self.m * self.E
        self.flush_stats()      # (a pending fold may read the metrics rows this slot holds)
        self.x_true[slot].copy_(device.as_dev(np.asarray(x_true).reshape(N, 6), self.dev))
        self.x_filter[slot].copy_(device.as_dev(np.asarray(x_filter).reshape(N, 6), self.dev))
        self.P_filter[slot].copy_(device.as_dev(np.asarray(P_filter).reshape(N, 6, 6), self.dev))
        self.status.zero_()
        self.fail_count.zero_()
        for e in range(self.E):
            sl = slice(e * self.m, (e + 1) * self.m)
            device.observe(self.x_true[slot, sl], self.x_filter[slot, sl], self.P_filter[slot, sl],
                           obs=self.obs[slot, sl], metrics=self.metrics[slot, e])
        device.reward_stats(self.metrics[slot], self.status, self.m, self.E, out=self.stats[slot])
        if self._order is not None:      # (statistics first, in the caller's order -- np.argmax's first maximum -- then into storage order)
            self._reorder(self._order_idx, [slot])

    def load_env_state(self, slot, e, x_true, x_filter, P_filter):
        """reset() of ONE environment of a vectorised batch: overwrite its slice of `slot`."""
        sl = slice(e * self.m, (e + 1) * self.m)
        self.x_true[slot, sl].copy_(device.as_dev(np.asarray(x_true).reshape(self.m, 6), self.dev))
        self.x_filter[slot, sl].copy_(device.as_dev(np.asarray(x_filter).reshape(self.m, 6), self.dev))
        self.P_filter[slot, sl].copy_(device.as_dev(np.ascontiguousarray(np.broadcast_to(P_filter, (self.m, 6, 6))), self.dev))
        self.status[sl].zero_()
        device.observe(self.x_true[slot, sl], self.x_filter[slot, sl], self.P_filter[slot, sl],
                       obs=self.obs[slot, sl], metrics=self.metrics[slot, e])
        device.reward_stats(self.metrics[slot, e:e + 1], self.status[sl], self.m, 1, out=self.stats[slot, e:e + 1])
        if self._order is not None:      # (statistics first, in the caller's order; then the env's rows into storage order)
            idx = torch.as_tensor(self._order.reshape(self.E, self.m)[e]).to(self.dev)
            for tns in (self.x_true, self.x_filter, self.P_filter, self.obs):
                tns[slot, sl].copy_(tns[slot, sl].index_select(0, idx))
            self.metrics[slot, e].copy_(self.metrics[slot, e].reshape(4, self.m).index_select(1, idx).reshape(self.metrics[slot, e].shape))

    def env_caller_rows(self, e, tensor):
        """rows of ONE env ([n_obj, ...], storage order) as the caller numbers that env's objects"""
        if self._order is None:
            return tensor
        idx = self._slot_of[e * self.m:(e + 1) * self.m] - e * self.m
        return tensor.index_select(0, idx)

    def snapshot(self, slot):
        """device-side copy of a history slot (initial state of an episode); remembers the storage layout it was taken under."""
        snap = _Snapshot((self.x_true[slot].clone(), self.x_filter[slot].clone(), self.P_filter[slot].clone(),
                          self.obs[slot].clone(), self.metrics[slot].clone(), self.stats[slot].clone()))
        snap.order = None if self._order is None else self._order.copy()
        return snap

    def restore(self, slot, snap):
        """reset(): device-to-device restore of an episode's initial state, asynchronous (and of the layout the snapshot was taken under)."""
        order = getattr(snap, "order", None)
        if (order is None) != (self._order is None) or (order is not None and not np.array_equal(order, self._order)):
            self.flush_stats()
            self.set_layout(order)
        self.flush_stats()      # (a pending fold may read the metrics rows this slot holds)
        xt, x, P, obs, met, st = snap[:6]
        self.x_true[slot].copy_(xt)
        self.x_filter[slot].copy_(x)
        self.P_filter[slot].copy_(P)
        self.obs[slot].copy_(obs)
        self.metrics[slot].copy_(met)
        self.stats[slot].copy_(st)
        self.status.zero_()
        self.fail_count.zero_()

    def snapshot_state(self, slot):
        """a history slot AND the per-object status words: what a launch that may have to be undone (the persistent closed loop
        when it gives up) restores"""
        base = self.snapshot(slot)
        snap = _Snapshot(tuple(base) + (self.status.clone(), self.fail_count.clone()))
        snap.order = base.order
        return snap

    def restore_state(self, slot, snap):
        self.restore(slot, snap)
        self.status.copy_(snap[6])
        self.fail_count.copy_(snap[7])

    # ------------------------------------------------------------------ one step
    def _spos_ptr(self, k):
        if self._spos_sets is None:
            self._spos_sets = torch.zeros((2, self.ntiles, 2), dtype=torch.int64, device=self.dev)
        return self._spos_sets[k].data_ptr()

    def _step_params(self, slot_in, slot_out, aer_out, stats_out, upd_out, shard_set, shards_out=0, shards_clear=0, aer_cols=4, obs_mirror=0,
                     argmax=False):
        """parameter block of a step between two history slots: everything but the time index, the action pointer and the
        deferred-fold hand-over is fixed per (slot pair, outputs, shard set), so the blocks are built once and cached -- a
        step then costs a handful of field stores on the host instead of twenty"""
        key = (slot_in, slot_out, aer_out, stats_out, upd_out, shard_set, shards_out, shards_clear, aer_cols, obs_mirror, argmax)
        ent = self._pcache.get(key)
        if ent is None:
            p = _lib.ssa_step_params()
            C.memmove(C.byref(p), C.byref(self._p), C.sizeof(p))
            p.x_true_in, p.x_true_out = self._bx_t + slot_in * self._sx, self._bx_t + slot_out * self._sx
            p.x_in, p.x_out = self._bx + slot_in * self._sx, self._bx + slot_out * self._sx
            p.P_in, p.P_out = self._bP + slot_in * self._sP, self._bP + slot_out * self._sP
            p.obs = self._bo + slot_out * self._so
            p.metrics = self._bm + slot_out * self._sm
            p.upd = upd_out if upd_out else self._bu + slot_out * self._su
            p.stats = stats_out if stats_out else self._bs + slot_out * self._ss   # e.g. straight into a send buffer
            p.aer_out = aer_out
            p.stat_shards = self._shard_sets[shard_set].data_ptr() if shard_set >= 0 else 0
            p.stat_shards_prev, p.stats_prev, p.launch_mask = 0, 0, 0
            p.stat_shards_clear, p.metrics_prev = 0, 0
            p.spos_tiles = self._spos_ptr(shard_set) if (argmax and shard_set >= 0) else 0
            p.spos_tiles_prev = 0
            p.aer_cols = int(aer_cols)
            p.obs_mirror = obs_mirror
            if shards_out:      # raw-shard consumer (include/ssa_hip.h: stat_shards_clear): no fold, no `stats`
                p.stat_shards, p.stats, p.stat_shards_clear = shards_out, 0, shards_clear
            ent = (p, C.byref(p), int(p.stats or 0), int(p.metrics))
            if len(self._pcache) > 4096:
                self._pcache.clear()
            self._pcache[key] = ent
        return ent

    def launch_step(self, slot_in, slot_out, time_offset, actions_ptr=None, stream=None, aer_out=0, stats_out=0, upd_out=0,
                    fast_stats=False, defer_fold=False, profile_slot=None, shards_out=0, shards_clear=0, aer_cols=4, action=None,
                    obs_mirror=0, fold_inside=False, env_words=None, argmax_spos=False, mirror_f32=False, sensors=None, sensor_envs=None):
        """enqueue the step; asynchronous, no host sync.  fast_stats: statistics by the step kernel's atomics (two
        launches, no arg-max of sigma_pos).  defer_fold (with fast_stats): ONE launch -- this step's
        statistics are folded by extra wavefronts of the NEXT deferred step, or by flush_stats().  action (one env): the
        action by value in the parameter block (SSA_LAUNCH_INLINE_ACTION) instead of a word in memory; obs_mirror: a second
        destination of the observation rows (host-mapped pinned memory: the observation reaches the host from inside the kernel).
        env_words = (time indices, actions) of all envs (n_env <= 8) by value in the parameter block (SSA_LAUNCH_INLINE_ENVS).
        argmax_spos (with fast_stats): np.argmax / np.max of sigma_pos in the step's statistics on the one-launch paths as well
        (ssa_step_params.spos_tiles; the 'shaped' reward) -- needs self.supports_argmax.
        sensors: an ssa_sensor_params block (host.make_sensor_params, actions and record destination set): the step of a sensor network
        (ssa_env_step_sensors_f64; see launch_step_sensors) -- `action` / actions_ptr / upd_out are then not used.
        sensor_envs (with sensors): an ssa_sensor_envs_params block, the network in each of the engine's envs
        (ssa_env_step_sensors_envs_f64; see launch_step_sensors_envs)."""
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        if shards_out:
            fast_stats, defer_fold = True, False
        defer = bool(defer_fold and fast_stats)
        # (statistics from the metrics rows: the plain deferred step of one env -- every other form keeps its atomics)
        from_metrics = defer and self.stats_from_metrics and not fold_inside and sensors is None
        if self._fold_pending is not None and (not defer or bool(self._fold_pending[3]) != from_metrics):
            self.flush_stats(s)       # a deferred step is followed by an immediate one, or by one of the other form: fold it first (same stream, in order)
        argmax = bool(argmax_spos and fast_stats and not shards_out)
        if argmax and not self.supports_argmax:
            raise _lib.SsaHipError("argmax_spos on the one-launch paths needs whole tiles per env (n_env == 1 or n_obj % 4 == 0)")
        p, pref, stats_ptr, metrics_ptr = self._step_params(slot_in, slot_out, aer_out, stats_out, upd_out, self._shard_cur if fast_stats else -1,
                                               shards_out, shards_clear, aer_cols, obs_mirror, argmax)
        p.time_offset = int(time_offset)
        if sensors is not None or self._site_moving:      # (an engine without a site table -- every plain env -- pays one attribute read)
            self._set_sites(p, sensors)
        p.actions = self._actions_ptr if actions_ptr is None else actions_ptr
        inline = _lib.LAUNCH_MIRROR_F32 if mirror_f32 else 0      # (obs_mirror / aer_out are float arrays: the host-facing copy in single precision)
        if env_words is not None:
            if self.E > _lib.INLINE_ENVS:
                raise _lib.SsaHipError("env_words: at most %d envs travel in the parameter block" % _lib.INLINE_ENVS)
            p.inline_time[:self.E] = env_words[0]
            p.inline_action[:self.E] = env_words[1]
            inline |= _lib.LAUNCH_INLINE_ENVS
        elif action is not None:
            p.action0, inline = int(action), inline | _lib.LAUNCH_INLINE_ACTION
        if fold_inside and fast_stats and not defer and not shards_out:
            inline |= _lib.LAUNCH_FOLD_INSIDE      # (the step kernel's last wavefront folds the statistics: no fold launch)
        if from_metrics:
            inline |= _lib.LAUNCH_STATS_FROM_METRICS
        if self.force_generic:
            inline |= _lib.LAUNCH_GENERIC
        if defer and self._fold_pending is not None:
            p.launch_mask = _lib.LAUNCH_DEFER_FOLD | inline
            p.stat_shards_prev = self._shard_ptr[self._fold_pending[0]]
            p.stats_prev = self._fold_pending[1]
            p.spos_tiles_prev = self._spos_ptr(self._fold_pending[0]) if self._fold_pending[2] else 0
            p.metrics_prev = self._fold_pending[3]
        else:
            p.launch_mask = (_lib.LAUNCH_DEFER_FOLD if defer else 0) | inline
            p.stat_shards_prev, p.stats_prev, p.spos_tiles_prev, p.metrics_prev = 0, 0, 0, 0
        if sensors is not None:
            if profile_slot is not None:
                raise _lib.SsaHipError("profile_slot: the step of a sensor network is not profiled by event pairs")
            if sensor_envs is not None:
                rc = self._lib.ssa_env_step_sensors_envs_f64(self._cref, pref, C.byref(sensors), C.byref(sensor_envs), s)
            else:
                rc = self._lib.ssa_env_step_sensors_f64(self._cref, pref, C.byref(sensors), s)
        elif profile_slot is None:
            rc = self._lib.ssa_env_step_f64(self._cref, pref, s)
        else:   # the dominant launch bracketed by event pair `profile_slot` (read back with profile_ms)
            rc = self._lib.ssa_env_step_profiled_f64(self._cref, pref, s, int(profile_slot))
        if rc:
            raise _lib.SsaHipError("%s failed with code %d" % ("ssa_env_step_sensors_envs_f64" if sensor_envs is not None else
                                                               "ssa_env_step_sensors_f64" if sensors is not None else "ssa_env_step_f64", rc))
        if defer:
            self._fold_pending = (self._shard_cur, stats_ptr, argmax, metrics_ptr if from_metrics else 0)
            self._shard_cur ^= 1

    # ------------------------------------------------------------------ the refusals several launches share
    def _one_env(self, what):
        """`what` (a launch of the one-env entries) on an engine of several envs"""
        if self.E != 1:
            raise _lib.SsaHipError("%s covers one env (n_env == 1)" % what)

    def _whole_tiles(self, what):
        """`what` (... several envs) where an env's objects do not fill whole tiles of four: a tile would straddle two envs"""
        if self.E > 1 and self.m % 4:
            raise _lib.SsaHipError("%s several envs needs n_obj %% 4 == 0 (whole tiles per env)" % what)

    def _schedule(self, actions, lead, S):
        """an open-loop schedule as the rollout kernels read it: `actions` must be a contiguous CUDA int32 tensor [K, *lead, S] or
        [K, *lead, MAX_SENSORS] with K >= 1; returned with its rows padded to MAX_SENSORS words (-1: idle), the ABI's row stride -- one
        aligned 32-byte read per step.  S None (launch_rollout: a word per env, no sensor axis): [K, *lead], returned as it is."""
        tails = [()] if S is None else [(S,), (_lib.MAX_SENSORS,)]
        if not (_dev_tensor(actions, torch.int32) and actions.dim() >= 1 and actions.shape[0] >= 1
                and tuple(actions.shape[1:]) in [lead + t for t in tails]):
            raise _lib.SsaHipError("rollout: actions must be a contiguous CUDA int32 tensor %s"
                                   % " or ".join("[K]" + "".join("[%d]" % v for v in lead + t) for t in tails))
        if S is not None and actions.shape[-1] != _lib.MAX_SENSORS:
            actions = torch.nn.functional.pad(actions, (0, _lib.MAX_SENSORS - S), value=-1)
        return actions

    def set_sun_table(self, sun, dark, sensors=()):
        """keep the Sun table of this engine's epoch on the device (include/ssa_hip.h: ssa_sensor_params.sun): sun [n_time, 3] unit vectors
        from the geocentre to the Sun in the frame of x_true, dark [n_time] integers whose bit s says that site s is dark at that row (the
        same rows as `trans`: one epoch, one table for all envs).  Every block of `sensors` (host.make_sensor_params) is pointed at it.
        Returns the [n_time, 4] float64 device tensor (the fourth column holds the words' bits)."""
        rows = host.pack_sun_rows(sun, dark)
        if rows.shape[0] != self.n_time:
            raise _lib.SsaHipError("the Sun table has %d rows, trans has %d" % (rows.shape[0], self.n_time))
        self.sun = device.as_dev(rows, self.dev)
        if self.sun.data_ptr() % 32:
            raise _lib.SsaHipError("the Sun table's device rows are not 32-byte aligned")
        for sp in sensors:
            sp.sun = self.sun.data_ptr()
        return self.sun

    def set_site_table(self, rows, moving, limb_radius):
        """keep the site rows of this engine's moving (space-based) sensors on the device (include/ssa_hip.h: ssa_step_params.site_rows):
        rows [n_time, S, 16] as host.pack_site_rows packs them (the same time rows as `trans`: one epoch, one table for all envs), moving S
        booleans -- True where sensor s takes its site from the table and is screened by line of sight instead of an elevation mask
        (never sensor 0) --, limb_radius [m] the sphere its line of sight must clear.  From now on every ssa_step_params block this engine
        builds for a launch that takes a sensor network of S sensors carries the table; the launches without a network never do.
        moving all False (or rows None) takes the table off.  Returns the device tensor."""
        flags = [bool(k) for k in moving] if moving is not None else []
        self._pcache.clear()      # (the cached step blocks may carry the table that was)
        if rows is None or not any(flags):
            self.site_rows, self._site_moving, self.limb_radius = None, 0, 0.0
            self._set_sites(self._p, None)
            return None
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.ndim != 3 or rows.shape[0] != self.n_time or rows.shape[1] != len(flags) or rows.shape[2] != host.SITE_ROW:
            raise _lib.SsaHipError("the site table must be [%d, %d, %d] (trans rows x sensors x %d), got %s"
                                   % (self.n_time, len(flags), host.SITE_ROW, host.SITE_ROW, rows.shape))
        if flags[0] or len(flags) > _lib.MAX_SENSORS:
            raise _lib.SsaHipError("sensor 0 is the primary observer and cannot move; a network has at most %d sensors" % _lib.MAX_SENSORS)
        if not float(limb_radius) >= 0.0:
            raise _lib.SsaHipError("limb_radius must be a number >= 0, got %r" % (limb_radius,))
        dev = device.as_dev(rows, self.dev)
        if dev.data_ptr() % 128:      # (the allocator's blocks are 512-byte aligned; a view would not be)
            raise _lib.SsaHipError("the site table's device rows are not 128-byte aligned")
        self.site_rows, self.limb_radius = dev, float(limb_radius)
        self._site_moving = sum(1 << k for k, f in enumerate(flags) if f)
        return dev

    def _set_sites(self, p, sensors):
        """the moving sensors' fields of the block `p` of a launch: the engine's table for a launch that takes the network `sensors`,
        zeros for one that takes none (its entry would refuse them)"""
        if sensors is None or not self._site_moving:
            p.site_rows, p.limb_radius, p.site_moving = 0, 0.0, 0
            return
        if int(sensors.n_sensor) != self.site_rows.shape[1]:
            raise _lib.SsaHipError("the engine's site table is that of %d sensors, the launch's network has %d"
                                   % (self.site_rows.shape[1], int(sensors.n_sensor)))
        p.site_rows, p.limb_radius, p.site_moving = self.site_rows.data_ptr(), self.limb_radius, self._site_moving

    def _check_sensor_noise(self, sensors, envs=False):
        """the extent of z_noise that the sensors of `sensors` index: sensor s reads z_noise[s * sensors.zn_stride_sensor ...]; envs: in
        every env of the engine, env e's tables zn_stride_env behind env e - 1's"""
        S = int(sensors.n_sensor)
        need = (S - 1) * int(sensors.zn_stride_sensor) + (self.n_time - 1) * self.zn_stride_time + (self.m - 1) * int(self._p.zn_stride_obj) + 3
        if envs:
            need += (self.E - 1) * self.zn_stride_env
        if self.z_noise.numel() < need:
            raise _lib.SsaHipError("z_noise: %d values needed for %d sensors, got %d" % (need, S, self.z_noise.numel()))

    def launch_step_sensors(self, slot_in, slot_out, time_offset, sensors, actions, upd_out, stream=None, **kw):
        """enqueue the step of a sensor network (include/ssa_hip.h: ssa_env_step_sensors_f64; one env): sensor s observes object
        actions[s] (< 0: idle; two sensors on one object: the lower one updates it) with its own site, elevation mask, R and noise table
        z_noise[s * sensors.zn_stride_sensor ...]; the per-sensor update records go to `upd_out` (a pointer to [S][UPD_STRIDE] doubles, may
        be 0).  `sensors`: host.make_sensor_params(); its action words and record pointer are set here.  Every other keyword as
        launch_step (fast_stats, fold_inside, argmax_spos, obs_mirror, aer_out, stats_out, ...).  Asynchronous, no host sync."""
        self._one_env("a sensor network's step")
        S = int(sensors.n_sensor)
        if len(actions) != S:
            raise _lib.SsaHipError("launch_step_sensors: %d actions for %d sensors" % (len(actions), S))
        self._check_sensor_noise(sensors)
        for k in range(S):
            sensors.action[k] = int(actions[k])
        sensors.upd = int(upd_out)
        self.launch_step(slot_in, slot_out, time_offset, stream=stream, sensors=sensors, **kw)

    def _sensor_envs_block(self):
        """(ssa_sensor_envs_params, the [E][8] int32 device action table, its host staging) of this engine; allocated on first use"""
        if self._sensor_envs is None:
            W = _lib.MAX_SENSORS
            self._sensor_envs = (_lib.ssa_sensor_envs_params(), torch.full((self.E, W), -1, dtype=torch.int32, device=self.dev),
                                 np.full((self.E, W), -1, dtype=np.int32))
        return self._sensor_envs

    def action_table(self):
        """this engine's [E][MAX_SENSORS] int32 device action table: what launch_step_sensors_envs copies rows into, what
        launch_assign_sensors_envs writes and what launch_step_sensors_envs(actions=None) reads"""
        return self._sensor_envs_block()[1]

    def launch_step_sensors_envs(self, slot_in, slot_out, time_offset, sensors, actions=None, upd_out=0, stream=None, env_words=None, **kw):
        """enqueue the step of a sensor network in EVERY env of the engine, one launch (include/ssa_hip.h: ssa_env_step_sensors_envs_f64):
        per env what launch_step_sensors does for one.  `sensors`: host.make_sensor_params(), the sites all envs share (its action words
        and record pointer are not read); `actions` [E][S]: sensor s of env e observes object actions[e][s] of that env (< 0 or >= n_obj:
        idle; two sensors of one env on one object: the lower one updates it), with the noise table z_noise[e * zn_stride_env +
        s * sensors.zn_stride_sensor ...]; the update records go to `upd_out` (a pointer to [E][S][UPD_STRIDE] doubles, may be 0).
        env_words: the envs' time words (E <= 8) -- rows and times then travel by value in the launch's argument block
        (SSA_LAUNCH_INLINE_ENVS); otherwise the rows travel through this engine's [E][8] int32 device table (a blocking copy in the
        current stream, which a launch still running from that table must not share a race with: synchronise between such launches, as
        the vector env does) and the times are the engine's env_time0 words.  Several envs need n_obj % 4 == 0.  Every other keyword as launch_step.
        actions=None: the table is read as launch_assign_sensors_envs left it -- no copy, the rows from device memory, the times from
        env_time0 (env_words is refused): the actions never touch the host.
        Asynchronous, no host sync."""
        S = int(sensors.n_sensor)
        if actions is None:
            if env_words is not None:
                raise _lib.SsaHipError("launch_step_sensors_envs: actions=None reads the rows and the time words from device memory (no env_words)")
        else:
            a = np.asarray(actions, dtype=np.int64)
            if a.shape != (self.E, S):
                raise _lib.SsaHipError("launch_step_sensors_envs: actions must be [%d][%d] (envs x sensors), got %s" % (self.E, S, a.shape))
        self._whole_tiles("a sensor network in")
        self._check_sensor_noise(sensors, envs=True)
        v, table, rows_np = self._sensor_envs_block()
        v.upd = int(upd_out)
        if actions is None:
            v.actions = table.data_ptr()
            self.launch_step(slot_in, slot_out, time_offset, stream=stream, sensors=sensors, sensor_envs=v, env_words=None, **kw)
            return
        a = np.clip(a, -1, 2 ** 31 - 1)      # (an int32 word; anything < 0 is idle, anything >= n_obj too)
        if env_words is not None:
            if self.E > _lib.INLINE_ENVS:
                raise _lib.SsaHipError("env_words: at most %d envs travel in the parameter block" % _lib.INLINE_ENVS)
            v.actions = 0
            rows = a.tolist()
            for e in range(self.E):
                v.inline_action[e][:S] = rows[e]
            words = ([int(t) for t in env_words], [-1] * self.E)
        else:
            # (a blocking copy from ordinary host memory, E x 32 bytes: it has left the host array when it returns, so the next call may
            # rewrite it, and it is in the table before anything is enqueued here, whatever stream the launch goes to.  The table itself is
            # the caller's to keep intact until the launch has run -- as the engine's action words are)
            rows_np[:, :S] = a
            table.copy_(torch.from_numpy(rows_np))
            v.actions = table.data_ptr()
            words = None
        self.launch_step(slot_in, slot_out, time_offset, stream=stream, sensors=sensors, sensor_envs=v, env_words=words, **kw)

    LOOKAHEAD_PARTS = ("x_prior", "P_prior", "P_post")

    def _lookahead_out(self, name, attr, lead, prior_lead, out):
        """(ssa_lookahead_out, result dict) of a lookahead launch: the output buffers `attr` of this engine -- score lead + [3], status /
        visible [lead], the parts of LOOKAHEAD_PARTS asked for in `out` (x_prior prior_lead + [6], P_prior prior_lead + [6, 6], P_post
        lead + [6, 6]) -- allocated on first use (again when `lead` changes) and reused by the next call"""
        want = tuple(out)
        bad = [k for k in want if k not in self.LOOKAHEAD_PARTS]
        if bad:
            raise ValueError("%s: unknown output(s) %s (choose from %s)" % (name, bad, self.LOOKAHEAD_PARTS))
        look = getattr(self, attr)
        if look is None or tuple(look["status"].shape) != lead:
            look = {"score": torch.empty(lead + (_lib.LOOK_NSCORE,), dtype=f64, device=self.dev),
                    "status": torch.empty(lead, dtype=torch.int32, device=self.dev),
                    "visible": torch.empty(lead, dtype=torch.uint8, device=self.dev)}
            setattr(self, attr, look)
        shapes = {"x_prior": prior_lead + (6,), "P_prior": prior_lead + (6, 6), "P_post": lead + (6, 6)}
        for k in want:
            if k not in look:
                look[k] = torch.empty(shapes[k], dtype=f64, device=self.dev)
        o = _lib.ssa_lookahead_out()
        o.score, o.status, o.visible = (look[k].data_ptr() for k in ("score", "status", "visible"))
        for k in self.LOOKAHEAD_PARTS:
            setattr(o, k, look[k].data_ptr() if k in want else 0)
        return o, {k: look[k] for k in ("score", "status", "visible") + want}

    def _lookahead_params(self, slot_in, time_offset):
        """the input-only parameter block of a lookahead from history slot `slot_in` (nothing of the engine's state is written)"""
        p = _lib.ssa_step_params()
        C.memmove(C.byref(p), C.byref(self._p), C.sizeof(p))
        sl = int(slot_in) % self.H
        p.x_true_in, p.x_in, p.P_in = self._bx_t + sl * self._sx, self._bx + sl * self._sx, self._bP + sl * self._sP
        p.time_offset, p.launch_mask = int(time_offset), 0
        return p

    def _set_env_times(self, p, env_times):
        """the envs' time words by value in the input block `p` of a query launch (SSA_LAUNCH_INLINE_ENVS); None: the engine's env_time0 words"""
        if env_times is None:
            return
        if self.E > _lib.INLINE_ENVS:
            raise _lib.SsaHipError("env_times: at most %d envs travel in the parameter block" % _lib.INLINE_ENVS)
        p.inline_time[:self.E] = [int(v) for v in env_times]
        p.launch_mask = _lib.LAUNCH_INLINE_ENVS

    def _launch_look(self, entry, attr, lead, prior_lead, out, slot_in, time_offset, stream, sensors=None, n_steps=None, env_times=None):
        """the launch of the lookahead family: entry ssa_X_f64 of method launch_X, its output buffers `attr` (_lookahead_out: score lead
        + [3], the prediction prior_lead + [6 ...]), the input block of history slot `slot_in`; env_times: the envs' time words by value
        in that block (SSA_LAUNCH_INLINE_ENVS); sensors: the network's block; n_steps: a forecast -- the outputs travel in an
        ssa_forecast_params block.  Returns the result dict."""
        o, res = self._lookahead_out("launch_" + entry[4:-4], attr, lead, prior_lead, out)
        p = self._lookahead_params(slot_in, time_offset)
        self._set_sites(p, sensors)
        self._set_env_times(p, env_times)
        if n_steps is not None:
            o = _lib.ssa_forecast_params(n_steps=n_steps, out=o)
        blocks = (p, o) if sensors is None else (p, sensors, o)
        _lib.check(getattr(self._lib, entry)(self._cref, *(C.byref(b) for b in blocks), device._stream(stream)), entry)
        return res

    def launch_lookahead(self, slot_in, time_offset, out=(), stream=None, env_times=None):
        """enqueue the one-step tasking lookahead (include/ssa_hip.h: ssa_lookahead_f64) from history slot `slot_in` for the step whose
        time index is env_time + time_offset (env_times: the envs' time words by value, n_env <= 8; else the engine's env_time0 words, as a
        step reads them).  Nothing of the engine's state is written.  `out`: which of LOOKAHEAD_PARTS to produce besides the scores, status
        and visibility.  Returns a dict of this engine's output tensors, rows at the caller's indices of every env: score [E*m, 3],
        status [E*m] int32, visible [E*m] uint8 and the parts asked for (x_prior [E*m, 6], P_prior / P_post [E*m, 6, 6]) -- the buffers
        are allocated on first use and reused by the next call.  Asynchronous, no host sync."""
        N = self.m * self.E
        return self._launch_look("ssa_lookahead_f64", "_look", (N,), (N,), out, slot_in, time_offset, stream, env_times=env_times)

    def launch_lookahead_sensors(self, slot_in, time_offset, sensors, out=(), stream=None):
        """enqueue the lookahead of a sensor network (include/ssa_hip.h: ssa_lookahead_sensors_f64; one env): launch_lookahead for every
        sensor of `sensors` (host.make_sensor_params; its action words and record pointer are not read) in one launch -- the predict once,
        the hypothetical update once per sensor, from its site with its elevation mask and R.  Nothing of the engine's state is written.
        Returns a dict of this engine's output tensors, objects at the caller's indices: score [S, m, 3], status [S, m] int32,
        visible [S, m] uint8 and the parts of LOOKAHEAD_PARTS asked for in `out` (x_prior [m, 6], P_prior [m, 6, 6] -- the prediction, the
        same for every sensor -- and P_post [S, m, 6, 6]).  The buffers are allocated on first use (again when S changes) and reused by
        the next call.  Asynchronous, no host sync."""
        self._one_env("the lookahead of a sensor network")
        return self._launch_look("ssa_lookahead_sensors_f64", "_look_s", (int(sensors.n_sensor), self.m), (self.m,), out, slot_in, time_offset,
                                 stream, sensors)

    def launch_lookahead_sensors_envs(self, slot_in, time_offset, sensors, out=(), stream=None, env_times=None):
        """enqueue the lookahead of a sensor network in EVERY env of the engine, one launch (include/ssa_hip.h:
        ssa_lookahead_sensors_envs_f64): per env what launch_lookahead_sensors does for one, the sites of `sensors` shared by all envs.
        env_times: as launch_lookahead's (the envs' time words by value, n_env <= 8; else the engine's env_time0 words).  Nothing of the
        engine's state is written.  Returns a dict of this engine's output tensors, objects at each env's own caller indices: score
        [E, S, m, 3], status [E, S, m] int32, visible [E, S, m] uint8 and the parts of LOOKAHEAD_PARTS asked for in `out` (x_prior
        [E, m, 6], P_prior [E, m, 6, 6], P_post [E, S, m, 6, 6]).  The buffers are its own, allocated on first use (again when S changes)
        and reused by the next call.  Several envs need n_obj % 4 == 0.  Asynchronous, no host sync."""
        return self._launch_look("ssa_lookahead_sensors_envs_f64", "_look_se", (self.E, int(sensors.n_sensor), self.m), (self.E, self.m), out,
                                 slot_in, time_offset, stream, sensors, env_times=env_times)

    def launch_assign_sensors_envs(self, look, column, fallback=None, picks=None, stream=None, rule='greedy'):
        """enqueue every env's tasking assignment, one launch (include/ssa_hip.h: ssa_assign_sensors_envs_f64), on `look`, the dict
        launch_lookahead_sensors_envs returned: per env what launch_assign_sensors does for one, written into this engine's own
        [E][MAX_SENSORS] action table (action_table()) -- the one launch_step_sensors_envs(actions=None) then reads: the actions never
        touch the host.  fallback: int32 CUDA [E, MAX_SENSORS] draws (None: a sensor left without an object stays idle, -1); picks:
        int64 CUDA [E, MAX_SENSORS, 2] or None.  The workspace is this engine's (zeroed once, again when S changes).  Returns the table.
        rule='optimal': every env's exact optimum instead (ssa_match_sensors_envs_f64), same table, same workspace.
        Asynchronous, no host sync."""
        entry = device.assign_entry(rule, envs=True)
        score = look["score"]
        W = _lib.MAX_SENSORS
        _tensor_args("assign", ((fallback, torch.int32, self.E * W, "fallback"), (picks, torch.int64, 2 * self.E * W, "picks")))
        if not (_dev_tensor(score, f64) and score.dim() == 4 and tuple(score.shape) == (self.E, score.shape[1], self.m, _lib.LOOK_NSCORE)):
            raise _lib.SsaHipError("assign: the contiguous CUDA float64 [%d, S, %d, %d] scores of launch_lookahead_sensors_envs are needed"
                                   % (self.E, self.m, _lib.LOOK_NSCORE))
        S = int(score.shape[1])
        if self._assign_envs_ws is None or self._assign_envs_ws[0] != S:
            self._assign_envs_ws = (S, device.assign_sensors_envs_workspace(self.m, S, self.E, self.dev))
        table = self.action_table()
        # (the launch half of device.assign_sensors_envs: what that function checks has been checked above, against this engine's E and m)
        device._assign_launch(entry, score, (self.m, S, self.E), column, fallback, table, picks, self._assign_envs_ws[1], stream)
        return table

    def launch_forecast_sensors(self, slot_in, time_offset, sensors, n_steps, out=(), stream=None):
        """enqueue the tasking forecast of a sensor network (include/ssa_hip.h: ssa_forecast_sensors_f64; one env): what
        launch_lookahead_sensors would return at each of H = n_steps consecutive steps -- time indices time_offset .. time_offset + H - 1
        -- if every sensor stayed idle in between, in ONE launch that keeps the objects' state on chip across the steps.  Nothing of the
        engine's state is written.  Returns a dict of this engine's output tensors, objects at the caller's indices: score [H, S, m, 3],
        status [H, S, m] int32, visible [H, S, m] uint8 and the parts of LOOKAHEAD_PARTS asked for in `out` (x_prior [H, m, 6], P_prior
        [H, m, 6, 6], P_post [H, S, m, 6, 6]).  The buffers are allocated on first use (again when H or S changes) and reused by the next
        call; the scores alone are 24 * H * S * m bytes, P_post 288 * H * S * m.  Asynchronous, no host sync."""
        self._one_env("the forecast of a sensor network")
        H = int(n_steps)
        if H < 1:
            raise _lib.SsaHipError("launch_forecast_sensors: n_steps must be >= 1, got %d" % H)
        return self._launch_look("ssa_forecast_sensors_f64", "_fore", (H, int(sensors.n_sensor), self.m), (H, self.m), out, slot_in, time_offset,
                                 stream, sensors, n_steps=H)

    def launch_forecast_sensors_envs(self, slot_in, time_offset, sensors, n_steps, out=(), stream=None, env_times=None):
        """enqueue the tasking forecast of a sensor network in EVERY env of the engine, one launch (include/ssa_hip.h:
        ssa_forecast_sensors_envs_f64): per env what launch_forecast_sensors does for one, the sites of `sensors` shared by all envs --
        env e's steps have the time indices (e's time word) + time_offset .. + H - 1.  env_times: as launch_lookahead_sensors_envs' (the
        envs' time words by value, n_env <= 8; else the engine's env_time0 words).  Nothing of the engine's state is written.  Returns a
        dict of this engine's output tensors, objects at each env's own caller indices: score [H, E, S, m, 3], status [H, E, S, m] int32,
        visible [H, E, S, m] uint8 and the parts of LOOKAHEAD_PARTS asked for in `out` (x_prior [H, E, m, 6], P_prior [H, E, m, 6, 6],
        P_post [H, E, S, m, 6, 6]) -- score[h] is the contiguous [E, S, m, 3] block launch_assign_sensors_envs takes.  The buffers are
        its own, allocated on first use (again when H or S changes) and reused by the next call; the scores alone are 24 * H * E * S * m
        bytes, P_post 288 * H * E * S * m.  Several envs need n_obj % 4 == 0.  Asynchronous, no host sync."""
        H = int(n_steps)
        if H < 1:
            raise _lib.SsaHipError("launch_forecast_sensors_envs: n_steps must be >= 1, got %d" % H)
        return self._launch_look("ssa_forecast_sensors_envs_f64", "_fore_e", (H, self.E, int(sensors.n_sensor), self.m), (H, self.E, self.m), out,
                                 slot_in, time_offset, stream, sensors, n_steps=H, env_times=env_times)

    def launch_access_sensors(self, slot_in, time_offset, sensors, n_steps, envs=None, n_left=None, summary=True, stream=None, env_times=None):
        """enqueue the pass table of a sensor network (include/ssa_hip.h: ssa_access_sensors_f64): from the truth of history slot
        `slot_in`, for each of T = n_steps chained steps -- time indices (env's time word) + time_offset .. + T - 1 -- which sensor of
        `sensors` sees which object, by the fused kernels' own visibility rule (elevation mask, dark site, Earth shadow, line of sight
        from orbit) and for every env of the engine, in ONE launch.  The filters do not enter: a failed filter's object is not masked out.
        envs: the envs to compute (a sequence, or an int32 CUDA tensor: no host-to-device copy here) -- every other env's slab of the
        tables is left as it is; None: all.  n_left: an int32 CUDA tensor [E], env e counts only its first min(T, n_left[e]) steps; None:
        T.  env_times: as launch_lookahead's.  Nothing of the engine's state is read but x_true and nothing is written but the result:
        {'bits': int64 [E, S, m, W] (W = ceil(T / 64); bit h mod 64 of word h div 64 = step h: device.access_mask /
        device.access_unpack), 'pass': int32 [E, S, m, 4] (first, length, count, passes: _lib.PASS_*; None with summary=False)}, objects
        at each env's own caller indices.  The tensors are this engine's, allocated on first use (again when S or W changes) and reused
        by the next call.  Asynchronous, no host sync."""
        T, S = int(n_steps), int(sensors.n_sensor)
        if T < 1:
            raise _lib.SsaHipError("launch_access_sensors: n_steps must be >= 1, got %d" % T)
        shape = (self.E, S, self.m, device.access_words(T))
        if self._access is None or tuple(self._access["bits"].shape) != shape:
            self._access = {"bits": torch.zeros(shape, dtype=torch.int64, device=self.dev),
                            "pass": torch.zeros(shape[:3] + (4,), dtype=torch.int32, device=self.dev)}
        if envs is not None and not isinstance(envs, torch.Tensor):
            envs = torch.as_tensor(np.asarray(envs, dtype=np.int32).reshape(-1)).to(self.dev)
        p = self._lookahead_params(slot_in, time_offset)
        self._set_sites(p, sensors)
        self._set_env_times(p, env_times)
        device.access_sensors(self.consts, p, sensors, T, bits=self._access["bits"], summary=self._access["pass"] if summary else None,
                              n_left=n_left, env_sel=envs, stream=stream)
        return {"bits": self._access["bits"], "pass": self._access["pass"] if summary else None}

    def launch_dryrun_sensors(self, slot_in, time_offset, sensors, actions, stream=None, gather=True):
        """enqueue the dry run of B candidate tasking schedules from history slot `slot_in` (include/ssa_hip.h: ssa_dryrun_sensors_envs_f64;
        one env): what each schedule `actions[b]` ([B, K, S] integers, the caller's object numbering; < 0 or >= n_obj: idle; two sensors
        on one object in a row: the lower one updates it) would do to the covariances if it were run from this state with every
        innovation zero -- step k has time index time_offset + k --, in ONE launch.  Only the objects a candidate names can change its
        value, so the launch runs on a gathered block: the distinct objects of each candidate (device.dryrun_rows), padded to W rows, B
        pseudo-envs of W rows gathered from the slot with torch index ops (through the layout's inverse table when one is set).
        gather=False (B == 1): the full-catalogue form on the slot itself -- every object predicted K times, the cost of a rollout; the
        tests' yardstick.  Nothing of the engine's state is written.  Returns this engine's record tensor [B, K, S, DRY_STRIDE] (a view
        of a buffer cached per (B, K, S, W), rewritten by the next call).  Asynchronous, no host sync."""
        self._one_env("the dry run of a sensor network's schedules")
        S = int(sensors.n_sensor)
        if isinstance(actions, torch.Tensor):
            actions = actions.detach().cpu().numpy()
        ids, words = device.dryrun_rows(actions, self.m, S)
        B, K = int(ids.shape[0]), int(words.shape[0])
        if not gather and B != 1:
            raise _lib.SsaHipError("launch_dryrun_sensors(gather=False) takes one candidate, got %d" % B)
        W = int(ids.shape[1]) if gather else 0
        with _in_stream(stream):
            buf, (dev_words, dev_ids) = self._dry_buffers(self._dry, B, K, S, W, (words, ids[:, :W]))
            p = self._lookahead_params(slot_in, time_offset)
            self._set_sites(p, sensors)
            if gather:
                dev_ids = dev_ids.view(B, W)
                # a padding row takes the state of the candidate's first object (object 0 for an all-idle candidate): a healthy row to predict
                rows = torch.where(dev_ids >= 0, dev_ids, dev_ids[:, :1].clamp(min=0).expand(B, W)).reshape(-1).to(torch.int64)
                if self._order is not None:
                    rows = self._slot_of.index_select(0, rows)
                sl = int(slot_in) % self.H
                buf["state"] = (self.x_true[sl].index_select(0, rows), self.x_filter[sl].index_select(0, rows),
                                self.P_filter[sl].index_select(0, rows), self.status.index_select(0, rows), self.env_time0[:1].repeat(B))
                _dry_target(p, buf["state"], dev_ids)
            device.dryrun_sensors(self.consts, p, sensors, dev_words.view(K, B, _lib.MAX_SENSORS), K, self.m, out=buf["out"], stream=stream)
        return buf["out"].permute(1, 0, 2, 3)

    def _dry_buffers(self, cache, n, K, S, W, parts):
        """the buffers of a dry run of n pseudo-envs, cached in `cache` per (n, K, S, W) -- "dev": the call's ONE upload, "out": the records
        [K, n, S, DRY_STRIDE] -- and the upload itself, in torch's current stream: the int32 arrays `parts` side by side (the action
        words first: the kernel reads them 32 bytes at a time).  Returns (the cache entry, the device views of the parts)."""
        up = np.concatenate([a.reshape(-1) for a in parts])
        buf = cache.get((n, K, S, W))
        if buf is None:
            buf = cache[(n, K, S, W)] = {"dev": torch.empty(up.size, dtype=torch.int32, device=self.dev),
                                         "out": torch.empty((K, n, S, _lib.DRY_STRIDE), dtype=f64, device=self.dev)}
        buf["dev"].copy_(torch.from_numpy(up))
        return buf, buf["dev"].split([a.size for a in parts])

    def launch_dryrun_sensors_envs(self, slot_in, time_offset, sensors, actions, stream=None, env_times=None):
        """enqueue the dry run of B candidate tasking schedules in EVERY env of the engine (any n_env, 1 included):
        `actions` integers [E, B, K, S], env e's candidates in e's own object numbering, each read as launch_dryrun_sensors reads one
        -- step k of env e has the time index (e's time word) + time_offset + k.  The E * B candidates are E * B pseudo-envs of ONE
        ssa_dryrun_sensors_envs_f64 launch on a gathered block of W rows each (device.dryrun_rows over all of them: W is the batch's),
        and the block is gathered by ONE ssa_dryrun_gather_f64 launch in front of it -- through the layout's inverse table when one
        is set -- which also hands every candidate its env's time word.  env_times: the envs' time words by value (any n_env: they
        travel in the call's one upload, behind the action words and the ids); else the engine's env_time0 words.  The gathered block
        has whole tiles whatever n_obj is.  Nothing of the engine's state is written.  Returns this engine's record tensor
        [E, B, K, S, DRY_STRIDE] (a view of a buffer cached per (E * B, K, S, W), rewritten by the next call).  Asynchronous, no host
        sync, no torch index op."""
        S, E = int(sensors.n_sensor), self.E
        if isinstance(actions, torch.Tensor):
            actions = actions.detach().cpu().numpy()
        actions = np.asarray(actions)
        if actions.ndim != 4 or actions.shape[0] != E:
            raise ValueError("dry run: actions must be an integer array [%d, B, K, S], got shape %s" % (E, actions.shape))
        B = int(actions.shape[1])
        ids, words = device.dryrun_rows(actions.reshape((E * B,) + actions.shape[2:]), self.m, S)
        EB, K, W = E * B, int(words.shape[0]), int(ids.shape[1])
        if env_times is not None and len(env_times) != E:
            raise ValueError("dry run: env_times must hold %d time words, got %d" % (E, len(env_times)))
        times = np.zeros(E, dtype=np.int32) if env_times is None else np.asarray([int(v) for v in env_times], dtype=np.int32)
        sl = int(slot_in) % self.H
        with _in_stream(stream):
            buf, (dev_words, dev_ids, dev_times) = self._dry_buffers(self._dry_envs, EB, K, S, W, (words, ids, times))
            dev_ids = dev_ids.view(EB, W)
            # (the gathered block is the entry's own: allocated by the first call's gather, written again by every later one)
            buf["state"] = device.dryrun_gather(dev_ids, dev_times if env_times is not None else self.env_time0,
                                                self.x_true[sl], self.x_filter[sl], self.P_filter[sl], self.status, E, B, self.m,
                                                slot_of=self._slot_of32 if self._order is not None else None, out=buf.get("state"), stream=stream)
            p = self._lookahead_params(slot_in, time_offset)
            self._set_sites(p, sensors)
            _dry_target(p, buf["state"], dev_ids)
            device.dryrun_sensors(self.consts, p, sensors, dev_words.view(K, EB, _lib.MAX_SENSORS), K, self.m, out=buf["out"], stream=stream)
        return buf["out"].view(K, E, B, S, _lib.DRY_STRIDE).permute(1, 2, 0, 3, 4)

    def launch_assign_sensors(self, look, column, action_row, fallback_row=None, picks=None, stream=None, rule='greedy'):
        """enqueue the tasking assignment of a sensor network (include/ssa_hip.h: ssa_assign_sensors_f64) on `look`, the dict
        launch_lookahead_sensors returned: one object per sensor by the global greedy rule of agents._assign_lookahead_sensors over score
        column `column` (_lib.LOOK_*), written to `action_row` -- a 32-byte aligned CUDA int32 row of MAX_SENSORS words, e.g. row k of the
        [K, MAX_SENSORS] tensor whose one-row slice the next launch_rollout_sensors takes: the actions never touch the host.
        fallback_row: int32 [MAX_SENSORS] draws for the sensors left without an object (None: they stay idle, -1); picks: int64
        [MAX_SENSORS, 2] or None.  The workspace is this engine's (zeroed once, again when S changes).  rule='optimal': the exact optimum
        instead (ssa_match_sensors_f64: most sensors tasked, then the largest sum), same row, same workspace.  Asynchronous, no host sync."""
        entry = device.assign_entry(rule)
        score = look["score"]
        W = _lib.MAX_SENSORS
        _tensor_args("assign", ((action_row, torch.int32, W, "action_row"), (fallback_row, torch.int32, W, "fallback_row"),
                                (picks, torch.int64, 2 * W, "picks")))
        if action_row is None or not (_dev_tensor(score, f64) and score.dim() == 3 and tuple(score.shape) == (score.shape[0], self.m, _lib.LOOK_NSCORE)):
            raise _lib.SsaHipError("assign: an action row and the contiguous CUDA float64 [S, %d, %d] scores of launch_lookahead_sensors "
                                   "are needed" % (self.m, _lib.LOOK_NSCORE))
        S = int(score.shape[0])
        if self._assign_ws is None or self._assign_ws[0] != S:
            self._assign_ws = (S, device.assign_sensors_workspace(self.m, S, self.dev))
        device._assign_launch(entry, score, (self.m, S), column, fallback_row, action_row, picks, self._assign_ws[1], stream)

    def launch_plan_sensors(self, forecast, column, picks=None, stream=None):
        """enqueue the horizon-wide optimal tasking plan (include/ssa_hip.h: ssa_plan_sensors_f64) on `forecast`, the dict
        launch_forecast_sensors or launch_forecast_sensors_envs returned: ONE assignment problem over all H' * S (step, sensor) slots of
        score column `column` (_lib.LOOK_*) -- the most slots filled, then the largest sum of scores, no object twice in an env's plan --
        in ONE launch.  Returns this engine's own int32 CUDA table, [H', MAX_SENSORS] for scores [H', S, m, 3] and [H', E, MAX_SENSORS]
        for scores [H', E, S, m, 3] (-1 beyond S and in unfilled slots): the schedule launch_rollout_sensors / launch_rollout_sensors_envs
        takes as it is.  picks: int64 CUDA [H', (E,) MAX_SENSORS, 2] or None.  The table and the workspace are cached as the forecast's
        buffers are (allocated on first use, again when H' or S changes).  H' * S > MAX_PLAN_SLOTS is a ValueError.  Asynchronous, no
        host sync."""
        score = forecast["score"]
        if not (_dev_tensor(score, f64) and score.dim() in (4, 5) and score.shape[-1] == _lib.LOOK_NSCORE and score.shape[-2] == self.m
                and (score.dim() == 4 or score.shape[1] == self.E) and (score.dim() == 5 or self.E == 1)):
            raise _lib.SsaHipError("plan: the contiguous CUDA float64 [H', S, %d, %d] (or [H', %d, S, %d, %d]) scores of a forecast are "
                                   "needed" % (self.m, _lib.LOOK_NSCORE, self.E, self.m, _lib.LOOK_NSCORE))
        Hp, S = int(score.shape[0]), int(score.shape[-3])
        device.check_plan_slots(Hp, S)
        lead = tuple(score.shape[:-3])
        _tensor_args("plan", ((picks, torch.int64, 2 * Hp * self.E * _lib.MAX_SENSORS, "picks"),))
        if self._plan is None or self._plan[0] != (lead, S):
            self._plan = ((lead, S), torch.full(lead + (_lib.MAX_SENSORS,), -1, dtype=torch.int32, device=self.dev),
                          device.plan_sensors_workspace(self.m, S, Hp, self.E, self.dev))
        return device.plan_sensors(score, column, out=self._plan[1], picks=picks, workspace=self._plan[2], stream=stream)

    def assign_row(self):
        """this engine's own int32 [MAX_SENSORS] action row, for a caller of launch_assign_sensors that reads one assignment back
        (agents._assign_lookahead_sensors); allocated on first use"""
        if self._assign_row is None:
            self._assign_row = torch.full((_lib.MAX_SENSORS,), -1, dtype=torch.int32, device=self.dev)
        return self._assign_row

    def launch_rollout(self, slot_in, time_offset, actions, stream=None, argmax_spos=False):
        """K = actions.shape[0] consecutive steps in one launch (include/ssa_hip.h: ssa_env_rollout_f64): step k reads
        history slot (slot_in + k) % H, writes (slot_in + k + 1) % H and has time index time_offset + k.  `actions`
        is a device int32 tensor [K][E] (open-loop schedule).  Statistics: the last min(K, H) steps' slots."""
        actions = self._schedule(actions, (self.E,), None)
        s = device._stream(stream)
        r = self._rollout_params(slot_in, time_offset, int(actions.shape[0]), argmax_spos, s)
        r.upd_ring, r.actions = self._bu, actions.data_ptr()
        _lib.check(self._lib.ssa_env_rollout_f64(self._cref, self._pref, C.byref(r), s), "ssa_env_rollout_f64")

    def _rollout_params(self, slot_in, time_offset, K, argmax_spos, s, sensors=None):
        """what launch_rollout, launch_rollout_sensors and launch_rollout_sensors_envs share: pending statistics folded, the ssa_rollout_params block of K steps from
        history slot `slot_in` (rings, per-step shard sets and -- argmax_spos -- arg-max slots; actions and record ring left to the
        caller) and self._p made the parameter block of the first step"""
        self.flush_stats(s)
        if self._roll_shards is None or self._roll_shards.shape[0] < K:
            self._roll_shards = torch.zeros((K, self.E, _lib.STAT_SHARDS, _lib.STAT_SHARD_WORDS), dtype=torch.int64, device=self.dev)
        r = _lib.ssa_rollout_params()
        r.n_steps, r.history, r.slot_out = K, self.H, (int(slot_in) + 1) % self.H
        r.x_true_ring, r.x_ring, r.P_ring = self._bx_t, self._bx, self._bP
        r.obs_ring, r.metrics_ring, r.stats_ring = self._bo, self._bm, self._bs
        r.upd_ring, r.actions, r.stat_shards = 0, 0, self._roll_shards.data_ptr()
        r.spos_tiles = 0
        if argmax_spos:     # per-step arg-max slots: every step's statistics carry np.argmax(sigma_pos) (the 'shaped' reward)
            if not self.supports_argmax:
                raise _lib.SsaHipError("argmax_spos needs whole tiles per env (n_env == 1 or n_obj % 4 == 0)")
            if self._roll_spos is None or self._roll_spos.shape[0] < K:
                self._roll_spos = torch.zeros((K, self.ntiles, 2), dtype=torch.int64, device=self.dev)
            r.spos_tiles = self._roll_spos.data_ptr()
        self._first_step_block(time_offset, sensors)
        return r

    def _first_step_block(self, time_offset, sensors=None):
        """self._p made the parameter block of the first step of a multi-step launch (rollout, closed loop; sensors: a network's)"""
        p = self._p
        p.time_offset = int(time_offset)
        self._set_sites(p, sensors)
        p.launch_mask, p.stat_shards_prev, p.stats_prev, p.aer_out, p.metrics_prev = 0, 0, 0, 0, 0
        p.spos_tiles, p.spos_tiles_prev = 0, 0

    def launch_rollout_sensors(self, slot_in, time_offset, sensors, actions, stream=None, argmax_spos=False):
        """launch_rollout for a sensor network (include/ssa_hip.h: ssa_env_rollout_sensors_f64; one env): the K = actions.shape[0] launches
        launch_step_sensors would make for the rows of `actions`, in one launch and bit-identical to them.  `sensors`:
        host.make_sensor_params() (its action words and record pointer are not read); `actions`: a contiguous CUDA int32 tensor [K, S]
        or [K, MAX_SENSORS] (row k = the sensors' objects at step k; < 0: idle; two sensors on one object: the lower one updates it).
        The per-sensor update records of the last min(K, H) steps are in self.upd_sensors [H, S, UPD_STRIDE] (allocated on first use,
        again when S changes), slot (slot_in + k + 1) % H for step k.  Asynchronous, no host sync."""
        self._one_env("a sensor network's rollout")
        S = int(sensors.n_sensor)
        actions = self._schedule(actions, (), S)
        self._check_sensor_noise(sensors)
        self._roll_sched = actions      # (kept until the next launch: the kernel reads it whatever stream it runs in)
        upd = self.upd_sensors
        if upd is None or upd.shape[1] != S:
            upd = self.upd_sensors = torch.zeros((self.H, S, _lib.UPD_STRIDE), dtype=f64, device=self.dev)
        s = device._stream(stream)
        r = self._rollout_params(slot_in, time_offset, int(actions.shape[0]), argmax_spos, s, sensors)
        rs = _lib.ssa_rollout_sensors_params()
        rs.actions, rs.upd_ring = actions.data_ptr(), upd.data_ptr()
        _lib.check(self._lib.ssa_env_rollout_sensors_f64(self._cref, self._pref, C.byref(r), C.byref(sensors), C.byref(rs), s),
                   "ssa_env_rollout_sensors_f64")

    def launch_rollout_sensors_envs(self, slot_in, time_offset, sensors, actions, stream=None, argmax_spos=False, records=False):
        """launch_rollout_sensors in EVERY env of the engine (include/ssa_hip.h: ssa_env_rollout_sensors_envs_f64): the K = actions.shape[0]
        launches launch_step_sensors_envs would make for the rows actions[k], in one launch and bit-identical to them -- step k reads
        history slot (slot_in + k) % H, writes (slot_in + k + 1) % H, and env e's time index is env_time0[e] + time_offset + k.
        `sensors`: host.make_sensor_params(), the sites all envs share; `actions`: a contiguous CUDA int32 tensor [K, E, S] or
        [K, E, MAX_SENSORS] (row (k, e) = the objects of env e's sensors at step k; < 0 or >= n_obj: idle; two sensors of one env on one
        object: the lower one updates it), kept alive until the next launch.  Returns (stats [K, E, STAT_STRIDE], upd
        [K, E, S, UPD_STRIDE] or None without `records`): device tensors of the engine's own -- every step's statistics and per-sensor
        update records whatever H is --, reused (and rewritten) by the next call.  Several envs need n_obj % 4 == 0.  Asynchronous, no
        host sync."""
        S = int(sensors.n_sensor)
        actions = self._schedule(actions, (self.E,), S)
        self._whole_tiles("a sensor network in")
        self._check_sensor_noise(sensors, envs=True)
        self._roll_sched = actions      # (kept until the next launch: the kernel reads it whatever stream it runs in)
        K = int(actions.shape[0])
        out = self._roll_envs_out
        if out is None or out[0].shape[0] < K or out[1].shape[2] != S or (records and out[1].shape[0] < K):
            out = self._roll_envs_out = (torch.zeros((K, self.E, _lib.STAT_STRIDE), dtype=f64, device=self.dev),
                                         torch.zeros((K if records else 0, self.E, S, _lib.UPD_STRIDE), dtype=f64, device=self.dev))
        s = device._stream(stream)
        r = self._rollout_params(slot_in, time_offset, K, argmax_spos, s, sensors)
        re = _lib.ssa_rollout_sensors_envs_params()
        re.actions, re.stats_out, re.upd_out = actions.data_ptr(), out[0].data_ptr(), out[1].data_ptr() if records else 0
        _lib.check(self._lib.ssa_env_rollout_sensors_envs_f64(self._cref, self._pref, C.byref(r), C.byref(sensors), C.byref(re), s),
                   "ssa_env_rollout_sensors_envs_f64")
        return out[0][:K], (out[1][:K] if records else None)

    def launch_closed_loop(self, slot_in, time_offset, kind, actions, stats_out, upd_out=None, fallback=None, picks=None, stream=None,
                           argmax_spos=False, wait_ticks=0, debug_withhold=False):
        """K steps AND the K decisions of a greedy agent in ONE persistent launch (include/ssa_hip.h:
        ssa_env_closed_loop_f64).  `actions`: device int32 [K + 1], actions[0] = the first step's action (given), the kernel
        writes actions[1..K]; `stats_out` device float64 [K][STAT_STRIDE]; `upd_out` [K][UPD_STRIDE] or None; `fallback`
        int32 [K + 1] or None; `picks` int64 [K + 1][2] or None.  Step k reads history slot (slot_in + k) % H and writes
        (slot_in + k + 1) % H with time index time_offset + k.  Returns False -- nothing enqueued -- when the library
        declines the configuration (several envs, or more objects than resident wavefronts x 4): the caller then issues
        the per-step launches.  self.loop_error (host-mapped int32, cleared before every launch) turns 1 if the launch gave up:
        a wavefront waited longer than `wait_ticks` (100 MHz ticks; 0 = 2 s) for a decision.  argmax_spos: the statistics carry
        np.argmax(sigma_pos) (SSA_LOOP_ARGMAX_SPOS).  debug_withhold: diagnostic -- the decision is never published (the test of
        the give-up path)."""
        if self.E != 1:
            return False
        K = int(actions.numel()) - 1
        if K < 1:
            raise _lib.SsaHipError("closed loop: actions must hold K + 1 >= 2 words")
        _tensor_args("closed loop", ((actions, torch.int32, K + 1, "actions"), (stats_out, f64, K * _lib.STAT_STRIDE, "stats_out"),
                                     (upd_out, f64, K * _lib.UPD_STRIDE, "upd_out"), (fallback, torch.int32, K + 1, "fallback"),
                                     (picks, torch.int64, 2 * (K + 1), "picks")), at_least=True)
        if self._loop_ws is None:
            nb = int(self._lib.ssa_closed_loop_workspace_bytes(self.m, self.E))
            if nb <= 0:
                return False
            self._loop_ws = torch.zeros(nb // 8, dtype=torch.int64, device=self.dev)
            self._loop_err_host = torch.zeros(1, dtype=torch.int32).pin_memory()
            self.loop_error = self._loop_err_host.numpy()
        s = device._stream(stream)
        self.flush_stats(s)
        self.loop_error[0] = 0      # (a launch that gave up must not poison the next one: nothing is in flight here, run_agent synchronises)
        r = _lib.ssa_closed_loop_params()
        r.n_steps, r.history, r.slot_out, r.agent = K, self.H, (int(slot_in) + 1) % self.H, int(kind)
        r.x_true_ring, r.x_ring, r.P_ring = self._bx_t, self._bx, self._bP
        r.obs_ring, r.metrics_ring = self._bo, self._bm
        r.upd_out = upd_out.data_ptr() if upd_out is not None else 0
        r.stats_out, r.actions = stats_out.data_ptr(), actions.data_ptr()
        r.fallback = fallback.data_ptr() if fallback is not None else 0
        r.picks = picks.data_ptr() if picks is not None else 0
        r.error = self._loop_err_host.data_ptr()
        r.workspace, r.workspace_bytes = self._loop_ws.data_ptr(), self._loop_ws.numel() * 8
        r.wait_ticks = int(wait_ticks)
        r.flags = (_lib.LOOP_ARGMAX_SPOS if argmax_spos else 0) | (_lib.LOOP_DEBUG_WITHHOLD if debug_withhold else 0)
        r.slot_of = self._slot_of32.data_ptr() if self._order is not None else 0     # (a storage layout: its inverse table)
        self._first_step_block(time_offset)
        rc = self._lib.ssa_env_closed_loop_f64(self._cref, self._pref, C.byref(r), s)
        if rc == _lib.E_UNSUPPORTED:
            return False
        _lib.check(rc, "ssa_env_closed_loop_f64")
        return True

    def launch_agent_select(self, slot_cur, time_offset, kind, action_ptr, fallback_ptr=0, pick_ptr=0, stream=None, have_prev=True):
        """enqueue the device-side agent (include/ssa_hip.h: ssa_agent_select_f64): choose, for every env, the action of
        the NEXT step from history slot `slot_cur` (and the slot before it for the Shannon agent) and store it in the
        int32 word(s) at `action_ptr` -- the pointer the next launch_step() is given as actions_ptr.  No host sync."""
        if self._agent_ws is None:
            nb = self._lib.ssa_agent_select_workspace_bytes(self.m, self.E)
            self._agent_ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=self.dev)
        sc = int(slot_cur) % self.H
        sp = (sc + self.H - 1) % self.H
        # (with a storage layout the candidates are named as the caller numbers them: ssa_agent_select_ids_f64)
        rc = self._lib.ssa_agent_select_ids_f64(self._cref, int(kind), self._bx_t + sc * self._sx, self._bx + sc * self._sx,
                                                self._bP + sc * self._sP, (self._bP + sp * self._sP) if have_prev else 0, self.trans.data_ptr(),
                                                self.env_time0.data_ptr(), int(time_offset), self.n_time, fallback_ptr,
                                                self._agent_ws.data_ptr(), action_ptr, pick_ptr, self.m, self.E,
                                                self._obj_ids.data_ptr() if self._order is not None else 0, device._stream(stream))
        _lib.check(rc, "ssa_agent_select_ids_f64")

    def profile_ms(self, slot):
        """duration [ms] of the dominant kernel of the step launched with profile_slot=slot (waits for it)."""
        ms = C.c_float(0.0)
        _lib.check(self._lib.ssa_env_step_profile_ms(int(slot), C.byref(ms)), "ssa_env_step_profile_ms")
        return float(ms.value)

    def flush_stats(self, stream=None):
        """fold the statistics of the last deferred step (no-op when nothing is pending)."""
        if self._fold_pending is None:
            return
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        k, dst, argmax, metrics = self._fold_pending
        if metrics:     # (a step whose statistics come from its metrics rows: the service wavefronts on their own)
            rc = self._lib.ssa_stats_fold_metrics_f64(metrics, self._shard_sets[k].data_ptr(), self._spos_ptr(k) if argmax else 0, dst, self.m, s)
        elif argmax:
            rc = self._lib.ssa_stats_fold_spos_f64(self._shard_sets[k].data_ptr(), self._spos_ptr(k), dst, self.m, self.E, s)
        else:
            rc = self._lib.ssa_stats_fold_f64(self._shard_sets[k].data_ptr(), dst, self.E, s)
        self._fold_pending = None
        if rc:
            raise _lib.SsaHipError("%s failed with code %d" % ("ssa_stats_fold_metrics_f64" if metrics else "ssa_stats_fold_spos_f64" if argmax
                                                               else "ssa_stats_fold_f64", rc))

    def set_actions(self, actions):
        a = torch.as_tensor(np.asarray(actions, dtype=np.int32).reshape(self.E))
        self.actions.copy_(a, non_blocking=True)
