"""SSA_Tasker_Env.run_policy, as a mixin: its graphs, streams, workspace and error are attributes of the env, declared where it is built."""
import numpy as np

from .. import _graphs, _lib


def _action_word(a):
    """what a policy handed back, as the int32 word the next step launch reads: a CUDA int32 tensor with one element, or -- what torch.argmax
    returns -- an int64 one, whose LOW word is the action (little endian; -1 stays -1): no cast kernel (5 us at 20 000 objects inside a replayed
    graph, profiles/r04_run_policy_timeline.txt)."""
    import torch
    if isinstance(a, torch.Tensor) and a.is_cuda and a.numel() == 1:
        if a.dtype == torch.int32:
            return a
        if a.dtype == torch.int64:
            return a.reshape(1).view(torch.int32)[:1]
    raise TypeError("run_policy: the policy must return a CUDA int32 (or int64) tensor with one element (the action)")


class _PolicyLoop:
    # ------------------------------------------------------------------ closed loop with ANY policy that lives on the GPU
    class PolicyView:
        """what a device-side policy sees at decision time: CUDA tensors of the env's CURRENT state (views of the history slot --
        valid until the next step is launched; nothing is copied, nothing crosses PCIe)."""

        def __init__(self, env, i, tix_off=None):
            self.env, self.i = env, i
            # inside a captured graph the step's time index lives on the DEVICE (engine.env_time0, which the graph advances between
            # replays) and this decision sits `tix_off` steps behind it: the GCRS -> ITRS matrix is then picked by the kernels themselves
            # (ssa_*_at_f64) instead of by a host integer that a capture would freeze
            self._tix_off = tix_off

        # (views are formed on access: a tensor slice costs the host 1-2 us, and most policies read one or two of them)
        obs = property(lambda s: s.env._engine.obs[s.i % s.env._engine.H])            # [m, 12]: x_filter | diag P   (results.py:61)
        x_filter = property(lambda s: s.env._engine.x_filter[s.i % s.env._engine.H])
        P_filter = property(lambda s: s.env._engine.P_filter[s.i % s.env._engine.H])
        x_true = property(lambda s: s.env._engine.x_true[s.i % s.env._engine.H])
        P_filter_prev = property(lambda s: s.env._engine.P_filter[(s.i - 1) % s.env._engine.H] if s.i >= 1 else None)

        def visible(self):
            """uint8 CUDA mask [m]: object_visibility() of the true states (ssa_tasker_simple_2.py:427-434)"""
            from .. import device
            e = self.env._engine
            if self._tix_off is not None:
                return device.visible_mask_at(self.x_true, e.trans, e.env_time0, self._tix_off, self.env._consts)
            return device.visible_mask(self.x_true, e.trans[self.i % e.n_time].reshape(3, 3), self.env._consts)

        def argmax(self, score, mask=None):
            """the policy's arg-max head in ONE launch: np.argmax(score[mask != 0]) mapped back to object indices (first maximum, NaN
            skipped, -1 when nothing is selected) as the int32 CUDA tensor [1] run_policy expects.  torch.argmax + a cast are two launches
            and 16 us at 20 000 objects (profiles/r04_run_policy_timeline.txt); this is 3-4."""
            from .. import device
            env = self.env
            if env._argmax_ws is None or env._argmax_ws_n < score.shape[0]:     # (owned by the env: its launches share a stream)
                env._argmax_ws, env._argmax_ws_n = device.masked_argmax_workspace(score.shape[0], score.device), score.shape[0]
            return device.masked_argmax_action(score, mask, env._argmax_ws)

        def scores(self):
            """(scores[4, m], mask[m]) of the reference's heuristic agents (trace P, visible, log-det ratio, delta_pos)"""
            from .. import device
            e = self.env._engine
            if self._tix_off is not None:
                return device.agent_scores_at(self.x_true, self.x_filter, self.P_filter, self.P_filter_prev, e.trans, e.env_time0, self._tix_off,
                                              self.env._consts)
            return device.agent_scores(self.x_true, self.x_filter, self.P_filter, self.P_filter_prev, e.trans[self.i % e.n_time].reshape(3, 3),
                                       self.env._consts)

    # ---- run_policy as a replayed hipGraph: K x [the policy's kernels + the step launch] captured once, replayed per chunk
    GRAPH_CHUNK = 32

    def _policy_graph(self, policy, K, i0):
        """capture (once per policy / chunk length / history phase) K steps of the closed loop -- for every step the policy's own kernels on
        the current history slot, then the step launch reading the action word the policy produced -- into ONE hipGraph.  What changes
        from replay to replay lives in device memory: the time index (engine.env_time0, advanced by K at the graph's end; the steps
        read env_time0 + their position), the history slots by parity (K is a multiple of the ring depth).  Returns the cache entry
        or None when the policy cannot be captured (it synchronises, allocates outside the graph's pool, ...): the caller enqueues
        eagerly."""
        import torch
        e = self._engine
        key = (id(policy), K, i0 % e.H)
        ent = self._policy_graphs.get(key)
        if ent is not None or key in self._policy_graphs:
            return ent
        stats_d = torch.zeros((K, _lib.STAT_STRIDE), dtype=torch.float64, device=e.dev)
        upd_d = torch.zeros((K, _lib.UPD_STRIDE), dtype=torch.float64, device=e.dev)
        acts_d = torch.full((K,), -1, dtype=torch.int32, device=e.dev)
        shaped = self.reward_type == 'shaped'

        acts_t = []          # the policy's K action tensors: they live in the graph's memory pool, at the same addresses in every replay

        def enqueue():
            for k in range(K):
                i = i0 + k + 1
                a = _action_word(policy(self.PolicyView(self, i - 1, tix_off=k)))
                acts_t.append(a)          # (read by the step below; gathered into acts_d ONCE per replay, behind the graph)
                e.launch_step((i - 1) % e.H, i % e.H, k + 1, actions_ptr=a.data_ptr(), fast_stats=True, defer_fold=True,
                              stats_out=stats_d[k].data_ptr(), upd_out=upd_d[k].data_ptr(), argmax_spos=shaped)
            e.flush_stats()
            torch.cat([a.reshape(1) for a in acts_t], out=acts_d)
            e.env_time0.add_(K)
        if self._policy_streams is None:      # capture / replay stream and the copy stream of the pipelined chunks: one pair per env
            self._policy_streams = (torch.cuda.Stream(device=e.dev), torch.cuda.Stream(device=e.dev))
        stream, copy_stream = self._policy_streams
        # two sets of pinned host buffers for the replay's results (statistics, update records, actions): chunk c is booked from one while
        # the copy behind replay c + 1 fills the other
        hosts = tuple(tuple(torch.empty(d.shape, dtype=d.dtype, pin_memory=True) for d in (stats_d, upd_d, acts_d)) for _ in range(2))
        self._policy_refs[id(policy)] = policy      # (while the entry exists, no other policy gets this id)
        try:
            policy(self.PolicyView(self, i0))      # (eagerly once, result unused: lazy initialisation must not happen inside the capture)
            g, exc = _graphs.capture(stream, enqueue)
        except Exception as err:  # noqa: BLE001  (the eager call raised: as a capture that failed)
            g, exc = None, err
        if isinstance(exc, TypeError):
            raise exc
        if exc is not None:      # (not capture-safe: remembered, the eager loop takes over)
            self.policy_graph_error = repr(exc)
            e._fold_pending = None
        torch.cuda.current_stream().wait_stream(stream)
        ent = (g, stats_d, upd_d, acts_d, stream, hosts, copy_stream) if g is not None else None
        self._policy_graphs[key] = ent
        return ent

    def run_policy(self, policy, n_steps, graph='auto'):
        """Closed loop with an ARBITRARY policy evaluated on the GPU (a torch module, a hand-written rule):
            a = policy(view)          # view: SSA_Tasker_Env.PolicyView -- CUDA tensors; returns an int32 (or int64: torch.argmax) CUDA tensor [1]
            step(a)
        repeated n_steps times with NO host round trip: the action never leaves the device (the step kernel reads it from the
        tensor the policy returned), the statistics and update records go to device rings, ONE synchronisation at the end, then the
        env's bookkeeping (actions, rewards, dones, failures, z_true / y / S records) is filled in as step() would have.  The
        reference's loop `a = agent(obs, env); env.step(a)` (run_environment.py:26-29) for agents that are not one of the built-in
        greedy ones (those: run_agent, one persistent launch).  Every reward type; a data-dependent `done` ('jones', 'shaped') is
        honoured at the bookkeeping -- the steps launched behind it are discarded (chunks of history - 1 steps, as run_agent).
        Returns (actions[k], rewards[k], dones[k])."""
        self._single_sensor('run_policy')
        self._caller_order()          # (the policy's views are the env's own object order)
        import torch
        shaped = self.reward_type == 'shaped'
        e = self._engine
        K = min(int(n_steps), self.n - 1 - self.i)
        actions, rewards, dones = [], [], []
        pos, done = 0, False
        # graph = 'auto' | True: chunks of GRAPH_CHUNK steps replayed from a captured hipGraph where that is possible -- a reward without a
        # data-dependent `done` ('trinary': every step of the call is wanted), a history ring whose depth divides the chunk, a policy
        # that can be captured; everything else (and graph = False) takes the eager loop below, step by step from the host
        G = self.GRAPH_CHUNK
        use_graph = bool(graph) and self.reward_type == 'trinary' and G % e.H == 0
        # The chunks are PIPELINED: replay c + 1 is enqueued before the host books chunk c.  A replay writes its statistics / update records /
        # actions at fixed device addresses, so right behind every replay a copy stream moves them into one of two pinned host buffers
        # (12 KB), and the next replay waits for that copy alone; the host then fills in chunk c's bookkeeping (5 us per step) while the
        # GPU runs chunk c + 1.  (Round 4 measurement, profiles/r04_run_policy_timeline.txt: inside a replay the GPU idles < 1 us between
        # kernels, but synchronise - copy - book - replay left it idle for 16 us per step at chunk boundaries.)  An invalid action is
        # therefore reported one chunk late: the steps enqueued behind it have run (with no update: the kernel ignores an action out of range).
        pend = None            # (host arrays, event) of the replay whose bookkeeping is outstanding

        def book(host, ev):
            nonlocal done
            ev.synchronize()
            stats, upd, acts = host       # (ring head: the replays run ahead of the booking)
            done = self._book_steps(acts, stats, upd, i_start + launched, (actions, rewards, dones), check_actions=True)
        launched, i_start, gstream = 0, self.i, None      # steps enqueued by replays (self.i follows as the chunks are booked)
        try:
            while use_graph and K - launched >= G and not done:
                i0 = i_start + launched
                ent = self._policy_graph(policy, G, i0)
                if ent is None:
                    break
                g, stats_d, upd_d, acts_d, gstream, hosts, copy_stream = ent
                if launched == 0:
                    e.flush_stats()
                    e.env_time0.fill_(i0)
                    gstream.wait_stream(torch.cuda.current_stream())
                slot = (launched // G) % 2
                with torch.cuda.stream(gstream):
                    g.replay()
                    ready = torch.cuda.Event()
                    ready.record(gstream)
                copy_stream.wait_event(ready)
                with torch.cuda.stream(copy_stream):
                    for h, d in zip(hosts[slot], (stats_d, upd_d, acts_d)):
                        h.copy_(d, non_blocking=True)
                    copied = torch.cuda.Event()
                    copied.record(copy_stream)
                gstream.wait_event(copied)         # the NEXT replay overwrites the device buffers only behind this copy
                launched += G
                if pend is not None:
                    book(*pend)                    # chunk c - 1, while the GPU runs chunk c
                pend = (tuple(h.numpy() for h in hosts[slot]), copied)
            if pend is not None:
                book(*pend)
        finally:
            if gstream is not None:
                torch.cuda.current_stream().wait_stream(gstream)
                e.env_time0.zero_()
        pos = launched
        while pos < K and not done:
            kk = (K - pos) if self.reward_type == 'trinary' else min(K - pos, e.H - 1)
            i0 = self.i
            stats_d = torch.empty((kk, _lib.STAT_STRIDE), dtype=torch.float64, device=e.dev)
            upd_d = torch.empty((kk, _lib.UPD_STRIDE), dtype=torch.float64, device=e.dev)
            acts_d = []
            for k in range(kk):
                i = i0 + k + 1
                a = _action_word(policy(self.PolicyView(self, i - 1)))
                acts_d.append(a)          # (kept alive until the launches that read it have run)
                e.launch_step((i - 1) % e.H, i % e.H, i, actions_ptr=a.data_ptr(), fast_stats=True, defer_fold=True,
                              stats_out=stats_d[k].data_ptr(), upd_out=upd_d[k].data_ptr(), argmax_spos=shaped)
                self.i = i                # (the view of the next decision indexes the history by it)
            e.flush_stats()
            stats = stats_d.cpu().numpy()                  # synchronises the stream
            upd = upd_d.cpu().numpy()
            acts = torch.cat([a.reshape(1) for a in acts_d]).cpu().numpy()
            self.i = i0
            done = self._book_steps(acts, stats, upd, i0 + kk, (actions, rewards, dones), check_actions=True)
            pos += kk
        return np.asarray(actions, dtype=int), np.asarray(rewards), np.asarray(dones, dtype=bool)
