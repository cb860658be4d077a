"""Observation buffers that are handed out WITHOUT a copy and come back by themselves.

The reference's `step()` returns a fresh array per call (`ssa_tasker_simple_2.py:360-366`: `.flatten()` / a history row that no later step
overwrites): a consumer may keep it -- replay buffers, sample collectors, frame stacks.  Copying the kernel-written, host-mapped buffer into a
fresh array costs a 1.9 MB host memcpy per step at 20 000 objects (65 us of a 124 us step; 5.1 MB for the vector env).  Instead the step kernel
writes each step's observation into a buffer NOBODY HOLDS: the array `step()` returns is a new ndarray over that buffer's memory whose base
is a small ctypes object; when the array and every view derived from it are gone, the object's finaliser puts the buffer back on the free
list.  A consumer that keeps more than `cap` observations alive at once gets copies beyond that (pinned memory is not for hoarding)."""
import ctypes
import weakref

import numpy as np


class ObsPool:
    def __init__(self, n_doubles, shape, cap=64, dtype=np.float64):
        self.n, self.shape, self.cap = int(n_doubles), tuple(shape), int(cap)
        self.dtype = np.dtype(dtype)         # float64 (the reference's), or float32 (config['obs_dtype']: the kernel writes the host copy in single)
        self._ctype = ctypes.c_float if self.dtype == np.float32 else ctypes.c_double
        self._bufs, self._np, self.ptrs, self._free = [], [], [], []
        self.handed_out = 0            # (diagnostic: arrays given out / buffers ever allocated)

    def acquire(self):
        """index of a buffer nobody holds (a new pinned one while fewer than `cap` exist), or None: the caller copies this step"""
        if self._free:
            return self._free.pop()
        if len(self._bufs) < self.cap:
            import torch
            t = torch.zeros(self.n, dtype=torch.float32 if self.dtype == np.float32 else torch.float64).pin_memory()
            self._bufs.append(t)
            self._np.append(t.numpy())
            self.ptrs.append(t.data_ptr())
            return len(self._bufs) - 1
        return None

    def release(self, k):
        self._free.append(k)

    def hand_out(self, k):
        """a FRESH ndarray over buffer k (its memory is pinned, host-mapped, just written by the kernel); buffer k is free again when this
        array and every view of it have been dropped"""
        # (from_buffer, not from_address: the ctypes object then OWNS a reference to the pinned tensor's array -- an observation a consumer still
        # holds keeps its memory alive even when the env that handed it out is gone)
        c = (self._ctype * self.n).from_buffer(self._np[k])
        weakref.finalize(c, self._free.append, k)
        self.handed_out += 1
        return np.frombuffer(c, dtype=self.dtype).reshape(self.shape)

    def __len__(self):
        return len(self._bufs)


class HostObs:
    """the host side of a step's observation, for SSA_Tasker_Env and SSA_Tasker_VecEnv: the step kernel writes the observation straight
    into host-mapped pinned memory (its epilogue's 'aer' block, or a second copy of the observation rows), `dest(k)` names that memory
    for step k's launch and `hand_out()` returns what step() gives the caller.  With a pool (`pool_cap`): a buffer nobody holds, handed
    out as a fresh array (ObsPool), or a copy of ring buffer k % depth when `pool_cap` buffers are out.  Without (pool_cap None): ring
    buffer k % depth itself -- config['obs_zero_copy'] (intact until `depth` further steps), or a depth-1 ring: the ONE persistent array
    of the reference's 'aer' observation (ssa_tasker_simple_2.py:362-363), refreshed in place.  f32: float32 buffers
    (config['obs_dtype']: the kernel writes the host copy in single precision)."""

    def __init__(self, n, shape, f32, depth, pool_cap):
        import torch
        self.f32 = bool(f32)
        self.dtype = np.dtype(np.float32 if self.f32 else np.float64)
        ring = [torch.zeros(n, dtype=torch.float32 if self.f32 else torch.float64).pin_memory() for _ in range(depth)]
        self._ring = ring
        self.ring_np = [b.numpy().reshape(shape) for b in ring]
        self._ring_ptr = [b.data_ptr() for b in ring]
        self._depth = depth
        self.pool = None if pool_cap is None else ObsPool(n, shape, cap=int(pool_cap), dtype=self.dtype)
        self._k, self._kp = 0, None

    def dest(self, k):
        """the host-mapped destination of step k's observation (call once per launch, before hand_out)"""
        pool = self.pool
        kp = self._kp = pool.acquire() if pool is not None else None
        if kp is not None:
            return pool.ptrs[kp]
        k = self._k = k % self._depth
        return self._ring_ptr[k]

    def hand_out(self):
        """the observation the last dest() named, once the launch has completed"""
        if self._kp is not None:
            return self.pool.hand_out(self._kp)     # fresh array, no copy: the buffer comes back when the consumer drops it
        if self.pool is not None:
            return self.ring_np[self._k].copy()     # (more than `pool_cap` observations alive at once)
        return self.ring_np[self._k]

    def cast(self, a):
        """an observation that reached the host through a device-to-host copy, in the dtype step() hands out"""
        return a.astype(np.float32) if self.f32 else a
