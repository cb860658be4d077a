"""The reference-shaped views SSA_Tasker_Env hands out: device-resident histories, records kept only at [i, action], failure messages."""
import numpy as np

from .. import _lib


class _History:
    """numpy-indexable view of a device-resident history tensor [H][E*m][...] for ONE env.

    `hist[i]` -> numpy array of step i (copied from HBM on access); `hist[i, j]`, `hist[i][mask]`,
    negative indices and slices over the time axis work like on the reference's (n, m, ...) arrays.
    Only the last H steps are resident when the env was built with a shorter history."""

    def __init__(self, env, tensor, m_axis_len, tail_shape):
        self._env, self._t = env, tensor
        self.shape = (env.n, m_axis_len) + tuple(tail_shape)
        self.dtype = np.dtype(np.float64)
        self.ndim = len(self.shape)

    def __len__(self):
        return self.shape[0]

    def _slot(self, i):
        env = self._env
        i = int(i)
        if i < 0:
            i += env.n
        if not 0 <= i < env.n:
            raise IndexError(i)
        env._caller_order()       # (the history arrays are read as the env numbers the objects: a storage layout ends here)
        H = env._engine.H
        if i > env.i or i <= env.i - H:
            if i > env.i:   # not simulated yet: the reference arrays hold zeros there after reset()
                return np.zeros(self.shape[1:])
            raise IndexError("step %d is no longer resident (history depth %d, current step %d); build the env "
                             "with config['history'] = 'full'" % (i, H, env.i))
        return self._t[i % H].cpu().numpy().reshape(self.shape[1:])

    def __getitem__(self, idx):
        if isinstance(idx, tuple):
            head, rest = idx[0], idx[1:]
        else:
            head, rest = idx, ()
        if isinstance(head, slice):
            arr = np.stack([self._slot(i) for i in range(*head.indices(self.shape[0]))])
            return arr[(slice(None),) + rest] if rest else arr
        arr = self._slot(head)
        return arr[rest] if rest else arr

    def __array__(self, dtype=None, copy=None):
        a = np.stack([self._slot(i) for i in range(self.shape[0])])
        return a.astype(dtype) if dtype is not None else a


class _Sparse:
    """reference-shaped (n, m, k...) view of a quantity the reference stores only at [i, action]
    (z_true, y: NaN elsewhere -- ssa_tasker_simple_2.py:139-142, 202)."""

    def __init__(self, env, store, tail):
        self._env, self._s = env, store
        self.shape = (env.n, env.m) + tuple(tail)

    def __getitem__(self, idx):
        env = self._env
        if isinstance(idx, tuple):
            i, rest = idx[0], idx[1:]
        else:
            i, rest = idx, ()
        if isinstance(i, slice):
            return np.stack([self[k] for k in range(*i.indices(env.n))])[(slice(None),) + rest]
        i = int(i) + (env.n if int(i) < 0 else 0)
        row = np.full(self.shape[1:], np.nan)
        a = env._upd_action[i]
        if a >= 0:
            row[a] = self._s[i]
        return row[rest] if rest else row

    def __array__(self, dtype=None, copy=None):
        return np.stack([self[i] for i in range(self.shape[0])])


class _FailureMessages:
    """`failed_filters_msg` of the reference (ssa_tasker_simple_2.py:147, 380): a list of m entries, "None" until filter j fails, then
    [message].  The message -- 'Object j failed on predict step i, LinAlgError. [dpos dvel spos svel]' -- is FORMATTED WHEN IT IS READ, from the
    record the kernel wrote at the failure: an episode of the default env loses a few filters per step late on, and formatting each as it
    happened cost a gym-style step tens of microseconds."""
    KINDS = {_lib.ST_PREDICT_NAN: ('predict', ', predict returned nan. '), _lib.ST_PREDICT_LINALG: ('predict', ', LinAlgError. '),
             _lib.ST_UPDATE_NAN: ('update', ', update returned nan. '), _lib.ST_UPDATE_LINALG: ('update', ', LinAlgError. ')}

    def __init__(self, m):
        self._m, self._rec = int(m), {}

    def record(self, j, step, status, err):
        self._rec[j] = (step, status, err)

    def __len__(self):
        return self._m

    def __getitem__(self, j):
        if isinstance(j, slice):
            return [self[k] for k in range(*j.indices(self._m))]
        j = int(j)
        if j < 0:
            j += self._m
        if not 0 <= j < self._m:
            raise IndexError(j)
        r = self._rec.get(j)
        if r is None:
            return "None"
        activity, error_type = self.KINDS[r[1]]
        return ["".join(['Object ', str(j), ' failed on ', activity, ' step ', str(r[0]), error_type, str(np.round(r[2], 2))])]

    def __iter__(self):
        return (self[j] for j in range(self._m))
