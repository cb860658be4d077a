"""A sensor network's lookahead and assignment in each of several envs: the engines of the GPU tests (one vector engine and its E
one-env twins from one batch), the numpy greedy assignment, and the single envs that take a vector env's noise draws."""
import numpy as np

from support.batches import c2t, make_batch
from support.sensors import BAD, N_TIME, sites_rad

MASKS_DEG = [15.0, -90.0, -80.0, 0.0, 5.0, -10.0, 20.0, -30.0]     # (sensor 1 sees everything: an object below sensor 0's mask is above its)
T0 = [2, 5, 3, 1, 4, 6, 8, 7, 9]      # env e's time index before the first step


def i64(a):
    return np.ascontiguousarray(a).view(np.int64)


def bad_of(m):
    """the object whose filter state is NaN (support.sensors.BAD, folded into envs smaller than that)"""
    return BAD if m > BAD else BAD % m


def network(host, S, obs_type, stride, masks=None):
    lla = sites_rad()[:S]
    lim = np.radians((MASKS_DEG if masks is None else masks)[:S])
    if obs_type == "aer":
        sig = [np.array([(1.0 + k) * host.arcsec2rad, (0.5 + 2.0 * k) * host.arcsec2rad, 1e3 / (1 + k)]) for k in range(S)]
    else:
        sig = [np.array([5e2 / (1 + 0.25 * k)] * 3) for k in range(S)]
    Rs = [np.diag(s ** 2) for s in sig]
    return lla, lim, Rs, sig, host.make_sensor_params(lla, lim, Rs, stride)


class Engines:
    """one batch of E x m objects (a NaN filter per env), a network of S sites, the vector engine and -- on demand -- the E one-env
    engines that hold env e's state slice, noise tables and time index"""

    def __init__(self, hip, E, m, S, propagator="hybrid", obs_type="aer", interval=1, history=2, layout=False, masks=None, nan=True):
        torch, host = hip.torch, hip.host
        self.hip, self.E, self.m, self.S, self.H = hip, E, m, S, history
        self.xt, self.x, self.P, g = make_batch(E * m, seed=123)
        if nan:
            for e in range(E):
                self.x[e * m + bad_of(m), 1] = np.nan
        self.trans = c2t()[:N_TIME]
        self.lla, self.lim, self.Rs, sig, self.sp = network(host, S, obs_type, N_TIME * m * 3, masks)
        self.consts = host.make_consts(g["Q"], self.Rs[0], 1e-4, 2.0, -3, 20.0, self.lim[0], self.lla[0], propagator=propagator,
                                       obs_type=obs_type, update_interval=interval)
        gen = torch.Generator(device="cuda").manual_seed(8)
        self.zn = torch.randn((E, S, N_TIME, m, 3), dtype=torch.float64, device="cuda", generator=gen) * \
            torch.as_tensor(np.stack(sig), device="cuda").view(1, S, 1, 1, 3)
        self.t0 = [2, 4] if E == 2 else T0[:E]
        self.orders = [np.random.RandomState(40 + e).permutation(m) for e in range(E)] if layout else None
        self.vec = hip.engine.HotPathEngine(self.consts, m, E, self.trans, self.zn, history=history, zn_stride_env=S * N_TIME * m * 3)
        if layout:
            self.vec.set_layout(np.stack(self.orders) if E > 1 else self.orders[0])
        self.vec.load_state(0, self.xt, self.x, self.P)
        self.vec.env_time0.copy_(torch.as_tensor(self.t0, dtype=torch.int32))

    def one(self, e):
        eng = self.hip.engine.HotPathEngine(self.consts, self.m, 1, self.trans, self.zn[e], history=self.H, zn_stride_env=0)
        if self.orders is not None:
            eng.set_layout(self.orders[e])
        sl = slice(e * self.m, (e + 1) * self.m)
        eng.load_state(0, self.xt[sl], self.x[sl], self.P[sl])
        return eng


def numpy_np(torch, r):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in r.items()}


def greedy_rows(score, fallback=None):
    """the global greedy assignment over score [S, m] in numpy: (rows [S] with the fallback rule applied, assigned [S], values [S])"""
    S, m = score.shape
    v = score.astype(np.float64).copy()
    act, val = np.full(S, -1, dtype=np.int64), np.zeros(S)
    for _ in range(S):
        live = np.flatnonzero(~np.isnan(v.reshape(-1)))
        if not len(live):
            break
        k = int(live[np.argmax(v.reshape(-1)[live])])       # (the first maximum: the lowest s * m + j; -0.0 == 0.0; -inf is a value)
        s, j = divmod(k, m)
        act[s], val[s] = j, v[s, j]
        v[s, :] = np.nan
        v[:, j] = np.nan
    assigned = act.copy()
    if fallback is not None:
        for s in range(S):
            f = int(fallback[s])
            if act[s] < 0 and 0 <= f < m and f not in act:
                act[s] = f
    return act, assigned, val


def single_envs(envs, cfg, vec, seed):
    """E single envs with seeds seed + e, their engines' noise tables overwritten with the vector env's draws (e, s, i) for every object"""
    singles = []
    for e in range(vec.E):
        one = envs.make(config=dict(cfg, seed=seed + e))
        z = vec._eng.z_noise[e]                                  # [S, n, 1, 3] ([n, 1, 3] without a network)
        one._engine.z_noise.copy_(z.expand(*z.shape[:-2], vec.m, 3).reshape(one._engine.z_noise.shape))
        singles.append(one)
    return singles
