"""The time row of the fused kernels once the index wraps (include/ssa_hip.h, ssa_step_params.n_time: "index = i % n_time"): a SHORT
engine of T rows against a LONG engine whose four time-indexed tables -- trans, z_noise, the Sun table, site_rows -- have 4 T rows,
long[r] = short[r % T], the rows chosen by numpy on the host.  On the long engine no index of the tests reaches n_time (the path the
oracle tests pin); on the short one it wraps; everything a launch leaves must be the same bits.  The control of every comparison: the
long tables with the rows at and after T of ONE table shifted by one, wrong[r] = short[(r + 1) % T] -- the result must then differ.
Here: the row choice, the scenes in which every table's row decides something at every row (asserted on the CPU oracle, with the
margins of support.illumination / support.orbiting), the engines, one runner per entry point, and the two absolute anchors."""
import numpy as np

from support import angles_only as ao
from support import illumination as il
from support import orbiting as ob

T = 16                      # rows of the short tables (support.sensors.N_TIME)
LONG = 4 * T                # rows of the long ones: the largest index of the tests is 3 T + 5 + a few steps
H = 6                       # history slots: a launch of up to 5 steps leaves every slot it wrote
TABLES = ("trans", "z_noise", "sun", "site_rows")
AXIS = {"trans": 0, "z_noise": -3, "sun": 0, "dark": 0, "site_rows": 0}      # the time axis of every array of a table set
OWNER = {"dark": "sun"}     # (the dark words travel in the Sun table's rows)
SINGLE = (T - 1, T, T + 1, 2 * T, 3 * T + 5)
WORDS3, WORDS2 = (T - 2, T + 3, 3 * T - 1), (T - 1, 2 * T + 1)
M_TILES = 10244             # 2 envs: 20 488 objects -- the grid-stride instance, a wavefront walks tiles of both envs
EPS = np.finfo(np.float64).eps
NEAR_ZENITH = np.radians(89.9)


# ---------------------------------------------------------------------------------------------------------------- the row choice
def long_rows():
    return np.arange(LONG) % T


def wrong_rows():
    r = np.arange(LONG)
    return np.where(r >= T, (r + 1) % T, r % T)


def extend(a, axis=0):
    """long[r] = short[r % T] along `axis`"""
    return np.ascontiguousarray(np.take(np.asarray(a), long_rows(), axis=axis))


def shift(a, axis=0):
    """wrong[r] = short[r] below T, short[(r + 1) % T] from T on, along `axis`"""
    return np.ascontiguousarray(np.take(np.asarray(a), wrong_rows(), axis=axis))


def variant(short, which=None):
    """a table set {trans [T, 9], z_noise [E, S, T, m, 3], sun [T, 3], dark [T], site_rows [T, S, 16] or None}: None -- itself;
    'long' -- every table extended; a name of TABLES -- every table extended, that ONE shifted"""
    if which is None:
        return short
    assert which == "long" or which in TABLES, which
    return {k: None if a is None else (shift if OWNER.get(k, k) == which else extend)(a, AXIS[k]) for k, a in short.items()}


def strides(tabs):
    """the noise strides of a table set, in doubles, recomputed from ITS row count: time, sensor, env"""
    E, S, n, m, _ = tabs["z_noise"].shape
    assert n == tabs["trans"].shape[0] == tabs["sun"].shape[0] == tabs["dark"].shape[0]
    assert tabs["site_rows"] is None or tabs["site_rows"].shape[0] == n
    return dict(time=3 * m, sensor=n * m * 3, env=S * n * m * 3, n_time=n)


def extent_ok(tabs):
    """the engine's own extent checks (HotPathEngine.__init__, _check_sensor_noise) on the recomputed strides"""
    E, S, n, m, _ = tabs["z_noise"].shape
    st = strides(tabs)
    need = (E - 1) * st["env"] + (S - 1) * st["sensor"] + (n - 1) * st["time"] + (m - 1) * 3 + 3
    return need == tabs["z_noise"].size


# ---------------------------------------------------------------------------------------------------------------- the scenes
class Scene:
    """kind 'moving': support.orbiting's network (a ground radar, a moving 'ae' telescope, a moving 'aer' sensor that needs its object
    sunlit; site_moving = 0b110); 'ground': support.illumination's (ground sites; sensors 1 and 2 need a sunlit object and a dark
    site).  E envs of m objects, every env the same eight objects (the first and the last eight rows of an env are objects 0 .. 7:
    sensor s is tasked with object s, or with the s-th of the last eight), high above the network for the whole table; the noise
    tables differ per env and sensor.  GOOD rows (r % 2 == phase): the Sun over the network, every site dark, sensor 1 under its
    object; the other rows: the Sun opposite object 2 (it stands in the shadow), sites 1 and 2 not dark, sensor 1 behind the Earth.
    Sensor 2 stands under its object, at another place in every row.  So every row differs from its neighbour in a cell of
    every table."""

    def __init__(self, oracle, oracle_ld, kind, m, E, phase, K=5, seed=7, edge=False):
        from support.batches import c2t
        self.kind, self.m, self.E, self.phase, self.K, self.oracle = kind, m, E, phase, K, oracle
        self.net = net = (ob.Net if kind == "moving" else il.Net)(oracle)
        self.moving = kind == "moving"
        trans = np.ascontiguousarray(c2t()[:T]).reshape(T, 9)
        xt, x, P = ao.scene(net, oracle_ld, trans[T // 2], 8, seed, high=True)
        if edge:
            xt[EDGE], x[EDGE], P[EDGE] = edge_object(net, oracle, oracle_ld, trans)
        self.eight = (xt, x, P)
        self.truth = il.truths(oracle, xt, K)          # truth[k]: the true states at step k of a launch (k + 1 steps of DT on)
        src = np.arange(m) % 8
        if m > 8:
            src[-8:] = np.arange(8)
        self.src = src
        self.state = tuple(np.concatenate([a[src]] * E) for a in (xt, x, P))
        # (m > 8: the even envs task objects of their first tile, the odd ones of their last-but-one -- at M_TILES the two tiles one
        # wavefront of the grid-stride instance walks)
        self.acts = np.array([[0, 1, 2] if (m <= 8 or e % 2 == 0) else [m - 8, m - 7, m - 6] for e in range(E)])
        mid = self.truth[K // 2]
        good = np.arange(T) % 2 == phase
        self.good = good
        up = il.zenith(net, trans[T // 2])
        sun = np.array([up if good[r] else il.sun_lighting(mid[2, :3], -1.0) for r in range(T)])
        dark = np.where(good, il.ALL_DARK, 0b001 if kind == "ground" else 0).astype(np.int64)
        rows = self.site_obs = None
        if self.moving:
            pos = {1: np.array([(ob.below if good[r] else ob.behind)(mid[1, :3], tilt=0.2 + 0.005 * r, seed=1) for r in range(T)]),
                   2: np.array([ob.below(mid[2, :3], tilt=0.3 + 0.02 * r, seed=2) for r in range(T)])}
            rows, self.site_obs = ob.table(trans, pos)
        S = net.S
        zn = np.random.RandomState(91 + m + E).normal(size=(E, S, T, m, 3)) * np.asarray(net.sig).reshape(1, S, 1, 1, 3)
        self.tabs = dict(trans=trans, z_noise=zn, sun=sun, dark=dark, site_rows=rows)

    def tables(self):
        """the tables of TABLES this scene's network reads"""
        return TABLES if self.moving else TABLES[:3]

    def visible(self, k, row):
        """([S, 8] booleans, sensor 0's -- 'ground': every sensor's -- margin from its mask): the numpy rules for the truth at step k
        of a launch under table row `row`"""
        t, tr = self.tabs, self.truth[k]
        if self.moving:
            return ob.expected_visible(self.net, self.oracle, tr, t["trans"][row], self.site_obs[row], t["sun"][row])
        return il.expected_visible(self.net, self.oracle, tr, t["trans"][row], t["sun"][row], t["dark"][row])

    def assert_margins(self, k, row):
        vis, gap = self.visible(k, row)
        il.assert_margins(self.truth[k], self.tabs["sun"][row], gap)
        if self.moving:
            for s in (1, 2):
                ob.assert_margins(self.truth[k][:, :3], self.tabs["trans"][row], self.site_obs[row, s])
        return vis

    def check(self, words, K=1):
        """the construction of a case that starts at the time indices `words` (one per env) and runs K steps: at every index the
        margins of the row and of its neighbour; at every WRAPPED index the tasked cells of sensor 0 visible (an update is taken: trans
        and z_noise matter), the Sun table's cell (sensor 2, object 2) and -- moving -- the site table's cell (sensor 1, object 1)
        decided the other way by the neighbour row, and sensor 2's place another.  Some wrapped index has both cells visible from
        the right row.  Returns the number of wrapped indices (0: the case pins bit-equality only -- a control cannot differ below T)"""
        wrapped, both = 0, False
        for w in words:
            for k in range(K):
                tix = int(w) + k
                row, nxt = tix % T, (tix + 1) % T
                vis, other = self.assert_margins(k, row), self.assert_margins(k, nxt)
                if tix < T:
                    continue
                wrapped += 1
                assert vis[0, 0], (tix, "sensor 0 does not see its object")
                assert vis[2, 2] != other[2, 2] and vis[2, 2] == bool(self.good[row]), (tix, "the Sun row decides nothing")
                if self.moving:
                    assert vis[1, 1] != other[1, 1] and vis[1, 1] == bool(self.good[row]), (tix, "the site row decides nothing")
                    assert not np.array_equal(self.tabs["site_rows"][row, 2], self.tabs["site_rows"][nxt, 2])
                    both |= bool(vis[1, 1] and vis[2, 2])
                else:
                    assert vis[1, 1] != other[1, 1], (tix, "the dark word decides nothing")
                    both |= bool(vis[2, 2] and vis[1, 1])
                assert not np.array_equal(self.tabs["trans"][row], self.tabs["trans"][nxt])
                assert not np.array_equal(self.tabs["z_noise"][:, :, row], self.tabs["z_noise"][:, :, nxt])
        assert both or not wrapped, (words, K, "no wrapped index at which the right row shows both cells")
        return wrapped


_SCENES = {}


def scene(oracle, oracle_ld, kind="moving", m=8, E=1, phase=0, edge=False):
    key = (kind, m, E, phase, edge)
    if key not in _SCENES:
        _SCENES[key] = Scene(oracle, oracle_ld, kind, m, E, phase, edge=edge)
    return _SCENES[key]


# the closed loop's own row: an object on the ground radar's elevation mask, for ssa_env_closed_loop_f64 from the state of step
# LOOP_I0 = T - 2 (run_closed_loop).  The greedy agent's visibility mask judges the truth of step i under row i % T; this object's
# covariance is the largest, so it is the agent's choice wherever the mask lets it through
EDGE, LOOP_I0 = 3, T - 2
EDGE_MARGIN = 1e-4      # [rad] from the mask, either side: 1e9 roundings of the elevation, a tenth of what one row turns the Earth by


def edge_elevations(net, oracle, truth, trans):
    """{(step after LOOP_I0, row): the elevation above the ground radar's horizon of the edge object's true state `truth[step]`}
    for the decisions after steps 0, 1, 2 (rows T - 2, T - 1, 0) and for the decision after step 2 under the NEIGHBOUR row 1"""
    el = lambda x, row: float(oracle.hx_aer(x[None], trans[row], net.lla[0], net.itrs[0])[0, 1])      # noqa: E731
    return {(0, T - 2): el(truth[0], T - 2), (1, T - 1): el(truth[1], T - 1), (2, 0): el(truth[2], 0), (2, 1): el(truth[2], 1)}


def edge_object(net, oracle, oracle_ld, trans):
    """(truth, filter mean, covariance) of the edge object at step LOOP_I0: in the west of the ground radar, 25 000 km away, climbing
    -- below the mask at steps T - 2 and T - 1, and at step T above it by half of what ONE row turns the Earth by: visible under row 0,
    the right one, and below the mask under row 1, which is 20 s later and has the site turned away from it"""
    rs = np.random.RandomState(5)
    site, itrs, lim = net.lla[0], net.itrs[0], net.lim[0]
    up = il.zenith(net, trans[0])
    el = lim
    for _ in range(3):      # (the elevation the object is placed at under row 0: the mask plus half the difference between the rows)
        p = ao.place(site, itrs, trans[0], np.radians(270.0), el, 2.5e7, rs)[:3]
        v = il.unit(up - (up @ il.unit(p)) * il.unit(p)) * np.sqrt(ao.MU / np.linalg.norm(p))
        x0 = oracle_ld.propagate(np.concatenate([p, v]), -2 * ao.DT)[0]
        truth = [x0] + [t[0] for t in il.truths(oracle, x0[None], 2)]
        e = edge_elevations(net, oracle, truth, trans)
        el += lim + 0.5 * (e[(2, 0)] - e[(2, 1)]) - e[(2, 0)]
    return x0, x0 + rs.normal(size=6) * ao.X_SIGMA, np.diag(ao.X_SIGMA ** 2) * 25.0


def check_edge(sc):
    """the edge object of scene `sc` does what edge_object says, with EDGE_MARGIN on every verdict; and its covariance is the largest"""
    truth = [sc.eight[0][EDGE]] + [t[EDGE] for t in sc.truth[:2]]
    e = edge_elevations(sc.net, sc.oracle, truth, sc.tabs["trans"])
    lim = sc.net.lim[0]
    assert all(abs(v - lim) >= EDGE_MARGIN for v in e.values()), (e, lim)
    assert e[(0, T - 2)] < lim and e[(1, T - 1)] < lim and e[(2, 0)] > lim > e[(2, 1)], (e, lim)
    tr = np.trace(sc.eight[2], axis1=1, axis2=2)
    assert tr.argmax() == EDGE and tr[EDGE] >= 20 * np.delete(tr, EDGE).max()


def phase_of(words, K=1):
    """the phase that makes the first wrapped index of a K-step launch from `words` a good row (none wraps: its first index)"""
    idx = [int(w) + k for w in words for k in range(K)]
    return ([i for i in idx if i >= T] or idx)[0] % 2


# what tests/test_time_wrap_gpu.py runs, as (kind, m, E, time words, steps): tests/test_time_wrap_host.py checks every one on the CPU
CASES = [(kind, m, 1, (tix,), 1) for kind in ("moving", "ground") for m in (8, 7) for tix in SINGLE] + \
        [("moving", 8, 3, WORDS3, 1), ("moving", 8, 2, WORDS2, 1), ("ground", 8, 3, WORDS3, 1), ("moving", M_TILES, 2, WORDS2, 1)] + \
        [("moving", m, 1, w, K) for m in (8, 7) for w, K in (((T - 2,), 5), ((T - 2,), 4), ((T - 1,), 4))] + \
        [("moving", 8, 3, WORDS3, 4), ("moving", 8, 2, WORDS2, 4), ("ground", 8, 2, WORDS2, 1)] + \
        [("moving", m, 1, (tix,), 1) for m in (8, 7) for tix in (T + 1, T + 2, 2 * T + 1)]


# ---------------------------------------------------------------------------------------------------------------- the engines
def make_engine(hip, sc, tabs, propagator="hybrid", interval=1):
    """(engine, sensor block) of scene `sc` on the table set `tabs`: the same consts, sensor block and (later) state whatever the
    tables' row count; the pointers and the strides are what differs"""
    from support.batches import make_batch
    torch, net = hip.torch, sc.net
    g = make_batch(1, seed=0)[3]
    consts = hip.host.make_consts(g["Q"], net.R[0], ao.ALPHA, 2.0, -3, ao.DT, net.lim[0], net.lla[0], propagator=propagator,
                                  update_interval=interval)
    st = strides(tabs)
    zn = torch.as_tensor(np.ascontiguousarray(tabs["z_noise"])).cuda()
    eng = hip.engine.HotPathEngine(consts, sc.m, sc.E, tabs["trans"], zn, history=H, zn_stride_env=st["env"] if sc.E > 1 else 0)
    assert eng.n_time == st["n_time"] and eng.zn_stride_time == st["time"]
    eng.set_sun_table(tabs["sun"], tabs["dark"])
    if sc.moving:
        eng.set_site_table(tabs["site_rows"], net.moving, ob.R_LIMB)
    return eng, net.params(st["sensor"], sun_ptr=eng.sun.data_ptr())


def load(hip, eng, sc, words, offset=1, slot=0):
    """the scene's state into `slot`, everything a launch accumulates cleared, env e's time word = words[e] - offset (a launch with
    time_offset = offset then has the time indices `words`)"""
    torch = hip.torch
    eng.load_state(slot, *sc.state)
    for t in (eng.status, eng.fail_count, eng.stats, eng.upd):
        t.zero_()
    eng.env_time0.copy_(torch.as_tensor([int(w) - offset for w in words], dtype=torch.int32))
    torch.cuda.synchronize()


def capture(hip, eng, **extra):
    """everything a launch leaves on the engine, as numpy: the whole ring, the status words, the statistics words, the update records
    (their defined fields), the failure records (sorted: concurrent wavefronts append in no order) -- and `extra` tensors (names
    that start with 'upd': update records)"""
    from support.sensors import _defined_fields
    torch, L = hip.torch, hip.lib
    eng.flush_stats()
    torch.cuda.synchronize()
    words = [L.STAT_MAX_DPOS, L.STAT_CNT_LT_1E4, L.STAT_CNT_LT_1E7, L.STAT_N_FAILED]
    out = {k: getattr(eng, k).cpu().numpy().copy() for k in ("x_true", "x_filter", "P_filter", "obs", "metrics", "status")}
    out["stats"] = eng.stats.cpu().numpy()[..., words].copy()
    out["upd_ring"] = _defined_fields(L, eng.upd.cpu().numpy())
    nf = int(eng.fail_count.cpu()[0])
    out["fail_count"] = np.array([nf])
    out["fail_log"] = np.array(sorted(map(tuple, np.nan_to_num(eng.fail_log[:nf], nan=-1.0).tolist())), dtype=np.float64).reshape(nf, L.FAIL_STRIDE)
    if eng.upd_sensors is not None:
        out["upd_sensors"] = _defined_fields(L, eng.upd_sensors.cpu().numpy())
    for k, v in extra.items():
        v = v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else np.asarray(v)
        out[k] = _defined_fields(L, v) if k.startswith("upd") else v
    return out


def differing(a, b):
    """the keys in which two captures differ, compared as il.same_bits compares"""
    bad = []
    for k in a:
        u, v = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if u.dtype == np.float64:
            u, v = u.view(np.int64), v.view(np.int64)
        if u.shape != v.shape or not np.array_equal(u, v):
            bad.append(k)
    return bad


def pin(run, sc, tables, what):
    """the comparison of one case: run(table set) on the short tables and on the long ones -- the same bits --, and on the long ones
    with each table of `tables` shifted alone -- not the same.  Returns the short engine's capture"""
    assert set(tables) <= set(sc.tables()), (what, tables)
    short = run(sc.tabs)
    il.same_bits(short, run(variant(sc.tabs, "long")), (what, "short vs long"))
    for name in tables:
        assert differing(short, run(variant(sc.tabs, name))), (what, "a wrong row of %s changes nothing" % name)
    return short


# ---------------------------------------------------------------------------------------------------------------- the runners
def _i32(hip, a):
    return hip.torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device="cuda").contiguous()


def run_step(hip, sc, tabs, words, propagator="hybrid", delivery="ptr", aer=0, two_launch=False, interval=1):
    """ssa_env_step_f64, one step at the time indices `words`: env e selects its sensor-0 object.  delivery 'ptr' (action and time words
    in memory), 'inline' (action=; one env), 'words' (env_words=); aer: the columns of the aer_out payload (0: none); two_launch: the
    statistics by the post kernel (which then writes the payload)"""
    torch = hip.torch
    eng, _ = make_engine(hip, sc, tabs, propagator, interval)
    acts = [int(a) for a in sc.acts[:, 0]]
    kw = dict(fast_stats=not two_launch, fold_inside=not two_launch and sc.E == 1 and not aer)
    extra = {}
    if aer:
        extra["aer"] = torch.full((sc.E * sc.m * aer,), -7.0, dtype=torch.float64, device="cuda")
        kw.update(aer_out=extra["aer"].data_ptr(), aer_cols=aer)
    if delivery == "ptr":
        load(hip, eng, sc, words, offset=1)
        eng.set_actions(acts)
        eng.launch_step(0, 1, 1, **kw)
    elif delivery == "inline":
        load(hip, eng, sc, [0], offset=0)
        eng.launch_step(0, 1, int(words[0]), action=acts[0], **kw)
    else:
        load(hip, eng, sc, [0] * sc.E, offset=0)
        eng.launch_step(0, 1, 0, env_words=([int(w) for w in words], acts), **kw)
    return capture(hip, eng, **extra)


def run_rollout(hip, sc, tabs, words, K, propagator="hybrid"):
    """ssa_env_rollout_f64: K steps from the time indices `words`, env e on its sensor-0 object at the even steps, nobody at the odd"""
    eng, _ = make_engine(hip, sc, tabs, propagator)
    load(hip, eng, sc, words, offset=1)
    sched = np.array([[int(a) if k % 2 == 0 else -1 for a in sc.acts[:, 0]] for k in range(K)])
    eng.launch_rollout(0, 1, _i32(hip, sched))
    return capture(hip, eng)


def run_lookahead(hip, sc, tabs, words, entry="plain", by_value=False, n_steps=None):
    """ssa_lookahead_f64 ('plain'), ssa_lookahead_sensors_f64 ('sensors'), ssa_lookahead_sensors_envs_f64 ('envs') at `words`, every
    output; n_steps: the forecasts instead (ssa_forecast_sensors_f64 / ssa_forecast_sensors_envs_f64).  by_value: the time words in
    the argument block"""
    eng, sp = make_engine(hip, sc, tabs)
    load(hip, eng, sc, [0] * sc.E if by_value else words, offset=0 if by_value else 1)
    kw = dict(out=("x_prior", "P_prior", "P_post"))
    if by_value:
        kw["env_times"] = [int(w) - 1 for w in words]
    if entry == "plain":
        res = eng.launch_lookahead(0, 1, **kw)
    elif entry == "sensors":
        assert not by_value
        res = eng.launch_lookahead_sensors(0, 1, sp, **kw) if n_steps is None else eng.launch_forecast_sensors(0, 1, sp, n_steps, **kw)
    else:
        res = eng.launch_lookahead_sensors_envs(0, 1, sp, **kw) if n_steps is None else \
            eng.launch_forecast_sensors_envs(0, 1, sp, n_steps, **kw)
    return il.read(hip.torch, res)


def run_step_sensors(hip, sc, tabs, words, propagator="hybrid", entry="sensors", by_value=False, interval=1, aer=0):
    """ssa_env_step_sensors_f64 ('sensors') / ssa_env_step_sensors_envs_f64 ('envs'): one step at `words`, sensor s of env e on sc.acts[e, s]"""
    torch, L = hip.torch, hip.lib
    eng, sp = make_engine(hip, sc, tabs, propagator, interval)
    S = sc.net.S
    upd = torch.zeros((sc.E, S, L.UPD_STRIDE), dtype=torch.float64, device="cuda")
    extra = {"upd": upd}
    kw = dict(fast_stats=True)
    if aer:
        extra["aer"] = torch.full((sc.E * sc.m * aer,), -7.0, dtype=torch.float64, device="cuda")
        kw.update(aer_out=extra["aer"].data_ptr(), aer_cols=aer)
    if entry == "sensors":
        load(hip, eng, sc, words, offset=1)
        eng.launch_step_sensors(0, 1, 1, sp, [int(a) for a in sc.acts[0]], upd.data_ptr(), fold_inside=True, **kw)
    elif by_value:
        load(hip, eng, sc, [0] * sc.E, offset=0)
        eng.launch_step_sensors_envs(0, 1, 0, sp, sc.acts, upd.data_ptr(), env_words=[int(w) for w in words], **kw)
    else:
        load(hip, eng, sc, words, offset=1)
        eng.launch_step_sensors_envs(0, 1, 1, sp, sc.acts, upd.data_ptr(), **kw)
    return capture(hip, eng, **extra)


def schedule(sc, K):
    """[K, E, S]: every sensor keeps its object at the even steps; at the odd ones the sensors swap objects (0 idle)"""
    a = sc.acts
    return np.array([a if k % 2 == 0 else np.stack([-np.ones_like(a[:, 0]), a[:, 2], a[:, 1]], axis=1) for k in range(K)])


def run_rollout_sensors(hip, sc, tabs, words, K, entry="sensors"):
    """ssa_env_rollout_sensors_f64 / ssa_env_rollout_sensors_envs_f64: K steps of schedule() from `words`"""
    eng, sp = make_engine(hip, sc, tabs)
    load(hip, eng, sc, words, offset=1)
    sched = schedule(sc, K)
    if entry == "sensors":
        eng.launch_rollout_sensors(0, 1, sp, _i32(hip, sched[:, 0]))
        return capture(hip, eng)
    stats, upd = eng.launch_rollout_sensors_envs(0, 1, sp, _i32(hip, sched), records=True)
    L = hip.lib
    return capture(hip, eng, upd=upd, roll_stats=stats[..., [L.STAT_MAX_DPOS, L.STAT_CNT_LT_1E4, L.STAT_CNT_LT_1E7, L.STAT_N_FAILED]])


def candidates(sc, K):
    """[E, B = 2, K, S]: schedule() and the same with steps reversed"""
    s = schedule(sc, K).transpose(1, 0, 2)
    return np.stack([s, s[:, ::-1]], axis=1)


def run_dryrun(hip, sc, tabs, words, K, form="gather"):
    """ssa_dryrun_sensors_envs_f64 from `words`: 'gather' / 'full' -- the engine's one-env call with and without the gathered block
    (full: one candidate); 'envs' -- launch_dryrun_sensors_envs with the engine's time words; 'envs_by_value' -- with env_times"""
    from support import dryrun
    eng, sp = make_engine(hip, sc, tabs)
    cand = candidates(sc, K)
    if form in ("gather", "full"):
        load(hip, eng, sc, words, offset=1)
        rec = eng.launch_dryrun_sensors(0, 1, sp, cand[0] if form == "gather" else cand[0, :1], gather=form == "gather")
    elif form == "envs":
        load(hip, eng, sc, words, offset=1)
        rec = eng.launch_dryrun_sensors_envs(0, 1, sp, cand)
    else:
        load(hip, eng, sc, [0] * sc.E, offset=0)
        rec = eng.launch_dryrun_sensors_envs(0, 1, sp, cand, env_times=[int(w) - 1 for w in words])
    return dryrun.record_bits(rec)


def run_chain(hip, sc, tabs, words):
    """the decision chain of step_agent: every env's lookahead, ssa_assign_sensors_envs_f64 into the action table, and the step that
    reads the table and the time words from device memory"""
    torch, L = hip.torch, hip.lib
    eng, sp = make_engine(hip, sc, tabs)
    load(hip, eng, sc, words, offset=1)
    look = eng.launch_lookahead_sensors_envs(0, 1, sp)
    table = eng.launch_assign_sensors_envs(look, L.LOOK_INFO_GAIN)
    upd = torch.zeros((sc.E, sc.net.S, L.UPD_STRIDE), dtype=torch.float64, device="cuda")
    eng.launch_step_sensors_envs(0, 1, 1, sp, None, upd.data_ptr(), fast_stats=True)
    return capture(hip, eng, upd=upd, table=table, visible=look["visible"], score=look["score"])


def run_closed_loop(hip, sc, tabs, i0, K, persistent, propagator="hybrid"):
    """the closed loop of one greedy agent (AGENT_VISIBLE_GREEDY) as the env enqueues it: the first decision from the state of step i0
    (slot i0 % H), then K steps with the time indices i0 + 1 .. i0 + K -- ssa_env_closed_loop_f64 (persistent) or step + decision
    launches"""
    torch, L = hip.torch, hip.lib
    eng, _ = make_engine(hip, sc, tabs, propagator)
    load(hip, eng, sc, [0], offset=0, slot=i0 % H)
    kind = L.AGENT_VISIBLE_GREEDY
    fb = _i32(hip, [(3 * k + 1) % sc.m for k in range(K + 1)])
    log = torch.full((K + 1,), -1, dtype=torch.int32, device="cuda")
    eng.launch_agent_select(i0, i0, kind, log.data_ptr(), fallback_ptr=fb.data_ptr(), have_prev=False)
    extra = {}
    if persistent:
        stats = torch.zeros((K, L.STAT_STRIDE), dtype=torch.float64, device="cuda")
        upd = torch.zeros((K, L.UPD_STRIDE), dtype=torch.float64, device="cuda")
        used = eng.launch_closed_loop(i0 % H, i0 + 1, kind, log, stats, upd, fallback=fb)
        torch.cuda.synchronize()
        assert used and int(eng.loop_error[0]) == 0, (used, "the persistent launch was declined or gave up")
        extra = dict(upd=upd, loop_stats=stats[:, [L.STAT_MAX_DPOS, L.STAT_CNT_LT_1E4, L.STAT_CNT_LT_1E7, L.STAT_N_FAILED]])
    else:
        for k in range(K):
            i = i0 + k + 1
            eng.launch_step((i - 1) % H, i % H, i, actions_ptr=log.data_ptr() + 4 * k, fast_stats=True, defer_fold=True)
            eng.launch_agent_select(i, i, kind, log.data_ptr() + 4 * (k + 1), fallback_ptr=fb.data_ptr() + 4 * (k + 1))
    return capture(hip, eng, log=log, **extra)


# ---------------------------------------------------------------------------------------------------------------- the anchors
def _wrap(d):
    return (np.asarray(d) + np.pi) % (2 * np.pi) - np.pi


def anchor_z_true(sc, oracle, rec, x_true, tix, L):
    """the SSA_UPD_Z_TRUE words of sensor 0's update record `rec` against oracle.hx_aer of the step's own truth `x_true` [6] under row
    tix % T of the SHORT trans table, at the bounds of tests/test_sensors_oracle_gpu.py (check_update): 1e-12 relative per component,
    the azimuth modulo 2 pi and to its conditioning over the horizontal distance"""
    net = sc.net
    zf = oracle.hx_aer(x_true[None], sc.tabs["trans"][tix % T], net.lla[0], net.itrs[0])[0]
    zt = rec[L.UPD_Z_TRUE:L.UPD_Z_TRUE + 3]
    assert abs(zf[1]) < NEAR_ZENITH
    dx = 4 * EPS * np.linalg.norm(x_true[:3])
    h = zf[2] * np.cos(zf[1])
    assert abs(_wrap(zt[0] - zf[0])) <= 1e-12 * 2 * np.pi + 2 * dx / h, (tix, zt, zf)
    assert abs(zt[1] - zf[1]) <= 1e-12 and abs(zt[2] - zf[2]) <= 1e-12 * zf[2], (tix, zt, zf)


def anchor_aer(sc, oracle, oracle_ld, aer, x_filter, tix):
    """the aer_out payload [m, 4] (az, el, range of the filter means x_filter [m, 6]) against oracle.hx_aer under row tix % T of the
    SHORT trans table, at the geometry bounds of tests/test_sensors_oracle_gpu.py (test_geometry_at_eight_sites, away from the zenith):
    elevation and azimuth 1e-13 rad (the azimuth: plus its conditioning), the range 1e-15 relative plus the rounding of the position"""
    net, M = sc.net, sc.tabs["trans"][tix % T]
    zf, zl = oracle.hx_aer(x_filter, M, net.lla[0], net.itrs[0]), oracle_ld.hx_aer(x_filter, M, net.lla[0], net.itrs[0])
    assert np.all(np.abs(zl[:, 1]) < NEAR_ZENITH)
    r = np.linalg.norm(x_filter[:, :3], axis=1)
    cond_az = 4 * EPS * r / (zl[:, 2] * np.cos(zl[:, 1]))
    assert np.abs(aer[:, 1] - zf[:, 1]).max() <= 1e-13 and np.all(np.abs(_wrap(aer[:, 0] - zf[:, 0])) <= 1e-13 + cond_az), tix
    assert np.all(np.abs(aer[:, 2] - zl[:, 2]) <= 1e-15 * zl[:, 2] + 4 * EPS * r), tix
