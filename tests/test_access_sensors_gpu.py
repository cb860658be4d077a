"""The pass table of a sensor network on the GPU, engine level (ssa_access_sensors_f64): the table and its
summary against the numpy statement (tests/support/access.py: the oracle's chain of truths judged by support.illumination /
support.orbiting) bit for bit, and against the project's own kernels -- the forecast's visibility and the record a real step leaves --
for every propagator; several envs with their own time words, a storage layout, a selection of envs, n_left, a NaN truth, the
feature's tables unread while no sensor asks for them, and nothing of the engine written.
Objects: rows of tests/golden/catalogue_subset.npy, m = 6 (a partial wavefront) and m = 65 (a second wavefront with one live lane);
T = 1, 64, 65 and 70 steps on 16-row tables (the index wraps four times, a word boundary is crossed); the two test networks: three
ground sites with sunlit_only = 0b110, and a ground radar with two sensors in orbit.  Every judged cell keeps its margins in the
oracle's chain -- elevation 1e-6 rad from the mask, support.illumination.assert_margins, support.orbiting.assert_margins -- asserted by
the scenes before anything is compared; no cell is left out."""
import ctypes as C

import numpy as np
import pytest

from support import access as ac
from support import angles_only as ao
from support import illumination as il
from support import orbiting as ob
from support.gpu import hip  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

T0, T1 = 3, 9                      # the time words of env 0 and env 1
STEPS = (1, 64, 65, 70)
ROWS = {6: ac.ROWS6, 65: ac.ROWS65}
_SCENES = {}


def _scene(oracle, kind, m, t0, flip=False):
    """the scene `kind` ('ground' / 'orbit') on the m chosen rows (flip: in reverse order, another env's objects) from time word t0, made
    once: dict(net, xt, sun, dark, rows (site rows or None), acc [70, S, m])"""
    key = (kind, m, t0, flip)
    if key not in _SCENES:
        rows = ROWS[m][::-1] if flip else ROWS[m]
        if kind == "ground":
            net, xt, sun, dark, acc = ac.ground_scene(oracle, rows, t0)
            site = None
        else:
            net, xt, site, sun, dark, acc = ac.orbit_scene(oracle, rows, t0)
        assert acc.any(axis=(0, 2)).all() and not acc.all(axis=(0, 2)).any(), acc.sum(axis=(0, 2))      # every sensor sees something, none everything
        acc.setflags(write=False)
        _SCENES[key] = dict(net=net, xt=xt, sun=sun, dark=dark, rows=site, acc=acc)
    return _SCENES[key]


def _engine(hip, kind, sc, m, propagator="hybrid", E=1):
    if kind == "ground":
        eng, sp, _ = il.make_engine(hip, sc["net"], m, sc["sun"], sc["dark"], propagator, E=E)
    else:
        eng, sp, _ = ob.make_engine(hip, sc["net"], m, sc["rows"], sc["sun"], sc["dark"], propagator, E=E)
    return eng, sp


def _filters(xt, seed=5):
    """consistent filters for the truths xt [n, 6]: the estimates and covariances a step or a forecast needs (the table reads neither)"""
    rs = np.random.RandomState(seed)
    return xt + rs.normal(size=xt.shape) * ao.X_SIGMA, np.tile(np.diag(ao.X_SIGMA ** 2), (len(xt), 1, 1))


def _load(eng, xt):
    x, P = _filters(xt)
    eng.load_state(0, xt, x, P)
    eng.status.zero_()


def _table(hip, eng, sp, T, t0=T0, **kw):
    """one launch from slot 0; (bits, pass) as numpy copies"""
    r = eng.launch_access_sensors(0, t0, sp, T, **kw)
    hip.torch.cuda.synchronize()
    return r["bits"].cpu().numpy().copy(), None if r["pass"] is None else r["pass"].cpu().numpy().copy()


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:6].tolist())


# ---------------------------------------------------------------------------------------------------------------- 1. the statement
@pytest.mark.parametrize("m", [6, 65])
@pytest.mark.parametrize("kind", ["ground", "orbit"])
@pytest.mark.parametrize("propagator", ["fg", "hybrid"])
def test_bits_and_pass_are_the_numpy_statement(hip, oracle, propagator, kind, m):
    sc = _scene(oracle, kind, m, T0)
    eng, sp = _engine(hip, kind, sc, m, propagator)
    _load(eng, sc["xt"])
    for T in STEPS:
        bits, summ = _table(hip, eng, sp, T)
        assert bits.shape == (1, 3, m, (T + 63) // 64) and summ.shape == (1, 3, m, 4) and summ.dtype == np.int32
        acc = sc["acc"][:T]
        _same(bits[0], ac.pack(acc), ("bits", T))
        _same(summ[0], ac.summary(acc), ("pass", T))
        # the device's own readers of the table
        un = hip.dev.access_unpack(eng._access["bits"], T).cpu().numpy()
        assert un.shape == (1, 3, m, T) and np.array_equal(np.moveaxis(un[0], -1, 0), acc)
        for k in sorted({0, T // 2, T - 1}):
            assert np.array_equal(hip.dev.access_mask(eng._access["bits"], k).cpu().numpy()[0], acc[k]), (T, k)
    # (summary=False: the table alone)
    r = eng.launch_access_sensors(0, T0, sp, 70, summary=False)
    hip.torch.cuda.synchronize()
    assert r["pass"] is None and np.array_equal(r["bits"].cpu().numpy()[0], ac.pack(sc["acc"]))


# ---------------------------------------------------------------------------------------------------------------- 2. the project's own kernels
@pytest.mark.parametrize("kind,m", [("ground", 6), ("orbit", 6), ("ground", 65)])
@pytest.mark.parametrize("propagator", ["fg", "elements", "j2", "hybrid"])
def test_the_table_is_the_forecasts_visibility_and_the_steps_record(hip, oracle, propagator, kind, m):
    """h below the forecast's horizon: visible[h, s, j] of ssa_forecast_sensors_f64 (no filter fails inside it); beyond: SSA_UPD_VISIBLE
    of the record a real step leaves when the step at h tasks object h mod m from each sensor in turn, along a stepped chain of 20"""
    torch, L = hip.torch, hip.lib
    H, K = 4, 20
    sc = _scene(oracle, kind, m, T0)
    eng, sp = _engine(hip, kind, sc, m, propagator)
    _load(eng, sc["xt"])
    bits, _ = _table(hip, eng, sp, K)
    acc = ac.unpack(bits[0], K)                                   # [K, S, m]
    if propagator in ("fg", "hybrid"):
        assert np.array_equal(acc, sc["acc"][:K])
    fc = il.read(torch, eng.launch_forecast_sensors(0, T0, sp, H))
    assert not fc["status"].any()
    assert np.array_equal(fc["visible"].astype(bool), acc[:H]), np.argwhere(fc["visible"].astype(bool) != acc[:H])[:6].tolist()
    for h in range(K):
        j = h % m
        for s in range(3):      # (each from the same slot; the last one's output is the chain's next state: the truth is the same in all)
            one = il.step(hip, eng, sp, None, T0 + h, [j if q == s else -1 for q in range(3)], slot=h % 2)
            assert one["upd"][s, L.UPD_ACTION] == j and not one["st"].any(), (h, s, one["upd"][s, L.UPD_ACTION])
            assert one["upd"][s, L.UPD_VISIBLE] == float(acc[h, s, j]), (h, s, j)
            assert one["upd"][s, L.UPD_OBS_TAKEN] == float(acc[h, s, j])


# ---------------------------------------------------------------------------------------------------------------- 3. several envs
def _two_envs(hip, oracle, kind, m, propagator="hybrid"):
    """an engine of two envs -- env 0 the chosen rows from time word T0, env 1 the same rows in reverse from T1 --, its block, and the
    two scenes"""
    a, b = _scene(oracle, kind, m, T0), _scene(oracle, kind, m, T1, flip=True)
    eng, sp = _engine(hip, kind, a, m, propagator, E=2)
    _load(eng, np.concatenate([a["xt"], b["xt"]]))
    return eng, sp, a, b


@pytest.mark.parametrize("kind,m", [("ground", 6), ("orbit", 65)])
def test_two_envs_are_two_one_env_launches(hip, oracle, kind, m):
    eng, sp, a, b = _two_envs(hip, oracle, kind, m)
    bits, summ = _table(hip, eng, sp, 70, t0=0, env_times=[T0, T1])
    for e, (sc, t0) in enumerate(((a, T0), (b, T1))):
        one, sp1 = _engine(hip, kind, sc, m)
        _load(one, sc["xt"])
        b1, s1 = _table(hip, one, sp1, 70, t0=t0)
        _same(bits[e], b1[0], ("bits", e))
        _same(summ[e], s1[0], ("pass", e))
        _same(bits[e], ac.pack(sc["acc"]), ("statement", e))
    # the words from memory instead of by value
    eng.env_time0.copy_(hip.torch.as_tensor([T0, T1], dtype=hip.torch.int32))
    b2, s2 = _table(hip, eng, sp, 70, t0=0)
    _same(b2, bits, "env_time from memory")
    _same(s2, summ, "env_time from memory")
    # ... and with time_offset added to them
    eng.env_time0.copy_(hip.torch.as_tensor([T0 - 2, T1 - 2], dtype=hip.torch.int32))
    b3, _ = _table(hip, eng, sp, 70, t0=2)
    _same(b3, bits, "time_offset")


@pytest.mark.parametrize("kind,m", [("ground", 65), ("orbit", 6)])
def test_a_selection_writes_its_envs_slabs_alone(hip, oracle, kind, m):
    torch = hip.torch
    eng, sp, a, b = _two_envs(hip, oracle, kind, m)
    bits, summ = _table(hip, eng, sp, 70, t0=0, env_times=[T0, T1])
    for t in eng._access.values():
        t.view(torch.uint8).fill_(0xA5)
    b1, s1 = _table(hip, eng, sp, 70, t0=0, env_times=[T0, T1], envs=[1])
    _same(b1[1], bits[1], "env 1's bits")
    _same(s1[1], summ[1], "env 1's pass")
    assert (b1[0].view(np.uint8) == 0xA5).all() and (s1[0].view(np.uint8) == 0xA5).all()
    # a selection on the device, every env named, in another order: the full table
    sel = torch.as_tensor([1, 0], dtype=torch.int32, device="cuda")
    b2, s2 = _table(hip, eng, sp, 70, t0=0, env_times=[T0, T1], envs=sel)
    _same(b2, bits, "both envs selected")
    _same(s2, summ, "both envs selected")


@pytest.mark.parametrize("kind,m", [("ground", 6), ("orbit", 65)])
def test_n_left_ends_an_envs_steps(hip, oracle, kind, m):
    torch = hip.torch
    eng, sp, a, b = _two_envs(hip, oracle, kind, m)
    left = torch.as_tensor([3, 70], dtype=torch.int32, device="cuda")
    bits, summ = _table(hip, eng, sp, 70, t0=0, env_times=[T0, T1], n_left=left)
    assert not ac.unpack(bits[0], 70)[3:].any()
    _same(bits[0], ac.pack(ac.cut(a["acc"], 3)), "env 0's bits")
    _same(summ[0], ac.summary(a["acc"][:3]), "env 0's pass is over three steps")
    _same(bits[1], ac.pack(b["acc"]), "env 1's bits")
    _same(summ[1], ac.summary(b["acc"]), "env 1's pass")
    # (a word at or below zero counts no step; one beyond T counts T)
    left = torch.as_tensor([-4, 1000], dtype=torch.int32, device="cuda")
    bits, summ = _table(hip, eng, sp, 70, t0=0, env_times=[T0, T1], n_left=left)
    assert not bits[0].any() and summ[0].reshape(-1, 4).tolist() == [[-1, 0, 0, 0]] * (3 * m)
    _same(bits[1], ac.pack(b["acc"]), "env 1's bits")


# ---------------------------------------------------------------------------------------------------------------- 4. a layout never shows
@pytest.mark.parametrize("kind,m", [("ground", 65), ("orbit", 6)])
def test_a_storage_layout_never_shows(hip, oracle, kind, m):
    sc = _scene(oracle, kind, m, T0)
    eng, sp = _engine(hip, kind, sc, m)
    eng.set_layout(np.random.RandomState(m).permutation(m))
    _load(eng, sc["xt"])
    assert eng._order is not None and not np.array_equal(eng._order, np.arange(m))
    bits, summ = _table(hip, eng, sp, 70)
    _same(bits[0], ac.pack(sc["acc"]), "bits")
    _same(summ[0], ac.summary(sc["acc"]), "pass")


# ---------------------------------------------------------------------------------------------------------------- 5. a NaN truth
@pytest.mark.parametrize("kind,m", [("ground", 6), ("orbit", 65)])
def test_a_nan_truth_is_never_seen(hip, oracle, kind, m):
    sc = _scene(oracle, kind, m, T0)
    eng, sp = _engine(hip, kind, sc, m)
    j = 2
    xt = sc["xt"].copy()
    xt[j, 1] = np.nan
    _load(eng, xt)
    bits, summ = _table(hip, eng, sp, 70)
    assert not bits[0, :, j].any() and summ[0, :, j].tolist() == [[-1, 0, 0, 0]] * 3
    keep = np.arange(m) != j
    _same(bits[0][:, keep], ac.pack(sc["acc"])[:, keep], "the neighbours' bits")
    _same(summ[0][:, keep], ac.summary(sc["acc"])[:, keep], "the neighbours' pass")


# ---------------------------------------------------------------------------------------------------------------- 6. the rules unread unless asked for
@pytest.mark.parametrize("m", [6, 65])
def test_no_bit_set_no_table_read(hip, oracle, m):
    """sunlit_only == 0 with `sun` pointing at NaNs and a NaN shadow radius, site_moving == 0 with `site_rows` pointing at NaNs and a NaN
    limb radius: the table of the clean block -- which is the three ground sites' elevation masks alone"""
    torch = hip.torch
    sc = _scene(oracle, "ground", m, T0)
    eng, sp = _engine(hip, "ground", sc, m)
    _load(eng, sc["xt"])
    nans = torch.full((ac.N_TIME * 3 * 16,), float("nan"), dtype=torch.float64, device="cuda")
    assert nans.data_ptr() % 128 == 0

    def run(spoiled):
        p = eng._lookahead_params(0, T0)
        s = type(sp)()
        C.memmove(C.byref(s), C.byref(sp), C.sizeof(s))
        s.sunlit_only, s.sun, s.shadow_radius = 0, 0, 0.0
        p.site_moving, p.site_rows, p.limb_radius = 0, 0, 0.0
        if spoiled:
            s.sun, s.shadow_radius = nans.data_ptr(), float("nan")
            p.site_rows, p.limb_radius = nans.data_ptr(), float("nan")
        bits, summ = hip.dev.access_sensors(eng.consts, p, s, 70, summary=True)
        torch.cuda.synchronize()
        return bits.cpu().numpy(), summ.cpu().numpy()
    clean, spoiled = run(False), run(True)
    _same(spoiled[0], clean[0], "bits")
    _same(spoiled[1], clean[1], "pass")
    from support.batches import c2t
    net = sc["net"]
    tr = ac.truths(oracle, sc["xt"], 70)
    want = np.array([[oracle.hx_aer(tr[h], c2t()[(T0 + h) % ac.N_TIME], net.lla[s], net.itrs[s])[:, 1] >= net.lim[s] for s in range(3)]
                     for h in range(70)])
    _same(clean[0][0], ac.pack(want), "the masks alone")
    assert (want & ~sc["acc"]).any()                            # (the night and the shadow do take cells away in the scene)


# ---------------------------------------------------------------------------------------------------------------- 7. nothing written
def test_nothing_of_the_engine_is_written(hip, oracle):
    torch = hip.torch
    eng, sp, a, b = _two_envs(hip, oracle, "orbit", 6)
    eng.status[3] = 2                                             # (a failed filter: the table does not know it)
    names = ("x_true", "x_filter", "P_filter", "obs", "metrics", "stats", "upd", "status", "fail_count", "time_actions", "z_noise",
             "stat_shards")
    torch.cuda.synchronize()
    before = {k: getattr(eng, k).clone() for k in names}
    bits, _ = _table(hip, eng, sp, 70, t0=0, env_times=[T0, T1])
    for k in names:
        assert torch.equal(getattr(eng, k).view(torch.uint8), before[k].view(torch.uint8)), k
    _same(bits[0], ac.pack(a["acc"]), "a failed filter is not masked out")
