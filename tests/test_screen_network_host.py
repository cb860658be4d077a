"""The catalogue screen by a network's own rule, without a GPU (include/ssa_hip.h: ssa_catalogue_screen_network_f64;
catalogue.visible_catalogue_network and catalogue_for_network): the ABI struct against its ctypes mirror, the numpy rule on crafted
geometry, every ValueError of the two Python functions and every refusal of the C entry before any launch, the mapping of an
env_config dict, and -- for every input set tests/test_screen_network_gpu.py uses -- that numpy's own decisions have margin and that
the scenes deliver what the GPU tests assert on."""
import ctypes as C
import os
import subprocess
from datetime import datetime

import numpy as np
import pytest

from conftest import ROOT
from support import illumination as il
from support import orbiting as ob
from support import screen_network as sn
from support.codeobj import header
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.screen import _SITES3, screen_numpy, site_rows


# ---------------------------------------------------------------------------------------------------------------- 1. the ABI
def test_network_params_layout_matches_the_header(tmp_path):
    """ssa_screen_network_params: sizeof / offsetof with gcc against the ctypes mirror, `base` first and whole; ABI 23; the entry bound"""
    import re
    from ssa_gym_amd import _lib
    st = _lib.ssa_screen_network_params
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssa_hip.h"', 'int main(void){',
           'printf("%zu\\n", sizeof(ssa_screen_network_params));', 'printf("%zu\\n", sizeof(((ssa_screen_network_params *)0)->base));',
           'printf("%zu\\n", sizeof(ssa_screen_params));', 'printf("%d\\n", SSA_ABI_VERSION);']
    want = [C.sizeof(st), C.sizeof(_lib.ssa_screen_params), C.sizeof(_lib.ssa_screen_params), 23]
    for f, _ in st._fields_:
        src.append('printf("%%zu\\n", offsetof(ssa_screen_network_params, %s));' % f)
        want.append(getattr(st, f).offset)
    src.append('return 0;}')
    c = tmp_path / "screen_network_layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "screen_network_layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).decode().split()] == want
    assert st.base.offset == 0 and _lib.ABI_VERSION == 23
    assert re.search(r"\bint ssa_catalogue_screen_network_f64\s*\(const ssa_screen_network_params \*p, void \*stream\);", header())
    assert "ssa_catalogue_screen_network_f64" in _lib.SIGNATURES


# ---------------------------------------------------------------------------------------------------------------- 2. the numpy rule
GEO = np.array([42164e3, 0.0, 0.0])


def _one(r, **kw):
    """the rule for ONE candidate that stands at the inertial position r at sample 0 (a circular orbit through r; T = 1, identity
    rotation): (accept, seen_by) with one sample, first window 1"""
    r = np.asarray(r, dtype=np.float64)
    a = np.linalg.norm(r)
    u = r / a
    lon, lat = np.arctan2(u[1], u[0]), np.arcsin(u[2])
    inc, raan, argp = np.pi / 2, lon, lat          # a polar orbit with its node at lon: P = (cos lon cos lat, sin lon cos lat, sin lat) = u
    cand = tuple(np.array([v]) for v in (a, 0.0, inc, raan, argp, 0.0))
    args = dict(M_t=np.eye(3)[None], times=np.zeros(1), first=1, max_gap=1, min_alt=-1e9)
    args.update(kw)
    acc, _, _, seen = sn.screen_network_numpy(cand, args.pop('M_t'), args.pop('times'), args.pop('sites'), args.pop('first'),
                                              args.pop('max_gap'), **args)
    return bool(acc[0]), int(seen[0])


def test_the_numpy_rule_on_crafted_geometry():
    """behind the Earth from the orbiting sensor; in shadow; a site that is not dark; a 'sunlit' orbiting sensor that ignores the dark
    word; a NaN that gives not visible"""
    site = site_rows([(0.0, 0.0, 0.0)], [10.0])      # on the equator under GEO: the candidate at GEO stands in its zenith
    unread = [(np.full((3, 3), np.nan), np.full(3, np.nan), np.nan)]
    sun_side, anti = np.array([[1.0, 0.0, 0.0]]), np.array([[-1.0, 0.0, 0.0]])
    # the position code puts the candidate where it is meant to be: the ground site sees it in its zenith
    assert _one(GEO, sites=site) == (True, 1)
    # an orbiting sensor below the candidate sees it; on the far side of the Earth it does not
    for o, want in ((ob.below(GEO), (True, 1)), (ob.behind(GEO), (False, 0))):
        assert _one(GEO, sites=unread, obs=o[None, None], site_moving=1) == want
    # ... and a larger limb sphere blocks a line of sight that clears the smaller one
    o = ob.LEO * il.unit(np.array([0.0, 1.0, 0.0]))          # 90 degrees round the Earth: the line passes 7 100 km from the geocentre
    assert _one(GEO, sites=unread, obs=o[None, None], site_moving=1, limb_radius=7.0e6) == (True, 1)
    assert _one(GEO, sites=unread, obs=o[None, None], site_moving=1, limb_radius=7.2e6) == (False, 0)
    # in shadow (the Sun opposite: the candidate on the axis of the cylinder), lit from its own side
    for sun, lit in ((sun_side, True), (anti, False)):
        assert _one(GEO, sites=site, sun=sun, dark=np.array([1]), sunlit_only=1) == (lit, int(lit))
    # a telescope whose site is not dark sees nothing, whatever the Sun does for the object
    assert _one(GEO, sites=site, sun=sun_side, dark=np.array([0]), sunlit_only=1) == (False, 0)
    # a 'sunlit' orbiting sensor never reads the dark word
    assert _one(GEO, sites=unread, obs=ob.below(GEO)[None, None], site_moving=1, sun=sun_side, dark=np.array([0]), sunlit_only=1) == (True, 1)
    assert _one(GEO, sites=unread, obs=ob.below(GEO)[None, None], site_moving=1, sun=anti, dark=np.array([1]), sunlit_only=1) == (False, 0)
    # two sensors: seen_by tells which
    two = site + unread
    assert _one(GEO, sites=two, obs=np.stack([np.zeros(3), ob.below(GEO)])[None], site_moving=2, sun=anti, dark=np.array([3]),
                sunlit_only=1) == (True, 2)
    # a NaN anywhere: not visible -- the sensor's position, the Sun, the candidate itself
    nan = np.full(3, np.nan)
    assert _one(GEO, sites=unread, obs=nan[None, None], site_moving=1) == (False, 0)
    assert _one(GEO, sites=site, sun=nan[None], dark=np.array([1]), sunlit_only=1) == (False, 0)
    assert _one(GEO * np.array([1.0, np.nan, 1.0]), sites=site) == (False, 0)


def test_zero_bits_is_screen_numpy():
    """with site_moving == sunlit_only == 0 the network rule is support.screen.screen_numpy bit for bit, tables or none"""
    sc = sn.scene('S3', 96)
    cand = sn.candidates(4099)
    sites = site_rows(_SITES3, [15.0, 10.0, 20.0])
    want = screen_numpy(*cand, sc['M_t'], sc['times'], sites, sc['first'], sc['max_gap'])
    for kw in (dict(), dict(obs=np.full_like(sc['obs'], np.nan), sun=np.full_like(sc['sun'], np.nan), dark=sc['dark'])):
        got = sn.screen_network_numpy(cand, sc['M_t'], sc['times'], sites, sc['first'], sc['max_gap'], **kw)
        assert all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3]))
        assert np.array_equal(got[3] != 0, (want[2] & 2 != 0) | (want[1] < 96))      # seen by someone <=> visible at some sample
    el, alt, sh, limb = sn.screen_network_margins(cand, sc['M_t'], sc['times'], sites, sc['first'], sc['max_gap'])
    assert np.array_equal(el, want[3]) and np.array_equal(alt, want[4]) and np.all(np.isinf(sh)) and np.all(np.isinf(limb))


# ---------------------------------------------------------------------------------------------------------------- 3. the Python layer
ORBIT = {'orbit': [ob.LEO, 0.0, 0.0, 0.0, 7.4e3, 0.0]}


@pytest.mark.parametrize("kw", [
    dict(sensors=[]),
    dict(sensors=[(0.0, 0.0, 0.0)] * 9),
    dict(sensors=ORBIT),
    dict(sensors=[{'orbit': ORBIT['orbit'], 'name': 'x'}]),
    dict(sensors=[{'orbit': ORBIT['orbit'][:5]}]),
    dict(sensors=[{'orbit': [float("nan")] + ORBIT['orbit'][1:]}]),
    dict(sensors=[(0.0, 0.0)]),
    dict(sensors=[(float("inf"), 0.0, 0.0)]),
    dict(sensors=[_SITES3[0], ORBIT], el_min_deg=[15.0, 10.0]),
    dict(sensors=[_SITES3[0], ORBIT], el_min_deg=[None, None]),
    dict(sensors=[_SITES3[0], ORBIT], el_min_deg=[15.0]),
    dict(sensors=[_SITES3[0], ORBIT], el_min_deg=[float("nan"), None]),
    dict(sensors=[_SITES3[0], ORBIT], el_min_deg=None),
    dict(sensors=[_SITES3[0], ORBIT], illumination=[None]),
    dict(sensors=[_SITES3[0], ORBIT], illumination='sunlit'),
    dict(sensors=[_SITES3[0], ORBIT], illumination=[None, -6.0]),
    dict(sensors=[_SITES3[0], ORBIT], illumination=['sunlit', None]),
    dict(sensors=[_SITES3[0], ORBIT], illumination=[-91.0, None]),
    dict(sensors=[_SITES3[0], ORBIT], illumination=[True, None]),
    dict(sensors=[_SITES3[0], ORBIT], limb_radius=-1.0),
    dict(sensors=[_SITES3[0], ORBIT], limb_radius=float("nan")),
    dict(sensors=[_SITES3[0], ORBIT], limb_radius=ob.LEO + 1.0),                       # the orbit starts inside the sphere
    dict(sensors=[_SITES3[0], ORBIT], illumination=[-6.0, None], shadow_radius=-1.0),
    dict(sensors=[_SITES3[0], ORBIT], illumination=[-6.0, None], sun_table=np.zeros((95, 3))),
    dict(sensors=[_SITES3[0], ORBIT], illumination=[None, 'sunlit'], sun_table=np.zeros((96, 4))),
    dict(sensors=[_SITES3[0]], step=0.0),
    dict(sensors=[_SITES3[0]], step=-150.0),
    dict(sensors=[_SITES3[0]], duration=100.0),
    dict(sensors=[_SITES3[0]], first_window=-1.0),
    dict(sensors=[_SITES3[0]], n=-1),
])
def test_visible_catalogue_network_rejects_bad_arguments_before_any_launch(kw, monkeypatch):
    from ssa_gym_amd import catalogue, device
    monkeypatch.setattr(device, "catalogue_screen_network", lambda *a, **k: pytest.fail("launched"))
    monkeypatch.setattr(device, "propagate", lambda *a, **k: pytest.fail("launched"))
    kw = dict(kw)
    with pytest.raises(ValueError):
        catalogue.visible_catalogue_network(kw.pop('n', 10), 0, **kw)


@pytest.mark.parametrize("fault,words", [("nan", "propagation fails at sample 3"), ("dip", "dips to")])
def test_an_orbit_that_fails_or_dips_is_refused(fault, words, monkeypatch):
    """the orbit table's own refusals, with the device's propagator replaced (no GPU): a NaN position at some sample, a position below
    limb_radius at some sample -- ValueError naming the sensor, before any screen launch"""
    import torch
    from ssa_gym_amd import catalogue, device
    calls = []

    def propagate(x, dt):
        calls.append(dt)
        out = x.clone()
        if len(calls) == 3:
            out[:, :3] = float("nan") if fault == "nan" else out[:, :3] * 0.5
        return out
    monkeypatch.setattr(device, "as_dev", lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64))
    monkeypatch.setattr(device, "propagate", propagate)
    with pytest.raises(ValueError, match=r"sensors\[1\].*" + words):
        catalogue._orbit_positions([None, np.array(ORBIT['orbit'])], 150.0, 8, ob.R_LIMB)
    assert calls == [150.0] * 7
    # a sound orbit: the positions of the orbiting sensor, zeros in the ground site's place
    monkeypatch.setattr(device, "propagate", lambda x, dt: x.clone())
    pos = catalogue._orbit_positions([None, np.array(ORBIT['orbit'])], 150.0, 8, ob.R_LIMB)
    assert pos.shape == (8, 2, 3) and not pos[:, 0].any() and np.array_equal(pos[:, 1], np.tile(ORBIT['orbit'][:3], (8, 1)))


def test_visible_catalogue_network_needs_its_sensors():
    from ssa_gym_amd import catalogue
    with pytest.raises(TypeError):
        catalogue.visible_catalogue_network(10)


def test_catalogue_for_network_maps_the_config(monkeypatch):
    """observers (else observer) with the orbiting ones kept, the masks, the illumination, both radii and the epoch; keyword arguments
    override; and the sun_table rule"""
    from ssa_gym_amd import catalogue
    from ssa_gym_amd import envs as E
    seen = []
    monkeypatch.setattr(catalogue, "visible_catalogue_network", lambda n, seed=0, **kw: seen.append((n, seed, kw)))
    t0 = datetime(2012, 6, 1)
    cfg = ob.orbit_cfg(E, t_0=t0, limb_radius=6.6e6, shadow_radius=6.4e6)
    catalogue.catalogue_for_network(cfg, n=500, seed=4)
    n, seed, kw = seen[-1]
    assert (n, seed) == (500, 4) and set(kw) == {'sensors', 'el_min_deg', 'illumination', 'limb_radius', 'shadow_radius', 't_0'}
    assert kw['sensors'] == [tuple(cfg['observers'][0]), cfg['observers'][1], cfg['observers'][2]]
    assert kw['el_min_deg'] == list(cfg['sensor_obs_limit']) and kw['el_min_deg'][1:] == [None, None]
    assert kw['illumination'] == [None, None, 'sunlit'] and kw['limb_radius'] == 6.6e6 and kw['shadow_radius'] == 6.4e6 and kw['t_0'] == t0
    # a network without per-sensor masks, radii or illumination: the defaults of visible_catalogue_network stay in force
    catalogue.catalogue_for_network(dict(observers=_SITES3[:2], obs_limit=-90, t_0=t0))
    assert seen[-1] == (20000, 0, dict(sensors=_SITES3[:2], t_0=t0))
    # a single observer: not the env's obs_limit
    catalogue.catalogue_for_network(dict(observer=(1.0, 2.0, 3.0), obs_limit=-90), n=7)
    assert seen[-1] == (7, 0, dict(sensors=[(1.0, 2.0, 3.0)]))
    # the env's own default config
    catalogue.catalogue_for_network(E.env_config, n=3)
    assert seen[-1] == (3, 0, dict(sensors=[tuple(E.env_config['observer'])], t_0=E.env_config['t_0']))
    # keyword arguments override what the config says, and pass through
    catalogue.catalogue_for_network(cfg, n=9, el_min_deg=[5.0, None, None], step=120.0, t_0=datetime(2019, 1, 1), limb_radius=6.5e6)
    assert seen[-1][2]['el_min_deg'] == [5.0, None, None] and seen[-1][2]['step'] == 120.0 and seen[-1][2]['t_0'] == datetime(2019, 1, 1)
    assert seen[-1][2]['limb_radius'] == 6.5e6 and seen[-1][2]['shadow_radius'] == 6.4e6
    # config['sun_table'] stands on the env's rows: refused unless the caller gives the screen's own
    table = np.tile([1.0, 0.0, 0.0], (16, 1))
    before = len(seen)
    with pytest.raises(ValueError):
        catalogue.catalogue_for_network(dict(cfg, sun_table=table), n=5)
    assert len(seen) == before
    mine = np.tile([0.0, 1.0, 0.0], (96, 1))
    catalogue.catalogue_for_network(dict(cfg, sun_table=table), n=5, sun_table=mine)
    assert seen[-1][2]['sun_table'] is mine


def test_the_pinned_functions_keep_their_words():
    import inspect
    from ssa_gym_amd import catalogue
    assert "GROUND sites only" in catalogue.catalogue_for_config.__doc__ and "catalogue_for_network" in catalogue.catalogue_for_config.__doc__
    sig = inspect.signature(catalogue.visible_catalogue_network).parameters
    assert [k for k in sig] == ['n', 'seed', 'sensors', 'el_min_deg', 'illumination', 't_0', 'step', 'duration', 'first_window', 'max_gap',
                                'min_altitude', 'limb_radius', 'shadow_radius', 'sun_table']
    assert sig['sensors'].kind is inspect.Parameter.KEYWORD_ONLY and sig['sensors'].default is inspect.Parameter.empty
    from ssa_gym_amd import host
    assert sig['limb_radius'].default == host.R_EQ_EARTH + 100e3 and sig['shadow_radius'].default == host.R_EQ_EARTH
    assert "two-body" in catalogue.visible_catalogue_network.__doc__.lower()


# ---------------------------------------------------------------------------------------------------------------- 4. the C entry
PTR, SITE_PTR, SUN_PTR = 0x1000, ob.SITE_PTR, il.SUN_PTR


def _block(n=8, **over):
    """a block that passes every check (its pointers are never dereferenced: with n > 0 only refusals are asked for)"""
    from ssa_gym_amd import _lib
    q = _lib.ssa_screen_network_params(site_rows=SITE_PTR, sun=SUN_PTR, limb_radius=ob.R_LIMB, shadow_radius=il.R_SHADOW, site_moving=0b101,
                                       sunlit_only=0b110, seen_by=PTR, reserved=0)
    q.base = _lib.ssa_screen_params(n=n, n_time=96, n_site=3, step=150.0, min_alt=300e3, first=18, max_gap=36, elements=PTR, trans=PTR,
                                    sites=PTR, accept=PTR, worst_gap=PTR, flags=PTR)
    for k, v in over.items():
        setattr(q.base if hasattr(q.base, k) else q, k, v)
    return q


OLD_REFUSALS = [dict(n=-1), dict(n_time=0), dict(n_site=0), dict(n_site=9), dict(first=-1), dict(elements=None), dict(trans=None),
                dict(sites=None), dict(accept=None)]
NEW_REFUSALS = [dict(reserved=1), dict(site_moving=0b1000), dict(site_moving=-2 ** 31), dict(site_rows=None), dict(site_rows=SITE_PTR + 64),
                dict(limb_radius=-1.0), dict(limb_radius=float("nan")), dict(sunlit_only=0b1000), dict(sun=None), dict(sun=SUN_PTR + 16),
                dict(shadow_radius=-1.0), dict(shadow_radius=float("nan"))]


def test_the_entry_refuses_before_any_launch(lib):
    """every refusal of ssa_catalogue_screen_f64 on `base`, then the new ones in the header's order -- each alone, and each behind every
    refusal of the old entry (the answer stays a refusal, nothing launches); n == 0 launches nothing"""
    from ssa_gym_amd import _lib
    fn, old = lib.ssa_catalogue_screen_network_f64, lib.ssa_catalogue_screen_f64
    assert fn(None, None) == _lib.E_INVALID
    for bad in OLD_REFUSALS:
        assert fn(C.byref(_block(**bad)), None) == _lib.E_INVALID, bad
        assert old(C.byref(_block(**bad).base), None) == _lib.E_INVALID, bad
    for bad in NEW_REFUSALS:
        assert fn(C.byref(_block(**bad)), None) == _lib.E_INVALID, bad
        assert fn(C.byref(_block(n=0, **bad)), None) == _lib.E_INVALID, bad          # (a refusal also where nothing would launch)
        for first in OLD_REFUSALS:
            assert fn(C.byref(_block(**dict(bad, **first))), None) == _lib.E_INVALID, (first, bad)
    # n == 0: nothing launched (these pointers could not be launched with), and every sensor bit allowed -- bit 0 of site_moving too
    assert fn(C.byref(_block(n=0)), None) == 0
    assert fn(C.byref(_block(n=0, site_moving=0b111, sunlit_only=0b111)), None) == 0
    assert fn(C.byref(_block(n=0, n_site=8, site_moving=0xff, sunlit_only=0xff)), None) == 0
    # what a word does not ask for is not checked: no bits, no tables, any radius
    assert fn(C.byref(_block(n=0, site_moving=0, site_rows=None, limb_radius=float("nan"))), None) == 0
    assert fn(C.byref(_block(n=0, sunlit_only=0, sun=None, shadow_radius=-1.0)), None) == 0
    assert fn(C.byref(_block(n=0, seen_by=None, worst_gap=None, flags=None)), None) == 0
    # with n == 0 the old entry's pointer refusals do not apply, as in the old entry
    assert fn(C.byref(_block(n=0, elements=None, trans=None, sites=None, accept=None)), None) == 0
    assert old(C.byref(_block(n=0, elements=None, trans=None, sites=None, accept=None).base), None) == 0


# ---------------------------------------------------------------------------------------------------------------- 5. the GPU module's inputs
@pytest.mark.parametrize("kind", ["S1", "S3", "S8"])
@pytest.mark.parametrize("T", sn.SIZES_T)
def test_the_gpu_inputs_have_margin(kind, T):
    """numpy's own decisions on every input set of the GPU module: fewer than 10 candidates per 100 000 inside a margin (1e-9 rad of
    elevation, 1e-3 m of altitude, shadow and limb) -- for the small sets that is none -- and something accepted, something rejected"""
    n = max(sn.SIZES_N)
    (acc, _, _, seen), close = sn.reference(kind, T, n)
    for k in sn.SIZES_N:
        assert sn.under_cap(int(close[:k].sum()), k), (k, int(close[:k].sum()))
    assert 0 < acc.sum() < n and (seen != 0).any()
    assert sn.scene(kind, T)['rows'].shape == (T, sn.scene(kind, T)['S'], 16)


def test_the_scenes_deliver_what_the_gpu_tests_assert_on():
    """the S = 3 scene at 20 000 candidates (and at 4 099): at least one candidate accepted only because of the orbiting sensor, one
    rejected only because of the illumination test, one whose seen_by holds a moving bit alone; the controls each change something"""
    for n in (sn.N_BIG, max(sn.SIZES_N)):
        (acc, _, _, _), close = sn.reference('S3', sn.T_BIG, n)
        assert sn.under_cap(int(close.sum()), n)
        by_orbit, by_sun, moving_only = sn.only_for('S3', sn.T_BIG, n)
        assert by_orbit.any() and by_sun.any() and moving_only.any(), (n, by_orbit.sum(), by_sun.sum(), moving_only.sum())
    n = max(sn.SIZES_N)
    sc, cand = sn.scene('S3c', sn.T_BIG), sn.candidates(n)
    (base, _, _, _), close = sn.reference('S3c', sn.T_BIG, n)
    assert not close.any()
    for name, over in sn.controls(sc).items():
        (acc2, _, _, _), close2 = sn.run_numpy(cand, sc, pos=sn.positions(n, sn.T_BIG), **over)
        assert (acc2 != base).any() and not close2.any(), name


def test_the_env_scene_delivers():
    """the env test's catalogue (seed ENV_SEED, chosen here with the numpy rule): every row is seen within the first window, at least one
    by the orbiting sensor alone, none inside a margin; and the ground-only screen of the telescope variant keeps rows this network never
    sees in the window.  (With a ground RADAR the ground-only screen cannot: whatever it accepts the radar sees within the window.)"""
    sc = sn.env_scene()
    el, _ = sn.numpy_draw(sn.ENV_N, sn.ENV_SEED, sc)
    seen, close = sn.window_seen(el, sc)
    assert (seen != 0).all() and (seen == 2).any() and not close.any()
    # the ground-mask screen knows neither night nor orbit: one draw stands for both variants of the ground sensor ...
    tel = sn.env_scene(sn.ENV_TELESCOPE)
    el_cfg, _ = sn.numpy_draw(sn.ENV_N, sn.ENV_SEED, tel, ground_only=True)
    # ... the radar sees every one of them within the window, the telescope network misses some
    seen_radar, _ = sn.window_seen(el_cfg, sc)
    assert (seen_radar & 1 != 0).all()
    seen_cfg, _ = sn.window_seen(el_cfg, tel)
    assert (seen_cfg == 0).sum() >= 3, (seen_cfg == 0).sum()
