"""CPU-only checks of the space-based sensors of a network (ssa_step_params.site_rows / limb_radius / site_moving; config['observers']
entries {'orbit': ...}): the appended fields against the header compiled with gcc, the packing of the site rows, the axes an orbiting
sensor measures in, the config rules, the header's words, the numpy rule on crafted geometry, and every new refusal at every entry --
each behind every older refusal."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from support import angles_only as ao
from support import illumination as il
from support import orbiting as ob
from support.codeobj import header
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.refusals import nan_mask

EPS = 2.0 ** -52
ONE, HIGH, ZERO = 0b10, 0b100, 0b01      # (the harness's blocks have two sensors: bit 1 is the one that may move, bit 2 is at n_sensor)
GOOD = (("p", "site_rows", ob.SITE_PTR), ("p", "limb_radius", ob.R_LIMB))
NEW = ("site_rows", "limb_radius", "site_moving", "reserved3")
NO_NETWORK = ("ssa_env_step_f64", "ssa_lookahead_f64", "ssa_env_rollout_f64")      # (of the harness; the closed loop asks the device first: tests/test_orbiting_gpu.py)


# ---------------------------------------------------------------------------------------------------------------- 1. the block
def test_the_step_block_grows_at_its_end_and_the_abi_keeps_its_version(lib, tmp_path):
    from ssa_gym_amd import _lib
    st, sp = _lib.ssa_step_params, _lib.ssa_sensor_params
    names = [f for f, _ in st._fields_]
    assert tuple(names[-4:]) == NEW and names[-5] == "metrics_prev"
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssa_hip.h"', 'int main(void){',
           'printf("%zu %zu %d %zu %zu\\n", offsetof(ssa_step_params, metrics_prev), sizeof(ssa_step_params), SSA_ABI_VERSION,'
           ' sizeof(ssa_sensor_params), offsetof(ssa_sensor_params, reserved2));']
    src += ['printf("%%zu %%zu\\n", offsetof(ssa_step_params, %s), sizeof(((ssa_step_params *)0)->%s));' % (f, f) for f in NEW]
    src.append('return 0;}')
    c = tmp_path / "site.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "site"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert out[:5] == [str(st.metrics_prev.offset), str(C.sizeof(st)), "23", str(C.sizeof(sp)), str(sp.reserved2.offset)]
    assert [int(v) for v in out[5:]] == [w for f in NEW for w in (getattr(st, f).offset, getattr(st, f).size)]
    assert st.site_rows.offset == st.metrics_prev.offset + 8 and C.sizeof(st) == st.metrics_prev.offset + 32
    # (ssa_sensor_params untouched: its tail is 8t's)
    assert [f for f, _ in sp._fields_][-4:] == ["sun", "shadow_radius", "sunlit_only", "reserved2"] and C.sizeof(sp) == sp.upd.offset + 32
    assert lib.ssa_abi_version() == 23
    assert re.search(r"int ssa_los_mask_f64\s*\(", header()) and "ssa_los_mask_f64" in _lib.SIGNATURES
    z = st()
    assert (z.site_rows, z.limb_radius, z.site_moving, z.reserved3) == (None, 0.0, 0, 0)


def test_the_header_states_the_rule_the_layout_and_the_refusals():
    h = " ".join(tok for tok in header().split() if tok != "*")
    for phrase in ("clear = (p <= 0) || (p >= dd) || (oo dd - p p >= R_b R_b dd)", "visible = clear && (no sunlit_only bit || object sunlit)",
                   "the Sun row's dark bit is NOT read for a moving sensor", "A NaN anywhere gives not visible",
                   "[n_time][n_sensor][16] doubles on the device, base 128-byte aligned", "enu[9] in the layout of ssa_sensor_params.enu[s], obs_itrs[3], then 4 words that are 0",
                   "With site_moving == 0 neither `site_rows` nor `limb_radius` is read", "a site_moving bit at or above n_sensor, or bit 0",
                   "`site_rows` is NULL or not 128-byte aligned", "!(limb_radius >= 0)", "obs_type is not SSA_OBS_AER",
                   "SSA_E_UNSUPPORTED by the entries that take no ssa_sensor_params", "obs_limit[s] is NOT read"):
        assert phrase in h, phrase


# ---------------------------------------------------------------------------------------------------------------- 2. the rows
def test_pack_site_rows():
    from ssa_gym_amd import host
    rs = np.random.RandomState(0)
    enu, obs = rs.normal(size=(5, 3, 9)), rs.normal(size=(5, 3, 3))
    rows = host.pack_site_rows(enu, obs)
    assert rows.shape == (5, 3, 16) and rows.dtype == np.float64 and rows.flags.c_contiguous and host.SITE_ROW == 16
    assert np.array_equal(rows[:, :, :9], enu) and np.array_equal(rows[:, :, 9:12], obs) and not rows[:, :, 12:].any()
    assert np.array_equal(host.pack_site_rows(enu.reshape(5, 3, 3, 3), obs), rows)
    for bad in ((enu[:, :, :8], obs), (enu, obs[:4]), (enu[0], obs[0]), (enu, obs[:, :, :2]), (np.zeros((2, 9, 9)), np.zeros((2, 9, 3))),
                (np.zeros((0, 2, 9)), np.zeros((0, 2, 3)))):
        with pytest.raises(ValueError):
            host.pack_site_rows(*bad)


def test_orbit_site_rows_measure_in_inertial_axes():
    """the kernel's local vector is uvw[j] = sum_i enu[i][j] d[i] with d = trans r - obs (hx_aer_enu; uvw = north, east, up, azimuth
    = atan2(east, north)).  For an orbiting sensor it must be r - o in INERTIAL axes with east = y, north = x, up = z: azimuth the
    topocentric right ascension.  Bound per component: 16 * 2^-52 * (|r| + |o|) -- two 3 x 3 products and one subtraction, each at most
    three roundings at that magnitude, with margin two."""
    from ssa_gym_amd import host
    from support.batches import c2t
    trans = c2t()[:ob.N_TIME].reshape(-1, 9)
    rs = np.random.RandomState(1)
    o = np.array([il.unit(rs.normal(size=3)) * ob.LEO for _ in range(ob.N_TIME)])
    enu, obs = host.orbit_site_rows(trans, o)
    assert enu.shape == (ob.N_TIME, 9) and obs.shape == (ob.N_TIME, 3)
    assert np.array_equal(host.orbit_site_rows(trans.reshape(-1, 3, 3), o)[1], obs)
    for t in range(ob.N_TIME):
        M = trans[t].reshape(3, 3)
        assert np.max(np.abs(obs[t] - M @ o[t])) <= 4 * EPS * ob.LEO
        for _ in range(4):
            r = il.unit(rs.normal(size=3)) * rs.uniform(7e6, 4.5e7)
            d = M @ r - obs[t]
            uvw = np.array([enu[t][j] * d[0] + enu[t][3 + j] * d[1] + enu[t][6 + j] * d[2] for j in range(3)])      # (the kernel's product)
            east, north, up = uvw[1], uvw[0], uvw[2]
            want = r - o[t]
            bound = 16 * EPS * (np.linalg.norm(r) + np.linalg.norm(o[t]))
            assert max(abs(east - want[1]), abs(north - want[0]), abs(up - want[2])) <= bound
            az = np.arctan2(east, north) % (2 * np.pi)
            assert abs(az - np.arctan2(want[1], want[0]) % (2 * np.pi)) <= 1e-9      # (right ascension, by uvw2aer's own convention)
    for bad in ((trans[:3], o), (trans, o[:, :2]), (trans[:, :8], o)):
        with pytest.raises(ValueError):
            host.orbit_site_rows(*bad)


# ---------------------------------------------------------------------------------------------------------------- 3. config rules
def test_config_rules():
    from ssa_gym_amd import envs as E
    from ssa_gym_amd import host
    from ssa_gym_amd.envs._config import resolve_config, resolve_sensors
    c = resolve_config(ob.orbit_cfg(E))
    assert c.net.moving.tolist() == [False, True, True] and c.net.sunlit_only.tolist() == [False, False, True]
    assert c.net.angles_only.tolist() == [False, True, False] and c.limb_radius == host.R_EQ_EARTH + 100e3
    assert c.net.orbit[0] is None and np.array_equal(c.net.orbit[1], ob.ENV_ORBITS[0]) and np.array_equal(c.net.orbit[2], ob.ENV_ORBITS[1])
    assert np.isfinite(c.net.obs_limit).all() and c.net.obs_limit[0] == np.radians(ao.MASKS_DEG[0])
    assert c.sun.shape == (c.trans.shape[0], 3)
    # (the default: nothing moves; and a network without the per-sensor list)
    off = resolve_config(ao.mixed_cfg(E))
    assert not off.net.moving.any() and off.net.orbit == [None] * 3 and resolve_sensors(ao.mixed_cfg(E))['orbit'] == [None] * 3
    cfg = ob.orbit_cfg(E)
    del cfg['sensor_obs_limit']
    assert resolve_config(cfg).net.moving.tolist() == [False, True, True]
    assert resolve_config(ob.orbit_cfg(E, limb_radius=6.4e6)).limb_radius == 6.4e6
    orbit = {'orbit': ob.ENV_ORBITS[0]}
    # observers[0] must be a ground site
    with pytest.raises(ValueError, match=r"observers'\]\[0\] must be a ground site"):
        resolve_sensors(ob.orbit_cfg(E, observers=[orbit, ao.SITES[1], ao.SITES[2]], sensor_obs_limit=None, sensor_illumination=None))
    # an entry that is neither a site nor {'orbit': six finite values}
    for bad in ({'orbit': ob.ENV_ORBITS[0][:5]}, {'orbit': [np.nan] + ob.ENV_ORBITS[0][1:]}, {'orbits': ob.ENV_ORBITS[0]}, {'orbit': 'leo'},
                {'orbit': ob.ENV_ORBITS[0], 'name': 'x'}):
        with pytest.raises(ValueError, match="observers"):
            resolve_sensors(ob.orbit_cfg(E, observers=[ao.SITES[0], bad, orbit]))
    # no elevation mask for an orbiting sensor; a ground site keeps its
    for bad in ([15.0, 5.0, None], [15.0, None, 0.0], [None, None, None], [15.0, None]):
        with pytest.raises(ValueError, match="sensor_obs_limit"):
            resolve_sensors(ob.orbit_cfg(E, sensor_obs_limit=bad))
    # illumination: None or 'sunlit', never a number; a ground site never 'sunlit'
    assert resolve_sensors(ob.orbit_cfg(E, sensor_illumination=[-12.0, 'sunlit', None]))['illumination'] == [-12.0, 0.0, None]
    for bad in ([None, -12.0, 'sunlit'], [None, None, 0], [None, 'lit', None], ['sunlit', None, None], [None, None, True]):
        with pytest.raises(ValueError, match="sensor_illumination"):
            resolve_sensors(ob.orbit_cfg(E, sensor_illumination=bad))
    # az-el-range only
    from support.sensors import xyz_net
    x = dict(ao.mixed_cfg(E, kinds=None, **xyz_net()))
    with pytest.raises(ValueError, match="obs_type 'aer'"):
        resolve_sensors(dict(x, observers=[x['observers'][0], orbit] + list(x['observers'][2:])))
    # the limb radius, and an orbit that starts inside it (what needs no propagation)
    for bad in (-1.0, float('nan')):
        with pytest.raises(ValueError, match="limb_radius"):
            resolve_config(ob.orbit_cfg(E, limb_radius=bad))
    low = {'orbit': [6.4e6, 0.0, 0.0, 0.0, 7.8e3, 0.0]}
    with pytest.raises(ValueError, match="inside config\\['limb_radius'\\]"):
        resolve_config(ob.orbit_cfg(E, observers=[ao.SITES[0], low, orbit]))


def test_the_catalogue_screens_on_the_ground_sites_only(monkeypatch):
    from ssa_gym_amd import catalogue
    from ssa_gym_amd import envs as E
    seen = []
    monkeypatch.setattr(catalogue, "visible_catalogue", lambda n, seed=0, **kw: seen.append(kw))
    catalogue.catalogue_for_config(ob.orbit_cfg(E), n=10)
    assert seen[-1]['sites'] == [tuple(ao.SITES[0])] and seen[-1]['el_min_deg'] == [ao.MASKS_DEG[0]]
    assert "GROUND sites only" in catalogue.catalogue_for_config.__doc__


# ---------------------------------------------------------------------------------------------------------------- 4. the rule
def test_the_numpy_rule_on_crafted_geometry():
    """identity trans, the sensor on the +x axis at LEO: an object on the sensor's side of the Earth; one directly behind the Earth;
    1e-6 R_b inside and outside the limb; the closest point of the line beyond either end of the segment; a NaN row"""
    R, o = ob.R_LIMB, np.array([ob.LEO, 0.0, 0.0])
    M = np.eye(3)
    # (a line through o that passes the geocentre at distance q: o + L g, with g = (-cos a, sin a, 0) and sin a = q / | o |)
    def along(q, L):
        a = np.arcsin(q / ob.LEO)
        return o + L * np.array([-np.cos(a), np.sin(a), 0.0])
    far = 4e7
    rows = np.array([[4.2e7, 1e6, 0.0], [0.0, 4.2e7, 0.0],          # on the sensor's side: the closest point before the sensor, or just behind it
                     [-4.2e7, 0.0, 0.0], along(1e3, far),             # directly behind the Earth, and 1 km off its centre
                     along(R * (1 - 1.001e-6), far), along(R * (1 + 1.001e-6), far),      # just inside, just outside the limb (1e-6 R_b and the construction's rounding)
                     along(R * 0.5, 1e6), along(R * 0.5, 2.0e6),      # the line cuts the sphere, the object stops short of it: beyond the far end
                     along(R * 0.5, far),                             # ... and the same line carried through
                     [np.nan, 1e7, 1e7]])
    want = [True, True, False, False, False, True, True, True, False, False]
    rel, p0, p1, inside = ob.margins(rows[:-1], M, o)
    assert np.all(rel[inside] >= 1e-6) and np.all(p0 >= 1e3) and np.all(p1 >= 1e3)
    assert inside.tolist() == [False, True, True, True, True, True, False, False, True]      # (row 1: just inside, and far outside the sphere)
    assert ob.los_clear(rows, M, o).tolist() == want
    # (the radius is the argument; a NaN sensor sees nothing; the matrix is applied to the object, not to the sensor)
    off_centre = np.delete(rows[:-1], 2, axis=0)      # (the line through the geocentre itself touches a sphere of radius 0)
    assert ob.los_clear(off_centre, M, o, R=0.0).all() and not ob.los_clear(rows, M, o * np.nan).any()
    Rz = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    assert ob.los_clear(rows @ Rz, Rz, o).tolist() == want      # (rows @ Rz = Rz^T rows: the same geometry after M)


# ---------------------------------------------------------------------------------------------------------------- 5. the refusals
def _answer(lib, entry, *fields, **kw):
    from ssa_gym_amd import _lib
    assert any(name == "site_moving" for name, _ in _lib.ssa_step_params._fields_), "ssa_step_params has no site_moving word"
    return ao.answer(lib, entry, *fields, **kw)


@pytest.mark.parametrize("entry", ao.SENSOR_ENTRIES)
def test_the_new_refusals_at_every_sensor_entry(lib, entry):
    """a bit at or above n_sensor (the blocks have two sensors) or bit 0; any bit while site_rows is NULL or not 128-byte aligned; any bit
    while !(limb_radius >= 0); any bit while obs_type is not SSA_OBS_AER: SSA_E_INVALID, before any launch (nothing here is launched:
    every call breaks a rule)"""
    from ssa_gym_amd import _lib
    assert len(ao.SENSOR_ENTRIES) == 9
    for bits in (HIGH, HIGH | ONE, ZERO, ZERO | ONE, 1 << 7, 1 << 8, 1 << 30, -1):
        assert _answer(lib, entry, ("p", "site_moving", bits), *GOOD) == _lib.E_INVALID, (entry, bits)
    assert _answer(lib, entry, ("p", "site_moving", ONE), ("sp", "n_sensor", 1), *GOOD) == _lib.E_INVALID, entry
    for ptr in (0, ob.SITE_PTR + 8, ob.SITE_PTR + 32, ob.SITE_PTR + 64, ob.SITE_PTR + 1):
        assert _answer(lib, entry, ("p", "site_moving", ONE), ("p", "site_rows", ptr), ("p", "limb_radius", ob.R_LIMB)) == _lib.E_INVALID, (entry, ptr)
    for rad in (-1.0, float("nan"), -float("inf")):
        assert _answer(lib, entry, ("p", "site_moving", ONE), ("p", "site_rows", ob.SITE_PTR), ("p", "limb_radius", rad)) == _lib.E_INVALID, (entry, rad)
    assert _answer(lib, entry, ("p", "site_moving", ONE), ("c", "obs_type", _lib.OBS_XYZ), *GOOD) == _lib.E_INVALID, entry


@pytest.mark.parametrize("entry", NO_NETWORK)
def test_an_entry_without_a_network_cannot_honour_a_moving_sensor(lib, entry):
    """the one-observer step, lookahead and rollout read ssa_consts: any bit is SSA_E_UNSUPPORTED, however good the table -- behind
    every other refusal of the entry (a NULL trans keeps SSA_E_INVALID)"""
    from ssa_gym_amd import _lib
    from support.refusals import refused, valid_blocks
    for bits in (ONE, ZERO, HIGH, -1):
        assert refused(getattr(lib, entry), valid_blocks(entry), ("p", "site_moving", bits), *GOOD) == _lib.E_UNSUPPORTED, (entry, bits)
        assert refused(getattr(lib, entry), valid_blocks(entry), ("p", "site_moving", bits)) == _lib.E_UNSUPPORTED, (entry, bits)
        assert refused(getattr(lib, entry), valid_blocks(entry), ("p", "site_moving", bits), ("p", "trans", 0), *GOOD) == _lib.E_INVALID
    if entry == "ssa_env_step_f64":
        assert refused(lib.ssa_env_step_instance, valid_blocks(entry), ("p", "site_moving", ONE), *GOOD) == _lib.E_UNSUPPORTED


@pytest.mark.parametrize("entry", ao.SENSOR_ENTRIES)
def test_the_new_refusals_rank_behind_an_unsupported_form(lib, entry):
    """a block that also breaks a rule answered with SSA_E_UNSUPPORTED keeps that code: several envs at a one-env entry, ragged envs at
    an *_envs one"""
    from ssa_gym_amd import _lib
    other = ("p", "n_obj", 6) if entry.endswith("_envs_f64") else ("p", "n_env", 2)
    assert _answer(lib, entry, other) == _lib.E_UNSUPPORTED, entry
    for extra in ((("p", "site_moving", HIGH),) + GOOD, (("p", "site_moving", ONE),), (("p", "site_moving", ONE), ("p", "site_rows", ob.SITE_PTR + 8)),
                  (("p", "site_moving", ONE), ("p", "site_rows", ob.SITE_PTR), ("p", "limb_radius", float("nan")))):
        assert _answer(lib, entry, other, *extra) == _lib.E_UNSUPPORTED, (entry, extra)


def _recorded_cases():
    """the recorded cases of tests/golden/refusal_order.json (entry, n_env, fields) with their codes"""
    table = json.load(open(os.path.join(GOLDEN, "refusal_order.json")))
    out = []
    for key in table:
        entry, n_env, *rest = key.split(" ")
        fields = []
        for tok in rest:
            blk, _, tail = tok.partition(".")
            name, _, val = tail.partition("=")
            fields.append((blk, name, float("nan") if val == "nan" else int(val)))
        out.append((key, entry, int(n_env.split("=")[1]), tuple(fields), table[key]))
    return out


def test_every_recorded_refusal_keeps_its_code_with_a_bad_site_moving_added(lib):
    """tests/golden/refusal_order.json: every recorded case, of the sensor entries and of the entries without a network alike, with
    each new fault added to its block, is answered as recorded -- the new rules rank last"""
    from ssa_gym_amd import _lib
    from support.refusals import refused, valid_blocks
    assert any(name == "site_moving" for name, _ in _lib.ssa_step_params._fields_)
    n = 0
    for key, entry, n_env, fields, code in _recorded_cases():
        plain = [f for f in fields if f[1] != "obs_limit[1]"]
        for extra in ((("p", "site_moving", HIGH),) + GOOD, (("p", "site_moving", ONE),), (("p", "site_moving", ZERO),) + GOOD,
                      (("p", "site_moving", ONE), ("p", "site_rows", ob.SITE_PTR), ("p", "limb_radius", -1.0))):
            got = refused(getattr(lib, entry), valid_blocks(entry, n_env), *plain, *extra, spoil=nan_mask if len(plain) != len(fields) else None)
            assert got == getattr(_lib, "E_" + code), (key, extra, got)
            n += 1
    assert n >= 4 * 30


def test_a_valid_block_with_the_tail_zero_is_not_refused_for_it(lib):
    """site_moving == 0 with a NULL table, a NaN radius and an xyz observation: nothing of the new rules applies (the call is made
    complete but for one older fault, so that nothing is launched, and answers that fault's code)"""
    from ssa_gym_amd import _lib
    for entry in ao.SENSOR_ENTRIES:
        got = _answer(lib, entry, ("p", "site_moving", 0), ("p", "limb_radius", float("nan")), ("c", "obs_type", _lib.OBS_XYZ), ("p", "trans", 0))
        assert got == _lib.E_INVALID, entry
    other = ("p", "n_env", 2)
    assert _answer(lib, "ssa_lookahead_sensors_f64", ("p", "site_moving", 0), ("p", "limb_radius", float("nan")), other) == _lib.E_UNSUPPORTED
