"""CPU-only checks of the sensor network (include/ssa_hip.h: ssa_env_step_sensors_f64; config['observers']): the export, the parameter
block's layout against the header, refusal of bad arguments before any launch, the config parser, the noise stream, no CPU fallback,
and the new kernels' resource budget in the shipped code object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from support.codeobj import KERNEL_FAMILIES, _kernels, assert_family_budget, header
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.refusals import STEP_PTRS, refused
from support.sensors import _bare_env, sites_rad


def test_sensor_step_is_exported_and_declared(lib):
    from ssa_gym_amd import _lib
    assert re.search(r"\bssa_env_step_sensors_f64\s*\(", header())
    assert "ssa_env_step_sensors_f64" in _lib.SIGNATURES
    assert hasattr(lib, "ssa_env_step_sensors_f64")
    m = re.search(r"#define SSA_MAX_SENSORS\s+(\d+)", header())
    assert m and int(m.group(1)) == _lib.MAX_SENSORS == 8


def test_sensor_params_layout_matches_the_header(lib, tmp_path):
    from ssa_gym_amd import _lib
    st = _lib.ssa_sensor_params
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssa_hip.h"', 'int main(void){',
           'printf("%zu\\n", sizeof(ssa_sensor_params));']
    want = [C.sizeof(st)]
    for f, _ in st._fields_:
        src.append('printf("%%zu\\n", offsetof(ssa_sensor_params, %s));' % f)
        want.append(getattr(st, f).offset)
    src.append('return 0;}')
    c = tmp_path / "sens.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "sens"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).decode().split()] == want


def test_sensor_step_refuses_bad_arguments_before_any_launch(lib):
    """NULL blocks, 0 or more than 8 sensors -> SSA_E_INVALID; several envs -> SSA_E_UNSUPPORTED; a missing step pointer -> SSA_E_INVALID.
    Nothing is launched (no device is touched: this runs without a GPU).  Every case spoils ONE field of blocks that are otherwise
    complete."""
    from ssa_gym_amd import _lib
    f = lib.ssa_env_step_sensors_f64
    for k in range(3):                                                     # NULL blocks
        assert refused(f, None, null=k) == _lib.E_INVALID, k
    for bad in (0, -1, 9):
        assert refused(f, None, ("sp", "n_sensor", bad)) == _lib.E_INVALID, bad
    assert refused(f, None, ("p", "n_env", 2)) == _lib.E_UNSUPPORTED
    for ptr in STEP_PTRS:
        assert refused(f, None, ("p", ptr, 0)) == _lib.E_INVALID, ptr
    assert refused(f, None, ("sp", "zn_stride_sensor", 0)) == _lib.E_INVALID      # two sensors cannot share one noise table


def test_config_parser_accepts_and_refuses():
    from ssa_gym_amd.envs._config import resolve_sensors
    assert resolve_sensors({}) is None
    net = resolve_sensors({'observers': [(38.8, -104.5, 1800), (28.4, -80.6, 3)], 'sensor_obs_limit': [15, 20],
                           'sensor_z_sigma': [(1, 1, 1e3), (2, 2, 2e3)]})
    assert net['sites'] == [(38.8, -104.5, 1800.0), (28.4, -80.6, 3.0)] and net['obs_limit'] == [15.0, 20.0]
    assert np.array_equal(net['z_sigma'][1], [2, 2, 2e3])
    one = resolve_sensors({'observers': [(38.8, -104.5, 1800)]})
    assert len(one['sites']) == 1 and one['obs_limit'] is None and one['z_sigma'] is None
    site = (0.0, 0.0, 0.0)
    for bad in ({'observers': []}, {'observers': [site] * 9}, {'observers': [(1.0, 2.0)]}, {'observers': [(np.nan, 0, 0)]},
                {'observers': 'nowhere'}, {'observers': [site, site], 'sensor_obs_limit': [10]},
                {'observers': [site], 'sensor_z_sigma': [(1, 1)]}, {'observers': [site], 'sensor_z_sigma': [(1, 1, -1)]},
                {'sensor_obs_limit': [10]}, {'sensor_z_sigma': [(1, 1, 1)]}):
        with pytest.raises(ValueError):
            resolve_sensors(bad)


def test_noise_stream_of_one_sensor_is_todays_and_the_others_follow_it():
    from ssa_gym_amd.envs._gymshim import np_random
    one = _bare_env(1)._draw_z_noise()
    ref, _ = np_random(5)
    want = ref.normal(size=(6, 10, 3)) * _bare_env(1).z_sigma          # the reference's draw (:219-221)
    assert one.shape == (6, 10, 3) and np.array_equal(one, want)
    env3 = _bare_env(3)
    three = env3._draw_z_noise()
    assert three.shape == (3, 6, 10, 3) and np.array_equal(three[0], want)
    for k in (1, 2):
        assert np.array_equal(three[k], ref.normal(size=(6, 10, 3)) * env3.sensor_z_sigma[k])


def test_step_refuses_two_sensors_on_one_object_and_has_no_cpu_fallback():
    from ssa_gym_amd import _lib
    env = _bare_env(3)
    with pytest.raises(_lib.SsaHipError):
        env.step([1, 2, 3])                 # no device state: no CPU fallback
    env._engine = object()                  # (the checks below come before anything touches the engine)
    with pytest.raises(ValueError):
        env.step([1, 2, 1])
    with pytest.raises(AssertionError):
        env.step([1, 2])
    with pytest.raises(AssertionError):
        env.step([1, 2, 10])


def test_multi_step_drivers_refuse_a_sensor_network():
    env = _bare_env(3)
    for call in (lambda: env.rollout([0, 1]), lambda: env.run_agent('agent_naive_greedy', 2), lambda: env.run_policy(None, 2),
                 lambda: env.lookahead()):
        with pytest.raises(NotImplementedError, match="sensor network"):
            call()


def test_sensor_kernels_keep_the_step_kernels_budget(tmp_path):
    """the eight sensor-network kernels (4 propagators x {one tile, multi tile}) fit the step kernel's register budget and LDS, use no
    more scratch than the step kernel of the same propagator and launch form, and touch it only around the out-of-line calls
    (SSA_PROP_ELEMENTS / SSA_PROP_HYBRID) -- FG and J2 none at all"""
    kern, ins_of = _kernels(tmp_path)
    assert_family_budget(kern, ins_of, "step_sensors_kernel", "step_fast_kernel", KERNEL_FAMILIES["step_sensors_kernel"])


# ---- the network's geometry at eight sites against the oracle's own (oracle/ssa_oracle.c: lla2ecef, ecef2aer), not the host's formulas.
def _net8():
    from ssa_gym_amd import host
    lla = sites_rad()
    lim = np.radians([15.0, -90.0, 30.0, 0.0, 5.0, -10.0, 20.0, 90.0])
    Rs = [np.diag([(1.0 + k) ** 2, (0.5 + 2.0 * k) ** 2, (1e3 / (1 + k)) ** 2]) * [host.arcsec2rad ** 2, host.arcsec2rad ** 2, 1]
          for k in range(8)]
    return lla, lim, Rs, host.make_sensor_params(lla, lim, Rs, 480 * 10 * 3)


def test_sensor_sites_against_the_oracle(lib, oracle):
    """each site's observer position within a few ulp of the oracle's lla2ecef, and enu^T d the oracle's ecef2aer (az, el, range) for
    directions all over the sky -- north and south of the horizon, through the zenith and the nadir"""
    lla, _, _, sp = _net8()
    rs = np.random.RandomState(0)
    dirs = rs.normal(size=(64, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    for s, site in enumerate(lla):
        o = oracle.lla2ecef(site)
        got = np.array(sp.obs_itrs[s][:])
        assert np.all(np.abs(got - o) <= 4 * np.spacing(np.linalg.norm(o))), (s, got - o)
        enu = np.array(sp.enu[s][:]).reshape(3, 3)
        for k, u in enumerate(dirs):
            d = u * (1e6 + 4e7 * k / len(dirs))
            ref = oracle.ecef2aer(site, o + d, o)
            R = enu.T @ d
            r = np.linalg.norm(d)
            assert abs(np.linalg.norm(R) - ref[2]) <= 1e-14 * ref[2], (s, k)
            el = np.arctan2(R[2], np.hypot(R[0], R[1]))
            assert abs(el - ref[1]) <= 1e-13 + 1e-15 / max(np.cos(ref[1]), 1e-12), (s, k, el, ref[1])   # (asin near +-90 deg)
            if np.hypot(R[0], R[1]) > 1e-3 * r:
                daz = (np.arctan2(R[1], R[0]) - ref[0] + np.pi) % (2 * np.pi) - np.pi
                assert abs(daz) <= 1e-13, (s, k, daz)


def test_sensor_params_slices_are_the_kernel_consts_of_each_site(lib):
    """site s's slice of make_sensor_params is, bit for bit, what kernel_consts gives an env observing from that site alone"""
    from ssa_gym_amd.envs import env_config
    from ssa_gym_amd.envs._config import kernel_consts
    lla, lim, Rs, sp = _net8()
    cfg = dict(env_config)
    Q = np.eye(6)
    for s in range(8):
        c, _ = kernel_consts(cfg, Q, Rs[s], 20.0, lim[s], lla[s])
        for name, got, want in (("enu", sp.enu[s][:], c.enu[:]), ("obs_itrs", sp.obs_itrs[s][:], c.obs_itrs[:]),
                                ("R", sp.R[s][:], c.R[:]), ("obs_limit", [sp.obs_limit[s]], [c.obs_limit])):
            assert np.array_equal(np.array(got).view(np.int64), np.array(want).view(np.int64)), (s, name)
