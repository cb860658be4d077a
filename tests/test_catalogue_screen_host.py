"""The visibility screen of a synthetic catalogue without a GPU (include/ssa_hip.h: ssa_catalogue_screen_params; catalogue.visible_catalogue
and catalogue_for_config): the ABI struct against its ctypes mirror, the numpy restatement of the rule for a network of sites that the GPU
tests judge the kernel by (equal to catalogue._accepted bit for bit with one site), argument validation before any launch, and the mapping
of an env_config dict to sites, masks and epoch."""
import ctypes as C
import os
import subprocess
from datetime import datetime

import numpy as np
import pytest

from conftest import ROOT
from support.codeobj import header
from support.screen import _SITES3, screen_numpy, site_rows


def test_screen_params_layout_matches_the_header(tmp_path):
    """ssa_screen_params: sizeof / offsetof with gcc against the ctypes mirror; the entry point declared and bound"""
    import re
    from ssa_gym_amd import _lib, catalogue
    st = _lib.ssa_screen_params
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssa_hip.h"', 'int main(void){',
           'printf("%zu\\n", sizeof(ssa_screen_params));']
    want = [C.sizeof(st)]
    for f, _ in st._fields_:
        src.append('printf("%%zu\\n", offsetof(ssa_screen_params, %s));' % f)
        want.append(getattr(st, f).offset)
    src.append('return 0;}')
    c = tmp_path / "screen_layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "screen_layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).decode().split()] == want
    hdr = header()
    assert re.search(r"\bint ssa_catalogue_screen_f64\s*\(const ssa_screen_params \*p, void \*stream\);", hdr)
    assert "ssa_catalogue_screen_f64" in _lib.SIGNATURES
    assert int(re.search(r"#define SSA_MAX_SENSORS\s+(\d+)", hdr).group(1)) == catalogue.MAX_SITES


def test_numpy_restatement_equals_accepted_with_one_site():
    """screen_numpy with the default site is catalogue._accepted bit for bit, 3 000 candidates per regime"""
    from ssa_gym_amd import catalogue
    from ssa_gym_amd.envs.transformations import trans_matrix_table
    step = 150.0
    times = step * np.arange(96)
    M_t = trans_matrix_table(datetime(2020, 5, 4), step, 96)
    (enu, obs_itrs, el_min), = site_rows([catalogue.DEFAULT_SITE], [15.0])
    rs = np.random.RandomState(11)
    n_acc = 0
    for k in range(5):
        cand = catalogue._draw_elements(rs, k, 3000)
        want = catalogue._accepted(*cand, M_t, times, enu, obs_itrs, el_min, 18, 36)
        got = screen_numpy(*cand, M_t, times, [(enu, obs_itrs, el_min)], 18, 36)[0]
        assert np.array_equal(got, want), k
        n_acc += int(want.sum())
    assert n_acc > 100      # the comparison covers accepted candidates too (GEO, Tundra, Molniya pass often)


@pytest.mark.parametrize("kw", [
    dict(sites=[]),
    dict(sites=[(0.0, 0.0, 0.0)] * 9),
    dict(sites=_SITES3, el_min_deg=[15.0, 10.0]),
    dict(sites=[(float("nan"), 0.0, 0.0)]),
    dict(sites=[(0.0, float("inf"), 0.0)]),
    dict(sites=[(0.0, 0.0)]),
    dict(sites=_SITES3, el_min_deg=[15.0, float("nan"), 20.0]),
    dict(step=0.0),
    dict(step=-150.0),
    dict(duration=100.0),
    dict(duration=0.0),
])
def test_visible_catalogue_rejects_bad_arguments_before_any_launch(kw):
    from ssa_gym_amd import catalogue
    with pytest.raises(ValueError):
        catalogue.visible_catalogue(10, 0, **kw)


def test_catalogue_for_config_rejects_bad_networks():
    from ssa_gym_amd import catalogue
    with pytest.raises(ValueError):
        catalogue.catalogue_for_config(dict(observers=[(0.0, 0.0, 0.0)] * 9), n=10)
    with pytest.raises(ValueError):
        catalogue.catalogue_for_config(dict(observers=_SITES3, sensor_obs_limit=[15.0]), n=10)
    with pytest.raises(ValueError):
        catalogue.catalogue_for_config(dict(observer=(0.0, 0.0, 0.0)), n=10, step=-1.0)


def test_catalogue_for_config_maps_sites_masks_and_epoch(monkeypatch):
    import inspect
    from ssa_gym_amd import catalogue
    assert inspect.signature(catalogue.visible_catalogue).parameters['el_min_deg'].default == 15.0
    seen = []
    monkeypatch.setattr(catalogue, "visible_catalogue", lambda n, seed=0, **kw: seen.append((n, seed, kw)))
    t0 = datetime(2012, 6, 1)
    # a network: its sites, per-sensor masks and epoch; NOT the env's obs_limit
    catalogue.catalogue_for_config(dict(observer=(1.0, 2.0, 3.0), observers=_SITES3, sensor_obs_limit=[15, 10, 20], obs_limit=-90, t_0=t0),
                                   n=500, seed=4)
    assert seen[-1] == (500, 4, dict(sites=_SITES3, el_min_deg=[15, 10, 20], t_0=t0))
    # a network without per-sensor masks: the el_min_deg default (15 deg) stays in force
    catalogue.catalogue_for_config(dict(observers=_SITES3[:2], obs_limit=-90, t_0=t0))
    assert seen[-1] == (20000, 0, dict(sites=_SITES3[:2], t_0=t0))
    # a single observer
    catalogue.catalogue_for_config(dict(observer=(38.828198, -77.305352, 20.0), obs_limit=-90, t_0=datetime(2020, 5, 4)), n=7)
    assert seen[-1] == (7, 0, dict(sites=[(38.828198, -77.305352, 20.0)], t_0=datetime(2020, 5, 4)))
    # keyword arguments override what the config says
    catalogue.catalogue_for_config(dict(observers=_SITES3, sensor_obs_limit=[15, 10, 20], t_0=t0), n=9, el_min_deg=5.0, step=120.0,
                                   t_0=datetime(2019, 1, 1))
    assert seen[-1] == (9, 0, dict(sites=_SITES3, el_min_deg=5.0, step=120.0, t_0=datetime(2019, 1, 1)))
    # the env's own default config: its observer, the default epoch, and a 15 deg mask rather than obs_limit = -90
    from ssa_gym_amd.envs import env_config
    catalogue.catalogue_for_config(env_config, n=3)
    assert seen[-1] == (3, 0, dict(sites=[tuple(env_config['observer'])], t_0=env_config['t_0']))
