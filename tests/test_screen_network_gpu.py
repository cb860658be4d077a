"""The catalogue screen by a network's own rule on the MI355X (include/ssa_hip.h: ssa_catalogue_screen_network_f64;
catalogue.visible_catalogue_network, catalogue_for_network).

The ground truth is the numpy rule of tests/support/screen_network.py.  The library is built with -ffp-contract=fast and the device
functions contract by hand, so the kernel's intermediate values are not numpy's bits: the contract is equal decisions (accept, worst gap,
flags, seen_by) for every candidate whose numpy margins are at least 1e-9 rad of elevation and 1e-3 m of altitude, shadow and limb at
every sample, and fewer than 10 candidates per 100 000 may lie inside them (tests/test_screen_network_host.py shows that the inputs
used here keep to that, and that the scenes deliver what is asserted on)."""
import numpy as np
import pytest

from support import screen_network as sn
from support.gpu import dev  # noqa: F401  (the module fixture)
from support.screen import _SITES3, site_rows

pytestmark = pytest.mark.gpu
NAMES = ("accept", "worst_gap", "flags", "seen_by")


def _launch(dev, cand, sc, tab=None, **over):
    """the network entry on candidates `cand` in scene `sc` (numpy_kw's overrides applied): (accept, worst_gap, flags, seen_by) as numpy"""
    kw = {k: (dev.as_dev(v) if isinstance(v, np.ndarray) else v) for k, v in sn.device_kw(sc, **over).items()}
    out = dev.catalogue_screen_network(dev.as_dev(np.stack(cand, axis=1)), dev.as_dev(sc['M_t']), dev.as_dev(sc['tab'] if tab is None else tab),
                                       sc['step'], 300e3, sc['first'], sc['max_gap'], want_gap=True, want_flags=True, want_seen_by=True, **kw)
    acc, gap, flags, seen = (t.cpu().numpy() for t in out)
    return acc.astype(bool), gap, flags, seen


def _same(got, want, keep, what):
    for name, g, w in zip(NAMES, got, want):
        bad = np.where(keep & (g != w))[0]
        assert bad.size == 0, (what, name, bad[:10], g[bad[:10]], w[bad[:10]])


@pytest.mark.parametrize("kind", ["S1", "S3", "S8"])
@pytest.mark.parametrize("T", sn.SIZES_T)
def test_the_operator_against_numpy(dev, kind, T):
    """S = 1 with bit 0 moving; S = 3: ground radar, ground telescope with a night limit, LEO 'sunlit' sensor; S = 8 with bit 7 moving --
    at T samples and 1, 3, 4, 5 and 4 099 candidates (less than a workgroup, one, one and a wavefront, 1 025 workgroups)"""
    sc = sn.scene(kind, T)
    want, close = sn.reference(kind, T, max(sn.SIZES_N))
    cand = sn.candidates(max(sn.SIZES_N))
    for n in sn.SIZES_N:
        got = _launch(dev, tuple(c[:n] for c in cand), sc)
        print("%s T = %d n = %d: %d accepted, %d within numpy's margins" % (kind, T, n, got[0].sum(), close[:n].sum()))
        assert sn.under_cap(int(close[:n].sum()), n)
        _same(got, [w[:n] for w in want], ~close[:n], (kind, T, n))


def test_the_operator_against_numpy_at_20000_candidates(dev):
    """the S = 3 scene, one launch of 20 000 candidates at T = 96; what only the new rule can decide is among them"""
    sc = sn.scene('S3', sn.T_BIG)
    want, close = sn.reference('S3', sn.T_BIG, sn.N_BIG)
    got = _launch(dev, sn.candidates(sn.N_BIG), sc)
    print("%d accepted, %d within numpy's margins" % (got[0].sum(), close.sum()))
    assert sn.under_cap(int(close.sum()), sn.N_BIG)
    _same(got, want, ~close, 'S3')
    by_orbit, by_sun, moving_only = sn.only_for('S3', sn.T_BIG, sn.N_BIG)
    assert (got[0] & by_orbit & ~close).any() and (~got[0] & by_sun & ~close).any()
    assert ((got[3] == sc['site_moving']) & moving_only & ~close).any()


@pytest.mark.parametrize("sites,masks", [(None, None), (_SITES3, [15.0, 10.0, 20.0])])
def test_off_means_off(dev, sites, masks):
    """site_moving == sunlit_only == 0: accept, worst_gap and flags are device.catalogue_screen's bytes on 20 000 candidates -- the
    default site, and 8e's 3-site network -- with no tables, and with tables full of NaN"""
    from ssa_gym_amd import catalogue
    sites, masks = ([catalogue.DEFAULT_SITE], [15.0]) if sites is None else (sites, masks)
    sc = sn.scene('S3', sn.T_BIG)
    tab = dev.as_dev(np.array([np.concatenate([enu.reshape(9), obs, [lim]]) for enu, obs, lim in site_rows(sites, masks)]))
    el, trans = dev.as_dev(np.stack(sn.candidates(sn.N_BIG), axis=1)), dev.as_dev(sc['M_t'])
    want = dev.catalogue_screen(el, trans, tab, sc['step'], 300e3, sc['first'], sc['max_gap'], want_gap=True, want_flags=True)
    assert 0 < int(want[0].sum()) < sn.N_BIG
    S = len(sites)
    nan_rows = dev.as_dev(np.full((sn.T_BIG, S, 16), np.nan))
    nan_sun = dev.as_dev(np.full((sn.T_BIG, 4), np.nan))
    for kw in (dict(), dict(site_rows=nan_rows, sun=nan_sun, limb_radius=float("nan"), shadow_radius=float("nan"))):
        got = dev.catalogue_screen_network(el, trans, tab, sc['step'], 300e3, sc['first'], sc['max_gap'], want_gap=True, want_flags=True,
                                           want_seen_by=True, **kw)
        for name, g, w in zip(NAMES, got, want):
            assert g.dtype == w.dtype and bool((g == w).all()), name
        # (seen by some sensor <=> visible at some sample: the run of invisible samples is shorter than T)
        assert bool(((got[3] != 0) == (want[1] < sn.T_BIG)).all())


def test_only_the_bits_select(dev):
    """a sensor without a moving bit never reads its rows of site_rows; a moving sensor never reads base.sites[s]: NaN there changes
    nothing"""
    sc = sn.scene('S3', sn.T_BIG)
    cand = sn.candidates(max(sn.SIZES_N))
    want = _launch(dev, cand, sc)
    tab = sc['tab'].copy()
    kw = sn.device_kw(sc)
    rows = kw['site_rows'].copy()
    for s in range(sc['S']):
        if (sc['site_moving'] >> s) & 1:
            tab[s] = np.nan
            rows[:, s, :9] = np.nan          # (and the enu words of a moving sensor's own rows are not read either)
            rows[:, s, 12:] = np.nan
        else:
            rows[:, s] = np.nan
    got = dev.catalogue_screen_network(dev.as_dev(np.stack(cand, axis=1)), dev.as_dev(sc['M_t']), dev.as_dev(tab), sc['step'], 300e3,
                                       sc['first'], sc['max_gap'], want_gap=True, want_flags=True, want_seen_by=True,
                                       site_rows=dev.as_dev(rows), site_moving=kw['site_moving'], limb_radius=kw['limb_radius'],
                                       sun=dev.as_dev(kw['sun']), sunlit_only=kw['sunlit_only'], shadow_radius=kw['shadow_radius'])
    for name, g, w in zip(NAMES, got, want):
        assert np.array_equal(g.cpu().numpy().astype(w.dtype), w), name
    assert want[0].any() and (want[3] == sc['site_moving']).any() and (want[3] & ~np.uint8(sc['site_moving']) != 0).any()


@pytest.mark.parametrize("control", ["sun_shift", "rows_shift", "dark_flip", "limb_raised"])
def test_controls(dev, control):
    """the Sun rows shifted by one sample, the moving sensor's rows shifted by one sample, a dark bit flipped, limb_radius raised: accept
    changes for the candidates numpy says it changes, and for no others"""
    n = max(sn.SIZES_N)
    sc, cand = sn.scene('S3c', sn.T_BIG), sn.candidates(n)
    (base_np, _, _, _), close0 = sn.reference('S3c', sn.T_BIG, n)
    over = sn.controls(sc)[control]
    (acc_np, _, _, _), close1 = sn.run_numpy(cand, sc, pos=sn.positions(n, sn.T_BIG), **over)
    base, got = _launch(dev, cand, sc)[0], _launch(dev, cand, sc, **over)[0]
    assert not close0.any() and not close1.any()
    assert np.array_equal(base, base_np) and np.array_equal(got, acc_np)
    assert np.array_equal(got != base, acc_np != base_np) and (got != base).any()


def test_visible_catalogue_network_with_ground_sites_is_visible_catalogue(dev):
    """ground sites only and no illumination: visible_catalogue's rows bit for bit (n = 60, seed = 3), default site and 3 sites"""
    from ssa_gym_amd import catalogue
    assert np.array_equal(catalogue.visible_catalogue_network(60, seed=3, sensors=[catalogue.DEFAULT_SITE]),
                          catalogue.visible_catalogue(60, seed=3))
    assert np.array_equal(catalogue.visible_catalogue_network(60, seed=3, sensors=_SITES3, el_min_deg=[15.0, 10.0, 20.0]),
                          catalogue.visible_catalogue(60, seed=3, sites=_SITES3, el_min_deg=[15.0, 10.0, 20.0]))
    assert catalogue.visible_catalogue_network(0, sensors=[catalogue.DEFAULT_SITE]).shape == (0, 6)


def test_an_orbit_that_dips_below_the_limb_sphere_is_refused(dev):
    """an eccentric orbit that starts at its apogee, 2 000 km above the LEO sensors, with its perigee 78 km below limb_radius: the
    device's propagation reaches the perigee after 57 minutes, inside the 4 h span -- ValueError, no catalogue"""
    from ssa_gym_amd import catalogue
    from support import orbiting as ob
    ra, rp = ob.LEO + 2000e3, ob.R_LIMB - 78e3
    v = np.sqrt(sn.MU * (2.0 / ra - 2.0 / (ra + rp)))
    with pytest.raises(ValueError, match=r"sensors\[1\].*dips to"):
        catalogue.visible_catalogue_network(10, sensors=[_SITES3[0], {'orbit': [ra, 0.0, 0.0, 0.0, v, 0.0]}], el_min_deg=[15.0, None])


def test_visible_catalogue_network_rows_pass_the_numpy_rule(dev, monkeypatch):
    """the S = 3 scene, n = 200: each row kept passes the numpy rule (on the scene's analytic orbit; the device's two-body arc of the
    same state differs from it by rounding), none of them inside a margin.  The rows' elements are read off the screen's own calls."""
    from ssa_gym_amd import catalogue, device
    sc = sn.scene('S3', sn.T_BIG)
    log, entry = [], device.catalogue_screen_network

    def logged(elements, *a, **kw):
        acc = entry(elements, *a, **kw)
        log.append((tuple(elements.cpu().numpy().T), acc.cpu().numpy().astype(bool)))
        return acc
    monkeypatch.setattr(device, "catalogue_screen_network", logged)
    rows = catalogue.visible_catalogue_network(200, seed=3, sensors=sc['sensors'], el_min_deg=sc['el_min_deg'], illumination=sc['illumination'],
                                               t_0=sn.T_0, step=sn.STEP)
    assert rows.shape == (200, 6) and np.all(np.isfinite(rows))
    el, order = sn.drawn_elements(log, 200, 3)
    a, ecc, inc, raan, argp, nu = el.T
    assert np.array_equal(catalogue.coe2rv_host(a * (1 - ecc ** 2), ecc, inc, raan, argp, nu), rows[order])
    (acc, _, _, seen), close = sn.run_numpy(tuple(el.T), sc)
    print("%d candidates screened for 200 rows; seen by the orbiting sensor alone: %d" % (sum(len(ok) for _, ok in log), (seen == 4).sum()))
    assert acc.all() and not close.any()


def test_the_env_sees_its_catalogue(dev):
    """an env with a ground radar and an orbiting 'sunlit' sensor, given the catalogue screened for it (catalogue_for_network, n = 200):
    stepped over the first window with lookahead_sensors() at each step, every object is visible to some sensor, and at least one to
    the orbiting sensor alone.  The control: catalogue_for_config screens on the ground mask only, so with the ground sensor a
    TELESCOPE (night limit -6 deg) it keeps objects this network never sees in the window.  (With a ground radar it cannot: whatever
    the ground mask accepts, the radar sees within the window.)  step() wants an object per sensor: the actions are arbitrary, the
    truth does not depend on them."""
    from ssa_gym_amd import catalogue
    from ssa_gym_amd import envs as E

    def seen_by(cfg):
        env = E.make('ssa_tasker_simple-v2', config=cfg)
        env.reset()
        seen = np.stack([env.object_visibility(sensor=s) for s in range(env.n_sensor)])          # sample 0
        for _ in range(sn.scene('S3', sn.T_BIG)['first'] - 1):                                    # samples 1 .. first - 1
            seen |= env.lookahead_sensors()["visible"].cpu().numpy().astype(bool)
            env.step(np.array([0, 1]))
        return seen

    cfg = sn.env_cfg(E)
    cfg['orbits'] = catalogue.catalogue_for_network(cfg, n=sn.ENV_N, seed=sn.ENV_SEED)
    assert cfg['orbits'].shape == (sn.ENV_N, 6)
    seen = seen_by(cfg)
    print("seen by the radar %d, by the orbiting sensor %d, by it alone %d of %d" % (seen[0].sum(), seen[1].sum(), (seen[1] & ~seen[0]).sum(), sn.ENV_N))
    assert seen.any(axis=0).all() and (seen[1] & ~seen[0]).any()
    tel = sn.env_cfg(E, telescope=sn.ENV_TELESCOPE)
    tel['orbits'] = catalogue.catalogue_for_config(tel, n=sn.ENV_N, seed=sn.ENV_SEED, step=sn.STEP)
    unseen = int((~seen_by(tel).any(axis=0)).sum())
    print("objects of the ground-mask catalogue the telescope network never sees in the window: %d of %d" % (unseen, sn.ENV_N))
    assert unseen > 0
