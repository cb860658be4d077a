"""The two recipes that make the UKF update fail inside a step (tests/support/update_failures.py), pinned to the fp64 oracle: if a batch
or a golden ever changes so that a recipe stops failing, it shows here, on the CPU, and not as a vacuous pass on the GPU.

The reference's behaviour (ssa_tasker_simple_2.py:300-315, 369-382): 'update returned nan' books the update first (obs_taken, y, S,
sigmas_h) and then calls filter_error; a LinAlgError of inv(S) books nothing; filter_error plants the sentinels."""
import numpy as np
import pytest

from ssa_gym_amd import host
from support.batches import make_batch
from support import update_failures as uf

CASES = [(ot, rs) for ot in ('aer', 'xyz') for rs in (False, True)]


def _inputs(obs_type):
    xt, x, P, g = make_batch(uf.HOST_M, seed=uf.HOST_SEED)
    zn = uf.noise_table(1, 8, uf.HOST_M)
    return xt, x, P, g, zn, uf.golden_R(g, obs_type)


def _sentinels(r, a):
    return np.array_equal(r["x"][a], host.X_FAILED) and np.array_equal(r["P"][a], host.P_FAILED)


@pytest.mark.parametrize("obs_type,resample", CASES)
def test_nan_noise_gives_update_nan_with_the_update_booked(oracle, obs_type, resample):
    xt, x, P, g, zn, R = _inputs(obs_type)
    a, tix = uf.HOST_ACTION, uf.HOST_TIX
    clean = uf.oracle_step(oracle, xt, x, P, g, a, tix, obs_type, resample, R, zn[0, tix, a])
    assert np.all(clean["status"] == 0) and clean["obs_taken"] and np.isfinite(clean["y"]).all()
    for comp in range(3):
        z = uf.nan_noise(zn, 0, tix, a, comp)
        r = uf.oracle_step(oracle, xt, x, P, g, a, tix, obs_type, resample, R, z[0, tix, a])
        want = np.zeros(uf.HOST_M, dtype=np.int32)
        want[a] = 3
        assert np.array_equal(r["status"], want), (comp, r["status"])
        assert r["obs_taken"] is True                                    # booked before filter_error (:305)
        assert np.isfinite(r["S"]).all() and uf.same_bits(r["S"], clean["S"])      # S does not depend on the noise
        assert uf.same_bits(r["z_true"], clean["z_true"]) and uf.same_bits(r["sigmas_h"], clean["sigmas_h"])
        nan_at = tuple(np.where(np.isnan(r["y"]))[0])
        assert nan_at == uf.Y_NAN[(obs_type, comp)], (obs_type, comp, r["y"])
        keep = ~np.isnan(r["y"])
        assert uf.same_bits(r["y"][keep], clean["y"][keep])
        assert _sentinels(r, a)
        others = np.arange(uf.HOST_M) != a
        assert uf.same_bits(r["x"][others], clean["x"][others]) and uf.same_bits(r["P"][others], clean["P"][others])


@pytest.mark.parametrize("obs_type,resample", CASES)
def test_overflowing_R_gives_update_linalg_with_nothing_booked(oracle, obs_type, resample):
    xt, x, P, g, zn, R = _inputs(obs_type)
    a, tix = uf.HOST_ACTION, uf.HOST_TIX
    clean = uf.oracle_step(oracle, xt, x, P, g, a, tix, obs_type, resample, R, zn[0, tix, a])
    r = uf.oracle_step(oracle, xt, x, P, g, a, tix, obs_type, resample, uf.R_OVERFLOW, zn[0, tix, a])
    want = np.zeros(uf.HOST_M, dtype=np.int32)
    want[a] = 4
    assert np.array_equal(r["status"], want), r["status"]
    assert r["obs_taken"] is False                                       # (:312-315: the except branch books nothing)
    assert _sentinels(r, a)
    assert uf.same_bits(r["z_true"], clean["z_true"])                    # hx(x_true) is recorded before the update is tried (:298)
    # R touches the updated object alone: every other object bit for bit as with the golden R
    others = np.arange(uf.HOST_M) != a
    assert np.all(clean["status"] == 0)
    for k in ("x", "P", "x_true"):
        assert uf.same_bits(r[k][others], clean[k][others]), k
    # the recipe is what it says: every entry of R finite, the determinant of S not
    assert np.isfinite(uf.R_OVERFLOW).all() and np.count_nonzero(uf.R_OVERFLOW) == 3
    with np.errstate(over='ignore'):
        assert np.isinf(np.prod(np.diag(uf.R_OVERFLOW)))


@pytest.mark.parametrize("obs_type,resample", CASES)
def test_hidden_object_with_overflowing_R_is_not_touched(oracle, obs_type, resample):
    """the visibility gate comes first (:299): below the elevation mask no update is tried, so nothing can fail"""
    xt, x, P, g, zn, R = _inputs(obs_type)
    tix, lim = uf.HOST_TIX, np.radians(15.0)
    z = oracle.hx_aer(oracle.propagate(xt, 20.0), uf.c2t()[tix], g["obs_lla"], g["obs_itrs"])
    hidden = int(np.where(z[:, 1] < lim - 0.1)[0][0])
    seen = int(np.where(z[:, 1] > lim + 0.1)[0][0])
    r = uf.oracle_step(oracle, xt, x, P, g, hidden, tix, obs_type, resample, uf.R_OVERFLOW, zn[0, tix, hidden], obs_limit=lim)
    assert np.all(r["status"] == 0) and r["obs_taken"] is False
    assert np.isfinite(r["x"]).all() and np.abs(r["x"]).max() < 1e9
    r = uf.oracle_step(oracle, xt, x, P, g, seen, tix, obs_type, resample, uf.R_OVERFLOW, zn[0, tix, seen], obs_limit=lim)
    assert r["status"][seen] == 4 and np.count_nonzero(r["status"]) == 1      # (the same mask lets a visible object fail)
