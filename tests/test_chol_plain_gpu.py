"""The plain family's factorisation (chol_step_fused / chol_row_regs_fused / chol_store_rows_zeroed, ssa_kernels.hip): the row broadcasts
folded into v_fmac_f64_dpp, no select per step, the verdicts on the scalar unit, the factor tile's lower triangle zeroed where the rows are
stored.  The yardstick is the generic instance (HotPathEngine.force_generic), which keeps chol_step as it was.

Everything a step writes -- truth, state, covariance, status, observation rows, metrics, the update record, the statistics rows once
flushed, the failure records and their count -- must be the same BITS in both instances:

  sizes and modes   3 objects (a ragged tile only), 4, 8, 66, 260; `hybrid` with and without a storage layout, `fg`; one step and ten
                    consecutive steps; a planted NaN state and a filter failed at entry in every one of them
  factorisations    one object per case, arranged so that the four rows of a wavefront always fail DIFFERENTLY and every case stands in
                    row 0 of one tile and in row 3 of another (and in rows 1 and 2 of two more): a NaN entry, +inf on the diagonal at each
                    index (an infinite pivot at J < 5 gives y = 0: only the finite test catches it), an infinite off-diagonal entry, a
                    negative pivot at each J; the ladder's hardest input (tests/golden/ladder_illconditioned_tile.npz) as recorded and
                    rotated by three rows; the 26 diverged priors of tests/golden/transform_tile_diverged.npz
  lower triangle    the plain instance's factor tile is not an output, its sigma points x +- U[row] are what everything downstream is
                    made of: a word the transform or the update of an earlier step left below the diagonal moves a sigma point and with
                    it the covariance's bits.  The ten-step cases run launch after launch on tiles whose factor block the previous step
                    used as scratch.  What the arithmetic itself leaves in the lanes below the diagonal is small for a symmetric matrix
                    (the terms cancel), so one tile of the factorisation cases holds healthy matrices with a LOWER triangle of 1e9's:
                    the factorisation reads the upper one only, and what it leaves below is then as large as the factor.  What the
                    factor has to be -- zeros below the diagonal, exactly +0.0 -- is pinned on the generic ladder through
                    ssa_ladder_probe_f64 for every planted matrix, so equal bits mean that factor.  (Checked once by hand: a library
                    built without the write of entries (5, 3) and (5, 4) fails this file.)

The planted matrices are checked through the probe (the generic ladder) before use: the non-finite ones exhaust the ladder, the negative
pivots fail the first attempt, so the comparison covers the first attempt's verdict, the ladder's, and the winning rung's re-factorisation."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
from support.batches import c2t, make_batch
from support.gpu import hip  # noqa: F401  (the module fixture)
from support.plain_step import H, bits, planted, slot_of

pytestmark = pytest.mark.gpu

SIZES = [3, 4, 8, 66, 260]
SCALE = 3e-8       # n + lambda of the module's filters: alpha = 1e-4, kappa = -3, n = 6


def _run(hip, m, propagator, layout, generic, n_steps, state=None):
    """n_steps deferred-fold steps on the two-slot ring: what every step wrote, every statistics row once folded, the failure log, the
    instances the launches took.  state: (x_true, x, P) instead of the planted batch"""
    from ssa_gym_amd import parallel
    L = hip.lib
    g = make_batch(8, seed=1)[3]
    consts = hip.host.make_consts(g["Q"], g["R"], 1e-4, 2.0, -3, 20.0, np.radians(20.0), g["obs_lla"], obs_type='aer', propagator=propagator)
    n_time = n_steps + 1
    if state is None:
        xt, x, P, _ = make_batch(m, seed=1300 + m)
        nan_obj, failed_obj = planted(m)
        x[nan_obj, 1] = np.nan
        sched = ([0, nan_obj, failed_obj, m - 1, 0, 1 % m] * 2)[:n_steps]
    else:
        xt, x, P = state
        sched = [(5 * k) % m for k in range(n_steps)]
    zn = np.random.RandomState(3).normal(size=(1, n_time, m, 3)) * np.array([4.8e-6, 4.8e-6, 1e3])
    eng = hip.engine.HotPathEngine(consts, m, 1, c2t()[:n_time], zn, history=H)
    eng.force_generic = generic
    if layout:
        eng.set_layout(np.random.RandomState(m).permutation(m))
    eng.load_state(0, xt, x, P)
    if state is None:
        eng.status[int(eng._slot_of[failed_obj]) if layout else failed_obj] = L.ST_UPDATE_LINALG
    assert eng.stats_from_metrics
    local = parallel.HipLocalStepper(eng, consts, fast_stats=True, defer_fold=True)
    local.load_schedule(sched)
    steps, rows = [], {}
    for _ in range(n_steps):
        local.step(-1)
        steps.append(slot_of(eng, local.tick % H))
        if local.tick > 1:
            rows[local.tick - 1] = bits(eng.stats[(local.tick - 1) % H])      # folded by the launch just enqueued
    local.flush()
    rows[local.tick] = bits(eng.stats[local.tick % H])
    hip.torch.cuda.synchronize()
    nf = int(eng.fail_count.cpu().numpy()[0])
    log = np.array(sorted(map(tuple, eng.fail_log[:nf]), key=lambda r: (r[L.FAIL_TIME], r[L.FAIL_OBJ])), dtype=np.float64)
    log = log.reshape(nf, -1) if nf else np.zeros((0, L.FAIL_STRIDE))
    lib = L.load()
    inst = {int(lib.ssa_env_step_instance(eng._cref, C.byref(ent[0]))) for ent in eng._pcache.values()}
    return dict(steps=steps, rows=rows, nfail=nf, fail_log=log, instances=inst)


def _assert_same_bits(hip, want, got, what):
    eq = hip.torch.equal
    assert want["instances"] == {0} and got["instances"] == {1}, what      # generic launches only | plain ones only
    assert len(want["steps"]) == len(got["steps"]) and sorted(want["rows"]) == sorted(got["rows"]) == list(range(1, len(want["steps"]) + 1))
    for t, (a, b) in enumerate(zip(want["steps"], got["steps"])):
        for k in a:
            assert eq(a[k], b[k]), (what, "step", t + 1, k)
    for t in want["rows"]:
        assert eq(want["rows"][t], got["rows"][t]), (what, "statistics row of step", t)
    assert want["nfail"] == got["nfail"], what
    assert np.array_equal(want["fail_log"].view(np.int64), got["fail_log"].view(np.int64)), what


@pytest.mark.parametrize("n_steps", [1, 10])
@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("case", ["hybrid", "hybrid-layout", "fg"])
def test_the_fused_factorisation_gives_the_generic_instances_bits(hip, case, m, n_steps):
    L = hip.lib
    propagator, layout = ("fg", False) if case == "fg" else ("hybrid", case == "hybrid-layout")
    want = _run(hip, m, propagator, layout, True, n_steps)
    got = _run(hip, m, propagator, layout, False, n_steps)
    _assert_same_bits(hip, want, got, (case, m, n_steps))
    # the comparison is one of live filters with a finite covariance, the two planted ones apart
    nan_obj, failed_obj = planted(m)
    order = np.random.RandomState(m).permutation(m) if layout else np.arange(m)
    at = {int(o): i for i, o in enumerate(order)}
    st = want["steps"][-1]["status"].cpu().numpy()
    assert st[at[failed_obj]] == L.ST_UPDATE_LINALG and st[at[nan_obj]] != 0 and want["nfail"] >= 1
    alive = st == 0
    assert alive.sum() >= m - 2
    P_end = want["steps"][-1]["P"].view(hip.torch.float64).cpu().numpy().reshape(m, 36)
    assert np.isfinite(P_end[alive]).all()


# ---- the factorisation cases

def _negative_pivot(P, J):
    """P with its diagonal entry J lowered so that pivot J of the factorisation of (n + lambda) P is the NEGATIVE of what it was (the
    pivots before it unchanged: they do not read the entry)"""
    U = np.linalg.cholesky(SCALE * P).T
    Q = P.copy()
    Q[J, J] -= 2.0 * U[J, J] ** 2 / SCALE
    return Q


def _cases(P):
    """(name, matrix) from the healthy covariance P: every one fails the first attempt in its own way"""
    out = []
    Q = P.copy()
    Q[2, 3] = Q[3, 2] = np.nan
    out.append(("nan", Q))
    for d in range(6):
        Q = P.copy()
        Q[d, d] = np.inf
        out.append(("inf-diagonal-%d" % d, Q))
    Q = P.copy()
    Q[1, 4] = Q[4, 1] = np.inf
    out.append(("inf-off-diagonal", Q))
    for J in range(6):
        out.append(("negative-pivot-%d" % J, _negative_pivot(P, J)))
    return out


@pytest.fixture(scope="module")
def planted_tiles(hip):
    """(x_true, x, P, names): tile i holds the cases i, i + 1, i + 2, i + 3 (cyclic) -- every case once in each row, no two rows of a
    wavefront alike -- then the ladder's recorded tile as it is and rotated by three rows, then healthy objects up to a ragged tile.
    Checked through the probe: what each matrix does to the generic ladder, and the factor's lower triangle."""
    xt0, x0, P0, _ = make_batch(4, seed=77)
    cases = _cases(P0[0])
    n = len(cases)
    names, mats = [], []
    for i in range(n):
        for r in range(4):
            name, Q = cases[(i + r) % n]
            names.append(name)
            mats.append(Q)
    tile = golden("ladder_illconditioned_tile.npz")
    lad_x = [tile["x_tile"][r] for r in range(4)] + [tile["x_tile"][(r + 1) % 4] for r in range(4)]
    lad_P = [tile["P_tile"][r] for r in range(4)] + [tile["P_tile"][(r + 1) % 4] for r in range(4)]      # (row 0 lands in row 3)
    m_cases = len(mats)
    m = m_cases + 8 + 4 + 6
    xt, x, P, _ = make_batch(m, seed=78)
    P[:m_cases] = np.array(mats)
    x[m_cases:m_cases + 8] = np.array(lad_x)
    xt[m_cases:m_cases + 8] = np.array(lad_x) + np.array([3e3, -2e3, 1e3, 1.0, -1.0, 0.5])
    P[m_cases:m_cases + 8] = np.array(lad_P)
    # one whole tile of healthy matrices whose LOWER triangle is something else altogether (the factorisation reads the upper one, as
    # scipy does): what the lanes below the diagonal are left with is then large, and only the zeros written over it keep it out
    for k in range(m_cases + 8, m_cases + 12):
        P[k][np.tril_indices(6, -1)] = 1e9 - 3.0 * P[k].T[np.tril_indices(6, -1)]
    names += ["ladder"] * 8 + ["healthy"] * 10
    for i in range(n):      # the arrangement is what the docstring says
        assert len({names[4 * i + r] for r in range(4)}) == 4
    for name, _ in cases:
        assert {k % 4 for k, nm in enumerate(names[:m_cases]) if nm == name} == {0, 1, 2, 3}
    rung, mask, U = hip.dev.ladder_probe(hip.dev.as_dev(P), SCALE)
    rung, mask, U = rung.cpu().numpy(), mask.cpu().numpy(), U.cpu().numpy().reshape(m, 6, 6)
    for k, nm in enumerate(names):
        if nm == "nan" or nm.startswith("inf"):
            assert rung[k] == 16, (k, nm, rung[k])
        elif nm.startswith("negative"):
            assert rung[k] >= 0 and not (mask[k] & 0x10000), (k, nm, rung[k])
        elif nm == "healthy":
            assert rung[k] == -1, (k, nm, rung[k])
    assert (rung[m_cases:m_cases + 8] >= 0).any()        # the recorded tile needs the ladder
    assert (rung[:m_cases] < 16).any() and (rung[:m_cases] == 16).any()
    low = U[:, np.tril_indices(6, -1)[0], np.tril_indices(6, -1)[1]]
    assert (low.view(np.int64) == 0).all()               # exactly +0.0 below the diagonal, failed ladders included
    return xt, x, P, names


@pytest.mark.parametrize("n_steps", [1, 3])
def test_every_way_to_fail_in_every_row_gives_the_generic_instances_bits(hip, planted_tiles, n_steps):
    L = hip.lib
    xt, x, P, names = planted_tiles
    state = (xt.copy(), x.copy(), P.copy())
    want = _run(hip, len(x), "hybrid", False, True, n_steps, state=state)
    got = _run(hip, len(x), "hybrid", False, False, n_steps, state=state)
    _assert_same_bits(hip, want, got, ("cases", n_steps))
    st = want["steps"][0]["status"].cpu().numpy()
    for k, nm in enumerate(names):
        if nm == "nan" or nm.startswith("inf"):
            assert st[k] == L.ST_PREDICT_LINALG, (k, nm, st[k])       # the ladder exhausted, in the step's own predict
        elif nm == "healthy":
            assert st[k] == 0, (k, nm, st[k])
    assert want["nfail"] >= sum(nm == "nan" or nm.startswith("inf") for nm in names)


@pytest.mark.parametrize("m", [26, 66])
def test_the_diverged_priors_give_the_generic_instances_bits(hip, m):
    f = golden("transform_tile_diverged.npz")
    xt, x, P = f["x_true"], f["x"], f["P"]
    assert len(x) == 26
    pick = (np.arange(m) * 3) % len(x)      # (26 and 3 are coprime: every prior, and at 66 objects in other rows and tiles again)
    assert set(pick) == set(range(len(x)))
    state = (xt[pick].copy(), x[pick].copy(), P[pick].copy())
    want = _run(hip, m, "hybrid", m > 26, True, 10, state=state)
    got = _run(hip, m, "hybrid", m > 26, False, 10, state=state)
    _assert_same_bits(hip, want, got, ("diverged", m))
    st0 = want["steps"][0]["status"].cpu().numpy()
    assert (st0 == 0).sum() >= (m + 1) // 2
