"""Operator-level parity of the heuristic-agent kernels (include/ssa_hip.h, "device-side agent primitives" and
ssa_agent_select_f64) against a high-precision restatement of the reference's agents.py in numpy.

The closed-loop tests compare the device with the device: agents.py, ssa_agent_select_f64 and closed_loop_kernel all evaluate the same
agent_score_rows / logdet_chol, so an error in that shared arithmetic passes all of them.  Here each score row is held against numpy:
  row 0  trace(P)                    bit-equal to the sequential index-order sum (= np.trace for a 6 x 6)
  row 1  log(det P / det P_prev)     against log-determinants from a batched LU with partial pivoting in np.longdouble (80-bit on x86):
                                     the device must be no further from that value than numpy's fp64 expression of agents.py:24 is
                                     (factor 3, as test_hip_step.check_parity), plus a stated floor;  NaN exactly where numpy's Cholesky
                                     of either matrix fails (logdet_chol takes a plain Cholesky factor: the documented deviation)
  rows 2, 3  |x - x_true| of position / velocity   within 4 ulp of np.linalg.norm
  mask   elevation(x_true) >= obs_limit             the oracle's hx_aer, exact outside a band of 3e-13 rad around the limit
and the two-pass selection (per-block first maxima, then one fold per env) against np.argmax over each env's qualifying objects.
"""
import fractions

import numpy as np
import pytest

from conftest import golden
from support.gpu import namespace

EPS = np.finfo(np.float64).eps
N_TIME = 480
LIM = np.radians(15.0)
BAND = 3e-13          # [rad] the device's hx_aer agrees with the oracle's to 1e-13 (test_hip_ops.test_visible_mask_observe_aerobs_vs_oracle)
SIZES = (1, 63, 255, 256, 257, 2049, 20000)
COND_CLASSES = ("P0", "Pu_a3", "cond 1e6", "cond 1e8", "cond 1e10", "cond 1e12", "cond 1e14")


# ------------------------------------------------------------------ the yardstick (CPU)
def lu_logdet_ld(A):
    """(sign, log|det|) of every matrix of A[n, 6, 6]: LU with partial pivoting in np.longdouble.  sign 0 / log -inf for a zero pivot,
    NaN for a non-finite matrix."""
    a = np.array(A, dtype=np.longdouble).reshape(-1, 6, 6)
    n = a.shape[0]
    rows = np.arange(n)
    sign = np.ones(n, dtype=np.longdouble)
    with np.errstate(all="ignore"):
        for k in range(6):
            p = k + np.argmax(np.abs(a[:, k:, k]), axis=1)
            swap = p != k
            rk = a[rows, k, :].copy()
            a[rows, k, :] = a[rows, p, :]
            a[rows, p, :] = rk
            sign[swap] = -sign[swap]
            piv = a[:, k, k]
            f = a[:, k + 1:, k] / piv[:, None]
            a[:, k + 1:, k:] -= f[:, :, None] * a[:, None, k, k:]
        d = np.diagonal(a, axis1=1, axis2=2)
        sign = sign * np.prod(np.sign(d), axis=1)
        logabs = np.sum(np.log(np.abs(d)), axis=1)
    return sign, logabs


def det_ld(A):
    """det of every matrix of A[n, 6, 6] as the product of the long-double LU pivots"""
    s, l = lu_logdet_ld(A)
    return s * np.exp(l)


def log_ratio_ld(P, Pp):
    """agents.py:24, log(det P / det P_prev), in long double: NaN where the two determinants do not share a sign"""
    s1, l1 = lu_logdet_ld(P)
    s2, l2 = lu_logdet_ld(Pp)
    with np.errstate(invalid="ignore"):
        return np.where(s1 * s2 > 0, l1 - l2, np.nan)


def log_ratio_f64(P, Pp):
    """the reference's own fp64 expression (agents.py:24)"""
    with np.errstate(all="ignore"):
        return np.log(np.linalg.det(P) / np.linalg.det(Pp))


def det_exact(M):
    """exact determinant of an integer matrix (fraction-free Gaussian elimination)"""
    a = [[fractions.Fraction(int(v)) for v in row] for row in M]
    n, det = len(a), fractions.Fraction(1)
    for k in range(n):
        p = next((r for r in range(k, n) if a[r][k] != 0), None)
        if p is None:
            return fractions.Fraction(0)
        if p != k:
            a[k], a[p] = a[p], a[k]
            det = -det
        det *= a[k][k]
        for r in range(k + 1, n):
            f = a[r][k] / a[k][k]
            for c in range(k, n):
                a[r][c] -= f * a[k][c]
    return det


def test_long_double_lu_yardstick_vs_exact_determinants():
    """the long-double LU against exact rational determinants of integer 6 x 6 matrices: a zero leading pivot (pivoting), negative
    determinants, a nearly singular matrix with a large cancellation, and large entries.  The bound is 64 units of the long double
    (2^-63 relative), far below what the fp64 expression can resolve on the same matrices."""
    rs = np.random.RandomState(11)
    mats = [rs.randint(-9, 10, size=(6, 6)) for _ in range(6)]
    z = rs.randint(-5, 6, size=(6, 6))
    z[0, 0] = 0
    mats.append(z)                                                     # a zero (1, 1) entry: row exchanges needed
    near = rs.randint(-4, 5, size=(6, 6))
    near[5] = near[0] + near[1] - near[2]
    near[5, 5] += 1                                                    # det small against the entries' products
    mats.append(near)
    mats.append(rs.randint(-10 ** 5, 10 ** 5, size=(6, 6)))
    sym = rs.randint(-3, 4, size=(6, 6))
    mats.append(sym @ sym.T + 6 * np.eye(6, dtype=np.int64))          # a covariance-like matrix
    A = np.array(mats, dtype=np.float64)
    got = det_ld(A)
    ulp = float(np.finfo(np.longdouble).eps)
    assert ulp < 1e-18, "np.longdouble is not the 80-bit extended type on this host"
    n_neg = 0
    for M, g in zip(mats, got):
        ex = det_exact(M)
        assert ex != 0
        n_neg += ex < 0
        rel = abs(fractions.Fraction(*g.as_integer_ratio()) - ex) / abs(ex)
        assert rel <= 64 * ulp, (M, float(ex), float(g), float(rel))
    assert n_neg >= 2
    # the log of the ratio: sign rule and value
    s, l = lu_logdet_ld(A)
    assert np.all(s == np.sign([float(det_exact(M)) for M in mats]))
    lr = log_ratio_ld(A[:-1], A[1:])
    for k in range(len(mats) - 1):
        q = det_exact(mats[k]) / det_exact(mats[k + 1])
        if q < 0:
            assert np.isnan(lr[k])
        else:
            exact = np.log(np.longdouble(str(q.numerator)) / np.longdouble(str(q.denominator)))
            assert abs(lr[k] - exact) <= 1e-17 * max(1.0, abs(float(exact))), (k, lr[k], exact)


# ------------------------------------------------------------------ helpers shared by the GPU tests
def sym(A):
    """exactly symmetric (the kernels read the upper triangle, numpy the whole matrix)"""
    return 0.5 * (A + np.swapaxes(A, -1, -2))


def upper(A):
    """the symmetric matrices of A's upper triangles (what the kernels read)"""
    return np.triu(A) + np.swapaxes(np.triu(A, 1), -1, -2)


def chol_fails(A):
    """numpy's Cholesky verdict per matrix: LinAlgError, or a factor with a non-finite entry (numpy returns NaN / inf factors for
    non-finite input instead of raising)"""
    A = np.asarray(A).reshape(-1, 6, 6)
    try:
        with np.errstate(all="ignore"):
            L = np.linalg.cholesky(A)
        return ~np.isfinite(L).all(axis=(1, 2))
    except np.linalg.LinAlgError:
        out = np.zeros(len(A), dtype=bool)
        for k, a in enumerate(A):
            try:
                with np.errstate(all="ignore"):
                    out[k] = not np.isfinite(np.linalg.cholesky(a)).all()
            except np.linalg.LinAlgError:
                out[k] = True
        return out


def scaled_cond(A):
    """condition number of the correlation matrix D^-1/2 A D^-1/2 (what a Cholesky factor's rounding error depends on)"""
    d = 1.0 / np.sqrt(np.abs(np.einsum("kii->ki", A)))
    return np.linalg.cond(A * d[:, :, None] * d[:, None, :])


def random_rotations(rs, n):
    q, r = np.linalg.qr(rs.normal(size=(n, 6, 6)))
    return q * np.sign(np.einsum("kii->ki", r))[:, None, :]


def covariances(rs, n):
    """n covariances cycling through COND_CLASSES: the golden P0 (diagonal), the golden Pu_a3 posteriors and s Q diag(lambda) Q^T
    with cond 1e6 .. 1e14; and P_prev, a grown copy: 1.5 P plus a rank-one term."""
    g = golden("ukf_step_golden.npz")
    cls = np.arange(n) % len(COND_CLASSES)
    P = np.empty((n, 6, 6))
    P[cls == 0] = g["P0"]
    k1 = np.where(cls == 1)[0]
    P[k1] = sym(g["Pu_a3"])[k1 % 64]
    for c, lg in zip(range(2, 7), (6, 8, 10, 12, 14)):
        kc = np.where(cls == c)[0]
        if len(kc):
            Q = random_rotations(rs, len(kc))
            lam = 10.0 ** np.linspace(0.0, -lg, 6)[None, :] * 10.0 ** rs.uniform(4, 10, size=(len(kc), 1))
            P[kc] = sym(np.einsum("kij,kj,klj->kil", Q, lam, Q))
    u = rs.normal(size=(n, 6)) * np.sqrt(np.einsum("kii->ki", P))
    Pp = sym(1.5 * P + 0.3 * u[:, :, None] * u[:, None, :])
    return P, Pp, cls


def states(rs, n):
    """true states from the catalogue subset (displaced a little, so that repeats differ) and perturbed filter means"""
    cat = golden("catalogue_subset.npy")
    xt = cat[rs.randint(0, len(cat), n)] + rs.normal(size=(n, 6)) * np.array([1e3] * 3 + [1.0] * 3)
    x = xt + rs.normal(size=(n, 6)) * np.array([1e5] * 3 + [1e2] * 3)
    return xt, x


def shannon_criterion(dev, P, Pp, tag, classes=None):
    """row 1 against the long-double value ld.  Per object: |dev - ld| <= 3 |fp64 - ld| + floor, floor = 1e-12 + 2 eps (k + k_prev), k the
    scaled condition numbers (a backward-stable factorisation's log-det moves by about eps k: two independent evaluations of an
    ill-conditioned determinant differ by that much whichever is "better" on a given matrix).  Per conditioning class of at least 50
    objects, as test_hip_step.check_parity: the median error within 3x the fp64 expression's + 1e-13.  Returns the device errors."""
    ld = log_ratio_ld(P, Pp)
    r64 = log_ratio_f64(P, Pp)
    fin = np.isfinite(ld)
    assert np.isfinite(dev[fin]).all() and np.isfinite(r64[fin]).all(), tag
    g = np.abs(dev - ld.astype(np.float64))
    r = np.abs(r64 - ld.astype(np.float64))
    floor = 1e-12 + 2 * EPS * (scaled_cond(P) + scaled_cond(Pp))
    bad = fin & (g > 3 * r + floor)
    assert not bad.any(), (tag, np.where(bad)[0][:8], g[bad][:8], r[bad][:8], floor[bad][:8])
    names = COND_CLASSES if classes is not None else ("all",)
    classes = np.zeros(len(P), dtype=int) if classes is None else classes
    for c in np.unique(classes[fin]):
        k = fin & (classes == c)
        print("[shannon %s %s] n=%d  |dev - ld| median %.2e max %.2e   |fp64 - ld| median %.2e max %.2e"
              % (tag, names[c], k.sum(), np.median(g[k]), g[k].max(), np.median(r[k]), r[k].max()))
        if k.sum() >= 50:
            assert np.median(g[k]) <= 3 * np.median(r[k]) + 1e-13, (tag, names[c])
    return g


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def hip():
    h = namespace()
    torch, device, host = h.torch, h.dev, h.host
    h.up = lambda a, dtype=torch.float64: device.as_dev(np.ascontiguousarray(a), "cuda", dtype)
    g = golden("ukf_step_golden.npz")
    h.g = g
    h.c2t = golden("c2t_2020-05-04_dt20_n480.npy")
    h.consts = lambda lim=LIM: host.make_consts(g["Q"], g["R"], 1e-4, 2.0, -3, 20.0, lim, g["obs_lla"], obs_type="aer")
    h.obs_itrs = np.array(h.consts().obs_itrs[:])
    return h


def elevation(oracle, hip, xt, M):
    return oracle.hx_aer(xt, M, hip.g["obs_lla"], hip.obs_itrs)[:, 1]


def scores_of(hip, xt, x, P, Pp, M, consts):
    sc, mask = hip.dev.agent_scores(hip.up(xt), hip.up(x), hip.up(P), hip.up(Pp) if Pp is not None else None, hip.up(M), consts)
    return sc.cpu().numpy(), mask.cpu().numpy()


@pytest.mark.gpu
def test_agent_scores_vs_numpy(hip, oracle):
    rs = np.random.RandomState(21)
    c = hip.consts()
    M = hip.c2t[3]
    band_total = 0
    for n in SIZES:
        xt, x = states(rs, n)
        P, Pp, cls = covariances(rs, n)
        sc, mask = scores_of(hip, xt, x, P, Pp, M, c)
        assert sc.shape == (4, n) and mask.shape == (n,)
        # row 0: the sequential sum in index order, which is what np.trace computes for six entries
        seq = np.zeros(n)
        for k in range(6):
            seq = seq + P[:, k, k]
        assert np.array_equal(seq, np.trace(P, axis1=1, axis2=2))
        assert np.array_equal(sc[0], seq), n
        # row 1
        assert not chol_fails(P).any() and not chol_fails(Pp).any()
        shannon_criterion(sc[1], P, Pp, "n=%d" % n, cls)
        # rows 2 and 3
        for row, sl in ((2, slice(0, 3)), (3, slice(3, 6))):
            ref = np.linalg.norm(x[:, sl] - xt[:, sl], axis=1)
            assert np.all(np.abs(sc[row] - ref) <= 4 * np.spacing(ref)), (n, row)
        # mask
        el = elevation(oracle, hip, xt, M)
        band = np.abs(el - LIM) < BAND
        band_total += band.sum()
        assert np.array_equal(mask[~band].astype(bool), (el >= LIM)[~band]), n
        assert band.sum() <= max(1, n // 10000), (n, band.sum())
        if n >= 2049:
            assert 0.02 < mask.mean() < 0.98, (n, mask.mean())
        # no previous covariance: row 1 all NaN, the rest unchanged
        sc0, mask0 = scores_of(hip, xt, x, P, None, M, c)
        assert np.isnan(sc0[1]).all()
        assert np.array_equal(sc0[[0, 2, 3]], sc[[0, 2, 3]]) and np.array_equal(mask0, mask)
    print("[mask] objects within %.0e rad of the limit (not compared): %d of %d" % (BAND, band_total, sum(SIZES)))


def broken_covariances(rs):
    """(name, matrix) pairs without a Cholesky factor"""
    g = golden("ukf_step_golden.npz")
    Q = random_rotations(rs, 3)
    out = [("det < 0", sym(Q[0] @ np.diag([1e10, 1e8, 1e6, 1e4, 1e2, -1e3]) @ Q[0].T)),
           ("two negative eigenvalues, det > 0", sym(Q[1] @ np.diag([1e10, 1e8, 1e6, 1e4, -1e2, -1e3]) @ Q[1].T))]
    # the late-episode case: diagonal entries 1e14 .. 1e21, rank five (J J^T), and a negative last pivot of 1e-12 of its diagonal entry:
    # the negative eigenvalue is far below the rounding of the largest one, yet both factorisations see it (their own rounding of that
    # pivot is ~1e-15 of the entry)
    d = 10.0 ** np.array([10.5, 10.0, 9.5, 8.0, 7.5, 7.0])
    J = d[:, None] * random_rotations(rs, 1)[0][:, :5]
    R = sym(J @ J.T)
    R[5, 5] -= 1e-12 * R[5, 5]
    out.append(("rank five, rounding-level negative eigenvalue", R))
    nan = sym(g["P0"].copy())
    nan[1, 4] = nan[4, 1] = np.nan
    out.append(("NaN entry", nan))
    inf = sym(g["P0"].copy())
    inf[0, 3] = inf[3, 0] = np.inf
    out.append(("inf entry", inf))
    out.append(("zero matrix", np.zeros((6, 6))))
    return out


@pytest.mark.gpu
def test_agent_scores_without_a_cholesky_factor(hip):
    """row 1 is NaN exactly where numpy's Cholesky of either matrix fails; rows 0, 2, 3 and the mask do not notice"""
    rs = np.random.RandomState(22)
    c = hip.consts()
    M = hip.c2t[7]
    cases = broken_covariances(rs)
    R = cases[2][1]
    lam = np.linalg.eigvalsh(R)
    print("[broken] rank-five case: |lambda|_min / lambda_max = %.1e (fp64 eigvalsh), diagonal %.1e .. %.1e"
          % (np.abs(lam).min() / lam[-1], np.diag(R).min(), np.diag(R).max()))
    assert lu_logdet_ld(R)[0][0] < 0 and np.abs(lam).min() < 3e-16 * lam[-1]     # one negative eigenvalue, below the rounding of the largest
    n = 300
    xt, x = states(rs, n)
    P, Pp, _ = covariances(rs, n)
    sc_clean, mask_clean = scores_of(hip, xt, x, P, Pp, M, c)
    Pb, Ppb = P.copy(), Pp.copy()
    where = {}
    for k, (name, A) in enumerate(cases):
        where[name] = (3 + 41 * k, 260 + 5 * k)       # in P_cur at the first slot, in P_prev at the second
        Pb[where[name][0]] = A
        Ppb[where[name][1]] = A
    sc, mask = scores_of(hip, xt, x, Pb, Ppb, M, c)
    fails = chol_fails(Pb) | chol_fails(Ppb)
    for name, (i, j) in where.items():
        assert fails[i] and fails[j], name
        assert np.isnan(sc[1, i]) and np.isnan(sc[1, j]), name
    assert np.array_equal(np.isnan(sc[1]), fails)
    assert np.array_equal(sc[1][~fails], sc_clean[1][~fails])
    assert np.array_equal(sc[0], np.trace(Pb, axis1=1, axis2=2), equal_nan=True)
    assert np.array_equal(sc[[2, 3]], sc_clean[[2, 3]]) and np.array_equal(mask, mask_clean)
    # the reference's fp64 expression still gives a finite score where the determinant ratio is positive
    r64 = log_ratio_f64(Pb, Ppb)
    i2, j2 = where["two negative eigenvalues, det > 0"]
    assert np.isfinite(r64[i2]) and np.isfinite(r64[j2])


@pytest.mark.gpu
def test_agent_scores_at_and_visible_mask_at_wrap_the_time_index(hip):
    """the _at variants pick row (env_time[0] + time_offset) % n_time of the table on the device: bit-identical to the plain operators
    given that row, including a sum that wraps past n_time"""
    torch = hip.torch
    rs = np.random.RandomState(23)
    c = hip.consts()
    n = 2049
    xt, x = states(rs, n)
    P, Pp, _ = covariances(rs, n)
    trans = hip.up(hip.c2t.reshape(N_TIME, 9))
    d = [hip.up(a) for a in (xt, x, P, Pp)]
    seen = set()
    for t, off in ((0, 5), (474, 5), (477, 5), (250, 230), (3, N_TIME)):
        k = (t + off) % N_TIME
        seen.add(t + off >= N_TIME)
        et = torch.tensor([t, 999, -7], dtype=torch.int32, device="cuda")     # (only the first word is read)
        sc_at, m_at = hip.dev.agent_scores_at(*d, trans, et, off, c)
        vm_at = hip.dev.visible_mask_at(d[0], trans, et, off, c)
        sc, m = hip.dev.agent_scores(*d, hip.up(hip.c2t[k]), c)
        vm = hip.dev.visible_mask(d[0], hip.up(hip.c2t[k]), c)
        sc_at, sc = sc_at.cpu().numpy(), sc.cpu().numpy()
        assert np.array_equal(sc_at.view(np.int64), sc.view(np.int64)), (t, off)
        assert torch.equal(m_at, m) and torch.equal(vm_at, vm) and torch.equal(vm, m), (t, off)
        assert 0 < int(m.sum().item()) < n
    assert seen == {False, True}


KINDS = ("NAIVE_GREEDY", "VISIBLE_GREEDY", "SHANNON", "POS_ERROR", "VEL_ERROR")
ROW = {"NAIVE_GREEDY": 0, "VISIBLE_GREEDY": 0, "SHANNON": 1, "POS_ERROR": 2, "VEL_ERROR": 3}


def select_case(hip, rs, n, Ms):
    """len(Ms) envs of n objects, env e seen through matrix Ms[e].  In every env a visible object is made the maximum of every kind's
    score (largest covariance, largest displacement, largest log-det ratio) and its row copied to later positions, the last one in the
    last 256-block: a tie across blocks, the first copy in block e where there is one.  A NaN covariance at a low index (trace and
    log-det ratio NaN) and a NaN previous covariance (log-det ratio NaN): both skipped."""
    E = len(Ms)
    g = golden("ukf_step_golden.npz")
    xt, x = states(rs, n * E)
    P, Pp, _ = covariances(rs, n * E)
    P = sym(P * (1.0 + 0.1 * rs.uniform(size=(n * E, 1, 1))))      # (distinct traces: no accidental ties of the golden repeats)
    if n >= 257:
        for e in range(E):
            b = e * n
            vis = hip.dev.visible_mask(hip.up(xt[b:b + n]), hip.up(Ms[e]), hip.consts()).cpu().numpy()
            lo = 256 * (e % ((n - 1) // 256))
            src = b + lo + 8 + int(np.argmax(vis[lo + 8:]))
            assert vis[src - b] and src < b + n - 1
            x[src] = xt[src] + 1e3 * (x[src] - xt[src])
            P[src] = 1e4 * g["P0"]
            Pp[src] = P[src] / 1e6
            dst = {b + n - 1} | ({src + 256} if src + 256 < b + n - 1 else set())
            for j in dst:
                xt[j], x[j], P[j], Pp[j] = xt[src], x[src], P[src], Pp[src]
    if n >= 63:
        for e in range(E):
            P[e * n + 1, 2, 2] = P[e * n + 1, 2, 2] * np.nan
            Pp[e * n + 5] = np.nan
    return xt, x, P, Pp


@pytest.mark.gpu
def test_agent_select_every_kind_vs_numpy_argmax(hip):
    torch = hip.torch
    lib = hip.lib
    rs = np.random.RandomState(24)
    trans_np = hip.c2t.reshape(N_TIME, 9)
    trans = hip.up(trans_np)
    off = 6
    for E in (1, 3):
        env_time = np.array([476, 5, 250][:E], dtype=np.int32)          # env 0: 476 + 6 wraps to row 2
        et = hip.up(env_time, torch.int32)
        fallback = np.array([11, 22, 33][:E], dtype=np.int32)
        fb = hip.up(fallback, torch.int32)
        for n in (1, 255, 256, 257, 4100, 20000):
            Ms = [trans_np[(t + off) % N_TIME].reshape(3, 3) for t in env_time]
            xt, x, P, Pp = select_case(hip, rs, n, Ms)
            d = [hip.up(a) for a in (xt, x, P, Pp)]
            c = hip.consts()
            ws = hip.dev.agent_select_workspace(n, E, "cuda")
            # the per-object values and masks of every env from the scoring operator (itself checked above), with that env's matrix
            rows, masks = [], []
            for e in range(E):
                sl = slice(e * n, (e + 1) * n)
                sc, mk = scores_of(hip, xt[sl], x[sl], P[sl], Pp[sl], Ms[e], c)
                rows.append(sc)
                masks.append(mk.astype(bool))
            for kind in KINDS:
                k = getattr(lib, "AGENT_" + kind)
                want = []
                for e in range(E):
                    v = rows[e][ROW[kind]]
                    q = ~np.isnan(v) & (masks[e] if kind != "NAIVE_GREEDY" else True)
                    want.append(int(np.where(q)[0][np.argmax(v[q])]) if q.any() else -1)
                    if kind == "NAIVE_GREEDY" and n >= 63:
                        tr = np.trace(P[e * n:(e + 1) * n], axis1=1, axis2=2)
                        assert np.isnan(tr[1]) and want[-1] == int(np.nanargmax(tr))
                for fbk in (fb, None):
                    for rep in range(2):                                # the same workspace twice
                        a, pk = hip.dev.agent_select(c, k, *d, trans, et, off, fallback=fbk, workspace=ws)
                        a, pk = a.cpu().numpy(), pk.cpu().numpy()
                        for e in range(E):
                            w = want[e]
                            assert pk[e, 0] == w, (kind, E, n, e, pk[e, 0], w)
                            assert a[e] == (w if w >= 0 else (fallback[e] if fbk is not None else -1)), (kind, E, n, e)
                            if w >= 0:
                                assert pk[e, 1] == rows[e][ROW[kind]][w:w + 1].view(np.int64)[0], (kind, E, n, e)
                if n >= 257:
                    for e in range(E):
                        v = rows[e][ROW[kind]]
                        q = ~np.isnan(v) & (masks[e] if kind != "NAIVE_GREEDY" else True)
                        top = np.where(q & (v == v[want[e]]))[0]
                        assert len(top) >= 2 and len(set(top // 256)) >= 2, (kind, n, e, top)   # a tie across blocks, the first one won
            # Shannon without a previous covariance: every env falls back
            a, pk = hip.dev.agent_select(c, lib.AGENT_SHANNON, d[0], d[1], d[2], None, trans, et, off, fallback=fb, workspace=ws)
            assert np.array_equal(a.cpu().numpy(), fallback) and (pk.cpu().numpy()[:, 0] == -1).all()
        # nothing visible: the visible kinds fall back (or -1), the naive one does not look at visibility
        n = 600
        xt, x, P, Pp = select_case(hip, rs, n, Ms)
        d = [hip.up(a) for a in (xt, x, P, Pp)]
        c = hip.consts(np.radians(89.999))
        assert not hip.dev.visible_mask(d[0], hip.up(Ms[0]), c).any()
        for kind in KINDS:
            k = getattr(lib, "AGENT_" + kind)
            a, pk = hip.dev.agent_select(c, k, *d, trans, et, off, fallback=fb)
            a2, _ = hip.dev.agent_select(c, k, *d, trans, et, off)
            a, a2, pk = a.cpu().numpy(), a2.cpu().numpy(), pk.cpu().numpy()
            if kind == "NAIVE_GREEDY":
                for e in range(E):
                    tr = np.trace(P[e * n:(e + 1) * n], axis1=1, axis2=2)
                    assert a[e] == a2[e] == pk[e, 0] == int(np.nanargmax(tr))
            else:
                assert np.array_equal(a, fallback) and (a2 == -1).all() and (pk[:, 0] == -1).all(), kind


@pytest.mark.gpu
def test_agent_select_ids_names_the_callers_objects(hip):
    """a storage layout (obj_ids): the state in storage order, the answer as the caller numbers the objects, the first maximum the one
    with the lowest CALLER index -- also when the tied copies sit in storage in the opposite order"""
    torch = hip.torch
    lib = hip.lib
    rs = np.random.RandomState(25)
    trans = hip.up(hip.c2t.reshape(N_TIME, 9))
    et = hip.up(np.array([100], dtype=np.int32), torch.int32)
    c = hip.consts()
    for n in (257, 4100):
        xt, x, P, Pp = select_case(hip, rs, n, [hip.c2t[100]])
        perm = rs.permutation(n).astype(np.int32)                     # storage position i holds the caller's object perm[i]
        pos = np.argsort(perm)
        for kind in KINDS:
            k = getattr(lib, "AGENT_" + kind)
            a, pk = hip.dev.agent_select(c, k, *[hip.up(v) for v in (xt, x, P, Pp)], trans, et, 0)
            w = int(pk[0, 0].item())
            v = hip.dev.agent_scores(*[hip.up(v) for v in (xt, x, P, Pp)], hip.up(hip.c2t[100]), c)[0][ROW[kind]].cpu().numpy()
            tied = np.where(v == v[w])[0]
            assert len(tied) >= 2 and tied[0] == w
            # the lowest caller index of the tie goes LAST in storage among the tied copies
            lo, rest = tied[0], tied[1:]
            if pos[lo] < pos[rest].max():
                j = rest[np.argmax(pos[rest])]
                perm[pos[lo]], perm[pos[j]] = perm[pos[j]], perm[pos[lo]]
                pos = np.argsort(perm)
            assert pos[lo] > pos[rest].max()
            st = [hip.up(v[perm]) for v in (xt, x, P, Pp)]
            a2, pk2 = hip.dev.agent_select(c, k, *st, trans, et, 0, obj_ids=hip.up(perm, torch.int32))
            assert torch.equal(a2, a) and torch.equal(pk2, pk), (kind, n, a.item(), a2.item())


def _run_episode(hip, w, steps):
    """episode_workload's round-robin episode on the device (as run_hip), hybrid propagator, to the given step: the engine"""
    torch = hip.torch
    g, m = w["g"], w["m"]
    consts = hip.host.make_consts(g["Q"], g["R"], 1e-4, 2.0, -3, 20.0, -np.pi / 2, g["obs_lla"], obs_type="aer", propagator="hybrid")
    eng = hip.engine.HotPathEngine(consts, m, 1, w["c2t"], w["z_noise"][None], history=steps + 1)
    eng.load_state(0, w["x_true"], w["x"], w["P"])
    sched = torch.as_tensor((np.arange(steps) % m).astype(np.int32)).cuda()
    for i in range(1, steps + 1):
        eng.launch_step(i - 1, i, i, actions_ptr=sched.data_ptr() + 4 * (i - 1), fast_stats=True)
    torch.cuda.synchronize()
    return eng, consts


@pytest.mark.gpu
def test_shannon_late_in_an_episode(hip):
    """seed-7 episode of tests/episode_workload.py (2 000 objects, every one visible) at steps 300 and 330, scored from the engine's own
    P_filter slots.  Where both covariances are well defined (lambda_min > 1e-12 lambda_max) the score meets the parity criterion; every
    device NaN is a matrix numpy's Cholesky rejects or one whose smallest eigenvalue is at rounding level; the device's pick is numpy's
    arg-max over the objects it scores finite unless the top two are within the error bound.  How often the reference's own arg-max
    (NaN-free fp64 expression over all objects) lands on a rounding-defined object is printed, not asserted."""
    import episode_workload as ew
    torch = hip.torch
    w = ew.workload(seed=7)
    eng, consts = _run_episode(hip, w, 330)
    rounding_picks = 0
    for step in (300, 330):
        Pf = eng.P_filter[step].cpu().numpy()
        Ppf = eng.P_filter[step - 1].cpu().numpy()
        # the filter's covariances are symmetric only up to rounding; logdet_chol factorises the symmetric matrix of their upper
        # triangle (numpy's Cholesky reads the lower one), so that matrix is what the device's score and verdict are judged on
        P, Pp = upper(Pf), upper(Ppf)
        sc, mask = hip.dev.agent_scores(eng.x_true[step], eng.x_filter[step], eng.P_filter[step], eng.P_filter[step - 1],
                                        hip.up(w["c2t"][step]), consts)
        s1 = sc[1].cpu().numpy()
        assert mask.cpu().numpy().all()
        fin_in = np.isfinite(P).all(axis=(1, 2)) & np.isfinite(Pp).all(axis=(1, 2))
        lam = np.full((len(P), 6), np.nan)
        lamp = np.full((len(P), 6), np.nan)
        lam[fin_in] = np.linalg.eigvalsh(P[fin_in])
        lamp[fin_in] = np.linalg.eigvalsh(Pp[fin_in])
        with np.errstate(invalid="ignore"):
            well = fin_in & (lam[:, 0] > 1e-12 * lam[:, -1]) & (lamp[:, 0] > 1e-12 * lamp[:, -1])
            # (fp64 eigvalsh resolves an eigenvalue to about n eps lambda_max: below 16 eps lambda_max its sign is rounding)
            rounding = fin_in & ((lam[:, 0] <= 16 * EPS * lam[:, -1]) | (lamp[:, 0] <= 16 * EPS * lamp[:, -1]))
        print("[episode step %d] both covariances with lambda_min > 1e-12 lambda_max: %d; either at rounding level: %d; non-finite: %d"
              % (step, well.sum(), rounding.sum(), (~fin_in).sum()))
        assert well.sum() >= 0.75 * len(P), well.sum()
        g = shannon_criterion(s1[well], P[well], Pp[well], "episode step %d" % step)
        asym = np.abs(Pf - np.swapaxes(Pf, 1, 2)).max(axis=(1, 2)) / np.abs(np.einsum("kii->ki", Pf)).max(axis=1)
        moved = np.abs(log_ratio_ld(Pf[well], Ppf[well]) - log_ratio_ld(P[well], Pp[well])).astype(np.float64)
        print("[episode step %d] asymmetry of P (relative to its largest diagonal entry) max %.1e; it moves the long-double score of the "
              "strictly compared objects by up to %.1e (median %.1e)" % (step, asym[fin_in].max(), moved.max(), np.median(moved)))
        # every device NaN: a matrix numpy's Cholesky rejects, or a rounding-level smallest eigenvalue
        nan = np.isnan(s1)
        fails = chol_fails(P) | chol_fails(Pp)
        assert not (nan & well).any()
        assert np.all(fails[nan] | rounding[nan]), np.where(nan & ~fails & ~rounding)[0]
        # the device's own pick (launch_agent_select on the engine's slots) = numpy's arg-max over the objects it scores finite
        act = torch.full((1,), -5, dtype=torch.int32, device="cuda")
        pick = torch.zeros((1, 2), dtype=torch.int64, device="cuda")
        eng.launch_agent_select(step, step, hip.lib.AGENT_SHANNON, act.data_ptr(), pick_ptr=pick.data_ptr())
        got = int(act.item())
        ld = log_ratio_ld(P, Pp).astype(np.float64)
        cand = np.where(~nan)[0]
        ref_j = int(cand[np.nanargmax(np.where(np.isnan(ld[cand]), -np.inf, ld[cand]))])
        assert got == int(pick[0, 0].item()) and got in set(cand.tolist())
        if got != ref_j:
            two = [got, ref_j]
            bound = 3 * np.abs(log_ratio_f64(P[two], Pp[two]) - ld[two]) + 1e-12 + 2 * EPS * (scaled_cond(P[two]) + scaled_cond(Pp[two]))
            assert abs(ld[got] - ld[ref_j]) <= bound.sum(), (step, got, ref_j, ld[got], ld[ref_j], bound)
        assert s1[got] == np.nanmax(s1)
        # the reference's agent: its fp64 expression over every object (the full matrices), NaN-free arg-max (np.argmax would stop at a NaN)
        r64 = log_ratio_f64(Pf, Ppf)
        ref_pick = int(np.nanargmax(np.where(np.isnan(r64), -np.inf, r64)))
        on_rounding = bool(rounding[ref_pick] or nan[ref_pick])
        rounding_picks += on_rounding
        print("[episode step %d] device NaN scores %d (numpy Cholesky rejects %d, rounding-level lambda_min %d); strictly compared %d, "
              "max |dev - ld| %.2e; device pick %d, long-double pick among them %d; the reference's pick %d is %s"
              % (step, nan.sum(), (fails & nan).sum(), (rounding & nan).sum(), well.sum(), g.max(), got, ref_j, ref_pick,
                 "rounding-defined" if on_rounding else "well defined"))
    print("[episode] reference picks on rounding-defined objects: %d of 2" % rounding_picks)
