"""The device math on the device.  tests/test_device_math_host.py pins csrc/ssa_math.hpp and csrc/ssa_conics.hpp compiled for the HOST,
where the hardware reciprocal estimates are emulated, floating-point contraction is off and every wave vote is the lane's own value.
Here the same bodies, with the same bounds, run on the GPU through the probe module tests/devmath/devmath.hip (the library's hipcc
flags, one item per lane in 64-lane blocks, in array order), plus:
- the edges the host shim cannot judge: the real v_rcp_f64 / v_rsq_f64 estimates under rcp_nr / rsqrt_nr, log_pos at denormals and
  non-finite arguments, atan2_fast at signed zeros / axes / fold points / extreme ratios, sincos_fast at its |x| = 64 branch (one
  wavefront mixing both sides), exp_fast at its reduction boundaries;
- bit-identity of every item whatever shares its wavefront: the regime-order storage layout (HotPathEngine.set_layout) is correct only
  if each wave-wide decision (kepler_uv_fast's TINY instance, the Halley / Laguerre loop exits, kepler_fg_fast's and the hybrid
  kernel's tiers, sincos_fast's libm branch, the Newton loops' votes, the padding lanes) leaves each lane's arithmetic its own."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
from support.devmath import (CONIC_FORMS, _conic_states, build_devmath, check_conic_branches_lean_form_vs_restatements_and_oracle,
                             check_device_math_vs_reference_conics_golden, check_elements_strong_elliptic_chain_vs_reference_golden, check_fast_atan2, check_fast_exp,
                             check_fast_sincos_and_reciprocals, check_fg_hyperbolic_and_near_parabolic_states,
                             check_fg_universal_solvers_vs_reference_golden, check_j2_rk4_vs_80bit, check_near_parabolic_bands_fast_vs_libm)
from support.gpu import namespace

pytestmark = pytest.mark.gpu

MU = 398600441800000.0


class DeviceMath:
    """the numpy-level backend of test_device_math_host.HostMath, on the device (tests/devmath)"""

    def __init__(self, lib, torch):
        self.lib, self.torch = lib, torch

    def _up(self, a):
        return self.torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()      # (a copy: the shared pools are read-only)

    def _call(self, name, *args):
        stream = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        conv = [C.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else a for a in args]
        rc = getattr(self.lib, "dm_" + name)(*conv, stream)
        assert rc == 0, (name, rc)
        self.torch.cuda.synchronize()

    def _states(self, name, x, dt, *pre):
        xd = self._up(x)
        out = self.torch.empty_like(xd)
        flag = self.torch.zeros(len(xd), dtype=self.torch.int32, device="cuda")
        self._call(name, xd, C.c_int64(len(xd)), C.c_double(dt), *pre, out, flag)
        return out.cpu().numpy(), flag.cpu().numpy().astype(bool)

    def propagate(self, x, dt, prop):
        return self._states("propagate", x, dt, C.c_int32(prop))

    def propagate_j2(self, x, dt, nsub, j2, r_eq):
        return self._states("propagate_j2", x, dt, C.c_double(j2), C.c_double(r_eq), C.c_int32(nsub))

    def uv_fast(self, x, dt):
        return self._states("uv_fast", x, dt)

    def uv_general(self, x, dt):
        return self._states("uv_general", x, dt)

    def general_libm(self, x, dt):
        return self._states("general_libm", x, dt)

    def general_fast(self, x, dt):
        return self._states("general_fast", x, dt)

    def conic_lean(self, x, dt):
        return self._states("conic_lean", x, dt)

    def _scalar(self, name, ins, n_out, *mid):
        ins = [self._up(a) for a in ins]
        outs = [self.torch.empty_like(ins[0]) for _ in range(n_out)]
        self._call(name, *ins, C.c_int64(len(ins[0])), *mid, *outs)
        outs = [o.cpu().numpy() for o in outs]
        return outs[0] if n_out == 1 else tuple(outs)

    def band(self, nu, ecc, q, tof):
        return self._scalar("band", (nu, ecc, q), 2, C.c_double(tof))

    def log_pos(self, x):
        return self._scalar("log_pos", (x,), 1)

    def sincos(self, x):
        return self._scalar("sincos_fast", (x,), 2)

    def atan2(self, y, x):
        return self._scalar("atan2_fast", (y, x), 1)

    def exp(self, x):
        return self._scalar("exp_fast", (x,), 1)

    def recip(self, x):
        return self._scalar("recip", (x,), 2)


@pytest.fixture(scope="module")
def dm():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    lib = C.CDLL(build_devmath())
    for f in ("propagate", "propagate_j2", "uv_fast", "uv_general", "general_libm", "general_fast", "conic_lean", "band", "log_pos", "sincos_fast",
              "atan2_fast", "exp_fast", "recip"):
        getattr(lib, "dm_" + f).restype = C.c_int
    return DeviceMath(lib, torch)


@pytest.fixture(scope="module")
def hip():
    h = namespace()
    return h.dev, h.torch


# ------------------------------------------------------------------ the host pins, on the device (bounds unchanged)
@pytest.mark.parametrize("idt", range(5))
def test_device_math_fg_universal_solvers_vs_reference_golden(dm, idt):
    check_fg_universal_solvers_vs_reference_golden(dm, idt)


def test_device_math_fg_hyperbolic_and_near_parabolic_states(dm, oracle_ld):
    check_fg_hyperbolic_and_near_parabolic_states(dm, oracle_ld)


def test_device_math_conic_branches_lean_form_vs_restatements_and_oracle(dm, oracle_ld):
    check_conic_branches_lean_form_vs_restatements_and_oracle(dm, oracle_ld)


@pytest.mark.parametrize("form", CONIC_FORMS)
def test_device_math_conic_branches_vs_reference_conics_golden(dm, oracle_ld, form):
    check_device_math_vs_reference_conics_golden(dm, form, oracle_ld)


def test_device_math_near_parabolic_bands_fast_vs_libm(dm):
    check_near_parabolic_bands_fast_vs_libm(dm)


@pytest.mark.parametrize("idt", range(3))
def test_device_math_elements_strong_elliptic_chain_vs_reference_golden(dm, idt):
    check_elements_strong_elliptic_chain_vs_reference_golden(dm, idt)


def test_device_math_j2_rk4_vs_80bit(dm):
    check_j2_rk4_vs_80bit(dm)


def test_device_math_fast_sincos_and_reciprocals(dm):
    check_fast_sincos_and_reciprocals(dm)


def test_device_math_fast_atan2(dm):
    check_fast_atan2(dm)


def test_device_math_fast_exp(dm):
    check_fast_exp(dm)


# ------------------------------------------------------------------ edges the host shim cannot judge
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_device_math_reciprocals_over_their_domain(dm):
    """rcp_nr / rsqrt_nr from the REAL hardware estimates, over the documented domain (finite, non-denormal), powers of two included.
    Bounds: the host pins' (|r v - 1| < 4.5e-16, |q^2 v - 1| < 9e-16), the products taken in 80-bit arithmetic so that they do not
    under- or overflow at the ends of the range.  rcp_nr's arguments stop at 2^1022: beyond, 1 / v is itself denormal and a relative
    bound does not describe it."""
    rs = np.random.RandomState(11)
    ld = np.longdouble
    k = np.arange(-1022, 1023)
    p2 = np.ldexp(1.0, k)
    v = np.concatenate([10.0 ** rs.uniform(-307, 307, 400000), p2, np.nextafter(p2, 0), np.nextafter(p2, np.inf),
                        rs.uniform(1.0, 2.0, 100000), [2.2250738585072014e-308, 1.7976931348623157e308]])
    v = v[v >= 2.2250738585072014e-308]
    r, q = dm.recip(v)
    ok = v <= 2.0 ** 1022
    er = np.abs((r[ok].astype(ld) * v[ok] - 1).astype(np.float64))
    eq = np.abs((q.astype(ld) * q.astype(ld) * v - 1).astype(np.float64))
    print("[recip] max |r v - 1| %.3e, max |q^2 v - 1| %.3e" % (er.max(), eq.max()))
    assert er.max() < 4.5e-16, (er.max(), v[ok][np.argmax(er)])
    assert eq.max() < 9e-16, (eq.max(), v[np.argmax(eq)])
    rn, _ = dm.recip(-v[ok])                                    # negative arguments (rcp_nr only)
    en = np.abs((rn.astype(ld) * -v[ok] - 1).astype(np.float64))
    assert en.max() < 4.5e-16, (en.max(), v[ok][np.argmax(en)])


def test_device_math_log_pos_special_arguments(dm):
    """log_pos is total: libm's pattern (NaN / -inf / +inf) at 0, -0, negatives, +-inf, NaN, and its values at denormals and across the
    range within the host bound (2e-16 relative to the largest |log x| of the set + 2e-16), set by set"""
    rs = np.random.RandomState(12)
    special = np.array([1e-320, 5e-324, 2.2250738585072014e-308, 2.225073858507201e-308, 1e-310, 0.0, -0.0, -1.0, -5e-324, -np.inf, np.inf,
                        np.nan, 1.0, 2.0, 0.5, 1e308, 1.7976931348623157e308, 0.7071067811865476, 0.7071067811865475, 1.4142135623730951])
    for xs in (special, 10.0 ** rs.uniform(-323.3, -307.7, 20000), 10.0 ** rs.uniform(-307, 308, 20000), rs.uniform(0.5, 2.0, 20000)):
        r = dm.log_pos(xs)
        with np.errstate(all="ignore"):
            want = np.log(xs)
        assert np.array_equal(np.isnan(r), np.isnan(want)) and np.array_equal(np.isinf(r), np.isinf(want))
        inf = np.isinf(want)
        assert np.array_equal(np.sign(r[inf]), np.sign(want[inf]))
        ok = np.isfinite(want)
        err = np.abs(r[ok] - want[ok])
        print("[log_pos] %.0e .. %.0e: max error %.2f ulp" % (np.nanmin(np.abs(xs)), np.nanmax(np.abs(xs[np.isfinite(xs)])),
                                                             (err / np.spacing(np.abs(want[ok]))).max()))
        assert err.max() <= 2e-16 * np.abs(want[ok]).max() + 2e-16, (err.max(), xs[ok][np.argmax(err)])


def test_device_math_atan2_signed_zeros_axes_folds_and_extremes(dm):
    rs = np.random.RandomState(13)
    # signed zeros and the axes: libm's result to the bit (pi and -pi included)
    y = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 0.0, -0.0, 1e-300, -1e300, 0.0, -0.0, 3.0, -3.0])
    x = np.array([0.0, 0.0, -0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 0.0, 0.0, -1e-300, 1e300, -0.0, 0.0])
    r = dm.atan2(y, x)
    want = np.arctan2(y, x)
    assert np.array_equal(_bits(r), _bits(want)), np.stack([y, x, r, want], 1)
    # the octant folds: |y| = |x| and |y| / |x| = tan(pi/8) (the `mid` switch), a few ulps either side, every quadrant; host bounds
    t8 = 0.41421356237309503
    base = np.concatenate([np.ones(1), np.full(1, t8)])
    m = np.concatenate([base] + [np.nextafter(base, s) for s in (0, 2)] + [np.nextafter(np.nextafter(base, s), s) for s in (0, 2)])
    mag = 10.0 ** rs.uniform(-100, 100, len(m))
    ys, xs = [], []
    for sy in (1, -1):
        for sx in (1, -1):
            ys += [sy * m * mag, sy * mag]
            xs += [sx * mag, sx * m * mag]
    y, x = np.concatenate(ys), np.concatenate(xs)
    # ... and ratios |y / x| from 1e-290 to 1e290 with both arguments between 1e-300 and 1e300
    ey = rs.uniform(-300, 300, 200000)
    ex = np.clip(ey - rs.uniform(-290, 290, len(ey)), -300, 300)
    sg = rs.choice([-1.0, 1.0], (2, len(ey)))
    y, x = np.concatenate([y, sg[0] * 10.0 ** ey]), np.concatenate([x, sg[1] * 10.0 ** ex])
    r = dm.atan2(y, x)
    ref = np.arctan2(y.astype(np.longdouble), x.astype(np.longdouble))
    err = np.abs((r - ref).astype(np.float64))
    assert err.max() < 6e-16 and (err / np.spacing(np.maximum(np.abs(r), 0.5))).max() < 1.5, (err.max(), y[np.argmax(err)], x[np.argmax(err)])
    small = np.abs(ref) < 0.3
    rel = err[small] / np.abs(ref[small]).astype(np.float64)
    assert rel.max() < 5e-16, (rel.max(), y[small][np.argmax(rel)], x[small][np.argmax(rel)])


def _sincos_error_ulp(x, s, c):
    ls, lc = np.sin(x.astype(np.longdouble)), np.cos(x.astype(np.longdouble))
    es = np.abs((s - ls).astype(np.float64)) / np.spacing(np.maximum(np.abs(ls.astype(np.float64)), 1e-2))
    ec = np.abs((c - lc).astype(np.float64)) / np.spacing(np.maximum(np.abs(lc.astype(np.float64)), 1e-2))
    return np.maximum(es, ec)


def test_device_math_sincos_at_the_libm_branch_and_in_a_mixed_wavefront(dm):
    """sincos_fast's `!__all(small)` branch: |x| = 63.99 / 64 / 64.01, +-inf, NaN; and one wavefront that mixes |x| < 64 and |x| >= 64 --
    every lane keeps its OWN branch's value: the bits of a wavefront that holds only its own kind.  Bounds: the host pins' (1.5 ulp class
    below 64, 1e-15 absolute for the libm branch)."""
    x = np.array([63.99, -63.99, 64.0, -64.0, 64.01, -64.01, np.nextafter(64.0, 0), -np.nextafter(64.0, 0), np.inf, -np.inf, np.nan])
    s, c = dm.sincos(x)
    assert np.isnan(s[-3:]).all() and np.isnan(c[-3:]).all()
    lo = np.abs(x) < 64
    assert _sincos_error_ulp(x[lo], s[lo], c[lo]).max() < 2.0
    hi = np.isfinite(x) & ~lo
    ls, lc = np.sin(x[hi].astype(np.longdouble)), np.cos(x[hi].astype(np.longdouble))
    assert np.abs((s[hi] - ls).astype(np.float64)).max() < 1e-15 and np.abs((c[hi] - lc).astype(np.float64)).max() < 1e-15
    rs = np.random.RandomState(14)
    small = rs.uniform(-63.99, 63.99, 64 * 64)
    big = rs.uniform(64.0, 1e6, 64 * 64) * rs.choice([-1, 1], 64 * 64)
    big[:8] = [64.0, -64.0, 64.01, np.inf, -np.inf, np.nan, 1e300, -1e22]
    s_lo, c_lo = dm.sincos(small)                               # wavefronts without a libm lane
    s_hi, c_hi = dm.sincos(big)                                 # wavefronts of libm lanes only
    mix = np.where(rs.uniform(size=len(small)) < 0.5, small, big)
    which = np.abs(mix) < 64
    mix[::64] = big[::64]                                       # every wavefront has a libm lane
    which[::64] = False
    s_m, c_m = dm.sincos(mix)
    want_s, want_c = np.where(which, s_lo, s_hi), np.where(which, c_lo, c_hi)
    fin = ~np.isnan(want_s)
    assert np.array_equal(_bits(s_m[fin]), _bits(want_s[fin])) and np.array_equal(_bits(c_m[fin]), _bits(want_c[fin]))
    assert np.array_equal(np.isnan(s_m), np.isnan(want_s)) and np.array_equal(np.isnan(c_m), np.isnan(want_c))
    assert _sincos_error_ulp(small, s_lo, c_lo).max() < 2.0


def test_device_math_exp_at_its_reduction_boundaries(dm):
    """exp_fast: exactly 1 at 0; the Cody-Waite rounding boundaries x = (k + 1/2) ln 2 (a few ulps either side, every k of the range);
    up to 709.  Bound: the host pin's 4.5e-16 relative."""
    k = np.arange(0, 1023)
    b = (k + 0.5) * np.log(2.0)
    b = b[b < 709.0]
    x = np.concatenate([b, np.nextafter(b, 0), np.nextafter(b, 1e3), np.nextafter(np.nextafter(b, 0), 0), np.nextafter(np.nextafter(b, 1e3), 1e3),
                        k[k * np.log(2.0) < 709.0] * np.log(2.0), [0.0, 5e-324, 1e-300, 1e-17, 708.0, 708.9, 708.99, 708.999999, np.nextafter(709.0, 0)]])
    r = dm.exp(x)
    assert r[np.flatnonzero(x == 0.0)[0]] == 1.0
    ref = np.exp(x.astype(np.longdouble))
    err = np.abs((r - ref) / ref).astype(np.float64)
    assert np.isfinite(r).all() and err.max() < 4.5e-16, (err.max(), x[np.argmax(err)])


# ------------------------------------------------------------------ bit-identity whatever shares the wavefront
CATALOGUE, ZSWEEP, CONIC, FAROUT, COLLAPSED, NONFINITE = range(6)


def _z0(x, dt):
    """kepler_uv_fast's first-order estimate of z (its TINY vote: |z0| < 1.5e-3)"""
    rr = (x[:, :3] ** 2).sum(1)
    vv = (x[:, 3:] ** 2).sum(1)
    ir = 1 / np.sqrt(rr)
    return (2 * ir - vv / MU) * (MU * dt * dt) * ir * ir


def _state_pool(dt, oracle_ld):
    """(x[N, 6], class[N]): the catalogue and the golden rows (the exactly equatorial and circular ones included); states whose z0 sweeps
    1.3e-3 .. 2.2e-3 at this dt (both sides of the 1.5e-3 vote and the 2e-3 series bound: elliptic up to e = 0.95, hyperbolic to e = 3);
    near-parabolic and hyperbolic conics; far-out diverged hyperbolic states; states collapsed towards the centre; NaN / inf states"""
    from ssa_gym_amd.catalogue import coe2rv_host
    rs = np.random.RandomState(int(dt) % 9973)
    cat = np.concatenate([golden("catalogue_subset.npy"), golden("kepler_golden.npz")["x"]])
    m = 384
    ecc = np.concatenate([rs.uniform(0.0, 0.95, m - m // 4), rs.uniform(1.05, 3.0, m // 4)])
    nu_max = np.where(ecc > 1, 0.8 * np.arccos(-1 / np.maximum(ecc, 1.000001)), np.pi)
    zs = coe2rv_host(1e7 * np.abs(1 - ecc ** 2), ecc, rs.uniform(0.2, 2.9, m), rs.uniform(0, 6.28, m), rs.uniform(0, 6.28, m),
                     rs.uniform(-1, 1, m) * nu_max)
    s = (np.abs(_z0(zs, dt)) / rs.uniform(1.3e-3, 2.2e-3, m)) ** (1 / 3)        # z0 ~ a^-3 at a fixed shape
    zs[:, :3] *= s[:, None]
    zs[:, 3:] /= np.sqrt(s)[:, None]
    conic, _ = _conic_states(rs, 250)
    far = cat[:150].copy()
    far[:, 3:] *= rs.uniform(30.0, 300.0, size=len(far))[:, None]
    far = oracle_ld.propagate(far, 5000.0)
    far = far[np.isfinite(far).all(1)]
    col = cat[rs.choice(len(cat), 60)].copy()
    col[:, :3] *= (10.0 ** rs.uniform(3.5, 5.0, len(col)) / np.linalg.norm(col[:, :3], axis=1))[:, None]      # r0 = 3e3 .. 1e5 m
    bad = cat[rs.choice(len(cat), 12)].copy()
    for j in range(len(bad)):
        bad[j, j % 6] = (np.nan, np.inf, -np.inf)[j % 3]
    x = np.concatenate([cat, zs, conic, far, col, bad])
    cls = np.repeat([CATALOGUE, ZSWEEP, CONIC, FAROUT, COLLAPSED, NONFINITE], [len(cat), len(zs), len(conic), len(far), len(col), len(bad)])
    return x, cls


def _same_bits(a, b):
    """per row: every value the same bits (any NaN equals any NaN)"""
    a, b = np.ascontiguousarray(a).reshape(len(a), -1), np.ascontiguousarray(b).reshape(len(b), -1)
    if a.dtype == np.float64:
        eq = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
    else:
        eq = a == b
    return eq.all(1)


def _check_layouts(run, items, cls, seed):
    """run(items[idx]) -> tuple of per-item output arrays.  Each item's outputs in several layouts against the item ALONE (a wavefront of
    64 copies of itself): random permutations, sorted by class, 63 ordinary (class 0) items + one forcing item per wavefront, and ragged
    n whose item 0 is a forcing item (the padding lanes recompute it)."""
    rs = np.random.RandomState(seed)
    n = len(items)
    alone = [a[::64] for a in run(np.repeat(items, 64, axis=0))]
    ordinary, forcing = np.flatnonzero(cls == 0), np.flatnonzero(cls != 0)
    layouts = [("permutation %d" % k, rs.permutation(n)) for k in range(3)]
    layouts.append(("sorted by class", np.argsort(cls, kind="stable")))
    adv = []
    for f in forcing:
        w = rs.choice(ordinary, 64)
        w[rs.randint(64)] = f
        adv.append(w)
    layouts.append(("63 ordinary + 1 forcing per wavefront", np.concatenate(adv)))
    for c in np.unique(cls[cls != 0]):
        f = np.flatnonzero(cls == c)
        for j in (f[0], f[-1]):
            layouts.append(("ragged, item 0 of class %d" % c, np.concatenate([[j], rs.choice(ordinary, 64 * 2 + 4)])))
    for what, idx in layouts:
        got = run(items[idx])
        bad = np.zeros(len(idx), dtype=bool)
        for g, a in zip(got, alone):
            bad |= ~_same_bits(g, a[idx])
        assert not bad.any(), (what, "%d items differ; their classes" % bad.sum(), np.unique(cls[idx][bad], return_counts=True),
                               [(int(idx[k]), [(g[k], a[idx[k]]) for g, a in zip(got, alone)]) for k in np.flatnonzero(bad)[:3]])


DTS = (20.0, 150.0, 5400.0, 86400.0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kernel", ["elements", "fg", "hybrid", "kepler_elements", "j2"])
def test_device_math_product_kernels_do_not_depend_on_wave_neighbours(hip, oracle_ld, kernel, dt):
    """ssa_propagate_f64 (ELEMENTS / FG / HYBRID), ssa_kepler_elements_f64 and ssa_propagate_j2_f64 (5 s sub-steps, 64 at the most:
    the NaN / inf rows of the pool among the others): each item's bits, whatever shares its wavefront"""
    device, torch = hip
    from ssa_gym_amd import _lib
    x, cls = _state_pool(dt, oracle_ld)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if kernel == "kepler_elements":
        run = lambda a: (device.kepler_elements(up(a), dt).cpu().numpy(),)
    elif kernel == "j2":
        run = lambda a: (device.propagate_j2(up(a), dt, 0.00108263, 6378136.6, min(64, int(np.ceil(dt / 5.0)))).cpu().numpy(),)
    else:
        prop = {"elements": _lib.PROP_ELEMENTS, "fg": _lib.PROP_FG, "hybrid": _lib.PROP_HYBRID}[kernel]
        run = lambda a: (device.propagate(up(a), dt, propagator=prop).cpu().numpy(),)
    _check_layouts(run, x, cls, seed=int(dt) + len(kernel))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kernel", ["uv_fast", "conic_lean"])
def test_device_math_solvers_do_not_depend_on_wave_neighbours(dm, oracle_ld, kernel, dt):
    """the probe's kepler_uv_fast (TINY vote, Halley loop exit) and kepler_conic_lean (newton_hyp and band loop votes)"""
    x, cls = _state_pool(dt, oracle_ld)

    def run(a):
        y, flag = getattr(dm, kernel)(a, dt)
        y[~flag] = np.nan          # (a lane the tier does not take is recomputed by the next tier: its `out` is scratch -- the flag is compared)
        return y, flag
    _check_layouts(run, x, cls, seed=int(dt) + 7)


def test_device_math_uv_fast_pool_straddles_the_votes(oracle_ld):
    """the z sweep of the pool does straddle kepler_uv_fast's 1.5e-3 vote and the 2e-3 series bound at every step length"""
    for dt in DTS:
        x, cls = _state_pool(dt, oracle_ld)
        z0 = np.abs(_z0(x[cls == ZSWEEP], dt))
        assert z0.min() < 1.4e-3 and (z0 < 1.5e-3).sum() > 50 and ((z0 >= 1.5e-3) & (z0 < 2e-3)).sum() > 50 and (z0 > 2e-3).sum() > 20


@pytest.mark.parametrize("tof", [20.0, 150.0, 5400.0])
def test_device_math_bands_do_not_depend_on_wave_neighbours(dm, tof):
    """genf:: band solvers (their __ballot(!done) Newton loops): elliptic states beyond the series as the ordinary items; near-parabolic
    both sides, the exact parabola, beyond-the-asymptote and NaN as the forcing ones"""
    rs = np.random.RandomState(15)
    m = 1200
    ecc = np.concatenate([rs.uniform(0.3, 0.9899, m // 2), rs.uniform(0.9901, 0.99999, m // 8), rs.uniform(1.00001, 1.0099, m // 8),
                          1 + 10.0 ** rs.uniform(-9, -2.1, m // 4) * rs.choice([-1, 1], m // 4)])
    ecc[-4:] = [1.0, 1.0, np.nan, 1.005]
    q = rs.uniform(6.8e6, 3e7, m)
    with np.errstate(invalid="ignore"):
        nu_max = np.where(ecc > 1, 0.95 * np.arccos(-1 / np.maximum(ecc, 1.000001)), 3.1)
    nu = rs.uniform(-1, 1, m) * nu_max
    nu[-1] = 0.5 * (np.arccos(-1 / 1.005) + np.pi)                   # between the asymptote and pi: NaN
    items = np.stack([nu, ecc, q], 1)
    cls = (np.arange(m) >= m // 2).astype(int)
    _check_layouts(lambda a: dm.band(a[:, 0], a[:, 1], a[:, 2], tof), items, cls, seed=int(tof))


def test_device_math_sincos_does_not_depend_on_wave_neighbours(dm):
    rs = np.random.RandomState(16)
    x = np.concatenate([rs.uniform(-63.99, 63.99, 3000), rs.uniform(64, 1e4, 40) * rs.choice([-1, 1], 40), [64.0, -64.0, np.inf, -np.inf, np.nan]])
    cls = (np.abs(x) >= 64) | np.isnan(x)
    _check_layouts(lambda a: dm.sincos(a), x, cls.astype(int), seed=16)
