"""CPU pins of the product's per-lane device math: csrc/ssa_math.hpp compiled for the host (tests/hostmath: HIP qualifiers
shimmed away, hardware reciprocal estimates emulated with their 2^-26-class error) and held to the goldens the reference's
own farnocchia.py produced.  What this covers without a GPU: the universal-variable solvers of SSA_PROP_FG (series / Halley
and closed-form / Laguerre, incl. which lanes each one accepts), the strong-elliptic SSA_PROP_ELEMENTS chain with its
refined-estimate divisions, bounded-argument sincos and the exactness requirements of the equatorial test, the third-order
reciprocal refinements.  The host build cannot see what the device adds: the real v_rcp_f64 / v_rsq_f64 estimates, the
library's -ffp-contract=fast, the wave votes.  Each test body (tests/support/devmath.py) therefore takes a numpy-level backend (HostMath
below); tests/test_device_math_gpu.py runs the same bodies, with the same bounds, on the device through the probe module
tests/devmath/devmath.hip (compiled with the library's own flags -- test_devmath_probe_cross_compiles builds it without a GPU),
adds the edges the shim cannot judge, and checks that no item's bits depend on what shares its wavefront."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from support.devmath import (CONIC_FORMS, build_devmath, check_conic_branches_lean_form_vs_restatements_and_oracle,
                             check_device_math_vs_reference_conics_golden, check_elements_strong_elliptic_chain_vs_reference_golden, check_fast_atan2, check_fast_exp,
                             check_fast_sincos_and_reciprocals, check_fg_hyperbolic_and_near_parabolic_states,
                             check_fg_universal_solvers_vs_reference_golden, check_near_parabolic_bands_fast_vs_libm)

HERE = os.path.dirname(os.path.abspath(__file__))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class HostMath:
    """numpy-level backend over tests/hostmath (ctypes).  States x[n, 6] -> (y[n, 6], flag[n] bool); scalars elementwise."""

    def __init__(self, lib):
        self.lib = lib

    def _states(self, fn, x, dt, *pre):
        x = _f64(x)
        out = np.empty_like(x)
        flag = np.zeros(len(x), dtype=np.int32)
        fn(_p(x), C.c_long(len(x)), C.c_double(dt), *pre, _p(out), _p(flag))
        return out, flag.astype(bool)

    def propagate(self, x, dt, prop):
        return self._states(self.lib.hm_propagate, x, dt, C.c_int(prop))

    def uv_fast(self, x, dt):
        return self._states(self.lib.hm_uv_fast, x, dt)

    def uv_general(self, x, dt):
        return self._states(self.lib.hm_uv_general, x, dt)

    def general_libm(self, x, dt):
        return self._states(self.lib.hm_general_libm, x, dt)

    def general_fast(self, x, dt):
        return self._states(self.lib.hm_general_fast, x, dt)

    def conic_lean(self, x, dt):
        return self._states(self.lib.hm_conic_lean, x, dt)

    def band(self, nu, ecc, q, tof):
        nu, ecc, q = _f64(nu), _f64(ecc), _f64(q)
        fast, libm = np.empty_like(nu), np.empty_like(nu)
        self.lib.hm_band(_p(nu), _p(ecc), _p(q), C.c_long(len(nu)), C.c_double(tof), _p(fast), _p(libm))
        return fast, libm

    def log_pos(self, x):
        x = _f64(x)
        r = np.empty_like(x)
        self.lib.hm_log_pos(_p(x), C.c_long(len(x)), _p(r))
        return r

    def sincos(self, x):
        x = _f64(x)
        s, c = np.empty_like(x), np.empty_like(x)
        self.lib.hm_sincos_fast(_p(x), C.c_long(len(x)), _p(s), _p(c))
        return s, c

    def atan2(self, y, x):
        y, x = _f64(y), _f64(x)
        r = np.empty_like(x)
        self.lib.hm_atan2_fast(_p(y), _p(x), C.c_long(len(x)), _p(r))
        return r

    def exp(self, x):
        x = _f64(x)
        r = np.empty_like(x)
        self.lib.hm_exp_fast(_p(x), C.c_long(len(x)), _p(r))
        return r

    def recip(self, x):
        x = _f64(x)
        r, q = np.empty_like(x), np.empty_like(x)
        self.lib.hm_recip(_p(x), C.c_long(len(x)), _p(r), _p(q))
        return r, q


@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostmath") / "libhostmath.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D_GNU_SOURCE", "-fPIC", "-shared", "-ffp-contract=off",
                           "-I" + os.path.join(HERE, "hostmath"), "-o", so, os.path.join(HERE, "hostmath", "hostmath.cpp")])
    return HostMath(C.CDLL(so))


# ---- the bodies on the host (tests/test_device_math_gpu.py runs them on the device)

@pytest.mark.parametrize("idt", range(5))
def test_fg_universal_solvers_vs_reference_golden(hm, idt):
    check_fg_universal_solvers_vs_reference_golden(hm, idt)


def test_fg_hyperbolic_and_near_parabolic_states(hm, oracle_ld):
    check_fg_hyperbolic_and_near_parabolic_states(hm, oracle_ld)


def test_conic_branches_lean_form_vs_restatements_and_oracle(hm, oracle_ld):
    check_conic_branches_lean_form_vs_restatements_and_oracle(hm, oracle_ld)


@pytest.mark.parametrize("form", CONIC_FORMS)
def test_conic_branches_vs_reference_conics_golden(hm, oracle_ld, form):
    check_device_math_vs_reference_conics_golden(hm, form, oracle_ld)


def test_near_parabolic_bands_fast_vs_libm(hm):
    check_near_parabolic_bands_fast_vs_libm(hm)


@pytest.mark.parametrize("idt", range(3))
def test_elements_strong_elliptic_chain_vs_reference_golden(hm, idt):
    check_elements_strong_elliptic_chain_vs_reference_golden(hm, idt)


def test_fast_sincos_and_reciprocals(hm):
    check_fast_sincos_and_reciprocals(hm)


def test_fast_atan2(hm):
    check_fast_atan2(hm)


def test_fast_exp(hm):
    check_fast_exp(hm)


def test_devmath_probe_cross_compiles():
    """the probe module of the GPU tests (tests/devmath) builds for gfx950 with the library's flags and exports every entry point: a
    header change that breaks it fails here, without a GPU"""
    so = build_devmath(force=True)
    lib = C.CDLL(so)
    for name in ("propagate", "uv_fast", "uv_general", "general_libm", "general_fast", "conic_lean", "band", "log_pos", "sincos_fast",
                 "atan2_fast", "exp_fast", "recip"):
        assert hasattr(lib, "dm_" + name), name
