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

import pytest

from support.devmath import (CONIC_FORMS, build_devmath, build_hostmath, check_conic_branches_lean_form_vs_restatements_and_oracle,
                             check_device_math_vs_reference_conics_golden, check_elements_strong_elliptic_chain_vs_reference_golden, check_fast_atan2, check_fast_exp,
                             check_fast_sincos_and_reciprocals, check_fg_hyperbolic_and_near_parabolic_states,
                             check_fg_universal_solvers_vs_reference_golden, check_j2_rk4_vs_80bit, check_near_parabolic_bands_fast_vs_libm)

@pytest.fixture(scope="module")
def hm(tmp_path_factory):
    return build_hostmath(str(tmp_path_factory.mktemp("hostmath")))


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


def test_j2_rk4_vs_80bit(hm):
    check_j2_rk4_vs_80bit(hm)


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
    for name in ("propagate", "propagate_j2", "uv_fast", "uv_general", "general_libm", "general_fast", "conic_lean", "band", "log_pos", "sincos_fast",
                 "atan2_fast", "exp_fast", "recip"):
        assert hasattr(lib, "dm_" + name), name
