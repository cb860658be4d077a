"""CPU-only checks of a sensor network's rollout (include/ssa_hip.h: ssa_env_rollout_sensors_f64; SSA_Tasker_Env.rollout_sensors): the
export, the parameter block's layout against the header, refusal of bad arguments before any launch, the env's guards without device
state, and the new kernels' resource budget in the shipped code object."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from support.codeobj import KERNEL_FAMILIES, _kernels, assert_family_budget, header
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.refusals import RING_PTRS, ROLL_PTRS, nan_mask, refused
from support.sensors import _bare_env


def test_sensor_rollout_is_exported_and_declared(lib):
    from ssa_gym_amd import _lib
    hdr = header()
    assert re.search(r"\bint ssa_env_rollout_sensors_f64\s*\(", hdr)
    assert "ssa_env_rollout_sensors_f64" in _lib.SIGNATURES
    assert hasattr(lib, "ssa_env_rollout_sensors_f64")
    assert lib.ssa_abi_version() == _lib.ABI_VERSION == 23          # (additive: the ABI version stays)


def test_rollout_sensors_params_layout_matches_the_header(lib, tmp_path):
    from ssa_gym_amd import _lib
    st = _lib.ssa_rollout_sensors_params
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssa_hip.h"', 'int main(void){',
           'printf("%zu\\n", sizeof(ssa_rollout_sensors_params));']
    want = [C.sizeof(st)]
    for f, _ in st._fields_:
        src.append('printf("%%zu\\n", offsetof(ssa_rollout_sensors_params, %s));' % f)
        want.append(getattr(st, f).offset)
    src.append('return 0;}')
    c = tmp_path / "rs.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "rs"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).decode().split()] == want


def test_sensor_rollout_refuses_bad_arguments_before_any_launch(lib):
    """every refusal of ssa_env_rollout_f64 and of the sensor step's checks, NULL actions and a shared noise table: each with its code and
    nothing launched (no device is touched: this runs without a GPU).  Every case spoils ONE field of blocks that are otherwise
    complete, so the code it gets back is that field's."""
    from ssa_gym_amd import _lib
    f = lib.ssa_env_rollout_sensors_f64
    for k in range(5):                                                     # NULL blocks
        assert refused(f, None, null=k) == _lib.E_INVALID, k
    invalid = [("r", "n_steps", 0), ("r", "history", 1), ("r", "slot_out", 4), ("r", "slot_out", -1), ("p", "n_obj", 0),
               ("c", "propagator", 7), ("c", "obs_type", 5), ("rs", "actions", 0), ("rs", "actions", 0x1004),
               ("sp", "zn_stride_sensor", 0), ("sp", "zn_stride_sensor", -3), ("sp", "n_sensor", 0), ("sp", "n_sensor", -1),
               ("sp", "n_sensor", 9)]
    invalid += [("r", nm, 0) for nm in RING_PTRS] + [("p", nm, 0) for nm in ROLL_PTRS]
    for case in invalid:
        assert refused(f, None, case) == _lib.E_INVALID, case
    assert refused(f, None, spoil=nan_mask) == _lib.E_INVALID
    assert refused(f, None, ("p", "n_env", 2)) == _lib.E_UNSUPPORTED
    # (S = 1 with stride 0 is the one-site block: not refused for the stride)
    assert refused(f, None, ("sp", "n_sensor", 1), ("sp", "zn_stride_sensor", 0), ("p", "n_env", 2)) == _lib.E_UNSUPPORTED


def test_env_guards_come_before_anything_is_launched():
    from ssa_gym_amd import _lib
    env = _bare_env(3)
    with pytest.raises(_lib.SsaHipError):
        env.rollout_sensors([[1, 2, 3]])          # no device state: no CPU fallback
    with pytest.raises(_lib.SsaHipError):
        _bare_env(1).rollout_sensors([[1]])
    env._engine = object()                        # (the checks below come before anything touches the engine)
    with pytest.raises(ValueError, match="row 1"):
        env.rollout_sensors([[1, 2, 3], [4, 2, 4]])
    with pytest.raises(AssertionError):
        env.rollout_sensors([[1, 2], [3, 4]])                               # a wrong width
    with pytest.raises(AssertionError):
        env.rollout_sensors([1, 2, 3])                                      # not a schedule
    with pytest.raises(AssertionError, match="row 2"):
        env.rollout_sensors([[1, 2, 3], [4, 5, 6], [1, 2, 10]])             # out of range
    with pytest.raises(AssertionError):
        env.rollout_sensors([[1, 2, -1]])
    with pytest.raises(NotImplementedError, match="sensor network"):        # rollout() keeps refusing a network
        env.rollout([0, 1])


def test_sensor_rollout_kernels_keep_the_rollout_kernels_budget(tmp_path):
    """the four rollout_sensors_kernel instances fit 96 VGPRs (5 wavefronts per SIMD), use the LDS of rollout_kernel of the same
    propagator and no more scratch or VGPR spills than it, and touch scratch only around the out-of-line calls (SSA_PROP_ELEMENTS /
    SSA_PROP_HYBRID) -- FG and J2 none at all"""
    kern, ins_of = _kernels(tmp_path)
    assert_family_budget(kern, ins_of, "rollout_sensors_kernel", "rollout_kernel", KERNEL_FAMILIES["rollout_sensors_kernel"])
