"""CPU-only checks of a sensor network in each of several envs (include/ssa_hip.h: ssa_env_step_sensors_envs_f64;
HotPathEngine.launch_step_sensors_envs; SSA_Tasker_VecEnv with config['observers']): the export, the parameter block's layout against the
header, refusal of bad arguments before any launch, the vector env's guards and rules without device state, and the new kernels'
resource budget in the shipped code object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from support.batches import c2t
from support.codeobj import KERNEL_FAMILIES, _kernels, assert_family_budget, header
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.refusals import STEP_PTRS, bad_rk4, nan_mask, refused, valid_blocks
from support.sensors import cfg3


def test_vector_sensor_step_is_exported_and_declared(lib):
    from ssa_gym_amd import _lib
    hdr = header()
    assert re.search(r"\bint ssa_env_step_sensors_envs_f64\s*\(", hdr)
    assert re.search(r"\}\s*ssa_sensor_envs_params\s*;", hdr)
    assert "ssa_env_step_sensors_envs_f64" in _lib.SIGNATURES
    assert hasattr(lib, "ssa_env_step_sensors_envs_f64")
    assert lib.ssa_abi_version() == _lib.ABI_VERSION == 23          # (additive: the ABI version stays)
    assert re.search(r"#define\s+SSA_ABI_VERSION\s+23\b", hdr)


def test_sensor_envs_params_layout_matches_the_header(lib, tmp_path):
    from ssa_gym_amd import _lib
    st = _lib.ssa_sensor_envs_params
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssa_hip.h"', 'int main(void){',
           'printf("%zu\\n", sizeof(ssa_sensor_envs_params));']
    want = [C.sizeof(st)]
    for f, _ in st._fields_:
        src.append('printf("%%zu\\n", offsetof(ssa_sensor_envs_params, %s));' % f)
        want.append(getattr(st, f).offset)
    # (the rows: SSA_MAX_SENSORS words each, SSA_INLINE_ENVS of them)
    src.append('printf("%zu\\n", offsetof(ssa_sensor_envs_params, inline_action[1]) - offsetof(ssa_sensor_envs_params, inline_action[0]));')
    src.append('printf("%zu\\n", sizeof(((ssa_sensor_envs_params*)0)->inline_action));')
    want += [4 * _lib.MAX_SENSORS, 4 * _lib.MAX_SENSORS * _lib.INLINE_ENVS]
    src.append('return 0;}')
    c = tmp_path / "se.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "se"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).decode().split()] == want


def test_vector_sensor_step_refuses_bad_arguments_before_any_launch(lib):
    """every refusal of ssa_env_step_sensors_f64 but its n_env one, and the entry's own: each with its code and nothing launched (no device
    is touched: this runs without a GPU).  Every case spoils ONE field of blocks that are otherwise complete."""
    from ssa_gym_amd import _lib
    fn = lib.ssa_env_step_sensors_envs_f64
    for k in range(4):                                                     # NULL blocks (`envs` among them)
        assert refused(fn, None, null=k) == _lib.E_INVALID, k
    invalid = [("p", "n_obj", 0), ("p", "n_obj", -4), ("p", "n_env", 0), ("c", "propagator", 7), ("c", "obs_type", 5),
               ("sp", "n_sensor", 0), ("sp", "n_sensor", -1), ("sp", "n_sensor", 9), ("sp", "zn_stride_sensor", -1),
               ("sp", "zn_stride_sensor", 0), ("p", "aer_cols", 3), ("p", "n_obj", (1 << 30)),
               ("v", "actions", 0), ("v", "actions", 0x1004), ("v", "actions", 0x1010),      # NULL / misaligned rows
               ("p", "launch_mask", _lib.LAUNCH_INLINE_ACTION), ("p", "launch_mask", _lib.LAUNCH_FOLD_INSIDE),
               ("p", "spos_tiles", 0x1000), ("p", "fail_log", 0x1000)]
    invalid += [("p", nm, 0) for nm in STEP_PTRS]
    for case in invalid:
        assert refused(fn, None, case) == _lib.E_INVALID, case
    nine = (("p", "n_env", 9), ("p", "launch_mask", _lib.LAUNCH_INLINE_ENVS))      # more envs than travel by value
    assert refused(fn, None, *nine) == _lib.E_INVALID
    assert refused(fn, None, *nine, ("v", "actions", 0)) == _lib.E_INVALID
    assert refused(fn, None, spoil=nan_mask) == _lib.E_INVALID
    assert refused(fn, None, spoil=bad_rk4) == _lib.E_INVALID
    # whole tiles per env; the statistics from the metrics rows are the plain one-env step's
    assert refused(fn, None, ("p", "n_obj", 6)) == _lib.E_UNSUPPORTED
    assert refused(fn, None, ("p", "n_env", 3), ("p", "n_obj", 7)) == _lib.E_UNSUPPORTED
    assert refused(fn, None, ("p", "launch_mask", _lib.LAUNCH_STATS_FROM_METRICS)) == _lib.E_UNSUPPORTED
    assert refused(fn, None, ("p", "launch_mask", _lib.LAUNCH_STATS_FROM_METRICS | _lib.LAUNCH_DEFER_FOLD),
                   ("p", "stat_shards", 0x1000)) == _lib.E_UNSUPPORTED
    assert refused(fn, None, ("p", "launch_mask", _lib.LAUNCH_MIRROR_F32)) == _lib.E_UNSUPPORTED      # (as the step: needs the one-launch statistics)
    assert refused(fn, None, ("p", "obj_ids", 0x1000)) == _lib.E_UNSUPPORTED
    # n_env == 1 takes any n_obj: the refusal that remains for these blocks is one of the step's own
    assert refused(fn, None, ("p", "n_env", 1), ("p", "n_obj", 7), ("p", "stat_ws", 0)) == _lib.E_INVALID


def test_one_env_sensor_entry_still_refuses_several_envs(lib):
    from ssa_gym_amd import _lib
    fn = lib.ssa_env_step_sensors_f64
    assert refused(fn, valid_blocks(fn.__name__, n_env=2)) == _lib.E_UNSUPPORTED


def test_vector_env_refuses_ragged_envs_before_the_gpu_is_touched(lib):
    """rso_count % 4 != 0 with several envs of a sensor network: a ValueError from the constructor, raised before any device object
    exists (this test runs without a GPU)"""
    from ssa_gym_amd import envs as E
    from ssa_gym_amd.envs.vector_env import SSA_Tasker_VecEnv
    cfg = cfg3(E, m=6, steps=12, trans_matrix=c2t()[:12])
    with pytest.raises(ValueError, match="rso_count % 4"):
        SSA_Tasker_VecEnv(cfg, 2, seed=1)


def test_vector_env_action_checks_need_no_device_state():
    from ssa_gym_amd.envs.vector_env import check_sensor_actions
    E, S, m = 3, 3, 8
    ok = np.array([[0, 1, 2], [2, 1, 0], [7, 0, 1]])                        # (object 0, 1, 2 in several envs: different objects)
    out = check_sensor_actions(ok, E, S, m)
    assert out.dtype == np.int64 and np.array_equal(out, ok)
    assert np.array_equal(check_sensor_actions(ok.tolist(), E, S, m), ok)
    for bad in (ok[:2], ok[:, :2], ok.reshape(-1), ok.astype(np.float64)):  # shape, dtype
        with pytest.raises(AssertionError):
            check_sensor_actions(bad, E, S, m)
    for j in (-1, m, m + 5):                                                # range
        bad = ok.copy()
        bad[1, 2] = j
        with pytest.raises(AssertionError, match="invalid"):
            check_sensor_actions(bad, E, S, m)
    dup = ok.copy()
    dup[2, 1] = 7                                                           # two sensors of env 2 on object 7
    with pytest.raises(ValueError, match="same object"):
        check_sensor_actions(dup, E, S, m)


def test_shaped_hit_rule_on_hand_made_arrays():
    """'shaped' pays an env its +1/n if ANY of its sensors tasked np.argmax(sigma_pos[i - 1]); one action per env: that action"""
    from ssa_gym_amd import _lib
    from ssa_gym_amd.envs._config import reward_done
    from ssa_gym_amd.envs.vector_env import shaped_hit
    prev = np.array([4, 0, 7, 2])
    acts = np.array([[1, 4, 2], [1, 2, 3], [7, 6, 5], [0, 1, 3]])
    hit = shaped_hit(acts, prev)
    assert hit.dtype == bool and hit.tolist() == [True, False, True, False]
    assert shaped_hit(np.array([4, 1, 7, 3]), prev).tolist() == [True, False, True, False]
    st = np.zeros((4, _lib.STAT_STRIDE))
    st[:, _lib.STAT_MAX_DPOS] = 1e5                                         # (neither won nor lost)
    rew, done = reward_done('shaped', st, hit, np.zeros(4), np.zeros(4, dtype=bool), 8, 10)
    assert rew.tolist() == [0.1, -0.1, 0.1, -0.1] and not done.any()


def test_vector_sensor_kernels_keep_the_sensor_step_kernels_budget(tmp_path):
    """the eight vector_sensors_kernel instances fit 96 VGPRs (5 wavefronts per SIMD), use the LDS of step_sensors_kernel's instance of
    the same propagator and launch form and no more scratch or VGPR spills than it, and touch scratch only around the out-of-line calls
    (SSA_PROP_ELEMENTS / SSA_PROP_HYBRID) -- FG and J2 none at all"""
    kern, ins_of = _kernels(tmp_path)
    assert_family_budget(kern, ins_of, "vector_sensors_kernel", "step_sensors_kernel", KERNEL_FAMILIES["vector_sensors_kernel"])
