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
from support.codeobj import _kernels, header, stray_scratch
from support.gpu import lib  # noqa: F401  (the module fixture)
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


def _valid_blocks():
    """blocks that pass every check (the pointers are never dereferenced on the host: a refusal comes before any launch) -- each case
    below spoils exactly one field, so nothing is ever launched"""
    from ssa_gym_amd import _lib, host
    c = host.make_consts(np.eye(6), np.eye(3), 1e-4, 2.0, -3, 20.0, -np.pi / 2, np.array([0.6, -1.3, 20.0]))
    p, sp, v = _lib.ssa_step_params(), _lib.ssa_sensor_params(), _lib.ssa_sensor_envs_params()
    p.n_obj, p.n_env = 8, 2
    for nm in ("x_true_in", "x_true_out", "x_in", "x_out", "P_in", "P_out", "status", "obs", "metrics", "trans", "env_time", "z_noise",
               "stat_ws"):
        setattr(p, nm, 0x1000)
    sp.n_sensor, sp.zn_stride_sensor = 2, 48
    v.actions = 0x1000
    return c, p, sp, v


def test_vector_sensor_step_refuses_bad_arguments_before_any_launch(lib):
    """every refusal of ssa_env_step_sensors_f64 but its n_env one, and the entry's own: each with its code and nothing launched (no device
    is touched: this runs without a GPU).  Every case spoils ONE field of blocks that are otherwise complete."""
    from ssa_gym_amd import _lib
    fn = lib.ssa_env_step_sensors_envs_f64

    def call(spoil=None, null=None):
        c, p, sp, v = _valid_blocks()
        if spoil:
            spoil(c, p, sp, v)
        args = [C.byref(c), C.byref(p), C.byref(sp), C.byref(v)]
        if null is not None:
            args[null] = None
        return fn(*args, None)

    def setter(*fields):
        def spoil(c, p, sp, v):
            for which, name, value in fields:
                setattr(dict(c=c, p=p, sp=sp, v=v)[which], name, value)
        return spoil
    for k in range(4):                                                     # NULL blocks (`envs` among them)
        assert call(null=k) == _lib.E_INVALID, k
    invalid = [("p", "n_obj", 0), ("p", "n_obj", -4), ("p", "n_env", 0), ("c", "propagator", 7), ("c", "obs_type", 5),
               ("sp", "n_sensor", 0), ("sp", "n_sensor", -1), ("sp", "n_sensor", 9), ("sp", "zn_stride_sensor", -1),
               ("sp", "zn_stride_sensor", 0), ("p", "aer_cols", 3), ("p", "n_obj", (1 << 30)),
               ("v", "actions", 0), ("v", "actions", 0x1004), ("v", "actions", 0x1010),      # NULL / misaligned rows
               ("p", "launch_mask", _lib.LAUNCH_INLINE_ACTION), ("p", "launch_mask", _lib.LAUNCH_FOLD_INSIDE),
               ("p", "spos_tiles", 0x1000), ("p", "fail_log", 0x1000)]
    invalid += [("p", nm, 0) for nm in ("x_true_in", "x_true_out", "x_in", "x_out", "P_in", "P_out", "status", "obs", "metrics", "trans",
                                        "env_time", "z_noise", "stat_ws")]
    for which, name, value in invalid:
        assert call(setter((which, name, value))) == _lib.E_INVALID, (which, name, value)
    assert call(setter(("p", "n_env", 9), ("p", "launch_mask", _lib.LAUNCH_INLINE_ENVS))) == _lib.E_INVALID      # more envs than travel by value
    assert call(setter(("p", "n_env", 9), ("p", "launch_mask", _lib.LAUNCH_INLINE_ENVS), ("v", "actions", 0))) == _lib.E_INVALID

    def nan_mask(c, p, sp, v):
        sp.obs_limit[1] = float("nan")
    assert call(nan_mask) == _lib.E_INVALID

    def bad_rk4(c, p, sp, v):
        c.propagator, c.rk4_substeps = _lib.PROP_J2_RK4, 0
    assert call(bad_rk4) == _lib.E_INVALID
    # whole tiles per env; the statistics from the metrics rows are the plain one-env step's
    assert call(setter(("p", "n_obj", 6))) == _lib.E_UNSUPPORTED
    assert call(setter(("p", "n_env", 3), ("p", "n_obj", 7))) == _lib.E_UNSUPPORTED
    assert call(setter(("p", "launch_mask", _lib.LAUNCH_STATS_FROM_METRICS))) == _lib.E_UNSUPPORTED
    assert call(setter(("p", "launch_mask", _lib.LAUNCH_STATS_FROM_METRICS | _lib.LAUNCH_DEFER_FOLD), ("p", "stat_shards", 0x1000))) == \
        _lib.E_UNSUPPORTED
    assert call(setter(("p", "launch_mask", _lib.LAUNCH_MIRROR_F32))) == _lib.E_UNSUPPORTED      # (as the step: needs the one-launch statistics)
    assert call(setter(("p", "obj_ids", 0x1000))) == _lib.E_UNSUPPORTED
    # n_env == 1 takes any n_obj: the refusal that remains for these blocks is one of the step's own
    assert call(setter(("p", "n_env", 1), ("p", "n_obj", 7), ("p", "stat_ws", 0))) == _lib.E_INVALID


def test_one_env_sensor_entry_still_refuses_several_envs(lib):
    from ssa_gym_amd import _lib
    c, p, sp, _ = _valid_blocks()
    assert p.n_env == 2
    assert lib.ssa_env_step_sensors_f64(C.byref(c), C.byref(p), C.byref(sp), None) == _lib.E_UNSUPPORTED


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
    new = [k for k in kern if "vector_sensors_kernel" in k]
    assert len(new) == 8, new
    for other in ("step_sensors_kernel", "rollout_sensors_kernel", "lookahead_sensors_kernel", "forecast_sensors_kernel", "lookahead_kernel",
                  "rollout_kernel", "closed_loop_kernel", "step_fast_kernel"):
        assert not any(other in k for k in new), other                      # (the names the other host tests count kernels by)
    checked = 0
    for name, ins in ins_of.items():
        if "vector_sensors_kernel" not in name:
            continue
        form = re.search(r"ILi(\d)ELb([01])E", name)
        prop = form.group(1)
        ref = [k for k in kern if "step_sensors_kernel" in k and form.group(0) in k]
        assert len(ref) == 1, (name, ref)
        k, b = kern[name], kern[ref[0]]
        assert k["vgpr_count"] <= 96 and k["group_segment_fixed_size"] == b["group_segment_fixed_size"], (name, k, b)
        assert k["private_segment_fixed_size"] <= b["private_segment_fixed_size"], (name, k, b)
        assert k["vgpr_spill_count"] <= b["vgpr_spill_count"], (name, k, b)
        calls = [i for i, op in enumerate(ins) if op == "s_swappc_b64"]
        assert not stray_scratch(ins), (name, stray_scratch(ins)[:8])
        if prop not in "03":
            assert not calls and k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        checked += 1
    assert checked == 8
