"""CPU-only checks of a sensor network's rollout (include/ssa_hip.h: ssa_env_rollout_sensors_f64; SSA_Tasker_Env.rollout_sensors): the
export, the parameter block's layout against the header, refusal of bad arguments before any launch, the env's guards without device
state, and the new kernels' resource budget in the shipped code object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from support.codeobj import _kernels, header, stray_scratch
from support.gpu import lib  # noqa: F401  (the module fixture)
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


def _valid_blocks():
    """blocks that pass every check (the pointers are never dereferenced on the host: a refusal comes before any launch) -- each case
    below spoils exactly one field"""
    from ssa_gym_amd import _lib, host
    g = dict(Q=np.eye(6), R=np.eye(3))
    c = host.make_consts(g["Q"], g["R"], 1e-4, 2.0, -3, 20.0, -np.pi / 2, np.array([0.6, -1.3, 20.0]))
    p, r, sp, rs = _lib.ssa_step_params(), _lib.ssa_rollout_params(), _lib.ssa_sensor_params(), _lib.ssa_rollout_sensors_params()
    p.n_obj, p.n_env = 8, 1
    p.status = p.trans = p.env_time = p.z_noise = 0x1000
    r.n_steps, r.history, r.slot_out = 3, 4, 1
    r.x_true_ring = r.x_ring = r.P_ring = r.obs_ring = r.metrics_ring = r.stats_ring = r.stat_shards = 0x1000
    sp.n_sensor, sp.zn_stride_sensor = 2, 8 * 3
    rs.actions = 0x1000
    return c, p, r, sp, rs


def test_sensor_rollout_refuses_bad_arguments_before_any_launch(lib):
    """every refusal of ssa_env_rollout_f64 and of the sensor step's checks, NULL actions and a shared noise table: each with its code and
    nothing launched (no device is touched: this runs without a GPU).  Every case spoils ONE field of blocks that are otherwise
    complete, so the code it gets back is that field's."""
    from ssa_gym_amd import _lib
    f = lib.ssa_env_rollout_sensors_f64

    def call(spoil=None, null=None):
        c, p, r, sp, rs = _valid_blocks()
        if spoil:
            spoil(p, r, sp, rs, c)
        args = [C.byref(c), C.byref(p), C.byref(r), C.byref(sp), C.byref(rs)]
        if null is not None:
            args[null] = None
        return f(*args, None)

    def setter(which, name, value):
        def spoil(p, r, sp, rs, c):
            setattr(dict(p=p, r=r, sp=sp, rs=rs, c=c)[which], name, value)
        return spoil
    for k in range(5):                                                     # NULL blocks
        assert call(null=k) == _lib.E_INVALID, k
    invalid = [("r", "n_steps", 0), ("r", "history", 1), ("r", "slot_out", 4), ("r", "slot_out", -1), ("p", "n_obj", 0),
               ("c", "propagator", 7), ("c", "obs_type", 5), ("rs", "actions", 0), ("rs", "actions", 0x1004),
               ("sp", "zn_stride_sensor", 0), ("sp", "zn_stride_sensor", -3), ("sp", "n_sensor", 0), ("sp", "n_sensor", -1),
               ("sp", "n_sensor", 9)]
    invalid += [("r", nm, 0) for nm in ("x_true_ring", "x_ring", "P_ring", "obs_ring", "metrics_ring", "stats_ring", "stat_shards")]
    invalid += [("p", nm, 0) for nm in ("status", "trans", "env_time", "z_noise")]
    for which, name, value in invalid:
        assert call(setter(which, name, value)) == _lib.E_INVALID, (which, name, value)

    def nan_mask(p, r, sp, rs, c):
        sp.obs_limit[1] = float("nan")
    assert call(nan_mask) == _lib.E_INVALID
    assert call(setter("p", "n_env", 2)) == _lib.E_UNSUPPORTED

    def one_sensor_shares_nothing(p, r, sp, rs, c):      # (S = 1 with stride 0 is the one-site block: not refused for the stride)
        sp.n_sensor, sp.zn_stride_sensor, p.n_env = 1, 0, 2
    assert call(one_sensor_shares_nothing) == _lib.E_UNSUPPORTED


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
    sens = [k for k in kern if "rollout_sensors_kernel" in k]
    assert len(sens) == 4, sens
    checked = 0
    for name, ins in ins_of.items():
        if "rollout_sensors_kernel" not in name:
            continue
        k = kern[name]
        roll = kern[name.replace("22rollout_sensors_kernel", "14rollout_kernel").replace("NS_9RollSensKE", "NS_5RollKE")]
        assert k["vgpr_count"] <= 96 and k["group_segment_fixed_size"] == roll["group_segment_fixed_size"], (name, k)
        assert k["private_segment_fixed_size"] <= roll["private_segment_fixed_size"], (name, k, roll)
        assert k["vgpr_spill_count"] <= roll["vgpr_spill_count"], (name, k, roll)
        calls = [i for i, op in enumerate(ins) if op == "s_swappc_b64"]
        assert not stray_scratch(ins), (name, stray_scratch(ins)[:8])
        if "ILi0E" not in name and "ILi3E" not in name:
            assert not calls and k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        checked += 1
    assert checked == 4
