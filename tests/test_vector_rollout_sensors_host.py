"""CPU-only checks of a sensor network's K-step schedule in each of several envs (include/ssa_hip.h: ssa_env_rollout_sensors_envs_f64;
HotPathEngine.launch_rollout_sensors_envs; SSA_Tasker_VecEnv.rollout_sensors / rollout): the export and the new block's layout,
refusal of bad arguments before any launch, the one-env entries' refusals kept, the vector env's guards and its booking function
without device state, and the new kernels' resource budget in the shipped code object."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from support.codeobj import KERNEL_FAMILIES, _kernels, assert_family_budget, family, header, twin
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.refusals import RING_PTRS, ROLL_PTRS, bad_rk4, nan_mask, refused, valid_blocks
from support.vector_rollout import bare_vec

ENTRY = "ssa_env_rollout_sensors_envs_f64"


def test_the_entry_is_exported_declared_and_bound(lib):
    from ssa_gym_amd import _lib
    hdr = header()
    assert re.search(r"\bint %s\s*\(" % ENTRY, hdr)
    assert re.search(r"\}\s*ssa_rollout_sensors_envs_params\s*;", hdr)
    assert ENTRY in _lib.SIGNATURES and hasattr(lib, ENTRY)
    res, args = _lib.SIGNATURES[ENTRY]
    assert res is C.c_int and len(args) == 6 and args[4] is C.POINTER(_lib.ssa_rollout_sensors_envs_params)
    assert args[:4] == _lib.SIGNATURES["ssa_env_rollout_sensors_f64"][1][:4]
    assert lib.ssa_abi_version() == _lib.ABI_VERSION == 23          # (additive: the ABI version stays)
    assert re.search(r"#define\s+SSA_ABI_VERSION\s+23\b", hdr)


def test_the_new_block_has_the_compilers_layout(tmp_path):
    from ssa_gym_amd import _lib
    st = _lib.ssa_rollout_sensors_envs_params
    names = [f for f, _ in st._fields_]
    assert names == ["actions", "stats_out", "upd_out"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssa_hip.h"', 'int main(void) {',
           'printf("%zu\\n", sizeof(ssa_rollout_sensors_envs_params));']
    for f in names:
        src.append('printf("%%zu\\n", offsetof(ssa_rollout_sensors_envs_params, %s));' % f)
    src.append('return 0; }')
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text("\n".join(src))
    subprocess.check_call(["gcc", "-I", ROOT + "/include", "-o", str(exe), str(c)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(st)] + [getattr(st, f).offset for f in names]


def test_vector_rollout_refuses_bad_arguments_before_any_launch(lib):
    """every refusal of ssa_env_rollout_sensors_f64 but its n_env one, and the entry's own: each with its code and nothing launched (no
    device is touched: this runs without a GPU).  Every case spoils ONE field of blocks that are otherwise complete."""
    from ssa_gym_amd import _lib
    fn = getattr(lib, ENTRY)
    for k in range(5):                                                     # NULL blocks
        assert refused(fn, None, null=k) == _lib.E_INVALID, k
    invalid = [("r", "n_steps", 0), ("r", "n_steps", -1), ("r", "history", 1), ("r", "slot_out", -1), ("r", "slot_out", 2),
               ("p", "n_obj", 0), ("p", "n_obj", -4), ("p", "n_env", 0), ("p", "n_env", -1), ("c", "propagator", 7), ("c", "obs_type", 5),
               ("sp", "n_sensor", 0), ("sp", "n_sensor", -1), ("sp", "n_sensor", 9), ("sp", "zn_stride_sensor", -1),
               ("sp", "zn_stride_sensor", 0)]
    invalid += [("r", nm, 0) for nm in RING_PTRS] + [("p", nm, 0) for nm in ROLL_PTRS]
    invalid += [("re", "actions", 0), ("re", "actions", 0x1004), ("re", "actions", 0x1010), ("re", "stats_out", 0)]
    invalid += [("p", "launch_mask", _lib.LAUNCH_INLINE_ENVS)]             # a resident tile reads the time words from memory
    for case in invalid:
        assert refused(fn, None, case) == _lib.E_INVALID, case
    assert refused(fn, None, spoil=nan_mask) == _lib.E_INVALID
    assert refused(fn, None, spoil=bad_rk4) == _lib.E_INVALID
    assert refused(fn, None, ("p", "n_obj", 1 << 30)) == _lib.E_INVALID                                      # 2 x 2^30 objects
    # whole tiles per env
    assert refused(fn, None, ("p", "n_obj", 6)) == _lib.E_UNSUPPORTED                                        # n_env = 2, n_obj = 6
    assert refused(fn, None, ("p", "n_env", 3), ("p", "n_obj", 7)) == _lib.E_UNSUPPORTED
    assert refused(fn, None, ("p", "n_obj", 6), ("r", "spos_tiles", 0x1000)) == _lib.E_UNSUPPORTED
    # n_env == 1 takes any n_obj, several envs take obj_ids: what is refused for these blocks is one of the entry's other checks
    assert refused(fn, None, ("p", "n_env", 1), ("p", "n_obj", 7), ("r", "n_steps", 0)) == _lib.E_INVALID
    assert refused(fn, None, ("p", "n_env", 1), ("p", "n_obj", 7), ("re", "stats_out", 0)) == _lib.E_INVALID
    assert refused(fn, None, ("p", "obj_ids", 0x1000), ("re", "stats_out", 0)) == _lib.E_INVALID
    assert refused(fn, None, ("p", "obj_ids", 0x1000), ("p", "n_obj", 6)) == _lib.E_UNSUPPORTED
    assert refused(fn, None, ("re", "upd_out", 0), ("re", "stats_out", 0)) == _lib.E_INVALID                 # (upd_out may be NULL; stats_out may not)


def test_one_env_entries_keep_their_refusals(lib):
    """ssa_env_rollout_sensors_f64 still answers SSA_E_UNSUPPORTED for two envs, and ssa_env_rollout_f64 for obj_ids with several envs"""
    from ssa_gym_amd import _lib
    fn = lib.ssa_env_rollout_sensors_f64
    assert refused(fn, valid_blocks(fn.__name__, n_env=2)) == _lib.E_UNSUPPORTED
    fn = lib.ssa_env_rollout_f64
    assert refused(fn, valid_blocks(fn.__name__, n_env=2), ("p", "obj_ids", 0x1000)) == _lib.E_UNSUPPORTED


def test_engine_keeps_the_one_env_refusal():
    """HotPathEngine.launch_rollout_sensors still covers one env -- before anything of the engine is read (an engine object without
    device state); launch_rollout_sensors_envs refuses a schedule that is not on the device before it reads anything else"""
    from ssa_gym_amd import _lib, engine, host
    eng = engine.HotPathEngine.__new__(engine.HotPathEngine)
    eng.E, eng.m = 3, 8
    with pytest.raises(_lib.SsaHipError, match="one env"):
        eng.launch_rollout_sensors(0, 1, None, None)
    sp = host.make_sensor_params([np.array([0.6, -1.3, 20.0])] * 2, [0.1, 0.2], [np.eye(3)] * 2, 48)
    for bad in (None, np.zeros((4, 3, 2), dtype=np.int32)):
        with pytest.raises(_lib.SsaHipError, match="actions"):
            eng.launch_rollout_sensors_envs(0, 1, sp, bad)


def test_vector_rollout_guards_need_no_device_state():
    """shape, dtype, a bad row naming its step, an env without a next step, several envs with m % 4 -- all before anything is launched
    or counted; rollout() points a network's user to rollout_sensors()"""
    for S in (1, 3):
        vec = bare_vec(S)
        good = np.stack([np.stack([np.arange(S) + k + e for k in range(4)]) for e in range(vec.E)])      # [E, 4, S]
        assert good.shape == (vec.E, 4, S)
        for bad in (good[0], good[:2], good[:, :, :S - 1] if S > 1 else good[:, :, [0, 0]], good[:, :0], good.astype(np.float64),
                    good.reshape(-1)):
            with pytest.raises(ValueError, match="shape"):
                vec.rollout_sensors(bad)
        worse = good.copy()
        worse[1, 2, 0] = vec.m                                   # out of range at step 2
        with pytest.raises(AssertionError, match="step 2"):
            vec.rollout_sensors(worse)
        if S > 1:
            worse = good.copy()
            worse[2, 3, 1] = worse[2, 3, 0]                      # two sensors of env 2 on one object at step 3
            with pytest.raises(ValueError, match="step 3"):
                vec.rollout_sensors(worse)
            with pytest.raises(NotImplementedError, match="rollout_sensors"):
                vec.rollout(good[:, :, 0])
        else:
            with pytest.raises(ValueError, match="shape"):
                vec.rollout(good)                                # [E, K, 1] is rollout_sensors' form
            with pytest.raises(AssertionError, match="step 1"):
                vec.rollout(np.array([[0, -1], [1, 2], [2, 3]]))
        vec.i[1] = vec.n - 1
        with pytest.raises(ValueError, match="no next step"):
            vec.rollout_sensors(good)
        assert vec.tick == 0 and vec.i.tolist() == [0, vec.n - 1, 0]      # (nothing counted)
    vec = bare_vec(3, E=2, m=6)
    with pytest.raises(ValueError, match="% 4"):
        vec.rollout_sensors(np.zeros((2, 2, 3), dtype=np.int64) + np.arange(3))
    one = bare_vec(3, E=1, m=6)                                  # (one env takes any m: the next thing it needs is the device)
    from ssa_gym_amd import _lib
    with pytest.raises(_lib.SsaHipError, match="no device state"):
        one.rollout_sensors(np.zeros((1, 2, 3), dtype=np.int64) + np.arange(3))


def _stats(C_, E, dpos=1e5, lt4=3.0, lt7=8.0, argmax=0.0):
    from ssa_gym_amd import _lib
    st = np.zeros((C_, E, _lib.STAT_STRIDE))
    st[..., _lib.STAT_MAX_DPOS], st[..., _lib.STAT_CNT_LT_1E4], st[..., _lib.STAT_CNT_LT_1E7] = dpos, lt4, lt7
    st[..., _lib.STAT_ARGMAX_SPOS] = argmax
    return st


def test_booking_on_hand_made_statistics():
    from ssa_gym_amd import _lib
    from ssa_gym_amd.envs._config import reward_done
    from ssa_gym_amd.envs.vector_env import book_rollout
    E, m, n, K = 3, 8, 12, 5
    acts = np.stack([np.stack([(np.arange(3) + k + e) % m for e in range(E)]) for k in range(K)])      # [K, E, S]
    zeros, i0 = np.zeros(E), np.array([0, 2, 1])
    # 'jones': env 1 wins at step 2 of 5 -- three steps are kept, the win pays 1, nobody else is done
    st = _stats(K, E)
    st[2, 1, _lib.STAT_MAX_DPOS] = 2.9e4
    paid0, prev0 = np.array([0.25, 0.5, 0.0]), np.array([4, 5, 6])
    r, d, paid, prev, keep = book_rollout('jones', st, acts, paid0, prev0, i0, m, n)
    assert keep == 3 and r.shape == d.shape == (E, 3) and d.dtype == bool
    assert d.tolist() == [[False] * 3, [False, False, True], [False] * 3] and r.tolist() == [[0.0] * 3, [0.0, 0.0, 1.0], [0.0] * 3]
    assert paid.tolist() == [0.25, 1.5, 0.0] and prev.tolist() == [4, 5, 6]                  # ('jones' keeps no arg-max)
    assert paid0.tolist() == [0.25, 0.5, 0.0] and prev0.tolist() == [4, 5, 6]                # (the inputs are not written)
    # ... a loss (5000 km off) ends it unpaid; a NaN max_dpos neither wins nor loses
    st = _stats(K, E)
    st[1, 0, _lib.STAT_MAX_DPOS] = np.nan
    st[3, 2, _lib.STAT_MAX_DPOS] = 5.1e6
    r, d, paid, prev, keep = book_rollout('jones', st, acts, zeros, prev0, i0, m, n)
    assert keep == 4 and not d[:, :3].any() and d[:, 3].tolist() == [False, False, True] and not r.any()
    # the time limit: env 1 (i = 2 in front of the chunk) takes its last step at k = 8 of a nine-step chunk, whatever the reward type
    for kind in ('trinary', 'jones', 'shaped', 'none'):
        st9 = _stats(9, E)
        acts9 = np.concatenate([acts, acts[:4]])
        r, d, paid, prev, keep = book_rollout(kind, st9, acts9, zeros, prev0, i0, m, n)
        assert keep == 9 and d[:, :8].sum() == 0 and d[:, 8].tolist() == [False, True, False], kind
        if kind == 'trinary':
            assert np.array_equal(r, np.full((E, 9), (3.0 + 8.0) / m / 2)) and np.array_equal(paid, r.sum(axis=1))
    # 'shaped': the hit of step k is against the arg-max of step k - 1 (argmax_prev for k = 0), any sensor counts
    st = _stats(K, E)
    st[:, :, _lib.STAT_ARGMAX_SPOS] = [[7, 7, 7], [2, 7, 7], [7, 7, 7], [7, 7, 7], [0, 0, 0]]
    prev0 = np.array([7, 2, 7])        # step 0: env 1's sensor 1 holds 2 (acts[0, 1] = [1, 2, 3])
    assert acts[0, 1].tolist() == [1, 2, 3] and acts[2, 0].tolist() == [2, 3, 4] and 7 not in acts[:3].reshape(-1)
    r, d, paid, prev, keep = book_rollout('shaped', st, acts, zeros, prev0, i0, m, n)
    want = -np.ones((E, K)) / n
    want[1, 0] = 1.0 / n               # against argmax_prev
    want[0, 2] = 1.0 / n               # step 2 of env 0 holds 2 = stats[1]'s arg-max of env 0 -- not stats[2]'s
    for k, e in ((3, 2), (4, 1), (4, 2)):      # (the schedule meets 7 in the later rows)
        assert 7 in acts[k, e]
        want[e, k] = 1.0 / n
    assert keep == K and np.array_equal(r, want) and not d.any() and prev.tolist() == [0, 0, 0]
    paid_k = np.zeros(E)
    for k in range(K):
        paid_k = paid_k + want[:, k]
    assert np.array_equal(paid, paid_k)
    # ... and rewards_sum feeds its win: 1 - (what the episode paid before the chunk + the chunk's steps before the win)
    st[1, 2, _lib.STAT_MAX_DPOS] = 100.0
    paid0 = np.array([0.0, 0.0, 0.375])
    r, d, paid, prev, keep = book_rollout('shaped', st, acts, paid0, prev0, i0, m, n)
    assert keep == 2 and d[:, 1].tolist() == [False, False, True]
    assert r[2, 1] == 1.0 - (0.375 + want[2, 0]) and paid[2] == (0.375 + want[2, 0]) + r[2, 1]
    assert prev.tolist() == [2, 7, 7]                                                        # (stats[1]'s arg-max: the last step kept)
    # every step equals reward_done on that step's rows
    r1, d1 = reward_done('shaped', st[0], np.array([False, True, False]), paid0, i0 + 2 >= n, m, n)
    assert np.array_equal(r[:, 0], r1) and np.array_equal(d[:, 0], d1)


def test_new_kernels_keep_the_rollout_kernels_budget(tmp_path):
    """exactly four rollout_sensor_envs_kernel instances, none under a name another host test counts kernels by, and one
    rollout_fold_steps_kernel; each instance fits 96 VGPRs, uses the LDS of rollout_sensors_kernel's instance of the same propagator
    (7 296 bytes) and no more scratch or VGPR spills than rollout_kernel's (which carries n_env at run time too), and touches scratch
    only around the out-of-line calls (SSA_PROP_ELEMENTS / SSA_PROP_HYBRID) -- FG and J2 none at all"""
    kern, ins_of = _kernels(tmp_path)
    assert len(family(kern, "rollout_fold_steps_kernel")) == KERNEL_FAMILIES["rollout_fold_steps_kernel"] == 1
    assert_family_budget(kern, ins_of, "rollout_sensor_envs_kernel", "rollout_sensors_kernel", KERNEL_FAMILIES["rollout_sensor_envs_kernel"],
                         same_args="kinds", scratch_against="rollout_kernel")
    for name in family(kern, "rollout_sensor_envs_kernel"):
        assert kern[twin(kern, name, "rollout_sensors_kernel")]["group_segment_fixed_size"] == 7296, name
