"""CPU-only checks of the pass table of a sensor network (ssa_access_sensors_f64): the new block against the
header compiled with gcc, every refusal of the entry -- nothing here is launched: every call breaks a rule --, the numpy statement of
the table (tests/support/access.py) against hand-made bit patterns, and the four kernels in the shipped code object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
from support import access as ac
from support import illumination as il
from support import orbiting as ob
from support.codeobj import _kernels, family, header, stray_scratch
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.refusals import bad_rk4, nan_mask

ONE, HIGH, ZERO = 0b10, 0b100, 0b01      # (the harness's blocks have two sensors)


# ---------------------------------------------------------------------------------------------------------------- 1. the block
def test_the_block_matches_the_header_and_the_abi_keeps_its_version(lib, tmp_path):
    from ssa_gym_amd import _lib
    st = _lib.ssa_access_params
    names = [f for f, _ in st._fields_]
    assert names == ["n_steps", "n_sel", "bits", "pass_", "n_left", "env_sel"]
    cname = {f: f.rstrip("_") for f in names}      # (`pass` is a keyword of the binding's language)
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssa_hip.h"', 'int main(void){',
           'printf("%zu %d %zu %zu\\n", sizeof(ssa_access_params), SSA_ABI_VERSION, sizeof(ssa_sensor_params), sizeof(ssa_step_params));']
    src += ['printf("%%zu %%zu\\n", offsetof(ssa_access_params, %s), sizeof(((ssa_access_params *)0)->%s));' % (cname[f], cname[f]) for f in names]
    src += ['printf("%d %d %d %d\\n", SSA_PASS_FIRST, SSA_PASS_LENGTH, SSA_PASS_COUNT, SSA_PASS_PASSES);', 'return 0;}']
    c = tmp_path / "access.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "access"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert out[:4] == [C.sizeof(st), 23, C.sizeof(_lib.ssa_sensor_params), C.sizeof(_lib.ssa_step_params)]
    assert out[4:-4] == [w for f in names for w in (getattr(st, f).offset, getattr(st, f).size)]
    assert out[-4:] == [_lib.PASS_FIRST, _lib.PASS_LENGTH, _lib.PASS_COUNT, _lib.PASS_PASSES] == [0, 1, 2, 3]
    # (the two blocks the entry shares with the others are untouched: their tails are 8t's and 8v's)
    sp, p = _lib.ssa_sensor_params, _lib.ssa_step_params
    assert [f for f, _ in sp._fields_][-4:] == ["sun", "shadow_radius", "sunlit_only", "reserved2"] and C.sizeof(sp) == sp.upd.offset + 32
    assert [f for f, _ in p._fields_][-4:] == ["site_rows", "limb_radius", "site_moving", "reserved3"]
    assert C.sizeof(p) == p.metrics_prev.offset + 32
    assert lib.ssa_abi_version() == 23 and _lib.ABI_VERSION == 23
    assert re.search(r"int ssa_access_sensors_f64\s*\(", header()) and "ssa_access_sensors_f64" in _lib.SIGNATURES
    assert hasattr(lib, "ssa_access_sensors_f64")
    z = st()
    assert (z.n_steps, z.n_sel, z.bits, z.pass_, z.n_left, z.env_sel) == (0, 0, None, None, None, None)


def test_the_header_states_the_definition_and_the_refusals():
    hdr = re.sub(r"\s+", " ", header().replace("\n *", " "))
    for words in ("CHAINED propagations", "bit (h mod 64) of word (h div 64)", "bits at h >= T are 0", "a NaN anywhere 0",
                  "access[h] AND (the update would be attempted", "every other byte is left as it is", "n_sel > n_env",
                  "n_env * n_sensor * n_obj * W >= 2^31", "Refused before any launch, SSA_E_INVALID, in this order"):
        assert words in hdr, words


# ---------------------------------------------------------------------------------------------------------------- 2. refusals
def test_every_refusal_of_the_entry(lib):
    from ssa_gym_amd import _lib
    inv = _lib.E_INVALID
    for k in range(4):                                             # a NULL block
        assert ac.answer(lib, null=k) == inv, k
    for blk, name, val in (("p", "n_obj", 0), ("p", "n_obj", -3), ("p", "n_env", 0), ("p", "x_true_in", 0), ("p", "trans", 0),
                           ("p", "env_time", 0),
                           ("c", "propagator", 7), ("c", "propagator", -1),
                           ("sp", "n_sensor", 0), ("sp", "n_sensor", _lib.MAX_SENSORS + 1), ("sp", "n_sensor", -1),
                           ("a", "n_steps", 0), ("a", "n_steps", -5),
                           ("a", "bits", 0), ("a", "bits", 0x1004), ("a", "bits", 0x1001),
                           ("a", "n_sel", -1), ("a", "n_sel", 1), ("a", "n_sel", 2)):      # (n_sel > 0 with a NULL env_sel)
        assert ac.answer(lib, (blk, name, val)) == inv, (blk, name, val)
    assert ac.answer(lib, ("a", "n_sel", 3), ("a", "env_sel", 0x3000)) == inv                 # n_sel > n_env (two envs)
    assert ac.answer(lib, ("a", "n_sel", 2), ("a", "env_sel", 0x3000), n_env=1) == inv
    assert ac.answer(lib, spoil=nan_mask) == inv                                             # a NaN elevation mask
    assert ac.answer(lib, spoil=bad_rk4) == inv                                              # SSA_PROP_J2_RK4 without sub-steps
    assert ac.answer(lib, ("p", "launch_mask", _lib.LAUNCH_INLINE_ENVS), n_env=_lib.INLINE_ENVS + 1) == inv
    # n_env * n_sensor * n_obj * W >= 2^31, reached through each factor (W = 2 at 70 steps; 2 envs x 2 sensors)
    assert ac.answer(lib, ("p", "n_obj", 2 ** 28)) == inv
    assert ac.answer(lib, ("p", "n_obj", 2 ** 31)) == inv and ac.answer(lib, ("p", "n_obj", 2 ** 40)) == inv
    assert ac.answer(lib, ("p", "n_obj", 2 ** 20), ("a", "n_steps", 64 * 2 ** 9)) == inv
    assert ac.answer(lib, ("p", "n_obj", 2 ** 20), ("p", "n_env", 2 ** 10), ("a", "n_steps", 64)) == inv
    assert ac.answer(lib, ("p", "n_env", 2 ** 31 - 1), ("sp", "n_sensor", 8), ("p", "n_obj", 2 ** 31 - 1)) == inv
    assert ac.answer(lib, ("p", "n_obj", 2 ** 20), ("sp", "n_sensor", 8), ("a", "n_steps", 64 * 2 ** 7)) == inv


def test_the_shared_sensor_tail_refuses_here_as_everywhere(lib):
    """support.illumination's and support.orbiting's faults, as the nine sensor entries are given them"""
    from ssa_gym_amd import _lib
    inv = _lib.E_INVALID
    good_sun = (("sp", "sun", il.SUN_PTR), ("sp", "shadow_radius", il.R_SHADOW))
    good_site = (("p", "site_rows", ob.SITE_PTR), ("p", "limb_radius", ob.R_LIMB))
    for bits in (HIGH, HIGH | ONE, 1 << 7, 1 << 8, 1 << 30, -1):
        assert ac.answer(lib, ("sp", "sunlit_only", bits), *good_sun) == inv, bits
    for ptr in (0, il.SUN_PTR + 8, il.SUN_PTR + 16, il.SUN_PTR + 1):
        assert ac.answer(lib, ("sp", "sunlit_only", ONE), ("sp", "sun", ptr), ("sp", "shadow_radius", il.R_SHADOW)) == inv, ptr
    for rad in (-1.0, float("nan"), -float("inf")):
        assert ac.answer(lib, ("sp", "sunlit_only", ONE), ("sp", "sun", il.SUN_PTR), ("sp", "shadow_radius", rad)) == inv, rad
    for bits in (HIGH, HIGH | ONE, ZERO, ZERO | ONE, 1 << 7, 1 << 8, 1 << 30, -1):
        assert ac.answer(lib, ("p", "site_moving", bits), *good_site) == inv, bits
    assert ac.answer(lib, ("p", "site_moving", ONE), ("sp", "n_sensor", 1), *good_site) == inv
    for ptr in (0, ob.SITE_PTR + 8, ob.SITE_PTR + 32, ob.SITE_PTR + 64, ob.SITE_PTR + 1):
        assert ac.answer(lib, ("p", "site_moving", ONE), ("p", "site_rows", ptr), ("p", "limb_radius", ob.R_LIMB)) == inv, ptr
    for rad in (-1.0, float("nan"), -float("inf")):
        assert ac.answer(lib, ("p", "site_moving", ONE), ("p", "site_rows", ob.SITE_PTR), ("p", "limb_radius", rad)) == inv, rad
    assert ac.answer(lib, ("p", "site_moving", ONE), ("c", "obs_type", _lib.OBS_XYZ), *good_site) == inv


# ---------------------------------------------------------------------------------------------------------------- 3. the numpy statement
def _col(text, T=None):
    col = np.array([c == "1" for c in text])
    return col if T is None else np.concatenate([col, np.zeros(T - len(col), dtype=bool)])


def test_packing_crosses_the_word_boundary():
    acc = np.zeros((70, 2), dtype=bool)
    acc[[0, 63, 64, 69], 0] = True
    acc[:, 1] = True
    bits = ac.pack(acc)
    assert bits.shape == (2, 2) and bits.dtype == np.int64
    u = bits.view(np.uint64)
    assert u[0].tolist() == [(1 << 63) | 1, (1 << 5) | 1] and u[1].tolist() == [2 ** 64 - 1, (1 << 6) - 1]
    assert bits[0, 0] < 0                                        # (bit 63 is the sign of the int64 word torch holds)
    assert np.array_equal(ac.unpack(bits, 70), acc)
    assert ac.pack(np.ones((64, 1), dtype=bool)).shape == (1, 1) and ac.pack(np.ones((65, 1), dtype=bool)).shape == (1, 2)
    assert ac.pack(np.ones((1, 1), dtype=bool)).tolist() == [[1]]


def test_the_summary_of_hand_made_patterns():
    for text, want in (("0", (-1, 0, 0, 0)), ("1", (0, 1, 1, 1)), ("0110", (1, 2, 2, 1)), ("1011", (0, 1, 3, 2)),
                       ("10110111", (0, 1, 6, 3)), ("0" * 63 + "11", (63, 2, 2, 1)), ("1" * 65, (0, 65, 65, 1)),
                       ("1" * 64 + "01", (0, 64, 65, 2))):
        got = ac.summary(_col(text)[:, None])
        assert got.shape == (1, 4) and got.dtype == np.int32 and tuple(got[0].tolist()) == want, (text, got)
    both = ac.summary(np.stack([_col("0110", 5), _col("10101", 5)], axis=1).reshape(5, 1, 2))
    assert both.shape == (1, 2, 4) and both[0].tolist() == [[1, 2, 2, 1], [0, 1, 3, 3]]


def test_n_left_cuts_a_pass():
    acc = _col("0011110011", 10)[:, None]
    assert ac.summary(acc)[0].tolist() == [2, 4, 6, 2]
    assert ac.summary(ac.cut(acc, 4))[0].tolist() == [2, 2, 2, 1]      # the first pass cut after two of its four steps
    assert ac.summary(ac.cut(acc, 2))[0].tolist() == [-1, 0, 0, 0] and ac.summary(ac.cut(acc, -1))[0].tolist() == [-1, 0, 0, 0]
    assert ac.summary(ac.cut(acc, 70))[0].tolist() == [2, 4, 6, 2]
    assert ac.pack(ac.cut(acc, 4)).view(np.uint64).tolist() == [[0b1100]]


# ---------------------------------------------------------------------------------------------------------------- 4. the code object
def _prop(name):
    return re.search(r"ILi(\d)E", name).group(1)


def test_the_four_kernels_in_the_shipped_code_object(tmp_path):
    """exactly four instances; no LDS, no VGPR spills, no atomics; scratch touched only where the stand-alone propagate kernel of the
    same propagator touches it (around its out-of-line calls) -- the VGPR counts are recorded in profiles/access_sensors_isa.txt, not
    pinned"""
    kern, ins = _kernels(tmp_path)
    names = family(kern, "access_sensors_kernel")
    assert len(names) == 4 and sorted(_prop(n) for n in names) == ["0", "1", "2", "3"], names
    alone = {"0": [k for k in family(kern, "propagate_kernel") if _prop(k) == "0"], "1": [k for k in family(kern, "propagate_kernel") if _prop(k) == "1"],
             "2": family(kern, "propagate_j2_kernel"), "3": family(kern, "propagate_hybrid_kernel")}
    for n in names:
        k, ops = kern[n], ins[n]
        (twin,) = alone[_prop(n)]
        assert k["group_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (n, k)
        assert not [op for op in ops if "atomic" in op or op.startswith(("ds_", "buffer_atomic"))], n
        assert not stray_scratch(ops), (n, stray_scratch(ops)[:8])
        if "s_swappc_b64" not in ins[twin]:      # (no out-of-line call in the operator: none here, and no scratch at all)
            assert "s_swappc_b64" not in ops and k["private_segment_fixed_size"] == 0, (n, k)
        if kern[twin]["private_segment_fixed_size"] == 0:
            assert k["private_segment_fixed_size"] == 0, (n, k)
