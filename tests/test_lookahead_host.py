"""CPU-only checks of the one-step tasking lookahead (include/ssa_hip.h: ssa_lookahead_f64): the export, the output struct's layout
and constants against the header, the kernel's resource budget in the shipped code object, and no CPU fallback."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from support.codeobj import KERNEL_FAMILIES, _kernels, assert_family_budget, family, header
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.refusals import LOOK_PTRS, OUT_PTRS, refused


def test_lookahead_is_exported_and_declared(lib):
    from ssa_gym_amd import _lib
    assert re.search(r"\bssa_lookahead_f64\s*\(", header())
    assert "ssa_lookahead_f64" in _lib.SIGNATURES
    assert hasattr(lib, "ssa_lookahead_f64")
    assert lib.ssa_abi_version() == _lib.ABI_VERSION == 23


def test_lookahead_out_layout_and_constants_match_the_header(lib, tmp_path):
    from ssa_gym_amd import _lib
    st = _lib.ssa_lookahead_out
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "ssa_hip.h"', 'int main(void){',
           'printf("%zu\\n", sizeof(ssa_lookahead_out));']
    want = [C.sizeof(st)]
    for f, _ in st._fields_:
        src.append('printf("%%zu\\n", offsetof(ssa_lookahead_out, %s));' % f)
        want.append(getattr(st, f).offset)
    src.append('return 0;}')
    c = tmp_path / "look.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "look"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).decode().split()] == want
    hdr = header()
    for name in ("LOOK_NSCORE", "LOOK_TRACE_GAIN", "LOOK_POS_TRACE_GAIN", "LOOK_INFO_GAIN"):
        m = re.search(r"#define SSA_%s\s+(\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(_lib, name), name


def test_lookahead_refuses_bad_arguments_before_any_launch(lib):
    """argument checks come first: NULL blocks / inputs / required outputs are refused with SSA_E_INVALID, no device is touched"""
    from ssa_gym_amd import _lib
    f = lib.ssa_lookahead_f64
    assert f(None, None, None, None) == _lib.E_INVALID
    for k in range(3):
        assert refused(f, None, null=k) == _lib.E_INVALID, k
    for case in [("o", nm, 0) for nm in OUT_PTRS] + [("p", nm, 0) for nm in LOOK_PTRS]:
        assert refused(f, None, ("p", "n_obj", 4), case) == _lib.E_INVALID, case


def test_env_lookahead_has_no_cpu_fallback(lib):
    from ssa_gym_amd import _lib
    from ssa_gym_amd.envs.ssa_tasker_simple_2 import SSA_Tasker_Env
    env = SSA_Tasker_Env.__new__(SSA_Tasker_Env)     # (an env without device state: what a machine without a GPU has)
    env._engine, env.i, env.n = None, 0, 480
    with pytest.raises(_lib.SsaHipError):
        env.lookahead()


def test_lookahead_kernels_keep_the_step_kernels_budget(tmp_path):
    """the lookahead instances fit the step kernel's register budget and LDS, and touch scratch only where the step kernel does:
    the save / restore around the out-of-line calls of SSA_PROP_ELEMENTS / SSA_PROP_HYBRID -- none on the common path"""
    kern, ins_of = _kernels(tmp_path)
    assert_family_budget(kern, ins_of, "lookahead_kernel", None, KERNEL_FAMILIES["lookahead_kernel"])      # 4 propagators x {one tile, multi tile}
    for name in family(kern, "lookahead_kernel"):
        assert kern[name]["group_segment_fixed_size"] <= 160 * 1024 // 20, (name, kern[name])
