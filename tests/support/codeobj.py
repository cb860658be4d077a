"""The public header's text, and the gfx950 code object of the built library: per-kernel metadata and instruction lists."""
import os

import pytest

from conftest import ROOT


def header():
    return open(os.path.join(ROOT, "include", "ssa_hip.h")).read()


def _code_object(tmp_path):
    """the gfx950 code object embedded in the built libssa_hip.so (the file that ships), its metadata and disassembly"""
    import shutil
    import subprocess
    import ssa_gym_amd
    from ssa_gym_amd import _build
    ssa_gym_amd.build()
    b = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(b, "clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools here")
    fb, co = str(tmp_path / "fb.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([os.path.join(b, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, _build.LIB, str(tmp_path / "copy.so")])
    subprocess.check_call([os.path.join(b, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fb, "--output=" + co])
    notes = subprocess.check_output([os.path.join(b, "llvm-readelf"), "--notes", co], text=True)
    dis = subprocess.check_output([os.path.join(b, "llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True)
    shutil.rmtree(str(tmp_path), ignore_errors=True)
    return notes, dis


_KERNELS = {}      # (library path, mtime) -> what _kernels returns: the 4.5 MB code object is extracted and disassembled once


def _kernels(tmp_path):
    """the built code object (_code_object) per kernel: {name: metadata} -- register counts, scratch, LDS, the arguments' value
    kinds and the offsets of the by-value ones -- and {name: instruction list} (the opcodes of its disassembly, in order)"""
    import re
    import ssa_gym_amd
    from ssa_gym_amd import _build
    ssa_gym_amd.build()
    key = (_build.LIB, os.path.getmtime(_build.LIB))
    if key in _KERNELS:
        return _KERNELS[key]
    notes, dis = _code_object(tmp_path)
    meta = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in
                      ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size")}
        meta[name]["arg_kinds"] = re.findall(r"\.value_kind:\s+(\w+)", blk)
        meta[name]["by_value_offsets"] = [int(v) for v in re.findall(r"\.offset:\s+(\d+)\s+\.size:\s+\d+\s+\.value_kind:\s+by_value", blk)]
    bodies = re.split(r"\n[0-9a-f]+ <([^>]+)>:\n", dis)
    ins = {name: [ln.split()[0] for ln in body.splitlines() if ln.strip() and not ln.strip().startswith(("//", ";"))]
           for name, body in zip(bodies[1::2], bodies[2::2])}
    _KERNELS[key] = meta, ins
    return meta, ins


def stray_scratch(ops):
    """(the indices of) the scratch accesses of an instruction list that lie away from every out-of-line call (s_swappc_b64)"""
    calls = [i for i, op in enumerate(ops) if op == "s_swappc_b64"]
    return [i for i, op in enumerate(ops) if op.startswith("scratch_") and not (calls and min(abs(i - c) for c in calls) <= 96)]


# the kernel families the host tests count, and the instances each has in the shipped code object: 4 propagators, x {one tile, multi
# tile} for the tile kernels (tests/test_abi_and_host.py checks the table against the code object)
KERNEL_FAMILIES = {"lookahead_kernel": 8, "step_sensors_kernel": 8, "lookahead_sensors_kernel": 8, "vector_sensors_kernel": 8,
                   "lookahead_sensor_envs_kernel": 8, "rollout_kernel": 4, "rollout_sensors_kernel": 4, "forecast_sensors_kernel": 4,
                   "forecast_sensor_envs_kernel": 4, "rollout_sensor_envs_kernel": 4, "rollout_fold_kernel": 1,
                   "rollout_fold_steps_kernel": 1, "assign_sensors_kernel": 1, "assign_sensors_envs_kernel": 1}


def family_of(name):
    """the function's own name, read from its mangled one (_Z<len><name>, _ZN<len><namespace>...<len><name>): exact, no substrings"""
    import re
    i, last = re.match(r"_ZN?|", name).end(), None
    while i and name[i:i + 1].isdigit():
        n = re.match(r"\d+", name[i:]).group(0)
        last = name[i + len(n):i + len(n) + int(n)]
        i += len(n) + int(n)
    return last


def family(kern, name):
    """the instances of the family `name`, sorted"""
    return sorted(k for k in kern if family_of(k) == name)


def _form(name):
    """a kernel's template arguments: (propagator, multi-tile or None for a resident kernel)"""
    import re
    m = re.search(r"ILi(\d)E(?:Lb([01])E)?E", name)
    return m.group(1), m.group(2)


def twin(kern, name, against):
    """the instance of the family `against` with `name`'s propagator and launch form (for a resident kernel: a tile kernel's one-tile form)"""
    prop, multi = _form(name)
    ref = [k for k in family(kern, against) if _form(k) in ((prop, multi), (prop, multi or "0"))]
    assert len(ref) == 1, (name, against, ref)
    return ref[0]


def assert_family_budget(kern, ins_of, name, against, instances, same_args=False, scratch_against=None):
    """every one of the `instances` kernels of the family `name`: at most 96 VGPRs (5 wavefronts per SIMD); scratch touched only around
    the out-of-line calls (SSA_PROP_ELEMENTS / SSA_PROP_HYBRID); FG and J2 without calls, scratch or spills.  against: a family -- the
    LDS of its instance of the same propagator and form, and no more scratch or VGPR spills than it (scratch_against: ... than that
    family's instead).  same_args: its argument kinds too, and -- unless 'kinds' -- the offsets of the by-value ones."""
    names = family(kern, name)
    assert len(names) == instances, (name, names)
    for k_name in names:
        k, ins = kern[k_name], ins_of[k_name]
        assert k["vgpr_count"] <= 96, (k_name, k)
        if against:
            b, s = kern[twin(kern, k_name, against)], kern[twin(kern, k_name, scratch_against or against)]
            assert k["group_segment_fixed_size"] == b["group_segment_fixed_size"], (k_name, k, b)
            assert k["private_segment_fixed_size"] <= s["private_segment_fixed_size"], (k_name, k, s)
            assert k["vgpr_spill_count"] <= s["vgpr_spill_count"], (k_name, k, s)
            if same_args:
                assert k["arg_kinds"] == b["arg_kinds"], k_name
                assert same_args == "kinds" or k["by_value_offsets"] == b["by_value_offsets"], k_name
        assert not stray_scratch(ins), (k_name, stray_scratch(ins)[:8])
        if _form(k_name)[0] not in "03":
            assert "s_swappc_b64" not in ins and k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (k_name, k)
