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


def _kernels(tmp_path):
    """the built code object (_code_object) per kernel: {name: metadata} -- register counts, scratch, LDS, the arguments' value
    kinds and the offsets of the by-value ones -- and {name: instruction list} (the opcodes of its disassembly, in order)"""
    import re
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
    return meta, ins


def stray_scratch(ops):
    """(the indices of) the scratch accesses of an instruction list that lie away from every out-of-line call (s_swappc_b64)"""
    calls = [i for i, op in enumerate(ops) if op == "s_swappc_b64"]
    return [i for i, op in enumerate(ops) if op.startswith("scratch_") and not (calls and min(abs(i - c) for c in calls) <= 96)]
