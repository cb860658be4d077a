"""Compare the gfx950 code objects of two builds of libssa_hip.so, kernel by kernel: resource notes and instruction lists.

    python profiles/isa_compare.py PARENT/libssa_hip.so THIS/libssa_hip.so > profiles/<change>_isa.txt

The extraction is tests/support/codeobj.py's (llvm-objcopy, clang-offload-bundler, llvm-readelf --notes, llvm-objdump -d); an
"instruction list" is the opcodes of a kernel's disassembly in order, the reader the test suite uses.  Beside it the operands are
compared too, so that a changed literal or offset is told apart from a changed instruction."""
import os
import re
import subprocess
import sys
import tempfile

BIN = "/opt/rocm/lib/llvm/bin"
KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count")


def kernels(lib):
    with tempfile.TemporaryDirectory() as tmp:
        fb, co = os.path.join(tmp, "fb.bin"), os.path.join(tmp, "dev.co")
        subprocess.check_call([os.path.join(BIN, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, lib, os.path.join(tmp, "copy.so")])
        subprocess.check_call([os.path.join(BIN, "clang-offload-bundler"), "--unbundle", "--type=o",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fb, "--output=" + co])
        notes = subprocess.check_output([os.path.join(BIN, "llvm-readelf"), "--notes", co], text=True)
        dis = subprocess.check_output([os.path.join(BIN, "llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True)
    meta = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in KEYS}
        meta[name]["kernarg"] = int(re.search(r"\.kernarg_segment_size:\s+(\d+)", blk).group(1))
    bodies = re.split(r"\n[0-9a-f]+ <([^>]+)>:\n", dis)
    lines = {}
    for name, body in zip(bodies[1::2], bodies[2::2]):
        rows = [ln.strip() for ln in body.splitlines() if ln.strip() and not ln.strip().startswith(("//", ";"))]
        lines[name] = [re.sub(r"\s*//.*$", "", r) for r in rows]
    return meta, lines


def opcodes(rows):
    return [r.split()[0] for r in rows]


def main(parent, this):
    pm, pl = kernels(parent)
    tm, tl = kernels(this)
    print("kernels: parent %d, this commit %d.  Added: %s.  Removed: %s." %
          (len(pm), len(tm), ", ".join(sorted(set(tm) - set(pm))) or "none", ", ".join(sorted(set(pm) - set(tm))) or "none"))
    same_all, same_ops, changed = [], [], []
    for name in sorted(set(pm) & set(tm)):
        notes_same = all(pm[name][k] == tm[name][k] for k in KEYS)
        if notes_same and pl[name] == tl[name]:
            same_all.append(name)
        elif notes_same and opcodes(pl[name]) == opcodes(tl[name]):
            same_ops.append(name)
        else:
            changed.append(name)
    print("\n1. identical disassembly (operands included) and resource notes: %d kernels" % len(same_all))
    print("\n2. identical instruction list and resource notes, operands differ: %d kernels" % len(same_ops))
    for name in same_ops:
        diff = [(a, b) for a, b in zip(pl[name], tl[name]) if a != b]
        kinds = sorted({a.split()[0] for a, _ in diff})
        print("   %-100s %5d lines differ: %s%s" % (name, len(diff), " ".join(kinds),
              "   kernarg %d->%d" % (pm[name]["kernarg"], tm[name]["kernarg"]) if pm[name]["kernarg"] != tm[name]["kernarg"] else ""))
    print("\n3. changed instruction list or resource notes: %d kernels (parent -> this commit)" % len(changed))
    print("   %-100s %10s %10s %6s %8s %7s %15s %9s" % ("kernel", "VGPR", "SGPR", "LDS", "scratch", "spills", "instructions", "s_load"))
    for name in changed:
        def col(k):
            a, b = pm[name][k], tm[name][k]
            return "%d" % a if a == b else "%d->%d" % (a, b)
        sl = lambda rows: sum(1 for op in opcodes(rows) if op.startswith("s_load_"))
        print("   %-100s %10s %10s %6s %8s %7s %15s %9s" % (name, col("vgpr_count"), col("sgpr_count"), col("group_segment_fixed_size"),
              col("private_segment_fixed_size"), col("vgpr_spill_count"), "%d->%d" % (len(pl[name]), len(tl[name])),
              "%d->%d" % (sl(pl[name]), sl(tl[name]))))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
