"""The plain family's factorisation (chol_step_fused / chol_row_regs_fused / chol_store_rows_zeroed, ssa_kernels.hip), what can be said
without a GPU: the built code object holds the fused form in the four step_plain_kernel instances and nowhere else, inside the register,
scratch and LDS figures the family runs at; and the two pieces of integer reasoning the kernel's source states in comments -- which
lanes write +0.0 where, and how a row's six finite-test bits become the row's sixteen -- hold for every input, with the constants read
from the source."""
import os
import re

import numpy as np

from conftest import ROOT
from support.codeobj import _form, _kernels, family, twin

SRC = os.path.join(ROOT, "ssa-gym_amd", "csrc", "ssa_kernels.hip")


def _body(name):
    """the text of the device function `name` in the kernel source, from its name to the closing brace in column 0"""
    text = open(SRC).read()
    m = re.search(r"\n[^\n]*\b%s\([^\n]*\)\n\{\n(.*?)\n\}\n" % re.escape(name), text, re.S)
    assert m, name
    return m.group(1)


def test_the_fused_form_is_in_the_four_plain_instances_and_nowhere_else(tmp_path):
    kern, ins_of = _kernels(tmp_path)
    plain = family(kern, "step_plain_kernel")
    assert len(plain) == 4
    for name, ins in ins_of.items():
        fused = ins.count("v_fmac_f64_dpp")
        if name in plain:
            # 15 per factorisation (one per pair i < J), the first attempt and the winning rung's re-factorisation
            assert fused == 30, (name, fused)
            assert ins.count("v_writelane_b32") == 0 and ins.count("v_readlane_b32") <= 32, name
        else:
            assert fused == 0, (name, fused)
    for name in plain:
        k, g = kern[name], kern[twin(kern, name, "step_fast_kernel")]
        assert k["group_segment_fixed_size"] <= 7680 and k["group_segment_fixed_size"] == g["group_segment_fixed_size"], (name, k)
        assert k["vgpr_count"] <= 96 and k["vgpr_spill_count"] <= g["vgpr_spill_count"], (name, k, g)
        assert k["private_segment_fixed_size"] <= g["private_segment_fixed_size"], (name, k, g)
        if _form(name)[0] == "3":      # the hybrid instance, the benchmark's
            assert k["vgpr_count"] <= 88 and k["sgpr_count"] <= 104 and k["private_segment_fixed_size"] == 76, (name, k)


def test_the_zero_writes_cover_the_strictly_lower_triangle_and_nothing_else():
    """chol_store_rows_zeroed: lane l of a row writes through &Ug[l]; entry (j, c) of the row-major 6 x 6 block is 6 j + c"""
    body = _body("chol_store_rows_zeroed")
    blocks = re.findall(r"if \(row_lanes\((0x[0-9A-Fa-f]+)ull\)\) \{(.*?)\}", body, re.S)
    assert len(blocks) == 3
    values, zeros = blocks[0], blocks[1:]
    assert int(values[0], 16) == 0x3F and "uc[j]" in values[1]      # the six owning lanes write the rows
    hit = []
    for mask, text in zeros:
        offs = [int(o) for o in re.findall(r"col\[(\d+)\] = z;", text)]
        assert len(offs) == 2                                       # one two-address write each
        lanes = [l for l in range(16) if (int(mask, 16) >> l) & 1]
        assert int(mask, 16) < (1 << 16) and lanes
        hit += [l + o for l in lanes for o in offs]
    lower = sorted(6 * j + c for j in range(6) for c in range(j))
    assert sorted(set(hit)) == lower and max(hit) < 36, (sorted(hit), lower)
    # and the mask of every row is the constant repeated: row_lanes
    assert re.search(r"row_lanes\(unsigned long long m16\) \{ return [a-z_0-9]+\(m16 \* 0x0001000100010001ull\); \}", open(SRC).read())


def _row_fill(nf):
    """chol_row_regs_fused's scalar arithmetic on the ballot of the finite tests, 64-bit wrap-around as the scalar unit's"""
    M = (1 << 64) - 1
    nf &= 0x003F003F003F003F
    h = ((nf + 0x7FFF7FFF7FFF7FFF) & M) & 0x8000800080008000
    return h | ((h - (h >> 15)) & M)


def test_six_bits_of_a_row_fill_its_sixteen():
    body = _body("chol_row_regs_fused")
    for const in ("0x003F003F003F003Full", "0x7FFF7FFF7FFF7FFFull", "0x8000800080008000ull", "h | (h - (h >> 15))"):
        assert const in body, const
    # every pattern of the six deciding lanes in every row, whatever the lanes 6 .. 15 and the other rows hold
    rs = np.random.RandomState(5)
    for row in range(4):
        for six in range(64):
            for _ in range(4):
                other = int(rs.randint(0, 1 << 16)) | (int(rs.randint(0, 1 << 16)) << 16) | (int(rs.randint(0, 1 << 16)) << 32) | (int(rs.randint(0, 1 << 16)) << 48)
                keep = other & ~(0x3F << (16 * row))
                got = _row_fill(keep | (six << (16 * row)))
                want = 0
                for r in range(4):
                    bits6 = six if r == row else (keep >> (16 * r)) & 0x3F
                    want |= (0xFFFF if bits6 else 0) << (16 * r)
                assert got == want, (row, six, hex(other))
    assert _row_fill(0) == 0 and _row_fill((1 << 64) - 1) == (1 << 64) - 1
