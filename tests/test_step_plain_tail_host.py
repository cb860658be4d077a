"""Static facts of the shipped code object about the plain family's whole-tile store stage (host test: nothing is launched)."""
import re

from support.codeobj import _code_object, family_of


def _plain_instances(tmp_path):
    """{name: [(opcode, operands)]} of the four step_plain_kernel instances, from the disassembly of the built library"""
    _, dis = _code_object(tmp_path)
    bodies = re.split(r"\n[0-9a-f]+ <([^>]+)>:\n", dis)
    out = {}
    for name, body in zip(bodies[1::2], bodies[2::2]):
        if family_of(name) != "step_plain_kernel":
            continue
        lines = [ln.split("//")[0].strip() for ln in body.splitlines()]
        out[name] = [(ln.split()[0], ln.split(None, 1)[1] if " " in ln else "") for ln in lines if ln and not ln.startswith(";")]
    return out


def test_plain_whole_tile_stores_carry_a_scalar_base_and_nothing_goes_through_the_flat_segment(tmp_path):
    """step_plain_kernel<P, false>, P = 0 .. 3.  No access through the FLAT segment: a destination pointer that reaches a store through an
    asm statement untyped is generic to the compiler, and the store waits for the LDS queue as well.  The whole-tile store stage
    (plain_tile_out) is found by its batch of LDS reads -- ds_read_b128 x 2, ds_read_b64 x 2 back to back, once per instance --: the two
    stores in front of it (metrics, status: from registers) and the five behind it (P, the tail of P, x, x_true, the observation rows)
    are all (scalar base) + (32-bit lane offset), i.e. one address register and an SGPR pair, never a 64-bit register pair and `off`."""
    inst = _plain_instances(tmp_path)
    assert len(inst) == 4, sorted(inst)
    batch = ["ds_read_b128", "ds_read_b128", "ds_read_b64", "ds_read_b64"]
    for name, ins in inst.items():
        ops = [op for op, _ in ins]
        assert not [op for op in ops if op.startswith("flat_")], name
        at = [i for i in range(len(ops) - 3) if ops[i:i + 4] == batch]
        assert len(at) == 1, (name, at)
        stores = [i for i, op in enumerate(ops) if op.startswith("global_store")]
        stage = [i for i in stores if i < at[0]][-2:] + [i for i in stores if i > at[0]][:5]
        assert len(stage) == 7, (name, stage)
        for i in stage:
            op, args = ins[i]
            assert re.match(r"v\d+, v(\d+|\[\d+:\d+\]), s\[\d+:\d+\]", args), (name, op, args)
        # ... and between the batch and the last of them nothing is fetched from the argument segment
        assert not [op for op in ops[at[0]:stage[-1]] if op.startswith("s_load")], name
