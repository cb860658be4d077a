"""Static facts of the shipped code object about how the one-tile step kernels fetch their inputs (host test: nothing is launched)."""
from support.codeobj import _kernels


def test_one_tile_step_kernels_load_nothing_through_the_flat_segment(tmp_path):
    """step_fast_kernel<P, false>, P = 0 .. 3: the action word, the time word and the tile's obj_ids are wave-uniform words that no wavefront
    of a step launch writes, so they come by scalar loads (several envs: per-lane global loads).  A load through the FLAT segment in one of
    these instances means the compiler was handed a generic pointer again -- a select between the argument segment and device memory -- and
    the wavefront waits for the vector-memory AND the LDS queue behind its tile's loads."""
    kern, ins_of = _kernels(tmp_path)
    one_tile = [n for n in ins_of if "step_fast_kernel" in n and "ELb0E" in n]
    assert len(one_tile) == 4, one_tile
    for name in one_tile:
        flat = [op for op in ins_of[name] if op.startswith("flat_load")]
        assert not flat, (name, flat[:8])
        assert any(op.startswith("global_load_lds") for op in ins_of[name]), name     # (the instance that loads its tile by LDS-DMA)
