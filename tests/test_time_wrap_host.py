"""The time-row tests' own construction, on the CPU (tests/support/time_wrap.py; the GPU half: tests/test_time_wrap_gpu.py): the row
choice of the long and the shifted tables on crafted arrays, the recomputed strides against the engine's extent rule, every scene's
margins and non-vacuity on the CPU oracle, and that a control's table set is wrong in one table and from row T on only."""
import numpy as np
import pytest

from support import time_wrap as tw

T = tw.T


def _crafted(E=2, S=3, m=5):
    """tables whose every element names its own (table, row): a wrong row anywhere is visible"""
    r = np.arange(T, dtype=np.float64)
    return dict(trans=r[:, None] * 100 + np.arange(9), z_noise=np.broadcast_to(r[None, None, :, None, None], (E, S, T, m, 3)) * 1000
                + np.arange(E * S * T * m * 3).reshape(E, S, T, m, 3) % 7, sun=r[:, None] * 10 + np.arange(3), dark=np.arange(T) + 1,
                site_rows=r[:, None, None] * 50 + np.arange(S * 16).reshape(1, S, 16))


def test_extend_and_shift_choose_the_rows_numpy_chooses():
    assert tw.LONG == 4 * T and np.array_equal(tw.long_rows(), np.arange(4 * T) % T)
    assert tw.wrong_rows().tolist() == list(range(T)) + [(r + 1) % T for r in range(T, 4 * T)]
    short = _crafted()
    long = tw.variant(short, "long")
    for k, a in short.items():
        ax = tw.AXIS[k] % a.ndim
        assert long[k].shape[ax] == 4 * T and long[k].flags.c_contiguous
        for r in range(4 * T):
            assert np.array_equal(np.take(long[k], r, axis=ax), np.take(a, r % T, axis=ax)), (k, r)
    assert tw.variant(short) is short
    # the largest index any case reaches stays on the long tables
    assert max(max(w) + K - 1 for _, _, _, w, K in tw.CASES) < tw.LONG and max(tw.SINGLE) == 3 * T + 5


@pytest.mark.parametrize("which", tw.TABLES)
def test_a_control_is_wrong_in_one_table_from_row_T_on(which):
    short = _crafted()
    long, wrong = tw.variant(short, "long"), tw.variant(short, which)
    for k, a in short.items():
        ax = tw.AXIS[k] % a.ndim
        if tw.OWNER.get(k, k) != which:
            assert np.array_equal(wrong[k], long[k]), k
            continue
        for r in range(4 * T):
            same = np.array_equal(np.take(wrong[k], r, axis=ax), np.take(long[k], r, axis=ax))
            assert same == (r < T), (k, r)
            assert np.array_equal(np.take(wrong[k], r, axis=ax), np.take(a, (r + 1) % T if r >= T else r, axis=ax)), (k, r)


@pytest.mark.parametrize("E,S,m", [(1, 3, 8), (1, 3, 7), (3, 3, 8), (2, 3, 12)])
def test_the_recomputed_strides_satisfy_the_engines_extent_rule(E, S, m):
    short = _crafted(E, S, m)
    for tabs in (short, tw.variant(short, "long"), tw.variant(short, "z_noise")):
        st = tw.strides(tabs)
        n = tabs["trans"].shape[0]
        assert st == dict(time=3 * m, sensor=n * m * 3, env=S * n * m * 3, n_time=n) and tw.extent_ok(tabs)
        # element (e, s, r, j, c) sits where the kernel looks for it
        flat = tabs["z_noise"].reshape(-1)
        for e, s, r, j in ((E - 1, S - 1, n - 1, m - 1), (0, 1, n // 2, 2)):
            assert flat[e * st["env"] + s * st["sensor"] + r * st["time"] + j * 3 + 1] == tabs["z_noise"][e, s, r, j, 1]
    # the short strides on the long table would read other rows: the recomputation is not optional
    assert tw.strides(short)["sensor"] != tw.strides(tw.variant(short, "long"))["sensor"]


@pytest.mark.parametrize("case", sorted(set(tw.CASES)), ids=lambda c: "%s-m%d-E%d-t%s-K%d" % (c[0], c[1], c[2], "_".join(map(str, c[3])), c[4]))
def test_every_scene_has_margin_and_a_cell_of_every_table_at_every_wrapped_index(oracle, oracle_ld, case):
    """what the GPU module relies on, found here when a scene cannot deliver it: every judged cell of the row and of its neighbour
    keeps the margins of support.illumination / support.orbiting, sensor 0 sees its object at every wrapped index, and the Sun row, the
    dark word and (moving) the site row each decide a tasked cell the other way than the neighbour row"""
    kind, m, E, words, K = case
    sc = tw.scene(oracle, oracle_ld, kind, m, E, tw.phase_of(words, K))
    assert sc.check(words, K) == sum(1 for w in words for k in range(K) if w + k >= T)
    assert sc.state[0].shape == (E * m, 6) and sc.acts.shape == (E, 3) and sc.acts.max() < m
    for e in range(E):      # the tasked rows hold objects 0, 1, 2
        assert sc.src[sc.acts[e]].tolist() == [0, 1, 2]
    for name in sc.tables():
        wrong = tw.variant(sc.tabs, name)
        assert tw.extent_ok(wrong) and wrong["trans"].shape[0] == tw.LONG


def test_the_multi_tile_case_puts_both_envs_updates_into_one_wavefronts_tiles():
    """2 x 10 244 objects = 5 122 tiles for the 5 120 wavefronts of the grid-stride instance: wavefront 0 walks tile 0 (env 0) and tile
    5 120 (env 1), and those are the tiles the two envs' sensors task"""
    m = tw.M_TILES
    assert m % 4 == 0 and 2 * m > 20480
    first, second = 0, m + (m - 8)
    assert first // 4 == 0 and second // 4 == 5120 and (second + 2) // 4 == 5120


@pytest.mark.parametrize("m", [8, 7])
def test_the_closed_loops_object_stands_on_the_mask(oracle, oracle_ld, m):
    """the object that makes the greedy agent's visibility mask depend on its row: hidden at rows T - 2 and T - 1, seen at step T under
    row 0 and hidden under row 1, 1e-4 rad from the mask every time; the others stay where the plain scene has them"""
    sc = tw.scene(oracle, oracle_ld, "moving", m, 1, 0, edge=True)
    tw.check_edge(sc)
    plain = tw.scene(oracle, oracle_ld, "moving", m, 1, 0)
    keep = np.arange(8) != tw.EDGE
    assert all(np.array_equal(a[keep], b[keep]) for a, b in zip(sc.eight, plain.eight)) and tw.EDGE < m
    for k in range(4):      # every other object is above the radar's mask at every step of the loop, under the row and its neighbour
        for row in ((T - 1 + k) % T, (T + k) % T):
            assert sc.visible(k, row)[0][0, keep].all(), (k, row)
