"""The plain family's whole-tile store stage (plain_tile_out, ssa_kernels.hip) against the generic step kernel at the sizes where it can
go wrong and tests/test_step_plain_gpu.py does not look: the metrics and the status word leave from the lanes that computed them, every
other word from one batch of LDS reads, through (scalar base) + (32-bit lane offset) stores.

  3 objects     a ragged tile only: the new stage must not run, and the ragged path next to it must be what it was
  4 objects     ONE whole tile, which also holds the update, the NaN state and the failed filter
  8 objects     two whole tiles
  20 480        the largest one-tile launch: the lane offsets and lane x n_obj of the metrics rows at their largest (5 120 wavefronts)

Each case runs 6 deferred-fold steps on a two-slot ring from one state in two engines -- one with HotPathEngine.force_generic -- and
compares, without tolerance, the whole slot every step wrote (truth, state, covariance, observation rows, metrics rows, status words,
update record), every step's statistics row -- folded by the NEXT launch's service wavefronts from the metrics rows, which now leave
from other lanes --, the failure log and its count.  Planted: a NaN filter state (the sentinels go through the batch) and a filter that
has failed at entry (the pass-through goes through the batch).  `hybrid` runs under a storage layout (obj_ids), `fg` without one."""
import pytest

from support.gpu import hip  # noqa: F401  (the module fixture)
from support.plain_step import N_STEPS, assert_same_bits, planted, run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("m", [3, 4, 8, 20480])
@pytest.mark.parametrize("propagator", ["hybrid", "fg"])
def test_plain_store_stage_equals_the_generic_one_bit_for_bit(hip, propagator, m):
    import numpy as np
    L = hip.lib
    layout = propagator == "hybrid"
    want = run(hip, m, propagator, layout, generic=True)
    got = run(hip, m, propagator, layout, generic=False)
    assert want["instances"] == {0} and got["instances"] == {1}      # the forced engine ran generic launches only, the other plain ones only
    assert_same_bits(hip, want, got, (propagator, m))
    # the planted state did its work in the generic run: the failed filter kept its status, the NaN state failed in the first step,
    # and the last statistics row counts both
    nan_obj, failed_obj = planted(m)
    order = np.random.RandomState(m).permutation(m) if layout else np.arange(m)
    at = {int(o): i for i, o in enumerate(order)}
    st = want["steps"][0][1]["status"].cpu().numpy()
    assert st[at[failed_obj]] == L.ST_UPDATE_LINALG and st[at[nan_obj]] != 0 and want["nfail"] >= 1
    last = want["rows"][N_STEPS].view(hip.torch.float64)[0].cpu().numpy()
    assert last[L.STAT_N_FAILED] >= 2
