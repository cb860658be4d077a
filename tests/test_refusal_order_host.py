"""CPU-only: the ORDER of the entries' argument checks.  A block that breaks two rules gets the code of the rule its entry checks first,
and siblings differ in that order (ssa_forecast_sensors_envs_f64 answers n_obj = 6, n_steps = 0 with SSA_E_UNSUPPORTED, the rollout's
*_envs entry with SSA_E_INVALID).  tests/golden/refusal_order.json holds the code every case below got from the library as it stood
BEFORE the checks were gathered into shared predicates (`python tests/test_refusal_order_host.py` on a build of that commit wrote
it): the order may only change on purpose, with that file.  Every case is refused before a launch."""
import json
import os

import pytest

from conftest import GOLDEN
from support.gpu import lib  # noqa: F401  (the module fixture)
from support.refusals import PTR, nan_mask, refused, valid_blocks

TABLE = os.path.join(GOLDEN, "refusal_order.json")
NAN = ("sp", "obs_limit[1]", "nan")
RAGGED = ("p", "n_obj", 6)
IDS, SHARDS = ("p", "obj_ids", PTR), ("p", "stat_shards", PTR)
MASK = {"INLINE_ENVS": 64, "MIRROR_F32": 128, "STATS_FROM_METRICS": 256}      # (checked against _lib below)
BAD_PROP = ("c", "propagator", 7)
NINE_INLINE = (("p", "n_env", 9), ("p", "launch_mask", MASK["INLINE_ENVS"]))
# (entry, n_env of the base blocks, the fields spoiled): 8 objects, 2 sensors, zn_stride_sensor = 384 otherwise
CASES = [
    ("ssa_env_step_sensors_f64", 2, (("sp", "n_sensor", 9),)),
    ("ssa_env_step_sensors_f64", 2, (NAN,)),
    ("ssa_env_step_sensors_f64", 2, (("sp", "zn_stride_sensor", 0),)),
    ("ssa_env_step_sensors_f64", 1, (("sp", "zn_stride_sensor", 0), ("p", "stat_ws", 0))),
    ("ssa_lookahead_sensors_f64", 2, (("o", "score", 0),)),
    ("ssa_lookahead_sensors_f64", 2, (("sp", "n_sensor", 0),)),
    ("ssa_lookahead_sensors_f64", 2, (NAN,)),
    ("ssa_forecast_sensors_f64", 2, (("f", "n_steps", 0),)),
    ("ssa_forecast_sensors_f64", 2, (("o", "score", 0),)),
    ("ssa_env_rollout_sensors_f64", 2, (("r", "n_steps", 0),)),
    ("ssa_env_rollout_sensors_f64", 2, (("rs", "actions", 0),)),
    ("ssa_env_rollout_sensors_f64", 2, (("sp", "n_sensor", 0),)),
    ("ssa_env_step_sensors_envs_f64", 2, (RAGGED, ("v", "actions", 0))),
    ("ssa_env_step_sensors_envs_f64", 2, (RAGGED, ("p", "stat_ws", 0))),
    ("ssa_env_step_sensors_envs_f64", 2, (RAGGED, ("p", "launch_mask", MASK["STATS_FROM_METRICS"]))),
    ("ssa_env_step_sensors_envs_f64", 2, (RAGGED, NAN)),
    ("ssa_lookahead_sensors_envs_f64", 2, (RAGGED, ("o", "score", 0))),
    ("ssa_lookahead_sensors_envs_f64", 2, (RAGGED, NAN)),
    ("ssa_forecast_sensors_envs_f64", 2, (RAGGED, ("f", "n_steps", 0))),
    ("ssa_forecast_sensors_envs_f64", 2, (RAGGED, ("o", "score", 0))),
    ("ssa_env_rollout_sensors_envs_f64", 2, (RAGGED, ("re", "actions", 0))),
    ("ssa_env_rollout_sensors_envs_f64", 2, (RAGGED, ("r", "n_steps", 0))),
    ("ssa_env_rollout_sensors_envs_f64", 2, (RAGGED, ("p", "launch_mask", MASK["INLINE_ENVS"]))),
    ("ssa_env_rollout_sensors_envs_f64", 2, (RAGGED, ("sp", "zn_stride_sensor", 0))),
    # step_launch: whole tiles per env (obj_ids, spos_tiles), the envs by value, the 2^31 rows -- each against a neighbour
    ("ssa_env_step_f64", 2, (RAGGED, IDS, SHARDS, ("p", "aer_cols", 3))),
    ("ssa_env_step_f64", 2, (RAGGED, ("p", "spos_tiles", PTR), SHARDS, BAD_PROP)),
    ("ssa_env_step_f64", 2, (RAGGED, IDS, SHARDS, ("p", "fail_log", PTR))),
    ("ssa_env_step_f64", 2, (("p", "n_env", 9), ("p", "launch_mask", MASK["INLINE_ENVS"] | MASK["MIRROR_F32"]))),
    ("ssa_env_step_f64", 2, (("p", "n_obj", (1 << 30) + 2), IDS, SHARDS)),
    ("ssa_env_step_f64", 2, (("p", "n_obj", 1 << 30), ("p", "launch_mask", MASK["STATS_FROM_METRICS"]))),
    ("ssa_env_step_sensors_envs_f64", 2, (("p", "n_obj", (1 << 30) + 2),)),
    # lookahead_args, and the sensor rows on top of it
    ("ssa_lookahead_f64", 2, NINE_INLINE + (RAGGED, IDS)),
    ("ssa_lookahead_f64", 2, (RAGGED, IDS, BAD_PROP)),
    ("ssa_lookahead_f64", 2, (RAGGED, IDS, ("o", "score", 0))),
    ("ssa_lookahead_f64", 2, (("p", "n_obj", (1 << 30) + 2), IDS)),
    ("ssa_lookahead_sensors_envs_f64", 2, (("p", "n_obj", (1 << 30) + 2),)),
    ("ssa_lookahead_sensors_envs_f64", 2, (("p", "n_obj", (1 << 28) + 2), ("sp", "n_sensor", 4))),
    ("ssa_forecast_sensors_envs_f64", 2, (("p", "n_obj", (1 << 28) + 2), ("sp", "n_sensor", 4))),
    ("ssa_forecast_sensors_envs_f64", 2, NINE_INLINE + (("p", "n_obj", 7),)),
    # rollout_args, and the network's checks behind it
    ("ssa_env_rollout_f64", 2, (RAGGED, ("r", "spos_tiles", PTR), BAD_PROP)),
    ("ssa_env_rollout_f64", 2, (("p", "n_obj", (1 << 30) + 2), ("r", "spos_tiles", PTR))),
    ("ssa_env_rollout_f64", 2, (RAGGED, ("r", "spos_tiles", PTR), ("p", "status", 0))),
    ("ssa_env_rollout_sensors_envs_f64", 2, (RAGGED, ("r", "spos_tiles", PTR), ("sp", "n_sensor", 0))),
    ("ssa_env_rollout_sensors_envs_f64", 2, (RAGGED, ("re", "stats_out", 0))),
    ("ssa_env_rollout_sensors_envs_f64", 2, (("p", "n_obj", (1 << 30) + 2), ("sp", "n_sensor", 0))),
    ("ssa_env_rollout_sensors_f64", 2, (("sp", "zn_stride_sensor", 0), ("rs", "actions", 0))),
]


def case_id(case):
    entry, n_env, fields = case
    return "%s n_env=%d %s" % (entry, n_env, " ".join("%s.%s=%s" % f for f in fields))


def answer(lib, case):
    entry, n_env, fields = case
    plain = [f for f in fields if f is not NAN]
    return refused(getattr(lib, entry), valid_blocks(entry, n_env), *plain, spoil=nan_mask if NAN in fields else None)


def test_the_mask_bits_are_the_bindings():
    from ssa_gym_amd import _lib
    assert MASK == {k: getattr(_lib, "LAUNCH_" + k) for k in MASK}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a_block_that_breaks_two_rules_gets_the_recorded_code(lib, case):
    from ssa_gym_amd import _lib
    want = json.load(open(TABLE))[case_id(case)]
    got = answer(lib, case)
    assert got in (_lib.E_INVALID, _lib.E_UNSUPPORTED) and got == getattr(_lib, "E_" + want), (case_id(case), got, want)


def test_the_table_holds_exactly_these_cases():
    assert sorted(json.load(open(TABLE))) == sorted(case_id(c) for c in CASES) and len(set(map(case_id, CASES))) == len(CASES)


if __name__ == "__main__":      # (run on a build of the commit whose order is to be recorded)
    from ssa_gym_amd import _lib
    names = {_lib.E_INVALID: "INVALID", _lib.E_UNSUPPORTED: "UNSUPPORTED"}
    json.dump({case_id(c): names[answer(_lib.load(), c)] for c in CASES}, open(TABLE, "w"), indent=0, sort_keys=True)
