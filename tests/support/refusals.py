"""The refusal harness of the host tests: per entry one builder of complete, valid argument blocks, and refused(), which spoils the
named fields of such blocks, calls the entry and returns its code.  Nothing is ever launched (the pointers are never dereferenced on
the host: a refusal comes before any launch), so all of this runs without a GPU."""
import collections
import ctypes as C

import numpy as np

PTR = 0x1000
STEP_PTRS = ("x_true_in", "x_true_out", "x_in", "x_out", "P_in", "P_out", "status", "obs", "metrics", "trans", "env_time", "z_noise", "stat_ws")
LOOK_PTRS = ("x_true_in", "x_in", "P_in", "status", "trans", "env_time")
ROLL_PTRS = ("status", "trans", "env_time", "z_noise")
RING_PTRS = ("x_true_ring", "x_ring", "P_ring", "obs_ring", "metrics_ring", "stats_ring", "stat_shards")
OUT_PTRS = ("score", "status", "visible")

# entry -> (the step block's pointers, its other blocks in argument order behind c and p)
ENTRIES = {"ssa_env_step_f64": (STEP_PTRS + ("actions",), ()),
           "ssa_lookahead_f64": (LOOK_PTRS, ("o",)),
           "ssa_env_step_sensors_f64": (STEP_PTRS, ("sp",)),
           "ssa_env_step_sensors_envs_f64": (STEP_PTRS, ("sp", "v")),
           "ssa_lookahead_sensors_f64": (LOOK_PTRS, ("sp", "o")),
           "ssa_lookahead_sensors_envs_f64": (LOOK_PTRS, ("sp", "o")),
           "ssa_forecast_sensors_f64": (LOOK_PTRS, ("sp", "f")),
           "ssa_forecast_sensors_envs_f64": (LOOK_PTRS, ("sp", "f")),
           "ssa_env_rollout_f64": (ROLL_PTRS, ("r",)),
           "ssa_env_rollout_sensors_f64": (ROLL_PTRS, ("r", "sp", "rs")),
           "ssa_env_rollout_sensors_envs_f64": (ROLL_PTRS, ("r", "sp", "re"))}
RAN = collections.Counter()      # the cases refused() ran, per entry


def _fill(blk, names, **values):
    for nm in names:
        setattr(blk, nm, PTR)
    for nm, v in values.items():
        setattr(blk, nm, v)
    return blk


def valid_blocks(entry, n_env=None):
    """{short name: block} in argument order: blocks of `entry` that pass every one of its checks -- 8 objects, 2 sensors, and n_env
    envs (default: 1, a *_envs entry 2)"""
    from ssa_gym_amd import _lib, host
    ptrs, others = ENTRIES[entry]
    if n_env is None:
        n_env = 2 if entry.endswith("_envs_f64") else 1
    make = {"sp": lambda: _fill(_lib.ssa_sensor_params(), (), n_sensor=2, zn_stride_sensor=384),
            "o": lambda: _fill(_lib.ssa_lookahead_out(), OUT_PTRS),
            "f": lambda: _fill(_lib.ssa_forecast_params(), (), n_steps=3),
            "r": lambda: _fill(_lib.ssa_rollout_params(), RING_PTRS + (("actions",) if entry == "ssa_env_rollout_f64" else ()),
                               n_steps=3, history=2, slot_out=1),
            "v": lambda: _fill(_lib.ssa_sensor_envs_params(), ("actions",)),
            "rs": lambda: _fill(_lib.ssa_rollout_sensors_params(), ("actions",)),
            "re": lambda: _fill(_lib.ssa_rollout_sensors_envs_params(), ("actions", "stats_out"))}
    b = {"c": host.make_consts(np.eye(6), np.eye(3), 1e-4, 2.0, -3, 20.0, -np.pi / 2, np.array([0.6, -1.3, 20.0])),
         "p": _fill(_lib.ssa_step_params(), ptrs, n_obj=8, n_env=n_env)}
    for nm in others:
        b[nm] = make[nm]()
    if "f" in b:
        _fill(b["f"].out, OUT_PTRS)
    return b


def nan_mask(b):
    b["sp"].obs_limit[1] = float("nan")


def bad_rk4(b):
    from ssa_gym_amd import _lib
    b["c"].propagator, b["c"].rk4_substeps = _lib.PROP_J2_RK4, 0


def refused(fn, blocks, *fields, null=None, spoil=None):
    """the code `fn` answers blocks with spoiled fields.  blocks: valid_blocks(...) of fn's entry, or None for its default ones;
    fields: (block, field, value) each -- block "o" of a forecast is its f.out; null: the index of an argument passed as NULL;
    spoil: a function that is given the blocks"""
    b = valid_blocks(fn.__name__) if blocks is None else blocks
    for which, name, value in fields:
        setattr(b["f"].out if which == "o" and "f" in b else b[which], name, value)
    if spoil:
        spoil(b)
    args = [C.byref(blk) for blk in b.values()]
    if null is not None:
        args[null] = None
    RAN[fn.__name__] += 1
    return fn(*args, None)
