"""The pass table of a sensor network (ssa_access_sensors_f64): its numpy statement -- the oracle's chain of
truths judged by support.illumination.expected_visible / support.orbiting.expected_visible, packed along time and summarised as
include/ssa_hip.h says --, the margins every judged cell must keep, the refusal harness's blocks, and the scenes of the GPU tests:
rows of tests/golden/catalogue_subset.npy under the two test networks, on 16-row tables so that the time index wraps."""
import numpy as np

from support import illumination as il
from support import orbiting as ob
from support.refusals import _fill

EL_MARGIN = 1e-6                    # rad: every judged elevation keeps this distance from its mask (the issue's condition on the inputs)
ACCESS_PTRS = ("x_true_in", "trans", "env_time")


# ---------------------------------------------------------------------------------------------------------------- packing and summary
def pack(acc):
    """access [T, ...] booleans -> bits [..., W] int64, W = ceil(T / 64): bit h mod 64 of word h div 64 is access[h]; bits at h >= T are 0"""
    acc = np.asarray(acc, dtype=bool)
    T = acc.shape[0]
    W = (T + 63) // 64
    out = np.zeros(acc.shape[1:] + (W,), dtype=np.uint64)
    for h in range(T):
        out[..., h >> 6] |= acc[h].astype(np.uint64) << np.uint64(h & 63)
    return out.view(np.int64)


def unpack(bits, T):
    """bits [..., W] int64 -> access [T, ...] booleans"""
    b = np.asarray(bits).view(np.uint64)
    return np.array([(b[..., h >> 6] >> np.uint64(h & 63)) & np.uint64(1) for h in range(T)]).astype(bool)


def summary(acc):
    """access [T, ...] booleans -> int32 [..., 4]: first (smallest h with the bit set, -1: none), length (consecutive set bits from
    first), count (set bits), passes (maximal runs of set bits) -- cell by cell, in plain Python"""
    acc = np.asarray(acc, dtype=bool)
    T = acc.shape[0]
    flat = acc.reshape(T, -1)
    out = np.zeros((flat.shape[1], 4), dtype=np.int32)
    for c in range(flat.shape[1]):
        col = flat[:, c].tolist()
        first = col.index(True) if True in col else -1
        length = 0
        if first >= 0:
            while first + length < T and col[first + length]:
                length += 1
        passes = sum(1 for h in range(T) if col[h] and (h == 0 or not col[h - 1]))
        out[c] = (first, length, sum(col), passes)
    return out.reshape(acc.shape[1:] + (4,))


def cut(acc, n_left):
    """access [T, ...] with every step at or beyond n_left cleared (ssa_access_params.n_left of one env; a value < 0 counts as 0)"""
    acc = np.array(acc, dtype=bool)
    acc[max(0, int(n_left)):] = False
    return acc


# ---------------------------------------------------------------------------------------------------------------- the statement
def truths(oracle, xt, T):
    """[T, m, 6]: the oracle's chain, x_{h+1} = propagate(x_h, DT) (support.illumination.truths)"""
    return np.array(il.truths(oracle, xt, T))


def ground_table(net, oracle, tr, t0, trans, sun, dark):
    """access [T, S, m] of the ground network (support.illumination.Net, sunlit_only = 0b110) along the chain tr [T, m, 6], step h at
    the time row (t0 + h) mod n_time; every judged cell's margins asserted: elevation EL_MARGIN from its mask,
    support.illumination.assert_margins as it stands.  No cell is left out."""
    n_time = len(trans)
    acc = []
    for h in range(len(tr)):
        t = (t0 + h) % n_time
        vis, gap = il.expected_visible(net, oracle, tr[h], trans[t], sun[t], dark[t])
        assert np.all(gap >= EL_MARGIN), (h, gap.min())
        il.assert_margins(tr[h], sun[t])
        acc.append(vis)
    return np.array(acc)


def orbit_table(net, oracle, tr, t0, trans, obs, sun):
    """access [T, S, m] of the network with two moving sensors (support.orbiting.Net) along the chain tr, step h at the time row
    (t0 + h) mod n_time, obs [n_time, 3, 3] the sensors' positions (support.orbiting.table); every judged cell's margins asserted:
    sensor 0's elevation EL_MARGIN from its mask, support.orbiting.assert_margins for sensors 1 and 2 and
    support.illumination.assert_margins as they stand.  No cell is left out."""
    n_time = len(trans)
    acc = []
    for h in range(len(tr)):
        t = (t0 + h) % n_time
        vis, gap = ob.expected_visible(net, oracle, tr[h], trans[t], obs[t], sun[t])
        assert np.all(gap >= EL_MARGIN), (h, gap.min())
        for s in (1, 2):
            ob.assert_margins(tr[h][:, :3], trans[t], obs[t, s])
        il.assert_margins(tr[h], sun[t])
        acc.append(vis)
    return np.array(acc)


# ---------------------------------------------------------------------------------------------------------------- refusals
def valid_blocks(n_env=2):
    """{short name: block} in argument order: blocks ssa_access_sensors_f64 does not refuse -- 8 objects, 2 sensors, n_env envs, 70 steps,
    every output asked for (the pointers are never followed on the host: a refusal comes before any launch)"""
    from ssa_gym_amd import _lib, host
    a = _fill(_lib.ssa_access_params(), ("bits", "pass_", "n_left"), n_steps=70, n_sel=0)
    return {"c": host.make_consts(np.eye(6), np.eye(3), 1e-4, 2.0, -3, 20.0, -np.pi / 2, np.array([0.6, -1.3, 20.0])),
            "p": _fill(_lib.ssa_step_params(), ACCESS_PTRS, n_obj=8, n_env=n_env),
            "sp": _fill(_lib.ssa_sensor_params(), (), n_sensor=2, zn_stride_sensor=384),
            "a": a}


def answer(lib, *fields, n_env=2, null=None, spoil=None):
    """the code ssa_access_sensors_f64 answers its valid blocks with the (block, field, value) fields spoiled"""
    from support.refusals import refused
    return refused(lib.ssa_access_sensors_f64, valid_blocks(n_env), *fields, null=null, spoil=spoil)


# ---------------------------------------------------------------------------------------------------------------- the GPU scenes
N_TIME = il.N_TIME
T_MAX = 70
# rows of tests/golden/catalogue_subset.npy whose every cell keeps every margin over T_MAX steps from the time words 3 and 9, under both
# scenes below (checked with the oracle; the scenes assert it again): the first 147 rows but seven
_NEAR = (33, 46, 52, 79, 88, 125, 138)
ROWS65 = [j for j in range(147) if j not in _NEAR][:65]      # a second wavefront with one live lane
ROWS6 = [0, 6, 12, 16, 8, 48]                                # a partial wavefront; passes that begin and end inside the 70 steps


def catalogue():
    from conftest import golden
    return golden("catalogue_subset.npy")


def _sun_dir():
    """a fixed Sun direction, away from every axis"""
    return il.unit([0.62, -0.41, 0.67])


def ground_scene(oracle, rows, t0, T=T_MAX):
    """the ground network on catalogue rows `rows`: (net, xt [m, 6], sun [16, 3], dark [16], access [T, S, m]); the dark words change
    along the table so that a site's night begins and ends inside every wrap of the index"""
    from support.batches import c2t
    net = il.Net(oracle)
    xt = catalogue()[np.asarray(rows)]
    sun, dark = il.table({t: (None, w) for t, w in enumerate([0b111, 0b111, 0b011, 0b011, 0b101, 0b111, 0b110, 0b111] * 2)}, _sun_dir())
    acc = ground_table(net, oracle, truths(oracle, xt, T), t0, c2t()[:N_TIME], sun, dark)
    return net, xt, sun, dark, acc


def orbit_scene(oracle, rows, t0, T=T_MAX):
    """the network with two moving sensors on catalogue rows `rows`: (net, xt, site rows, sun, dark, access [T, S, m]); the sensors ride
    two circular LEO arcs sampled by the oracle over the 16 rows of the table (an arc the index wraps on: the table is a table)"""
    from support.batches import c2t
    net = ob.Net(oracle)
    xt = catalogue()[np.asarray(rows)]
    trans = c2t()[:N_TIME]
    arcs = {1: ob.leo_arc(lambda x, dt: oracle.propagate(x, dt), ob.leo_state([0.3, 0.9, 0.2], [0.1, -0.2, 0.95])),
            2: ob.leo_arc(lambda x, dt: oracle.propagate(x, dt), ob.leo_state([-0.7, 0.1, 0.65], [0.6, 0.7, 0.3]))}
    site_rows, obs = ob.table(trans, {s: a[:, :3] for s, a in arcs.items()})
    sun, dark = il.table({}, _sun_dir(), default_dark=0)
    acc = orbit_table(net, oracle, truths(oracle, xt, T), t0, trans, obs, sun)
    return net, xt, site_rows, sun, dark, acc
