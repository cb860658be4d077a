"""How the one-tile step kernels bring a tile in and take it out again: LDS-DMA for a whole tile, registers for a ragged one, the action /
time words and the tile's obj_ids by scalar loads, the whole tile's stores from the state / covariance tiles.  None of this may change a value, so every
comparison is exact: against the rollout of the same schedule, against the grid-stride instance, with a storage layout against without.
Object counts are the smallest at which each path can go wrong: 4 (one whole tile), 5 and 7 (a ragged tile of 1 and 3 rows beside a whole one),
8, 66, 260."""
import numpy as np
import pytest

from support.batches import c2t, make_batch
from support.gpu import hip  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

M_MAX = 260
COUNTS = (4, 5, 7, 8, 66, 260)
NAMES = ("x_true", "x_filter", "P_filter", "obs", "metrics", "status", "upd")
_MASTER = {}


def master():
    """the 260-object problem every case takes its first m objects of (so that 7 objects are the first 7 of 8): a third of the filters
    inflated, so that the ladder, the conic tier and the failure path run and the status words are not all zero"""
    if not _MASTER:
        xt, x, P, g = make_batch(M_MAX, seed=41)
        rs = np.random.RandomState(5)
        P[rs.uniform(size=M_MAX) < 0.33] *= 3e4
        zn = rs.normal(size=(480, M_MAX, 3)) * np.array([4.8e-6, 4.8e-6, 1e3])
        _MASTER.update(xt=xt, x=x, P=P, g=g, zn=zn, order=rs.permutation(M_MAX))
    return _MASTER


def positions(m):
    """storage positions to select, one per step: in the first tile, in the last whole tile, in the ragged tile (none: nobody, action -1)"""
    whole = m // 4
    return [1, 4 * (whole - 1) + 2, (4 * whole + m % 4 - 1) if m % 4 else -1]


def layout_of(m):
    """a non-identity permutation of 0 .. m - 1: position i holds the object the caller calls layout_of(m)[i]"""
    o = master()["order"]
    return o[o < m].copy()


def play(hip, prop, m, pos, E=1, layout=None, delivery="ptr", mirror=None, rollout=False, t0=None, checks=True):
    """len(pos) consecutive steps of E envs x m objects (every env the same problem), the first at time index t0 (default: the last row
    of the time table, so that the second step wraps); step k selects the object at storage position pos[k].  delivery: 'ptr' (the action
    word in memory), 'inline' (action=), 'words' (env_words=); rollout: the same schedule as ONE launch_rollout.  Returns the history
    ring, the status words and the update records as numpy arrays, in storage order, and the same in the caller's order."""
    torch = hip.torch
    M = master()
    consts = hip.host.make_consts(M["g"]["Q"], M["g"]["R"], 1e-4, 2.0, -3, 20.0, -np.pi / 2, M["g"]["obs_lla"], propagator=prop)
    zn = torch.as_tensor(np.ascontiguousarray(M["zn"][:, :m])).cuda()
    eng = hip.engine.HotPathEngine(consts, m, E, c2t(), zn, history=2, zn_stride_env=0)
    if layout is not None:
        eng.set_layout(np.tile(layout, (E, 1)) if E > 1 else layout)
    eng.load_state(0, np.tile(M["xt"][:m], (E, 1)), np.tile(M["x"][:m], (E, 1)), np.tile(M["P"][:m], (E, 1, 1)))
    t0 = eng.n_time - 1 if t0 is None else t0
    acts = [-1 if p < 0 else int(p if layout is None else layout[p]) for p in pos]
    ring = (eng.x_true, eng.x_filter, eng.P_filter, eng.obs, eng.metrics)
    if rollout:
        sched = torch.as_tensor(np.repeat(np.asarray(acts, dtype=np.int32)[:, None], E, axis=1)).cuda().contiguous()
        eng.launch_rollout(0, t0, sched)
    else:
        buf = None
        # (a rollout writes the update records of its last H steps only: the earlier steps' records go to a scratch block here as well, so
        # that the fields a later, shorter record leaves alone hold the same in both rings)
        scratch = torch.zeros(E * hip.lib.UPD_STRIDE, dtype=torch.float64, device="cuda")
        if mirror:
            buf = torch.zeros(E * m * 12, dtype=torch.float32 if mirror == "f32" else torch.float64).pin_memory()
        for k, a in enumerate(acts):
            sin, sout = k % 2, (k + 1) % 2
            before = [r[sin].clone() for r in ring]
            kw = dict(fast_stats=True, defer_fold=True, obs_mirror=buf.data_ptr() if mirror else 0, mirror_f32=mirror == "f32",
                      upd_out=scratch.data_ptr() if k < len(acts) - eng.H else 0)
            if delivery == "inline":
                kw["action"] = a
            elif delivery == "words":
                kw["env_words"] = ([0] * E, [a] * E)
            else:
                eng.set_actions([a] * E)
            eng.launch_step(sin, sout, t0 + k, **kw)
            torch.cuda.synchronize()
            if not checks:
                continue
            for name, r, b in zip(NAMES, ring, before):      # the input slot of the ring: no stray store
                assert torch.equal(r[sin].view(torch.int64), b.view(torch.int64)), (k, name, "input slot changed")
            obs = eng.obs[sout].cpu().numpy()
            rows = np.concatenate([eng.x_filter[sout].cpu().numpy(), np.einsum("jii->ji", eng.P_filter[sout].cpu().numpy())], axis=1)
            assert np.array_equal(obs, rows, equal_nan=True), (k, "obs rows != [x_filter, diag P_filter]")
            if mirror:
                want = obs
                if layout is not None:      # rows at the caller's indices: position i of env e -> row e m + layout[i]
                    want = np.empty_like(obs)
                    for e in range(E):
                        want[e * m + np.asarray(layout)] = obs[e * m:(e + 1) * m]
                got = buf.numpy().reshape(E * m, 12)
                assert np.array_equal(got, want.astype(np.float32) if mirror == "f32" else want, equal_nan=True), (k, "obs_mirror")
        eng.flush_stats()
    torch.cuda.synchronize()
    stored = [r.cpu().numpy().copy() for r in ring] + [eng.status.cpu().numpy().copy(), eng.upd.cpu().numpy().copy()]
    eng.to_caller_order()
    torch.cuda.synchronize()
    caller = [r.cpu().numpy().copy() for r in ring] + [eng.status.cpu().numpy().copy(), eng.upd.cpu().numpy().copy()]
    return stored, caller


def same(a, b, what):
    for name, va, vb in zip(NAMES, a, b):
        assert va.shape == vb.shape and np.array_equal(va, vb, equal_nan=True), (what, name)


# (prop, m) -> how the action reaches the kernel and what the mirror is, rotated so that every form meets every count in one of the propagators
def forms(prop, m):
    i = COUNTS.index(m) + (prop == "fg")
    return ("ptr", "inline", "words")[i % 3], (None, "f64", "f32")[(i + 1) % 3], ("f32", None, "f64")[(i + 1) % 3]


@pytest.mark.parametrize("m", COUNTS)
@pytest.mark.parametrize("prop", ["hybrid", "fg"])
def test_per_step_launches_equal_the_rollout_with_and_without_a_layout(hip, prop, m):
    """Three steps (time indices n_time - 1, n_time -- the wrap --, n_time + 1; history 2), selecting an object of the first tile, of the
    last whole tile and of the ragged tile (or nobody).  Per-step launches -- which check, step by step, the observation rows, the mirror
    and that the input slot is untouched -- against launch_rollout of the same schedule, with a storage layout and without; and the layout
    against no layout in the caller's order."""
    pos = positions(m)
    delivery, mir_plain, mir_layout = forms(prop, m)
    plain, plain_caller = play(hip, prop, m, pos, delivery=delivery, mirror=mir_plain)
    same(plain, play(hip, prop, m, pos, rollout=True)[0], "per-step launches vs rollout")
    lay = layout_of(m)
    assert not np.array_equal(lay, np.arange(m))
    # (the same OBJECTS selected: position p of the plain run is the object the layout stores at position where(lay == p))
    where = [-1 if p < 0 else int(np.nonzero(lay == p)[0][0]) for p in pos]
    stored, caller = play(hip, prop, m, where, layout=lay, delivery=delivery, mirror=mir_layout)
    same(stored, play(hip, prop, m, where, layout=lay, rollout=True)[0], "per-step launches vs rollout, storage layout")
    same(caller, plain_caller, "storage layout vs none, in the caller's order")
    # ... and the layout's own first / last whole / ragged tile selected
    stored, _ = play(hip, prop, m, pos, layout=lay, delivery="ptr", mirror="f64")
    same(stored, play(hip, prop, m, pos, layout=lay, rollout=True)[0], "per-step launches vs rollout, storage layout, its tiles selected")


@pytest.mark.parametrize("prop", ["hybrid", "fg"])
def test_every_action_delivery_gives_the_same_step(hip, prop):
    """the action word in memory, `action=` and `env_words=` (one env) are three routes of the same word into the kernel: 7 objects, a
    whole and a ragged tile, one step each selecting the ragged tile, and one selecting nobody"""
    for pos in ([6], [-1], [1, 5]):
        ref = play(hip, prop, 7, pos, delivery="ptr")[0]
        same(ref, play(hip, prop, 7, pos, delivery="inline", checks=False)[0], ("inline", pos))
        same(ref, play(hip, prop, 7, pos, delivery="words", checks=False)[0], ("words", pos))


@pytest.mark.parametrize("prop", ["hybrid", "fg"])
def test_seven_objects_are_the_first_seven_of_eight(hip, prop):
    """a ragged tile (the register path) against a whole one (LDS-DMA): objects 0 .. 6 of the 7-object run equal objects 0 .. 6 of the
    8-object run"""
    pos = [1, 6, -1]
    a = play(hip, prop, 7, pos, delivery="inline")[0]
    b = play(hip, prop, 8, pos, delivery="inline")[0]
    for name, va, vb in zip(NAMES, a, b):
        if name == "metrics":
            va, vb = va[..., :7], vb[..., :7]
        elif name == "status":
            va, vb = va[:7], vb[:7]
        elif name != "upd":
            va, vb = va[:, :7], vb[:, :7]
        assert np.array_equal(va, vb, equal_nan=True), name


@pytest.mark.parametrize("delivery", ["ptr", "words"])
@pytest.mark.parametrize("prop", ["hybrid", "fg"])
def test_two_envs_take_the_per_lane_path(hip, prop, delivery):
    """2 envs x 8 objects: the action / time words are per-lane loads.  Against the rollout of the same schedule; and with a layout per
    env and a mirror, each env against the same env alone."""
    pos = [1, 6, -1]
    lay = layout_of(8)
    # (the rollout takes several envs in the caller's order only)
    same(play(hip, prop, 8, pos, E=2, delivery=delivery, mirror="f32")[0], play(hip, prop, 8, pos, E=2, rollout=True)[0],
         "two envs: per-step launches vs rollout")
    two = play(hip, prop, 8, pos, E=2, layout=lay, delivery=delivery, mirror="f64")[0]
    one = play(hip, prop, 8, pos, layout=lay, delivery=delivery)[0]
    for name, va, vb in zip(NAMES, two, one):
        for e in range(2):
            if name in ("metrics", "upd"):
                got = va[:, e]
                want = vb[:, 0]
            elif name == "status":
                got, want = va.reshape(2, 8)[e], vb
            else:
                got, want = va.reshape((2, 2, 8) + va.shape[2:])[:, e], vb
            assert np.array_equal(got, want, equal_nan=True), (name, e)


@pytest.mark.parametrize("m", COUNTS)
@pytest.mark.parametrize("prop", ["hybrid", "fg"])
def test_one_tile_instance_equals_the_grid_stride_instance(hip, prop, m):
    """the same env alone (one tile per wavefront) and as every env of a batch of more than 20 480 objects (the grid-stride instance,
    forced by the batch's size): the first, a middle and the last env of the batch equal the env alone, bit for bit"""
    pos = positions(m)
    E = 20481 // m + 1
    big = play(hip, prop, m, pos, E=E, checks=False)[0]
    one = play(hip, prop, m, pos, checks=False)[0]
    for name, va, vb in zip(NAMES, big, one):
        for e in (0, E // 2, E - 1):
            if name in ("metrics", "upd"):
                got, want = va[:, e], vb[:, 0]
            elif name == "status":
                got, want = va.reshape(E, m)[e], vb
            else:
                got, want = va.reshape((2, E, m) + va.shape[2:])[:, e], vb
            assert np.array_equal(got, want, equal_nan=True), (name, e)
