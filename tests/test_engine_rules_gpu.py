"""The engine's sensor launches on a stream of the caller's, on the MI355X: the lookahead, both assignment rules, the forecast, the plan
and a rollout of the plan given a side torch.cuda.Stream as `stream=` leave, bit for bit, what a twin engine with the same state leaves
that does the same on torch's current stream -- through the device.* functions where one exists, which the engine's launches hand their
arguments to.  The two paths run the same kernels on the same inputs: no tolerance."""
import numpy as np
import pytest

from support.gpu import hip  # noqa: F401  (the module fixture)
from support.vector_lookahead import Engines

pytestmark = pytest.mark.gpu

S, HP, HIST = 2, 2, 4      # sensors (below MAX_SENSORS: the -1 padding matters), steps of the forecast and the plan, history depth


def _run(hip, X, stream, through_device):
    """the sequence on X's engine; stream: the side stream handed to every launch, or None (torch's current stream).  Returns what it left,
    by name.  The sequence runs twice from the same state and the second pass counts: the first one, always in the current stream,
    allocates the engine's cached buffers and zeroed workspaces -- torch fills those in ITS current stream whatever stream a launch
    goes to, so a first launch elsewhere would not be ordered behind the fill."""
    torch, L, dev = hip.torch, hip.lib, hip.dev
    e, one, W = X.vec, X.E == 1, hip.lib.MAX_SENSORS
    lead = () if one else (X.E,)
    col = L.LOOK_INFO_GAIN
    fb = torch.as_tensor(np.arange(int(np.prod(lead + (W,)))).reshape(lead + (W,)) % X.m, dtype=torch.int32).cuda()
    picks = {r: torch.zeros(lead + (W, 2), dtype=torch.int64, device="cuda") for r in ("greedy", "optimal")}
    plan_picks = torch.zeros((HP,) + lead + (W, 2), dtype=torch.int64, device="cuda")
    rows = {r: torch.full((W,), -7, dtype=torch.int32, device="cuda") for r in picks}
    got = {}

    def keep(name, t):
        """wait for the stream the launches went to -- and for nothing else -- then read"""
        (torch.cuda.current_stream() if where is None else where).synchronize()
        a = t.cpu().numpy()
        got[name] = a.view(np.int64).copy() if a.dtype == np.float64 else a.copy()

    for where in (None, stream):
        e.load_state(0, X.xt, X.x, X.P)
        e.env_time0.copy_(torch.as_tensor(X.t0, dtype=torch.int32))
        torch.cuda.synchronize()
        got.clear()
        look = (e.launch_lookahead_sensors if one else e.launch_lookahead_sensors_envs)(0, 1, X.sp, out=("P_post",), stream=where)
        keep("look score", look["score"])
        keep("look P_post", look["P_post"])
        for rule in ("greedy", "optimal"):
            if through_device:
                table = (dev.assign_sensors if one else dev.assign_sensors_envs)(look["score"], col, fallback=fb, picks=picks[rule], rule=rule)
            elif one:
                e.launch_assign_sensors(look, col, rows[rule], fallback_row=fb, picks=picks[rule], stream=where, rule=rule)
                table = rows[rule]
            else:
                table = e.launch_assign_sensors_envs(look, col, fallback=fb, picks=picks[rule], stream=where, rule=rule)
            keep(rule + " table", table)
            keep(rule + " picks", picks[rule])
        fore = (e.launch_forecast_sensors if one else e.launch_forecast_sensors_envs)(0, 1, X.sp, HP, stream=where)
        keep("forecast score", fore["score"])
        if through_device:
            plan = dev.plan_sensors(fore["score"], col, picks=plan_picks)
        else:
            plan = e.launch_plan_sensors(fore, col, picks=plan_picks, stream=where)
        keep("plan table", plan)
        keep("plan picks", plan_picks)
        (e.launch_rollout_sensors if one else e.launch_rollout_sensors_envs)(0, 1, X.sp, plan, stream=where)
        keep("P_filter", e.P_filter[HP % HIST])
        keep("x_filter", e.x_filter[HP % HIST])
    return got


@pytest.mark.parametrize("E,m", [(1, 6), (2, 8)], ids=["one_env_ragged_tile", "two_envs"])
def test_launches_on_a_side_stream_equal_the_device_functions_on_the_current_one(hip, E, m):
    torch, L = hip.torch, hip.lib
    a, b = Engines(hip, E, m, S, history=HIST), Engines(hip, E, m, S, history=HIST)
    side = torch.cuda.Stream()
    got = _run(hip, a, side, False)
    want = _run(hip, b, None, True)
    assert sorted(got) == sorted(want) and len(got) == 11
    for name in want:
        assert got[name].shape == want[name].shape and np.array_equal(got[name], want[name]), name
    # the launches did something: sensors tasked, padding beyond S, the rollout's slot written
    lead = () if E == 1 else (E,)
    assert got["plan table"].shape == (HP,) + lead + (L.MAX_SENSORS,)
    assert (got["plan table"][..., S:] == -1).all() and (got["plan table"][..., :S] >= 0).any()
    assert (got["greedy table"][..., S:] == -1).all() and (got["optimal table"][..., S:] == -1).all()
    assert got["P_filter"].any()
    # a raw handle is a stream too: the same lookahead through the side stream's handle
    look = (a.vec.launch_lookahead_sensors if E == 1 else a.vec.launch_lookahead_sensors_envs)(HP % HIST, 1 + HP, a.sp, stream=side.cuda_stream)
    side.synchronize()
    ref = (b.vec.launch_lookahead_sensors if E == 1 else b.vec.launch_lookahead_sensors_envs)(HP % HIST, 1 + HP, b.sp)
    torch.cuda.synchronize()
    assert torch.equal(look["score"].view(torch.int64), ref["score"].view(torch.int64))


def test_plan_refuses_more_slots_than_the_cap_on_the_device(hip):
    """MAX_PLAN_SLOTS through the engine: reached only with a forecast's CUDA scores (the host table of refusals has no row for it)"""
    torch, L = hip.torch, hip.lib
    X = Engines(hip, 1, 6, S, history=HIST)
    steps = L.MAX_PLAN_SLOTS // S + 1
    with pytest.raises(ValueError, match="SSA_MAX_PLAN_SLOTS"):
        X.vec.launch_plan_sensors({"score": torch.zeros((steps, S, 6, L.LOOK_NSCORE), dtype=torch.float64, device="cuda")}, L.LOOK_INFO_GAIN)
