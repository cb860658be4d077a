"""One launch of the fused env step on the device and the oracle's step from the same inputs: the two runners of the parity tests
(tests/test_hip_step.py, tests/test_unit_weights_gpu.py)."""
import numpy as np

import oracle as orc
from support.batches import c2t


def run_gpu(hip, xt, x, P, g, action, tix, alpha, obs_type='aer', propagator='fg', resample=False,
            obs_limit=-np.pi / 2, E=1, status=None, R=None, z_noise=None, zn_strides=None):
    m = x.shape[0] // E
    R = g["R"] if R is None else R
    consts = hip.host.make_consts(g["Q"], R, alpha, 2.0, -3, 20.0, obs_limit, g["obs_lla"], obs_type=obs_type,
                                  propagator=propagator, resample=resample)
    rs = np.random.RandomState(99)
    if z_noise is None:
        z_noise = rs.normal(size=(E, 480, m, 3)) * np.array([4.8e-6, 4.8e-6, 1e3])
    if zn_strides is None:
        eng = hip.engine.HotPathEngine(consts, m, E, c2t(), z_noise, history=2)
    else:   # (env, time, object) strides of a compact noise table
        eng = hip.engine.HotPathEngine(consts, m, E, c2t(), z_noise, history=2, zn_stride_env=zn_strides[0],
                                       zn_stride_time=zn_strides[1], zn_stride_obj=zn_strides[2])
    eng.load_state(0, xt, x, P)
    if status is not None:
        eng.status.copy_(hip.torch.as_tensor(status))
    eng.set_actions(action)
    eng.launch_step(0, 1, tix)
    hip.torch.cuda.synchronize()
    out = dict(x_true=eng.x_true[1].cpu().numpy(), x=eng.x_filter[1].cpu().numpy(),
               P=eng.P_filter[1].cpu().numpy(), obs=eng.obs[1].cpu().numpy(),
               metrics=eng.metrics[1].cpu().numpy(), status=eng.status.cpu().numpy(),
               upd=eng.upd[1].cpu().numpy(), stats=eng.stats[1].cpu().numpy(), z_noise=z_noise)
    return out


def run_oracle(o, xt, x, P, g, action, tix, alpha, obs_type=0, centred=False, resample=False,
               obs_limit=-np.pi / 2, status=None, R=None, z_noise3=None):
    Wm, Wc, scale = orc.merwe_weights(alpha, 2.0, -3)
    st = np.zeros(x.shape[0], dtype=np.int32) if status is None else status.copy()
    R = g["R"] if R is None else R
    r = o.env_step(xt, x, P, st, 20.0, g["Q"], R, Wm, Wc, scale, action, c2t()[tix], g["obs_lla"], g["obs_itrs"],
                   obs_limit, z_noise3, obs_type=obs_type, centred=centred, resample=resample)
    r["status"] = st
    return r
