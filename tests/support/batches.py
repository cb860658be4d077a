"""Batches of catalogue states from the goldens, the GCRS -> ITRS table that goes with them, and the error measures of the parity tests."""
import numpy as np

from conftest import golden

C2T = None


def c2t():
    global C2T
    if C2T is None:
        C2T = golden("c2t_2020-05-04_dt20_n480.npy")
    return C2T


def make_batch(m, seed, tight_fraction=0.0):
    rs = np.random.RandomState(seed)
    cat = golden("catalogue_subset.npy")
    g = golden("ukf_step_golden.npz")
    xt = cat[rs.randint(0, len(cat), m)]
    x = xt + rs.normal(size=(m, 6)) * np.array([1e5] * 3 + [1e2] * 3)
    P = np.tile(g["P0"], (m, 1, 1))
    if tight_fraction > 0:
        # posterior-like covariances (after an az/el/range update): sample from the golden posteriors
        k = rs.uniform(size=m) < tight_fraction
        idx = rs.randint(0, 64, m)
        P[k] = 0.5 * (g["Pu_a3"][idx[k]] + np.swapaxes(g["Pu_a3"][idx[k]], 1, 2))
        x[k] = xt[k] + rs.normal(size=(k.sum(), 6)) * np.array([30.0] * 3 + [0.05] * 3)
    return xt, x, P, g


def errs(a, b):
    """per-object relative error of position / velocity blocks and sd-normalised covariance error"""
    ep = np.linalg.norm((a["x"] - b["x"])[:, :3], axis=1) / np.linalg.norm(b["x"][:, :3], axis=1)
    ev = np.linalg.norm((a["x"] - b["x"])[:, 3:], axis=1) / np.linalg.norm(b["x"][:, 3:], axis=1)
    sd = np.sqrt(np.abs(np.einsum('jii->ji', b["P"])))
    eP = np.max(np.abs(a["P"] - b["P"]) / (sd[:, :, None] * sd[:, None, :]), axis=(1, 2))
    return ep, ev, eP


def relnorm(a, b, sl):
    return np.linalg.norm((a - b)[..., sl], axis=-1) / np.linalg.norm(b[..., sl], axis=-1)
