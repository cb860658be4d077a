"""Generates tests/golden/episode_failures_reference.json: the failure statistics of the SAME five episodes as
episode_failures_oracle.json (episode_workload.workload(m=2000, seed) for SEEDS; 479 round-robin steps, obs_limit -90 deg, alpha 1e-4),
run by the reference's own callbacks -- fx_xyz_farnocchia, robust_cholesky, hx_aer_erfa, mean_z_uvw, residual_z_aer, loaded by
_ref_loader.py -- driving oracle/ukf_numpy.py, as gen_golden.py::make_filter does: the REFERENCE COMPOSITE.  A filter fails as in
ssa_tasker_simple_2.py:271-285: on any exception, or on NaN in x after predict / update; LinAlgError -> ST_*_LINALG, everything else
(the bare `except:` included: farnocchia.py's AssertionError on a parabola) -> ST_*_NAN.  Per seed, under "reference_composite", the
dictionary episode_workload.run_oracle returns, plus the first-failure exception names.  Filters are independent of each other, so they
run over a process pool (at most 8 workers), one seed at a time; a finished seed is written at once and an interrupted run resumes.
About 5 minutes per seed on 8 cores, under the interpreter that has pyerfa (gen_golden.py's docstring names it).  From the repo root:
    python tests/golden/gen_episode_failures_reference.py
"""
import json
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import episode_workload as ew  # noqa: E402
import oracle as orc  # noqa: E402
import ukf_numpy as U  # noqa: E402

OUT = os.path.join(HERE, "episode_failures_reference.json")
DT, ALPHA = 20.0, 1e-4
_S = {}


def _init(seed):
    import _ref_loader as L
    far = L.load_farnocchia()
    tr, dy = L.load_transformations_and_dynamics()
    _S.update(w=ew.workload(m=2000, seed=seed), fx=far.fx_xyz_farnocchia, dy=dy)


def _fail(f, kind, exc, i):
    f.x = orc.X_FAILED.copy()
    return kind, i, exc


def episode_of_one_filter(j):
    """-> (status, first-failure step or 0, exception name, delta_pos[479], filter mean at DIVERGED_STEP (NaN when failed by then))"""
    w, fx, dy = _S["w"], _S["fx"], _S["dy"]
    g, m = w["g"], w["m"]
    pts = U.MerweScaledSigmaPoints(n=6, alpha=ALPHA, beta=2., kappa=3 - 6, sqrt_method=dy.robust_cholesky)
    f = U.UnscentedKalmanFilter(dim_x=6, dim_z=3, dt=DT, fx=fx, hx=dy.hx_aer_erfa, points=pts, z_mean_fn=dy.mean_z_uvw,
                                residual_z=dy.residual_z_aer, sqrt_fn=dy.robust_cholesky)
    f.x, f.P, f.Q, f.R = w["x"][j].copy(), w["P"][j].copy(), g["Q"].copy(), g["R"].copy()
    xt = w["x_true"][j].copy()
    status, step, exc = orc.ST_OK, 0, None
    dpos = np.empty(ew.N_STEPS)
    x_div = np.full(6, np.nan)
    for i in range(1, ew.N_STEPS + 1):
        xt = fx(xt, DT)
        if status == orc.ST_OK:
            try:
                f.predict()
                if np.any(np.isnan(f.x)):
                    status, step, exc = _fail(f, orc.ST_PREDICT_NAN, "nan", i)
            except np.linalg.LinAlgError:
                status, step, exc = _fail(f, orc.ST_PREDICT_LINALG, "LinAlgError", i)
            except BaseException as e:      # (the env's bare `except:`)
                if isinstance(e, (KeyboardInterrupt, SystemExit)):
                    raise
                status, step, exc = _fail(f, orc.ST_PREDICT_NAN, type(e).__name__, i)
        if (i - 1) % m == j and status == orc.ST_OK:
            kw = dict(trans_matrix=w["c2t"][i], observer_itrs=g["obs_itrs"], observer_lla=g["obs_lla"], time=None)
            z = dy.hx_aer_erfa(xt, **kw)          # (obs_limit -90 deg: always visible)
            try:
                f.update(z + w["z_noise"][i, j], **kw)
                if np.any(np.isnan(f.x)):
                    status, step, exc = _fail(f, orc.ST_UPDATE_NAN, "nan", i)
            except np.linalg.LinAlgError:
                status, step, exc = _fail(f, orc.ST_UPDATE_LINALG, "LinAlgError", i)
            except BaseException as e:
                if isinstance(e, (KeyboardInterrupt, SystemExit)):
                    raise
                status, step, exc = _fail(f, orc.ST_UPDATE_NAN, type(e).__name__, i)
        dpos[i - 1] = np.sqrt(np.sum((f.x[:3] - xt[:3]) ** 2))
        if i == ew.DIVERGED_STEP and status == orc.ST_OK:
            x_div = f.x.copy()
    return status, step, exc, dpos, x_div


def run_seed(seed, workers):
    m = 2000
    with mp.Pool(workers, initializer=_init, initargs=(seed,)) as pool:
        res = pool.map(episode_of_one_filter, range(m), chunksize=10)
    status = np.array([r[0] for r in res], dtype=np.int32)
    first = {j: r[1] for j, r in enumerate(res) if r[0] != orc.ST_OK}
    steps = np.array([r[1] if r[0] != orc.ST_OK else ew.N_STEPS + 1 for r in res])
    n_failed = [int((steps <= i).sum()) for i in range(1, ew.N_STEPS + 1)]
    dpos = np.array([r[3] for r in res])
    max_dpos = [np.nan if np.isnan(dpos[:, k]).any() else float(dpos[:, k].max()) for k in range(ew.N_STEPS)]
    out = ew.summarise(n_failed, status, max_dpos, first)
    out["diverged_at_%d" % ew.DIVERGED_STEP] = ew.diverged_ids(np.array([r[4] for r in res]))
    out["failed_exception"] = [res[j][2] for j in out["failed_ids"]]
    return out


if __name__ == "__main__":
    done = json.load(open(OUT)) if os.path.exists(OUT) else {}
    workers = min(8, os.cpu_count() or 1)
    for seed in ew.SEEDS:
        key = "seed%d" % seed
        if key in done:
            continue
        r = run_seed(seed, workers)
        done[key] = {"reference_composite": r}
        json.dump(done, open(OUT, "w"), indent=1)
        print("seed %d: failed %s, status mix %s, jones step %s, exceptions %s" % (
            seed, r["failed_at"], r["status_mix"], r["jones_done_step"],
            {e: r["failed_exception"].count(e) for e in sorted(set(r["failed_exception"]))}), flush=True)
