"""time of the catalogue screen kernels: batches of 4 096 and 27 000 candidates at T = 96.
usage (from the repository root):
  python profiles/screen_network_cost.py run [launches]
      per batch size, `launches` (default 110; the first 10 are warm-up) launches each of
        old   ssa_catalogue_screen_f64, the S = 3 scene's site table read as three ground sites (the orbiting sensor's row: (0, 0, 0), mask 0)
        zero  ssa_catalogue_screen_network_f64 with site_moving == sunlit_only == 0 on the same inputs
        s3    the S = 3 scene: ground radar, ground telescope with a night limit, LEO 'sunlit' sensor
        s8m   S = 8, four sensors moving and four sunlit-only (two of them both)
        old2  `old` once more: with the first, the old entry's own run-to-run spread inside the session
      every launch between two events of its own.  Quoted: median, minimum and the two half-medians in microseconds of device time
      between the events -- a launch's own overhead included.
  python profiles/screen_network_cost.py reduce TRACE_DIR [launches]
      the kernels' own time of such a run made under `rocprofv3 --kernel-trace --output-format csv -d TRACE_DIR -- python
      profiles/screen_network_cost.py run [launches]`: the screen kernels' dispatches in order, cut into the run's groups, the same
      four figures (End_Timestamp - Start_Timestamp: no launch overhead), and zero / old per batch size.
  python profiles/screen_network_cost.py draw
      wall clock of visible_catalogue(20000, seed=0) against visible_catalogue_network(20000, seed=0) at the default site, and of
      the S = 3 scene's draw, with the number of candidates each screened."""
import sys
import time

import numpy as np

BATCHES, MODES, WARM = (4096, 27000), ("old", "zero", "s3", "s8m", "old2"), 10


def figures(t):
    half = len(t) // 2
    return "median %8.2f us  min %8.2f  halves %8.2f / %8.2f  (%d)" % (np.median(t), t.min(), np.median(t[:half]), np.median(t[half:]), len(t))


if sys.argv[1] == "reduce":
    import csv
    import glob
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 110
    f = glob.glob(sys.argv[2] + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f)))
    rows = [(b - a) * 1e-3 for a, b, name in rows if "catalogue_screen" in name]
    assert len(rows) == n * len(BATCHES) * len(MODES), len(rows)
    med = {}
    for g, (batch, mode) in enumerate((b, m) for b in BATCHES for m in MODES):
        t = np.array(rows[g * n:(g + 1) * n][WARM:])
        med[batch, mode] = np.median(t)
        print("kernel %6d %-5s %s" % (batch, mode, figures(t)))
    for batch in BATCHES:
        print("%6d: zero / old %.4f   old2 / old %.4f   s3 / old %.4f   s8m / old %.4f" % (
            batch, med[batch, "zero"] / med[batch, "old"], med[batch, "old2"] / med[batch, "old"], med[batch, "s3"] / med[batch, "old"],
            med[batch, "s8m"] / med[batch, "old"]))
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import ssa_gym_amd  # noqa: E402,F401
from ssa_gym_amd import catalogue, device  # noqa: E402
from support import screen_network as sn  # noqa: E402

if sys.argv[1] == "draw":
    counts = []
    for name in ("catalogue_screen", "catalogue_screen_network"):
        def counted(elements, *a, _f=getattr(device, name), **kw):
            counts[-1] += elements.shape[0]
            return _f(elements, *a, **kw)
        setattr(device, name, counted)
    sc = sn.scene('S3', 96)
    runs = (("visible_catalogue(20000, seed=0)", lambda: catalogue.visible_catalogue(20000, seed=0)),
            ("visible_catalogue_network(20000, seed=0), default site", lambda: catalogue.visible_catalogue_network(20000, seed=0, sensors=[catalogue.DEFAULT_SITE])),
            ("visible_catalogue_network(20000, seed=0), S = 3 scene", lambda: catalogue.visible_catalogue_network(
                20000, seed=0, sensors=sc['sensors'], el_min_deg=sc['el_min_deg'], illumination=sc['illumination'], t_0=sn.T_0, step=sn.STEP)))
    for rep in range(3):
        for label, fn in runs:
            counts.append(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            print("run %d  %-58s %.3f s  %8d candidates screened" % (rep, label, time.perf_counter() - t0, counts[-1]))
    sys.exit(0)

n = int(sys.argv[2]) if len(sys.argv) > 2 else 110
for batch in BATCHES:
    el = device.as_dev(np.stack(sn.candidates(batch), axis=1))
    for mode in MODES:
        sc = sn.scene('S8m' if mode == "s8m" else 'S3', 96)
        trans, tab = device.as_dev(sc['M_t']), device.as_dev(sc['tab'])
        kw = {k: (device.as_dev(v) if isinstance(v, np.ndarray) else v) for k, v in sn.device_kw(sc).items()}
        if mode in ("old", "old2"):
            def launch():
                return device.catalogue_screen(el, trans, tab, sc['step'], 300e3, sc['first'], sc['max_gap'])
        elif mode == "zero":
            def launch():
                return device.catalogue_screen_network(el, trans, tab, sc['step'], 300e3, sc['first'], sc['max_gap'])
        else:
            def launch():
                return device.catalogue_screen_network(el, trans, tab, sc['step'], 300e3, sc['first'], sc['max_gap'], **kw)
        out = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            acc = launch()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) * 1e3)
        print("events %6d %-5s %s  accepted %d" % (batch, mode, figures(np.array(out[WARM:])), int(acc.sum())))
