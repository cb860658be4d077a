"""kernel time of the dry run and of the forecast from a rocprofv3 kernel trace of `dryrun_sensors_cost.py S early|late REPS kernels`:
the dispatches of dryrun_sensors_kernel grouped by grid size (B = 1, 64, 512 gathered, and the full-catalogue form), those of
forecast_sensors_kernel, and the torch kernels a call brings with it (everything else between the env's last step and the trace's end).
usage: python profiles/dryrun_sensors_reduce.py TRACE_DIR S early|late"""
import collections
import csv
import glob
import sys

import numpy as np

d, S, phase = sys.argv[1], int(sys.argv[2]), sys.argv[3]
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], int(r.get("Grid_Size_X") or r["Grid_Size"]) // max(1, int(r.get("Workgroup_Size_X") or r["Workgroup_Size"])))
               for r in csv.DictReader(open(f))))
first = next(k for k, r in enumerate(rows) if "dryrun_sensors_kernel" in r[2])
groups = collections.defaultdict(list)
for t0, t1, name, wgs in rows:
    if "dryrun_sensors_kernel" in name or "forecast_sensors_kernel" in name:
        groups[(name.split("<")[0].split("(")[0].replace("void ", "").replace("ssa::", ""), wgs)].append((t1 - t0) / 1e3)
for (name, wgs), v in sorted(groups.items()):
    v = np.array(v)
    print("S=%d %-5s kernel time [us] %-26s %5d wavefronts  median %8.2f  min %8.2f  max %8.2f  (%d dispatches)"
          % (S, phase, name, wgs, np.median(v), v.min(), v.max(), len(v)))
other = collections.defaultdict(list)
for t0, t1, name, _ in rows[first:]:
    if "dryrun_sensors_kernel" not in name and "forecast_sensors_kernel" not in name:
        other[name[:60]].append((t1 - t0) / 1e3)
for name, v in sorted(other.items(), key=lambda kv: -sum(kv[1]))[:10]:
    print("S=%d %-5s other kernels from the first dry run on: %-60s %6d dispatches, median %6.2f us, sum %9.1f us" % (S, phase, name, len(v), np.median(v), sum(v)))
