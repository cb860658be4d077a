"""kernel time of the vector dry run from a rocprofv3 kernel trace of `dryrun_sensors_envs_cost.py S early|late REPS kernels`: the
dispatches of dryrun_gather_kernel, dryrun_sensors_kernel and dryrun_totals_kernel grouped by grid size (B = 1 and B = 64 per env).
usage: python profiles/dryrun_sensors_envs_reduce.py TRACE_DIR S early|late|both"""
import collections
import csv
import glob
import sys

import numpy as np

d, S, phase = sys.argv[1], int(sys.argv[2]), sys.argv[3]
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
groups = collections.defaultdict(list)
order = []
for r in sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"])):
    name = r["Kernel_Name"]
    if "dryrun_" not in name:
        continue
    wgs = int(r.get("Grid_Size_X") or r["Grid_Size"]) // max(1, int(r.get("Workgroup_Size_X") or r["Workgroup_Size"]))
    key = (name.split("<")[0].split("(")[0].replace("void ", "").replace("ssa::", ""), wgs)
    if key not in groups:
        order.append(key)
    groups[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
phases = ["early", "late"] if phase == "both" else [phase]
for key in order:      # (in the order they first ran: B = 1, then B = 64; `both`: a grid's first half of dispatches is the early state's)
    n = len(groups[key]) // len(phases)
    for k, ph in enumerate(phases):
        v = np.array(groups[key][k * n:(k + 1) * n])
        print("S=%d %-5s kernel time [us] %-24s %5d workgroups  median %8.2f  min %8.2f  max %8.2f  (%d dispatches)"
              % (S, ph, key[0], key[1], np.median(v), v.min(), v.max(), len(v)))
