"""kernel time of the two assignment kernels from a rocprofv3 kernel trace of `match_sensors_cost.py S early|late REPS kernels` (the
script's last round: 200 assign_sensors_kernel launches, then 200 match_sensors_kernel launches, on the same scores).
usage: python profiles/match_sensors_reduce.py TRACE_DIR S early|late"""
import csv
import glob
import sys

import numpy as np

d, S, phase, n = sys.argv[1], int(sys.argv[2]), sys.argv[3], 200
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))))
asg = np.array([r[1] - r[0] for r in rows if "assign_sensors_kernel" in r[2]][-n:], dtype=float) / 1e3
mat = np.array([r[1] - r[0] for r in rows if "match_sensors_kernel" in r[2]][-n:], dtype=float) / 1e3
assert len(asg) == n and len(mat) == n, (len(asg), len(mat))
for name, v in (("assign_sensors_kernel", asg), ("match_sensors_kernel", mat)):
    print("S=%d %-5s kernel time [us] %-24s median %7.2f  min %7.2f  max %7.2f  (%d)" % (S, phase, name, np.median(v), v.min(), v.max(), len(v)))
print("S=%d %-5s match / assign (kernel time): %.2f" % (S, phase, np.median(mat) / np.median(asg)))
