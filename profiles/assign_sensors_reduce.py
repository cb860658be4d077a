"""kernel time of the assignment alone from a rocprofv3 kernel trace of `assign_sensors_cost.py S early|late REPS kernels` (the script's
last round: 200 assign launches, then 200 * S masked arg-max launches over the S*m*3 scores, then 200 over 20 000 entries).
usage: python profiles/assign_sensors_reduce.py TRACE_DIR S early|late"""
import csv
import glob
import sys

import numpy as np

d, S, phase, n = sys.argv[1], int(sys.argv[2]), sys.argv[3], 200
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))))
asg = np.array([r[1] - r[0] for r in rows if "assign_sensors_kernel" in r[2]][-n:], dtype=float) / 1e3
amax = np.array([r[1] - r[0] for r in rows if "masked_argmax_kernel" in r[2]][-n * (S + 1):], dtype=float) / 1e3
assert len(asg) == n and len(amax) == n * (S + 1), (len(asg), len(amax))
net, one = amax[:n * S].reshape(n, S).sum(axis=1), amax[n * S:]
look = np.array([r[1] - r[0] for r in rows if "lookahead_sensors_kernel" in r[2]][-1:], dtype=float) / 1e3
for name, v in (("assign_sensors_kernel (one launch)", asg), ("masked_argmax_kernel, S launches over S*m*3 entries (sum)", net),
                ("masked_argmax_kernel, one launch over 20000 entries", one), ("lookahead_sensors_kernel (the launch that made the scores)", look)):
    print("S=%d %-5s kernel time [us] %-62s median %7.2f  min %7.2f  max %7.2f  (%d)" % (S, phase, name, np.median(v), v.min(), v.max(), len(v)))
