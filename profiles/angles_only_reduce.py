"""kernel time of step_sensors_kernel and lookahead_sensors_kernel from a rocprofv3 kernel trace of profiles/angles_only_cost.py: the
last `launches` dispatches of each (the cost script's own; the env's five steps and the first lookahead come before them).
usage: python profiles/angles_only_reduce.py TRACE_DIR LABEL [launches]"""
import csv
import glob
import sys

import numpy as np

d, label, n = sys.argv[1], sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 40
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f)))
for name in ("step_sensors_kernel", "lookahead_sensors_kernel"):
    v = np.array([(t1 - t0) / 1e3 for t0, t1, k in rows if name in k and "envs" not in k][-n:])
    print("%-22s kernel time [us] %-26s median %8.2f  min %8.2f  max %8.2f  (%d dispatches)" % (label, name, np.median(v), v.min(), v.max(), len(v)))
