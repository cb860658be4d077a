"""kernel time per step from a rocprofv3 kernel trace of rollout_sensors_cost.py (the LAST reps x K dispatches of each kernel family:
the env's own steps to the start state come first).  usage: python profiles/rollout_sensors_reduce.py TRACE_DIR S early|late REPS"""
import csv
import glob
import sys

import numpy as np

d, S, phase, reps, K = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), 63
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))))


def fam(sub, n, per):
    sel = [r for r in rows if sub in r[2]][-n:]
    assert len(sel) == n, (sub, len(sel), n)
    dur = np.array([r[1] - r[0] for r in sel], dtype=float).reshape(-1, per).sum(axis=1) / 1e3
    return dur


a = fam("rollout_sensors_kernel", reps, 1) / K
c = fam("rollout_kernel", reps, 1) / K
b = fam("step_sensors_kernel", reps * K, K) / K
fold = np.array([r[1] - r[0] for r in rows if "rollout_fold_kernel" in r[2]][-2 * reps:], dtype=float) / 1e3
for name, v in (("a rollout_sensors_kernel", a), ("b step_sensors_kernel x63 (fold wavefronts inside)", b), ("c rollout_kernel", c)):
    print("S=%s %-5s kernel time per step [us] %-52s median %7.2f  min %7.2f  max %7.2f" % (S, phase, name, np.median(v), v.min(), v.max()))
print("S=%s %-5s rollout_fold_kernel per launch [us] median %.2f" % (S, phase, np.median(fold)))
