"""Workload for the rocprofv3 counter passes over the PLAIN step instance (ssa::step_plain_kernel), and their reduction.

The workload steps exactly as bench.py's headline does -- HipLocalStepper(fast_stats=True, defer_fold=True), the regime storage layout,
whole episodes of 479 steps with device-side resets -- so every launch takes the plain form.  (profiles/pmc_workload.py steps without
the deferred fold, a form outside the plain one: its passes run the generic instance.)

One counter pass per run, alone with the kernel trace -- never next to any other tracing:

    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_LDS SQ_INSTS_VMEM_WR SQ_INSTS_VMEM_RD SQ_WAVES \
              --kernel-trace --output-format csv -d OUT/insts -- python3 profiles/pmc_plain_workload.py
    python3 profiles/pmc_plain_workload.py --reduce OUT/insts          (several passes: one directory each)

--reduce prints, per counter, the mean per launch and per wavefront of the plain instance's launches (the compute wavefronts: one per
four objects; a launch also carries the 32 service wavefronts that fold the previous step's statistics), and fails if a pass saw a
step launch of another instance.  Environment: M (objects, default 20 000), PROP (default hybrid), EPISODES (default 1)."""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reduce(dirs, m):
    out = {"kernel": None, "workload": "%d objects = %d compute wavefronts per launch, profiles/pmc_plain_workload.py" % (m, (m + 3) // 4),
           "counters": {}}
    for d in dirs:
        fs = glob.glob(os.path.join(d, '**', '*counter_collection.csv'), recursive=True)
        if not fs:
            out["counters"][os.path.basename(d)] = "pass produced no counter file (counter not available on this build?)"
            continue
        acc = {}
        for r in csv.DictReader(open(fs[0])):
            if 'step_fast_kernel' in r['Kernel_Name']:
                raise SystemExit("%s: a launch of the generic instance (%s): the workload left the plain form" % (d, r['Kernel_Name'][:60]))
            if 'step_plain_kernel' not in r['Kernel_Name']:
                continue
            if out["kernel"] is None:
                out["kernel"] = r['Kernel_Name'].split('(')[0]
            acc.setdefault(r['Counter_Name'], []).append(float(r['Counter_Value']))
        for k, v in acc.items():
            v = v[20:] if len(v) > 40 else v      # (the first launches: code-object load, cold caches)
            out["counters"][k] = {"mean_per_launch": sum(v) / len(v), "per_wavefront": sum(v) / len(v) / ((m + 3) // 4), "launches": len(v)}
    print(json.dumps(out, indent=1))


def workload(m, episodes, propagator):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.argv = ['bench.py']
    import bench
    from ssa_gym_amd import engine, host, parallel
    from ssa_gym_amd.catalogue import regime_order
    pb = bench.build_problem(m, seed=100)
    consts = host.make_consts(pb["Q"], pb["R"], 1e-4, 2.0, -3, 20.0, -np.pi / 2, pb["obs_lla"], obs_type='aer', propagator=propagator)
    gen = torch.Generator(device="cuda").manual_seed(1)
    zn = torch.randn((1, 480, m, 3), dtype=torch.float64, device="cuda", generator=gen) * torch.as_tensor(pb["z_sigma"], device="cuda")
    eng = engine.HotPathEngine(consts, m, 1, pb["trans"], zn, history=2)
    eng.set_layout(regime_order(pb["x_true"]))
    eng.load_state(0, pb["x_true"], pb["x"], np.broadcast_to(pb["P0"], (m, 6, 6)))
    local = parallel.HipLocalStepper(eng, consts, fast_stats=True, defer_fold=True)
    local.load_schedule(list(np.arange(479) % m))
    snap = eng.snapshot(0)
    for ep in range(episodes):
        if ep:
            local.reset_episode(snap, 480)
        for _ in range(479):
            local.step(-1)
    local.flush()
    torch.cuda.synchronize()


if __name__ == "__main__":
    M = int(os.environ.get('M', '20000'))
    if len(sys.argv) > 1 and sys.argv[1] == "--reduce":
        reduce(sys.argv[2:], M)
    else:
        workload(M, int(os.environ.get('EPISODES', '1')), os.environ.get('PROP', 'hybrid'))
