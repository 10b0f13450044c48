"""Grouped allele counts against the calls they replace, on bench.py's workload (chr1-2504 by default), built the way bench.py builds
it (its own functions, imported).  One handle; the legs alternate in one process, each a loop of --steps steps kept --depth deep as
bench.py's loop keeps them, repeated --reps times:

  type6          vs_query_var_in_ref_device (rows + carrier lists: the expansion)
  counts_all     vs_query_allele_counts over the whole cohort
  groups_G       vs_query_group_counts with a random partition of the cohort into G = 2, 5, 26 and 64 groups
  separate_G     G = 2, 5, 26: the G vs_query_allele_counts(regions, group g) calls one grouped call replaces -- a step is all G of them

Prints one JSON line: per leg ms per step (median, min, max over the repeats), regions/s and the median of each batch's own kernel
time (vs_result_fill_ms; separate_G: summed over the step's G calls), and per G the ratio separate / grouped of step and kernel time.

    python tools/bench_groups.py [--steps 20] [--reps 5] [--workload chr1-2504]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # (as bench.py: the plan and the batch run on two streams)

import numpy as np  # noqa: E402

import bench  # noqa: E402
from variantstore_amd import DeviceArray, VariantStore  # noqa: E402

GROUPS = (2, 5, 26, 64)
SEPARATE = (2, 5, 26)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--workload", default="chr1-2504", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--regions", type=int, default=0)
    args = ap.parse_args()
    import torch
    w = bench.WORKLOADS[args.workload]
    nreg = args.regions or w["regions"]
    regions = bench.make_regions(w, 0, nreg)
    t_build = time.perf_counter()
    vs = VariantStore.synthetic(device=0, **bench.synth_kwargs(w))
    t_build = time.perf_counter() - t_build
    ns = vs.info().num_samples - 1
    regions_dev = torch.from_numpy(regions.astype(np.int64)).cuda().contiguous()
    torch.cuda.synchronize()
    dev = DeviceArray(regions_dev.data_ptr(), nreg)
    rng = np.random.default_rng(7)
    members = {}
    for g in GROUPS:   # a random partition of the whole cohort
        label = rng.integers(0, g, size=ns)
        members[g] = [[int(i) + 1 for i in np.nonzero(label == k)[0]] for k in range(g)]

    def grouped(g):
        return lambda: [vs.group_counts(dev, members[g])]

    def separate(g):
        return lambda: [vs.allele_counts(dev, m) for m in members[g]]

    legs = {"type6": lambda: [vs.get_var_in_ref_device(dev.ptr, nreg)], "counts_all": lambda: [vs.allele_counts(dev)]}
    for g in GROUPS:
        legs[f"groups_{g}"] = grouped(g)
        if g in SEPARATE:
            legs[f"separate_{g}"] = separate(g)

    def loop(call, steps):
        alive, fills = [], []

        def retire():
            rs = alive.pop(0)
            fills.append(sum(r.fill_ms() for r in rs))
            for r in rs:
                r.close()

        t0 = time.perf_counter()
        for _ in range(steps):
            alive.append(call())
            if len(alive) >= args.depth:
                retire()
        while alive:
            retire()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps, fills

    for call in legs.values():
        loop(call, args.warmup)
    ms = {k: [] for k in legs}
    fills = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, call in legs.items():
            m, f = loop(call, args.steps)
            ms[k].append(m)
            fills[k] += [x for x in f if x >= 0]
    probe = vs.group_counts(dev, members[2])
    table_rows = probe.layout()[1]
    probe.close()
    out = {"workload": args.workload, "regions_per_step": nreg, "steps": args.steps, "reps": args.reps, "table_rows": table_rows,
           "samples": ns, "build_s": round(t_build, 1), "legs": {}}
    for k in legs:
        med = float(np.median(ms[k]))
        out["legs"][k] = {"ms_per_step_median": round(med, 4), "ms_per_step_min": round(min(ms[k]), 4), "ms_per_step_max": round(max(ms[k]), 4),
                          "regions_per_s": round(nreg / (med / 1e3)), "kernel_ms_median": round(float(np.median(fills[k])), 4) if fills[k] else None}
    out["separate_over_grouped"] = {}
    for g in SEPARATE:
        a, b = out["legs"][f"separate_{g}"], out["legs"][f"groups_{g}"]
        out["separate_over_grouped"][str(g)] = {"step": round(a["ms_per_step_median"] / b["ms_per_step_median"], 3),
                                                "kernel": round(a["kernel_ms_median"] / b["kernel_ms_median"], 3)}
    out["output_bytes"] = {str(g): table_rows * g * 16 for g in GROUPS}
    print(json.dumps(out), flush=True)
    vs.close()


if __name__ == "__main__":
    main()
