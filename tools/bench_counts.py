"""Allele-count queries against type 6 on bench.py's workload (chr1-2504 by default), built the way bench.py builds it (its own
functions, imported).  One handle; the four legs alternate in one process, each a loop of --steps batches kept --depth deep as
bench.py's loop keeps them, repeated --reps times:

  type6        vs_query_var_in_ref_device (rows + carrier lists: the expansion)
  counts_all   vs_query_allele_counts over the whole cohort
  counts_100   ... over a 100-sample subset
  counts_1252  ... over a 1,252-sample subset (half the cohort)

Prints one JSON line: ms per step (median, min, max over the repeats), regions/s, the median of each batch's own kernel time
(vs_result_fill_ms: the expansion, or the counting kernel), and the count path's algorithmic bytes for the batch (computed below
from its sizes) with the fraction of the 8 TB/s HBM spec they are of the whole-cohort step and kernel.

    python tools/bench_counts.py [--steps 20] [--reps 5] [--workload chr1-2504]
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


def count_path_bytes(vs, counts, table_rows):
    """What the whole-cohort count step must move, from the batch's sizes: k_share_rows2 reads the 32-byte site row and writes the
    32-byte table row and the row's site (4), k_allele_counts reads the site (4) and its parameters (count 4, class 4, genotype offset
    8), the genotype words of the row's carriers (4 bytes per 8 carriers) and writes 16 bytes of counts."""
    gt_words = int(((counts["carriers"].astype(np.int64) + 7) // 8).sum())
    rows = table_rows * (32 + 32 + 4) + table_rows * (4 + 4 + 4 + 8) + table_rows * 16
    return {"rows_bytes": rows, "genotype_bytes": gt_words * 4, "total_bytes": rows + gt_words * 4}


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
    ptr = regions_dev.data_ptr()
    rng = np.random.default_rng(7)
    sub100 = [int(i) for i in np.sort(rng.choice(np.arange(1, ns + 1), size=min(100, ns), replace=False))]
    sub_half = [int(i) for i in np.sort(rng.choice(np.arange(1, ns + 1), size=ns // 2, replace=False))]
    legs = {
        "type6": lambda: vs.get_var_in_ref_device(ptr, nreg),
        "counts_all": lambda: vs.allele_counts(DeviceArray(ptr, nreg)),
        "counts_100": lambda: vs.allele_counts(DeviceArray(ptr, nreg), sub100),
        f"counts_{len(sub_half)}": lambda: vs.allele_counts(DeviceArray(ptr, nreg), sub_half),
    }

    def loop(call, steps):
        alive, fills = [], []
        t0 = time.perf_counter()
        for _ in range(steps):
            alive.append(call())
            if len(alive) >= args.depth:
                r = alive.pop(0)
                fills.append(r.fill_ms())
                r.close()
        while alive:
            r = alive.pop(0)
            fills.append(r.fill_ms())
            r.close()
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
    whole = vs.allele_counts(regions)
    table_rows = whole.layout()[1]
    traffic = count_path_bytes(vs, whole.allele_counts()["counts"], table_rows)
    whole.close()
    out = {"workload": args.workload, "regions_per_step": nreg, "steps": args.steps, "reps": args.reps, "table_rows": table_rows,
           "build_s": round(t_build, 1), "legs": {}}
    for k in legs:
        med = float(np.median(ms[k]))
        out["legs"][k] = {"ms_per_step_median": round(med, 4), "ms_per_step_min": round(min(ms[k]), 4), "ms_per_step_max": round(max(ms[k]), 4),
                          "regions_per_s": round(nreg / (med / 1e3)), "kernel_ms_median": round(float(np.median(fills[k])), 4) if fills[k] else None}
    ca = out["legs"]["counts_all"]
    out["count_path_bytes"] = traffic
    out["count_step_frac_of_8TBps"] = round(traffic["total_bytes"] / (ca["ms_per_step_median"] / 1e3) / 8e12, 4)
    if ca["kernel_ms_median"]:
        kb = traffic["genotype_bytes"] + table_rows * (4 + 4 + 4 + 8 + 16)
        out["count_kernel_bytes"] = kb
        out["count_kernel_frac_of_8TBps"] = round(kb / (ca["kernel_ms_median"] / 1e3) / 8e12, 4)
    t6 = out["legs"]["type6"]["ms_per_step_median"]
    out["speedup_vs_type6"] = {k: round(t6 / v["ms_per_step_median"], 3) for k, v in out["legs"].items() if k != "type6"}
    print(json.dumps(out), flush=True)
    vs.close()


if __name__ == "__main__":
    main()
