"""Genotype-matrix queries against type 6 and the count query on bench.py's workload (chr1-2504 by default), built the way
bench.py builds it (its own functions, imported).  One handle; the legs alternate in one process, each a loop of --steps batches
kept --depth deep as bench.py's loop keeps them, repeated --reps times:

  type6             vs_query_var_in_ref_device (rows + carrier lists: what a caller scatters on the host today)
  matrix_100        vs_query_genotype_matrix over the whole batch and a 100-sample subset
  matrix_1252       ... and a 1,252-sample subset (half the cohort)
  matrix_all_10k    ... over the whole cohort for the first --whole-regions regions of the batch (the whole batch's whole-cohort
                    matrix is about 12.5 GB per step: allowed, but not a leg to time in a loop)
  counts_*          vs_query_allele_counts over the same regions and samples as each matrix leg: the yardstick kernel

Prints one JSON line: ms per step (median, min, max over the repeats), regions/s, the median of each batch's own kernel time
(vs_result_fill_ms: the expansion, the matrix kernel, the count kernel), each matrix's rows, pitch and bytes, and the two ratios
the matrix kernel is held against: its bytes at the streaming ceiling (--ceiling-tbps, or what tools/microbench/hbm_ceiling
--quick reports on this box for its store-heavy mix, as bench.py runs it) over its kernel time, and its kernel time over the
count kernel's.
--tile sets option matrix_tile_cols.

    python tools/bench_genotypes.py [--steps 10] [--reps 3] [--workload chr1-2504] [--tile 0]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--workload", default="chr1-2504", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--regions", type=int, default=0)
    ap.add_argument("--whole-regions", type=int, default=10_000)
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--ceiling-tbps", type=float, default=0.0, help="0: measure with tools/microbench/hbm_ceiling, 6.4 when it is not built")
    args = ap.parse_args()
    box = None if args.ceiling_tbps else bench.box_ceilings()   # (a child process, before this one touches the GPU)
    ceiling = args.ceiling_tbps or (box["mix_2to3_GBps"] / 1e3 if box and box.get("mix_2to3_GBps") else 0.0)
    ceiling_from = "argument" if args.ceiling_tbps else "hbm_ceiling --quick: mix_2to3" if ceiling else "assumed"
    ceiling = ceiling or 6.4
    import torch
    w = bench.WORKLOADS[args.workload]
    nreg = args.regions or w["regions"]
    regions = bench.make_regions(w, 0, nreg)
    t_build = time.perf_counter()
    vs = VariantStore.synthetic(device=0, **bench.synth_kwargs(w))
    t_build = time.perf_counter() - t_build
    if args.tile:
        vs.set_option("matrix_tile_cols", args.tile)
    ns = vs.info().num_samples - 1
    regions_dev = torch.from_numpy(regions.astype(np.int64)).cuda().contiguous()
    torch.cuda.synchronize()
    ptr = regions_dev.data_ptr()
    rng = np.random.default_rng(7)
    sub100 = [int(i) for i in np.sort(rng.choice(np.arange(1, ns + 1), size=min(100, ns), replace=False))]
    sub_half = [int(i) for i in np.sort(rng.choice(np.arange(1, ns + 1), size=ns // 2, replace=False))]
    dev = DeviceArray(ptr, nreg)
    n_whole = min(args.whole_regions, nreg)
    dev_whole = DeviceArray(ptr, n_whole)
    k_half, k_whole = f"{len(sub_half)}", f"all_{n_whole // 1000}k"
    legs = {
        "type6": (lambda: vs.get_var_in_ref_device(ptr, nreg), nreg),
        "matrix_100": (lambda: vs.genotype_matrix(dev, sub100), nreg),
        "counts_100": (lambda: vs.allele_counts(dev, sub100), nreg),
        "matrix_" + k_half: (lambda: vs.genotype_matrix(dev, sub_half), nreg),
        "counts_" + k_half: (lambda: vs.allele_counts(dev, sub_half), nreg),
        "matrix_" + k_whole: (lambda: vs.genotype_matrix(dev_whole), n_whole),
        "counts_" + k_whole: (lambda: vs.allele_counts(dev_whole), n_whole),
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

    for call, _n in legs.values():
        loop(call, args.warmup)
    ms = {k: [] for k in legs}
    fills = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, (call, _n) in legs.items():
            m, f = loop(call, args.steps)
            ms[k].append(m)
            fills[k] += [x for x in f if x >= 0]
    out = {"workload": args.workload, "regions_per_step": nreg, "steps": args.steps, "reps": args.reps,
           "matrix_tile_cols": args.tile or "default", "ceiling_tbps": ceiling, "ceiling_from": ceiling_from, "box_ceilings": box, "build_s": round(t_build, 1), "legs": {}}
    for k, (call, n) in legs.items():
        med = float(np.median(ms[k]))
        leg = {"ms_per_step_median": round(med, 4), "ms_per_step_min": round(min(ms[k]), 4), "ms_per_step_max": round(max(ms[k]), 4),
               "regions": n, "regions_per_s": round(n / (med / 1e3)), "kernel_ms_median": round(float(np.median(fills[k])), 4) if fills[k] else None}
        if k.startswith("matrix_"):
            one = call()
            _ptr, rows, cols, pitch = one.genotype_matrix_device()
            leg.update(rows=rows, columns=cols, row_pitch=pitch, matrix_bytes=rows * pitch, nonzero_cells=one.totals()[2])
            one.close()
            leg["store_floor_ms"] = round(leg["matrix_bytes"] / (ceiling * 1e12) * 1e3, 4)
            if leg["kernel_ms_median"]:
                leg["store_floor_frac_of_kernel"] = round(leg["store_floor_ms"] / leg["kernel_ms_median"], 4)
        out["legs"][k] = leg
    for k, leg in out["legs"].items():
        if k.startswith("matrix_"):
            c = out["legs"]["counts_" + k[len("matrix_"):]]["kernel_ms_median"]
            if c and leg["kernel_ms_median"]:
                leg["kernel_vs_count_kernel"] = round(leg["kernel_ms_median"] / c, 3)
    t6 = out["legs"]["type6"]["ms_per_step_median"]
    out["step_vs_type6"] = {k: round(v["ms_per_step_median"] / t6, 3) for k, v in out["legs"].items() if v["regions"] == nreg and k != "type6"}
    print(json.dumps(out), flush=True)
    vs.close()


if __name__ == "__main__":
    main()
