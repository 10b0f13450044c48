"""Burden queries against type 6 on bench.py's workload (chr1-2504 by default), built the way bench.py builds it (its own
functions, imported).  One handle; the legs alternate in one process, each a loop of --steps batches kept --depth deep as
bench.py's loop keeps them, repeated --reps times:

  type6             vs_query_var_in_ref_device (rows + carrier lists: the expansion every route to this matrix takes today)
  burden_all        vs_query_sample_burden over the whole cohort
  burden_100        ... over a 100-sample subset
  burden_1252       ... over a 1,252-sample subset (half the cohort)
  burden_all_ac25   ... over the whole cohort, rows of at most 25 alternate alleles (about 0.5 % AF: the rare-variant use)

Prints one JSON line: ms per step (median, min, max over the repeats), regions/s, the median of each batch's own kernel time
(vs_result_fill_ms: the expansion, or the burden kernels with the window's count kernel), the bytes each leg's matrix stores and
the fraction of the streaming ceiling (--ceiling-tbps, what tools/microbench/hbm_ceiling reads) that store alone is of the
kernel time.  --chunk sets option burden_chunk (rows per workgroup before a region is split); --long adds a leg of 64 regions of
--long-kb each, all of them split, for sizing the chunk.

    python tools/bench_burden.py [--steps 10] [--reps 3] [--workload chr1-2504] [--chunk 0]
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
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--long", type=int, default=0, help="add a leg of this many regions of --long-kb each (split regions)")
    ap.add_argument("--long-kb", type=int, default=2_000)
    ap.add_argument("--ceiling-tbps", type=float, default=6.4)
    args = ap.parse_args()
    import torch
    w = bench.WORKLOADS[args.workload]
    nreg = args.regions or w["regions"]
    regions = bench.make_regions(w, 0, nreg)
    t_build = time.perf_counter()
    vs = VariantStore.synthetic(device=0, **bench.synth_kwargs(w))
    t_build = time.perf_counter() - t_build
    if args.chunk:
        vs.set_option("burden_chunk", args.chunk)
    ns = vs.info().num_samples - 1
    regions_dev = torch.from_numpy(regions.astype(np.int64)).cuda().contiguous()
    torch.cuda.synchronize()
    ptr = regions_dev.data_ptr()
    rng = np.random.default_rng(7)
    sub100 = [int(i) for i in np.sort(rng.choice(np.arange(1, ns + 1), size=min(100, ns), replace=False))]
    sub_half = [int(i) for i in np.sort(rng.choice(np.arange(1, ns + 1), size=ns // 2, replace=False))]
    dev = DeviceArray(ptr, nreg)
    legs = {
        "type6": (lambda: vs.get_var_in_ref_device(ptr, nreg), 0, nreg),
        "burden_all": (lambda: vs.sample_burden(dev), ns, nreg),
        "burden_100": (lambda: vs.sample_burden(dev, sub100), len(sub100), nreg),
        f"burden_{len(sub_half)}": (lambda: vs.sample_burden(dev, sub_half), len(sub_half), nreg),
        "burden_all_ac25": (lambda: vs.sample_burden(dev, None, 0, 25), ns, nreg),
    }
    if args.long:
        L = vs.info().ref_length
        span = args.long_kb * 1_000
        starts = np.sort(rng.integers(1, max(2, L - span), size=args.long)).astype(np.uint64)
        long_regions = np.stack([starts, starts + np.uint64(span)], axis=1)
        legs["burden_all_long"] = (lambda: vs.sample_burden(long_regions), ns, args.long)

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

    for call, _c, _n in legs.values():
        loop(call, args.warmup)
    ms = {k: [] for k in legs}
    fills = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, (call, _c, _n) in legs.items():
            m, f = loop(call, args.steps)
            ms[k].append(m)
            fills[k] += [x for x in f if x >= 0]
    one = vs.sample_burden(dev)
    totals = one.totals()
    table_rows, reported = one.layout()[1], one.layout()[0]
    one.close()
    out = {"workload": args.workload, "regions_per_step": nreg, "steps": args.steps, "reps": args.reps, "table_rows": table_rows,
           "rows_reported": reported, "carriers_in_matrix": totals[2], "burden_chunk": args.chunk or "default",
           "ceiling_tbps": args.ceiling_tbps, "build_s": round(t_build, 1), "legs": {}}
    for k, (_call, cols, n) in legs.items():
        med = float(np.median(ms[k]))
        leg = {"ms_per_step_median": round(med, 4), "ms_per_step_min": round(min(ms[k]), 4), "ms_per_step_max": round(max(ms[k]), 4),
               "regions_per_s": round(n / (med / 1e3)), "kernel_ms_median": round(float(np.median(fills[k])), 4) if fills[k] else None}
        if cols:
            leg["matrix_bytes"] = n * cols * 16
            leg["store_floor_ms"] = round(leg["matrix_bytes"] / (args.ceiling_tbps * 1e12) * 1e3, 4)
            if leg["kernel_ms_median"]:
                leg["store_floor_frac_of_kernel"] = round(leg["store_floor_ms"] / leg["kernel_ms_median"], 4)
        out["legs"][k] = leg
    t6 = out["legs"]["type6"]["ms_per_step_median"]
    out["step_vs_type6"] = {k: round(v["ms_per_step_median"] / t6, 3) for k, v in out["legs"].items() if k not in ("type6", "burden_all_long")}
    print(json.dumps(out), flush=True)
    vs.close()


if __name__ == "__main__":
    main()
