"""Window statistics against the step they contain and the route they replace, on bench.py's workload (chr1-2504 by default), built
the way bench.py builds it (its own functions, imported).  One handle; the GPU legs alternate in one process, each a loop of --steps
steps kept --depth deep as bench.py's loop keeps them, repeated --reps times; per G = 1, 2, 5, 26 and 64 (a random partition of the
cohort), with pair records:

  groups_G    (a) vs_query_group_counts alone: the step the new query contains
  windows_G   (b) vs_query_window_stats: the same group kernel into a temporary, then k_window_stats
  host_G      (c) what a caller does without the query: group_counts, the records (and the table's rows, for the dropped flags)
              brought to the host, np.add.reduceat over the same fields per region -- run --host-reps times, not in the loop.  The
              pair fields are reduced on the host up to --host-pairs-max groups (default 5: at 26 groups the 325 pairs take minutes
              in numpy); beyond, host_G is the route WITHOUT pair records, a lower bound of what the query replaces; beyond
              --host-groups-max groups (default 26: 64 groups are 5 GB of records and as much again in every numpy temporary) it is
              the query and the copy alone, a lower bound again

Prints one JSON line and writes it to profiles/windows_bench.json: per leg ms per step (median, min, max over the repeats) and the
median of each batch's own kernel time (vs_result_fill_ms: for windows_G the group kernel and the reduction between one pair of
events), per G the reduction kernel's time b - a, the bytes it reads (the rows all regions report x G x 16) and the rate that makes,
c / b, and the bytes that leave the GPU in b (the records) and in c (rows x G x 16 and the table's rows).

    python tools/bench_windows.py [--steps 10] [--reps 3] [--workload chr1-2504]
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

GROUPS = (1, 2, 5, 26, 64)


def spans_sum(x, begin, count):
    """Sum of x[begin[q] : begin[q] + count[q]] per region (regions overlap): np.add.reduceat over interleaved span ends."""
    x = np.concatenate([x, np.zeros((1,) + x.shape[1:], x.dtype)])   # (a span may end at the table's end)
    idx = np.stack([begin, begin + count], axis=1).reshape(-1)
    out = np.add.reduceat(x, idx, axis=0)[::2]
    out[count == 0] = 0                                               # (reduceat gives x[begin] for an empty span)
    return out


def host_route(vs, dev, members, with_pairs, reduce=True):
    """(c): -> (seconds, bytes brought to the host, a checksum of the reduced fields); reduce=False: the query and the copy alone."""
    t0 = time.perf_counter()
    res = vs.group_counts(dev, members)
    gc = res.group_counts()
    res.close()
    if not reduce:
        return time.perf_counter() - t0, gc["counts"].nbytes + gc["rows"].nbytes, 0
    counts, begin, count = gc["counts"], gc["row_begin"].astype(np.int64), gc["row_count"].astype(np.int64)
    live = ((gc["rows"]["count_flags"] >> 31) == 0).astype(np.int64)
    cn = 2 * gc["group_sizes"].astype(np.int64)
    ac = counts["alt_alleles"].astype(np.int64)
    het = counts["carriers"].astype(np.int64) - counts["hom_alt"].astype(np.int64)
    total = ac.sum(axis=1, keepdims=True)
    fields = {"rows": spans_sum(live, begin, count), "seg": spans_sum(((ac > 0) & (ac < cn)).astype(np.int64), begin, count),
              "singletons": spans_sum((ac == 1).astype(np.int64), begin, count), "doubletons": spans_sum((ac == 2).astype(np.int64), begin, count),
              "private": spans_sum(((ac > 0) & (ac == total)).astype(np.int64), begin, count),
              "fixed": spans_sum(((cn > 0) & (ac == cn)).astype(np.int64), begin, count), "sum_ac": spans_sum(ac, begin, count),
              "sum_ac2": spans_sum(ac * ac, begin, count), "obs_het": spans_sum(het, begin, count)}
    check = int(sum(int(v.sum()) for v in fields.values()))
    if with_pairs:
        g_n = ac.shape[1]
        for g in range(g_n):
            for h in range(g + 1, g_n):
                a, b = ac[:, g], ac[:, h]
                check += int(spans_sum(a * b, begin, count).sum())
                check += int(spans_sum(((a + b > 0) & (a + b < cn[g] + cn[h])).astype(np.int64), begin, count).sum())
                check += int(spans_sum(((cn[g] > 0) & (cn[h] > 0) & (((a == 0) & (b == cn[h])) | ((a == cn[g]) & (b == 0)))).astype(np.int64),
                                       begin, count).sum())
    return time.perf_counter() - t0, counts.nbytes + gc["rows"].nbytes, check


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-pairs-max", type=int, default=5)
    ap.add_argument("--host-groups-max", type=int, default=26)
    ap.add_argument("--workload", default="chr1-2504", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--regions", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows_bench.json"))
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
    legs = {}
    for g in GROUPS:
        legs[f"groups_{g}"] = (lambda g: lambda: [vs.group_counts(dev, members[g])])(g)
        legs[f"windows_{g}"] = (lambda g: lambda: [vs.window_stats(dev, members[g], pairs=True)])(g)

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
    probe = vs.window_stats(dev, members[2])
    reported, table_rows = probe.layout()[:2]
    probe.close()
    out = {"workload": args.workload, "regions_per_step": nreg, "steps": args.steps, "reps": args.reps, "table_rows": table_rows,
           "rows_reported": reported, "samples": ns, "build_s": round(t_build, 1), "legs": {}, "per_groups": {}}
    for k in legs:
        med = float(np.median(ms[k]))
        out["legs"][k] = {"ms_per_step_median": round(med, 4), "ms_per_step_min": round(min(ms[k]), 4), "ms_per_step_max": round(max(ms[k]), 4),
                          "kernel_ms_median": round(float(np.median(fills[k])), 4) if fills[k] else None}
    for g in GROUPS:
        a, b = out["legs"][f"groups_{g}"], out["legs"][f"windows_{g}"]
        pairs = g * (g - 1) // 2
        red_ms = b["kernel_ms_median"] - a["kernel_ms_median"]
        read = reported * g * 16
        per = {"pairs": pairs, "reduction_kernel_ms": round(red_ms, 4), "reduction_over_group_kernel": round(red_ms / a["kernel_ms_median"], 3),
               "reduction_reads_bytes": read, "reduction_read_gb_per_s": round(read / (red_ms * 1e6), 1) if red_ms > 0 else None,
               "step_b_minus_a_ms": round(b["ms_per_step_median"] - a["ms_per_step_median"], 4),
               "bytes_off_gpu_b": nreg * (48 * g + 16 * pairs), "bytes_off_gpu_c": None, "host_route_ms": None, "host_route_pairs": None,
               "host_route_reduced": None, "c_over_b": None}
        try:
            with_pairs, reduce = g <= args.host_pairs_max, g <= args.host_groups_max
            runs = [host_route(vs, dev, members[g], with_pairs, reduce) for _ in range(args.host_reps)]
            c_ms = float(np.median([r[0] for r in runs])) * 1e3
            per.update(bytes_off_gpu_c=runs[0][1], host_route_ms=round(c_ms, 1), host_route_pairs=with_pairs and reduce, host_route_reduced=reduce,
                       c_over_b=round(c_ms / b["ms_per_step_median"], 1))
        except Exception as e:   # (host memory: the route's own limit, recorded instead of a figure)
            per["host_route_ms"] = f"failed: {type(e).__name__}: {e}"[:200]
        out["per_groups"][str(g)] = per
    line = json.dumps(out)
    print(line, flush=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    vs.close()


if __name__ == "__main__":
    main()
