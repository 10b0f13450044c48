"""LD pruning queries (vs_query_ld_prune) on bench.py's cohort (chr1-2504 by default), built the way bench.py builds it (its own
functions, imported), beside the band query and the route the query replaces.  One handle; per leg the calls alternate in one
process, each a loop of --steps calls, repeated --reps times.  Two legs, both over the whole cohort:

  regions  --regions regions of the bench's own length (10 kb, about 200 rows each): one wave per region, thousands of walks at once
  one      ONE region of --one-len bases (about as many rows as the other leg's table): a single sequential chain

Per leg and call it records ms per call (median, min, max over the repeats) and the median of the batch's own kernel time
(vs_result_fill_ms) of
  ld_prune       the query at --window and --r2
  ld_band_r2     ld_band(stat="r2") on the same batch and window
and of the route without the query, timed as a whole with its copy:
  host_route     ld_band(stat="r2") -> the band copied to the host -> a sequential greedy in numpy over every region (float r2 > bound
                 where the query compares integers; eligibility from the count records): its three stages are recorded as well
and from them stage_ms (the mask kernel and the walk: the pruning batch's kernel time minus the counts' and the matrix query's on
the same batch), walk_ns_per_row for the `one` leg (what a single chain costs per row), and how many verdicts of the host route
differ from the query's.

Prints one JSON line and writes it to --out (profiles/prune_bench.json).

    python tools/bench_prune.py [--steps 5] [--reps 3] [--workload chr1-2504]
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
from variantstore_amd import VariantStore, quantise_r2  # noqa: E402


def host_greedy(band, counts, dropped, n, row_begin, row_count, bound):
    """The forward greedy on the host from the float band: (state per reported row, seconds).  A 'blocked' bit vector per walk, as
    the kernel keeps it, so that the loop does one numpy operation per kept row."""
    t0 = time.perf_counter()
    window = band.shape[1]
    ac = counts["alt_alleles"].astype(np.int64)
    v = np.int64(n) * (ac + 2 * counts["hom_alt"].astype(np.int64)) - ac * ac
    code = np.where(dropped, 3, np.where(v > 0, 0, 2)).astype(np.uint8)
    hits = band > np.float32(bound)
    out = []
    for a0, m in zip(row_begin.tolist(), row_count.tolist()):
        state = code[a0:a0 + m].copy()
        blocked = np.zeros(m + window, bool)
        for i in np.nonzero(state == 0)[0].tolist():
            if not blocked[i]:
                state[i] = 1
                blocked[i + 1:i + 1 + window] |= hits[a0 + i]
        out.append(state)
    return (np.concatenate(out) if out else np.zeros(0, np.uint8)), time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--regions", type=int, default=2000)
    ap.add_argument("--one-len", type=int, default=20_000_000)
    ap.add_argument("--window", type=int, default=256)
    ap.add_argument("--r2", type=float, default=0.2)
    ap.add_argument("--legs", default="regions,one")
    ap.add_argument("--workload", default="chr1-2504", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_bench.json"))
    args = ap.parse_args()
    w = bench.WORKLOADS[args.workload]
    t0 = time.perf_counter()
    vs = VariantStore.synthetic(device=0, **bench.synth_kwargs(w))
    build_s = time.perf_counter() - t0
    n_cols = vs.info().num_samples - 1
    threshold = quantise_r2(args.r2)
    bound = threshold / (1 << 20)
    mid = (w["first_pos"] + w["ref_length"]) // 2
    all_legs = {"regions": np.ascontiguousarray(bench.make_regions(w, 0, w["regions"])[:: max(1, w["regions"] // args.regions)][: args.regions]),
                "one": np.asarray([[mid - args.one_len // 2, mid + args.one_len // 2]], np.uint64)}
    legs = {k: all_legs[k] for k in args.legs.split(",")}

    def fill_ms(r):
        ms = r.fill_ms()   # (waits for the batch)
        r.close()
        return ms

    last_host = {}

    def host_route(reg):
        t = [time.perf_counter()]
        r = vs.ld_band(reg, window=args.window, stat="r2")
        r.fill_ms()
        t.append(time.perf_counter())
        got = r.ld_band()   # the copy: rows x window x 4 bytes over the link
        r.close()
        t.append(time.perf_counter())
        dropped = (got["rows"]["count_flags"] >> 31) != 0
        state, secs = host_greedy(got["band"], got["counts"], dropped, n_cols, got["row_begin"].astype(np.int64), got["row_count"].astype(np.int64), bound)
        t.append(time.perf_counter())
        last_host["state"] = state
        return [(b - a) * 1e3 for a, b in zip(t[:-1], t[1:])]

    def timed(call, steps):
        t0 = time.perf_counter()
        extra = [call() for _ in range(steps)]
        return (time.perf_counter() - t0) * 1e3 / steps, extra

    out = {"workload": args.workload, "steps": args.steps, "reps": args.reps, "build_s": round(build_s, 1), "window": args.window, "r2": args.r2,
           "threshold_q20": threshold, "legs": {}}
    for name, reg in legs.items():
        calls = {"ld_prune": lambda: fill_ms(vs.ld_prune(reg, window=args.window, r2=args.r2)),
                 "ld_band_r2": lambda: fill_ms(vs.ld_band(reg, window=args.window, stat="r2")),
                 "counts": lambda: fill_ms(vs.allele_counts(reg)), "matrix": lambda: fill_ms(vs.genotype_matrix(reg))}
        for c in calls.values():
            timed(c, args.warmup)
        ms = {k: [] for k in calls}
        extra = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, c in calls.items():
                m, e = timed(c, args.steps)
                ms[k].append(m)
                extra[k] += e
        host_ms, host_stages = timed(lambda: host_route(reg), 1)   # (seconds of Python: once)
        one = vs.ld_prune(reg, window=args.window, r2=args.r2)
        got = one.ld_prune()
        one.close()
        rows, states = int(got["rows"].shape[0]), int(got["state"].shape[0])
        pitch = (n_cols + 15) // 16 * 16
        leg = {"regions": int(reg.shape[0]), "rows": rows, "verdicts": states, "columns": int(n_cols), "row_pitch": int(pitch),
               "rows_per_region_median": int(np.median(got["row_count"])), "rows_per_region_max": int(got["row_count"].max()),
               "kept": int(got["n_kept"].sum()), "pruned": int((got["state"] == 0).sum()), "ineligible": int((got["state"] == 2).sum()),
               "matrix_bytes": rows * pitch, "mask_bytes": rows * 4 * ((args.window + 31) // 32), "band_bytes": rows * 4 * args.window,
               "state_bytes": states}
        for k in calls:
            leg[k + "_ms_per_call"] = {"median": round(float(np.median(ms[k])), 4), "min": round(min(ms[k]), 4), "max": round(max(ms[k]), 4)}
        kern = {k: float(np.median(extra[k])) for k in calls}
        leg["fill_ms"] = {k: round(v, 4) for k, v in kern.items()}
        stage = kern["ld_prune"] - kern["counts"] - kern["matrix"]
        leg["stage_ms"] = round(stage, 4)
        leg["band_stage_ms"] = round(kern["ld_band_r2"] - kern["counts"] - kern["matrix"], 4)
        if name == "one" and rows:
            leg["walk_ns_per_row"] = round((stage - leg["band_stage_ms"]) * 1e6 / rows, 3) if stage > leg["band_stage_ms"] else None
            leg["stage_ns_per_row"] = round(stage * 1e6 / rows, 3)
        leg["host_route_ms"] = round(host_ms, 2)
        hs = host_stages[0]
        leg["host_route_stage_ms"] = {"ld_band_query": round(hs[0], 3), "band_to_host": round(hs[1], 3), "numpy_greedy": round(hs[2], 3)}
        leg["host_route_verdicts_that_differ"] = int((last_host["state"] != got["state"]).sum())
        leg["ld_prune_vs_host_route"] = round(leg["ld_prune_ms_per_call"]["median"] / host_ms, 5)
        out["legs"][name] = leg
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    vs.close()


if __name__ == "__main__":
    main()
