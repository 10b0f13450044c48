"""LD-score queries (vs_query_ld_scores) on bench.py's cohort (chr1-2504 by default), built the way bench.py builds it (its own
functions, imported), beside the LD-matrix query -- the same MFMA work with the cells stored -- and the route the query replaces.
One handle; the calls alternate in one process, each a loop of --steps calls, repeated --reps times.  The batch is
tools/bench_prune.py's `regions` leg: --regions regions of the bench's own length (10 kb, about 200 rows each), the whole cohort.

Per call it records ms per call (median, min, max over the repeats) and the median of the batch's own kernel time
(vs_result_fill_ms) of
  ld_scores      the query at --window (0: no row limit) and --bp
  ld_matrix_r2   ld_matrix(stat="r2") on the same batch
  counts, matrix the two stages both share
and of the route without the query, timed once as a whole with its copy:
  host_route     ld_matrix(stat="r2") -> the cells copied to the host -> masked row sums in numpy over every region
and from them stage_ms (the score kernels, and the block kernel: a batch's kernel time minus the counts' and the matrix query's on
the same batch), the tile pairs both kernels work on and ns per tile pair, and the largest difference between the query's
sums / 2^32 and the host route's float sums.

Prints one JSON line and writes it to --out (profiles/ldscore_bench.json).

    python tools/bench_ldscore.py [--steps 5] [--reps 3] [--workload chr1-2504]
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
from variantstore_amd import VariantStore  # noqa: E402


def host_sums(got, scored, pos, window, max_bp):
    """The masked row sums of an ld_matrix() dict on the host: (float64 per slot, seconds)."""
    t0 = time.perf_counter()
    out = []
    bb = got["block_begin"].astype(np.int64)
    for q, (a0, m) in enumerate(zip(got["row_begin"].astype(np.int64).tolist(), got["row_count"].astype(np.int64).tolist())):
        r2 = got["cells"][bb[q]:bb[q + 1]].reshape(m, m).astype(np.float64)
        ok = scored[a0:a0 + m]
        mask = ok[:, None] & ok[None, :]
        if window:
            idx = np.arange(m)
            mask &= np.abs(idx[:, None] - idx[None, :]) <= window
        if max_bp:
            p = pos[a0:a0 + m]
            mask &= np.abs(p[:, None] - p[None, :]) <= max_bp
        out.append(np.where(mask, r2, 0.0).sum(axis=1))
    return (np.concatenate(out) if out else np.zeros(0)), time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--regions", type=int, default=2000)
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--bp", type=int, default=1_000_000)
    ap.add_argument("--workload", default="chr1-2504", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldscore_bench.json"))
    args = ap.parse_args()
    w = bench.WORKLOADS[args.workload]
    t0 = time.perf_counter()
    vs = VariantStore.synthetic(device=0, **bench.synth_kwargs(w))
    build_s = time.perf_counter() - t0
    n_cols = vs.info().num_samples - 1
    reg = np.ascontiguousarray(bench.make_regions(w, 0, w["regions"])[:: max(1, w["regions"] // args.regions)][: args.regions])

    def fill_ms(r):
        ms = r.fill_ms()   # (waits for the batch)
        r.close()
        return ms

    def timed(call, steps):
        t0 = time.perf_counter()
        extra = [call() for _ in range(steps)]
        return (time.perf_counter() - t0) * 1e3 / steps, extra

    calls = {"ld_scores": lambda: fill_ms(vs.ld_scores(reg, window=args.window, max_bp=args.bp)),
             "ld_matrix_r2": lambda: fill_ms(vs.ld_matrix(reg, stat="r2")),
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
    one = vs.ld_scores(reg, window=args.window, max_bp=args.bp)
    got = one.ld_scores()
    one.close()
    # the route without the query, once
    t = [time.perf_counter()]
    r = vs.ld_matrix(reg, stat="r2")
    r.fill_ms()
    t.append(time.perf_counter())
    mat = r.ld_matrix()   # the copy: 4 m^2 bytes per region over the link (the cells stay the result's: it is closed behind the sums)
    t.append(time.perf_counter())
    kb = got["keep_begin"].astype(np.int64)
    scored = np.zeros(got["rows"].shape[0], bool)
    for q, (a0, m) in enumerate(zip(got["row_begin"].astype(np.int64).tolist(), got["row_count"].astype(np.int64).tolist())):
        scored[a0:a0 + m] = got["state"][kb[q]:kb[q] + m] == 1   # (eligibility belongs to the table row, whichever region reports it)
    host, secs = host_sums(mat, scored, got["rows"]["pos"].astype(np.int64), args.window, args.bp)
    t.append(time.perf_counter())
    cell_bytes = int(mat["cells"].nbytes)
    r.close()
    host_stage = [(b - a) * 1e3 for a, b in zip(t[:-1], t[1:])]
    rows, slots = int(got["rows"].shape[0]), int(got["sums"].shape[0])
    pitch = (n_cols + 15) // 16 * 16
    tiles = (got["row_count"].astype(np.int64) + 63) // 64
    reach = np.minimum(tiles - 1, (args.window + 63) // 64) if args.window else tiles - 1
    score_pairs = int(np.where(tiles > 0, tiles * (reach + 1) - reach * (reach + 1) // 2, 0).sum())   # workgroups that do not leave at once
    score_wgs = int(np.where(tiles > 0, tiles * (reach + 1), 0).sum())
    block_pairs = int((tiles * (tiles + 1) // 2).sum())
    out = {"workload": args.workload, "steps": args.steps, "reps": args.reps, "build_s": round(build_s, 1), "window": args.window, "max_bp": args.bp,
           "regions": int(reg.shape[0]), "rows": rows, "slots": slots, "columns": int(n_cols), "row_pitch": int(pitch),
           "rows_per_region_median": int(np.median(got["row_count"])), "rows_per_region_max": int(got["row_count"].max()),
           "scored": int(got["n_scored"].sum()), "ineligible": int((got["state"] == 2).sum()), "pairs_summed": int(got["n_pairs"].astype(np.int64).sum()),
           "mean_score": round(float(got["scores"][got["state"] == 1].mean()), 4) if (got["state"] == 1).any() else None,
           "matrix_bytes": rows * pitch, "slot_bytes": 13 * slots, "ld_matrix_cell_bytes": cell_bytes,
           "score_workgroups": score_wgs, "score_tile_pairs": score_pairs, "ld_matrix_tile_pairs": block_pairs}
    for k in calls:
        out[k + "_ms_per_call"] = {"median": round(float(np.median(ms[k])), 4), "min": round(min(ms[k]), 4), "max": round(max(ms[k]), 4)}
    kern = {k: float(np.median(extra[k])) for k in calls}
    out["fill_ms"] = {k: round(v, 4) for k, v in kern.items()}
    stage = kern["ld_scores"] - kern["counts"] - kern["matrix"]
    block_stage = kern["ld_matrix_r2"] - kern["counts"] - kern["matrix"]
    out["stage_ms"] = round(stage, 4)
    out["ld_matrix_stage_ms"] = round(block_stage, 4)
    out["stage_ns_per_tile_pair"] = round(stage * 1e6 / score_pairs, 2) if score_pairs else None
    out["ld_matrix_stage_ns_per_tile_pair"] = round(block_stage * 1e6 / block_pairs, 2) if block_pairs else None
    out["host_route_ms"] = round(sum(host_stage), 2)
    out["host_route_stage_ms"] = {"ld_matrix_query": round(host_stage[0], 3), "cells_to_host": round(host_stage[1], 3), "numpy_row_sums": round(host_stage[2], 3)}
    out["largest_difference_from_host_route"] = float(np.abs(host - got["scores"]).max()) if slots else 0.0
    out["ld_scores_vs_host_route"] = round(out["ld_scores_ms_per_call"]["median"] / out["host_route_ms"], 5)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    vs.close()


if __name__ == "__main__":
    main()
