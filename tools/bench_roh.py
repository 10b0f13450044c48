"""ROH queries (vs_query_roh) against the genotype-matrix query over the same regions and samples, on one box in one run, the legs
alternating:

  chr1-2504 (bench.py's cohort, built the way bench.py builds it), the whole cohort's 2,504 columns.
  shape "many"   --many-regions regions of bench.py's batch (10 kb each): thousands of short walks, ten column tiles each
  shape "long"   --long-regions regions of --long-bp bases each, laid end to end from the first position: a few long walks -- the
                 sequential case, (regions x 10 column tiles) workgroups on a device of 256 compute units

  leg a   genotype_matrix: k_genotype_matrix writes the matrix once
  leg b   roh with segments: k_allele_counts, k_genotype_matrix into the temporary, k_roh_sites, k_roh_walk twice around the scan and
          its host wait (inside the pair of events: the kernel time of this leg contains that wait)
  leg c   allele_counts: k_allele_counts alone
  leg d   roh without segments: one walk, no host wait

Per leg: ms per call (median, min, max over --reps loops of --steps calls, each call read back to the point where its kernels have
finished) and the batch's own kernel time (vs_result_fill_ms).  The walk alone is d - a - c (sites kernel included); the matrix
bytes (rows x row pitch) over it are the walk's bytes per second.  No threshold is set anywhere.

Prints one JSON line and writes it to --out (profiles/roh_bench.json).

    python tools/bench_roh.py [--steps 5] [--reps 3]
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


def spread(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--many-regions", type=int, default=2000)
    ap.add_argument("--long-regions", type=int, default=4)
    ap.add_argument("--long-bp", type=int, default=2_500_000)
    ap.add_argument("--min-sites", type=int, default=50)
    ap.add_argument("--max-het", type=int, default=1)
    ap.add_argument("--workload", default="chr1-2504", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roh_bench.json"))
    args = ap.parse_args()
    w = bench.WORKLOADS[args.workload]
    regions = bench.make_regions(w, 0, w["regions"])
    t0 = time.perf_counter()
    vs = VariantStore.synthetic(device=0, **bench.synth_kwargs(w))
    build_s = time.perf_counter() - t0
    first = int(np.asarray(regions)[:, 0].min())
    long_regions = np.asarray([(first + k * args.long_bp, first + (k + 1) * args.long_bp - 1) for k in range(args.long_regions)], np.uint64)
    legs = {f"many_{args.many_regions}_regions": np.ascontiguousarray(regions[: args.many_regions]),
            f"long_{args.long_regions}_regions_of_{args.long_bp}_bp": long_regions}
    kw = dict(min_sites=args.min_sites, max_het=args.max_het)

    def fill_ms(r):
        ms = r.fill_ms()   # (waits for the batch)
        r.close()
        return ms

    def timed(call, steps):
        t0 = time.perf_counter()
        extra = [call() for _ in range(steps)]
        return (time.perf_counter() - t0) * 1e3 / steps, extra

    out = {"workload": args.workload, "steps": args.steps, "reps": args.reps, "build_s": round(build_s, 1), "params": kw, "legs": {}}
    for name, reg in legs.items():
        calls = {"a_matrix": lambda: fill_ms(vs.genotype_matrix(reg)), "b_roh_segments": lambda: fill_ms(vs.roh(reg, **kw)),
                 "c_counts": lambda: fill_ms(vs.allele_counts(reg)), "d_roh_summaries": lambda: fill_ms(vs.roh(reg, segments=False, **kw))}
        for c in calls.values():
            timed(c, args.warmup)
        ms = {k: [] for k in calls}
        kern = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, c in calls.items():
                m, e = timed(c, args.steps)
                ms[k].append(m)
                kern[k].append(float(np.median(e)))
        one = vs.roh(reg, **kw)
        got = one.roh()
        one.close()
        rows, cols = int(got["rows"].shape[0]), int(got["columns"].shape[0])
        pitch = (cols + 15) // 16 * 16
        leg = {"regions": int(reg.shape[0]), "rows": rows, "columns": cols, "row_pitch": pitch, "matrix_bytes": rows * pitch,
               "sites": int(got["n_sites"].astype(np.int64).sum()), "segments": int(got["segments"].shape[0]),
               "workgroups_of_the_walk": int(reg.shape[0]) * ((cols + 255) // 256)}
        for k in calls:
            leg[k + "_ms_per_call"] = spread(ms[k])
            leg[k + "_kernel_ms"] = spread(kern[k])
        a, b, c, d = (float(np.median(kern[k])) for k in ("a_matrix", "b_roh_segments", "c_counts", "d_roh_summaries"))
        leg["b_over_a_kernel"] = round(b / a, 3) if a > 0 else None
        leg["d_over_a_kernel"] = round(d / a, 3) if a > 0 else None
        walk = d - a - c
        leg["walk_kernel_ms"] = round(walk, 4)
        leg["second_pass_scan_and_wait_ms"] = round(b - d, 4)
        if walk > 0:
            leg["walk_matrix_gb_per_s"] = round(rows * pitch / walk / 1e6, 1)
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
