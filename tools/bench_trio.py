"""Trio queries (vs_query_trio_scan) against the genotype-matrix query over the same member columns, on one box in one run, the
legs alternating:

  chr1-2504 (bench.py's cohort, built the way bench.py builds it), batches of --small-regions and --large-regions regions of
  bench.py's batch, 600 disjoint trios drawn from the 2,504 samples with a fixed seed (1,800 member columns).

  leg a   genotype_matrix over the member columns: k_genotype_matrix writes the matrix once
  leg b   trio_scan over the same regions and trios: k_allele_counts, k_genotype_matrix into the temporary, k_ibs_n_used and
          k_trio_scan, which reads the matrix once
  leg c   allele_counts over the member columns: k_allele_counts alone

Per leg: ms per call (median, min, max over --reps loops of --steps calls, each call read back to the point where its kernels have
finished) and the batch's own kernel time (vs_result_fill_ms).  The trio stage -- k_ibs_n_used and k_trio_scan -- is b - a - c;
b - a (the scan with the counts it skips by) and the ratio b / a are reported beside it.  The matrix bytes the scan reads (rows x
row pitch, once per trio chunk) over the stage are its bytes per second, held against the copy rate of tools/microbench/hbm_ceiling
where --ceiling-tb-s gives that run's figure.

--chunks a,b,c sweeps option trio_chunk (0: the default by shape) on every leg and reports the kernel time of leg b per setting
(median, min, max over the repeats).

Prints one JSON line and writes it to --out (profiles/trio_bench.json).

    python tools/bench_trio.py [--steps 5] [--reps 3] [--chunks 0,64,128,256,640]
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

N_TRIOS = 600
TRIO_SEED = 602


def spread(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small-regions", type=int, default=200)
    ap.add_argument("--large-regions", type=int, default=2000)
    ap.add_argument("--chunks", default="0,64,128,256,640", help="comma-separated trio_chunk settings to sweep (kernel ms of leg b per setting)")
    ap.add_argument("--ceiling-tb-s", type=float, default=0.0, help="the copy rate of the same box's hbm_ceiling run, TB/s (0: not measured)")
    ap.add_argument("--workload", default="chr1-2504", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trio_bench.json"))
    args = ap.parse_args()
    w = bench.WORKLOADS[args.workload]
    regions = bench.make_regions(w, 0, w["regions"])   # (sorted by start and overlapping: a stretch of the reference per leg)
    t0 = time.perf_counter()
    vs = VariantStore.synthetic(device=0, **bench.synth_kwargs(w))
    build_s = time.perf_counter() - t0
    n_samples = vs.info().num_samples - 1
    rng = np.random.default_rng(TRIO_SEED)
    trios = (rng.permutation(n_samples)[: 3 * N_TRIOS] + 1).astype(np.uint32).reshape(N_TRIOS, 3)
    members = np.unique(trios)
    legs = {f"{args.workload}_{args.small_regions}_regions": np.ascontiguousarray(regions[: args.small_regions]),
            f"{args.workload}_{args.large_regions}_regions": np.ascontiguousarray(regions[: args.large_regions])}

    def fill_ms(r):
        ms = r.fill_ms()   # (waits for the batch)
        r.close()
        return ms

    def timed(call, steps):
        t0 = time.perf_counter()
        extra = [call() for _ in range(steps)]
        return (time.perf_counter() - t0) * 1e3 / steps, extra

    out = {"workload": args.workload, "steps": args.steps, "reps": args.reps, "build_s": round(build_s, 1), "n_trios": N_TRIOS,
           "member_columns": int(members.shape[0]), "trio_seed": TRIO_SEED, "copy_ceiling_tb_s": args.ceiling_tb_s or None, "legs": {}}
    for name, reg in legs.items():
        vs.set_option("trio_chunk", 0)
        calls = {"a_matrix": lambda: fill_ms(vs.genotype_matrix(reg, members)), "b_trio_scan": lambda: fill_ms(vs.trio_scan(reg, trios)),
                 "c_counts": lambda: fill_ms(vs.allele_counts(reg, members))}
        for c in calls.values():
            timed(c, args.warmup)
        ms = {k: [] for k in calls}
        kern = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, c in calls.items():
                m, e = timed(c, args.steps)
                ms[k].append(m)
                kern[k].append(float(np.median(e)))
        one = vs.trio_scan(reg, trios)
        got = one.trio_scan()
        one.close()
        rows, pitch = int(got["rows"].shape[0]), (int(members.shape[0]) + 15) // 16 * 16
        live = int(np.count_nonzero(got["counts"]["carriers"]))
        leg = {"rows": rows, "rows_with_a_carrier_among_the_members": live, "columns": int(members.shape[0]), "row_pitch": pitch,
               "regions": int(reg.shape[0]), "matrix_bytes": rows * pitch,
               "errors": int(got["row_stats"]["errors"].astype(np.int64).sum()), "transmitted": int(got["row_stats"]["transmitted"].astype(np.int64).sum())}
        for k in calls:
            leg[k + "_ms_per_call"] = spread(ms[k])
            leg[k + "_kernel_ms"] = spread(kern[k])
        a, b, c = (float(np.median(kern[k])) for k in ("a_matrix", "b_trio_scan", "c_counts"))
        leg["b_over_a_kernel"] = round(b / a, 3) if a > 0 else None
        leg["b_minus_a_kernel_ms"] = round(b - a, 4)
        stage = b - a - c
        leg["trio_stage_kernel_ms"] = round(stage, 4)
        if stage > 0:
            leg["trio_stage_matrix_gb_per_s"] = round(rows * pitch / stage / 1e6, 1)
            if args.ceiling_tb_s:
                leg["trio_stage_share_of_copy_ceiling"] = round(rows * pitch / stage / 1e9 / args.ceiling_tb_s, 4)
        sweep = {}
        for ch in [int(x) for x in args.chunks.split(",") if x != ""]:
            vs.set_option("trio_chunk", ch)
            timed(calls["b_trio_scan"], args.warmup)
            sweep[str(ch)] = spread([float(np.median(timed(calls["b_trio_scan"], args.steps)[1])) for _ in range(args.reps)])
        vs.set_option("trio_chunk", 0)
        leg["chunk_sweep_b_kernel_ms"] = sweep
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
