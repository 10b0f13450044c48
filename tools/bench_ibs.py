"""Pairwise IBS queries (vs_query_sample_ibs) against the Gram query on the same batch and against the path a caller had before
them: genotype_matrix_device() -> three indicator matrices in bf16 (het, hom-alt, carrier) -> three X.T @ X (float32 accumulation,
exact while a cell stays below 2^24; the time of the conversions counts).  One process, one box, the legs alternating:

  chr1-2504 (bench.py's cohort, built the way bench.py builds it), the whole cohort, batches of --small-regions and
  --large-regions regions of bench.py's batch (about 10 k and about 100 k table rows), and a 300-sample cohort (the GPU tests'
  larger one) with 3,000 regions.

Per leg and statistic ("counts", "king"): ms per call (median, min, max over --reps loops of --steps calls, each call read back to
the point where its kernels have finished), the batch's own kernel time (vs_result_fill_ms: counts, temporary matrix and the IBS
kernels together), the kernel times of an allele-count batch and of a genotype-matrix batch over the same regions and samples (the
first two stages on their own), their difference to the IBS batch (the IBS stage: k_ibs_n_used, k_sample_ibs, k_ibs_finish),
beside it the same for sample_gram ("dot") on the same batch, the ratio IBS stage / Gram stage (three products against one), the
int8 multiply-accumulates of the three products -- useful: 3 A n (n + 1) / 2; issued: every launched 128 x 128 tile pair over
the rows rounded up to 64, three times -- and their rate over the IBS stage, and the torch path's ms per call with its stages.

--chunk sets option ibs_chunk (0: the default by shape); --chunks a,b,c sweeps it on every leg ("counts" only) and reports the
kernel time per setting.

Prints one JSON line and writes it to --out (profiles/ibs_bench.json).

    python tools/bench_ibs.py [--steps 5] [--reps 3]
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

TILE = 128   # kGramTile of k_gram.hip.h: k_sample_ibs takes its tiles
T6_KW = dict(ref_length=8_000_000, num_variants=150_000, num_samples=300, seed=5, first_pos=1_000, frac_ins=0.05, frac_del=0.05,
             frac_multi=0.02, max_indel=6, af_exponent=2.0)


class _DeviceBytes:
    """rows x pitch bytes of device memory for torch.as_tensor."""

    def __init__(self, ptr, rows, pitch):
        self.__cuda_array_interface__ = {"shape": (rows, pitch), "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small-regions", type=int, default=200)
    ap.add_argument("--large-regions", type=int, default=2000)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--chunks", default="", help="comma-separated ibs_chunk settings to sweep (kernel ms of 'counts' per setting)")
    ap.add_argument("--workload", default="chr1-2504", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ibs_bench.json"))
    args = ap.parse_args()
    import torch
    w = bench.WORKLOADS[args.workload]
    regions = bench.make_regions(w, 0, w["regions"])   # (sorted by start and overlapping: a stretch of the reference per leg)
    t0 = time.perf_counter()
    big = VariantStore.synthetic(device=0, **bench.synth_kwargs(w))
    small = VariantStore.synthetic(device=0, **T6_KW)
    build_s = time.perf_counter() - t0
    for vs in (big, small):
        vs.set_option("ibs_chunk", args.chunk)
    rng = np.random.default_rng(12)
    s = np.sort(rng.integers(1_000, 7_990_000, size=3_000))
    r300 = np.stack([s, s + rng.integers(50, 3_000, size=3_000)], axis=1).astype(np.uint64)
    legs = {f"{args.workload}_{args.small_regions}_regions": (big, np.ascontiguousarray(regions[: args.small_regions])),
            f"{args.workload}_{args.large_regions}_regions": (big, np.ascontiguousarray(regions[: args.large_regions])),
            "300_samples_3000_regions": (small, r300)}

    def fill_ms(r):
        ms = r.fill_ms()   # (waits for the batch)
        r.close()
        return ms

    via_host = [False]

    def torch_path(vs, reg):
        t = [time.perf_counter()]
        r = vs.genotype_matrix(reg)
        ptr, rows, cols, pitch = r.genotype_matrix_device()
        t.append(time.perf_counter())
        if rows:
            try:
                cells = torch.as_tensor(_DeviceBytes(ptr, rows, pitch), device="cuda")[:, :cols]
            except (TypeError, RuntimeError, ValueError):   # this torch does not take the interface: through the host (slower: said in the output)
                via_host[0] = True
                cells = torch.from_numpy(np.ascontiguousarray(r.genotype_matrix()["cells"])).cuda()
            d = ((cells >> 1) & 1) + ((cells >> 2) & 1)
            xs = [(d == 1).to(torch.bfloat16), (d == 2).to(torch.bfloat16), (d > 0).to(torch.bfloat16)]
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            gs = [x.T @ x for x in xs]
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            del gs, xs, d, cells
        else:
            t += [t[-1], t[-1]]
        r.close()
        return [(b - a) * 1e3 for a, b in zip(t[:-1], t[1:])]

    def timed(call, steps):
        t0 = time.perf_counter()
        extra = [call() for _ in range(steps)]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps, extra

    out = {"workload": args.workload, "steps": args.steps, "reps": args.reps, "build_s": round(build_s, 1), "tile": TILE, "ibs_chunk": args.chunk,
           "legs": {}}
    for name, (vs, reg) in legs.items():
        calls = {"ibs_counts": lambda: fill_ms(vs.sample_ibs(reg, stat="counts")), "ibs_king": lambda: fill_ms(vs.sample_ibs(reg, stat="king")),
                 "gram_dot": lambda: fill_ms(vs.sample_gram(reg, stat="dot")), "counts": lambda: fill_ms(vs.allele_counts(reg)),
                 "matrix": lambda: fill_ms(vs.genotype_matrix(reg)), "torch": lambda: torch_path(vs, reg)}
        for c in calls.values():
            timed(c, args.warmup)
        ms = {k: [] for k in calls}
        extra = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, c in calls.items():
                m, e = timed(c, args.steps)
                ms[k].append(m)
                extra[k] += e
        one = vs.sample_ibs(reg)
        _pm, _pk, _pc, rows, n, _st = one.sample_ibs_device()
        one.close()
        tiles = (n + TILE - 1) // TILE
        pairs = tiles * (tiles + 1) // 2
        useful = 3 * rows * n * (n + 1) // 2
        issued = 3 * pairs * TILE * TILE * ((rows + 63) // 64 * 64)
        leg = {"rows": rows, "columns": n, "regions": int(reg.shape[0]), "tile_pairs": pairs, "mac_useful": useful, "mac_issued": issued}
        for k in calls:
            leg[k + "_ms_per_call"] = {"median": round(float(np.median(ms[k])), 4), "min": round(min(ms[k]), 4), "max": round(max(ms[k]), 4)}
        kern = {k: float(np.median(extra[k])) for k in calls if k != "torch"}
        leg["kernel_ms"] = {k: round(v, 4) for k, v in kern.items()}
        gram_stage = kern["gram_dot"] - kern["counts"] - kern["matrix"]
        leg["gram_stage_ms_dot"] = round(gram_stage, 4)
        for stat in ("counts", "king"):
            stage = kern["ibs_" + stat] - kern["counts"] - kern["matrix"]
            leg[f"ibs_stage_ms_{stat}"] = round(stage, 4)
            if stage > 0:
                leg[f"useful_tmac_per_s_{stat}"] = round(useful / stage / 1e9, 3)
                leg[f"issued_tmac_per_s_{stat}"] = round(issued / stage / 1e9, 3)
            if gram_stage > 0:
                leg[f"ibs_stage_over_gram_stage_{stat}"] = round(stage / gram_stage, 3)
        tp = np.median(np.asarray(extra["torch"]), axis=0)
        leg["torch_stage_ms"] = {"matrix_query": round(float(tp[0]), 4), "to_bf16_indicators": round(float(tp[1]), 4), "products": round(float(tp[2]), 4)}
        leg["ibs_counts_vs_torch"] = round(leg["ibs_counts_ms_per_call"]["median"] / leg["torch_ms_per_call"]["median"], 3)
        leg["ibs_counts_vs_gram_dot"] = round(leg["ibs_counts_ms_per_call"]["median"] / leg["gram_dot_ms_per_call"]["median"], 3)
        if args.chunks:
            sweep = {}
            for ch in [int(x) for x in args.chunks.split(",")]:
                vs.set_option("ibs_chunk", ch)
                timed(calls["ibs_counts"], args.warmup)
                sweep[str(ch)] = round(float(np.median([np.median(timed(calls["ibs_counts"], args.steps)[1]) for _ in range(args.reps)])), 4)
            vs.set_option("ibs_chunk", args.chunk)
            leg["chunk_sweep_kernel_ms_counts"] = sweep
        out["legs"][name] = leg
    out["torch_matrix_via_host"] = via_host[0]
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    big.close()
    small.close()


if __name__ == "__main__":
    main()
