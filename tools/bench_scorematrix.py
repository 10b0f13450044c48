"""Score-matrix queries on the first --regions regions of bench.py's workload (chr1-2504 by default), built the way bench.py builds
it (its own functions, imported), beside the two routes of DESIGN 5m.  One handle; the legs alternate in one process, each a loop of
its steps, repeated --reps times, after a warm-up:

  matrix_K     vs_query_score_matrix, K weight columns (host float32, report order), whole cohort
  scores_K     route (b): ceil(K / 8) vs_query_sample_scores batches of 8 columns over the same weights
  torch_K      route (c): vs_query_genotype_matrix, then on genotype_matrix_device() in torch the cells to dosages (float64) and
               the product dosages^T @ (rows x K float64) -- neither exact nor reproducible

Writes one JSON document (--out, default profiles/scorematrix_bench.json) and prints it: per leg ms per step (median, min, max over
the repeats; the host's pass over the weights and their upload are inside) and the median of each batch's own pair of events
(vs_result_fill_ms: count kernel, matrix kernel, weight and limb passes with their two host waits, k_score_matrix, the finish; for
route (b) the sum over its batches).

    python tools/bench_scorematrix.py [--steps 10] [--reps 3] [--regions 10000] [--scores 8,16,64,512] [--routes matrix,scores,torch]
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


class _DeviceBytes:
    """(A, pitch) uint8 in device memory, for torch.as_tensor."""

    def __init__(self, ptr, a, pitch):
        self.__cuda_array_interface__ = {"shape": (a, pitch), "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workload", default="chr1-2504", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--regions", type=int, default=10_000)
    ap.add_argument("--scores", default="8,16,64,512")
    ap.add_argument("--routes", default="matrix,scores,torch")
    ap.add_argument("--chunk", type=int, default=0, help="option score_matrix_chunk")
    ap.add_argument("--overlap", type=int, default=0, help="every region this many times in the batch: every row reported that many times more")
    ap.add_argument("--weights", default="normal", choices=["normal", "max", "small"],
                    help="standard normal; every weight at its column's largest (four reports of a row need five limbs); or a hundredth of "
                    "the column's largest (the totals stay within four limbs however many regions report a row)")
    ap.add_argument("--budget-ms", type=float, default=1500.0, help="a leg's steps are cut so that one repeat stays near this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scorematrix_bench.json"))
    args = ap.parse_args()
    import torch
    w = bench.WORKLOADS[args.workload]
    nreg = min(args.regions, w["regions"])
    regions = bench.make_regions(w, 0, w["regions"])[:nreg]
    if args.overlap > 1:
        regions = np.repeat(np.ascontiguousarray(regions), args.overlap, axis=0)
        nreg = regions.shape[0]
    routes = set(args.routes.split(","))
    t_build = time.perf_counter()
    vs = VariantStore.synthetic(device=0, **bench.synth_kwargs(w))
    t_build = time.perf_counter() - t_build
    vs.set_option("score_matrix_chunk", args.chunk)
    ns = vs.info().num_samples - 1
    regions_dev = torch.from_numpy(np.ascontiguousarray(regions).astype(np.int64)).cuda().contiguous()
    torch.cuda.synchronize()
    dev = DeviceArray(regions_dev.data_ptr(), nreg)
    # the reports: the rows the regions list, the dropped ones left out
    probe = vs.allele_counts(dev)
    got = probe.allele_counts()
    table_rows = probe.layout()[1]
    probe.close()
    kept = np.concatenate([[0], np.cumsum((got["rows"]["count_flags"] >> 31) == 0)])
    b, c = got["row_begin"].astype(np.int64), got["row_count"].astype(np.int64)
    n_reports = int((kept[b + c] - kept[b]).sum())
    del got
    rng = np.random.default_rng(7)
    scores = [int(k) for k in args.scores.split(",")]
    kmax = max(scores)
    if args.weights == "max":
        w_all = np.full((n_reports, kmax), 1.0, np.float32)
    else:
        w_all = rng.standard_normal(size=(n_reports, kmax)).astype(np.float32)
        if args.weights == "small":
            w_all *= np.float32(0.01)
            w_all[0, :] = 4.0
    t_dev = torch.from_numpy(rng.standard_normal(size=(table_rows, kmax))).cuda() if "torch" in routes else None

    def matrix(k):
        wk = np.ascontiguousarray(w_all[:, :k])
        return lambda: [vs.score_matrix(dev, wk)]

    def batches(k):
        parts = [np.ascontiguousarray(w_all[:, j:j + 8]) for j in range(0, k, 8)]

        def call():
            out = []
            for p in parts:   # (each batch is closed as the next one is in flight: the route keeps one set of cells alive)
                out.append(vs.sample_scores(dev, p))
                if len(out) > 2:
                    done.append(out[0].fill_ms())
                    out.pop(0).close()
            return out
        done = []
        call.extra_fill = done
        return call

    def torch_route(k):
        def call():
            m = vs.genotype_matrix(dev)
            ptr, a, c, pitch = m.genotype_matrix_device()
            cells = torch.as_tensor(_DeviceBytes(ptr, a, pitch), device="cuda")[:, :c]
            dosage = (((cells >> 1) & 1) + ((cells >> 2) & 1)).to(torch.float64)
            out = dosage.T @ t_dev[:, :k]
            torch.cuda.synchronize()
            del out, dosage, cells
            return [m]
        return call

    legs, limbs = {}, {}
    for k in scores:
        if "matrix" in routes:
            legs[f"matrix_{k}"] = matrix(k)
        if "scores" in routes:
            legs[f"scores_{k}"] = batches(k)
        if "torch" in routes:
            legs[f"torch_{k}"] = torch_route(k)

    def loop(name, call, steps):
        fills = []
        extra = getattr(call, "extra_fill", None)
        t0 = time.perf_counter()
        for _ in range(steps):
            rs = call()
            f = sum(r.fill_ms() for r in rs)
            if extra is not None:
                f += sum(extra)
                extra.clear()
            fills.append(f)
            if name.startswith("matrix_") and name not in limbs:
                limbs[name] = rs[0].score_matrix()["limbs"]
            for r in rs:
                r.close()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps, fills

    steps_of = {}
    for k, call in legs.items():   # warm-up; it also sizes the leg's steps
        m, _ = loop(k, call, max(1, args.warmup))
        steps_of[k] = int(max(1, min(args.steps, args.budget_ms // max(m, 1e-3))))
    ms = {k: [] for k in legs}
    fills = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, call in legs.items():
            m, f = loop(k, call, steps_of[k])
            ms[k].append(m)
            fills[k] += [x for x in f if x >= 0]
    out = {"workload": args.workload, "regions_per_step": nreg, "overlap": args.overlap, "weights": args.weights, "chunk": args.chunk,
           "reps": args.reps, "table_rows": table_rows, "reports": n_reports, "samples": ns, "scores": scores, "build_s": round(t_build, 1),
           "limbs": limbs, "legs": {}}
    for k in legs:
        med = float(np.median(ms[k]))
        out["legs"][k] = {"steps": steps_of[k], "ms_per_step_median": round(med, 4), "ms_per_step_min": round(min(ms[k]), 4),
                          "ms_per_step_max": round(max(ms[k]), 4), "events_ms_median": round(float(np.median(fills[k])), 4) if fills[k] else None}
    leg = out["legs"]
    if "matrix" in routes:
        for other in ("scores", "torch"):
            if other in routes:
                out[f"{other}_over_matrix"] = {str(k): round(leg[f"{other}_{k}"]["ms_per_step_median"] / leg[f"matrix_{k}"]["ms_per_step_median"], 3) for k in scores}
    text = json.dumps(out)
    if args.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)
    vs.close()


if __name__ == "__main__":
    main()
