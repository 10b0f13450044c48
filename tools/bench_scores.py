"""Per-sample scores on bench.py's workload (chr1-2504 by default), built the way bench.py builds it (its own functions, imported),
beside the yardsticks of DESIGN 5h.  One handle; the legs alternate in one process, each a loop of --steps steps kept --depth deep as
bench.py's loop keeps them, repeated --reps times.  The weights lie in device memory (N x K float32 in report order, N of the order
of 2 x 10^7 for the 100 k x 10 kb batch: a host array would be uploaded every step):

  type6                     the type-6 step over the same regions
  burden_all / burden_sub   vs_query_sample_burden, whole cohort / the 1,252-sample subset: the same walk with every weight 1
  scores_K / scores_K_sub   vs_query_sample_scores at K = 1, 4, 8, standard-normal weights, whole cohort / the subset
  scores_8_sparse           K = 8 with weights on 1 % of the reports (a score file names few of a region's rows)
  matrix_route              the first --route-regions regions, whole cohort: vs_query_genotype_matrix, then on genotype_matrix_device()
                            in torch the cells to dosages (float32) and dosage^T @ W (K = 8) -- the route the query replaces;
                            scores_route: the query over the same regions

Writes one JSON document (--out, default profiles/scores_bench.json) and prints it: per leg ms per step (median, min, max over the
repeats), regions/s and the median of each batch's own pair of events (vs_result_fill_ms: offsets, scale, the host wait, integer
weights, the walk, the scores).

    python tools/bench_scores.py [--steps 20] [--reps 5] [--workload chr1-2504]
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

SCORES = (1, 4, 8)


class _DeviceBytes:
    """(A, pitch) uint8 in device memory, for torch.as_tensor."""

    def __init__(self, ptr, a, pitch):
        self.__cuda_array_interface__ = {"shape": (a, pitch), "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": None}


def reports(vs, regions):
    """(N, table rows) of a batch: the rows its regions report, dropped ones left out."""
    c = vs.allele_counts(regions)
    got = c.allele_counts()
    c.close()
    dropped = np.concatenate([[0], np.cumsum((got["rows"]["count_flags"] >> 31) != 0)])
    b, n = got["row_begin"].astype(np.int64), got["row_count"].astype(np.int64)
    return int((n - (dropped[b + n] - dropped[b])).sum()), got["rows"].shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--workload", default="chr1-2504", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--regions", type=int, default=0)
    ap.add_argument("--route-regions", type=int, default=10_000)
    ap.add_argument("--route-steps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=0, help="option score_chunk (0: the default)")
    ap.add_argument("--tile-cols", type=int, default=0, help="option score_tile_cols (0: the default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scores_bench.json"))
    args = ap.parse_args()
    import torch
    w = bench.WORKLOADS[args.workload]
    nreg = args.regions or w["regions"]
    regions = bench.make_regions(w, 0, nreg)
    t_build = time.perf_counter()
    vs = VariantStore.synthetic(device=0, **bench.synth_kwargs(w))
    t_build = time.perf_counter() - t_build
    vs.set_option("score_chunk", args.chunk)
    vs.set_option("score_tile_cols", args.tile_cols)
    ns = vs.info().num_samples - 1
    regions_dev = torch.from_numpy(regions.astype(np.int64)).cuda().contiguous()
    torch.cuda.synchronize()
    dev = DeviceArray(regions_dev.data_ptr(), nreg)
    n_route = min(args.route_regions, nreg)
    route_dev = DeviceArray(regions_dev.data_ptr(), n_route)
    rng = np.random.default_rng(7)
    sub = sorted(int(i) for i in rng.choice(np.arange(1, ns + 1), size=min(1_252, ns), replace=False))
    n_rep, table_rows = reports(vs, regions)
    n_rep_route, route_rows = reports(vs, regions[:n_route])
    gen = torch.Generator(device="cuda").manual_seed(7)
    w_dev = {k: torch.randn((n_rep, k), generator=gen, device="cuda", dtype=torch.float32) for k in SCORES}
    w_sparse = w_dev[8] * (torch.rand((n_rep, 1), generator=gen, device="cuda") < 0.01)
    w_route = torch.randn((n_rep_route, 8), generator=gen, device="cuda", dtype=torch.float32)
    w_table = torch.randn((route_rows, 8), generator=gen, device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()
    names = {k: [str(i) for i in range(k)] for k in SCORES}

    def scores(t, k, ids=None, where=None):
        return lambda: [vs.sample_scores(where or dev, DeviceArray(t.data_ptr(), t.numel()), ids, names[k])]

    def matrix_route():
        m = vs.genotype_matrix(route_dev)
        ptr, a, c, pitch = m.genotype_matrix_device()
        cells = torch.as_tensor(_DeviceBytes(ptr, a, pitch), device="cuda")[:, :c]
        dosage = (((cells >> 1) & 1) + ((cells >> 2) & 1)).to(torch.float32)
        out = dosage.T @ w_table
        torch.cuda.synchronize()
        del out, dosage, cells
        return [m]

    legs = {"type6": lambda: [vs.get_var_in_ref_device(dev.ptr, nreg)], "burden_all": lambda: [vs.sample_burden(dev)], "burden_sub": lambda: [vs.sample_burden(dev, sub)]}
    for k in SCORES:
        legs[f"scores_{k}"] = scores(w_dev[k], k)
        legs[f"scores_{k}_sub"] = scores(w_dev[k], k, sub)
    legs["scores_8_sparse"] = scores(w_sparse, 8)
    route = {"matrix_route": matrix_route, "scores_route": scores(w_route, 8, where=route_dev)}

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

    steps_of = {k: args.steps for k in legs}
    steps_of.update({k: args.route_steps for k in route})
    legs.update(route)
    for k, call in legs.items():
        loop(call, min(args.warmup, steps_of[k]))
    ms = {k: [] for k in legs}
    fills = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, call in legs.items():
            m, f = loop(call, steps_of[k])
            ms[k].append(m)
            fills[k] += [x for x in f if x >= 0]
    out = {"workload": args.workload, "regions_per_step": nreg, "steps": args.steps, "reps": args.reps, "table_rows": table_rows,
           "reports": n_rep, "samples": ns, "subset": len(sub), "route_regions": n_route, "route_rows": route_rows,
           "route_reports": n_rep_route, "route_steps": args.route_steps, "score_chunk": args.chunk, "score_tile_cols": args.tile_cols,
           "build_s": round(t_build, 1), "legs": {}}
    for k in legs:
        med = float(np.median(ms[k]))
        n = n_route if k in route else nreg
        out["legs"][k] = {"ms_per_step_median": round(med, 4), "ms_per_step_min": round(min(ms[k]), 4), "ms_per_step_max": round(max(ms[k]), 4),
                          "regions_per_s": round(n / (med / 1e3)), "kernel_ms_median": round(float(np.median(fills[k])), 4) if fills[k] else None}
    leg = out["legs"]
    out["matrix_route_over_scores"] = round(leg["matrix_route"]["ms_per_step_median"] / leg["scores_route"]["ms_per_step_median"], 3)
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)
    vs.close()


if __name__ == "__main__":
    main()
