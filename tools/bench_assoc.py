"""Association scans on bench.py's workload (chr1-2504 by default), built the way bench.py builds it (its own functions, imported),
beside the two yardsticks of DESIGN 5g.  One handle; the legs alternate in one process, each a loop of --steps steps kept --depth
deep as bench.py's loop keeps them, repeated --reps times:

  counts_all / counts_sub   vs_query_allele_counts, whole cohort / the 1,252-sample subset (the scan runs the same kernel first)
  groups_2                  vs_query_group_counts at G = 2: the nearest kernel, one LDS look-up and one add per carrier
  dot_K / chi2_K            vs_query_assoc_scan over the whole cohort, K = 1, 4, 8
  dot_K_sub                 the same over a 1,252-sample subset
  dot_8_lds / dot_8_global  K = 8 with the phenotype table staged in LDS (assoc_lds_max_kib = 128) / read through global memory (1);
                            the same for the subset (_sub)
  matrix_route              the first --route-regions regions, whole cohort: vs_query_genotype_matrix, then on genotype_matrix_device()
                            in torch the cells to dosages (float32) and the product with Y (K = 8) -- the route the scan replaces;
                            scan_route: the scan over the same regions

Writes one JSON document (--out, default profiles/assoc_bench.json) and prints it: per leg ms per step (median, min, max over the
repeats), regions/s and the median of each batch's own kernel time (vs_result_fill_ms: for a scan k_allele_counts + k_assoc_scan).

    python tools/bench_assoc.py [--steps 20] [--reps 5] [--workload chr1-2504]
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

TRAITS = (1, 4, 8)


class _DeviceBytes:
    """(A, pitch) uint8 in device memory, for torch.as_tensor."""

    def __init__(self, ptr, a, pitch):
        self.__cuda_array_interface__ = {"shape": (a, pitch), "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": None}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assoc_bench.json"))
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
    n_route = min(args.route_regions, nreg)
    route_dev = DeviceArray(regions_dev.data_ptr(), n_route)
    rng = np.random.default_rng(7)
    sub = sorted(int(i) for i in rng.choice(np.arange(1, ns + 1), size=min(1_252, ns), replace=False))
    y_all = rng.standard_normal(size=(ns, 8)).astype(np.float32)
    y_sub = rng.standard_normal(size=(len(sub), 8)).astype(np.float32)
    label = rng.integers(0, 2, size=ns)
    members2 = [[int(i) + 1 for i in np.nonzero(label == k)[0]] for k in range(2)]
    y_dev = torch.from_numpy(y_all).cuda()

    def scan(k, stat, subset=False, kib=0, where=None):
        y, ids = (y_sub[:, :k], sub) if subset else (y_all[:, :k], None)

        def call():
            vs.set_option("assoc_lds_max_kib", kib)
            try:
                return [vs.assoc_scan(where or dev, y, ids, stat)]
            finally:
                vs.set_option("assoc_lds_max_kib", 0)
        return call

    def matrix_route():
        m = vs.genotype_matrix(route_dev)
        ptr, a, c, pitch = m.genotype_matrix_device()
        cells = torch.as_tensor(_DeviceBytes(ptr, a, pitch), device="cuda")[:, :c]
        dosage = (((cells >> 1) & 1) + ((cells >> 2) & 1)).to(torch.float32)
        scores = dosage @ y_dev
        torch.cuda.synchronize()
        del scores, dosage, cells
        return [m]

    legs = {"counts_all": lambda: [vs.allele_counts(dev)], "counts_sub": lambda: [vs.allele_counts(dev, sub)],
            "groups_2": lambda: [vs.group_counts(dev, members2)]}
    for k in TRAITS:
        legs[f"dot_{k}"] = scan(k, "dot")
        legs[f"chi2_{k}"] = scan(k, "chi2")
        legs[f"dot_{k}_sub"] = scan(k, "dot", subset=True)
    legs["dot_8_lds"] = scan(8, "dot", kib=128)
    legs["dot_8_global"] = scan(8, "dot", kib=1)
    legs["dot_8_sub_lds"] = scan(8, "dot", subset=True, kib=128)
    legs["dot_8_sub_global"] = scan(8, "dot", subset=True, kib=1)
    route = {"matrix_route": matrix_route, "scan_route": scan(8, "dot", where=route_dev)}

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
    probe = vs.allele_counts(dev)
    table_rows = probe.layout()[1]
    probe.close()
    probe = vs.allele_counts(route_dev)
    route_rows = probe.layout()[1]
    probe.close()
    out = {"workload": args.workload, "regions_per_step": nreg, "steps": args.steps, "reps": args.reps, "table_rows": table_rows,
           "samples": ns, "subset": len(sub), "route_regions": n_route, "route_rows": route_rows, "route_steps": args.route_steps,
           "build_s": round(t_build, 1), "legs": {}}
    for k in legs:
        med = float(np.median(ms[k]))
        n = n_route if k in route else nreg
        out["legs"][k] = {"ms_per_step_median": round(med, 4), "ms_per_step_min": round(min(ms[k]), 4), "ms_per_step_max": round(max(ms[k]), 4),
                          "regions_per_s": round(n / (med / 1e3)), "kernel_ms_median": round(float(np.median(fills[k])), 4) if fills[k] else None}
    leg = out["legs"]
    out["scan_kernel_ms"] = {k: round(leg[k]["kernel_ms_median"] - leg["counts_sub" if "sub" in k else "counts_all"]["kernel_ms_median"], 4)
                             for k in leg if k.startswith(("dot_", "chi2_"))}   # k_assoc_scan alone: the pair of events less k_allele_counts
    out["matrix_route_over_scan"] = round(leg["matrix_route"]["ms_per_step_median"] / leg["scan_route"]["ms_per_step_median"], 3)
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)
    vs.close()


if __name__ == "__main__":
    main()
