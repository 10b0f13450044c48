"""Trait-matrix association scans on the first --regions regions of bench.py's workload (chr1-2504 by default), built the way
bench.py builds it (its own functions, imported), beside the two routes of DESIGN 5l.  One handle; the legs alternate in one
process, each a loop of its steps kept --depth deep, repeated --reps times, after a warm-up:

  matrix_K[_sub]   vs_query_assoc_matrix, K = 8, 64, 512, 4096, whole cohort / the 1,252-sample subset, stat dot
  chi2_K           the same under chi2 (whole cohort)
  scan_K[_sub]     route (a): ceil(K / 8) vs_query_assoc_scan batches of 8 traits
  torch_K[_sub]    route (b): vs_query_genotype_matrix, then on genotype_matrix_device() in torch the cells to dosages (float64) and
                   the product with Y (float64)

Writes one JSON document (--out, default profiles/assocmatrix_bench.json) and prints it: per leg ms per step (median, min, max over
the repeats; the host's quantisation and limb panel are inside) and the median of each batch's own kernel time (vs_result_fill_ms:
k_allele_counts + k_genotype_matrix + k_assoc_matrix; for route (a) the sum over its batches).

    python tools/bench_assocmatrix.py [--steps 10] [--reps 3] [--traits 8,64,512,4096]
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
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--workload", default="chr1-2504", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--regions", type=int, default=10_000)
    ap.add_argument("--traits", default="8,64,512,4096")
    ap.add_argument("--budget-ms", type=float, default=1500.0, help="a leg's steps are cut so that one repeat stays near this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assocmatrix_bench.json"))
    args = ap.parse_args()
    import torch
    w = bench.WORKLOADS[args.workload]
    nreg = min(args.regions, w["regions"])
    regions = bench.make_regions(w, 0, w["regions"])[:nreg]
    t_build = time.perf_counter()
    vs = VariantStore.synthetic(device=0, **bench.synth_kwargs(w))
    t_build = time.perf_counter() - t_build
    ns = vs.info().num_samples - 1
    regions_dev = torch.from_numpy(np.ascontiguousarray(regions).astype(np.int64)).cuda().contiguous()
    torch.cuda.synchronize()
    dev = DeviceArray(regions_dev.data_ptr(), nreg)
    rng = np.random.default_rng(7)
    sub = sorted(int(i) for i in rng.choice(np.arange(1, ns + 1), size=min(1_252, ns), replace=False))
    traits = [int(k) for k in args.traits.split(",")]
    kmax = max(traits)
    y_all = rng.standard_normal(size=(ns, kmax)).astype(np.float32)
    y_sub = np.ascontiguousarray(y_all[np.asarray(sub) - 1])
    y_dev = {False: torch.from_numpy(y_all.astype(np.float64)).cuda(), True: torch.from_numpy(y_sub.astype(np.float64)).cuda()}

    def pick(k, subset):
        return (np.ascontiguousarray(y_sub[:, :k]), sub) if subset else (np.ascontiguousarray(y_all[:, :k]), None)

    def matrix(k, subset, stat="dot"):
        y, ids = pick(k, subset)
        return lambda: [vs.assoc_matrix(dev, y, ids, stat)]

    def scan(k, subset):
        y, ids = pick(k, subset)
        parts = [np.ascontiguousarray(y[:, j:j + 8]) for j in range(0, k, 8)]

        def call():
            out = []
            for p in parts:   # (each batch is closed as the next one is in flight: the route keeps one set of cells alive)
                out.append(vs.assoc_scan(dev, p, ids, "dot"))
                if len(out) > 2:
                    done.append(out[0].fill_ms())
                    out.pop(0).close()
            return out
        done = []
        call.extra_fill = done
        return call

    def torch_route(k, subset):
        ids = sub if subset else None

        def call():
            m = vs.genotype_matrix(dev, ids)
            ptr, a, c, pitch = m.genotype_matrix_device()
            cells = torch.as_tensor(_DeviceBytes(ptr, a, pitch), device="cuda")[:, :c]
            dosage = (((cells >> 1) & 1) + ((cells >> 2) & 1)).to(torch.float64)
            scores = dosage @ y_dev[subset][:, :k]
            torch.cuda.synchronize()
            del scores, dosage, cells
            return [m]
        return call

    legs = {}
    for k in traits:
        for subset in (False, True):
            tag = "_sub" if subset else ""
            legs[f"matrix_{k}{tag}"] = matrix(k, subset)
            legs[f"scan_{k}{tag}"] = scan(k, subset)
            legs[f"torch_{k}{tag}"] = torch_route(k, subset)
        legs[f"chi2_{k}"] = matrix(k, False, "chi2")

    def loop(call, steps):
        alive, fills = [], []
        extra = getattr(call, "extra_fill", None)

        def retire():
            rs = alive.pop(0)
            f = sum(r.fill_ms() for r in rs)
            if extra is not None:
                f += sum(extra)
                extra.clear()
            fills.append(f)
            for r in rs:
                r.close()

        t0 = time.perf_counter()
        for _ in range(steps):
            alive.append(call())
            if len(alive) >= (1 if extra is not None else args.depth):
                retire()
        while alive:
            retire()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps, fills

    steps_of = {}
    for k, call in legs.items():   # warm-up; it also sizes the leg's steps
        m, _ = loop(call, max(1, args.warmup))
        steps_of[k] = int(max(1, min(args.steps, args.budget_ms // max(m, 1e-3))))
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
    out = {"workload": args.workload, "regions_per_step": nreg, "reps": args.reps, "table_rows": table_rows, "samples": ns, "subset": len(sub),
           "traits": traits, "build_s": round(t_build, 1), "legs": {}}
    for k in legs:
        med = float(np.median(ms[k]))
        out["legs"][k] = {"steps": steps_of[k], "ms_per_step_median": round(med, 4), "ms_per_step_min": round(min(ms[k]), 4),
                          "ms_per_step_max": round(max(ms[k]), 4), "kernel_ms_median": round(float(np.median(fills[k])), 4) if fills[k] else None}
    leg = out["legs"]
    out["scan_over_matrix"] = {f"{k}{t}": round(leg[f"scan_{k}{t}"]["ms_per_step_median"] / leg[f"matrix_{k}{t}"]["ms_per_step_median"], 3)
                               for k in traits for t in ("", "_sub")}
    out["torch_over_matrix"] = {f"{k}{t}": round(leg[f"torch_{k}{t}"]["ms_per_step_median"] / leg[f"matrix_{k}{t}"]["ms_per_step_median"], 3)
                                for k in traits for t in ("", "_sub")}
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)
    vs.close()


if __name__ == "__main__":
    main()
