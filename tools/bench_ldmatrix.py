"""LD-matrix queries (vs_query_ld_matrix) on bench.py's cohort (chr1-2504 by default), built the way bench.py builds it (its own
functions, imported), beside the band query and the torch path they replace.  One handle; per leg the calls alternate in one process,
each a loop of --steps calls, repeated --reps times.  Three legs, all over the whole cohort:

  small    --small-regions regions of the bench's own length (10 kb, about 200 rows each)
  medium   --medium-regions loci of --medium-len bases (about 1,000 rows each)
  large    --large-regions loci of --large-len bases (several thousand rows each)

Per leg and call -- ld_matrix (r^2 and dot), ld_band at window 256, allele_counts, genotype_matrix, torch -- it records ms per call
(median, min, max over the repeats) and the median of the batch's own kernel time (vs_result_fill_ms); from them
  stage_ms                 the block kernel alone: the LD-matrix batch's kernel time minus the counts' and the matrix query's on the
                           same batch (an LD-matrix batch runs those two kernels, then k_ld_block); band_stage_ms likewise
  stage_ns_per_cell        stage time per stored cell, for the blocks (sum of m^2) and for the band (rows x 256)
  ld_matrix_vs_torch       this query / the torch path: genotype_matrix_device() -> dosages as float32 -> one D_q @ D_q.T per region,
                           then the r^2 arithmetic in float64 (the three stages' times are recorded as well)
and the arithmetic of the kernel's traffic: panel bytes read, m^2 pitch / 64 per region summed, against 4 m^2 bytes written.

Prints one JSON line and writes it to --out (profiles/ldmatrix_bench.json).

    python tools/bench_ldmatrix.py [--steps 5] [--reps 3] [--workload chr1-2504]
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

TILE = 64   # kLdBlockTile of k_ld_block.hip.h


class _DeviceBytes:
    """rows x pitch bytes of device memory for torch.as_tensor."""

    def __init__(self, ptr, rows, pitch):
        self.__cuda_array_interface__ = {"shape": (rows, pitch), "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small-regions", type=int, default=2000)
    ap.add_argument("--medium-regions", type=int, default=200)
    ap.add_argument("--medium-len", type=int, default=50_000)
    ap.add_argument("--large-regions", type=int, default=6)
    ap.add_argument("--large-len", type=int, default=250_000)
    ap.add_argument("--legs", default="small,medium,large")
    ap.add_argument("--workload", default="chr1-2504", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldmatrix_bench.json"))
    args = ap.parse_args()
    import torch
    w = bench.WORKLOADS[args.workload]
    t0 = time.perf_counter()
    vs = VariantStore.synthetic(device=0, **bench.synth_kwargs(w))
    build_s = time.perf_counter() - t0
    rng = np.random.default_rng(21)

    def loci(n, length):
        s = np.sort(rng.integers(w["first_pos"], w["ref_length"] - length, size=n, dtype=np.int64))
        return np.stack([s, s + length], axis=1).astype(np.uint64)

    all_legs = {"small": np.ascontiguousarray(bench.make_regions(w, 0, w["regions"])[:: max(1, w["regions"] // args.small_regions)][: args.small_regions]),
                "medium": loci(args.medium_regions, args.medium_len), "large": loci(args.large_regions, args.large_len)}
    legs = {k: all_legs[k] for k in args.legs.split(",")}

    def fill_ms(r):
        ms = r.fill_ms()   # (waits for the batch)
        r.close()
        return ms

    via_host = [False]

    def torch_path(reg):
        t = [time.perf_counter()]
        r = vs.genotype_matrix(reg)
        ptr, rows, cols, pitch = r.genotype_matrix_device()
        raw = r.raw(with_carriers=False)
        begin, count = raw["row_begin"].astype(np.int64), raw["row_count"].astype(np.int64)
        t.append(time.perf_counter())
        if rows:
            try:
                cells = torch.as_tensor(_DeviceBytes(ptr, rows, pitch), device="cuda")[:, :cols]
            except (TypeError, RuntimeError, ValueError):   # this torch does not take the interface: through the host (slower: said in the output)
                via_host[0] = True
                cells = torch.from_numpy(np.ascontiguousarray(r.genotype_matrix()["cells"])).cuda()
            d = (((cells >> 1) & 1) + ((cells >> 2) & 1)).to(torch.float32)
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            n = float(cols)
            sx = d.sum(dim=1, dtype=torch.float64)
            v = n * (d * d).sum(dim=1, dtype=torch.float64) - sx * sx
            outs = []
            for b, c in zip(begin.tolist(), count.tolist()):
                dq = d[b:b + c]
                g = (dq @ dq.T).to(torch.float64)
                cov = n * g - sx[b:b + c, None] * sx[None, b:b + c]
                den = v[b:b + c, None] * v[None, b:b + c]
                outs.append(torch.where(den != 0, cov * cov / torch.where(den != 0, den, torch.ones_like(den)), torch.zeros_like(den)).to(torch.float32))
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            del outs, d, cells
        else:
            t += [t[-1], t[-1]]
        r.close()
        return [(b - a) * 1e3 for a, b in zip(t[:-1], t[1:])]

    def timed(call, steps):
        t0 = time.perf_counter()
        extra = [call() for _ in range(steps)]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps, extra

    out = {"workload": args.workload, "steps": args.steps, "reps": args.reps, "build_s": round(build_s, 1), "tile": TILE, "legs": {}}
    for name, reg in legs.items():
        calls = {"ld_matrix_r2": lambda: fill_ms(vs.ld_matrix(reg, stat="r2")), "ld_matrix_dot": lambda: fill_ms(vs.ld_matrix(reg, stat="dot")),
                 "ld_band_w256": lambda: fill_ms(vs.ld_band(reg, window=256, stat="r2")), "counts": lambda: fill_ms(vs.allele_counts(reg)),
                 "matrix": lambda: fill_ms(vs.genotype_matrix(reg)), "torch": lambda: torch_path(reg)}
        for c in calls.values():
            timed(c, args.warmup)
        ms = {k: [] for k in calls}
        extra = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, c in calls.items():
                m, e = timed(c, args.steps)
                ms[k].append(m)
                extra[k] += e
        one = vs.ld_matrix(reg)
        _pc, _pb, _pn, nq, rows, cols, _st = one.ld_matrix_device()
        mq = one.raw(with_carriers=False)["row_count"].astype(np.int64)
        one.close()
        pitch = (cols + 15) // 16 * 16
        cells = int((mq * mq).sum())
        tiles = (mq + TILE - 1) // TILE
        pairs = int((tiles * (tiles + 1) // 2).sum())
        diag = int(tiles.sum())
        leg = {"regions": int(nq), "rows": int(rows), "columns": int(cols), "row_pitch": int(pitch), "rows_per_region_median": int(np.median(mq)),
               "rows_per_region_max": int(mq.max()) if mq.size else 0, "cells": cells, "cell_bytes": 4 * cells, "matrix_bytes": int(rows * pitch),
               "workgroups": pairs, "panel_bytes_read": int((2 * pairs - diag) * TILE * pitch), "band_cells": int(rows) * 256}
        for k in calls:
            leg[k + "_ms_per_call"] = {"median": round(float(np.median(ms[k])), 4), "min": round(min(ms[k]), 4), "max": round(max(ms[k]), 4)}
        kern = {k: float(np.median(extra[k])) for k in calls if k != "torch"}
        leg["kernel_ms"] = {k: round(v, 4) for k, v in kern.items()}
        for stat in ("r2", "dot"):
            stage = kern["ld_matrix_" + stat] - kern["counts"] - kern["matrix"]
            leg["stage_ms_" + stat] = round(stage, 4)
            if cells and stage > 0:
                leg["stage_ns_per_cell_" + stat] = round(stage * 1e6 / cells, 5)
                leg["stage_store_GBps_" + stat] = round(4 * cells / stage / 1e6, 1)
        band_stage = kern["ld_band_w256"] - kern["counts"] - kern["matrix"]
        leg["band_stage_ms"] = round(band_stage, 4)
        if rows and band_stage > 0:
            leg["band_stage_ns_per_cell"] = round(band_stage * 1e6 / (rows * 256), 5)
            if "stage_ns_per_cell_r2" in leg:
                leg["stage_per_cell_vs_band"] = round(leg["stage_ns_per_cell_r2"] / leg["band_stage_ns_per_cell"], 3)
        tp = np.median(np.asarray(extra["torch"]), axis=0)
        leg["torch_stage_ms"] = {"matrix_query": round(float(tp[0]), 4), "to_float_dosages": round(float(tp[1]), 4), "products_and_r2": round(float(tp[2]), 4)}
        leg["ld_matrix_vs_torch"] = round(leg["ld_matrix_r2_ms_per_call"]["median"] / leg["torch_ms_per_call"]["median"], 3)
        leg["ld_matrix_vs_ld_band_w256"] = round(leg["ld_matrix_r2_ms_per_call"]["median"] / leg["ld_band_w256_ms_per_call"]["median"], 3)
        out["legs"][name] = leg
    out["torch_matrix_via_host"] = via_host[0]
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    vs.close()


if __name__ == "__main__":
    main()
