"""Banded LD queries against type 6 and the genotype-matrix query on bench.py's workload (chr1-2504 by default), built the way
bench.py builds it (its own functions, imported).  One handle; the legs alternate in one process, each a loop of --steps batches
kept --depth deep as bench.py's loop keeps them, repeated --reps times:

  type6                 vs_query_var_in_ref_device
  ld_all_10k_w64        vs_query_ld_band, r^2, the whole cohort, the first --whole-regions regions of the batch, W = 64
  ld_1252_w64           ... r^2, a 1,252-sample subset (half the cohort), the whole batch, W = 64
  ld_100_w16 / _w256    ... r^2, a 100-sample subset, the whole batch, W = 16 and W = 256
  matrix_*              vs_query_genotype_matrix over the same regions and samples as each LD leg: the step the LD step is held
                        against (the LD batch runs the same matrix kernel into a temporary, the count kernel and the band kernel)

Prints one JSON line and writes it to --out (profiles/ld_bench.json): ms per step (median, min, max over the repeats), regions/s,
the median of each batch's own kernel time (vs_result_fill_ms: an LD batch's three kernels together -- a kernel trace splits them),
per LD leg its rows, pitch, window and bytes, the ratio LD step / matrix step, and the two floors of the band kernel:
  bytes   the matrix read (R + W) / R times (R = 64 rows a workgroup, the halo rounded up to 16) plus the band written, at the copy
          rate tools/microbench/hbm_ceiling --quick reports on this box (--copy-tbps overrides)
  mfma    A / 16 row tiles x ((W + 15) / 16 + 1) column tiles x pitch / 64 instructions of v_mfma_i32_16x16x64_i8 at --mfma-cycles
          cycles per instruction and SIMD (16: the cycles of the bf16 16x16x32 form at twice its K), 4 SIMDs a CU, --cus x --mhz

    python tools/bench_ld.py [--steps 10] [--reps 3] [--workload chr1-2504]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # (as bench.py: the plan and the batch run on two streams)
# (where the variable is not set already this takes effect, and every leg -- type 6, matrix_* and ld_* alike -- then runs with more
#  hardware queues than the engine's tests use: compare legs of one run with each other, not with timings taken elsewhere)

import numpy as np  # noqa: E402

import bench  # noqa: E402
from variantstore_amd import DeviceArray, VariantStore  # noqa: E402

LD_ROWS = 64   # kLdRows of k_ld.hip.h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--workload", default="chr1-2504", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--regions", type=int, default=0)
    ap.add_argument("--whole-regions", type=int, default=10_000)
    ap.add_argument("--copy-tbps", type=float, default=0.0, help="0: measure with tools/microbench/hbm_ceiling, 6.4 when it is not built")
    ap.add_argument("--cus", type=int, default=256)
    ap.add_argument("--mhz", type=float, default=2400.0)
    ap.add_argument("--mfma-cycles", type=float, default=16.0, help="cycles of one v_mfma_i32_16x16x64_i8 on a SIMD")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ld_bench.json"))
    args = ap.parse_args()
    box = None if args.copy_tbps else bench.box_ceilings()   # (a child process, before this one touches the GPU)
    copy = args.copy_tbps or (box["copy_1to1_GBps"] / 1e3 if box and box.get("copy_1to1_GBps") else 0.0)
    copy_from = "argument" if args.copy_tbps else "hbm_ceiling --quick: copy_1to1" if copy else "assumed"
    copy = copy or 6.4
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
    ptr = regions_dev.data_ptr()
    rng = np.random.default_rng(7)
    sub100 = [int(i) for i in np.sort(rng.choice(np.arange(1, ns + 1), size=min(100, ns), replace=False))]
    sub_half = [int(i) for i in np.sort(rng.choice(np.arange(1, ns + 1), size=ns // 2, replace=False))]
    dev = DeviceArray(ptr, nreg)
    n_whole = min(args.whole_regions, nreg)
    dev_whole = DeviceArray(ptr, n_whole)
    k_half, k_whole = f"{len(sub_half)}", f"all_{n_whole // 1000}k"
    legs = {
        "type6": (lambda: vs.get_var_in_ref_device(ptr, nreg), nreg, None),
        f"ld_{k_whole}_w64": (lambda: vs.ld_band(dev_whole, None, window=64), n_whole, "matrix_" + k_whole),
        "matrix_" + k_whole: (lambda: vs.genotype_matrix(dev_whole), n_whole, None),
        f"ld_{k_half}_w64": (lambda: vs.ld_band(dev, sub_half, window=64), nreg, "matrix_" + k_half),
        "matrix_" + k_half: (lambda: vs.genotype_matrix(dev, sub_half), nreg, None),
        "ld_100_w16": (lambda: vs.ld_band(dev, sub100, window=16), nreg, "matrix_100"),
        "ld_100_w256": (lambda: vs.ld_band(dev, sub100, window=256), nreg, "matrix_100"),
        "matrix_100": (lambda: vs.genotype_matrix(dev, sub100), nreg, None),
    }

    def loop(call, steps):
        alive, fills = [], []
        t0 = time.perf_counter()
        for _ in range(steps):
            alive.append(call())
            if len(alive) >= args.depth:
                r = alive.pop(0)
                fills.append(r.fill_ms())
                r.close()
        while alive:
            r = alive.pop(0)
            fills.append(r.fill_ms())
            r.close()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps, fills

    for call, _n, _m in legs.values():
        loop(call, args.warmup)
    ms = {k: [] for k in legs}
    fills = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, (call, _n, _m) in legs.items():
            m, f = loop(call, args.steps)
            ms[k].append(m)
            fills[k] += [x for x in f if x >= 0]
    mfma_per_s = args.cus * 4 * args.mhz * 1e6 / args.mfma_cycles
    out = {"workload": args.workload, "regions_per_step": nreg, "steps": args.steps, "reps": args.reps, "copy_tbps": copy,
           "copy_from": copy_from, "box_ceilings": box, "mfma_i8_16x16x64_per_s": mfma_per_s, "build_s": round(t_build, 1), "legs": {}}
    for k, (call, n, _m) in legs.items():
        med = float(np.median(ms[k]))
        leg = {"ms_per_step_median": round(med, 4), "ms_per_step_min": round(min(ms[k]), 4), "ms_per_step_max": round(max(ms[k]), 4),
               "regions": n, "regions_per_s": round(n / (med / 1e3)), "kernel_ms_median": round(float(np.median(fills[k])), 4) if fills[k] else None}
        if k.startswith("ld_"):
            one = call()
            _pb, _pc, rows, cols, window, stat = one.ld_band_device()
            one.close()
            pitch = (cols + 15) // 16 * 16
            tiles = (window + 15) // 16 + 1
            read = rows * pitch * (LD_ROWS + 16 * (tiles - 1)) / LD_ROWS
            band = rows * window * 4
            mfma = (rows + 15) // 16 * tiles * ((pitch + 63) // 64)
            leg.update(rows=rows, columns=cols, row_pitch=pitch, window=window, stat=stat, matrix_bytes=rows * pitch, band_bytes=band,
                       band_kernel_read_bytes=int(read), band_kernel_mfma=mfma,
                       band_bytes_floor_ms=round((read + band) / (copy * 1e12) * 1e3, 4),
                       band_mfma_floor_ms=round(mfma / mfma_per_s * 1e3, 4))
        out["legs"][k] = leg
    for k, (_call, _n, against) in legs.items():
        if against:
            out["legs"][k]["step_vs_matrix_step"] = round(out["legs"][k]["ms_per_step_median"] / out["legs"][against]["ms_per_step_median"], 3)
            if out["legs"][k]["kernel_ms_median"] and out["legs"][against]["kernel_ms_median"]:
                out["legs"][k]["kernels_vs_matrix_kernel"] = round(out["legs"][k]["kernel_ms_median"] / out["legs"][against]["kernel_ms_median"], 3)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    vs.close()


if __name__ == "__main__":
    main()
