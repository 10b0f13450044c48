"""LD clumping queries (vs_query_ld_clump) on bench.py's cohort (chr1-2504 by default), built the way bench.py builds it (its own
functions, imported), beside the pruning query on the same batch and the route the query replaces.  One handle; per leg and p-value
family the calls alternate in one process, each a loop of --steps calls, repeated --reps times.  The two legs of tools/bench_prune.py,
both over the whole cohort:

  regions  --regions regions of the bench's own length (10 kb, about 200 rows each): one workgroup per region
  one      ONE region of --one-len bases (about as many rows as the other leg's table): one workgroup walks all of it

and two p-value families:

  uniform  uniform random p-values, --p1 / --p2 (1e-4 / 1e-2): the usage -- few rows lead, the rounds are few
  ordered  p increasing in table order, p1 = p2 = 1: every row is a candidate and the priority is the table's order -- the forward
           greedy of ld_prune, the worst case for the rounds

Per leg and family it records ms per call (median, min, max over the repeats) and the median of the batch's own kernel time
(vs_result_fill_ms) of ld_clump, and per leg of ld_prune on the same batch, window and bound; the rounds the regions took (the
kernel's diagnostic: max and median); and the route without the query, run once with its parts: ld_band(stat="r2") -> the band
copied to the host -> the sequential clumping in numpy (float r2 > bound where the query compares integers), and how many verdicts
and owners of that route differ from the query's.

Prints one JSON line and writes it to --out (profiles/clump_bench.json).

    python tools/bench_clump.py [--steps 3] [--reps 3] [--workload chr1-2504]
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
from variantstore_amd import VariantStore, pvalue_keys, quantise_r2  # noqa: E402

NO_OWNER = 0xFFFFFFFF


def host_clump(band, counts, dropped, n, row_begin, row_count, bound, keys, key1, key2):
    """The sequential clumping on the host from the float band: (state, owner per reported row, seconds).  One numpy operation
    each way per index row."""
    t0 = time.perf_counter()
    window = band.shape[1]
    ac = counts["alt_alleles"].astype(np.int64)
    v = np.int64(n) * (ac + 2 * counts["hom_alt"].astype(np.int64)) - ac * ac
    cand = ~dropped & (v > 0) & (keys <= np.uint64(key2))
    lead = cand & (keys <= np.uint64(key1))
    code = np.where(dropped, 3, 2).astype(np.uint8)
    hits = band > np.float32(bound)
    states, owners = [], []
    for a0, m in zip(row_begin.tolist(), row_count.tolist()):
        st, own = code[a0:a0 + m].copy(), np.full(m, NO_OWNER, np.uint32)
        free = cand[a0:a0 + m].copy()
        leads = np.nonzero(lead[a0:a0 + m])[0]
        for x in leads[np.lexsort((leads, keys[a0 + leads]))].tolist():
            if not free[x]:
                continue
            st[x], own[x], free[x] = 1, x, False
            hi = min(m, x + 1 + window)
            fwd = x + 1 + np.nonzero(hits[a0 + x, :hi - x - 1] & free[x + 1:hi])[0]
            j = np.arange(max(0, x - window), x)
            back = j[hits[a0 + j, x - j - 1] & free[j]]
            for got in (fwd, back):
                st[got], own[got], free[got] = 0, x, False
        st[free] = 4
        states.append(st)
        owners.append(own)
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dt)   # noqa: E731
    return cat(states, np.uint8), cat(owners, np.uint32), time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--regions", type=int, default=2000)
    ap.add_argument("--one-len", type=int, default=20_000_000)
    ap.add_argument("--window", type=int, default=256)
    ap.add_argument("--r2", type=float, default=0.5)
    ap.add_argument("--p1", type=float, default=1e-4)
    ap.add_argument("--p2", type=float, default=1e-2)
    ap.add_argument("--legs", default="regions,one")
    ap.add_argument("--families", default="uniform,ordered")
    ap.add_argument("--workload", default="chr1-2504", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clump_bench.json"))
    args = ap.parse_args()
    w = bench.WORKLOADS[args.workload]
    t0 = time.perf_counter()
    vs = VariantStore.synthetic(device=0, **bench.synth_kwargs(w))
    build_s = time.perf_counter() - t0
    n_cols = vs.info().num_samples - 1
    threshold = quantise_r2(args.r2)
    bound = threshold / (1 << 20)
    mid = (w["first_pos"] + w["ref_length"]) // 2
    all_legs = {"regions": np.ascontiguousarray(bench.make_regions(w, 0, w["regions"])[:: max(1, w["regions"] // args.regions)][: args.regions]),
                "one": np.asarray([[mid - args.one_len // 2, mid + args.one_len // 2]], np.uint64)}
    legs = {k: all_legs[k] for k in args.legs.split(",")}

    def fill_ms(r):
        ms = r.fill_ms()   # (waits for the batch)
        r.close()
        return ms

    def timed(call, steps):
        t0 = time.perf_counter()
        extra = [call() for _ in range(steps)]
        return (time.perf_counter() - t0) * 1e3 / steps, extra

    def stats(ms):
        return {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}

    out = {"workload": args.workload, "steps": args.steps, "reps": args.reps, "build_s": round(build_s, 1), "window": args.window, "r2": args.r2,
           "threshold_q20": threshold, "max_bp": 0, "legs": {}}
    for name, reg in legs.items():
        probe = vs.allele_counts(reg)
        rows = int(probe.allele_counts()["rows"].shape[0])
        probe.close()
        families = {"uniform": (np.random.default_rng(77).random(rows), args.p1, args.p2), "ordered": ((np.arange(rows) + 1.0) / (rows + 1.0), 1.0, 1.0)}
        families = {k: families[k] for k in args.families.split(",")}
        calls = {"ld_prune": lambda: fill_ms(vs.ld_prune(reg, window=args.window, r2=args.r2))}
        for fam, (p, p1, p2) in families.items():
            calls["ld_clump_" + fam] = lambda p=p, p1=p1, p2=p2: fill_ms(vs.ld_clump(reg, p, window=args.window, r2=args.r2, max_bp=0, p1=p1, p2=p2))
        for c in calls.values():
            timed(c, args.warmup)
        ms = {k: [] for k in calls}
        extra = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, c in calls.items():
                m, e = timed(c, args.steps)
                ms[k].append(m)
                extra[k] += e
        # the route without the query: the band once (it does not depend on the p-values), the clumping per family
        t = [time.perf_counter()]
        r = vs.ld_band(reg, window=args.window, stat="r2")
        r.fill_ms()
        t.append(time.perf_counter())
        band = r.ld_band()   # the copy: rows x window x 4 bytes over the link
        r.close()
        t.append(time.perf_counter())
        dropped = (band["rows"]["count_flags"] >> 31) != 0
        leg = {"regions": int(reg.shape[0]), "rows": rows, "columns": int(n_cols), "ld_prune_ms_per_call": stats(ms["ld_prune"]),
               "ld_prune_fill_ms": round(float(np.median(extra["ld_prune"])), 4),
               "host_route_shared_ms": {"ld_band_query": round((t[1] - t[0]) * 1e3, 3), "band_to_host": round((t[2] - t[1]) * 1e3, 3)}, "families": {}}
        for fam, (p, p1, p2) in families.items():
            one = vs.ld_clump(reg, p, window=args.window, r2=args.r2, max_bp=0, p1=p1, p2=p2)
            got = one.ld_clump()
            one.close()
            keys = pvalue_keys(p)
            hstate, howner, secs = host_clump(band["band"], band["counts"], dropped, n_cols, band["row_begin"].astype(np.int64),
                                              band["row_count"].astype(np.int64), bound, keys, int(pvalue_keys(p1)), int(pvalue_keys(p2)))
            k = "ld_clump_" + fam
            states = int(got["state"].shape[0])
            words = (args.window + 31) // 32
            f = {"p1": p1, "p2": p2, "verdicts": states, "index": int(got["n_index"].sum()), "member": int((got["state"] == 0).sum()),
                 "unclumped": int((got["state"] == 4).sum()), "ineligible": int((got["state"] == 2).sum()),
                 "rounds_max": int(got["rounds"].max()), "rounds_median": float(np.median(got["rounds"])),
                 "ms_per_call": stats(ms[k]), "fill_ms": round(float(np.median(extra[k])), 4),
                 "blocker_bytes": states * 8 * words, "key_bytes": rows * 8,
                 "vs_ld_prune": round(float(np.median(ms[k])) / float(np.median(ms["ld_prune"])), 3),
                 "host_numpy_clump_ms": round(secs * 1e3, 2),
                 "host_route_ms": round((t[2] - t[0]) * 1e3 + secs * 1e3, 2),
                 "host_route_verdicts_that_differ": int((hstate != got["state"]).sum()), "host_route_owners_that_differ": int((howner != got["owner"]).sum())}
            leg["families"][fam] = f
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
