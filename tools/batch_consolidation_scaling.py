"""How a batch of independent consolidations scales with the number of clusters.

One gs_consolidate_rerun launches K1/K2, the simulation kernel and K3 for one
cluster, synchronises and copies back; gs_batch_consolidate_run launches the
same kernels once per group for every cluster of a batch.  For N = 1, 4, 16,
64, 256, 1024 C1-sized clusters (24 nodes, one SINGLE simulation per node, a
handful of pods each; 16 distinct clusters taken in turn), in three
alternating repetitions per leg (ranges reported, as DESIGN does):

  (a) batch_ms   gs_batch_consolidate_run wall (median of --steps runs) and
                 device_ms (first to last batched kernel, HIP events)
  (b) fetch_ms   gs_batch_consolidate_fetch of all N slots after one run (the
                 copies back and the decisions, which a rerun includes)
  (b') fetch_all_ms  gs_batch_consolidate_fetch_all after one run: the same N
                 decided tables from one device pass (two launches per group,
                 one transfer; two in the warm-up call) instead of five copies
                 and one synchronisation per slot
  (c) serial_ms  the comparison that counts: the same N clusters resident on
                 ordinary contexts, N gs_consolidate_rerun calls in turn (at
                 most 64 contexts, reused in turn for larger N: a rerun does
                 the same work on whichever context holds the cluster)

(a) + (b), or (a) + (b'), is what a caller pays for N decided tables; (c)
includes both parts.  Slot 0 and the last slot of every batch are compared
with the rerun of the same cluster, and fetch_all's tables with the per-slot
fetch's.  Run on the GPU box:
  python tools/batch_consolidation_scaling.py --out profiles/r7/batch_consolidation_fetch_all.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "karpenter-provider-ibm-cloud_amd"))
sys.path.insert(0, ROOT)

from gpusched import abi, synth  # noqa: E402
from gpusched.consolidation import ConsolidationInput  # noqa: E402
from gpusched.lib import Solver  # noqa: E402

MAX_CONTEXTS = 64
DISTINCT = 16


def rng(xs):
    return [round(min(xs), 4), round(max(xs), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,4,16,64,256,1024")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    clusters = [synth.random_consolidation(200 + s, n_nodes=24, n_pending=s % 3) for s in range(DISTINCT)]
    inputs = [ConsolidationInput(p, list(range(len(p.nodes))), mode=abi.CONSOLIDATE_SINGLE) for p in clusters]
    rows = []
    batch = Solver(0)
    singles = []
    try:
        for n in [int(x) for x in args.sizes.split(",") if x]:
            while len(singles) < min(n, MAX_CONTEXTS):
                singles.append(Solver(0))
            ctxs = singles[:min(n, MAX_CONTEXTS)]
            for k, s in enumerate(ctxs):
                s.consolidate(inputs[k % DISTINCT])
            status = batch.batch_consolidate_prepare([inputs[i % DISTINCT] for i in range(n)])
            assert status == [abi.GS_OK] * n
            batch.batch_consolidate_run()
            # the first fetch_all of a larger batch grows the staging buffers: timed apart, and the warm-up
            t0 = time.perf_counter()
            batch.batch_consolidate_fetch_all(raw=True)
            fa_first = (time.perf_counter() - t0) * 1e3
            a_wall, a_dev, f_wall, fa_wall, b_wall = [], [], [], [], []
            for _ in range(args.reps):
                w, d = [], []
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    batch.batch_consolidate_run()
                    w.append((time.perf_counter() - t0) * 1e3)
                    d.append(batch.batch_consolidate_stats()["device_ms"])
                a_wall.append(statistics.median(w))
                a_dev.append(statistics.median(d))
                t0 = time.perf_counter()
                for i in range(n):
                    batch.batch_consolidate_fetch(i, raw=True)
                f_wall.append((time.perf_counter() - t0) * 1e3)
                batch.batch_consolidate_run()  # the tables are the run's: none is cached
                t0 = time.perf_counter()
                batch.batch_consolidate_fetch_all(raw=True)
                fa_wall.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                for i in range(n):
                    ctxs[i % len(ctxs)].consolidate_rerun(raw=True)
                b_wall.append((time.perf_counter() - t0) * 1e3)
            stats = batch.batch_consolidate_stats()
            exact = all(batch.batch_consolidate_fetch(i)[:3] == ctxs[i % len(ctxs)].consolidate_rerun()[:3]
                        for i in {0, n - 1})
            fstats = batch.batch_consolidate_fetch_stats()
            batch.batch_consolidate_run()
            tables, fst = batch.batch_consolidate_fetch_all()
            counters = ("pods_simulated", "checks", "node_evals", "node_prefix", "pops")
            table = lambda t: (t[:3], [int(getattr(t[3], k)) for k in counters])  # noqa: E731
            batch.batch_consolidate_run()
            exact_all = fst == [abi.GS_OK] * n and all(table(tables[i]) == table(batch.batch_consolidate_fetch(i))
                                                       for i in range(n))
            both = statistics.median(a_wall) + statistics.median(f_wall)
            both_all = statistics.median(a_wall) + statistics.median(fa_wall)
            row = {"n": n, "simulations": 24 * n, "batch_ms": rng(a_wall), "device_ms": rng(a_dev), "fetch_ms": rng(f_wall),
                   "fetch_all_ms": rng(fa_wall), "fetch_all_first_ms": round(fa_first, 4),
                   "fetch_ms_reps": [round(x, 4) for x in f_wall], "fetch_all_ms_reps": [round(x, 4) for x in fa_wall],
                   "serial_ms": rng(b_wall),
                   "serial_over_batch": round(statistics.median(b_wall) / statistics.median(a_wall), 2),
                   "serial_over_batch_and_fetch": round(statistics.median(b_wall) / both, 2),
                   "fetch_ms_per_slot": round(statistics.median(f_wall) / n, 4),
                   "fetch_over_fetch_all": round(statistics.median(f_wall) / statistics.median(fa_wall), 2),
                   "fetch_all_below_fetch_by_more_than_its_spread":
                       bool(min(f_wall) - max(fa_wall) > max(f_wall) - min(f_wall)),
                   "serial_over_batch_and_fetch_all": round(statistics.median(b_wall) / both_all, 2),
                   "fetch_all_launches": fstats["n_launches"], "fetch_all_copies": fstats["n_copies"],
                   "fetch_all_bytes": fstats["bytes"], "fetch_all_device_ms": round(fstats["device_ms"], 4),
                   "fetch_all_exact": bool(exact_all),
                   "n_batched": stats["n_batched"], "n_fallback": stats["n_fallback"], "n_groups": stats["n_groups"],
                   "n_launches": stats["n_launches"], "prepare_ms": round(stats["prepare_ms"], 2),
                   "bit_exact": bool(exact)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    finally:
        batch.close()
        for s in singles:
            s.close()
    out = {"what": "gs_batch_consolidate_run of N C1-sized clusters (a), the fetch of all N slots one by one (b) and by "
                   "gs_batch_consolidate_fetch_all (b') against N gs_consolidate_rerun calls in turn on ordinary "
                   "contexts holding the same clusters (c, at most 64 contexts reused in turn); [min, max] over the "
                   "repetitions, ms",
           "reps": args.reps, "steps": args.steps, "rows": rows}
    print("| N | simulations | batch ms | device ms | fetch ms | fetch_all ms | N x rerun ms | rerun / batch | "
          "rerun / (batch + fetch) | rerun / (batch + fetch_all) |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        f = lambda x: f"{x[0]:.2f}-{x[1]:.2f}"  # noqa: E731
        print(f"| {r['n']} | {r['simulations']} | {f(r['batch_ms'])} | {f(r['device_ms'])} | {f(r['fetch_ms'])} | "
              f"{f(r['fetch_all_ms'])} | {f(r['serial_ms'])} | {r['serial_over_batch']} | "
              f"{r['serial_over_batch_and_fetch']} | {r['serial_over_batch_and_fetch_all']} |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
