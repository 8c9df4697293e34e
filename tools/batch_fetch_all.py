"""What fetching a Solve batch costs, per slot and in one device pass.

gs_batch_run solves N clusters in five launches per kernel group; the results
then come back either one slot at a time (gs_batch_fetch: up to six synchronous
copies per slot and the decode on the calling thread) or all at once
(gs_batch_fetch_all: two launches, one transfer, the decode on up to 16
threads).  For N copies of C1 at N = 1, 16, 64, 256, 1024 and of C2 at N = 64,
in one session, after one warm-up, in three alternating repetitions:

  (a)  run_ms        gs_batch_run wall (median of --steps runs) and device_ms
  (b)  fetch_ms      gs_batch_fetch of all N slots after one run
  (b') fetch_all_ms  one gs_batch_fetch_all after a fresh run

Every slot of (b') is compared with (b): the decoded result and the raw
counters.  Reported beside them: run + fetch_all against run + per-slot fetch,
the bytes fetch_all transfers per slot, and the share of its wall clock the
host decode takes (the rest is the device pass and the transfer).  Run on the
GPU box:
  python tools/batch_fetch_all.py --out profiles/r7/batch_fetch_all.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "karpenter-provider-ibm-cloud_amd"))
sys.path.insert(0, ROOT)

from gpusched import abi, synth  # noqa: E402
from gpusched.lib import Solver  # noqa: E402

COUNTERS = ("checks", "pops", "cand_evals", "cand_full", "claim_prefix", "node_prefix", "sorts_fast", "sorts_generic",
            "t_ffd_sort_ms", "t_ffd_scan_ms", "t_ffd_template_ms", "words", "n_templates", "n_variants")


def rng(xs):
    return [round(min(xs), 4), round(max(xs), 4)]


def split_ms(s):
    """the last fetch_all's wall clock up to the end of the device pass, and of the decode"""
    out = (C.c_double * 2)()
    s.L.gs_debug_batch_fetch_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    s.L.gs_debug_batch_fetch_ms.restype = C.c_int
    assert s.L.gs_debug_batch_fetch_ms(s.ctx, out) == abi.GS_OK
    return out[0], out[1]


def leg(batch, name, problem, n, steps, reps):
    status = batch.batch_prepare([problem] * n)
    assert status == [abi.GS_OK] * n
    batch.batch_run()
    # the first fetch_all after a prepare learns the total (and may grow the staging buffers): timed apart, the warm-up
    t0 = time.perf_counter()
    batch.batch_fetch_all(raw=True)
    fa_first = (time.perf_counter() - t0) * 1e3
    first_stats = batch.batch_fetch_stats()
    for i in range(n):
        batch.batch_fetch(i)
    a_wall, a_dev, f_wall, fa_wall, decode_share = [], [], [], [], []
    res = abi.GsResult()
    for _ in range(reps):
        w, d = [], []
        for _ in range(steps):
            t0 = time.perf_counter()
            batch.batch_run()
            w.append((time.perf_counter() - t0) * 1e3)
            d.append(batch.batch_stats()["device_ms"])
        a_wall.append(statistics.median(w))
        a_dev.append(statistics.median(d))
        t0 = time.perf_counter()
        for i in range(n):
            assert batch.L.gs_batch_fetch(batch.ctx, i, C.byref(res)) == abi.GS_OK
        f_wall.append((time.perf_counter() - t0) * 1e3)
        batch.batch_run()
        t0 = time.perf_counter()
        batch.batch_fetch_all(raw=True)
        fa_wall.append((time.perf_counter() - t0) * 1e3)
        fs = batch.batch_fetch_stats()
        decode_share.append(split_ms(batch)[1] / fs["wall_ms"] if fs["wall_ms"] else 0.0)
    fstats = batch.batch_fetch_stats()
    stats = batch.batch_stats()
    # every slot of fetch_all against the per-slot fetch, on the same run
    batch.batch_run()
    results, fst = batch.batch_fetch_all()
    exact = fst == [abi.GS_OK] * n
    for i in range(n):
        got, raw = batch.batch_fetch(i)
        exact = exact and results[i][0] == got and all(getattr(results[i][1], k) == getattr(raw, k) for k in COUNTERS)
    med = statistics.median
    return {"problem": name, "n": n, "pods": len(problem.pods), "run_ms": rng(a_wall), "device_ms": rng(a_dev),
            "fetch_ms": rng(f_wall), "fetch_all_ms": rng(fa_wall), "fetch_all_first_ms": round(fa_first, 4),
            "fetch_ms_reps": [round(x, 4) for x in f_wall], "fetch_all_ms_reps": [round(x, 4) for x in fa_wall],
            "fetch_ms_per_slot": round(med(f_wall) / n, 4), "fetch_all_ms_per_slot": round(med(fa_wall) / n, 4),
            "fetch_over_fetch_all": round(med(f_wall) / med(fa_wall), 2),
            "fetch_all_below_fetch_by_more_than_its_spread": bool(min(f_wall) - max(fa_wall) > max(f_wall) - min(f_wall)),
            "run_plus_fetch_ms": round(med(a_wall) + med(f_wall), 4),
            "run_plus_fetch_all_ms": round(med(a_wall) + med(fa_wall), 4),
            "fetch_all_launches": fstats["n_launches"], "fetch_all_copies": fstats["n_copies"],
            "fetch_all_first_copies": first_stats["n_copies"], "fetch_all_first_launches": first_stats["n_launches"],
            "fetch_all_bytes": fstats["bytes"], "fetch_all_bytes_per_slot": round(fstats["bytes"] / n, 1),
            "fetch_all_device_ms": round(fstats["device_ms"], 4),
            "fetch_all_decode_share": rng(decode_share),
            "fetch_all_exact": bool(exact), "n_decided": fstats["n_decided"], "n_per_slot": fstats["n_per_slot"],
            "n_batched": stats["n_batched"], "n_fallback": stats["n_fallback"], "n_groups": stats["n_groups"],
            "prepare_ms": round(stats["prepare_ms"], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,64,256,1024", help="N copies of C1")
    ap.add_argument("--c2-sizes", default="64", help="N copies of C2")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    c1, c2 = synth.make_c1(), synth.make_c2(n_pods=2000)  # the problems of tools/batch_scaling.py
    legs = [("C1", c1, int(x)) for x in args.sizes.split(",") if x] + [("C2", c2, int(x)) for x in args.c2_sizes.split(",") if x]
    rows = []
    batch = Solver(0)
    try:
        for name, problem, n in legs:
            row = leg(batch, name, problem, n, args.steps, args.reps)
            rows.append(row)
            print(json.dumps(row), flush=True)
    finally:
        batch.close()
    out = {"what": "gs_batch_run of N copies of a problem (a), gs_batch_fetch of all N slots one by one (b) and one "
                   "gs_batch_fetch_all after a fresh run (b'); [min, max] over the repetitions, ms, one session",
           "reps": args.reps, "steps": args.steps, "rows": rows}
    print("| problem | N | run ms | device ms | fetch ms | fetch_all ms | fetch / fetch_all | run + fetch ms | "
          "run + fetch_all ms | bytes / slot | decode share |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        f = lambda x: f"{x[0]:.2f}-{x[1]:.2f}"  # noqa: E731
        print(f"| {r['problem']} | {r['n']} | {f(r['run_ms'])} | {f(r['device_ms'])} | {f(r['fetch_ms'])} | "
              f"{f(r['fetch_all_ms'])} | {r['fetch_over_fetch_all']} | {r['run_plus_fetch_ms']:.2f} | "
              f"{r['run_plus_fetch_all_ms']:.2f} | {r['fetch_all_bytes_per_slot']:.0f} | {f(r['fetch_all_decode_share'])} |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
