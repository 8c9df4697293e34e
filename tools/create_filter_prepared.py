"""The Create re-filter with the catalog resident on the device, against the
per-call path, on CM's NodeClaims (the claims bench.py's create_filter leg
uses, built by its claim_queries).

One session, one context.  The catalog is prepared once; then --rounds rounds
alternate --steps gs_create_filter calls with --steps gs_create_filter_run
calls, first with GS_CF_BITSETS and then without, and once more with the
claims in a pool of their own (own string ids, no pods or catalog strings),
which is what a controller sends.  Every call is timed on the host clock
(results stay in library memory, as in the bench leg); the run's phases come
from gs_create_filter_last_run.

The claim to establish, per mode: the median gs_create_filter_run call lies
below the fastest gs_create_filter call of the session.  The reference is the
existing entry point in the same session, never the new path.  Run on the GPU
box:
  python tools/create_filter_prepared.py --out profiles/r7/create_filter_prepared.json
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

from bench import claim_queries  # noqa: E402
from gpusched import synth  # noqa: E402
from gpusched.lib import Solver  # noqa: E402

PHASES = ("encode_ms", "upload_ms", "kernel_ms", "fetch_ms")


def mmm(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 5

    problem = synth.make_cm(n_pods=args.pods, seed=0x5EED0006)
    s = Solver(0)
    try:
        result, _ = s.solve(problem)
        p2 = claim_queries(problem, result)
        pool = p2.claims_pool()
        want = s.create_filter(p2)
        s.create_filter_prepare(p2)
        prep = s.create_filter_last_run()
        rows = []
        for mode, claims, bitsets in (("bitsets", p2, True), ("no_bitsets", p2, False),
                                      ("bitsets_own_pool", pool, True), ("no_bitsets_own_pool", pool, False)):
            got = s.create_filter_run(claims, bitsets=bitsets)
            if bitsets:
                exact = got == want
            else:
                exact = [(g["n_compatible"], g["selected"], g["capacity_type"]) for g in got] == \
                        [(w["n_compatible"], w["selected"], w["capacity_type"]) for w in want]
            old, new, phases = [], [], {k: [] for k in PHASES}
            for _ in range(args.rounds):
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    s.create_filter(p2, raw=True)
                    old.append((time.perf_counter() - t0) * 1e3)
                for _ in range(args.steps):
                    t0 = time.perf_counter()
                    s.create_filter_run(claims, bitsets=bitsets, raw=True)
                    new.append((time.perf_counter() - t0) * 1e3)
                    st = s.create_filter_last_run()
                    for k in PHASES:
                        phases[k].append(st[k])
            row = {"mode": mode, "claims": claims.n_claim_queries, "instance_types": len(p2.instance_types),
                   "pool_strings": len(claims.strings), "calls_each": args.rounds * args.steps,
                   "create_filter_ms": mmm(old), "run_ms": mmm(new),
                   "run_phases_ms": {k: mmm(v) for k, v in phases.items()},
                   "h2d_bytes": st["h2d_bytes"], "d2h_bytes": st["d2h_bytes"], "n_launches": st["n_launches"],
                   "n_staged_lds": st["n_staged_lds"],
                   "create_filter_min_over_run_median": round(min(old) / statistics.median(new), 2),
                   "run_median_below_create_filter_min": bool(statistics.median(new) < min(old)),
                   "same_results": bool(exact)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    finally:
        s.close()
    out = {"what": "gs_create_filter (catalog reduced and uploaded per call) against gs_create_filter_run on one "
                   "prepared catalog, alternating in one session; host clock per call, ms; phases from "
                   "gs_create_filter_last_run",
           "rounds": args.rounds, "steps": args.steps,
           "prepare": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in prep.items()}, "rows": rows}
    print("| mode | gs_create_filter ms (median, min-max) | run ms (median, min-max) | encode | upload | kernel | "
          "fetch | min / median |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        f = lambda x: f"{x['median']:.3f} ({x['min']:.3f}-{x['max']:.3f})"  # noqa: E731
        ph = r["run_phases_ms"]
        print(f"| {r['mode']} | {f(r['create_filter_ms'])} | {f(r['run_ms'])} | {ph['encode_ms']['median']:.3f} | "
              f"{ph['upload_ms']['median']:.3f} | {ph['kernel_ms']['median']:.4f} | {ph['fetch_ms']['median']:.3f} | "
              f"{r['create_filter_min_over_run_median']} |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
