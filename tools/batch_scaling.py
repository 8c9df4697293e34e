"""How a batch of independent Solves scales with the number of problems.

One gs_run occupies one workgroup, so one CU; gs_batch_run gives every problem
of a batch its own workgroup in the same launches.  For C1 (500 pods) at
N = 1, 16, 64, 256, 1024 slots and C2 (2,000 pods) at N = 1, 16, 64, 256, in
three alternating repetitions per leg (ranges reported, as DESIGN does):

  (a) batch_ms   gs_batch_run wall (median of --steps runs) and device_ms
                 (first to last batched kernel, HIP events)
  (b) serial_ms  the comparison that counts: the same N problems prepared on
                 ordinary contexts, N sequential gs_run calls (at most 64
                 contexts, reused in turn for larger N)
  (c) cpu_ms     the 1-core oracle Solve of one problem (input build
                 excluded) times N

The condition DESIGN §4 states: at N = 64 on C1, (a) is below (b) by more
than the run-to-run spread of (b).  Slot 0 and the last slot of every batch
are compared with the oracle (bit-exact).  Run on the GPU box:
  python tools/batch_scaling.py --out profiles/r7/batch_scaling.json
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
from gpusched.lib import Solver  # noqa: E402

MAX_CONTEXTS = 64


def rng(xs):
    return [round(min(xs), 4), round(max(xs), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c1", default="1,16,64,256,1024")
    ap.add_argument("--c2", default="1,16,64,256")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from oracle import pyoracle  # the checker and the CPU baseline, never the product path

    legs = [("C1", synth.make_c1(), [int(x) for x in args.c1.split(",") if x]),
            ("C2", synth.make_c2(n_pods=2000), [int(x) for x in args.c2.split(",") if x])]
    rows = []
    batch = Solver(0)
    singles = []
    try:
        for name, p, sizes in legs:
            st, want, _ = pyoracle.solve(p)
            assert st == abi.GS_OK
            for n in sizes:
                while len(singles) < min(n, MAX_CONTEXTS):
                    singles.append(Solver(0))
                ctxs = singles[:min(n, MAX_CONTEXTS)]
                for s in ctxs:
                    s.prepare(p)
                    s.run()
                status = batch.batch_prepare([p] * n)
                assert status == [abi.GS_OK] * n
                batch.batch_run()
                a_wall, a_dev, b_wall, c_cpu = [], [], [], []
                for _ in range(args.reps):
                    w, d = [], []
                    for _ in range(args.steps):
                        t0 = time.perf_counter()
                        batch.batch_run()
                        w.append((time.perf_counter() - t0) * 1e3)
                        d.append(batch.batch_stats()["device_ms"])
                    a_wall.append(statistics.median(w))
                    a_dev.append(statistics.median(d))
                    t0 = time.perf_counter()
                    for i in range(n):
                        ctxs[i % len(ctxs)].run()
                    b_wall.append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    _, _, raw = pyoracle.solve(p)
                    c_cpu.append(((time.perf_counter() - t0) * 1e3 - float(raw.t_encode_ms)) * n)
                stats = batch.batch_stats()
                exact = all(batch.batch_fetch(i)[0] == want for i in {0, n - 1})
                row = {"config": name, "pods": len(p.pods), "n": n, "batch_ms": rng(a_wall), "device_ms": rng(a_dev),
                       "serial_ms": rng(b_wall), "cpu_ms": rng(c_cpu),
                       "serial_over_batch": round(statistics.median(b_wall) / statistics.median(a_wall), 2),
                       "solves_per_s": round(n / statistics.median(a_wall) * 1e3, 1),
                       "n_batched": stats["n_batched"], "n_groups": stats["n_groups"],
                       "n_launches": stats["n_launches"], "prepare_ms": round(stats["prepare_ms"], 2),
                       "bit_exact": bool(exact)}
                rows.append(row)
                print(json.dumps(row), flush=True)
    finally:
        batch.close()
        for s in singles:
            s.close()
    c64 = next((r for r in rows if r["config"] == "C1" and r["n"] == 64), None)
    cond = None
    if c64:
        spread = c64["serial_ms"][1] - c64["serial_ms"][0]
        cond = {"batch_ms_max": c64["batch_ms"][1], "serial_ms_min": c64["serial_ms"][0], "serial_spread_ms": round(spread, 4),
                "met": bool(c64["batch_ms"][1] < c64["serial_ms"][0] - spread)}
    out = {"what": "gs_batch_run of N copies of one problem (a) against N sequential gs_run calls on ordinary "
                   "contexts (b) and N times the 1-core oracle Solve (c); [min, max] over the repetitions, ms",
           "reps": args.reps, "steps": args.steps, "rows": rows, "c1_n64_condition": cond}
    print(json.dumps({"c1_n64_condition": cond}))
    print("| config | N | batch ms | device ms | N x gs_run ms | N x CPU ms | serial / batch | Solves/s |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        f = lambda x: f"{x[0]:.2f}-{x[1]:.2f}"  # noqa: E731
        print(f"| {r['config']} | {r['n']} | {f(r['batch_ms'])} | {f(r['device_ms'])} | {f(r['serial_ms'])} | "
              f"{f(r['cpu_ms'])} | {r['serial_over_batch']} | {r['solves_per_s']} |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
