"""Autoplacement ranking with the catalog resident on the device, against the
per-call path and the CPU port.

One session, one context.  For a catalog of CM's size (198 profiles) and one of
2,000 types (the bench's ranking leg), and nq NodeClass queries for nq in
{1, 8, 64, 512, 4096}: the catalog is prepared once, then --rounds rounds
alternate
  * one gs_rank_run over the nq queries, returning every kept type with its
    score (what nq gs_rank_instance_types calls return), and one returning the
    top 60 indices only,
  * nq sequential gs_rank_instance_types calls on the same queries,
  * nq sequential oracle_rank_instance_types calls (the CPU port, one core).
Every sample is one such pass timed on the host clock, through ctypes with the
arguments marshalled beforehand; the run's phases come from gs_rank_last_run.
The reference is the existing entry point and the oracle in the same session,
never the new path.  Run on the GPU box:
  python tools/rank_batch.py --out profiles/r7/rank_batch.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "karpenter-provider-ibm-cloud_amd"))
sys.path.insert(0, ROOT)

from gpusched import abi, lib  # noqa: E402
from gpusched.lib import Solver  # noqa: E402
from oracle import pyoracle  # noqa: E402

PHASES = ("encode_ms", "upload_ms", "kernel_ms", "fetch_ms")
NQS = (1, 8, 64, 512, 4096)
MODES = (("all_with_scores", 0, True), ("top60_indices", 60, False))


def mm(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4)}


def make_catalog(seed, n):
    """the shapes and prices of the bench's ranking leg (exact score ties), two architectures"""
    rng = np.random.default_rng(seed)
    vcpu = rng.choice([2, 4, 8, 16, 32, 48, 64, 96], size=n)
    ratio = rng.choice([2, 4, 8], size=n)
    cpu = (vcpu * 1000).astype(np.int64)
    mem = (vcpu * ratio * (1 << 30)).astype(np.int64)
    price = np.round(vcpu * ratio * rng.choice([0.01, 0.0125, 0.02], size=n), 4)
    arch = rng.integers(0, 2, size=n).astype(np.uint32)
    return cpu, mem, price, arch


def make_queries(seed, nq, price):
    rng = np.random.default_rng(seed)
    qs = []
    for _ in range(nq):
        qs.append(dict(want_arch=int(rng.choice([abi.GS_ARCH_ANY, 0, 1])), min_cpu=int(rng.choice([0, 2, 4, 8])),
                       min_memory_gb=int(rng.choice([0, 8, 16, 64])),
                       max_price=float(rng.choice([0.0, np.median(price), np.max(price)]))))
    return qs


class PerCall:
    """nq sequential calls of a gs_rank_instance_types-shaped function, arguments marshalled once"""

    def __init__(self, fn, cols, qs):
        self.fn, self.n, self.qs = fn, len(cols[0]), qs
        self.cols = [np.ascontiguousarray(a, dtype=t) for a, t in zip(cols, (np.int64, np.int64, np.float64, np.uint32))]
        self.ptrs = [a.ctypes.data_as(t) for a, t in zip(self.cols, abi.RANK_ARGTYPES[1:5])]
        self.order = np.zeros(max(self.n, 1), np.uint32)
        self.score = np.zeros(max(self.n, 1), np.float64)
        self.kept = C.c_uint32(0)
        self.out = (self.order.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(self.kept),
                    self.score.ctypes.data_as(C.POINTER(C.c_double)))
        self.args = [(q["want_arch"], q["min_cpu"], q["min_memory_gb"], q["max_price"]) for q in qs]

    def pass_(self, collect=False):
        got = []
        for a in self.args:
            st = self.fn(self.n, *self.ptrs, *a, *self.out)
            assert st == abi.GS_OK
            if collect:
                k = self.kept.value
                got.append((self.order[:k].tolist(), self.score[:k].view(np.uint64).tolist()))
        return got


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 5

    s = Solver(0)
    rows, prepares = [], {}
    try:
        for label, n in (("cm_198", 198), ("c5_2000", 2000)):
            cols = make_catalog(5, n)
            s.rank_prepare(*cols)
            prepares[label] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in s.rank_last_run().items()}
            for nq in NQS:
                qs = make_queries(100 + nq, nq, cols[2])
                arr = abi.rank_queries(qs)
                gpu = PerCall(lib.load().gs_rank_instance_types, cols, qs)
                cpu = PerCall(pyoracle.lib().oracle_rank_instance_types, cols, qs)
                want = cpu.pass_(collect=True)
                same_seq = gpu.pass_(collect=True) == want
                orders, scores, kept = s.rank_run((arr, nq), scores=True)
                same_run = [(o, np.array(sc, np.float64).view(np.uint64).tolist()) for o, sc in zip(orders, scores)] == want
                same_top = s.rank_run((arr, nq), max_out=60)[0] == [w[0][:60] for w in want]
                t_run = {m[0]: [] for m in MODES}
                phases = {m[0]: {k: [] for k in PHASES} for m in MODES}
                stats = {}
                t_seq, t_cpu = [], []
                for _ in range(args.rounds):
                    for name, max_out, sc in MODES:
                        flags = abi.GS_RANK_SCORES if sc else 0
                        res = abi.GsRankResult()
                        t_run[name].append(timed(lambda: s.L.gs_rank_run(s.ctx, arr, nq, max_out, flags, C.byref(res))))
                        stats[name] = s.rank_last_run()
                        for k in PHASES:
                            phases[name][k].append(stats[name][k])
                    t_seq.append(timed(gpu.pass_))
                    t_cpu.append(timed(cpu.pass_))
                row = {"catalog": label, "instance_types": n, "queries": nq, "samples_each": args.rounds,
                       "sequential_gs_rank_instance_types_ms": mm(t_seq), "oracle_1core_ms": mm(t_cpu),
                       "same_results": bool(same_seq and same_run and same_top)}
                for name, _, _ in MODES:
                    st = stats[name]
                    row[name] = {"run_ms": mm(t_run[name]),
                                 "phases_ms": {k: mm(v) for k, v in phases[name].items()},
                                 "h2d_bytes": st["h2d_bytes"], "d2h_bytes": st["d2h_bytes"],
                                 "n_launches": st["n_launches"],
                                 "sequential_min_over_run_median": round(min(t_seq) / statistics.median(t_run[name]), 2),
                                 "oracle_min_over_run_median": round(min(t_cpu) / statistics.median(t_run[name]), 2)}
                rows.append(row)
                print(json.dumps(row), flush=True)
    finally:
        s.close()
    out = {"what": "gs_rank_run on a resident catalog against nq sequential gs_rank_instance_types calls and nq "
                   "oracle_rank_instance_types calls (CPU port, 1 core) on the same queries, alternating in one "
                   "session; host clock per pass of nq queries, ms; phases from gs_rank_last_run",
           "rounds": args.rounds, "prepare": prepares, "rows": rows}
    print("| catalog | nq | run, all + scores ms (median, min) | run, top 60 ms | kernel ms | nq x gs_rank_instance_types ms "
          "| nq x oracle, 1 core ms | sequential min / run median | oracle min / run median |")
    print("|---|---|---|---|---|---|---|---|---|")
    f = lambda x: f"{x['median']:.4f} ({x['min']:.4f})"  # noqa: E731
    for r in rows:
        a, t = r["all_with_scores"], r["top60_indices"]
        print(f"| {r['instance_types']} | {r['queries']} | {f(a['run_ms'])} | {f(t['run_ms'])} | "
              f"{a['phases_ms']['kernel_ms']['median']:.4f} | {f(r['sequential_gs_rank_instance_types_ms'])} | "
              f"{f(r['oracle_1core_ms'])} | {a['sequential_min_over_run_median']} | {a['oracle_min_over_run_median']} |")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
