"""What gs_explain costs beside gs_feasibility, at full size.

Prepares CM (100k pods), and in one session, after one warm-up of each,
alternates gs_feasibility and gs_explain(NULL, 0, GS_EXPLAIN_AS_GIVEN) for
--rounds rounds (at least 5): both judge every pod's first variant against
every template and read the same resident sets; the explain kernels add the
seven group reductions and skip the cheapest-offering scan.  Then one Solve,
and gs_explain of its actual error_pods alone (the intended call).

Per call: the kernel time (HIP events), t_total_ms, n_variants, d2h_bytes.  The
yardstick is gs_feasibility's kernel time in the same rounds: the explain
kernels are allowed K1's median plus K1's own max - min spread.  The script
also asserts, at full size, that GS_WHY_STATE as given holds exactly where
gs_feasibility finds a cheapest type.  Run on the GPU box:
  python tools/explain_cost.py --out profiles/r7/explain.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "karpenter-provider-ibm-cloud_amd"))
sys.path.insert(0, ROOT)

from gpusched import abi, explain, synth  # noqa: E402
from gpusched.lib import Solver  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 5
    problem = synth.make_cm(a.pods)
    s = Solver(0)
    try:
        s.prepare(problem)
        feas, fres = s.feasibility()  # warm-up (builds the grid-order tables) and the equivalence's reference
        why = s.explain(as_given=True)
        state = why["cause"] == abi.GS_WHY_STATE
        assert (state == (feas["cheapest"] != -1)).all(), "STATE differs from gs_feasibility's cheapest_it"
        k1, ex, ex_total = [], [], []
        for _ in range(a.rounds):
            _, fres = s.feasibility()
            k1.append(fres.t_kernel_ms)
            r = s.explain(as_given=True, raw=True)
            ex.append(r.t_kernel_ms)
            ex_total.append(r.t_total_ms)
            n_variants, d2h = r.n_variants, r.d2h_bytes
        s.run()
        result, res = s.fetch()
        err = s.explain(pods=(res.error_pods, res.n_errors))
        err_relaxed_all = s.explain()
        hist = {explain.CAUSE_NAMES[c]: int(n) for c, n in
                enumerate(np.bincount(err["cause"].ravel(), minlength=abi.GS_WHY_COUNT)) if n}
        allowed = statistics.median(k1) + (max(k1) - min(k1))
        out = {
            "workload": f"CM {a.pods} pods", "rounds": a.rounds,
            "words": int(res.words), "n_templates": int(res.n_templates), "n_nodepools": int(why["cause"].shape[1]),
            "feasibility_kernel_ms": [round(x, 4) for x in k1],
            "explain_kernel_ms": [round(x, 4) for x in ex],
            "explain_total_ms": [round(x, 3) for x in ex_total],
            "feasibility_kernel_median_ms": round(statistics.median(k1), 4),
            "feasibility_kernel_spread_ms": round(max(k1) - min(k1), 4),
            "explain_kernel_median_ms": round(statistics.median(ex), 4),
            "allowed_ms": round(allowed, 4),
            "within_allowance": bool(statistics.median(ex) <= allowed),
            "explain_all": {"n_variants": int(n_variants), "d2h_bytes": int(d2h)},
            "state_equals_cheapest_it": True,
            "solve_errors": int(res.n_errors),
            "explain_error_pods": {"n_pods": int(res.n_errors), "kernel_ms": round(err["t_kernel_ms"], 4),
                                   "total_ms": round(err["t_total_ms"], 3), "n_variants": err["n_variants"],
                                   "d2h_bytes": err["d2h_bytes"], "causes": hist},
            "explain_all_relaxed": {"kernel_ms": round(err_relaxed_all["t_kernel_ms"], 4),
                                    "total_ms": round(err_relaxed_all["t_total_ms"], 3),
                                    "n_variants": err_relaxed_all["n_variants"]},
        }
    finally:
        s.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
