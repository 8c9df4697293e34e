"""Run mode's per-pod chain in the single-wave Solve (round 10).

Round 10 takes the vector-memory drains and the work a fast accept never
reads off the run loop: one vector-memory wait at run entry, the exact check
and its winner's Add as one region, one stop value of qhead for the pop
bound, the ring-slot release and the heartbeat in one section (a cursor for
the choosePivot samples was built, timed and dropped).  No result and no
counter may move, so every case is bit for bit against the oracle
(claim_prefix and node_prefix included) and its library and run counters are
compared with tests/golden/run_chain_counters.json, recorded from the library
before round 10.  What each shape pins:

 - cm-tail-4000: a run that reaches the end of the first pass.  The run leaves
   at the last first-pass pod (the general path pops it and wraps the queue), so
   a stop value off by one changes the run-pod count.  Checked on the CPU from the
   oracle's result and the queue order (cpu, memory descending, creation time,
   uid): the last pod repeats its predecessor's spec, both land on NodeClaims
   that already hold pods, and the Solve opens >= 100 NodeClaims.
   (The pods of one request vector alone do not reach run mode: the most
   frequent selector-free vector of a 4,000-pod CM problem has 184-234 pods,
   which open 2-3 NodeClaims, and all selector-free pods of 4,400 open 37;
   run mode needs 50 in flight.  The whole problem is the smallest shape
   where the queue's tail is a run.)
 - cm-2500, c2-3000, c2-3500: touched pivot samples.  The library before
   round 10 leaves runs by the pivot exit 114, 305 and 209 times on them; a
   diagnostic build of it counted the exits by M mod 4 as [28, 12, 52, 22],
   [55, 107, 34, 109] and [80, 56, 64, 9], so every residue -- modpos == t and
   modpos + 1 == t for each of the three samples -- is taken.  (The library
   reports no M, so the histogram is a record of the choice, not an
   assertion; the pivot exit counts against the golden are.)
 - c2-3000-x: the exact check inside runs (167 batches) with a window rebase
   (rare at these sizes: one seed of 64), also with the claim state in HBM and
   as three slots of one batch (the HBM Solve's counters are the golden's
   "c2-3000-x@hbm", each slot's library counters the single Solve's).
 - e2e-6x60 and c5-3000: one topology and one wide-row problem (no run mode;
   the shared header serves them), counters against the golden as well.
"""
import ctypes as C
import json
import os

import pytest

from gpusched import abi, synth
from oracle import pyoracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_chain_counters.json")

RUN_CASES = {
    "cm-tail-4000": lambda: synth.make_cm(n_pods=4000, seed=0x5EED0D08),
    "cm-2500": lambda: synth.make_cm(n_pods=2500, seed=0x5EED0D09),
    "c2-3000": lambda: synth.make_c2(n_pods=3000, seed=0x5EED0D07),
    "c2-3500": lambda: synth.make_c2(n_pods=3500, seed=0x5EED0D05),
    "c2-3000-x": lambda: synth.make_c2(n_pods=3000, seed=0x5EED0D06),
}
OTHER_CASES = {
    "e2e-6x60": lambda: synth.e2e_deployments(n_deployments=6, replicas=60, seed=0x5EED0A04),
    "c5-3000": lambda: synth.make_c5(n_pods=3000, seed=0x5EED0A05),
}
PIVOT_CASES = ("cm-2500", "c2-3000", "c2-3500")
HBM_KEY = "c2-3000-x@hbm"  # the golden's entry for c2-3000-x with the claim state in HBM
RUN_KEYS = ("pods", "entries", "pivot", "window", "spec", "scan", "exact")
LIB_KEYS = ("pops", "cand_evals", "cand_full", "sorts_fast", "sorts_generic")

_CACHE = {}


def case(name):
    """the problem and its oracle Solve, computed once and shared"""
    if name not in _CACHE:
        p = (RUN_CASES.get(name) or OTHER_CASES[name])()
        st, want, raw = pyoracle.solve(p)
        assert st == abi.GS_OK
        _CACHE[name] = (p, want, (int(raw.claim_prefix), int(raw.node_prefix)))
    return _CACHE[name]


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def counters(s, res):
    """the library's counters of the last run and the kernel's run counters
    (dbg[8..13]: pods placed in runs, entries, exits by pivot / window / spec /
    scan; dbg[14]: exact batches in runs)"""
    out = (C.c_uint64 * 16)()
    s.L.gs_debug_ctrl.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32]
    s.L.gs_debug_ctrl(s.ctx, out, 16)
    c = {k: int(getattr(res, k)) for k in LIB_KEYS}
    c.update({k: int(out[8 + i]) for i, k in enumerate(RUN_KEYS)})
    return c


def solve_checked(s, name):
    from test_gpu_parity import _diff
    p, want, prefixes = case(name)
    s.prepare(p)
    s.run()
    got, res = s.fetch()
    d = _diff(got, want)
    assert d is None, d
    assert (int(res.claim_prefix), int(res.node_prefix)) == prefixes
    return got, res


def pod_spec(p, i):
    """what run mode compares of a CM pod: its requests and its node selector"""
    pod = p.pods[i]

    def span(field, table, cols):
        o, n = int(pod[field][0]), int(pod[field][1])
        return tuple(tuple(int(table[k][c]) for c in cols) for k in range(o, o + n))

    return span("requests", p.quantities, ("resource", "milli")), span("node_selector", p.labels, ("key", "value"))


def check_tail(p, want):
    """the queue's last pod repeats its predecessor's spec, both were placed
    on NodeClaims that hold other pods, and >= 100 NodeClaims open"""
    res = {p.strings[i]: i for i in range(len(p.strings)) if p.strings[i] in ("cpu", "memory")}

    def key(i):
        rq = dict(pod_spec(p, i)[0])
        uid = p.strings[int(p.pods[i]["uid"])]
        return (-rq.get(res["cpu"], 0), -rq.get(res["memory"], 0), int(p.pods[i]["creation_ns"]),
                uid.encode() if isinstance(uid, str) else uid)

    order = sorted(range(len(p.pods)), key=key)
    last, prev = order[-1], order[-2]
    assert pod_spec(p, last) == pod_spec(p, prev), "the last pod opens a new spec"
    assert len(want["claims"]) >= 100, len(want["claims"])
    holder = {i: c for c in want["claims"] for i in c["pods"]}
    for i in (prev, last):
        assert i in holder and len(holder[i]["pods"]) > 2, "the tail pod was not added to a NodeClaim in flight"


def test_tail_problem_ends_in_a_run():
    p, want, _ = case("cm-tail-4000")
    check_tail(p, want)


def test_golden_shows_the_paths():
    """the recorded counters of the library before round 10: the pivot exits,
    the exact batches and the rebase the shapes were chosen for"""
    g = golden()
    assert set(g) == set(RUN_CASES) | set(OTHER_CASES) | {HBM_KEY}
    for name in PIVOT_CASES:
        assert g[name]["pivot"] >= 3, (name, g[name])
    assert g["c2-3000-x"]["exact"] >= 20 and g["c2-3000-x"]["window"] >= 1, g["c2-3000-x"]
    assert g["cm-tail-4000"]["pods"] > 0


@pytest.fixture(scope="module")
def wave():
    from gpusched.lib import Solver
    s = Solver(0, 0)
    yield s
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RUN_CASES))
def test_gpu_run_chain_counters(wave, name):
    _, res = solve_checked(wave, name)
    ctr = counters(wave, res)
    print(name, json.dumps(ctr))
    assert ctr == golden()[name]


@pytest.mark.gpu
def test_gpu_run_chain_claims_in_hbm():
    from gpusched.lib import Solver
    s = Solver(0, abi.GS_CFG_CLAIMS_HBM)
    try:
        _, res = solve_checked(s, "c2-3000-x")
        ctr = counters(s, res)
        print(HBM_KEY, json.dumps(ctr))
        assert ctr == golden()[HBM_KEY]
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_run_chain_batch_slots(wave):
    """three slots of one gs_batch_run, each equal to the single Solve, its
    library counters the golden's"""
    from test_gpu_parity import _diff
    p, want, prefixes = case("c2-3000-x")
    single, _ = solve_checked(wave, "c2-3000-x")
    want_ctr = golden()["c2-3000-x"]
    assert wave.batch_prepare([p, p, p]) == [abi.GS_OK] * 3
    wave.batch_run()
    for i in range(3):
        got, res = wave.batch_fetch(i)
        assert _diff(got, single) is None and _diff(got, want) is None, i
        assert (int(res.claim_prefix), int(res.node_prefix)) == prefixes, i
        assert {k: int(getattr(res, k)) for k in LIB_KEYS} == {k: want_ctr[k] for k in LIB_KEYS}, i


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OTHER_CASES))
def test_gpu_run_chain_other_instantiations(wave, name):
    _, res = solve_checked(wave, name)
    ctr = counters(wave, res)
    print(name, json.dumps(ctr))
    assert ctr == golden()[name]
