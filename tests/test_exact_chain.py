"""The exact NodeClaim.CanAdd check and the general path of the single-wave
Solve (round 11).

Round 11 loads the threshold rows of every resource in one memory round trip
(run mode's check and the general path's phase B) and takes the loads out of
the winner's Add (the header's capacity-type mask is carried, ctb is narrowed
by a no-return atomic); a phase A that passes a chunk with no candidate at
once was built, timed and dropped.  No result and no counter may
move, so every case is bit for bit against the oracle (claim_prefix and
node_prefix included) and its library and run counters are compared with
tests/golden/exact_chain_counters.json, recorded from the library of commit
5164a26 (the parent of round 11).  What each shape pins:

 - two-cursors-600: 600 pods of 4-16 vCPU and 16-64 GiB on the C2 catalog, a
   node selector on every pod, so no pod is simple and every placement on a
   NodeClaim in flight goes through phase B.  Checked on the CPU from the
   oracle's result and the catalog's allocatable values: at least one Add moves
   the cpu cursor and the memory cursor at once (the claim's totals before and
   after the pod lie on either side of a distinct allocatable value of each),
   so one batch needs the rows of two resources.
 - c2-3000-y: a C2 shape that opens >= 50 NodeClaims and runs exact batches
   inside runs (the golden's run "exact" count), as a single Solve, with the
   claim state in HBM (the golden's "c2-3000-y@hbm") and as three slots of one
   gs_batch_run; each claim's requirement string and capacity types against
   the oracle's (what the Add's cm / ctb feed).
 - six-resources-400: six requested resources, so two cursors and totals live
   in ClaimRec.tot_hi / thr_hi (the pods resource among them: its cursor moves
   whenever a claim passes 30 or 60 pods).
 - c3-400 and e2e-6x60: the topology instantiation (zone spreads, selectors,
   four NodePools, one with limits; hostname spreads).  It shares phase B's
   code; it measured slower with every row loaded and keeps a load per moved
   cursor, chosen at compile time in the same function.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from gpusched import abi, catalog as cat, synth
from gpusched.problem import ProblemBuilder
from oracle import pyoracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exact_chain_counters.json")

GI = synth.GI
MI = synth.MI
DAEMON = {"cpu": 200, "memory": 256 * MI * 1000, "pods": 2000}


def _c2_pool(b, rng, extra_capacity=None):
    """the C2 catalog and its NodePool; extra_capacity(vcpu) adds resources"""
    profs = synth.c2_profiles(200)
    if extra_capacity is None:
        synth.build_catalog(b, profs, synth.FAKE_ZONES, spot=True, prices=synth.price_table(profs), rng=rng,
                            unavailable_frac=0.02)
    else:
        prices = synth.price_table(profs)
        its = cat.list_instance_types([cat.Profile(n, v, m, "amd64", g, ("enum", ["standard", "spot"]))
                                       for n, v, m, g in profs], synth.FAKE_ZONES, lambda name, zone: prices.get(name))
        for it, (_, v, _, _) in zip(its, profs):
            cap = dict(it.capacity)
            cap.update(extra_capacity(v))
            b.add_instance_type(it.name, it.requirements, cap, it.overhead, it.offerings)
    b.add_nodepool("default", weight=0,
                   requirements=[("kubernetes.io/arch", "In", ["amd64"]), ("kubernetes.io/os", "In", ["linux"])],
                   daemon=DAEMON)


def two_cursors(n_pods=600, seed=0x5EED0B01):
    rng = np.random.default_rng(seed)
    b = ProblemBuilder()
    _c2_pool(b, rng)
    cpu = rng.choice(np.array([4000, 6000, 8000, 12000, 16000]), size=n_pods)
    mem = rng.choice(np.array([16, 24, 32, 48, 64]), size=n_pods)
    ts = 1_700_000_000_000_000_000 + rng.integers(0, 8, size=n_pods) * 1_000_000_000
    fams = ["bx2", "bx3d", "mx2", "mx3d"]
    for i in range(n_pods):
        sel = {"kubernetes.io/arch": "amd64"} if rng.random() < 0.6 else \
            {"karpenter-ibm.sh/instance-family": fams[rng.integers(0, len(fams))]}
        b.add_pod(synth._uid(rng), int(ts[i]), {"cpu": int(cpu[i]), "memory": int(mem[i]) * GI * 1000, "pods": 1000},
                  node_selector=sel)
    return b.build()


def six_resources(n_pods=400, seed=0x5EED0B02):
    rng = np.random.default_rng(seed)
    b = ProblemBuilder()
    _c2_pool(b, rng, lambda v: {"ephemeral-storage": v * 25 * GI * 1000, "example.com/nic": (1 + v // 16) * 1000})
    cpu = rng.choice(synth.CPU_CHOICES, size=n_pods, p=synth.CPU_W / synth.CPU_W.sum())
    mem = rng.choice(synth.MEM_CHOICES, size=n_pods)
    disk = rng.choice(np.array([1, 2, 5, 10, 20]), size=n_pods)
    ts = 1_700_000_000_000_000_000 + rng.integers(0, 8, size=n_pods) * 1_000_000_000
    for i in range(n_pods):
        req = {"cpu": int(cpu[i]), "memory": int(mem[i]), "pods": 1000, "ephemeral-storage": int(disk[i]) * GI * 1000}
        if rng.random() < 0.15:
            req["example.com/nic"] = 1000
        if rng.random() < 0.03:
            req["nvidia.com/gpu"] = 1000
        sel = {"kubernetes.io/arch": "amd64"} if rng.random() < 0.3 else {}
        b.add_pod(synth._uid(rng), int(ts[i]), req, node_selector=sel)
    return b.build()


RUN_CASE = "c2-3000-y"
HBM_KEY = RUN_CASE + "@hbm"  # the golden's entry for the run case with the claim state in HBM
CASES = {
    "two-cursors-600": two_cursors,
    RUN_CASE: lambda: synth.make_c2(n_pods=3000, seed=0x5EED0B03),
    "six-resources-400": six_resources,
    "c3-400": lambda: synth.make_c3(n_pods=400, seed=0x5EED0B04, spread_frac=0.3),
    "e2e-6x60": lambda: synth.e2e_deployments(n_deployments=6, replicas=60, seed=0x5EED0B05),
}
RUN_KEYS = ("pods", "entries", "pivot", "window", "spec", "scan", "exact")
LIB_KEYS = ("pops", "cand_evals", "cand_full", "sorts_fast", "sorts_generic")

_CACHE = {}


def case(name):
    """the problem and its oracle Solve, computed once and shared"""
    if name not in _CACHE:
        p = CASES[name]()
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


def claim_outcomes(result):
    """per claim: its requirement string and the capacity types it admits"""
    out = []
    for c in result["claims"]:
        ct = [ln for ln in c["requirements"].split("\n") if ln.startswith("karpenter.sh/capacity-type|")]
        out.append((c["requirements"], tuple(ct)))
    return out


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


def allocatable(p, resource):
    """the distinct allocatable values (capacity - overhead) of one resource"""
    rid = {p.strings[int(q["resource"])]: None for q in p.quantities}
    assert resource in rid

    def qty(span):
        o, n = int(span["begin"]), int(span["count"])
        return {p.strings[int(p.quantities[k]["resource"])]: int(p.quantities[k]["milli"]) for k in range(o, o + n)}

    vals = set()
    for it in p.instance_types:
        vals.add(qty(it["capacity"]).get(resource, 0) - qty(it["overhead"]).get(resource, 0))
    return sorted(vals)


def straddling_adds(p, want):
    """the Adds of the oracle's result after which both the cpu and the memory
    threshold cursor (lower_bound of the claim's total over the distinct
    allocatable values) stand further than before"""
    a_cpu, a_mem = allocatable(p, "cpu"), allocatable(p, "memory")

    def requests(i):
        o, n = int(p.pods[i]["requests"]["begin"]), int(p.pods[i]["requests"]["count"])
        return {p.strings[int(p.quantities[k]["resource"])]: int(p.quantities[k]["milli"]) for k in range(o, o + n)}

    def moves(vals, before, after):
        return any(before <= a < after for a in vals)

    hits = 0
    for c in want["claims"]:
        cpu, mem = DAEMON["cpu"], DAEMON["memory"]
        for k, i in enumerate(c["pods"]):
            rq = requests(i)
            ncpu, nmem = cpu + rq.get("cpu", 0), mem + rq.get("memory", 0)
            if k > 0 and moves(a_cpu, cpu, ncpu) and moves(a_mem, mem, nmem):
                hits += 1
            cpu, mem = ncpu, nmem
        assert cpu == c["requests"]["cpu"] and mem == c["requests"]["memory"], "the claim's pods are not in Add order"
    return hits


def test_two_cursors_move_in_one_add():
    p, want, _ = case("two-cursors-600")
    assert all(int(pod["node_selector"]["count"]) > 0 for pod in p.pods), "a pod without a selector may be simple"
    assert len(want["claims"]) >= 20, len(want["claims"])
    hits = straddling_adds(p, want)
    print("Adds that move the cpu and the memory cursor:", hits)
    assert hits >= 1


def test_six_resources_are_requested():
    p, want, _ = case("six-resources-400")
    names = {p.strings[int(q["resource"])] for q in p.quantities}
    assert len(names) == 6, names
    assert any(len(c["pods"]) > 60 for c in want["claims"]), "no claim passes the 30- and 60-pod allocatable values"


def test_golden_shows_the_paths():
    """the recorded counters of the library before round 11: exact batches
    inside runs and >= 50 NodeClaims on the run case, phase-B candidates
    everywhere"""
    g = golden()
    assert set(g) == set(CASES) | {HBM_KEY}
    assert g[RUN_CASE]["exact"] > 0 and g[HBM_KEY]["exact"] > 0, g[RUN_CASE]
    assert len(case(RUN_CASE)[1]["claims"]) >= 50
    for name in CASES:
        assert g[name]["cand_full"] > 0, (name, g[name])
    assert g["two-cursors-600"]["pods"] == 0, "a selector pod was placed in run mode"


@pytest.fixture(scope="module")
def wave():
    from gpusched.lib import Solver
    s = Solver(0, 0)
    yield s
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_exact_chain_counters(wave, name):
    got, res = solve_checked(wave, name)
    ctr = counters(wave, res)
    print(name, json.dumps(ctr))
    assert claim_outcomes(got) == claim_outcomes(case(name)[1])
    assert ctr == golden()[name]


@pytest.mark.gpu
def test_gpu_exact_chain_claims_in_hbm():
    from gpusched.lib import Solver
    s = Solver(0, abi.GS_CFG_CLAIMS_HBM)
    try:
        got, res = solve_checked(s, RUN_CASE)
        ctr = counters(s, res)
        print(HBM_KEY, json.dumps(ctr))
        assert claim_outcomes(got) == claim_outcomes(case(RUN_CASE)[1])
        assert ctr == golden()[HBM_KEY]
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_exact_chain_batch_slots(wave):
    """three slots of one gs_batch_run, each equal to the single Solve, its
    library counters the golden's"""
    from test_gpu_parity import _diff
    p, want, prefixes = case(RUN_CASE)
    single, _ = solve_checked(wave, RUN_CASE)
    want_ctr = golden()[RUN_CASE]
    assert wave.batch_prepare([p, p, p]) == [abi.GS_OK] * 3
    wave.batch_run()
    for i in range(3):
        got, res = wave.batch_fetch(i)
        assert _diff(got, single) is None and _diff(got, want) is None, i
        assert (int(res.claim_prefix), int(res.node_prefix)) == prefixes, i
        assert claim_outcomes(got) == claim_outcomes(want), i
        assert {k: int(getattr(res, k)) for k in LIB_KEYS} == {k: want_ctr[k] for k in LIB_KEYS}, i
