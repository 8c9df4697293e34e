"""The single-wave Solve's per-pod chain (round 9).

Round 9 took work off the chain every placed pod runs -- the kernel-argument
pointers of the add log, the claim records and the exact check come from
register lanes instead of scalar loads, every wave vote is the comparison's own
mask, the code arithmetic of a fast accept has no branch, and the queue-run
array with its ring lane is gone -- and must move no result and no counter.

The smallest shapes that reach those paths (run mode needs >= 50 NodeClaims
in flight), each bit for bit against the oracle with the first-fit CanAdd
counts: CM, C2 and CM onto 150 state nodes (run mode, its exact batches and
window rebases, shown by the kernel's own run counters), the same CM problem
with the claim state in HBM and as three slots of one batch, one topology
problem and one wide-row problem (the emit, the votes and the codes serve
every instantiation).  The library's counters on the three run-mode shapes are
compared with tests/golden/pod_chain_counters.json, recorded from the library
before round 9.

A window rebase needs 64 NodeClaims of one pod count behind the raised one,
which is rare at these sizes: of 48 seeds per shape, two C2 seeds show one
rebase each and no CM or C4 seed any (the shapes' seeds are the ones with the
most rebases, then the most exact batches).  tests/test_run_mode.py holds the
larger problems where rebases are frequent.
"""
import ctypes as C
import json
import os

import pytest

from gpusched import abi, synth
from oracle import pyoracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pod_chain_counters.json")

SEEDS = {"cm-2500": 0x5EED0A91, "c2-3000": 0x5EED0A82, "c4-150-4000": 0x5EED0BB3}
RUN_CASES = {
    "cm-2500": lambda: synth.make_cm(n_pods=2500, seed=SEEDS["cm-2500"]),
    "c2-3000": lambda: synth.make_c2(n_pods=3000, seed=SEEDS["c2-3000"]),
    "c4-150-4000": lambda: synth.make_c4(n_nodes=150, n_pending=4000, seed=SEEDS["c4-150-4000"]),
}
OTHER_CASES = {
    "e2e-6x60": lambda: synth.e2e_deployments(n_deployments=6, replicas=60, seed=0x5EED0904),
    "c5-3000": lambda: synth.make_c5(n_pods=3000, seed=0x5EED0905),
}
RUN_KEYS = ("pods", "entries", "pivot", "window", "spec", "scan", "exact")
LIB_KEYS = ("pops", "cand_evals", "cand_full", "sorts_fast", "sorts_generic")

_CACHE = {}
_SEEN = {}


def case(name):
    """the problem and its oracle Solve, computed once and shared"""
    if name not in _CACHE:
        p = (RUN_CASES.get(name) or OTHER_CASES[name])()
        st, want, raw = pyoracle.solve(p)
        assert st == abi.GS_OK
        _CACHE[name] = (p, want, (int(raw.claim_prefix), int(raw.node_prefix)))
    return _CACHE[name]


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


@pytest.fixture(scope="module")
def wave():
    from gpusched.lib import Solver
    s = Solver(0, 0)
    yield s
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RUN_CASES))
def test_gpu_pod_chain_run_mode(wave, name):
    _, res = solve_checked(wave, name)
    ctr = counters(wave, res)
    print(name, json.dumps(ctr))
    _SEEN[name] = ctr
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert ctr == golden[name]


@pytest.mark.gpu
def test_gpu_pod_chain_run_paths_taken(wave):
    """over the three run-mode shapes: pods placed in runs, exact batches in
    runs and window rebases"""
    for name in RUN_CASES:
        if name not in _SEEN:  # run alone: the cases above did not
            _SEEN[name] = counters(wave, solve_checked(wave, name)[1])
    tot = {k: sum(c[k] for c in _SEEN.values()) for k in RUN_KEYS}
    print(json.dumps(tot))
    assert tot["pods"] > 0 and tot["exact"] > 0 and tot["window"] > 0, tot
    assert all(c["pods"] > 0 for c in _SEEN.values()), _SEEN


@pytest.mark.gpu
def test_gpu_pod_chain_claims_in_hbm():
    from gpusched.lib import Solver
    s = Solver(0, abi.GS_CFG_CLAIMS_HBM)
    try:
        solve_checked(s, "cm-2500")
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_pod_chain_batch_slots(wave):
    """three slots of one gs_batch_run, each equal to the single Solve"""
    from test_gpu_parity import _diff
    p, want, prefixes = case("cm-2500")
    single, _ = solve_checked(wave, "cm-2500")
    assert wave.batch_prepare([p, p, p]) == [abi.GS_OK] * 3
    wave.batch_run()
    for i in range(3):
        got, res = wave.batch_fetch(i)
        assert _diff(got, single) is None and _diff(got, want) is None, i
        assert (int(res.claim_prefix), int(res.node_prefix)) == prefixes, i


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OTHER_CASES))
def test_gpu_pod_chain_other_instantiations(wave, name):
    solve_checked(wave, name)
