"""gs_consolidation_results: the scheduling Results of one consolidation
simulation (<U> SimulateScheduling's return value; computeConsolidation builds
Command.Replacements from results.NewNodeClaims[0]).

A command says how a simulation ended, not where its pods went: a simulation
kernel that placed a Delete's pods on the wrong existing nodes, within
capacity, passes every command comparison.  The tests here compare the whole
result -- NodeClaims (NodePool, pods in add order, instance types,
requirements, requests), the pods each existing node received in add order,
and the error pods -- with the oracle's Solve of the problem the simulation
solves: consolidation.sub_problem builds it (pending pods plus the candidates'
bound pods over the nodes that are not candidates), exactly as the oracle's
own simulate() does, and the CPU tests pin that equivalence against
pyoracle.consolidate's commands.
"""
import functools

import pytest

from gpusched import abi, lib, synth
from gpusched.consolidation import ConsolidationInput, n_multi_sims, sub_problem
from oracle import pyoracle

SINGLE, MULTI, EVAL = abi.CONSOLIDATE_SINGLE, abi.CONSOLIDATE_MULTI, abi.CONSOLIDATE_EVAL
MODES = [SINGLE, MULTI]


def _c4_small():
    return synth.make_c4(n_nodes=40, n_pending=3, seed=0, util=(0.85, 0.99), full_frac=0.6, big_frac=0.6)


def _c4_narrow():
    # 1,100 simulations: the 128-thread simulation shape on a 256-CU part
    return synth.make_c4(n_nodes=1100, n_pending=0, util=(0.9, 0.99), full_frac=0.5, big_frac=1.0, pack=True)


FAMILIES = {
    "rand": lambda s: synth.random_consolidation(s),
    "c4": lambda s: _c4_small(),
    "general": lambda s: synth.random_consolidation_general(s),
    "minvalues": lambda s: synth.random_consolidation_general(100 + s, min_values=True),
    "ct": lambda s: synth.random_consolidation_general(s, ct_spreads=True),
    "np": lambda s: synth.random_consolidation_general(s, np_spreads=True),
    "honor": lambda s: synth.random_honor_filter(s, consolidation=True),
}
SEEDS = {"rand": range(12), "c4": range(1), "general": range(24), "minvalues": range(12), "ct": range(12),
         "np": range(12), "honor": range(24)}
BASE_KINDS = ["rand", "c4"]                         # the clusters the CPU tests pin sub_problem on
GPU_KINDS = BASE_KINDS + ["general", "minvalues", "ct", "np"]


@functools.lru_cache(maxsize=None)
def problem(kind, seed):
    return FAMILIES[kind](seed)


def sets_of(mode, cands, sets=None):
    """the candidate set of every simulation (consolidate.cpp build_sets)"""
    if mode == EVAL:
        return [list(cands[b:b + n]) for b, n in sets]
    if mode == SINGLE:
        return [[c] for c in cands]
    return [list(cands[:mid + 1]) for mid in range(1, n_multi_sims(len(cands)) + 1)]


def oracle_results(p, cset):
    """the oracle's Solve of the simulation's problem, in the cluster's pod and
    node numbering -> the dict gs_consolidation_results must equal"""
    q, pm, nm = sub_problem(p, cset)
    st, r, _ = pyoracle.solve(q)
    assert st == abi.GS_OK
    nodes = [[] for _ in range(len(p.nodes))]
    for j, pods in enumerate(r["nodes"]):
        nodes[int(nm[j])] = [int(pm[x]) for x in pods]
    claims = [dict(c, pods=[int(pm[x]) for x in c["pods"]]) for c in r["claims"]]
    return {"claims": claims, "nodes": nodes, "errors": sorted(int(pm[x]) for x in r["errors"])}


def failed_pods(p, res):
    """<U> !AllNonPendingPodsScheduled: error pods that are not pending, and
    non-pending pods placed on uninitialized nodes"""
    n = len(p.pods)
    bad = sum(1 for x in res["errors"] if x >= n)
    for node, pods in enumerate(res["nodes"]):
        if not p.nodes["initialized"][node]:
            bad += sum(1 for x in pods if x >= n)
    return bad


@functools.lru_cache(maxsize=None)
def reference(kind, seed, mode):
    """the oracle's result of every simulation, computed once and shared
    (never modified) by the tests below"""
    p = problem(kind, seed)
    cands = list(range(len(p.nodes)))
    return [oracle_results(p, s) for s in sets_of(mode, cands)]


@functools.lru_cache(maxsize=None)
def oracle_commands(kind, seed, mode):
    p = problem(kind, seed)
    st, cmds, _, _ = pyoracle.consolidate(ConsolidationInput(p, list(range(len(p.nodes))), mode=mode))
    assert st == abi.GS_OK
    return cmds


# ---------------------------------------------------------------------- CPU
@pytest.mark.parametrize("kind", BASE_KINDS)
@pytest.mark.parametrize("mode", MODES)
def test_sub_problem_is_the_simulations_solve(kind, mode):
    """a plain Solve of sub_problem(...) ends as the oracle's simulate() does:
    same NodeClaim count, same failed non-pending pods"""
    for seed in SEEDS[kind]:
        p = problem(kind, seed)
        cmds, results = oracle_commands(kind, seed, mode), reference(kind, seed, mode)
        assert len(cmds) == len(results)
        for i, (c, r) in enumerate(zip(cmds, results)):
            assert len(r["claims"]) == c["n_new_claims"], (seed, i)
            assert failed_pods(p, r) == c["n_failed_pods"], (seed, i)


def test_sub_problem_maps():
    p = _c4_small()
    q, pm, nm = sub_problem(p, [5, 2])
    n = len(p.pods)
    moved = [b for c in (5, 2) for b in range(len(p.bound_pods)) if p.bound_node[b] == c]
    assert [int(x) for x in pm] == list(range(n)) + [n + b for b in moved]
    assert [int(x) for x in nm] == [x for x in range(len(p.nodes)) if x not in (2, 5)]
    assert q.struct.n_pods == n + len(moved) and q.struct.n_nodes == len(p.nodes) - 2
    assert q.struct.n_bound_pods == len(p.bound_pods) - len(moved)
    assert (q.pods[n:] == p.bound_pods[moved]).all()
    stay = [b for b in range(len(p.bound_pods)) if p.bound_node[b] not in (2, 5)]
    assert [int(nm[x]) for x in q.bound_node] == [int(p.bound_node[b]) for b in stay]
    # the cluster itself is untouched
    assert p.struct.n_pods == n and p.struct.n_nodes == len(p.nodes)


def test_oracle_results_cover_the_ground():
    """the clusters the GPU tests compare on hold every kind of result: a
    changed generator cannot hollow those tests out"""
    two, many, failed, deletes, replaces = 0, 0, 0, 0, 0
    for kind, seed in [(k, x) for k in BASE_KINDS for x in SEEDS[k]]:
        p = problem(kind, seed)
        for mode in MODES:
            for c, r in zip(oracle_commands(kind, seed, mode), reference(kind, seed, mode)):
                two += len(r["claims"]) == 2
                many += len(r["claims"]) >= 3
                failed += failed_pods(p, r) > 0
                deletes += c["decision"] == abi.DECISION_DELETE and sum(len(x) for x in r["nodes"]) >= 2
                replaces += c["decision"] == abi.DECISION_REPLACE
    print("claims == 2:", two, " >= 3:", many, " failed pods:", failed, " deletes placing >= 2 pods:", deletes,
          " replaces:", replaces)
    assert two + many >= 1 and failed >= 1 and deletes >= 1 and replaces >= 1


# ---------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def solver():
    from gpusched.lib import Solver
    s = Solver(0)
    yield s
    s.close()


def consistent(p, cmd, res):
    """the result agrees with the command the sweep decided"""
    assert len(res["claims"]) == cmd["n_new_claims"]
    assert failed_pods(p, res) == cmd["n_failed_pods"]
    if cmd["decision"] == abi.DECISION_REPLACE:
        assert res["claims"][0]["nodepool"] == cmd["nodepool"]
        it = iter(res["claims"][0]["its"])
        assert all(o in it for o in cmd["options"]), (cmd["options"], res["claims"][0]["its"])  # subsequence, in order


def check_all(solver, p, mode, want_results):
    """every simulation's results against the oracle's, their consistency with
    the commands, and that asking disturbs neither the commands nor a rerun"""
    cands = list(range(len(p.nodes)))
    first = solver.consolidate(ConsolidationInput(p, cands, mode=mode))[:3]
    cmds = first[0]
    assert len(cmds) == len(want_results)
    got = []
    for i, cmd in enumerate(cmds):
        res, _ = solver.consolidation_results(i)
        assert res == want_results[i], (i, res, want_results[i])
        consistent(p, cmd, res)
        got.append(res)
    assert solver.consolidate_rerun()[:3] == first
    for i in {0, len(cmds) - 1} & set(range(len(cmds))):
        assert solver.consolidation_results(i)[0] == got[i]  # after a rerun
        assert solver.consolidation_results(i)[0] == got[i]  # and twice


@pytest.mark.gpu
@pytest.mark.parametrize("kind", GPU_KINDS)
@pytest.mark.parametrize("mode", MODES)
def test_gpu_results_match_oracle(solver, kind, mode):
    for seed in SEEDS[kind]:
        check_all(solver, problem(kind, seed), mode, reference(kind, seed, mode))


@pytest.mark.gpu
def test_gpu_results_honor_filter(solver):
    """a seed the product refuses is left out, as tests/test_consolidation_general.py does"""
    ran = 0
    for seed in SEEDS["honor"]:
        p = problem("honor", seed)
        if len(p.nodes) == 0:
            continue
        try:
            solver.consolidate(ConsolidationInput(p, list(range(len(p.nodes))), mode=SINGLE))
        except lib.GpuSchedError as e:
            if e.status == abi.GS_E_UNSUPPORTED and "without its owner's node affinity" in str(e):
                continue
            raise
        check_all(solver, p, SINGLE, reference("honor", seed, SINGLE))
        ran += 1
    assert ran > 0


@pytest.mark.gpu
def test_gpu_results_eval_sets(solver):
    p = synth.random_consolidation(7, n_nodes=12, n_pending=2)
    cands = list(range(12))
    sets = [(0, 1), (1, 3), (0, 0), (4, 8), (2, 10)]
    cmds = solver.consolidate(ConsolidationInput(p, cands, mode=EVAL, sets=sets))[0]
    st, want, _, _ = pyoracle.consolidate(ConsolidationInput(p, cands, mode=EVAL, sets=sets))
    assert st == abi.GS_OK and cmds == want
    for i, cset in enumerate(sets_of(EVAL, cands, sets)):
        res, _ = solver.consolidation_results(i)
        assert res == oracle_results(p, cset), i
        consistent(p, cmds[i], res)


@pytest.mark.gpu
def test_gpu_results_shard_filter(solver):
    kind, seed = "rand", 3
    p = problem(kind, seed)
    cands = list(range(len(p.nodes)))
    results = reference(kind, seed, SINGLE)
    cmds = solver.consolidate(ConsolidationInput(p, cands, mode=SINGLE, shard=(1, 3)))[0]
    assert len(cmds) >= 4
    for i, cmd in enumerate(cmds):
        if i % 3 != 1:
            assert cmd["decision"] == abi.DECISION_SKIPPED
            with pytest.raises(lib.GpuSchedError) as e:
                solver.consolidation_results(i)
            assert e.value.status == abi.GS_E_INVALID
        else:
            assert solver.consolidation_results(i)[0] == results[i], i


@pytest.mark.gpu
def test_gpu_results_misuse():
    from gpusched.lib import Solver
    s = Solver(0)
    try:
        s.cluster = problem("rand", 0)
        with pytest.raises(lib.GpuSchedError) as e:
            s.consolidation_results(0)
        assert e.value.status == abi.GS_E_INVALID
        p = problem("rand", 0)
        cmds = s.consolidate(ConsolidationInput(p, list(range(len(p.nodes))), mode=SINGLE))[0]
        with pytest.raises(lib.GpuSchedError) as e:
            s.consolidation_results(len(cmds))
        assert e.value.status == abi.GS_E_INVALID
        s.consolidation_results(len(cmds) - 1)
        # a provisioning Solve replaces the resident consolidation
        s.solve(synth.make_c1(n_pods=20))
        with pytest.raises(lib.GpuSchedError) as e:
            s.consolidation_results(0)
        assert e.value.status == abi.GS_E_INVALID
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_results_library_shards(mode):
    from gpusched.lib import Solver
    kind, seed = "general", 5
    p = problem(kind, seed)
    s = Solver(0, shard_devices=[0, 0])
    try:
        check_all(s, p, mode, reference(kind, seed, mode))
    finally:
        s.close()


@pytest.fixture(scope="module")
def narrow():
    return _c4_narrow()


@pytest.mark.gpu
def test_gpu_results_after_narrow_sweep(solver, narrow):
    """1,100 simulations run in the 128-thread shape with their add logs in
    LDS; the requested simulation runs again alone.  A sample against the
    oracle's Solve of each derived problem (the oracle's whole consolidate
    takes half a minute on this cluster)."""
    p = narrow
    cmds = solver.consolidate(ConsolidationInput(p, list(range(1100)), mode=SINGLE))[0]
    assert len(cmds) == 1100
    sample = list(range(0, 1100, 70))
    for i in sample:
        res, raw = solver.consolidation_results(i)
        assert res == oracle_results(p, [i]), i
        consistent(p, cmds[i], res)
        assert sum(len(x) for x in res["nodes"]) >= 1, i  # every one places pods on existing nodes
        assert raw.pops >= sum(len(x) for x in res["nodes"])
    assert {cmds[i]["decision"] for i in sample} == {abi.DECISION_DELETE, abi.DECISION_REPLACE, abi.DECISION_NOOP}
    assert solver.consolidate_rerun()[0] == cmds


@pytest.mark.gpu
def test_gpu_results_widest_multi_prefix(solver, narrow):
    """MultiNodeConsolidation's last prefix: 101 candidates' pods onto the 999 nodes kept"""
    p = narrow
    cands = list(range(1100))
    cmds = solver.consolidate(ConsolidationInput(p, cands, mode=MULTI))[0]
    assert len(cmds) == 100
    cset = sets_of(MULTI, cands)[99]
    assert len(cset) == 101
    res, _ = solver.consolidation_results(99)
    assert res == oracle_results(p, cset)
    consistent(p, cmds[99], res)
