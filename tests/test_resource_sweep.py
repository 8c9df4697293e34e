"""Every resource count R = 1..8 on every Solve kernel family.

The library compiles one kernel body per resource count for the wave Solve
(ffdw_kernel<R, TOPO, CH, WIDE>), the block and simulation kernel
(ffd_kernel<R, SIM, NT, TOPO>) and their batched forms; K1 and gs_explain loop
over the resources.  tests/resource_sweep.py builds, for each of 13 (R, layout)
pairs, the smallest problems that reach each of them; the layouts put cpu,
memory and pods below resource slot 4 (tail) or push them above it (head),
because the kernels keep slots 0..3 in LDS codes and slots 4..7 in the claim
records and only the first take the fast accept, run mode and the claim hint.

The CPU part shows, on the oracle alone, that the inputs are what they claim:
R names, the base resources in the promised slots, and every resource decides
something (taking its requests off the pods changes where pods land, or a
consolidation command).  The GPU part is bit for bit against the oracle.
"""
import pytest

import resource_sweep as rs
from gpusched import abi, lib

SINGLE, MULTI = abi.CONSOLIDATE_SINGLE, abi.CONSOLIDATE_MULTI
PAIR_IDS = [rs.pair_id(p) for p in rs.PAIRS]
pairs = pytest.mark.parametrize("pair", rs.PAIRS, ids=PAIR_IDS)
TAIL_HIGH = [p for p in rs.PAIRS if p[1] == "tail" and p[0] >= 5]   # only a pod asking for an extra has a high request
PODS_LOW = [p for p in rs.PAIRS if p[1] == "tail" or p[0] == 4]     # `pods` (if any) sits below slot 4


def slot(names, resource):
    return names.index(resource)


def high_pod(names, requests):
    """the pod has a request in a resource slot >= 4"""
    return any(slot(names, r) >= 4 for r, q in requests.items() if q)


# ============================================================ CPU: the inputs
@pairs
def test_names_and_slots(pair):
    R, layout = pair
    want = rs.resource_names(R, layout)
    assert len(want) == R
    for case in rs.CASES:
        names = rs.names_of(rs.problem(case, R, layout))
        assert len(names) == R and names == want, (case, names)
    base = [r for r in rs.BASE if r in want]
    assert base == list(rs.BASE[:min(R, 3)])
    for k, r in enumerate(base):
        assert slot(want, r) == (k if layout == "tail" else R - 3 + k), r
    if layout == "head":
        assert (slot(want, "pods") >= 4) == (R >= 5)
        assert all(slot(want, r) >= 4 for r in rs.BASE) == (R >= 7)


def test_nine_resources_are_nine():
    p = rs.nine_resources()
    assert len(rs.names_of(p)) == 9
    st, msg = lib.validate(p)
    assert st == abi.GS_E_UNSUPPORTED and "more than 8 distinct resources" in msg, (st, msg)


@pairs
@pytest.mark.parametrize("case", rs.SOLVE_CASES)
def test_every_resource_binds(pair, case):
    """the oracle solves the problem, and without the pod requests of any one
    resource its pods land elsewhere"""
    R, layout = pair
    assert lib.validate(rs.problem(case, R, layout)) == (abi.GS_OK, "")
    st, want, _ = rs.solved(case, R, layout)
    assert st == abi.GS_OK
    placed = rs.assignment(want)
    for r in rs.resource_names(R, layout):
        st, other, _ = rs.solved(case, R, layout, drop=r)
        assert st == abi.GS_OK
        assert rs.assignment(other) != placed, r


@pairs
@pytest.mark.parametrize("case", rs.CLUSTER_CASES)
def test_every_resource_binds_in_consolidation(pair, case):
    R, layout = pair
    assert lib.validate(rs.problem(case, R, layout)) == (abi.GS_OK, "")
    st, cmds, _, _ = rs.consolidated(case, R, layout)
    assert st == abi.GS_OK
    assert 60 <= len(cmds) <= 80
    kinds = {c["decision"] for c in cmds}
    assert len(kinds) >= 2 and abi.DECISION_REPLACE in kinds, kinds
    # one command that changes is enough: the candidate that runs the resource's
    # nine-tenths pod (a simulation does not depend on the other candidates)
    for k, r in enumerate(rs.resource_names(R, layout)):
        node = rs.CLUSTER_NODES + k
        assert rs.single_command(case, R, layout, node) == (abi.GS_OK, cmds[node])
        st, other = rs.single_command(case, R, layout, node, drop=r)
        assert st == abi.GS_OK
        assert other != cmds[node], r


@pairs
def test_shapes(pair):
    """what makes each case reach its kernels"""
    R, layout = pair
    for case in ("plain", "runs", "nodes", "general"):
        assert len(rs.problem(case, R, layout).instance_types) <= 64                 # one option word
    for case in ("wide", "wide_spread"):
        assert len(rs.problem(case, R, layout).instance_types) >= 257                # five: more than WREG
    for case in ("plain", "runs", "nodes", "wide", "cluster"):
        assert len(rs.problem(case, R, layout).spreads) == 0
    for case in ("general", "wide_spread", "cluster_general"):
        p = rs.problem(case, R, layout)
        keys = {p.strings[int(k)] for k in p.spreads["topology_key"]}
        assert keys == {rs.ZONE_KEY, rs.HOST_KEY}, (case, keys)
    p = rs.problem("general", R, layout)
    assert len(p.nodepools) == 2 and any(int(q["min_values"]) > 0 for q in p.reqs)
    assert len(rs.solved("runs", R, layout)[1]["claims"]) >= 60
    p, (_, want, _) = rs.problem("nodes", R, layout), rs.solved("nodes", R, layout)
    assert len(p.nodes) == 30 and len(p.bound_pods) > 0
    assert sum(len(x) for x in want["nodes"]) >= 0.2 * len(p.pods)
    assert len(want["claims"]) >= 3


@pairs
def test_plain_has_an_error_pod_per_slot(pair):
    """per resource slot (the high ones included) a pod that the oracle leaves
    unscheduled and that exceeds every type in that resource alone"""
    R, layout = pair
    p = rs.problem("plain", R, layout)
    names, top, rq = rs.names_of(p), rs.max_allocatable(p), rs.pod_requests(p)
    errors = rs.solved("plain", R, layout)[1]["errors"]
    short = {}
    for i in errors:
        over = [r for r, q in rq[i].items() if q > top[r]]
        if len(over) == 1:
            short.setdefault(slot(names, over[0]), []).append(i)
    assert sorted(short) == list(range(R)), short


@pytest.mark.parametrize("pair", TAIL_HIGH, ids=[rs.pair_id(p) for p in TAIL_HIGH])
@pytest.mark.parametrize("case", ["plain", "runs", "nodes"])
def test_tail_mixes_pods_with_and_without_high_requests(pair, case):
    R, layout = pair
    p = rs.problem(case, R, layout)
    names, rq = rs.names_of(p), rs.pod_requests(p)
    high = sum(high_pod(names, q) for q in rq)
    with_extra = sum(bool(set(q) - set(rs.BASE)) for q in rq)
    assert len(rq) - with_extra >= 0.3 * len(rq) and with_extra >= 0.1 * len(rq)
    assert high >= 0.1 * len(rq) and len(rq) - high >= 0.3 * len(rq)
    assert rs.hand_overs(p) >= 10


# ===================================================================== GPU
# Three tests, each a loop over the 13 pairs: the per-pair checks take
# milliseconds on the device, and the suite is kept to few test ids.  A check
# that fails is collected with its (solver, case, pair) and the loop goes on;
# anything but an AssertionError (a device error first of all) ends the test.
FLAGS = {"wave": 0, "hbm": abi.GS_CFG_CLAIMS_HBM, "block": abi.GS_CFG_BLOCK_SOLVE}


@pytest.fixture(scope="module")
def references():
    """every oracle result the GPU tests compare with, computed once"""
    for pair in rs.PAIRS:
        for case in rs.SOLVE_CASES + (rs.ROOMY,):
            assert rs.solved(case, *pair)[0] == abi.GS_OK
        for case in rs.CLUSTER_CASES:
            for mode in (SINGLE, MULTI) if pair in MULTI_PAIRS else (SINGLE,):
                assert rs.consolidated(case, *pair, mode)[0] == abi.GS_OK


@pytest.fixture(scope="module")
def wave(references):
    from gpusched.lib import Solver
    s = Solver(0, 0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def other(references):
    """a second context: gs_solve / gs_consolidate of one input alone"""
    from gpusched.lib import Solver
    s = Solver(0, 0)
    yield s
    s.close()


def each(check, items):
    """check(*item) for every item; the failed ones reported together"""
    failed = []
    for item in items:
        try:
            check(*item)
        except AssertionError as e:
            failed.append((item[1:] if hasattr(item[0], "ctx") else item, str(e)[:400]))
    assert not failed, failed


def solve_checked(s, case, pair):
    from test_gpu_parity import _diff
    st, want, prefixes = rs.solved(case, *pair)
    assert st == abi.GS_OK
    got, res = s.solve(rs.problem(case, *pair))
    d = _diff(got, want)
    assert d is None, d
    assert (int(res.claim_prefix), int(res.node_prefix)) == prefixes
    return got, res


def check_feasibility(s, case, pair):
    from test_gpu_parity import check_feas
    check_feas(s, rs.problem(case, *pair))


def joins(p, got):
    """the pods placed on a NodeClaim in flight (every pod of a claim but its
    first), and how many of them have a request in a slot >= 4"""
    names, rq = rs.names_of(p), rs.pod_requests(p)
    joined = [i for c in got["claims"] for i in c["pods"][1:]]
    return len(joined), sum(high_pod(names, rq[i]) for i in joined)


def check_runs_reach_run_mode(s, pair):
    """run mode and exact batches inside runs at this R, from the counters the
    library has: dbg[8] (pods placed in runs), dbg[14] (exact batches in runs)"""
    from test_exact_chain import counters
    got, res = solve_checked(s, "runs", pair)
    ctr = counters(s, res)
    joined, joined_high = joins(rs.problem("runs", *pair), got)
    print(rs.pair_id(pair), ctr, "joined a claim:", joined, "of them with a high request:", joined_high)
    if pair in PODS_LOW:
        assert ctr["pods"] > 0
    if pair in TAIL_HIGH:
        assert ctr["exact"] > 0
    # a pod with a high request joins a claim through the exact check only, as one of its candidates
    assert ctr["cand_full"] >= joined_high


def check_fast_accept_below_slot_four_only(s, pair):
    """gs_result's cand_full counts the candidates given the exact check, and a
    pod that joins a NodeClaim through the check was one of them.  So more
    joins than cand_full means pods accepted without the check (none of them
    has requirements here: simple pods), and cand_full below the joins of pods
    with a high request would mean one of those skipped it"""
    got, res = solve_checked(s, rs.ROOMY, pair)
    joined, joined_high = joins(rs.problem(rs.ROOMY, *pair), got)
    print(rs.pair_id(pair), "joined a claim:", joined, "with a high request:", joined_high,
          "cand_evals:", int(res.cand_evals), "cand_full:", int(res.cand_full))
    assert joined >= 170 and res.cand_evals >= joined
    assert res.cand_full >= joined_high
    if pair in PODS_LOW:
        # at R = 5 one of the two extended resources sits in slot 3: half of the 30 pods are high
        assert joined_high >= 10 if pair in TAIL_HIGH else joined_high == 0
        assert joined > res.cand_full
    else:
        assert joined_high == joined   # every pod asks for `pods` in a high slot


def check_explain_error_pods(s, pair):
    """gs_explain over the error pods of `plain` against tests/test_explain.py's
    model; a pod short in one resource, whatever its slot, is short of
    resources and not incompatible"""
    from test_explain import Model, _same
    p = rs.problem("plain", *pair)
    want = rs.solved("plain", *pair)[1]
    s.prepare(p)
    s.run()
    got, res = s.fetch()
    assert got["errors"] == want["errors"] and res.n_errors >= pair[0]
    errors = [int(res.error_pods[i]) for i in range(res.n_errors)]
    why = s.explain(pods=(res.error_pods, res.n_errors))
    assert why["pods"].tolist() == errors
    _same(why, Model(p).explain(pods=errors), rs.pair_id(pair))
    names, top, rq = rs.names_of(p), rs.max_allocatable(p), rs.pod_requests(p)
    seen = set()
    for j, i in enumerate(errors):
        over = [r for r, q in rq[i].items() if q > top[r]]
        if len(over) == 1:
            assert why["cause"][j, 0] == abi.GS_WHY_IT_RESOURCES, (i, over, int(why["cause"][j, 0]))
            seen.add(slot(names, over[0]))
    assert sorted(seen) == list(range(pair[0]))


@pytest.mark.gpu
def test_gpu_wave_context(wave):
    """on the default context, for every pair: the six Solve cases
    (ffdw_kernel<R, TOPO, 0, WIDE>; TOPO by the case: general, wide_spread;
    WIDE by the catalog: wide, wide_spread), K1 on plain and wide, the run and
    fast-accept counters, gs_explain on plain's error pods"""
    each(solve_checked, [(wave, case, pair) for case in rs.SOLVE_CASES for pair in rs.PAIRS])
    each(check_feasibility, [(wave, case, pair) for case in ("plain", "wide") for pair in rs.PAIRS])
    each(check_runs_reach_run_mode, [(wave, pair) for pair in rs.PAIRS])
    each(check_fast_accept_below_slot_four_only, [(wave, pair) for pair in rs.PAIRS])
    each(check_explain_error_pods, [(wave, pair) for pair in rs.PAIRS])


@pytest.mark.gpu
def test_gpu_hbm_and_block_contexts(references):
    """the six Solve cases of every pair with the claim state in HBM
    (ffdw_kernel<R, TOPO, 1, WIDE>) and on the block kernel
    (ffd_kernel<R, false, FB_MAX, TOPO>)"""
    from gpusched.lib import Solver
    for name in ("hbm", "block"):
        s = Solver(0, FLAGS[name])
        try:
            each(solve_checked, [(s, case, pair) for case in rs.SOLVE_CASES for pair in rs.PAIRS])
        finally:
            s.close()


# MultiNode mode on an odd and an even R of each layout, low and high (the
# oracle's prefix sweep costs as much as the rest of a pair's consolidation checks)
MULTI_PAIRS = [(1, "tail"), (6, "tail"), (5, "head"), (8, "head")]


def _sim_of(cmds, decision):
    return next(i for i, c in enumerate(cmds) if c["decision"] == decision)


def check_consolidation(s, case, pair):
    """ffd_kernel<R, true, FB_SIM, TOPO>: SingleNode commands (and, on
    MULTI_PAIRS, MultiNode ones) equal the oracle's; the scheduling Results of
    one Delete and one Replace simulation equal the oracle's Solve of that
    simulation's problem"""
    from test_consolidation_results import consistent, oracle_results
    p = rs.problem(case, *pair)
    for mode in ((MULTI, SINGLE) if pair in MULTI_PAIRS else (SINGLE,)):
        st, want, chosen, multi = rs.consolidated(case, *pair, mode)
        assert st == abi.GS_OK
        cmds, got_chosen, got_multi, _ = s.consolidate(rs.cluster_input(case, *pair, mode))
        assert cmds == want, next((i, a, b) for i, (a, b) in enumerate(zip(cmds, want)) if a != b)
        assert (got_chosen, got_multi) == (chosen, multi)
    for decision in (abi.DECISION_DELETE, abi.DECISION_REPLACE):
        i = _sim_of(cmds, decision)
        got, _ = s.consolidation_results(i)
        assert got == oracle_results(p, [i]), (decision, i)
        consistent(p, cmds[i], got)


BATCH = [("plain", p) for p in rs.PAIRS] + [("general", (r, "tail")) for r in range(1, 9)]


def check_batch_solve(wave, other):
    """ffd_wave_batch_r<R>_t<T>: one batch over the plain problem of every pair
    and the general one of R = 1..8; every slot equals the oracle and gs_solve
    alone, through gs_batch_fetch and gs_batch_fetch_all"""
    from test_gpu_parity import _diff
    problems = [rs.problem(case, *pair) for case, pair in BATCH]
    assert wave.batch_prepare(problems) == [abi.GS_OK] * len(BATCH)
    wave.batch_run()
    stats = wave.batch_stats()
    assert stats["n_fallback"] == 0 and stats["n_groups"] >= 8 and stats["n_batched"] == len(BATCH), stats
    everything, statuses = wave.batch_fetch_all()
    assert statuses == [abi.GS_OK] * len(BATCH)
    for i, (case, pair) in enumerate(BATCH):
        st, want, prefixes = rs.solved(case, *pair)
        alone, _ = other.solve(problems[i])
        for got, res in (wave.batch_fetch(i), everything[i]):
            assert _diff(got, want) is None and _diff(got, alone) is None, (i, case, pair, _diff(got, want))
            assert (int(res.claim_prefix), int(res.node_prefix)) == prefixes, (i, case, pair)


def check_batch_consolidate(wave, other):
    """ffd_sim_batch_r<R>_t<T>: the cluster inputs of R = 1..8 in both forms in
    one batch; every slot equals the oracle and gs_consolidate alone, through
    the per-slot fetch and fetch_all"""
    from test_batch_consolidation import Case, _check_slot
    from test_batch_consolidation_fetch_all import Tables
    which = [(case, r) for case in rs.CLUSTER_CASES for r in range(1, 9)]
    cases = [Case(rs.problem(case, r, "tail"), SINGLE) for case, r in which]
    for c, (case, r) in zip(cases, which):
        c._oracle = rs.consolidated(case, r, "tail")[1:]  # computed once, shared with the checks above
    assert wave.batch_consolidate_prepare([c.input() for c in cases]) == [abi.GS_OK] * len(cases)
    wave.batch_consolidate_run()
    stats = wave.batch_consolidate_stats()
    assert stats["n_fallback"] == 0 and stats["n_batched"] == len(cases) and stats["n_groups"] >= 8, stats
    tables, statuses = wave.batch_consolidate_fetch_all()
    assert statuses == [abi.GS_OK] * len(cases)
    for i, c in enumerate(cases):
        _check_slot(wave, i, c, other)
        _check_slot(Tables(tables), i, c, other)


def check_nine_resources_are_refused(wave):
    from test_gpu_parity import _diff
    nine = rs.nine_resources()
    with pytest.raises(lib.GpuSchedError) as e:
        wave.solve(nine)
    assert e.value.status == abi.GS_E_UNSUPPORTED and "more than 8 distinct resources" in str(e.value)
    solve_checked(wave, "plain", (8, "tail"))   # the context goes on
    eight, one = rs.problem("plain", 8, "head"), rs.problem("plain", 1, "tail")
    assert wave.batch_prepare([eight, nine, one]) == [abi.GS_OK, abi.GS_E_UNSUPPORTED, abi.GS_OK]
    assert "more than 8 distinct resources" in wave.batch_error(1)
    wave.batch_run()
    assert _diff(wave.batch_fetch(0)[0], rs.solved("plain", 8, "head")[1]) is None
    assert _diff(wave.batch_fetch(2)[0], rs.solved("plain", 1, "tail")[1]) is None
    with pytest.raises(lib.GpuSchedError) as e:
        wave.batch_fetch(1)
    assert e.value.status == abi.GS_E_UNSUPPORTED


@pytest.mark.gpu
def test_gpu_consolidation_batches_and_the_limit(wave, other):
    """the simulation kernel on both cluster forms of every pair, the batched
    Solve and consolidation kernels, and the refusal of a ninth resource"""
    each(check_consolidation, [(wave, case, pair) for case in rs.CLUSTER_CASES for pair in rs.PAIRS])
    check_batch_solve(wave, other)
    check_batch_consolidate(wave, other)
    check_nine_resources_are_refused(wave)
