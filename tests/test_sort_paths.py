"""Every build of the device NodeClaim sort, driven through Solve.

Solve re-sorts the in-flight NodeClaims with Go's unstable sort.Slice before
every pod, and the tie order decides which NodeClaim a pod lands on.  The
device has several builds of that sort (the single-wave LDS and HBM builds,
RegSort for at most 64 NodeClaims, the known-shape first partition, the block
kernel's own restatement, which the consolidation simulations also run).  The
scripted scenarios of tests/sort_scenarios.py hand each of them the hard
arrays through gs_solve / gs_consolidate with configuration flags only.

CPU tests (conditions on the inputs, no device): the oracle reports which
sort paths each scenario really reached (pyoracle.last_sort_paths) and floors
on that report make the coverage claim a checked fact; a mutant Solve with a
stable sort shows that every scenario's result depends on Go's tie order; the
builder's model is checked against the oracle; a census records what the
older random suites reach, which is the gap these scenarios close.

Neither Go's heapSort fallback nor choosePivot's reversal is reached: a
search over builder parameters (K 70..180, steering 0.8..1.0, steering at
q-1 only / the lower samples / all six, 667 scenarios, a minute of oracle
time) never counted heap_sort or reverse_range from a Solve, whose sort
inputs are one change away from sorted.  tests/test_wave_sort.py's
test_heapsort_inputs and test_register_frames_every_size stay their only
cover.

GPU tests: the whole Solve result bit-exact against the oracle on the three
solvers, the kernels' generic / fast sort counters against the oracle's
classes, and one consolidation simulation that replays a script.
"""
import pytest

import sort_scenarios as S
from gpusched import abi, synth
from gpusched.consolidation import ConsolidationInput
from oracle import pyoracle

VARIANTS = S.VARIANTS
IDS = [S.variant_id(v) for v in VARIANTS]
WAVE = [v for v in VARIANTS if v["k"] > 64]
REG_MID = [v for v in VARIANTS if v["k"] == 40]
REG_TOP = [v for v in VARIANTS if v["k"] in (60, 64)]

_oracle = {}


def oracle_of(v):
    """(result, sort paths) of the oracle's Solve of a variant, computed once"""
    key = S.variant_id(v)
    if key not in _oracle:
        st, want, _ = pyoracle.solve(S.scenario(v).problem)
        assert st == abi.GS_OK
        _oracle[key] = (want, pyoracle.last_sort_paths())
    return _oracle[key]


# ----------------------------------------------------------------- CPU: floors
@pytest.mark.parametrize("v", WAVE, ids=S.variant_id)
def test_wave_path_floors(v):
    """more than 64 NodeClaims: the wave-path pdqsort with its first partition
    (touched pivot), the one-rotation path (untouched), partitionEqual and
    breakPatterns"""
    _, h = oracle_of(v)
    big = h["hist"]["gt64"]
    assert big["touched"] >= 200, big
    assert all(n >= 10 for n in h["positions"]["gt64"].values()), h["positions"]["gt64"]
    assert big["untouched"] >= 100, big
    assert h["partition_equal"] >= 100
    assert h["break_patterns"] >= 50


@pytest.mark.parametrize("v", REG_MID, ids=S.variant_id)
def test_regsort_range_floors(v):
    """13-49 NodeClaims: every inversion runs the whole pdqsort in registers"""
    want, h = oracle_of(v)
    assert len(want["claims"]) == 40
    mid = h["hist"]["13_49"]
    assert mid["untouched"] + mid["touched"] + mid["multi"] >= 200, mid
    assert h["full_pdq"] == mid["untouched"] + mid["touched"] + mid["multi"]


@pytest.mark.parametrize("v", REG_TOP, ids=S.variant_id)
def test_regsort_boundary_floors(v):
    """50-64 NodeClaims with a touched pivot; the K = 64 scenarios open one
    more NodeClaim mid-script and go on at 65, on the wave path"""
    want, h = oracle_of(v)
    assert h["hist"]["50_64"]["touched"] >= 50, h["hist"]["50_64"]
    if v["k"] == 64:
        assert len(want["claims"]) == 65
        assert h["hist"]["gt64"]["touched"] >= 50, h["hist"]["gt64"]
    else:
        assert len(want["claims"]) == 60
        assert sum(h["hist"]["gt64"].values()) == 0


@pytest.mark.parametrize("v", [v for v in VARIANTS if v.get("late")], ids=S.variant_id)
def test_appended_claims_open_out_of_order(v):
    """the late openers wait until every count is >= 2, so each appended
    NodeClaim (count 1) is an inversion at the array's end, at M > 64"""
    want, h = oracle_of(v)
    assert len(want["claims"]) == v["k"] + v["late"]
    assert v["k"] > 64 and v["late"] >= 10
    assert S.scenario(v).appends_out_of_order == v["late"]
    assert h["tail"]["gt64"] >= v["late"], h["tail"]


# ---------------------------------------------- CPU: tie order, model, census
@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_result_depends_on_go_tie_order(v):
    want, _ = oracle_of(v)
    st, mutant, _ = pyoracle.solve_stable_ties(S.scenario(v).problem)
    assert st == abi.GS_OK
    assert mutant != want
    # the mutant leaves nothing behind: the next plain Solve is Go's again
    st, again, _ = pyoracle.solve(S.scenario(v).problem)
    assert again == want


@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_model_counts_equal_the_oracles(v):
    want, _ = oracle_of(v)
    assert not want["errors"]
    assert S.claim_counts(want) == S.scenario(v).model_counts


def test_topo_twins_run_the_same_script():
    for v in VARIANTS:
        if v.get("topo"):
            plain = dict(v, topo=False)
            assert oracle_of(v)[1] == oracle_of(plain)[1]
            assert S.claim_counts(oracle_of(v)[0]) == S.claim_counts(oracle_of(plain)[0])
            assert abi.GS_OK == pyoracle.solve(S.scenario(v).problem)[0]


def _sum_hist(problems):
    tot = {b: {s: 0 for s in pyoracle.SORT_STATES} for b in pyoracle.SORT_M_BUCKETS}
    for p in problems:
        assert pyoracle.solve(p)[0] == abi.GS_OK
        h = pyoracle.last_sort_paths()["hist"]
        for b in tot:
            for s in tot[b]:
                tot[b][s] += h[b][s]
    return tot


def test_census_of_the_random_suites():
    """what the older inputs reach, which is why the scenarios above exist:
    test_solve_random never leaves insertionSort (at most 12 NodeClaims), and
    test_solve_random_many_pods never sorts more than 64 NodeClaims with a
    touched pivot.  If synth changes and these flip, look at both suites."""
    small = _sum_hist(synth.random_problem(seed) for seed in range(150))
    assert sum(small["le12"].values()) > 0
    for b in ("13_49", "50_64", "gt64"):
        assert sum(small[b].values()) == 0, (b, small[b])
    many = _sum_hist(synth.random_problem(1000 + seed, n_pods=400, with_nodes=False) for seed in range(10))
    assert many["gt64"]["touched"] == 0, many["gt64"]


# ------------------------------------------------- consolidation (CPU part)
CONS_KW = [dict(k=100, n=600, seed=60, pods_milli=10_000), dict(k=100, n=600, seed=62, pods_milli=10_000)]
N_CAND = 8


def _cons_id(kw):
    return f"k{kw['k']}-s{kw['seed']}"


def _cons_input(kw):
    p = S.build(candidates=N_CAND, **kw).problem
    return p, ConsolidationInput(p, list(range(N_CAND)), mode=abi.CONSOLIDATE_EVAL, sets=[(0, N_CAND)])


@pytest.mark.parametrize("kw", CONS_KW, ids=_cons_id)
def test_consolidation_script_is_tie_order_sensitive(kw):
    """a command carries counts only: with ten pods of room per NodeClaim the
    NodeClaims fill up, and the tie order changes how many the replayed
    script opens -- the command's n_new_claims.  The simulation's Solve is
    the plain Solve of the same pods (same sort paths, same claim count), so
    the mutant's claim count on the plain problem is the mutant command's."""
    plain = S.build(**kw).problem
    st, want, _ = pyoracle.solve(plain)
    assert st == abi.GS_OK and not want["errors"]
    h = pyoracle.last_sort_paths()
    st, mutant, _ = pyoracle.solve_stable_ties(plain)
    assert st == abi.GS_OK and not mutant["errors"]
    assert len(mutant["claims"]) != len(want["claims"])
    _, cin = _cons_input(kw)
    st, cmds, _, _ = pyoracle.consolidate(cin)
    assert st == abi.GS_OK and len(cmds) == 1
    assert pyoracle.last_sort_paths() == h
    assert cmds[0]["n_new_claims"] == len(want["claims"]) and cmds[0]["n_failed_pods"] == 0
    assert cmds[0]["reason"] == abi.NOOP_MULTIPLE_CLAIMS
    assert h["hist"]["gt64"]["touched"] >= 100 and h["hist"]["gt64"]["untouched"] >= 100, h["hist"]["gt64"]


# ------------------------------------------------------------------------ GPU
SOLVER_FLAGS = {"wave": 0, "block": abi.GS_CFG_BLOCK_SOLVE, "hbm": abi.GS_CFG_CLAIMS_HBM}


@pytest.fixture(scope="module", params=list(SOLVER_FLAGS))
def solver(request):
    from gpusched.lib import Solver
    s = Solver(0, SOLVER_FLAGS[request.param])
    s.kind = request.param
    yield s
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("v", VARIANTS, ids=IDS)
def test_gpu_solve_equals_oracle(solver, v):
    """bit-exact parity of the whole result, and the sort counters.

    The block kernel counts at one place (ffd.hip, "the decision, identical in
    every wave"): an unsorted array of more than 12 NodeClaims is a fast sort
    when M >= 50 and choosePivot's hint on the whole array is "increasing",
    else a generic one.  Those are the oracle's one_rotation and full_pdq
    classes exactly, so the block kernel's counters must equal them.  The
    single-wave kernel counts fast sorts at several places (window rotation,
    run mode, batched placement), every one of them behind M >= 50, and a
    generic sort for every other unsorted array of more than 12: with K = 40
    (M stays below 50, where Go has no one-rotation path) its counters equal
    the oracle's too, fast = 0 among them; at M >= 50 they keep floors."""
    from test_gpu_parity import _diff
    want, h = oracle_of(v)
    got, res = solver.solve(S.scenario(v).problem)
    d = _diff(got, want)
    assert d is None, d
    print(f"sorts {S.variant_id(v)} {solver.kind}: generic {res.sorts_generic} fast {res.sorts_fast}"
          f" oracle full_pdq {h['full_pdq']} one_rotation {h['one_rotation']}")
    if solver.kind == "block" or v["k"] == 40:
        assert (res.sorts_generic, res.sorts_fast) == (h["full_pdq"], h["one_rotation"])
    else:
        assert res.sorts_generic >= 1 and res.sorts_fast >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("kw", CONS_KW, ids=_cons_id)
def test_gpu_consolidation_simulation_replays_the_script(kw):
    """one CONSOLIDATE_EVAL set over all candidates: the simulation kernel
    replays the script onto new NodeClaims (more than 64, touched pivots),
    and its command -- the claim count among it -- equals the oracle's"""
    from gpusched.lib import Solver
    from test_consolidation import check
    p, _ = _cons_input(kw)
    s = Solver(0)
    try:
        got = check(s, p, abi.CONSOLIDATE_EVAL, cands=list(range(N_CAND)), sets=[(0, N_CAND)])
    finally:
        s.close()
    assert got[0]["n_new_claims"] > 64
