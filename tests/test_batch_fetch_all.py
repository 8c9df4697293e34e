"""gs_batch_fetch_all: every slot of a Solve batch fetched in one device pass.

Every result must equal, field by field, what gs_batch_fetch yields for the
slot on the same run (and the oracle's Solve, and gs_solve of the problem
alone); a refused or failed slot must leave the others alone; the number of
device operations must not depend on the number of slots.  The oracle results
are computed once per problem and shared; the edge slots the GPU tests rely on
are checked on the oracle in the CPU part.
"""
import ctypes as C

import pytest

from gpusched import abi, lib, synth
from gpusched.problem import ProblemBuilder
from oracle import pyoracle
from test_batch import _accepted, _claim_overflow, _diff, _duplicate_uid, _empty_pods, _two_domain_keys, mixed

# the raw gs_result fields the contract lists beside the structural ones
COUNTERS = ("checks", "pops", "cand_evals", "cand_full", "claim_prefix", "node_prefix", "sorts_fast", "sorts_generic",
            "t_ffd_sort_ms", "t_ffd_scan_ms", "t_ffd_template_ms", "words", "n_templates", "n_variants")


# ------------------------------------------------------------ the edge slots
def _placed_and_errors():
    """existing nodes take some pods, NodeClaims others, the rest are errors"""
    return synth.random_problem(0)


def _all_errors():
    """every pod asks for more cpu than any instance type has"""
    b = ProblemBuilder()
    synth.build_catalog(b, synth.FAKE_PROFILES, synth.FAKE_ZONES, spot=False, prices=synth.price_table(synth.FAKE_PROFILES))
    b.add_nodepool("default")
    for i in range(7):
        b.add_pod(f"huge{i}", i, {"cpu": 10_000_000, "memory": 1 << 30, "pods": 1000})
    return b.build()


def _sixty_and_fewer():
    """200 instance types; a small pod per zone (a required zone keeps the
    three apart): the first two fit more than 60 types, so their NodeClaims
    carry the full Truncate(60) row; the third asks for 200 cpu, which only a
    few types offer"""
    b = ProblemBuilder()
    profs = synth.c2_profiles(200)
    synth.build_catalog(b, profs, synth.FAKE_ZONES, spot=False, prices=synth.price_table(profs))
    b.add_nodepool("default")
    z = "topology.kubernetes.io/zone"
    b.add_pod("small0", 0, {"cpu": 500, "memory": 1 << 30, "pods": 1000}, node_selector={z: synth.FAKE_ZONES[0]})
    b.add_pod("small1", 1, {"cpu": 500, "memory": 1 << 30, "pods": 1000}, node_selector={z: synth.FAKE_ZONES[1]})
    b.add_pod("large", 2, {"cpu": 200_000, "memory": 1 << 30, "pods": 1000}, node_selector={z: synth.FAKE_ZONES[2]})
    return b.build()


def _many_claims():
    """more than 64 NodeClaims: more than one wave of claim records"""
    return synth.random_problem(1000, n_pods=400, with_nodes=False)


def _truncation_drop():
    """Truncate(60) drops the only NodeClaim (minValues on the family, the 60
    cheapest options all one family): its pods come back as errors.  This is
    synth.min_values_truncation, the repository's constructed case:
    synth.random_min_values gives no way to tell a truncation drop from any
    other pod error in the oracle's Results, so no seed search is made."""
    return synth.min_values_truncation()


_EDGES = []


def edges():
    """[(name, problem, oracle result)] of the edge slots (built once)"""
    if not _EDGES:
        for name, make in (("empty", _empty_pods), ("placed_and_errors", _placed_and_errors),
                           ("all_errors", _all_errors), ("sixty_and_fewer", _sixty_and_fewer),
                           ("many_claims", _many_claims), ("truncation_drop", _truncation_drop)):
            p = make()
            assert lib.validate(p) == (abi.GS_OK, ""), name
            st, want, _ = pyoracle.solve(p)
            assert st == abi.GS_OK, name
            _EDGES.append((name, p, want))
    return _EDGES


_C2 = []


def c2_slot():
    """synth.make_c2(2000): a 32 KB add log and 54 NodeClaims, more than one
    workgroup pass of the copy kernel"""
    if not _C2:
        p = synth.make_c2(2000)
        st, want, _ = pyoracle.solve(p)
        assert st == abi.GS_OK
        _C2.append((p, want))
    return _C2[0]


_TEN = []


def ten():
    """the ten 60-pod problems of test_batch.test_more_workgroups_than_cus"""
    if not _TEN:
        _TEN.extend(_accepted(lambda s: synth.random_problem(5000 + s, n_pods=60), 0, 10))
    return _TEN


@pytest.fixture(scope="module")
def solver():
    from gpusched.lib import Solver
    s = Solver(0)
    yield s
    s.close()


def _prepare_run(s, cases):
    st = s.batch_prepare([p for p, _ in cases])
    s.batch_run()
    return st


def _check_all(s, cases, skip=()):
    """batch_fetch_all: every slot GS_OK and equal to its oracle result -> (results, fetch stats)"""
    results, st = s.batch_fetch_all()
    assert len(results) == len(cases)
    for i, (_, want) in enumerate(cases):
        if i in skip:
            continue
        assert st[i] == abi.GS_OK, (i, st[i], s.batch_error(i))
        d = _diff(results[i][0], want)
        assert d is None, (i, d)
    return results, s.batch_fetch_stats()


# ------------------------------------------------------------------ CPU
def test_null_context():
    """both entry points refuse a NULL context without touching a device"""
    L = lib.load()
    res = (abi.GsResult * 1)()
    status = (C.c_int * 1)()
    stats = abi.GsBatchFetchStats()
    assert L.gs_batch_fetch_all(None, res, status) == abi.GS_E_INVALID
    assert L.gs_batch_last_fetch(None, C.byref(stats)) == abi.GS_E_INVALID


def test_exported_and_declared():
    assert {"gs_batch_fetch_all", "gs_batch_last_fetch"} <= set(lib.EXPORTS)
    assert lib.load().gs_batch_fetch_stats_size() == C.sizeof(abi.GsBatchFetchStats)


def test_edge_slots_are_what_they_claim():
    """on the oracle: the inputs of the GPU tests have the shapes they are there for"""
    e = {name: (p, want) for name, p, want in edges()}
    p, want = e["empty"]
    assert len(p.pods) == 0 and not want["claims"] and not want["errors"]
    p, want = e["placed_and_errors"]
    placed = sum(len(c["pods"]) for c in want["claims"]) + sum(len(n) for n in want["nodes"])
    assert placed > 0 and want["errors"] and any(want["nodes"]) and want["claims"]
    assert placed + len(want["errors"]) == len(p.pods)
    p, want = e["all_errors"]
    assert len(p.pods) == 7 and want["errors"] == list(range(7)) and not want["claims"]
    p, want = e["sixty_and_fewer"]
    sizes = sorted(len(c["its"]) for c in want["claims"])
    assert not want["errors"] and sizes[-1] == 60 and 0 < sizes[0] < 60, sizes
    p, want = e["many_claims"]
    assert len(want["claims"]) > 64
    p, want = e["truncation_drop"]
    assert not want["claims"] and want["errors"] == [0, 1, 2]
    p, want = c2_slot()
    assert len(p.pods) == 2000 and len(want["claims"]) > 16


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_mixed_batch_equals_per_slot_fetch(solver):
    """mixed() (at least four kernel groups), the edge slots and one C2 slot:
    every result equals the oracle, batch_fetch(i) on a second context that ran
    the same batch (raw counters included) and gs_solve of the problem alone"""
    from gpusched.lib import Solver
    cases = list(mixed()) + [(p, want) for _, p, want in edges()] + [c2_slot()]
    n = len(cases)
    st = _prepare_run(solver, cases)
    assert st == [abi.GS_OK] * n
    stats = solver.batch_stats()
    assert stats["n_groups"] >= 4 and stats["n_fallback"] == 0 and stats["n_batched"] == n, stats
    results, fs = _check_all(solver, cases)
    assert fs["n_slots"] == n and fs["n_decided"] == n and fs["n_per_slot"] == 0, fs
    assert fs["n_launches"] > 0 and 1 <= fs["n_copies"] <= 2 and fs["bytes"] > 0, fs
    t_fetch = {results[i][1].t_fetch_ms for i in range(n)}
    assert len(t_fetch) == 1 and t_fetch.pop() == pytest.approx(fs["wall_ms"])
    other = Solver(0)
    try:
        assert _prepare_run(other, cases) == [abi.GS_OK] * n
        for i in range(n):
            got, raw = other.batch_fetch(i)
            d = _diff(results[i][0], got)
            assert d is None, (i, d)
            for k in COUNTERS:
                assert getattr(results[i][1], k) == getattr(raw, k), (i, k)
            for k in ("t_encode_ms", "t_upload_ms", "t_feas_ms", "t_ffd_ms", "t_truncate_ms"):
                assert getattr(results[i][1], k) >= 0
    finally:
        other.close()
    plain = Solver(0)
    try:
        for i, (p, _) in enumerate(cases):
            alone, _ = plain.solve(p)
            d = _diff(results[i][0], alone)
            assert d is None, (i, d)
    finally:
        plain.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_slots(solver, n):
    cases = [mixed()[1], c2_slot()][:n]
    assert _prepare_run(solver, cases) == [abi.GS_OK] * n
    _, fs = _check_all(solver, cases)
    assert fs["n_decided"] == n and fs["n_per_slot"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [63, 64, 65, 257, 600])
def test_slot_counts_across_wave_and_workgroup_edges(solver, n):
    """the sizing pass scans 64 slots per wave and 256 per round"""
    cases = [ten()[i % 10] for i in range(n)]
    assert _prepare_run(solver, cases) == [abi.GS_OK] * n
    _, fs = _check_all(solver, cases)
    assert fs["n_decided"] == n and fs["n_per_slot"] == 0, fs


@pytest.mark.gpu
def test_the_largest_batch(solver):
    """GS_BATCH_MAX slots of a five-pod problem"""
    p = synth.make_c1(n_pods=5)
    st, want, _ = pyoracle.solve(p)
    assert st == abi.GS_OK
    n = abi.GS_BATCH_MAX
    assert solver.batch_prepare([p] * n) == [abi.GS_OK] * n
    solver.batch_run()
    raw, st = solver.batch_fetch_all(raw=True)
    assert st == [abi.GS_OK] * n
    fs = solver.batch_fetch_stats()
    assert fs["n_decided"] == n and fs["n_copies"] <= 2, fs
    for i in range(n):
        assert abi.result_to_dict(raw[i], p) == want, i


@pytest.mark.gpu
def test_bad_slots_and_invalid_calls(solver):
    cases = list(mixed()[:6])
    cases.insert(2, (_two_domain_keys(), None))
    cases.insert(5, (_duplicate_uid(), None))
    st = solver.batch_prepare([p for p, _ in cases])
    want = [abi.GS_OK] * 8
    want[2], want[5] = abi.GS_E_UNSUPPORTED, abi.GS_E_INVALID
    assert st == want
    # before the run: the call is refused
    res = (abi.GsResult * 8)()
    status = (C.c_int * 8)()
    assert solver.L.gs_batch_fetch_all(solver.ctx, res, status) == abi.GS_E_INVALID
    assert solver.batch_fetch_stats()["n_slots"] == 0  # zero before the first fetch_all
    solver.batch_run()
    assert solver.L.gs_batch_fetch_all(solver.ctx, None, status) == abi.GS_E_INVALID
    assert solver.L.gs_batch_fetch_all(solver.ctx, res, None) == abi.GS_E_INVALID
    results, st = solver.batch_fetch_all()
    assert st == want
    for i in (2, 5):
        assert results[i] is None
        assert solver.batch_error(i) == lib.validate(cases[i][0])[1] != ""
    _check_all(solver, cases, skip=(2, 5))
    fs = solver.batch_fetch_stats()
    assert fs["n_slots"] == 8 and fs["n_decided"] == 6 and fs["n_per_slot"] == 0, fs
    # a refused slot's out[i] is zeroed
    raw, _ = solver.batch_fetch_all(raw=True)
    for i in (2, 5):
        assert bytes(raw[i]) == bytes(C.sizeof(abi.GsResult))
    # n == 0: GS_OK and no device operation
    assert solver.batch_prepare([]) == []
    solver.batch_run()
    assert solver.L.gs_batch_fetch_all(solver.ctx, None, None) == abi.GS_OK
    fs = solver.batch_fetch_stats()
    assert fs["n_launches"] == 0 and fs["n_copies"] == 0 and fs["n_slots"] == 0, fs


@pytest.mark.gpu
def test_fallback_slot_takes_the_per_slot_path(solver):
    """the slot that outgrows its LDS NodeClaims reruns alone and is fetched as
    gs_batch_fetch does, between two gathered slots"""
    from gpusched.lib import Solver
    big = _claim_overflow()
    blk = Solver(0, abi.GS_CFG_BLOCK_SOLVE)
    try:
        want_big, _ = blk.solve(big)
    finally:
        blk.close()
    assert len(want_big["claims"]) == 2700 and not want_big["errors"]
    small = mixed()[1:3]
    cases = [small[0], (big, want_big), small[1]]
    assert _prepare_run(solver, cases) == [abi.GS_OK] * 3
    for run in range(2):
        if run:
            solver.batch_run()
        stats = solver.batch_stats()
        assert stats["n_fallback"] == 1 and stats["n_batched"] == 2, (run, stats)
        _, fs = _check_all(solver, cases)
        assert fs["n_per_slot"] == 1 and fs["n_decided"] == 2, (run, fs)


@pytest.mark.gpu
def test_block_solve_context_fetches_every_slot_alone():
    from gpusched.lib import Solver
    cases = mixed()[:6]
    s = Solver(0, abi.GS_CFG_BLOCK_SOLVE)
    try:
        assert _prepare_run(s, cases) == [abi.GS_OK] * 6
        _, fs = _check_all(s, cases)
        assert fs["n_decided"] == 0 and fs["n_per_slot"] == 6 and fs["n_launches"] == 0, fs
    finally:
        s.close()


@pytest.mark.gpu
def test_operations_do_not_depend_on_the_slot_count(solver):
    """the same launches and steady-state transfers for 14 and for 42 slots; one
    transfer of the same size once a run repeats on the same upload"""
    seen = {}
    for cases in (list(mixed()), [c for c in mixed() for _ in range(3)]):
        n = len(cases)
        assert _prepare_run(solver, cases) == [abi.GS_OK] * n
        _, first = _check_all(solver, cases)
        assert first["n_copies"] <= 2, first
        solver.batch_run()
        _, second = _check_all(solver, cases)
        solver.batch_run()
        _, third = _check_all(solver, cases)
        assert second["n_copies"] == 1 and third["n_copies"] == 1, (second, third)
        assert second["bytes"] == third["bytes"] and second["n_launches"] == third["n_launches"]
        seen[n] = second
    assert seen[14]["n_launches"] == seen[42]["n_launches"] > 0
    assert seen[14]["n_copies"] == seen[42]["n_copies"] == 1
    assert seen[42]["bytes"] > seen[14]["bytes"]


@pytest.mark.gpu
def test_ordering_and_reuse(solver):
    cases = list(mixed())
    own_p, own_want = cases[3]
    solver.prepare(own_p)
    solver.run()
    assert _prepare_run(solver, cases) == [abi.GS_OK] * 14
    before = [solver.batch_fetch(i)[0] for i in range(14)]
    results, _ = _check_all(solver, cases)
    assert [r[0] for r in results] == before
    assert [solver.batch_fetch(i)[0] for i in range(14)] == before
    # a second fetch_all without a run in between
    again, st = solver.batch_fetch_all()
    assert st == [abi.GS_OK] * 14 and [r[0] for r in again] == before
    # all n results are valid at once: slot 0's still decodes after slot 13's was written
    raw, _ = solver.batch_fetch_all(raw=True)
    assert [abi.result_to_dict(raw[i], cases[i][0]) for i in (13, 0, 7)] == [before[13], before[0], before[7]]
    # the context's own prepared problem survives
    got, _ = solver.fetch()
    assert _diff(got, own_want) is None
    # a smaller batch after a larger one
    three = cases[7:10]
    assert _prepare_run(solver, three) == [abi.GS_OK] * 3
    _, fs = _check_all(solver, three)
    assert fs["n_slots"] == 3 and fs["n_decided"] == 3
