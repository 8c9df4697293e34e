"""gs_batch_consolidate_fetch_all: every slot of a consolidation batch decided
in one device pass.

For every slot the call must give what the per-slot fetch gives: the oracle's
consolidation of the input (the comparison of test_batch_consolidation.py) and,
field by field with bit-equal prices and the counters, the per-slot fetch of a
second context that holds the same batch.  The inputs are chosen so that the
oracle's own commands hold every decision class; the shapes cross the gather's
wave and group boundaries; a bad slot leaves the others alone; the number of
device operations does not grow with the slots.
"""
import ctypes as C

import pytest

from gpusched import abi, lib, synth
from gpusched.consolidation import ConsolidationInput
from oracle import pyoracle  # noqa: F401  (the cases' oracle)

from test_batch_consolidation import (COUNTERS, EVAL, MULTI, SINGLE, Case, _check_slot, _zone_affinity_cluster, mixed)


def _c4(seed, n_nodes=28):
    return synth.make_c4(n_nodes=n_nodes, n_pending=3, seed=seed, util=(0.85, 0.99), full_frac=0.6, big_frac=0.6)


_CASES = {}


def case(name):
    """the inputs this file adds to test_batch_consolidation.mixed(), built once"""
    if not _CASES:
        _CASES.update({
            "min_values": Case(synth.random_consolidation_general(175, min_values=True), SINGLE),  # a MIN_VALUES NoOp
            "not_cheaper": Case(_c4(30), SINGLE),    # the price filter leaves no option: 16 NOT_CHEAPER
            "sixty": Case(_c4(5), SINGLE),           # Replace commands that keep all 60 options
            "multi_replace": Case(_c4(6), MULTI),    # a chosen MULTI Replace with multi_options
            "one_sim": Case(synth.random_consolidation(5), SINGLE, cands=[2]),
        })
    return _CASES[name]


def mixed25():
    return mixed() + [case(n) for n in ("min_values", "not_cheaper", "sixty", "multi_replace")]


def _reasons(cmds):
    return {c["reason"] for c in cmds if c["decision"] == abi.DECISION_NOOP}


# ------------------------------------------------------------------ CPU
def test_fetch_all_null_context():
    """the new entry points refuse a NULL context without touching a device"""
    L = lib.load()
    res = abi.GsConsolidationResult()
    status = (C.c_int * 1)()
    stats = abi.GsBatchFetchStats()
    assert L.gs_batch_consolidate_fetch_all(None, C.byref(res), status) == abi.GS_E_INVALID
    assert L.gs_batch_consolidate_last_fetch(None, C.byref(stats)) == abi.GS_E_INVALID
    assert L.gs_batch_fetch_stats_size() > 0


def test_fetch_stats_layout():
    assert lib.load().gs_batch_fetch_stats_size() == C.sizeof(abi.GsBatchFetchStats)


def test_inputs_cover_every_outcome():
    """the oracle's own commands over the mixed batch hold every class the
    decision separates, so a gather that drops one cannot pass vacuously"""
    decisions, reasons, multi_replace, sixty = set(), set(), False, False
    for c in mixed25():
        cmds, chosen, multi = c.oracle()
        decisions |= {x["decision"] for x in cmds}
        reasons |= _reasons(cmds)
        sixty = sixty or any(len(x["options"]) == 60 for x in cmds)
        if c.mode == MULTI and chosen >= 0 and cmds[chosen]["decision"] == abi.DECISION_REPLACE and multi:
            multi_replace = True
    assert {abi.DECISION_DELETE, abi.DECISION_REPLACE} <= decisions
    assert {abi.NOOP_UNSCHEDULABLE, abi.NOOP_MULTIPLE_CLAIMS, abi.NOOP_NOT_CHEAPER, abi.NOOP_SPOT_TO_SPOT,
            abi.NOOP_MIN_VALUES} <= reasons
    assert multi_replace and sixty
    assert {c.mode for c in mixed25()} == {SINGLE, MULTI, EVAL}


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def solver():
    from gpusched.lib import Solver
    s = Solver(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def other():
    """the second context: the same batch, fetched slot by slot"""
    from gpusched.lib import Solver
    s = Solver(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def plain():
    """the third context of _check_slot: every input alone through gs_consolidate"""
    from gpusched.lib import Solver
    s = Solver(0)
    yield s
    s.close()


class Tables:
    """fetch_all's tables behind the per-slot fetch's name, for _check_slot"""

    def __init__(self, tables):
        self.tables = tables

    def batch_consolidate_fetch(self, i):
        return self.tables[i]


def _full(t):
    """every field of the contract: the commands with their options and
    bit-equal prices, chosen, multi_options, pods_simulated and the counters"""
    cmds, chosen, multi, res = t
    return cmds, chosen, multi, {k: int(getattr(res, k)) for k in COUNTERS}


def _prepare_run(s, cases):
    st = s.batch_consolidate_prepare([c.input() for c in cases])
    s.batch_consolidate_run()
    return st


def _both(solver, other, cases):
    """the batch on both contexts; fetch_all on the first -> (tables, fetch stats)"""
    assert _prepare_run(solver, cases) == [abi.GS_OK] * len(cases)
    assert _prepare_run(other, cases) == [abi.GS_OK] * len(cases)
    tables, status = solver.batch_consolidate_fetch_all()
    assert status == [abi.GS_OK] * len(cases)
    fs = solver.batch_consolidate_fetch_stats()
    run = solver.batch_consolidate_stats()
    assert fs["n_slots"] == len(cases)
    assert fs["n_decided"] + fs["n_per_slot"] == run["n_accepted"], (fs, run)
    return tables, fs


def _check_all(solver, other, plain, cases):
    tables, fs = _both(solver, other, cases)
    for i, c in enumerate(cases):
        _check_slot(Tables(tables), i, c, plain)
        assert _full(tables[i]) == _full(other.batch_consolidate_fetch(i)), i
        assert tables[i][3].t_fetch_ms == fs["wall_ms"]
    return tables, fs


@pytest.mark.gpu
def test_mixed_batch_parity(solver, other, plain):
    """25 slots over both simulation-kernel forms, a minValues group, every
    mode, a shard filter and empty candidate lists"""
    cases = mixed25()
    tables, fs = _check_all(solver, other, plain, cases)
    run = solver.batch_consolidate_stats()
    assert run["n_groups"] >= 3 and run["n_fallback"] == 0, run
    no_sims = sum(1 for t in tables if all(c["decision"] == abi.DECISION_SKIPPED for c in t[0]))
    assert no_sims == 2 and fs["n_per_slot"] == no_sims and fs["n_decided"] == len(cases) - no_sims, fs
    assert [c["decision"] for c in tables[17][0]].count(abi.DECISION_SKIPPED) == 40 - 13


@pytest.mark.gpu
def test_one_slot_one_simulation(solver, other, plain):
    tables, fs = _check_all(solver, other, plain, [case("one_sim")])
    assert len(tables[0][0]) == 1 and fs["n_decided"] == 1


@pytest.mark.gpu
def test_simulation_counts_cross_waves(solver, other, plain):
    """one group whose slots hold 1, 63, 64, 65 and 130 simulations: the grid is
    sized by the largest, the others' waves return early"""
    p = _c4(5)
    sets = sorted((b, n) for n in range(1, 6) for b in range(28 - n + 1))  # 28 + 27 + 26 + 25 + 24 ranges
    assert len(sets) == 130
    cases = [Case(p, EVAL, sets=sets[:n]) for n in (63, 1, 130, 64, 65)]
    tables, fs = _check_all(solver, other, plain, cases)
    assert solver.batch_consolidate_stats()["n_groups"] == 1
    assert [len(t[0]) for t in tables] == [63, 1, 130, 64, 65] and fs["n_decided"] == 5
    assert any(c["decision"] == abi.DECISION_REPLACE for c in tables[2][0][64:])


@pytest.mark.gpu
def test_sixty_options_and_none(solver, other, plain):
    tables, _ = _check_all(solver, other, plain, [case("sixty"), case("not_cheaper")])
    assert any(len(c["options"]) == 60 for c in tables[0][0])
    assert abi.NOOP_NOT_CHEAPER in _reasons(tables[1][0])


@pytest.mark.gpu
def test_empty_option_region_first(solver, other, plain):
    """two groups, one without any single-NodeClaim simulation: in either group
    order, and with both kinds in both groups"""
    m = mixed()
    lack_plain, have_plain, lack_general, have_general = m[4], m[2], m[8], m[11]
    for c in (lack_plain, lack_general):
        assert all(x["n_new_claims"] != 1 or x["n_failed_pods"] for x in c.oracle()[0])
    for c in (have_plain, have_general):
        assert any(x["decision"] == abi.DECISION_REPLACE for x in c.oracle()[0])
    for cases in ([lack_plain, have_general], [have_plain, lack_general],
                  [lack_plain, lack_general, have_general, have_plain]):
        _, fs = _check_all(solver, other, plain, cases)
        assert solver.batch_consolidate_stats()["n_groups"] >= 2
        assert fs["n_copies"] == 2, fs  # a prepared batch's first call: the records, then the options
    # no option list anywhere: the records alone
    _, fs = _check_all(solver, other, plain, [lack_plain, lack_general])
    assert fs["n_copies"] == 1, fs


@pytest.mark.gpu
def test_bad_slots(solver, other, plain):
    """test_batch_consolidation's refused slots: GS_E_INVALID at 1 and 7,
    GS_E_UNSUPPORTED at 3; the five good slots are exact"""
    good = mixed()[:3] + mixed()[8:10]
    ins = [c.input() for c in good]
    p = synth.random_consolidation(8)
    no_cluster = ConsolidationInput(p, [0])
    no_cluster.struct.cluster = C.POINTER(abi.GsProblem)()
    ins.insert(1, ConsolidationInput(p, [0, len(p.nodes) + 5]))
    ins.insert(3, ConsolidationInput(_zone_affinity_cluster(), [0]))
    ins.append(no_cluster)
    bad = {1: abi.GS_E_INVALID, 3: abi.GS_E_UNSUPPORTED, 7: abi.GS_E_INVALID}
    want = [bad.get(i, abi.GS_OK) for i in range(8)]
    for s in (solver, other):
        assert s.batch_consolidate_prepare(ins) == want
        s.batch_consolidate_run()
    tables, status = solver.batch_consolidate_fetch_all()
    assert status == want
    fs = solver.batch_consolidate_fetch_stats()
    assert fs["n_slots"] == 8 and fs["n_decided"] + fs["n_per_slot"] == 5, fs
    for i in bad:
        assert tables[i] is None
        assert solver.batch_consolidate_error(i) == other.batch_consolidate_error(i) != ""
    assert "out of range" in solver.batch_consolidate_error(1)
    assert "null" in solver.batch_consolidate_error(7)
    for i, c in zip([i for i in range(8) if i not in bad], good):
        _check_slot(Tables(tables), i, c, plain)
        assert _full(tables[i]) == _full(other.batch_consolidate_fetch(i)), i


@pytest.mark.gpu
def test_operations_independent_of_slots(solver, other, plain):
    """4 slots of two families, then 48: the same launches and transfers"""
    fam = [Case(synth.random_consolidation(s, n_nodes=24, n_pending=s % 3), SINGLE) for s in (30, 31)]
    fam += [mixed()[2], mixed()[11]]
    _, f4 = _check_all(solver, other, plain, fam)
    g4 = solver.batch_consolidate_stats()["n_groups"]
    many = [fam[i % 4] for i in range(48)]
    tables, f48 = _both(solver, other, many)
    for i in range(48):
        assert _full(tables[i]) == _full(other.batch_consolidate_fetch(i)), i
    assert solver.batch_consolidate_stats()["n_groups"] == g4 >= 2
    assert f48["n_launches"] == f4["n_launches"] > 0
    assert f48["n_copies"] == f4["n_copies"] > 0
    assert f48["n_decided"] == 48 and f4["n_decided"] == 4


@pytest.mark.gpu
def test_ordering_and_reuse(solver, other, plain):
    cases = mixed()[6:12] + [case("sixty")]
    n = len(cases)
    ins = [c.input() for c in cases]
    assert solver.batch_consolidate_prepare(ins) == [abi.GS_OK] * n
    with pytest.raises(lib.GpuSchedError) as e:  # before a run
        solver.batch_consolidate_fetch_all()
    assert e.value.status == abi.GS_E_INVALID
    solver.batch_consolidate_run()
    assert _prepare_run(other, cases) == [abi.GS_OK] * n
    want = [_full(other.batch_consolidate_fetch(i)) for i in range(n)]
    # a slot fetched on its own first keeps its table
    assert _full(solver.batch_consolidate_fetch(2)) == want[2]
    tables, status = solver.batch_consolidate_fetch_all()
    assert status == [abi.GS_OK] * n and [_full(t) for t in tables] == want
    fs = solver.batch_consolidate_fetch_stats()
    assert fs["n_decided"] == n - 1 and fs["n_per_slot"] == 1, fs
    # every slot counts as fetched: the per-slot fetch returns the same table
    assert [_full(solver.batch_consolidate_fetch(i)) for i in range(n)] == want
    # twice: identical, from the cached tables
    tables, status = solver.batch_consolidate_fetch_all()
    assert status == [abi.GS_OK] * n and [_full(t) for t in tables] == want
    assert solver.batch_consolidate_fetch_stats()["n_decided"] == 0
    # a new run invalidates the tables; the gathered ones are the same again
    solver.batch_consolidate_run()
    tables, _ = solver.batch_consolidate_fetch_all()
    assert [_full(t) for t in tables] == want
    fs = solver.batch_consolidate_fetch_stats()
    assert fs["n_decided"] == n and fs["n_copies"] == 1, fs  # the options ride with the records now
    # a Replace's simulation again: its Results agree with the command
    slot, sim = next((i, k) for i, t in enumerate(tables) for k, c in enumerate(t[0])
                     if c["decision"] == abi.DECISION_REPLACE)
    cmd = tables[slot][0][sim]
    res, _ = solver.batch_consolidate_results(slot, sim)
    assert len(res["claims"]) == cmd["n_new_claims"] == 1
    its = iter(res["claims"][0]["its"])
    assert all(o in its for o in cmd["options"])  # a subsequence of claim_its
    assert [_full(solver.batch_consolidate_fetch(i)) for i in range(n)] == want
    # a smaller batch afterwards on the same context: the staging is reused
    _check_all(solver, other, plain, cases[4:6])
