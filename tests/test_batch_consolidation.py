"""gs_batch_consolidate_*: the consolidation simulations of many independent
clusters on one context, in a number of device operations that does not
depend on how many clusters they are.

Every slot of a batch must equal the oracle's consolidation of its input
(commands, chosen, multi_options) and gs_consolidate of the input alone on a
second context (also options, prices and the counters), whatever the mix of
kernel instantiations, modes and shard filters; a bad slot must leave the
others alone; the number of device operations must not grow with the number
of slots; the batch must leave the context's other resident state alone.
The oracle's and the solo context's outcomes are computed once per input and
shared.
"""
import ctypes as C

import numpy as np
import pytest

from gpusched import abi, lib, synth
from gpusched.consolidation import ConsolidationInput
from gpusched.problem import ProblemBuilder
from oracle import pyoracle

SINGLE, MULTI, EVAL = abi.CONSOLIDATE_SINGLE, abi.CONSOLIDATE_MULTI, abi.CONSOLIDATE_EVAL
Z = "topology.kubernetes.io/zone"
COUNTERS = ("pods_simulated", "checks", "node_evals", "node_prefix", "pops")


class Case:
    """one consolidation input with what it must give (filled lazily, once)"""

    def __init__(self, problem, mode=SINGLE, cands=None, sets=None, shard=(0, 0), max_candidates=0):
        self.problem = problem
        self.mode, self.sets, self.shard, self.max_candidates = mode, sets, shard, max_candidates
        self.cands = list(range(len(problem.nodes))) if cands is None else list(cands)
        self._oracle = self._solo = None

    def input(self, shard=None):
        return ConsolidationInput(self.problem, self.cands, mode=self.mode, sets=self.sets,
                                  max_candidates=self.max_candidates, shard=self.shard if shard is None else shard)

    def oracle(self):
        """(commands, chosen, multi_options) of the whole input (the oracle knows no shard filter)"""
        if self._oracle is None:
            st, cmds, chosen, multi = pyoracle.consolidate(self.input(shard=(0, 0)))
            assert st == abi.GS_OK
            self._oracle = (cmds, chosen, multi)
        return self._oracle

    def solo(self, plain):
        """gs_consolidate of the input alone: (commands, chosen, multi_options, counters)"""
        if self._solo is None:
            cmds, chosen, multi, res = plain.consolidate(self.input())
            self._solo = (cmds, chosen, multi, {k: int(getattr(res, k)) for k in COUNTERS})
        return self._solo


def _c4_small(seed=0):
    return synth.make_c4(n_nodes=40, n_pending=3, seed=seed, util=(0.85, 0.99), full_frac=0.6, big_frac=0.6)


_MIXED = []


def mixed():
    """the 21 inputs of the mixed batch (built once)"""
    if not _MIXED:
        c = []
        c += [Case(synth.random_consolidation(s), SINGLE) for s in (0, 1)]
        c += [Case(synth.random_consolidation(s), MULTI) for s in (2, 3)]
        c += [Case(synth.random_consolidation(s, n_nodes=24, n_pending=s % 3), SINGLE) for s in (20, 22)]
        c += [Case(_c4_small(0), SINGLE), Case(_c4_small(0), MULTI)]
        c += [Case(synth.random_consolidation_general(s), SINGLE) for s in (0, 1)]
        c += [Case(synth.random_consolidation_general(s), MULTI) for s in (2, 3)]
        c += [Case(synth.random_consolidation_general(0, ct_spreads=True), SINGLE),
              Case(synth.random_consolidation_general(1, ct_spreads=True), MULTI)]
        c += [Case(synth.random_consolidation_general(100, min_values=True), SINGLE),
              Case(synth.random_consolidation_general(101, min_values=True), MULTI)]
        # hand-made sets (tests/test_consolidation.py test_gpu_consolidation_eval_sets)
        c.append(Case(synth.random_consolidation(7, n_nodes=12, n_pending=2), EVAL, cands=range(12),
                      sets=[(0, 1), (1, 3), (0, 0), (4, 8), (2, 10)]))
        c.append(Case(_c4_small(1), SINGLE, shard=(1, 3)))           # SKIPPED elsewhere
        c.append(Case(synth.random_consolidation(4), SINGLE, cands=[]))  # no simulation at all
        c.append(Case(synth.random_consolidation(5), SINGLE, cands=[2]))
        c.append(Case(synth.random_consolidation(6), MULTI, cands=[1]))  # MULTI of one candidate: no simulation
        assert len(c) == 21
        _MIXED.extend(c)
    return _MIXED


@pytest.fixture(scope="module")
def solver():
    from gpusched.lib import Solver
    s = Solver(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def plain():
    """the second context: every input alone through gs_consolidate"""
    from gpusched.lib import Solver
    s = Solver(0)
    yield s
    s.close()


def _run(s, cases):
    ins = [c.input() for c in cases]
    st = s.batch_consolidate_prepare(ins)
    s.batch_consolidate_run()
    return st, s.batch_consolidate_stats(), ins


def _fetch(s, i):
    cmds, chosen, multi, res = s.batch_consolidate_fetch(i)
    return cmds, chosen, multi, {k: int(getattr(res, k)) for k in COUNTERS}


def _check_slot(s, i, case, plain, oracle=True):
    got = _fetch(s, i)
    assert got == case.solo(plain), (i, got, case.solo(plain))
    if not oracle:
        return
    want, want_chosen, want_multi = case.oracle()
    cmds, chosen, multi, _ = got
    assert len(cmds) == len(want), i
    sc = case.shard[1]
    for k, (g, w) in enumerate(zip(cmds, want)):
        if sc and k % sc != case.shard[0]:
            assert g["decision"] == abi.DECISION_SKIPPED, (i, k)
        else:
            assert g == w, (i, k, g, w)
    if not sc:
        assert (chosen, multi) == (want_chosen, want_multi), i


# ------------------------------------------------------------------ CPU
def test_batch_consolidate_null_context():
    """every entry point refuses a NULL context without touching a device"""
    L = lib.load()
    cin = ConsolidationInput(synth.random_consolidation(0), [0])
    ptrs = (C.POINTER(abi.GsConsolidation) * 1)(C.pointer(cin.struct))
    status = (C.c_int * 1)()
    res = abi.GsConsolidationResult()
    sres = abi.GsResult()
    stats = abi.GsBatchStats()
    buf = C.create_string_buffer(64)
    assert L.gs_batch_consolidate_prepare(None, ptrs, 1, status) == abi.GS_E_INVALID
    assert L.gs_batch_consolidate_run(None) == abi.GS_E_INVALID
    assert L.gs_batch_consolidate_fetch(None, 0, C.byref(res)) == abi.GS_E_INVALID
    assert L.gs_batch_consolidate_results(None, 0, 0, C.byref(sres)) == abi.GS_E_INVALID
    assert L.gs_batch_consolidate_error(None, 0, buf, 64) == 0
    assert L.gs_batch_consolidate_last_run(None, C.byref(stats)) == abi.GS_E_INVALID


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_mixed_batch_bit_exact(solver, plain):
    """21 slots over at least three kernel groups, every mode, a shard filter,
    an empty candidate list and a single candidate: every slot equals the
    oracle and gs_consolidate of the input alone"""
    cases = mixed()
    st, stats, _ = _run(solver, cases)
    assert st == [abi.GS_OK] * len(cases)
    assert stats["n_problems"] == len(cases) and stats["n_accepted"] == len(cases)
    assert stats["n_groups"] >= 3, stats
    assert stats["n_fallback"] == 0 and stats["n_batched"] == len(cases), stats
    for i, c in enumerate(cases):
        _check_slot(solver, i, c, plain)
    # the slots the test is about are what they claim to be
    assert [c["decision"] for c in _fetch(solver, 17)[0]].count(abi.DECISION_SKIPPED) == 40 - 13
    assert _fetch(solver, 18)[0] == [] and _fetch(solver, 20)[0] == []
    assert len(_fetch(solver, 19)[0]) == 1


@pytest.mark.gpu
def test_launches_independent_of_slots(solver, plain):
    """2 slots of one family, then 48: the same groups, the same number of
    device operations"""
    fam = [Case(synth.random_consolidation(s, n_nodes=24, n_pending=s % 3), SINGLE) for s in (30, 31)]
    st, s2, _ = _run(solver, fam)
    assert st == [abi.GS_OK] * 2
    for i, c in enumerate(fam):
        _check_slot(solver, i, c, plain)
    many = [fam[i % 2] for i in range(48)]
    st, s48, _ = _run(solver, many)
    assert st == [abi.GS_OK] * 48
    for i, c in enumerate(many):
        _check_slot(solver, i, c, plain, oracle=False)
    assert s48["n_batched"] == 48 and s48["n_fallback"] == 0, s48
    assert s48["n_groups"] == s2["n_groups"] >= 1
    assert s48["n_launches"] == s2["n_launches"] > 0


@pytest.mark.gpu
def test_more_simulations_than_workgroups(solver, plain):
    """24-node SINGLE sweeps, enough slots that the simulations exceed 8 per
    CU: the persistent loop draws more than once and workgroups queue behind
    residency; every slot equals its solo run"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    four = [Case(synth.random_consolidation(s, n_nodes=24, n_pending=s % 3), SINGLE) for s in (32, 33, 34, 35)]
    n = (8 * cus) // 24 + 1
    cases = [four[i % 4] for i in range(n)]
    assert sum(len(c.cands) for c in cases) > 8 * cus
    st, stats, _ = _run(solver, cases)
    assert st == [abi.GS_OK] * n
    assert stats["n_batched"] == n and stats["n_fallback"] == 0, stats
    for i, c in enumerate(cases):
        _check_slot(solver, i, c, plain, oracle=i < 4)


def _zone_affinity_cluster():
    """a pending pod with required pod affinity on the zone key: refused"""
    b = ProblemBuilder()
    synth.build_catalog(b, synth.FAKE_PROFILES, synth.FAKE_ZONES, spot=False,
                        prices=synth.price_table(synth.FAKE_PROFILES))
    b.add_nodepool("default")
    b.add_node("n0", {Z: synth.FAKE_ZONES[0]}, {"cpu": 4000, "memory": 8 << 30, "pods": 110_000})
    b.add_pod("x", 0, {"cpu": 1}, affinity=[{"key": Z, "required": True, "selector": {"labels": {"app": "web"}}}])
    return b.build()


@pytest.mark.gpu
def test_bad_slots_poison_nothing(solver, plain):
    good = mixed()[:3] + mixed()[8:10]
    ins = [c.input() for c in good]
    p = synth.random_consolidation(8)
    out_of_range = ConsolidationInput(p, [0, len(p.nodes) + 5])
    unsupported = ConsolidationInput(_zone_affinity_cluster(), [0])
    no_cluster = ConsolidationInput(p, [0])
    no_cluster.struct.cluster = C.POINTER(abi.GsProblem)()
    ins.insert(1, out_of_range)
    ins.insert(3, unsupported)
    ins.append(no_cluster)
    bad = {1: abi.GS_E_INVALID, 3: abi.GS_E_UNSUPPORTED, 7: abi.GS_E_INVALID}
    st = solver.batch_consolidate_prepare(ins)
    assert st == [bad.get(i, abi.GS_OK) for i in range(8)]
    solver.batch_consolidate_run()
    stats = solver.batch_consolidate_stats()
    assert stats["n_problems"] == 8 and stats["n_accepted"] == 5 and stats["n_fallback"] == 0, stats
    # each bad slot's message is its own: the one gs_consolidate gives for that input
    for i, want in bad.items():
        with pytest.raises(lib.GpuSchedError) as alone:
            plain.consolidate(ins[i])
        assert alone.value.status == want
        msg = solver.batch_consolidate_error(i)
        assert msg != "" and str(alone.value).endswith(msg), (i, msg, str(alone.value))
        with pytest.raises(lib.GpuSchedError) as e:
            solver.batch_consolidate_fetch(i)
        assert e.value.status == want
    assert "out of range" in solver.batch_consolidate_error(1)
    assert "null" in solver.batch_consolidate_error(7)
    slots = [i for i in range(8) if i not in bad]
    for i, c in zip(slots, good):
        _check_slot(solver, i, c, plain)


@pytest.mark.gpu
def test_reuse(solver, plain):
    cases = mixed()[6:12]
    # a smaller batch first, then a larger one on the same context
    st, _, _ = _run(solver, cases[:2])
    assert st == [abi.GS_OK] * 2
    for i, c in enumerate(cases[:2]):
        _check_slot(solver, i, c, plain)
    st, _, ins = _run(solver, cases)
    assert st == [abi.GS_OK] * 6
    first = [_fetch(solver, i) for i in range(6)]
    for i, c in enumerate(cases):
        assert first[i] == c.solo(plain), i
    # run twice: identical (and a fetch without a run in between too)
    assert [_fetch(solver, i) for i in range(6)] == first
    solver.batch_consolidate_run()
    assert [_fetch(solver, i) for i in range(6)] == first
    # every caller array overwritten: the batch kept none of them
    rng = np.random.default_rng(0)
    scratch = [Case(synth.random_consolidation_general(50 + k), SINGLE) for k in range(2)]
    scratch += [Case(_c4_small(5), MULTI)]
    want = [c.solo(plain) for c in scratch]
    sins = [c.input() for c in scratch]
    assert solver.batch_consolidate_prepare(sins) == [abi.GS_OK] * 3
    for c, cin in zip(scratch, sins):
        p = c.problem
        for arr in (p.quantities, p.reqs, p.labels, p.offerings, p.instance_types, p.nodes, p.pods, p.bound_pods,
                    p.value_ids, p.bound_node, cin.candidates):
            if len(arr):
                raw = arr.view(np.uint8)
                raw[:] = rng.integers(0, 256, size=raw.shape, dtype=np.uint8)
    solver.batch_consolidate_run()
    assert [_fetch(solver, i) for i in range(3)] == want
    solver.batch_consolidate_run()
    assert [_fetch(solver, i) for i in range(3)] == want


@pytest.mark.gpu
def test_independence(solver, plain):
    """a Solve, a Solve batch and a resident consolidation on the context
    survive the consolidation batch"""
    own = synth.random_problem(3)
    st, own_want, _ = pyoracle.solve(own)
    assert st == abi.GS_OK
    solver.prepare(own)
    solver.run()
    assert solver.fetch()[0] == own_want
    bp = [synth.random_problem(s) for s in (5, 6)]
    assert solver.batch_prepare(bp) == [abi.GS_OK] * 2
    solver.batch_run()
    batch_want = [solver.batch_fetch(i)[0] for i in range(2)]
    # (gs_consolidate replaces the context's prepared Solve by design: take the
    # resident consolidation on the context first, the Solve after it)
    resident = Case(_c4_small(2), SINGLE)
    res_want = solver.consolidate(resident.input())[:3]
    assert res_want == resident.solo(plain)[:3]
    cases = mixed()[:4] + mixed()[8:10]
    st, _, _ = _run(solver, cases)
    assert st == [abi.GS_OK] * 6
    for i, c in enumerate(cases):
        _check_slot(solver, i, c, plain, oracle=False)
    assert [solver.batch_fetch(i)[0] for i in range(2)] == batch_want
    assert solver.consolidate_rerun()[:3] == res_want
    # the single prepared Solve next to a consolidation batch
    solver.prepare(own)
    solver.run()
    st, _, _ = _run(solver, cases)
    assert st == [abi.GS_OK] * 6
    assert solver.fetch()[0] == own_want
    for i, c in enumerate(cases):
        _check_slot(solver, i, c, plain, oracle=False)


@pytest.mark.gpu
def test_results_per_slot(solver, plain):
    """batch_consolidate_results(i, sim) equals consolidation_results(sim) of
    the input alone, for every simulation of a simple, a general and a MULTI
    slot; asking changes neither a fetch nor a run"""
    cases = [Case(synth.random_consolidation(9), SINGLE), Case(synth.random_consolidation_general(4), SINGLE),
             Case(synth.random_consolidation_general(100, min_values=True), SINGLE),
             Case(synth.random_consolidation_general(5), MULTI),
             Case(_c4_small(1), SINGLE, shard=(1, 3))]
    st, _, _ = _run(solver, cases)
    assert st == [abi.GS_OK] * 5
    for i, c in enumerate(cases[:4]):
        want_cmds = c.solo(plain)
        plain.consolidate(c.input())  # the solo context holds this input again
        n = len(want_cmds[0])
        assert n > 0
        for sim in range(n):
            got, _ = solver.batch_consolidate_results(i, sim)  # (before any fetch of the slot on the first pass)
            want, _ = plain.consolidation_results(sim)
            assert got == want, (i, sim, got, want)
        assert _fetch(solver, i) == want_cmds, i
        with pytest.raises(lib.GpuSchedError) as e:
            solver.batch_consolidate_results(i, n)
        assert e.value.status == abi.GS_E_INVALID
    # a SKIPPED simulation
    with pytest.raises(lib.GpuSchedError) as e:
        solver.batch_consolidate_results(4, 0)
    assert e.value.status == abi.GS_E_INVALID
    assert solver.batch_consolidate_results(4, 1)[0] is not None
    solver.batch_consolidate_run()
    for i, c in enumerate(cases):
        _check_slot(solver, i, c, plain, oracle=False)


@pytest.mark.gpu
def test_overlay_epoch_wraps(plain):
    """the overlay stamp prefix has 4,095 values and every run and every
    per-slot results call draws one: past the wrap, in a run and inside a
    results call (where every group's overlay cells are cleared), each slot
    still gives its solo outcome"""
    from gpusched.lib import Solver
    cases = [Case(synth.random_consolidation_general(s), SINGLE) for s in (6, 7)]
    cases.append(Case(synth.random_consolidation_general(102, min_values=True), SINGLE))
    want = [c.solo(plain) for c in cases]
    plain.consolidate(cases[0].input())
    sims = range(len(want[0][0]))
    assert len(sims) >= 4
    res_want = [plain.consolidation_results(k)[0] for k in sims]
    s = Solver(0)
    try:
        st, _, _ = _run(s, cases)  # draw 1
        assert st == [abi.GS_OK] * 3
        draws = 1
        while draws < 4095 + 5:  # the wrap falls in a run
            s.batch_consolidate_run()
            draws += 1
        assert [_fetch(s, i) for i in range(3)] == want
        while draws % 4095 != 4093:  # two prefixes left: the wrap falls in the results calls
            s.batch_consolidate_run()
            draws += 1
        assert [s.batch_consolidate_results(0, k)[0] for k in sims] == res_want
        assert [_fetch(s, i) for i in range(3)] == want
        s.batch_consolidate_run()
        assert [_fetch(s, i) for i in range(3)] == want
    finally:
        s.close()


@pytest.mark.gpu
def test_call_level_errors(plain):
    from gpusched.lib import Solver
    one = mixed()[0].input()
    fresh = Solver(0)
    try:
        assert fresh.L.gs_batch_consolidate_run(fresh.ctx) == abi.GS_E_INVALID  # run before prepare
        with pytest.raises(lib.GpuSchedError) as e:
            fresh.batch_consolidate_prepare([one] * (abi.GS_BATCH_MAX + 1))
        assert e.value.status == abi.GS_E_CAPACITY
        assert fresh.batch_consolidate_prepare([]) == []  # n == 0 is fine
        fresh.batch_consolidate_run()
        stats = fresh.batch_consolidate_stats()
        assert stats["n_problems"] == 0 and stats["n_launches"] == 0 and stats["n_groups"] == 0
        res = abi.GsConsolidationResult()
        assert fresh.L.gs_batch_consolidate_fetch(fresh.ctx, 0, C.byref(res)) == abi.GS_E_INVALID
    finally:
        fresh.close()
    sh = Solver(0, 0, shard_devices=[0, 0])
    try:
        with pytest.raises(lib.GpuSchedError) as e:
            sh.batch_consolidate_prepare([one])
        assert e.value.status == abi.GS_E_INVALID
    finally:
        sh.close()
