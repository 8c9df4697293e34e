"""gs_batch_*: many independent Solves on one context, one workgroup each.

Every slot of a batch must equal the oracle's Solve of its problem bit for
bit (and gs_solve of the problem alone), whatever the order, the number of
slots or the mix of kernel instantiations; a refused slot must leave the
others alone; the number of kernel launches must not grow with the number of
problems.  The oracle results are computed once per problem and shared.
"""
import ctypes as C

import pytest

from gpusched import abi, lib, synth
from gpusched.problem import ProblemBuilder
from oracle import pyoracle

Z = "topology.kubernetes.io/zone"
CT = "karpenter.sh/capacity-type"


def _diff(a, b):
    if a == b:
        return None
    for k in ("errors", "nodes"):
        if a[k] != b[k]:
            return f"{k}: {a[k][:20]} vs {b[k][:20]}"
    if len(a["claims"]) != len(b["claims"]):
        n = min(len(a["claims"]), len(b["claims"]))
        for i in range(n):
            if a["claims"][i] != b["claims"][i]:
                return f"claim {i} first differs; counts {len(a['claims'])} vs {len(b['claims'])}: {a['claims'][i]} vs {b['claims'][i]}"
        return f"claim counts {len(a['claims'])} vs {len(b['claims'])}"
    for i, (x, y) in enumerate(zip(a["claims"], b["claims"])):
        if x != y:
            fields = {k: (x[k], y[k]) for k in x if x[k] != y[k]}
            return f"claim {i}: {fields}"
    return "differs"


def _empty_pods():
    b = synth.ProblemBuilder()
    synth.build_catalog(b, synth.FAKE_PROFILES, synth.FAKE_ZONES, spot=False, prices=synth.price_table(synth.FAKE_PROFILES))
    b.add_nodepool("default")
    return b.build()


def _accepted(make, first, count):
    """`count` problems make(seed), seed = first, first + 1, ..., skipping
    seeds the library or the oracle refuses -> [(problem, oracle result)]"""
    out, seed = [], first
    while len(out) < count:
        p = make(seed)
        seed += 1
        if lib.validate(p)[0] != abi.GS_OK:
            continue
        st, want, _ = pyoracle.solve(p)
        if st == abi.GS_OK:
            out.append((p, want))
    return out


_MIXED = []


def mixed():
    """the 14 problems of the mixed batch with their oracle results (built once)"""
    if not _MIXED:
        cases = _accepted(lambda s: synth.make_c1(), 0, 1)
        cases += _accepted(synth.random_problem, 0, 6)  # existing nodes, limits, free keys; 4 or 5 resources
        cases += _accepted(synth.random_topology, 0, 2)  # TOPO instantiations, lazy groups
        cases += _accepted(synth.random_relax, 0, 1)
        cases += _accepted(synth.random_min_values, 0, 1)
        cases += _accepted(lambda s: synth.make_c5(n_pods=50, n_its=300, seed=0x5EED0005 + s), 0, 1)  # W = 5 > WREG: wide rows
        cases += _accepted(lambda s: _empty_pods(), 0, 1)  # P == 0
        # enough NodeClaims for the register pdqsort and the one-rotation path
        cases += _accepted(lambda s: synth.random_problem(1000 + s, n_pods=400, with_nodes=False), 0, 1)
        assert len(cases) == 14
        _MIXED.extend(cases)
    return _MIXED


def _check_slots(s, cases, skip=()):
    for i, (_, want) in enumerate(cases):
        if i in skip:
            continue
        got, _ = s.batch_fetch(i)
        d = _diff(got, want)
        assert d is None, (i, d)


def _run_batch(s, cases):
    st = s.batch_prepare([p for p, _ in cases])
    s.batch_run()
    return st, s.batch_stats()


@pytest.fixture(scope="module")
def solver():
    from gpusched.lib import Solver
    s = Solver(0)
    yield s
    s.close()


# ------------------------------------------------------------------ CPU
def test_batch_stats_layout():
    assert lib.load().gs_batch_stats_size() == C.sizeof(abi.GsBatchStats)


def test_batch_null_context():
    """every entry point refuses a NULL context without touching a device"""
    L = lib.load()
    p = synth.make_c1(n_pods=5)
    ptrs = (C.POINTER(abi.GsProblem) * 1)(C.pointer(p.struct))
    status = (C.c_int * 1)()
    res = abi.GsResult()
    stats = abi.GsBatchStats()
    buf = C.create_string_buffer(64)
    assert L.gs_batch_prepare(None, ptrs, 1, status) == abi.GS_E_INVALID
    assert L.gs_batch_run(None) == abi.GS_E_INVALID
    assert L.gs_batch_fetch(None, 0, C.byref(res)) == abi.GS_E_INVALID
    assert L.gs_batch_error(None, 0, buf, 64) == 0
    assert L.gs_batch_last_run(None, C.byref(stats)) == abi.GS_E_INVALID


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_mixed_batch_bit_exact(solver):
    """14 problems over at least four kernel groups: every slot equals the
    oracle and gs_solve of the problem alone on a second, plain context"""
    from gpusched.lib import Solver
    cases = mixed()
    st, stats = _run_batch(solver, cases)
    assert st == [abi.GS_OK] * 14
    assert stats["n_problems"] == 14 and stats["n_accepted"] == 14
    assert stats["n_groups"] >= 4, stats
    assert stats["n_fallback"] == 0 and stats["n_batched"] == 14, stats
    _check_slots(solver, cases)
    plain = Solver(0)
    try:
        for i, (p, _) in enumerate(cases):
            alone, _ = plain.solve(p)
            got, _ = solver.batch_fetch(i)
            d = _diff(got, alone)
            assert d is None, (i, d)
    finally:
        plain.close()


@pytest.mark.gpu
def test_order_and_repetition(solver):
    """reversed order, then every pointer three times: the same groups and the
    same number of launches for 14 and for 42 slots"""
    cases = list(reversed(mixed()))
    st, s14 = _run_batch(solver, cases)
    assert st == [abi.GS_OK] * 14
    _check_slots(solver, cases)
    tripled = [c for c in cases for _ in range(3)]
    st, s42 = _run_batch(solver, tripled)
    assert st == [abi.GS_OK] * 42
    _check_slots(solver, tripled)
    assert s42["n_batched"] == 42 and s42["n_fallback"] == 0
    assert s42["n_groups"] == s14["n_groups"]
    assert s42["n_launches"] == s14["n_launches"] and s14["n_launches"] > 0


@pytest.mark.gpu
def test_more_workgroups_than_cus(solver):
    """600 slots over ten small problems with existing nodes: more workgroups
    than the device has CUs, each slot still its own problem's result"""
    ten = _accepted(lambda s: synth.random_problem(5000 + s, n_pods=60), 0, 10)
    cases = [ten[i % 10] for i in range(600)]
    st, stats = _run_batch(solver, cases)
    assert st == [abi.GS_OK] * 600
    assert stats["n_batched"] == 600 and stats["n_fallback"] == 0, stats
    _check_slots(solver, cases)


def _two_domain_keys():
    """zone and capacity-type spreads in one problem (tests/test_topology.py
    test_refusals): the oracle solves it, the library refuses it"""
    b = ProblemBuilder()
    synth.build_catalog(b, synth.FAKE_PROFILES, synth.FAKE_ZONES, spot=False,
                        prices=synth.price_table(synth.FAKE_PROFILES))
    b.add_nodepool("default", requirements=[(Z, "In", synth.FAKE_ZONES)])
    b.add_pod("p0", 0, {"cpu": 1500, "memory": 1 << 30, "pods": 1000}, labels={"app": "web"},
              spreads=[{"key": Z, "max_skew": 1, "selector": {"labels": {"app": "web"}}},
                       {"key": CT, "max_skew": 1, "selector": {"labels": {"app": "web"}}}])
    return b.build()


def _duplicate_uid():
    b = synth.ProblemBuilder()
    synth.build_catalog(b, synth.FAKE_PROFILES, synth.FAKE_ZONES, spot=False, prices={})
    b.add_nodepool("default")
    b.add_pod("u1", 0, {"cpu": 100, "pods": 1000})
    b.add_pod("u1", 0, {"cpu": 100})
    return b.build()


@pytest.mark.gpu
def test_refused_slot_does_not_poison_the_batch(solver):
    cases = list(mixed()[:6])
    cases.insert(2, (_two_domain_keys(), None))
    cases.insert(5, (_duplicate_uid(), None))
    assert lib.validate(cases[2][0])[0] == abi.GS_E_UNSUPPORTED
    assert lib.validate(cases[5][0])[0] == abi.GS_E_INVALID
    st, stats = _run_batch(solver, cases)
    want = [abi.GS_OK] * 8
    want[2], want[5] = abi.GS_E_UNSUPPORTED, abi.GS_E_INVALID
    assert st == want
    assert stats["n_problems"] == 8 and stats["n_accepted"] == 6
    for i in (2, 5):
        assert solver.batch_error(i) == lib.validate(cases[i][0])[1] != ""
        with pytest.raises(lib.GpuSchedError) as e:
            solver.batch_fetch(i)
        assert e.value.status == want[i]
    _check_slots(solver, cases, skip=(2, 5))


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [abi.GS_CFG_BLOCK_SOLVE, abi.GS_CFG_CLAIMS_HBM])
def test_fallback_contexts(flags):
    """a context that asks for the block kernel or the HBM claim mode solves
    every slot through the single-problem path"""
    from gpusched.lib import Solver
    cases = mixed()[:6]
    s = Solver(0, flags)
    try:
        st, stats = _run_batch(s, cases)
        assert st == [abi.GS_OK] * 6
        assert stats["n_fallback"] == 6 and stats["n_batched"] == 0, stats
        assert stats["n_groups"] == 0 and stats["n_launches"] == 0
        _check_slots(s, cases)
    finally:
        s.close()


def _claim_overflow():
    """6,000 state nodes and one NodeClaim per pod (the problem of
    test_gpu_wave_claim_overflow_reruns_in_hbm_mode, with fewer pods).  The
    nodes' slack codes take 8 + 17 x 6,000 = 102,008 B of the workgroup's
    160 KiB of LDS and a NodeClaim takes 23 B, so whatever else the kernel
    keeps there the slot's max_claims_wave is at most
    (163,840 - 102,008) / 23 = 2,688: 2,700 pods exceed it."""
    b = ProblemBuilder()
    synth.build_catalog(b, synth.FAKE_PROFILES, synth.FAKE_ZONES, spot=False,
                        prices=synth.price_table(synth.FAKE_PROFILES))
    b.add_nodepool("default")
    for k in range(6000):
        b.add_node(f"n{k:05d}", {"topology.kubernetes.io/zone": synth.FAKE_ZONES[k % 3]},
                   {"cpu": 100, "memory": 1 << 30, "pods": 110_000})
    for i in range(2700):
        b.add_pod(f"p{i:05d}", 0, {"cpu": 1000, "memory": 1 << 30, "pods": 1000}, labels={"app": "one-per-node"},
                  anti_affinity=[{"required": True, "selector": {"labels": {"app": "one-per-node"}}}])
    return b.build()


@pytest.mark.gpu
def test_claim_overflow_slot_falls_back(solver):
    """a batched slot that opens more NodeClaims than its LDS holds reruns
    alone with its claim state in HBM and stays a fallback slot"""
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
    for run in range(2):
        if run == 0:
            st, stats = _run_batch(solver, cases)
            assert st == [abi.GS_OK] * 3
        else:
            solver.batch_run()
            stats = solver.batch_stats()
        assert stats["n_fallback"] == 1 and stats["n_batched"] == 2, (run, stats)
        _check_slots(solver, cases)


@pytest.mark.gpu
def test_reuse_and_independence(solver):
    from gpusched.lib import Solver
    cases = mixed()
    # the context's own prepared problem survives a batch
    own_p, own_want = cases[3]
    solver.prepare(own_p)
    solver.run()
    st, _ = _run_batch(solver, cases)
    assert st == [abi.GS_OK] * 14
    first = [solver.batch_fetch(i)[0] for i in range(14)]
    solver.batch_run()
    assert [solver.batch_fetch(i)[0] for i in range(14)] == first
    got, _ = solver.fetch()
    assert _diff(got, own_want) is None
    # a smaller batch replaces the larger one
    three = cases[7:10]
    st, stats = _run_batch(solver, three)
    assert st == [abi.GS_OK] * 3 and stats["n_problems"] == 3
    _check_slots(solver, three)
    res = abi.GsResult()
    assert solver.L.gs_batch_fetch(solver.ctx, 5, C.byref(res)) == abi.GS_E_INVALID
    # n == 0 and n == 1
    st, stats = _run_batch(solver, [])
    assert st == [] and stats["n_problems"] == 0 and stats["n_launches"] == 0
    st, stats = _run_batch(solver, cases[:1])
    assert st == [abi.GS_OK] and stats["n_batched"] == 1
    _check_slots(solver, cases[:1])
    # more than GS_BATCH_MAX problems: the call is refused before any work
    with pytest.raises(lib.GpuSchedError) as e:
        solver.batch_prepare([cases[0][0]] * (abi.GS_BATCH_MAX + 1))
    assert e.value.status == abi.GS_E_CAPACITY
    # a sharded context runs no batch
    sh = Solver(0, 0, shard_devices=[0, 0])
    try:
        with pytest.raises(lib.GpuSchedError) as e:
            sh.batch_prepare([cases[0][0]])
        assert e.value.status == abi.GS_E_INVALID
    finally:
        sh.close()
