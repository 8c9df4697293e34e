"""The Create re-filter against a catalog kept on the device:
gs_create_filter_prepare / _run / _set_available / _last_run.

Every GPU test compares exactly (== on the list-of-dicts form) with
pyoracle.create_filter and with gs_create_filter on the same problem.  The CPU
tests check the exports and the stats layout, and that the inputs the GPU
tests rely on really are what they claim (unknown keys and values, an
availability change that moves a selection and a capacity type).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from gpusched import abi, lib
from gpusched.problem import ProblemBuilder
from oracle import pyoracle
from test_create_filter import (CT, CT_CASES, CUSTOM, GI, GIT_CASES, ITK, ZONE, _git_problem, _kat_problem,
                                claim_queries_from_solve, random_catalog)

OP_NAMES = {v: k for k, v in abi.OPS.items()}
NEW = ("gs_create_filter_prepare", "gs_create_filter_run", "gs_create_filter_set_available",
       "gs_create_filter_last_run", "gs_create_filter_stats_size")


# ------------------------------------------------------------------------ CPU
def test_exports_and_stats_layout():
    L = lib.load()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in lib.EXPORTS
    assert L.gs_create_filter_stats_size() == C.sizeof(abi.GsCreateFilterStats)


def _req_strings(p, rng):
    """the requirement rows of range rng as (key, op name, values)"""
    out = []
    for r in p.reqs[rng[0]:rng[0] + rng[1]]:
        vb, vn = int(r["values"]["begin"]), int(r["values"]["count"])
        out.append((p.strings[r["key"]], OP_NAMES[int(r["op"])], [p.strings[i] for i in p.value_ids[vb:vb + vn]]))
    return out


def claims_of(p):
    """p's claim queries as strings: [(requirements, requests)]"""
    out = []
    for i in range(p.n_claim_queries):
        q = p.claim_queries[i]
        reqs = _req_strings(p, (q.requirements.begin, q.requirements.count))
        qty = p.quantities[q.requests.begin:q.requests.begin + q.requests.count]
        out.append((reqs, {p.strings[x["resource"]]: int(x["milli"]) for x in qty}))
    return out


def pool_of(claims):
    """a problem that holds nothing but these claims (its own string ids)"""
    b = ProblemBuilder()
    b.s("a string the catalog does not have, so that the ids shift")
    for reqs, requests in claims:
        b.add_claim_query(reqs, requests)
    return b.build()


def catalog_vocabulary(p):
    """every key and value string of the instance types' and offerings' requirements"""
    keys, vals = set(), set()
    ranges = [tuple(t["requirements"]) for t in p.instance_types] + [tuple(o["requirements"]) for o in p.offerings]
    for rng in ranges:
        for k, _op, vs in _req_strings(p, rng):
            keys.add(k)
            vals.update(vs)
    return keys, vals


@functools.lru_cache(maxsize=None)
def case(seed, n_types, n_claims):
    """(problem, oracle result), computed once and shared"""
    p = random_catalog(seed, n_types, n_claims)
    st, want = pyoracle.create_filter(p)
    assert st == abi.GS_OK
    return p, want


# run B of the call-local-id test: a key and values no catalog here has
UNSEEN_KEY, UNSEEN_VALUE = "example.org/never-listed", "value-never-listed"
B_CLAIMS = [([(UNSEEN_KEY, "In", [UNSEEN_VALUE])], {"cpu": 1000}),
            ([(UNSEEN_KEY, "NotIn", [UNSEEN_VALUE, "another-one"]), (ZONE, "In", ["us-south-2", UNSEEN_VALUE])], {}),
            ([(CUSTOM, "In", ["a", UNSEEN_VALUE])], {"unlisted.example/resource": 1}),
            ([(UNSEEN_KEY, "DoesNotExist", [])], {"cpu": 500, "unlisted.example/resource": 0})]


def test_b_claims_are_unknown_to_the_catalog():
    keys, vals = catalog_vocabulary(case(105, 300, 60)[0])
    assert UNSEEN_KEY not in keys and UNSEEN_VALUE not in vals and "another-one" not in vals
    assert ZONE in keys and "us-south-2" in vals  # ... beside ones it does know


# claims that name no instance type, on values every catalog here has
PLAIN_CLAIMS = [([(CT, "In", ["spot"])], {"cpu": 1000}),
                ([(ZONE, "In", ["us-south-1"])], {"cpu": 2000, "memory": 4 * GI * 1000}),
                ([], {}),
                ([("karpenter-ibm.sh/instance-cpu", "Gt", ["4"]), (CT, "NotIn", ["spot"])], {"cpu": 500})]


def test_plain_claims_are_known_to_both_catalogs():
    for seed, n in ((104, 65), (106, 1188)):
        keys, vals = catalog_vocabulary(case(seed, n, 30 if n == 65 else 100)[0])
        assert {CT, ZONE, "karpenter-ibm.sh/instance-cpu"} <= keys and {"spot", "us-south-1"} <= vals


def _offering_is_spot(p, o):
    return _req_strings(p, tuple(p.offerings[o]["requirements"]))[1][2] == ["spot"]


@functools.lru_cache(maxsize=None)
def flip_case():
    """A 150-type catalog and about 30 availability changes, chosen from the
    oracle's answer so that they matter: every offering of one claim's selected
    type goes, every spot offering of the types one spot claim keeps goes, a
    few unavailable offerings come back, and others flip at random up to 30
    in all.  -> (problem, oracle before,
    indices, flags, problem with the flags applied, oracle after)"""
    p, before = case(100, 150, 40)
    off = p.instance_types["offerings"]
    a = next(q for q in before if q["selected"] >= 0)
    idx = list(range(int(off[a["selected"]]["begin"]), int(off[a["selected"]]["begin"] + off[a["selected"]]["count"])))
    spot_claims = [q for q in before if q["capacity_type"] == abi.GS_CAPACITY_SPOT]
    b = min(spot_claims, key=lambda q: q["n_compatible"])
    for t in b["compatible"]:
        idx += [o for o in range(int(off[t]["begin"]), int(off[t]["begin"] + off[t]["count"]))
                if _offering_is_spot(p, o) and o not in idx]
    flags = [0] * len(idx)
    back = [o for o in range(len(p.offerings)) if not p.offerings[o]["available"] and o not in idx][:6]
    idx, flags = idx + back, flags + [1] * len(back)
    # ... and others at random, each to the opposite of what it is, up to 30 in all
    rest = [int(o) for o in np.random.default_rng(1).permutation(len(p.offerings)) if o not in idx][:30 - len(idx)]
    idx, flags = idx + rest, flags + [0 if p.offerings[o]["available"] else 1 for o in rest]
    p1 = random_catalog(100, 150, 40)
    for o, f in zip(idx, flags):
        p1.offerings["available"][o] = f
    st, after = pyoracle.create_filter(p1)
    assert st == abi.GS_OK
    return p, before, idx, flags, p1, after


def test_flip_case_moves_a_selection_and_a_capacity_type():
    _p, before, idx, flags, _p1, after = flip_case()
    assert 30 <= len(idx) <= 45 and len(set(idx)) == len(idx) and 0 in flags and 1 in flags
    assert any(x["selected"] != y["selected"] for x, y in zip(before, after))
    assert any(x["capacity_type"] != y["capacity_type"] for x, y in zip(before, after))


# ------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def solver():
    s = lib.Solver()
    yield s
    s.close()


def _three(rows):
    return [(r["n_compatible"], r["selected"], r["capacity_type"]) for r in rows]


SHAPES = [(101, 1, 5), (102, 63, 30), (103, 64, 30), (104, 65, 30), (108, 257, 40), (105, 300, 60), (112, 2000, 20)]


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n_types,n_claims", SHAPES, ids=[f"{n}x{q}" for _, n, q in SHAPES])
def test_gpu_prepared_parity(solver, seed, n_types, n_claims):
    """1 / 63 / 64 / 65 / 257 types: below a wave, a wave's edge, one past it,
    one past the 256-type chunk"""
    p, want = case(seed, n_types, n_claims)
    solver.create_filter_prepare(p)
    got = solver.create_filter_run(p)
    assert got == want
    assert got == solver.create_filter(p)
    st = solver.create_filter_last_run()
    assert st["n_queries"] == n_claims and st["n_instance_types"] == n_types and st["n_launches"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("case_", CT_CASES, ids=[c["name"] for c in CT_CASES])
def test_gpu_prepared_capacity_type_kats(solver, case_):
    p = _kat_problem(case_)
    solver.create_filter_prepare(p)
    got = solver.create_filter_run(p)
    assert got[0]["capacity_type"] == (abi.GS_CAPACITY_SPOT if case_["want"] == "spot" else abi.GS_CAPACITY_ON_DEMAND)
    assert got == pyoracle.create_filter(p)[1]


@pytest.mark.gpu
@pytest.mark.parametrize("case_", GIT_CASES, ids=[c["name"] for c in GIT_CASES])
def test_gpu_prepared_get_instance_types_kats(solver, case_):
    """includes the catalog without instance types"""
    p = _git_problem(case_)
    solver.create_filter_prepare(p)
    got = solver.create_filter_run(p)
    assert len(got[0]["requirements"]) == case_["want"]
    assert got == pyoracle.create_filter(p)[1]


@pytest.mark.gpu
def test_gpu_prepared_separate_pool(solver):
    """the claims rebuilt in a problem of their own: other string ids, same answer"""
    p, want = case(105, 300, 60)
    pool = pool_of(claims_of(p))
    assert len(pool.instance_types) == 0 and pool.strings[:40] != p.strings[:40]
    solver.create_filter_prepare(p)
    assert solver.create_filter_run(pool) == want


@pytest.mark.gpu
def test_gpu_prepared_without_bitsets(solver):
    p, want = case(105, 300, 60)
    solver.create_filter_prepare(p)
    res = solver.create_filter_run(p, bitsets=False, raw=True)
    assert not res.compatible and not res.requirements
    assert res.n_queries == 60 and res.words == 5
    got = abi.claim_filter_to_list(res, 300, bitsets=False)
    assert all(r["compatible"] is None and r["requirements"] is None for r in got)
    assert _three(got) == _three(want)
    st = solver.create_filter_last_run()
    assert st["d2h_bytes"] == 16 * 60
    solver.create_filter_run(p, bitsets=True)
    assert solver.create_filter_last_run()["d2h_bytes"] == 16 * 60 + 2 * 8 * 5 * 60


@pytest.mark.gpu
def test_gpu_prepared_run_sends_nothing_of_the_catalog(solver):
    pool = pool_of(PLAIN_CLAIMS)
    sent, prep = [], []
    for seed, n_types, n_claims in ((104, 65, 30), (106, 1188, 100)):
        p, _ = case(seed, n_types, n_claims)
        solver.create_filter_prepare(p)
        prep.append(solver.create_filter_last_run()["h2d_bytes"])
        got = solver.create_filter_run(pool)
        st = solver.create_filter_last_run()
        assert st["n_launches"] == 1 and st["n_instance_types"] == n_types
        sent.append(st["h2d_bytes"])
        # the answer is the oracle's for these claims on that catalog
        both = random_catalog(seed, n_types, 0).extended(
            lambda b: [b.add_claim_query(r, q) for r, q in PLAIN_CLAIMS])
        assert got == pyoracle.create_filter(both)[1]
    assert sent[0] == sent[1] and 0 < sent[1] < prep[1]


@pytest.mark.gpu
def test_gpu_prepared_call_local_ids_do_not_persist(solver):
    p, want = case(105, 300, 60)
    solver.create_filter_prepare(p)
    a1 = solver.create_filter_run(p)
    h1 = solver.create_filter_last_run()["h2d_bytes"]
    both = random_catalog(105, 300, 0).extended(lambda b: [b.add_claim_query(r, q) for r, q in B_CLAIMS])
    assert solver.create_filter_run(pool_of(B_CLAIMS)) == pyoracle.create_filter(both)[1]
    a2 = solver.create_filter_run(p)
    assert a1 == want and a2 == a1
    assert solver.create_filter_last_run()["h2d_bytes"] == h1
    # ... nor does anything of a larger run, whose buffers regrow, or of a re-prepare
    _check_buffers_regrow_and_shrink()


@pytest.mark.gpu
def test_gpu_prepared_long_claim(solver):
    """an instance-type In of 1,500 names is past the kernel's LDS budget of
    1,024 values per claim: that claim is read from global memory"""
    base, _ = case(112, 2000, 20)
    names = [base.strings[i] for i in base.instance_types["name"]]
    rng = np.random.default_rng(5)
    long_names = [names[i] for i in rng.choice(2000, size=1500, replace=False)]
    p = random_catalog(112, 2000, 20).extended(
        lambda b: (b.add_claim_query([(ITK, "In", long_names), (CT, "In", ["spot", "on-demand"])], {"cpu": 1000}),
                   b.add_claim_query([])))
    want = pyoracle.create_filter(p)[1]
    assert want[20]["n_compatible"] > 256  # the long claim keeps types in several chunks
    solver.create_filter_prepare(p)
    assert solver.create_filter_run(p) == want
    st = solver.create_filter_last_run()
    assert st["n_queries"] == 22 and st["n_staged_lds"] == 21


@pytest.mark.gpu
def test_gpu_prepared_availability(solver):
    p, before, idx, flags, p1, after = flip_case()
    solver.create_filter_prepare(p)
    assert solver.create_filter_run(p) == before
    solver.create_filter_set_available(idx, flags)
    got = solver.create_filter_run(p)
    assert got == after and got == solver.create_filter(p1)
    assert any(x["selected"] != y["selected"] for x, y in zip(before, got))
    assert any(x["capacity_type"] != y["capacity_type"] for x, y in zip(before, got))
    # back again
    solver.create_filter_set_available(idx, [int(p.offerings["available"][o]) for o in idx])
    assert solver.create_filter_run(p) == before
    # a repeated index takes its last value
    o = idx[0]
    solver.create_filter_set_available([o, o, o], [1, 0, 1])
    assert solver.create_filter_run(p) == before
    solver.create_filter_set_available(idx + [idx[0]], flags + [1 - flags[0]])
    solver.create_filter_set_available([idx[0]], [flags[0]])
    assert solver.create_filter_run(p) == after
    # an index out of range changes nothing
    with pytest.raises(lib.GpuSchedError) as e:
        solver.create_filter_set_available([idx[1], len(p.offerings)], [1, 1])
    assert e.value.status == abi.GS_E_INVALID
    assert solver.create_filter_run(p) == after
    solver.create_filter_set_available([], [])
    assert solver.create_filter_run(p) == after


@pytest.mark.gpu
def test_gpu_prepared_availability_overlapping_ranges(solver):
    """two instance types that share one offering both see its change"""
    b = ProblemBuilder()
    b.add_instance_type("first", [], {"cpu": 4000}, {}, [("us-south-1", "on-demand", 1.0, True)])
    b.instance_types.append((b.s("second"), b._reqs([]), b._qty({"cpu": 4000}), b._qty({}), (0, 1)))
    b.add_claim_query([], {"cpu": 1000})
    p = b.build()
    solver.create_filter_prepare(p)
    assert solver.create_filter_run(p)[0]["compatible"] == [0, 1]
    solver.create_filter_set_available([0], [0])
    assert solver.create_filter_run(p)[0]["compatible"] == []


def _run_status(s, p, nq=None, struct=None):
    res = abi.GsClaimFilterResult()
    return s.L.gs_create_filter_run(s.ctx, C.byref(struct if struct is not None else p.struct), p.claim_queries,
                                    p.n_claim_queries if nq is None else nq, abi.GS_CF_BITSETS, C.byref(res))


@pytest.mark.gpu
def test_gpu_prepared_errors():
    p, want = case(102, 63, 30)
    s = lib.Solver()
    try:
        with pytest.raises(lib.GpuSchedError) as e:
            s.create_filter_run(p)
        assert e.value.status == abi.GS_E_INVALID and "before gs_create_filter_prepare" in str(e.value)
        s.create_filter_prepare(p)
        assert s.create_filter_run(p) == want
        # too many claims
        assert _run_status(s, p, nq=70000) == abi.GS_E_INVALID
        assert s.create_filter_run(p) == want
        # a null pool array with a non-zero count
        for field in ("quantities", "reqs", "value_ids"):
            bad = abi.GsProblem()
            C.memmove(C.byref(bad), C.byref(p.struct), C.sizeof(bad))
            setattr(bad, field, None)
            assert _run_status(s, p, struct=bad) == abi.GS_E_INVALID, field
        assert s.create_filter_run(p) == want
        # a bad claim: the status gs_create_filter gives
        bad_pool = pool_of([([("karpenter-ibm.sh/instance-cpu", "Gt", ["x"])], {})])
        with pytest.raises(lib.GpuSchedError) as e:
            s.create_filter_run(bad_pool)
        assert e.value.status == abi.GS_E_INVALID and "not an integer" in str(e.value)
        assert s.create_filter_run(p) == want
        # a prepare that fails leaves the first catalog answering
        other, _ = case(103, 64, 30)
        bad = abi.GsProblem()
        C.memmove(C.byref(bad), C.byref(other.struct), C.sizeof(bad))
        bad.instance_types = None
        assert s.L.gs_create_filter_prepare(s.ctx, C.byref(bad)) == abi.GS_E_INVALID
        assert s.create_filter_run(p) == want
        # gs_create_filter on the same context neither uses nor disturbs it
        assert s.create_filter(other) == case(103, 64, 30)[1]
        assert s.create_filter_run(p) == want
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(2))
def test_gpu_prepared_after_solve(solver, seed):
    from gpusched import synth
    p = synth.random_problem(seed, n_pods=300, with_nodes=False, with_limits=False)
    res, _ = solver.solve(p)
    assert res["claims"]
    p2 = p.extended(lambda b: claim_queries_from_solve(p, res, b))
    solver.create_filter_prepare(p2)
    assert solver.create_filter_run(p2) == pyoracle.create_filter(p2)[1]


def _check_buffers_regrow_and_shrink():
    """One context: 1 claim, then 40 (the run's device buffer and both pinned
    sides regrow), then the 1 again; the same after a re-prepare, whose answers
    follow the new catalog; and gs_create_filter's own arena through the same
    sequence.  Each answer is a fresh context's for the same input."""
    cats = (case(108, 257, 40)[0], case(102, 63, 30)[0])
    claims = claims_of(cats[0])
    assert len(claims) == 40
    one = claims[2:3]  # a claim that keeps many types of either catalog
    pools = (pool_of(one), pool_of(claims))
    whole = [random_catalog(108, 257, 0).extended(lambda b, cs=cs: [b.add_claim_query(r, q) for r, q in cs])
             for cs in (one, claims)]

    def fresh(fn):
        s = lib.Solver()
        try:
            return fn(s)
        finally:
            s.close()

    def prepared_run(s, cat, pool):
        s.create_filter_prepare(cat)
        return s.create_filter_run(pool)

    want = [[fresh(lambda s, cat=cat, pool=pool: prepared_run(s, cat, pool)) for pool in pools] for cat in cats]
    assert want[0][1] == case(108, 257, 40)[1] and want[0][0] == want[0][1][2:3]  # ... which is the oracle's
    assert want[0][0][0]["n_compatible"] > want[1][0][0]["n_compatible"] > 0 and want[1][1] != want[0][1]
    want_whole = [fresh(lambda s, p=p: s.create_filter(p)) for p in whole]
    assert want_whole[1] == want[0][1]
    s = lib.Solver()
    try:
        for cat, w in zip(cats, want):
            s.create_filter_prepare(cat)
            for j in (0, 1, 0):
                assert s.create_filter_run(pools[j]) == w[j], j
        for j in (0, 1, 0):
            assert s.create_filter(whole[j]) == want_whole[j], j
    finally:
        s.close()
