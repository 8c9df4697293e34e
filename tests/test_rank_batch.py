"""Autoplacement ranking against a catalog kept on the device:
gs_rank_prepare / gs_rank_run / gs_rank_last_run.

The scores and a catalog-wide order key per type are computed once per
catalog; a run filters, compacts, sorts and gathers for many queries in one
launch.  Every GPU test compares bit for bit (List indices, and float64 score
patterns under GS_RANK_SCORES) with pyoracle.rank_instance_types of each query
alone and with gs_rank_instance_types.  The CPU tests check the exports and
layouts, the shared rules (csrc/rank_rules.hpp) on the host under sanitizers,
and the premise of the design: sorting a kept subset by its CATALOG-wide dense
ranks gives the oracle's permutation.
"""
import ctypes as C
import functools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from gpusched import abi, lib
from oracle import pyoracle
from test_rank import GI, RANK_ORDER_CASES, _check_rank_order, _kats, _rank_cols, catalog

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_rank_prepare", "gs_rank_run", "gs_rank_last_run", "gs_rank_query_size", "gs_rank_result_size",
       "gs_rank_stats_size")
ANY = abi.GS_ARCH_ANY
NAN = float("nan")
# kept counts around pdqsort's insertion-sort (12) and ninther (50) thresholds
KEPT_COUNTS = (0, 1, 12, 13, 49, 50, 51)


# ------------------------------------------------------------------------ CPU
def test_exports_and_layouts():
    L = lib.load()
    header = open(os.path.join(ROOT, "include", "gpusched.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert name in lib.EXPORTS
        assert hasattr(L, name), name
    assert L.gs_rank_query_size() == C.sizeof(abi.GsRankQuery) == 32
    assert L.gs_rank_result_size() == C.sizeof(abi.GsRankResult)
    assert L.gs_rank_stats_size() == C.sizeof(abi.GsRankStats)
    # no padding: the fields' sizes add up to the struct's
    assert sum(C.sizeof(t) for _, t in abi.GsRankQuery._fields_) == C.sizeof(abi.GsRankQuery)
    assert abi.GS_RANK_BATCH_MAX == 4096 and abi.GS_RANK_SCORES == 1


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# (cpu_milli, memory_bytes, price, arch): the corners of the two rules
RULE_ROWS = [
    (4000, 16 * GI, 0.5, 0), (2000, 8 * GI, 0.0, 0), (16000, 64 * GI, 2.0, 0),  # the score KATs of test_rank.py
    (0, 16 * GI, 0.0, 1),            # cpu 0
    (4000, 0, 0.0, 0),               # mem 0
    (0, 0, 0.0, 0),                  # both, price 0: score 0
    (0, 8 * GI, 0.25, 1),            # price > 0 with cpu 0: price / 0 = +inf
    (2000, 0, 0.25, 0),              # ... with mem 0
    (0, 0, 0.25, 0),
    (4000, 16 * GI - 1, 0.2, 0),     # 16 GiB - 1 against min_memory_gb = 16
    (4000, 16 * GI, 0.2, 1),
    (3999, 16 * 10**9, 0.4, 1),      # Value() and ScaledValue(Giga) round up
    (4001, 16 * 10**9 + 1, 0.4, 0),
    (8000, 32 * GI, 0.4, 1), (1000, 1, 1e-300, 0), (64000, 512 * GI, 1e300, 1),
]
# (want_arch, min_cpu, min_memory_gb, max_price)
RULE_QUERIES = [
    (ANY, 0, 0, 0.0), (0, 0, 0, 0.0), (1, 0, 0, 0.0), (7, 0, 0, 0.0),
    (ANY, 4, 0, 0.0), (ANY, 5, 0, 0.0), (ANY, 1, 0, 0.0), (ANY, -3, 0, 0.0),
    (ANY, 0, 16, 0.0), (ANY, 0, 17, 0.0), (ANY, 0, 1, 0.0), (ANY, 0, -1, 0.0),
    (ANY, 0, 0, 0.4), (ANY, 0, 0, 0.2), (ANY, 0, 0, -1.0), (ANY, 0, 0, NAN), (ANY, 0, 0, float("inf")),
    (ANY, 0, 0, 1e-300), (1, 4, 16, 0.4), (0, 1, 1, 2.0),
]


@pytest.fixture(scope="module")
def rules_host(tmp_path_factory):
    """tools/rank_rules_host.cpp: rank_rules.hpp on the host, under ASan + UBSan"""
    if shutil.which("g++") is None:
        pytest.skip("g++ absent")
    out = str(tmp_path_factory.mktemp("rank_rules") / "rank_rules_host")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-o", out, os.path.join(ROOT, "tools", "rank_rules_host.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_rules_on_the_host_match_the_oracle(rules_host):
    text = [f"{len(RULE_ROWS)} {len(RULE_QUERIES)}"]
    text += [f"{c} {m} {_bits(p):x} {a}" for c, m, p, a in RULE_ROWS]
    text += [f"{a} {c} {m} {_bits(p):x}" for a, c, m, p in RULE_QUERIES]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([rules_host], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = [ln.split() for ln in r.stdout.strip().split("\n")]
    assert len(lines) == len(RULE_ROWS) and all(len(ln) == 1 + len(RULE_QUERIES) for ln in lines)
    score = pyoracle.lib().oracle_instance_score
    for (c, m, p, _a), ln in zip(RULE_ROWS, lines):
        assert int(ln[0], 16) == _bits(score(c, m, p)), (c, m, p)
    assert [int(ln[0], 16) for ln in lines[:3]] == [_bits(x) for x in (0.0763888888888889, 11.0, 0.0769927536231884)]
    assert int(lines[6][0], 16) == _bits(float("inf"))
    cols = [[r_[k] for r_ in RULE_ROWS] for k in range(4)]
    seen = set()
    for j, (a, c, m, p) in enumerate(RULE_QUERIES):
        st, order, _ = pyoracle.rank_instance_types(*cols, want_arch=a, min_cpu=c, min_memory_gb=m, max_price=p)
        assert st == abi.GS_OK
        got = [i for i, ln in enumerate(lines) if ln[1 + j] == "1"]
        assert got == sorted(order), RULE_QUERIES[j]
        seen.add(len(got))
    assert 0 in seen and len(RULE_ROWS) in seen and len(seen) > 4  # the filters do bite, and differently


def _dense_ranks(cpu, mem, price):
    """per type: how many DISTINCT catalog scores lie below its own (order-isomorphic to the device key)"""
    score = pyoracle.lib().oracle_instance_score
    scores = [score(int(c), int(m), float(p)) for c, m, p in zip(cpu, mem, price)]
    dense = {s: i for i, s in enumerate(sorted(set(scores)))}
    return [dense[s] for s in scores], scores


def _filters(seed, price):
    """the six filter forms of test_rank.py's test_gpu_rank_parity"""
    rng = np.random.default_rng(1000 + seed)
    return [dict(), dict(want_arch=int(rng.integers(0, 2))), dict(min_cpu=8), dict(min_memory_gb=64),
            dict(max_price=float(np.median(price)) if len(price) else 1.0),
            dict(want_arch=0, min_cpu=4, min_memory_gb=16, max_price=2.0)]


@pytest.mark.parametrize("seed", range(12))
def test_catalog_wide_keys_sort_every_kept_subset_as_the_oracle(seed):
    """the design's premise, without the kernel: the kept subset, in List
    order, keyed by its catalog-wide dense ranks and sorted by Go's sort.Slice
    is the permutation the oracle returns for that filter"""
    n = [0, 1, 12, 13, 49, 50, 51, 200, 1188, 2000, 4096, 777][seed]
    cpu, mem, price, arch = catalog(seed, n)
    ranks, _ = _dense_ranks(cpu, mem, price)
    for kw in _filters(seed, price):
        st, want, _ = pyoracle.rank_instance_types(cpu, mem, price, arch, **kw)
        assert st == abi.GS_OK
        kept = sorted(want)  # List order
        k = len(kept)
        keys = (C.c_int64 * max(1, k))(*[ranks[i] for i in kept])
        perm = (C.c_uint32 * max(1, k))()
        pyoracle.lib().oracle_go_sort_ints(keys, perm, k)
        assert [kept[p] for p in list(perm)[:k]] == want, kw
    if n >= 200:  # the subset's own dense ranks differ from the catalog's somewhere: the premise is not vacuous
        st, want, _ = pyoracle.rank_instance_types(cpu, mem, price, arch, min_cpu=8)
        sub = sorted(want)
        own, _ = _dense_ranks(cpu[sub], mem[sub], price[sub])
        assert own != [ranks[i] for i in sub]


# ------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def solver():
    s = lib.Solver()
    yield s
    s.close()


def _u64(xs):
    return np.array(xs, dtype=np.float64).view(np.uint64).tolist()


@functools.lru_cache(maxsize=None)
def _cat(seed, n):
    return catalog(seed, n)


def _want(cols, kw):
    st, order, score = pyoracle.rank_instance_types(*cols, **kw)
    assert st == abi.GS_OK
    return order, _u64(score)


def _check_runs(solver, cols, distinct, nqs=(1, 2, 65)):
    """prepare cols; for each nq a run over `distinct` cycled (from another
    start each time), with and without scores, against the oracle and
    gs_rank_instance_types of each query alone"""
    n = len(cols[0])
    want = [_want(cols, kw) for kw in distinct]
    for kw, (order, score) in zip(distinct, want):
        got_order, got_score = lib.rank_instance_types(*cols, **kw)
        assert got_order == order and _u64(got_score) == score, kw
    solver.rank_prepare(*cols)
    assert solver.rank_last_run()["n_instance_types"] == n
    for nq in nqs:
        pick = [(j + nq) % len(distinct) for j in range(nq)]
        qs = [distinct[p] for p in pick]
        orders, scores, kept = solver.rank_run(qs, scores=True)
        assert len(orders) == len(scores) == len(kept) == nq
        for j, p in enumerate(pick):
            assert orders[j] == want[p][0], (n, nq, j, distinct[p])
            assert _u64(scores[j]) == want[p][1], (n, nq, j, distinct[p])
            assert kept[j] == len(want[p][0])
        orders2, none, kept2 = solver.rank_run(qs)
        assert none is None and orders2 == orders and kept2 == kept
    return want


PARITY_N = (0, 1, 63, 64, 65, 257, 1188, 4096)


@pytest.mark.gpu
@pytest.mark.parametrize("n", PARITY_N)
def test_gpu_rank_batch_parity(solver, n):
    """below a wave, a wave's edge, one past it, one past rank_kernel's
    256-type chunk, CM-scale, and GS_RANK_MAX; the six filter forms, then
    catalogs whose arch column keeps exactly k types"""
    seed = PARITY_N.index(n)
    cols = _cat(seed, n)
    _check_runs(solver, cols, _filters(seed, cols[2]))
    rng = np.random.default_rng(2000 + seed)
    for k in sorted({k for k in KEPT_COUNTS if k <= n} | {n}):
        arch = np.zeros(n, dtype=np.uint32)
        arch[rng.permutation(n)[:k]] = 1
        kcols = (cols[0], cols[1], cols[2], arch)
        want = _check_runs(solver, kcols, [dict(want_arch=1), dict(), dict(want_arch=1, max_price=-1.0)])
        assert len(want[0][0]) == k and len(want[1][0]) == n


@pytest.mark.gpu
def test_gpu_rank_batch_all_scores_equal(solver):
    """one key for the whole catalog: every Less is false, the order is what
    pdqsort's moves alone leave (the oracle's, whatever that is)"""
    n = 777
    rng = np.random.default_rng(7)
    cols = (np.full(n, 4000, np.int64), np.full(n, 16 * GI, np.int64), np.full(n, 0.2),
            rng.integers(0, 2, size=n).astype(np.uint32))
    want = _check_runs(solver, cols, [dict(), dict(want_arch=1), dict(want_arch=0, min_cpu=4), dict(min_cpu=5)])
    assert len(set(want[0][1])) == 1 and len(want[0][0]) == n and 0 < len(want[1][0]) < n and want[3][0] == []


@pytest.mark.gpu
def test_gpu_rank_batch_kats(solver):
    """the reference_kats.json rank-order cases and the zero-resources score, through prepare / run"""
    for case in RANK_ORDER_CASES:
        cols = _rank_cols(case)
        solver.rank_prepare(*cols)
        orders, scores, kept = solver.rank_run([{}], scores=True)
        _check_rank_order(case, orders[0])
        want = _want(cols, {})
        assert orders[0] == want[0] and _u64(scores[0]) == want[1] and kept == [len(cols[0])]
    solver.rank_prepare([4000, 2000, 16000], [16 * GI, 8 * GI, 64 * GI], [0.5, 0.0, 2.0], [0] * 3)
    orders, scores, _ = solver.rank_run([{}], scores=True)
    assert orders == [[0, 2, 1]] and scores == [[0.0763888888888889, 0.0769927536231884, 11.0]]
    k = _kats()["score_zero_resources"]
    solver.rank_prepare([k["cpu_milli"]], [k["memory_bytes"]], [k["price"]], [0])
    assert solver.rank_run([{}], scores=True)[1] == [[k["want"]]]


@pytest.mark.gpu
def test_gpu_rank_batch_max_out(solver):
    n = 300
    cols = _cat(21, n)
    qs = [dict(), dict(min_cpu=8), dict(want_arch=1, min_memory_gb=128)]
    want = [_want(cols, kw) for kw in qs]
    assert len(want[0][0]) == n and 60 < len(want[1][0]) < n and 1 < len(want[2][0]) < 60
    solver.rank_prepare(*cols)
    for max_out in (1, 60, n, n + 5):
        res = solver.rank_run(qs, max_out=max_out, raw=True)
        stride = min(max_out, n)
        assert res.stride == stride and res.n_queries == 3 and not res.score
        orders, scores, kept = solver.rank_run(qs, max_out=max_out, scores=True)
        assert kept == [len(w[0]) for w in want]
        for j, w in enumerate(want):
            assert orders[j] == w[0][:stride] and _u64(scores[j]) == w[1][:stride], (max_out, j)
        assert solver.rank_last_run()["d2h_bytes"] == 3 * (4 + 12 * stride)
    assert solver.rank_run(qs, raw=True).stride == n  # max_out = 0: every kept type


@pytest.mark.gpu
def test_gpu_rank_batch_run_before_prepare():
    s = lib.Solver()
    try:
        with pytest.raises(lib.GpuSchedError) as e:
            s.rank_run([{}])
        assert e.value.status == abi.GS_E_INVALID
        assert s.rank_last_run()["n_launches"] == 0
    finally:
        s.close()


@pytest.mark.gpu
def test_gpu_rank_batch_refused_prepare_keeps_the_catalog(solver):
    cols = _cat(22, 200)
    qs = [dict(), dict(min_cpu=8), dict(want_arch=0, max_price=1.0)]
    want = [_want(cols, kw) for kw in qs]
    solver.rank_prepare(*cols)
    before = solver.rank_run(qs, scores=True)
    assert [(o, _u64(s)) for o, s in zip(before[0], before[1])] == want
    big = abi.GS_RANK_MAX + 1
    for bad, status in ((([-1], [GI], [0.1], [0]), abi.GS_E_INVALID), (([1000], [-GI], [0.1], [0]), abi.GS_E_INVALID),
                        (([1000], [GI], [NAN], [0]), abi.GS_E_INVALID),
                        (([1000] * big, [GI] * big, [0.1] * big, [0] * big), abi.GS_E_CAPACITY)):
        with pytest.raises(lib.GpuSchedError) as e:
            solver.rank_prepare(*bad)
        assert e.value.status == status
        assert solver.rank_run(qs, scores=True) == before
    # a second prepare replaces the first: other prices, the oracle's answer for them
    price2 = np.round(cols[2][::-1] * 1.5 + 0.01, 4)
    cols2 = (cols[0], cols[1], price2, cols[3])
    want2 = [_want(cols2, kw) for kw in qs]
    assert want2 != want
    solver.rank_prepare(*cols2)
    after = solver.rank_run(qs, scores=True)
    assert [(o, _u64(s)) for o, s in zip(after[0], after[1])] == want2
    # ... also between runs whose buffers regrow and are reused
    _check_buffers_regrow_and_shrink()


@pytest.mark.gpu
def test_gpu_rank_batch_too_many_queries(solver):
    solver.rank_prepare([4000], [16 * GI], [0.5], [0])
    nq = abi.GS_RANK_BATCH_MAX + 1
    arr = (abi.GsRankQuery * nq)()
    for x in arr:
        x.want_arch = ANY
    with pytest.raises(lib.GpuSchedError) as e:
        solver.rank_run((arr, nq))
    assert e.value.status == abi.GS_E_CAPACITY
    orders, _, kept = solver.rank_run((arr, abi.GS_RANK_BATCH_MAX))  # the context stays usable, at the bound too
    assert orders == [[0]] * abi.GS_RANK_BATCH_MAX and kept == [1] * abi.GS_RANK_BATCH_MAX
    assert solver.rank_run([]) == ([], None, [])  # nq = 0
    assert solver.rank_last_run()["n_launches"] == 0


@pytest.mark.gpu
def test_gpu_rank_batch_shares_the_context(solver):
    """a gs_solve and a gs_create_filter_run on the same context between two runs disturb nothing"""
    from gpusched import synth
    from test_create_filter import random_catalog
    cols = _cat(23, 257)
    qs = _filters(23, cols[2])
    want = [_want(cols, kw) for kw in qs]
    solver.rank_prepare(*cols)
    first = solver.rank_run(qs, scores=True)
    assert [(o, _u64(s)) for o, s in zip(first[0], first[1])] == want
    problem = synth.make_c1(n_pods=200)
    got, _ = solver.solve(problem)
    assert got == pyoracle.solve(problem)[1]
    p = random_catalog(102, 63, 30)
    solver.create_filter_prepare(p)
    assert solver.create_filter_run(p) == pyoracle.create_filter(p)[1]
    assert solver.rank_run(qs, scores=True) == first
    assert solver.create_filter_run(p) == pyoracle.create_filter(p)[1]  # ... nor the other way round


@pytest.mark.gpu
def test_gpu_rank_batch_shape_of_a_run(solver):
    """one launch whatever nq is, and nothing of the catalog crosses the bus"""
    n = 1188
    cols = _cat(24, n)
    solver.rank_prepare(*cols)
    st = solver.rank_last_run()
    assert st["h2d_bytes"] == 28 * n and st["n_launches"] == 1 and st["n_instance_types"] == n
    for nq in (1, 65):
        qs = [dict(min_cpu=(j % 3) * 4) for j in range(nq)]
        for scores, per in ((False, 4), (True, 12)):
            for max_out, stride in ((0, n), (60, 60)):
                solver.rank_run(qs, max_out=max_out, scores=scores)
                st = solver.rank_last_run()
                assert st["n_launches"] == 1
                assert st["h2d_bytes"] == nq * C.sizeof(abi.GsRankQuery)
                assert st["d2h_bytes"] == nq * (4 + per * stride)
                assert st["n_queries"] == nq and st["n_instance_types"] == n


def _check_buffers_regrow_and_shrink():
    """One context, a 70-type catalog (one past a wave): 1 query, then 40 (the
    run's device buffer and both pinned sides regrow), then the 1 again; the
    same after a re-prepare, whose answers follow the new catalog.  Each answer
    is a fresh context's for the same input."""
    cats = (_cat(25, 70), _cat(26, 70))
    calls = ([dict(min_cpu=4)], [dict(min_cpu=(j % 5) * 2, want_arch=j % 2) for j in range(40)])

    def fresh(cols, qs):
        s = lib.Solver()
        try:
            s.rank_prepare(*cols)
            return s.rank_run(qs, scores=True)
        finally:
            s.close()

    want = [[fresh(cols, qs) for qs in calls] for cols in cats]
    for w, cols in zip(want, cats):  # ... which is the oracle's
        assert w[0][0] == [_want(cols, calls[0][0])[0]] and [len(o) for o in w[1][0]] == w[1][2]
    assert want[0][0] != want[1][0] and want[0][1] != want[1][1]
    s = lib.Solver()
    try:
        for cols, w in zip(cats, want):
            s.rank_prepare(*cols)
            for j in (0, 1, 0):
                assert s.rank_run(calls[j], scores=True) == w[j], j
    finally:
        s.close()
