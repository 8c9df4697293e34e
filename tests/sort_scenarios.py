"""Solve problems whose order of adds is scripted so that the per-pod
`sort.Slice(newNodeClaims, len(Pods) asc)` sees the hard arrays by
construction: a raised key on one of choosePivot's sampled triples, long runs
of equal keys, appended NodeClaims out of order, at more than 64 NodeClaims
(the wave path), at 13-49 (the whole pdqsort in registers) and around the
64 | 65 boundary.

Every pod asks for the same resources and carries an increasing creation
timestamp, so the queue order is the construction order.  A *class* is one
(instance-family, instance-size, zone) triple selected by node selector: a pod
pinned to a class can only join that class's NodeClaim.  Phase A opens K
NodeClaims with K pinned pods.  In phase B a pod is either *steered* -- pinned
to the NodeClaim that sits at one of the six pivot-adjacent positions of Go's
order right now -- or scoped at random (pinned, zone only, family only, free);
a scoped pod lands on the first compatible NodeClaim in sorted order, which is
what makes the tie order visible in the result.

The builder keeps a model of Go's order (the claims re-permuted before each
pod with the oracle's Go sort on the counts) only to steer.  Whether a
scenario reaches a sort path is decided by the oracle's histogram
(pyoracle.last_sort_paths), and the model itself is checked against the
oracle's result (tests/test_sort_paths.py).
"""
import ctypes as C

import numpy as np

from gpusched import catalog as cat
from gpusched import synth
from gpusched.problem import ProblemBuilder
from oracle import pyoracle

FAMILY_KEY = "karpenter-ibm.sh/instance-family"
SIZE_KEY = "karpenter-ibm.sh/instance-size"
ZONE_KEY = "topology.kubernetes.io/zone"
REQUESTS = {"cpu": 50, "memory": 64 * synth.MI * 1000, "pods": 1000}
TS0 = 1_700_000_000_000_000_000


def go_order(counts):
    """Go's sort.Slice permutation of `counts` (indices into it)"""
    n = len(counts)
    k = (C.c_int64 * max(1, n))(*counts)
    p = (C.c_uint32 * max(1, n))()
    pyoracle.lib().oracle_go_sort_ints(k, p, n)
    return list(p)[:n]


class Scenario:
    def __init__(self, name, problem, model_counts, n_claims, appends_out_of_order=0):
        self.appends_out_of_order = appends_out_of_order  # late NodeClaims opened below every other count
        self.name = name
        self.problem = problem
        self.model_counts = model_counts  # pods per NodeClaim in creation order, by the model
        self.n_claims = n_claims

    def __repr__(self):
        return self.name


def build(k, n, seed, topo=False, late=0, late_at=None, steer=0.6, positions=(0, 1, 2, 3, 4, 5), name=None,
          pods_milli=1000, candidates=0):
    """k: phase A NodeClaims; n: phase B pods; topo: the first pod owns a zone
    spread that selects only itself (the TOPO kernel instantiations, same
    script); late: NodeClaims opened in phase B once every existing count is
    >= 2 (MOD_APPEND inversions); late_at: phase B indices at which a
    NodeClaim opens whatever the counts (the 64 -> 65 step); positions: which
    of x = q-1, q, 2q-1, 2q, 3q-1, 3q steering may raise; pods_milli: each
    pod's `pods` request (more than 1000 tightens the room until NodeClaims
    fill up: the model then only steers and its counts go stale);
    candidates: instead of pending pods, a cluster of that many full
    consolidation candidates holding the script's pods as bound pods, plus
    two full nodes that stay (one simulation over all candidates replays the
    script onto new NodeClaims)"""
    rng = np.random.default_rng(seed)
    b = ProblemBuilder()
    profs = synth.c2_profiles(60)
    its = synth.build_catalog(b, profs, synth.FAKE_ZONES, spot=False, prices=synth.price_table(profs))
    # the zone requirement gives a zone spread its domains (the twin's first pod)
    b.add_nodepool("default", requirements=[(ZONE_KEY, "In", synth.FAKE_ZONES)])
    requests = dict(REQUESTS, pods=pods_milli)
    for j in range(candidates + 2 if candidates else 0):
        it = its[j % len(its)]
        labels = {r[0]: r[2][0] for r in it.requirements}
        labels.update({ZONE_KEY: synth.FAKE_ZONES[j % 3], "karpenter.sh/capacity-type": "on-demand",
                       "karpenter.sh/nodepool": "default", "kubernetes.io/hostname": f"node-{j:03d}"})
        b.add_node(f"node-{j:03d}", labels, {"cpu": 0, "memory": 0, "pods": 0})
    classes = [(cat.instance_family(p[0]), cat.instance_size(p[0]), z) for p in profs for z in synth.FAKE_ZONES]
    classes = [classes[i] for i in rng.permutation(len(classes))]
    late_at = set(late_at or ())
    assert k + late + len(late_at) <= len(classes)
    n_pods = [0]

    def pod(sel, **kw):
        i = n_pods[0]
        n_pods[0] += 1
        if candidates:
            b.add_bound_pod(i % candidates, f"sp-{i:05d}", TS0 + i, requests, node_selector=sel, **kw)
        else:
            b.add_pod(f"sp-{i:05d}", TS0 + i, requests, node_selector=sel, **kw)

    def pin(c):
        return {FAMILY_KEY: c[0], SIZE_KEY: c[1], ZONE_KEY: c[2]}

    order = []   # claim ids in Go's order after the last sort
    count = []   # pods per claim id (creation order)
    for c in range(k):
        if c == 0 and topo:
            pod(pin(classes[c]), labels={"sort-paths": "twin"},
                spreads=[{"key": ZONE_KEY, "max_skew": 1,
                         "selector": {"labels": {"sort-paths": "twin"}}}])
        else:
            pod(pin(classes[c]))
        order = [order[i] for i in go_order([count[x] for x in order])]
        order.append(c)
        count.append(1)
    turn = 0
    out_of_order = 0
    for i in range(n):
        order = [order[j] for j in go_order([count[x] for x in order])]
        m = len(order)
        keys = [count[x] for x in order]
        if i in late_at or (late and min(keys) >= 2 and rng.random() < 0.25):
            if i not in late_at:
                late -= 1
            c = len(count)
            out_of_order += min(keys) >= 2
            pod(pin(classes[c]))
            order.append(c)
            count.append(1)
            continue
        fill = late and min(keys) < 2 and i > n // 4
        if not fill and rng.random() < steer:
            q = m // 4
            xs = [(1 + p // 2) * q - 1 + p % 2 for p in positions]
            # prefer a position whose right neighbour holds the same count:
            # raising it is an inversion on a sampled triple
            hot = [x for x in xs if x + 1 < m and keys[x + 1] == keys[x]]
            pick = hot or xs
            x = pick[turn % len(pick)]
            turn += 1
            target = order[x]
            pod(pin(classes[target]))
        else:
            kind = 3 if fill else int(rng.integers(0, 4))
            ref = classes[order[int(rng.integers(0, m))]]
            if kind == 0:
                sel, ok = pin(ref), (lambda c: c == ref)
            elif kind == 1:
                sel, ok = {ZONE_KEY: ref[2]}, (lambda c: c[2] == ref[2])
            elif kind == 2:
                sel, ok = {FAMILY_KEY: ref[0]}, (lambda c: c[0] == ref[0])
            else:
                sel, ok = {}, (lambda c: True)
            target = next(x for x in order if ok(classes[x]))
            pod(sel)
        count[target] += 1
    name = name or f"k{k}-n{n}-s{seed}" + ("-topo" if topo else "") + ("-late" if late_at or len(count) > k else "")
    return Scenario(name, b.build(), count, len(count), out_of_order)


def _variants():
    out = []
    for seed in range(3):
        for topo in (False, True):
            # the wave path (more than 64 NodeClaims)
            out.append(dict(k=100, n=600, seed=10 + seed, topo=topo))
            out.append(dict(k=160, n=800, seed=20 + seed, topo=topo, late=12))
            # RegSort: every inversion at 13-49 runs the whole pdqsort in registers
            out.append(dict(k=40, n=400, seed=30 + seed, topo=topo))
            # RegSort's upper range, the 64 | 65 boundary, and 64 -> 65 mid-script
            out.append(dict(k=60, n=400, seed=40 + seed, topo=topo))
            out.append(dict(k=64, n=400, seed=50 + seed, topo=topo, late_at=(200,)))
    return out


VARIANTS = _variants()
_cache = {}


def variant_id(v):
    return "k{k}-s{seed}".format(**v) + ("-topo" if v.get("topo") else "")


def scenario(v):
    """the built scenario of a VARIANTS entry (built once per process)"""
    key = variant_id(v)
    if key not in _cache:
        _cache[key] = build(name=key, **v)
    return _cache[key]


def is_wave(v):
    return v["k"] > 64


def claim_counts(result):
    """pods per NodeClaim in creation order of a solve()'s result dict"""
    return [len(c["pods"]) for c in result["claims"]]
