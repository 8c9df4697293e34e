"""gs_explain: why each NodePool could not take a pod (include/gpusched.h).

The reference here is a plain-Python restatement of the header's table over
problems built with synth.ProblemBuilder, restricted to: In / NotIn / Exists /
DoesNotExist on zone, capacity type, arch, instance-family and instance-type;
one custom label key set by a NodePool label; tolerations, requests, limits,
minValues on NodePool requirements; unavailable offerings; preferred
node-affinity terms.  On the CPU the model is first tied to the oracle (its
STATE is exactly pyoracle.feasibility's "a cheapest type exists") and shown to
reach every one of the 17 codes; on the GPU the product must equal the model
pair by pair.
"""
import ctypes as C

import numpy as np
import pytest

from gpusched import abi, explain, lib
from gpusched.problem import ProblemBuilder
from oracle import pyoracle

ZONE = "topology.kubernetes.io/zone"
CT = "karpenter.sh/capacity-type"
ARCH = "kubernetes.io/arch"
FAMILY = "karpenter-ibm.sh/instance-family"
ITYPE = "node.kubernetes.io/instance-type"
NODEPOOL = "karpenter.sh/nodepool"
HOSTNAME = "kubernetes.io/hostname"
TEAM = "example.com/team"  # the custom (not well-known) key
WELL_KNOWN = {NODEPOOL, ZONE, "topology.kubernetes.io/region", ITYPE, ARCH, "kubernetes.io/os", CT,
              "node.kubernetes.io/windows-build", "karpenter-ibm.sh/instance-size", FAMILY,
              "karpenter-ibm.sh/instance-cpu", "karpenter-ibm.sh/instance-memory"}
GI = 1 << 30
W = abi  # the GS_WHY_* / GS_MET_* constants


# ===================================================================== model
# a requirement on one key: (complement, frozenset of values)
def _req(op, values):
    op = {abi.OP_IN: "In", abi.OP_NOTIN: "NotIn", abi.OP_EXISTS: "Exists", abi.OP_DNE: "DoesNotExist"}.get(op, op)
    return {"In": (False, frozenset(values)), "NotIn": (True, frozenset(values)), "Exists": (True, frozenset()),
            "DoesNotExist": (False, frozenset())}[op]


def _and(a, b):
    if a[0] and b[0]:
        return (True, a[1] | b[1])
    if a[0]:
        return (False, b[1] - a[1])
    if b[0]:
        return (False, a[1] - b[1])
    return (False, a[1] & b[1])


def _has(r, v):
    return (v not in r[1]) if r[0] else (v in r[1])


def _exempt(r):  # operator NotIn or DoesNotExist
    return bool(r[1]) if r[0] else not r[1]


def _add(reqs, key, r):
    reqs[key] = _and(reqs[key], r) if key in reqs else r


def _compatible(have, incoming):
    """Requirements.Compatible(incoming, AllowUndefinedWellKnownLabels)"""
    for k, r in incoming.items():
        if k in WELL_KNOWN or k in have or _exempt(r):
            continue
        return False
    for k, r in incoming.items():
        if k in have:
            x = _and(have[k], r)
            if not x[0] and not x[1] and not (_exempt(have[k]) and _exempt(r)):
                return False
    return True


class Model:
    def __init__(self, problem):
        b = self.b = problem._builder
        s = self.s = b.strings
        self.res = sorted({s[q[0]] for q in b.quantities})
        self.types = []
        zones, cts = [], []
        for name, rq, cap, ovh, (ob, on) in b.instance_types:
            vals = {k: next(iter(r[1])) for k, r in self.reqs(rq).items()}
            c, o = self.qty(cap), self.qty(ovh)
            offs = []
            for orq, _price, avail in b.offerings[ob:ob + on]:
                orr = self.reqs(orq)
                z, ct = next(iter(orr[ZONE][1])), next(iter(orr[CT][1]))
                if z not in zones:
                    zones.append(z)
                if ct not in cts:
                    cts.append(ct)
                if avail:
                    offs.append((z, ct))
            self.types.append({"name": s[name], "vals": vals, "cap": c,
                               "alloc": {k: v - o.get(k, 0) for k, v in c.items()}, "offs": offs})
        self.zones, self.cts = zones, cts
        self.it_keys = set(self.types[0]["vals"])
        self.pools = [self.pool(np_) for np_ in b.nodepools]

    def reqs(self, rng, mins=None):
        out = {}
        for key, op, (vb, vn), mv in self.b.reqs[rng[0]:rng[0] + rng[1]]:
            k = self.s[key]
            _add(out, k, _req(op, [self.s[v] for v in self.b.value_ids[vb:vb + vn]]))
            if mins is not None and mv > 0:
                mins[k] = max(mins.get(k, 0), mv)
        return out

    def qty(self, rng):
        out = {}
        for r, m in self.b.quantities[rng[0]:rng[0] + rng[1]]:
            out[self.s[r]] = out.get(self.s[r], 0) + m
        return out

    def labels(self, rng):
        return [(self.s[k], self.s[v]) for k, v in self.b.labels[rng[0]:rng[0] + rng[1]]]

    def grid(self, reqs):
        zs = {z for z in self.zones if ZONE not in reqs or _has(reqs[ZONE], z)}
        cs = {c for c in self.cts if CT not in reqs or _has(reqs[CT], c)}
        return zs, cs

    def offered(self, it, grid):
        return any(z in grid[0] and c in grid[1] for z, c in it["offs"])

    def it_has(self, it, reqs):
        return all(_has(reqs[k], it["vals"][k]) for k in self.it_keys if k in reqs)

    def pool(self, np_):
        name, _w, rq, lb, tn, lim, has_lim, dm, (rb, rn) = np_
        mins = {}
        spec = self.reqs(rq, mins)
        tr = dict(spec)
        for k, v in self.labels(lb) + [(NODEPOOL, self.s[name])]:
            _add(tr, k, _req("In", [v]))
        grid = self.grid(tr)
        opts = []
        for i in self.b.it_refs[rb:rb + rn]:
            it = self.types[i]
            itr = {k: _req("In", [v]) for k, v in it["vals"].items()}
            if (_compatible(spec, itr) and all(v >= 0 for v in it["alloc"].values()) and self.it_has(it, tr)
                    and self.offered(it, grid)):
                opts.append(i)
        ok = bool(opts)
        for k, mv in mins.items():
            if k not in self.it_keys or len({self.types[i]["vals"][k] for i in opts}) < mv:
                ok = False
        limits = self.qty(lim)
        lim_opts = [i for i in opts if all(self.types[i]["cap"].get(r, 0) <= x for r, x in limits.items())]
        _add(tr, HOSTNAME, _req("In", ["\x01placeholder"]))
        return {"ok": ok, "reqs": tr, "mins": mins, "S": lim_opts if has_lim else opts, "daemon": self.qty(dm),
                "taints": [(tn[0] + j, tuple(self.s[x] for x in self.b.taints[tn[0] + j])) for j in range(tn[1])]}

    def pod_reqs(self, pod, as_given):
        """NewPodRequirements of the first variant (as given) or of the last
        one Preferences.Relax reaches: no preferred term, the last required one"""
        sel, req_t, pref_t = pod[3], pod[4], pod[5]
        out = {}
        for k, v in self.labels(sel):
            _add(out, k, _req("In", [v]))
        terms = self.b.terms
        if as_given and pref_t[1]:
            best = max(range(pref_t[1]), key=lambda j: (terms[pref_t[0] + j][1], -j))  # heaviest, first among equals
            for k, r in self.reqs(terms[pref_t[0] + best][0]).items():
                _add(out, k, r)
        if req_t[1]:
            j = 0 if as_given else req_t[1] - 1
            for k, r in self.reqs(terms[req_t[0] + j][0]).items():
                _add(out, k, r)
        return out

    def tolerates(self, pod, taint):
        k, v, eff = taint
        for tk, op, tv, te in self.b.tolerations[pod[6][0]:pod[6][0] + pod[6][1]]:
            tk, tv, te = self.s[tk], self.s[tv], self.s[te]
            if (te and te != eff) or (tk and tk != k):
                continue
            if op == abi.TOL_EXISTS or tv == v:
                return True
        return False

    def pair(self, pod, pl, as_given):
        """-> (cause, met, taint)"""
        if not pl["ok"]:
            return W.GS_WHY_NO_OPTIONS, 0, -1
        pre, taint = 0, -1
        if not pl["S"]:
            pre |= explain.PRE_LIMITS
        for idx, tn in pl["taints"]:
            if not self.tolerates(pod, tn):
                pre |= explain.PRE_TAINTS
                taint = idx
                break
        pr = self.pod_reqs(pod, as_given)
        if not _compatible(pl["reqs"], pr):
            pre |= explain.PRE_INCOMPATIBLE
        merged = dict(pl["reqs"])
        for k, r in pr.items():
            _add(merged, k, r)
        grid = self.grid(merged)
        dem = dict(pl["daemon"])
        for r, m in self.qty(pod[2]).items():
            dem[r] = dem.get(r, 0) + m
        met, alls = 0, []
        for i in pl["S"]:
            it = self.types[i]
            r = self.it_has(it, merged)
            f = all(m <= it["alloc"].get(x, 0) for x, m in dem.items())
            o = self.offered(it, grid)
            met |= (W.GS_MET_REQUIREMENTS if r else 0) | (W.GS_MET_FITS if f else 0) | (W.GS_MET_OFFERING if o else 0)
            met |= W.GS_MET_REQ_FITS_ONLY if r and f and not o else 0
            met |= W.GS_MET_REQ_OFFERING_ONLY if r and o and not f else 0
            met |= W.GS_MET_FITS_OFFERING_ONLY if f and o and not r else 0
            if r and f and o:
                met |= W.GS_MET_ALL
                alls.append(i)
        if any(len({self.types[i]["vals"][k] for i in alls}) < mv for k, mv in pl["mins"].items()):
            pre |= explain.PRE_MIN_VALUES
        cause = explain.cause_of(met, pre)
        early = cause in (W.GS_WHY_LIMITS, W.GS_WHY_TAINTS, W.GS_WHY_INCOMPATIBLE)
        return cause, 0 if early else met, taint if cause == W.GS_WHY_TAINTS else -1

    def explain(self, as_given=False, pods=None):
        pods = range(len(self.b.pods)) if pods is None else pods
        out = {"cause": np.zeros((len(pods), len(self.pools)), np.uint8),
               "met": np.zeros((len(pods), len(self.pools)), np.uint8),
               "taint": np.full((len(pods), len(self.pools)), -1, np.int32)}
        for j, p in enumerate(pods):
            for t, pl in enumerate(self.pools):
                out["cause"][j, t], out["met"][j, t], out["taint"][j, t] = self.pair(self.b.pods[p], pl, as_given)
        return out


# ================================================================= generators
TOL_ALL = [("", "Exists", "", "")]
TINY = {"cpu": 500, "memory": 1 * GI * 1000, "pods": 1000}
MID = {"cpu": 8000, "memory": 8 * GI * 1000, "pods": 1000}
HUGE = {"cpu": 1_000_000, "memory": 1 * GI * 1000, "pods": 1000}


def _it(b, name, family, arch, cpu, mem_gi, offerings):
    """offerings: (zone, capacity type, available)"""
    return b.add_instance_type(name, [(ITYPE, "In", [name]), (ARCH, "In", [arch]), (FAMILY, "In", [family])],
                               {"cpu": cpu * 1000, "memory": mem_gi * GI * 1000, "pods": 110_000},
                               {"cpu": 100, "memory": GI * 100},
                               [(z, ct, 0.05 * cpu + (0.0 if ct == "on-demand" else -0.01 * cpu) + 0.001 * k, av)
                                for k, (z, ct, av) in enumerate(offerings)])


def kat_catalog(b):
    """6 types, 2 zones, on-demand + spot"""
    _it(b, "a-small", "a", "amd64", 2, 4, [("z1", "on-demand", 1), ("z1", "spot", 1), ("z2", "on-demand", 1)])
    _it(b, "a-large", "a", "amd64", 16, 64, [("z1", "on-demand", 1)])
    _it(b, "b-small", "b", "amd64", 2, 4, [("z2", "on-demand", 1), ("z2", "spot", 1)])
    _it(b, "b-large", "b", "amd64", 16, 64, [("z2", "on-demand", 1)])
    _it(b, "c-small", "c", "arm64", 2, 4, [("z1", "on-demand", 1), ("z2", "spot", 0)])
    _it(b, "c-large", "c", "arm64", 16, 64, [("z1", "spot", 1)])


_uid = iter(range(1 << 30))


def _pod(b, requests=TINY, tolerations=TOL_ALL, **kw):
    return b.add_pod(f"pod-{next(_uid):08d}", 0, requests, tolerations=tolerations, **kw)


def kat_codes():
    """one pod per code against NodePool 0; NodePool 1 is within no limit,
    NodePool 2 keeps no option -> (problem, {code: (pod, nodepool)}, taint index)"""
    b = ProblemBuilder()
    kat_catalog(b)
    b.add_nodepool("main", requirements=[(FAMILY, "Exists", [], 2)], labels={TEAM: "a"},
                   taints=[("dedicated", "x", "NoSchedule"), ("gpu", "y", "NoSchedule")])
    b.add_nodepool("capped", limits={"cpu": 1000})
    b.add_nodepool("empty", requirements=[(ARCH, "In", ["s390x"])])
    ppc, z9 = (ARCH, "In", ["ppc64le"]), (ZONE, "In", ["z9"])
    z2spot = [(ZONE, "In", ["z2"]), (CT, "In", ["spot"])]
    smalls = (ITYPE, "In", ["a-small", "b-small", "c-small"])
    at = {
        W.GS_WHY_STATE: _pod(b),
        W.GS_WHY_TAINTS: _pod(b, tolerations=[("dedicated", "Equal", "x", "NoSchedule")]),
        W.GS_WHY_INCOMPATIBLE: _pod(b, node_selector={TEAM: "b"}),
        W.GS_WHY_MIN_VALUES: _pod(b, required_terms=[[(FAMILY, "In", ["a"])]]),
        W.GS_WHY_IT_NONE: _pod(b, HUGE, required_terms=[[ppc, z9]]),
        W.GS_WHY_IT_REQ_OR_FITS: _pod(b, HUGE, required_terms=[[ppc]]),
        W.GS_WHY_IT_REQ_OR_OFFERING: _pod(b, required_terms=[[ppc, z9]]),
        W.GS_WHY_IT_FITS_OR_OFFERING: _pod(b, HUGE, required_terms=[[z9]]),
        W.GS_WHY_IT_REQUIREMENTS: _pod(b, required_terms=[[ppc]]),
        W.GS_WHY_IT_RESOURCES: _pod(b, HUGE),
        W.GS_WHY_IT_OFFERING: _pod(b, required_terms=[[z9]]),
        # a-* meet R and F but are not offered in z2 spot; b-small is, and misses R
        W.GS_WHY_IT_REQ_FITS_NO_OFFERING: _pod(b, required_terms=[[(FAMILY, "In", ["a"])] + z2spot]),
        # the small types meet R and miss F; the large ones fit, are offered and miss R
        W.GS_WHY_IT_FITS_OFFERING_NO_REQ: _pod(b, MID, required_terms=[[smalls]]),
        # b-small meets R and O, not F; the types that fit meet neither R nor O
        W.GS_WHY_IT_REQ_OFFERING_NO_FITS: _pod(b, MID, required_terms=[[(ITYPE, "In", ["b-small"])] + z2spot]),
        # a-small meets only R, the large types only F, b-small only O
        W.GS_WHY_IT_TUPLE: _pod(b, MID, required_terms=[[(ITYPE, "In", ["a-small"])] + z2spot]),
    }
    where = {code: (pod, 0) for code, pod in at.items()}
    where[W.GS_WHY_LIMITS] = (at[W.GS_WHY_STATE], 1)
    where[W.GS_WHY_NO_OPTIONS] = (at[W.GS_WHY_STATE], 2)
    return b.build(), where, 1  # the second taint of "main" (taints 0 and 1)


def kat_distinctions():
    """INCOMPATIBLE versus IT_OFFERING / IT_REQUIREMENTS: K1 leaves an empty row for all of them"""
    b = ProblemBuilder()
    kat_catalog(b)
    b.add_nodepool("pinned", requirements=[(ZONE, "In", ["z1"]), (ARCH, "In", ["amd64"])])
    b.add_nodepool("open")
    b.add_nodepool("wide", requirements=[(ZONE, "In", ["z1", "z9"])])
    I, S, OFF, REQ = W.GS_WHY_INCOMPATIBLE, W.GS_WHY_STATE, W.GS_WHY_IT_OFFERING, W.GS_WHY_IT_REQUIREMENTS
    want = {
        _pod(b, required_terms=[[(ZONE, "In", ["z2"])]]): (I, S, I),
        _pod(b, required_terms=[[(ZONE, "In", ["z9"])]]): (I, OFF, OFF),   # a zone no offering has
        _pod(b, required_terms=[[(ZONE, "NotIn", ["z1", "z2"])]]): (I, OFF, OFF),
        _pod(b, required_terms=[[(ARCH, "In", ["arm64"])]]): (I, S, S),
        _pod(b, required_terms=[[(ARCH, "In", ["ppc64le"])]]): (I, REQ, REQ),  # an arch no type has
        _pod(b, required_terms=[[(ARCH, "DoesNotExist", [])]]): (I, REQ, REQ),
        _pod(b): (S, S, S),
    }
    return b.build(), want


def shape_problem(n, n_pools):
    """n types that differ only in the last one: its family, its size and the
    one zone only it is offered in.  Every type has an offering in every
    (zone, capacity type) a pod without a zone term can use, so ~O is all padding."""
    b = ProblemBuilder()
    for i in range(n):
        last = i == n - 1
        _it(b, f"t{i:05d}", "z" if last else "a", "amd64", 32 if last else 2, 128 if last else 4,
            [("z1", "on-demand", 1), ("z1", "spot", 1)] + ([("zlast", "on-demand", 1)] if last else []))
    b.add_nodepool("p0")
    if n_pools == 3:
        b.add_nodepool("p1", taints=[("t", "v", "NoSchedule")])
        b.add_nodepool("p2", requirements=[(FAMILY, "NotIn", ["z"])])
    pods = {
        "last_R": _pod(b, required_terms=[[(FAMILY, "In", ["z"])]]),
        "last_F": _pod(b, MID),
        "last_O": _pod(b, required_terms=[[(ZONE, "In", ["zlast"])]]),
        "all": _pod(b),
        "none_R": _pod(b, required_terms=[[(FAMILY, "In", ["q"])]]),
        "untolerated": _pod(b, tolerations=[]),
        "last_R_other_zone": _pod(b, required_terms=[[(FAMILY, "In", ["z"]), (ZONE, "In", ["z1"])]]),
    }
    return b.build(), pods


def random_problem(seed):
    """a sparse catalog (each type: one family, one size, few offerings), three
    NodePools with every restricted feature, pods that combine the terms"""
    rng = np.random.default_rng(0xE791A1 + seed)
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]  # noqa: E731
    b = ProblemBuilder()
    zones, cts, fams = ["z1", "z2", "z3"], ["on-demand", "spot"], ["a", "b", "c"]
    names = []
    for f in fams:
        for size, (cpu, mem) in (("s", (2, 4)), ("l", (16, 64))):
            offs = []
            for z in zones:
                for ct in cts:
                    if rng.random() < 0.3:
                        offs.append((z, ct, 0 if rng.random() < 0.2 else 1))
            offs = offs or [(pick(zones), pick(cts), 1)]
            names.append(f"{f}-{size}")
            _it(b, names[-1], f, "arm64" if f == "c" else "amd64", cpu, mem, offs)
    taints = [("dedicated", "x", "NoSchedule"), ("gpu", "y", "NoSchedule"), ("batch", "", "NoExecute")]
    for t in range(3):
        kw, reqs = {}, []
        u = rng.random()
        if u < 0.25:
            reqs.append((ZONE, pick(["In", "NotIn"]), [pick(zones)]))
        elif u < 0.4:
            reqs.append((ARCH, "In", [pick(["amd64", "arm64", "s390x"])]))
        elif u < 0.5:
            reqs.append((CT, "In", [pick(cts)]))
        if rng.random() < 0.3:
            reqs.append((FAMILY, "Exists", [], 2) if rng.random() < 0.5 else (FAMILY, "NotIn", [pick(fams)], 2))
        if rng.random() < 0.4:
            kw["labels"] = {TEAM: pick(["a", "b"])}
        if rng.random() < 0.4:
            kw["taints"] = [taints[i] for i in rng.permutation(3)[:int(rng.integers(1, 3))]]
        if rng.random() < 0.3:
            kw["limits"] = {"cpu": pick([1000, 4000, 64000])}
        if rng.random() < 0.3:
            kw["daemon"] = {"cpu": 500, "memory": GI * 500}
        if rng.random() < 0.2:
            kw["instance_types"] = sorted(int(i) for i in rng.permutation(len(names))[:3])
        b.add_nodepool(f"np{t}", weight=int(rng.integers(0, 3)), requirements=reqs, **kw)

    def term():
        out = []
        if rng.random() < 0.5:
            out.append((FAMILY, pick(["In", "In", "NotIn"]), [pick(fams)]))
        if rng.random() < 0.5:
            out.append((ZONE, pick(["In", "In", "In", "NotIn", "Exists"]), [pick(zones + ["z9"])]))
            if out[-1][1] == "Exists":
                out[-1] = (ZONE, "Exists", [])
        if rng.random() < 0.3:
            out.append((CT, "In", [pick(cts)]))
        if rng.random() < 0.25:
            out.append((ARCH, pick(["In", "In", "NotIn", "DoesNotExist"]), [pick(["amd64", "arm64", "ppc64le"])]))
            if out[-1][1] == "DoesNotExist":
                out[-1] = (ARCH, "DoesNotExist", [])
        if rng.random() < 0.3:
            out.append((ITYPE, pick(["In", "NotIn"]), [pick(names), pick(names)]))
        if rng.random() < 0.15:
            out.append((TEAM, pick(["In", "NotIn", "Exists", "DoesNotExist"]), [pick(["a", "b"])]))
            if out[-1][1] in ("Exists", "DoesNotExist"):
                out[-1] = (TEAM, out[-1][1], [])
        return out

    for _ in range(24):
        kw = {}
        if rng.random() < 0.15:
            # one small type named, one (zone, capacity type), a request only the
            # large types fit: the rare "exactly two" and tuple causes
            _pod(b, MID, required_terms=[[(ITYPE, "In", [pick(names[0::2])]), (ZONE, "In", [pick(zones)]),
                                          (CT, "In", [pick(cts)])]])
            continue
        if rng.random() < 0.8:
            kw["required_terms"] = [term()]
        if rng.random() < 0.3:
            kw["preferred_terms"] = [(int(rng.integers(1, 100)), term()) for _ in range(int(rng.integers(1, 3)))]
        if rng.random() < 0.2:
            kw["node_selector"] = {pick([ZONE, TEAM]): pick(["z1", "a"])}
        tols = []
        for k, v, eff in taints:
            if rng.random() < 0.7:
                tols.append((k, "Equal", v, eff) if rng.random() < 0.5 else (k, "Exists", "", ""))
        _pod(b, pick([TINY, TINY, MID, MID, HUGE]), tolerations=TOL_ALL if rng.random() < 0.3 else tols, **kw)
    return b.build()


SEEDS = list(range(40))


@pytest.fixture(scope="module")
def random_cases():
    """(problem, model results as given, model results relaxed) per seed, computed once"""
    out = []
    for seed in SEEDS:
        pr = random_problem(seed)
        m = Model(pr)
        out.append((pr, m.explain(as_given=True), m.explain(as_given=False)))
    return out


# ======================================================================== CPU
def test_exported_and_layout_matches_library():
    L = lib.load()
    assert "gs_explain" in lib.EXPORTS and "gs_explain_result_size" in lib.EXPORTS
    assert hasattr(L, "gs_explain")
    assert L.gs_explain_result_size() == C.sizeof(abi.GsExplainResult)


def test_model_reaches_every_code(random_cases):
    """keeps the GPU parity test from passing on STATE alone"""
    counts = np.zeros(abi.GS_WHY_COUNT, np.int64)
    for _, given, relaxed in random_cases:
        for r in (given, relaxed):
            counts += np.bincount(r["cause"].ravel(), minlength=abi.GS_WHY_COUNT)
    print({explain.CAUSE_NAMES[c]: int(n) for c, n in enumerate(counts)})
    assert (counts >= 5).all(), {explain.CAUSE_NAMES[c]: int(n) for c, n in enumerate(counts)}


def test_model_state_is_the_oracles_feasibility(random_cases):
    """the model is checked before it checks the product: as given, STATE holds
    exactly where the oracle finds a cheapest type, for every pair"""
    for seed, (pr, given, _) in zip(SEEDS, random_cases):
        st, feas = pyoracle.feasibility(pr)
        assert st == abi.GS_OK, seed
        assert ((given["cause"] == W.GS_WHY_STATE) == (feas["cheapest"] != -1)).all(), seed


def test_model_on_the_kats():
    pr, where, taint = kat_codes()
    m = Model(pr).explain()
    for code, (pod, pool) in where.items():
        assert m["cause"][pod, pool] == code, explain.CAUSE_NAMES[code]
    assert sorted(where) == list(range(abi.GS_WHY_COUNT))
    pr, want = kat_distinctions()
    m = Model(pr).explain()
    for pod, causes in want.items():
        assert tuple(m["cause"][pod]) == causes, pod


# ======================================================================== GPU
@pytest.fixture(scope="module")
def solver():
    s = lib.Solver(0)
    yield s
    s.close()


def _same(got, want, what):
    for k in ("cause", "met", "taint"):
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (what, k, bad[:5].tolist(), [(int(got[k][tuple(x)]), int(want[k][tuple(x)])) for x in bad[:5]])


@pytest.mark.gpu
def test_kat_one_pod_per_code(solver):
    pr, where, taint = kat_codes()
    solver.prepare(pr)
    got = solver.explain()
    assert got["cause"].shape == (len(pr.pods), 3)
    pod = lambda code: where[code]  # noqa: E731
    assert got["cause"][pod(W.GS_WHY_STATE)] == W.GS_WHY_STATE
    assert got["cause"][pod(W.GS_WHY_NO_OPTIONS)] == W.GS_WHY_NO_OPTIONS
    assert got["cause"][pod(W.GS_WHY_LIMITS)] == W.GS_WHY_LIMITS
    assert got["cause"][pod(W.GS_WHY_TAINTS)] == W.GS_WHY_TAINTS
    assert got["cause"][pod(W.GS_WHY_INCOMPATIBLE)] == W.GS_WHY_INCOMPATIBLE
    assert got["cause"][pod(W.GS_WHY_MIN_VALUES)] == W.GS_WHY_MIN_VALUES
    assert got["cause"][pod(W.GS_WHY_IT_NONE)] == W.GS_WHY_IT_NONE
    assert got["cause"][pod(W.GS_WHY_IT_REQ_OR_FITS)] == W.GS_WHY_IT_REQ_OR_FITS
    assert got["cause"][pod(W.GS_WHY_IT_REQ_OR_OFFERING)] == W.GS_WHY_IT_REQ_OR_OFFERING
    assert got["cause"][pod(W.GS_WHY_IT_FITS_OR_OFFERING)] == W.GS_WHY_IT_FITS_OR_OFFERING
    assert got["cause"][pod(W.GS_WHY_IT_REQUIREMENTS)] == W.GS_WHY_IT_REQUIREMENTS
    assert got["cause"][pod(W.GS_WHY_IT_RESOURCES)] == W.GS_WHY_IT_RESOURCES
    assert got["cause"][pod(W.GS_WHY_IT_OFFERING)] == W.GS_WHY_IT_OFFERING
    assert got["cause"][pod(W.GS_WHY_IT_REQ_FITS_NO_OFFERING)] == W.GS_WHY_IT_REQ_FITS_NO_OFFERING
    assert got["cause"][pod(W.GS_WHY_IT_FITS_OFFERING_NO_REQ)] == W.GS_WHY_IT_FITS_OFFERING_NO_REQ
    assert got["cause"][pod(W.GS_WHY_IT_REQ_OFFERING_NO_FITS)] == W.GS_WHY_IT_REQ_OFFERING_NO_FITS
    assert got["cause"][pod(W.GS_WHY_IT_TUPLE)] == W.GS_WHY_IT_TUPLE
    # the NodePool's second taint is the untolerated one; -1 everywhere else
    assert got["taint"][pod(W.GS_WHY_TAINTS)] == taint
    assert (got["taint"][got["cause"] != W.GS_WHY_TAINTS] == -1).all()
    # met is 0 where the cause is decided before the instance types
    early = np.isin(got["cause"], [W.GS_WHY_NO_OPTIONS, W.GS_WHY_LIMITS, W.GS_WHY_TAINTS, W.GS_WHY_INCOMPATIBLE])
    assert (got["met"][early] == 0).all()
    assert got["met"][pod(W.GS_WHY_IT_TUPLE)] == W.GS_MET_REQUIREMENTS | W.GS_MET_FITS | W.GS_MET_OFFERING
    assert got["met"][pod(W.GS_WHY_MIN_VALUES)] & W.GS_MET_ALL
    _same(got, Model(pr).explain(), "kat")
    texts = explain.pod_error(got, pod(W.GS_WHY_TAINTS)[0], ["main", "capped", "empty"],
                              [tuple(pr.strings[x] for x in t) for t in pr._builder.taints])
    assert texts == ["main: did not tolerate taint gpu=y:NoSchedule",
                     "capped: all available instance types exceed limits for nodepool"]


@pytest.mark.gpu
def test_kat_incompatible_versus_instance_type_causes(solver):
    pr, want = kat_distinctions()
    solver.prepare(pr)
    got = solver.explain()
    for pod, causes in want.items():
        assert tuple(got["cause"][pod]) == causes, pod
    _same(got, Model(pr).explain(), "distinctions")
    # K1 folds them together: every non-STATE pair has an empty row
    feas, _ = solver.feasibility()
    assert ((got["cause"] == W.GS_WHY_STATE) == (feas["cheapest"] != -1)).all()


@pytest.mark.gpu
def test_random_parity_with_the_model(solver, random_cases):
    for seed, (pr, given, relaxed) in zip(SEEDS, random_cases):
        solver.prepare(pr)
        _same(solver.explain(as_given=True), given, (seed, "as given"))
        _same(solver.explain(), relaxed, (seed, "relaxed"))
        feas, _ = solver.feasibility()
        st, ofeas = pyoracle.feasibility(pr)
        assert st == abi.GS_OK
        state = solver.explain(as_given=True)["cause"] == W.GS_WHY_STATE
        assert (state == (feas["cheapest"] != -1)).all(), seed
        assert (state == (ofeas["cheapest"] != -1)).all(), seed


SHAPES = [(n, n_pools) for n in (3, 64, 65, 130, 2100) for n_pools in (1, 3)]


@pytest.mark.gpu
def test_shapes_last_bit_and_padding(solver):
    """1, 2, 3 and 33 words, one template and three; the only type that meets a
    criterion is the last valid bit of the last word; 7 x n_pools pairs are no
    multiple of the pairs per wave (64, 32, 16 for the first four sizes).  One
    test over all ten shapes: each takes a few milliseconds."""
    for n, n_pools in SHAPES:
        _check_shape(solver, n, n_pools)


def _check_shape(solver, n, n_pools):
    pr, pods = shape_problem(n, n_pools)
    solver.prepare(pr)
    feas, _ = solver.feasibility()
    for as_given in (True, False):
        got = solver.explain(as_given=as_given)
        c, m = got["cause"][:, 0], got["met"][:, 0]
        for name in ("last_R", "last_F", "last_O", "last_R_other_zone"):
            assert c[pods[name]] == W.GS_WHY_STATE, (n, n_pools, name)
            assert feas["cheapest"][pods[name], 0] == n - 1, (n, n_pools, name)
        every = W.GS_MET_REQUIREMENTS | W.GS_MET_FITS | W.GS_MET_OFFERING | W.GS_MET_ALL
        # every type meets all three: a counted padding bit would set an "exactly two" flag
        assert m[pods["all"]] == every
        # only the last type meets R; the others meet F and O
        assert m[pods["last_R"]] == every | W.GS_MET_FITS_OFFERING_ONLY
        assert m[pods["last_F"]] == every | W.GS_MET_REQ_OFFERING_ONLY
        assert m[pods["last_O"]] == every | W.GS_MET_REQ_FITS_ONLY
        assert c[pods["none_R"]] == W.GS_WHY_IT_REQUIREMENTS
        assert m[pods["none_R"]] == W.GS_MET_FITS | W.GS_MET_OFFERING | W.GS_MET_FITS_OFFERING_ONLY
        if n_pools == 3:
            assert got["cause"][pods["untolerated"], 1] == W.GS_WHY_TAINTS
            assert got["cause"][pods["last_R"], 2] == W.GS_WHY_INCOMPATIBLE  # family NotIn [z] against In [z]
        assert ((got["cause"] == W.GS_WHY_STATE) == (feas["cheapest"] != -1)).all()
    if n <= 130:  # (the model walks every type in Python)
        _same(solver.explain(), Model(pr).explain(), n)


@pytest.mark.gpu
def test_call_forms(solver):
    fresh = lib.Solver(0)  # nothing prepared: GS_E_INVALID
    try:
        assert fresh.L.gs_explain(fresh.ctx, None, 0, 0, C.byref(abi.GsExplainResult())) == abi.GS_E_INVALID
    finally:
        fresh.close()
    pr = random_problem(3)
    n = len(pr.pods)
    solver.prepare(pr)
    full = solver.explain()
    assert full["pods"].tolist() == list(range(n))
    _same(solver.explain(pods=list(range(n))), full, "explicit list")
    rng = np.random.default_rng(7)
    some = [int(x) for x in rng.integers(0, n, size=2 * n + 5)]  # shuffled, with repeats
    got = solver.explain(pods=some)
    assert got["pods"].tolist() == some and got["n_variants"] <= len(set(some))
    _same(got, {k: full[k][some] for k in ("cause", "met", "taint")}, "subset")
    n_templates = int((full["cause"][0] != W.GS_WHY_NO_OPTIONS).sum())  # a NodePool without options has no template
    assert 0 < n_templates <= 3
    assert got["d2h_bytes"] == 4 * got["n_variants"] * n_templates and got["t_kernel_ms"] > 0 and got["t_total_ms"] > 0
    # n = 0 with a list: accepted, empty, no device work
    empty = solver.explain(pods=[])
    assert empty["pods"].size == 0 and empty["cause"].shape == (0, 3) and empty["d2h_bytes"] == 0
    assert empty["n_variants"] == 0 and empty["t_kernel_ms"] == 0
    # an index out of range: GS_E_INVALID, the previous result intact
    keep = solver.explain(pods=some, raw=True)
    before = abi.explain_to_dict(keep)
    res = abi.GsExplainResult()
    bad = (C.c_uint32 * 3)(0, n, 1)
    assert solver.L.gs_explain(solver.ctx, bad, 3, 0, C.byref(res)) == abi.GS_E_INVALID
    assert "out of range" in solver._err()
    assert solver.L.gs_explain(solver.ctx, bad, 1, 2, C.byref(res)) == abi.GS_E_INVALID  # unknown flag
    assert solver.L.gs_explain(solver.ctx, None, 3, 0, C.byref(res)) == abi.GS_E_INVALID
    assert solver.L.gs_explain(solver.ctx, bad, 1, 0, None) == abi.GS_E_INVALID
    _same(abi.explain_to_dict(keep), before, "previous result")
    assert abi.explain_to_dict(keep)["pods"].tolist() == some
    # the list may be the previous explain result's own
    again = abi.GsExplainResult()
    assert solver.L.gs_explain(solver.ctx, keep.pods, keep.n_pods, 0, C.byref(again)) == abi.GS_OK
    _same(abi.explain_to_dict(again), before, "own list")
    # a short list, every pod, the short list again: the buffers regrow and are reused
    _check_buffers_regrow_and_shrink()


@pytest.mark.gpu
def test_sharded_context_answers_on_the_solve_device():
    """a context with shards (one device, repeated) runs the call on the parent"""
    pr, where, _ = kat_codes()
    s = lib.Solver(0, shard_devices=[0, 0])
    try:
        s.prepare(pr)
        _same(s.explain(), Model(pr).explain(), "sharded")
        _same(s.explain(as_given=True), Model(pr).explain(as_given=True), "sharded, as given")
    finally:
        s.close()


@pytest.mark.gpu
def test_relaxation(solver):
    """a preferred term on a zone no offering has, and a request no type fits"""
    b = ProblemBuilder()
    kat_catalog(b)
    b.add_nodepool("open")
    p = _pod(b, HUGE, preferred_terms=[(10, [(ZONE, "In", ["z9"])])])
    pr = b.build()
    solver.prepare(pr)
    assert solver.explain()["cause"][p, 0] == W.GS_WHY_IT_RESOURCES
    assert solver.explain(as_given=True)["cause"][p, 0] == W.GS_WHY_IT_FITS_OR_OFFERING
    _same(solver.explain(as_given=True), Model(pr).explain(as_given=True), "as given")


def _check_buffers_regrow_and_shrink():
    """One context: 2 pods, then all 64 (2 -> 64 variants: the device buffer and
    both pinned sides regrow), then the 2 again.  Each answer is a fresh
    context's for the same call, and the model's."""
    b = ProblemBuilder()
    kat_catalog(b)
    b.add_nodepool("open")
    b.add_nodepool("tainted", taints=[("dedicated", "x", "NoSchedule")])
    for i in range(64):
        kw = {"required_terms": [[(ARCH, "In", ["ppc64le"])]]} if i % 7 == 3 else {}
        _pod(b, HUGE if i % 5 == 2 else {"cpu": 500 + 10 * i, "memory": GI * 1000, "pods": 1000},
             tolerations=TOL_ALL if i % 3 == 0 else [], **kw)
    pr = b.build()
    calls = ([5, 2], None)

    def fresh(pods):
        s = lib.Solver(0)
        try:
            s.prepare(pr)
            return s.explain(pods=pods)
        finally:
            s.close()

    want = [fresh(pods) for pods in calls]
    assert want[0]["n_variants"] == 2 and want[1]["n_variants"] == 64
    assert len({tuple(want[1]["cause"][p]) for p in calls[0]}) == 2  # a stale row would show
    s = lib.Solver(0)
    try:
        s.prepare(pr)
        for j in (0, 1, 0):
            got = s.explain(pods=calls[j])
            assert got["pods"].tolist() == want[j]["pods"].tolist() and got["n_variants"] == want[j]["n_variants"]
            _same(got, want[j], ("call", j))
    finally:
        s.close()
    _same(want[1], Model(pr).explain(), "model")
    _same(want[0], Model(pr).explain(pods=calls[0]), "model, two pods")


def _solve_problem():
    """some unschedulable pods; no topology, limits, host ports or volumes"""
    b = ProblemBuilder()
    kat_catalog(b)
    b.add_nodepool("open")
    b.add_nodepool("tainted", taints=[("dedicated", "x", "NoSchedule")])
    for i in range(40):
        kw = {}
        if i % 7 == 3:
            kw["required_terms"] = [[(ARCH, "In", ["ppc64le"])]]
        if i % 9 == 4:
            kw["preferred_terms"] = [(5, [(ZONE, "In", ["z2"])])]
        _pod(b, HUGE if i % 5 == 2 else TINY, tolerations=[], **kw)
    return b.build()


@pytest.mark.gpu
def test_with_a_solve():
    """gs_explain(res.error_pods, res.n_errors) with the pointer straight from
    the result, on the default context and on the block Solve kernel"""
    for flags in (0, abi.GS_CFG_BLOCK_SOLVE):
        _check_with_a_solve(flags)


def _check_with_a_solve(flags):
    pr = _solve_problem()
    s = lib.Solver(0, flags=flags)
    try:
        s.prepare(pr)
        feas0, _ = s.feasibility()
        s.run()
        before, res = s.fetch()
        assert res.n_errors >= 8
        errors = [int(res.error_pods[i]) for i in range(res.n_errors)]
        why = s.explain(pods=(res.error_pods, res.n_errors))
        assert why["pods"].tolist() == errors
        # without Solve state to blame, some NodePool names a cause for every error pod
        assert not (why["cause"] == W.GS_WHY_STATE).all(axis=1).any()
        assert set(why["cause"][:, 1]) == {W.GS_WHY_TAINTS}
        _same(why, Model(pr).explain(pods=errors), "error pods")
        # the gs_result read afterwards is unchanged
        assert [int(res.error_pods[i]) for i in range(res.n_errors)] == errors
        assert abi.result_to_dict(res, pr) == before
        # ... and so are a following run + fetch and a following feasibility
        s.run()
        after, _ = s.fetch()
        assert after == before
        feas1, _ = s.feasibility()
        for k in ("rows", "cheapest", "n_feasible_offerings", "cheapest_key"):
            assert (feas0[k] == feas1[k]).all(), k
        st, want, _ = pyoracle.solve(pr)
        assert st == abi.GS_OK and before == want
    finally:
        s.close()
