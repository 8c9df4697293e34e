"""Solve problems for every resource count R = 1..8 the kernels are compiled for.

A resource's slot is the rank of its name among the problem's sorted resource
names, and the kernels treat slots 0..3 (LDS slack / room codes, fast accept,
run mode, the claim hint) and slots 4..7 (ClaimRec.tot_hi / thr_hi, exact check
only) differently.  resource_names(R, layout) picks the names so that both
sides of that line are reached from both directions:

  tail  cpu, memory, pods keep slots 0..2 and the extended resources
        (vendor.example/r*) follow; at R >= 5 only a pod that asks for an
        extended resource has a request in a high slot
  head  the extended resources (acme.example/r*) sort first and push cpu,
        memory, pods to slots R-3..R-1: at R >= 5 every pod's `pods` request
        is high, at R >= 7 cpu, memory and pods all are (R >= 4 only)

Every (R, layout) pair of PAIRS gets the same seeded cases (CASES), each the
smallest shape that reaches the kernels named beside it:

  plain            36 types, 300 pods, family selectors, one pod per resource
                   that no type holds in that resource alone
                   (plain wave / HBM / block Solve, K1, gs_explain)
  runs             18 small types, 1,500 pods in blocks of identical pods
                   (run mode, exact batches in runs, the claim hint)
  nodes            30 existing nodes with bound pods, 300 pending
                   (ExistingNode.CanAdd, node codes, the node hint)
  general          nodes + zone and hostname spreads + a minValues NodePool
                   (the TOPO instantiations)
  wide             264 types (5 option words), 200 pods (WIDE instantiations)
  wide_spread      wide with zone spreads (WIDE and TOPO)
  cluster          64 nodes with bound pods, every node a candidate
                   (the simulation kernel)
  cluster_general  cluster with spreads on the bound pods (its general form)

and one shape beside them, "roomy": 150 identical small pods without
requirements, then 30 like them that ask for one extended resource each, into
a few large NodeClaims with room to spare, so that whether a pod was placed
with or without the exact check shows in gs_result's cand_full.

Capacities of the extended resources differ per family and size.  So that
each resource decides something whatever else is tight, every Solve case also
holds, per resource, pods that ask for nine tenths of the largest allocatable
of it (they lead the queue and cannot share a NodeClaim), and every cluster a
node per resource that runs one such pod.

problem(case, R, layout, drop=resource) is the same problem with that
resource's requests set to zero on every pod (the deliberately unschedulable
ones keep theirs; node availability is left as it was): tests/test_resource_sweep.py
uses it to show that each resource decides something.
"""
import copy
import ctypes as C
import functools

import numpy as np

from gpusched import abi, synth
from gpusched.consolidation import ConsolidationInput
from gpusched.problem import ProblemBuilder
from oracle import pyoracle

GI, MI = synth.GI, synth.MI
FAMILY_KEY = "karpenter-ibm.sh/instance-family"
SIZE_KEY = "karpenter-ibm.sh/instance-size"
ZONE_KEY = "topology.kubernetes.io/zone"
HOST_KEY = "kubernetes.io/hostname"
ZONES = synth.FAKE_ZONES
TS0 = 1_700_000_000_000_000_000

BASE = ("cpu", "memory", "pods")
LAYOUTS = ("tail", "head")
PAIRS = [(r, "tail") for r in range(1, 9)] + [(r, "head") for r in range(4, 9)]
CASES = ("plain", "runs", "nodes", "general", "wide", "wide_spread", "cluster", "cluster_general")
SOLVE_CASES = CASES[:6]
CLUSTER_CASES = CASES[6:]
ROOMY = "roomy"   # beside CASES: a counter probe, not a parity shape


def pair_id(pair):
    return f"r{pair[0]}-{pair[1]}"


def resource_names(R, layout):
    """the R resource names of a layout, in slot order"""
    assert R >= 1 and layout in LAYOUTS and (layout == "tail" or R >= 4)
    base = list(BASE[:min(R, 3)])
    extras = [("vendor.example" if layout == "tail" else "acme.example") + f"/r{k}" for k in range(max(0, R - 3))]
    names = sorted(base + extras)
    assert names == (base + extras if layout == "tail" else extras + base)
    return names


def extras_of(names):
    return [n for n in names if n not in BASE]


SIZES = [2, 4, 8, 16, 32, 48]
SIZES_SMALL = [2, 4, 8]
SIZES_WIDE = [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16]
FAMS = synth.FAMILIES[:6]
FAMS_WIDE = synth.FAMILIES + [f + "a" for f in synth.FAMILIES]
DAEMON = {"cpu": 200, "memory": 256 * MI * 1000, "pods": 2000}
OVERHEAD = {"cpu": 200, "memory": 2560 * MI * 1000}
CPUS = [int(x) for x in synth.CPU_CHOICES]
MEMS = [int(x) for x in synth.MEM_CHOICES]
LIGHT_ROOM = {"cpu": 4000, "memory": 6 * GI * 1000, "pods": 5000}
HEAVY_CPU = 2500       # above every other pod's: the heavy pods lead the queue
USES_EXTRAS = 0.6      # share of pods that may ask for extended resources ...
EACH_EXTRA = 0.25      # ... so that about this share asks for each one


def _only(d, names):
    return {k: v for k, v in d.items() if k in names}


class _Gen:
    """one problem under construction: the names decide which resources exist at all"""

    def __init__(self, seed, names):
        self.rng = np.random.default_rng(seed)
        self.names, self.extras = names, extras_of(names)
        self.b = ProblemBuilder()
        self.types = []   # (name, requirements, capacity, allocatable, family, size index)
        self.kept = []    # pending pods whose requests `without` leaves alone

    def catalog(self, fams, sizes):
        for fi, fam in enumerate(fams):
            ratio = synth.MEM_RATIO[fam[0]]
            for si, v in enumerate(sizes):
                name = f"{fam}-{v}x{v * ratio}"
                cap = {"cpu": v * 1000, "memory": v * ratio * GI * 1000, "pods": min(110, 4 + v) * 1000}
                # per family and size, so each extended resource has many distinct allocatable values
                units = [-(-v // 4) * ((fi + k) % 3 + 1) for k in range(len(self.extras))]
                cap.update({x: u * 1000 for x, u in zip(self.extras, units)})
                cap = _only(cap, self.names)
                ovh = _only(OVERHEAD, self.names)
                reqs = [("node.kubernetes.io/instance-type", "In", [name]), ("kubernetes.io/arch", "In", ["amd64"]),
                        (FAMILY_KEY, "In", [fam]), (SIZE_KEY, "In", [name.split("-", 1)[1]])]
                price = round(0.0475 * v + 0.006 * v * ratio + 0.011 * sum(units), 4)
                offs = [(z, ct, price * (0.6 if ct == "spot" else 1.0), True) for z in ZONES for ct in ("on-demand", "spot")]
                self.b.add_instance_type(name, reqs, cap, ovh, offs)
                self.types.append((name, reqs, cap, {r: cap[r] - ovh.get(r, 0) for r in cap}, fam, si))

    def pool(self, name="default", **kw):
        self.b.add_nodepool(name, requirements=[(ZONE_KEY, "In", ZONES)] + kw.pop("requirements", []),
                            daemon=_only(DAEMON, self.names), **kw)

    def requests(self, cpu=None, mem=None):
        rng = self.rng
        cpu = int(rng.choice(CPUS, p=synth.CPU_W / synth.CPU_W.sum())) if cpu is None else cpu
        mem = int(rng.choice(MEMS)) if mem is None else mem
        req = {"cpu": cpu, "memory": mem, "pods": 1000}
        uses = rng.random() < USES_EXTRAS
        for x in self.extras:
            if rng.random() < EACH_EXTRA / USES_EXTRAS and uses:
                req[x] = int(rng.choice([1000, 2000]))
        return _only(req, self.names)

    def uid(self):
        return synth._uid(self.rng)

    def ts(self):
        return TS0 + int(self.rng.integers(0, 8)) * 1_000_000_000

    def pod(self, req, keep=False, **kw):
        i = self.b.add_pod(self.uid(), kw.pop("ts", None) or self.ts(), req, **kw)
        if keep:
            self.kept.append(i)
        return i

    def error_pods(self):
        """per resource, a pod that exceeds every type's allocatable in that resource alone"""
        small = _only({"cpu": 100, "memory": 128 * MI * 1000, "pods": 1000}, self.names)
        for r in self.names:
            top = max(t[3][r] for t in self.types)
            self.pod(dict(small, **{r: top + 1000}), keep=True)

    def heavy(self, r):
        """requests that take nine tenths of what the largest type of r leaves a pod, and little else"""
        small = _only({"cpu": HEAVY_CPU, "memory": 128 * MI * 1000, "pods": 1000}, self.names)
        return dict(small, **{r: (max(t[3][r] for t in self.types) - DAEMON.get(r, 0)) * 9 // 10})

    def heavy_pods(self, per_resource=2):
        """per resource, pods that no NodeClaim holding a tenth of it can take:
        where they land depends on that resource alone"""
        for r in self.names:
            for _ in range(per_resource):
                self.pod(self.heavy(r))

    def heavy_nodes(self, first):
        """per resource, a node of the largest type of it that runs one such pod
        and has little room left, as the light nodes: the pod fits no other
        node for that resource alone"""
        for k, r in enumerate(self.names, start=first):
            name, reqs, cap, alloc, fam, si = max(self.types, key=lambda t: (t[3][r], t[2]["cpu"]))
            labels = {q[0]: q[2][0] for q in reqs}
            labels.update({ZONE_KEY: ZONES[k % 3], "karpenter.sh/capacity-type": "on-demand",
                           "karpenter.sh/nodepool": "default", "kubernetes.io/os": "linux", HOST_KEY: f"node-{k:03d}"})
            req = self.heavy(r)
            self.b.add_bound_pod(k, self.uid(), self.ts(), req)
            daemon = _only(DAEMON, self.names)
            avail = {x: min(alloc[x] - daemon.get(x, 0) - req.get(x, 0), LIGHT_ROOM.get(x, 2000)) for x in alloc}
            self.b.add_node(f"node-{k:03d}", labels, avail)

    def nodes(self, n, sizes, util, spread_apps=None, fill=None, light=None):
        """n state nodes of the catalog's types in `sizes` with bound pods up to
        `util` of their cpu, memory and pods (or until an extended resource is
        full).  light = (every, size index, util): every that-many-th node is of
        the larger size and lightly used (its pods fit no other node, a cheaper
        type holds them); the other nodes are then packed with the smallest pod
        shape after the first misfit"""
        rng = self.rng
        daemon = _only(DAEMON, self.names)
        for k in range(n):
            is_light = light is not None and k % light[0] == light[0] // 2
            cand = [t for t in self.types if (t[5] == light[1] if is_light else t[5] in sizes)]
            name, reqs, cap, alloc, fam, si = cand[int(rng.integers(0, len(cand)))]
            labels = {r[0]: r[2][0] for r in reqs}
            labels.update({ZONE_KEY: ZONES[k % 3], "karpenter.sh/capacity-type": "on-demand",
                           "karpenter.sh/nodepool": "default", "kubernetes.io/os": "linux", HOST_KEY: f"node-{k:03d}"})
            used = {r: daemon.get(r, 0) for r in alloc}
            target = float(rng.uniform(*(light[2] if is_light else util)))
            ts = self.ts()

            def fits(req):
                return all(used[r] + q <= (target if r in BASE else 1.0) * alloc[r] for r, q in req.items())

            packing = False
            for _ in range(200):
                req = self.requests(*(fill(rng) if fill else ()))
                if packing:
                    req = _only({"cpu": CPUS[2], "memory": MEMS[0], "pods": 1000}, self.names)
                if not fits(req):
                    if packing or light is None or is_light:
                        break
                    packing = True
                    continue
                for r, q in req.items():
                    used[r] += q
                kw = self.spread(spread_apps) if spread_apps else {}
                self.b.add_bound_pod(k, self.uid(), ts, req, **kw)
            avail = {r: alloc[r] - used[r] for r in alloc}
            if is_light:
                # pods that do not move hold the rest: little room is left
                avail = {r: min(q, LIGHT_ROOM.get(r, 2000)) for r, q in avail.items()}
            self.b.add_node(f"node-{k:03d}", labels, avail)

    def spread(self, apps):
        """labels and the app's spread: zone (DoNotSchedule / ScheduleAnyway),
        hostname only (VF_HOSTFA), or none"""
        app = apps[int(self.rng.integers(0, len(apps)))]
        sel = {"labels": {"app": app}}
        sp = {"web": [{"key": ZONE_KEY, "max_skew": 1, "selector": sel}],
              "api": [{"key": HOST_KEY, "max_skew": 3, "selector": sel}],
              "cache": [{"key": ZONE_KEY, "max_skew": 2, "when": "ScheduleAnyway", "selector": sel}]}.get(app, [])
        return {"labels": {"app": app}, "spreads": sp}

    def pending(self, n, selector_frac=0.0, apps=None):
        fams = sorted({t[4] for t in self.types})
        for _ in range(n):
            req = self.requests()
            kw = self.spread(apps) if apps else {}
            if self.rng.random() < selector_frac and not kw.get("spreads"):
                kw["node_selector"] = {FAMILY_KEY: fams[int(self.rng.integers(0, len(fams)))]}
            self.pod(req, **kw)


APPS = ["web", "api", "batch", "cache"]
RUN_SPECS = [(2000, 4 * GI * 1000), (1000, 2 * GI * 1000), (1000, 1 * GI * 1000), (500, 1 * GI * 1000),
             (250, 512 * MI * 1000), (100, 128 * MI * 1000)]
RUN_BLOCK, RUN_BLOCKS = 25, 10
CLUSTER_NODES = 64   # node CLUSTER_NODES + k runs the nine-tenths pod of resource slot k


def _build(case, names, seed):
    g = _Gen(seed, names)
    if case == "plain":
        g.catalog(FAMS, SIZES)
        g.pool()
        g.pending(300, selector_frac=0.15)
        g.heavy_pods()
        g.error_pods()
    elif case == "runs":
        # per (cpu, memory) spec ten blocks of 25 identical pods, a block's pods
        # one creation time: the queue keeps each block together, and every odd
        # block asks for one extended resource on top (the hint hand-over)
        g.catalog(FAMS, SIZES_SMALL)
        g.pool()
        for s, (cpu, mem) in enumerate(RUN_SPECS):
            for blk in range(RUN_BLOCKS):
                req = _only({"cpu": cpu, "memory": mem, "pods": 1000}, names)
                if blk % 2 and g.extras:
                    req[g.extras[(s + blk // 2) % len(g.extras)]] = 1000
                for _ in range(RUN_BLOCK):
                    g.pod(req, ts=TS0 + blk * 1_000_000_000)
        g.heavy_pods()
    elif case in ("nodes", "general"):
        general = case == "general"
        g.catalog(FAMS, SIZES)
        if general:
            g.pool("several", weight=10, requirements=[(FAMILY_KEY, "Exists", [], 2)], limits={"cpu": 96_000})
        g.pool()
        g.nodes(30, (2, 3, 4), (0.7, 0.97), spread_apps=APPS if general else None)
        g.pending(300, selector_frac=0.10, apps=APPS if general else None)
        g.heavy_pods()
    elif case in ("wide", "wide_spread"):
        g.catalog(FAMS_WIDE, SIZES_WIDE)
        g.pool()
        g.pending(200, selector_frac=0.03, apps=APPS if case == "wide_spread" else None)
        g.heavy_pods(3)
    elif case in ("cluster", "cluster_general"):
        g.catalog(FAMS, SIZES)
        g.pool()
        big = lambda rng: (int(rng.choice([500, 1000, 2000, 3000])), int(rng.choice(MEMS[2:])))  # noqa: E731
        g.nodes(CLUSTER_NODES, (1, 2), (0.9, 1.0), spread_apps=APPS if case == "cluster_general" else None, fill=big,
                light=(CLUSTER_NODES, 4, (0.2, 0.35)))
        g.heavy_nodes(CLUSTER_NODES)
    elif case == ROOMY:
        g.catalog(FAMS, SIZES)
        g.pool()
        req = _only({"cpu": 100, "memory": 128 * MI * 1000, "pods": 1000}, names)
        for _ in range(150):
            g.pod(req, ts=TS0)
        for k in range(30):
            g.pod(dict(req, **({g.extras[k % len(g.extras)]: 1000} if g.extras else {})), ts=TS0 + 1_000_000_000)
    else:
        raise KeyError(case)
    p = g.b.build()
    p.sweep_kept = tuple(g.kept)
    return p


def without(p, resource):
    """p with the requests of `resource` taken off its pending and bound pods
    (set to zero; the pods of sweep_kept keep theirs), everything else shared"""
    q = copy.copy(p)
    q.quantities = p.quantities.copy()
    mine = np.zeros(len(q.quantities), dtype=bool)
    for i, pod in enumerate(p.pods):
        if i not in p.sweep_kept:
            mine[int(pod["requests"]["begin"]):int(pod["requests"]["begin"]) + int(pod["requests"]["count"])] = True
    for pod in p.bound_pods:
        mine[int(pod["requests"]["begin"]):int(pod["requests"]["begin"]) + int(pod["requests"]["count"])] = True
    sid = p.strings.index(resource)
    q.quantities["milli"][mine & (q.quantities["resource"] == sid)] = 0
    q.struct = abi.GsProblem()
    C.memmove(C.byref(q.struct), C.byref(p.struct), C.sizeof(abi.GsProblem))
    q.struct.quantities = q.quantities.ctypes.data
    return q


def _seed(case, R, layout):
    return 0x5EED5000 + 4096 * (CASES + (ROOMY,)).index(case) + 16 * R + LAYOUTS.index(layout)


@functools.lru_cache(maxsize=None)
def problem(case, R, layout, drop=None):
    """the problem of one case at one (R, layout), built once and never modified"""
    if drop is not None:
        return without(problem(case, R, layout), drop)
    return _build(case, resource_names(R, layout), _seed(case, R, layout))


@functools.lru_cache(maxsize=None)
def nine_resources():
    """the plain case with one resource more than the kernels are compiled for"""
    return _build("plain", resource_names(8, "tail") + ["vendor.example/r5"], _seed("plain", 9, "tail"))


@functools.lru_cache(maxsize=None)
def solved(case, R, layout, drop=None):
    """the oracle's Solve -> (status, result dict, (claim_prefix, node_prefix)), computed once"""
    st, want, raw = pyoracle.solve(problem(case, R, layout, drop))
    return st, want, (int(raw.claim_prefix), int(raw.node_prefix)) if st == abi.GS_OK else None


def cluster_input(case, R, layout, mode=abi.CONSOLIDATE_SINGLE):
    p = problem(case, R, layout)
    return ConsolidationInput(p, list(range(len(p.nodes))), mode=mode)


@functools.lru_cache(maxsize=None)
def consolidated(case, R, layout, mode=abi.CONSOLIDATE_SINGLE):
    """the oracle's consolidation -> (status, commands, chosen, multi_options), computed once"""
    return pyoracle.consolidate(cluster_input(case, R, layout, mode))


def single_command(case, R, layout, node, drop=None):
    """the oracle's SingleNode command for one candidate (a simulation does not
    depend on which other nodes are candidates) -> (status, command)"""
    st, cmds, _, _ = pyoracle.consolidate(ConsolidationInput(problem(case, R, layout, drop), [node]))
    return st, cmds[0] if st == abi.GS_OK else None


def assignment(result):
    """pod -> claim and pod -> node of a Solve result, and nothing else"""
    return ([tuple(c["pods"]) for c in result["claims"]], [tuple(x) for x in result["nodes"]], tuple(result["errors"]))


# ------------------------------------------------------- reading a problem back
def names_of(p):
    return sorted({p.strings[int(q["resource"])] for q in p.quantities})


def quantities(p, span):
    o, n = int(span["begin"]), int(span["count"])
    out = {}
    for k in range(o, o + n):
        r = p.strings[int(p.quantities[k]["resource"])]
        out[r] = out.get(r, 0) + int(p.quantities[k]["milli"])
    return out


def pod_requests(p):
    return [quantities(p, pod["requests"]) for pod in p.pods]


def max_allocatable(p):
    """per resource, the largest capacity - overhead over the instance types"""
    top = {}
    for it in p.instance_types:
        cap, ovh = quantities(p, it["capacity"]), quantities(p, it["overhead"])
        for r, c in cap.items():
            top[r] = max(top.get(r, 0), c - ovh.get(r, 0))
    return top


def has_requirements(p, i):
    pod = p.pods[i]
    return any(int(pod[k]["count"]) for k in ("node_selector", "required_terms", "preferred_terms", "spreads"))


def queue_order(p):
    """the Solve queue: cpu desc, memory desc, creation time, uid"""
    rq = pod_requests(p)
    return sorted(range(len(p.pods)), key=lambda i: (-rq[i].get("cpu", 0), -rq[i].get("memory", 0),
                                                     int(p.pods[i]["creation_ns"]), p.strings[int(p.pods[i]["uid"])]))


def hand_overs(p):
    """places in queue order where a pod that asks for an extended resource
    directly follows one that asks for none, has the same cpu and memory and
    carries no requirements: a hint the first sets is applied to the second"""
    rq, order = pod_requests(p), queue_order(p)
    n = 0
    for a, b in zip(order, order[1:]):
        same = all(rq[a].get(r, 0) == rq[b].get(r, 0) for r in ("cpu", "memory"))
        n += same and not has_requirements(p, a) and not set(rq[a]) - set(BASE) and bool(set(rq[b]) - set(BASE))
    return n
