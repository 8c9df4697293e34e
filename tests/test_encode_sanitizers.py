"""The host encoder (csrc/encode.cpp and the units it drives: encode_*.cpp,
reqs.cpp, par.cpp) under AddressSanitizer + UBSan on the CPU.

The encoder parses caller-owned arrays (ranges, string ids, value ids) before
anything reaches the device, so it is built here with
g++ -fsanitize=address,undefined (host only, tools/encode_harness.cpp) and run
over the randomised generators the parity tests use — Solve problems, topology
problems, consolidation clusters with bound pods — plus deliberately corrupted
inputs (out-of-range ranges and ids), which must come back as GS_E_INVALID
instead of reading out of bounds.  Statuses must agree with the product
library's gs_validate (same encoder, compiled by hipcc).

The Create re-filter's host side (csrc/filter_encode.cpp: the reduction of
the caller's requirement lists; csrc/filter_rules.hpp: the rule for one
(claim, instance type) pair that both kernels call) is in the same build:
encode_harness -f reduces a catalog and claims as the entry points do and
evaluates the rule on the CPU.  Its answer must be the oracle's, bit for bit,
and corrupt ranges and ids on either side must come back as GS_E_INVALID.
"""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import resource_sweep
from gpusched import abi, lib, synth
from oracle import pyoracle
from test_create_filter import CT_CASES, GIT_CASES, _git_problem, _kat_problem, random_catalog

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "karpenter-provider-ibm-cloud_amd", "csrc")


# the library's host units that need the HIP runtime (ctx.hpp) or the build's
# digest define; every other csrc/*.cpp is the encoder's and builds with g++
HIP_UNITS = {"batch.cpp", "build_id.cpp", "capi.cpp", "consolidate.cpp", "multi.cpp"}


def _encoder_units():
    """a unit added to csrc joins the harness builds unless it is listed above
    (one that needs HIP and is not fails the compile)"""
    return [os.path.join(CSRC, n) for n in sorted(os.listdir(CSRC)) if n.endswith(".cpp") and n not in HIP_UNITS]


def _build_harness(out, flags):
    if shutil.which("g++") is None:
        pytest.skip("g++ absent")
    cxx = ["g++", "-std=c++17", "-O1"] + flags + ["-pthread"]

    def compile_unit(src):
        obj = out + "." + os.path.basename(src) + ".o"
        r = subprocess.run(cxx + ["-c", "-o", obj, src], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-4000:]
        return obj

    with ThreadPoolExecutor(max_workers=8) as ex:  # one compiler process per unit
        objs = list(ex.map(compile_unit, [os.path.join(ROOT, "tools", "encode_harness.cpp")] + _encoder_units()))
    r = subprocess.run(cxx + ["-o", out] + objs, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build_harness(str(tmp_path_factory.mktemp("asan") / "encode_harness_asan"),
                          ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


@pytest.fixture(scope="module")
def plain_harness(tmp_path_factory):
    return _build_harness(str(tmp_path_factory.mktemp("plain") / "encode_harness"), [])


def _sweep_problems():
    """every resource count 1..8 in both name layouts (tests/resource_sweep.py):
    the plain problem and the general one (nodes, bound pods, spreads, minValues)"""
    return [(f"{case}-{resource_sweep.pair_id(pair)}", resource_sweep.problem(case, *pair))
            for pair in resource_sweep.PAIRS for case in ("plain", "general")]


def _problems():
    out = []
    for s in range(24):
        out.append((f"solve{s}", synth.random_problem(s)))
    for s in range(12):
        out.append((f"topo{s}", synth.random_topology(s)))
    for s in range(8):
        out.append((f"cons{s}", synth.random_consolidation(s)))
    for s in range(10):
        out.append((f"anti{s}", synth.random_affinity(s)))
    for s in range(8):
        out.append((f"minv{s}", synth.random_min_values(s)))
    for s in range(8):
        out.append((f"vol{s}", synth.random_volumes(s)))
    out.append(("c1", synth.make_c1()))
    out.append(("c3_2k", synth.make_c3(n_pods=2000)))
    out.append(("c4_200", synth.make_c4(n_nodes=200, n_pending=5)))
    out += _sweep_problems()
    return out


def _corrupt(kind):
    p = synth.random_problem(3, with_nodes=True)
    if kind == "pod_requests_range":
        p.pods["requests"]["begin"][0] = len(p.quantities) + 5
    elif kind == "req_key_id":
        p.reqs["key"][0] = len(p.strings) + 100
    elif kind == "value_range":
        p.reqs["values"]["count"][len(p.reqs) - 1] = 1 << 30
    elif kind == "it_offerings_range":
        p.instance_types["offerings"]["begin"][0] = len(p.offerings)
        p.instance_types["offerings"]["count"][0] = 3
    elif kind == "node_labels_range":
        if len(p.nodes):
            p.nodes["labels"]["begin"][0] = len(p.labels) + 1
            p.nodes["labels"]["count"][0] = 1
    elif kind == "quantity_resource_id":
        p.quantities["resource"][0] = len(p.strings) + 7
    elif kind == "nodepool_it_refs":
        p.nodepools["instance_types"]["count"][0] = len(p.it_refs) + 1
    elif kind == "anti_affinity_range":
        p.pods["anti_affinity"]["begin"][0] = len(p.affinity_terms) + 2
        p.pods["anti_affinity"]["count"][0] = 1
    elif kind == "host_port_range":
        p.pods["host_ports"]["count"][len(p.pods) - 1] = 1 << 31
    return p


CORRUPT = ["pod_requests_range", "req_key_id", "value_range", "it_offerings_range", "node_labels_range",
           "quantity_resource_id", "nodepool_it_refs", "anti_affinity_range", "host_port_range"]


def _run(harness, dumps):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([harness] + dumps, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return [int(line.split()[0]) for line in r.stdout.strip().split("\n")]


def test_encoder_clean_under_asan_ubsan(harness, tmp_path):
    probs = _problems()
    dumps = []
    for name, p in probs:
        path = str(tmp_path / f"{name}.gspd")
        p.dump(path)
        dumps.append(path)
    got = _run(harness, dumps)
    for (name, p), st in zip(probs, got):
        want, msg = lib.validate(p)
        if want == abi.GS_E_CAPACITY:  # device capacity check runs after encode
            want = abi.GS_OK
        assert st == want, (name, st, want, msg)


def test_encoder_rejects_corrupt_inputs_under_asan(harness, tmp_path):
    dumps = []
    for kind in CORRUPT:
        path = str(tmp_path / f"{kind}.gspd")
        _corrupt(kind).dump(path)
        dumps.append(path)
    got = _run(harness, dumps)
    for kind, st in zip(CORRUPT, got):
        assert st == abi.GS_E_INVALID, (kind, st)


def test_encoding_independent_of_thread_count(plain_harness, tmp_path):
    """the encoder's parallel loops promise the serial encoder's result ("one
    order whatever the split"): status, message and the digest of every
    Encoded array (encode_harness -d) are the same on 1 and on 4 threads"""
    probs = ([synth.random_problem(s) for s in range(3)] + [synth.random_topology(s) for s in range(3)] +
             [synth.random_relax(s) for s in range(2)] + [synth.random_consolidation(s) for s in range(2)] +
             [p for _, p in _sweep_problems()])
    dumps = []
    for i, p in enumerate(probs):
        dumps.append(str(tmp_path / f"p{i}.gspd"))
        p.dump(dumps[-1])
    out = {}
    for threads in (1, 4):
        r = subprocess.run([plain_harness, "-d"] + dumps, capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, GS_ENCODE_THREADS=str(threads)))
        assert r.returncode == 0, r.stderr[-4000:]
        lines = r.stdout.strip().split("\n")
        # "<status> <ms> <path>": the time is the one field that may differ
        out[threads] = [" ".join(ln.split()[::2]) if ln.endswith(".gspd") else ln for ln in lines]
    assert len(out[1]) > 50 * len(dumps) and sum(ln.endswith(".gspd") for ln in out[1]) == len(dumps)
    assert out[1] == out[4]


def test_dump_roundtrip_status_matches_validate(tmp_path):
    """the dump carries the whole problem: a plain (unsanitised) harness
    build gives the library's statuses too"""
    p = synth.random_problem(5)
    path = str(tmp_path / "p.gspd")
    p.dump(path)
    with open(path, "rb") as f:
        assert f.read(4) == b"GSPD"
    assert os.path.getsize(path) > np.asarray(p.pods).nbytes


# ------------------------------------------------------ the Create re-filter
def _bits(words):
    """'3,0,80' (hex u64 words) -> the set bit indices"""
    if words == "-":
        return []
    return [64 * w + i for w, x in enumerate(words.split(",")) for i in range(64) if (int(x, 16) >> i) & 1]


def _run_filter(harness, pairs):
    """encode_harness -f over (catalog dump, claims dump) pairs -> per pair
    (status, rows in pyoracle.create_filter's form); a disagreement between
    the per-call and the prepared form is a non-zero exit"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([harness, "-f"] + [x for pair in pairs for x in pair], capture_output=True, text=True,
                       timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    out = []
    for line in r.stdout.strip().split("\n"):
        f = line.split()
        if line.endswith(".gspd"):
            out.append((int(f[0]), []))
        elif f[0] != "msg":
            n, sel, ct, create, reqs = f
            out[-1][1].append(dict(compatible=_bits(create), requirements=_bits(reqs), n_compatible=int(n),
                                   selected=int(sel), capacity_type=int(ct)))
    assert len(out) == len(pairs)
    return out


def test_create_filter_reducer_matches_oracle_under_asan(harness, tmp_path):
    """the reducer and pair_verdict against the oracle, in the prepared form
    and (same file on both sides) in the per-call form too"""
    probs = [(f"cat{s}", random_catalog(s, 150, 40)) for s in range(6)]
    probs += [(f"ct{i}", _kat_problem(c)) for i, c in enumerate(CT_CASES)]
    probs += [(f"git{i}", _git_problem(c)) for i, c in enumerate(GIT_CASES)]
    pairs, want = [], []
    for name, p in probs:
        path = str(tmp_path / f"{name}.gspd")
        p.dump(path)
        pairs.append((path, path))
        want.append(pyoracle.create_filter(p))
    # the claims in a pool of their own (other string ids) against the first catalog
    pool = str(tmp_path / "pool.gspd")
    probs[0][1].claims_pool().dump(pool)
    pairs.append((pairs[0][0], pool))
    want.append(want[0])
    # the inputs are not trivial: some claim keeps no type, some claim keeps several
    kept = [q["n_compatible"] for st, rows in want[:6] for q in rows]
    assert 0 in kept and max(kept) > 1
    got = _run_filter(harness, pairs)
    for (cat, claims), (st, rows), (wst, wrows) in zip(pairs, got, want):
        assert wst == abi.GS_OK and st == wst, (cat, claims, st)
        assert rows == wrows, (cat, claims)


def _corrupt_filter(kind):
    p = random_catalog(3, 30, 8)
    it0 = p.instance_types[0]
    if kind == "req_key_id":
        p.reqs["key"][it0["requirements"]["begin"]] = len(p.strings) + 100
    elif kind == "value_range":
        p.reqs["values"]["count"][it0["requirements"]["begin"]] = 1 << 30
    elif kind == "quantity_resource_id":
        p.quantities["resource"][it0["capacity"]["begin"]] = len(p.strings) + 7
    elif kind == "it_offerings_range":
        p.instance_types["offerings"]["begin"][0] = len(p.offerings)
        p.instance_types["offerings"]["count"][0] = 3
    elif kind == "claim_reqs_range":
        p.claim_queries[0].requirements.count = len(p.reqs) + 1
    elif kind == "claim_requests_range":
        p.claim_queries[0].requests.begin = len(p.quantities) + 2
        p.claim_queries[0].requests.count = 1
    elif kind == "claim_gt_not_integer":
        p = p.extended(lambda b: b.add_claim_query([("karpenter-ibm.sh/instance-cpu", "Gt", ["x"])]))
    return p


CORRUPT_FILTER = ["req_key_id", "value_range", "quantity_resource_id", "it_offerings_range", "claim_reqs_range",
                  "claim_requests_range", "claim_gt_not_integer"]


def test_create_filter_reducer_rejects_corrupt_inputs_under_asan(harness, tmp_path):
    pairs = []
    for kind in CORRUPT_FILTER:
        path = str(tmp_path / f"{kind}.gspd")
        _corrupt_filter(kind).dump(path)
        pairs.append((path, path))
    # the claims' side alone, against a sound catalog
    sound = str(tmp_path / "sound.gspd")
    random_catalog(3, 30, 8).dump(sound)
    pairs += [(sound, path) for (path, _), kind in zip(pairs, CORRUPT_FILTER) if kind.startswith("claim_")]
    got = _run_filter(harness, pairs)
    assert got[-1][0] == abi.GS_E_INVALID and len(got) == len(CORRUPT_FILTER) + 3
    for (cat, claims), (st, rows) in zip(pairs, got):
        assert st == abi.GS_E_INVALID and not rows, (cat, claims, st)
