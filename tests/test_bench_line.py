"""bench.py's stdout contract (CPU): the last line is a compact headline the
driver can parse from its 8 KB stdout tail (a 24 KB line was not
parsed), carrying the contract keys, `roofline` and `cpu_baseline`."""
import copy
import io
import json
import os
import sys
from contextlib import redirect_stdout

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

R3_LINE = os.path.join(ROOT, "profiles", "r3", "bench_v3.json")


def _full_line():
    with open(R3_LINE) as f:
        line = json.load(f)
    # the round-4 bench adds the unique-byte view beside the §8(d) roofline
    line["roofline_unique_bytes"] = copy.deepcopy(line["roofline"])
    return line


def test_headline_fits_and_has_contract_keys():
    line = _full_line()
    assert len(json.dumps(line)) > 20000  # the round-3 record the driver could not parse
    h = bench.headline(line)
    s = json.dumps(h)
    assert len(s) <= bench.HEADLINE_MAX_BYTES
    for k in bench.HEADLINE_KEYS:
        assert k in h, k
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in h["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in h["cpu_baseline"], k
    assert h["value"] > 0 and h["ms_per_step"] > 0
    assert "legs" in h and "C5_SOLVE" in h["legs"] and "c4_e2e" in h["legs"]


def test_headline_sheds_detail_never_contract_keys():
    line = _full_line()
    line["config"]["workload"] = "x" * 3000
    for i in range(200):  # a bench with many more legs
        line.setdefault("configs", {})[f"EXTRA{i}"] = line["configs"]["C3"]
    h = bench.headline(line)
    assert len(json.dumps(h)) <= bench.HEADLINE_MAX_BYTES
    for k in bench.HEADLINE_KEYS:
        assert k in h, k


def test_emit_last_stdout_line_is_the_headline(tmp_path):
    line = _full_line()
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.emit(line, str(tmp_path / "detail.json"), 0)
    out = buf.getvalue().splitlines()
    last = json.loads(out[-1])
    assert len(out[-1].encode()) <= bench.HEADLINE_MAX_BYTES
    assert last["metric"] == bench.METRIC and last["roofline"] and last["cpu_baseline"]
    assert all(x.startswith("# leg ") for x in out[:-1])
    with open(tmp_path / "detail.json") as f:
        detail = json.load(f)
    assert detail["configs"]["C3"] == line["configs"]["C3"]
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert bench.emit(_full_line(), None, 1) is None
    assert buf.getvalue() == ""


# ---------------------------------------------- N > 1: the strong-scaling legs
def _scaling_worker(rank, world, port, q):
    """one gloo rank: bench's max-over-ranks reduction and the section builder"""
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)

    def max_over_ranks(x):
        t = torch.tensor([x], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    per_rank = {
        "c5_static_matrix_it_columns": {"ms_per_step": 0.2, "kernel_ms": 0.05 + 0.01 * rank,
                                        "combine_ms": 0.03 * (rank + 1), "words_per_rank": 32 // world,
                                        "checks_per_s": 1e12, "shards_equal_whole": True},
        "c4_candidates": {"ms_per_sweep": 1.0, "sim_kernel_ms": 0.3 - 0.1 * rank, "gather_choose_ms": 0.2 + rank,
                          "simulations": 5000, "simulations_per_s": 5e6},
    }
    sec = bench.strong_scaling_section(per_rank, dist.get_world_size(), dist.get_backend(), max_over_ranks)
    q.put((rank, sec))
    dist.destroy_process_group()


def test_strong_scaling_section_gloo_world2():
    import socket
    import torch.multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_scaling_worker, args=(r, world, port, q)) for r in range(world)]
    for p_ in procs:
        p_.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p_ in procs:
        p_.join(timeout=60)
        assert p_.exitcode == 0
    sec = res[0]
    assert res[1] == sec  # every rank holds the same reduced section
    assert sec["ranks"] == 2 and sec["backend"] == "gloo" and sec["scaling"] == "strong"
    c5 = sec["c5_static_matrix_it_columns"]
    assert c5["kernel_ms"] == 0.06 and c5["combine_ms"] == 0.06 and c5["words_per_rank"] == 16
    c4 = sec["c4_candidates"]
    assert c4["sim_kernel_ms"] == 0.3 and c4["gather_choose_ms"] == 1.2 and c4["simulations"] == 5000
    # the headline carries it, within the driver's size budget
    line = _full_line()
    line["n_gpus"] = 2
    line["strong_scaling"] = sec
    h = bench.headline(line)
    assert h["strong_scaling"] == sec and len(json.dumps(h)) <= bench.HEADLINE_MAX_BYTES


# ------------------------------------------- the plain run, --full, --dump-outputs
def test_plain_run_is_the_cm_leg_alone_and_full_keeps_every_leg():
    plain = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert plain.steps == 7 and plain.warmup == 3 and not plain.full
    assert plain.only == "cm" and plain.latency_steps == 0 and plain.detail_json is None
    assert bench.parse_args(["--only", "cm"]).only == "cm"
    full = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3", "--full"])
    assert full.only is None and full.latency_steps == 3 and not full.no_cpu_baseline
    assert full.detail_json.endswith(os.path.join("bench_out", "bench_detail.json"))
    assert bench.parse_args(["--full", "--only", "c4", "--detail-json", "x.json"]).detail_json == "x.json"
    for bad in (["--only", "c4"], ["--steps", "0"], ["--warmup", "-1"]):
        try:
            bench.parse_args(bad)
        except SystemExit as e:
            assert e.code == 2
        else:
            raise AssertionError(bad)


_RESULT = {
    "claims": [
        {"nodepool": 0, "pods": [4, 0, 2], "its": [7, 1], "requirements": "zone|In|a,b|-|-|0\nk|Exists||3|-|0",
         "requests": {"cpu": 2500, "memory": (1 << 52) + 1}},
        {"nodepool": 1, "pods": [3], "its": [5], "requirements": "", "requests": {"cpu": 100, "pods": 1}},
    ],
    "nodes": [[], [1, 5]],
    "errors": [6],
}


def test_dump_outputs_writes_the_result_exactly(tmp_path):
    import numpy as np
    d = tmp_path / "out" / "run0"
    bench.dump_outputs(str(d), _RESULT)
    got = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_MAX_BYTES
    lists = lambda off, flat: [[int(v) for v in flat[int(a):int(b)]] for a, b in zip(off[:-1], off[1:])]  # noqa: E731
    assert lists(got["claim_pod_offsets"], got["claim_pods"]) == [c["pods"] for c in _RESULT["claims"]]
    assert lists(got["claim_it_offsets"], got["claim_its"]) == [c["its"] for c in _RESULT["claims"]]
    assert lists(got["node_pod_offsets"], got["node_pods"]) == _RESULT["nodes"]
    assert got["claim_nodepool"].tolist() == [0, 1] and got["error_pods"].tolist() == [6]
    # columns: cpu, memory, pods (sorted names); int64 quantities survive float64
    assert got["claim_requests"].astype(np.int64).tolist() == [[2500, (1 << 52) + 1, 0], [100, 0, 1]]
    text = bytes(got["claim_requirements_utf8"].astype(np.uint8)).decode()
    assert text.split("\0") == [c["requirements"] for c in _RESULT["claims"]]
    # no file is empty: a list the caller receives empty is left out, its offsets stay
    assert all(a.size for a in got.values())
    no_nodes = dict(_RESULT, nodes=[], errors=[])
    bench.dump_outputs(str(tmp_path / "no_nodes"), no_nodes)
    assert sorted(set(os.listdir(d)) - set(os.listdir(tmp_path / "no_nodes"))) == ["error_pods.npy", "node_pods.npy"]
    assert np.load(tmp_path / "no_nodes" / "node_pod_offsets.npy").tolist() == [0.0]


@pytest.mark.gpu
def test_gpu_plain_run_times_its_steps_and_dumps_the_last_result(tmp_path):
    """bench.py as a process: a plain run reports the steps it was asked for
    and nothing beside the headline leg; --dump-outputs holds the Solve result
    of the same seeded problem, identical from run to run"""
    import subprocess
    import numpy as np
    from gpusched import synth
    from gpusched.lib import Solver
    pods = 3000
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--pods", str(pods), "--dump-outputs", str(tmp_path / "dump")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.strip().splitlines()
    assert len(out) == 1  # no leg lines
    h = json.loads(out[0])
    assert h["metric"] == bench.METRIC and h["unit"] == "checks/s" and h["higher_is_better"] is True
    assert h["dtype"] == "int64" and h["steps"] == 3 and h["warmup"] == 1 and h["ms_per_step"] > 0
    assert h["config"]["pods"] == pods
    assert abs(h["value"] - h["config"]["checks_per_step"] / (h["ms_per_step"] * 1e-3)) <= 1e-5 * h["value"]
    assert h["cpu_baseline"] is None and h["solve_latency_ms"] is None and "legs" not in h and "detail_file" not in h
    s = Solver(0)
    try:
        want, _ = s.solve(synth.make_cm(n_pods=pods, seed=0x5EED0006))
    finally:
        s.close()
    want = {k: a for k, a in bench.result_arrays_f64(want).items() if a.size}
    assert "node_pods" not in want  # CM has no existing nodes
    got = {f[:-4]: np.load(tmp_path / "dump" / f) for f in os.listdir(tmp_path / "dump")}
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == np.float64 and np.array_equal(got[k], want[k]), k
    assert len(want["claim_pods"]) + len(want["error_pods"]) == pods
