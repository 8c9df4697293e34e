"""The launch rules of csrc/layout.hpp (which Solve kernel variant a problem
runs, wide option rows, the dynamic LDS a launch requests) against values
worked out by hand for one small shape.

tools/launch_rules_harness.cpp is a stand-alone host program (g++, no HIP).
The shape: 10 NodeClaims (7 in the single-wave Solve), 5 thresholds, 3 node
bitmap words, 4 existing nodes, 2 zone groups with a stride of 3, 1 hostname
group, a 16-slot overlay hash.

  topology   (2*8 + 64*8 + 2*3*4 + 1*4 -> 556, up to 8) = 560; with 65 lazy
             groups + 2*8 (created bits) + (65*4 -> 260, up to 8) 264 = 840
  block      (23*10 -> 230, up to 8) 232 + (5+4)*8 + 3*4 = 316, up to 8 = 320;
             + 560 = 880
  simulation 880 + 8*16 = 1008; with the queue in LDS + 32*10 = 1328
  wave       (23*7 -> 161, up to 8) 168 + 72 = 240; + 560 + (8 + 4*17) = 876
  wave, HBM  0 + 72 + 560 + 76 = 708
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "launch_rules_harness.cpp")


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ absent")
    out = str(tmp_path_factory.mktemp("launch_rules") / "launch_rules_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", out, SRC],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr[-4000:])
    return dict(kv.split("=") for kv in r.stdout.split())


def test_general_variant_each_cause_alone(rules):
    """TG, any_mv and any_vol each select the general variant; on DevProblem and on Encoded alike"""
    assert {k: rules[k] for k in ("none", "tg", "mv", "vol")} == {"none": "00", "tg": "11", "mv": "11", "vol": "11"}


def test_wide_rows_boundary(rules):
    assert (rules["wide4"], rules["wide5"]) == ("0", "1")


def test_dynamic_lds_sizes(rules):
    want = {"topo": 560, "topo_enc": 560, "topo_lazy": 840, "block": 880, "block_plain": 320, "sim": 1008,
            "sim_queue": 1328, "sim_args": 1008, "sim_args_queue": 1328, "wave": 876, "wave_ch": 708}
    assert {k: int(rules[k]) for k in want} == want
