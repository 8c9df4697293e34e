"""csrc/qcode.hpp: the branch-free 16-bit code arithmetic.

tests/qcode_check.cpp is a stand-alone program: it includes the header the
kernels include and carries the early-return definitions the header replaced.
Built with g++ -O1 -fsanitize=undefined,address and run here, it checks
qcode_value over all 65,536 codes and qcode_floor / qcode_ceil over every v in
[-4096, 4096], 2^k - 1, 2^k, 2^k + 1 (k = 1..62) and their negatives,
INT64_MIN, INT64_MAX and 10^6 seeded random 63-bit values: equality with the
replaced definitions (qcode_value: where they are defined, codes below 33,280;
above, the header's own rule, the shift count modulo 64), qcode_value(qcode_floor(v)) <= v <=
qcode_value(qcode_ceil(v)) for v > 0, every code within 16 bits, and (the
sanitizer) no shift count outside 0..63 on any input.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "karpenter-provider-ibm-cloud_amd", "csrc")


def test_qcode_header_matches_replaced_definitions(tmp_path):
    exe = str(tmp_path / "qcode_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined",
                        "-Wall", "-Werror", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "qcode_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    # 65,536 codes + 8,193 + 372 + 2 + 2 x 10^6 values
    assert r.stdout.split() == ["ok", str(65536 + 8193 + 62 * 6 + 2 + 2_000_000)], r.stdout
