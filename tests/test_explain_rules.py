"""gs_explain's one rule (csrc/explain_rules.hpp) under AddressSanitizer +
UBSan on the CPU.

tools/explain_rules_harness.cpp is a stand-alone program (its own main) that
includes only that header; it prints the cause code for all 128 combinations
of the seven booleans times the 32 pre-check states.  It is built with
g++ -fsanitize=address,undefined and run directly: nothing is preloaded.  The
output is compared with the table of include/gpusched.h written out here.
"""
import os
import shutil
import subprocess

import pytest

from gpusched import abi, explain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "explain_rules_harness.cpp")
HEADER = os.path.join(ROOT, "karpenter-provider-ibm-cloud_amd", "csrc", "explain_rules.hpp")

R, F, O, RF_ONLY, RO_ONLY, FO_ONLY, ALL = (1 << i for i in range(7))
NO_OPTIONS, LIMITS, TAINTS, INCOMPATIBLE, MIN_VALUES = (1 << i for i in range(5))

# (condition on (met, pre), code): the issue's table, top to bottom
TABLE = [
    (lambda m, p: p & NO_OPTIONS, abi.GS_WHY_NO_OPTIONS),
    (lambda m, p: p & LIMITS, abi.GS_WHY_LIMITS),
    (lambda m, p: p & TAINTS, abi.GS_WHY_TAINTS),
    (lambda m, p: p & INCOMPATIBLE, abi.GS_WHY_INCOMPATIBLE),
    (lambda m, p: m & ALL and p & MIN_VALUES, abi.GS_WHY_MIN_VALUES),
    (lambda m, p: m & ALL, abi.GS_WHY_STATE),
    (lambda m, p: not m & R and not m & F and not m & O, abi.GS_WHY_IT_NONE),
    (lambda m, p: not m & R and not m & F, abi.GS_WHY_IT_REQ_OR_FITS),
    (lambda m, p: not m & R and not m & O, abi.GS_WHY_IT_REQ_OR_OFFERING),
    (lambda m, p: not m & F and not m & O, abi.GS_WHY_IT_FITS_OR_OFFERING),
    (lambda m, p: not m & R, abi.GS_WHY_IT_REQUIREMENTS),
    (lambda m, p: not m & F, abi.GS_WHY_IT_RESOURCES),
    (lambda m, p: not m & O, abi.GS_WHY_IT_OFFERING),
    (lambda m, p: m & RF_ONLY, abi.GS_WHY_IT_REQ_FITS_NO_OFFERING),
    (lambda m, p: m & FO_ONLY, abi.GS_WHY_IT_FITS_OFFERING_NO_REQ),
    (lambda m, p: m & RO_ONLY, abi.GS_WHY_IT_REQ_OFFERING_NO_FITS),
    (lambda m, p: True, abi.GS_WHY_IT_TUPLE),
]


def table_cause(met, pre):
    for cond, code in TABLE:
        if cond(met, pre):
            return code
    raise AssertionError


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ absent")
    out = str(tmp_path_factory.mktemp("explain_rules") / "explain_rules_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-o", out, SRC],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([out], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]


def test_header_is_host_only():
    """no HIP include and no other header of the library"""
    txt = open(HEADER).read()
    includes = [ln.split()[1] for ln in txt.splitlines() if ln.startswith("#include")]
    assert includes == ["<stdint.h>"], includes


def test_every_combination_matches_the_table(lines):
    assert len(lines) == 128 * 32
    assert [(m, p) for m, p, *_ in lines] == [(m, p) for m in range(128) for p in range(32)]
    seen = set()
    for met, pre, cause, reported, roundtrip in lines:
        assert cause == table_cause(met, pre), (met, pre, cause)
        early = pre & (NO_OPTIONS | LIMITS | TAINTS | INCOMPATIBLE)
        assert reported == (0 if early else met), (met, pre, reported)
        assert roundtrip == 1, (met, pre)
        seen.add(cause)
    assert seen == set(range(abi.GS_WHY_COUNT))


def test_python_rule_is_the_same(lines):
    """gpusched.explain.cause_of (what the reference model of
    tests/test_explain.py calls) agrees with the header on every line"""
    for met, pre, cause, _, _ in lines:
        assert explain.cause_of(met, pre) == cause, (met, pre)
    assert len(explain.CAUSE_NAMES) == abi.GS_WHY_COUNT and set(explain.CAUSE_TEXT) == set(range(abi.GS_WHY_COUNT))
