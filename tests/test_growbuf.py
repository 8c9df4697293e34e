"""GrowBuf (csrc/growbuf.hpp), the owner of every grow-only device buffer and
pinned mirror of the library, under AddressSanitizer + UBSan on the CPU.

tools/growbuf_harness.cpp is a stand-alone program (its own main) that includes
only that header.  Its memory policy is malloc-backed, records every call ('a'
an allocation, 'x' an allocation told to throw, 'f' a free) and can be told to
fail, so the order of calls is asserted here and a double free, a leak or a
read of a freed block ends in a sanitizer report and a non-zero exit.  The
program is built with g++ -fsanitize=address,undefined and run directly:
nothing is preloaded.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "growbuf_harness.cpp")
HEADER = os.path.join(ROOT, "karpenter-provider-ibm-cloud_amd", "csrc", "growbuf.hpp")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ absent")
    out = str(tmp_path_factory.mktemp("growbuf") / "growbuf_harness")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-o", out, SRC],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def _run(harness, case):
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([harness, case], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (case, r.stdout, r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (case, r.stderr[-4000:])
    return r.stdout


def _facts(harness, case):
    return dict(kv.split("=") for kv in _run(harness, case).split())


def test_header_is_host_only():
    """standard headers only: no HIP include and no other header of the library"""
    txt = open(HEADER).read()
    includes = [ln.split()[1] for ln in txt.splitlines() if ln.startswith("#include")]
    assert sorted(includes) == ["<cstddef>", "<cstring>"], includes


def test_reserve_grows_with_headroom(harness):
    """within capacity no call; growth frees once, then allocates bytes + bytes / 4"""
    got = _facts(harness, "reserve")
    assert got == {"within": "a", "cap1": "125", "cap2": "157", "events": "afaf", "sizes": "125,157"}, got


def test_reserve_exact_has_no_headroom(harness):
    got = _facts(harness, "reserve_exact")
    assert got == {"within": "a", "cap1": "100", "cap2": "101", "events": "afaf", "sizes": "100,101"}, got


def test_zero_bytes_on_an_empty_buffer_makes_no_call(harness):
    assert _facts(harness, "zero") == {"events": "-", "null": "1", "cap": "0"}


def test_failed_allocation_leaves_an_empty_buffer(harness):
    """the old block is freed exactly once (before the allocation), and a later reserve succeeds"""
    got = _facts(harness, "alloc_throws")
    assert got == {"caught": "1", "null": "1", "cap": "0", "later": "12", "events": "afxaf"}, got


def test_reserve_keep(harness):
    """keeps the prefix, allocates before it frees, and a failed allocation leaves the old block intact"""
    got = _facts(harness, "keep")
    assert got == {"kept": "1", "cap2": "250", "grown": "aaf", "caught": "1", "same": "1", "cap3": "250",
                   "intact": "1", "events": "aafxf", "sizes": "80,250"}, got


def test_moves_leave_the_source_empty(harness):
    """move-assignment frees the destination's former block once; nothing is freed twice at scope exit"""
    got = _facts(harness, "move")
    assert got == {"assigned": "aaf", "constructed": "aaf", "a_empty": "1", "b_took": "1", "b_empty": "1",
                   "c_took": "1", "events": "aaff"}, got


def test_free_errors(harness):
    """reserve reports a failed free and still owns the block; the destructor and move-assignment swallow one"""
    got = _facts(harness, "free_throws")
    # reserve_exact(10), the failed free, then free + allocate, a and b, the move's free, three destructors
    assert got == {"survived": "1", "caught": "1", "owned": "1", "events": "af" + "fa" + "aa" + "f" + "ff"}, got


def test_up256(harness):
    assert _run(harness, "up256").split() == ["0", "256", "256", "256", "512"]
