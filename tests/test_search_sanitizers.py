"""The pure-host parts of BURST SEARCH (rtldavis_amd/csrc/rd_host.cpp: the list's rules, the candidate range of step 2s,
step 7s) in a stand-alone program, tests/search_asan.cpp, built with -fsanitize=address,undefined and run here on the
CPU: the list's limits on either side with every list in a heap block of its own size, the range against a naive
enumeration over a grid of shapes, and step 7s at every offset around SL with the 64-bit clock near its wrap.  The
library compiles the same rd_host.cpp (csrc/Makefile)."""
import os
import subprocess

import pytest

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "_build")
EXE = os.path.join(BUILD, "search_asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "search_asan.cpp"), os.path.join(ROOT, "rtldavis_amd", "csrc", "rd_host.cpp")]
    deps = srcs + [os.path.join(ROOT, "rtldavis_amd", "csrc", "rd_host.h"), os.path.join(ROOT, "include", "rtldavis_hip.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-Wall", "-Wextra", "-o", EXE] + srcs)
    return EXE


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{args}: rc {r.returncode}\n{r.stdout}\n{r.stderr[-3000:]}"
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout


def test_centre_list_rules_under_sanitizers(exe):
    assert "centres ok" in run(exe, "centres")


def test_candidate_range_against_a_naive_enumeration_under_sanitizers(exe):
    out = run(exe, "range")
    assert "range ok" in out
    assert int(out.split()[2]) > 100 and int(out.split()[5]) > 10, out   # chunks with candidates and chunks too short for any


def test_step_7s_under_sanitizers(exe):
    assert "repeats ok" in run(exe, "repeats")
