"""The pure-host part of BURST CLIPS (rtldavis_amd/csrc/rd_host.h and rd_host.cpp: the clamp of a request to the two chunks
and to whole 16-byte vectors) in a stand-alone program, tests/clip_asan.cpp, built with -fsanitize=address,undefined and
run here on the CPU as a child process: the clamp against a naive enumeration over random (block_size, have_prev, a, e),
and the library's clamp against the model's on the crafted launches' own requests.  The library compiles the same
rd_host.cpp (csrc/Makefile); the kernel evaluates the same inline function."""
import os
import subprocess

import numpy as np
import pytest

import burst_clip_cases as CC
from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "_build")
EXE = os.path.join(BUILD, "clip_asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "clip_asan.cpp"), os.path.join(ROOT, "rtldavis_amd", "csrc", "rd_host.cpp")]
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


def test_clamp_against_a_naive_enumeration_under_sanitizers(exe):
    for seed in (1, 2):
        out = run(exe, "naive", seed, 4000)
        assert "naive ok" in out
        w = out.replace(",", "").split()
        clips, cut_start, cut_end, from_prev, none, far = (int(w[i]) for i in (2, 4, 6, 8, 10, 12))
        assert clips > 1500 and cut_start > 200 and cut_end > 200 and from_prev > 200 and none > 500 and far > 800, out


def test_library_clamp_equals_the_models(exe, tmp_path):
    """Every request of the crafted launches, with and without a chunk before, and each moved by every offset 0 .. 7."""
    cases, want = [], []
    for X in CC.crafted_launches():
        for c in range(X.n_ch):
            for _, a, e, _ in CC.requests(c, X.sl, X.n_sym, X.bs, X.prev is not None, X.sources, X.pre, X.post,
                                          None if X.owed_prev is None else X.owed_prev[c], X.runs[c, : int(X.n_runs[c])],
                                          X.msgs[c, : int(X.n_msgs[c])], [], []):
                for have_prev in (0, 1):
                    for d in range(8):
                        cases.append([X.bs, have_prev, a + d, e - d])
                        got = CC.clamp(X.bs, bool(have_prev), a + d, e - d)
                        want.append([0] * 4 if got is None else [1] + list(got))
    for bs, have_prev, a, e in ((128, 0, -50, 0), (128, 0, 128, 300), (128, 1, -300, -128), (128, 1, 5, 5), (128, 1, 9, 3)):
        assert CC.clamp(bs, bool(have_prev), a, e) is None       # wholly outside the two chunks, or empty
        cases.append([bs, have_prev, a, e])
        want.append([0] * 4)
    fin, fout = tmp_path / "cases.bin", tmp_path / "clamped.bin"
    np.asarray(cases, np.int64).tofile(fin)
    assert f"file ok: {len(cases)} cases" in run(exe, "file", fin, fout)
    res = np.fromfile(fout, np.int32).reshape(-1, 4)
    assert res.tolist() == want
    assert sum(w[0] for w in want) > 500 and sum(1 - w[0] for w in want) >= 4
