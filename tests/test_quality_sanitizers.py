"""The pure-host part of BURST QUALITY (rtldavis_amd/csrc/rd_host.h and rd_host.cpp: the three windows of a record and
the clipping that gives n_noise) in a stand-alone program, tests/quality_asan.cpp, built with
-fsanitize=address,undefined and run here on the CPU as a child process: the windows against a naive enumeration over
random (SL, N, block_size, have_prev, tau, gap), and the library's windows against the model's on the crafted launches'
own records.  The library compiles the same rd_host.cpp (csrc/Makefile); the kernel evaluates the same inline function."""
import os
import subprocess

import numpy as np
import pytest

import burst_quality_cases as QC
from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "_build")
EXE = os.path.join(BUILD, "quality_asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "quality_asan.cpp"), os.path.join(ROOT, "rtldavis_amd", "csrc", "rd_host.cpp")]
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


def test_windows_against_a_naive_enumeration_under_sanitizers(exe):
    for seed in (1, 2):
        out = run(exe, "naive", seed, 4000)
        assert "naive ok" in out
        w = out.replace(",", "").split()
        measurable, cut, empty, far = int(w[2]), int(w[4]), int(w[6]), int(w[8])
        assert measurable > 500 and cut > 50 and empty > 50 and far > 300, out


def test_library_windows_equal_the_models(exe, tmp_path):
    """Every record of the crafted launches - the unmeasurable ones included - under its launch's gap and under the largest."""
    cases, want = [], []
    for X in QC.crafted_launches():
        sl, n, bs = int(X.cfg.symbol_length), int(X.cfg.packet_symbols), int(X.cfg.block_size)
        for c in range(X.n_ch):
            for m in X.msgs[c, : int(X.n_msgs[c])]:
                for gap in (X.gap, QC.MAX_GAP):
                    cases.append([sl, n, bs, int(X.prev is not None), int(m["tau"]), gap])
                    got = QC.windows(sl, n, bs, X.prev is not None, int(m["tau"]), gap)
                    want.append([0] * 6 if got is None else [1] + list(got))
    fin, fout = tmp_path / "cases.bin", tmp_path / "windows.bin"
    np.asarray(cases, np.int64).tofile(fin)
    assert f"file ok: {len(cases)} cases" in run(exe, "file", fin, fout)
    res = np.fromfile(fout, np.int32).reshape(-1, 6)
    assert res.tolist() == want
    assert sum(w[0] for w in want) > 50 and sum(1 - w[0] for w in want) >= 4
