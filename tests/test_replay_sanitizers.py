"""The pure-host part of CLIP DECODE (rtldavis_amd/csrc/rd_host.cpp: rd_cd_check_jobs) in a stand-alone program,
tests/replay_asan.cpp, built with -fsanitize=address,undefined and run here on the CPU as a child process: every rule at
its limit on either side, the largest list, and random lists against the restatement of tests/clip_replay_cases.py.  The
library compiles the same rd_host.cpp (csrc/Makefile)."""
import os
import subprocess

import numpy as np
import pytest

import clip_replay_cases as RC
from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "_build")
EXE = os.path.join(BUILD, "replay_asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "replay_asan.cpp"), os.path.join(ROOT, "rtldavis_amd", "csrc", "rd_host.cpp")]
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


def test_every_rule_at_its_limits_under_sanitizers(exe):
    out = run(exe, "limits")
    assert "limits ok" in out
    w = out.replace(",", "").split()
    assert int(w[2]) >= 15 and int(w[4]) >= 30, out


def test_random_lists_equal_the_restatement(exe, tmp_path):
    rng = np.random.default_rng(21)
    edge = {"offset": (4, 2 ** 63, 2 ** 64 - 8, 50000), "n": (0, 2 ** 32 - 1, 50001), "tau_lo": (-2 ** 31, -2 ** 30 - 1, 2 ** 30),
            "tau_hi": (2 ** 31 - 1, 2 ** 30 + 1, -2 ** 30), "id": (8, 0xFF, 2 ** 32 - 1), "corr_re": (-32769, 32768, -32768),
            "corr_im": (32768, 32767), "pad": (1,)}
    want, blob = [], b""
    for _ in range(300):
        k = int(rng.integers(1, 9))
        pool = int(rng.integers(1, 60000))
        jobs = RC.jobs_of([RC.job_row(8 * int(rng.integers(0, 4000)), int(rng.integers(1, 3000)), lo, lo + int(rng.integers(0, 2060)))
                           for lo in rng.integers(-3000, 3000, k)])
        if rng.integers(0, 2):
            f = list(edge)[int(rng.integers(0, len(edge)))]
            jobs[int(rng.integers(0, k))][f] = edge[f][int(rng.integers(0, len(edge[f])))]
        want.append(list(RC.check_jobs(jobs, pool)))
        blob += np.asarray([k, pool], np.int64).tobytes() + jobs.tobytes()
    fin, fout = tmp_path / "lists.bin", tmp_path / "answers.bin"
    fin.write_bytes(blob)
    assert f"file ok: {len(want)} lists" in run(exe, "file", fin, fout)
    assert np.fromfile(fout, np.int32).reshape(-1, 2).tolist() == want
    assert sum(w[0] == 0 for w in want) >= 30 and sum(w[0] != 0 for w in want) >= 100
