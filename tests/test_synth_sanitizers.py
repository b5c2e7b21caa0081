"""The pure-host part of CLIP SYNTH (rtldavis_amd/csrc/rd_host.cpp: rd_cs_check_specs, rd_cs_table) in a stand-alone
program, tests/synth_asan.cpp, built with -fsanitize=address,undefined and run here on the CPU as a child process: every
rule at its limit on either side, the largest list, the table into a buffer of exactly its size, and random lists
against the restatement of tests/clip_synth_cases.py.  The library compiles the same rd_host.cpp (csrc/Makefile)."""
import os
import subprocess

import numpy as np
import pytest

import clip_synth_cases as SC
from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "_build")
EXE = os.path.join(BUILD, "synth_asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "synth_asan.cpp"), os.path.join(ROOT, "rtldavis_amd", "csrc", "rd_host.cpp")]
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
    assert int(w[2]) >= 25 and int(w[4]) >= 30, out


def test_table_into_a_buffer_of_its_size(exe, tmp_path):
    assert "table ok" in run(exe, "table", tmp_path / "table.bin")
    assert np.array_equal(np.fromfile(tmp_path / "table.bin", np.int16).astype(np.int64), SC.TABLE)


def test_random_lists_equal_the_restatement(exe, tmp_path):
    rng = np.random.default_rng(5400)
    edge = {"offset": (4, 2 ** 63, 2 ** 64 - 8, 50000), "n": (0, 2 ** 32 - 1, 2 ** 24, 2 ** 24 + 1), "at": (-2 ** 31, -2 ** 30 - 1, 2 ** 30),
            "n_sym": (193, 192, 2 ** 32 - 1), "pre": (4096, 4097, 65535), "post": (4097, 0), "amp_q": (2 ** 16, 2 ** 16 + 1),
            "noise_q": (2 ** 20 + 1, 2 ** 20), "f_d": (2 ** 31, 2 ** 31 - 1), "pad": (1,)}
    want, blob = [], b""
    for _ in range(300):
        k = int(rng.integers(1, 9))
        rows = [SC.spec_row(int(rng.integers(1, 3000)), at=int(rng.integers(-3000, 3000)), sym=rng.integers(0, 2, int(rng.integers(0, 193))),
                            seed=int(rng.integers(0, 2 ** 63))) for _ in range(k)]
        specs = SC.lay_out(rows, gaps=rng.integers(0, 4, k))
        pool = max(0, SC.default_pool(specs) + int(rng.integers(-20, 60000)))
        kind = int(rng.integers(0, 4))
        i = int(rng.integers(0, k))
        if kind == 1:
            f = list(edge)[int(rng.integers(0, len(edge)))]
            specs[i][f] = edge[f][int(rng.integers(0, len(edge[f])))]
        elif kind == 2:
            specs[i]["bits"][int(rng.integers(0, 24))] |= 1 << int(rng.integers(0, 8))
        elif kind == 3 and i:
            specs[i]["offset"] = max(0, int(specs[i - 1]["offset"]) + 8 * int(rng.integers(-3, 4)))
        want.append(list(SC.check_specs(specs, pool)))
        blob += np.asarray([k], np.int64).tobytes() + np.asarray([pool], np.uint64).tobytes() + specs.tobytes()
    fin, fout = tmp_path / "lists.bin", tmp_path / "answers.bin"
    fin.write_bytes(blob)
    assert f"file ok: {len(want)} lists" in run(exe, "file", fin, fout)
    assert np.fromfile(fout, np.int32).reshape(-1, 2).tolist() == want
    assert sum(w[0] == 0 for w in want) >= 30 and sum(w[0] != 0 for w in want) >= 100
