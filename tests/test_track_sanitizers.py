"""The pure-host parts of BURST EXPECT (rtldavis_amd/csrc/rd_host.cpp: the table's rules, an expectation's candidate
range for a clock, step 7') in a stand-alone program, tests/track_asan.cpp, built with -fsanitize=address,undefined and
run here on the CPU: the table's limits on either side, the range against a naive enumeration with the 64-bit clock near
its wrap, and the library's range against the model's on the crafted launches' own tables.  The library compiles the
same rd_host.cpp (csrc/Makefile)."""
import os
import subprocess

import numpy as np
import pytest

import burst_track_cases as TK
from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "_build")
EXE = os.path.join(BUILD, "track_asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "track_asan.cpp"), os.path.join(ROOT, "rtldavis_amd", "csrc", "rd_host.cpp")]
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


def test_table_rules_and_step_7_prime_under_sanitizers(exe):
    out = run(exe, "table")
    assert "table ok" in out and "repeats ok" in out


def test_candidate_ranges_against_a_naive_enumeration_under_sanitizers(exe):
    for seed in (1, 2):
        out = run(exe, "range", seed, 3000)
        assert "range ok" in out
        active, wrapped = int(out.split()[2]), int(out.split()[6])
        assert active > 300 and wrapped > 10, out              # windows were met, some across 2^64


def test_library_range_equals_the_models(exe, tmp_path):
    """Every expectation of the crafted launches at its own clock, and the same tables moved to the end of the clock."""
    cases, want = [], []
    launches = [TK.edges_launch()[0], *TK.seam_launches()[:2], TK.gap_window0_off()[1], *TK.first_chunk_launches(), TK.alignment_launch()[0],
                TK.largest_launch(), TK.full_table_launch(), TK.all_idle_launch()]
    for X in launches:
        for move in (0, 2 ** 64 - X.clock - 700):
            for e in X.table:
                sl, n = int(X.cfg.symbol_length), int(X.cfg.packet_symbols)
                clock, t_lo = (X.clock + move) % 2 ** 64, (int(e["t_lo"]) + move) % 2 ** 64
                t_hi = t_lo + int(e["t_hi"]) - int(e["t_lo"])
                if t_hi >= 2 ** 64:                               # (the table's rule: t_lo <= t_hi)
                    continue
                cases.append([sl, n, int(X.cfg.block_size), int(X.prev is not None), clock, t_lo, t_hi])
                got = TK.candidate_range(X.cfg, X.prev is not None, clock, t_lo, t_hi)
                want.append([0, 0, -1] if got is None else [1, got[0], got[1]])
    fin, fout = tmp_path / "cases.bin", tmp_path / "ranges.bin"
    np.asarray(cases, np.uint64).tofile(fin)
    assert f"file ok: {len(cases)} cases" in run(exe, "file", fin, fout)
    res = np.fromfile(fout, np.int32).reshape(-1, 3)
    assert res.tolist() == want
    assert sum(w[0] for w in want) > 100 and sum(1 - w[0] for w in want) > 20
