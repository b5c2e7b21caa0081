"""The host half of the channelizer's tables (rtldavis_amd/csrc/rd_chan_tables.cpp, and the functions of rd_chan_tables.h
that it shares with k_chan_retune) in a stand-alone program, tests/chan_tables_asan.cpp, built with
-fsanitize=address,undefined and run here on the CPU: the builder against a forward model of the tables over a grid of
shapes, the host path of a retune, every rule of create and of the gain check on either side of its limit, and the float
form of the two-term f16 split against the direct one.  The library compiles the same rd_chan_tables.cpp (csrc/Makefile).
The compiler is the clang++ of the ROCm installation the Makefile's hipcc belongs to: it has _Float16 on x86-64."""
import os
import subprocess

import pytest

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "_build")
EXE = os.path.join(BUILD, "chan_tables_asan")
CSRC = os.path.join(ROOT, "rtldavis_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "chan_tables_asan.cpp"), os.path.join(CSRC, "rd_chan_tables.cpp")]
    deps = srcs + [os.path.join(CSRC, "rd_chan_tables.h"), os.path.join(CSRC, "rd_host.h"), os.path.join(ROOT, "include", "rtldavis_hip.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call([CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-ffp-contract=off", "-Wall", "-Wextra", "-o", EXE] + srcs)
    return EXE


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{args}: rc {r.returncode}\n{r.stdout}\n{r.stderr[-3000:]}"
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout


def test_tables_against_the_forward_model_under_sanitizers(exe):
    out = run(exe, "tables")
    assert "tables ok" in out
    # the grid: 4 formats x n_taps {1, 8, 13, 64, 255} x decim {4, 100} x n_channels {1, 17, 65}; a configuration's A operand
    # is [groups of 64 channels][t_pad / kc + 1 K steps][2 terms][4 row blocks][64 lanes][8] 16-bit entries
    configs = entries = 0
    for kc in (8, 8, 4, 4):
        for n_taps in (1, 8, 13, 64, 255):
            for _decim in (4, 100):
                for n_ch in (1, 17, 65):
                    t_pad = (n_taps + 7) // 8 * 8
                    configs += 1
                    entries += ((n_ch + 63) // 64) * (t_pad // kc + 1) * 2 * 4 * 64 * 8
    assert configs == 120
    assert int(out.split()[2]) == configs and int(out.split()[4]) == entries, out


def test_host_retune_under_sanitizers(exe):
    out = run(exe, "retune")
    assert "retune ok" in out and int(out.split()[2]) == 4 * 2 * 4, out


def test_argument_rules_under_sanitizers(exe):
    assert "args ok" in run(exe, "args")


def test_f16_split_float_form_equals_the_direct_form(exe):
    out = run(exe, "split")
    assert "split ok" in out and int(out.split()[2]) == 121 * 8000 * 2 and int(out.split()[4]) == 0, out
