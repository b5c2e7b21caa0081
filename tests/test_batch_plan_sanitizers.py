"""The decisions of the batch demodulator (rtldavis_amd/csrc/rd_batch_plan.cpp: a handle's sizes, the launch plan of a run, the
overflow ladder, what results() copies) in a stand-alone program, tests/batch_plan_asan.cpp, built with
-fsanitize=address,undefined and run here on the CPU.  Each is compared with a literal restatement, kept in that program, of
the flat host code of rd_batch.hip it replaced - HIP calls as tokens - over the cross product of its inputs, and the ladder
as a whole over scripted counters with a fake device.  The library compiles the same rd_batch_plan.cpp (csrc/Makefile)."""
import os
import subprocess

import pytest

from conftest import ROOT

BUILD = os.path.join(ROOT, "tests", "_build")
EXE = os.path.join(BUILD, "batch_plan_asan")
CSRC = os.path.join(ROOT, "rtldavis_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "batch_plan_asan.cpp"), os.path.join(CSRC, "rd_batch_plan.cpp"), os.path.join(CSRC, "rd_host.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("rd_batch_plan.h", "rd_host.h", "rd_slots.h", "rd_parse.h")] + \
        [os.path.join(ROOT, "include", "rtldavis_hip.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-ffp-contract=off", "-Wall", "-Wextra", "-o", EXE] + srcs)
    return EXE


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{args}: rc {r.returncode}\n{r.stdout}\n{r.stderr[-3000:]}"
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout


def test_ladder_step_equals_the_flat_loop_body_under_sanitizers(exe):
    out = run(exe, "ladder")
    # run flags (ft_run, second_pass, dev_order, fast_ok) x what the handle had learned (tail_off, ft_sticky) x 9 overflow
    # masks x FIX and MATCH at cap - 1, cap, cap + 1 x 8 attempts x 3 list lengths x the bucket hook off / on
    assert "ladder ok" in out and int(out.split()[2]) == 64 * 9 * 3 * 3 * 8 * 3 * 2, out
    assert 0 < int(out.split()[4]) < int(out.split()[2]) and int(out.split()[6]) > 0, out


def test_ladder_scenarios_with_a_fake_device_under_sanitizers(exe):
    out = run(exe, "runs")
    assert "runs ok" in out and int(out.split()[2]) >= 8, out


def test_sizes_and_create_limit_under_sanitizers(exe):
    out = run(exe, "sizes")
    # 4 configurations x 6 stream counts x 6 block counts x RD_TAIL_IMPL unset / legacy x 3 hooks absent / below / at / above
    assert "sizes ok" in out and int(out.split()[2]) == 4 * 6 * 6 * 2 * 4 * 4 * 4, out
    assert int(out.split()[4]) > 0, out   # (some of them have the one-launch tail's buffers)


def test_launch_plan_equals_the_three_branches_under_sanitizers(exe):
    out = run(exe, "plan")
    assert "plan ok" in out and int(out.split()[2]) == 256, out
    assert int(out.split()[4]) == 256 * 3 // 32 and int(out.split()[7]) == 256 * 3 // 16, out   # buckets: 1/8 x 3/4; deferred: 1/4 x 3/4


def test_result_counts_stay_inside_the_record_array_under_sanitizers(exe):
    out = run(exe, "counts")
    assert "counts ok" in out and int(out.split()[2]) > 10000, out
