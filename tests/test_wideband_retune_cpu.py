"""WidebandReceiver.retune / tuning() (rd_wb_retune, rd_wb_tuning), the part that needs no device: the integer phase
arithmetic against Python integers, reset(), the argument errors, the symbols, and - on the float64 model alone - the sign
of the frequency loop and the share of bytes the GPU comparison of tests/test_wideband_retune.py has to exempt."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import chan_bound as CB
import retune_cases as RC
from oracle import channelizer_oracle as CHO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECIM = 100
FO = 19200 * 14
FW = FO * DECIM
# shifts of the plan below: negative, 0 Hz, both band edges
PLAN_SHIFTS = [-3000017, 0, FW // 2, -(FW // 2), 1234567]


def _receiver(block_size=1024):
    from rtldavis_amd import wideband
    # shift = f - centre - if_hz with if_hz = -Fo / 4
    chans = [RC.CENTRE + s - FO // 4 for s in PLAN_SHIFTS]
    w = wideband.WidebandReceiver(RC.packet_config(block_size), chans, RC.CENTRE, decim=DECIM)
    assert [int(s) for s in w.shift_hz] == PLAN_SHIFTS
    return w


def _tuning(w):
    s, p = w.tuning()
    assert s.dtype == np.int64 and p.dtype == np.int64
    return [int(v) for v in s], [int(v) for v in p]


def test_phase_arithmetic_against_python_integers():
    """tuning() = the tuning the next chunk would use: the pending shifts take over at the clock's value t_b, with
    P' = (P + (s - s') t_b) mod Fo.  Without a device no chunk is ever submitted, so (s, P) stays (plan, 0) and the
    clock moves through _debug_advance_clock; the chains of boundaries are the GPU tests'."""
    w = _receiver()
    assert _tuning(w) == (PLAN_SHIFTS, [0] * 5)
    w.retune([17, 17, -17, 17, 17])                     # at clock 0 every phase stays 0
    assert _tuning(w) == ([s + o for s, o in zip(PLAN_SHIFTS, [17, 17, -17, 17, 17])], [0] * 5)
    clock = 0
    rng = np.random.default_rng(5)
    for n in [128, 2 ** 40 + 128 * 3, 128 * 999983, 2 ** 52, 128 * (FO - 1), 2 ** 62]:
        w._debug_advance_clock(n)
        clock += n
        # to the band edges and 0 Hz, at random over the whole band, and across the band from edge to edge
        for new in ([-(FW // 2), FW // 2, 0, 0, -1],
                    [int(v) for v in rng.integers(-(FW // 2), FW // 2 + 1, 5)],
                    [FW // 2, -(FW // 2), -(FW // 2), FW // 2, 0]):
            w.retune(np.asarray(new, np.int64) - np.asarray(PLAN_SHIFTS, np.int64))
            assert [int(s) for s in w.shift_hz] == new
            assert _tuning(w) == (new, RC.next_phase([0] * 5, PLAN_SHIFTS, new, clock, FO)), (clock, new)
    assert clock > 2 ** 62


def test_retune_collapses_and_follows_the_clock():
    w = _receiver()
    w._debug_advance_clock(2 ** 41 + 128)
    t = 2 ** 41 + 128
    w.retune([5, -7, -1, 1, 0])
    w.retune([-20000, 300, -9000, 9000, 12])            # the last call wins, relative to the plan
    new = [s + o for s, o in zip(PLAN_SHIFTS, [-20000, 300, -9000, 9000, 12])]
    assert _tuning(w) == (new, RC.next_phase([0] * 5, PLAN_SHIFTS, new, t, FO))
    w._debug_advance_clock(128 * 5)                     # a pending retune takes effect at the boundary that comes
    assert _tuning(w) == (new, RC.next_phase([0] * 5, PLAN_SHIFTS, new, t + 640, FO))
    w.retune(0)                                         # back to the tuning in force: nothing pending in effect
    assert _tuning(w) == (PLAN_SHIFTS, [0] * 5)
    assert any(RC.next_phase([0] * 5, PLAN_SHIFTS, new, t, FO))


def test_scalar_offset_and_shift_hz():
    w = _receiver()
    w._debug_advance_clock(128 * 12345)
    with pytest.raises(ValueError):
        w.retune(1)                                     # channel 2 sits at +Fw/2
    w.retune([-1, -1, -1, 1, -1])
    new = [s + o for s, o in zip(PLAN_SHIFTS, [-1, -1, -1, 1, -1])]
    assert [int(s) for s in w.shift_hz] == new
    assert _tuning(w)[1] == RC.next_phase([0] * 5, PLAN_SHIFTS, new, 128 * 12345, FO)
    from rtldavis_amd import wideband
    v = wideband.WidebandReceiver(RC.packet_config(1024))        # the default plan, a scalar for all 51 channels
    v._debug_advance_clock(2 ** 40)
    v.retune(-2500)
    plan = [int(s) for s in v._plan_shift_hz]
    assert _tuning(v) == ([s - 2500 for s in plan], [(2500 * 2 ** 40) % FO] * 51)
    v.retune(np.int32(0))
    assert _tuning(v) == (plan, [0] * 51)


def test_reset_restores_the_plan():
    w = _receiver()
    w._debug_advance_clock(2 ** 40 + 128)
    w.retune([-20000, 300, -9000, 9000, 12])
    assert any(_tuning(w)[1])
    w.reset()
    assert _tuning(w) == (PLAN_SHIFTS, [0] * 5)
    assert [int(s) for s in w.shift_hz] == PLAN_SHIFTS
    w.retune([-20000, 300, -9000, 9000, 12])            # the clock is back at 0: no phase
    assert _tuning(w) == ([s + o for s, o in zip(PLAN_SHIFTS, [-20000, 300, -9000, 9000, 12])], [0] * 5)


def test_argument_errors_leave_the_tuning_unchanged():
    from rtldavis_amd import _lib
    w = _receiver()
    w._debug_advance_clock(128 * 777)
    w.retune([-20000, 300, -9000, 9000, 12])
    before = _tuning(w)
    kept = w.shift_hz.copy()
    for bad in ([1, 2, 3, 4], [1, 2, 3, 4, 5, 6], [[0] * 5], 0.5, [0.0] * 5, [0, 0, 1, 0, 0], [0, 0, 0, -1, 0],
                [0, FW, 0, 0, 0], -FW):
        with pytest.raises(ValueError):
            w.retune(bad)
        assert _tuning(w) == before and np.array_equal(w.shift_hz, kept), bad
    L = _lib.lib()
    sh = np.asarray(before[0], np.int64)
    out_s, out_p = np.empty(5, np.int64), np.empty(5, np.int64)
    assert L.rd_wb_retune(w._h, sh.ctypes.data, 4) == _lib.RD_ERR_ARG
    assert L.rd_wb_retune(w._h, sh.ctypes.data, 6) == _lib.RD_ERR_ARG
    assert L.rd_wb_retune(w._h, None, 5) == _lib.RD_ERR_ARG
    assert L.rd_wb_retune(None, sh.ctypes.data, 5) == _lib.RD_ERR_ARG
    for c, v in ((0, FW // 2 + 1), (4, -(FW // 2) - 1), (1, 2 ** 62)):
        over = sh.copy()
        over[c] = v
        assert L.rd_wb_retune(w._h, over.ctypes.data, 5) == _lib.RD_ERR_ARG
        assert "outside the captured band" in _lib.last_error()
    assert L.rd_wb_tuning(w._h, out_s.ctypes.data, out_p.ctypes.data, 4) == _lib.RD_ERR_ARG
    assert L.rd_wb_tuning(w._h, None, out_p.ctypes.data, 5) == _lib.RD_ERR_ARG
    assert L.rd_wb_tuning(None, out_s.ctypes.data, out_p.ctypes.data, 5) == _lib.RD_ERR_ARG
    assert _tuning(w) == before
    assert L.rd_wb_retune(w._h, sh.ctypes.data, 5) == _lib.RD_OK    # (the shifts as given are accepted)
    assert _tuning(w) == before


def test_symbols_declared_exported_and_in_the_ctypes_table():
    from rtldavis_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtldavis_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for n, proto in (("rd_wb_retune", r"int\s+rd_wb_retune\s*\(\s*rd_wideband\s*\*\s*w\s*,\s*const\s+int64_t\s*\*\s*shift_hz\s*,\s*int\s+n\s*\)"),
                     ("rd_wb_tuning", r"int\s+rd_wb_tuning\s*\(\s*rd_wideband\s*\*\s*w\s*,\s*int64_t\s*\*\s*shift_hz\s*,\s*int64_t\s*\*\s*phase\s*,\s*int\s+n\s*\)")):
        assert re.search(proto, src), n
        assert n in _lib.SIGNATURES
        assert hasattr(L, n)
    assert _lib.SIGNATURES["rd_wb_retune"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int])
    assert _lib.SIGNATURES["rd_wb_tuning"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])


def test_loop_sign_on_the_model():
    """The CPU half of test_wideband_retune.py's closed loop: the float64 model's bytes through the dsp oracle's parse.
    Burst A gives e_A; retune(offset = e_A) - the reference's channel_freq + freq_corr - from chunk LOOP_RETUNE_CHUNK on
    leaves burst B at most a quarter of it; the opposite sign pushes burst B out of the demodulator's reach."""
    lc = RC.loop_capture()
    assert [i[0] for i in lc.info] == [lc.payload] * 2
    a_end = lc.info[0][1] + 120 * 14
    assert a_end < 2 * RC.LOOP_B and lc.info[1][1] >= RC.LOOP_RETUNE_CHUNK * RC.LOOP_B
    open_loop = RC.loop_messages(RC.loop_model_blocks(lc, {}))
    assert [m[0] for m in open_loop] == [2, 5]
    e_a, e_open = open_loop[0][2], open_loop[1][2]
    assert abs(e_a - RC.LOOP_CFO) < 500 and abs(e_open - RC.LOOP_CFO) < 500     # both bursts sit ~LOOP_CFO Hz high
    closed = RC.loop_messages(RC.loop_model_blocks(lc, {RC.LOOP_RETUNE_CHUNK: e_a}))
    assert [m[:2] for m in closed] == [m[:2] for m in open_loop] and closed[0] == open_loop[0]   # both CRC-valid, where they were
    e_b = closed[1][2]
    print(f"\n[retune-loop model] e_A {e_a} Hz, e_B {e_b} Hz (open loop {e_open} Hz)")
    assert abs(e_b) <= abs(e_a) / 4
    wrong = RC.loop_messages(RC.loop_model_blocks(lc, {RC.LOOP_RETUNE_CHUNK: -e_a}))
    assert wrong == open_loop[:1]


@pytest.mark.parametrize("name", list(RC.CASES) + ["large_clock"])
def test_exempt_share_of_the_model_cases(name):
    """For every model case of the GPU tests: the share of bytes within delta of a rounding boundary, from the model
    alone, is at most 10 % - the comparison cannot hide a failure behind its exemption."""
    t_off = RC.LARGE_CLOCK if name == "large_clock" else 0
    cs = RC.case(RC.LARGE_CLOCK_CASE if name == "large_clock" else name)
    sched = RC.large_clock_schedule(cs) if name == "large_clock" else cs.schedule
    for k, (shift, phase) in enumerate(RC.tunings(cs, sched, t_off)):
        Z, delta = RC.segment_model(cs, k, shift, phase, t_off)
        s = CB.check_against_model(CHO.quantise(Z), Z, delta)
        assert s["bad_lsb"] == 0 and s["bad_exact"] == 0 and s["mismatches"] == 0
        assert s["exempt"] <= 0.10, (name, k, s)
