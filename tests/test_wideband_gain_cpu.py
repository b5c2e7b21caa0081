"""WidebandReceiver.set_gain / gains() / levels() and agc.GainControl, the part that needs no device: the control rule
step by step on hand-made level records, the argument checks and recorded values on a receiver that never submits, the
symbols, and - on the float64 model alone - the share of bytes the GPU comparison of tests/test_wideband_gain.py has to
exempt and the reason for per-channel gains: a capture whose weak packet the scalar gain loses and the gain loop keeps."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import chan_bound as CB
import gain_cases as GC
import retune_cases as RC
from oracle import channelizer_oracle as CHO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2 * 128                     # components per chunk of the hand-made records


def _ctl(n=2, **kw):
    from rtldavis_amd import agc
    args = dict(min_gain=1.0, max_gain=8.0, step_db=6.0, start_gain=2.0, low_power=9 * N, high_power=144 * N,
                clip_max=10, hold=3)
    args.update(kw)
    return agc.GainControl(n, 128, **args)


def _lv(*rows):
    """Level records (power, clipped) as the structured array levels() returns."""
    from rtldavis_amd import wideband
    out = np.zeros(len(rows), wideband.LEVEL_DTYPE)
    for i, (power, clipped) in enumerate(rows):
        out[i]["power"], out[i]["clipped"] = power, clipped
    return out


QUIET, MID, LOUD = (9 * N - 1, 0), (9 * N, 0), (144 * N + 1, 0)


def test_gain_table():
    c = _ctl()
    want = [np.float32(10.0 ** (i * 6.0 / 20.0)) for i in range(4)]       # 1, 2.0, 3.98, 7.94; the next one is 15.8 > 8
    assert c.table.dtype == np.float32 and c.table.tolist() == [float(v) for v in want]
    assert c.index == [1, 1] and c.quiet == [0, 0]                         # the largest entry <= start_gain = 2.0
    assert c.gains().dtype == np.float32 and c.gains().tolist() == [float(want[1])] * 2
    assert _ctl(start_gain=0.5).index == [0, 0] and _ctl(start_gain=100.0).index == [3, 3]
    from rtldavis_amd import agc
    d = agc.GainControl(51, 8192)                                          # the defaults
    assert d.table[0] == np.float32(0.25) and d.table[-1] <= 512.0 and d.table[-1] * 10 ** (3 / 20) > 512.0
    assert d.low_power == 9 * 16384 and d.high_power == 144 * 16384 and d.clip_max == 4096 and d.hold == 4
    assert float(d.gains()[0]) <= 3.0 < float(d.table[d.index[0] + 1])


def test_step_down_on_clipping_and_on_power():
    c = _ctl()
    assert c.update(_lv((MID[0], 10), MID)) is None                       # clipped == clip_max: not above it
    g = c.update(_lv((MID[0], 11), MID))                                  # clipping alone
    assert g.tolist() == [1.0, float(c.table[1])] and c.index == [0, 1]
    g = c.update(_lv(MID, LOUD))                                          # power alone
    assert g.tolist() == [1.0, 1.0] and c.index == [0, 0]
    assert c.update(_lv(MID, (144 * N, 0))) is None                       # power == high_power: not above it
    assert c.update(_lv(LOUD, (0, 11))) is None and c.index == [0, 0]     # the table's lower end: nothing to set


def test_step_up_only_after_hold_and_counter_reset():
    c = _ctl(n=3)
    assert c.update(_lv(QUIET, QUIET, QUIET)) is None and c.quiet == [1, 1, 1]
    assert c.update(_lv(QUIET, MID, (QUIET[0], 1))) is None               # not below low_power / a clipped byte: reset
    assert c.quiet == [2, 0, 0] and c.index == [1, 1, 1]
    g = c.update(_lv(QUIET, QUIET, QUIET))
    assert c.index == [2, 1, 1] and c.quiet == [0, 1, 1]                  # the third quiet chunk in a row, channel 0 only
    assert g.tolist() == [float(c.table[2]), float(c.table[1]), float(c.table[1])]
    assert c.update(_lv(MID, QUIET, LOUD)) .tolist() == [float(c.table[2]), float(c.table[1]), 1.0]
    assert c.quiet == [0, 2, 0] and c.index == [2, 1, 0]                  # a step down clears the counter too
    g = c.update(_lv(MID, QUIET, QUIET))
    assert g.tolist() == [float(c.table[2]), float(c.table[2]), 1.0] and c.quiet == [0, 0, 1]


def test_the_tables_upper_end():
    c = _ctl(n=1, hold=1, start_gain=4.0)
    assert c.index == [2]
    assert c.update(_lv(QUIET)).tolist() == [float(c.table[3])]
    for _ in range(3):
        assert c.update(_lv(QUIET)) is None and c.index == [3]            # the upper end: nothing to set
    assert c.update(_lv(LOUD)).tolist() == [float(c.table[2])]


def test_update_is_deterministic_and_takes_levels_objects():
    from rtldavis_amd import wideband
    rng = np.random.default_rng(7)
    seq = [_lv(*[(int(rng.integers(0, 200 * N)), int(rng.integers(0, 20))) for _ in range(4)]) for _ in range(200)]
    runs = []
    for wrap in (False, True):
        c, out = _ctl(n=4), []
        for lv in seq:
            g = c.update(wideband.Levels(lv, wideband.InputLevel(1, 0, 1), 0) if wrap else lv)
            out.append(None if g is None else g.tolist())
        runs.append((out, list(c.index), list(c.quiet)))
    assert runs[0] == runs[1] and any(o is not None for o in runs[0][0]) and any(o is None for o in runs[0][0])
    with pytest.raises(ValueError):
        _ctl(n=4).update(seq[0][:3])


def _receiver(gain=3.0, n=5):
    from rtldavis_amd import wideband
    chans = [RC.CENTRE + 100000 * (c - 2) for c in range(n)]
    return wideband.WidebandReceiver(RC.packet_config(1024), chans, RC.CENTRE, gain=gain)


def test_set_gain_records_and_reset_restores():
    w = _receiver(gain=2.5)
    assert w.gains().dtype == np.float64 and w.gains().tolist() == [2.5] * 5
    w.set_gain([0.25, 1.0, 3.0, 40.0, 300.0])
    assert w.gains().tolist() == [0.25, 1.0, 3.0, 40.0, 300.0]
    w.set_gain(0.1)                                                       # a scalar for all; stored as float32
    assert w.gains().tolist() == [float(np.float32(0.1))] * 5
    w.set_gain(np.float32(7.0))
    w.set_gain(np.asarray([1, 2, 3, 4, 5]))                               # integers are numbers
    assert w.gains().tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
    w.reset()
    assert w.gains().tolist() == [2.5] * 5
    with pytest.raises(RuntimeError):
        w.levels()                                                        # nothing fetched
    w.set_levels(True)
    w.set_levels(False)


def test_argument_errors_record_nothing():
    from rtldavis_amd import _lib
    w = _receiver()
    w.set_gain([0.25, 1.0, 3.0, 40.0, 300.0])
    kept = w.gains().tolist()
    nan, inf = float("nan"), float("inf")
    for bad in ([1.0] * 4, [1.0] * 6, [[1.0] * 5], 0, 0.0, -1.0, nan, inf, -inf, [1, 1, 0, 1, 1], [1, 1, 1, -2, 1],
                [1, nan, 1, 1, 1], [1, 1, 1, 1, inf], 1e39, 1e-46, "x", None):
        with pytest.raises(ValueError):
            w.set_gain(bad)
        assert w.gains().tolist() == kept, bad
    L = _lib.lib()
    g = np.asarray(kept, np.float64)
    out = np.empty(5, np.float64)
    assert L.rd_wb_set_gain(w._h, g.ctypes.data, 4) == _lib.RD_ERR_ARG
    assert L.rd_wb_set_gain(w._h, g.ctypes.data, 6) == _lib.RD_ERR_ARG
    assert L.rd_wb_set_gain(w._h, None, 5) == _lib.RD_ERR_ARG
    assert L.rd_wb_set_gain(None, g.ctypes.data, 5) == _lib.RD_ERR_ARG
    for c, v in ((0, 0.0), (4, -3.0), (2, nan), (1, inf), (3, 1e39), (3, 1e-46)):
        b = g.copy()
        b[c] = v
        assert L.rd_wb_set_gain(w._h, b.ctypes.data, 5) == _lib.RD_ERR_ARG
        assert f"channel {c}" in _lib.last_error()
    assert L.rd_wb_gains(w._h, out.ctypes.data, 4) == _lib.RD_ERR_ARG
    assert L.rd_wb_gains(w._h, None, 5) == _lib.RD_ERR_ARG
    assert L.rd_wb_gains(None, out.ctypes.data, 5) == _lib.RD_ERR_ARG
    assert L.rd_wb_levels(w._h, None, 5, None) == _lib.RD_ERR_ARG
    assert L.rd_wb_set_levels(None, 1) == _lib.RD_ERR_ARG
    recs = (_lib.RdChanLevel * 5)()
    assert L.rd_wb_levels(w._h, recs, 4, None) == _lib.RD_ERR_ARG
    assert L.rd_wb_levels(w._h, recs, 5, None) == _lib.RD_ERR_STATE
    assert w.gains().tolist() == kept
    assert L.rd_wb_set_gain(w._h, g.ctypes.data, 5) == _lib.RD_OK


def test_channelizer_set_gain_argument_errors():
    from rtldavis_amd import _lib, channelizer
    ch = channelizer.Channelizer([RC.CENTRE - 100000, RC.CENTRE + 100000], RC.CENTRE)
    ch.set_gain(2.0)
    ch.set_gain([0.25, 300.0])
    for bad in ([1.0], [1.0] * 3, 0, -1.0, float("nan"), float("inf"), [1.0, 0.0]):
        with pytest.raises(ValueError):
            ch.set_gain(bad)
    g = np.asarray([1.0, 2.0])
    assert _lib.lib().rd_chan_set_gain(ch._h, g.ctypes.data, 3) == _lib.RD_ERR_ARG
    assert _lib.lib().rd_chan_set_gain(None, g.ctypes.data, 2) == _lib.RD_ERR_ARG


def test_symbols_declared_exported_and_in_the_ctypes_table():
    from rtldavis_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtldavis_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    protos = {
        "rd_chan_set_gain": r"int\s+rd_chan_set_gain\s*\(\s*rd_chan\s*\*\s*h\s*,\s*const\s+double\s*\*\s*gain\s*,\s*int\s+n\s*\)",
        "rd_wb_set_gain": r"int\s+rd_wb_set_gain\s*\(\s*rd_wideband\s*\*\s*w\s*,\s*const\s+double\s*\*\s*gain\s*,\s*int\s+n\s*\)",
        "rd_wb_gains": r"int\s+rd_wb_gains\s*\(\s*rd_wideband\s*\*\s*w\s*,\s*double\s*\*\s*gain\s*,\s*int\s+n\s*\)",
        "rd_wb_set_levels": r"int\s+rd_wb_set_levels\s*\(\s*rd_wideband\s*\*\s*w\s*,\s*int\s+enabled\s*\)",
        "rd_wb_levels": r"int\s+rd_wb_levels\s*\(\s*rd_wideband\s*\*\s*w\s*,\s*rd_chan_level\s*\*\s*out\s*,\s*int\s+n\s*,\s*rd_input_level\s*\*\s*in\s*\)",
    }
    for n, proto in protos.items():
        assert re.search(proto, src), n
        assert n in _lib.SIGNATURES and hasattr(L, n)
    # the records' layout, as the header declares it
    assert [(f, t) for f, t in _lib.RdChanLevel._fields_] == [("power", C.c_uint64), ("peak", C.c_uint32),
                                                              ("clipped", C.c_uint32), ("gain", C.c_float), ("chunk", C.c_uint32)]
    assert C.sizeof(_lib.RdChanLevel) == 24 and C.sizeof(_lib.RdInputLevel) == 24
    for st, fields in (("rd_chan_level", "uint64_t power; uint32_t peak; uint32_t clipped; float gain; uint32_t chunk;"),
                       ("rd_input_level", "uint64_t power; uint64_t chunk; uint32_t peak; uint32_t clipped;")):
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}" % st, src, flags=re.S).group(1)
        assert " ".join(body.split()) == fields, st


def test_level_helpers_on_hand_made_bytes():
    blk = np.full((2, 8), 127, np.uint8)
    blk[1] = [0, 255, 128, 127, 1, 254, 200, 3]
    assert GC.channel_levels(blk) == [(1, 0, 8), (255, 2, 2 * 255 ** 2 + 1 + 1 + 2 * 253 ** 2 + 145 ** 2 + 249 ** 2)]
    assert GC.input_levels(np.asarray([0, 255, 127, 128], np.uint8), "u8") == (255, 2, 2 * 255 ** 2 + 2)
    assert GC.input_levels(np.asarray([-128, 127, 0, -3], np.int8), "s8") == (128, 2, 128 ** 2 + 127 ** 2 + 9)
    assert GC.input_levels(np.asarray([-32768, 32767, 5, -32767], np.int16), "s16") == (32768, 2, 32768 ** 2 + 2 * 32767 ** 2 + 25)


@pytest.mark.parametrize("name", list(RC.CASES))
def test_exempt_share_of_the_model_cases(name):
    """For every chunk of every case under its gain schedule (and the retune before chunk 3): the share of bytes within
    delta of a rounding boundary, from the model alone, is at most 6 % - the GPU comparison, which may exempt 10 %,
    cannot hide a failure behind its exemption."""
    gc = GC.case(name)
    gains = GC.gains_per_chunk(gc)
    assert min(g.min() for g in gains) == 0.25 and max(g.max() for g in gains) == 300.0
    if name == "s16":
        assert 300.0 in gains[0]
    worst = 0.0
    for k, (Z, delta, g, _) in enumerate(GC.schedule_models(gc)):
        s = CB.check_against_model(CHO.quantise(Z), Z, delta)
        assert s["bad_lsb"] == 0 and s["bad_exact"] == 0 and s["mismatches"] == 0
        worst = max(worst, s["exempt"])
        assert s["exempt"] <= GC.MODEL_EXEMPT_CAP, (name, k, s)
    print(f"\n[gain-model] {name}: worst exempt share {worst:.2%}")


def test_scalar_gain_loses_the_weak_packet_and_the_loop_keeps_both():
    """Model only (float64 channelizer -> dsp oracle): the capture of gain_cases.loop_capture at the scalar gain 3.0
    yields the strong channel's packet alone; with the gains GainControl reaches from the model's own levels, fed as
    the device test feeds them, both come back."""
    lc = GC.loop_capture()
    strong, weak = lc.info
    assert (strong[1] + 1680) // GC.LOOP_B == strong[1] // GC.LOOP_B == 2 and weak[1] // GC.LOOP_B == 9
    amp = np.abs(lc.raw.astype(np.int64))
    assert amp.max() > 0.85 * 32768                                      # the strong burst: near full scale
    scalar = GC.loop_messages([GC.loop_model_block(k, [GC.LOOP_SCALAR_GAIN] * 2) for k in range(GC.LOOP_NK)])
    assert scalar == [(0, 3, strong[0])]
    blocks, used = GC.loop_run_model()
    assert GC.loop_messages(blocks) == [(0, 3, strong[0]), (1, 10, weak[0])]
    assert used[2].tolist() == [3.0, 3.0] and used[9][1] == 300.0 and used[9][0] < 95.0
    # the weak channel's bytes at 3.0: a constant
    assert all(np.all(GC.loop_model_block(k, [3.0, 3.0])[1] == 127) for k in (9, 10))
