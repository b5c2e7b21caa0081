"""k_chan_bursts and k_chan_burst_decode alone on crafted bytes, through the test hooks rd_debug_bursts and
rd_debug_burst_decode (include/rtldavis_hip.h): exact bytes, exact ties, exact offsets and run records k_chan_bursts
never writes - what the channelizer's bytes of a synthesised capture never put in front of either kernel.  The cases and
the conditions that make each one reach its edge are built, and asserted on the models, in tests/burst_cases.py and
tests/burst_decode_cases.py (tests/test_wideband_bursts_cpu.py, tests/test_wideband_burst_decode_cpu.py run them without
a device).  Here the device's whole slot - every field of every record, floor row and header, and 0xA5 in every place the
kernel must leave alone - equals the model's.  Equality throughout.  The last test is the seam through a real receiver:
a packet whose end crosses a chunk boundary output by output is delivered exactly once (BURST DECODE, step 7)."""
import ctypes as C

import numpy as np
import pytest

import burst_cases as BC
import burst_decode_cases as DC
from rtldavis_amd import acquire
from rtldavis_amd.wideband import BURST_DTYPE, BURST_FLOOR_DTYPE, BURST_MSG_DTYPE

pytestmark = pytest.mark.gpu


def _lib_with_device():
    from rtldavis_amd import _lib
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    return _lib


# ------------------------------------------------------------------------------------------ k_chan_bursts
def _run_bursts(_lib, cs):
    cap = BC.cap_of(cs.n_win)
    recs, floor = np.zeros((cs.n_ch, cap), BURST_DTYPE), np.zeros(cs.n_ch, BURST_FLOOR_DTYPE)
    chan = np.ascontiguousarray(cs.chan)
    _lib.check(_lib.lib().rd_debug_bursts(chan.ctypes.data, cs.stride, cs.n_ch, cs.n_out, cs.thr.ctypes.data, cs.seq,
                                          recs.ctypes.data, floor.ctypes.data))
    return recs, floor


def _assert_bursts(cs, recs, floor):
    want_recs, want_floor = BC.slot_model(cs)
    for f in BURST_FLOOR_DTYPE.names:
        assert np.array_equal(floor[f], want_floor[f]), (cs.name, f, floor[f], want_floor[f])
    for c in range(cs.n_ch):
        n = int(want_floor["n_bursts"][c])
        for f in BURST_DTYPE.names:
            assert np.array_equal(recs[c, :n][f], want_recs[c, :n][f]), (cs.name, c, f, recs[c, :n][f], want_recs[c, :n][f])
        assert recs[c, n:].tobytes() == want_recs[c, n:].tobytes(), (cs.name, c, "a place past n_bursts was written")
    assert recs.tobytes() == want_recs.tobytes() and floor.tobytes() == want_floor.tobytes(), cs.name


def test_bursts_on_crafted_bytes_equal_the_model():
    """Window counts 1 .. 193 around the 16 windows of a pass and the 64 of a group, with and without a gap of 255 between
    the channels; runs carried over two group boundaries; every record place filled (odd nW included); saturated bytes at
    the int32 / uint32 bounds; the threshold at exactly p_w, one above, 0 and 2^32 - 1."""
    _lib = _lib_with_device()
    for cs in BC.crafted_small():
        _assert_bursts(cs, *_run_bursts(_lib, cs))


def test_bursts_on_the_largest_chunk():
    """nW = 4096: 48 KiB of LDS, one run of 4096 saturated windows per channel, sums of 6.8e10."""
    _lib = _lib_with_device()
    cs = BC.crafted_largest()
    recs, floor = _run_bursts(_lib, cs)
    _assert_bursts(cs, recs, floor)
    assert int(recs[0, 0]["power"]) == 68183654400 and int(recs[1, 0]["corr_re"]) == -67650969600


def test_debug_bursts_launches_nothing_for_a_refused_chunk():
    _lib = _lib_with_device()
    chan = np.full(4096, 127, np.uint8)
    thr = np.zeros(1, np.uint32)
    recs, floor = np.zeros(8, BURST_DTYPE), np.zeros(1, BURST_FLOOR_DTYPE)
    for n_out in BC.BAD_N_OUT:
        stride = max(16, 2 * n_out + (-2 * n_out) % 16)
        assert _lib.lib().rd_debug_bursts(chan.ctypes.data, stride, 1, n_out, thr.ctypes.data, 0, recs.ctypes.data,
                                          floor.ctypes.data) == _lib.RD_ERR_ARG, n_out
    assert not recs.tobytes().strip(b"\0") and not floor.tobytes().strip(b"\0")


# ------------------------------------------------------------------------------------------ k_chan_burst_decode
def _run_decode(_lib, L):
    cfg = _lib.make_config(L.cfg.bit_rate, L.cfg.symbol_length, L.cfg.preamble_symbols, L.cfg.packet_symbols, L.cfg.preamble,
                           L.cfg.block_size)
    msgs = np.zeros(L.msgs.shape, BURST_MSG_DTYPE)
    n_msgs, long_runs, chunk = (np.zeros(L.n_ch, np.uint32) for _ in range(3))
    _lib.check(_lib.lib().rd_debug_burst_decode(C.byref(cfg), L.cur.ctypes.data, None if L.prev is None else L.prev.ctypes.data,
                                                L.cur.shape[1], L.n_ch, L.clock, L.seq, L.runs.ctypes.data, L.n_runs.ctypes.data,
                                                msgs.ctypes.data, n_msgs.ctypes.data, long_runs.ctypes.data, chunk.ctypes.data))
    return msgs, n_msgs, long_runs, chunk


def _assert_decode(L, got):
    msgs, n_msgs, long_runs, chunk = got
    assert np.array_equal(n_msgs, L.n_msgs), (L.name, n_msgs, L.n_msgs)
    assert np.array_equal(long_runs, L.long_runs) and np.array_equal(chunk, L.chunk), (L.name, long_runs, chunk)
    for c in range(L.n_ch):
        n = int(L.n_msgs[c])
        for f in BURST_MSG_DTYPE.names:
            assert np.array_equal(msgs[c, :n][f], L.msgs[c, :n][f]), (L.name, c, f, msgs[c, :n][f], L.msgs[c, :n][f])
        assert msgs[c, n:].tobytes() == L.msgs[c, n:].tobytes(), (L.name, c, "a place past n_msgs was written")
    assert msgs.tobytes() == L.msgs.tobytes(), L.name


def test_decode_ties_and_the_ends_of_the_candidate_range():
    """Equal 64-bit margins in one lane's stride, across waves and far apart go to the smallest tau, one step of
    amplitude turns it; tau = t0 + SL and tau + SL (N - 1) = t1 - 1 are candidates, one output further is not."""
    _lib = _lib_with_device()
    for L in (DC.tie_launch(), DC.range_launch()):
        _assert_decode(L, _run_decode(_lib, L))


def test_decode_look_back_at_the_seam():
    """The packet's last output at boundary - SL .. boundary + SL, a channel per position: chunk 0 alone, chunk 1 with
    chunk 0 behind it (tau + SL (N - 1) = 0 among them), chunk 1 with no chunk behind it (no look-back)."""
    _lib = _lib_with_device()
    for L in DC.seam_launches():
        _assert_decode(L, _run_decode(_lib, L))


def test_decode_longest_region_run_length_and_need():
    """32 + 16 windows (all of the LDS, 24 outputs per lane); runs of 32 and 33 windows; regions of need - 1 and more."""
    _lib = _lib_with_device()
    for L in (DC.longest_launch(), DC.run_length_launch(), DC.need_launch()):
        _assert_decode(L, _run_decode(_lib, L))


def test_decode_packet_shapes():
    """N in 40, 64, 80 x SL in 1, 8, 14, 25, 51 where N SL + 1 <= 2048: data[N / 8:] zero, chunk = the low 32 bits of seq."""
    _lib = _lib_with_device()
    for n, sl in DC.GRID:
        L = DC.grid_launch(n, sl)
        _assert_decode(L, _run_decode(_lib, L))


def test_decode_several_runs_handwritten_records_and_the_overflow_bound():
    """Three messages in run order beside a channel with none and the CRC-invalid twin, the clock wrapping at 2^64; corr =
    0, windows = 0, first = nW, first + windows = nW + 1 and n_runs = cap + 3 give nothing and hide nothing; a
    correlation sum of +-(2^30 - 1) over saturated bytes."""
    _lib = _lib_with_device()
    for L in (DC.several_launch(), DC.handwritten_launch(), DC.overflow_launch()):
        _assert_decode(L, _run_decode(_lib, L))


# ------------------------------------------------------------------------------------------ the seam, through a receiver
@pytest.mark.parametrize("followed", [True, False])
def test_receiver_reports_a_packet_at_the_seam_once(followed):
    """The decim-4 "s16" plan, block_size 2048, one synthesised burst with j = 0 .. 2 SL more outputs of noise in front,
    so that the packet's end crosses the boundary between chunks 0 and 1 output by output.  For every j the receiver's
    messages equal decode_stream (steps 1 .. 7) of its own bytes and burst records.
    followed (burst_decode_cases.seam_capture): a next transmission's lead-in begins where the burst ends, so chunk 1's
    run is sliced near the carrier.  The payload is delivered exactly once for every j, and for at least one j
    decode_model (steps 1 .. 6) of those bytes reports it in both chunks - the sweep covers the seam (on the float64
    channelizer model's bytes: 10 of 29 positions, packet ends 2043 .. 2052).
    not followed: noise behind the burst.  Chunk 1's run is the 8 trailing 0-symbols, its correlation sum lies a
    deviation below the carrier, and chunk 1 decodes nothing until 12 outputs of the packet reach into it: no position
    is reported twice even without step 7, and the float64 model's bytes lose the packet at j = 19 .. 25 - a limit of
    the definition (steps 3 and 4), not of step 7; here only device = model and "never twice" are asserted."""
    _lib_with_device()
    bs, sl = DC.SEAM_BS, DC.SEAM_SL
    w = DC.device_receiver(bs)
    w.set_bursts(True)
    w.set_burst_decode(True)
    quiet, _ = DC.device_capture()
    w.demodulate(quiet[: 2 * DC.DEV_DECIM * bs])
    thr = acquire.Acquisition(3, w.cfg).thresholds(w.bursts().floor).astype(np.uint64)
    payload = DC.VALID[1]
    before, after = [], []
    for j in range(2 * sl + 1):
        chunks = DC.chunks_of(DC.seam_capture(j, followed), bs)
        w.reset()
        w.set_burst_threshold(thr)
        blocks, bursts, got = [], [], []
        for chunk in chunks:
            w.demodulate(chunk)
            blocks.append(w.channelized())
            bursts.append(w.bursts())
            got.append(w.burst_messages())
        want = DC.decode_stream(blocks, thr, w.cfg, bursts=bursts)
        for g, (_, m) in zip(got, want):
            DC.assert_equals_model(g, m)
        plain = [DC.decode_model(blocks[k], blocks[k - 1] if k else None, bursts[k], w.cfg, k >= 1, k * bs) for k in range(len(blocks))]
        before.append(sum(bytes(r["data"]).hex() == payload for m in plain for r in m.records))
        after.append(sum(bytes(r["data"]).hex() == payload for m in got for r in m.records))
    print(f"\n[seam receiver, followed={followed}] reports of the packet per j without step 7 {before}, delivered {after}")
    if followed:
        assert after == [1] * (2 * sl + 1)
        assert 2 in before and set(before) <= {1, 2}
    else:
        assert max(after) == 1 and after == before
