"""The narrow-band filter of k_chan_burst_decode (include/rtldavis_hip.h, BURST DECODE, step 4n) on the device.  The hook
rd_debug_burst_decode_narrow on every crafted launch of tests/burst_narrow_cases.py at narrow = 1 and max_flips = 0, 1
and 2: the whole slot - every field of every record, every header, and 0xA5 wherever the kernel must not write - equals
the model's (tests/test_burst_narrow_cpu.py asserts each case's edge without a device).  At narrow = 0 the hook hands
back what rd_debug_burst_decode_repair does, byte for byte.  Then a receiver: bursts in noise in which the wide decoder
finds nothing, streamed at two chunk sizes with narrow on, equal the narrow stream model of the receiver's own
channelized bytes, twice alike; with narrow never switched on the records are the wide model's.  Equality throughout."""
import ctypes as C

import numpy as np
import pytest

import burst_decode_cases as DC
import burst_narrow_cases as NB
import burst_repair_cases as RP
from rtldavis_amd import acquire
from rtldavis_amd.wideband import BURST_MSG_DTYPE

pytestmark = pytest.mark.gpu


def _lib_with_device():
    from rtldavis_amd import _lib
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    return _lib


def _run(_lib, L, max_flips, narrow):
    """The hook with narrow; None: the hook without the argument (rd_debug_burst_decode_repair)."""
    cfg = _lib.make_config(L.cfg.bit_rate, L.cfg.symbol_length, L.cfg.preamble_symbols, L.cfg.packet_symbols, L.cfg.preamble,
                           L.cfg.block_size)
    msgs = np.zeros(L.msgs.shape, BURST_MSG_DTYPE)
    n_msgs, long_runs, chunk = (np.zeros(L.n_ch, np.uint32) for _ in range(3))
    head = (C.byref(cfg), L.cur.ctypes.data, None if L.prev is None else L.prev.ctypes.data, L.cur.shape[1], L.n_ch, L.clock, L.seq,
            L.runs.ctypes.data, L.n_runs.ctypes.data, max_flips)
    tail = (msgs.ctypes.data, n_msgs.ctypes.data, long_runs.ctypes.data, chunk.ctypes.data)
    if narrow is None:
        _lib.check(_lib.lib().rd_debug_burst_decode_repair(*head, *tail))
    else:
        _lib.check(_lib.lib().rd_debug_burst_decode_narrow(*head, narrow, *tail))
    return msgs, n_msgs, long_runs, chunk


def _assert_slot(name, r, got, want):
    msgs, n_msgs, long_runs, chunk = got
    w_msgs, w_n, w_long, w_chunk = want
    assert np.array_equal(n_msgs, w_n), (name, r, n_msgs, w_n)
    assert np.array_equal(long_runs, w_long) and np.array_equal(chunk, w_chunk), (name, r, long_runs, chunk)
    for c in range(msgs.shape[0]):
        n = int(w_n[c])
        for f in BURST_MSG_DTYPE.names:
            assert np.array_equal(msgs[c, :n][f], w_msgs[c, :n][f]), (name, r, c, f, msgs[c, :n][f], w_msgs[c, :n][f])
        assert msgs[c, n:].tobytes() == w_msgs[c, n:].tobytes(), (name, r, c, "a place past n_msgs was written")
    assert msgs.tobytes() == w_msgs.tobytes(), (name, r)


def _check(launches):
    _lib = _lib_with_device()
    for L in launches:
        for r in (0, 1, 2):
            _assert_slot(L.name, r, _run(_lib, L, r, 1), L.narrow[r])


@pytest.mark.parametrize("n", [40, 64, 80])
def test_packet_shapes_each_at_a_grid_point_of_its_own(n):
    """narrow_grid_n{40,64,80}_sl{4,8,14,25,51}: 5 to 107 taps, two carriers per launch."""
    _check(tuple(NB.grid_launch(m, sl) for m, sl in NB.NGRID if m == n))


def test_grid_choice_ties_and_shifts():
    """Hand-written run records: a tie between g = 0 and g = 1, the four axes, corr_re = -1, bit length 31."""
    _check((NB.choice_launch(),))


def test_zero_extension_seam_and_saturated_bytes():
    """The region cut out of a longer carrier (zeros beyond t0 and t1, not the bytes that lie there); the look-back with
    flags = 5; bytes 0 and 255 with f sums beyond 32 bits."""
    first, back, *_ = NB.seam_launches()
    _check((NB.edge_launch()[0], first, back, NB.saturated_launch()))


def test_the_longest_regions():
    """32 + 16 windows at SL 25 and at SL 51: y, the padded int16 region in s's place, 107 taps."""
    _check(NB.longest_launches())


def test_repair_behind_the_filter():
    """One wrong symbol: nothing at R = 0, pad = (1, k, 0, g) and flags = 6 at R = 1 and 2."""
    _check((NB.repair_launch(),))


def test_narrow_off_is_the_hook_before_it():
    """narrow = 0 against rd_debug_burst_decode_repair on the crafted repair launches and on this file's own: the same
    slot byte for byte, and that slot is the wide model's."""
    _lib = _lib_with_device()
    for L in (RP.one_flip_launch(), RP.two_flips_launch(), RP.longest_launch(), NB.choice_launch(), NB.saturated_launch()) + NB.longest_launches():
        for r in (0, 2):
            a, b = _run(_lib, L, r, 0), _run(_lib, L, r, None)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes(), (L.name, r)
            _assert_slot(L.name, r, a, L.want[r])


# ------------------------------------------------------------------------------------------ through a receiver
def _stream(bs, narrow):
    """The capture in chunks of bs through a receiver with decode on and set_burst_narrow(narrow) (None: never called):
    (cfg, thr, blocks, bursts, messages) per chunk from a reset, thresholds at CAP_FACTOR x the floor of the quiet first
    chunk."""
    w = DC.device_receiver(bs, 8, offsets_hz=DC.S8_OFFSETS_HZ)
    chunks = DC.chunks_of(NB.cap_capture(), bs)
    w.set_bursts(True)
    w.set_burst_decode(True)
    if narrow is not None:
        w.set_burst_narrow(narrow)
    w.demodulate(chunks[0])
    thr = acquire.Acquisition(3, w.cfg, factor=NB.CAP_FACTOR).thresholds(w.bursts().floor).astype(np.uint64)
    w.reset()                                                 # (keeps decode and narrow)
    assert w.burst_narrow() is bool(narrow)
    w.set_burst_threshold(thr)
    blocks, bursts, got = [], [], []
    for chunk in chunks:
        w.demodulate(chunk)
        blocks.append(w.channelized())
        bursts.append(w.bursts())
        got.append(w.burst_messages())
    return w.cfg, thr, blocks, bursts, got


@pytest.mark.parametrize("bs", NB.CAP_BS)
def test_receiver_with_narrow_equals_the_stream_model(bs):
    """Seven bursts on three channels in noise of 0.09 against an amplitude of 0.12.  burst_messages() with narrow on
    equals the narrow stream model (steps 1 .. 7) of the receiver's own bytes and burst records, chunk by chunk, and a
    second run gives the same bits; the wide stream model of those bytes decodes none of them, the narrow one at least 3
    (on the float64 channelizer model: 0 and 4 in chunks of 1024, 0 and 5 in chunks of 2048), every row a planted
    payload; with narrow never switched on the receiver gives the wide model's records."""
    _lib_with_device()
    cfg, thr, blocks, bursts, got = _stream(bs, True)
    want = NB.decode_stream(blocks, thr, cfg, 0, bursts=bursts)
    for g, (_, m) in zip(got, want):
        DC.assert_equals_model(g, m)
    rows = np.concatenate([g.records for g in got])
    wide = RP.decode_stream(blocks, thr, cfg, 0, bursts=bursts)
    rows_wide = np.concatenate([m.records for _, m in wide])
    print(f"\n[receiver, chunks of {bs}] narrow rows {rows.size} (g {[int(r['pad'][3]) for r in rows]}), wide rows {rows_wide.size}")
    assert rows_wide.size == 0 and rows.size >= 3
    assert all(bytes(r["data"]) in NB.cap_packets() for r in rows) and acquire.narrowband(rows).all()
    assert not acquire.repaired(rows).any()
    again = _stream(bs, True)
    assert all(np.array_equal(a, b) for a, b in zip(again[2], blocks))
    assert [g.records.tobytes() for g in again[4]] == [g.records.tobytes() for g in got]
    # never switched on
    cfg, thr0, blocks0, bursts0, got0 = _stream(bs, None)
    assert np.array_equal(thr0, thr) and all(np.array_equal(a, b) for a, b in zip(blocks0, blocks))
    for g, (_, m) in zip(got0, DC.decode_stream(blocks0, thr0, cfg, bursts=bursts0)):
        DC.assert_equals_model(g, m)
    assert not acquire.narrowband(np.concatenate([g.records for g in got0])).any()


def test_state_rules_on_the_device():
    _lib = _lib_with_device()
    bs = NB.CAP_BS[0]
    w = DC.device_receiver(bs, 8, offsets_hz=DC.S8_OFFSETS_HZ)
    chunks = DC.chunks_of(NB.cap_capture(), bs)
    w.set_bursts(True)
    with pytest.raises(RuntimeError):
        w.set_burst_narrow(True)                             # decode is off
    w.set_burst_decode(True)
    w.submit(chunks[0])                                      # submitted with narrow off: no table is uploaded
    with pytest.raises(RuntimeError):
        w.set_burst_narrow(True)                             # a chunk in flight
    assert "in flight" in _lib.last_error() and not w.burst_narrow()
    w.fetch()
    assert not acquire.narrowband(w.burst_messages()).any()
    w.set_burst_narrow(True)                                 # the next submit uploads the table
    w.set_burst_repair(2)
    w.demodulate(chunks[1])
    w.reset()
    assert w.burst_narrow() and w.burst_repair() == 2
    w.set_burst_decode(False)
    assert not w.burst_narrow()
    w.set_burst_decode(True)
    w.demodulate(chunks[0])                                  # and a chunk with it off again
    assert w.burst_messages().records.size == 0
