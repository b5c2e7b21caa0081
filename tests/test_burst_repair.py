"""CRC-guided repair in k_chan_burst_decode (include/rtldavis_hip.h, BURST DECODE, steps 5a, 5b, 6') on the device.  The
hook rd_debug_burst_decode_repair on every crafted launch of tests/burst_repair_cases.py at max_flips = 0, 1 and 2: the
whole slot - every field of every record, every header, and 0xA5 wherever the kernel must not write - equals the model's
(tests/test_burst_repair_cpu.py asserts each case's edge without a device).  At max_flips = 0 the hook hands back what
rd_debug_burst_decode does, byte for byte.  Then a receiver: a capture with damaged bursts streamed at two chunk sizes
with repair on equals the stream model of its own channelized bytes, twice alike; with repair never switched on it gives
the records of a receiver without the feature.  Equality throughout."""
import ctypes as C

import numpy as np
import pytest

import burst_decode_cases as DC
import burst_repair_cases as RP
from rtldavis_amd import acquire
from rtldavis_amd.wideband import BURST_MSG_DTYPE

pytestmark = pytest.mark.gpu


def _lib_with_device():
    from rtldavis_amd import _lib
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    return _lib


def _run(_lib, L, max_flips):
    """The hook with max_flips; None: the hook without the argument (rd_debug_burst_decode)."""
    cfg = _lib.make_config(L.cfg.bit_rate, L.cfg.symbol_length, L.cfg.preamble_symbols, L.cfg.packet_symbols, L.cfg.preamble,
                           L.cfg.block_size)
    msgs = np.zeros(L.msgs.shape, BURST_MSG_DTYPE)
    n_msgs, long_runs, chunk = (np.zeros(L.n_ch, np.uint32) for _ in range(3))
    head = (C.byref(cfg), L.cur.ctypes.data, None if L.prev is None else L.prev.ctypes.data, L.cur.shape[1], L.n_ch, L.clock, L.seq,
            L.runs.ctypes.data, L.n_runs.ctypes.data)
    tail = (msgs.ctypes.data, n_msgs.ctypes.data, long_runs.ctypes.data, chunk.ctypes.data)
    if max_flips is None:
        _lib.check(_lib.lib().rd_debug_burst_decode(*head, *tail))
    else:
        _lib.check(_lib.lib().rd_debug_burst_decode_repair(*head, max_flips, *tail))
    return msgs, n_msgs, long_runs, chunk


def _assert_slot(L, r, got):
    msgs, n_msgs, long_runs, chunk = got
    w_msgs, w_n, w_long, w_chunk = L.want[r]
    assert np.array_equal(n_msgs, w_n), (L.name, r, n_msgs, w_n)
    assert np.array_equal(long_runs, w_long) and np.array_equal(chunk, w_chunk), (L.name, r, long_runs, chunk)
    for c in range(L.n_ch):
        n = int(w_n[c])
        for f in BURST_MSG_DTYPE.names:
            assert np.array_equal(msgs[c, :n][f], w_msgs[c, :n][f]), (L.name, r, c, f, msgs[c, :n][f], w_msgs[c, :n][f])
        assert msgs[c, n:].tobytes() == w_msgs[c, n:].tobytes(), (L.name, r, c, "a place past n_msgs was written")
    assert msgs.tobytes() == w_msgs.tobytes(), (L.name, r)


def _check(launches):
    _lib = _lib_with_device()
    for L in launches:
        for r in (0, 1, 2):
            _assert_slot(L, r, _run(_lib, L, r))


def test_one_and_two_flips():
    """A weak wrong symbol at k = 16, N - 1, 23, 24: pad = (1, k, 0, 0) and the planted data, nothing at R = 0; pairs
    (16, N - 1), (40, 41), (23, 24): nothing at R = 1, the record at R = 2."""
    _check((RP.one_flip_launch(), RP.two_flips_launch()))


def test_the_list_its_edge_and_its_ties():
    """The wrong symbol at rank 7 is repaired, at rank 8 and 9 it is not; a wrong symbol of full magnitude or inside the
    sync word gives nothing; of two pairs with one syndrome the first in (a, b) order is reported; two symbols of equal
    64-bit |s| at the list's end: the smaller k is in; saturated bytes: the ranking needs all 64 bits."""
    _check((RP.rank_edge_launch(), RP.strong_wrong_launch(), RP.alias_pair_launch()[0], RP.rank_tie_launch()[0], RP.saturated_launch()))


def test_the_runs_winner_and_the_seam():
    """(flips ascending, margin descending, tau ascending): an exact packet beats a louder damaged one, one flip beats
    two louder ones, of two identical damaged copies the earlier; the damaged packet reached by the look-back has
    flags = 3."""
    first, back, *_ = RP.seam_launches()
    _check((RP.winner_launch(), first, back))


def test_the_longest_region_with_repair_on():
    """SL 25, 32 + 16 windows: s and the bytes fill 60 KiB of LDS, the syndrome table lies beside them."""
    _check((RP.longest_launch(),))


@pytest.mark.parametrize("n", [40, 64, 80])
def test_packet_shapes(n):
    _check(tuple(RP.grid_launch(n, sl) for m, sl in RP.GRID if m == n))


def test_hook_without_repair_equals_the_hook_before_it():
    """rd_debug_burst_decode_repair at max_flips = 0 against rd_debug_burst_decode on every crafted launch of the decode
    tests: the same slot, byte for byte - and that slot is the model's."""
    _lib = _lib_with_device()
    for L in DC.hook_launches():
        a, b = _run(_lib, L, 0), _run(_lib, L, None)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), L.name
        assert a[0].tobytes() == L.msgs.tobytes() and np.array_equal(a[1], L.n_msgs), L.name


# ------------------------------------------------------------------------------------------ through a receiver
def _stream(bs, repair):
    """The capture in chunks of bs through a receiver with decode on and set_burst_repair(repair) (None: never called):
    (cfg, thr, blocks, bursts, messages) per chunk from a reset, thresholds at 4 x the floor of the quiet first chunk."""
    w = DC.device_receiver(bs, 8, offsets_hz=DC.S8_OFFSETS_HZ)
    chunks = DC.chunks_of(RP.cap_capture(), bs)
    w.set_bursts(True)
    w.set_burst_decode(True)
    if repair is not None:
        w.set_burst_repair(repair)
    w.demodulate(chunks[0])
    thr = acquire.Acquisition(3, w.cfg).thresholds(w.bursts().floor).astype(np.uint64)
    w.reset()                                                 # (keeps decode and repair)
    assert w.burst_repair() == (repair or 0)
    w.set_burst_threshold(thr)
    blocks, bursts, got = [], [], []
    for chunk in chunks:
        w.demodulate(chunk)
        blocks.append(w.channelized())
        bursts.append(w.bursts())
        got.append(w.burst_messages())
    return w.cfg, thr, blocks, bursts, got


@pytest.mark.parametrize("bs", RP.CAP_BS)
def test_receiver_with_repair_equals_the_stream_model(bs):
    """Six bursts on three channels: one weak wrong symbol (twice), two of them, a strong one, a wrong sync symbol, and an
    undamaged packet.  burst_messages() at max_flips = 2 equals the stream model (steps 1 .. 7) of the receiver's own
    bytes and burst records, chunk by chunk, and a second run gives the same bits; repaired rows of one and of two flips
    are among them, each with a planted payload; with repair never switched on, the same capture gives the model at
    max_flips = 0: pad all zero, bit 1 clear."""
    _lib_with_device()
    cfg, thr, blocks, bursts, got = _stream(bs, 2)
    want = RP.decode_stream(blocks, thr, cfg, 2, bursts=bursts)
    for g, (_, m) in zip(got, want):
        DC.assert_equals_model(g, m)
    rows = np.concatenate([g.records for g in got])
    flips = sorted(len(acquire.flipped_symbols(r)) for r in rows)
    print(f"\n[receiver, chunks of {bs}] flips per row {flips}, planted " + str([bytes(r['data']) in RP.cap_packets() for r in rows]))
    assert {0, 1, 2} <= set(flips) and all(bytes(r["data"]) in RP.cap_packets() for r in rows)
    assert np.array_equal(acquire.repaired(rows), [len(acquire.flipped_symbols(r)) > 0 for r in rows])
    again = _stream(bs, 2)
    assert all(np.array_equal(a, b) for a, b in zip(again[2], blocks))
    assert [g.records.tobytes() for g in again[4]] == [g.records.tobytes() for g in got]
    # never switched on
    cfg, thr0, blocks0, bursts0, got0 = _stream(bs, None)
    assert np.array_equal(thr0, thr) and all(np.array_equal(a, b) for a, b in zip(blocks0, blocks))
    want0 = DC.decode_stream(blocks0, thr0, cfg, bursts=bursts0)
    for g, (_, m) in zip(got0, want0):
        DC.assert_equals_model(g, m)
    rows0 = np.concatenate([g.records for g in got0])
    assert rows0.size < rows.size and not rows0["pad"].any() and not acquire.repaired(rows0).any()
    assert [r.tobytes() for r in rows if not acquire.repaired(np.asarray([r]))[0]] == [r.tobytes() for r in rows0]


def test_state_rules_and_acquisition():
    _lib = _lib_with_device()
    bs = RP.CAP_BS[0]
    w = DC.device_receiver(bs, 8, offsets_hz=DC.S8_OFFSETS_HZ)
    chunks = DC.chunks_of(RP.cap_capture(), bs)
    w.set_bursts(True)
    with pytest.raises(RuntimeError):
        w.set_burst_repair(1)                                # decode is off
    assert "decode" in _lib.last_error() and w.burst_repair() == 0
    w.set_burst_decode(True)
    w.set_burst_repair(1)
    w.submit(chunks[0])
    with pytest.raises(RuntimeError):
        w.set_burst_repair(2)                                # a chunk in flight
    assert "in flight" in _lib.last_error() and w.burst_repair() == 1
    w.fetch()
    w.set_burst_repair(2)
    w.reset()
    assert w.burst_repair() == 2                             # reset() keeps it
    w.set_burst_decode(False)
    assert w.burst_repair() == 0                             # decode off puts it back
    w.set_burst_decode(True)
    assert w.burst_repair() == 0
    w.set_burst_repair(2)
    w.set_bursts(False)
    assert w.burst_repair() == 0
    for bad in (-1, 3, True):
        with pytest.raises(ValueError):
            w.set_burst_repair(bad)
    # Acquisition: a chunk whose only rows are repaired ones proposes nothing unless asked to use them
    cfg, thr, blocks, bursts, got = _stream(bs, 2)
    k = next(j for j, g in enumerate(got) if g.records.size and acquire.repaired(g.records).all())
    assert acquire.Acquisition(3, cfg).update(bursts[k], [], k + 1, got[k]) is None
    new = acquire.Acquisition(3, cfg, use_repaired=True).update(bursts[k], [], k + 1, got[k])
    assert isinstance(new, int)
    hz = [h for c, _, h, _ in RP.CAP_BURSTS if c == int(got[k].records[0]["channel"])][0]
    print(f"\n[acquisition from a repaired row] proposed {new} Hz, planted {hz} Hz")
    assert abs(new - hz) <= 1500
