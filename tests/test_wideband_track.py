"""WidebandReceiver.set_burst_expect / expected_messages and track.Tracker on the device: the small receiver of
burst_decode_cases.device_receiver (decim 4, "s16", three channels) at block_size 1152 and 2048.  With the thresholds left
at their default nothing is ON and burst_messages() is empty, while expected_messages() equals the model of
tests/burst_track_cases.py on the receiver's own channelized bytes, chunk by chunk; a table set with two chunks in flight
takes force at the right chunk; reset and switching decode or bursts off clear the table; and a short Tracker loop on a
station that hops a made-up three-channel pattern receives every planted packet, counts the omitted one as missed and
picks the station up again at the following hop."""
import functools

import numpy as np
import pytest

import burst_decode_cases as DC
import burst_track_cases as TK
from rtldavis_amd import acquire, synth, track
from rtldavis_amd.wideband import BURST_MSG_DTYPE, BURST_THRESHOLD_OFF

pytestmark = pytest.mark.gpu

OUT_RATE = 19200 * 14
IF_HZ = -OUT_RATE // 4
FIRST_SYMBOL_END = 32 * 14 + 14 - 1 + DC.SEAM_LAG            # from a burst's first output to the end of its packet's first symbol


def _table(half=50):
    """One expectation per valid burst of burst_decode_cases.DEV_BURSTS (the twin has none), +-half outputs around the end
    of its first symbol, at the carrier it was planted at."""
    rows = []
    for c, payload, start in DC.DEV_BURSTS:
        if payload == DC.TWIN:
            continue
        t = start + FIRST_SYMBOL_END
        rows.append(TK.expect_row(c, t - half, t + half, TK.corr_of((IF_HZ + DC.DEV_PLANTED[c]) / OUT_RATE)))
    return TK.table(rows)


def _stream(bs, tab, repair=0, narrow=False):
    """(blocks, [ExpectedMessages], [BurstMessages]) of the device capture streamed at block size bs under one table."""
    _, stream = DC.device_capture()
    rx = DC.device_receiver(bs)
    rx.set_bursts(True)
    rx.set_burst_decode(True)
    if repair:
        rx.set_burst_repair(repair)
    if narrow:
        rx.set_burst_narrow(True)
    blocks, got, runs = [], [], []
    for chunk in DC.chunks_of(stream, bs):
        rx.set_burst_expect(tab)
        rx.demodulate(chunk)
        blocks.append(rx.channelized())
        got.append(rx.expected_messages())
        runs.append(rx.burst_messages())
    return rx, blocks, got, runs


@functools.lru_cache(maxsize=None)
def _streamed(bs, repair, narrow):
    return _stream(bs, _table(), repair, narrow)[1:]


def _assert_equal(got, want):
    assert got.chunk == want.chunk and np.array_equal(got.candidates, want.candidates), (got.chunk, got.candidates, want.candidates)
    assert got.records.dtype == BURST_MSG_DTYPE and got.records.shape == want.records.shape, (got.chunk, got.records, want.records)
    for f in BURST_MSG_DTYPE.names:
        assert np.array_equal(got.records[f], want.records[f]), (got.chunk, f, got.records[f], want.records[f])


@pytest.mark.parametrize("bs", [1152, 2048])
@pytest.mark.parametrize("repair,narrow", [(0, False), (2, True)])
def test_expected_messages_equal_the_model_with_every_threshold_off(bs, repair, narrow):
    blocks, got, runs = _streamed(bs, repair, narrow)
    cfg = DC.device_receiver(bs).cfg
    want = TK.expect_stream(blocks, [_table()] * len(blocks), cfg, repair, narrow)
    for g, w, r in zip(got, want, runs):
        _assert_equal(g, w)
        assert r.records.size == 0                            # no run anywhere: the run-driven path reports nothing
        assert acquire.expected(g.records).all()
    found = {(int(r["first"]), bytes(r["data"])) for g in got for r in g.records}
    valid = [bytes.fromhex(p) for _, p, _ in DC.DEV_BURSTS if p != DC.TWIN]
    assert found == {(i, d) for i, d in enumerate(valid)}     # every planted packet, at its own expectation, once


def test_both_block_sizes_give_the_same_messages():
    sets = []
    for bs in (1152, 2048):
        _, got, _ = _streamed(bs, 0, False)
        sets.append({(int(r["channel"]), int(r["time"]), bytes(r["data"])) for g in got for r in g.records})
    assert sets[0] == sets[1] and len(sets[0]) == 4


def test_a_table_set_with_two_chunks_in_flight_holds_from_the_next_submit():
    bs = 2048
    _, stream = DC.device_capture()
    chunks = DC.chunks_of(stream, bs)
    rx = DC.device_receiver(bs)
    rx.set_bursts(True)
    rx.set_burst_decode(True)
    tab = _table(half=300)                                    # (channel 0's first packet ends in chunk 0)
    rx.submit(chunks[0])
    rx.submit(chunks[1])
    rx.set_burst_expect(tab[:1])                              # collapses into the next call
    rx.set_burst_expect(tab)
    assert rx.burst_expect().tobytes() == tab.tobytes()
    blocks, got = [], []
    for k in range(2, 5):
        rx.fetch()
        blocks.append(rx.channelized())
        got.append(rx.expected_messages())
        rx.submit(chunks[k])
    for _ in range(2):
        rx.fetch()
        blocks.append(rx.channelized())
        got.append(rx.expected_messages())
    assert [g.chunk for g in got] == [0, 1, 2, 3, 4]
    assert got[0].candidates.size == 0 == got[1].candidates.size and got[0].records.size == 0 == got[1].records.size
    want = TK.expect_stream(blocks, [tab[:0], tab[:0], tab, tab, tab], rx.cfg, 0, False)
    for g, w in zip(got[2:], want[2:]):
        _assert_equal(g, w)
    assert sum(g.records.size for g in got) >= 1 and all(g.candidates.size == tab.size for g in got[2:])
    rx.reset()                                                # the clock restarts: the table goes
    assert rx.burst_expect().size == 0
    rx.set_burst_expect(tab)
    rx.set_burst_decode(False)
    assert rx.burst_expect().size == 0
    rx.set_burst_decode(True)
    rx.set_burst_expect(tab)
    rx.set_bursts(False)
    assert rx.burst_expect().size == 0


# ------------------------------------------------------------------------------------------ a station that hops
HOP_BS = 2048
HOP_FIRST, HOP_PERIOD, HOP_PACKETS, HOP_OMIT = 2448, 2500, 6, 3
HOP_OFFSET_HZ = 20000


@functools.lru_cache(maxsize=None)
def _hop_capture():
    """DEV_OUTPUTS outputs: one station (one payload, so one id) that sends every HOP_PERIOD outputs on the next channel
    of TK.TRACK_PATTERN, 20 kHz above each channel's centre; packet HOP_OMIT is left out."""
    plan = [(j, TK.TRACK_PATTERN[j % 3], HOP_FIRST + j * HOP_PERIOD) for j in range(HOP_PACKETS) if j != HOP_OMIT]
    pieces, at = [], 0
    n_out = 2 * synth.BLOCK_SIZE + DC.BURST_OUTPUTS + 2048     # (burst_decode_cases._piece's)
    for i, (j, c, s) in enumerate(plan):
        end = DC.DEV_OUTPUTS if i + 1 == len(plan) else (s + DC.BURST_OUTPUTS + plan[i + 1][2]) // 2
        seed = next(q for q in range(300 + 40 * j, 340 + 40 * j) if abs(DC.drawn_cfo(q, n_out)) < 400.0)   # a transmitter's carrier stays put
        pieces.append(DC._piece(seed, DC.DEV_OFFSETS_HZ[c] + HOP_OFFSET_HZ, DC.VALID[1], s - at, end - s - DC.BURST_OUTPUTS))
        at = end
    stream = np.concatenate(pieces)
    assert stream.size == 2 * DC.DEV_DECIM * DC.DEV_OUTPUTS
    return plan, stream


def test_tracker_follows_a_hopping_station_and_counts_the_missed_packet():
    plan, stream = _hop_capture()
    rx = DC.device_receiver(HOP_BS)
    rx.set_bursts(True)
    rx.set_burst_decode(True)
    acq = acquire.Acquisition(rx.n_channels, rx.cfg, factor=4)
    trk = track.Tracker(rx.cfg, TK.TRACK_PATTERN, period_outputs=HOP_PERIOD)
    clock, by_run, by_expectation = 0, [], []
    for k, chunk in enumerate(DC.chunks_of(stream, HOP_BS)):
        rx.set_burst_expect(trk.table(clock, HOP_BS))
        rx.demodulate(chunk)
        clock += HOP_BS
        if not trk.stats():                                   # until the station has been heard once: runs at 4 x floor
            rx.set_burst_threshold(acq.thresholds(rx.bursts().floor))
        m, x = rx.burst_messages(), rx.expected_messages()
        trk.observe(m.records)
        trk.observe(x.records)
        by_run += list(m.records)
        by_expectation += list(x.records)
        if trk.stats():                                       # heard: from here on the expectations alone
            rx.set_burst_threshold(BURST_THRESHOLD_OFF)
    data = bytes.fromhex(DC.VALID[1])
    assert len(by_run) == 1 and all(bytes(r["data"]) == data for r in by_run + by_expectation)
    ident = int(by_run[0]["id"])
    times = [int(by_run[0]["time"])] + [int(r["time"]) for r in by_expectation]
    want = [s + FIRST_SYMBOL_END for _, _, s in plan]
    assert len(times) == len(want) and all(abs(a - b) <= 14 for a, b in zip(times, want)), (times, want)
    assert [int(r["channel"]) for r in by_run + by_expectation] == [c for _, c, _ in plan]
    assert trk.stats() == {ident: {"received": HOP_PACKETS - 1, "missed": 1, "lost": 0}}
    assert abs(trk.stations()[ident][3] - HOP_OFFSET_HZ) < 1500
