"""WidebandReceiver.set_burst_search / searched_messages and track.Tracker's provisional stations on the device: the small
receiver of burst_decode_cases.device_receiver (decim 4, "s16", three channels) at block_size 1152 and 2048.  With every
threshold left off nothing is ON and burst_messages() is empty, while searched_messages() equals the model of
tests/burst_search_cases.py on the receiver's own channelized bytes, chunk by chunk, and holds every valid planted
packet; a list set with two chunks in flight takes force at the right chunk; an empty list changes nothing; and a
Tracker fed searched and expected rows alone seeds, confirms and follows a hopping station."""
import functools

import numpy as np
import pytest

import burst_decode_cases as DC
import burst_search_cases as SC
import burst_track_cases as TK
import test_wideband_track as WT
from rtldavis_amd import acquire, track
from rtldavis_amd.wideband import BURST_MSG_DTYPE

pytestmark = pytest.mark.gpu

OUT_RATE = 19200 * 14


def _centres():
    return acquire.search_centres(DC.DEV_PLANTED, OUT_RATE)


@functools.lru_cache(maxsize=None)
def _streamed(bs):
    """(cfg, blocks, [SearchedMessages], [BurstMessages]) of the device capture streamed at block size bs."""
    _, stream = DC.device_capture()
    rx = DC.device_receiver(bs)
    rx.set_bursts(True)
    rx.set_burst_decode(True)
    rx.set_burst_search(_centres())
    blocks, got, runs = [], [], []
    for chunk in DC.chunks_of(stream, bs):
        rx.demodulate(chunk)
        blocks.append(rx.channelized())
        got.append(rx.searched_messages())
        runs.append(rx.burst_messages())
    return rx.cfg, blocks, got, runs


def _assert_equal(got, want):
    assert got.chunk == want.chunk, (got.chunk, want.chunk)
    assert np.array_equal(got.sync_hits, want.sync_hits) and got.sync_hits.shape == want.sync_hits.shape, (got.chunk, got.sync_hits, want.sync_hits)
    assert np.array_equal(got.dropped, want.dropped) and got.dropped.shape == want.dropped.shape, (got.chunk, got.dropped, want.dropped)
    assert got.records.dtype == BURST_MSG_DTYPE and got.records.shape == want.records.shape, (got.chunk, got.records, want.records)
    for f in BURST_MSG_DTYPE.names:
        assert np.array_equal(got.records[f], want.records[f]), (got.chunk, f, got.records[f], want.records[f])


@pytest.mark.parametrize("bs", [1152, 2048])
def test_searched_messages_equal_the_model_with_every_threshold_off(bs):
    cfg, blocks, got, runs = _streamed(bs)
    centres = [int(g) for g in _centres()]
    assert len(centres) == 3
    want = SC.search_stream(blocks, [centres] * len(blocks), cfg)
    for g, w, r in zip(got, want, runs):
        _assert_equal(g, w)
        assert r.records.size == 0                            # no run anywhere: the run-driven path reports nothing
        assert acquire.searched(g.records).all() and acquire.narrowband(g.records).all()
        assert np.all(acquire.search_hits(g.records) >= 1)
    # every valid planted packet once per centre that decodes it - the centre of its own channel's carrier at the least
    found = [(int(r["channel"]), bytes(r["data"]), int(r["pad"][3])) for g in got for r in g.records]
    assert len(found) == len(set(found)), found
    valid = [(c, bytes.fromhex(p)) for c, p, _ in DC.DEV_BURSTS if p != DC.TWIN]
    for c, d in valid:
        assert (c, d, int(acquire.search_centres([DC.DEV_PLANTED[c]], OUT_RATE)[0])) in found, (c, found)
    assert {(c, d) for c, d, _ in found} == set(valid)        # and nothing that was not planted (the twin fails its CRC)


def test_both_block_sizes_give_the_same_messages():
    sets = []
    for bs in (1152, 2048):
        _, _, got, _ = _streamed(bs)
        sets.append({(int(r["channel"]), int(r["time"]), bytes(r["data"]), int(r["pad"][3])) for g in got for r in g.records})
    assert sets[0] == sets[1] and len(sets[0]) >= 4


def test_a_list_set_with_two_chunks_in_flight_holds_from_the_next_submit():
    bs = 2048
    _, stream = DC.device_capture()
    chunks = DC.chunks_of(stream, bs)
    rx = DC.device_receiver(bs)
    with pytest.raises(RuntimeError):
        rx.set_burst_search([5])                              # decode is off
    rx.set_bursts(True)
    rx.set_burst_decode(True)
    centres = [int(g) for g in _centres()]
    rx.submit(chunks[0])
    rx.submit(chunks[1])
    rx.set_burst_search(centres[:1])                          # collapses into the next call
    rx.set_burst_search(centres)
    assert list(rx.burst_search()) == centres
    for bad in ([64], [5, 5], list(range(9)), [-1], [300]):
        with pytest.raises(ValueError):
            rx.set_burst_search(bad)
    assert list(rx.burst_search()) == centres                 # (a refused list changes nothing)
    blocks, got = [], []
    for k in range(2, 5):
        rx.fetch()
        blocks.append(rx.channelized())
        got.append(rx.searched_messages())
        rx.submit(chunks[k])
    for _ in range(2):
        rx.fetch()
        blocks.append(rx.channelized())
        got.append(rx.searched_messages())
    assert [g.chunk for g in got] == [0, 1, 2, 3, 4]
    assert got[0].records.size == 0 == got[1].records.size and got[0].sync_hits.shape == (0, 3) == got[1].sync_hits.shape
    want = SC.search_stream(blocks, [[], [], centres, centres, centres], rx.cfg)
    for g, w in zip(got, want):
        _assert_equal(g, w)
    assert sum(g.records.size for g in got) >= 1 and all(g.sync_hits.shape == (3, 3) for g in got[2:])
    rx.reset()                                                # the list stays
    assert list(rx.burst_search()) == centres
    rx.set_burst_decode(False)
    assert rx.burst_search().size == 0
    rx.set_burst_decode(True)
    rx.set_burst_search(centres)
    rx.set_bursts(False)
    assert rx.burst_search().size == 0


def test_an_empty_list_changes_nothing():
    """A receiver that never called set_burst_search, one that set the empty list, and one that set a list and cleared
    it before the first submit: the same burst and expected messages byte for byte, and no searched row."""
    bs = 2048
    _, stream = DC.device_capture()
    tab = WT._table()
    outs = []
    for mode in range(3):
        rx = DC.device_receiver(bs)
        rx.set_bursts(True)
        rx.set_burst_decode(True)
        rx.set_burst_narrow(True)
        if mode == 1:
            rx.set_burst_search([])
        if mode == 2:
            rx.set_burst_search(_centres())
            rx.set_burst_search([])
        acq = acquire.Acquisition(rx.n_channels, rx.cfg, factor=4)
        seen = []
        for chunk in DC.chunks_of(stream, bs):
            rx.set_burst_expect(tab)
            rx.demodulate(chunk)
            rx.set_burst_threshold(acq.thresholds(rx.bursts().floor))
            s = rx.searched_messages()
            assert s.records.size == 0 and s.sync_hits.shape == (0, 3) and s.dropped.shape == (0, 3)
            m, x = rx.burst_messages(), rx.expected_messages()
            seen.append((m.records.tobytes(), m.long_runs.tobytes(), x.records.tobytes(), x.candidates.tobytes()))
        outs.append(seen)
    assert outs[0] == outs[1] == outs[2]
    assert sum(len(s[2]) for s in outs[0]) > 0                # (the comparison is not one of empty lists)


def test_the_search_beside_every_other_burst_feature():
    """Narrow, repair, quality, thresholds and expectations on: the search equals its model, and switching it on changes
    no byte of what the other paths deliver."""
    bs = 2048
    _, stream = DC.device_capture()
    tab = WT._table()
    centres = [int(g) for g in _centres()]
    outs = []
    for on in (False, True):
        rx = DC.device_receiver(bs)
        rx.set_bursts(True)
        rx.set_burst_decode(True)
        rx.set_burst_narrow(True)
        rx.set_burst_repair(2)
        rx.set_burst_quality(True)
        if on:
            rx.set_burst_search(centres)
        acq = acquire.Acquisition(rx.n_channels, rx.cfg, factor=4)
        seen, blocks, got = [], [], []
        for chunk in DC.chunks_of(stream, bs):
            rx.set_burst_expect(tab)
            rx.demodulate(chunk)
            rx.set_burst_threshold(acq.thresholds(rx.bursts().floor))
            m, x = rx.burst_messages(), rx.expected_messages()
            seen.append((m.records.tobytes(), x.records.tobytes(), x.candidates.tobytes(), rx.burst_message_quality().tobytes(),
                         rx.expected_message_quality().tobytes()))
            blocks.append(rx.channelized())
            got.append(rx.searched_messages())
        outs.append(seen)
        if on:
            for g, w in zip(got, SC.search_stream(blocks, [centres] * len(blocks), rx.cfg)):
                _assert_equal(g, w)
            assert sum(g.records.size for g in got) >= 4
    assert outs[0] == outs[1]


def test_tracker_seeds_confirms_and_follows_a_station_from_searched_rows_alone():
    """No threshold is ever set: the first packet is found by the search and seeds a provisional station, the second is
    decoded at its expectation and promotes it, the omitted one is counted as missed, and the rest follow."""
    plan, stream = WT._hop_capture()
    rx = DC.device_receiver(WT.HOP_BS)
    rx.set_bursts(True)
    rx.set_burst_decode(True)
    rx.set_burst_search(acquire.search_centres([WT.HOP_OFFSET_HZ], OUT_RATE))
    trk = track.Tracker(rx.cfg, TK.TRACK_PATTERN, period_outputs=WT.HOP_PERIOD)
    clock, by_search, by_expectation, provisional = 0, [], [], []
    for chunk in DC.chunks_of(stream, WT.HOP_BS):
        rx.set_burst_expect(trk.table(clock, WT.HOP_BS))
        rx.demodulate(chunk)
        clock += WT.HOP_BS
        assert rx.burst_messages().records.size == 0
        s, x = rx.searched_messages(), rx.expected_messages()
        trk.observe(s)
        trk.observe(x)
        by_search += list(s.records)
        by_expectation += list(x.records)
        provisional.append(trk.provisional())
    data = bytes.fromhex(DC.VALID[1])
    assert all(bytes(r["data"]) == data for r in by_search + by_expectation)
    ident = int(by_search[0]["id"])
    want = [s + WT.FIRST_SYMBOL_END for _, _, s in plan]
    assert len(by_search) == len(plan) and all(abs(int(r["time"]) - t) <= 14 for r, t in zip(by_search, want))
    assert len(by_expectation) == len(plan) - 1 and all(abs(int(r["time"]) - t) <= 14 for r, t in zip(by_expectation, want[1:]))
    assert [ident] in provisional and provisional[-1] == []
    assert trk.search_stats() == {"seeded": 1, "promoted": 1, "expired": 0, "ignored": len(plan) - 1}
    assert trk.stats() == {ident: {"received": len(plan) - 1, "missed": 1, "lost": 0}}
    assert abs(trk.stations()[ident][3] - WT.HOP_OFFSET_HZ) < 1500
