"""WidebandReceiver.set_burst_quality / burst_message_quality / expected_message_quality on the device: the small receiver
of burst_decode_cases.device_receiver (decim 4, "s16", three channels) on device_capture and seam_capture.  The quality
rows are parallel to burst_messages() and expected_messages() and equal the model of tests/burst_quality_cases.py on the
receiver's own channelized bytes of consecutive chunks; a record that step 7 drops at a seam takes its quality row with it;
two chunks in flight, repair and the narrow decoder, and a noise gap changed between chunks change nothing but what the
definition says; the state rules hold; and with quality off the receiver hands out what one that never heard of it does."""
import functools

import numpy as np
import pytest

import burst_decode_cases as DC
import burst_quality_cases as QC
import burst_track_cases as TK
from rtldavis_amd import acquire, wideband
from rtldavis_amd.wideband import QUALITY_DTYPE

pytestmark = pytest.mark.gpu

OUT_RATE = 19200 * 14
IF_HZ = -OUT_RATE // 4
FIRST_SYMBOL_END = 32 * 14 + 14 - 1 + DC.SEAM_LAG            # from a burst's first output to the end of its packet's first symbol


def _table(half=50):
    """One expectation per valid burst of burst_decode_cases.DEV_BURSTS, +-half outputs around the end of its first symbol."""
    rows = []
    for c, payload, start in DC.DEV_BURSTS:
        if payload != DC.TWIN:
            t = start + FIRST_SYMBOL_END
            rows.append(TK.expect_row(c, t - half, t + half, TK.corr_of((IF_HZ + DC.DEV_PLANTED[c]) / OUT_RATE)))
    return TK.table(rows)


@functools.lru_cache(maxsize=None)
def _thresholds(bs):
    from rtldavis_amd import _lib
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    w = DC.device_receiver(bs)
    w.set_bursts(True)
    quiet, _ = DC.device_capture()
    w.demodulate(quiet[: 2 * DC.DEV_DECIM * bs])
    return acquire.Acquisition(3, w.cfg).thresholds(w.bursts().floor).astype(np.uint64)


def _receiver(bs, repair=0, narrow=False, quality=None):
    rx = DC.device_receiver(bs)
    rx.set_bursts(True)
    rx.set_burst_decode(True)
    rx.set_burst_threshold(_thresholds(bs))
    if repair:
        rx.set_burst_repair(repair)
    if narrow:
        rx.set_burst_narrow(True)
    if quality is not None:
        rx.set_burst_quality(True, quality)
    return rx


def _take(rx, quality=True):
    """What the last fetch left: (channelized bytes, Bursts, BurstMessages, ExpectedMessages, quality rows of both)."""
    q = (rx.burst_message_quality(), rx.expected_message_quality()) if quality else (None, None)
    return (rx.channelized(), rx.bursts(), rx.burst_messages(), rx.expected_messages()) + q


def _stream(rx, chunks, tab, gaps=None, quality=True):
    out = []
    for k, chunk in enumerate(chunks):
        if gaps is not None:
            rx.set_burst_quality(True, gaps[k])                  # (quiet: the chunk before has been fetched)
        rx.set_burst_expect(tab)
        packets = rx.demodulate(chunk)
        out.append(_take(rx, quality) + (packets,))
    return out


def _assert_rows(run, cfg, gaps):
    """Every chunk's quality rows are parallel to its message rows and equal the model on the receiver's own bytes."""
    prev, n_rows, n_inband = None, [0, 0], 0
    for k, (block, _, m, x, qm, qx, _) in enumerate(run):
        for j, (recs, got) in enumerate(((m.records, qm), (x.records, qx))):
            assert got.dtype == QUALITY_DTYPE and got.shape == recs.shape, (k, j, got.shape, recs.shape)
            want = QC.quality_rows(block, prev, cfg, recs, gaps[k], k)
            for f in QUALITY_DTYPE.names:
                assert np.array_equal(got[f], want[f]), (k, ("burst", "expected")[j], f, got[f], want[f])
            n_rows[j] += got.size
            n_inband += int((got["flags"] == QC.INBAND).sum())
        prev = block
    return n_rows, n_inband


@pytest.mark.parametrize("bs", [1152, 2048])
@pytest.mark.parametrize("repair,narrow", [(0, False), (2, True)])
def test_rows_are_parallel_and_equal_the_model(bs, repair, narrow):
    _, stream = DC.device_capture()
    chunks = DC.chunks_of(stream, bs)
    rx = _receiver(bs, repair, narrow, quality=0)
    run = _stream(rx, chunks, _table())
    n_rows, n_inband = _assert_rows(run, rx.cfg, [0] * len(chunks))
    print(f"\n[quality bs {bs} repair {repair} narrow {narrow}] rows: {n_rows[0]} burst, {n_rows[1]} expected")
    assert n_rows[0] >= 3 and n_rows[1] >= 4 and n_inband == sum(n_rows)          # the planted packets, by either path
    # the decoders' own choices (repair, narrow) reach the quality row through the record's (tau, f) alone
    for _, _, m, x, qm, qx, _ in run:
        for recs, q in ((m.records, qm), (x.records, qx)):
            for r, row in zip(recs, q):
                assert int(row["g"]) == QC.NB.grid_choice(r["f_re"], r["f_im"], 14)[3] and int(row["chunk"]) == m.chunk
    # and the figures are sane: a planted burst stands well above the quiet in front of it
    first = next(q for _, _, _, _, _, q, _ in run if q.size)[0]
    assert acquire.rssi_db(first, 14) < 0 and np.isfinite(acquire.snr_db(first, 14)) and np.isfinite(acquire.snr_inband_db(first, 14))


def test_a_record_dropped_at_the_seam_takes_its_quality_row_with_it():
    bs, sl = DC.SEAM_BS, DC.SEAM_SL
    rx = _receiver(bs, quality=0)
    thr = _thresholds(bs)
    payload = DC.VALID[1]
    dropped = 0
    for j in range(2 * sl + 1):
        chunks = DC.chunks_of(DC.seam_capture(j, True), bs)
        rx.reset()
        rx.set_burst_threshold(thr)
        run = _stream(rx, chunks, TK.table([]))
        _assert_rows(run, rx.cfg, [0] * len(chunks))
        plain = [DC.decode_model(run[k][0], run[k - 1][0] if k else None, run[k][1], rx.cfg, k >= 1, k * bs) for k in range(len(run))]
        before = sum(bytes(r["data"]).hex() == payload for m in plain for r in m.records)
        after = sum(bytes(r["data"]).hex() == payload for r_ in run for r in r_[2].records)
        assert after == 1 and sum(r_[4].size for r_ in run) == sum(r_[2].records.size for r_ in run)
        dropped += before - after
    assert dropped >= 1                                           # the sweep covers a seam at which step 7 drops a record


def test_two_chunks_in_flight_give_the_same_rows():
    bs = 2048
    _, stream = DC.device_capture()
    chunks = DC.chunks_of(stream, bs)
    tab = _table()
    rx = _receiver(bs, quality=16)
    one = _stream(rx, chunks, tab)
    rx.reset()
    rx.set_burst_threshold(_thresholds(bs))
    assert rx.burst_quality() == (True, 16)
    rx.set_burst_expect(tab)
    got = []
    rx.submit(chunks[0])
    for k in range(1, len(chunks)):
        rx.submit(chunks[k])
        with pytest.raises(RuntimeError):
            rx.set_burst_quality(True, 0)                         # not quiet
        rx.fetch()
        got.append(_take(rx))
    rx.fetch()
    got.append(_take(rx))
    assert len(got) == len(one)
    for a, b in zip(one, got):
        for i in (2, 3):
            assert a[i].records.tobytes() == b[i].records.tobytes() and a[i].chunk == b[i].chunk
        assert a[4].tobytes() == b[4].tobytes() and a[5].tobytes() == b[5].tobytes()
    _assert_rows([g + (None,) for g in got], rx.cfg, [16] * len(chunks))


def test_a_noise_gap_changed_between_chunks_holds_for_the_chunks_submitted_after_it():
    bs = 1152
    _, stream = DC.device_capture()
    chunks = DC.chunks_of(stream, bs)
    gaps = [(0, 40, 1024, 7, 300)[k % 5] for k in range(len(chunks))]
    rx = _receiver(bs, quality=0)
    run = _stream(rx, chunks, _table(), gaps=gaps)
    n_rows, _ = _assert_rows(run, rx.cfg, gaps)
    assert sum(n_rows) >= 7
    # some rows come from chunks with a gap, and there the gap shows: the model at gap 0 gives another noise sum
    moved, prev = 0, None
    for k, (block, _, m, x, qm, qx, _) in enumerate(run):
        for recs, got in ((m.records, qm), (x.records, qx)):
            if gaps[k] and got.size:
                moved += int((QC.quality_rows(block, prev, rx.cfg, recs, 0, k)["noise"] != got["noise"]).sum())
        prev = block
    assert moved >= 2


def test_state_rules():
    bs = 2048
    _, stream = DC.device_capture()
    chunks = DC.chunks_of(stream, bs)
    rx = _receiver(bs)
    assert rx.burst_quality() == (False, 0)
    rx.demodulate(chunks[0])
    for fn in (rx.burst_message_quality, rx.expected_message_quality):
        with pytest.raises(RuntimeError, match="quality off"):
            fn()                                                  # the chunk was submitted with quality off
    rx.submit(chunks[1])
    with pytest.raises(RuntimeError, match="in flight"):
        rx.set_burst_quality(True)
    rx.fetch()
    rx.set_burst_quality(True, 12)
    with pytest.raises(RuntimeError):
        rx.burst_message_quality()                                # still the chunk fetched last: quality was off for it
    rx.demodulate(chunks[2])
    assert rx.burst_message_quality().shape == rx.burst_messages().records.shape
    assert rx.expected_message_quality().size == 0                # no table
    rx.reset()
    assert rx.burst_quality() == (True, 12)
    with pytest.raises(RuntimeError):
        rx.burst_message_quality()                                # no chunk fetched since the reset
    rx.set_burst_decode(False)
    assert rx.burst_quality()[0] is False
    with pytest.raises(RuntimeError):
        rx.set_burst_quality(True)                                # decode is off
    rx.set_burst_decode(True)
    rx.set_burst_quality(True)
    rx.set_bursts(False)
    assert rx.burst_quality()[0] is False
    with pytest.raises(ValueError):
        rx.set_burst_quality(True, wideband.QUALITY_MAX_GAP + 1)


def test_quality_off_is_the_receiver_that_never_heard_of_it():
    bs = 2048
    _, stream = DC.device_capture()
    chunks = DC.chunks_of(stream, bs)
    tab = _table()
    plain = _receiver(bs, repair=1, narrow=True)
    a = _stream(plain, chunks, tab, quality=False)
    rx = _receiver(bs, repair=1, narrow=True, quality=5)
    rx.set_burst_expect(tab)
    rx.demodulate(chunks[0])
    assert rx.burst_message_quality().shape == rx.burst_messages().records.shape
    rx.set_burst_quality(False)
    rx.reset()
    rx.set_burst_threshold(_thresholds(bs))
    b = _stream(rx, chunks, tab, quality=False)
    with pytest.raises(RuntimeError):
        rx.burst_message_quality()
    for k, (x, y) in enumerate(zip(a, b)):
        assert x[0].tobytes() == y[0].tobytes(), k
        assert x[1].records.tobytes() == y[1].records.tobytes() and x[1].floor.tobytes() == y[1].floor.tobytes(), k
        assert x[2].records.tobytes() == y[2].records.tobytes() and x[2].long_runs.tobytes() == y[2].long_runs.tobytes(), k
        assert x[3].records.tobytes() == y[3].records.tobytes() and x[3].candidates.tobytes() == y[3].candidates.tobytes(), k
        assert [[(p.index, bytes(p.data), p.rssi, p.snr) for p in ch] for ch in x[6]] == [[(p.index, bytes(p.data), p.rssi, p.snr) for p in ch] for ch in y[6]], k
    assert sum(x[2].records.size for x in a) >= 3 and sum(x[3].records.size for x in a) >= 4
