"""WidebandReceiver.set_burst_clips / burst_clips on the device: the small receiver of burst_decode_cases.device_receiver
(decim 4, "s16", three channels) on device_capture and seam_capture, with thresholds, decode, an expectation table and one
search centre in force, as tests/test_wideband_quality.py and tests/test_wideband_search.py build them.

Truth without the model: every clip's bytes are the slice [time, time + n) of the receiver's own channelized() blocks laid
end to end.  Then the records against the model of tests/burst_clip_cases.py on those blocks; every message row and every
run has its clip; the stitched recordings hold every planted burst; two chunks in flight, settings changed between chunks
and reset() do what the definition says; and every other accessor is untouched by clips.

Condition, not a measurement: these tests assume nothing was dropped, so the quota (8192) is checked on the MODEL - its
`dropped` is 0 on these captures - before the device is compared to it."""
import functools

import numpy as np
import pytest

import burst_clip_cases as CC
import burst_decode_cases as DC
import burst_search_cases as SC
import burst_track_cases as TK
import test_wideband_quality as WQ
from rtldavis_amd import acquire, clips
from rtldavis_amd.wideband import BURST_MSG_DTYPE, CLIP_DTYPE

pytestmark = pytest.mark.gpu

SL, N = 14, 80
DEFAULT = (CC.RUNS | CC.MESSAGES, 256, 128, 8192)


def _centres():
    return [int(g) for g in acquire.search_centres(DC.DEV_PLANTED, WQ.OUT_RATE)[:1]]


def _receiver(bs, settings=DEFAULT):
    rx = WQ._receiver(bs)
    rx.set_burst_search(_centres())
    if settings is not None and settings[0]:
        rx.set_burst_clips(*settings)
    return rx


def _take(rx, clips_on=True):
    if not clips_on:
        with pytest.raises(RuntimeError, match="clips off"):
            rx.burst_clips()                                       # the chunk was submitted with clips off
    return dict(block=rx.channelized(), bursts=rx.bursts(), msgs=rx.burst_messages(), expected=rx.expected_messages(),
                searched=rx.searched_messages(), clips=rx.burst_clips() if clips_on else None)


def _stream(rx, chunks, tab, settings=None):
    """One chunk at a time; settings: None, or per chunk what set_burst_clips gets before it is submitted."""
    out = []
    for k, chunk in enumerate(chunks):
        if settings is not None:
            rx.set_burst_clips(*settings[k])
        rx.set_burst_expect(tab)
        packets = rx.demodulate(chunk)
        got = _take(rx, settings is None or bool(settings[k][0]))
        got["packets"] = packets
        out.append(got)
    return out


@functools.lru_cache(maxsize=None)
def _streamed(bs):
    _, stream = DC.device_capture()
    rx = _receiver(bs)
    return rx.cfg, _stream(rx, DC.chunks_of(stream, bs), WQ._table())


def _rows(items):
    return np.asarray(list(items), BURST_MSG_DTYPE).reshape(-1)


def _model(cfg, run, tab, centres, settings):
    """burst_clip_cases.stream_model on the receiver's own blocks and runs, with the rows the kernels wrote - the models of
    the decode, expect and search cases BEFORE the host's steps 7 / 7' / 7s."""
    bs = int(cfg.block_size)
    blocks = [g["block"] for g in run]
    dec, exp, sea = [], [], []
    for k, g in enumerate(run):
        prev = blocks[k - 1] if k else None
        dec.append(DC.decode_model(g["block"], prev, g["bursts"], cfg, k >= 1, k * bs).records)
        exp.append(_rows(r[1] for r in TK.decode_chunk(g["block"], prev, tab, cfg, k >= 1, k * bs, 0, False) if r is not None and r[1] is not None))
        sea.append(SC.chunk_records(SC.search_chunk(g["block"], prev, centres, cfg, k >= 1, k * bs)))
    want = CC.stream_model(blocks, cfg, settings, [g["bursts"].records for g in run], dec, exp, sea)
    return want, dec, exp, sea


def _assert_equals_model(run, want):
    n = 0
    for k, (g, w) in enumerate(zip(run, want)):
        if w is None:
            assert g["clips"] is None
            continue
        recs, data, dropped, _ = w
        assert not dropped.any(), (k, dropped)                    # the condition: the MODEL drops nothing at this quota
        got = g["clips"]
        assert got.chunk == k and got.records.dtype == CLIP_DTYPE and got.records.shape == recs.shape, (k, got.records, recs)
        for f in CLIP_DTYPE.names:
            assert np.array_equal(got.records[f], recs[f]), (k, f, got.records[f], recs[f])
        assert np.array_equal(got.dropped, dropped) and got.iq.tobytes() == data.tobytes(), k
        n += recs.size
    return n


@pytest.mark.parametrize("bs", [1152, 2048])
def test_every_clip_is_a_slice_of_the_receivers_own_channelized_bytes(bs):
    cfg, run = _streamed(bs)
    laid = np.concatenate([g["block"] for g in run], axis=1).reshape(3, -1, 2)     # [channel, output, (I, Q)]
    n, kinds, from_prev, tails = 0, set(), 0, 0
    for k, g in enumerate(run):
        c = g["clips"]
        assert c.chunk == k and not c.dropped.any() and c.iq.shape == (int(c.records["n"].sum()), 2)
        assert np.array_equal(c.records["offset"], (np.cumsum(c.records["n"]) - c.records["n"]).astype(np.uint32))
        assert np.all(np.diff(c.records["channel"]) >= 0)
        for i, r in enumerate(c.records):
            t, m = int(r["time"]), int(r["n"])
            assert t == k * bs + int(r["t0"]) and t >= 0 and m % 8 == 0 and t % 8 == 0 and int(r["chunk"]) == k
            assert np.array_equal(c.clip(i), laid[int(r["channel"]), t: t + m]), (k, i, r)
            kinds.add(int(r["source"]))
            from_prev += bool(int(r["flags"]) & CC.FROM_PREV)
            tails += int(r["source"]) == CC.TAIL
        n += c.records.size
    print(f"\n[clips bs {bs}] {n} clips, sources {sorted(kinds)}, {from_prev} reach into the chunk before, {tails} tails")
    assert kinds == {CC.TAIL, CC.RUN, CC.DECODE, CC.EXPECTED, CC.SEARCHED} and from_prev >= 3 and tails >= 1


@pytest.mark.parametrize("bs", [1152, 2048])
def test_records_equal_the_model_and_every_row_and_run_has_its_clip(bs):
    cfg, run = _streamed(bs)
    want, dec, exp, sea = _model(cfg, run, WQ._table(), _centres(), [DEFAULT] * len(run))
    assert _assert_equals_model(run, want) >= 20
    n_rows = 0
    for k, g in enumerate(run):
        recs = g["clips"].records
        # the rows the fetch delivered (after steps 7) and the rows the kernels wrote (before them) alike
        for source, rows in ((CC.DECODE, g["msgs"].records), (CC.EXPECTED, g["expected"].records), (CC.SEARCHED, g["searched"].records),
                             (CC.DECODE, dec[k]), (CC.EXPECTED, exp[k]), (CC.SEARCHED, sea[k])):
            for row in rows:
                hit = recs[(recs["channel"] == row["channel"]) & (recs["ref"] == row["time"]) & (recs["source"] == source)]
                assert hit.size >= 1, (k, source, row)
                p0 = int(row["time"]) - SL + 1
                assert all(int(h["time"]) <= p0 and p0 + N * SL <= int(h["time"]) + int(h["n"]) for h in hit), (k, source, row, hit)
                n_rows += 1
        for b in g["bursts"].records:
            hit = recs[(recs["channel"] == b["channel"]) & (recs["source"] == CC.RUN) & (recs["ref"] == b["first"])]
            assert hit.size == 1, (k, b)
            assert int(hit[0]["t0"]) <= 128 * int(b["first"]) and 128 * (int(b["first"]) + int(b["windows"])) <= int(hit[0]["t0"]) + int(hit[0]["n"])
    assert n_rows >= 16


@pytest.mark.parametrize("bs", [1152, 2048])
def test_stitched_recordings_hold_every_planted_burst(bs):
    """A planted burst's first output b0 lies DC.SEAM_LAG behind its place in the capture (the channel filter's delay).  Its
    run begins with the window that holds b0 or, when too little of the burst lies in that window to switch it ON, with
    the next: 128 first <= b0 + 127.  So the run's clip, and the recording it is merged into, begins at or before
    b0 + 127 - pre; and the run ends with the window that holds the burst's last output or the one before, so with
    post = 128 the recording reaches past that output - where the last window holds enough of the burst to be ON: the channel
    filter spans 512 / 4 = 128 outputs and smears the edge over 64 to either side, so for the twin, which has a run and no
    message, the bound is b1 - 64; a decoded burst's packet clip ends at P0 + N SL + post = b1 + 16 by definition.  The
    packet's own clip begins pre outputs before the packet."""
    cfg, run = _streamed(bs)
    pre = DEFAULT[1]
    st = clips.ClipStitcher(bs)
    recordings = []
    for k, g in enumerate(run):
        recordings += st.add(g["clips"], k * bs)                 # (never raises: overlapping clips are copies of one stream)
    recordings += st.flush()
    laid = np.concatenate([g["block"] for g in run], axis=1).reshape(3, -1, 2)
    for r in recordings:
        assert np.array_equal(r.iq, laid[r.channel, r.time: r.time + len(r.iq)])
    for c, payload, start in DC.DEV_BURSTS:
        b0, b1 = start + DC.SEAM_LAG, start + DC.SEAM_LAG + DC.BURST_OUTPUTS
        lo = max(0, b0 + 127 - pre)
        hi = b1 if payload != DC.TWIN else b1 - 64
        holds = [r for r in recordings if r.channel == c and r.time <= lo and hi <= r.time + len(r.iq)]
        assert len(holds) == 1, (c, start, [(r.channel, r.time, len(r.iq)) for r in recordings])
        if payload != DC.TWIN:
            p0 = b0 + 32 * SL                                      # the packet behind the 32 lead-in symbols, give or take a symbol
            assert holds[0].time <= max(0, p0 - pre + SL)
            assert any(s in (CC.DECODE, CC.EXPECTED, CC.SEARCHED) for s, _ in holds[0].refs)
    assert len(recordings) >= len(DC.DEV_BURSTS)


def test_two_chunks_in_flight_give_the_same_clips():
    bs = 2048
    _, one = _streamed(bs)
    _, stream = DC.device_capture()
    chunks = DC.chunks_of(stream, bs)
    rx = _receiver(bs)
    rx.set_burst_expect(WQ._table())
    got = []
    rx.submit(chunks[0])
    for k in range(1, len(chunks)):
        rx.submit(chunks[k])
        with pytest.raises(RuntimeError, match="in flight"):
            rx.set_burst_clips()                                   # not quiet
        rx.fetch()
        got.append(rx.burst_clips())                               # chunk k - 1's, while chunk k is in flight
    rx.fetch()
    got.append(rx.burst_clips())
    assert len(got) == len(one)
    for a, b in zip(one, got):
        a = a["clips"]
        assert a.chunk == b.chunk and a.records.tobytes() == b.records.tobytes() and a.iq.tobytes() == b.iq.tobytes()
        assert np.array_equal(a.dropped, b.dropped)


def test_settings_changed_between_chunks_hold_from_that_chunk():
    """Rolls, sources and quota change on the quiet receiver in front of every chunk: a chunk behind one with clips off gets no
    tail, and a quota that grows (the slots are made again) keeps what the chunk before owes."""
    bs = 1152
    _, stream = DC.device_capture()
    chunks = DC.chunks_of(stream, bs)
    cycle = [(CC.RUNS | CC.MESSAGES, 256, 128, 4096), (CC.RUNS, 0, 1024, 4096), (CC.MESSAGES, 1024, 0, 8192), (0, 8, 8, 64),
             (CC.RUNS | CC.MESSAGES, 8, 512, 16384)]
    settings = [cycle[k % 5] for k in range(len(chunks))]
    settings[6] = (CC.RUNS | CC.MESSAGES, 64, 1024, 4096)          # burst 2 crosses 7 x 1152: chunk 6 owes ...
    settings[7] = (CC.RUNS | CC.MESSAGES, 64, 64, 32768)           # ... chunk 7, whose slots are new
    rx = _receiver(bs, None)
    tab = WQ._table()
    run = _stream(rx, chunks, tab, settings)
    want, _, _, _ = _model(rx.cfg, run, tab, _centres(), settings)
    assert _assert_equals_model(run, want) >= 12
    owed6 = [p[1][2] for p in want[6][3]]
    assert max(owed6) > 0 and any(int(r["source"]) == CC.TAIL for r in run[7]["clips"].records)
    for k, s in enumerate(settings):
        if not s[0]:
            assert run[k]["clips"] is None                         # (_take saw burst_clips() raise)
        elif k and not settings[k - 1][0]:
            assert not np.any(run[k]["clips"].records["source"] == CC.TAIL)


def test_reset_forgets_what_was_owed():
    bs = 2048
    cfg, one = _streamed(bs)
    want, _, _, _ = _model(cfg, one, WQ._table(), _centres(), [DEFAULT] * len(one))
    owing = next(k for k, w in enumerate(want) if max(p[1][2] for p in w[3]) > 0)   # a chunk that owes its successor a tail
    _, stream = DC.device_capture()
    chunks = DC.chunks_of(stream, bs)
    rx = _receiver(bs)
    _stream(rx, chunks[: owing + 1], WQ._table())
    assert max(int(r["flags"]) & CC.CUT_END for r in rx.burst_clips().records) == CC.CUT_END
    rx.reset()
    assert rx.burst_clips_config() == DEFAULT                      # the settings stay
    with pytest.raises(RuntimeError):
        rx.burst_clips()                                           # no chunk fetched since the reset
    rx.set_burst_threshold(WQ._thresholds(bs))
    again = _stream(rx, chunks[:2], WQ._table())
    for a, b in zip(one, again):
        assert a["clips"].records.tobytes() == b["clips"].records.tobytes() and a["clips"].iq.tobytes() == b["clips"].iq.tobytes()
    assert not np.any(again[0]["clips"].records["source"] == CC.TAIL)


def test_clips_change_nothing_else_and_off_raises():
    bs = 2048
    _, with_clips = _streamed(bs)
    _, stream = DC.device_capture()
    chunks = DC.chunks_of(stream, bs)
    plain = _receiver(bs, None)
    assert plain.burst_clips_config()[0] == 0
    run = []
    for chunk in chunks:
        plain.set_burst_expect(WQ._table())
        packets = plain.demodulate(chunk)
        run.append(dict(_take(plain, False), packets=packets))
    for k, (x, y) in enumerate(zip(run, with_clips)):
        assert x["block"].tobytes() == y["block"].tobytes(), k
        assert x["bursts"].records.tobytes() == y["bursts"].records.tobytes() and x["bursts"].floor.tobytes() == y["bursts"].floor.tobytes(), k
        assert x["msgs"].records.tobytes() == y["msgs"].records.tobytes() and x["msgs"].long_runs.tobytes() == y["msgs"].long_runs.tobytes(), k
        assert x["expected"].records.tobytes() == y["expected"].records.tobytes() and x["expected"].candidates.tobytes() == y["expected"].candidates.tobytes(), k
        assert x["searched"].records.tobytes() == y["searched"].records.tobytes() and x["searched"].sync_hits.tobytes() == y["searched"].sync_hits.tobytes(), k
        key = lambda run_: [[(p.index, bytes(p.data), p.rssi, p.snr) for p in ch] for ch in run_["packets"]]
        assert key(x) == key(y), k
    assert sum(x["msgs"].records.size for x in run) >= 3 and sum(x["searched"].records.size for x in run) >= 1


def test_a_chunk_submitted_with_bursts_off_has_no_clips():
    """Chunks 0 and 1 with clips on, then bursts - and with them clips - off: chunk 2 reuses chunk 0's slots and must not take
    chunk 0's clips for its own."""
    bs = 2048
    _, stream = DC.device_capture()
    chunks = DC.chunks_of(stream, bs)
    rx = _receiver(bs)
    _stream(rx, chunks[:2], TK.table([]))
    assert rx.burst_clips().chunk == 1
    rx.set_bursts(False)
    assert rx.burst_clips_config()[0] == 0
    rx.demodulate(chunks[2])
    with pytest.raises(RuntimeError, match="clips off"):
        rx.burst_clips()
    rx.set_bursts(True)
    rx.set_burst_clips(CC.RUNS, 8, 8, 4096)
    rx.set_burst_threshold(WQ._thresholds(bs))
    rx.demodulate(chunks[3])
    c = rx.burst_clips()
    assert c.chunk == 3 and not np.any(c.records["source"] == CC.TAIL)      # chunk 2 owed nothing: it had no clips


def test_a_burst_at_the_seam_is_recorded_whole():
    """seam_capture(j): the packet's last symbol ends within a symbol of the chunk boundary.  Whichever chunk reports it, the
    clips equal the model's, and one recording holds the packet with its pre- and post-roll across the boundary."""
    bs = DC.SEAM_BS
    rx = _receiver(bs)
    thr = WQ._thresholds(bs)
    tab = TK.table([])
    for j in (0, DC.SEAM_SL - 1, DC.SEAM_SL, 2 * DC.SEAM_SL):
        rx.reset()
        rx.set_burst_threshold(thr)
        run = _stream(rx, DC.chunks_of(DC.seam_capture(j, True), bs), tab)
        want, dec, _, _ = _model(rx.cfg, run, tab, _centres(), [DEFAULT] * len(run))
        assert _assert_equals_model(run, want) >= 3
        st = clips.ClipStitcher(bs)
        recordings = [r for k, g in enumerate(run) for r in st.add(g["clips"], k * bs)] + st.flush()
        rows = [r for d in dec for r in d if bytes(r["data"]).hex() == DC.VALID[1]]
        assert rows, j
        for row in rows:
            p0 = int(row["time"]) - SL + 1
            assert any(r.channel == 1 and r.time <= p0 - DEFAULT[1] and p0 + N * SL + DEFAULT[2] <= r.time + len(r.iq) for r in recordings), (j, row)
