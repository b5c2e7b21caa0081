"""BURST SEARCH without a device (include/rtldavis_hip.h): the model of tests/burst_search_cases.py on noise-free packets of
every shape, on a silent chunk and on the noisy bursts of the gain sweep, where runs at the policy threshold decode
nothing; step 7s around a chunk boundary; every crafted launch's own conditions; the C ABI's argument and state rules;
acquire's helpers; and track.Tracker's provisional stations."""
import ctypes as C

import numpy as np
import pytest

import burst_cases as BC
import burst_decode_cases as DC
import burst_narrow_cases as NB
import burst_repair_cases as RP
import burst_search_cases as SC
import burst_track_cases as TK
import retune_cases as RC
from rtldavis_amd import acquire, track
from rtldavis_amd.wideband import BURST_MSG_DTYPE, SEARCH_HDR_DTYPE


# ------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("shape", SC.SHAPES, ids=lambda s: f"sl{s[0]}_n{s[1]}_b{s[2]}")
def test_a_noise_free_packet_is_found_at_sl_adjacent_positions_and_reported_once(shape):
    sl, n, bs = shape
    cfg = DC.config(sl, n, bs)
    at = bs // 4
    data, row = SC.plain_row(sl, n, bs, at)
    sync_hits, passing = SC.search_positions(row, None, SC.G_CARRIER, cfg, False)
    taus = sorted(passing)
    assert len(taus) in (sl - 1, sl) and taus == list(range(taus[0], taus[-1] + 1)) and taus[0] <= at <= taus[-1], (shape, taus)
    assert sync_hits >= len(taus)
    assert all(bytes(np.packbits(passing[t][1])) == data for t in taus)
    hits, rows = SC.search_channel(row, None, SC.G_CARRIER, 0, 0, cfg, False, 5 * bs)
    assert len(rows) == 1                                    # step 4s: once
    r = np.asarray(rows, BURST_MSG_DTYPE)[0]
    assert bytes(r["data"][: n // 8]) == data and int(r["pad"][0]) == len(taus) and int(r["pad"][3]) == SC.G_CARRIER
    assert int(r["flags"]) == SC.SEARCHED | NB.NARROW and int(r["time"]) == 5 * bs + int(r["tau"]) and abs(int(r["tau"]) - at) <= sl // 2
    hz = acquire.burst_message_offset_hz(r, 64000, 0, 64000 * DC.deviation(sl), n)     # (f_re, f_im) serve unchanged
    assert abs(hz - 64000 * SC.CARRIER) < 0.02 * 64000


def test_a_silent_chunk_gives_no_sync_hit_and_no_row():
    for sl, n, bs in SC.SHAPES:
        cfg = DC.config(sl, n, bs)
        row = np.full(2 * bs, 128, np.uint8)
        for prev in (None, row):
            for g in (0, SC.G_CARRIER, 32, 63):
                assert SC.search_channel(row, prev, g, 0, 0, cfg, prev is not None, 0) == (0, [])


GAIN = {}


def _gain(k=30, noise=0.20, seed=7, cfo=1500.0):
    """(policy records, search records at the nearest centre, planted payloads) of the stream models over the sweep's
    blocks; made once."""
    if not GAIN:
        datas, blocks = RP.gain_blocks(k, noise, seed, cfo)
        cfg = DC.config(RP.GAIN_SL, 80, RP.GAIN_BS)
        floor = BC.model_bursts(blocks[1], 2 ** 32 - 1, 1).floor           # chunk 1 holds noise alone
        thr = acquire.Acquisition(1, cfg, factor=4).thresholds(floor)
        bursts = [BC.model_bursts(b, thr, j) for j, b in enumerate(blocks)]
        policy = [rec for _, m in NB.decode_stream(blocks, thr, cfg, 0, True, bursts=bursts) for rec in m.records]
        centres = [int(g) for g in acquire.search_centres([cfo], 19200 * RP.GAIN_SL)]
        found = SC.search_stream(blocks, [centres] * len(blocks), cfg)
        GAIN["v"] = (policy, found, datas, centres)
    return GAIN["v"]


def test_policy_runs_decode_no_burst_at_noise_0_20():
    policy, _, datas, _ = _gain()
    assert NB.tally(policy, datas) == (0, 0)


def test_the_search_decodes_at_least_20_of_30_at_noise_0_20_with_no_wrong_payload():
    """The prototype, which sliced around the unnormalised sum, got 29 of 30; the bound of 20 covers the 16-bit direction
    and the zero extension.  The measured values are printed (and stand in profiles/burst_search_gain.txt)."""
    _, found, datas, centres = _gain()
    recs = [r for m in found for r in m.records]
    decoded, wrong = NB.tally(recs, datas)
    positions = sum(m.sync_hits.size * (RP.GAIN_BS - 14 * 79) for m in found)
    print(f"burst search, noise 0.20, 30 bursts, seed 7, centre {centres}: decoded {decoded}, wrong {wrong}, "
          f"sync_hits {sum(int(m.sync_hits.sum()) for m in found)} of about {positions} positions")
    assert centres == [48]
    assert wrong == 0 and decoded >= 20
    assert len(recs) == decoded                              # every burst once: step 4s within a chunk, 7s across


def test_step_7s_delivers_a_packet_at_every_offset_around_a_boundary_once():
    first, back, data = SC.seam_launches()
    a, b = SC.launch_records(first), SC.launch_records(back)
    kept = SC.drop_repeats(b, a, DC.SEAM_SL)
    chans = sorted([int(x["channel"]) for x in a] + [int(x["channel"]) for x in kept])
    assert chans == list(range(len(DC.SEAM_LAST))), chans
    assert all(bytes(x["data"][: DC.SEAM_N // 8]) == data for x in list(a) + list(kept))
    assert len(a) and len(kept) and len(a) + len(b) > len(DC.SEAM_LAST)      # both sides report, some packets twice
    assert all(int(x["flags"]) & 1 for x in b)
    other = a.copy()
    other["pad"][:, 3] ^= 1                                  # another centre's records repeat nothing
    assert len(SC.drop_repeats(b, other, DC.SEAM_SL)) == len(b)
    # the stream model runs the same rule
    data2, b0, b1 = DC.seam_rows()
    cfg = DC.config(DC.SEAM_SL, DC.SEAM_N, DC.SEAM_BS)
    got = SC.search_stream([b0, b1], [[SC.G_CARRIER]] * 2, cfg)
    assert got[0].records.tobytes() == a.tobytes() and got[1].records.tobytes() == kept.tobytes()


def test_crafted_cases_reach_their_edges():
    for L in SC.hook_launches():
        msgs, hdr = L.want()
        n = len(L.centres)
        assert np.all(hdr[:n]["chunk"] == (L.seq & 0xFFFFFFFF)) and hdr[n:].tobytes() == bytes([SC.FILL]) * hdr[n:].nbytes
        assert msgs[n:].tobytes() == bytes([SC.FILL]) * msgs[n:].nbytes
    assert SC.TILE == 1024 and SC.candidate_range(DC.config(14, 80, 128), False) is None


# ------------------------------------------------------------------------------------------ the C ABI and acquire
def _receiver(bs=2048, n_ch=3, sl=14):
    from rtldavis_amd import wideband
    chans = [RC.CENTRE - 100000 + 50000 * c for c in range(n_ch)]
    return wideband.WidebandReceiver(RC.packet_config(bs, sl), chans, RC.CENTRE, decim=100, taps=np.ones(8) / 8)


def test_set_burst_search_argument_and_state_rules():
    from rtldavis_amd import _lib, wideband
    L = _lib.lib()
    w = _receiver()
    with pytest.raises(RuntimeError):
        w.set_burst_search([7])                              # decode is off
    assert "decode" in _lib.last_error() and w.burst_search().size == 0
    w.set_bursts(True)
    w.set_burst_decode(True)
    w.set_burst_search([7, 8, 63, 0])
    assert list(w.burst_search()) == [7, 8, 63, 0] and w.burst_search().dtype == np.uint8
    for bad in ([64], [7, 8, 7], [255], [-1], [1.5], list(range(9))):
        with pytest.raises(ValueError):
            w.set_burst_search(bad)
        assert list(w.burst_search()) == [7, 8, 63, 0]       # nothing changed
    eight = np.arange(10, 18, dtype=np.uint8)
    w.set_burst_search(eight)
    assert list(w.burst_search()) == list(eight)
    assert L.rd_wb_set_burst_search(w._h, eight.ctypes.data, -1) == _lib.RD_ERR_ARG
    assert L.rd_wb_set_burst_search(w._h, None, 1) == _lib.RD_ERR_ARG and L.rd_wb_set_burst_search(None, None, 0) == _lib.RD_ERR_ARG
    n = C.c_int(0)
    assert L.rd_wb_burst_search(w._h, None, 0, C.byref(n)) == _lib.RD_ERR_CAPACITY and n.value == 8
    w.set_burst_search([])                                   # n = 0 clears
    assert w.burst_search().size == 0
    for clear in (lambda: w.set_burst_decode(False), lambda: w.set_bursts(False)):
        w.set_bursts(True)
        w.set_burst_decode(True)
        w.set_burst_search([7])
        clear()
        assert w.burst_search().size == 0
    w.set_bursts(True)
    w.set_burst_decode(True)
    w.set_burst_search([7])
    w.reset()                                                # the list stays
    assert list(w.burst_search()) == [7]
    with pytest.raises(RuntimeError):
        w.searched_messages()                                # no chunk fetched
    short = _receiver(sl=2)                                  # the filter needs symbol_length >= 4
    short.set_bursts(True)
    short.set_burst_decode(True)
    with pytest.raises(ValueError):
        short.set_burst_search([7])
    short.set_burst_search([])
    assert wideband.BURST_MSG_SEARCHED == 16 == acquire.MSG_SEARCHED == SC.SEARCHED and SEARCH_HDR_DTYPE.itemsize == 16
    assert (wideband.BURST_SEARCH_MAX_CENTRES, wideband.BURST_SEARCH_PER, wideband.BURST_SEARCH_TILE) == (SC.MAX_CENTRES, SC.PER, SC.TILE)


def test_hook_arguments_are_refused_before_any_device_work():
    from rtldavis_amd import _lib
    L = _lib.lib()
    X = SC.first_chunk_launch()
    cfg = _lib.make_config(X.cfg.bit_rate, X.cfg.symbol_length, X.cfg.preamble_symbols, X.cfg.packet_symbols, X.cfg.preamble, X.cfg.block_size)
    msgs, hdr = np.zeros((8, X.n_ch, 4), BURST_MSG_DTYPE), np.zeros((8, X.n_ch), SEARCH_HDR_DTYPE)

    def call(centres, c=cfg, stride=X.cur.shape[1], n_ch=X.n_ch):
        g = np.ascontiguousarray(centres, np.uint8)
        return L.rd_debug_burst_search(C.byref(c), X.cur.ctypes.data, None, stride, n_ch, 0, 0, g.ctypes.data, g.size, msgs.ctypes.data, hdr.ctypes.data)
    for centres in ([], [7, 7], [64], list(range(9))):
        assert call(centres) == _lib.RD_ERR_ARG, centres
    assert call([7], stride=X.cur.shape[1] - 16) == _lib.RD_ERR_ARG and call([7], n_ch=0) == _lib.RD_ERR_ARG
    sl2 = _lib.make_config(X.cfg.bit_rate, 2, X.cfg.preamble_symbols, X.cfg.packet_symbols, X.cfg.preamble, X.cfg.block_size)
    assert call([7], c=sl2) == _lib.RD_ERR_ARG
    assert not msgs.tobytes().strip(b"\0") and not hdr.tobytes().strip(b"\0")


def test_acquire_helpers():
    out_rate = 19200 * 14
    assert list(acquire.search_centres([1500.0], out_rate)) == [48]                       # -Fs / 4 + 1.5 kHz: 48 / 64 - 1
    assert list(acquire.search_centres([1500.0], out_rate, spread=2)) == [46, 47, 48, 49, 50]
    assert list(acquire.search_centres(DC.DEV_PLANTED, out_rate)) == [5, 41, 53]
    assert list(acquire.search_centres([0, 100], out_rate, if_hz=0, spread=1)) == [0, 1, 63]
    assert acquire.search_centres([], out_rate).size == 0 and acquire.search_centres([0], out_rate).dtype == np.uint8
    with pytest.raises(ValueError):
        acquire.search_centres([0], out_rate, spread=-1)
    L = SC.shape_launch(14, 80, 2048)
    rows = SC.launch_records(L)
    assert len(rows) == 2 and acquire.searched(rows).all() and acquire.narrowband(rows).all() and not acquire.expected(rows).any()
    assert list(acquire.search_hits(rows)) == [int(r["pad"][0]) for r in rows] and min(acquire.search_hits(rows)) >= 12
    plain = TK.edges_launch()[0].recs()
    assert not acquire.searched(plain).any() and not acquire.search_hits(plain).any()


# ------------------------------------------------------------------------------------------ the tracker
CFG = DC.config(14, 80, 2048)
PATTERN = (2, 0, 1)


def _row(channel, ident, time, flags, like=None):
    """A message row of station ``ident``: the fields a Tracker reads."""
    r = np.zeros(1, BURST_MSG_DTYPE)[0]
    r["channel"], r["id"], r["time"], r["flags"] = channel, ident, time, flags
    r["f_re"], r["f_im"], r["ones"] = 0, -1000, 40            # a carrier at -Fs / 4: offset 0
    return r


def _rows(*rows):
    return np.asarray(list(rows), BURST_MSG_DTYPE).reshape(-1)


def test_tracker_seeds_a_provisional_station_and_an_expected_row_promotes_it():
    t = track.Tracker(CFG, PATTERN, period_outputs=10000)
    assert t.provisional() == [] and t.search_stats() == {"seeded": 0, "promoted": 0, "expired": 0, "ignored": 0}
    t.observe(_rows(_row(2, 3, 1000, 16 | 4)))
    assert t.provisional() == [3] and t.stations() == {} and t.stats() == {}
    assert t.search_stats() == {"seeded": 1, "promoted": 0, "expired": 0, "ignored": 0}
    e = t.table(10000, 2048)                                  # it gets expectations like any station
    g = t.guard(3, 0)
    assert e.size == 1 and (int(e[0]["channel"]), int(e[0]["id"]), int(e[0]["t_lo"]), int(e[0]["t_hi"])) == (0, 3, 11000 - g, 11000 + g)
    t.observe(_rows(_row(0, 3, 11003, 16 | 4)))               # a searched row of a provisional id: ignored, no re-anchor
    assert t.provisional() == [3] and t.search_stats()["ignored"] == 1
    assert int(t.table(10000, 2048)[0]["t_lo"]) == 11000 - g
    t.observe(_rows(_row(0, 3, 11003, 8 | 4)))                # the expected row
    assert t.provisional() == [] and t.stations()[3][:3] == (0, 11003, 0)
    assert t.stats() == {3: {"received": 1, "missed": 0, "lost": 0}}
    assert t.search_stats() == {"seeded": 1, "promoted": 1, "expired": 0, "ignored": 1}
    t.observe(_rows(_row(1, 3, 21003, 16 | 4 | 1)))           # a searched row of a known station: ignored, never re-anchors
    assert t.stations()[3][:3] == (0, 11003, 0) and t.stats()[3]["received"] == 1 and t.search_stats()["ignored"] == 2


def test_a_provisional_station_expires_after_two_misses_without_touching_stats():
    t = track.Tracker(CFG, PATTERN, period_outputs=10000)
    t.observe(_rows(_row(2, 5, 1000, 16 | 4), _row(7, 6, 1000, 16 | 4)))    # (channel 7 is outside the pattern)
    assert t.provisional() == [5] and t.search_stats() == {"seeded": 1, "promoted": 0, "expired": 0, "ignored": 1}
    body = 14 * 79
    assert t.table(11000 + t.guard(5, 0) + body + 1, 12000).size == 1 and t.provisional() == [5]   # one miss: a hop on
    assert t.table(21000 + t.guard(5, 1) + body + 1, 12000).size == 0 and t.provisional() == []    # two: gone
    assert t.stats() == {} and t.stations() == {}
    assert t.search_stats() == {"seeded": 1, "promoted": 0, "expired": 1, "ignored": 1}
    u = track.Tracker(CFG, PATTERN, period_outputs=10000, provisional_missed=1)
    u.observe(_rows(_row(2, 5, 1000, 16 | 4)))
    assert u.table(11000 + u.guard(5, 0) + body + 1, 12000).size == 0 and u.search_stats()["expired"] == 1
    with pytest.raises(ValueError):
        track.Tracker(CFG, PATTERN, provisional_missed=0)


def test_stats_are_those_of_a_run_without_searched_rows():
    """The same burst and expected rows with and without searched rows of the known station and of a chance id mixed in:
    the same tables, stations() and stats()."""
    def run(with_search):
        t = track.Tracker(CFG, PATTERN, period_outputs=10000)
        tabs = []
        for k in range(8):
            at = 1000 + 10000 * k
            if with_search and k == 2:
                t.observe(_rows(_row(PATTERN[k % 3], 6, at - 3000, 16 | 4)))     # a chance hit: id 6 is never confirmed
            if k not in (4,):                                                      # packet 4 is missed
                t.observe(_rows(_row(PATTERN[k % 3], 1, at, 8 if k else 0)))
                if with_search:
                    t.observe(_rows(_row(PATTERN[k % 3], 1, at + 2, 16 | 4)))
            tab = t.table(at + 5000, 2048)
            tabs.append(tab[tab["id"] == 1].tobytes())
        return tabs, t.stations(), t.stats(), t.search_stats()
    a, b = run(False), run(True)
    assert a[:3] == b[:3]
    assert a[2] == {1: {"received": 7, "missed": 1, "lost": 0}}
    assert a[3] == {"seeded": 0, "promoted": 0, "expired": 0, "ignored": 0}
    assert b[3] == {"seeded": 1, "promoted": 0, "expired": 1, "ignored": 7}       # id 6 came and went; id 1's seven were ignored
