"""BURST EXPECT without a device (include/rtldavis_hip.h): the model of tests/burst_track_cases.py against the run model it
is built beside, every crafted launch's own conditions, the library's candidate range against the model's, the C ABI's
argument and state rules, and track.Tracker - seeding, misses, the guard and its cap, the drop, retuned, determinism."""
import ctypes as C

import numpy as np
import pytest

import burst_decode_cases as DC
import burst_narrow_cases as NB
import burst_track_cases as TK
import retune_cases as RC
from rtldavis_amd import acquire, track
from rtldavis_amd.wideband import BURST_MSG_DTYPE, EXPECT_DTYPE


# ------------------------------------------------------------------------------------------ the model
def test_an_expectation_equal_to_a_runs_region_gives_the_runs_record():
    """The wide form: an expectation whose candidates are exactly a run's, carrying the run's correlation sum shifted into
    16 bits, slices in the same direction - tau, data, ones, id and the f sums equal the run model's record; the margin
    is the run's scaled by the shift, to within the shift's floor."""
    for n, sl in ((80, 14), (40, 8)):
        L = NB.grid_launch(n, sl)
        for c in range(2):
            rec, want = L.runs[c, 0], L.records(c)[0]
            sh, ca, cb, _ = NB.grid_choice(rec["corr_re"], rec["corr_im"], sl)
            t0, t1 = 128 * int(rec["first"]), 128 * (int(rec["first"]) + int(rec["windows"]))
            e = TK.table([TK.expect_row(c, L.clock + t0 + sl, L.clock + t1 - 1 - sl * (n - 1), (ca, cb))])[0]
            cand, row = TK.decode_expect(L.cur[c], None, e, 0, L.cfg, False, L.clock, 0, False)
            assert cand == t1 - sl * (n - 1) - (t0 + sl)
            got = np.asarray([row], BURST_MSG_DTYPE)[0]
            for f in ("channel", "tau", "time", "f_re", "f_im", "ones", "id"):
                assert got[f] == want[f], (n, sl, c, f)
            assert bytes(got["data"]) == bytes(want["data"]) and int(got["flags"]) == TK.EXPECTED and int(got["first"]) == 0
            assert abs(int(got["margin"]) - (int(want["margin"]) >> sh)) <= 2 ** 20


def test_step_7_prime_equals_step_7_on_the_seam():
    """At a chunk seam the second report always has its region below t = 0 (flags bit 0), so the rule of step 7' and
    burst_decode_cases.drop_repeats - which looks at that bit - drop the same records; one report survives per packet."""
    from rtldavis_amd.wideband import BurstMessages
    first, back, data = TK.seam_launches()
    for r, nb in TK.FORMS:
        a, b = first.recs(r, nb), back.recs(r, nb)
        kept = TK.drop_repeats(b, a, DC.SEAM_SL)
        same = DC.drop_repeats(BurstMessages(b, np.zeros(1, np.uint32), 1), a, DC.SEAM_SL).records
        assert kept.tobytes() == same.tobytes()
        chans = sorted([int(x["channel"]) for x in a] + [int(x["channel"]) for x in kept])
        assert chans == list(range(len(DC.SEAM_LAST))), (r, nb, chans)
        assert all(bytes(x["data"]) == data for x in list(a) + list(kept))
    assert len(first.recs()) and len(TK.drop_repeats(back.recs(), first.recs(), DC.SEAM_SL)) and len(back.recs()) + len(first.recs()) > len(DC.SEAM_LAST)


def test_crafted_cases_reach_their_edges():
    TK.edges_launch()
    TK.gap_window0_off()
    TK.gap_long_run()
    TK.gap_trailing_only()
    TK.first_chunk_launches()
    TK.alignment_launch()
    TK.id_launches()
    TK.largest_launch()
    TK.full_table_launch()
    TK.all_idle_launch()
    TK.tie_launch()
    TK.bounds_launch()
    TK.repair_launches()
    for n, sl in NB.NGRID:
        TK.grid_launch(n, sl)


# ------------------------------------------------------------------------------------------ the C ABI
def _receiver(bs=2048, n_ch=3, sl=14):
    from rtldavis_amd import wideband
    chans = [RC.CENTRE - 100000 + 50000 * c for c in range(n_ch)]
    return wideband.WidebandReceiver(RC.packet_config(bs, sl), chans, RC.CENTRE, decim=100, taps=np.ones(8) / 8)


def test_set_burst_expect_argument_and_state_rules():
    from rtldavis_amd import _lib, wideband
    L = _lib.lib()
    w = _receiver()
    good = TK.table([TK.expect_row(1, 1000, 1200, (16384, 0), 3), TK.expect_row(2, 2 ** 64 - 100, 2 ** 64 - 1, (-32768, 32767))])
    with pytest.raises(RuntimeError):
        w.set_burst_expect(good)                              # decode is off
    assert "decode" in _lib.last_error() and w.burst_expect().size == 0
    w.set_bursts(True)
    w.set_burst_decode(True)
    w.set_burst_expect(good)
    assert w.burst_expect().tobytes() == good.tobytes() and w.burst_expect().dtype == EXPECT_DTYPE
    for field, value in (("channel", 3), ("channel", -1), ("id", 8), ("id", 0xFE), ("t_hi", 999), ("t_hi", 1000 + 2049),
                         ("corr_re", 32768), ("corr_im", -32769)):
        bad = good.copy()
        bad[0][field] = value
        with pytest.raises(ValueError):
            w.set_burst_expect(bad)
        assert "entry 0" in _lib.last_error(), (field, _lib.last_error())
        assert w.burst_expect().tobytes() == good.tobytes()   # nothing changed
    bad = good.copy()
    bad[1]["corr_re"], bad[1]["corr_im"] = 0, 0
    with pytest.raises(ValueError):
        w.set_burst_expect(bad)
    assert "entry 1" in _lib.last_error()
    span = good.copy()
    span[0]["t_hi"] = 1000 + 2048                             # the widest window
    w.set_burst_expect(span)
    big = np.repeat(good[:1], wideband.BURST_EXPECT_MAX + 1)
    assert L.rd_wb_set_burst_expect(w._h, big.ctypes.data, big.size) == _lib.RD_ERR_ARG
    assert L.rd_wb_set_burst_expect(w._h, big.ctypes.data, -1) == _lib.RD_ERR_ARG
    assert L.rd_wb_set_burst_expect(w._h, None, 1) == _lib.RD_ERR_ARG and L.rd_wb_set_burst_expect(None, None, 0) == _lib.RD_ERR_ARG
    w.set_burst_expect(big[: wideband.BURST_EXPECT_MAX])
    assert w.burst_expect().size == 64
    n = C.c_int(0)
    assert L.rd_wb_burst_expect(w._h, None, 0, C.byref(n)) == _lib.RD_ERR_CAPACITY and n.value == 64
    w.set_burst_expect(good[:0])                              # n = 0 clears
    assert w.burst_expect().size == 0
    for clear in (lambda: w.set_burst_decode(False), lambda: w.set_bursts(False), w.reset):
        w.set_bursts(True)
        w.set_burst_decode(True)
        w.set_burst_expect(good)
        clear()
        assert w.burst_expect().size == 0
    w.set_bursts(True)
    w.set_burst_decode(True)
    with pytest.raises(RuntimeError):
        w.expected_messages()                                 # no chunk fetched
    assert wideband.BURST_MSG_EXPECTED == 8 == acquire.MSG_EXPECTED and EXPECT_DTYPE == track.EXPECT_DTYPE and EXPECT_DTYPE.itemsize == 32


def test_hook_arguments_are_refused_before_any_device_work():
    from rtldavis_amd import _lib
    L = _lib.lib()
    X, _ = TK.edges_launch()
    cfg = _lib.make_config(X.cfg.bit_rate, X.cfg.symbol_length, X.cfg.preamble_symbols, X.cfg.packet_symbols, X.cfg.preamble, X.cfg.block_size)
    msgs, hdr = np.zeros(64, BURST_MSG_DTYPE), np.zeros(64, TK.HDR_DTYPE)

    def call(tab, n_e, flips=0, narrow=0, n_ch=1):
        return L.rd_debug_burst_expect(C.byref(cfg), X.cur.ctypes.data, None, X.cur.shape[1], n_ch, 0, 0, tab.ctypes.data, n_e, flips, narrow,
                                       msgs.ctypes.data, hdr.ctypes.data)
    bad = X.table.copy()
    bad[1]["channel"] = 1
    assert call(bad, bad.size) == _lib.RD_ERR_ARG and "entry 1" in _lib.last_error()
    assert call(X.table, 0) == _lib.RD_ERR_ARG and call(X.table, 65) == _lib.RD_ERR_ARG
    assert call(X.table, X.table.size, flips=3) == _lib.RD_ERR_ARG and call(X.table, X.table.size, narrow=2) == _lib.RD_ERR_ARG
    assert not msgs.tobytes().strip(b"\0") and not hdr.tobytes().strip(b"\0")


def test_acquire_expected_mask():
    X, _ = TK.edges_launch()
    assert acquire.expected(X.recs()).all() and not acquire.expected(DC.seam_launches()[1].records(0)).any()


# ------------------------------------------------------------------------------------------ the tracker
CFG = DC.config(14, 80, 2048)
OUT_RATE = 19200 * 14


def test_tracker_defaults_and_seeding():
    t = track.Tracker(CFG, (2, 0, 1))
    assert t.period(0) == 41 * OUT_RATE // 16 == int(2.5625 * OUT_RATE) and t.period(3) == 44 * OUT_RATE // 16
    assert t.guard(0, 0) == 28 + 69 and t.guard(0, 1) == 28 + 138 and t.max_missed == 50
    assert t.table(0, 2048).size == 0 and t.stats() == {}
    t.observe_at(0, 3, 5000, 1200.0)
    t.observe_at(7, 4, 5000, 0.0)                             # a channel outside the pattern: ignored
    assert t.stats() == {3: {"received": 1, "missed": 0, "lost": 0}}
    p = t.period(3)
    tab = t.table(5000 + p - 1000, 2048)
    assert tab.dtype == EXPECT_DTYPE and tab.size == 1
    e = tab[0]
    g = t.guard(3, 0)
    assert (int(e["channel"]), int(e["id"]), int(e["t_lo"]), int(e["t_hi"])) == (1, 3, 5000 + p - g, 5000 + p + g)
    f = (-OUT_RATE // 4 + 1200.0) / OUT_RATE
    assert (int(e["corr_re"]), int(e["corr_im"])) == TK.corr_of(f)
    assert t.table(5000, 2048).size == 0                      # the window begins beyond the horizon
    t.observe_at(0, 3, 5003, 1300.0)                          # the same packet by another path: the carrier alone moves
    assert t.stats()[3]["received"] == 1 and t.stations()[3][3] == 1300.0


def test_tracker_counts_misses_widens_the_guard_and_drops():
    t = track.Tracker(CFG, (2, 0, 1), period_outputs=10000, drift_ppm=1000, max_missed=4)
    t.observe_at(2, 1, 1000, 0.0)
    assert [t.guard(1, m) for m in (0, 1, 2, 200)] == [38, 48, 58, 1024]      # 2 SL + 10 (m + 1), capped at 2048 / 2
    body = 14 * 79
    e = t.table(11000, 2048)[0]
    assert (int(e["channel"]), int(e["t_lo"]), int(e["t_hi"])) == (0, 11000 - 38, 11000 + 38)
    assert t.table(11000 + 38 + body, 2048).size == 1 and t.stats()[1]["missed"] == 0     # a packet at t_hi ends at this clock
    e = t.table(11000 + 38 + body + 1, 12000)[0]              # passed: one miss, one hop on, a wider window
    assert t.stats()[1]["missed"] == 1
    assert (int(e["channel"]), int(e["t_lo"]), int(e["t_hi"])) == (1, 21000 - 48, 21000 + 48)
    t.observe_at(1, 1, 21007, 50.0)                           # picked up again: re-anchored, misses in a row back to 0
    assert t.stations()[1][:3] == (1, 21007, 0) and t.stats()[1] == {"received": 2, "missed": 1, "lost": 0}
    e = t.table(30000, 2048)[0]
    assert (int(e["channel"]), int(e["t_lo"]), int(e["t_hi"])) == (2, 31007 - 38, 31007 + 38)
    assert t.table(21007 + 4 * 10000 + 5000, 2048).size == 0  # four windows passed: dropped
    assert t.stats()[1] == {"received": 2, "missed": 5, "lost": 1} and t.stations() == {}
    t.observe_at(0, 1, 90000, 0.0)                            # heard again: seeded anew
    assert t.stats()[1]["received"] == 3 and t.table(99000, 2048).size == 1


def test_tracker_fixed_guard_horizon_retuned_and_determinism():
    t = track.Tracker(CFG, (2, 0, 1), period_outputs=3000, guard_outputs=5000)
    assert t.guard(0, 0) == 1024 == t.guard(0, 7)             # capped: t_hi - t_lo <= 2048
    t.observe_at(2, 0, 500, 100.0)
    tab = t.table(0, 10000)                                   # every window that begins inside the horizon
    assert [int(c) for c in tab["channel"]] == [0, 1, 2] and [int(x) for x in tab["t_hi"] - tab["t_lo"]] == [2048] * 3
    t.retuned(40.0)
    assert t.stations()[0][3] == 60.0

    def run():
        u = track.Tracker(CFG, (2, 0, 1), period_outputs=3000)
        out = []
        for k in range(12):
            if k in (1, 4, 5, 9):
                u.observe_at((2, 0, 1)[k % 3], k % 2, 700 * k + 13, 321.5 * k)
            out.append(u.table(700 * k, 2048).tobytes())
        return out, u.stats()
    assert run() == run()
    with pytest.raises(ValueError):
        track.Tracker(CFG, ())
    with pytest.raises(ValueError):
        track.Tracker(CFG, (0, 1), period_outputs=0)


def test_tracker_observe_rows_ignores_repaired_unless_asked():
    X, flip = TK.id_launches()
    rows = flip.recs(1)                                       # repaired rows of id 2 on channel 0
    assert len(rows) and acquire.repaired(rows).all()
    cfg = flip.cfg
    t = track.Tracker(cfg, (0,))
    t.observe(rows)
    assert t.stats() == {}
    u = track.Tracker(cfg, (0,), use_repaired=True)
    u.observe(rows)
    assert u.stats()[2]["received"] == 1
    v = track.Tracker(cfg, (0,))
    v.observe(X.recs())
    hz = acquire.burst_message_offset_hz(X.recs()[0], v.out_rate, v.if_hz, 4800.0, 80)
    assert v.stations()[3] == (0, int(X.recs()[0]["time"]), 0, hz)
