"""BURST QUALITY without a device (include/rtldavis_hip.h): hand-derived values of the integer model, the header's bounds
on the worst bytes, the library's window arithmetic against the model's, the dB helpers and their fallbacks, burst_packets
through the parser's front half, the argument rules that need no device, and every crafted launch's own conditions
(tests/burst_quality_cases.py asserts them when a launch is built)."""
import ctypes as C
import math

import numpy as np
import pytest

import burst_decode_cases as DC
import burst_narrow_cases as NB
import burst_quality_cases as QC
from rtldavis_amd import acquire, wideband
from rtldavis_amd.wideband import BURST_MSG_DTYPE, QUALITY_DTYPE


def test_layout_and_constants():
    assert QUALITY_DTYPE.itemsize == 64 and QUALITY_DTYPE.fields["n_noise"][1] == 48 and QUALITY_DTYPE.fields["chunk"][1] == 60
    assert (wideband.QUALITY_INBAND, wideband.QUALITY_UNMEASURABLE, wideband.QUALITY_MAX_GAP) == (QC.INBAND, QC.UNMEASURABLE, QC.MAX_GAP)
    assert acquire.QUALITY_INBAND == wideband.QUALITY_INBAND


def test_every_crafted_launch_meets_its_conditions():
    names = [L.name for L in QC.crafted_launches()]
    assert len(names) == len(set(names)) == 12


def test_all_bytes_255_by_hand():
    sl, n = 14, 80
    L = QC.flat_launch()
    r = L.row(2)
    assert 2 * 255 * 255 == 130050
    assert int(r["pkt"]) == 130050 * n * sl and int(r["clipped"]) == 2 * n * sl and int(r["peak"]) == 255
    assert int(r["sig"]) == 130050 * 16 * sl
    assert acquire.rssi_db(r, sl) == pytest.approx(10 * math.log10(2), abs=1e-12)
    assert acquire.snr_db(r, sl) == pytest.approx(0.0, abs=1e-12)          # the window in front holds the same bytes
    # behind the filter a constant passes with the taps' sum (2^14 give or take the rounding) over 2^11: y = 2040 +- 1
    y2 = int(r["pkt_nb"]) / (n * sl)
    assert 2 * 2039 ** 2 <= y2 <= 2 * 2041 ** 2
    assert acquire.snr_inband_db(r, sl) == pytest.approx(0.0, abs=1e-12)


def test_bounds_on_the_worst_bytes():
    # raw: the longest packet of saturated bytes
    sl, n = 51, 40
    bs = QC.smallest_block(sl, n)
    cfg = DC.config(sl, n, bs)
    rows = [np.full(2 * bs, 255, np.uint8)]
    q = QC.measure(np.stack(rows), None, cfg, 0, sl - 1, 1, 0, 0, 1)
    assert q[0] == 130050 * 2040 < 2047 * 130050 < 2 ** 28
    # in-band: the bytes that drive one output of the filter to its bound, at every grid point of the smallest and the largest filter
    for sl in (4, 51):
        worst = 0
        for g in range(NB.GRID):
            zi, zq, t = NB.worst_region(sl, g)
            _, (yr, yi) = NB.filter_region(zi, zq, NB.table(sl)[0][g])
            worst = max(worst, int((yr * yr + yi * yi).max()))
        assert worst <= QC.Y2_MAX == 2 * 3192 * 3192 < 2 ** 25
    assert 2047 * QC.Y2_MAX < 2 ** 36


def test_library_windows_equal_the_model():
    from rtldavis_amd import _lib
    L = _lib.lib()
    out = np.zeros(5, np.int32)

    def lib(sl, n, bs, have_prev, tau, gap):
        ok = L.rd_bq_window(sl, n, bs, have_prev, tau, gap, out.ctypes.data)
        return tuple(int(v) for v in out) if ok else None

    for X in QC.crafted_launches():
        sl, n, bs = int(X.cfg.symbol_length), int(X.cfg.packet_symbols), int(X.cfg.block_size)
        for c in range(X.n_ch):
            for m in X.msgs[c, : int(X.n_msgs[c])]:
                assert lib(sl, n, bs, X.prev is not None, int(m["tau"]), X.gap) == QC.windows(sl, n, bs, X.prev is not None, int(m["tau"]), X.gap)
    rng = np.random.default_rng(5)
    for _ in range(2000):
        sl, n = int(rng.integers(1, 52)), int(rng.choice((40, 48, 64, 80)))
        if n * sl + 1 > 2048:
            continue
        bs = QC.smallest_block(sl, n) * int(rng.integers(1, 3))
        hp, gap = int(rng.integers(0, 2)), int(rng.integers(0, 1025))
        tau = int(rng.integers(-bs - 60, bs + 60))
        want = QC.windows(sl, n, bs, hp, tau, gap)
        assert lib(sl, n, bs, hp, tau, gap) == want
        naive = QC.naive_windows(sl, n, bs, hp, tau, gap)
        assert (naive is None) == (want is None)
        if want is not None:
            p0, p1, s1, n0, n1 = want
            assert naive == (list(range(p0, p1)), list(range(p0, s1)), list(range(n0, n1)))
    assert lib(14, 80, 1152, 1, -2 ** 31, 0) is None and lib(14, 80, 1152, 1, 2 ** 31 - 1, 0) is None
    assert lib(14, 80, 1152, 1, 2 ** 62, 0) is None and lib(14, 80, 1152, 1, 13, -1) is None


def _q(**kw):
    r = np.zeros(1, QUALITY_DTYPE)[0]
    for k, v in kw.items():
        r[k] = v
    return r


def test_db_helpers_and_fallbacks():
    sl = 14
    fs = 16 * sl * 255 ** 2
    assert acquire.rssi_db(_q(sig=fs), sl) == pytest.approx(0.0, abs=1e-12)
    assert acquire.rssi_db(_q(sig=0), sl) == -120
    # a quarter of full scale in the signal, a hundredth of that in 100 outputs of noise
    q = _q(sig=fs // 4, noise=100 * 255 ** 2 // 400, n_noise=100)
    assert acquire.snr_db(q, sl) == pytest.approx(10 * math.log10((fs // 4 / fs) / ((100 * 255 ** 2 // 400) / (100 * 255 ** 2))), abs=1e-12)
    assert abs(acquire.snr_db(q, sl) - 20.0) < 0.01
    # no noise region: 1e-9 full-scale^2; a noise sum of 0: 50
    assert acquire.snr_db(_q(sig=fs, n_noise=0), sl) == pytest.approx(90.0, abs=1e-9)
    assert acquire.snr_db(_q(sig=fs, n_noise=7, noise=0), sl) == 50
    assert math.isnan(acquire.snr_db(_q(flags=128), sl)) and acquire.rssi_db(_q(flags=128), sl) == -120
    # in-band: NaN without bit 0; full scale is 8 x 255 there
    assert math.isnan(acquire.snr_inband_db(_q(sig_nb=5, noise_nb=5, n_noise=5), sl))
    qi = _q(flags=1, sig_nb=64 * fs, noise_nb=64 * 100 * 255 ** 2 // 100, n_noise=100)
    assert acquire.snr_inband_db(qi, sl) == pytest.approx(20.0, abs=1e-9)
    assert acquire.snr_inband_db(_q(flags=1, sig_nb=64 * fs, n_noise=0), sl) == pytest.approx(90.0, abs=1e-9)
    assert acquire.snr_inband_db(_q(flags=1, sig_nb=64 * fs, n_noise=3), sl) == 50
    # the floor: power_off / (128 windows_off)
    floor = np.zeros(1, wideband.BURST_FLOOR_DTYPE)[0]
    floor["windows_off"], floor["power_off"] = 5, 5 * 128 * 255 ** 2 // 1000
    assert acquire.snr_floor_db(_q(sig=fs), floor, sl) == pytest.approx(30.0, abs=0.01)
    floor["windows_off"] = 0
    assert acquire.snr_floor_db(_q(sig=fs), floor, sl) == pytest.approx(90.0, abs=1e-9)
    floor["windows_off"], floor["power_off"] = 3, 0
    assert acquire.snr_floor_db(_q(sig=fs), floor, sl) == 50


def test_burst_packets_go_through_the_parsers_front_half():
    import rtldavis_amd
    sl, n = 14, 80
    X = QC.default_launch()
    datas = [DC.packet(n, seed=1 + c) for c in range(3)]
    recs = np.zeros(4, BURST_MSG_DTYPE)
    for c in range(3):
        recs[c] = X.msgs[c, 0]
        recs[c]["data"] = list(datas[c])
    recs[3] = recs[1]
    recs[3]["flags"] = wideband.BURST_MSG_REPAIRED
    quality = np.asarray([X.row(0), X.row(1), X.row(2), X.row(1)], QUALITY_DTYPE)
    per = rtldavis_amd.burst_packets(recs, quality, 3, sl)
    assert [len(p) for p in per] == [1, 1, 1]
    for c in range(3):
        p = per[c][0]
        assert p.index == -1 and bytes(p.data) == datas[c]
        assert p.rssi == acquire.rssi_db(X.row(c), sl) and p.snr == acquire.snr_db(X.row(c), sl)
        got = rtldavis_amd.parse_packet(p.data)
        assert got is not None and got[0] == synth_id(datas[c])
        assert -20 < p.rssi < -5 and math.isfinite(p.snr)          # amplitude 40 of 127.5: about -10 dB
    assert [len(p) for p in wideband.burst_packets(recs, quality, 3, sl, use_repaired=True)] == [1, 2, 1]
    inband = wideband.burst_packets(recs, quality, 3, sl, inband=True)
    assert inband[0][0].snr == acquire.snr_inband_db(X.row(0), sl) and inband[0][0].rssi == per[0][0].rssi
    with pytest.raises(ValueError):
        wideband.burst_packets(recs, quality[:3], 3, sl)


def synth_id(data):
    from rtldavis_amd import synth
    return synth._swap_bits8(data[2]) & 7


def test_hook_arguments_are_refused_before_any_device_work():
    from rtldavis_amd import _lib
    L = _lib.lib()
    X = QC.default_launch()
    out = np.zeros(X.want.size, QUALITY_DTYPE)

    def call(cfg, gap=0, n_msgs=X.n_msgs):
        c = _lib.make_config(cfg.bit_rate, cfg.symbol_length, cfg.preamble_symbols, cfg.packet_symbols, cfg.preamble, cfg.block_size)
        return L.rd_debug_burst_quality(C.byref(c), X.cur.ctypes.data, X.prev.ctypes.data, X.cur.shape[1], X.n_ch, gap, X.msgs.ctypes.data,
                                        np.ascontiguousarray(n_msgs, np.uint32).ctypes.data, out.ctypes.data)
    assert call(X.cfg, gap=-1) == _lib.RD_ERR_ARG and call(X.cfg, gap=1025) == _lib.RD_ERR_ARG and "noise_gap" in _lib.last_error()
    assert call(X.cfg, n_msgs=[1, X.cap + 1, 1]) == _lib.RD_ERR_ARG
    assert call(DC.config(14, 80, 1024)) == _lib.RD_ERR_ARG          # block_size below LOOK
    assert not out.tobytes().strip(b"\0")


def test_receiver_rules_that_need_no_device():
    rx = DC.device_receiver(2048)
    assert rx.burst_quality() == (False, 0)
    with pytest.raises(RuntimeError):
        rx.set_burst_quality(True)                             # decode is off
    rx.set_bursts(True)
    rx.set_burst_decode(True)
    for gap in (-1, 1025):
        with pytest.raises(ValueError):
            rx.set_burst_quality(True, gap)
    assert rx.burst_quality() == (False, 0)
    rx.set_burst_quality(True, 1024)
    assert rx.burst_quality() == (True, 1024)
    rx.reset()
    assert rx.burst_quality() == (True, 1024)                 # reset keeps it
    with pytest.raises(RuntimeError):
        rx.burst_message_quality()                             # no chunk fetched
    with pytest.raises(RuntimeError):
        rx.expected_message_quality()
    rx.set_burst_decode(False)
    assert rx.burst_quality()[0] is False
    rx.set_burst_decode(True)
    rx.set_burst_quality(True, 3)
    rx.set_bursts(False)
    assert rx.burst_quality()[0] is False
    rx.set_bursts(True)
    rx.set_burst_decode(True)
    rx.set_burst_quality(False, 9)
    assert rx.burst_quality() == (False, 9)


def test_estimators_stay_within_the_recorded_spread_of_the_model():
    """profiles/burst_quality_model.txt records, per noise level and estimator, the mean, the standard deviation over
    bursts and the spread of the recorded seeds' means (tools/burst_quality_model.py).  A seed that is not in the file
    must give a mean within 3 sd / sqrt(bursts) + that spread: three standard errors of its own mean, plus what the
    recorded seeds differ by among themselves."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("burst_quality_model", os.path.join(ROOT, "tools", "burst_quality_model.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rows = {}
    with open(os.path.join(ROOT, "profiles", "burst_quality_model.txt")) as fh:
        head = fh.readline()
        for line in fh:
            if not line.startswith("#"):
                left, *cells = line.split("|")
                rows[float(left.split()[0])] = (tuple(float(v) for v in left.split()[1:]), [tuple(float(v) for v in c.split()) for c in cells])
    assert "--seeds 7 8 9" in head and set(rows) == set(tool.NOISE)
    k, seed = 20, 11
    for noise in (0.06, 0.15, 0.30):
        planted, cells = rows[noise]
        assert planted == pytest.approx([round(v, 1) for v in tool.planted_db(noise)], abs=0.051)
        got = tool.estimates(k, noise, seed).mean(axis=0)
        for name, g, (mean, sd, spread) in zip(tool.ESTIMATORS, got, cells):
            print(f"noise {noise} {name}: {g:.2f} dB, recorded {mean:.2f} (sd {sd:.2f}, seed spread {spread:.2f})")
            assert abs(g - mean) <= 3 * sd / math.sqrt(k) + spread + 0.005, (noise, name, g, mean, sd, spread)      # (0.005: the file's rounding)
    # what the figures say: the reference's window holds the lead-in (0 dB); past it the estimators follow (S + N) / N
    for noise, (planted, cells) in rows.items():
        ch, nb = planted
        assert abs(cells[0][0]) < 0.1
        assert abs(cells[1][0] - 10 * math.log10(1 + 10 ** (ch / 10))) < 0.5 and abs(cells[3][0] - cells[1][0]) < 0.5
        assert abs(cells[2][0] - 10 * math.log10(1 + 10 ** (nb / 10))) < 1.5
