"""Burst detection and coarse acquisition, the part that needs no GPU: the model of k_chan_bursts on hand-made bytes,
the estimator and the closed loop on the float64 channelizer model's bytes, acquire.merge and acquire.Acquisition on
made-up records, and the argument and state errors through the C ABI (host bookkeeping: no device is touched).
The device's records are compared with the same model in tests/test_wideband_bursts.py."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import burst_cases as BC
import retune_cases as RC
from rtldavis_amd import acquire
from rtldavis_amd.wideband import BURST_DTYPE, BURST_FLOOR_DTYPE, BURST_THRESHOLD_OFF, Bursts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = BC.W


# ------------------------------------------------------------------------------------------ the model on hand-made bytes
def _bytes(levels, seed=5):
    """One channel whose window w holds a tone of amplitude levels[w] (byte steps) plus +-1 dither: p_w grows with it."""
    rng = np.random.default_rng(seed)
    t = np.arange(W)
    out = np.empty(2 * W * len(levels), np.uint8)
    for w, a in enumerate(levels):
        z = a * np.exp(2j * np.pi * (0.11 * t + 0.3 * w))
        out[2 * W * w: 2 * W * (w + 1): 2] = np.clip(np.rint(127.5 + z.real + rng.integers(-1, 2, W)), 0, 255)
        out[2 * W * w + 1: 2 * W * (w + 1): 2] = np.clip(np.rint(127.5 + z.imag + rng.integers(-1, 2, W)), 0, 255)
    return out[None, :]


LOUD, QUIET, THR = 60, 2, 4 * W * 30 * 30      # p of a loud window ~ 4 x 128 x 60^2, of a quiet one < 4 x 128 x 4^2


def _runs(levels, thr=THR):
    recs, floor = BC.burst_model(_bytes(levels), thr)
    return [(int(r["first"]), int(r["windows"]), int(r["flags"])) for r in recs], floor[0]


def test_window_sums_from_the_definition():
    """p and r of the model against a plain complex evaluation, and their stated ranges at the extreme bytes."""
    rng = np.random.default_rng(1)
    b = rng.integers(0, 256, (3, 2 * W * 5), dtype=np.uint8)
    p, re, im = BC.window_sums(b)
    z = (2.0 * b[:, 0::2] - 255) + 1j * (2.0 * b[:, 1::2] - 255)
    for c in range(3):
        for w in range(5):
            zw = z[c, W * w: W * (w + 1)]
            r = (zw[1:] * np.conj(zw[:-1])).sum()
            assert p[c, w] == round((np.abs(zw) ** 2).sum()) and re[c, w] == round(r.real) and im[c, w] == round(r.imag)
    full = np.full((1, 2 * W), 255, np.uint8)
    p, re, im = BC.window_sums(full)
    assert p[0, 0] == 16646400 and re[0, 0] == 254 * 65025 and im[0, 0] == 0
    alt = np.tile(np.asarray([255, 0, 0, 0, 0, 255, 255, 255], np.uint8), W // 4)[None, :]   # z = 255 (1-j), (-1-j), (-1+j), (1+j)
    p, re, im = BC.window_sums(alt)
    assert re[0, 0] == 0 and im[0, 0] == -127 * 2 * 65025                                     # a quarter turn back per output


def test_the_kernels_byte_identities():
    """What k_chan_bursts computes from the bytes (rd_bursts.hip, header): packed-byte dot products of the window's byte
    stream with itself, with ones and with itself 1, 2 and 3 bytes back (zeros in front of the window), then
    p = 4 S2 - 1020 S1 + 256 x 65025, re r = 4 X2 - 510 (2 S1 - b0 - b1 - b254 - b255) + 254 x 65025,
    im r = 4 (X3 - X1) - 510 (b0 - b1 - b254 + b255) - equal to the definition on random and on extreme bytes."""
    rng = np.random.default_rng(2)
    blocks = [rng.integers(0, 256, (4, 2 * W * 3), dtype=np.uint8), np.zeros((1, 2 * W), np.uint8), np.full((1, 2 * W), 255, np.uint8),
              rng.choice(np.asarray([0, 255], np.uint8), (3, 2 * W * 2))]
    for block in blocks:
        p, re, im = BC.window_sums(block)
        b = block.astype(np.int64).reshape(block.shape[0], -1, 2 * W)
        back = lambda s: np.concatenate([np.zeros(b.shape[:2] + (s,), np.int64), b[:, :, : 2 * W - s]], axis=2)
        odd = np.arange(2 * W) % 2 == 1
        s1, s2 = b.sum(axis=2), (b * b).sum(axis=2)
        x2 = (b * back(2)).sum(axis=2)
        x3 = (b * back(3))[:, :, odd].sum(axis=2)
        x1 = (b * back(1))[:, :, ~odd].sum(axis=2)
        b0, b1, b254, b255 = b[:, :, 0], b[:, :, 1], b[:, :, 254], b[:, :, 255]
        assert np.array_equal(p, 4 * s2 - 1020 * s1 + 256 * 65025)
        assert np.array_equal(re, 4 * x2 - 510 * (2 * s1 - b0 - b1 - b254 - b255) + 254 * 65025)
        assert np.array_equal(im, 4 * (x3 - x1) - 510 * (b0 - b1 - b254 + b255))
        assert p.max() <= 16646400 and np.abs(re).max() <= 254 * 65025 and np.abs(im).max() <= 254 * 65025


def test_model_all_off_and_all_on():
    levels = [LOUD, QUIET, LOUD, LOUD, QUIET, QUIET]
    block = _bytes(levels)
    p, re, im = BC.window_sums(block)
    recs, floor = BC.burst_model(block, BURST_THRESHOLD_OFF)
    assert recs.size == 0 and recs.dtype == BURST_DTYPE
    f = floor[0]
    assert (f["threshold"], f["windows_off"], f["n_bursts"]) == (BURST_THRESHOLD_OFF, 6, 0)
    assert (f["power_off"], f["corr_re_off"], f["corr_im_off"]) == (p.sum(), re.sum(), im.sum())
    recs, floor = BC.burst_model(block, 0)
    assert recs.size == 1 and floor[0]["windows_off"] == 0 and floor[0]["n_bursts"] == 1 and floor[0]["power_off"] == 0
    r = recs[0]
    assert (r["channel"], r["first"], r["windows"], r["flags"], r["pad"]) == (0, 0, 6, 3, 0)
    assert (r["power"], r["peak"], r["corr_re"], r["corr_im"]) == (p.sum(), p.max(), re.sum(), im.sum())


@pytest.mark.parametrize("n_win", [6, 7])
def test_model_alternating_windows(n_win):
    levels = [LOUD if w % 2 == 0 else QUIET for w in range(n_win)]
    runs, f = _runs(levels)
    assert len(runs) == -(-n_win // 2) == f["n_bursts"] and f["windows_off"] == n_win // 2
    assert [r[0] for r in runs] == list(range(0, n_win, 2)) and all(r[1] == 1 for r in runs)
    assert runs[0][2] == 1 and runs[-1][2] == (2 if n_win % 2 else 0) and all(r[2] == 0 for r in runs[1:-1])


def test_model_runs_touching_one_end():
    assert _runs([LOUD, LOUD, QUIET, QUIET, QUIET])[0] == [(0, 2, 1)]
    assert _runs([QUIET, QUIET, LOUD, LOUD, LOUD])[0] == [(2, 3, 2)]
    assert _runs([QUIET, LOUD, LOUD, QUIET, LOUD, QUIET])[0] == [(1, 2, 0), (4, 1, 0)]


def test_model_one_window_and_the_threshold_is_inclusive():
    block = _bytes([LOUD])
    p = int(BC.window_sums(block)[0][0, 0])
    recs, floor = BC.burst_model(block, p)
    assert [(r["first"], r["windows"], r["flags"]) for r in recs] == [(0, 1, 3)] and floor[0]["windows_off"] == 0
    recs, floor = BC.burst_model(block, p + 1)
    assert recs.size == 0 and floor[0]["windows_off"] == 1 and floor[0]["power_off"] == p


def test_model_per_channel_thresholds_and_order():
    block = np.concatenate([_bytes([LOUD, QUIET, LOUD], 1), _bytes([QUIET, LOUD, LOUD], 2), _bytes([LOUD, LOUD, LOUD], 3)])
    recs, floor = BC.burst_model(block, [THR, THR, BURST_THRESHOLD_OFF], chunk=9)
    assert [(r["channel"], r["first"], r["windows"]) for r in recs] == [(0, 0, 1), (0, 2, 1), (1, 1, 2)]
    assert list(floor["n_bursts"]) == [2, 1, 0] and list(floor["chunk"]) == [9, 9, 9]
    assert list(floor["threshold"]) == [THR, THR, BURST_THRESHOLD_OFF]


# ------------------------------------------------------------------------------------------ estimator and closed loop on the model
@functools.lru_cache(maxsize=None)
def _open_loop(planted):
    """The model's blocks of the capture with no retune, and the thresholds Acquisition takes from chunk 0's floor."""
    lc = BC.acq_capture(planted)
    blocks = RC.loop_model_blocks(lc, {})
    thr = BC.new_acquisition().thresholds(BC.burst_model(blocks[0], BURST_THRESHOLD_OFF)[1])
    return lc, blocks, thr


@pytest.mark.parametrize("planted", BC.PLANTED)
def test_estimator_on_the_model(planted):
    """Both bursts of the capture, found with thresholds from chunk 0's floor: each a run of packet length whose
    estimate lies within 1500 Hz of the planted offset."""
    lc, blocks, thr = _open_loop(planted)
    acq = BC.new_acquisition()
    found = []
    for k, block in enumerate(blocks):
        b = BC.model_bursts(block, thr, k)
        for r in b.records:
            if acq.min_windows <= r["windows"] <= acq.max_windows:
                found.append((k, acquire.burst_offset_hz(r, b.floor[0], acq.out_rate, acq.if_hz)))
    print(f"\n[bursts model] planted {planted} Hz: " + ", ".join(f"chunk {k}: {e:.0f} Hz ({e - planted:+.0f})" for k, e in found))
    assert [k for k, _ in found] == [s // RC.LOOP_B for _, s in lc.info] == [1, 4]
    for _, e in found:
        assert abs(e - planted) <= BC.ESTIMATE_TOL_HZ


@pytest.mark.parametrize("planted", BC.PLANTED)
def test_closed_loop_on_the_model(planted):
    """No retune: no message.  Acquisition(need=1), fed in the device test's order, asks once, for a retune that holds
    from chunk 4; with it the second burst is CRC-valid, with the planted payload, where the dsp oracle finds it."""
    from oracle import dsp_oracle as O
    lc, blocks, thr = _open_loop(planted)
    assert RC.loop_messages(blocks) == []
    cfg = O.OracleConfig(19200, 14, 16, 80, RC.PREAMBLE, RC.LOOP_B)
    acq = BC.new_acquisition(need=1)
    st = dict(blocks=blocks, rows=[[]] * RC.LOOP_NK, submitted=0, fetched=0)

    def submit(k):
        st["submitted"] += 1

    def fetch():
        k = st["fetched"]
        st["fetched"] += 1
        return BC.model_bursts(st["blocks"][k], thr, k), st["rows"][k]

    def retune(off):                                     # holds from the next chunk submitted; the chunks before are as they were
        st["blocks"] = RC.loop_model_blocks(lc, {st["submitted"]: off})
        st["rows"] = [[r for r in call if r[2]] for call in O.parse_calls(st["blocks"], cfg)]

    asked = BC.run_loop(RC.LOOP_NK, submit, fetch, acq, retune)
    assert len(asked) == 1 and asked[0][0] == RC.LOOP_RETUNE_CHUNK == acq.valid_from
    est = asked[0][1]
    assert abs(est - planted) <= BC.ESTIMATE_TOL_HZ and acq.offset == est
    assert all(np.array_equal(x, y) for x, y in zip(st["blocks"][: RC.LOOP_RETUNE_CHUNK], blocks))
    assert [(k, r[1]) for k, call in enumerate(st["rows"]) for r in call] == [(5, lc.payload)]
    assert acq.locked                                    # the message of chunk 5 ends the acquisition
    print(f"\n[bursts loop model] planted {planted} Hz: estimate {est} Hz, residual freq_err {st['rows'][5][0][4]} Hz")


# ------------------------------------------------------------------------------------------ merge
def _rec(channel, first, windows, flags, power=1000, peak=300, re=50, im=-70):
    return np.asarray([(channel, first, windows, flags, power, peak, 0, re, im)], BURST_DTYPE)[0]


def test_merge_joins_a_run_split_at_the_boundary():
    """A block of 12 windows cut into two chunks of 6: the run across the cut, merged, equals the uncut run."""
    levels = [QUIET, LOUD, QUIET, QUIET, LOUD, LOUD, LOUD, LOUD, QUIET, LOUD, QUIET, LOUD]
    whole = _bytes(levels)
    a, b = whole[:, : 2 * W * 6], whole[:, 2 * W * 6:]
    want = BC.burst_model(whole, THR)[0]
    ra, rb = BC.burst_model(a, THR)[0], BC.burst_model(b, THR)[0]
    done_a, tail = acquire.merge(None, ra)
    assert [int(r["first"]) for r in done_a] == [1] and [int(r["first"]) for r in tail] == [4]
    done_b, tail_b = acquire.merge(tail, rb)
    assert [int(r["first"]) for r in tail_b] == [5] and int(tail_b[0]["flags"]) == 2
    joined = done_b[0]
    uncut = want[1]
    assert (uncut["first"], uncut["windows"]) == (4, 4)
    for f in ("windows", "power", "peak", "corr_re", "corr_im"):
        assert joined[f] == uncut[f] == (max(ra[1][f], rb[0][f]) if f == "peak" else ra[1][f] + rb[0][f]), f
    assert (joined["first"], joined["flags"]) == (4, 0)
    assert [(int(r["first"]), int(r["windows"])) for r in done_b[1:]] == [(3, 1)]
    assert np.array_equal(rb, BC.burst_model(b, THR)[0])                                 # (the input is not written to)


def test_merge_without_a_partner_and_across_channels():
    tail = np.asarray([_rec(0, 60, 4, 2), _rec(2, 63, 1, 2)])
    nxt = np.asarray([_rec(1, 0, 3, 1), _rec(2, 0, 64, 3, power=7, peak=400, re=1, im=1)])
    done, new_tail = acquire.merge(tail, nxt)
    assert [(int(r["channel"]), int(r["first"]), int(r["windows"])) for r in done] == [(0, 60, 4), (1, 0, 3)]
    t = new_tail[0]
    assert new_tail.size == 1 and (t["channel"], t["first"], t["windows"], t["flags"]) == (2, 63, 65, 2)
    assert (t["power"], t["peak"], t["corr_re"], t["corr_im"]) == (1007, 400, 51, -69)


# ------------------------------------------------------------------------------------------ Acquisition
CFG = RC.packet_config(8192)
OUT_RATE, IF_HZ = 268800, -67200


def _at(hz, mag=10 ** 6):
    """corr_re, corr_im of a burst `hz` off the channel centre."""
    ph = 2 * np.pi * (hz + IF_HZ) / OUT_RATE
    return int(round(mag * np.cos(ph))), int(round(mag * np.sin(ph)))


def _chunk(k, runs, n_ch=3, n_win=64):
    """Bursts of chunk k: runs = [(channel, first, windows, Hz)]; a quiet floor."""
    recs = [_rec(c, a, n, (1 if a == 0 else 0) | (2 if a + n == n_win else 0), 10 ** 6 * n, 10 ** 6, *_at(hz)) for c, a, n, hz in runs]
    floor = np.zeros(n_ch, BURST_FLOOR_DTYPE)
    floor["threshold"], floor["windows_off"], floor["chunk"], floor["power_off"] = 2000, n_win, k, 500 * n_win
    return Bursts(np.asarray(recs, BURST_DTYPE).reshape(-1), floor, k)


def _valid(*channels):
    return np.asarray([(c,) for c in channels], np.dtype([("stream", np.int32)]))


def test_burst_offset_hz_and_its_debias():
    floor = _chunk(0, [])[1][0]
    for hz in (0, 4000, -20000, 38000, -60000, 190000):
        assert abs(acquire.burst_offset_hz(_rec(0, 5, 12, 0, 1, 1, *_at(hz)), floor, OUT_RATE, IF_HZ) - hz) < 0.5
    # the floor's own correlation, scaled to the run's length, is taken off: a run that is all floor plus a burst
    floor = floor.copy()
    floor["corr_re_off"], floor["corr_im_off"], floor["windows_off"] = 64 * 3000, 64 * -2000, 64
    re, im = _at(20000)
    rec = _rec(0, 5, 12, 0, 1, 1, re + 12 * 3000, im - 12 * 2000)
    assert abs(acquire.burst_offset_hz(rec, floor, OUT_RATE, IF_HZ) - 20000) < 0.5
    floor["windows_off"] = 0                                                            # no OFF window: no correction
    assert abs(acquire.burst_offset_hz(_rec(0, 0, 64, 3, 1, 1, re, im), floor, OUT_RATE, IF_HZ) - 20000) < 0.5


def test_acquisition_defaults_and_thresholds():
    acq = acquire.Acquisition(3, CFG)
    assert (acq.factor, acq.need, acq.min_windows, acq.max_windows, acq.out_rate, acq.if_hz) == (4, 3, 8, 18, OUT_RATE, IF_HZ)
    floor = _chunk(0, [])[1]
    floor["power_off"] = [64 * 500, 64 * 700 + 5, 123456]
    floor["windows_off"] = [64, 64, 0]
    t = acq.thresholds(floor)
    assert t.dtype == np.uint32 and list(t) == [2000, 4 * (64 * 700 + 5) // 64, BURST_THRESHOLD_OFF]
    floor["windows_off"] = [0, 1, 64]
    floor["power_off"] = [1, 2 ** 40, 640]
    assert list(acq.thresholds(floor)) == [2000, BURST_THRESHOLD_OFF, 40]                 # kept, clamped, new
    with pytest.raises(ValueError):
        acq.thresholds(floor[:2])
    for bad in (dict(n_channels=0), dict(need=0), dict(factor=0), dict(min_windows=0), dict(min_windows=9, max_windows=8)):
        with pytest.raises(ValueError):
            acquire.Acquisition(**{"n_channels": 3, "cfg": CFG, **bad})


def test_acquisition_stays_silent_below_need_then_proposes_the_median():
    acq = acquire.Acquisition(3, CFG, need=3)
    assert acq.update(_chunk(0, [(0, 5, 12, 20100), (2, 30, 13, 19900)]), _valid(), 2) is None
    assert acq.update(_chunk(1, [(1, 8, 12, 30000), (1, 40, 3, -50000), (0, 20, 25, -50000)]), _valid(), 3) is None   # two estimates so far
    assert len(acq.estimates) == 2
    new = acq.update(_chunk(2, []), _valid(), 4)           # chunk 1's candidate of plausible length has waited its chunk
    assert new == 20100 and acq.offset == 20100 and acq.valid_from == 4 and acq.estimates == []
    # the next proposals are relative to the plan: offset + median
    for k in (4, 5, 6):
        assert acq.update(_chunk(k, [(0, 5, 12, -300)]), _valid(), k + 2) is None
    assert acq.update(_chunk(7, []), _valid(), 9) == 19800 and acq.valid_from == 9


def test_acquisition_ignores_chunks_older_than_its_retune():
    acq = acquire.Acquisition(3, CFG, need=1)
    assert acq.update(_chunk(0, [(0, 5, 12, 20000)]), _valid(), 2) is None
    assert acq.update(_chunk(1, [(0, 5, 12, 20000)]), _valid(), 3) == 20000 and acq.valid_from == 3
    # chunks 1 (its candidate went with the proposal) and 2 were submitted under the old tuning: nothing of them counts
    assert acq.update(_chunk(2, [(1, 5, 12, 20000)]), _valid(), 4) is None
    assert acq.update(_chunk(3, [(1, 5, 12, 150)]), _valid(), 5) is None and acq.estimates == []
    assert acq.update(_chunk(4, []), _valid(), 6) == 20150                                # chunk 3's, under the new tuning
    # a gap in the chunk numbers (a fetch that timed out) drops what waited
    acq = acquire.Acquisition(3, CFG, need=1)
    assert acq.update(_chunk(0, [(0, 5, 12, 20000)]), _valid(), 2) is None
    assert acq.update(_chunk(2, []), _valid(), 4) is None and acq.estimates == []


def test_acquisition_ignores_channels_with_a_valid_message_and_locks():
    """A burst whose message arrives - with its own chunk or the next - never becomes an estimate, and from then on
    nothing is proposed: the AFC has messages to work with."""
    for late in (0, 1):
        acq = acquire.Acquisition(3, CFG, need=1)
        rows = [_valid(1) if late == 0 else _valid(), _valid(1) if late == 1 else _valid()]
        assert acq.update(_chunk(0, [(1, 5, 12, 900)]), rows[0], 2) is None
        assert acq.update(_chunk(1, []), rows[1], 3) is None
        assert acq.locked and acq.estimates == [] and acq.offset == 0
        for k in (2, 3, 4):
            assert acq.update(_chunk(k, [(0, 5, 12, 20000)]), _valid(), k + 2) is None
        acq.reset()
        assert not acq.locked
        assert acq.update(_chunk(5, [(0, 5, 12, 20000)]), _valid(), 7) is None
        assert acq.update(_chunk(6, []), _valid(), 8) == 20000
    # without the message the same burst is proposed
    acq = acquire.Acquisition(3, CFG, need=1)
    acq.update(_chunk(0, [(1, 5, 12, 900)]), _valid(), 2)
    assert acq.update(_chunk(1, []), _valid(), 3) == 900


def test_acquisition_joins_a_run_across_the_boundary():
    acq = acquire.Acquisition(3, CFG, need=1)
    assert acq.update(_chunk(0, [(2, 58, 6, 20000)]), _valid(), 2) is None               # 6 windows: too short alone, and it may go on
    assert acq.update(_chunk(1, [(2, 0, 6, 20000)]), _valid(), 3) is None                 # 12 windows: a candidate now
    assert acq.update(_chunk(2, []), _valid(), 4) == 20000


# ------------------------------------------------------------------------------------------ C ABI without a device
def _receiver(bs=1024, decim=100, n_ch=2):
    from rtldavis_amd import wideband
    chans = [RC.CENTRE - 100000 + 50000 * c for c in range(n_ch)]
    return wideband.WidebandReceiver(RC.packet_config(bs), chans, RC.CENTRE, decim=decim, taps=np.ones(8) / 8)


def test_threshold_arguments():
    from rtldavis_amd import _lib
    L = _lib.lib()
    w = _receiver()
    assert w.burst_thresholds().dtype == np.uint32 and list(w.burst_thresholds()) == [BURST_THRESHOLD_OFF] * 2
    w.set_burst_threshold(5)
    assert list(w.burst_thresholds()) == [5, 5]
    w.set_burst_threshold([0, 2 ** 32 - 1])
    w.set_burst_threshold(np.asarray([7, 9], np.uint64))
    kept = [7, 9]
    for bad in ([1], [1, 2, 3], [[1, 2]], -1, 2 ** 32, [0, -1], [0, 2 ** 32], 1.0, [1.0, 2.0], "5", None):
        with pytest.raises(ValueError):
            w.set_burst_threshold(bad)
        assert list(w.burst_thresholds()) == kept, bad
    t = np.asarray(kept, np.uint32)
    assert L.rd_wb_set_burst_threshold(w._h, t.ctypes.data, 1) == _lib.RD_ERR_ARG
    assert L.rd_wb_set_burst_threshold(w._h, t.ctypes.data, 3) == _lib.RD_ERR_ARG
    assert L.rd_wb_set_burst_threshold(w._h, None, 2) == _lib.RD_ERR_ARG
    assert L.rd_wb_set_burst_threshold(None, t.ctypes.data, 2) == _lib.RD_ERR_ARG
    assert L.rd_wb_burst_thresholds(w._h, t.ctypes.data, 3) == _lib.RD_ERR_ARG
    assert L.rd_wb_burst_thresholds(w._h, None, 2) == _lib.RD_ERR_ARG
    assert L.rd_wb_burst_thresholds(None, t.ctypes.data, 2) == _lib.RD_ERR_ARG
    assert list(w.burst_thresholds()) == kept
    w.reset()                                                                            # the default table, no device needed
    assert list(w.burst_thresholds()) == [BURST_THRESHOLD_OFF] * 2


def test_bursts_before_any_fetch_and_the_window_limit():
    from rtldavis_amd import _lib
    L = _lib.lib()
    w = _receiver()
    assert w.submitted == 0
    with pytest.raises(RuntimeError):
        w.bursts()                                                                       # off, nothing fetched
    w.set_bursts(True)
    with pytest.raises(RuntimeError):
        w.bursts()                                                                       # on, nothing fetched
    assert "no chunk fetched" in _lib.last_error()
    n = C.c_int(-1)
    recs = np.empty(4, BURST_DTYPE)
    floor = np.empty(2, BURST_FLOOR_DTYPE)
    assert L.rd_wb_bursts(w._h, recs.ctypes.data, 4, C.byref(n), floor.ctypes.data, 2) == _lib.RD_ERR_STATE
    assert L.rd_wb_bursts(w._h, recs.ctypes.data, 4, C.byref(n), floor.ctypes.data, 3) == _lib.RD_ERR_ARG
    assert L.rd_wb_bursts(w._h, None, 4, C.byref(n), None, 0) == _lib.RD_ERR_ARG
    assert L.rd_wb_bursts(w._h, recs.ctypes.data, -1, C.byref(n), None, 0) == _lib.RD_ERR_ARG
    assert L.rd_wb_bursts(w._h, recs.ctypes.data, 4, None, None, 0) == _lib.RD_ERR_ARG
    assert L.rd_wb_bursts(None, recs.ctypes.data, 4, C.byref(n), None, 0) == _lib.RD_ERR_ARG
    assert L.rd_wb_set_bursts(None, 1) == _lib.RD_ERR_ARG
    w.set_bursts(False)
    w.reset()
    with pytest.raises(RuntimeError):
        w.bursts()
    # 4096 windows are the most; a longer chunk is refused when bursts are switched on, and only then
    w.set_bursts(True)
    ok = _receiver(bs=128 * 4096, decim=4, n_ch=1)
    ok.set_bursts(True)
    big = _receiver(bs=128 * 4097, decim=4, n_ch=1)
    big.set_bursts(False)
    with pytest.raises(ValueError):
        big.set_bursts(True)
    assert "4096" in _lib.last_error()
    assert L.rd_wb_set_bursts(big._h, 1) == _lib.RD_ERR_ARG
    big.set_burst_threshold(1)                                                           # (the table itself has no such limit)


def test_symbols_layouts_and_the_ctypes_table():
    from rtldavis_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtldavis_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    protos = {
        "rd_wb_set_bursts": r"int\s+rd_wb_set_bursts\s*\(\s*rd_wideband\s*\*\s*w\s*,\s*int\s+enabled\s*\)",
        "rd_wb_set_burst_threshold": r"int\s+rd_wb_set_burst_threshold\s*\(\s*rd_wideband\s*\*\s*w\s*,\s*const\s+uint32_t\s*\*\s*thr\s*,\s*int\s+n\s*\)",
        "rd_wb_burst_thresholds": r"int\s+rd_wb_burst_thresholds\s*\(\s*rd_wideband\s*\*\s*w\s*,\s*uint32_t\s*\*\s*thr\s*,\s*int\s+n\s*\)",
        "rd_wb_bursts": r"int\s+rd_wb_bursts\s*\(\s*rd_wideband\s*\*\s*w\s*,\s*rd_burst\s*\*\s*out\s*,\s*int\s+cap\s*,\s*int\s*\*\s*n\s*,\s*rd_burst_floor\s*\*\s*floor\s*,\s*int\s+n_floor\s*\)",
    }
    for name, proto in protos.items():
        assert re.search(proto, src), name
        assert name in _lib.SIGNATURES and hasattr(L, name)
    for struct, ctype, dtype, size in (("rd_burst", _lib.RdBurst, BURST_DTYPE, 48), ("rd_burst_floor", _lib.RdBurstFloor, BURST_FLOOR_DTYPE, 40)):
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}" % struct, src, flags=re.S).group(1)
        names = [n for decl in body.split(";") for n in re.sub(r"^\s*\w+\s+", "", decl.strip()).replace(" ", "").split(",") if n]
        assert names == [f for f, _ in ctype._fields_] == list(dtype.names), struct
        assert C.sizeof(ctype) == dtype.itemsize == size
        assert [getattr(ctype, f).offset for f in names] == [dtype.fields[f][1] for f in names]
        assert [C.sizeof(t) for _, t in ctype._fields_] == [dtype.fields[f][0].itemsize for f in names]


# ------------------------------------------------------------------------------------------ crafted bytes
def test_crafted_cases_reach_their_edges():
    """burst_cases.crafted_small / crafted_largest build every case with its condition asserted on the model; here the
    conditions that span cases, and the slot the hook must hand back."""
    cases = {cs.name: cs for cs in BC.crafted_small() + (BC.crafted_largest(),)}
    assert {cs.n_win for cs in cases.values()} >= {1, 15, 16, 17, 63, 64, 65, 129, 192, 193, 256, 4096}
    assert any(cs.stride == 2 * cs.n_out + 16 and np.all(cs.chan[:, 2 * cs.n_out:] == 255) for cs in cases.values())
    assert all(2 <= cs.n_ch <= 4 for cs in cases.values())
    for cs in cases.values():
        recs, floor = BC.slot_model(cs)
        cap = BC.cap_of(cs.n_win)
        assert recs.shape == (cs.n_ch, cap) and floor.shape == (cs.n_ch,)
        for c in range(cs.n_ch):
            n = int(floor["n_bursts"][c])
            assert np.all(recs[c, :n]["channel"] == c) and np.all(np.diff(recs[c, :n]["first"].astype(np.int64)) > 1)
            assert recs[c, n:].tobytes() == bytes([BC.FILL]) * ((cap - n) * BURST_DTYPE.itemsize)
            assert int(floor["windows_off"][c]) + int(recs[c, :n]["windows"].sum()) == cs.n_win
    # an odd window count with every place filled, and a carried run that is carried again in every long-run channel
    assert cases["alternating_w129"].floor["n_bursts"][0] == 65 == BC.cap_of(129)
    assert all(BC._groups_between(r) for n in (193, 256) for r in cases[f"long_runs_w{n}"].records)
    # the largest sums: 32 bits are not enough for a run's power, 2^31 not for its correlation
    big = cases["largest_w4096"]
    assert int(big.records["power"][0]) == 68183654400 > 2 ** 32 and int(big.records["corr_re"][1]) == -67650969600 < -2 ** 31
    assert big.floor["chunk"][0] == 9                        # the low 32 bits of seq


def test_debug_bursts_refuses_what_rd_bursts_check_refuses():
    """The hook's argument rule is rd_bursts_check's, before any device work: no GPU needed."""
    from rtldavis_amd import _lib
    L = _lib.lib()
    chan = np.full(4096, 127, np.uint8)
    thr = np.zeros(1, np.uint32)
    recs, floor = np.zeros(8, BURST_DTYPE), np.zeros(1, BURST_FLOOR_DTYPE)
    for n_out in BC.BAD_N_OUT:
        stride = max(16, 2 * n_out + (-2 * n_out) % 16)
        assert L.rd_debug_bursts(chan.ctypes.data, stride, 1, n_out, thr.ctypes.data, 0, recs.ctypes.data,
                                 floor.ctypes.data) == _lib.RD_ERR_ARG, n_out
        assert "bursts" in _lib.last_error()
    assert L.rd_debug_bursts(chan.ctypes.data, 256 + 8, 1, 128, thr.ctypes.data, 0, recs.ctypes.data, floor.ctypes.data) == _lib.RD_ERR_ARG
    assert L.rd_debug_bursts(chan.ctypes.data, 240, 1, 128, thr.ctypes.data, 0, recs.ctypes.data, floor.ctypes.data) == _lib.RD_ERR_ARG
    assert L.rd_debug_bursts(None, 256, 1, 128, thr.ctypes.data, 0, recs.ctypes.data, floor.ctypes.data) == _lib.RD_ERR_ARG
    assert not recs.tobytes().strip(b"\0") and not floor.tobytes().strip(b"\0")      # nothing was written
