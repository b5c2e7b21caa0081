"""Burst detection on the device (rd_wb_set_bursts -> k_chan_bursts, rd_bursts.hip): every record and floor row of every
chunk equal to the integer model (tests/burst_cases.py) of the receiver's own channelized bytes - the retune cases'
plans (one window per chunk, eight, 70 channels, int16 input) and chunks of 65 and 128 windows, where runs cross the
64 windows the kernel takes at a time -; thresholds that change with chunks in flight; bursts off; the acquisition loop
closed through bursts() and retune(); and bit-identical records from run to run."""
import functools

import numpy as np
import pytest

import burst_cases as BC
import chan_bound as CB
import retune_cases as RC
from rtldavis_amd.wideband import BURST_THRESHOLD_OFF
from stream_parse_helpers import _rows

pytestmark = pytest.mark.gpu
W = BC.W


def _device():
    from rtldavis_amd import _lib
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"


def _feed(w, chunks, thr=None):
    """reset, set the thresholds, feed the chunks one at a time: [(channelized bytes, Bursts)] per chunk."""
    w.reset()
    if thr is not None:
        w.set_burst_threshold(thr)
    out = []
    for chunk in chunks:
        w.demodulate(chunk)
        out.append((w.channelized(), w.bursts()))
    return out


def _check(run, thr):
    for k, (block, got) in enumerate(run):
        BC.assert_equals_model(got, block, thr, k)


@pytest.mark.parametrize("name", list(RC.CASES))
def test_records_equal_the_model(name):
    """With the default thresholds the floor covers every window; with each channel's threshold at the median of its
    window energies about half the windows are ON, in runs of every length the capture happens to hold."""
    _device()
    cs = RC.case(name)
    w = RC.receiver(cs)
    w.set_bursts(True)
    first = _feed(w, cs.chunks)
    _check(first, BURST_THRESHOLD_OFF)
    n_win = cs.bs // W
    assert all(b.records.size == 0 and np.all(b.floor["windows_off"] == n_win) for _, b in first)
    thr = BC.median_thresholds(np.concatenate([block for block, _ in first], axis=1))
    second = _feed(w, cs.chunks, thr)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(first, second))
    _check(second, thr)
    n_on = sum(int(b.records["windows"].sum()) for _, b in second)
    assert 0.4 * cs.n_ch * cs.nk * n_win <= n_on <= 0.6 * cs.n_ch * cs.nk * n_win + cs.n_ch
    if n_win == 1:
        assert all(np.all(b.records["flags"] == 3) for _, b in second)


# ------------------------------------------------------------------------------------------ 65 and 128 windows per chunk
# Chunk 0 of each capture is loud over the listed windows (inclusive) and 26 dB down elsewhere, chunk 1 is loud
# throughout.  The loud stretch begins half a window early: the 256 taps reach 64 outputs back, so the window in front of a
# run and the one behind it hold about a quarter of a loud window's energy, and a threshold at 0.55 of the loud windows'
# median puts exactly the listed windows ON.
LONG = {
    (65, "a"): [(0, 1), (5, 5), (20, 63)],               # a run that ends at window 63 with window 64 OFF: written by lane 0 of the next 64
    (65, "b"): [(3, 10), (30, 64)],                      # a run carried over window 63 that ends with the chunk
    (128, "a"): [(0, 2), (40, 63), (66, 66), (100, 127)],
    (128, "b"): [(10, 70), (127, 127)],                  # carried, and ended inside the next 64
}


@functools.lru_cache(maxsize=None)
def _long_capture(n_win, which):
    cs = RC.case("d4_t256_b128")
    bs = W * n_win
    n = 2 * bs * cs.decim
    raw = CB.capture(n, 1000 + n_win + ord(which), cs.fw).astype(np.float64).reshape(-1, 2)
    env = np.full(n, 0.05)
    for a, e in LONG[(n_win, which)]:
        env[max(0, (W * a - W // 2) * cs.decim): W * (e + 1) * cs.decim] = 1.0
    env[bs * cs.decim:] = 1.0
    raw = np.clip(np.rint(127.4 + (raw - 127.4) * env[:, None]), 0, 255).astype(np.uint8).reshape(-1)
    step = 2 * bs * cs.decim
    return cs, bs, [raw[:step], raw[step:]]


@pytest.mark.parametrize("n_win,which", list(LONG))
def test_runs_across_the_64_window_groups(n_win, which):
    _device()
    from rtldavis_amd import wideband
    cs, bs, chunks = _long_capture(n_win, which)
    w = wideband.WidebandReceiver(RC.packet_config(bs, cs.sl), cs.chans, RC.CENTRE, decim=cs.decim, taps=cs.user_taps, gain=cs.gain)
    w.set_bursts(True)
    first = _feed(w, chunks)
    _check(first, BURST_THRESHOLD_OFF)
    p = BC.window_sums(first[0][0])[0]
    loud = np.concatenate([np.arange(a, e + 1) for a, e in LONG[(n_win, which)]])
    thr = (0.55 * np.median(p[:, loud], axis=1)).astype(np.uint64)
    designed = _feed(w, chunks, thr)
    _check(designed, thr)
    got = designed[0][1].records
    for c in range(cs.n_ch):                             # the designed runs are what the device found, on every channel
        mine = got[got["channel"] == c]
        assert [(int(r["first"]), int(r["first"] + r["windows"] - 1)) for r in mine] == LONG[(n_win, which)], c
    med = BC.median_thresholds(np.concatenate([block for block, _ in first], axis=1))
    _check(_feed(w, chunks, med), med)
    every = _feed(w, chunks, 0)
    _check(every, 0)
    assert all(b.records.size == cs.n_ch and np.all(b.records["windows"] == n_win) and np.all(b.records["flags"] == 3)
               and np.all(b.floor["windows_off"] == 0) for _, b in every)
    _check(_feed(w, chunks, BURST_THRESHOLD_OFF), BURST_THRESHOLD_OFF)


# ------------------------------------------------------------------------------------------ chunks in flight
def test_thresholds_change_at_the_chunk_boundary_with_two_in_flight():
    """bursts() after each fetch names that chunk; thresholds set while chunks 2 and 3 are in flight hold from chunk 4
    on and not before; set again to the same values they change nothing; reset() restores the default table."""
    _device()
    cs = RC.case("s16")
    w = RC.receiver(cs)
    w.set_bursts(True)
    blocks = [block for block, _ in _feed(w, cs.chunks)]
    p = BC.window_sums(np.concatenate(blocks, axis=1))[0]
    thr_a, thr_b = np.sort(p, axis=1)[:, 1].astype(np.uint64), np.sort(p, axis=1)[:, -2].astype(np.uint64)
    assert np.all(thr_a < thr_b)

    def run(again):
        w.reset()
        assert w.submitted == 0
        w.set_burst_threshold(thr_a)
        got = []

        def take():
            w.fetch()
            got.append(w.bursts())

        for k, chunk in enumerate(cs.chunks):
            if k == 4:
                assert w.inflight == 2 and w.submitted == 4
                w.set_burst_threshold(thr_b)             # chunks 2 and 3 are in flight
                assert np.array_equal(w.burst_thresholds(), thr_b)
            elif again:
                w.set_burst_threshold(thr_b if k > 4 else thr_a)
            if k >= 2:
                take()
            w.submit(chunk)
            assert w.submitted == k + 1
        take()
        take()
        return got

    got = run(False)
    assert [b.chunk for b in got] == list(range(cs.nk))
    for k, b in enumerate(got):
        BC.assert_equals_model(b, blocks[k], thr_a if k < 4 else thr_b, k)
    assert any(not np.array_equal(BC.burst_model(blocks[k], thr_a)[0], BC.burst_model(blocks[k], thr_b)[0]) for k in (4, 5))
    again = run(True)
    for a, b in zip(got, again):
        assert a.records.tobytes() == b.records.tobytes() and a.floor.tobytes() == b.floor.tobytes()
    w.reset()
    assert np.all(w.burst_thresholds() == BURST_THRESHOLD_OFF)
    w.demodulate(cs.chunks[0])
    BC.assert_equals_model(w.bursts(), blocks[0], BURST_THRESHOLD_OFF, 0)


def test_off_by_default_and_nothing_else_changes():
    _device()
    cs = RC.case("d4_t256_b128")
    w = RC.receiver(cs)
    plain = []
    for chunk in cs.chunks:
        pk = w.demodulate(chunk)
        plain.append((w.channelized(), [[(p.index, bytes(p.data), p.rssi, p.snr) for p in ps] for ps in pk]))
        with pytest.raises(RuntimeError):
            w.bursts()
    w.set_bursts(True)
    w.reset()
    w.set_burst_threshold(BC.median_thresholds(np.concatenate([b for b, _ in plain], axis=1)))
    for k, chunk in enumerate(cs.chunks):
        pk = w.demodulate(chunk)
        assert np.array_equal(w.channelized(), plain[k][0])
        assert [[(p.index, bytes(p.data), p.rssi, p.snr) for p in ps] for ps in pk] == plain[k][1]
        assert w.bursts().chunk == k
    w.submit(cs.chunks[0])
    with pytest.raises(RuntimeError):
        w.set_bursts(False)                              # a chunk in flight: not now
    w.fetch()
    w.set_bursts(False)
    w.demodulate(cs.chunks[1])
    with pytest.raises(RuntimeError):
        w.bursts()


def test_records_are_bit_identical_from_run_to_run():
    _device()
    cs = RC.case("70ch")
    w = RC.receiver(cs)
    w.set_bursts(True)
    first = _feed(w, cs.chunks[:1])
    thr = BC.median_thresholds(first[0][0])
    runs = [_feed(w, cs.chunks[:1], thr)[0][1] for _ in range(3)]
    assert runs[0].records.size > cs.n_ch
    for b in runs[1:]:
        assert b.records.tobytes() == runs[0].records.tobytes() and b.floor.tobytes() == runs[0].floor.tobytes()


def test_more_records_than_the_first_buffer_holds():
    """rd_wb_bursts with too little room: RD_ERR_CAPACITY, the count, and nothing lost."""
    import ctypes as C
    from rtldavis_amd import _lib
    _device()
    cs = RC.case("70ch")
    w = RC.receiver(cs)
    w.set_bursts(True)
    block = _feed(w, cs.chunks[:1])[0][0]
    thr = BC.median_thresholds(block)
    got = _feed(w, cs.chunks[:1], thr)[0][1]
    want = BC.burst_model(block, thr)[0]
    assert want.size > 64 and got.records.size == want.size      # (more than bursts() makes room for at first)
    n = C.c_int(0)
    assert _lib.lib().rd_wb_bursts(w._h, None, 0, C.byref(n), None, 0) == _lib.RD_ERR_CAPACITY and n.value == want.size
    assert w.bursts().records.tobytes() == got.records.tobytes()


# ------------------------------------------------------------------------------------------ closed loop
@pytest.mark.parametrize("planted", BC.PLANTED)
def test_closed_loop_on_the_device(planted):
    """The capture of the CPU test: without acquisition parsed() stays empty; with Acquisition(need=1), two chunks in
    flight, the retune holds from chunk 4 and the second burst's message is CRC-valid with the planted payload.
    The estimate is held to 1500 Hz of the planted offset and printed (the float64 model's: DESIGN.md section 5.3)."""
    _device()
    from rtldavis_amd import wideband
    lc = BC.acq_capture(planted)
    chunks = [lc.raw[lc.step * k: lc.step * (k + 1)] for k in range(RC.LOOP_NK)]
    w = wideband.WidebandReceiver(RC.packet_config(RC.LOOP_B), lc.chans)
    w.set_parse(True)
    w.set_bursts(True)
    w.demodulate(chunks[0])                              # chunk 0 holds no burst: its floor gives the thresholds
    thr = BC.new_acquisition().thresholds(w.bursts().floor)

    def loop(acq):
        w.reset()
        w.set_burst_threshold(thr)
        rows = []

        def fetch():
            w.fetch()
            r = w.parsed()
            rows.extend(_rows(r))
            return w.bursts(), r

        asked = BC.run_loop(RC.LOOP_NK, lambda k: w.submit(chunks[k]), fetch, acq, w.retune)
        return asked, rows

    class Deaf:
        def update(self, bursts, rows, submitted):
            return None

    asked, rows = loop(Deaf())
    assert asked == [] and rows == []
    acq = BC.new_acquisition(need=1)
    asked, rows = loop(acq)
    assert len(asked) == 1 and asked[0][0] == RC.LOOP_RETUNE_CHUNK
    est = asked[0][1]
    print(f"\n[bursts loop] planted {planted} Hz: estimate {est} Hz ({est - planted:+d}), "
          f"messages {[(r[1], r[4]) for r in rows]}")
    assert abs(est - planted) <= BC.ESTIMATE_TOL_HZ
    assert [(r[1], r[5]) for r in rows] == [(5, lc.payload)]
    assert acq.locked and [int(s) for s in w.shift_hz] == [int(lc.plan.shift_hz[0]) + est]
