"""Burst decode on the device (rd_wb_set_burst_decode -> k_chan_burst_decode, rd_burst_decode.hip): every record of every
chunk equal to the integer model (tests/burst_decode_cases.py) of the receiver's own channelized bytes and burst records -
three channels at decim 4 with bursts 30 kHz below and 20 and 90 kHz above their centres, in chunks of 1152 (the look-back
is the whole chunk before), 2048 and 4608 outputs (a run of 36 windows under a low threshold), and one plan with 8 samples
per symbol -; the same with two chunks in flight; the 64-bit clock; decode off; determinism and reset; and the
acquisition loop closed from one burst."""
import numpy as np
import pytest

import burst_cases as BC
import burst_decode_cases as DC
import retune_cases as RC
from rtldavis_amd import acquire
from stream_parse_helpers import _rows

pytestmark = pytest.mark.gpu
V = DC.VALID
# name: (block_size, symbol_length, channel 0's threshold (None: as the others), (chunk, channel, payload, flags) expected -
# what the float64 channelizer model's bytes give; the device's differ from them by one step at most)
PLANS = {
    "b1152": (1152, 14, None, [(1, 0, V[0], 1), (5, 1, V[1], 1), (7, 2, V[2], 1), (13, 0, V[1], 1)]),
    "b2048": (2048, 14, None, [(0, 0, V[0], 0), (2, 1, V[1], 0), (4, 2, V[2], 1), (7, 0, V[1], 1)]),
    "b4608_low": (4608, 14, 0, [(1, 1, V[1], 1), (1, 2, V[2], 0)]),
    "sym8": (DC.S8_BS, 8, None, [(2, 1, V[0], 1), (4, 2, V[2], 1)]),
}


def _device():
    from rtldavis_amd import _lib
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"


def _plan(name):
    """(receiver with bursts and decode on, chunks, thresholds at 4 x the first chunk's floor)."""
    bs, sl, thr0, _ = PLANS[name]
    if sl == 8:
        w = DC.device_receiver(bs, 8, offsets_hz=DC.S8_OFFSETS_HZ)
        chunks = DC.chunks_of(DC.s8_capture(), bs)
        quiet = chunks[0]                                    # (the first burst begins in chunk 1)
    else:
        w = DC.device_receiver(bs)
        q, stream = DC.device_capture()
        chunks, quiet = DC.chunks_of(stream, bs), q[: 2 * DC.DEV_DECIM * bs]
    w.set_bursts(True)
    w.set_burst_decode(True)
    w.demodulate(quiet)
    assert w.burst_messages().records.size == 0 and w.burst_messages().chunk == 0      # default thresholds: no runs
    thr = acquire.Acquisition(3, w.cfg).thresholds(w.bursts().floor).astype(np.uint64)
    if thr0 is not None:
        thr[0] = thr0
    return w, chunks, thr


def _feed(w, chunks, thr, advance=0):
    """reset, thresholds, one chunk at a time: [(channelized bytes, Bursts, BurstMessages)]."""
    w.reset()
    w.set_burst_threshold(thr)
    if advance:
        w._debug_advance_clock(advance)
    out = []
    for chunk in chunks:
        w.demodulate(chunk)
        out.append((w.channelized(), w.bursts(), w.burst_messages()))
    return out


def _check(run, cfg, clock0=0):
    prev = None
    for k, (block, b, got) in enumerate(run):
        DC.assert_equals_model(got, DC.decode_model(block, prev, b, cfg, k >= 1, clock0 + k * (block.shape[1] // 2)))
        prev = block


def _found(run):
    return [(k, int(r["channel"]), bytes(r["data"]).hex(), int(r["flags"])) for k, (_, _, m) in enumerate(run) for r in m.records]


@pytest.mark.parametrize("name", list(PLANS))
def test_messages_equal_the_model(name):
    """One chunk at a time against the model of the device's own bytes and burst records, field for field, long_runs and
    chunk included; the planted packets are the ones found, the CRC-invalid twin never; and the same chunks fed with two
    in flight give the same records."""
    _device()
    bs, sl, thr0, expect = PLANS[name]
    w, chunks, thr = _plan(name)
    run = _feed(w, chunks, thr)
    bursts_of = [b for _, b, _ in run]
    for k, (block, b, _) in enumerate(run):
        BC.assert_equals_model(b, block, thr, k)
    _check(run, w.cfg)
    print(f"\n[burst decode {name}] " + ", ".join(f"chunk {k} ch {c} {d[:8]} flags {f}" for k, c, d, f in _found(run)))
    assert _found(run) == expect
    # the twin was found as a run on channel 1 and gave no message
    lo, hi = (3500, 4460) if sl == 8 else (11000, 12680)
    span = range(lo // bs, hi // bs + 1)
    assert any(r["channel"] == 1 and r["windows"] >= 3 for k in span for r in bursts_of[k].records)
    assert not any(r["channel"] == 1 for k in span for r in run[k][2].records)
    if thr0 == 0:
        assert all(list(m.long_runs) == [1, 0, 0] for _, _, m in run)
        assert all(b.records[0]["windows"] == bs // 128 > DC.MAX_W for b in bursts_of)
    else:
        assert all(not m.long_runs.any() for _, _, m in run)
    if name == "b2048":                                      # the very first chunk, from window 0, with no chunk before it
        m0 = run[0][2].records[0]
        assert (m0["first"], m0["flags"], m0["channel"]) == (0, 0, 0) and m0["tau"] > 0 and m0["time"] == m0["tau"]
    if name == "b1152":                                      # every packet is longer than what is left of its chunk
        assert all(int(r["flags"]) & 1 and int(r["tau"]) < 0 for _, _, m in run for r in m.records)
    # two in flight: chunk k - 2 is fetched before chunk k is submitted
    w.reset()
    w.set_burst_threshold(thr)
    got = []
    for k, chunk in enumerate(chunks):
        if k >= 2:
            w.fetch()
            got.append(w.burst_messages())
        w.submit(chunk)
    for _ in range(2):
        w.fetch()
        got.append(w.burst_messages())
    assert [m.chunk for m in got] == list(range(len(chunks)))
    for m, (_, _, want) in zip(got, run):
        assert m.records.tobytes() == want.records.tobytes() and m.long_runs.tobytes() == want.long_runs.tobytes()


def test_time_carries_the_64_bit_clock():
    _device()
    w, chunks, thr = _plan("b2048")
    run = _feed(w, chunks[:5], thr, advance=RC.LARGE_CLOCK)
    _check(run, w.cfg, RC.LARGE_CLOCK)
    rows = [(k, r) for k, (_, _, m) in enumerate(run) for r in m.records]
    assert len(rows) == 3 and any(int(r["tau"]) < 0 for _, r in rows)
    for k, r in rows:
        assert int(r["time"]) == RC.LARGE_CLOCK + 2048 * k + int(r["tau"]) > 2 ** 40


def test_off_changes_nothing_and_burst_messages_raises():
    """Packets, parsed(), bursts() and the channelized bytes with decode on are those of a receiver that was never asked;
    with decode off, or bursts off, burst_messages() raises."""
    _device()
    w, chunks, thr = _plan("b2048")
    w.set_parse(True)

    def run(decode):
        w.reset()
        w.set_burst_decode(decode)
        w.set_burst_threshold(thr)
        out = []
        for chunk in chunks[:5]:
            pk = w.demodulate(chunk)
            b = w.bursts()
            out.append((w.channelized().tobytes(), [[(p.index, bytes(p.data), p.rssi, p.snr) for p in ps] for ps in pk],
                        _rows(w.parsed()), b.records.tobytes(), b.floor.tobytes()))
            if decode:
                assert w.burst_messages().chunk == len(out) - 1
            else:
                with pytest.raises(RuntimeError):
                    w.burst_messages()
        return out

    plain = run(False)
    assert run(True) == plain
    w.submit(chunks[0])
    with pytest.raises(RuntimeError):
        w.set_burst_decode(False)                            # a chunk in flight: not now
    w.fetch()
    w.set_bursts(False)                                      # takes decode with it
    w.demodulate(chunks[1])
    with pytest.raises(RuntimeError):
        w.burst_messages()
    with pytest.raises(RuntimeError):
        w.set_burst_decode(True)
    w.set_bursts(True)
    w.set_burst_decode(True)
    w.demodulate(chunks[2])
    assert w.burst_messages().chunk == w.bursts().chunk


def test_records_are_bit_identical_and_reset_drops_the_look_back():
    _device()
    w, chunks, thr = _plan("b2048")
    runs = [_feed(w, chunks[:5], thr) for _ in range(3)]
    assert sum(m.records.size for _, _, m in runs[0]) == 3
    for other in runs[1:]:
        for (_, _, a), (_, _, b) in zip(runs[0], other):
            assert a.records.tobytes() == b.records.tobytes() and a.long_runs.tobytes() == b.long_runs.tobytes()
    # chunk 4 alone after a reset: its run begins at window 0 and there is no chunk before it - the packet that began in
    # chunk 3 is not found (with chunk 3 in front of it, it is: runs[0])
    assert [bytes(r["data"]).hex() for r in runs[0][4][2].records] == [DC.VALID[2]]
    alone = _feed(w, chunks[4:5], thr)
    _check(alone, w.cfg)
    assert alone[0][1].records.size and alone[0][1].records[0]["flags"] & 1 and alone[0][2].records.size == 0


# ------------------------------------------------------------------------------------------ closed loop
@pytest.mark.parametrize("planted", BC.PLANTED)
def test_closed_loop_on_the_device(planted):
    """burst_cases.acq_capture, the default plan's channel 25, two chunks in flight: burst A gives one row, that row one
    retune (held to 1500 Hz of planted + drawn cfo, printed), and burst B arrives in parsed() with the planted payload."""
    _device()
    from rtldavis_amd import wideband
    lc, want = DC.acq_plan(planted)
    chunks = [lc.raw[lc.step * k: lc.step * (k + 1)] for k in range(RC.LOOP_NK)]
    w = wideband.WidebandReceiver(RC.packet_config(RC.LOOP_B), lc.chans)
    w.set_parse(True)
    w.set_bursts(True)
    w.set_burst_decode(True)
    w.demodulate(chunks[0])                                  # chunk 0 holds no burst: its floor gives the thresholds
    thr = BC.new_acquisition().thresholds(w.bursts().floor)
    w.reset()
    w.set_burst_threshold(thr)
    acq = acquire.Acquisition(1, w.cfg)                      # need = 3, which two bursts never reach
    rows, msgs = [], []

    def fetch():
        w.fetch()
        r = w.parsed()
        rows.extend(_rows(r))
        msgs.append(w.burst_messages())
        return w.bursts(), r

    class WithMessages:
        def update(self, bursts, parsed_rows, submitted):
            return acq.update(bursts, parsed_rows, submitted, msgs[-1])

    asked = BC.run_loop(RC.LOOP_NK, lambda k: w.submit(chunks[k]), fetch, WithMessages(), w.retune)
    found = [(m.chunk, bytes(r["data"]).hex()) for m in msgs for r in m.records]
    print(f"\n[burst decode loop] planted {planted} Hz: asked {asked} (planted + cfo {want[0]:.0f}), rows {found}, "
          f"messages {[(r[1], r[4]) for r in rows]}")
    assert found[0] == (1, lc.payload) and all(p == lc.payload for _, p in found)
    assert asked[0][0] == 3
    for (_, off), wnt in zip(asked, want):
        assert abs(off - wnt) <= BC.ESTIMATE_TOL_HZ
    assert rows and all(r[5] == lc.payload for r in rows) and rows[0][1] in (4, 5)
    assert acq.locked
