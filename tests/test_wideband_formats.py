"""The live wideband receiver on signed captures (WidebandReceiver(sample_format="s8" | "s16")): the streamed bytes
equal the one-shot channelizer's on the whole capture, byte for byte, and the packets equal the batch demodulator's on
those bytes - as tests/test_wideband_stream.py holds for uint8.  PARITY UNPINNED, as for the channelizer."""
import numpy as np
import pytest

import chan_bound as CB
import chan_bound_fmt as CF
from rtldavis_amd import synth

B = 8192
SIX = [0, 7, 24, 25, 26, 50]
W = 0.01


def _cfg(block_size=B):
    from rtldavis_amd import dsp
    return dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", block_size)


def _key(calls):
    return [[(p.index, bytes(p.data), p.rssi, p.snr) for p in ps] for ps in calls]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["s8", "s16"])
def test_streamed_chunks_equal_the_whole_capture(fmt):
    """Six channels, five chunks: demodulate() chunk by chunk, submit / fetch two in flight, across a reset(), and with
    the clock moved past 2^37 - always the one-shot form's bytes on the whole capture, within the bound of the model,
    and BatchDemodulator's packets on those bytes."""
    from rtldavis_amd import batch, wideband
    from rtldavis_amd import channelizer as CZ
    nk = 5
    chans = [CZ.US_CHANNELS_HZ[c] for c in SIX]
    raw, info = synth.synth_wideband([21, 22, 23, 24, 25, 26], [f - CZ.DEFAULT_CENTRE_HZ for f in chans], nk * B,
                                     sample_format=fmt)
    cz = CZ.Channelizer(chans, sample_format=fmt)
    cz.upload(raw)
    whole = cz.run_host()
    Z = CF.model_z(raw, fmt, cz.shift_hz, cz.taps, cz.decim, cz.out_rate, cz.gain)
    s = CB.assert_matches_model(whole, Z, CF.error_bound_fmt(cz, cz.taps, Z, raw, fmt))
    print(f"\n[chan-fmt-stream] {fmt}: exempt {s['exempt']:.2%}, mismatches {s['mismatches']}/{whole.size}, "
          f"worst distance {s['worst_dist']:.2e} ({s['worst_ratio']:.2f} of delta)")
    want = batch.BatchDemodulator(_cfg(), len(SIX), nk).demodulate(whole)
    w = wideband.WidebandReceiver(_cfg(), chans, sample_format=fmt)
    assert w.chunk_bytes == raw.nbytes // nk
    step = 2 * w.chunk_samples
    chunks = [raw[step * k: step * (k + 1)] for k in range(nk)]
    got = []
    for k in range(nk):
        got.append(w.demodulate(chunks[k].reshape(-1, 2) if k == 1 else chunks[k]))
        assert np.array_equal(w.channelized(), whole[:, 2 * B * k: 2 * B * (k + 1)]), k
    found = 0
    for k in range(nk):
        for c in range(len(SIX)):
            g, x = got[k][c], want[c][k]
            assert [(p.index, bytes(p.data)) for p in g] == [(p.index, bytes(p.data)) for p in x], (k, c)
            for p, q in zip(g, x):
                assert abs(p.rssi - q.rssi) < 1e-3 and abs(p.snr - q.snr) < 1e-3
    for c, (payload, start) in enumerate(info):
        found += any(bytes(p.data).hex() == payload for k in range(nk) for p in got[k][c])
    assert found == len(SIX)
    # reset(), then two in flight
    w.reset()
    got2, bytes2 = [], []
    w.submit(chunks[0])
    for k in range(1, nk):
        w.submit(chunks[k])
        assert w.inflight == 2
        got2.append(w.fetch())
        bytes2.append(w.channelized())
    got2.append(w.fetch())
    bytes2.append(w.channelized())
    for k in range(nk):
        assert _key(got2[k]) == _key(got[k]), k
        assert np.array_equal(bytes2[k], whole[:, 2 * B * k: 2 * B * (k + 1)]), k
    # a receiver that runs for days
    w2 = wideband.WidebandReceiver(_cfg(), chans, sample_format=fmt)
    w2.demodulate(chunks[0])
    jump = 10 ** 6 * w2.out_rate
    assert jump % 128 == 0 and jump > 2 ** 37
    w2._debug_advance_clock(jump)
    for k in range(1, nk):
        assert _key(w2.demodulate(chunks[k])) == _key(got[k]), k
        assert np.array_equal(w2.channelized(), whole[:, 2 * B * k: 2 * B * (k + 1)]), k


@pytest.mark.gpu
def test_51_packets_of_the_weak_16_bit_capture_streamed():
    """51 bursts at 1 % of full scale, int16, gain 300, four chunks two in flight: every burst comes back where it was
    put, and the packets equal BatchDemodulator's on the one-shot channelizer's bytes."""
    from rtldavis_amd import batch, wideband
    from rtldavis_amd import channelizer as CZ
    nk = 4
    off = [f - CZ.DEFAULT_CENTRE_HZ for f in CZ.US_CHANNELS_HZ]
    raw, info = synth.synth_wideband(range(300, 351), off, nk * B, amplitude=0.12 * W, noise=0.02 * W, sample_format="s16")
    cz = CZ.Channelizer(gain=3.0 / W, sample_format="s16")
    cz.upload(raw)
    want = batch.BatchDemodulator(_cfg(), 51, nk).demodulate(cz.run_host())
    w = wideband.WidebandReceiver(_cfg(), gain=3.0 / W, sample_format="s16")
    step = 2 * w.chunk_samples
    got = []
    w.submit(raw[:step])
    for k in range(1, nk):
        w.submit(raw[step * k: step * (k + 1)])
        got.append(w.fetch())
    got.append(w.fetch())
    for k in range(nk):
        for c in range(51):
            assert [(p.index, bytes(p.data)) for p in got[k][c]] == [(p.index, bytes(p.data)) for p in want[c][k]], (k, c)
    found = 0
    for c, (payload, start) in enumerate(info):
        hits = [(k, p.index) for k in range(nk) for p in got[k][c] if bytes(p.data).hex() == payload]
        if hits:
            pos = (hits[0][0] - 1) * B + hits[0][1]
            found += 0 <= pos - (start + 32 * 14) <= 30
    assert found == 51


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["s8", "s16"])
def test_streamed_form_at_a_small_block(fmt):
    """block_size 128 (one workgroup per group and chunk), decim 4, 256 taps reaching into the previous chunk."""
    from rtldavis_amd import dsp, wideband
    from rtldavis_amd import channelizer as CZ
    decim, T, bs, nk = 4, 256, 128, 6
    cfg = dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", bs)
    fo = 19200 * 14
    taps = CB.random_taps(T, 99)
    centre = CZ.DEFAULT_CENTRE_HZ
    chans = [centre + 100000, centre - 400001, centre + 7]
    w = wideband.WidebandReceiver(cfg, chans, centre, decim=decim, taps=taps, sample_format=fmt)
    cz = CZ.Channelizer(chans, centre, decim=decim, taps=taps, out_rate=fo, sample_format=fmt)
    raw = CF.capture_fmt(nk * bs * decim, 99, fmt)
    step = 2 * w.chunk_samples
    streamed = []
    for k in range(nk):
        w.demodulate(raw[step * k: step * (k + 1)])
        streamed.append(w.channelized())
    streamed = np.concatenate(streamed, axis=1)
    cz.upload(raw)
    assert np.array_equal(streamed, cz.run_host())
    Z = CF.model_z(raw, fmt, cz.shift_hz, cz.taps, decim, fo, cz.gain)
    CB.assert_matches_model(streamed, Z, CF.error_bound_fmt(cz, cz.taps, Z, raw, fmt))
