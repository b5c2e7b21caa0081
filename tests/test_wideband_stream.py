"""Live wideband receiver (rtldavis_amd/wideband.py, csrc/rd_wideband.hip): one capture fed chunk by chunk
through the streaming channelizer and the multi-stream demodulator.  PARITY UNPINNED, as for the
channelizer: the streamed bytes are tied to the one-shot channelizer on the whole capture (bit-exact) and
to its float64 model (oracle/channelizer_oracle.py), the packets to the batch demodulator on those bytes
and to the bursts the capture carries."""
import os
import re

import numpy as np
import pytest

from rtldavis_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 8192
SIX = [0, 7, 24, 25, 26, 50]   # both band edges, the centre and its neighbours


def _cfg(block_size=B):
    from rtldavis_amd import dsp
    return dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", block_size)


def _key(calls):
    return [[(p.index, bytes(p.data), p.rssi, p.snr) for p in ps] for ps in calls]


# ------------------------------------------------------------------------------------------------ CPU
def test_module_imports_and_is_exported():
    import rtldavis_amd
    from rtldavis_amd import wideband
    assert rtldavis_amd.WidebandReceiver is wideband.WidebandReceiver


def test_create_needs_no_gpu():
    """Construction does host work only (safe before fork, like Demodulator / Channelizer)."""
    from rtldavis_amd import channelizer as CZ
    from rtldavis_amd import wideband
    w = wideband.WidebandReceiver(_cfg())
    assert w.n_channels == 51 and w.chunk_bytes == 2 * 100 * B and w.taps.size == 512
    cz = CZ.Channelizer()
    assert np.array_equal(w.shift_hz, cz.shift_hz) and np.array_equal(w.taps, cz.taps)
    assert w.inflight == 0


def test_argument_errors():
    from rtldavis_amd import wideband
    w = wideband.WidebandReceiver(_cfg(), channels_hz=[914963100])
    with pytest.raises(ValueError, match="Incompatible array sizes"):
        w.submit(np.zeros(w.chunk_bytes - 2, np.uint8))
    with pytest.raises(ValueError, match="Incompatible array sizes"):
        w.demodulate(np.zeros(w.chunk_bytes + 2, np.uint8))
    with pytest.raises(ValueError):
        wideband.WidebandReceiver(_cfg(8000))                                        # block_size % 128 != 0
    with pytest.raises(ValueError):
        wideband.WidebandReceiver(_cfg(), channels_hz=[902419338], centre_hz=990000000)  # outside the band
    with pytest.raises(ValueError):
        w._debug_advance_clock(100)                                                  # not a multiple of 128


def test_symbols_declared_exported_and_in_the_ctypes_table():
    from rtldavis_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtldavis_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rd_wideband_[a-z0-9_]+)\s*\(", src))
    want = {"rd_wideband_" + n for n in ("create", "destroy", "reset", "submit", "fetch", "refetch", "inflight",
                                          "copy_channelized", "copy_discriminated", "debug_advance_clock")}
    assert declared == want
    L = _lib.lib()
    for n in want:
        assert n in _lib.SIGNATURES
        assert hasattr(L, n)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def six():
    """Six channels, five chunks: the capture, the one-shot channelizer on the whole of it, and the receiver's
    channelized chunks and packets, chunk by chunk."""
    from rtldavis_amd import _lib
    from rtldavis_amd import channelizer as CZ
    from rtldavis_amd import wideband
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    nk = 5
    chans = [CZ.US_CHANNELS_HZ[c] for c in SIX]
    raw, info = synth.synth_wideband([21, 22, 23, 24, 25, 26], [f - CZ.DEFAULT_CENTRE_HZ for f in chans], nk * B)
    cz = CZ.Channelizer(chans)
    cz.upload(raw)
    whole = cz.run_host()
    w = wideband.WidebandReceiver(_cfg(), chans)
    step = w.chunk_bytes
    chunks = [raw[step * k: step * (k + 1)] for k in range(nk)]
    got, bytes_ = [], []
    for k in range(nk):
        got.append(w.demodulate(chunks[k]))
        bytes_.append(w.channelized())
    return dict(raw=raw, chunks=chunks, whole=whole, cz=cz, chans=chans, got=got, bytes=bytes_, nk=nk)


@pytest.mark.gpu
def test_streamed_chunks_equal_the_whole_capture_bit_exact(six):
    from oracle import channelizer_oracle as CHO
    whole, cz = six["whole"], six["cz"]
    for k, b in enumerate(six["bytes"]):
        assert b.shape == (len(SIX), 2 * B)
        assert np.array_equal(b, whole[:, 2 * B * k: 2 * B * (k + 1)]), f"chunk {k}"
    streamed = np.concatenate(six["bytes"], axis=1)
    want = CHO.channelize(six["raw"], cz.shift_hz, cz.taps, cz.decim, cz.out_rate, cz.gain)
    d = streamed.astype(np.int32) - want.astype(np.int32)
    assert np.abs(d).max() <= 1
    assert (d != 0).mean() < 1e-3


@pytest.mark.gpu
def test_chunks_on_their_own_differ_history_and_phase(six):
    """What the streaming form fixes: the one-shot channelizer on each chunk alone is wrong from chunk 1 on - in
    the first outputs (no history) and after them (the mixer phase restarts at every chunk)."""
    from rtldavis_amd import channelizer as CZ
    one = CZ.Channelizer(six["chans"])
    n_early = -(-(one.taps.size - 1) // one.decim)
    for k, chunk in enumerate(six["chunks"]):
        one.upload(chunk)
        alone = one.run_host()
        s = six["bytes"][k]
        if k == 0:
            assert np.array_equal(alone, s)
            continue
        assert not np.array_equal(alone[:, : 2 * n_early], s[:, : 2 * n_early]), k
        assert not np.array_equal(alone[:, 2 * 64:], s[:, 2 * 64:]), k


@pytest.mark.gpu
def test_pipelined_submit_fetch_and_reset(six):
    from rtldavis_amd import wideband
    chunks, nk = six["chunks"], six["nk"]
    w = wideband.WidebandReceiver(_cfg(), six["chans"])
    got, bytes_ = [], []
    w.submit(chunks[0])
    for k in range(1, nk):
        w.submit(chunks[k])            # chunk k's copy runs beside chunk k-1's kernels
        assert w.inflight == 2
        with pytest.raises(RuntimeError):
            w.submit(chunks[k])        # a third chunk in flight is refused, nothing is consumed
        got.append(w.fetch())
        bytes_.append(w.channelized())
    got.append(w.fetch())
    bytes_.append(w.channelized())
    assert w.inflight == 0
    with pytest.raises(RuntimeError):
        w.fetch()
    for k in range(nk):
        assert _key(got[k]) == _key(six["got"][k]), k
        assert np.array_equal(bytes_[k], six["bytes"][k]), k
    # reset(): the same chunks give the same bytes and packets as a fresh receiver
    w.reset()
    for k in range(nk):
        assert _key(w.demodulate(chunks[k])) == _key(six["got"][k]), k
        assert np.array_equal(w.channelized(), six["bytes"][k]), k
    d = w.discriminated(3)
    assert d.shape == (2 * B,) and np.isfinite(d).all() and np.abs(d).max() > 0


@pytest.mark.gpu
def test_a_receiver_that_runs_for_days(six):
    """The output clock past 2^37: after chunk 0, one receiver's clock moves on by 10^6 * out_rate (a whole number of
    mixer periods); every byte and packet that follows equals a receiver's whose clock did not move."""
    from rtldavis_amd import wideband
    chunks, nk = six["chunks"], six["nk"]
    w = wideband.WidebandReceiver(_cfg(), six["chans"])
    w.demodulate(chunks[0])
    jump = 10 ** 6 * w.out_rate
    assert jump % 128 == 0 and jump > 2 ** 37
    w._debug_advance_clock(jump)
    for k in range(1, nk):
        assert _key(w.demodulate(chunks[k])) == _key(six["got"][k]), k
        assert np.array_equal(w.channelized(), six["bytes"][k]), k


@pytest.mark.gpu
def test_51_channels_packets_equal_the_batch_path():
    """All 51 hop channels over four chunks: per channel and chunk, the receiver's packets (index, bytes, order,
    RSSI/SNR) equal BatchDemodulator's on the whole channelized capture, and every injected burst comes back where
    it was put - bursts that cross a chunk boundary included."""
    from rtldavis_amd import batch
    from rtldavis_amd import channelizer as CZ
    from rtldavis_amd import wideband
    nk = 4
    off = [f - CZ.DEFAULT_CENTRE_HZ for f in CZ.US_CHANNELS_HZ]
    raw, info = synth.synth_wideband(range(100, 151), off, nk * B, amplitude=0.05)
    cz = CZ.Channelizer()
    cz.upload(raw)
    want = batch.BatchDemodulator(_cfg(), 51, nk).demodulate(cz.run_host())
    w = wideband.WidebandReceiver(_cfg())
    step = w.chunk_bytes
    got = []
    w.submit(raw[:step])
    for k in range(1, nk):
        w.submit(raw[step * k: step * (k + 1)])
        got.append(w.fetch())
    got.append(w.fetch())
    for k in range(nk):
        for c in range(51):
            g, x = got[k][c], want[c][k]
            assert [(p.index, bytes(p.data)) for p in g] == [(p.index, bytes(p.data)) for p in x], (k, c)
            for p, q in zip(g, x):
                assert abs(p.rssi - q.rssi) < 1e-3 and abs(p.snr - q.snr) < 1e-3
    burst = (32 + 80 + 8) * 14                              # preamble + packet + tail symbols, output samples
    crossing = 0
    for c, (payload, start) in enumerate(info):
        hits = [(k, p.index) for k in range(nk) for p in got[k][c] if bytes(p.data).hex() == payload]
        assert hits, (c, payload)
        pos = (hits[0][0] - 1) * B + hits[0][1]
        assert 0 <= pos - (start + 32 * 14) <= 30, (c, pos, start)
        crossing += start // B != (start + burst - 1) // B
    assert crossing >= 1


@pytest.mark.gpu
def test_multi_launch_form_takes_the_block_from_device_memory(six, monkeypatch):
    """RD_STREAM_IMPL=legacy (read when the device state is made): the demodulator's multi-launch form, which copies
    the channelized block device to device instead of reading it in place - the same packets."""
    from rtldavis_amd import wideband
    monkeypatch.setenv("RD_STREAM_IMPL", "legacy")
    w = wideband.WidebandReceiver(_cfg(), six["chans"])
    for k, chunk in enumerate(six["chunks"]):
        assert _key(w.demodulate(chunk)) == _key(six["got"][k]), k
        assert np.array_equal(w.channelized(), six["bytes"][k]), k


@pytest.mark.gpu
def test_timed_out_fetch_loses_the_packets_not_the_stream(six):
    """A fetch past its deadline (rd_set_wait_timeout_ms(0): an ordinary chunk times out, nothing is made to hang)
    drops that chunk's packets; the channelizer's clock and history and the demodulators' state advance as if it had
    been processed, so every later chunk equals the uninterrupted run."""
    from rtldavis_amd import _lib, wideband
    L = _lib.lib()
    w = wideband.WidebandReceiver(_cfg(), six["chans"])
    for k, chunk in enumerate(six["chunks"]):
        if k == 2:
            L.rd_set_wait_timeout_ms(0)
            try:
                with pytest.raises(_lib.HipError, match="timed out"):
                    w.demodulate(chunk)
                with pytest.raises(RuntimeError):   # its packets are gone: nothing to fetch
                    w.fetch()
            finally:
                assert L.rd_set_wait_timeout_ms(-1) == 0
            assert w.inflight == 0
            continue
        assert _key(w.demodulate(chunk)) == _key(six["got"][k]), k
        assert np.array_equal(w.channelized(), six["bytes"][k]), k


# name: (n_channels, decim, taps (T, or None for the default design), block_size, symbol_length, chunks)
STREAM_CONFIGS = {
    "70ch_two_groups": (70, 100, None, 1024, 14, 4),
    "d4_t256_block128": (3, 4, 256, 128, 14, 6),       # one workgroup per group and chunk; taps reach into the last chunk
    "sym8_t255": (4, 100, 255, 1024, 8, 4),            # out_rate 153600
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STREAM_CONFIGS))
def test_streamed_form_at_other_configs(name):
    """The streamed bytes equal Channelizer.run_host on the whole capture, byte for byte, and stay within the bound of
    the float64 model; after reset() in mid-stream the chunks equal the one-shot form on the capture from there on."""
    import chan_bound as CB
    from oracle import channelizer_oracle as CHO
    from rtldavis_amd import channelizer as CZ
    from rtldavis_amd import dsp, wideband
    n_ch, decim, T, bs, sl, nk = STREAM_CONFIGS[name]
    seed = sum(map(ord, name))
    cfg = dsp.PacketConfig(19200, sl, 16, 80, "1100101110001001", bs)
    fo = 19200 * sl
    fw = fo * decim
    taps = None if T is None else CB.random_taps(T, seed)
    rng = np.random.default_rng(seed)
    centre = CZ.DEFAULT_CENTRE_HZ
    chans = [int(centre + f) for f in rng.integers(-fw // 2 + fo, fw // 2 - fo, n_ch)]
    w = wideband.WidebandReceiver(cfg, chans, centre, decim=decim, taps=taps)
    cz = CZ.Channelizer(chans, centre, decim=decim, taps=taps, out_rate=fo)
    assert w.out_rate == fo and np.array_equal(w.shift_hz, cz.shift_hz)
    raw = CB.capture(nk * bs * decim, seed, fw)
    step = w.chunk_bytes
    streamed = []
    for k in range(nk):
        w.demodulate(raw[step * k: step * (k + 1)])
        streamed.append(w.channelized())
    streamed = np.concatenate(streamed, axis=1)
    cz.upload(raw)
    assert np.array_equal(streamed, cz.run_host())
    Z = CHO.channelize_z(raw, cz.shift_hz, cz.taps, decim, fo, cz.gain)
    s = CB.assert_matches_model(streamed, Z, CB.error_bound(cz, cz.taps, Z, raw))
    print(f"\n[chan-stream] {name}: exempt {s['exempt']:.2%}, mismatches {s['mismatches']}/{streamed.size}, "
          f"worst distance {s['worst_dist']:.2e} ({s['worst_ratio']:.2f} of delta)")
    # reset() after chunk 1: chunks 2.. are a new capture
    k0 = 2
    w.reset()
    again = []
    for k in range(k0, nk):
        w.demodulate(raw[step * k: step * (k + 1)])
        again.append(w.channelized())
    cz.upload(raw[step * k0:])
    assert np.array_equal(np.concatenate(again, axis=1), cz.run_host())
