"""WidebandReceiver.set_spectrum / spectrum() and Channelizer.spectrum on the device (k_chan_spectrum, rd_spectrum.hip):
every format against the float64 model within its a-priori tolerance (tests/spectrum_model.py) at the smallest shapes
that reach each path - one and several segments, leftover samples, more segments than workgroups, the largest N -; the
record bit-identical from run to run and between the streaming and the one-shot form; two chunks in flight; the state
rules; and a receiver's bytes, packets and levels untouched by the spectrum beside them."""
import numpy as np
import pytest

import retune_cases as RC
import spectrum_model as SM
from stream_parse_helpers import _pkey

pytestmark = pytest.mark.gpu
CHANS = [RC.CENTRE - 100000, RC.CENTRE + 100000]
TAPS = np.hanning(10)[1:-1] / np.hanning(10).sum()


def _device():
    from rtldavis_amd import _lib
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"


def _receiver(fmt, decim, bs):
    from rtldavis_amd import wideband
    _device()
    return wideband.WidebandReceiver(RC.packet_config(bs), CHANS, RC.CENTRE, decim=decim, taps=TAPS, sample_format=fmt)


def _check(sp, fmt, decim, bs, n_bins, level=1.0, chunk=0):
    ref, s, tol = SM.reference(fmt, decim * bs, n_bins, level)
    assert sp.power.dtype == np.float64 and sp.power.shape == (n_bins,) and np.all(np.isfinite(sp.power))
    assert sp.segments == s and sp.chunk == chunk
    assert np.array_equal(sp.freqs_hz, SM.freqs(RC.CENTRE, 19200 * 14 * decim, n_bins))
    err = float(np.abs(sp.power - ref).max())
    print(f"\n[spectrum] {fmt} L={decim * bs} N={n_bins} S={s} level={level:g}: max |P_dev - P_ref| / tol = {err / tol:.4f}")
    assert err <= tol, (fmt, decim, bs, n_bins, err / tol)


@pytest.mark.parametrize("fmt", SM.FORMATS)
@pytest.mark.parametrize("shape", SM.SHAPES, ids=lambda s: "d%d_b%d_n%d" % s)
def test_against_the_model(fmt, shape):
    decim, bs, n_bins = shape
    w = _receiver(fmt, decim, bs)
    w.set_spectrum(n_bins)
    w.demodulate(SM.chunk_input(fmt, decim * bs, n_bins))
    _check(w.spectrum(), fmt, decim, bs, n_bins)


def test_small_signal_s16():
    """-80 dBFS overall: the tolerance scales with the total power, so only a relative error passes."""
    w = _receiver("s16", 20, 128)
    w.set_spectrum(1024)
    w.demodulate(SM.chunk_input("s16", 2560, 1024, 1e-4))
    _check(w.spectrum(), "s16", 20, 128, 1024, 1e-4)


@pytest.mark.parametrize("fmt", SM.FORMATS)
def test_bit_identical_runs_and_one_shot(fmt):
    from rtldavis_amd import channelizer
    decim, bs, n_bins = 100, 128, 64                                       # 200 segments on 64 workgroups
    a, b = SM.chunk_input(fmt, decim * bs, n_bins), SM.chunk_input(fmt, decim * bs, 4096)
    w = _receiver(fmt, decim, bs)
    w.set_spectrum(n_bins)
    w.demodulate(a)
    first = w.spectrum()
    w.demodulate(b)
    second = w.spectrum()                                                  # chunk 1: no state from chunk 0
    assert second.chunk == 1 and not np.array_equal(first.power, second.power)
    w.reset()
    w.demodulate(a)
    again = w.spectrum()
    assert again.chunk == 0 and again.segments == first.segments and np.array_equal(first.power, again.power)
    ch = channelizer.Channelizer(CHANS, RC.CENTRE, decim=decim, taps=TAPS, sample_format=fmt)
    for chunk, got in ((a, first), (b, second)):
        ch.upload(chunk)
        one = ch.spectrum(n_bins)
        assert one.chunk == 0 and one.segments == got.segments and np.array_equal(one.freqs_hz, got.freqs_hz)
        assert np.array_equal(one.power, got.power)
    ch.upload(a)
    big = ch.spectrum(4096)                                                # another N on the same handle, and back
    ref, s = SM.model(a, fmt, 4096)
    assert big.segments == s == 3 and np.abs(big.power - ref).max() <= SM.tol(ref, 4096)
    assert np.array_equal(ch.spectrum(n_bins).power, first.power)
    ch.upload(a[: 2 * 1000])
    with pytest.raises(ValueError):
        ch.spectrum(1024)                                                  # more bins than samples


def test_two_chunks_in_flight():
    fmt, decim, bs, n_bins = "s8", 20, 128, 1024
    chunks = [SM.chunk_input(fmt, decim * bs, n) for n in (1024, 64, 512)]
    w = _receiver(fmt, decim, bs)
    w.set_spectrum(n_bins)
    alone = []
    for c in chunks:
        w.demodulate(c)
        alone.append(w.spectrum().power)
    w.reset()
    w.submit(chunks[0])
    w.submit(chunks[1])
    with pytest.raises(RuntimeError):
        w.set_spectrum(64)                                                 # chunks in flight
    w.fetch()
    sp = w.spectrum()
    assert sp.chunk == 0 and np.array_equal(sp.power, alone[0])
    w.fetch()
    sp = w.spectrum()
    assert sp.chunk == 1 and np.array_equal(sp.power, alone[1])
    w.submit(chunks[2])                                                    # reuses chunk 0's slot
    sp = w.spectrum()
    assert sp.chunk == 1 and np.array_equal(sp.power, alone[1])            # chunk 1's record is the fetch's copy
    w.fetch()
    sp = w.spectrum()
    assert sp.chunk == 2 and np.array_equal(sp.power, alone[2])


def test_state_rules():
    fmt, decim, bs = "u8", 4, 128
    a = SM.chunk_input(fmt, decim * bs, 64)
    w = _receiver(fmt, decim, bs)
    w.demodulate(a)
    with pytest.raises(RuntimeError):
        w.spectrum()                                                       # that chunk was submitted with it off
    w.set_spectrum(64)
    with pytest.raises(RuntimeError):
        w.spectrum()                                                       # still that chunk
    w.demodulate(a)
    _check(w.spectrum(), fmt, decim, bs, 64, chunk=1)
    w.set_spectrum(512)                                                    # another N between chunks, on a quiet receiver
    assert w.spectrum().power.shape == (64,)                               # the record kept is chunk 1's
    w.demodulate(SM.chunk_input(fmt, decim * bs, 512))
    _check(w.spectrum(), fmt, decim, bs, 512, chunk=2)
    w.set_spectrum(64)
    w.demodulate(a)
    _check(w.spectrum(), fmt, decim, bs, 64, chunk=3)
    w.reset()                                                              # keeps the setting, drops the record
    with pytest.raises(RuntimeError):
        w.spectrum()
    w.demodulate(a)
    _check(w.spectrum(), fmt, decim, bs, 64, chunk=0)
    w.set_spectrum(None)
    w.demodulate(a)
    with pytest.raises(RuntimeError):
        w.spectrum()


@pytest.mark.parametrize("name", ["d4_t256_b128", "s16"])
def test_nothing_else_moves(name):
    """The retune cases' captures with the spectrum on, alone and beside the levels: bytes, packets and level records per
    chunk equal those of a twin that never called set_spectrum."""
    _device()
    cs = RC.case(name)
    n_bins = 64 if name == "d4_t256_b128" else 256
    twin, both, only = RC.receiver(cs), RC.receiver(cs), RC.receiver(cs)
    twin.set_levels(True)
    both.set_levels(True)
    both.set_spectrum(n_bins)
    only.set_spectrum(n_bins)
    for k, chunk in enumerate(cs.chunks):
        want = _pkey(twin.demodulate(chunk))
        assert _pkey(both.demodulate(chunk)) == want and _pkey(only.demodulate(chunk)) == want
        ref = twin.channelized()
        assert np.array_equal(both.channelized(), ref) and np.array_equal(only.channelized(), ref)
        a, b = twin.levels(), both.levels()
        assert a.chunk == b.chunk == k and a.input == b.input and a.channels.tobytes() == b.channels.tobytes()
        with pytest.raises(RuntimeError):
            only.levels()
        p, s = SM.model(chunk, cs.fmt, n_bins)
        for w in (both, only):
            sp = w.spectrum()
            assert sp.chunk == k and sp.segments == s and np.abs(sp.power - p).max() <= SM.tol(p, n_bins)
        assert np.array_equal(both.spectrum().power, only.spectrum().power)
