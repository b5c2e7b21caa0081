"""WidebandReceiver.set_spectrum / spectrum() and Channelizer.spectrum on the device (k_chan_spectrum, rd_spectrum.hip):
every format against the float64 model within its a-priori per-bin tolerance (tests/spectrum_model.py: tol_bin) at the
smallest shapes that reach each path - one and several segments, leftover samples, more segments than workgroups, the
largest N -; the record bit-identical from run to run and between the streaming and the one-shot form; two chunks in
flight; the state rules; and a receiver's bytes, packets and levels untouched by the spectrum beside them.  Then the
crafted inputs, in which every bin and table entry matters, at every N; one handle through many shapes; the asynchronous
rd_chan_spectrum_dev on a caller's stream; and zero chunks between strong ones with two in flight."""
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
    ref, s, _ = SM.reference(fmt, decim * bs, n_bins, level)
    assert sp.power.dtype == np.float64 and sp.power.shape == (n_bins,) and np.all(np.isfinite(sp.power))
    assert sp.segments == s and sp.chunk == chunk
    assert np.array_equal(sp.freqs_hz, SM.freqs(RC.CENTRE, 19200 * 14 * decim, n_bins))
    ratio = SM.excess(sp.power, ref, n_bins)
    print(f"\n[spectrum] {fmt} L={decim * bs} N={n_bins} S={s} level={level:g}: max |P_dev - P_ref| / tol_bin = {ratio:.4f}")
    assert ratio <= 1.0, (fmt, decim, bs, n_bins, ratio)


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
    assert big.segments == s == 3 and SM.excess(big.power, ref, 4096) <= 1.0
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
            assert sp.chunk == k and sp.segments == s and SM.excess(sp.power, p, n_bins) <= 1.0
        assert np.array_equal(both.spectrum().power, only.spectrum().power)


# ------------------------------------------------------------------------------------------ crafted inputs, every N
def _one_shot(fmt):
    from rtldavis_amd import channelizer
    _device()
    return channelizer.Channelizer(CHANS, RC.CENTRE, decim=4, taps=TAPS, sample_format=fmt)


def _assert_record(sp, ref, s, n_bins, decim, chunk, what):
    assert sp.power.dtype == np.float64 and sp.power.shape == (n_bins,) and np.all(np.isfinite(sp.power)), what
    assert sp.segments == s and sp.chunk == chunk, what
    assert np.array_equal(sp.freqs_hz, SM.freqs(RC.CENTRE, 19200 * 14 * decim, n_bins)), what
    if not ref.any():                                                      # the all-zero input: exactly nothing
        assert not sp.power.any() and np.all(np.isfinite(sp.db())), what
    ratio = SM.excess(sp.power, ref, n_bins)
    assert ratio <= 1.0, (what, ratio)
    return ratio


@pytest.mark.parametrize("fmt", SM.FORMATS)
@pytest.mark.parametrize("n_bins", sorted(SM.CRAFTED_SHAPES))
def test_crafted_inputs_at_every_size(fmt, n_bins):
    """Every crafted input of spectrum_model (two impulses per segment, full-band noise, a weak tone beside a strong one,
    a tone per segment, constant bytes) at every N with one segment, a few with leftover samples, and 65 .. 70 on 64
    workgroups, within tol_bin in every bin: through a receiver wherever the shape is a valid chunk, else uploaded to a
    Channelizer."""
    worst, at = 0.0, None
    for shape in SM.CRAFTED_SHAPES[n_bins]:
        L = SM.shape_samples(shape)
        if shape[0] == "rx":
            w = _receiver(fmt, shape[1], shape[2])
            w.set_spectrum(n_bins)
        else:
            ch = _one_shot(fmt)
        for k, kind in enumerate(SM.kinds(fmt)):
            raw = SM.crafted(kind, fmt, L, n_bins)
            ref, s = SM.crafted_reference(kind, fmt, L, n_bins)
            if shape[0] == "rx":
                w.demodulate(raw)
                ratio = _assert_record(w.spectrum(), ref, s, n_bins, shape[1], k, (fmt, n_bins, shape, kind))
            else:
                ch.upload(raw)
                ratio = _assert_record(ch.spectrum(n_bins), ref, s, n_bins, 4, 0, (fmt, n_bins, shape, kind))
            worst, at = (ratio, f"{kind} S={s}") if ratio > worst else (worst, at)
    print(f"\n[spectrum-crafted] {fmt} N={n_bins}: max |P_dev - P_ref| / tol_bin = {worst:.4f} ({at})")


@pytest.mark.parametrize("fmt", SM.FORMATS)
def test_one_handle_many_shapes(fmt):
    """One Channelizer, uploads that take (S, G) through 200 -> 3 -> 70 -> 1 -> 64 at one N, then another N and back: the
    reuse branch of rd_spec_prepare (same N, fewer workgroups than prepared), the stale rows of the partial sums and the
    ticket word.  Every record is bit-identical to a fresh handle's on the same upload, and within tol_bin."""
    plan = [(64, 200 * 64), (64, 3 * 64 + 40), (64, 70 * 64 + 8), (64, 64 + 24), (64, 64 * 64),
            (1024, 66 * 1024 + 8), (1024, 2 * 1024 + 16), (64, 70 * 64 + 8), (64, 3 * 64 + 40)]
    assert [SM.launch_plan(L, n)[:2] for n, L in plan[:5]] == [(200, 64), (3, 3), (70, 64), (1, 1), (64, 64)]
    ch = _one_shot(fmt)
    for step, (n_bins, L) in enumerate(plan):
        raw = SM.crafted("hop", fmt, L, n_bins)
        ref, s = SM.crafted_reference("hop", fmt, L, n_bins)
        ch.upload(raw)
        got = ch.spectrum(n_bins)
        fresh = _one_shot(fmt)
        fresh.upload(raw)
        want = fresh.spectrum(n_bins)
        assert got.segments == want.segments == s, step
        assert got.power.tobytes() == want.power.tobytes(), (fmt, step, n_bins, L)
        assert SM.excess(got.power, ref, n_bins) <= 1.0, (fmt, step, n_bins, L)


def _spectrum_dev_child():
    """The body of test_spectrum_dev_on_a_stream, in a process of its own in which torch was imported first."""
    import torch
    from rtldavis_amd import _lib
    _device()
    L = _lib.lib()
    fmt = "s16"
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    ch = _one_shot(fmt)
    # the first call builds the tables on that stream; then the reuse branch; then another N and fewer segments
    for n_bins, n_samples in ((2048, 67 * 2048 + 8), (2048, 67 * 2048 + 8), (256, 3 * 256 + 40), (2048, 2048 + 24)):
        raw = SM.crafted("hop", fmt, n_samples, n_bins)
        ref, s = SM.crafted_reference("hop", fmt, n_samples, n_bins)
        ch.upload(raw)
        n_rec = 16 + 8 * n_bins
        buf = torch.full((n_rec + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert buf.data_ptr() % 16 == 0
        assert L.rd_chan_spectrum_dev(ch._h, n_bins, buf.data_ptr() + 8, stream.cuda_stream) == _lib.RD_ERR_ARG
        assert L.rd_chan_spectrum_dev(ch._h, n_bins, None, stream.cuda_stream) == _lib.RD_ERR_ARG
        assert L.rd_chan_spectrum_dev(ch._h, n_bins, buf.data_ptr(), stream.cuda_stream) == _lib.RD_OK, _lib.last_error()
        stream.synchronize()
        rec = buf.cpu().numpy()
        assert rec[:8].view(np.uint64)[0] == 0 and rec[8:16].view(np.uint32).tolist() == [s, n_bins]
        assert np.all(rec[n_rec:] == 0xA5)
        power = rec[16:n_rec].view(np.float64)
        host = ch.spectrum(n_bins)
        assert host.segments == s and power.tobytes() == host.power.tobytes(), (n_bins, n_samples)
        assert SM.excess(power, ref, n_bins) <= 1.0
    print("spectrum_dev ok")


def test_spectrum_dev_on_a_stream():
    """rd_chan_spectrum_dev: asynchronous on a caller's (non-default) stream into a 16-byte aligned device buffer - a torch
    tensor on a torch stream: the header {0, S, N}, the doubles bit-identical to rd_chan_spectrum's, the bytes behind the
    record untouched; a misaligned destination is RD_ERR_ARG.  In a child process that imports torch before the library:
    torch brings a HIP runtime of the library's soname, so whichever of the two is loaded first serves both, and only
    then is a torch stream a stream of the runtime the library calls (the order bench.py has)."""
    import os
    import subprocess
    import sys
    _device()
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; import torch; torch.cuda.init(); sys.path[:0] = [%r, %r]; "
            "import test_wideband_spectrum as T; T._spectrum_dev_child()" % (here, os.path.dirname(here)))
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "spectrum_dev ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("fmt", SM.FORMATS)
def test_quiet_chunks_between_strong_ones(fmt):
    """Two chunks in flight, strong noise and the all-zero input (uint8: the constant byte 127) in turn, 66 segments on 64
    workgroups: every record is the bits of that chunk run alone, and the zero chunk's is exactly 0.0 in every bin -
    nothing leaks through the partial sums or the ticket."""
    decim, bs, n_bins = 28, 2432, 1024
    quiet_kind = "const127" if fmt == "u8" else "zero"
    strong, quiet = SM.crafted("noise", fmt, decim * bs, n_bins), SM.crafted(quiet_kind, fmt, decim * bs, n_bins)
    assert SM.launch_plan(decim * bs, n_bins)[:2] == (66, 64)
    w = _receiver(fmt, decim, bs)
    w.set_spectrum(n_bins)
    alone = []
    for c in (strong, quiet):
        w.demodulate(c)
        alone.append(w.spectrum().power)
    assert SM.excess(alone[0], SM.crafted_reference("noise", fmt, decim * bs, n_bins)[0], n_bins) <= 1.0
    assert SM.excess(alone[1], SM.crafted_reference(quiet_kind, fmt, decim * bs, n_bins)[0], n_bins) <= 1.0
    w.reset()
    order = [0, 1, 0, 1, 1, 0]
    got = []
    for k, i in enumerate(order):
        if k >= 2:
            w.fetch()
            got.append(w.spectrum())
        w.submit((strong, quiet)[i])
    for _ in range(2):
        w.fetch()
        got.append(w.spectrum())
    for k, (i, sp) in enumerate(zip(order, got)):
        assert sp.chunk == k and sp.segments == 66
        assert sp.power.tobytes() == alone[i].tobytes(), (fmt, k)
        if i == 1 and fmt != "u8":
            assert not sp.power.any() and np.all(np.isfinite(sp.db())), (fmt, k)
