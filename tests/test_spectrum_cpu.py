"""The per-chunk power spectrum (include/rtldavis_hip.h, SPECTRUM), the part that needs no device: the float64 model of
tests/spectrum_model.py on inputs whose answer is known in closed form, that every fault the GPU comparison is meant to
catch moves the model's own output past the tolerance by orders of magnitude, the Spectrum helpers, and the argument and
state errors of rd_wb_set_spectrum / rd_wb_spectrum / rd_chan_spectrum through the library, which does no device work
there."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import retune_cases as RC
import spectrum_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n_bins", [64, 1024, 4096])
def test_bin_centre_tone_reads_its_power(n_bins):
    amp, k = 0.3, n_bins // 8 + 3                                          # X[k] of the FFT; ascending index k + N/2
    n = np.arange(3 * n_bins)
    x = amp * np.exp(2j * np.pi * k * n / n_bins)
    p, s = SM.model(SM.quantise(x, "cf32"), "cf32", n_bins)
    assert s == 3
    t = SM.tol(p, n_bins)
    j = k + n_bins // 2
    assert abs(p[j] - amp ** 2) < t and abs(p[j - 1] - amp ** 2 / 4) < t and abs(p[j + 1] - amp ** 2 / 4) < t
    far = np.ones(n_bins, bool)
    far[j - 1: j + 2] = False
    assert p[far].max() < t
    # a full-scale tone reads 1.0 = 0 dBFS
    p1, _ = SM.model(SM.quantise(np.exp(2j * np.pi * k * n / n_bins), "cf32"), "cf32", n_bins)
    assert abs(p1[j] - 1.0) < SM.tol(p1, n_bins)


def test_white_noise_total_power():
    """sum_j P[j] = sum w^2 / (sum w)^2 N sigma^2 = 1.5 sigma^2 for white noise under the periodic Hann window
    (sum w^2 = 3 N / 8, sum w = N / 2), within the spread of 2 L real Gaussians."""
    n_bins, segs, sigma = 256, 400, 0.1
    rng = np.random.default_rng(5)
    x = sigma * (rng.standard_normal(n_bins * segs) + 1j * rng.standard_normal(n_bins * segs)) / np.sqrt(2)
    p, s = SM.model(SM.quantise(x, "cf32"), "cf32", n_bins)
    assert s == segs
    assert abs(p.sum() / (1.5 * sigma ** 2) - 1.0) < 6.0 / np.sqrt(n_bins * segs)
    # flat: every bin's mean is the same 1.5 sigma^2 / N; an average of 400 exponentials lies within 6 / sqrt(400) of it
    assert np.all(np.abs(p * n_bins / (1.5 * sigma ** 2) - 1.0) < 0.3)


@pytest.mark.parametrize("fmt", SM.FORMATS)
def test_formats_mean_the_channelizers_samples(fmt):
    raw = {"u8": [0, 255, 127, 128], "s8": [-128, 127, 0, -1], "s16": [-32768, 32767, 1, 0],
           "cf32": [np.nan, 9.0, -np.inf, 0.25]}[fmt]
    dtype = {"u8": np.uint8, "s8": np.int8, "s16": np.int16, "cf32": np.float32}[fmt]
    want = {"u8": [(0 - 127.4) / 127.6 + 1j, (127 - 127.4) / 127.6 + 1j * (128 - 127.4) / 127.6],
            "s8": [-1 + 1j * 127 / 128, 0 - 1j / 128], "s16": [-1 + 1j * 32767 / 32768, 1 / 32768 + 0j],
            "cf32": [0 + 8j, -8 + 0.25j]}[fmt]
    assert np.allclose(SM.samples(np.asarray(raw, dtype), fmt), want, rtol=0, atol=1e-15)
    # the kernel's uint8 form: (10 k - 1274) * f32(1 / 1276) is (k - 127.4) / 127.6 to 1.5 ulp RELATIVE, every k
    k = np.arange(256)
    dev = (10 * k - 1274).astype(np.float32) * np.float32(1.0 / 1276.0)
    ref = (k - 127.4) / 127.6
    assert np.all(np.abs(dev.astype(np.float64) - ref) <= 1.5 * SM.U * np.abs(ref))


def test_freqs_and_spectrum_helpers():
    from rtldavis_amd import wideband
    centre, rate = RC.CENTRE, 268800 * 100
    for n_bins in (64, 2048):
        f = wideband.spectrum_freqs(centre, rate, n_bins)
        assert f.dtype == np.float64 and np.all(np.diff(f) > 0) and f[n_bins // 2] == centre
        assert np.array_equal(f, SM.freqs(centre, rate, n_bins))
        assert f[0] == centre - rate / 2 and f[-1] == centre + rate / 2 - rate / n_bins
    power = np.asarray([0.0, 1.0, 0.25, 1e-12, 0.5, 0.0, 0.125, 2.0])
    sp = wideband.Spectrum(power, wideband.spectrum_freqs(1000, 800, 8), 3, 7)
    assert sp.freqs_hz.tolist() == [600.0, 700.0, 800.0, 900.0, 1000.0, 1100.0, 1200.0, 1300.0]
    assert sp.segments == 3 and sp.chunk == 7
    db = sp.db()
    assert db[1] == 0.0 and abs(db[2] - 10 * np.log10(0.25)) < 1e-12 and abs(db[3] + 120.0) < 1e-9
    assert np.isfinite(db).all() and db[0] == 10 * np.log10(np.finfo(np.float64).tiny)
    assert sp.band_power(700, 900) == 1.0 + 0.25 + 1e-12                   # the ends are in the band
    assert sp.band_power(701, 899) == 0.25 and sp.band_power(0, 500) == 0.0
    assert sp.band_power(-1e12, 1e12) == float(power.sum())


def test_launch_plan():
    assert SM.launch_plan(512, 64) == (8, 8, [[k] for k in range(8)])
    assert SM.launch_plan(512, 512) == (1, 1, [[0]])
    assert SM.launch_plan(2560, 1024)[:2] == (2, 2)
    s, g, lists = SM.launch_plan(12800, 64)
    assert (s, g) == (200, 64) and lists[0] == [0, 64, 128, 192] and lists[7] == [7, 71, 135, 199] and lists[8] == [8, 72, 136]
    assert sorted(v for seg in lists for v in seg) == list(range(200))
    assert SM.launch_plan(12800, 4096)[:2] == (3, 3)
    assert SM.launch_plan(819200, 2048)[:2] == (400, 64)


@pytest.mark.parametrize("fmt", SM.FORMATS)
@pytest.mark.parametrize("shape", SM.SHAPES)
def test_every_fault_exceeds_the_tolerance(fmt, shape):
    """The inputs of the GPU comparison: a wrong bin order, a missed fftshift, a conjugated transform or a dropped segment
    applied to the model's own output is at least 100 tol away from it - the tolerance hides none of them."""
    decim, bs, n_bins = shape
    raw = SM.chunk_input(fmt, decim * bs, n_bins)
    ref, s, t = SM.reference(fmt, decim * bs, n_bins)
    good, bad = SM.faults(raw, fmt, n_bins)
    assert np.array_equal(good, ref) and s == (decim * bs) // n_bins
    assert len(bad) == (5 if s > 1 else 3)
    for name, p in bad.items():
        assert np.abs(p - ref).max() > 100 * t, (name, np.abs(p - ref).max() / t)
    # reading the samples behind the last whole segment (full scale, or NaN / 1e30) would show as well
    if decim * bs > s * n_bins:
        late, _ = SM.model(np.asarray(raw)[-2 * n_bins * s:], fmt, n_bins)   # the S segments that END with the chunk
        assert np.abs(late - ref).max() > 100 * t


def test_small_signal_case_is_small():
    raw = SM.chunk_input("s16", 2560, 1024, 1e-4)
    ref, _, t = SM.reference("s16", 2560, 1024, 1e-4)
    assert np.abs(raw[: 2 * 2048]).max() <= 3                              # a count or two: -80 dBFS
    assert 1e-10 < ref.sum() < 1e-8 and t < 1e-13


def _receiver(fmt="u8", bs=1024, decim=100):
    from rtldavis_amd import wideband
    chans = [RC.CENTRE - 100000, RC.CENTRE + 100000]
    return wideband.WidebandReceiver(RC.packet_config(bs), chans, RC.CENTRE, decim=decim, taps=np.ones(8) / 8, sample_format=fmt)


def test_set_spectrum_argument_and_state_errors():
    from rtldavis_amd import _lib
    L = _lib.lib()
    w = _receiver()                                                        # 102400 samples per chunk
    for n in (64, 128, 256, 512, 1024, 2048, 4096, 0, None):
        w.set_spectrum(n)
    for bad in (1, 2, 32, 63, 65, 96, 1000, 4095, 4097, 8192, 65536, -64, -1, 2 ** 31, 64.0, "64", True, [64]):
        with pytest.raises(ValueError):
            w.set_spectrum(bad)
    assert L.rd_wb_set_spectrum(None, 64) == _lib.RD_ERR_ARG
    assert L.rd_wb_set_spectrum(w._h, 8192) == _lib.RD_ERR_ARG and "power of two" in _lib.last_error()
    small = _receiver(bs=128, decim=4)                                     # 512 samples per chunk
    small.set_spectrum(512)
    with pytest.raises(ValueError):
        small.set_spectrum(1024)                                           # a power of two in range, but > chunk_samples
    assert "exceeds" in _lib.last_error()
    # nothing fetched: no record, whatever the setting
    w.set_spectrum(256)
    with pytest.raises(RuntimeError):
        w.spectrum()
    power = np.empty(256, np.float64)
    info = _lib.RdSpectrumInfo()
    assert L.rd_wb_spectrum(w._h, power.ctypes.data, 256, C.byref(info)) == _lib.RD_ERR_STATE
    assert L.rd_wb_spectrum(w._h, None, 256, None) == _lib.RD_ERR_ARG
    assert L.rd_wb_spectrum(None, power.ctypes.data, 256, None) == _lib.RD_ERR_ARG
    w.reset()                                                              # keeps the setting, needs no device
    with pytest.raises(RuntimeError):
        w.spectrum()


def test_channelizer_spectrum_argument_errors():
    from rtldavis_amd import _lib, channelizer
    ch = channelizer.Channelizer([RC.CENTRE - 100000], RC.CENTRE)
    assert ch.centre_hz == RC.CENTRE
    for bad in (0, 63, 100, 8192, -64, 64.0, None, True):
        with pytest.raises(ValueError):
            ch.spectrum(bad)
    with pytest.raises(RuntimeError):
        ch.spectrum(64)                                                    # no capture uploaded
    power = np.empty(64, np.float64)
    assert _lib.lib().rd_chan_spectrum(None, 64, power.ctypes.data, None) == _lib.RD_ERR_ARG
    assert _lib.lib().rd_chan_spectrum(ch._h, 64, None, None) == _lib.RD_ERR_ARG


def test_symbols_declared_exported_and_in_the_ctypes_table():
    from rtldavis_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtldavis_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    protos = {
        "rd_wb_set_spectrum": r"int\s+rd_wb_set_spectrum\s*\(\s*rd_wideband\s*\*\s*w\s*,\s*int\s+n_bins\s*\)",
        "rd_wb_spectrum": r"int\s+rd_wb_spectrum\s*\(\s*rd_wideband\s*\*\s*w\s*,\s*double\s*\*\s*power\s*,\s*int\s+n_bins\s*,\s*rd_spectrum_info\s*\*\s*info\s*\)",
        "rd_chan_spectrum": r"int\s+rd_chan_spectrum\s*\(\s*rd_chan\s*\*\s*h\s*,\s*int\s+n_bins\s*,\s*double\s*\*\s*power_host\s*,\s*uint32_t\s*\*\s*segments\s*\)",
    }
    for n, proto in protos.items():
        assert re.search(proto, src), n
        assert n in _lib.SIGNATURES and hasattr(L, n)
    assert [(f, t) for f, t in _lib.RdSpectrumInfo._fields_] == [("chunk", C.c_uint64), ("segments", C.c_uint32), ("n_bins", C.c_uint32)]
    assert C.sizeof(_lib.RdSpectrumInfo) == 16
    body = re.search(r"typedef\s+struct\s+rd_spectrum_info\s*\{(.*?)\}", src, flags=re.S).group(1)
    assert " ".join(body.split()) == "uint64_t chunk; uint32_t segments; uint32_t n_bins;"
