"""The per-chunk power spectrum (include/rtldavis_hip.h, SPECTRUM), the part that needs no device: the float64 model of
tests/spectrum_model.py on inputs whose answer is known in closed form, that every fault the GPU comparison is meant to
catch moves the model's own output past the tolerance by orders of magnitude, the Spectrum helpers, and the argument and
state errors of rd_wb_set_spectrum / rd_wb_spectrum / rd_chan_spectrum through the library, which does no device work
there.  And the per-bin tolerance with the crafted inputs of the device test: the float32 restatement of the kernel
(spectrum_model.kernel_f32) stays within a quarter of tol_bin on every one of them, each of its mutants leaves tol_bin on
a named input, and the inputs are what they claim (closed form of the impulses, the weak tone's margin, exact zeros)."""
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


# ------------------------------------------------------------------------------------------ per-bin tolerance
def _crafted_cases(fmt, n_bins):
    """(label, raw, P_ref, S) of every input the device test feeds at this format and N."""
    for shape in SM.CRAFTED_SHAPES[n_bins]:
        L = SM.shape_samples(shape)
        for kind in SM.kinds(fmt):
            ref, s = SM.crafted_reference(kind, fmt, L, n_bins)
            yield f"{kind} L={L}", SM.crafted(kind, fmt, L, n_bins), ref, s
    for decim, bs, n in SM.SHAPES:
        if n == n_bins:
            ref, s, _ = SM.reference(fmt, decim * bs, n)
            yield f"three tones L={decim * bs}", SM.chunk_input(fmt, decim * bs, n), ref, s


def test_tol_bin_never_exceeds_tol():
    rng = np.random.default_rng(3)
    for n_bins in (64, 512, 4096):
        for p in (rng.random(n_bins), np.eye(1, n_bins, 5)[0], 1e-9 * rng.random(n_bins) + np.eye(1, n_bins, 7)[0], np.zeros(n_bins)):
            tb = SM.tol_bin(p, n_bins)
            assert tb.shape == (n_bins,) and np.all(tb <= SM.tol(p, n_bins)) and np.all(tb >= SM.eps(n_bins) ** 2 * p.sum())
    ref = np.asarray([4.0, 0.0, 1e-12, 0.0])
    assert SM.excess(ref, ref, 64) == 0.0 and SM.excess(np.zeros(4), np.zeros(4), 64) == 0.0
    assert SM.excess(np.asarray([0.0, 0.0, 1e-300, 0.0]), np.zeros(4), 64) == float("inf")
    assert SM.excess(np.asarray([4.0, np.nan, 0.0, 0.0]), ref, 64) == float("inf")
    t = SM.tol_bin(ref, 64)
    assert SM.excess(ref + 0.5 * t, ref, 64) == pytest.approx(0.5) and SM.excess(ref - np.eye(1, 4, 1)[0] * 2 * t[1], ref, 64) == pytest.approx(2.0)


@pytest.mark.parametrize("fmt", SM.FORMATS)
@pytest.mark.parametrize("n_bins", sorted(SM.CRAFTED_SHAPES))
def test_float32_model_keeps_a_quarter_of_tol_bin(fmt, n_bins):
    """A condition on the reference alone: the kernel's arithmetic in NumPy float32, no contraction, is within 0.25
    tol_bin in every bin of every input of the device test (measured: 0.043 at worst, uint8 at N = 64)."""
    worst, at = 0.0, None
    for label, raw, ref, s in _crafted_cases(fmt, n_bins):
        assert s == np.asarray(raw).size // 2 // n_bins
        r = SM.excess(SM.kernel_f32(raw, fmt, n_bins), ref, n_bins)
        worst, at = (r, label) if r > worst else (worst, at)
        assert r <= 0.25, (fmt, n_bins, label, r)
    print(f"\n[spectrum-f32] {fmt} N={n_bins}: max err / tol_bin = {worst:.4f} ({at})")


def test_crafted_shapes_reach_what_they_claim():
    assert sorted(SM.CRAFTED_SHAPES) == [64, 128, 256, 512, 1024, 2048, 4096]
    for n_bins, shapes in SM.CRAFTED_SHAPES.items():
        plans = [SM.launch_plan(SM.shape_samples(sh), n_bins) for sh in shapes]
        segs = [p[0] for p in plans]
        assert 1 in segs and any(65 <= s <= 70 for s in segs), (n_bins, segs)
        assert any(1 < s < 64 and SM.shape_samples(sh) % n_bins for s, sh in zip(segs, shapes)), (n_bins, segs)
        for (s, g, lists), sh in zip(plans, shapes):
            assert g == min(s, 64) and (s <= 64 or (s % 64 and {len(v) for v in lists} == {1, 2}))
            assert SM.shape_samples(sh) <= 290304
            if sh[0] == "rx":                                              # a valid receiver chunk of every format
                assert sh[1] % 4 == 0 and 4 <= sh[1] <= 160 and sh[2] % 128 == 0 and sh[2] >= 128
            else:                                                          # whole 16-byte vectors in every format
                assert sh[1] % 8 == 0


@pytest.mark.parametrize("fmt", SM.FORMATS)
def test_crafted_inputs_are_what_they_claim(fmt):
    dtype = {"u8": np.uint8, "s8": np.int8, "s16": np.int16, "cf32": np.float32}[fmt]
    for n_bins, shapes in SM.CRAFTED_SHAPES.items():
        for shape in shapes:
            L = SM.shape_samples(shape)
            s = L // n_bins
            for kind in SM.kinds(fmt):
                raw = SM.crafted(kind, fmt, L, n_bins)
                assert raw.dtype == dtype and raw.shape == (2 * L,) and not raw.flags.writeable
                assert SM.crafted(kind, fmt, L, n_bins) is raw
                tail = raw[2 * s * n_bins:]                                # the poison behind the last whole segment
                if fmt == "cf32":
                    assert np.all(np.isnan(tail[0::2])) and np.all(tail[1::2] == np.float32(1e30))
                    assert np.all(np.isfinite(raw[: 2 * s * n_bins]))
                else:
                    assert np.all(tail[0::2] == np.iinfo(dtype).max) and np.all(tail[1::2] == np.iinfo(dtype).min)
                ref, s_ref = SM.crafted_reference(kind, fmt, L, n_bins)
                assert s_ref == s and np.all(np.isfinite(ref))
                if kind == "zero":
                    # exactly nothing: the model, the float32 kernel, and a finite db()
                    from rtldavis_amd import wideband
                    assert not ref.any() and not SM.kernel_f32(raw, fmt, n_bins).any()
                    assert np.all(np.isfinite(wideband.Spectrum(ref, SM.freqs(0, 1, n_bins), s, 0).db()))
                elif kind == "noise":
                    # flat and strong: -10 dBFS in all (sum P = 1.5 sigma^2, relative spread sqrt(sum w^4 / (sum w^2)^2 / S) =
                    # sqrt(1.94 / (N S)); four of them), the median bin near its share (one segment: an exponential,
                    # median ln 2 of the mean), no bin empty
                    mean = ref.sum() / n_bins
                    assert abs(10 * np.log10(ref.sum() / 1.5) + 10.0) < 4.0 * 4.343 * np.sqrt(1.94 / (n_bins * s)) + 0.1
                    assert 0.4 * mean < np.median(ref) < 1.3 * mean and ref.min() > 1e-7 * mean
                elif kind == "hop":
                    k = [SM.hop_bin(v, n_bins) for v in range(s)]
                    assert len(set(k)) == s or s > n_bins
                    assert all(a != b for a, b in zip(k, k[1:])) and all(a != b for a, b in zip(k, k[64:]))
                    if fmt != "u8":                                        # (uint8 carries the -0.4 / 127.6 offset at DC)
                        seg = SM.segment_spectra(raw, fmt, n_bins)
                        assert [int(np.argmax(row)) for row in seg] == k
                elif kind == "impulses":
                    n0, n1 = SM.impulse_sites(fmt, L, n_bins)
                    assert np.all(n0 % 2 == 0) and np.all(n1 % 2 == 1) and n0.min() >= n_bins // 8 and n1.max() < n_bins
                    x = SM.samples(raw, fmt)[: s * n_bins].reshape(s, n_bins)
                    quiet = (-0.4 / 127.6) * (1 + 1j) if fmt == "u8" else 0.0
                    assert np.all((np.abs(x - quiet) > 1e-9).sum(axis=1) == 2)
                    assert np.all(np.abs(x[np.arange(s), n0]) > 0.55) and np.all(np.abs(x[np.arange(s), n1]) > 0.45)
                    # every bin carries power (two impulses of 0.6 w0 and 0.5 w1 cannot cancel in all segments at once
                    # unless S = 1 and the weights meet; then the bound below is the draw's own, asserted)
                    assert ref.min() > 1e-6 * ref.max()
                    if fmt != "u8":
                        cf = SM.impulses_closed_form(fmt, L, n_bins)
                        assert np.abs(cf - ref).max() <= 1e-13 * ref.sum(), (n_bins, shape)
                elif kind == "tones":
                    # the weak tone's bin stands at least 10 tol_bin above nothing: a kernel that loses it fails
                    tb = SM.tol_bin(ref, n_bins)
                    j = (int(np.floor(SM.WEAK_FREQ * n_bins + 0.5)) + n_bins // 2) % n_bins
                    js = SM.strong_bin(n_bins) + n_bins // 2
                    assert abs(j - js) > n_bins // 4 and int(np.argmax(ref)) == js
                    assert abs(ref[js] - SM.STRONG_AMP ** 2) < 1e-3
                    assert ref[j] >= 10.0 * tb[j], (n_bins, shape, ref[j] / tb[j])
                    assert 10 * np.log10(ref[j] / ref[js]) < SM.WEAK_DB + 0.1
                else:                                                      # constant bytes: DC and its two Hann neighbours
                    far = np.ones(n_bins, bool)
                    far[n_bins // 2 - 1: n_bins // 2 + 2] = False
                    assert ref[n_bins // 2] > 0 and ref[far].max() < 1e-25 * ref[n_bins // 2]


# mutant -> (the N it must be told apart at, the shapes tried: index into CRAFTED_SHAPES[N], None = all)
_S1, _SMANY = 0, -1
MUTANT_PLAN = {
    "last owned bin": ((4096, 512), None),
    "twiddle last stage": ((4096, 2048), None),
    "twiddle middle stage": ((4096, 2048), None),
    "w2 from stage h": ((64, 512, 4096), None),
    "lone stage skipped": ((128, 512, 2048), None),
    "store unpadded": ((64, 128, 4096), None),
    "window shifted": ((64, 1024, 4096), None),
    "vector reversed": ((64, 256, 4096), None),
    "iq swapped": ((64, 2048), None),
    "second segment dropped": ((64, 256, 4096), _SMANY),
    "segment twice": ((64, 256, 4096), _SMANY),
    "scale by groups": ((64, 256, 4096), _SMANY),
}


@pytest.mark.parametrize("mutant", SM.MUTANTS)
def test_every_mutant_leaves_tol_bin(mutant):
    """Each fault a kernel could have, applied to the float32 model, exceeds tol_bin in some bin on a named input at every
    N listed for it and in every format (the formats differ in the vector layout and the conversion)."""
    sizes, which = MUTANT_PLAN[mutant]
    for n_bins in sizes:
        for fmt in SM.FORMATS:
            best, at = 0.0, None
            shapes = SM.CRAFTED_SHAPES[n_bins] if which is None else (SM.CRAFTED_SHAPES[n_bins][which],)
            for shape in shapes:
                L = SM.shape_samples(shape)
                for kind in SM.kinds(fmt):
                    if kind == "zero":
                        continue
                    ref, s = SM.crafted_reference(kind, fmt, L, n_bins)
                    r = SM.excess(SM.kernel_f32(SM.crafted(kind, fmt, L, n_bins), fmt, n_bins, mutant), ref, n_bins)
                    best, at = (r, f"{kind} S={s}") if r > best else (best, at)
            print(f"\n[spectrum-mutant] {mutant}: {fmt} N={n_bins} caught by {at} at {best:.3g} tol_bin")
            assert best > 1.0, (mutant, fmt, n_bins, best)
    assert set(MUTANT_PLAN) == set(SM.MUTANTS)


def test_weak_bins_now_matter():
    """What the norm-wise tolerance could not see: the three-tone input's weak bins set to zero stays inside tol and
    leaves tol_bin, as does a thread's last owned bin at N = 4096 on that very input."""
    decim, bs, n_bins = 100, 128, 4096
    for fmt in SM.FORMATS:
        ref, _, t = SM.reference(fmt, decim * bs, n_bins)
        cut = np.where(ref < 1e-6 * ref.max(), 0.0, ref)
        assert np.abs(cut - ref).max() < 0.2 * t and SM.excess(cut, ref, n_bins) > 1.0
        lost = SM.kernel_f32(SM.chunk_input(fmt, decim * bs, n_bins), fmt, n_bins, "last owned bin")
        assert np.abs(lost - ref).max() < 0.2 * t and SM.excess(lost, ref, n_bins) > 1.0


def test_uint8_float_offset_variant_is_reported():
    """Not required to be caught: the uint8 sample as (float) k - 127.4f leaves an ABSOLUTE error of f32(127.4) - 127.4 =
    1.5e-6 counts, 3.8e-6 of the constant byte 127's value - beside 2 eps sqrt(T / P) it is marginal.  Printed per N."""
    for n_bins in sorted(SM.CRAFTED_SHAPES):
        L = SM.shape_samples(SM.CRAFTED_SHAPES[n_bins][0])
        out = []
        for kind in ("const127", "const128", "const127_128"):
            ref, _ = SM.crafted_reference(kind, "u8", L, n_bins)
            out.append((kind, SM.excess(SM.kernel_f32(SM.crafted(kind, "u8", L, n_bins), "u8", n_bins, SM.U8_FLOAT_OFFSET), ref, n_bins)))
        print(f"\n[spectrum-mutant] {SM.U8_FLOAT_OFFSET}: N={n_bins} " + ", ".join(f"{k} {r:.2f} tol_bin ({'caught' if r > 1 else 'not caught'})" for k, r in out))
        assert all(np.isfinite(r) for _, r in out)
