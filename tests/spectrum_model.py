"""Helpers shared by tests/test_spectrum_cpu.py and tests/test_wideband_spectrum.py (no tests in here): the float64 model of
the per-chunk power spectrum (include/rtldavis_hip.h, SPECTRUM), its a-priori tolerance, the launch arithmetic restated,
and the test inputs.  Nothing here touches a device.

Model: N = n_bins, L IQ pairs, S = L // N segments, periodic Hann w[n] = 0.5 - 0.5 cos(2 pi n / N),
    X_s[k] = sum_n w[n] x[s N + n] e^{-2 pi i k n / N},   P[j] = 1 / (S (N/2)^2) sum_s |X_s[(j + N/2) mod N]|^2
with x the samples in float64 (u8: (k - 127.4) / 127.6, s8: k / 128, s16: k / 32768, cf32: the float32 value clamped to
[-8, 8], a NaN taken as 0), NumPy's float64 FFT.

Tolerance, derived and not tuned.  With u = 2^-24, a Cooley-Tukey FFT in float32 with correctly rounded twiddles gives
||X^ - X||_2 <= eps ||X||_2, eps = (6.7 log2 N + 4) u: the first term is Higham's bound eta = mu + gamma_4 (sqrt 2 + mu)
per stage with mu = u (Accuracy and Stability of Numerical Algorithms, 2nd ed., theorem 24.2), the second covers the
sample conversion (1.5 u for u8), the float32 window, its product and the magnitude.  Per bin |X^|^2 - |X|^2 =
2 Re(conj X d) + |d|^2 <= (2 eps + eps^2) ||X||_2^2 at worst, and the float64 sums add nothing visible, hence
    |P_dev[j] - P_ref[j]| <= 2.01 eps sum_k P_ref[k] = tol,
about 1.0e-5 of the total power at N = 4096.  A measured excess is a bug in the kernel."""
import functools

import numpy as np

U = 2.0 ** -24
MAX_GROUPS = 64
FORMATS = ("u8", "s8", "s16", "cf32")
# (decim, block_size, n_bins): L = decim * block_size.  S = 8 and S = 1; S = 2 with 512 leftover samples; S = 200 > 64
# (several segments per workgroup, 64 partials) and S = 3 at the largest N
SHAPES = ((4, 128, 64), (4, 128, 512), (20, 128, 1024), (100, 128, 64), (100, 128, 4096))
TONES = ((0.5, 0.1137), (0.05, -0.3071), (0.005, 0.4219))     # (amplitude, cycles per sample): no two mirror each other


def samples(raw, fmt):
    """The capture (flat I,Q array of the format's dtype) as complex128, the definition's x."""
    a = np.asarray(raw).reshape(-1)
    if fmt == "cf32":
        v = a.astype(np.float64)
        v = np.where(np.isnan(v), 0.0, np.clip(v, -8.0, 8.0))
    elif fmt == "u8":
        v = (a.astype(np.float64) - 127.4) / 127.6
    else:
        v = a.astype(np.float64) / (128.0 if fmt == "s8" else 32768.0)
    return v[0::2] + 1j * v[1::2]


def window(n_bins):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_bins, dtype=np.float64) / n_bins)


def segment_spectra(raw, fmt, n_bins):
    """|X_s[k]|^2 in FFT order, float64 [S, N]."""
    x = samples(raw, fmt)
    s = x.size // n_bins
    assert s >= 1
    seg = x[: s * n_bins].reshape(s, n_bins) * window(n_bins)[None, :]
    return np.abs(np.fft.fft(seg, axis=1)) ** 2


def model(raw, fmt, n_bins):
    """(P float64 [N] in ascending frequency, S)."""
    m = segment_spectra(raw, fmt, n_bins)
    return np.fft.fftshift(m.sum(axis=0)) / (m.shape[0] * (n_bins / 2.0) ** 2), m.shape[0]


def eps(n_bins):
    return (6.7 * np.log2(n_bins) + 4.0) * U


def tol(p_ref, n_bins):
    return 2.01 * eps(n_bins) * float(np.sum(p_ref))


def freqs(centre_hz, wide_rate, n_bins):
    return np.asarray([centre_hz + (j - n_bins // 2) * wide_rate / n_bins for j in range(n_bins)], np.float64)


def launch_plan(n_samples, n_bins):
    """(S, G, the segments of every workgroup in the order it takes them)."""
    s = n_samples // n_bins
    g = min(s, MAX_GROUPS)
    return s, g, [list(range(k, s, g)) for k in range(g)]


def quantise(x, fmt):
    """complex128 -> the flat I,Q array of a format (the inverse of `samples` up to rounding)."""
    v = np.empty(2 * x.size, np.float64)
    v[0::2], v[1::2] = x.real, x.imag
    if fmt == "cf32":
        return v.astype(np.float32)
    dtype, scale, off = {"u8": (np.uint8, 127.6, 127.4), "s8": (np.int8, 128.0, 0.0), "s16": (np.int16, 32768.0, 0.0)}[fmt]
    lim = np.iinfo(dtype)
    return np.clip(np.rint(v * scale + off), lim.min, lim.max).astype(dtype)


@functools.lru_cache(maxsize=None)
def chunk_input(fmt, n_samples, n_bins, level=1.0):
    """One chunk of L IQ pairs: the three tones of TONES (none on a bin centre of any N used) plus seeded noise, scaled
    by `level`; the samples behind the last whole segment hold full-scale values (cf32: NaN and 1e30), so a kernel that
    reads them fails; cf32 also carries components at +-9 and NaN inside the used segments (the clamp, and NaN as 0)."""
    rng = np.random.default_rng(1000 * n_samples + n_bins + FORMATS.index(fmt))
    n = np.arange(n_samples, dtype=np.float64)
    x = sum(a * np.exp(2j * np.pi * (f * n + rng.random())) for a, f in TONES)
    x = level * (x + 0.002 * (rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples)))
    raw = quantise(x, fmt)
    used = 2 * (n_samples // n_bins) * n_bins
    if fmt == "cf32":
        raw[used::2] = np.nan
        raw[used + 1::2] = 1e30
        for i, v in ((5, 9.0), (2 * n_bins - 3, -9.0), (used // 2 + 1, np.nan), (used - 2, np.inf), (17, -np.inf)):
            raw[i] = v
    else:
        lim = np.iinfo(raw.dtype)
        raw[used::2] = lim.max
        raw[used + 1::2] = lim.min
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def reference(fmt, n_samples, n_bins, level=1.0):
    """(P_ref, S, tol) of chunk_input; computed once, read-only."""
    p, s = model(chunk_input(fmt, n_samples, n_bins, level), fmt, n_bins)
    p.setflags(write=False)
    return p, s, tol(p, n_bins)


def faults(raw, fmt, n_bins):
    """The model's output with one fault each: what a wrong kernel would give."""
    m = segment_spectra(raw, fmt, n_bins)
    s = m.shape[0]
    scale = s * (n_bins / 2.0) ** 2
    good = np.fft.fftshift(m.sum(axis=0)) / scale
    out = {"bin order reversed": good[::-1].copy(),
           "no fftshift": m.sum(axis=0) / scale,
           "conjugated transform": np.fft.fftshift(m.sum(axis=0)[(-np.arange(n_bins)) % n_bins]) / scale}
    if s > 1:
        out["last segment dropped"] = np.fft.fftshift(m[:-1].sum(axis=0)) / scale
        out["first segment dropped"] = np.fft.fftshift(m[1:].sum(axis=0)) / scale
    return good, out
