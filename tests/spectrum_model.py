"""Helpers shared by tests/test_spectrum_cpu.py and tests/test_wideband_spectrum.py (no tests in here): the float64 model of
the per-chunk power spectrum (include/rtldavis_hip.h, SPECTRUM), its two a-priori tolerances (per bin, which the device
comparisons use, and norm-wise, its upper bound), the launch arithmetic restated, a float32 restatement of k_chan_spectrum
with the faults a kernel could have, and the test inputs.  Nothing here touches a device.

Model: N = n_bins, L IQ pairs, S = L // N segments, periodic Hann w[n] = 0.5 - 0.5 cos(2 pi n / N),
    X_s[k] = sum_n w[n] x[s N + n] e^{-2 pi i k n / N},   P[j] = 1 / (S (N/2)^2) sum_s |X_s[(j + N/2) mod N]|^2
with x the samples in float64 (u8: (k - 127.4) / 127.6, s8: k / 128, s16: k / 32768, cf32: the float32 value clamped to
[-8, 8], a NaN taken as 0), NumPy's float64 FFT.

Tolerances, derived and not tuned.  With u = 2^-24, a Cooley-Tukey FFT in float32 with correctly rounded twiddles gives
||X^_s - X_s||_2 <= eps ||X_s||_2 per segment, eps = (6.7 log2 N + 4) u: the first term is Higham's bound eta = mu +
gamma_4 (sqrt 2 + mu) per stage with mu = u (Accuracy and Stability of Numerical Algorithms, 2nd ed., theorem 24.2), the
second covers the sample conversion (1.5 u for u8), the float32 window, its product and the magnitude.  Per bin the error
d_sk = X^_s[k] - X_s[k] has |d_sk| <= ||d_s||_2 <= eps ||X_s||_2 and |X^|^2 - |X|^2 = 2 Re(conj X d) + |d|^2, so with T =
sum_k P_ref[k] (Parseval: sum_s ||X_s||^2 = S (N/2)^2 T) and Cauchy-Schwarz over the segments
    |P_dev[k] - P_ref[k]| <= 2 eps sqrt(P_ref[k] T) + eps^2 T = tol_bin[k]:
a weak bin is held to an error in proportion to its own amplitude, so a kernel that loses or misplaces a weak bin fails.
The float64 sums add nothing visible.  P_ref[k] <= T gives the norm-wise figure every bin shares,
    tol_bin[k] <= (2 eps + eps^2) T <= 2.01 eps T = tol,
about 1.0e-5 of the total power at N = 4096; the CPU tests of the model's own faults use it, the device comparisons use
tol_bin.  A measured excess over either is a bug in the kernel.

kernel_f32 restates k_chan_spectrum (rd_spectrum.hip) in NumPy float32 - conversions, tables, bit-reversed store, fused
radix-2 passes, float32 |X|^2, float64 sums in the kernel's order, scale - one rounding per operation, as the library is
built (no contraction).  Bit equality with the device is not asserted: the tables come from another cos and sin.  It shows
(tests/test_spectrum_cpu.py) that the arithmetic stays within 0.25 tol_bin on every input of the device test and that each
fault of MUTANTS leaves tol_bin on one of them."""
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


def tol_bin(p_ref, n_bins):
    """float64 [N]: 2 eps sqrt(P_ref[k] T) + eps^2 T, T = sum_k P_ref[k]; every entry <= tol(p_ref, n_bins)."""
    p = np.asarray(p_ref, np.float64)
    e, t = eps(n_bins), float(np.sum(p))
    return 2.0 * e * np.sqrt(p * t) + e * e * t


def excess(p, p_ref, n_bins):
    """max_k |p[k] - p_ref[k]| / tol_bin[k]: <= 1 passes.  An all-zero reference (tol_bin = 0) admits only zeros: 0.0 then,
    inf otherwise."""
    d = np.abs(np.asarray(p, np.float64) - p_ref)
    t = tol_bin(p_ref, n_bins)
    if not np.all(np.isfinite(d)):
        return float("inf")
    if float(t.max()) == 0.0:
        return 0.0 if float(d.max()) == 0.0 else float("inf")
    return float((d / t).max())


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


# ------------------------------------------------------------------------------------------ crafted inputs
# Inputs in which every bin and every table entry matters (chunk_input's three tones leave most bins at the noise floor,
# where the norm-wise tolerance saw nothing).  Seeded, read-only, the same poison behind the last whole segment.
#   impulses   two impulses per segment at drawn positions n0 != n1 of opposite parity (so that they meet in the LAST
#              butterfly stage, through its twiddle) with complex values of 0.6 and 0.5 of full scale, everything else
#              the format's zero (uint8: byte 127, the value -0.4 / 127.6): every bin carries power that depends on the
#              relative phase e^{-2 pi i k (n0 - n1) / N}
#   noise      white Gaussian noise at -10 dBFS: a flat spectrum, every bin strong
#   tones      (s16 and cf32) a bin-centred tone at 0.9 of full scale and one WEAK_DB below it at a distant frequency off
#              every bin centre.  WEAK_DB = -76: at -80 dB the weak tone's bin exceeds tol_bin there by 7.9x only at N =
#              4096 (about sqrt(P_k / T) / (2 eps)); at -76 dB by 12x there and more at every smaller N
#              (test_spectrum_cpu.py asserts 10x)
#   hop        a different tone in every segment, its frequency a function of the segment index
#   const127, const128, const127_128 (uint8)   constant bytes, the last with I = 127 and Q = 128
#   zero       (s8, s16, cf32) all zero: every bin reads exactly 0.0
WEAK_DB = -76.0
STRONG_AMP = 0.9
WEAK_FREQ = -0.3071
IMPULSE_AMPS = (0.6, 0.5)


def kinds(fmt):
    """The crafted inputs of a format, in the order the tests take them."""
    base = ["impulses", "noise", "hop"]
    if fmt in ("s16", "cf32"):
        base.append("tones")
    return tuple(base + (["const127", "const128", "const127_128"] if fmt == "u8" else ["zero"]))


def strong_bin(n_bins):
    """FFT index of the strong tone of `tones` (ascending index: + N/2)."""
    return n_bins // 8 + 3


def hop_bin(seg, n_bins):
    """FFT index of segment seg's tone in `hop`: distinct for neighbouring segments and for segments G = 64 apart."""
    return (37 * seg + 5 + seg // 64) % n_bins


def impulse_sites(fmt, n_samples, n_bins):
    """(n0, n1) int64 [S] each: the impulses' positions in their segments, n0 even and n1 odd, both in the window's upper
    three quarters (w >= 0.14)."""
    rng = np.random.default_rng(77 * n_samples + n_bins + FORMATS.index(fmt))
    s = n_samples // n_bins
    lo, hi = n_bins // 8, n_bins - n_bins // 8
    n0 = 2 * rng.integers((lo + 1) // 2, hi // 2, s)
    n1 = 2 * rng.integers(lo // 2, hi // 2, s) + 1
    return n0.astype(np.int64), n1.astype(np.int64)


def _poison(raw, n_samples, n_bins, fmt):
    used = 2 * (n_samples // n_bins) * n_bins
    if fmt == "cf32":
        raw[used::2] = np.nan
        raw[used + 1::2] = 1e30
    else:
        lim = np.iinfo(raw.dtype)
        raw[used::2] = lim.max
        raw[used + 1::2] = lim.min
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def crafted(kind, fmt, n_samples, n_bins):
    """One chunk of n_samples IQ pairs of the crafted input `kind` (above) for n_bins: flat I,Q of the format's dtype."""
    assert kind in kinds(fmt), (kind, fmt)
    rng = np.random.default_rng(9000 * n_samples + 10 * n_bins + FORMATS.index(fmt) + 100003 * kinds(fmt).index(kind))
    s = n_samples // n_bins
    n = np.arange(n_samples, dtype=np.float64)
    seg, m = np.divmod(np.arange(n_samples), n_bins)
    if kind == "noise":
        sigma = np.sqrt(0.1 / 2.0)
        raw = quantise(sigma * (rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples)), fmt)
    elif kind == "tones":
        weak = STRONG_AMP * 10.0 ** (WEAK_DB / 20.0)
        x = STRONG_AMP * np.exp(2j * np.pi * (strong_bin(n_bins) * m / n_bins + rng.random()))
        raw = quantise(x + weak * np.exp(2j * np.pi * (WEAK_FREQ * n + rng.random())), fmt)
    elif kind == "hop":
        k = np.asarray([hop_bin(v, n_bins) for v in range(s + 1)], np.float64)
        raw = quantise(0.5 * np.exp(2j * np.pi * (k[seg] * m / n_bins + rng.random(s + 1)[seg])), fmt)
    elif kind == "impulses":
        raw = quantise(np.zeros(n_samples, np.complex128), fmt)
        if fmt == "u8":
            raw[:] = 127
        n0, n1 = impulse_sites(fmt, n_samples, n_bins)
        for sites, amp in ((n0, IMPULSE_AMPS[0]), (n1, IMPULSE_AMPS[1])):
            at = np.arange(s) * n_bins + sites
            v = quantise(amp * np.exp(2j * np.pi * rng.random(s)), fmt)
            raw[2 * at], raw[2 * at + 1] = v[0::2], v[1::2]
    else:
        dtype = {"u8": np.uint8, "s8": np.int8, "s16": np.int16, "cf32": np.float32}[fmt]
        raw = np.zeros(2 * n_samples, dtype)
        if kind != "zero":
            raw[0::2] = 128 if kind == "const128" else 127
            raw[1::2] = 127 if kind == "const127" else 128
    return _poison(raw, n_samples, n_bins, fmt)


@functools.lru_cache(maxsize=None)
def crafted_reference(kind, fmt, n_samples, n_bins):
    """(P_ref, S) of crafted(...); computed once, read-only."""
    p, s = model(crafted(kind, fmt, n_samples, n_bins), fmt, n_bins)
    p.setflags(write=False)
    return p, s


def impulses_closed_form(fmt, n_samples, n_bins):
    """P of the `impulses` input from |X[k]|^2 = |a0|^2 w0^2 + |a1|^2 w1^2 + 2 Re(a0 conj(a1) w0 w1 e^{-2 pi i k (n0 - n1) / N})
    per segment, a0 and a1 the quantised values: float64 [N] ascending.  Not for uint8, whose zero is not zero."""
    assert fmt != "u8"
    x = samples(crafted("impulses", fmt, n_samples, n_bins), fmt)
    n0, n1 = impulse_sites(fmt, n_samples, n_bins)
    s = n_samples // n_bins
    w = window(n_bins)
    k = np.arange(n_bins, dtype=np.float64)
    acc = np.zeros(n_bins)
    for i in range(s):
        a0, a1 = x[i * n_bins + n0[i]] * w[n0[i]], x[i * n_bins + n1[i]] * w[n1[i]]
        acc += abs(a0) ** 2 + abs(a1) ** 2 + 2.0 * np.real(a0 * np.conj(a1) * np.exp(-2j * np.pi * k * ((n0[i] - n1[i]) % n_bins) / n_bins))
    return np.fft.fftshift(acc) / (s * (n_bins / 2.0) ** 2)


# Shapes per N, the smallest that reach each path: S = 1; a small S with leftover samples; S = 65 .. 70 (64 workgroups
# with one or two segments each).  ("rx", decim, block_size) is a valid receiver chunk (block_size % 128 == 0, decim % 4
# == 0, decim <= 160) and goes through WidebandReceiver; a chunk is a multiple of 512 samples, so the shapes no receiver
# can have - S = 1 below N = 512, leftover samples up to N = 512, 65 .. 70 segments at N = 64 - are ("one", L): L samples
# uploaded to a Channelizer, the same kernel and launch helper.  The largest chunk, 28 * 10368, is 290304 samples.
CRAFTED_SHAPES = {
    64: (("one", 64 + 24), ("rx", 4, 128), ("one", 3 * 64 + 40), ("one", 67 * 64 + 8)),
    128: (("one", 128 + 24), ("one", 3 * 128 + 40), ("rx", 68, 128)),
    256: (("one", 256 + 24), ("one", 3 * 256 + 40), ("rx", 132, 128)),
    512: (("rx", 4, 128), ("one", 3 * 512 + 40), ("rx", 20, 1664)),
    1024: (("rx", 12, 128), ("rx", 28, 128), ("rx", 28, 2432)),
    2048: (("rx", 20, 128), ("rx", 52, 128), ("rx", 36, 3712)),
    4096: (("rx", 40, 128), ("rx", 100, 128), ("rx", 28, 10368)),
}


def shape_samples(shape):
    return shape[1] if shape[0] == "one" else shape[1] * shape[2]


# ------------------------------------------------------------------------------------------ the kernel in float32
F32 = np.float32
VECTOR_SAMPLES = {"u8": 8, "s8": 8, "s16": 4, "cf32": 2}      # samples per 16-byte vector
MUTANTS = ("last owned bin", "twiddle last stage", "twiddle middle stage", "w2 from stage h", "lone stage skipped",
           "store unpadded", "window shifted", "vector reversed", "iq swapped", "second segment dropped", "segment twice",
           "scale by groups")
U8_FLOAT_OFFSET = "u8 as k - 127.4f"                          # reported, not required to be caught


def pad(i):
    """rd_sp_pad: element i of the segment lives at i + (i >> 5)."""
    return i + (i >> 5)


def bit_reverse(n_bins):
    b = int(n_bins).bit_length() - 1
    i = np.arange(n_bins)
    r = np.zeros(n_bins, np.int64)
    for k in range(b):
        r |= ((i >> k) & 1) << (b - 1 - k)
    return r


@functools.lru_cache(maxsize=None)
def tables_f32(n_bins):
    """(win float32 [N], twiddle re, im float32 [N]) as rd_spec_prepare builds them: float64, rounded once; twiddle entry
    h + j = e^{-2 pi i j / 2h}, j < h, entry 0 = 1."""
    win = window(n_bins).astype(F32)
    tr, ti = np.zeros(n_bins, F32), np.zeros(n_bins, F32)
    tr[0] = 1.0
    h = 1
    while h < n_bins:
        ph = -2.0 * np.pi * np.arange(h, dtype=np.float64) / (2 * h)
        tr[h: 2 * h], ti[h: 2 * h] = np.cos(ph), np.sin(ph)
        h <<= 1
    for a in (win, tr, ti):
        a.setflags(write=False)
    return win, tr, ti


def samples_f32(raw, fmt, mutant=None):
    """(I, Q) float32 of a capture by sp_sample's arithmetic."""
    a = np.asarray(raw).reshape(-1)
    if fmt == "cf32":
        v = a.astype(F32)
        v = np.where(np.isnan(v), F32(0.0), np.minimum(np.maximum(v, F32(-8.0)), F32(8.0))).astype(F32)
    elif fmt == "u8":
        if mutant == U8_FLOAT_OFFSET:
            v = (a.astype(F32) - F32(127.4)) / F32(127.6)
        else:
            v = (10 * a.astype(np.int64) - 1274).astype(F32) * (F32(1.0) / F32(1276.0))
    else:
        v = a.astype(F32) * (F32(1.0) / F32(128.0 if fmt == "s8" else 32768.0))
    assert v.dtype == F32
    return v[0::2], v[1::2]


def _cmul(wr, wi, ar, ai):
    return wr * ar - wi * ai, wr * ai + wi * ar


def kernel_f32(raw, fmt, n_bins, mutant=None):
    """k_chan_spectrum restated: P float64 [N] ascending.  `mutant`: None, one of MUTANTS or U8_FLOAT_OFFSET."""
    assert mutant is None or mutant in MUTANTS or mutant == U8_FLOAT_OFFSET, mutant
    n = int(n_bins)
    log2n = n.bit_length() - 1
    a = np.asarray(raw).reshape(-1)
    s = a.size // 2 // n
    g = min(s, MAX_GROUPS)
    re, im = samples_f32(a[: 2 * s * n], fmt, mutant)
    if mutant == "iq swapped":
        re, im = im, re
    re, im = re.reshape(s, n), im.reshape(s, n)
    if mutant == "vector reversed":
        vs = VECTOR_SAMPLES[fmt]
        re, im = (v.reshape(s, n // vs, vs)[:, :, ::-1].reshape(s, n) for v in (re, im))
    win, tr, ti = tables_f32(n)
    if mutant == "window shifted":
        win = np.roll(win, -1)                                    # win[nn + 1]
    if mutant in ("twiddle last stage", "twiddle middle stage"):
        h = n // 2 if mutant == "twiddle last stage" else 1 << (log2n // 2)
        tr, ti = tr.copy(), ti.copy()
        tr[h + h // 3], ti[h + h // 3] = tr[h + h // 3 + 1], ti[h + h // 3 + 1]
    br = bit_reverse(n)
    xr, xi = np.zeros((s, pad(n)), F32), np.zeros((s, pad(n)), F32)     # the padded segment in LDS
    at = br if mutant == "store unpadded" else pad(br)
    xr[:, at], xi[:, at] = re * win, im * win
    xr, xi = xr[:, pad(np.arange(n))], xi[:, pad(np.arange(n))]         # logical order from here on
    h = 1
    if log2n & 1:
        if mutant != "lone stage skipped":
            ar, ai, b_r, b_i = xr[:, 0::2].copy(), xi[:, 0::2].copy(), xr[:, 1::2].copy(), xi[:, 1::2].copy()
            xr[:, 0::2], xi[:, 0::2], xr[:, 1::2], xi[:, 1::2] = ar + b_r, ai + b_i, ar - b_r, ai - b_i
        h = 2
    q = np.arange(n // 4)
    while h < n:
        j = q & (h - 1)
        b = ((q - j) << 2) + j
        i0, i1, i2, i3 = b, b + h, b + 2 * h, b + 3 * h
        h2 = h if mutant == "w2 from stage h" else 2 * h
        a0r, a0i, a1r, a1i, a2r, a2i, a3r, a3i = (v[:, i] for i in (i0, i1, i2, i3) for v in (xr, xi))
        t1r, t1i = _cmul(tr[h + j], ti[h + j], a1r, a1i)
        t3r, t3i = _cmul(tr[h + j], ti[h + j], a3r, a3i)
        b0r, b0i, b1r, b1i = a0r + t1r, a0i + t1i, a0r - t1r, a0i - t1i
        b2r, b2i, b3r, b3i = a2r + t3r, a2i + t3i, a2r - t3r, a2i - t3i
        u2r, u2i = _cmul(tr[h2 + j], ti[h2 + j], b2r, b2i)
        u3r, u3i = _cmul(tr[3 * h + j], ti[3 * h + j], b3r, b3i)
        xr[:, i0], xi[:, i0] = b0r + u2r, b0i + u2i
        xr[:, i2], xi[:, i2] = b0r - u2r, b0i - u2i
        xr[:, i1], xi[:, i1] = b1r + u3r, b1i + u3i
        xr[:, i3], xi[:, i3] = b1r - u3r, b1i - u3i
        h <<= 2
    assert xr.dtype == F32 and xi.dtype == F32
    src = np.arange(n) ^ (n >> 1)
    p32 = xr[:, src] * xr[:, src] + xi[:, src] * xi[:, src]
    assert p32.dtype == F32
    part = np.zeros((g, n), np.float64)
    for seg in range(s):                                          # workgroup seg % G takes its segments in ascending order
        if mutant == "second segment dropped" and g <= seg < 2 * g:
            continue
        part[seg % g] += p32[seg].astype(np.float64)
        if mutant == "segment twice" and seg == g:
            part[seg % g] += p32[seg].astype(np.float64)
    total = np.zeros(n, np.float64)
    for k in range(g):                                            # the last workgroup adds the partials in ascending g
        total += part[k]
    if mutant == "last owned bin":
        total[n - 256:] = 0.0                                     # bin tid + 256 (N / 256 - 1) of every thread
    scale = 1.0 / (float(g if mutant == "scale by groups" else s) * float(n // 2) * float(n // 2))
    return total * scale
