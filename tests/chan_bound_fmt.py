"""The channelizer's contract for the signed sample formats (include/rtldavis_hip.h: RD_IQ_S8, RD_IQ_S16): the float64
model of a format, the a-priori bound of the kernel's distance from it, and test signals.  The companion of
tests/chan_bound.py (uint8), whose comparator (assert_matches_model) serves every format: the output is uint8 whatever
the input.  A helper module of the suite, imported by tests/test_channelizer_formats.py and tests/test_wideband_formats.py."""
import numpy as np

import chan_bound as CB
from oracle import channelizer_oracle as CHO

U = CB.U
DTYPE = {"u8": np.uint8, "s8": np.int8, "s16": np.int16}
FULL_SCALE = {"u8": 127.6, "s8": 128.0, "s16": 32768.0}


def to_complex(raw, fmt):
    """The definition's x[n] of a capture (I,Q interleaved, flat or [n, 2]) in format fmt, complex128."""
    raw = np.asarray(raw)
    assert raw.dtype == DTYPE[fmt], (raw.dtype, fmt)
    raw = raw.reshape(-1)
    if fmt == "u8":
        return CHO.lut(raw)
    return (raw[0::2].astype(np.float64) + 1j * raw[1::2].astype(np.float64)) / FULL_SCALE[fmt]


def model_z(raw, fmt, shift_hz, taps, decim, out_rate, gain, n_out=None):
    """The value in front of the quantiser for a capture in format fmt: channelize_z with the format's x."""
    x = to_complex(raw, fmt)
    decim = int(decim)
    n_out = x.size // decim if n_out is None else int(n_out)
    z = CHO.filter_decimate(x, CHO.mod_taps(taps, shift_hz, int(out_rate) * decim), decim, n_out)
    z *= CHO.out_phasor(shift_hz, out_rate, n_out)
    return gain * z * 127.6 + 127.4 * (1 + 1j)


def error_bound_fmt(cfg, taps, Z, raw, fmt):
    """delta[c, t] >= |Z_kernel - Z_model| for both components of output t of channel c, in LSB, for a capture `raw`
    in format fmt; Z = model_z(raw, fmt, ...).  "u8" is chan_bound.error_bound.  Nothing here looks at a kernel result.

    Units: the kernel's accumulator holds a = FS z in the format's own counts (FS = 128 or 32768), so that
    Z - 127.4 (1+j) = G a with G = gain 127.6 / FS, and M = |a|.  Term by term as chan_bound.error_bound (same numbers):

    "s8" - the kernel flips bit 7 of every byte while staging, b = s + 128 in 0 .. 255, and then runs the uint8 loop;
    a sample outside the capture is staged as 0x80, the value 0, so every output carries the steady DC term:
      1. fp32 taps against |b - 128| <= 128: E1 = 128 U sum_k (|g_r| + |g_i|) (+ 2^-48 255 sum |h|).
      2. the f16 split against b <= 255: E2 = 255 sum_k (eps(g_r) + eps(g_i)), as uint8.
      3. the fp32 accumulation, E3 = 32 U sum_q (|A_{q-1}| + P_q) over K steps of 8 window samples, from the exact
         partial sums of this capture's offset bytes, the samples before the capture being 128 (not 0, as for uint8).
      4. the fp32 DC term d0 = (float)(-128 (1+j) sum g): E4 = 128 sum (|g_r| + |g_i|)(U + t_pad 2^-53).
      5. fl(acc 2^-s + d0): U (M + E1..4).     6. the phasor, 7. the scale and the quantiser's constants: as uint8
         (the scale (float)gain / 128 has one rounding less than gain (1/127.6f); the 5 U are kept).

    "s16" - a component s = sg (256 mh + ml) is staged as two f16 subnormals sg ml 2^-24, sg mh 2^-24 (sign-magnitude
    digits, mh <= 128, ml <= 255; K = 16 is 4 window samples x 2 components x 2 digits), the low digit against taps
    scaled 2^(s-8), the high one against taps scaled 2^s, each tap in two f16 terms; there is no DC term, a sample
    outside the capture is the value 0 exactly:
      1. fp32 taps: |dg| <= U |g| against this capture's samples: E1 = U P, P = sum_k (|g_r| |s_I| + |g_i| |s_Q|) for part
         re (g_i, g_r for im) - the sum of |products| of term 3 (+ 2^-48 32768 sum |h| for the float64 phase).
      2. the f16 split: the high digit's tap is off by max(2^-22 |g 2^s|, 2^-25), the low one's by max(2^-22 |g 2^(s-8)|,
         2^-25) (f16 subnormal spacing 2^-24); times the digit and back in counts (2^(8-s)) a product is off by at most
         2^-22 |g| (256 mh + ml) + 2^-25 2^(8-s) (mh + ml):  E2 = 2^-22 P + 2 t_pad 383 2^(-17-s).
      3. the fp32 accumulation.  Products are exact (11 x 8 bits).  Both digits of a component have its sign, so the
         products of one sample do not cancel: |g 256 mh| + |g ml| = |g| |s|, and |A_{q-1}| + P_q bounds the running value
         inside K step q as for uint8, with A the exact partial sums of g s and P_q the step's sum of |g| |s|; two MFMAs
         of 16 products per step: E3 = 32 U sum_q (|A_{q-1}| + P_q) over the t_pad/4 + 1 steps of 4 window samples.
         Because the digits are signed, A and P are of the signal's size, not of full scale - offset-binary digits would
         put 32768 sum g into every partial sum.
      4. no DC term: E4 = 0.     5. acc 2^(8-s) is exact; U (M + E) is kept.     6., 7.: as uint8.
    """
    if fmt == "u8":
        return CB.error_bound(cfg, taps, Z, raw)
    assert fmt in ("s8", "s16"), fmt
    decim, fo, gain = int(cfg.decim), int(cfg.out_rate), float(cfg.gain)
    Z = np.asarray(Z)
    n_ch, n_out = Z.shape
    taps = np.asarray(taps, np.float64)
    T = taps.size
    t_pad = (T + 7) // 8 * 8
    ks = 8 if fmt == "s8" else 4
    n_q = t_pad // ks + 1
    g = CHO.mod_taps(taps, cfg.shift_hz, fo * decim).astype(np.complex64).astype(np.complex128)  # the fp32 taps
    hmax = np.abs(taps).max()
    sexp = int(np.clip(14 - int(np.ceil(np.log2(hmax))), -60, 60)) if hmax > 0 else 0
    ag = np.abs(g.real) + np.abs(g.imag)
    raw = np.asarray(raw)
    assert raw.dtype == DTYPE[fmt], (raw.dtype, fmt)
    raw = raw.reshape(-1).astype(np.float64)
    if fmt == "s8":
        v = (raw[0::2] + 128.0) + 1j * (raw[1::2] + 128.0)      # the staged offset bytes
        front = np.full(t_pad, 128.0 * (1 + 1j))
        e1 = (128.0 * U * ag.sum(1) + 2.0 ** -48 * 255 * np.abs(taps).sum())[:, None]
        e2 = (255 * (CB._split_err(g.real, sexp) + CB._split_err(g.imag, sexp)).sum(1))[:, None]
        e4 = (128.0 * ag.sum(1) * (U + t_pad * 2.0 ** -53))[:, None]
    else:
        v = raw[0::2] + 1j * raw[1::2]
        front = np.zeros(t_pad, np.complex128)
        e4 = 0.0
    vpad = np.concatenate([front, v, np.zeros(8, np.complex128)])
    wins = np.lib.stride_tricks.sliding_window_view(vpad, ks * n_q)[::decim][:n_out]
    gw = np.zeros((n_ch, ks * n_q), np.complex128)
    gw[:, t_pad - T + 1: t_pad + 1] = g[:, ::-1]
    agr, agi = np.abs(gw.real), np.abs(gw.imag)
    gwt = np.ascontiguousarray(gw.T)
    e3r, e3i = np.empty((n_out, n_ch)), np.empty((n_out, n_ch))
    pr_all, pi_all = np.empty((n_out, n_ch)), np.empty((n_out, n_ch))
    step = max(1, (1 << 21) // max(n_ch, ks * n_q))
    for a in range(0, n_out, step):
        w = np.ascontiguousarray(wins[a:a + step])
        wr, wi = np.abs(w.real), np.abs(w.imag)
        pr = wr @ agr.T + wi @ agi.T       # the whole window's sum of |products|, part re; part im:
        pi = wr @ agi.T + wi @ agr.T
        acc = np.zeros((w.shape[0], n_ch), np.complex128)
        sr = np.zeros((w.shape[0], n_ch))
        si = np.zeros((w.shape[0], n_ch))
        for q in range(n_q):
            sr += np.abs(acc.real)
            si += np.abs(acc.imag)
            acc += w[:, ks * q: ks * q + ks] @ gwt[ks * q: ks * q + ks]
        e3r[a:a + step] = 32 * U * (sr + pr)
        e3i[a:a + step] = 32 * U * (si + pi)
        pr_all[a:a + step], pi_all[a:a + step] = pr, pi
    e3r, e3i = e3r.T * (1 + 2.0 ** -10), e3i.T * (1 + 2.0 ** -10)
    if fmt == "s16":
        floor = 2 * t_pad * 383 * 2.0 ** (-17 - sexp)
        phase = 2.0 ** -48 * 32768 * np.abs(taps).sum()
        e12r = (U + 2.0 ** -22) * pr_all.T + floor + phase
        e12i = (U + 2.0 ** -22) * pi_all.T + floor + phase
    else:
        e12r = e12i = e1 + e2
    G = gain * 127.6 / FULL_SCALE[fmt]
    M = np.abs(Z - 127.4 * (1 + 1j)) / G
    e_re = e3r + e12r + e4
    e_im = e3i + e12i + e4
    e_re = e_re + U * (M + e_re)
    e_im = e_im + U * (M + e_im)
    E = np.hypot(e_re, e_im)
    e_ph = np.sqrt(2) * CB.SIN_ABS_ERR + 2 * np.pi * 2.0 ** -25 + 24 * U
    E_rot = M * e_ph + E * (1 + e_ph) + 3 * np.sqrt(2) * U * (M + E)
    zabs = np.maximum(np.abs(Z.real), np.abs(Z.imag))
    delta = G * E_rot + 5 * U * G * (M + E_rot) + abs(CB.Q127_4 - 127.4) + U * (zabs + 1)
    return delta * (1 + 2.0 ** -10) + 1e-9


def capture_fmt(n_samples, seed, fmt, level=1.0, ends=True):
    """chan_bound.capture's analogue in a signed format: random samples plus three tones, scaled so that the sum
    reaches both ends of the format's range (ends: the ends themselves are planted at samples 3 and 5)."""
    hi = {"s8": 127, "s16": 32767}[fmt]
    rng = np.random.default_rng(seed)
    n = np.arange(n_samples)
    x = 40.0 * rng.standard_normal((n_samples, 2))
    for f, a in ((0.0071, 35.0), (-0.19, 30.0), (0.33, 25.0)):
        x[:, 0] += a * np.cos(2 * np.pi * f * n)
        x[:, 1] += a * np.sin(2 * np.pi * f * n)
    out = np.clip(np.rint(x * (level * (hi + 1) / 128.0)), -hi - 1, hi).astype(DTYPE[fmt])
    if ends and n_samples > 5:
        out[3] = (-hi - 1, hi)
        out[5] = (hi, -hi - 1)
    return out.reshape(-1)
