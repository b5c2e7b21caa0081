"""The channelizer's contract for float32 captures (include/rtldavis_hip.h: RD_IQ_CF32): the admitted value adm, the
float64 model, the a-priori bound of the kernel's distance from it, and test signals with the special values planted.
The companion of tests/chan_bound.py (uint8) and tests/chan_bound_fmt.py (int8, int16), whose comparator
(chan_bound.assert_matches_model) serves every format: the output is uint8 whatever the input.  A helper module of the
suite, imported by tests/test_channelizer_cf32.py and tests/test_wideband_cf32.py.  Nothing here touches a device."""
import numpy as np

import chan_bound as CB
from oracle import channelizer_oracle as CHO

U = CB.U
CLAMP = 8.0
PRESCALE_LOG2 = 12          # the kernel stages s = 2^12 adm(v) (rd_channelizer.hip: RD_CF32_PRESCALE_LOG2)
OFFSET = 127.4 * (1 + 1j)

# the values capture_cf32 plants: NaN, both infinities, a value past the clamp, -0.0, a float32 subnormal, 2^-15 (one
# int16 count), a UHD-scaled int16 (k / 32767 is no k' / 32768) and the largest float32 below 1
SPECIALS = np.array([np.nan, np.inf, -np.inf, 9.5, -0.0, 1e-40, 2.0 ** -15, 12345 / 32767, 1 - 2.0 ** -24], np.float32)


def adm(v):
    """The admitted value of float32 components: 0 for a NaN, otherwise clamped to [-8, +8] (so +-Inf is +-8); float64."""
    v = np.asarray(v)
    assert v.dtype == np.float32, v.dtype
    v = v.astype(np.float64)
    return np.where(np.isnan(v), 0.0, np.clip(v, -CLAMP, CLAMP))


def to_complex(raw):
    """The definition's x[n] of a capture (float32 I,Q interleaved, flat or [n, 2], or complex64 [n]), complex128."""
    raw = np.asarray(raw)
    if raw.dtype == np.complex64:
        raw = raw.view(np.float32)
    raw = raw.reshape(-1)
    return adm(raw[0::2]) + 1j * adm(raw[1::2])


def model_of_x(x, shift_hz, taps, decim, out_rate, gain, n_out=None):
    """The value in front of the quantiser for the complex signal x[n]: filter, mixer, gain (a number, or one per channel)."""
    decim = int(decim)
    n_out = x.size // decim if n_out is None else int(n_out)
    z = CHO.filter_decimate(x, CHO.mod_taps(taps, shift_hz, int(out_rate) * decim), decim, n_out)
    z *= CHO.out_phasor(shift_hz, out_rate, n_out)
    g = np.asarray(gain, np.float64)
    return (g[:, None] if g.ndim else g) * z * 127.6 + OFFSET


def model_z_cf32(raw, shift_hz, taps, decim, out_rate, gain, n_out=None):
    """channelize_z with x = adm(I) + j adm(Q)."""
    return model_of_x(to_complex(raw), shift_hz, taps, decim, out_rate, gain, n_out)


def split_f16(s):
    """The kernel's two digits of float32 values s: hi = f16(s), lo = f16(s - hi), numpy's round-to-nearest-even
    conversions (subnormal results kept), s - hi in float32.  Returns (hi, lo) as float16."""
    s = np.asarray(s, np.float32)
    hi = s.astype(np.float16)
    lo = (s - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def error_bound_cf32(cfg, taps, Z, raw):
    """delta[c, t] >= |Z_kernel - Z_model| for both components of output t of channel c, in LSB, for a float32 capture
    `raw`; Z = model_z_cf32(raw, ...).  cfg: .decim, .out_rate, .gain (a number or one per channel), .shift_hz.  Nothing
    here looks at a kernel result.

    The kernel (rd_channelizer.hip, RD_IQ_CF32) stages a component as s = 2^12 adm(v) - an exact power-of-two pre-scale
    whose inverse is folded into the tap scale: acc 2^(-sexp - 12) is the sum in x's units, and |s| <= 2^15 stays inside
    f16 - in two f16 digits hi = f16(s), lo = f16(s - hi), and runs int16's loop: K = 16 is 4 window samples x 2
    components x 2 digits, both digits against the same tap, each tap in two f16 terms, fp32 accumulation, no DC term, a
    sample outside the capture exactly 0.  FLOAT MODE: lo is an f16 subnormal whenever |s| < 2^-3, so the bound relies on
    the f32 -> f16 conversion producing subnormals (f16 denormals enabled, the default mode of a HIP kernel, round to
    nearest even); flushed, term 3's floor would be 2^-14 2^-11, not 2^-25.
    Units: x's own (full scale 1), G = gain 127.6, M = |Z - 127.4 (1+j)| / G.  Term by term as chan_bound.error_bound:
      1. fp32 taps: |dg| <= U |g| against this capture's samples: E1 = U P, P = sum_k (|g_r| |x_I| + |g_i| |x_Q|) for part
         re (g_i, g_r for im) (+ 2^-48 8 sum |h| for the float64 phase, |x| <= 8).
      2. the two-term f16 split of the taps: a scaled tap is off by max(2^-22 |g 2^sexp|, 2^-25); it meets both digits,
         |hi| + |lo| <= (1 + 2^-10) |s|: E2 = (1 + 2^-10) (2^-22 P + 2^(-25 - sexp) S), S = the window's sum of |x_I| + |x_Q|.
      3. the sample split: s - hi is exact in fp32 (both are multiples of ulp(s)), hi is off by at most 2^-11 |s|, lo by
         2^-11 of that or, in the subnormal range, half the spacing 2^-24: |s - hi - lo| <= max(2^-22 |s|, 2^-25), in
         x's units max(2^-22 |x|, 2^-37) - the pre-scale moved the floor from 2^-25; s itself is exact (a float32
         subnormal times 2^12 is below the floor either way).  Against the taps: E3 = 2^-22 P + 2^-37 sum_k (|g_r| + |g_i|).
      4. the fp32 accumulation.  Products are exact: 11 x 11 bits, the smallest non-zero one 2^-24 2^-24 = 2^-48, the
         largest 2^15 2^15, no underflow or overflow in fp32.  The digits of a component have its sign or are 2^-11 of
         it, so its products do not cancel beyond that: |A_{q-1}| + (1 + 2^-10) P_q bounds the running value inside K
         step q, with A the exact partial sums of g x and P_q the step's sum of |g| |x|; two MFMAs of 16 products per
         step: E4 = 32 U (1 + 2^-10) sum_q (|A_{q-1}| + P_q) over the t_pad/4 + 1 steps of 4 window samples, and the
         factor (1 + 2^-10) of chan_bound for the second-order terms.
      5. acc 2^(-sexp - 12) is exact, there is no DC term; U (M + E) is kept.
      6. the phasor: as uint8.     7. scale = gains[ch] (float32), the final * 127.6f + 127.4f: the 5 U are kept.
    """
    decim, fo = int(cfg.decim), int(cfg.out_rate)
    gain = np.asarray(cfg.gain, np.float64)
    Z = np.asarray(Z)
    n_ch, n_out = Z.shape
    G = (np.broadcast_to(gain, (n_ch,))[:, None] if gain.ndim else float(gain)) * 127.6
    taps = np.asarray(taps, np.float64)
    T = taps.size
    t_pad = (T + 7) // 8 * 8
    ks = 4
    n_q = t_pad // ks + 1
    g = CHO.mod_taps(taps, cfg.shift_hz, fo * decim).astype(np.complex64).astype(np.complex128)  # the fp32 taps
    hmax = np.abs(taps).max()
    sexp = int(np.clip(14 - int(np.ceil(np.log2(hmax))), -60, 60)) if hmax > 0 else 0
    ag = np.abs(g.real) + np.abs(g.imag)
    v = to_complex(raw)
    vpad = np.concatenate([np.zeros(t_pad, np.complex128), v, np.zeros(8, np.complex128)])
    wins = np.lib.stride_tricks.sliding_window_view(vpad, ks * n_q)[::decim][:n_out]
    gw = np.zeros((n_ch, ks * n_q), np.complex128)
    gw[:, t_pad - T + 1: t_pad + 1] = g[:, ::-1]
    agr, agi = np.abs(gw.real), np.abs(gw.imag)
    gwt = np.ascontiguousarray(gw.T)
    e4r, e4i = np.empty((n_out, n_ch)), np.empty((n_out, n_ch))
    pr_all, pi_all = np.empty((n_out, n_ch)), np.empty((n_out, n_ch))
    s_all = np.empty((n_out, 1))
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
        e4r[a:a + step] = 32 * U * (sr + pr)
        e4i[a:a + step] = 32 * U * (si + pi)
        pr_all[a:a + step], pi_all[a:a + step] = pr, pi
        s_all[a:a + step, 0] = wr.sum(1) + wi.sum(1)
    e4r, e4i = e4r.T * (1 + 2.0 ** -10) ** 2, e4i.T * (1 + 2.0 ** -10) ** 2
    phase = 2.0 ** -48 * CLAMP * np.abs(taps).sum()
    tap_floor = (1 + 2.0 ** -10) * 2.0 ** (-25 - sexp) * s_all.T                        # [1, n_out]
    smp_floor = (2.0 ** (-25 - PRESCALE_LOG2) * ag.sum(1))[:, None]                     # [n_ch, 1]
    rel = U + (1 + 2.0 ** -10) * 2.0 ** -22 + 2.0 ** -22
    e123r = rel * pr_all.T + tap_floor + smp_floor + phase
    e123i = rel * pi_all.T + tap_floor + smp_floor + phase
    M = np.abs(Z - OFFSET) / G
    e_re = e4r + e123r
    e_im = e4i + e123i
    e_re = e_re + U * (M + e_re)
    e_im = e_im + U * (M + e_im)
    E = np.hypot(e_re, e_im)
    e_ph = np.sqrt(2) * CB.SIN_ABS_ERR + 2 * np.pi * 2.0 ** -25 + 24 * U
    E_rot = M * e_ph + E * (1 + e_ph) + 3 * np.sqrt(2) * U * (M + E)
    zabs = np.maximum(np.abs(Z.real), np.abs(Z.imag))
    delta = G * E_rot + 5 * U * G * (M + E_rot) + abs(CB.Q127_4 - 127.4) + U * (zabs + 1)
    return delta * (1 + 2.0 ** -10) + 1e-9


def special_sites(n_samples):
    """Where capture_cf32 plants SPECIALS[j]: (sample, component) pairs.  Each value goes to sample j, component j % 2 -
    the first outputs of every dense configuration see it - and, where the capture is long enough, also to the samples
    160 (j + 1 + 9 m) - (j + m) % 8, m < 8: the sparsest configuration (decim 160, 8 taps: output t reads samples
    160 t - 7 .. 160 t, every sample meets one tap of one output) meets it once with each of its taps, so that not
    every output that sees a value of magnitude 8 is driven into the clip."""
    sites = []
    for j in range(SPECIALS.size):
        here = [j] + [160 * (j + 1 + 9 * m) - (j + m) % 8 for m in range(8)]
        sites.append([(n, j % 2) for n in here if n < n_samples])
    return sites


def plant_specials(pairs, base=0):
    """Write SPECIALS into the float32 [n, 2] array `pairs` at special_sites, shifted by `base` samples; in place."""
    assert pairs.dtype == np.float32 and pairs.ndim == 2
    for j, sites in enumerate(special_sites(pairs.shape[0] - base)):
        for n, comp in sites:
            pairs[base + n, comp] = SPECIALS[j]
    return pairs


def capture_cf32(n_samples, seed, level=1.0, specials=True):
    """chan_bound.capture's analogue in float32: random samples plus three tones, scaled so that the sum reaches the
    nominal full scale +-1 at level 1, where it is clipped as chan_bound_fmt.capture_fmt clips; `specials` plants
    SPECIALS (values past full scale among them) at special_sites.  Flat float32, I,Q interleaved."""
    rng = np.random.default_rng(seed)
    n = np.arange(n_samples)
    x = 40.0 * rng.standard_normal((n_samples, 2))
    for f, a in ((0.0071, 35.0), (-0.19, 30.0), (0.33, 25.0)):
        x[:, 0] += a * np.cos(2 * np.pi * f * n)
        x[:, 1] += a * np.sin(2 * np.pi * f * n)
    out = np.clip(x * (level / 128.0), -1.0, 1.0).astype(np.float32)
    if specials:
        plant_specials(out)
    return out.reshape(-1)


def input_levels(raw):
    """The input level record of a float32 chunk by its definition (include/rtldavis_hip.h), exact Python integers:
    k = clip(rint(adm(v) 32768), -32768, 32767), (peak, clipped, power)."""
    raw = np.asarray(raw, np.float32).reshape(-1)
    k = np.clip(np.rint(adm(raw) * 32768.0), -32768, 32767).astype(np.int64)
    clipped = int(((k == -32768) | (k == 32767) | np.isnan(raw)).sum())
    return int(np.abs(k).max()), clipped, int((k * k).sum())
