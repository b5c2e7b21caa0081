"""The channelizer's contract, made precise: an a-priori bound on how far the HIP kernel
(rtldavis_amd/csrc/rd_channelizer.hip, k_channelize) can land from the float64 model
(oracle/channelizer_oracle.py:channelize_z) in front of the quantiser, and a comparator that holds
every output byte to it; and the test signals.  A helper module of the suite (not a conftest): imported by
tests/test_channelizer.py and tests/test_wideband_stream.py."""
import numpy as np

from oracle import channelizer_oracle as CHO

U = 2.0 ** -24              # fp32 unit roundoff: |fl(a op b) - a op b| <= U |a op b|
# ASSUMPTION, not a measurement: the absolute error of the hardware v_sin_f32 / v_cos_f32 (their argument in
# revolutions, |x| < 1) on gfx950.  AMD does not document it and nobody here has measured it; the GPU sweep reports
# the room the whole bound leaves (assert_matches_model's `worst_ratio`), which is where a wrong figure would show.
SIN_ABS_ERR = 2.0 ** -16
Q127_4 = float(np.float32(127.4))


def _split_err(a, sexp):
    """|a - (hi + lo)| for the kernel's two-digit f16 split of a (rd_chan_create: hi = f16(a 2^s), lo = f16(a 2^s - hi)):
    with 2^e <= |a 2^s| < 2^(e+1), hi is off by at most 2^(e-11), lo (exponent <= e-11) by at most 2^(e-22) <= 2^-22 |a 2^s|;
    f16 subnormals (spacing 2^-24) floor this at 2^-25.  In the taps' own units (the kernel multiplies by 2^-s back)."""
    return np.maximum(2.0 ** -22 * np.abs(a), 2.0 ** -25 * 2.0 ** -sexp)


def error_bound(cfg, taps, Z, raw):
    """delta[c, t] >= |Z_kernel - Z_model| for both components of output t of channel c, in LSB (quantiser steps).

    cfg: .decim, .out_rate, .gain, .shift_hz (a Channelizer, a WidebandReceiver or a SimpleNamespace); taps: float64
    [T]; Z: channelize_z's value [n_channels, n_out]; raw: the capture (uint8 I,Q), whose bytes set the accumulator's
    partial sums.  Nothing here looks at a kernel result.

    The kernel (as a real GEMM on the raw bytes b, see the .hip header) computes, per channel, output and part,
        re = fl(acc 2^-s + d0),  acc = sum over K steps q of two MFMAs (f16 digits hi, lo of the fp32 taps g) of b,
    rotates (re, im) by a phasor (cs, sn) and quantises fl(fl(zr 127.6f) + 127.4f).  In accumulator units
    (w = 127.6 z, so Z - 127.4 = gain w), with M = |w| = |Z - 127.4 (1+j)| / gain, the terms are:
      1. fp32 taps (rd_chan_create: g = (float)(h e^{j phi}), phi from an exact remainder in float64):
         |dg| <= U |g| per component; d0 is summed from the same fp32 taps, so the error meets (b - 127.4) with
         |b - 127.4| <= 127.6:  E1 = 127.6 U sum_k (|g_r| + |g_i|)  (+ 2^-48 255 sum |h| for the float64 phase).
      2. the two-digit f16 split (_split_err, <= 2^-22 max|h| per tap), against bytes b <= 255:
         E2 = 255 sum_k (eps(g_r) + eps(g_i)).
      3. the fp32 accumulation.  The products are exact (an f16 digit times a byte 2^-24 has <= 19 significant bits).
         Each of the 2 (t_pad/8 + 1) MFMAs (K steps of 8 window samples, the hi digit then the lo one) adds 16 products
         to the accumulator; with no wider internal accumulation (the f32-input MFMA is a k-ordered fma chain; the f16
         form is assumed no better) that is 16 roundings, each of a value no larger than |A_{q-1}| + P_q, the exact
         partial sum before K step q plus the step's sum of |products| (for both digits: |A_{q-1}| + P_q bounds the
         running value inside the lo MFMA too).  So E3 = 32 U sum_q (|A_{q-1}| + P_q) per part, from the exact
         partial sums of this capture's bytes in the kernel's K order (taps t_pad .. 0) - a worst-case bound on the
         rounding, not a statistical one, and a factor (1 + 2^-10) for the second-order terms.
      4. the fp32 DC term d0 = (float)(-127.4 (1+j) sum g) (float64 sum): E4 = 127.4 sum(|g_r| + |g_i|)(U + t_pad 2^-53).
      5. fl(acc 2^-s + d0): U (M + E1..4).
      Before the rotation: E = |(E_re, E_im)|.
      6. the phasor: SIN_ABS_ERR per component of the hardware sine / cosine (an assumption, above), 2 pi 2^-25 from the
         argument rounded to fp32 revolutions, and up to three rotations by the fp32 32-step constant, each adding at
         most 8 U (constant off by sqrt2 U, three roundings of a 2x2 product): e_ph = sqrt2 SIN_ABS_ERR + 2 pi 2^-25 + 24 U;
         the rotated value is off by M e_ph + E (1 + e_ph), and its own arithmetic adds 3 sqrt2 U (M + E).
      7. scale = (float)gain * (1/127.6f) and the final * 127.6f: 5 U relative on Z - 127.4; 127.4f - 127.4 absolute;
         the last add U |Z|.
    """
    decim = int(cfg.decim)
    fo = int(cfg.out_rate)
    gain = float(cfg.gain)
    Z = np.asarray(Z)
    n_ch, n_out = Z.shape
    taps = np.asarray(taps, np.float64)
    T = taps.size
    t_pad = (T + 7) // 8 * 8
    n_q = t_pad // 8 + 1
    g = CHO.mod_taps(taps, cfg.shift_hz, fo * decim).astype(np.complex64).astype(np.complex128)  # the fp32 taps
    hmax = np.abs(taps).max()
    sexp = int(np.clip(14 - int(np.ceil(np.log2(hmax))), -60, 60)) if hmax > 0 else 0
    ag = np.abs(g.real) + np.abs(g.imag)
    e1 = 127.6 * U * ag.sum(1) + 2.0 ** -48 * 255 * np.abs(taps).sum()
    e2 = 255 * (_split_err(g.real, sexp) + _split_err(g.imag, sexp)).sum(1)
    e4 = 127.4 * ag.sum(1) * (U + t_pad * 2.0 ** -53)
    # 3: the kernel's window of output t is samples D t - t_pad + i, i < 8 n_q, against tap t_pad - i
    raw = np.asarray(raw, np.uint8).reshape(-1)
    b = raw[0::2].astype(np.float64) + 1j * raw[1::2].astype(np.float64)
    bpad = np.concatenate([np.zeros(t_pad, np.complex128), b, np.zeros(8, np.complex128)])
    wins = np.lib.stride_tricks.sliding_window_view(bpad, 8 * n_q)[::decim][:n_out]
    gw = np.zeros((n_ch, 8 * n_q), np.complex128)
    gw[:, t_pad - T + 1: t_pad + 1] = g[:, ::-1]
    agr, agi = np.abs(gw.real), np.abs(gw.imag)
    gwt = np.ascontiguousarray(gw.T)
    e3r = np.empty((n_out, n_ch))
    e3i = np.empty((n_out, n_ch))
    step = max(1, (1 << 21) // max(n_ch, 8 * n_q))
    for a in range(0, n_out, step):
        w = np.ascontiguousarray(wins[a:a + step])
        wr, wi = np.ascontiguousarray(w.real), np.ascontiguousarray(w.imag)
        # sum of |products| over the whole window: part re = |g_r| b_I + |g_i| b_Q, part im = |g_i| b_I + |g_r| b_Q
        pr = wr @ agr.T + wi @ agi.T
        pi = wr @ agi.T + wi @ agr.T
        acc = np.zeros((w.shape[0], n_ch), np.complex128)
        sr = np.zeros((w.shape[0], n_ch))
        si = np.zeros((w.shape[0], n_ch))
        for q in range(n_q):
            sr += np.abs(acc.real)
            si += np.abs(acc.imag)
            acc += w[:, 8 * q: 8 * q + 8] @ gwt[8 * q: 8 * q + 8]
        e3r[a:a + step] = 32 * U * (sr + pr)
        e3i[a:a + step] = 32 * U * (si + pi)
    e3r, e3i = e3r.T * (1 + 2.0 ** -10), e3i.T * (1 + 2.0 ** -10)
    M = np.abs(Z - 127.4 * (1 + 1j)) / gain
    base = (e1 + e2 + e4)[:, None]
    e_re = e3r + base
    e_im = e3i + base
    e_re = e_re + U * (M + e_re)
    e_im = e_im + U * (M + e_im)
    E = np.hypot(e_re, e_im)
    e_ph = np.sqrt(2) * SIN_ABS_ERR + 2 * np.pi * 2.0 ** -25 + 24 * U
    E_rot = M * e_ph + E * (1 + e_ph) + 3 * np.sqrt(2) * U * (M + E)
    zabs = np.maximum(np.abs(Z.real), np.abs(Z.imag))
    delta = gain * E_rot + 5 * U * gain * (M + E_rot) + abs(Q127_4 - 127.4) + U * (zabs + 1)
    return delta * (1 + 2.0 ** -10) + 1e-9


def random_taps(T, seed, highpass=False):
    """Asymmetric taps of mixed sign, unit L2 norm (highpass: their sum ~0, so the DC term dominates the output)."""
    h = np.random.default_rng(seed).standard_normal(T)
    if highpass:
        h -= h.mean()
    return h / np.linalg.norm(h)


def capture(n_samples, seed, fw):
    """Random bytes plus three tones at fixed frequencies: the outputs cover the quantiser's range."""
    rng = np.random.default_rng(seed)
    n = np.arange(n_samples)
    x = 40.0 * rng.standard_normal((n_samples, 2))
    for f, a in ((0.0071, 35.0), (-0.19, 30.0), (0.33, 25.0)):
        x[:, 0] += a * np.cos(2 * np.pi * f * n)
        x[:, 1] += a * np.sin(2 * np.pi * f * n)
    return np.clip(np.rint(127.4 + x), 0, 255).astype(np.uint8).reshape(-1)


def boundary_distance(F):
    """Distance of each real F to the nearest value where clip(rint(F), 0, 255) changes: k + 1/2, k = 0 .. 254."""
    F = np.asarray(F, np.float64)
    inner = np.abs(F - np.floor(F) - 0.5)
    return np.where(F < 0.5, 0.5 - F, np.where(F > 254.5, F - 254.5, inner))


def _interleave(Z):
    Z = np.asarray(Z)
    F = np.empty((Z.shape[0], 2 * Z.shape[1]))
    F[:, 0::2] = Z.real
    F[:, 1::2] = Z.imag
    return F


def check_against_model(got, Z, delta):
    """The comparison without the assertion: a dict with
    bad_lsb    - bytes more than one step from clip(rint(Z))                         (must be 0)
    bad_exact  - bytes that differ although Z is more than delta from every boundary (must be 0)
    exempt     - fraction of bytes within delta of a boundary (free to differ by one)
    mismatches - bytes that differ at all
    worst_dist - the largest boundary distance among the mismatches (LSB)
    worst_ratio- the largest boundary distance / delta among the mismatches: the share of the bound a kernel used
    delta_max  - the largest delta."""
    got = np.asarray(got)
    F = _interleave(Z)
    dl = np.broadcast_to(np.asarray(delta, np.float64), np.asarray(Z).shape)
    D = np.repeat(dl, 2, axis=1)
    assert got.shape == F.shape, (got.shape, F.shape)
    want = np.clip(np.rint(F), 0, 255)
    diff = np.abs(got.astype(np.float64) - want)
    dist = boundary_distance(F)
    exempt = dist <= D
    mism = diff != 0
    return dict(bad_lsb=int((diff > 1).sum()), bad_exact=int((mism & ~exempt).sum()), exempt=float(exempt.mean()),
                mismatches=int(mism.sum()), worst_dist=float(dist[mism].max()) if mism.any() else 0.0,
                worst_ratio=float((dist[mism] / D[mism]).max()) if mism.any() else 0.0, delta_max=float(D.max()))


def assert_matches_model(got, Z, delta):
    """Every byte of got (uint8 [n_channels, 2 n_out]) against the model Z (complex [n_channels, n_out]) with the
    bound delta (LSB, broadcast to Z): (i) never more than one step from clip(rint(Z), 0, 255); (ii) equal to it
    wherever Z is more than delta from every rounding boundary k + 1/2 (the clip edges included); (iii) returns the
    statistics of check_against_model, which a GPU run prints to show how much room the bound has."""
    s = check_against_model(got, Z, delta)
    assert s["bad_lsb"] == 0 and s["bad_exact"] == 0, s
    return s
