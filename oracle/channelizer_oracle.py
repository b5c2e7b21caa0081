"""TEST INFRASTRUCTURE - float64 restatement of the wideband channelizer's definition
(rtldavis_amd/csrc/rd_channelizer.hip).  PARITY UNPINNED: rtldavis has no channelizer (it retunes
one dongle per hop, /root/reference/src/rtldavis/runners/rtlsdr.py:51,72), so there is no reference
output to pin this against; the tests tie it to the reference through the packets the (pinned)
demodulator recovers from its output.  Only tests/ may import this module."""
import numpy as np


def lut(raw):
    """uint8 I,Q interleaved -> complex128 x = lut(I) + j lut(Q), lut(k) = (k - 127.4) / 127.6 (dsp.py:20-39)."""
    raw = np.asarray(raw, np.uint8).reshape(-1)
    return (raw[0::2].astype(np.float64) - 127.4) / 127.6 + 1j * ((raw[1::2].astype(np.float64) - 127.4) / 127.6)


def mod_taps(taps, shift_hz, fw):
    """g_c[k] = h[k] e^{+j 2 pi shift_c k / Fw}, complex128 [n_channels, T]; the phase through an exact integer remainder."""
    taps = np.asarray(taps, np.float64)
    k = np.arange(taps.size, dtype=np.int64)
    sh = np.asarray([int(s) % fw for s in shift_hz], np.int64)      # < 2^38; times k < 2^13: exact in int64
    return taps[None, :] * np.exp(2j * np.pi * ((sh[:, None] * k[None, :]) % fw).astype(np.float64) / fw)


def out_phasor(shift_hz, out_rate, n_out):
    """e^{-j 2 pi frac(shift_c t / Fo)}, complex128 [n_channels, n_out]; the phase through an exact integer remainder."""
    fo = int(out_rate)
    t = np.arange(n_out, dtype=np.int64)
    sh = np.asarray([int(s) % fo for s in shift_hz], np.int64)      # < 2^26; times t < 2^37: exact in int64
    return np.exp(-2j * np.pi * ((sh[:, None] * t[None, :]) % fo).astype(np.float64) / fo)


def channelize_z(raw, shift_hz, taps, decim, out_rate, gain, n_out=None):
    """The value in front of the quantiser, complex128 [n_channels, n_out]:
    Z = gain z 127.6 + 127.4 (1 + j), z_c[t] = sum_k h[k] x[D t - k] e^{-j 2 pi shift_c (D t - k) / Fw} (x[n<0] = 0),
    evaluated in the factorised form z_c[t] = e^{-j 2 pi frac(shift_c t / Fo)} sum_k g_c[k] x[D t - k] (equal to the
    definition in exact arithmetic; tests/test_channelizer.py checks the two against each other in float64)."""
    x = lut(raw)
    decim = int(decim)
    n_out = x.size // decim if n_out is None else int(n_out)
    z = filter_decimate(x, mod_taps(taps, shift_hz, int(out_rate) * decim), decim, n_out)
    z *= out_phasor(shift_hz, out_rate, n_out)
    return gain * z * 127.6 + 127.4 * (1 + 1j)


def filter_decimate(x, g, decim, n_out):
    """sum_k g_c[k] x[D t - k] (x[n<0] = 0) for t < n_out, complex128 [n_channels, n_out]; x complex [n], g [n_channels, T]."""
    g = np.asarray(g)
    T = g.shape[1]
    xpad = np.concatenate([np.zeros(T - 1, np.complex128), x])
    # window of output t: xpad[D t .. D t + T - 1] = x[D t - T + 1 .. D t], i.e. taps T-1 .. 0
    wins = np.lib.stride_tricks.sliding_window_view(xpad, T)[::decim][:n_out]
    grev = np.ascontiguousarray(g[:, ::-1].T)
    z = np.empty((g.shape[0], n_out), np.complex128)
    step = max(1, (1 << 22) // T)
    for a in range(0, n_out, step):
        z[:, a:a + step] = (np.ascontiguousarray(wins[a:a + step]) @ grev).T   # (a strided view would miss BLAS)
    return z


def quantise(Z):
    """clip(rint(Z), 0, 255) per component, uint8 [n_channels, 2 n_out] (I, Q interleaved)."""
    Z = np.asarray(Z)
    out = np.empty((Z.shape[0], 2 * Z.shape[1]), np.uint8)
    out[:, 0::2] = np.clip(np.rint(Z.real), 0, 255)
    out[:, 1::2] = np.clip(np.rint(Z.imag), 0, 255)
    return out


def channelize(raw, shift_hz, taps, decim, out_rate, gain, n_out=None):
    """raw: uint8 I,Q interleaved capture at decim*out_rate; returns uint8 [n_channels, 2*n_out]:
    out = clip(rint(Z), 0, 255) of channelize_z."""
    return quantise(channelize_z(raw, shift_hz, taps, decim, out_rate, gain, n_out))
