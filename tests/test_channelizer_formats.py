"""The wideband front end on signed captures (RD_IQ_S8, RD_IQ_S16; include/rtldavis_hip.h).  PARITY UNPINNED, as for
uint8: the reference has no channelizer.  CPU tests: the model of each format against the definition, the limits of
rd_chan_create_fmt at their edges, the derived bound (tests/chan_bound_fmt.py) and its teeth, the packets a weak 16-bit
capture carries.  GPU tests: the kernel against the model at that bound across the configuration space."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import chan_bound as CB
import chan_bound_fmt as CF
from rtldavis_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FO = 268800
FMT_CODE = {"u8": 0, "s8": 1, "s16": 2}
W = 0.01   # the weak capture: full scale x W, peak ~437 counts of int16


# ---------------------------------------------------------------- the cases
# name: decim per format, taps per format, shifts, gain, n_out, capture
SWEEP = {
    "weak51": ({"s8": 100, "s16": 100}, "default", "us", 3.0 / W, 3 * 8192, "weak"),
    "fullscale": ({"s8": 4, "s16": 4}, 256, [0, -2 * FO, FO + 4321], 0.8, 1024, "full"),     # reaches both ends of the range
    "odd_t255": ({"s8": 8, "s16": 8}, 255, [4 * FO, -123457, 300001, -2 * FO, 77777], 0.8, 129, "full"),
    "clip": ({"s8": 20, "s16": 20}, 64, [1000, -FO // 3, 2 * FO + 11], 1.5, 1024, "full"),
    "highpass": ({"s8": 16, "s16": 16}, 128, [0, 5 * FO + 1, -FO // 7], 0.8, 1024, "full"),
    "max_decim": ({"s8": 644, "s16": 160}, 8, [13, -80 * FO + 1], 0.8, 300, "full"),        # the LDS edge of each format
    "lds_long": ({"s8": 640, "s16": 156}, {"s8": 512, "s16": 656}, [78 * FO - 1, -3 * FO - 5], 0.8, 300, "full"),
    "t8192": ({"s8": 128, "s16": 96}, 8192, [7 * FO + 3, -1], 0.8, 512, "full"),             # the longest filter
    "g65": ({"s8": 100, "s16": 100}, 512, 65, 0.8, 512, "full"),
    "g4096": ({"s8": 100, "s16": 100}, 512, 4096, 0.8, 300, "full"),
}


def _weak_capture(fmt, n_out):
    from rtldavis_amd import channelizer as CZ
    off = [f - CZ.DEFAULT_CENTRE_HZ for f in CZ.US_CHANNELS_HZ]
    return synth.synth_wideband(range(300, 351), off, n_out, amplitude=0.12 * W, noise=0.02 * W, sample_format=fmt)


def _case(name, fmt):
    """(plan, taps, raw, n_out, info): plan carries decim, out_rate, gain, shift_hz, taps; every capture has a ragged
    tail of 37 samples."""
    from rtldavis_amd import channelizer as CZ
    decim, T, shifts, gain, n_out, kind = SWEEP[name]
    decim = decim[fmt]
    T = T[fmt] if isinstance(T, dict) else T
    seed = sum(map(ord, name))
    fw = decim * FO
    taps = CZ.design_taps() if T == "default" else CB.random_taps(T, seed, highpass=name == "highpass")
    info = None
    if shifts == "us":
        shifts = [f - CZ.DEFAULT_CENTRE_HZ + FO // 4 for f in CZ.US_CHANNELS_HZ]
    elif isinstance(shifts, int):
        shifts = np.random.default_rng(seed).integers(-fw // 2, fw // 2 + 1, shifts)
    if kind == "weak":
        raw, info = _weak_capture(fmt, n_out)
        raw = np.concatenate([raw, CF.capture_fmt(37, seed, fmt, level=W, ends=False)])
    else:
        raw = CF.capture_fmt(n_out * decim + 37, seed, fmt)
    plan = types.SimpleNamespace(decim=decim, out_rate=FO, gain=gain, shift_hz=np.asarray(shifts, np.int64),
                                 taps=np.asarray(taps, np.float64))
    return plan, plan.taps, raw, n_out, info


def _model(plan, raw, fmt, n_out):
    return CF.model_z(raw, fmt, plan.shift_hz, plan.taps, plan.decim, plan.out_rate, plan.gain, n_out)


def _model_of_x(plan, x, n_out):
    """The model on an arbitrary complex x[n] (for the wrong models)."""
    from oracle import channelizer_oracle as CHO
    z = CHO.filter_decimate(x, CHO.mod_taps(plan.taps, plan.shift_hz, plan.out_rate * plan.decim), plan.decim, n_out)
    z *= CHO.out_phasor(plan.shift_hz, plan.out_rate, n_out)
    return plan.gain * z * 127.6 + 127.4 * (1 + 1j)


# ---------------------------------------------------------------- CPU: the model against the definition
def _definition(x, shift_hz, taps, decim, out_rate, gain, n_out):
    """The header's definition as a plain double loop over outputs and taps (Python ints for the phase)."""
    fw = decim * out_rate
    Z = np.zeros((len(shift_hz), n_out), np.complex128)
    for c, sh in enumerate(shift_hz):
        for t in range(n_out):
            acc = 0j
            for k, h in enumerate(taps):
                n = decim * t - k
                if n >= 0:
                    acc += h * x[n] * np.exp(-2j * np.pi * ((int(sh) * n) % fw) / fw)
            Z[c, t] = gain * acc * 127.6 + 127.4 * (1 + 1j)
    return Z


@pytest.mark.parametrize("fmt", ["s8", "s16"])
@pytest.mark.parametrize("decim,T,n_wide", [(4, 5, 61), (4, 13, 64), (8, 3, 83), (8, 17, 130)])
def test_model_equals_the_definition(fmt, decim, T, n_wide):
    """model_z of a signed format against a naive double loop of the definition with x = I / FS + j Q / FS written out
    here, both ends of the range and a ragged length included."""
    fo = 1000
    fw = decim * fo
    taps = CB.random_taps(T, T)
    shifts = [0, 1, -1, 333, -fo - 17, fo, 3 * fo, fw // 2, -fw // 2, fw + 123, -5 * fw - 7, 10 ** 12 + 5]
    raw = CF.capture_fmt(n_wide, n_wide, fmt)
    lo, hi = (-128, 127) if fmt == "s8" else (-32768, 32767)
    pairs = raw.reshape(-1, 2)
    assert pairs.min() == lo and pairs.max() == hi and pairs.dtype == CF.DTYPE[fmt]
    fs = 128.0 if fmt == "s8" else 32768.0
    x = np.array([int(i) / fs + 1j * (int(q) / fs) for i, q in pairs])
    n_out = n_wide // decim
    want = _definition(x, shifts, taps, decim, fo, 1.7, n_out)
    got = CF.model_z(raw, fmt, shifts, taps, decim, fo, 1.7, n_out)
    assert got.shape == want.shape and np.abs(got - want).max() < 1e-9
    assert np.array_equal(CF.model_z(raw.reshape(-1, 2), fmt, shifts, taps, decim, fo, 1.7), got)   # n_out from the length


def test_u8_model_and_bound_are_the_existing_ones():
    from oracle import channelizer_oracle as CHO
    fo, decim = 1000, 4
    taps = CB.random_taps(13, 13)
    raw = CB.capture(64, 64, fo * decim)
    plan = types.SimpleNamespace(decim=decim, out_rate=fo, gain=1.7, shift_hz=np.asarray([0, 333, -1017]))
    Z = CHO.channelize_z(raw, plan.shift_hz, taps, decim, fo, 1.7)
    assert np.array_equal(CF.model_z(raw, "u8", plan.shift_hz, taps, decim, fo, 1.7), Z)
    assert np.array_equal(CF.error_bound_fmt(plan, taps, Z, raw, "u8"), CB.error_bound(plan, taps, Z, raw))


# ---------------------------------------------------------------- CPU: the C ABI - limits, sizes, symbols
def _create(fmt, decim, T, n_ch=1):
    """rd_chan_create_fmt through the C ABI (host work only, no device): ValueError past a limit."""
    from rtldavis_amd import _lib
    cfg = _lib.RdChanConfig(FO, decim, T, n_ch, 1.0)
    taps = np.ones(T, np.float64) / T
    shifts = np.zeros(n_ch, np.int64)
    h = C.c_void_p()
    _lib.check(_lib.lib().rd_chan_create_fmt(C.byref(cfg), fmt, taps.ctypes.data, shifts.ctypes.data, C.byref(h)))
    _lib.lib().rd_chan_destroy(h)


@pytest.mark.parametrize("fmt,ok,bad", [
    ("u8", (644, 8), (648, 8)),          # the 8-bit formats: 2 (127 D + t_pad + 8) + 16 <= 160 KiB
    ("s8", (644, 8), (648, 8)),
    ("s8", (640, 512), (644, 512)),
    ("u8", (4, 256), (4, 257)),          # ... and n_early = ceil((t_pad - 1) / D) <= 64
    ("s8", (4, 256), (4, 257)),
    ("s8", (8, 512), (8, 513)),
    ("s16", (160, 8), (164, 8)),         # int16 stages 8 bytes per sample: 8 (127 D + t_pad + 4) + 16 <= 160 KiB
    ("s16", (156, 656), (156, 657)),
    ("s16", (96, 8192), (100, 8192)),
    ("s16", (4, 8192), (4, 8193)),       # no n_early limit for int16 (no DC table); taps <= 8192
    ("s8", (128, 8192), (256, 8193)),
])
def test_create_fmt_limits_at_their_edges(fmt, ok, bad):
    _create(FMT_CODE[fmt], *ok)
    with pytest.raises(ValueError):
        _create(FMT_CODE[fmt], *bad)


def test_unknown_format_is_an_error():
    from rtldavis_amd import channelizer as CZ
    from rtldavis_amd import dsp, wideband
    for code in (-1, 3, 16):
        with pytest.raises(ValueError):
            _create(code, 100, 8)
    cfg = dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", 8192)
    for name in ("f32", "S16", None, 2):
        with pytest.raises(ValueError):
            CZ.Channelizer(sample_format=name)
        with pytest.raises(ValueError):
            wideband.WidebandReceiver(cfg, sample_format=name)
    # ... through the receiver's C constructor too
    from rtldavis_amd import _lib
    ccfg = _lib.RdChanConfig(FO, 100, 8, 1, 1.0)
    taps, sh, h = np.ones(8) / 8, np.zeros(1, np.int64), C.c_void_p()
    rc = _lib.lib().rd_wb_create_fmt(C.byref(dsp._cfg_struct(cfg)), C.byref(ccfg), 3, taps.ctypes.data, sh.ctypes.data, C.byref(h))
    assert rc == _lib.RD_ERR_ARG and not h


def test_new_entry_points_declared_exported_and_in_the_ctypes_table():
    from rtldavis_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtldavis_hip.h")).read(), flags=re.S)
    for n in ("rd_chan_create_fmt", "rd_wb_create_fmt"):
        assert re.search(r"\b" + n + r"\s*\(", src), n
        assert n in _lib.SIGNATURES and hasattr(_lib.lib(), n)
    assert (_lib.RD_IQ_U8, _lib.RD_IQ_S8, _lib.RD_IQ_S16) == (0, 1, 2)
    for name, val in (("RD_IQ_U8", 0), ("RD_IQ_S8", 1), ("RD_IQ_S16", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), src)


@pytest.mark.parametrize("fmt,itemsize", [("u8", 1), ("s8", 1), ("s16", 2)])
def test_sizes_follow_the_format(fmt, itemsize):
    """chunk_bytes / chunk_samples, and a byte count that is not a whole number of the format's IQ pairs or chunks
    is "Incompatible array sizes" - in Python and in the C ABI, before any device work."""
    from rtldavis_amd import _lib, dsp, wideband
    from rtldavis_amd import channelizer as CZ
    cfg = dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", 1024)
    w = wideband.WidebandReceiver(cfg, channels_hz=[914963100], sample_format=fmt)
    assert w.sample_format == fmt and w.dtype == CF.DTYPE[fmt]
    assert w.chunk_samples == 100 * 1024 and w.chunk_bytes == 2 * itemsize * w.chunk_samples
    for n in (2 * w.chunk_samples - 2, 2 * w.chunk_samples + 2, w.chunk_samples):
        with pytest.raises(ValueError, match="Incompatible array sizes"):
            w.submit(np.zeros(n, CF.DTYPE[fmt]))
        with pytest.raises(ValueError, match="Incompatible array sizes"):
            w.demodulate(np.zeros((n // 2, 2), CF.DTYPE[fmt]))
    buf = np.zeros(2 * w.chunk_samples + 8, CF.DTYPE[fmt])
    for nbytes in (w.chunk_bytes - 2 * itemsize, w.chunk_bytes + 2 * itemsize, w.chunk_bytes // 2):
        assert _lib.lib().rd_wideband_submit(w._h, buf.ctypes.data, nbytes) == _lib.RD_ERR_ARG
        assert "Incompatible array sizes" in _lib.last_error()
    cz = CZ.Channelizer([914963100], sample_format=fmt)
    assert cz.sample_format == fmt and cz.dtype == CF.DTYPE[fmt]
    with pytest.raises(ValueError, match="Incompatible array sizes"):
        cz.upload(np.zeros(7, CF.DTYPE[fmt]))
    assert _lib.lib().rd_chan_upload(cz._h, buf.ctypes.data, 2 * itemsize * 5 + itemsize) == _lib.RD_ERR_ARG
    assert "Incompatible array sizes" in _lib.last_error()


def test_no_silent_cast_into_a_signed_format():
    from rtldavis_amd import dsp, wideband
    from rtldavis_amd import channelizer as CZ
    cfg = dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", 128)
    for fmt in ("s8", "s16"):
        w = wideband.WidebandReceiver(cfg, channels_hz=[914963100], decim=4, taps=np.ones(8) / 8, sample_format=fmt)
        cz = CZ.Channelizer([914963100], sample_format=fmt)
        for bad in (np.zeros(w.chunk_samples, np.complex64), np.zeros(2 * w.chunk_samples, np.float32),
                    np.full(2 * w.chunk_samples, 40000, np.int32)):
            with pytest.raises(ValueError):
                w.submit(bad)
            with pytest.raises(ValueError):
                cz.upload(bad)


def test_synth_formats_come_from_one_signal():
    """The default output is the uint8 one (byte-identical to the explicit "u8"); the signed formats quantise the same
    complex signal: off the clip, each is within half a step of its own grid from the other's."""
    from rtldavis_amd import channelizer as CZ
    off = [CZ.US_CHANNELS_HZ[c] - CZ.DEFAULT_CENTRE_HZ for c in (0, 50)]
    u8, info = synth.synth_wideband([1, 2], off, 3 * 8192)
    u8b, _ = synth.synth_wideband([1, 2], off, 3 * 8192, sample_format="u8")
    assert u8.dtype == np.uint8 and np.array_equal(u8, u8b)
    s16, info16 = synth.synth_wideband([1, 2], off, 3 * 8192, sample_format="s16")
    s8, _ = synth.synth_wideband([1, 2], off, 3 * 8192, sample_format="s8")
    assert s16.dtype == np.int16 and s8.dtype == np.int8 and info16 == info and s16.size == u8.size == s8.size
    x16 = s16.astype(np.float64) / 32768
    assert np.abs(x16 - (u8.astype(np.float64) - 127.4) / 127.6).max() <= 0.5 / 127.6 + 0.5 / 32768 + 1e-12
    assert np.abs(x16 - s8.astype(np.float64) / 128).max() <= 0.5 / 128 + 0.5 / 32768 + 1e-12


# ---------------------------------------------------------------- CPU: the bound and its teeth
def test_exempt_share_of_the_weak_16_bit_capture():
    """The share of bytes the comparator lets differ by one step (Z within delta of a rounding boundary) on the weak
    default-plan capture: at most 10 % for int16.  It follows from the model and the derived bound alone.  (Signed
    digits keep the accumulator at signal size; offset-binary digits would carry 32768 sum g and exempt a third.)"""
    plan, taps, raw, n_out, _ = _case("weak51", "s16")
    assert np.abs(raw.astype(np.int32)).max() < 600       # a weak capture: ~437 counts
    Z = _model(plan, raw, "s16", n_out)
    delta = CF.error_bound_fmt(plan, taps, Z, raw, "s16")
    from oracle import channelizer_oracle as CHO
    s = CB.assert_matches_model(CHO.quantise(Z), Z, delta)
    print(f"\n[chan-fmt] weak51 s16: delta median {np.median(delta):.2e} max {delta.max():.2e}, exempt {s['exempt']:.2%}")
    assert s["exempt"] <= 0.10


def _wrong_models_s16(plan, raw, n_out, Z):
    """Models that are wrong the way an int16 kernel could plausibly be; each a uint8 [n_ch, 2 n_out]."""
    from oracle import channelizer_oracle as CHO
    s = raw.reshape(-1, 2).astype(np.int64)
    cx = lambda a: (a[:, 0] + 1j * a[:, 1]) / 32768.0
    sgn, mag = np.sign(s), np.abs(s)
    g = CHO.mod_taps(plan.taps, plan.shift_hz, plan.out_rate * plan.decim)
    G = plan.gain * 127.6 / 32768.0
    dc8 = -128.0 * (1 + 1j) * g.sum(1)[:, None] * CHO.out_phasor(plan.shift_hz, plan.out_rate, n_out)
    return {
        "hi and lo byte swapped": CHO.quantise(_model(plan, raw.byteswap(), "s16", n_out)),
        "hi digit unsigned": CHO.quantise(_model_of_x(plan, cx(np.where(s < 0, s + 65536, s)), n_out)),
        "lo digit dropped": CHO.quantise(_model_of_x(plan, cx(sgn * (mag & ~255)), n_out)),
        "the DC term of int8": CHO.quantise(Z + G * dc8),
        "I and Q swapped": CHO.quantise(_model_of_x(plan, cx(s[:, ::-1]), n_out)),
    }


TEETH = ["fullscale", "clip", "max_decim"]


@pytest.mark.parametrize("name", TEETH)
def test_comparator_rejects_wrong_int16_models(name):
    """Each wrong model fails assert_matches_model at this config's delta on bytes outside the delta band."""
    from oracle import channelizer_oracle as CHO
    plan, taps, raw, n_out, _ = _case(name, "s16")
    Z = _model(plan, raw, "s16", n_out)
    delta = CF.error_bound_fmt(plan, taps, Z, raw, "s16")
    assert CB.assert_matches_model(CHO.quantise(Z), Z, delta)["mismatches"] == 0
    for what, got in _wrong_models_s16(plan, raw, n_out, Z).items():
        s = CB.check_against_model(got, Z, delta)
        assert s["bad_lsb"] + s["bad_exact"] > 0, (name, what, s)
        with pytest.raises(AssertionError):
            CB.assert_matches_model(got, Z, delta)


def _capture_at_the_top_boundary(plan, raw, n_out):
    """raw with the window of channel 0's last output replaced by samples that put its real part just below the
    boundary 254.5 (imaginary part at mid-scale), half way between delta and the step a scale error of 2^-15 makes
    there.  Returns (capture, Z, delta)."""
    from oracle import channelizer_oracle as CHO
    D, T, fo = plan.decim, plan.taps.size, plan.out_rate
    G = plan.gain * 127.6 / 32768.0
    tt = n_out - 1
    gp = CHO.mod_taps(plan.taps, plan.shift_hz[:1], fo * D)[0] * CHO.out_phasor(plan.shift_hz[:1], fo, n_out)[0, tt]
    s = raw.copy().reshape(-1, 2)
    idx = D * tt - np.arange(T)
    rng = np.random.default_rng(5)
    target = 254.5 - 0.0037
    v = (target - 127.4) / G * np.conj(gp) / np.sum(np.abs(gp) ** 2)     # the matched window: sum g v = real
    v = np.clip(np.rint(v.real), -32767, 32767) + 1j * np.clip(np.rint(v.imag), -32767, 32767)
    basis = np.concatenate([gp.real, (1j * gp).real])                       # what +1 on I_k, on Q_k adds to the real part
    for _ in range(3):
        res = (target - 127.4) / G - np.sum(gp * v).real
        P = rng.integers(-3, 4, (200000, 2 * T))                            # small integer moves: a dense set of sums
        best = P[np.argmin(np.abs(P @ basis - res))]
        v = v + best[:T] + 1j * best[T:]
        s[idx, 0], s[idx, 1] = v.real, v.imag
        cap = s.reshape(-1).astype(np.int16)
        Z = _model(plan, cap, "s16", n_out)
        delta = CF.error_bound_fmt(plan, plan.taps, Z, cap, "s16")
        target = 254.5 - (delta[0, tt] + (Z[0, tt].real - 127.4) / 32767.0) / 2
    return cap, Z, delta


@pytest.mark.parametrize("decim", [160, 100, 4])
def test_comparator_rejects_a_full_scale_of_32767(decim):
    """x = s / 32767 instead of s / 32768 moves Z - 127.4 by 2^-15 of itself: at most 0.0039 steps, at the clip
    boundaries.  The bound cannot be below sqrt2 2^-16 |Z - 127.4 (1+j)| (the assumed accuracy of the hardware sine,
    chan_bound.SIN_ABS_ERR) = 0.0029 there, and the accumulation term grows with the filter (0.0023 more at 64 taps), so
    this wrong model can only be told apart where the filter is short and one component sits at a clip boundary with
    the other at mid-scale.  Hence its own three configs - 8 taps, the largest, the default and the smallest decimation -
    and a capture that puts one output there (as test_channelizer.py builds one for the dropped tap digit)."""
    from oracle import channelizer_oracle as CHO
    plan = types.SimpleNamespace(decim=decim, out_rate=FO, gain=0.8, shift_hz=np.asarray([13, -FO + 1], np.int64),
                                 taps=CB.random_taps(8, 1000 + decim))
    n_out = 64
    raw = CF.capture_fmt(n_out * decim + 37, decim, "s16", level=0.25)
    cap, Z, delta = _capture_at_the_top_boundary(plan, raw, n_out)
    assert CB.assert_matches_model(CHO.quantise(Z), Z, delta)["mismatches"] == 0
    got = CHO.quantise(127.4 * (1 + 1j) + (Z - 127.4 * (1 + 1j)) * (32768.0 / 32767.0))
    s = CB.check_against_model(got, Z, delta)
    assert s["bad_exact"] > 0, s
    with pytest.raises(AssertionError):
        CB.assert_matches_model(got, Z, delta)


@pytest.mark.parametrize("name", TEETH)
def test_comparator_rejects_wrong_int8_models(name):
    from oracle import channelizer_oracle as CHO
    plan, taps, raw, n_out, _ = _case(name, "s8")
    Z = _model(plan, raw, "s8", n_out)
    delta = CF.error_bound_fmt(plan, taps, Z, raw, "s8")
    assert CB.assert_matches_model(CHO.quantise(Z), Z, delta)["mismatches"] == 0
    s = raw.reshape(-1, 2).astype(np.int64)
    cx = lambda a, fs=128.0: (a[:, 0] + 1j * a[:, 1]) / fs
    wrong = {
        "read as uint8 with the uint8 look-up": CHO.channelize(raw.view(np.uint8), plan.shift_hz, taps, plan.decim, plan.out_rate, plan.gain, n_out),
        "bit 7 not flipped": CHO.quantise(_model_of_x(plan, cx(np.where(s < 0, s + 256, s) - 128), n_out)),
        "the DC term of uint8": CHO.quantise(_model_of_x(plan, cx(s + 0.6), n_out)),
        "/ 127.6": CHO.quantise(_model_of_x(plan, cx(s, 127.6), n_out)),
        "I and Q swapped": CHO.quantise(_model_of_x(plan, cx(s[:, ::-1]), n_out)),
    }
    for what, got in wrong.items():
        st = CB.check_against_model(got, Z, delta)
        assert st["bad_lsb"] + st["bad_exact"] > 0, (name, what, st)


# ---------------------------------------------------------------- CPU: the packets of a weak 16-bit capture
def test_weak_16_bit_capture_through_the_model_and_the_pinned_demodulator():
    """51 bursts at 1 % of full scale (peak ~437 counts), int16, gain 3 / w, default plan -> float64 model -> C oracle
    demodulator: 51 of 51 packets where they were injected.  (The same signal in uint8 gives 51 of 51 as well - the
    carriers dither each other -, so this is no claim that uint8 loses them: the case for int16 is the interface and
    the headroom.)"""
    from oracle import c_oracle as CO
    from oracle import channelizer_oracle as CHO
    plan, taps, raw, n_out, info = _case("weak51", "s16")
    nb = CHO.quantise(_model(plan, raw, "s16", n_out))
    assert 0 < nb.min() and nb.max() < 255                # no clipping
    res, _ = CO.demod_batch(nb, CO.make_cfg(), threads=4)
    found = 0
    for (payload, start), pk in zip(info, res):
        hits = [(p.call, p.index) for p in pk if bytes(p.data).hex() == payload]
        if hits:
            pos = (hits[0][0] - 1) * 8192 + hits[0][1]
            found += 0 <= pos - (start + 32 * 14) <= 30
    assert found == 51


# ---------------------------------------------------------------- GPU: the kernel across the sweep
def _channelizer(plan, fmt):
    from rtldavis_amd import channelizer as CZ
    return CZ.Channelizer(plan.shift_hz, centre_hz=0, decim=plan.decim, taps=plan.taps, gain=plan.gain,
                          out_rate=plan.out_rate, if_hz=0, sample_format=fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["s8", "s16"])
@pytest.mark.parametrize("name", list(SWEEP))
def test_kernel_within_the_bound_across_configs(name, fmt):
    """Channelizer.run_host against model_z with assert_matches_model at delta = error_bound_fmt; prints delta, the
    exempt share, the mismatches and the largest boundary distance among them (the room the bound leaves).  The first
    outputs of every capture see the zero history; every capture has a ragged tail."""
    from oracle import channelizer_oracle as CHO
    plan, taps, raw, n_out, _ = _case(name, fmt)
    cz = _channelizer(plan, fmt)
    assert np.array_equal(cz.shift_hz, plan.shift_hz)
    cz.upload(raw.reshape(-1, 2) if name == "clip" else raw)
    got = cz.run_host(n_out)
    Z = _model(plan, raw, fmt, n_out)
    delta = CF.error_bound_fmt(plan, taps, Z, raw, fmt)
    s = CB.check_against_model(got, Z, delta)
    print(f"\n[chan-fmt-sweep] {name} {fmt}: delta median {np.median(delta):.2e} max {s['delta_max']:.2e}, exempt "
          f"{s['exempt']:.2%}, mismatches {s['mismatches']}/{got.size}, bad {s['bad_lsb']}+{s['bad_exact']}, worst distance "
          f"{s['worst_dist']:.2e} ({s['worst_ratio']:.2f} of delta)")
    CB.assert_matches_model(got, Z, delta)
    if name == "weak51" and fmt == "s16":
        assert s["exempt"] <= 0.10
    if name == "fullscale":
        v = raw.astype(np.int32)
        assert v.min() == np.iinfo(raw.dtype).min and v.max() == np.iinfo(raw.dtype).max
    if name == "clip":
        q = CHO.quantise(Z)
        assert 0.01 <= (q == 0).mean() <= 0.10 and 0.01 <= (q == 255).mean() <= 0.10
    if name == "highpass":
        assert abs(taps.sum()) < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["s8", "s16"])
def test_strided_destination_leaves_the_gaps_alone(fmt):
    """rd_chan_run into device memory with dst_stream_stride > 2 n_out (n_out not a multiple of 128): channel c's bytes
    at c * stride equal run_host's, and every byte in the gaps and after n_out keeps its sentinel."""
    from rtldavis_amd import _lib
    plan, taps, raw, _, _ = _case("odd_t255", fmt)
    n_out, stride, n_ch = 129, 2 * 129 + 70, plan.shift_hz.size
    cz = _channelizer(plan, fmt)
    cz.upload(raw)
    want = cz.run_host(n_out)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    size = n_ch * stride
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), size) == 0
    try:
        assert hip.hipMemset(dev, 0xA5, size) == 0
        _lib.check(_lib.lib().rd_chan_run(cz._h, n_out, dev, stride, None))
        host = np.empty(size, np.uint8)
        assert hip.hipMemcpy(host.ctypes.data, dev, size, 2) == 0     # hipMemcpyDeviceToHost, after the null stream
    finally:
        hip.hipFree(dev)
    host = host.reshape(n_ch, stride)
    assert np.array_equal(host[:, : 2 * n_out], want)
    assert (host[:, 2 * n_out:] == 0xA5).all()


@pytest.mark.gpu
def test_uint8_is_unchanged_by_the_format_argument():
    """Channelizer() and Channelizer(sample_format="u8") give identical bytes on the default-plan capture (which the
    existing suite pins to the model)."""
    from rtldavis_amd import channelizer as CZ
    off = [f - CZ.DEFAULT_CENTRE_HZ for f in CZ.US_CHANNELS_HZ]
    raw, _ = synth.synth_wideband(range(300, 351), off, 3 * 8192, amplitude=0.05)
    a, b = CZ.Channelizer(), CZ.Channelizer(sample_format="u8")
    a.upload(raw)
    b.upload(raw)
    assert np.array_equal(a.run_host(), b.run_host())
