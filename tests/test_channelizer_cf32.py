"""The wideband front end on float32 captures (RD_IQ_CF32, sample_format="cf32"; include/rtldavis_hip.h).  PARITY
UNPINNED, as for the other formats: the reference has no channelizer.  CPU tests: the model against the definition, the
digit split the kernel stages, the limits of rd_chan_create_fmt at their edges, sizes and the no-silent-cast rule, the
derived bound (tests/chan_bound_cf32.py), its teeth and the share of bytes it exempts on the weak default-plan capture.
GPU tests: the kernel against the model at that bound across the configuration space."""
import ctypes as C
import functools
import os
import re
import types

import numpy as np
import pytest

import chan_bound as CB
import chan_bound_cf32 as CC
import chan_bound_fmt as CF
from rtldavis_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FO = 268800
W = 0.01   # the weak capture: 1 % of full scale

# name: decim, taps, shifts (a list, a count of random ones, "us"), gain, n_out, capture
SWEEP = {
    "fullscale": (4, 256, [0, -2 * FO, FO + 4321], 0.8, 1024, "full"),
    "odd_t255": (8, 255, [4 * FO, -123457, 300001, -2 * FO, 77777], 0.8, 129, "full"),
    "clip": (20, 64, [1000, -FO // 3, 2 * FO + 11], 1.5, 1024, "full"),
    "max_decim": (160, 8, [13, -80 * FO + 1], 0.8, 300, "full"),           # the LDS edge at 8 taps
    "lds_long": (156, 656, [78 * FO - 1, -3 * FO - 5], 0.8, 300, "full"),  # the LDS edge with a long filter
    "t8192": (96, 8192, [7 * FO + 3, -1], 0.8, 512, "full"),               # the longest filter
    "g65": (100, 512, 65, 0.8, 512, "full"),                               # a second channel group
    "weak51": (100, "default", "us", 3.0 / W, 3 * 8192, "weak"),
}


def _weak_capture(n_out):
    from rtldavis_amd import channelizer as CZ
    off = [f - CZ.DEFAULT_CENTRE_HZ for f in CZ.US_CHANNELS_HZ]
    return synth.synth_wideband(range(300, 351), off, n_out, amplitude=0.12 * W, noise=0.02 * W, sample_format="cf32")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(plan, raw, n_out, info): plan carries decim, out_rate, gain, shift_hz, taps; every capture has a ragged tail of
    37 samples and the special values planted."""
    from rtldavis_amd import channelizer as CZ
    decim, T, shifts, gain, n_out, kind = SWEEP[name]
    seed = sum(map(ord, name))
    fw = decim * FO
    taps = CZ.design_taps() if T == "default" else CB.random_taps(T, seed)
    info = None
    if shifts == "us":
        shifts = [f - CZ.DEFAULT_CENTRE_HZ + FO // 4 for f in CZ.US_CHANNELS_HZ]
    elif isinstance(shifts, int):
        shifts = np.random.default_rng(seed).integers(-fw // 2, fw // 2 + 1, shifts)
    if kind == "weak":
        raw, info = _weak_capture(n_out)
        raw = np.concatenate([raw, CC.capture_cf32(37, seed, level=W, specials=False)])
        CC.plant_specials(raw.reshape(-1, 2))
    else:
        raw = CC.capture_cf32(n_out * decim + 37, seed)
    raw.setflags(write=False)
    plan = types.SimpleNamespace(decim=decim, out_rate=FO, gain=gain, shift_hz=np.asarray(shifts, np.int64),
                                 taps=np.asarray(taps, np.float64))
    return plan, raw, n_out, info


def _model(plan, raw, n_out):
    return CC.model_z_cf32(raw, plan.shift_hz, plan.taps, plan.decim, plan.out_rate, plan.gain, n_out)


def _model_of_x(plan, x, n_out):
    return CC.model_of_x(x, plan.shift_hz, plan.taps, plan.decim, plan.out_rate, plan.gain, n_out)


@functools.lru_cache(maxsize=None)
def _model_and_bound(name):
    """(Z, delta) of a sweep case, computed once and shared (read-only)."""
    plan, raw, n_out, _ = _case(name)
    Z = _model(plan, raw, n_out)
    delta = CC.error_bound_cf32(plan, plan.taps, Z, raw)
    Z.setflags(write=False)
    delta.setflags(write=False)
    return Z, delta


# ---------------------------------------------------------------- CPU 1: the model against the definition
@pytest.mark.parametrize("decim,T,n_wide", [(4, 5, 61), (4, 13, 64), (8, 3, 83), (8, 17, 130)])
def test_model_equals_the_definition(decim, T, n_wide):
    """model_z_cf32 against a naive double loop of the definition, with adm written out here: NaN -> 0, clamp to
    [-8, 8]; the special values are in the capture."""
    fo = 1000
    fw = decim * fo
    taps = CB.random_taps(T, T)
    shifts = [0, 1, -1, 333, -fo - 17, fo, 3 * fo, fw // 2, -fw // 2, fw + 123, -5 * fw - 7, 10 ** 12 + 5]
    raw = CC.capture_cf32(n_wide, n_wide)
    assert raw.dtype == np.float32 and raw.size == 2 * n_wide
    assert np.isnan(raw).sum() == 1 and np.isinf(raw).sum() == 2 and (raw == np.float32(9.5)).sum() == 1

    def admit(v):
        v = float(v)
        if v != v:
            return 0.0
        return min(max(v, -8.0), 8.0)

    x = np.array([admit(i) + 1j * admit(q) for i, q in raw.reshape(-1, 2)])
    assert np.abs(x.real).max() == 8.0 and np.isfinite(x).all()
    n_out = n_wide // decim
    want = np.zeros((len(shifts), n_out), np.complex128)
    for c, sh in enumerate(shifts):
        for t in range(n_out):
            acc = 0j
            for k, h in enumerate(taps):
                n = decim * t - k
                if n >= 0:
                    acc += h * x[n] * np.exp(-2j * np.pi * ((int(sh) * n) % fw) / fw)
            want[c, t] = 1.7 * acc * 127.6 + 127.4 * (1 + 1j)
    got = CC.model_z_cf32(raw, shifts, taps, decim, fo, 1.7, n_out)
    assert got.shape == want.shape and np.abs(got - want).max() < 1e-9
    assert np.array_equal(CC.model_z_cf32(raw.reshape(-1, 2), shifts, taps, decim, fo, 1.7), got)   # n_out from the length
    assert np.array_equal(CC.model_z_cf32(raw.view(np.complex64), shifts, taps, decim, fo, 1.7), got)


# ---------------------------------------------------------------- CPU 2: the digit split
def test_digit_split_is_exact_to_the_stated_bound():
    """hi = f16(s), lo = f16(s - hi) of s = 2^12 adm(v) by numpy's float16 conversion (round to nearest even, subnormals
    kept - what the kernel's conversion does in the default float mode): |s - hi - lo| <= max(2^-22 |s|, 2^-25), i.e.
    max(2^-22 |x|, 2^-37) in the capture's units; hi, lo and their products with 11-bit taps are exact in float32."""
    rng = np.random.default_rng(7)
    n = 10 ** 6
    v = (rng.choice([-1.0, 1.0], n) * (1 + rng.random(n)) * 2.0 ** rng.uniform(-44, 4, n)).astype(np.float32)
    v = np.concatenate([v, CC.SPECIALS, -CC.SPECIALS, np.float32([8.0, -8.0, 2.0 ** -14, 2.0 ** -26, 2.0 ** -37])])
    x = CC.adm(v)
    s32 = x.astype(np.float32) * np.float32(2.0 ** CC.PRESCALE_LOG2)
    s = s32.astype(np.float64)
    normal = np.abs(x) >= 2.0 ** -126
    assert np.array_equal(s[normal], x[normal] * 4096.0)                   # the pre-scale is exact
    hi, lo = CC.split_f16(s32)
    hi64, lo64 = hi.astype(np.float64), lo.astype(np.float64)
    assert np.isfinite(hi64).all() and np.abs(hi64).max() == 32768.0
    assert np.array_equal((s32 - hi.astype(np.float32)).astype(np.float64), s - hi64)   # s - hi is exact in fp32
    err = np.abs(s - hi64 - lo64)
    assert (err <= np.maximum(2.0 ** -22 * np.abs(s), 2.0 ** -25)).all()
    assert (err[normal] * 2.0 ** -12 <= np.maximum(2.0 ** -22 * np.abs(x[normal]), 2.0 ** -37)).all()
    assert (np.abs(lo64) <= 2.0 ** -10 * np.abs(hi64) + 2.0 ** -25).all()
    assert ((lo64 != 0) & (np.abs(lo64) < 2.0 ** -14)).any()               # subnormal low digits occur
    # 11-bit taps as the A operand holds them: normal f16 up to 2^15 and subnormal low terms m 2^-24
    taps = np.concatenate([rng.integers(1024, 2048, 500) * 2.0 ** rng.integers(-24, 5, 500), rng.integers(1, 1024, 500) * 2.0 ** -24])
    taps = (taps * rng.choice([-1.0, 1.0], taps.size)).astype(np.float16)
    t32, t64 = taps.astype(np.float32), taps.astype(np.float64)
    assert np.array_equal(t64, t32.astype(np.float64))
    for d in (hi[:: 997], lo[:: 997]):
        p32 = d.astype(np.float32)[:, None] * t32[None, :]
        p64 = d.astype(np.float64)[:, None] * t64[None, :]
        assert np.array_equal(p32.astype(np.float64), p64)
        nz = p64 != 0
        assert np.abs(p64[nz]).min() >= 2.0 ** -48 and np.abs(p64).max() <= 2.0 ** 31


# ---------------------------------------------------------------- CPU 3-5: the C ABI - limits, sizes, symbols
def _create(fmt, decim, T, n_ch=1):
    from rtldavis_amd import _lib
    cfg = _lib.RdChanConfig(FO, decim, T, n_ch, 1.0)
    taps = np.ones(T, np.float64) / T
    shifts = np.zeros(n_ch, np.int64)
    h = C.c_void_p()
    _lib.check(_lib.lib().rd_chan_create_fmt(C.byref(cfg), fmt, taps.ctypes.data, shifts.ctypes.data, C.byref(h)))
    _lib.lib().rd_chan_destroy(h)


@pytest.mark.parametrize("ok,bad", [
    ((160, 8), (164, 8)),            # 8 bytes per staged sample: 8 (127 D + t_pad + 4) + 16 <= 160 KiB
    ((156, 656), (156, 657)),
    ((96, 8192), (100, 8192)),
    ((4, 8192), (4, 8193)),          # no n_early limit (no DC table); taps <= 8192
])
def test_create_limits_at_their_edges(ok, bad):
    _create(4, *ok)
    with pytest.raises(ValueError):
        _create(4, *bad)
    _create(4, 100, 512, 4096)
    with pytest.raises(ValueError):
        _create(4, 100, 512, 4097)


def test_sizes_and_no_silent_cast():
    """chunk_bytes = 8 chunk_samples; a byte count that is no whole number of 8-byte IQ pairs, or of chunks, is
    "Incompatible array sizes" in Python and in the C ABI, before any device work; complex128, float64 and integers are
    a ValueError, complex64 and float32 (flat, [n, 2]) pass the argument check."""
    from rtldavis_amd import _lib, dsp, wideband
    from rtldavis_amd import channelizer as CZ
    cfg = dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", 1024)
    w = wideband.WidebandReceiver(cfg, channels_hz=[914963100], sample_format="cf32")
    assert w.sample_format == "cf32" and w.dtype == np.float32
    assert w.chunk_samples == 100 * 1024 and w.chunk_bytes == 8 * w.chunk_samples
    for n in (2 * w.chunk_samples - 2, 2 * w.chunk_samples + 2, w.chunk_samples):
        with pytest.raises(ValueError, match="Incompatible array sizes"):
            w.submit(np.zeros(n, np.float32))
        with pytest.raises(ValueError, match="Incompatible array sizes"):
            w.demodulate(np.zeros((n // 2, 2), np.float32))
        with pytest.raises(ValueError, match="Incompatible array sizes"):
            w.submit(np.zeros(n // 2, np.complex64))
    buf = np.zeros(2 * w.chunk_samples + 8, np.float32)
    for nbytes in (w.chunk_bytes - 8, w.chunk_bytes + 8, w.chunk_bytes // 2):
        assert _lib.lib().rd_wideband_submit(w._h, buf.ctypes.data, nbytes) == _lib.RD_ERR_ARG
        assert "Incompatible array sizes" in _lib.last_error()
    cz = CZ.Channelizer([914963100], sample_format="cf32")
    assert cz.sample_format == "cf32" and cz.dtype == np.float32
    with pytest.raises(ValueError, match="Incompatible array sizes"):
        cz.upload(np.zeros(7, np.float32))
    for nbytes in (8 * 5 + 4, 8 * 5 + 1):
        assert _lib.lib().rd_chan_upload(cz._h, buf.ctypes.data, nbytes) == _lib.RD_ERR_ARG
        assert "Incompatible array sizes" in _lib.last_error()
    n = w.chunk_samples
    for bad in (np.zeros(n, np.complex128), np.zeros(2 * n, np.float64), np.zeros(2 * n, np.int16),
                np.zeros((n, 2), np.float64), np.zeros((2, n), np.complex64), np.zeros((n, 2, 1), np.float32)):
        with pytest.raises(ValueError):
            w.submit(bad)
        with pytest.raises(ValueError):
            cz.upload(bad)
        with pytest.raises(ValueError):
            _lib.iq_array(bad, np.float32)
    # what is accepted, through the argument check alone (no device work): a view, never a cast
    c64 = (np.arange(6) + 1j * np.arange(6, 12)).astype(np.complex64)
    a = _lib.iq_array(c64, np.float32)
    assert a.dtype == np.float32 and np.shares_memory(a, c64) and np.array_equal(a, [0, 6, 1, 7, 2, 8, 3, 9, 4, 10, 5, 11])
    f = np.arange(12, dtype=np.float32)
    assert np.shares_memory(_lib.iq_array(f, np.float32), f) and np.array_equal(_lib.iq_array(f.reshape(-1, 2), np.float32), f)
    assert np.array_equal(_lib.iq_array(f.reshape(-1, 2)[::2], np.float32), [0, 1, 4, 5, 8, 9])    # a strided [n, 2]
    assert w._check_chunk(np.zeros(n, np.complex64)).nbytes == w.chunk_bytes


def test_constant_declared_exported_and_in_the_ctypes_table():
    from rtldavis_amd import _lib
    text = open(os.path.join(ROOT, "include", "rtldavis_hip.h")).read()
    assert re.search(r"#define\s+RD_IQ_CF32\s+4\b", text)
    assert "unassigned" in text and '"f32"' in text          # the header says what 3 and "f32" are
    assert _lib.RD_IQ_CF32 == 4 and _lib.SAMPLE_FORMATS["cf32"] == (4, np.float32)
    assert _lib.sample_format("cf32") == (4, np.float32)
    assert "f32" not in _lib.SAMPLE_FORMATS and 3 not in [c for c, _ in _lib.SAMPLE_FORMATS.values()]
    for n in ("rd_chan_create_fmt", "rd_wb_create_fmt"):
        assert hasattr(_lib.lib(), n)
    _create(4, 100, 512, 51)                                 # the exported constructor takes the code


def test_synth_cf32_is_the_same_signal():
    from rtldavis_amd import channelizer as CZ
    off = [CZ.US_CHANNELS_HZ[c] - CZ.DEFAULT_CENTRE_HZ for c in (0, 50)]
    f32, info = synth.synth_wideband([1, 2], off, 3 * 8192, sample_format="cf32")
    s16, info16 = synth.synth_wideband([1, 2], off, 3 * 8192, sample_format="s16")
    assert f32.dtype == np.float32 and f32.size == s16.size and info == info16
    assert np.abs(f32.astype(np.float64) - s16.astype(np.float64) / 32768).max() <= 0.5 / 32768 + 2.0 ** -25


# ---------------------------------------------------------------- CPU 6: the bound's teeth
def _capture_at_the_top_boundary(plan, raw, n_out):
    """raw with the window of channel 0's last output replaced: zeros but for the five samples under taps 0 .. 4 (the
    last two K steps, so that the accumulation term stays small whatever the filter's length), which put its real part
    just below the boundary 254.5 with the imaginary part at mid-scale - half way between delta and the step a scale
    error of 1/32767 makes there.  Floats need no search: the window is solved for.  Returns (capture, Z, delta)."""
    from oracle import channelizer_oracle as CHO
    D, T, fo = plan.decim, plan.taps.size, plan.out_rate
    G = plan.gain * 127.6
    tt = n_out - 1
    gp = CHO.mod_taps(plan.taps, plan.shift_hz[:1], fo * D)[0] * CHO.out_phasor(plan.shift_hz[:1], fo, n_out)[0, tt]
    s = raw.copy().reshape(-1, 2)
    s[D * tt - T + 1:] = 0
    use = np.arange(min(5, T))
    idx = D * tt - use
    step = (254.5 - 127.4) / 32767.0
    aim = 254.5 - 0.0034
    for _ in range(4):
        v = np.conj(gp[use]) / np.abs(gp[use]) * ((aim - 127.4) / G / np.abs(gp[use]).sum())   # sum g v is real
        assert np.abs(v.real).max() < 8 and np.abs(v.imag).max() < 8
        s[idx, 0], s[idx, 1] = v.real, v.imag
        cap = s.reshape(-1)
        Z = _model(plan, cap, n_out)
        delta = CC.error_bound_cf32(plan, plan.taps, Z, cap)
        aim += 254.5 - (delta[0, tt] + step) / 2 - Z[0, tt].real     # (the samples are float32: correct what that leaves)
    assert abs(Z[0, tt].imag - 127.4) < 1e-3
    return cap, Z, delta


def _wrong_models(plan, raw, n_out):
    """Models that are wrong the way a float32 kernel could plausibly be, on the case's own capture."""
    from oracle import channelizer_oracle as CHO
    v = raw.reshape(-1, 2)
    x = CC.to_complex(raw)
    f16 = lambda a: a.astype(np.float32).astype(np.float16).astype(np.float64)
    wide = v.astype(np.float64)
    no_clamp = np.where(np.isfinite(wide), wide, np.nan_to_num(np.clip(wide, -8, 8), nan=0.0))   # 9.5 passed through
    nan_one = np.where(np.isnan(wide), 1.0, np.clip(np.nan_to_num(wide, nan=0.0), -8, 8))
    return {
        "lo digit dropped": CHO.quantise(_model_of_x(plan, f16(x.real) + 1j * f16(x.imag), n_out)),
        "I and Q swapped": CHO.quantise(_model_of_x(plan, x.imag + 1j * x.real, n_out)),
        "no clamp": CHO.quantise(_model_of_x(plan, no_clamp[:, 0] + 1j * no_clamp[:, 1], n_out)),
        "NaN treated as 1.0": CHO.quantise(_model_of_x(plan, nan_one[:, 0] + 1j * nan_one[:, 1], n_out)),
    }


@pytest.mark.parametrize("name", ["fullscale", "max_decim"])
def test_comparator_rejects_wrong_float_models(name):
    """Each wrong model fails the comparator at this config's delta on bytes outside the delta band."""
    from oracle import channelizer_oracle as CHO
    plan, raw, n_out, _ = _case(name)
    Z, delta = _model_and_bound(name)
    assert CB.assert_matches_model(CHO.quantise(Z), Z, delta)["mismatches"] == 0
    for what, got in _wrong_models(plan, raw, n_out).items():
        s = CB.check_against_model(got, Z, delta)
        assert s["bad_lsb"] + s["bad_exact"] > 0, (name, what, s)
        with pytest.raises(AssertionError):
            CB.assert_matches_model(got, Z, delta)


@pytest.mark.parametrize("name", ["fullscale", "max_decim"])
def test_comparator_rejects_a_scale_of_32768_over_32767(name):
    """A kernel that took the floats for int16 / 32767 scaled to / 32768 moves Z - 127.4 by 2^-15 of itself: 0.0039
    steps at a clip boundary, where the bound cannot be below sqrt2 2^-16 |Z - 127.4 (1+j)| = 0.0029 (the assumed
    accuracy of the hardware sine).  So the capture puts one output there, with a window that keeps the accumulation
    term small (_capture_at_the_top_boundary)."""
    from oracle import channelizer_oracle as CHO
    plan, raw, n_out, _ = _case(name)
    cap, Z, delta = _capture_at_the_top_boundary(plan, raw, n_out)
    tt = n_out - 1
    assert delta[0, tt] < 254.5 - Z[0, tt].real < (254.5 - 127.4) / 32767.0
    assert CB.assert_matches_model(CHO.quantise(Z), Z, delta)["mismatches"] == 0
    got = CHO.quantise(127.4 * (1 + 1j) + (Z - 127.4 * (1 + 1j)) * (32768.0 / 32767.0))
    s = CB.check_against_model(got, Z, delta)
    assert s["bad_exact"] > 0, s
    with pytest.raises(AssertionError):
        CB.assert_matches_model(got, Z, delta)


# ---------------------------------------------------------------- CPU 7: the exempt share and the packets
def test_exempt_share_and_packets_of_the_weak_float_capture():
    """The weak default-plan capture (1 % of full scale, gain 300) as floats: the share of bytes the bound lets differ
    by one step is at most 10 % - the cap of the int16 test, a condition on the bound, from the model alone - and the
    model's bytes carry 51 of 51 packets through the pinned demodulator."""
    from oracle import c_oracle as CO
    from oracle import channelizer_oracle as CHO
    plan, raw, n_out, info = _case("weak51")
    body = raw.reshape(-1, 2).copy()
    for sites in CC.special_sites(body.shape[0]):
        for n, comp in sites:
            body[n, comp] = 0
    assert np.abs(body).max() < 600 / 32768                 # a weak capture but for the planted values
    Z, delta = _model_and_bound("weak51")
    nb = CHO.quantise(Z)
    s = CB.assert_matches_model(nb, Z, delta)
    print(f"\n[chan-cf32] weak51: delta median {np.median(delta):.2e} max {delta.max():.2e}, exempt {s['exempt']:.2%}")
    assert s["exempt"] <= 0.10
    res, _ = CO.demod_batch(nb, CO.make_cfg(), threads=4)
    found = 0
    for (payload, start), pk in zip(info, res):
        hits = [(p.call, p.index) for p in pk if bytes(p.data).hex() == payload]
        if hits:
            pos = (hits[0][0] - 1) * 8192 + hits[0][1]
            found += 0 <= pos - (start + 32 * 14) <= 30
    assert found == 51


# ---------------------------------------------------------------- GPU 8: the kernel across the sweep
def _channelizer(plan, fmt="cf32"):
    from rtldavis_amd import channelizer as CZ
    return CZ.Channelizer(plan.shift_hz, centre_hz=0, decim=plan.decim, taps=plan.taps, gain=plan.gain,
                          out_rate=plan.out_rate, if_hz=0, sample_format=fmt)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SWEEP))
def test_kernel_within_the_bound_across_configs(name):
    """Channelizer.run_host against model_z_cf32 with assert_matches_model at delta = error_bound_cf32; prints delta, the
    exempt share, the mismatches and the largest boundary distance among them.  Every capture has the special values in
    front (the first outputs also see the zero history) and a ragged tail."""
    from oracle import channelizer_oracle as CHO
    plan, raw, n_out, _ = _case(name)
    cz = _channelizer(plan)
    assert np.array_equal(cz.shift_hz, plan.shift_hz)
    cz.upload(raw.view(np.complex64) if name == "clip" else raw.reshape(-1, 2) if name == "g65" else raw)
    got = cz.run_host(n_out)
    Z, delta = _model_and_bound(name)
    s = CB.check_against_model(got, Z, delta)
    print(f"\n[chan-cf32-sweep] {name}: delta median {np.median(delta):.2e} max {s['delta_max']:.2e}, exempt "
          f"{s['exempt']:.2%}, mismatches {s['mismatches']}/{got.size}, bad {s['bad_lsb']}+{s['bad_exact']}, worst distance "
          f"{s['worst_dist']:.2e} ({s['worst_ratio']:.2f} of delta)")
    CB.assert_matches_model(got, Z, delta)
    assert np.isnan(raw).any() and np.isinf(raw).any()
    if name == "weak51":
        assert s["exempt"] <= 0.10
    if name == "clip":
        q = CHO.quantise(Z)
        assert 0.01 <= (q == 0).mean() <= 0.10 and 0.01 <= (q == 255).mean() <= 0.10


# ---------------------------------------------------------------- GPU 9: one model, two formats
@pytest.mark.gpu
def test_one_model_two_formats():
    """An int16 capture s and the float32 capture s / 32768 (exact) have one model; each kernel's bytes satisfy its own
    bound against it."""
    plan, _, n_out, _ = _case("odd_t255")
    s16 = CF.capture_fmt(n_out * plan.decim + 37, 11, "s16")
    f32 = (s16.astype(np.float32) / np.float32(32768.0))
    assert np.array_equal(f32.astype(np.float64) * 32768.0, s16.astype(np.float64))
    Z = CF.model_z(s16, "s16", plan.shift_hz, plan.taps, plan.decim, plan.out_rate, plan.gain, n_out)
    assert np.array_equal(_model(plan, f32, n_out), Z)
    for fmt, raw, delta in (("s16", s16, CF.error_bound_fmt(plan, plan.taps, Z, s16, "s16")),
                            ("cf32", f32, CC.error_bound_cf32(plan, plan.taps, Z, f32))):
        cz = _channelizer(plan, fmt)
        cz.upload(raw)
        s = CB.assert_matches_model(cz.run_host(n_out), Z, delta)
        print(f"\n[chan-cf32-two] {fmt}: delta max {s['delta_max']:.2e}, exempt {s['exempt']:.2%}, mismatches {s['mismatches']}")


# ---------------------------------------------------------------- GPU 10: a strided destination
@pytest.mark.gpu
def test_strided_destination_leaves_the_gaps_alone():
    from rtldavis_amd import _lib
    plan, raw, _, _ = _case("odd_t255")
    n_out, stride, n_ch = 129, 2 * 129 + 70, plan.shift_hz.size
    cz = _channelizer(plan)
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


# ---------------------------------------------------------------- GPU 11: the formats do not share state
@pytest.mark.gpu
def test_uint8_bytes_do_not_change_beside_a_float_channelizer():
    """The "u8" bytes of a small capture before and after a cf32 channelizer of the same plan was constructed and run in
    the same process: tables and handles are per instance."""
    plan, raw, n_out, _ = _case("odd_t255")
    u8 = CB.capture(n_out * plan.decim + 37, 3, plan.decim * FO)
    a = _channelizer(plan, "u8")
    a.upload(u8)
    before = a.run_host(n_out)
    f = _channelizer(plan)
    f.upload(raw)
    f.run_host(n_out)
    again = a.run_host(n_out)
    b = _channelizer(plan, "u8")
    b.upload(u8)
    assert np.array_equal(before, again) and np.array_equal(before, b.run_host(n_out))
