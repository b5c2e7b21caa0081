"""Wideband front end.  PARITY UNPINNED: rtldavis has no channelizer, so the
oracle here (oracle/channelizer_oracle.py) is this repo's own float64 restatement; what ties it to
the reference is that the reference-pinned demodulator recovers the injected packets from its
output.  CPU tests cover the definition and the tap design, GPU tests the HIP kernel against it."""
import os

import numpy as np
import pytest

from rtldavis_amd import synth


def _cz():
    from rtldavis_amd import channelizer
    return channelizer


def test_tap_design_passes_the_channel_and_stops_the_neighbours():
    CZ = _cz()
    h = CZ.design_taps()
    assert h.size == 512 and abs(h.sum() - 1.0) < 1e-12 and np.allclose(h, h[::-1])
    fw = CZ.OUT_RATE * CZ.DEFAULT_DECIM
    f = np.array([0.0, 67.2e3 + 15e3, 501750.0 - 67.2e3 - 20e3, 501750.0 + 67.2e3 + 20e3])
    H = np.abs(np.exp(-2j * np.pi * np.outer(f / fw, np.arange(h.size))) @ h)
    assert H[0] > 0.999 and H[1] > 0.7          # carrier at |IF| + deviation + data still passed
    assert 20 * np.log10(H[2:].max()) < -60.0    # both edges of the neighbouring channel


def test_oracle_channelizer_feeds_the_pinned_demodulator():
    """Three bursts at the band edges and next to the capture's centre, one wideband capture ->
    float64 channelizer -> C oracle demodulator: every injected packet comes back."""
    from oracle import c_oracle as CO
    from oracle import channelizer_oracle as CHO
    CZ = _cz()
    chans = [0, 25, 50]
    off = [CZ.US_CHANNELS_HZ[c] - CZ.DEFAULT_CENTRE_HZ for c in chans]
    raw, info = synth.synth_wideband([1, 2, 3], off, 3 * 8192)
    shifts = [f + CZ.OUT_RATE // 4 for f in off]
    nb = CHO.channelize(raw, shifts, CZ.design_taps(), CZ.DEFAULT_DECIM, CZ.OUT_RATE, 3.0)
    assert nb.shape == (3, 2 * 3 * 8192)
    res, _ = CO.demod_batch(nb, CO.make_cfg(), threads=3)
    for (payload, start), pk in zip(info, res):
        hits = [(p.call, p.index) for p in pk if bytes(p.data).hex() == payload]
        assert hits, payload
        # the preamble sits 32 symbols after the burst start; the filters and the oversampled match add ~20 samples
        call, idx = hits[0]
        pos = (call - 1) * 8192 + idx
        assert 0 <= pos - (start + 32 * 14) <= 30


@pytest.mark.gpu
def test_channelizer_matches_float64_model():
    from oracle import channelizer_oracle as CHO
    CZ = _cz()
    chans = [0, 7, 24, 25, 26, 50]
    off = [CZ.US_CHANNELS_HZ[c] - CZ.DEFAULT_CENTRE_HZ for c in chans]
    raw, _ = synth.synth_wideband([11, 12, 13, 14, 15, 16], off, 3 * 8192)
    cz = CZ.Channelizer([CZ.US_CHANNELS_HZ[c] for c in chans])
    cz.upload(raw)
    got = cz.run_host()
    want = CHO.channelize(raw, cz.shift_hz, cz.taps, cz.decim, cz.out_rate, cz.gain)
    d = got.astype(np.int32) - want.astype(np.int32)
    # fp32 sums of 512 products against float64: never more than the last bit, and that rarely
    assert np.abs(d).max() <= 1
    assert (d != 0).mean() < 1e-3
    # a shorter output and a ragged capture length
    cz.upload(raw[: 2 * (8192 * 100 + 37)])
    got2 = cz.run_host(8000)
    assert np.array_equal(got2, got[:, : 2 * 8000])
    with pytest.raises(ValueError):
        cz.run_host(8193)


@pytest.mark.gpu
def test_51_hop_channels_from_one_capture():
    """BASELINE configs[2]: 51 channels, one capture, one channelizer launch straight into the
    batch demodulator's input; every channel's packet is recovered where it was injected."""
    from rtldavis_amd import batch, dsp
    CZ = _cz()
    nb = 3
    off = [f - CZ.DEFAULT_CENTRE_HZ for f in CZ.US_CHANNELS_HZ]
    raw, info = synth.synth_wideband(range(100, 151), off, nb * 8192, amplitude=0.05)
    cz = CZ.Channelizer()
    cz.upload(raw)
    cfg = dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", 8192)
    bd = batch.BatchDemodulator(cfg, 51, nb)
    cz.run_into(bd)
    bd.run()
    recs = bd.results()
    for c, (payload, start) in enumerate(info):
        hits = [(int(r["call"]), int(r["index"])) for r in recs
                if int(r["stream"]) == c and r["data"][: int(r["nbytes"])].tobytes().hex() == payload]
        assert hits, (c, payload)
        pos = (hits[0][0] - 1) * 8192 + hits[0][1]
        assert 0 <= pos - (start + 32 * 14) <= 30, (c, pos, start)
    # the demodulator saw exactly the channelizer's bytes
    host = cz.run_host(nb * 8192)
    bd2 = batch.BatchDemodulator(cfg, 51, nb)
    got = bd2.demodulate(host)
    flat = sorted((s, c, p.index, bytes(p.data)) for s in range(51) for c, ps in enumerate(got[s]) for p in ps)
    assert flat == sorted((int(r["stream"]), int(r["call"]), int(r["index"]), r["data"][: int(r["nbytes"])].tobytes())
                          for r in recs)


# ------------------------------------------------------------------------------------------------
# The contract at the edges of the configuration space (tests/chan_bound.py: the bound and the comparator)
# ------------------------------------------------------------------------------------------------
import ctypes as C
import types

import chan_bound as CB

FO = 268800


# name: decim, taps (T or "default"), shifts (Hz), gain, n_out, out_rate, what it reaches
SWEEP = {
    "plan51": (100, "default", "us", 3.0, 3 * 8192, FO),                        # today's plan, under the new comparator
    "d4_t256": (4, 256, [0, -2 * FO, FO + 4321], 0.8, 1024, FO),            # n_early = 64; -Fw/2; > Fo
    "d8_t255_odd": (8, 255, [4 * FO, -123457, 300001, -2 * FO, 77777], 0.8, 129, FO),   # padding; 1 + partial workgroup
    "d640_t512_lds": (640, 512, [320 * FO - 1, -3 * FO - 5], 0.8, 300, FO),  # 160 KiB of LDS
    "d644_t8_lds": (644, 8, [13, -322 * FO + 1], 0.8, 300, FO),
    "d128_t8192": (128, 8192, [7 * FO + 3, -1], 0.8, 512, FO),               # the longest filter
    "g65": (100, 512, "spread", 0.8, 512, FO),                               # 2 groups, the last with 1 channel
    "g130": (100, 512, "spread", 0.8, 512, FO),                              # 3 groups, the last with 2
    "g4096": (100, 512, "spread", 0.8, 300, FO),                             # 64 full groups
    "d12_t37_prime": (12, 37, [0, 100003, -100003 * 3, 250001, -77, 6 * 100003 - 1, -600018], 0.8, 1000, 100003),
    "clip": (20, 64, [1000, -FO // 3, 2 * FO + 11], 1.5, 1024, FO),          # 1-10 % of the bytes clip at each end
    "highpass": (16, 128, [0, 5 * FO + 1, -FO // 7], 0.8, 1024, FO),        # sum of taps ~0: the DC term dominates
}
N_SPREAD = {"g65": 65, "g130": 130, "g4096": 4096}


def _sweep_case(name):
    """(plan, taps, raw, n_out): plan carries decim, out_rate, gain, shift_hz; raw has a ragged tail of 37 samples."""
    from rtldavis_amd import channelizer as CZ
    decim, T, shifts, gain, n_out, fo = SWEEP[name]
    seed = sum(map(ord, name))
    fw = decim * fo
    if T == "default":
        taps = CZ.design_taps()
    else:
        taps = CB.random_taps(T, seed, highpass=name == "highpass")
    if shifts == "us":
        shifts = [f - CZ.DEFAULT_CENTRE_HZ + fo // 4 for f in CZ.US_CHANNELS_HZ]
        off = [f - CZ.DEFAULT_CENTRE_HZ for f in CZ.US_CHANNELS_HZ]
        raw, _ = synth.synth_wideband(range(300, 351), off, n_out, amplitude=0.05)
        raw = np.concatenate([raw, CB.capture(37, seed, fw)])
    else:
        if shifts == "spread":
            shifts = np.random.default_rng(seed).integers(-fw // 2, fw // 2 + 1, N_SPREAD[name])
        raw = CB.capture(n_out * decim + 37, seed, fw)
    plan = types.SimpleNamespace(decim=decim, out_rate=fo, gain=gain, shift_hz=np.asarray(shifts, np.int64),
                                 taps=np.asarray(taps, np.float64))
    return plan, plan.taps, raw, n_out


def _model(plan, taps, raw, n_out):
    from oracle import channelizer_oracle as CHO
    return CHO.channelize_z(raw, plan.shift_hz, taps, plan.decim, plan.out_rate, plan.gain, n_out)


# ---------------------------------------------------------------- CPU: the model against the definition
def _definition(raw, shift_hz, taps, decim, out_rate, gain, n_out):
    """The header's definition as a plain double loop over outputs and taps (Python ints for the phase)."""
    from oracle import channelizer_oracle as CHO
    x = CHO.lut(raw)
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


@pytest.mark.parametrize("decim,T,n_wide", [(4, 5, 61), (4, 13, 64), (8, 3, 83), (8, 17, 130)])
def test_model_equals_the_definition(decim, T, n_wide):
    """channelize_z (the factorised form, as the kernel computes it) against the definition, at shifts the C ABI takes
    and plan_channels refuses: negative, >= out_rate, beyond +-Fw/2, = 0 mod out_rate; a ragged capture length."""
    from oracle import channelizer_oracle as CHO
    fo = 1000
    fw = decim * fo
    taps = CB.random_taps(T, T)
    shifts = [0, 1, -1, 333, -fo - 17, fo, 3 * fo, fw // 2, -fw // 2, fw + 123, -5 * fw - 7, 10 ** 12 + 5]
    raw = CB.capture(n_wide, n_wide, fw)
    n_out = n_wide // decim
    want = _definition(raw, shifts, taps, decim, fo, 1.7, n_out)
    got = CHO.channelize_z(raw, shifts, taps, decim, fo, 1.7, n_out)
    assert np.abs(got - want).max() < 1e-9
    assert np.array_equal(CHO.channelize(raw, shifts, taps, decim, fo, 1.7), CHO.quantise(want))
    # the factorised form itself: g_c[k] = h[k] e^{+j 2 pi shift k / Fw}, phasor e^{-j 2 pi frac((shift mod Fo) t / Fo)}
    x = CHO.lut(raw)
    for c, sh in enumerate(shifts):
        for t in range(n_out):
            s = sum(taps[k] * np.exp(2j * np.pi * ((sh * k) % fw) / fw) * x[decim * t - k] for k in range(T) if decim * t >= k)
            ph = np.exp(-2j * np.pi * (((sh % fo) * t) % fo) / fo)
            assert abs(1.7 * s * ph * 127.6 + 127.4 * (1 + 1j) - want[c, t]) < 1e-9


def test_model_is_channelize_quantised():
    from oracle import channelizer_oracle as CHO
    plan, taps, raw, n_out = _sweep_case("d12_t37_prime")
    Z = _model(plan, taps, raw, n_out)
    q = CHO.channelize(raw, plan.shift_hz, taps, plan.decim, plan.out_rate, plan.gain, n_out)
    assert np.array_equal(q[:, 0::2], np.clip(np.rint(Z.real), 0, 255)) and q.dtype == np.uint8
    assert np.array_equal(q[:, 1::2], np.clip(np.rint(Z.imag), 0, 255))


# ---------------------------------------------------------------- CPU: rd_chan_create's limits at their edges
def _create(decim, T, n_ch=1, out_rate=FO):
    """rd_chan_create through the C ABI (host work only, no device): ValueError past a limit."""
    from rtldavis_amd import _lib
    cfg = _lib.RdChanConfig(out_rate, decim, T, n_ch, 1.0)
    taps = np.ones(T, np.float64) / T
    shifts = np.zeros(n_ch, np.int64)
    h = C.c_void_p()
    _lib.check(_lib.lib().rd_chan_create(C.byref(cfg), taps.ctypes.data, shifts.ctypes.data, C.byref(h)))
    _lib.lib().rd_chan_destroy(h)


@pytest.mark.parametrize("ok,bad", [
    ((644, 8), (648, 8)),          # LDS: 2 (127 D + t_pad + 8) + 16 <= 160 KiB
    ((640, 512), (644, 512)),
    ((4, 256), (4, 257)),          # n_early = ceil((t_pad - 1) / D) <= 64
    ((8, 512), (8, 513)),
    ((128, 8192), (256, 8193)),    # taps <= 8192
])
def test_create_limits_at_their_edges(ok, bad):
    _create(*ok)
    with pytest.raises(ValueError):
        _create(*bad)


def test_create_channel_limit_at_its_edge():
    _create(100, 8, 4096)
    with pytest.raises(ValueError):
        _create(100, 8, 4097)


# ---------------------------------------------------------------- CPU: the comparator has teeth
def _wrong_models(plan, taps, raw, n_out, Z):
    """Models that are wrong the way a kernel could be; each a uint8 [n_ch, 2 n_out]."""
    from oracle import channelizer_oracle as CHO
    D, fo, gain, sh = plan.decim, plan.out_rate, plan.gain, plan.shift_hz
    z = (Z - 127.4 * (1 + 1j)) / (gain * 127.6)
    ph = CHO.out_phasor(sh, fo, n_out)
    g = CHO.mod_taps(taps, sh, fo * D)
    T = taps.size
    t = np.arange(n_out)
    n_early = -(-((T + 7) // 8 * 8 - 1) // D)
    # the steady DC term (all taps) where the window still reaches before the capture: the kernel would add
    # -127.4 (1 + j) sum_{k > D t} g[k] / 127.6 before the phasor
    tail = np.cumsum(g[:, ::-1], axis=1)[:, ::-1]                      # tail[k] = sum_{k' >= k} g[k']
    early = np.zeros_like(z)
    for tt in range(min(n_early, n_out)):
        if D * tt + 1 < T:
            early[:, tt] = -127.4 * (1 + 1j) / 127.6 * tail[:, D * tt + 1] * ph[:, tt]
    # the hi f16 digit alone, as rd_chan_create makes it
    hmax = np.abs(taps).max()
    s = 2.0 ** (14 - int(np.ceil(np.log2(hmax))))
    g32 = g.astype(np.complex64)
    g_hi = ((g32.real * s).astype(np.float16).astype(np.float64) + 1j * (g32.imag * s).astype(np.float16)) / s
    # the capture for this one: in four windows of channel 0, bytes 0 / 255 by the sign of the dropped digit of its real
    # part, so that the digits add up there (on random bytes they largely cancel, below the accumulation bound); the
    # other bytes are the sweep's, so that few bytes differ at all
    lo = g32[0].astype(np.complex128) - g_hi[0]
    adv = raw.copy().reshape(-1, 2)
    t_pad = (T + 7) // 8 * 8
    for tt in range(n_out - 1, 0, -max(t_pad // D + 2, n_out // 4))[:4]:
        k = np.arange(min(T, D * tt + 1))
        adv[D * tt - k, 0] = np.where(lo.real[k] > 0, 255, 0)
        adv[D * tt - k, 1] = np.where(lo.imag[k] > 0, 0, 255)
    adv = adv.reshape(-1)
    z_hi = CHO.filter_decimate(CHO.lut(adv), g_hi, D, n_out) * ph
    restart = ph[:, t % 128] / ph                                       # the mixer clock back to 0 every 128 outputs
    moved = np.concatenate([raw[2:], raw[:2]])                          # the window one wideband sample late
    Q = lambda zz: CHO.quantise(gain * zz * 127.6 + 127.4 * (1 + 1j))
    return {   # what: (the capture it was run on, its bytes)
        "taps reversed": (raw, CHO.channelize(raw, sh, taps[::-1], D, fo, gain, n_out)),
        "window moved by one sample": (raw, CHO.channelize(moved, sh, taps, D, fo, gain, n_out)),
        "shift off by 1 Hz": (raw, CHO.channelize(raw, sh + 1, taps, D, fo, gain, n_out)),
        "I and Q swapped": (raw, Q(1j * np.conj(z))),
        "Q negated": (raw, Q(np.conj(z))),
        "mixer restarts every 128 outputs": (raw, Q(z * restart)),
        "steady DC term for the first outputs": (raw, Q(z + early)),
        "low f16 tap digit dropped": (adv, Q(z_hi)),
    }


TEETH = ["d4_t256", "d8_t255_odd", "d640_t512_lds", "d644_t8_lds", "d128_t8192", "g65", "d12_t37_prime", "clip",
         "highpass", "plan51"]


@pytest.mark.parametrize("name", TEETH)
def test_comparator_rejects_wrong_models(name):
    """Each wrong model fails assert_matches_model at this config's delta, on bytes outside the delta band: the bound
    is tight enough to tell a kernel that is wrong in any of these ways from one that rounds differently."""
    plan, taps, raw, n_out = _sweep_case(name)
    if np.allclose(taps, taps[::-1]):   # (a symmetric filter cannot tell the tap order)
        taps = CB.random_taps(taps.size, 7)
    Z = _model(plan, taps, raw, n_out)
    delta = CB.error_bound(plan, taps, Z, raw)
    from oracle import channelizer_oracle as CHO
    assert CB.assert_matches_model(CHO.quantise(Z), Z, delta)["mismatches"] == 0
    for what, (cap, got) in _wrong_models(plan, taps, raw, n_out, Z).items():
        if cap is not raw:
            Z, delta = _model(plan, taps, cap, n_out), None
            delta = CB.error_bound(plan, taps, Z, cap)
        s = CB.check_against_model(got, Z, delta)
        assert s["bad_lsb"] + s["bad_exact"] > 0, (name, what, s)
        with pytest.raises(AssertionError):
            CB.assert_matches_model(got, Z, delta)



# ---------------------------------------------------------------- GPU: the kernel across the sweep
def _channelizer(plan):
    from rtldavis_amd import channelizer as CZ
    # centre 0 and IF 0: channel "frequency" = shift
    return CZ.Channelizer(plan.shift_hz, centre_hz=0, decim=plan.decim, taps=plan.taps, gain=plan.gain,
                          out_rate=plan.out_rate, if_hz=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SWEEP))
def test_kernel_within_the_bound_across_configs(name):
    """Channelizer.run_host against channelize_z with assert_matches_model at every sweep config; prints delta, the
    exempt fraction and the largest boundary distance among the mismatches (the room the bound leaves)."""
    from oracle import channelizer_oracle as CHO
    plan, taps, raw, n_out = _sweep_case(name)
    cz = _channelizer(plan)
    assert np.array_equal(cz.shift_hz, plan.shift_hz)
    cz.upload(raw)
    got = cz.run_host(n_out)
    Z = _model(plan, taps, raw, n_out)
    delta = CB.error_bound(plan, taps, Z, raw)
    s = CB.assert_matches_model(got, Z, delta)
    print(f"\n[chan-sweep] {name}: delta median {np.median(delta):.2e} max {s['delta_max']:.2e}, exempt "
          f"{s['exempt']:.2%}, mismatches {s['mismatches']}/{got.size}, worst distance {s['worst_dist']:.2e} "
          f"({s['worst_ratio']:.2f} of delta)")
    # the old tolerance still holds
    d = got.astype(np.int32) - CHO.quantise(Z).astype(np.int32)
    assert np.abs(d).max() <= 1 and (d != 0).mean() < 1e-3
    if name == "clip":
        q = CHO.quantise(Z)
        assert 0.01 <= (q == 0).mean() <= 0.10 and 0.01 <= (q == 255).mean() <= 0.10
    if name == "highpass":
        assert abs(taps.sum()) < 1e-12


@pytest.mark.gpu
def test_strided_destination_leaves_the_gaps_alone():
    """rd_chan_run into device memory with dst_stream_stride > 2 n_out (n_out not a multiple of 128): channel c's bytes
    at c * stride equal run_host's, and every byte in the gaps and after n_out keeps its sentinel."""
    from rtldavis_amd import _lib
    plan, taps, raw, _ = _sweep_case("d8_t255_odd")
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
