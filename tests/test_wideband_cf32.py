"""The live wideband receiver on float32 captures (WidebandReceiver(sample_format="cf32")): the streamed bytes equal
the one-shot channelizer's on the whole capture, byte for byte, and lie within the bound of the float64 model
(tests/chan_bound_cf32.py); the weak default-plan capture fed as complex64 chunks; retune, set_gain and the level
records on a float receiver.  PARITY UNPINNED, as for the channelizer."""
import functools
import types

import numpy as np
import pytest

import chan_bound as CB
import chan_bound_cf32 as CC
import gain_cases as GC
import retune_cases as RC
from rtldavis_amd import synth
from stream_parse_helpers import _oracle_expected, _rows, assert_rows_match

pytestmark = pytest.mark.gpu
B = 8192
W = 0.01
# the small block: one workgroup per chunk, 256 taps reaching into the previous chunk
DECIM, T, BS, NK = 4, 256, 128, 6
FO = 19200 * 14
GAIN = 0.8
BOUNDARY = 3          # retune / set_gain before chunk 3


def _cfg(block_size=B):
    from rtldavis_amd import dsp
    return dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", block_size)


@functools.lru_cache(maxsize=None)
def _small():
    """The small-block case: plan, capture (the special values in chunk 0 and in chunk 4) and its chunks."""
    from rtldavis_amd import channelizer as CZ
    centre = CZ.DEFAULT_CENTRE_HZ
    chans = [centre + 100000, centre - 400001, centre + 7]
    taps = CB.random_taps(T, 99)
    plan = types.SimpleNamespace()
    CZ.plan_channels(plan, chans, centre, DECIM, taps, GAIN, FO)
    raw = CC.capture_cf32(NK * BS * DECIM, 99)
    CC.plant_specials(raw.reshape(-1, 2), base=4 * BS * DECIM + 5)
    raw.setflags(write=False)
    step = 2 * BS * DECIM
    chunks = [raw[step * k: step * (k + 1)] for k in range(NK)]
    assert all(np.isnan(chunks[k]).any() and np.isinf(chunks[k]).any() for k in (0, 4))
    return types.SimpleNamespace(chans=chans, centre=centre, taps=taps, plan=plan, raw=raw, chunks=chunks)


def _receiver(sm):
    from rtldavis_amd import wideband
    return wideband.WidebandReceiver(_cfg(BS), sm.chans, sm.centre, decim=DECIM, taps=sm.taps, gain=GAIN, sample_format="cf32")


@functools.lru_cache(maxsize=None)
def _model_at(shift, gain):
    """(Z, delta) of the whole small capture at shifts `shift` and per-channel gains `gain` (tuples)."""
    sm = _small()
    cfg = types.SimpleNamespace(decim=DECIM, out_rate=FO, gain=np.asarray(gain, np.float64), shift_hz=np.asarray(shift, np.int64))
    Z = CC.model_z_cf32(sm.raw, cfg.shift_hz, sm.taps, DECIM, FO, cfg.gain)
    return Z, CC.error_bound_cf32(cfg, sm.taps, Z, sm.raw)


@functools.lru_cache(maxsize=None)
def _plain():
    """The chunks' bytes of a receiver that is neither retuned nor re-gained, one chunk at a time."""
    sm = _small()
    w = _receiver(sm)
    out = []
    for chunk in sm.chunks:
        w.demodulate(chunk)
        out.append(w.channelized())
    return out


def test_streamed_chunks_equal_the_one_shot_form():
    """Case 12: six chunks of 128 outputs, decim 4, 256 taps, 3 channels - the streamed bytes are the one-shot form's
    on the whole capture and satisfy the bound; the special values lie in chunk 0 and in chunk 4."""
    from rtldavis_amd import channelizer as CZ
    sm = _small()
    streamed = np.concatenate(_plain(), axis=1)
    cz = CZ.Channelizer(sm.chans, sm.centre, decim=DECIM, taps=sm.taps, gain=GAIN, out_rate=FO, sample_format="cf32")
    assert np.array_equal(cz.shift_hz, sm.plan.shift_hz)
    cz.upload(sm.raw)
    assert np.array_equal(streamed, cz.run_host())
    Z, delta = _model_at(tuple(sm.plan.shift_hz), (GAIN,) * 3)
    s = CB.assert_matches_model(streamed, Z, delta)
    print(f"\n[chan-cf32-stream] small block: delta max {s['delta_max']:.2e}, exempt {s['exempt']:.2%}, mismatches "
          f"{s['mismatches']}/{streamed.size}, worst distance {s['worst_dist']:.2e} ({s['worst_ratio']:.2f} of delta)")
    # two in flight, after a reset: the same bytes
    w = _receiver(sm)
    w.demodulate(sm.chunks[0])
    w.reset()
    got = []
    w.submit(sm.chunks[0])
    for k in range(1, NK):
        w.submit(sm.chunks[k].reshape(-1, 2) if k == 2 else sm.chunks[k])
        assert w.inflight == 2
        w.fetch()
        got.append(w.channelized())
    w.fetch()
    got.append(w.channelized())
    assert np.array_equal(np.concatenate(got, axis=1), streamed)


def test_weak_default_plan_capture_as_complex64_chunks():
    """Case 13: 51 bursts at 1 % of full scale, gain 300, three chunks of complex64 with two in flight: every burst
    comes back where it was put, and with parse on the CRC-valid messages are the dsp oracle's on the channelized bytes."""
    from rtldavis_amd import wideband
    from rtldavis_amd import channelizer as CZ
    nk = 3
    off = [f - CZ.DEFAULT_CENTRE_HZ for f in CZ.US_CHANNELS_HZ]
    raw, info = synth.synth_wideband(range(300, 351), off, nk * B, amplitude=0.12 * W, noise=0.02 * W, sample_format="cf32")
    cx = raw.view(np.complex64)
    assert cx.dtype == np.complex64 and cx.size == nk * B * 100
    w = wideband.WidebandReceiver(_cfg(), gain=3.0 / W, sample_format="cf32")
    assert w.chunk_bytes == 8 * w.chunk_samples == cx.nbytes // nk
    w.set_parse(True)
    n = w.chunk_samples
    got, rows, blocks = [], [], []

    def take():
        got.append(w.fetch())
        rows.append(_rows(w.parsed()))
        blocks.append(w.channelized())

    w.submit(cx[:n])
    for k in range(1, nk):
        w.submit(cx[n * k: n * (k + 1)])
        assert w.inflight == 2
        take()
    take()
    found = 0
    for c, (payload, start) in enumerate(info):
        hits = [(k, p.index) for k in range(nk) for p in got[k][c] if bytes(p.data).hex() == payload]
        if hits:
            pos = (hits[0][0] - 1) * B + hits[0][1]
            found += 0 <= pos - (start + 32 * 14) <= 30
    assert found == 51
    orc = _oracle_expected([[blocks[k][c] for k in range(nk)] for c in range(51)], B)
    assert sum(assert_rows_match(rows[k], orc[k], ("oracle", k)) for k in range(nk)) >= 1
    assert sum(len(r) for r in rows) >= 51


def test_retune_on_a_float_receiver():
    """Case 14: two of the three channels retuned before chunk 3, with chunks in flight: every chunk satisfies the
    bound against the model of its tuning (s', P') - the piecewise model of tests/retune_cases.py: the whole capture at
    shifts s', rotated by P' - and the channel that stays is untouched.  This runs k_chan_retune on float tables."""
    sm = _small()
    plain = _plain()
    plan_shift = [int(s) for s in sm.plan.shift_hz]
    off = np.asarray([9001, 0, -17777], np.int64)
    new = [s + int(o) for s, o in zip(plan_shift, off)]
    phase = RC.next_phase([0, 0, 0], plan_shift, new, BOUNDARY * BS, FO)
    assert phase[1] == 0 and phase[0] != 0 and phase[2] != 0
    w = _receiver(sm)
    got = []
    w.submit(sm.chunks[0])
    for k in range(1, NK):
        if k == BOUNDARY:
            assert w.inflight == 1
            w.retune(off)
        w.submit(sm.chunks[k])
        w.fetch()
        got.append(w.channelized())
    w.fetch()
    got.append(w.channelized())
    s_now, p_now = w.tuning()
    assert [int(v) for v in s_now] == new and [int(v) for v in p_now] == phase
    Z0, d0 = _model_at(tuple(plan_shift), (GAIN,) * 3)
    Z1, d1 = _model_at(tuple(new), (GAIN,) * 3)
    rot = np.exp(-2j * np.pi * np.asarray(phase, np.float64) / FO)[:, None]
    for k in range(NK):
        a, b = k * BS, (k + 1) * BS
        if k < BOUNDARY:
            assert np.array_equal(got[k], plain[k]), k
            CB.assert_matches_model(got[k], Z0[:, a:b], d0[:, a:b])
        else:
            Zs = RC.OFFSET + (Z1[:, a:b] - RC.OFFSET) * rot
            s = CB.assert_matches_model(got[k], Zs, d1[:, a:b])
            print(f"\n[chan-cf32-retune] chunk {k}: exempt {s['exempt']:.2%}, mismatches {s['mismatches']}/{got[k].size}, "
                  f"worst distance {s['worst_dist']:.2e} ({s['worst_ratio']:.2f} of delta)")
            assert np.array_equal(got[k][1], plain[k][1]), k
            assert not np.array_equal(got[k][0], plain[k][0]) and not np.array_equal(got[k][2], plain[k][2])


def test_levels_of_a_float_chunk_are_the_definition():
    """Case 15: with levels on, the input record equals the numpy evaluation of the definition (k = clip(rint(32768
    adm(v)), -32768, 32767); NaN counted as clipped, value 0) exactly, every special value present; the per-channel
    records equal numpy on channelized(); agc.GainControl takes the result."""
    from rtldavis_amd import agc
    sm = _small()
    plain = _plain()
    w = _receiver(sm)
    w.set_levels(True)
    ctl = agc.GainControl(3, BS)
    for k in range(NK):
        w.demodulate(sm.chunks[k])
        block = w.channelized()
        assert np.array_equal(block, plain[k]), k
        lv = w.levels()
        assert lv.chunk == k
        assert tuple(lv.input) == CC.input_levels(sm.chunks[k]), k
        want = GC.channel_levels(block)
        for c in range(3):
            r = lv.channels[c]
            assert (int(r["peak"]), int(r["clipped"]), int(r["power"])) == want[c], (k, c)
            assert float(r["gain"]) == float(np.float32(GAIN))
        g = ctl.update(lv)
        assert g is None or (g.shape == (3,) and np.all(g > 0))
    peak, clipped, power = CC.input_levels(sm.chunks[0])
    assert peak == 32768 and clipped >= 5          # NaN, +-Inf, 9.5 and 1 - 2^-24 at least
    for v, k in ((np.nan, 0), (np.inf, 32767), (-np.inf, -32768), (9.5, 32767), (-0.0, 0), (1e-40, 0), (2.0 ** -15, 1),
                 (12345 / 32767, 12345), (1 - 2.0 ** -24, 32767), (0.5 / 32768, 0), (1.5 / 32768, 2), (-1.0, -32768)):
        one = np.zeros(8, np.float32)
        one[3] = v
        pk, cl, pw = CC.input_levels(one)
        assert (pk, pw) == (abs(k), k * k) and cl == int(k in (32767, -32768) or v != v), v


def test_set_gain_at_a_chunk_boundary():
    """Case 16: per-channel gains changed before chunk 3 take effect exactly there: the bytes on each side satisfy the
    bound at that side's gains, the channel whose gain stays is untouched."""
    sm = _small()
    plain = _plain()
    after = (GAIN, 0.4, 1.2)
    w = _receiver(sm)
    got = []
    w.submit(sm.chunks[0])
    for k in range(1, NK):
        if k == BOUNDARY:
            w.set_gain(after)
        w.submit(sm.chunks[k])
        w.fetch()
        got.append(w.channelized())
    w.fetch()
    got.append(w.channelized())
    assert np.array_equal(w.gains(), np.asarray(after, np.float32).astype(np.float64))
    shift = tuple(int(s) for s in sm.plan.shift_hz)
    Z0, d0 = _model_at(shift, (GAIN,) * 3)
    Z1, d1 = _model_at(shift, tuple(float(np.float32(g)) for g in after))
    for k in range(NK):
        a, b = k * BS, (k + 1) * BS
        Z, d = (Z0, d0) if k < BOUNDARY else (Z1, d1)
        s = CB.assert_matches_model(got[k], Z[:, a:b], d[:, a:b])
        assert np.array_equal(got[k][0], plain[k][0]), k
        if k < BOUNDARY:
            assert np.array_equal(got[k], plain[k]), k
        else:
            assert not np.array_equal(got[k][1], plain[k][1]) and not np.array_equal(got[k][2], plain[k][2])
            # the old gains' model does not pass for the new bytes
            bad = CB.check_against_model(got[k], Z0[:, a:b], d0[:, a:b])
            assert bad["bad_lsb"] + bad["bad_exact"] > 0
            print(f"\n[chan-cf32-gain] chunk {k}: exempt {s['exempt']:.2%}, mismatches {s['mismatches']}/{got[k].size}")
