"""Helpers shared by tests/test_wideband_gain_cpu.py and tests/test_wideband_gain.py (no tests in here): the gain sets
and schedules at which WidebandReceiver.set_gain is tested on the four configurations of retune_cases.CASES, the float64
model of a chunk evaluated per channel at that channel's gain with its a-priori bound, the level records restated in
NumPy integers, and the weak-and-strong capture of the closed gain loop with its model.  Nothing here touches a device.

Model of a chunk at gains g (rd_channelizer.hip, GAIN): row c of the model and of the bound are those of the scalar
model at gain g[c] - chan_bound_fmt.model_z / error_bound_fmt, whose `gain` is the only place the gain enters - under the
tuning (s', P') of retune_cases.segment_model.  The gains come from PALETTE, so a case needs one evaluation per palette
entry and tuning, not one per channel.

Share of bytes the model alone leaves within the bound of a rounding boundary (test_wideband_gain_cpu.py asserts <= 6 %
for every chunk; the GPU tests may exempt 10 %), worst chunk of the schedule below, measured:
    d4_t256_b128  4.04 %      70ch  3.25 %      t255_sym8  3.12 %      s16  0.94 %
"""
import functools
from types import SimpleNamespace

import numpy as np

import chan_bound_fmt as CF
import retune_cases as RC
from rtldavis_amd import channelizer as CZ
from rtldavis_amd import synth

# 0.25 .. 300, three decades; the first three entries span the range (the smallest case has three channels)
PALETTE = (0.25, 300.0, 3.0, 40.0, 1.0)
MODEL_EXEMPT_CAP = 0.06
GPU_EXEMPT_CAP = 0.10


@functools.lru_cache(maxsize=None)
def case(name):
    """retune_cases.case plus the gain schedule {chunk: gains}: distinct gains before chunk 0, a subset of the channels
    (retune_cases' subset) changes before chunk 2, every channel before chunk 3 - where retune_cases' schedule[3] also
    retunes every channel."""
    cs = RC.case(name)
    n, L = cs.n_ch, len(PALETTE)
    ia = np.arange(n) % L
    ib = np.where(cs.subset, (ia + 1) % L, ia)
    ic = (ib + 2) % L
    pal = np.asarray(PALETTE, np.float64)
    ga, gb, gc = pal[ia], pal[ib], pal[ic]
    assert np.all((ga != gb) == cs.subset) and np.all(gb != gc)
    assert ga.min() == 0.25 and ga.max() == 300.0
    return SimpleNamespace(cs=cs, name=name, n_ch=n, nk=cs.nk, gain_schedule={0: ga, 2: gb, 3: gc},
                           retune_schedule={3: cs.schedule[3]})


def gains_per_chunk(gc):
    """The gains in force for each chunk under the case's schedule (float32 values, as float64)."""
    g, out = np.full(gc.n_ch, gc.cs.gain), []
    for k in range(gc.nk):
        g = gc.gain_schedule.get(k, g)
        out.append(np.asarray(g, np.float32).astype(np.float64))
    return out


@functools.lru_cache(maxsize=None)
def _model_of(name, shift, gain):
    """(Z, delta) of the whole capture, every channel at the scalar gain `gain`, shifts `shift` (a tuple)."""
    cs = RC.case(name)
    cfg = SimpleNamespace(decim=cs.decim, out_rate=cs.fo, gain=float(gain), shift_hz=np.asarray(shift, np.int64))
    Z = CF.model_z(cs.raw, cs.fmt, cfg.shift_hz, cs.taps, cs.decim, cs.fo, float(gain))
    return Z, CF.error_bound_fmt(cfg, cs.taps, Z, cs.raw, cs.fmt)


def chunk_model(cs, k, shift, phase, gains):
    """(Z, delta) of chunk k tuned to (shift, phase), channel c at gains[c]."""
    a, b = k * cs.bs, (k + 1) * cs.bs
    rot = np.exp(-2j * np.pi * np.asarray([int(p) % cs.fo for p in phase], np.float64) / cs.fo)
    Z = np.empty((cs.n_ch, cs.bs), np.complex128)
    delta = np.empty((cs.n_ch, cs.bs))
    for g in sorted(set(float(v) for v in gains)):
        Zg, dg = _model_of(cs.name, tuple(int(s) for s in shift), g)
        rows = np.flatnonzero(np.asarray(gains, np.float64) == g)
        Z[rows] = RC.OFFSET + (Zg[rows, a:b] - RC.OFFSET) * rot[rows, None]
        delta[rows] = dg[rows, a:b]
    return Z, delta


def schedule_models(gc):
    """Per chunk: (Z, delta, gains, (shift, phase)) under the case's gain schedule and its retune before chunk 3."""
    cs = gc.cs
    tun = RC.tunings(cs, gc.retune_schedule)
    return [chunk_model(cs, k, *tun[k], g) + (g, tun[k]) for k, g in enumerate(gains_per_chunk(gc))]


# ------------------------------------------------------------------------------------------ levels in NumPy integers
def channel_levels(block):
    """(peak, clipped, power) per channel of a channelized chunk uint8 [n_channels, 2 B], Python integers."""
    a = 2 * np.asarray(block, np.uint8).astype(np.int64) - 255
    b = np.asarray(block)
    return [(int(np.abs(r).max()), int(((q == 0) | (q == 255)).sum()), int((r * r).sum())) for r, q in zip(a, b)]


def input_levels(chunk, fmt):
    """(peak, clipped, power) of a capture chunk in format fmt."""
    k = np.asarray(chunk).reshape(-1)
    assert k.dtype == CF.DTYPE[fmt]
    info = np.iinfo(k.dtype)
    a = k.astype(np.int64)
    a = 2 * a - 255 if fmt == "u8" else a
    return int(np.abs(a).max()), int(((k == info.min) | (k == info.max)).sum()), int((a * a).sum())


# ------------------------------------------------------------------------------------------ closed gain loop
# An int16 capture on the default plan (decim 100, 512 taps), chunks of LOOP_B outputs, built like retune_cases' closed-loop
# capture: a STRONG burst at 0.9 of full scale in one channel, a WEAK burst of LOOP_WEAK counts in another, LOOP_NOISE
# counts of noise per component.  At the scalar gain 3.0 the weak burst is 127.6 x 3 x 6 / 32768 = 0.07 quantiser steps
# about the offset 127.4: every byte rounds to 127, the channel is a constant and its packet is lost; the strong one
# clips (344 steps) and is received.  The loop: every channel starts at 3.0 and, its noise far below one step, climbs one
# LOOP_AGC step (10 dB) after every second quiet chunk to the table's top, 300, where the weak burst spans +-7 steps.
# Fed with two chunks in flight, the levels of chunk k decide the gains of chunk k + 2.  The seeds (retune_cases') put the
# strong burst into chunk 2, before the climb, and the weak one into chunk 9, after it.
# Found while choosing the amplitudes (model and dsp oracle, no device): (i) a weak burst of "a few tens of counts" is NOT
# lost at 3.0 - at 40 counts, 0.47 steps, the bytes toggle between 127 and 128 about the offset and the demodulator reads
# the packet from the toggling; the scalar gain loses it only below 0.1 step, 8 counts, hence 6.  (ii) The strong burst is
# received clipped 2.7 times over (gain 3.0) but not as the pure square wave it is at gains of 95 and 300, hence its
# place before the climb: a loop that steers on the noise floor alone does not protect a burst that strong.
LOOP_B = 4096
LOOP_NK = 12
LOOP_CHANNELS = (8, 40)            # strong, weak
LOOP_SEEDS = (29, 4)
LOOP_STRONG = 0.9                  # of full scale
LOOP_WEAK = 6.0 / 32768.0
LOOP_NOISE = 3.0 / 32768.0
LOOP_SCALAR_GAIN = 3.0
LOOP_AGC = dict(min_gain=3.0, max_gain=300.0, step_db=10.0, start_gain=3.0, low_power=9 * 2 * LOOP_B,
                high_power=2000 * 2 * LOOP_B, clip_max=2 * LOOP_B, hold=2)


@functools.lru_cache(maxsize=None)
def loop_capture():
    chans = [CZ.US_CHANNELS_HZ[c] for c in LOOP_CHANNELS]
    f = [c - RC.CENTRE for c in chans]
    n_out = LOOP_NK * LOOP_B
    payloads = [synth.payload_of(s) for s in LOOP_SEEDS]
    strong, i0 = synth.synth_wideband(LOOP_SEEDS[:1], f[:1], n_out, amplitude=LOOP_STRONG, noise=LOOP_NOISE,
                                      sample_format="s16", payloads=payloads[:1])
    weak, i1 = synth.synth_wideband(LOOP_SEEDS[1:], f[1:], n_out, amplitude=LOOP_WEAK, noise=0.0, sample_format="s16",
                                    payloads=payloads[1:])
    raw = np.clip(strong.astype(np.int32) + weak.astype(np.int32), -32768, 32767).astype(np.int16)
    plan = SimpleNamespace()
    CZ.plan_channels(plan, chans, RC.CENTRE, CZ.DEFAULT_DECIM, None, LOOP_SCALAR_GAIN, CZ.OUT_RATE)
    return SimpleNamespace(raw=raw, info=i0 + i1, payloads=payloads, plan=plan, chans=chans,
                           step=2 * LOOP_B * CZ.DEFAULT_DECIM)


@functools.lru_cache(maxsize=None)
def _loop_z1():
    """The model in front of the quantiser at gain 1 (Z - 127.4 (1 + j) is linear in the gain)."""
    lc = loop_capture()
    return CF.model_z(lc.raw, "s16", lc.plan.shift_hz, lc.plan.taps, CZ.DEFAULT_DECIM, CZ.OUT_RATE, 1.0)


def loop_model_block(k, gains):
    """The model's quantised chunk k, channel c at the float32 gain gains[c]: uint8 [2, 2 LOOP_B]."""
    from oracle import channelizer_oracle as CHO
    g = np.asarray(gains, np.float32).astype(np.float64)[:, None]
    return CHO.quantise(RC.OFFSET + (_loop_z1()[:, k * LOOP_B: (k + 1) * LOOP_B] - RC.OFFSET) * g)


def loop_messages(blocks):
    """The dsp oracle's parse of the chunks' bytes (a list of uint8 [2, 2 LOOP_B]): the CRC-valid messages as a sorted
    list of (channel, chunk, payload hex) - the result the CPU and the GPU test compare."""
    from oracle import dsp_oracle as O
    cfg = O.OracleConfig(19200, 14, 16, 80, RC.PREAMBLE, LOOP_B)
    out = []
    for c in range(len(LOOP_CHANNELS)):
        for k, rows in enumerate(O.parse_calls([b[c] for b in blocks], cfg)):
            out += [(c, k, r[1]) for r in rows if r[2]]
    return sorted(out)


def loop_run_model():
    """The closed loop on the model, in the order of the device test (two chunks in flight: the levels of chunk k are
    read when chunk k + 1 has been submitted, so they decide chunk k + 2).  Returns (blocks, gains per chunk)."""
    from rtldavis_amd import agc
    ctl = agc.GainControl(len(LOOP_CHANNELS), LOOP_B, **LOOP_AGC)
    nxt = np.asarray(ctl.gains(), np.float64)
    blocks, used = [], []
    for k in range(LOOP_NK):
        if k >= 2:
            lv = [dict(zip(("peak", "clipped", "power"), r)) for r in channel_levels(blocks[k - 2])]
            new = ctl.update(lv)
            if new is not None:
                nxt = np.asarray(new, np.float64)
        used.append(nxt.copy())
        blocks.append(loop_model_block(k, nxt))
    return blocks, used
