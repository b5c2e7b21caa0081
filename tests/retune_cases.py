"""Helpers shared by tests/test_wideband_retune_cpu.py and tests/test_wideband_retune.py (no tests in here): the
configurations at which WidebandReceiver.retune is tested, their captures and retune schedules, the float64 model of a
retuned segment with its a-priori bound, the phase accumulator restated with Python integers, and the closed-loop
capture (two bursts of one payload, both off the channel's centre) with its model.  Nothing here touches a device.

Model of a segment tuned to (s', P') (rd_channelizer.hip, RETUNE): with Z_{s'} the float64 model of the WHOLE capture at
shifts s' (every output filtered with the new band-pass, history included),
    Z_seg = 127.4 (1 + j) + (Z_{s'} - 127.4 (1 + j)) exp(-2 pi j P' / Fo)
over the segment's outputs; the bound is that of the shifts s' - the rotation is part of the output phasor's exact integer
remainder, so it adds no rounding, and M = |Z - 127.4 (1 + j)| / gain does not change under it."""
import functools
from types import SimpleNamespace

import numpy as np

import chan_bound as CB
import chan_bound_fmt as CF
from rtldavis_amd import channelizer as CZ
from rtldavis_amd import synth

PREAMBLE = "1100101110001001"
CENTRE = CZ.DEFAULT_CENTRE_HZ
OFFSET = 127.4 * (1 + 1j)

# name: (sample format, channels, decim, taps (None: the default design), block_size, symbol_length, chunks); the
# captures are chan_bound.capture / chan_bound_fmt.capture_fmt at their own level, with which the model alone leaves at
# most 6 % of the bytes within the bound of a rounding boundary (test_wideband_retune_cpu.py holds every case to 10 %).
CASES = {
    "d4_t256_b128": ("u8", 3, 4, 256, 128, 14, 6),     # all 64 early DC entries, one workgroup per chunk, windows into the previous chunk
    "70ch": ("u8", 70, 100, None, 1024, 14, 4),        # two groups, a part-filled row block
    "t255_sym8": ("s8", 4, 100, 255, 1024, 8, 4),      # tap padding, DC level 128, Fo = 153600
    "s16": ("s16", 5, 8, 64, 128, 14, 6),              # digit layout, kc = 4, no DC term
}
LARGE_CLOCK_CASE = "d4_t256_b128"
LARGE_CLOCK = 2 ** 40 + 128 * 77


def packet_config(block_size, symbol_length=14):
    from rtldavis_amd import dsp
    return dsp.PacketConfig(19200, symbol_length, 16, 80, PREAMBLE, block_size)


def next_phase(phase, shift, new_shift, t_b, fo):
    """P' = (P + (s - s') t_b) mod Fo per channel, Python integers throughout."""
    return [(int(p) + (int(s) - int(s2)) * int(t_b)) % int(fo) for p, s, s2 in zip(phase, shift, new_shift)]


EXTRA = {}      # cases another module brings along (full_stack_cases): name -> a namespace with the fields of case()


def case(name):
    """Everything a test needs of one configuration: the receiver's arguments, the capture and its chunks, and the
    retune schedule {chunk index: offsets}: a subset of the channels before chunk 2, all of them before chunk 3
    (negative shifts and both band edges among them)."""
    return EXTRA[name] if name in EXTRA else _case(name)


@functools.lru_cache(maxsize=None)
def _case(name):
    fmt, n_ch, decim, T, bs, sl, nk = CASES[name]
    seed = sum(map(ord, name))
    fo = 19200 * sl
    fw = fo * decim
    rng = np.random.default_rng(seed)
    taps = None if T is None else CB.random_taps(T, seed)
    chans = [int(CENTRE + f) for f in rng.integers(-fw // 2 + fo, fw // 2 - fo, n_ch)]
    plan = SimpleNamespace()
    CZ.plan_channels(plan, chans, CENTRE, decim, taps, 3.0, fo)
    n = nk * bs * decim
    raw = CB.capture(n, seed, fw) if fmt == "u8" else CF.capture_fmt(n, seed, fmt)
    step = 2 * bs * decim
    chunks = [raw[step * k: step * (k + 1)] for k in range(nk)]
    # before chunk 2: every other channel moves by up to +-20 kHz, the others stay
    sub = np.arange(n_ch) % 2 == 0
    off_a = np.where(sub, rng.integers(-20000, 20001, n_ch), 0).astype(np.int64)
    off_a[0] = 9001 if off_a[0] == 0 else off_a[0]
    # before chunk 3: every channel moves - the band edges, one step inside the lower one, 0 Hz, the rest negative
    target = -rng.integers(1, fw // 2, n_ch).astype(np.int64)
    for c, v in enumerate((-(fw // 2), fw // 2, -(fw // 2) + 1, 0)[:n_ch]):
        target[c] = v
    off_b = target - plan.shift_hz
    assert np.all(plan.shift_hz + off_a != target)
    return SimpleNamespace(name=name, fmt=fmt, n_ch=n_ch, decim=decim, taps=plan.taps, user_taps=taps, bs=bs, sl=sl, nk=nk,
                           fo=fo, fw=fw, chans=chans, plan_shift=plan.shift_hz.copy(), gain=3.0, raw=raw, chunks=chunks,
                           subset=sub, schedule={2: off_a, 3: off_b}, cfg=packet_config(bs, sl))


def receiver(cs, chans=None):
    from rtldavis_amd import wideband
    return wideband.WidebandReceiver(cs.cfg, cs.chans if chans is None else chans, CENTRE, decim=cs.decim, taps=cs.user_taps,
                                     gain=cs.gain, sample_format=cs.fmt)


def tunings(cs, schedule=None, t_off=0):
    """Per chunk, the tuning (shift, P) the schedule leads to - the boundaries at t_off + k block_size."""
    schedule = cs.schedule if schedule is None else schedule
    shift, phase, out = [int(s) for s in cs.plan_shift], [0] * cs.n_ch, []
    for k in range(cs.nk):
        if k in schedule:
            new = [int(s) + int(o) for s, o in zip(cs.plan_shift, np.broadcast_to(schedule[k], (cs.n_ch,)))]
            phase = next_phase(phase, shift, new, t_off + k * cs.bs, cs.fo)
            shift = new
        out.append((tuple(shift), tuple(phase)))
    return out


def large_clock_schedule(cs):
    """The large-clock case: the clock starts at LARGE_CLOCK and every channel is retuned at the first boundary after it."""
    return {1: cs.schedule[3]}


@functools.lru_cache(maxsize=None)
def _model_of(name, shift):
    """(Z_{s'}, delta) of the whole capture at shifts s' (a tuple)."""
    cs = case(name)
    cfg = SimpleNamespace(decim=cs.decim, out_rate=cs.fo, gain=cs.gain, shift_hz=np.asarray(shift, np.int64))
    Z = CF.model_z(cs.raw, cs.fmt, cfg.shift_hz, cs.taps, cs.decim, cs.fo, cs.gain)
    return Z, CF.error_bound_fmt(cfg, cs.taps, Z, cs.raw, cs.fmt)


def segment_model(cs, k, shift, phase, t_off=0):
    """(Z_seg, delta) of chunk k tuned to (shift, phase) on a receiver whose clock started at t_off: the rotation
    constant is (s' t_off + P') mod Fo."""
    Z, delta = _model_of(cs.name, tuple(shift))
    a, b = k * cs.bs, (k + 1) * cs.bs
    rot = np.asarray([(int(s) * int(t_off) + int(p)) % cs.fo for s, p in zip(shift, phase)], np.float64)
    Zs = OFFSET + (Z[:, a:b] - OFFSET) * np.exp(-2j * np.pi * rot / cs.fo)[:, None]
    return Zs, delta[:, a:b]


# ------------------------------------------------------------------------------------------ closed loop
# One channel of the default plan, two bursts of one payload on it, both LOOP_CFO Hz above the channel's centre (on top
# of the +25 and +45 Hz synth_wideband draws for these seeds); chunks of 8192 outputs, fed with two in flight: the message
# of burst A (in chunk 1, reported with chunk 2) is read while chunk 3 is in flight, so the retune asked for then holds
# from chunk 4 on, where burst B lies.
# LOOP_CFO: the demodulator slices the discriminator's sign and the deviation is +-4.8 kHz, so a burst further off than
# that cannot be received at all (at +-9 kHz the float64 model and the dsp oracle find no CRC-valid message, at 4.5 kHz
# both); 4 kHz leaves the device's bytes, one step from the model's at most, some room.
LOOP_B = 8192
LOOP_NK = 6
LOOP_CHANNEL = 25
LOOP_CFO = 4000
LOOP_SEEDS = (29, 4)        # bursts at outputs 9747 and 37509
LOOP_RETUNE_CHUNK = 4


@functools.lru_cache(maxsize=None)
def loop_capture():
    f = CZ.US_CHANNELS_HZ[LOOP_CHANNEL] - CENTRE
    payload = synth.payload_of(LOOP_SEEDS[0])
    raw, info = synth.synth_wideband(LOOP_SEEDS, [f + LOOP_CFO, f + LOOP_CFO], LOOP_NK * LOOP_B, payloads=[payload, payload])
    plan = SimpleNamespace()
    CZ.plan_channels(plan, [CZ.US_CHANNELS_HZ[LOOP_CHANNEL]], CENTRE, CZ.DEFAULT_DECIM, None, 3.0, CZ.OUT_RATE)
    return SimpleNamespace(raw=raw, info=info, payload=payload, plan=plan, chans=[CZ.US_CHANNELS_HZ[LOOP_CHANNEL]],
                           step=2 * LOOP_B * CZ.DEFAULT_DECIM)


def loop_messages(blocks):
    """The dsp oracle's parse of one channel's blocks: [(call, index, freq_err)] of the CRC-valid messages."""
    from oracle import dsp_oracle as O
    cfg = O.OracleConfig(19200, 14, 16, 80, PREAMBLE, LOOP_B)
    return [(k, r[0], r[4]) for k, rows in enumerate(O.parse_calls(blocks, cfg)) for r in rows if r[2]]


def loop_model_blocks(lc, schedule):
    """The model's channelized blocks (quantised) of the loop capture under {chunk: offset}."""
    from oracle import channelizer_oracle as CHO
    fo = CZ.OUT_RATE
    shift, phase, blocks = [int(lc.plan.shift_hz[0])], [0], []
    zs = {}
    for k in range(LOOP_NK):
        if k in schedule:
            new = [int(lc.plan.shift_hz[0]) + int(schedule[k])]
            phase = next_phase(phase, shift, new, k * LOOP_B, fo)
            shift = new
        if shift[0] not in zs:
            zs[shift[0]] = CHO.channelize_z(lc.raw, shift, lc.plan.taps, CZ.DEFAULT_DECIM, fo, 3.0)
        Z = OFFSET + (zs[shift[0]][:, k * LOOP_B: (k + 1) * LOOP_B] - OFFSET) * np.exp(-2j * np.pi * phase[0] / fo)
        blocks.append(CHO.quantise(Z)[0])
    return blocks
