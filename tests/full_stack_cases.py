"""Helpers shared by tests/test_full_stack_cpu.py and tests/test_wideband_full_stack.py (no tests in here): the two
configurations at which a WidebandReceiver runs with every per-chunk feature switched on at once - per-channel gain,
retune, levels, spectrum, the device-side parse, burst detection with per-chunk thresholds, burst decode, CRC repair, the
narrow-band filter, expected-slot decode and burst quality -, their captures, the schedule of changes made with two
chunks in flight, and compose(): what every accessor must return, put together from the models the suite already has
(gain_cases, retune_cases, spectrum_model, stream_parse_helpers, burst_cases, burst_narrow_cases, burst_track_cases,
burst_quality_cases).  No model is written here.  Nothing here touches a device.

small   burst_decode_cases.device_receiver(2048): "s16", decim 4, the default 512 taps, 3 channels, nW = 16.  The capture
        is device_capture()'s 9 chunks as they are, then 3 chunks made here in the same way (TAIL): device_capture has no
        packet that ends within SL outputs of a multiple of 2048 and none with a damaged symbol, so on it alone step 7
        never drops a record and repair never acts.  The tail plants one burst whose packet ends at the boundary 10 | 11
        with the next transmission right behind it (so that chunk 11's first window is ON and its run looks back), and
        one with two weak wrong symbols inside chunk 11.  device_capture's bursts lie 20 .. 90 kHz off their channels'
        centres, outside the demodulator's +-4.8 kHz, so the retune moves channel 0 by -30 kHz, onto its second burst
        (chunk 7): the one way parsed() and burst_messages() come to hold the same packet here.  The other two channels
        move by +700 and -1500 Hz.  The retune (with a gain change of every channel) is made before chunk 4, not 3: the
        one packet of device_capture that straddles a chunk boundary straddles 3 | 4.
wide    "u8", 70 channels (two row-block groups of k_channelize, the last part-filled; n_ch > 64 and no multiple of 16),
        block_size 2048, symbol length 14, 5 chunks.  decim 8 with 128 taps (channelizer.design_taps(128) at the
        capture's rate: cut-off 110 kHz, a transition of about 70 kHz): at decim 4 the capture is 1.08 MHz wide and every
        channel's pass band holds one of three carriers spread over it, so no channel is free of bursts; decim 8 is the
        next legal value.  128 taps keep the transition inside the 260 kHz by which every noise channel keeps off the
        carriers; the float64 model of all 70 channels takes well under a second.  Bursts on channels 0 (-700 kHz),
        33 (+50 kHz) and 69 (+700 kHz), on the channels' centres within 1 kHz, so the demodulator reads them too.  The
        capture is the signal synth.synth_wideband defines (32 lead-in symbols, the packet, 8 trailing zeros, +-4.8 kHz
        about the carrier, white noise, the same quantiser), written out in _synth because synth_wideband draws every
        start from a range that is empty below 16384 outputs and cannot weaken a symbol.

Schedule (actions(), applied submit, submit, [actions], fetch, submit, ...): before chunk 0 distinct gains from
gain_cases.PALETTE, thresholds from a quiet chunk's floor, a table with one row per planted burst of the first chunks, one
idle row and one row on a channel that never holds a burst, and every switch; before chunk 2 a gain change of every
other channel, its thresholds scaled with the gain's square, and a new table; before chunk RETUNE_AT a retune of every
channel, a gain change of every channel and the thresholds scaled likewise.
Gains: PALETTE without 300 (0.25, 3, 40, 1 - a range of 160).  At 300 the noise alone clips, a quiet window's energy
is a third of a saturated one's, the threshold a floor gives (4 x the floor) is above anything a window can reach and no
run is ever ON: on the model the bursts of those channels are then found by their expectations alone.  At 0.25 a burst of
0.12 of full scale is 4 counts and still decodes, by run and by expectation.

What the float64 model alone gives (test_full_stack_cpu.py asserts the conditions and prints these counts):
                                                    small        wide
    burst_messages() records, on channels           6 (0 1 2)    5 (0 33 69)
    expected_messages() records                     7            6
    repaired records (either decoder)               2            2
    records with tau < 0 right after the retune     2            1
    dropped by step 7, its quality row with it      1            1
    quality rows, all INBAND with n_noise = 224     13           11
    CRC-valid parsed() rows, also a burst message   1, 1         4, 3
    worst exempt share of a chunk (cap 6 %)         0.84 %       1.88 %
"""
import functools
from types import SimpleNamespace

import numpy as np

import burst_cases as BC
import burst_decode_cases as DC
import burst_narrow_cases as NB
import burst_quality_cases as QC
import burst_repair_cases as RP
import burst_track_cases as TK
import chan_bound_fmt as CF
import gain_cases as GC
import retune_cases as RC
import spectrum_model as SM
from stream_parse_helpers import _oracle_expected
from rtldavis_amd import acquire, synth
from rtldavis_amd import channelizer as CZ
from rtldavis_amd.wideband import BURST_THRESHOLD_OFF

NAMES = ("small", "wide")
SL, N_SYM = 14, 80
FO = 19200 * SL
IF_HZ = -FO // 4
BS = 2048
LEAD = 32 * SL                                               # a burst's lead-in, outputs
BURST_OUTPUTS = DC.BURST_OUTPUTS
GAINS = tuple(g for g in GC.PALETTE if g != 300.0)            # (0.25, 3.0, 40.0, 1.0): see the docstring
MAX_FLIPS, NARROW = 2, True
EXPECT_HALF = 50                                             # an expectation's window: +-50 outputs

# ------------------------------------------------------------------------------------------ the signal of synth_wideband
def _synth(fmt, decim, n_out, bursts, seed, amplitude=0.12, noise=0.02):
    """synth.synth_wideband's signal with every start given instead of drawn: ``bursts`` = (Hz off the capture's centre,
    first output, on-air bytes or hex, {packet symbol: factor of its deviation})."""
    fw = decim * FO
    n = n_out * decim
    rng = np.random.default_rng(seed)
    x = noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for hz, start, payload, scale in bursts:
        bits = synth.packet_bits(payload) if isinstance(payload, str) else np.unpackbits(np.frombuffer(bytes(payload), np.uint8))
        sym = np.concatenate([np.tile(np.array([1, 0], np.uint8), 16), bits, np.zeros(8, np.uint8)])
        dev = np.where(sym == 1, 4800.0, -4800.0)
        for k, f in scale.items():
            dev[32 + k] *= f
        freq = float(hz) + np.repeat(dev, SL * decim)
        lo = start * decim
        assert 0 <= lo and lo + freq.size <= n
        x[lo: lo + freq.size] += amplitude * np.exp(2j * np.pi * (float(hz) * lo + np.cumsum(freq)) / fw)
    dtype, scale_, offset = {"u8": (np.uint8, 127.6, 127.4), "s16": (np.int16, 32768.0, 0.0)}[fmt]
    lim = np.iinfo(dtype)
    out = np.empty(2 * n, dtype)
    out[0::2] = np.clip(np.rint(x.real * scale_ + offset), lim.min, lim.max)
    out[1::2] = np.clip(np.rint(x.imag * scale_ + offset), lim.min, lim.max)
    return out


@functools.lru_cache(maxsize=None)
def weak_packet():
    """A CRC-valid packet whose symbols 41 and 66 are lonely (burst_repair_cases.lonely): sent weak and wrong, they stay
    wrong at every tau, so the packet has no exact candidate and decodes with two flips."""
    return RP.find_packet(N_SYM, lambda b: RP.lonely(b, 41) and RP.lonely(b, 66), 5000)


WEAK = {41: -0.5, 66: -0.6}                                  # (burst_repair_cases.CAP_BURSTS' two-flip burst)

# small: the tail behind device_capture()'s 18432 outputs - (channel, payload, first output, weak symbols).  The first
# burst's packet ends SMALL_SEAM_J outputs past 22528 - 14 (the boundary 10 | 11), the lag of the channel filter included.
SMALL_LAG = DC.SEAM_LAG
SMALL_SEAM_J = 16
SMALL_TAIL_CHUNKS = 3
SMALL_SEAM_AT = 11 * BS - SL + SMALL_SEAM_J - (LEAD + N_SYM * SL) - SMALL_LAG
SMALL_TAIL = ((1, DC.VALID[1], SMALL_SEAM_AT, {}),
              (1, DC.VALID[2], SMALL_SEAM_AT + BURST_OUTPUTS, {}),      # the next transmission: chunk 11's window 0 is ON
              (2, None, 11 * BS + 150, WEAK))
SMALL_RETUNE = (-30000, 700, -1500)                          # channel 0: onto its burst at output 14000
# wide: (channel, payload, first output, weak symbols); the packet of the third ends WIDE_SEAM_J outputs past 6144 - 14
WIDE_DECIM, WIDE_TAPS, WIDE_NK, WIDE_NCH = 8, 128, 5, 70
WIDE_LAG = 8                                                 # (127 / 2) / 8 outputs
WIDE_SEAM_J = 16
WIDE_CARRIERS = {0: -700000, 33: 50000, 69: 700000}          # Hz off the capture's centre: the channels' centres
WIDE_CFO = {0: 420, 33: -610, 69: 250}                       # a transmitter's own error, Hz
WIDE_SEAM_AT = 3 * BS - SL + WIDE_SEAM_J - (LEAD + N_SYM * SL) - WIDE_LAG
WIDE_BURSTS = ((0, DC.VALID[0], 150, {}),                    # inside chunk 0
               (69, DC.VALID[2], 2200, {}),                  # inside chunk 1
               (33, DC.VALID[1], WIDE_SEAM_AT, {}),          # ends at 2 | 3
               (33, DC.VALID[0], WIDE_SEAM_AT + BURST_OUTPUTS, {}),     # the next transmission: chunk 3's window 0 is ON
               (69, None, 3 * BS + 160, WEAK),               # wholly inside chunk 3, the first after the retune
               (0, DC.VALID[1], 4 * BS + 200, {}))           # inside chunk 4
WIDE_KEEP_OFF = 260000                                       # a noise channel's centre keeps this far from every carrier


def _payload(p):
    return bytes(weak_packet()) if p is None else bytes.fromhex(p)


def _wide_channels():
    rng = np.random.default_rng(7070)
    fw = WIDE_DECIM * FO
    chans = []
    while len(chans) < WIDE_NCH:
        c = len(chans)
        if c in WIDE_CARRIERS:
            chans.append(WIDE_CARRIERS[c])
            continue
        f = int(rng.integers(-fw // 2 + FO, fw // 2 - FO))
        if all(abs(f - x) > WIDE_KEEP_OFF for x in WIDE_CARRIERS.values()) and f not in chans:
            chans.append(f)
    return chans


@functools.lru_cache(maxsize=None)
def config(name):
    """Everything of one configuration: the fields of retune_cases.case (so that gain_cases.chunk_model and
    retune_cases.tunings take it), the planted bursts as (channel, on-air bytes, first output, Hz off the channel's
    constructed centre), a chunk of noise alone, the spectrum size, the noise gaps and the chunk of the retune."""
    if name == "small":
        fmt, decim, user_taps, n_bins, retune_at = DC.DEV_FORMAT, DC.DEV_DECIM, None, 64, 4
        offs = list(DC.DEV_OFFSETS_HZ)
        quiet, stream = DC.device_capture()
        nk0 = DC.DEV_OUTPUTS // BS
        tail = _synth(fmt, decim, SMALL_TAIL_CHUNKS * BS,
                      [(offs[c] + DC.DEV_PLANTED[c], s - nk0 * BS, _payload(p), w) for c, p, s, w in SMALL_TAIL], 4242)
        raw = np.concatenate([stream, tail])
        quiet = quiet[: 2 * decim * BS]
        planted = [(c, _payload(p), s, DC.DEV_PLANTED[c]) for c, p, s in DC.DEV_BURSTS if p != DC.TWIN]
        planted += [(c, _payload(p), s, DC.DEV_PLANTED[c]) for c, p, s, _ in SMALL_TAIL]
        lag, retune = SMALL_LAG, np.asarray(SMALL_RETUNE, np.int64)
        no_burst = None                                      # every channel holds a burst: the row sits where none is
        late = {}
        model_rows = [0, 1, 2]
    else:
        fmt, decim, n_bins, retune_at = "u8", WIDE_DECIM, 2048, 3
        offs = _wide_channels()
        user_taps = CZ.design_taps(WIDE_TAPS, wide_rate=float(decim * FO))
        raw = _synth(fmt, decim, WIDE_NK * BS,
                     [(WIDE_CARRIERS[c] + WIDE_CFO[c], s, _payload(p), w) for c, p, s, w in WIDE_BURSTS], 7171)
        quiet = _synth(fmt, decim, BS, [], 7172)
        planted = [(c, _payload(p), s, WIDE_CFO[c]) for c, p, s, _ in WIDE_BURSTS]
        lag = WIDE_LAG
        rng = np.random.default_rng(7173)
        retune = (rng.integers(300, 2001, WIDE_NCH) * rng.choice([-1, 1], WIDE_NCH)).astype(np.int64)
        retune[[0, 33, 69]] = (-900, 1400, 500)              # (the bursts stay within 2.1 kHz of the tuned centres)
        no_burst = 12
        # the window of the burst at 2 | 3 begins at the first position chunk 2 cannot take (its packet would end in chunk
        # 3), so only chunk 3 - submitted right after the retune - finds it, looking back: a delivered record with tau < 0
        late = {WIDE_SEAM_AT: 3 * BS - SL * (N_SYM - 1)}
        model_rows = [0, 33, 69, 1, 34, 68]
    chans = [int(RC.CENTRE + f) for f in offs]
    plan = SimpleNamespace()
    CZ.plan_channels(plan, chans, RC.CENTRE, decim, user_taps, 3.0, FO)
    nk = raw.size // (2 * decim * BS)
    assert raw.size == nk * 2 * decim * BS
    n_ch = len(chans)
    ia = np.arange(n_ch) % len(GAINS)
    subset = np.arange(n_ch) % 2 == 0
    ib = np.where(subset, (ia + 1) % len(GAINS), ia)
    ic = (ib + 2) % len(GAINS)
    pal = np.asarray(GAINS, np.float64)
    return SimpleNamespace(name="full_stack_" + name, short=name, fmt=fmt, n_ch=n_ch, decim=decim, taps=plan.taps, user_taps=user_taps,
                           bs=BS, sl=SL, nk=nk, fo=FO, fw=FO * decim, chans=chans, plan_shift=plan.shift_hz.copy(), gain=3.0,
                           raw=raw, chunks=DC.chunks_of(raw, BS, decim), cfg=RC.packet_config(BS, SL), quiet=quiet,
                           planted=planted, lag=lag, retune=retune, retune_at=retune_at, subset=subset,
                           gains={0: pal[ia], 2: pal[ib], retune_at: pal[ic]}, n_bins=n_bins, gap=16, other_gap=300,
                           no_burst=no_burst, model_rows=model_rows, late=late)


def receiver(cfg):
    from rtldavis_amd import wideband
    return wideband.WidebandReceiver(cfg.cfg, cfg.chans, RC.CENTRE, decim=cfg.decim, taps=cfg.user_taps, gain=cfg.gain,
                                     sample_format=cfg.fmt)


# ------------------------------------------------------------------------------------------ the schedule
def first_symbol_end(cfg, start):
    """The absolute output at which the first symbol of a packet ends whose burst begins at output ``start``."""
    return start + LEAD + SL - 1 + cfg.lag


def expect_table(cfg, bursts, retuned, extra=True):
    """One row per burst of ``bursts`` (entries of cfg.planted): +-EXPECT_HALF outputs around the end of its first symbol,
    sliced around its carrier in the channel's bytes - ``retuned``: as the channel is tuned from the retune on -, then
    (``extra``) an idle row, whose window lies behind the capture's end, and a row where no burst is."""
    rows = []
    for c, _, s, hz in bursts:
        t = first_symbol_end(cfg, s)
        f = IF_HZ + hz - (int(cfg.retune[c]) if retuned and t >= cfg.retune_at * BS else 0)
        rows.append(TK.expect_row(c, cfg.late.get(s, t - EXPECT_HALF), t + EXPECT_HALF, TK.corr_of(f / FO)))
    if extra:
        rows.append(TK.expect_row(cfg.n_ch - 1, 10 ** 9, 10 ** 9 + 100, TK.corr_of(IF_HZ / FO)))        # idle in every chunk
        quiet_c, quiet_t = (cfg.no_burst, 3 * BS + 700) if cfg.no_burst is not None else quiet_place(cfg)
        rows.append(TK.expect_row(quiet_c, quiet_t - EXPECT_HALF, quiet_t + EXPECT_HALF, TK.corr_of(IF_HZ / FO)))
    return TK.table(rows)


def quiet_place(cfg):
    """small has a burst on every channel: the no-burst row lies on channel 1 in chunk 4, 2000 outputs from any burst."""
    return 1, 4 * BS + 1000


def tables(cfg):
    """{chunk: table}: before chunk 0 the bursts whose first symbol ends in chunks 0 .. 2, before chunk 2 those of the
    rest of the capture (the burst that straddles 2 | 3 is in both)."""
    t_of = lambda p: first_symbol_end(cfg, p[2])
    early = [p for p in cfg.planted if t_of(p) < 3 * BS]
    late = [p for p in cfg.planted if t_of(p) >= 2 * BS]
    return {0: expect_table(cfg, early, False), 2: expect_table(cfg, late, True)}


def scaled(thr, g_old, g_new):
    """Thresholds that follow a gain change: a window's energy goes with the gain's square."""
    t = np.asarray(thr, np.float64) * (np.asarray(g_new, np.float64) / np.asarray(g_old, np.float64)) ** 2
    return np.minimum(np.rint(t), BURST_THRESHOLD_OFF - 1).astype(np.uint64)


def thresholds_of(cfg, floor):
    """The thresholds before chunk 0 from the floor records of the quiet chunk received at the first gains."""
    return acquire.Acquisition(cfg.n_ch, cfg.cfg).thresholds(floor).astype(np.uint64)


def actions(cfg, thr0):
    """{chunk: [(method, argument)]} in the order they are applied, all between the same two submits."""
    g0, g2, g3 = cfg.gains[0], cfg.gains[2], cfg.gains[cfg.retune_at]
    tab = tables(cfg)
    thr2 = scaled(thr0, g0, g2)
    return {0: [("set_gain", g0), ("set_burst_threshold", np.asarray(thr0, np.uint64)), ("set_burst_expect", tab[0])],
            2: [("set_gain", g2), ("set_burst_threshold", thr2), ("set_burst_expect", tab[2])],
            cfg.retune_at: [("retune", cfg.retune), ("set_gain", g3), ("set_burst_threshold", scaled(thr2, g2, g3))]}


SWITCHES_NEED_QUIET = ("set_levels", "set_spectrum", "set_parse", "set_bursts", "set_burst_decode", "set_burst_repair",
                       "set_burst_narrow", "set_burst_quality")


def switch_on(rx, cfg, gap=None):
    """Every switch, on a quiet receiver (each of them refuses a receiver with chunks in flight)."""
    rx.set_levels(True)
    rx.set_spectrum(cfg.n_bins)
    rx.set_parse(True)
    rx.set_bursts(True)
    rx.set_burst_decode(True)
    rx.set_burst_repair(MAX_FLIPS)
    rx.set_burst_narrow(NARROW)
    rx.set_burst_quality(True, cfg.gap if gap is None else gap)


def apply(rx, acts):
    for method, arg in acts:
        getattr(rx, method)(arg)


def in_force(cfg, sched, nk=None):
    """Per chunk what its submit saw: dict(gains (float32 values as float64), thr, table, tuning (shift, phase))."""
    nk = cfg.nk if nk is None else nk
    g = np.full(cfg.n_ch, cfg.gain)
    thr = np.full(cfg.n_ch, BURST_THRESHOLD_OFF, np.uint64)
    tab = TK.table([])
    retunes = {k: arg for k, acts in sched.items() for m, arg in acts if m == "retune"}
    tun = RC.tunings(SimpleNamespace(plan_shift=cfg.plan_shift, n_ch=cfg.n_ch, nk=nk, bs=BS, fo=FO), retunes)
    out = []
    for k in range(nk):
        for m, arg in sched.get(k, ()):
            if m == "set_gain":
                g = np.asarray(arg, np.float32).astype(np.float64)
            elif m == "set_burst_threshold":
                thr = np.asarray(arg, np.uint64)
            elif m == "set_burst_expect":
                tab = arg
        out.append(dict(gains=np.asarray(g, np.float32).astype(np.float64), thr=thr, table=tab, tuning=tun[k]))
    return out


# ------------------------------------------------------------------------------------------ the float64 model's bytes
@functools.lru_cache(maxsize=None)
def _z1(name, which, shift):
    """The model in front of the quantiser at gain 1, all channels, of the capture or of the quiet chunk."""
    cfg = config(name)
    raw = cfg.raw if which == "raw" else cfg.quiet
    return CF.model_z(raw, cfg.fmt, np.asarray(shift, np.int64), cfg.taps, cfg.decim, FO, 1.0)


def _quantised(z1, gains, phase):
    """The model in front of the quantiser at the gains and the phase accumulators of a tuning (retune_cases' rotation)."""
    rot = np.exp(-2j * np.pi * np.asarray([int(p) % FO for p in phase], np.float64) / FO)
    return RC.OFFSET + (z1 - RC.OFFSET) * (np.asarray(gains, np.float64) * rot)[:, None]


def model_blocks(cfg, sched):
    """The float64 model's channelized chunks (quantised) under the schedule, all channels."""
    from oracle import channelizer_oracle as CHO
    out = []
    for k, f in enumerate(in_force(cfg, sched)):
        shift, phase = f["tuning"]
        z = _z1(cfg.short, "raw", tuple(shift))[:, k * BS: (k + 1) * BS]
        out.append(CHO.quantise(_quantised(z, f["gains"], phase)))
    return out


def model_quiet_floor(cfg, gains):
    """The floor records of the quiet chunk at the first gains, with no window ON: the model's side of thresholds_of."""
    from oracle import channelizer_oracle as CHO
    z = _z1(cfg.short, "quiet", tuple(int(s) for s in cfg.plan_shift))
    return BC.model_bursts(CHO.quantise(_quantised(z, gains, [0] * cfg.n_ch)), BURST_THRESHOLD_OFF, 0).floor


def sub_case(cfg):
    """The rows of cfg.model_rows as a case of their own, registered with retune_cases so that gain_cases.chunk_model
    finds it by name: the float64 model and its bound are per channel, so a subset's are the whole plan's rows."""
    rows = cfg.model_rows
    sub = SimpleNamespace(**vars(cfg))
    sub.name, sub.n_ch = cfg.name + "_rows", len(rows)
    sub.chans = [cfg.chans[c] for c in rows]
    sub.plan_shift = cfg.plan_shift[rows].copy()
    RC.EXTRA[sub.name] = sub
    return sub


def channel_models(cfg, sched):
    """Per chunk (rows, Z, delta): gain_cases.chunk_model under retune_cases.tunings for the channels of cfg.model_rows."""
    sub = sub_case(cfg)
    rows = cfg.model_rows
    out = []
    for k, f in enumerate(in_force(cfg, sched)):
        shift, phase = f["tuning"]
        Z, delta = GC.chunk_model(sub, k, [shift[c] for c in rows], [phase[c] for c in rows], f["gains"][rows])
        out.append((rows, Z, delta))
    return out


# ------------------------------------------------------------------------------------------ compose
def compose(cfg, run, sched, gaps=None, channel_model=True, clock0=0):
    """What every accessor must return for a run that delivered, per chunk, dict(block = channelized bytes [n_ch, 2 B],
    bursts = the Bursts, chunk = the capture chunk submitted): per chunk a dict of
        channelized   (rows, Z, delta) for chan_bound.check_against_model          (None without ``channel_model``)
        levels        (gain_cases.channel_levels(block), float32 gains, gain_cases.input_levels(chunk))
        spectrum      (P, segments, tol) of spectrum_model
        parsed        [(row, x)] of stream_parse_helpers._oracle_expected, for assert_rows_match
        thr           the thresholds for burst_cases.assert_equals_model(bursts, block, thr, chunk)
        messages      BurstMessages: burst_narrow_cases.decode_stream on the blocks and the given burst records
        expected      ExpectedMessages: burst_track_cases.expect_stream under the table in force
        quality       (rows parallel to messages.records, rows parallel to expected.records) of burst_quality_cases
    ``gaps``: the noise gap per chunk (default cfg.gap for all)."""
    nk = len(run)
    force = in_force(cfg, sched, nk)
    blocks = [np.asarray(r["block"]) for r in run]
    gaps = [cfg.gap] * nk if gaps is None else gaps
    models = channel_models(cfg, sched) if channel_model else [None] * nk
    parsed = _oracle_expected([[b[c] for b in blocks] for c in range(cfg.n_ch)], BS)
    decoded = NB.decode_stream(blocks, None, cfg.cfg, MAX_FLIPS, NARROW, clock0=clock0, bursts=[r["bursts"] for r in run])
    expected = TK.expect_stream(blocks, [f["table"] for f in force], cfg.cfg, MAX_FLIPS, NARROW, clock0=clock0)
    out = []
    for k in range(nk):
        prev = blocks[k - 1] if k else None
        p, s = SM.model(run[k]["chunk"], cfg.fmt, cfg.n_bins)
        m, x = decoded[k][1], expected[k]
        out.append(dict(channelized=models[k],
                        levels=(GC.channel_levels(blocks[k]), force[k]["gains"].astype(np.float32), GC.input_levels(run[k]["chunk"], cfg.fmt)),
                        spectrum=(p, s, SM.tol(p, cfg.n_bins)), parsed=parsed[k], thr=force[k]["thr"], messages=m, expected=x,
                        quality=(QC.quality_rows(blocks[k], prev, cfg.cfg, m.records, gaps[k], k),
                                 QC.quality_rows(blocks[k], prev, cfg.cfg, x.records, gaps[k], k))))
    return out


def undropped(cfg, run, clock0=0):
    """Per chunk the BurstMessages without step 7 (decode_model alone): a record here and not in compose()'s messages
    was dropped as a repeat."""
    blocks = [np.asarray(r["block"]) for r in run]
    return [NB.decode_model(blocks[k], blocks[k - 1] if k else None, run[k]["bursts"], cfg.cfg, k >= 1, clock0 + k * BS,
                            MAX_FLIPS, NARROW) for k in range(len(run))]


def model_run(cfg):
    """(run, sched) on the float64 model alone: the bytes of model_blocks, the model's Bursts under the thresholds in
    force, thresholds from the model's quiet floor."""
    thr0 = thresholds_of(cfg, model_quiet_floor(cfg, cfg.gains[0]))
    sched = actions(cfg, thr0)
    force = in_force(cfg, sched)
    blocks = model_blocks(cfg, sched)
    return [dict(block=b, bursts=BC.model_bursts(b, force[k]["thr"], k), chunk=cfg.chunks[k]) for k, b in enumerate(blocks)], sched


def counts(cfg, run, want):
    """The figures the non-vacuity conditions are about, from compose()'s result (or a device's records in its shape)."""
    msgs = [r for w in want for r in w["messages"].records]
    exps = [r for w in want for r in w["expected"].records]
    plain = undropped(cfg, run)
    dropped = sum(p.records.size for p in plain) - len(msgs)
    qual = [q for w in want for part in w["quality"] for q in part]
    parsed_ota = {(row[0], row[5]) for w in want for row, _ in w["parsed"]}
    both = [r for r in msgs if (int(r["channel"]), bytes(r["data"]).hex()) in parsed_ota]
    after = want[cfg.retune_at]
    return dict(messages=len(msgs), message_channels=sorted({int(r["channel"]) for r in msgs}), expected=len(exps),
                repaired=sum(1 for r in msgs + exps if int(r["flags"]) & RP.REPAIRED), dropped=dropped,
                lookback_after_retune=sum(1 for r in list(after["messages"].records) + list(after["expected"].records) if int(r["tau"]) < 0),
                quality_rows=len(qual), inband=sum(1 for q in qual if int(q["flags"]) == QC.INBAND),
                with_noise=sum(1 for q in qual if int(q["n_noise"]) > 0), parsed=len(parsed_ota), in_both=len(both))
