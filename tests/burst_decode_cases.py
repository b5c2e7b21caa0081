"""Helpers shared by tests/test_wideband_burst_decode_cpu.py and tests/test_wideband_burst_decode.py (no tests in here):
the model of k_chan_burst_decode in NumPy int64 and Python integers, written from the definition
(include/rtldavis_hip.h, BURST DECODE) and not from the kernel - it forms d[t] sample by sample and s[t] as its running
sum, where the kernel multiplies the correlation sum into window sums of p -; the chunk-by-chunk driver that stands for
a receiver; and the captures of the device tests.  Nothing here touches a device."""
import functools

import numpy as np

import burst_cases as BC
import retune_cases as RC
from rtldavis_amd import synth
from rtldavis_amd.wideband import BURST_MSG_DTYPE, BurstMessages

W = 128
MAX_W = 32


def shape(cfg):
    """(SL, N, sync bits, LOOK) of a packet configuration."""
    sl, n = int(cfg.symbol_length), int(cfg.packet_symbols)
    sync = [int(ch) for ch in cfg.preamble]
    assert len(sync) == 16 and n % 8 == 0 and n >= 40 and n * sl + 1 <= 2048
    return sl, n, sync, W * (-(-(n * sl + 1) // W))


def _crc_ok(data):
    """The CRC gate of rd_parse_packet: CRC-16-CCITT over the bit-swapped bytes [2:] is 0."""
    return synth._crc16_ccitt(bytes(synth._swap_bits8(b) for b in data[2:])) == 0


def decode_run(cur, prev, rec, cfg, have_prev):
    """Steps 2 .. 6 of the definition for one channel's bytes (uint8 [2 B]; prev: the chunk before or None) and one
    burst record of at most MAX_W windows: None, or (tau, flags, margin, f_re, f_im, data, ones, id)."""
    sl, n, sync, look = shape(cfg)
    cre, cim = int(rec["corr_re"]), int(rec["corr_im"])
    if cre == 0 and cim == 0:
        return None
    back = bool(int(rec["flags"]) & 1) and have_prev
    t0 = W * int(rec["first"]) - (look if back else 0)
    t1 = W * (int(rec["first"]) + int(rec["windows"]))
    if t1 - t0 < n * sl + 1:
        return None
    B = cur.size // 2
    b = np.concatenate([prev, cur]).astype(np.int64) if back else cur.astype(np.int64)
    org = B if back else 0                                   # index of t = 0
    a = 2 * b - 255
    ai, aq = a[0::2], a[1::2]
    t = np.arange(t0 + 1, t1)
    zi, zq, wi, wq = ai[org + t], aq[org + t], ai[org + t - 1], aq[org + t - 1]
    p_re, p_im = zi * wi + zq * wq, zq * wi - zi * wq        # z[t] conj(z[t-1]), t0 < t < t1
    assert max(np.abs(p_re).max(), np.abs(p_im).max()) < 2 ** 18
    d = p_im * cre - p_re * cim                              # |d| < 2^48: int64 is exact
    cs = np.concatenate([[0], np.cumsum(d)])                 # cs[j] = sum d[t0 + 1 .. t0 + j]
    s_of = lambda tt: cs[tt - t0] - cs[tt - t0 - sl]         # s[t] = d[t - sl + 1] + .. + d[t], t0 + sl <= t < t1
    taus = np.arange(t0 + sl, t1 - sl * (n - 1))
    taus = taus[taus + sl * (n - 1) >= 0]
    if taus.size == 0:
        return None
    s = s_of(taus[:, None] + sl * np.arange(n)[None, :])     # [candidates, N]
    bits = (s > 0).astype(np.uint8)
    best = None
    for j in np.flatnonzero(np.all(bits[:, :16] == np.asarray(sync, np.uint8), axis=1)):
        data = bytes(np.packbits(bits[j]))
        if not _crc_ok(data):
            continue
        margin = int(np.abs(s[j]).min())
        if best is None or margin > best[2]:                 # (ascending tau: a tie keeps the smaller)
            best = (int(taus[j]), 1 if back else 0, margin, j, data, int(bits[j].sum()))
    if best is None:
        return None
    tau, flags, margin, j, data, ones = best
    tt = np.arange(tau - sl + 1, tau + sl * (n - 1) + 1) - (t0 + 1)
    assert tt.size == n * sl and tt[0] >= 0
    return tau, flags, margin, int(p_re[tt].sum()), int(p_im[tt].sum()), data, ones, synth._swap_bits8(data[2]) & 7


def decode_model(cur, prev, bursts, cfg, have_prev, clock):
    """The BurstMessages of one chunk: ``cur`` / ``prev`` channelized bytes uint8 [n_channels, 2 B] (prev None: no chunk
    before), ``bursts`` the chunk's Bursts (records in channel and run order), ``clock`` the absolute time of its first
    output."""
    cur = np.atleast_2d(cur)
    long_runs = np.zeros(cur.shape[0], np.uint32)
    rows = []
    for rec in bursts.records:
        c = int(rec["channel"])
        if int(rec["windows"]) > MAX_W:
            long_runs[c] += 1
            continue
        got = decode_run(cur[c], None if prev is None else np.atleast_2d(prev)[c], rec, cfg, have_prev)
        if got is None:
            continue
        tau, flags, margin, f_re, f_im, data, ones, ident = got
        rows.append((c, int(rec["first"]), tau, flags, (int(clock) + tau) % 2 ** 64, margin, f_re, f_im,
                     list(data) + [0] * (10 - len(data)), ones, ident, [0, 0, 0, 0]))
    return BurstMessages(np.asarray(rows, BURST_MSG_DTYPE).reshape(-1), long_runs, int(bursts.chunk))


def decode_stream(blocks, thr, cfg, clock0=0):
    """A receiver in NumPy: per chunk (channelized bytes [n_channels, 2 B], in order from a reset) the model's Bursts
    under the thresholds ``thr`` and the model's BurstMessages."""
    out, prev = [], None
    for k, block in enumerate(blocks):
        block = np.atleast_2d(block)
        b = BC.model_bursts(block, thr, k)
        out.append((b, decode_model(block, prev, b, cfg, k >= 1, clock0 + k * (block.shape[1] // 2))))
        prev = block
    return out


def assert_equals_model(got, want):
    """A receiver's BurstMessages against the model's: every field of every record, long_runs and chunk."""
    assert got.chunk == want.chunk
    assert got.records.dtype == BURST_MSG_DTYPE and got.long_runs.dtype == np.uint32
    assert np.array_equal(got.long_runs, want.long_runs), (got.chunk, got.long_runs, want.long_runs)
    assert got.records.shape == want.records.shape, (got.chunk, got.records, want.records)
    for f in BURST_MSG_DTYPE.names:
        assert np.array_equal(got.records[f], want.records[f]), (got.chunk, f, got.records[f], want.records[f])


def rechunk(blocks, bs):
    """The same channelized stream in chunks of ``bs`` outputs."""
    whole = np.concatenate([np.atleast_2d(b) for b in blocks], axis=1)
    assert whole.shape[1] % (2 * bs) == 0
    return [whole[:, 2 * bs * k: 2 * bs * (k + 1)] for k in range(whole.shape[1] // (2 * bs))]


def drawn_cfo(seed, n_out):
    """The cfo synth_wideband(..., n_out) draws for burst ``seed`` (its third draw: payload, start, cfo)."""
    r = np.random.default_rng(seed)
    r.integers(0, len(synth.OTA_PACKETS))
    r.integers(synth.BLOCK_SIZE, n_out - BURST_OUTPUTS - synth.BLOCK_SIZE)
    return float(r.uniform(-2000.0, 2000.0))


# ------------------------------------------------------------------------------------------ device captures
# Three channels at decim 4 (1.0752 MS/s) with the default 512 taps - which at this decimation only a 16-bit capture admits
# (rtldavis_hip.h: n_taps / decim), so the captures are "s16" -; bursts 30 kHz below, 20 kHz above and 90 kHz above their channels' centres, which
# puts the runs' correlation sums (the channel lies at -67.2 kHz in its bytes) at -130, -63 and +31 degrees: three quadrants.
DEV_DECIM = 4
DEV_FORMAT = "s16"
DEV_OFFSETS_HZ = (-300000, 0, 300000)
DEV_PLANTED = (-30000, 20000, 90000)
DEV_OUTPUTS = 18432                                          # 16 chunks of 1152, 9 of 2048, 4 of 4608
VALID = synth.OTA_PACKETS[4], synth.OTA_PACKETS[1], synth.OTA_PACKETS[2]
TWIN = synth.make_packet(3, bytes([0x50, 1, 2, 3, 4, 5]), flip_bit=17).hex()      # sync-valid, CRC-invalid
BURST_OUTPUTS = 120 * 14                                     # 32 lead-in symbols, 80 of the packet, 8 trailing
# (channel, payload, the stream output at which the burst begins)
DEV_BURSTS = (
    (0, VALID[0], -100),      # begins before the stream: ON from window 0 of the very first chunk, no chunk before it;
                              # the packet (outputs 348 .. 1468) lies inside chunk 0 of 2048 and crosses 1152
    (1, VALID[1], 4196),      # inside chunk 2 of 2048 (4096 .. 6143)
    (2, VALID[2], 7400),      # the packet (7848 .. 8968) crosses 8064 (7 x 1152) and 8192 (4 x 2048)
    (1, TWIN, 11000),         # the twin: found as a run, decoded by nobody
    (0, VALID[1], 14000),     # a second message on channel 0
)


def _piece(seed, shift_hz, payload, pre, post, decim=DEV_DECIM):
    """One burst of synth_wideband with ``pre`` outputs in front of its first output (negative: the piece begins inside
    the burst) and ``post`` behind its last: the raw bytes of those outputs."""
    n_out = 2 * synth.BLOCK_SIZE + BURST_OUTPUTS + 2048
    raw, info = synth.synth_wideband([seed], [shift_hz], n_out, decim=decim, noise_seed=seed + 77, payloads=[payload],
                                     sample_format=DEV_FORMAT)
    start = info[0][1]
    assert pre <= synth.BLOCK_SIZE and post <= synth.BLOCK_SIZE
    return raw[2 * decim * (start - pre): 2 * decim * (start + BURST_OUTPUTS + post)]


@functools.lru_cache(maxsize=None)
def device_capture():
    """(noise chunk source, stream): the wideband bytes of DEV_OUTPUTS outputs holding DEV_BURSTS, spliced from one
    synth_wideband capture per burst (white noise on both sides of every cut), and 4608 outputs of noise alone."""
    pieces, at = [], 0
    starts = [s for _, _, s in DEV_BURSTS] + [None]
    for j, (c, payload, s) in enumerate(DEV_BURSTS):
        end = DEV_OUTPUTS if starts[j + 1] is None else (s + BURST_OUTPUTS + starts[j + 1]) // 2   # cut half way to the next
        pieces.append(_piece(100 + j, DEV_OFFSETS_HZ[c] + DEV_PLANTED[c], payload, s - at, end - s - BURST_OUTPUTS))
        at = end
    stream = np.concatenate(pieces)
    assert stream.size == 2 * DEV_DECIM * DEV_OUTPUTS
    quiet = _piece(99, 0, VALID[0], 4608 + 100, -BURST_OUTPUTS - 100)
    assert quiet.size == 2 * DEV_DECIM * 4608
    return quiet, stream


def device_receiver(bs, symbol_length=14, decim=DEV_DECIM, offsets_hz=DEV_OFFSETS_HZ):
    from rtldavis_amd import wideband
    chans = [RC.CENTRE + f for f in offsets_hz]
    return wideband.WidebandReceiver(RC.packet_config(bs, symbol_length), chans, RC.CENTRE, decim=decim, sample_format=DEV_FORMAT)


def chunks_of(raw, bs, decim=DEV_DECIM):
    step = 2 * decim * bs
    assert raw.size % step == 0
    return [raw[step * k: step * (k + 1)] for k in range(raw.size // step)]


# symbol_length 8: 153600 outputs/s, a burst of 960 outputs, LOOK = 768.  synth_wideband plants 14 x decim samples per
# symbol, so the capture is made here, the same way: (payload, first output, Hz off the capture's centre) per burst.
S8_BS = 1024
S8_OUTPUTS = 6 * S8_BS
S8_OFFSETS_HZ = (-150000, 0, 150000)                        # (the capture is 614.4 kHz wide)
S8_BURSTS = ((VALID[0], 1024 + 300, S8_OFFSETS_HZ[1] + 20000),         # crosses 2048
             (TWIN, 3500, S8_OFFSETS_HZ[1] + 20000),
             (VALID[2], 4096 + 30, S8_OFFSETS_HZ[2] - 30000))          # inside chunk 4


@functools.lru_cache(maxsize=None)
def s8_capture(sl=8, decim=DEV_DECIM, amplitude=0.12, noise=0.02):
    fw = decim * 19200 * sl
    n = S8_OUTPUTS * decim
    rng = np.random.default_rng(808)
    x = noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for payload, start, hz in S8_BURSTS:
        sym = np.concatenate([np.tile(np.array([1, 0], np.uint8), 16), synth.packet_bits(payload), np.zeros(8, np.uint8)])
        chips = np.repeat(sym, sl * decim)
        lo = start * decim
        freq = float(hz) + np.where(chips == 1, 4800.0, -4800.0)
        x[lo: lo + chips.size] += amplitude * np.exp(2j * np.pi * np.cumsum(freq) / fw)
    out = np.empty(2 * n, np.int16)                          # "s16", as synth_wideband makes it
    out[0::2] = np.clip(np.rint(x.real * 32768.0), -32768, 32767)
    out[1::2] = np.clip(np.rint(x.imag * 32768.0), -32768, 32767)
    return out


def acq_plan(planted):
    """burst_cases.acq_capture with what the decode tests add: the drawn cfo of both bursts."""
    lc = BC.acq_capture(planted)
    return lc, [planted + drawn_cfo(s, RC.LOOP_NK * RC.LOOP_B) for s in RC.LOOP_SEEDS]
