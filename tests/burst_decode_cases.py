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


def drop_repeats(msgs, delivered, sl):
    """Step 7 of the definition, the host's: ``msgs`` without the records that report a packet again - a record with
    flags & 1 whose channel and data equal those of a record in ``delivered`` (what the fetch of the chunk before handed
    out) and whose time lies less than SL from that record's, on the 64-bit clock."""
    def again(r):
        for q in delivered:
            d = (int(r["time"]) - int(q["time"])) % 2 ** 64
            if q["channel"] == r["channel"] and bytes(q["data"]) == bytes(r["data"]) and min(d, 2 ** 64 - d) < sl:
                return True
        return False
    keep = [i for i, r in enumerate(msgs.records) if not (int(r["flags"]) & 1 and again(r))]
    return BurstMessages(msgs.records[keep], msgs.long_runs, msgs.chunk)


def decode_stream(blocks, thr, cfg, clock0=0, bursts=None):
    """A receiver in NumPy: per chunk (channelized bytes [n_channels, 2 B], in order from a reset) the model's Bursts
    under the thresholds ``thr`` (or the given ``bursts``, one per chunk) and the BurstMessages a fetch delivers:
    decode_model's, less the repeats of what the chunk before delivered (step 7)."""
    out, prev, delivered = [], None, ()
    for k, block in enumerate(blocks):
        block = np.atleast_2d(block)
        b = BC.model_bursts(block, thr, k) if bursts is None else bursts[k]
        m = decode_model(block, prev, b, cfg, k >= 1, clock0 + k * (block.shape[1] // 2))
        m = drop_repeats(m, delivered, int(cfg.symbol_length))
        out.append((b, m))
        prev, delivered = block, m.records
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


# ------------------------------------------------------------------------------------------ crafted bytes
# Inputs for k_chan_burst_decode alone (the hook rd_debug_burst_decode): FSK bursts written straight into channelized
# bytes, exact ties and exact offsets, and run records k_chan_bursts never writes.  Every case names the edge it is built
# for as a condition on the model of its own bytes, asserted when the case is built.
FILL = BC.FILL
THR = 200000          # between quiet_bytes (p_w <= 2304) and a window three quarters full of a burst of amplitude 40
AMP = 40


def config(sl, n, bs):
    from rtldavis_amd import dsp
    return dsp.PacketConfig(19200, sl, 16, n, RC.PREAMBLE, bs)


def packet(n, ident=1, seed=0, flip_bit=None):
    """On-air bytes of a CRC-valid packet of n symbols (sync word first), or its CRC-invalid twin."""
    body = bytes(np.random.default_rng(1000 + seed).integers(0, 256, n // 8 - 4, dtype=np.uint8))
    return synth.make_packet(ident, body, n_bytes=n // 8, flip_bit=flip_bit)


def deviation(sl):
    """A quarter turn per symbol, as 4.8 kHz at 19200 symbols/s, in cycles per output; 0.1 at most."""
    return min(0.1, 0.25 / sl)


def fsk_bytes(freqs, amp=AMP, phase0=0.0):
    """Quantised 127.5 + amp e^{j phi}, phase-continuous: output i advances phi by 2 pi freqs[i] (cycles per output)."""
    ph = phase0 + 2 * np.pi * np.cumsum(np.asarray(freqs, np.float64))
    out = np.empty(2 * ph.size, np.uint8)
    out[0::2] = np.clip(np.rint(127.5 + amp * np.cos(ph)), 0, 255)
    out[1::2] = np.clip(np.rint(127.5 + amp * np.sin(ph)), 0, 255)
    return out


def fsk_burst(data, sl, carrier=0.11, lead=64, trail=32, amp=AMP, dev=None, invert=False):
    """``lead`` outputs of carrier, the packet's symbols (1: carrier + deviation) and ``trail`` outputs of carrier.  The
    packet's symbol i lies at outputs lead + SL i .. lead + SL i + SL - 1 of the piece."""
    dev = deviation(sl) if dev is None else dev
    bits = np.repeat(np.unpackbits(np.frombuffer(bytes(data), np.uint8)), sl).astype(np.int64)
    sym = np.where(bits == (0 if invert else 1), dev, -dev)
    return fsk_bytes(np.concatenate([np.zeros(lead), sym, np.zeros(trail)]) + carrier, amp)


def put(row, at, piece):
    """Write a piece of bytes into a channel's row so that its first output is output ``at``."""
    assert at >= 0 and 2 * at + piece.size <= row.size
    row[2 * at: 2 * at + piece.size] = piece
    return row


def candidates(cur, prev, rec, cfg, have_prev):
    """Every candidate of step 5 for one run, ascending: [(tau, margin)] - what step 6 chooses among."""
    sl, n, sync, look = shape(cfg)
    back = bool(int(rec["flags"]) & 1) and have_prev
    t0 = W * int(rec["first"]) - (look if back else 0)
    t1 = W * (int(rec["first"]) + int(rec["windows"]))
    B = cur.size // 2
    a = 2 * (np.concatenate([prev, cur]) if back else cur).astype(np.int64) - 255
    zi, zq = a[0::2], a[1::2]
    org = B if back else 0
    out = []
    for tau in range(max(t0 + sl, -sl * (n - 1)), t1 - sl * (n - 1)):
        s = []
        for i in range(n):
            acc = 0
            for t in range(tau + sl * i - sl + 1, tau + sl * i + 1):
                pr = int(zi[org + t] * zi[org + t - 1] + zq[org + t] * zq[org + t - 1])
                pi = int(zq[org + t] * zi[org + t - 1] - zi[org + t] * zq[org + t - 1])
                acc += pi * int(rec["corr_re"]) - pr * int(rec["corr_im"])
            s.append(acc)
            if i < 16 and (acc > 0) != bool(sync[i]):
                break
        else:
            if _crc_ok(bytes(np.packbits([1 if v > 0 else 0 for v in s]))):
                out.append((tau, min(abs(v) for v in s)))
    return out


def runs_of(block, thr, chunk=0):
    """The burst slot's record places [n_ch][cap] and run counts of a chunk's bytes: the model's runs, FILL behind them."""
    block = np.atleast_2d(block)
    cs = BC.crafted("runs", list(block), thr, seq=chunk)
    recs, floor = BC.slot_model(cs)
    return recs, floor["n_bursts"].astype(np.uint32)


def slot_decode_model(cfg, cur, prev, runs, n_runs, clock, seq):
    """What rd_debug_burst_decode must hand back: the whole message slot [n_ch][cap] (a channel's messages first, FILL
    behind them), n_msgs, long_runs and chunk per channel.  The definition run by run, over the record places as given:
    at most cap of them; a run of more than MAX_W windows is counted; a record k_chan_bursts never writes (windows = 0,
    first >= nW, first + windows > nW) is skipped; the rest is decode_run."""
    cur = np.atleast_2d(cur)
    n_ch, n_win = cur.shape[0], cur.shape[1] // (2 * W)
    cap = BC.cap_of(n_win)
    assert runs.shape == (n_ch, cap)
    msgs = np.frombuffer(bytes([FILL]) * (n_ch * cap * BURST_MSG_DTYPE.itemsize), BURST_MSG_DTYPE).reshape(n_ch, cap).copy()
    n_msgs, long_runs = np.zeros(n_ch, np.uint32), np.zeros(n_ch, np.uint32)
    for c in range(n_ch):
        for rec in runs[c, : min(int(n_runs[c]), cap)]:
            first, windows = int(rec["first"]), int(rec["windows"])
            if windows > MAX_W:
                long_runs[c] += 1
                continue
            if windows == 0 or first >= n_win or first + windows > n_win:
                continue
            assert (int(rec["flags"]) & 1) == (1 if first == 0 else 0)       # (flags as k_chan_bursts writes them)
            got = decode_run(cur[c], None if prev is None else np.atleast_2d(prev)[c], rec, cfg, prev is not None)
            if got is None:
                continue
            tau, flags, margin, f_re, f_im, data, ones, ident = got
            msgs[c, n_msgs[c]] = (c, first, tau, flags, (int(clock) + tau) % 2 ** 64, margin, f_re, f_im,
                                  list(data) + [0] * (10 - len(data)), ones, ident, [0, 0, 0, 0])
            n_msgs[c] += 1
    return msgs, n_msgs, long_runs, np.full(n_ch, seq & 0xFFFFFFFF, np.uint32)


class Launch:
    """One launch of the hook: configuration, bytes (rows: one uint8 [2 B] per channel; prev alike or None), the run
    records (the model's of ``rows`` under THR unless given) and what the model expects back."""

    def __init__(self, name, cfg, rows, prev=None, runs=None, n_runs=None, clock=0, seq=0, thr=THR):
        self.name, self.cfg, self.clock, self.seq = name, cfg, clock, seq
        self.cur = np.ascontiguousarray(np.stack(rows), np.uint8)
        self.prev = None if prev is None else np.ascontiguousarray(np.stack(prev), np.uint8)
        assert self.cur.shape[1] == 2 * cfg.block_size and (self.prev is None or self.prev.shape == self.cur.shape)
        if runs is None:
            runs, n_runs = runs_of(self.cur, thr, seq & 0xFFFFFFFF)
        self.runs, self.n_runs = np.ascontiguousarray(runs), np.ascontiguousarray(n_runs, np.uint32)
        self.n_ch = self.cur.shape[0]
        self.msgs, self.n_msgs, self.long_runs, self.chunk = slot_decode_model(cfg, self.cur, self.prev, self.runs, self.n_runs, clock, seq)

    def records(self, c):
        return self.msgs[c, : int(self.n_msgs[c])]

    def candidates(self, c, r=0):
        return candidates(self.cur[c], None if self.prev is None else self.prev[c], self.runs[c, r], self.cfg, self.prev is not None)


def _quiet(seed, bs):
    return BC.quiet_bytes(np.random.default_rng(seed), bs)


@functools.lru_cache(maxsize=None)
def tie_launch():
    """Two byte-identical copies of one burst in one run, d outputs apart, the stretch between them carrier: two
    candidates with the same 64-bit margin, the record takes the smaller tau - from the same lane's next stride
    (d = 256), from another wave (d = 300), from further on (d = 1300); and with the later copy one step louder, the later."""
    sl, n, bs = 2, 40, 2048
    cfg = config(sl, n, bs)
    data = packet(n)
    piece = fsk_burst(data, sl, lead=8, trail=4)
    rows = []
    for c, (d, amp2) in enumerate(((256, AMP), (300, AMP), (1300, AMP), (300, AMP + 1))):
        row = put(_quiet(c, bs), 128, fsk_bytes(np.full(d + 300, 0.11)))            # carrier under and between the copies
        put(row, 170, piece)
        rows.append(put(row, 170 + d, fsk_burst(data, sl, lead=8, trail=4, amp=amp2)))
    L = Launch("ties", cfg, rows)
    for c, d in enumerate((256, 300, 1300)):
        cand = L.candidates(c)
        best = max(m for _, m in cand)
        taus = [t for t, m in cand if m == best]
        assert L.n_runs[c] == 1 and L.runs[c, 0]["windows"] <= MAX_W
        assert len(taus) >= 2 and taus[1] - taus[0] == d, (c, cand)
        assert L.n_msgs[c] == 1 and L.msgs[c, 0]["tau"] == taus[0] == 170 + 8 + sl - 1 and L.msgs[c, 0]["margin"] == best
        lanes = [(t - 128 - sl) % 256 for t in taus[:2]]                             # the kernel's thread for a tau
        assert (lanes[0] == lanes[1]) == (d == 256) and (d != 300 or lanes[0] // 64 != lanes[1] // 64)
    cand = L.candidates(3)
    best = max(m for _, m in cand)
    assert [t for t, m in cand if m == best] == [170 + 300 + 8 + sl - 1] and len(cand) >= 2
    assert L.n_msgs[3] == 1 and L.msgs[3, 0]["tau"] == 170 + 300 + 8 + sl - 1
    return L


@functools.lru_cache(maxsize=None)
def range_launch():
    """The ends of the candidate range, SL 2 (a tau one output off decodes nothing): the first symbol ends at t0 + SL and
    one output earlier; the last symbol ends at t1 - 1 and one output later."""
    sl, n, bs = 2, 80, 2048
    cfg = config(sl, n, bs)
    data = packet(n)
    t0, t1 = 128 * 3, 128 * 9
    rows = [put(_quiet(10, bs), t0, fsk_burst(data, sl, lead=1, trail=200)),         # output t0 is carrier, symbol 0 is t0 + 1, t0 + 2
            put(_quiet(11, bs), t0 - 1, fsk_burst(data, sl, lead=1, trail=200)),
            put(_quiet(12, bs), t1 - n * sl - 60, fsk_burst(data, sl, lead=60, trail=0)),   # the last symbol is t1 - 2, t1 - 1
            put(_quiet(13, bs), t1 - n * sl - 60 + 1, fsk_burst(data, sl, lead=60, trail=0))]
    L = Launch("range_ends", cfg, rows)
    assert list(L.n_runs) == [1, 1, 1, 1] and list(L.n_msgs) == [1, 0, 1, 0], (L.n_runs, L.n_msgs)
    assert L.runs[0, 0]["first"] == 3 == L.runs[1, 0]["first"] and L.msgs[0, 0]["tau"] == t0 + sl
    assert all(int(L.runs[c, 0]["first"]) + int(L.runs[c, 0]["windows"]) == 9 for c in (2, 3))
    assert int(L.msgs[2, 0]["tau"]) + sl * (n - 1) == t1 - 1
    return L


SEAM_SL, SEAM_N, SEAM_BS = 14, 80, 2048
SEAM_LAST = tuple(range(-SEAM_SL, SEAM_SL + 1))              # the packet's last output, relative to the boundary


@functools.lru_cache(maxsize=None)
def seam_rows():
    """Per position of SEAM_LAST one channel of two chunks: a noise-free burst whose packet's last output is boundary +
    last, then 300 outputs of carrier, so that the run goes on into chunk 1 and looks back."""
    data = packet(SEAM_N, seed=3)
    piece = fsk_burst(data, SEAM_SL, lead=56, trail=300)
    rows = []
    for j, last in enumerate(SEAM_LAST):
        row = _quiet(100 + j, 2 * SEAM_BS)
        rows.append(put(row, SEAM_BS + last - (SEAM_N * SEAM_SL - 1) - 56, piece))
    both = np.stack(rows)
    return data, both[:, : 2 * SEAM_BS], both[:, 2 * SEAM_BS:]


@functools.lru_cache(maxsize=None)
def seam_launches():
    """(chunk 0 alone, chunk 1 with chunk 0 behind it, chunk 1 with no chunk behind it), a channel per position."""
    data, b0, b1 = seam_rows()
    cfg = config(SEAM_SL, SEAM_N, SEAM_BS)
    first = Launch("seam_chunk0", cfg, list(b0), seq=0)
    back = Launch("seam_chunk1", cfg, list(b1), prev=list(b0), clock=SEAM_BS, seq=1)
    alone = Launch("seam_chunk1_no_prev", cfg, list(b1), clock=SEAM_BS, seq=1)
    ends = [int(back.msgs[c, 0]["tau"]) + SEAM_SL * (SEAM_N - 1) if back.n_msgs[c] else None for c in range(back.n_ch)]
    assert 0 in ends and None in ends and all(e is None or e >= 0 for e in ends), ends
    assert all(int(r["flags"]) & 1 and int(r["tau"]) < 0 and bytes(r["data"]) == data for c in range(back.n_ch) for r in back.records(c))
    assert np.all(back.runs[:, 0]["flags"] & 1)
    assert all(not int(r["flags"]) & 1 and int(r["tau"]) >= 0 for c in range(alone.n_ch) for r in alone.records(c))
    return first, back, alone


@functools.lru_cache(maxsize=None)
def longest_launch():
    """SL 25, N 80 (need 2001, LOOK 16 windows), block_size 4096: the run is the whole chunk, 32 windows, and looks back
    over a packet that straddles t = 0: a region of 6144 outputs, all of the kernel's LDS, 24 outputs per lane."""
    sl, n, bs = 25, 80, 4096
    cfg = config(sl, n, bs)
    assert shape(cfg)[3] == 16 * W
    data = packet(n, seed=4)
    both = put(_quiet(20, 2 * bs), bs - 1000 - 100, fsk_burst(data, sl, lead=100, trail=bs - 1000))
    idle = put(_quiet(21, 2 * bs), bs, fsk_bytes(np.full(bs, 0.11)))                 # the same run with no packet in it
    L = Launch("longest_region", cfg, [both[2 * bs:], idle[2 * bs:]], prev=[both[: 2 * bs], idle[: 2 * bs]], clock=7 * bs, seq=7)
    assert list(L.n_runs) == [1, 1] and np.all(L.runs[:, 0]["windows"] == 32) and np.all(L.runs[:, 0]["flags"] == 3)
    assert list(L.n_msgs) == [1, 0] and list(L.long_runs) == [0, 0]
    assert L.msgs[0, 0]["tau"] == -1000 + sl - 1 and L.msgs[0, 0]["flags"] == 1 and bytes(L.msgs[0, 0]["data"]) == data
    return L


@functools.lru_cache(maxsize=None)
def run_length_launch():
    """A run of exactly 32 windows is decoded, the same burst in a run of 33 is counted in long_runs."""
    sl, n, bs = 14, 80, 34 * W
    cfg = config(sl, n, bs)
    data = packet(n, seed=5)
    rows = [put(_quiet(30 + k, bs), W, fsk_burst(data, sl, lead=100, trail=(32 + k) * W - 100 - n * sl)) for k in (0, 1)]
    L = Launch("run_length", cfg, rows)
    assert [int(L.runs[c, 0]["windows"]) for c in (0, 1)] == [32, 33] and list(L.n_runs) == [1, 1]
    assert list(L.long_runs) == [0, 1] and list(L.n_msgs) == [1, 0] and bytes(L.msgs[0, 0]["data"]) == data
    return L


@functools.lru_cache(maxsize=None)
def need_launch():
    """SL 16, N 40: need = 641 outputs.  A run of 5 windows - the packet's 640 outputs exactly - is skipped; with 100
    outputs of carrier in front the run has 6 windows and the packet is decoded."""
    sl, n, bs = 16, 40, 2048
    cfg = config(sl, n, bs)
    data = packet(n, seed=6)
    rows = [put(_quiet(40, bs), 2 * W, fsk_burst(data, sl, lead=0, trail=0)),
            put(_quiet(41, bs), 2 * W - 100, fsk_burst(data, sl, lead=100, trail=0))]
    L = Launch("need", cfg, rows)
    assert [int(L.runs[c, 0]["windows"]) for c in (0, 1)] == [5, 6] and list(L.n_runs) == [1, 1]
    assert list(L.n_msgs) == [0, 1] and L.msgs[1, 0]["tau"] == 2 * W + sl - 1
    return L


GRID = tuple((n, sl) for n in (40, 64, 80) for sl in (1, 8, 14, 25, 51) if n * sl + 1 <= 2048)


@functools.lru_cache(maxsize=None)
def grid_launch(n, sl):
    """One decodable burst per channel - above and below the channel's centre - for a packet shape rd_burst_decode_check
    admits; data[N / 8:] stays zero."""
    bs = 4096 if n * sl > 1500 else 2048
    cfg = config(sl, n, bs)
    data = packet(n, ident=(n + sl) % 8, seed=n + sl)
    rows = [put(_quiet(50 + k, bs), 200 + 17 * k, fsk_burst(data, sl, carrier=f)) for k, f in enumerate((0.11, -0.07))]
    L = Launch(f"grid_n{n}_sl{sl}", cfg, rows, seq=2 ** 32 + n)
    for c in range(2):
        assert L.n_msgs[c] == 1, (n, sl, c)
        r = L.msgs[c, 0]
        assert bytes(r["data"][: n // 8]) == data and not r["data"][n // 8:].any() and r["tau"] == 200 + 17 * c + 64 + sl - 1
        assert r["id"] == (n + sl) % 8 and L.chunk[c] == n
    return L


@functools.lru_cache(maxsize=None)
def several_launch():
    """Three runs that all decode beside a channel whose run holds no packet and one whose only run is the CRC-invalid
    twin; the clock is 700 outputs short of 2^64, so two of the three times wrap."""
    sl, n, bs = 8, 40, 2048
    cfg = config(sl, n, bs)
    datas = [packet(n, ident=k, seed=60 + k) for k in range(3)]
    row = _quiet(60, bs)
    for k, at in enumerate((100, 800, 1500)):
        put(row, at, fsk_burst(datas[k], sl))
    rows = [row, put(_quiet(61, bs), 300, fsk_bytes(np.full(500, 0.11))),
            put(_quiet(62, bs), 800, fsk_burst(packet(n, seed=61, flip_bit=9), sl))]
    clock = 2 ** 64 - 700
    L = Launch("several_runs", cfg, rows, clock=clock, seq=11)
    assert list(L.n_runs) == [3, 1, 1] and list(L.n_msgs) == [3, 0, 0]
    assert [bytes(r["data"][:5]) for r in L.records(0)] == datas and [int(r["id"]) for r in L.records(0)] == [0, 1, 2]
    assert [int(r["first"]) for r in L.records(0)] == [int(x) for x in L.runs[0, :3]["first"]]
    assert [int(r["time"]) for r in L.records(0)] == [(clock + int(r["tau"])) % 2 ** 64 for r in L.records(0)]
    assert sum(int(r["time"]) < 2 ** 32 for r in L.records(0)) == 2 and int(L.msgs[0, 0]["time"]) > 2 ** 63
    return L


@functools.lru_cache(maxsize=None)
def handwritten_launch():
    """Run records k_chan_bursts never writes, in front of a correct one: corr = (0, 0); windows = 0; first = nW;
    first + windows = nW + 1; and n_runs = cap + 3, behind which the next channel's decodable records lie."""
    sl, n, bs = 8, 40, 2048
    cfg = config(sl, n, bs)
    data = packet(n, seed=70)
    row = put(_quiet(70, bs), 500, fsk_burst(data, sl))
    good = runs_of(row, THR)[0][0, 0].copy()
    n_win, cap = bs // W, BC.cap_of(bs // W)

    def edit(**kw):
        r = good.copy()
        for k, v in kw.items():
            r[k] = v
        return r

    runs = np.zeros((4, cap), BC.BURST_DTYPE)                 # (windows = 0 everywhere else)
    runs[0, :2] = [edit(corr_re=0, corr_im=0), good]
    runs[1, :4] = [edit(windows=0), edit(first=n_win), edit(first=n_win + 1 - int(good["windows"])), good]
    runs[2, 0] = good
    runs[3, :3] = [good, good, edit(windows=MAX_W + 1)]
    n_runs = np.asarray([2, 4, cap + 3, 3], np.uint32)
    L = Launch("handwritten", cfg, [row] * 4, runs=runs, n_runs=n_runs, seq=5)
    assert list(L.n_msgs) == [1, 1, 1, 2] and list(L.long_runs) == [0, 0, 0, 1]
    assert all(bytes(r["data"][:5]) == data for c in range(4) for r in L.records(c))
    return L


def _saturated_fsk(data, sl, turns, lead, trail, invert):
    """Bytes 0 and 255 only: z steps by +-90 degrees per output for `turns` outputs of a symbol (1: +, or - when
    inverted) and by 180 degrees for the rest, so that both parts of p are +-2 x 255^2 or 0 and both products of
    s = corr_re SI - corr_im SR are large."""
    bits = np.unpackbits(np.frombuffer(bytes(data), np.uint8)).astype(np.int64)
    step = np.concatenate([np.where(np.arange(sl) < turns, (1 if b != invert else -1), 2) for b in bits])
    quad = np.cumsum(np.concatenate([np.zeros(lead, np.int64), step, np.zeros(trail, np.int64)])) % 4
    out = np.empty(2 * quad.size, np.uint8)
    out[0::2], out[1::2] = 255 * np.isin(quad, (0, 3)), 255 * np.isin(quad, (0, 1))
    return out


@functools.lru_cache(maxsize=None)
def overflow_launch():
    """A correct run over saturated bytes with its correlation sum replaced by (+-(2^30 - 1), +-(2^30 - 1)): |d| just
    under 2^48, |s| near 2^51, both 32 x 32 -> 64-bit products of the kernel at their largest."""
    sl, n, bs = 14, 80, 2048
    cfg = config(sl, n, bs)
    data = packet(n, seed=80)
    big = 2 ** 30 - 1
    signs = ((1, 1), (1, -1), (-1, 1), (-1, -1))
    rows = [put(_quiet(80 + c, bs), 3 * W, _saturated_fsk(data, sl, 10, 40, 40, invert=sr < 0)) for c, (sr, _) in enumerate(signs)]
    runs, n_runs = runs_of(np.stack(rows), THR)
    for c, (sr, si) in enumerate(signs):
        assert n_runs[c] == 1 and runs[c, 0]["peak"] == BC.P_MAX
        runs[c, 0]["corr_re"], runs[c, 0]["corr_im"] = sr * big, si * big
    L = Launch("overflow_bound", cfg, rows, runs=runs, n_runs=n_runs)
    assert list(L.n_msgs) == [1, 1, 1, 1]
    for c in range(4):
        r = L.msgs[c, 0]
        # (the 10 turning outputs of every symbol fit into 5 adjacent taus alike: a tie among neighbouring lanes)
        assert bytes(r["data"]) == data and r["tau"] == 3 * W + 40 + 10 - 1
        assert [m for _, m in L.candidates(c)].count(int(r["margin"])) == 5
        assert int(r["margin"]) == 6 * 2 * 65025 * big > 2 ** 49                    # |+-10 + 4| x |p| x |corr| at the least
    return L


def hook_launches():
    """Every launch of the crafted decode cases, each with its conditions asserted."""
    return (tie_launch(), range_launch()) + seam_launches() + (longest_launch(), run_length_launch(), need_launch(),
            several_launch(), handwritten_launch(), overflow_launch()) + tuple(grid_launch(n, sl) for n, sl in GRID)


SEAM_LAG = 65         # outputs by which the 512-tap channel filter at decim 4 delays the burst (measured on the float64 model)


SEAM_NEXT = 32 * SEAM_SL   # outputs of the next transmission's lead-in behind the burst


@functools.lru_cache(maxsize=None)
def seam_capture(j, followed=True, seed=140):
    """Two chunks of SEAM_BS outputs for device_receiver(SEAM_BS): one burst of synth_wideband on channel 1 whose
    packet's last symbol ends at output SEAM_BS - SEAM_SL + j of the channelized stream, give or take one, with noise in
    front.  ``followed``: the lead-in (alternating symbols) of a next transmission begins where the burst ends, so that
    chunk 1's run is sliced near the carrier, as the run of chunk 0 is; otherwise noise follows, chunk 1's run is the
    burst's 8 trailing 0-symbols alone, and its correlation sum lies a deviation below the carrier."""
    start = SEAM_BS - (32 + SEAM_N) * SEAM_SL + 1 - SEAM_SL + j - SEAM_LAG
    hz = DEV_OFFSETS_HZ[1] + DEV_PLANTED[1]
    pieces = [_piece(seed, hz, VALID[1], start, 0)]
    rest = 2 * SEAM_BS - start - BURST_OUTPUTS
    if followed:
        pieces.append(_piece(seed + 1, hz, VALID[2], 0, SEAM_NEXT - BURST_OUTPUTS))
        rest -= SEAM_NEXT
    pieces.append(_piece(99, 0, VALID[0], rest + 100, -BURST_OUTPUTS - 100))          # noise alone
    raw = np.concatenate(pieces)
    assert raw.size == 2 * DEV_DECIM * 2 * SEAM_BS
    return raw
