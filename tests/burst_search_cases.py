"""Helpers shared by tests/test_burst_search_cpu.py, tests/test_burst_search.py, tests/test_wideband_search.py and
tools/burst_search_gain.py (no tests in here): the NumPy integer model of k_chan_burst_search, written from the
definition (include/rtldavis_hip.h, BURST SEARCH) - one filter pass over the whole of lo .. B - 1 as a convolution that
sees zeros outside it, every candidate of the chunk at once, where the kernel walks tiles with halos -; the slot model of
the hook rd_debug_burst_search; step 7s; the stream model; and the crafted launches.  The filter is burst_narrow_cases'
filter_region, sync and CRC are burst_repair_cases' repair_model at max_flips 0, the bytes come from burst_decode_cases'
builders.  Every case asserts the edge it is built for on the model of its own bytes when it is built.  Nothing here
touches a device."""
import functools

import numpy as np

import burst_cases as BC
import burst_decode_cases as DC
import burst_narrow_cases as NB
import burst_repair_cases as RP
from rtldavis_amd import synth
from rtldavis_amd.wideband import BURST_MSG_DTYPE, SEARCH_HDR_DTYPE, SearchedMessages

FILL = DC.FILL
SEARCHED = 16                                                # RD_BURST_MSG_SEARCHED
MAX_CENTRES, PER, TILE = 8, 4, 1024                          # RD_BS_MAX_CENTRES, RD_BS_PER, RD_BS_TILE
CARRIER = 0.11                                               # burst_decode_cases.fsk_burst's default
G_CARRIER = 7                                                # the centre nearest to it: round(64 x 0.11)
SHAPES = ((4, 40, 2048), (8, 64, 2048), (14, 80, 2048), (25, 80, 4096), (51, 40, 4096))   # (SL, N, B)


# ------------------------------------------------------------------------------------------ the definition
def candidate_range(cfg, have_prev):
    """None, or (tau_a, tau_b) of step 2s."""
    sl, n, _, look = DC.shape(cfg)
    lo = -look if have_prev else 0
    a, b = max(lo + sl, -sl * (n - 1)), int(cfg.block_size) - 1 - sl * (n - 1)
    return (a, b) if a <= b else None


def search_positions(cur, prev, g, cfg, have_prev):
    """Steps 1s .. 3s for one channel's bytes and one centre: (sync_hits, {tau: (margin, bits, f_re, f_im)}) over the
    passing positions."""
    sl, n, sync, look = DC.shape(cfg)
    bs = cur.size // 2
    rng = candidate_range(cfg, have_prev)
    if rng is None:
        return 0, {}
    lo = -look if have_prev else 0
    a = 2 * (np.concatenate([prev[2 * (bs - look):], cur]) if have_prev else cur).astype(np.int64) - 255
    H, _ = NB.table(sl)
    _, (y_re, y_im) = NB.filter_region(a[0::2], a[1::2], H[int(g)])      # y[lo + j] at j; z is 0 outside lo .. B - 1
    p_re = y_re[1:] * y_re[:-1] + y_im[1:] * y_im[:-1]                   # p'[lo + 1 + j] at j
    p_im = y_im[1:] * y_re[:-1] - y_re[1:] * y_im[:-1]
    ones = np.ones(sl, np.int64)
    s_re, s_im = np.convolve(p_re, ones, "valid"), np.convolve(p_im, ones, "valid")   # S[lo + sl + j] at j
    assert max(np.abs(s_re).max(), np.abs(s_im).max()) < 2 ** 31
    taus = np.arange(rng[0], rng[1] + 1)
    idx = (taus - lo - sl)[:, None] + sl * np.arange(n)[None, :]
    k_re, k_im = s_re[idx], s_im[idx]
    d_re, d_im = k_re[:, :16].sum(axis=1), k_im[:, :16].sum(axis=1)
    big = np.maximum(np.abs(d_re), np.abs(d_im))
    assert big.max() < 2 ** 35
    sh = np.zeros(taus.size, np.int64)
    for b in range(15, 36):
        sh += (big >> b) > 0                                             # bitlength(big) - 15, not below 0
    ca, cb = d_re >> sh, d_im >> sh                                      # (floor)
    ok = (big > 0) & ((ca != 0) | (cb != 0))
    s = k_im * ca[:, None] - k_re * cb[:, None]
    assert np.abs(s).max() < 2 ** 47
    ok &= np.all((s[:, :16] > 0) == np.asarray(sync, bool)[None, :], axis=1)
    passing = {}
    for j in np.flatnonzero(ok):
        r = RP.repair_model(s[j], 0, tuple(sync))
        if r is not None:
            passing[int(taus[j])] = (r[2], r[1], int(k_re[j].sum()), int(k_im[j].sum()))
    return int(ok.sum()), passing


def reported(passing, sl):
    """Step 4s: [(tau, hits)] of the reported positions, ascending."""
    out = []
    for tau in sorted(passing):
        near = [t for t in passing if abs(t - tau) < sl]
        if not any(passing[t][0] > passing[tau][0] or (passing[t][0] == passing[tau][0] and t < tau) for t in near if t != tau):
            out.append((tau, len(near)))
    return out


def search_channel(cur, prev, g, index, channel, cfg, have_prev, clock):
    """(sync_hits, rows) of one (centre, channel): every reported position's record, ascending in tau (the slot keeps
    the first PER)."""
    sl, n, _, _ = DC.shape(cfg)
    hits, passing = search_positions(cur, prev, g, cfg, have_prev)
    rows = []
    for tau, near in reported(passing, sl):
        margin, bits, f_re, f_im = passing[tau]
        data = bytes(np.packbits(bits))
        rows.append((int(channel), int(index), tau, SEARCHED | NB.NARROW | (1 if tau - sl < 0 else 0), (int(clock) + tau) % 2 ** 64, margin,
                     f_re, f_im, list(data) + [0] * (10 - len(data)), int(sum(bits)), synth._swap_bits8(data[2]) & 7, [near, 0, 0, int(g)]))
    return hits, rows


def search_chunk(cur, prev, centres, cfg, have_prev, clock):
    """[[(sync_hits, rows)] per channel] per centre of the list."""
    cur = np.atleast_2d(cur)
    prev = None if prev is None else np.atleast_2d(prev)
    return [[search_channel(cur[c], prev[c] if have_prev else None, g, i, c, cfg, have_prev, clock) for c in range(cur.shape[0])]
            for i, g in enumerate(centres)]


def drop_repeats(records, delivered, sl):
    """Step 7s: the records without those whose channel, pad[3] and data equal a delivered record's less than SL away."""
    def again(r):
        for q in delivered:
            d = (int(r["time"]) - int(q["time"])) % 2 ** 64
            if (q["channel"] == r["channel"] and q["pad"][3] == r["pad"][3] and bytes(q["data"]) == bytes(r["data"])
                    and min(d, 2 ** 64 - d) < sl):
                return True
        return False
    return records[[i for i, r in enumerate(records) if not again(r)]]


def chunk_records(got):
    """The records a fetch sees before step 7s: centres in list order, channels ascending, the first PER by tau."""
    return np.asarray([r for per_c in got for _, rows in per_c for r in rows[:PER]], BURST_MSG_DTYPE).reshape(-1)


def search_stream(blocks, lists, cfg, clock0=0):
    """A receiver in NumPy: per chunk (channelized bytes [n_channels, 2 B], in order from a reset) and its list of
    centres the SearchedMessages a fetch delivers."""
    out, prev, delivered = [], None, np.zeros(0, BURST_MSG_DTYPE)
    for k, (block, centres) in enumerate(zip(blocks, lists)):
        block = np.atleast_2d(block)
        got = search_chunk(block, prev, centres, cfg, k >= 1, clock0 + k * (block.shape[1] // 2))
        recs = drop_repeats(chunk_records(got), delivered, int(cfg.symbol_length))
        shape = (len(centres), block.shape[0])
        out.append(SearchedMessages(recs, np.asarray([[h for h, _ in per_c] for per_c in got], np.uint32).reshape(shape),
                                    np.asarray([[max(0, len(rows) - PER) for _, rows in per_c] for per_c in got], np.uint32).reshape(shape), k))
        prev, delivered = block, recs
    return out


def slot_model(L):
    """What rd_debug_burst_search must hand back: (msgs [8, n_ch, 4], hdr [8, n_ch]); FILL wherever nothing is written."""
    msgs = np.frombuffer(bytes([FILL]) * (MAX_CENTRES * L.n_ch * PER * BURST_MSG_DTYPE.itemsize), BURST_MSG_DTYPE).copy().reshape(MAX_CENTRES, L.n_ch, PER)
    hdr = np.frombuffer(bytes([FILL]) * (MAX_CENTRES * L.n_ch * SEARCH_HDR_DTYPE.itemsize), SEARCH_HDR_DTYPE).copy().reshape(MAX_CENTRES, L.n_ch)
    got = search_chunk(L.cur, L.prev, L.centres, L.cfg, L.prev is not None, L.clock)
    for i, per_c in enumerate(got):
        for c, (hits, rows) in enumerate(per_c):
            hdr[i, c] = (min(len(rows), PER), hits, L.seq & 0xFFFFFFFF, max(0, len(rows) - PER))
            for r, row in enumerate(rows[:PER]):
                msgs[i, c, r] = row
    return msgs, hdr


class SLaunch:
    """One launch of the hook: configuration, bytes, clock, centres; ``want()`` is the model's slot."""

    def __init__(self, name, cfg, rows, centres, prev=None, clock=0, seq=0):
        self.name, self.cfg, self.clock, self.seq = name, cfg, int(clock), int(seq)
        self.cur = np.ascontiguousarray(np.stack(rows), np.uint8)
        self.prev = None if prev is None else np.ascontiguousarray(np.stack(prev), np.uint8)
        assert self.cur.shape[1] == 2 * cfg.block_size and (self.prev is None or self.prev.shape == self.cur.shape)
        self.centres = [int(g) for g in centres]
        assert 1 <= len(self.centres) <= MAX_CENTRES
        self.n_ch = self.cur.shape[0]
        self._want = None

    def want(self):
        if self._want is None:
            self._want = slot_model(self)
        return self._want

    def recs(self, i=0, c=0):
        msgs, hdr = self.want()
        return msgs[i, c, : int(hdr[i, c]["n_msgs"])]


def _quiet(seed, bs):
    return BC.quiet_bytes(np.random.default_rng(seed), bs)


def _data(r, n):
    return bytes(r["data"][: n // 8])


def plain_row(sl, n, bs, at, seed=0, ident=1, background=None, **kw):
    """(data, bytes): one fsk_burst whose packet's first symbol ends at output ``at`` (tau = at), on ``background``
    (default: bytes 128, a noise-free channel)."""
    data = DC.packet(n, ident=ident, seed=seed)
    lead = kw.pop("lead", 64)
    piece = DC.fsk_burst(data, sl, lead=lead, **kw)
    row = np.full(2 * bs, 128, np.uint8) if background is None else background
    first = at - (sl - 1) - lead
    cut = max(0, -first)                                     # (a piece that begins before the row is cut)
    return data, DC.put(row, first + cut, piece[2 * cut:])


# ------------------------------------------------------------------------------------------ crafted bytes
@functools.lru_cache(maxsize=None)
def shape_launch(sl, n, bs):
    """The grid.  Three channels behind a quiet chunk: a packet in mid-chunk, a packet that begins in the previous chunk
    (its first symbol ends 3 SL outputs before t = 0), and quiet bytes alone."""
    cfg = DC.config(sl, n, bs)
    d0, r0 = plain_row(sl, n, bs, bs // 3, seed=300 + sl, background=_quiet(300 + sl, bs))
    d1 = DC.packet(n, ident=2, seed=400 + sl)
    both = _quiet(400 + sl, 2 * bs)
    DC.put(both, bs - 3 * sl - (sl - 1) - 64, DC.fsk_burst(d1, sl))
    L = SLaunch(f"shape_sl{sl}_n{n}", cfg, [r0, both[2 * bs:], _quiet(500 + sl, bs)], [G_CARRIER],
                prev=[_quiet(301 + sl, bs), both[: 2 * bs], _quiet(501 + sl, bs)], clock=3 * bs, seq=3)
    a, b = L.recs(0, 0), L.recs(0, 1)
    assert len(a) == 1 and _data(a[0], n) == d0 and abs(int(a[0]["tau"]) - bs // 3) <= sl // 2 and not int(a[0]["flags"]) & 1
    assert len(b) == 1 and _data(b[0], n) == d1 and abs(int(b[0]["tau"]) + 3 * sl) <= sl // 2 and int(b[0]["flags"]) & 1
    assert len(L.recs(0, 2)) == 0
    return L


@functools.lru_cache(maxsize=None)
def ends_launch():
    """Packets whose last output is output 0, SL - 1 and B - 1 (tau = -SL (N - 1), the first candidate; SL - 1 later; and
    B - 1 - SL (N - 1), the last candidate), a channel each, behind a chunk that holds the first two's beginnings."""
    sl, n, bs = 8, 40, 1152
    cfg = DC.config(sl, n, bs)
    body = sl * (n - 1)
    rows, prevs, datas = [], [], []
    for j, last in enumerate((0, sl - 1, bs - 1)):
        data = DC.packet(n, ident=j, seed=600 + j)
        both = _quiet(600 + j, 2 * bs)
        DC.put(both, bs + last - body - (sl - 1) - 64, DC.fsk_burst(data, sl, trail=0 if last == bs - 1 else 32))
        prevs.append(both[: 2 * bs])
        rows.append(both[2 * bs:])
        datas.append(data)
    L = SLaunch("packet_ends", cfg, rows, [G_CARRIER], prev=prevs, clock=bs, seq=1)
    a, b = candidate_range(cfg, True)
    assert (a, b) == (-body, bs - 1 - body)
    for c, (last, lim) in enumerate(((0, a), (sl - 1, None), (bs - 1, b))):
        r = L.recs(0, c)
        assert len(r) == 1 and _data(r[0], n) == datas[c], (c, r)
        if lim is not None:                                  # the true tau is the range's end: nothing beyond it is a candidate
            assert (int(r[0]["tau"]) - lim) * (1 if lim == a else -1) >= 0 and abs(int(r[0]["tau"]) - lim) <= sl // 2
    return L


@functools.lru_cache(maxsize=None)
def first_chunk_launch():
    """No chunk before.  Channel 0: the packet's first symbol is outputs 0 .. SL - 1, tau = SL - 1 - no candidate, for
    p'[0] does not exist; channel 1: one output later, tau = SL, the first candidate."""
    sl, n, bs = 8, 40, 1152
    cfg = DC.config(sl, n, bs)
    rows = []
    for j in range(2):
        data = DC.packet(n, ident=6, seed=930)
        row = _quiet(930 + j, bs)
        rows.append(DC.put(row, j, DC.fsk_burst(data, sl, lead=0, trail=100)))
    L = SLaunch("first_chunk", cfg, rows, [G_CARRIER])
    assert candidate_range(cfg, False)[0] == sl
    _, passing = search_positions(rows[1], None, G_CARRIER, cfg, False)
    assert sl in passing and all(t >= sl for t in passing)
    assert all(int(r["tau"]) >= sl and not int(r["flags"]) & 1 for c in range(2) for r in L.recs(0, c))
    return L


@functools.lru_cache(maxsize=None)
def six_packets_launch():
    """Six packets back to back on one channel at SL 4, N 40: four records, dropped = 2."""
    sl, n, bs = 4, 40, 2048
    cfg = DC.config(sl, n, bs)
    datas = [DC.packet(n, ident=j, seed=700 + j) for j in range(6)]
    bits = np.concatenate([np.unpackbits(np.frombuffer(d, np.uint8)) for d in datas])
    sym = np.where(np.repeat(bits, sl) == 1, DC.deviation(sl), -DC.deviation(sl))
    row = DC.put(_quiet(700, bs), 300, DC.fsk_bytes(np.concatenate([np.zeros(64), sym, np.zeros(32)]) + CARRIER))
    L = SLaunch("six_packets", cfg, [row], [G_CARRIER], seq=2)
    _, hdr = L.want()
    assert int(hdr[0, 0]["n_msgs"]) == 4 and int(hdr[0, 0]["dropped"]) == 2
    assert [_data(r, n) for r in L.recs()] == datas[:4]
    return L


@functools.lru_cache(maxsize=None)
def tile_launch():
    """SL 14, N 80, B 4096 behind a chunk: the tiles begin at tau_min + 1024 j.  For every tile boundary two channels: a
    packet whose tau is the boundary tile's first position, and one whose tau is the position before it - their passing
    positions, and the SL - 1 neighbours the rule of step 4s looks at, lie on both sides."""
    sl, n, bs = 14, 80, 4096
    cfg = DC.config(sl, n, bs)
    a, b = candidate_range(cfg, True)
    bounds = list(range(a + TILE, b + 1, TILE))
    assert len(bounds) == 3
    rows, prevs, datas, at = [], [], [], []
    for j, t in enumerate(x - d for x in bounds for d in (0, 1)):
        data = DC.packet(n, ident=j % 8, seed=800 + j)
        both = _quiet(800 + j, 2 * bs)
        DC.put(both, bs + t - (sl - 1) - 64, DC.fsk_burst(data, sl))
        prevs.append(both[: 2 * bs])
        rows.append(both[2 * bs:])
        datas.append(data)
        at.append(t)
    L = SLaunch("tile_boundaries", cfg, rows, [G_CARRIER], prev=prevs, clock=bs, seq=1)
    for c, t in enumerate(at):
        _, passing = search_positions(L.cur[c], L.prev[c], G_CARRIER, cfg, True)
        near = [x for x in passing if abs(x - t) < sl]
        x = bounds[c // 2]
        assert min(near) < x <= max(near), (c, near, x)
        r = L.recs(0, c)
        assert len(r) == 1 and _data(r[0], n) == datas[c] and int(r[0]["pad"][0]) == len(near)
    return L


@functools.lru_cache(maxsize=None)
def largest_launch():
    """8 centres x 70 channels, SL 8, N 40, B 1152: a packet on every seventh channel, its carrier at centre 3 + (c // 7):
    found by that centre and its neighbours in the list."""
    sl, n, bs = 8, 40, 1152
    cfg = DC.config(sl, n, bs)
    centres = [4, 5, 6, 7, 8, 9, 10, 40]
    rows, datas = [], {}
    for c in range(70):
        row = _quiet(1000 + c, bs)
        if c % 7 == 0:
            datas[c] = DC.packet(n, ident=c % 8, seed=1000 + c)
            DC.put(row, 100 + 9 * c, DC.fsk_burst(datas[c], sl, carrier=(3 + c // 7) / 64.0))
        rows.append(row)
    L = SLaunch("largest_grid", cfg, rows, centres, prev=[_quiet(2000 + c, bs) for c in range(70)], clock=9 * bs, seq=9)
    msgs, hdr = L.want()
    for c, d in datas.items():
        g = 3 + c // 7
        if g in centres:
            r = L.recs(centres.index(g), c)
            assert len(r) == 1 and _data(r[0], n) == d and int(r[0]["first"]) == centres.index(g) and int(r[0]["pad"][3]) == g
    assert np.all(hdr["chunk"] == 9)
    return L


@functools.lru_cache(maxsize=None)
def seam_launches():
    """burst_decode_cases.seam_rows: the packet's last output at boundary + last for last in -SL .. SL, a channel per
    position: (chunk 0, chunk 1 behind it, data)."""
    data, b0, b1 = DC.seam_rows()
    cfg = DC.config(DC.SEAM_SL, DC.SEAM_N, DC.SEAM_BS)
    first = SLaunch("seam_chunk0", cfg, list(b0), [G_CARRIER], seq=0)
    back = SLaunch("seam_chunk1", cfg, list(b1), [G_CARRIER], prev=list(b0), clock=DC.SEAM_BS, seq=1)
    return first, back, data


def launch_records(L):
    """The records of a launch's model as a fetch sees them."""
    msgs, hdr = L.want()
    n = len(L.centres)
    return np.asarray([msgs[i, c, r] for i in range(n) for c in range(L.n_ch) for r in range(int(hdr[i, c]["n_msgs"]))],
                      BURST_MSG_DTYPE).reshape(-1)


TIE_SL, TIE_N, TIE_BS, TIE_G, TIE_SEED = 8, 40, 1152, 32, 21


@functools.lru_cache(maxsize=None)
def tie_launch():
    """Several positions with equal margins less than SL apart: the smallest tau is reported.  Margins of whole bursts are
    40-bit numbers that do not tie, so the tie is built at margin 0: a packet at half a cycle per output (centre 32,
    where constant bytes give y = 0 exactly) whose last three symbols are 0 and whose transmission ends where the third
    last begins.  Behind the filter's ringing the last symbol's S is 0 at every position near the true tau, so s = 0
    there - bit 0, as sent - and every passing position has margin 0.  (Seed 21 is the first packet of
    burst_decode_cases.packet with such an ending whose ringing symbols also slice to 0 at two positions or more.)"""
    sl, n, bs = TIE_SL, TIE_N, TIE_BS
    cfg = DC.config(sl, n, bs)
    data = DC.packet(n, ident=TIE_SEED % 8, seed=TIE_SEED)
    assert not np.unpackbits(np.frombuffer(data, np.uint8))[-3:].any()
    row = np.full(2 * bs, 128, np.uint8)
    at = 200
    DC.put(row, at, DC.fsk_burst(data, sl, carrier=TIE_G / 64.0, lead=64, trail=0))
    row[2 * (at + 64 + sl * (n - 3)):] = 128
    L = SLaunch("equal_margins", cfg, [row], [TIE_G], seq=4)
    _, passing = search_positions(row, None, TIE_G, cfg, False)
    near = sorted(passing)
    assert len(near) >= 2 and near[-1] - near[0] < sl and all(passing[t][0] == 0 for t in near), (near, [passing[t][0] for t in near])
    r = L.recs()
    assert len(r) == 1 and int(r[0]["tau"]) == near[0] and int(r[0]["margin"]) == 0 and _data(r[0], n) == data
    assert int(r[0]["pad"][0]) == len(near)
    return L


@functools.lru_cache(maxsize=None)
def hook_launches():
    first, back, _ = seam_launches()
    return tuple(shape_launch(*s) for s in SHAPES) + (ends_launch(), first_chunk_launch(), six_packets_launch(), tile_launch(),
                                                      largest_launch(), first, back, tie_launch())
