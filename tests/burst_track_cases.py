"""Helpers shared by tests/test_burst_track_cpu.py, tests/test_burst_track.py, tests/test_wideband_track.py and
tools/burst_track_gain.py (no tests in here): the NumPy / Python integer model of k_chan_burst_expect, written from the
definition (include/rtldavis_hip.h, BURST EXPECT) - the candidate range in signed Python integers where the library
works modulo 2^64, the region cut out of the two chunks' bytes at t0 itself where the kernel loads from a multiple of 8,
the filter as a convolution over an array that holds zeros outside zf0 .. zf1 -; the slot model of the hook
rd_debug_burst_expect; step 7'; the stream model; and the crafted launches.  Steps 5 .. 6' are burst_repair_cases'
repair_model, the filter is burst_narrow_cases' filter_region, the bytes come from burst_decode_cases' builders.  Every
case asserts the edge it is built for on the model of its own bytes when it is built.  Nothing here touches a device."""
import functools
import math

import numpy as np

import burst_cases as BC
import burst_decode_cases as DC
import burst_narrow_cases as NB
import burst_repair_cases as RP
from rtldavis_amd import synth
from rtldavis_amd.wideband import BURST_MSG_DTYPE, EXPECT_DTYPE, ExpectedMessages

W, FILL = DC.W, DC.FILL
EXPECTED = 8                                                 # RD_BURST_MSG_EXPECTED
MAX, MAX_SPAN, ANY = 64, 2048, 0xFF
HDR_DTYPE = np.dtype([("n_msgs", np.uint32), ("candidates", np.uint32), ("chunk", np.uint32), ("pad", np.uint32)])
FORMS = ((0, False), (2, False), (0, True), (2, True))       # (max_flips, narrow): the kernel's four instantiations
ALL_FORMS = tuple((r, nb) for nb in (False, True) for r in (0, 1, 2))


def corr_of(f, scale=16384.0):
    """round(scale e^{j 2 pi f}) for a carrier at f cycles per output."""
    return int(round(scale * math.cos(2 * math.pi * f))), int(round(scale * math.sin(2 * math.pi * f)))


def expect_row(channel, t_lo, t_hi, corr, ident=ANY):
    return (int(channel), int(ident), int(t_lo) % 2 ** 64, int(t_hi) % 2 ** 64, int(corr[0]), int(corr[1]))


def table(rows):
    return np.asarray(list(rows), EXPECT_DTYPE).reshape(-1)


# ------------------------------------------------------------------------------------------ the definition
def candidate_range(cfg, have_prev, clock, t_lo, t_hi):
    """None, or (tau_a, tau_b): the least and greatest tau with t_lo <= clock + tau <= t_hi, 0 <= tau + SL (N - 1) < B and
    tau - SL >= 0 unless have_prev.  The distance from the chunk to the window is taken as a signed number."""
    sl, n, _, _ = DC.shape(cfg)
    body, bs = sl * (n - 1), int(cfg.block_size)
    lo_b, hi_b = (-body if have_prev else sl), bs - 1 - body
    d = (int(t_lo) - int(clock)) % 2 ** 64
    d = d - 2 ** 64 if d >= 2 ** 63 else d                   # tau of t_lo
    a, b = max(lo_b, d), min(hi_b, d + (int(t_hi) - int(t_lo)))
    return (a, b) if a <= b else None


def symbol_sums(cur, prev, e, cfg, have_prev, clock, narrow):
    """None (idle), or (taus, s [candidates, N], t0, p_re, p_im, g): steps 4 / 4n for one expectation; p (or p') over
    t0 < t < t1 at index t - t0 - 1."""
    sl, n, _, look = DC.shape(cfg)
    rng = candidate_range(cfg, have_prev, clock, e["t_lo"], e["t_hi"])
    if rng is None:
        return None
    tau_a, tau_b = rng
    t0, t1 = tau_a - sl, tau_b + sl * (n - 1) + 1
    bs = cur.size // 2
    assert t0 >= (-look if have_prev else 0) and t1 <= bs and t1 - t0 <= MAX_SPAN + 2048
    a = 2 * (np.concatenate([prev, cur]) if have_prev else cur).astype(np.int64) - 255
    org = bs if have_prev else 0
    ai, aq = a[0::2], a[1::2]
    cre, cim = int(e["corr_re"]), int(e["corr_im"])
    g = 0
    if not narrow:
        zi, zq = ai[org + t0: org + t1], aq[org + t0: org + t1]
        p_re = zi[1:] * zi[:-1] + zq[1:] * zq[:-1]
        p_im = zq[1:] * zi[:-1] - zi[1:] * zq[:-1]
    else:
        m = sl + 2
        zf0, zf1 = max(t0 - m, -look if have_prev else 0), min(t1 + m, bs)
        tt = np.arange(t0 - m, t1 + m)
        inside = (tt >= zf0) & (tt < zf1)
        zi, zq = np.zeros(tt.size, np.int64), np.zeros(tt.size, np.int64)
        zi[inside], zq[inside] = ai[org + tt[inside]], aq[org + tt[inside]]
        H, C = NB.table(sl)
        score = [cre * int(C[k, 0]) + cim * int(C[k, 1]) for k in range(NB.GRID)]   # ca = corr_re, cb = corr_im: sh = 0
        assert max(abs(v) for v in score) < 2 ** 30
        g = score.index(max(score))
        _, (y_re, y_im) = NB.filter_region(zi, zq, H[g])
        y_re, y_im = y_re[m: m + t1 - t0], y_im[m: m + t1 - t0]
        p_re = y_re[1:] * y_re[:-1] + y_im[1:] * y_im[:-1]
        p_im = y_im[1:] * y_re[:-1] - y_re[1:] * y_im[:-1]
    d = p_im * cre - p_re * cim
    s_all = np.convolve(d, np.ones(sl, np.int64), "valid")   # s[t0 + sl + j] at j
    assert np.abs(s_all).max() < (2 ** 47 if narrow else 2 ** 41)
    taus = np.arange(tau_a, tau_b + 1)
    s = s_all[(taus - t0 - sl)[:, None] + sl * np.arange(n)[None, :]]
    return taus, s, t0, p_re, p_im, g


def decode_expect(cur, prev, e, index, cfg, have_prev, clock, max_flips, narrow):
    """None (idle), or (candidates, row or None) for one expectation: steps 4 .. 6' and the id filter."""
    sl, n, sync, _ = DC.shape(cfg)
    got = symbol_sums(cur, prev, e, cfg, have_prev, clock, narrow)
    if got is None:
        return None
    taus, s, t0, p_re, p_im, g = got
    best = None
    for j in np.flatnonzero(np.all((s[:, :16] > 0) == np.asarray(sync, bool)[None, :], axis=1)):
        r = RP.repair_model(s[j], max_flips, tuple(sync))
        if r is None:
            continue
        data = bytes(np.packbits(r[1]))
        if int(e["id"]) < 8 and (synth._swap_bits8(data[2]) & 7) != int(e["id"]):
            continue
        key = (len(r[0]), -r[2], int(taus[j]))
        if best is None or key < best[0]:
            best = (key, r)
    if best is None:
        return taus.size, None
    (n_flip, neg_margin, tau), (ks, bits, _) = best
    data = bytes(np.packbits(bits))
    tt = np.arange(tau - sl + 1, tau + sl * (n - 1) + 1) - (t0 + 1)
    assert tt.size == n * sl and tt[0] >= 0
    pad = [n_flip] + list(ks) + [0] * (2 - len(ks)) + [g]
    flags = EXPECTED | (1 if t0 < 0 else 0) | (RP.REPAIRED if n_flip else 0) | (NB.NARROW if narrow else 0)
    row = (int(e["channel"]), index, tau, flags, (int(clock) + tau) % 2 ** 64, -neg_margin, int(p_re[tt].sum()), int(p_im[tt].sum()),
           list(data) + [0] * (10 - len(data)), int(sum(bits)), synth._swap_bits8(data[2]) & 7, pad)
    return taus.size, row


def decode_chunk(cur, prev, tab, cfg, have_prev, clock, max_flips, narrow):
    """[(candidates, row or None) or None] per expectation of the table."""
    cur = np.atleast_2d(cur)
    prev = None if prev is None else np.atleast_2d(prev)
    return [decode_expect(cur[int(e["channel"])], None if not have_prev else prev[int(e["channel"])], e, i, cfg, have_prev, clock,
                          max_flips, narrow) for i, e in enumerate(tab)]


def drop_repeats(records, delivered, sl):
    """Step 7': the records without those whose channel and data equal a delivered record's less than SL away in time."""
    def again(r):
        for q in delivered:
            d = (int(r["time"]) - int(q["time"])) % 2 ** 64
            if q["channel"] == r["channel"] and bytes(q["data"]) == bytes(r["data"]) and min(d, 2 ** 64 - d) < sl:
                return True
        return False
    return records[[i for i, r in enumerate(records) if not again(r)]]


def expect_stream(blocks, tables, cfg, max_flips, narrow, clock0=0):
    """A receiver in NumPy: per chunk (channelized bytes [n_channels, 2 B], in order from a reset) and its table the
    ExpectedMessages a fetch delivers."""
    out, prev, delivered = [], None, np.zeros(0, BURST_MSG_DTYPE)
    for k, (block, tab) in enumerate(zip(blocks, tables)):
        block = np.atleast_2d(block)
        got = decode_chunk(block, prev, tab, cfg, k >= 1, clock0 + k * (block.shape[1] // 2), max_flips, narrow)
        recs = np.asarray([g[1] for g in got if g is not None and g[1] is not None], BURST_MSG_DTYPE).reshape(-1)
        recs = drop_repeats(recs, delivered, int(cfg.symbol_length))
        out.append(ExpectedMessages(recs, np.asarray([0 if g is None else g[0] for g in got], np.uint32), k))
        prev, delivered = block, recs
    return out


def slot_model(X, max_flips, narrow):
    """What rd_debug_burst_expect must hand back: (msgs [64], hdr [64]); FILL wherever nothing is written - everywhere
    when no expectation has a candidate, for then nothing is launched."""
    msgs = np.frombuffer(bytes([FILL]) * (MAX * BURST_MSG_DTYPE.itemsize), BURST_MSG_DTYPE).copy()
    hdr = np.frombuffer(bytes([FILL]) * (MAX * HDR_DTYPE.itemsize), HDR_DTYPE).copy()
    got = decode_chunk(X.cur, X.prev, X.table, X.cfg, X.prev is not None, X.clock, max_flips, narrow)
    if all(g is None for g in got):
        return msgs, hdr
    for i, g in enumerate(got):
        hdr[i] = (0, 0, X.seq & 0xFFFFFFFF, 0) if g is None else (0 if g[1] is None else 1, g[0], X.seq & 0xFFFFFFFF, 0)
        if g is not None and g[1] is not None:
            msgs[i] = g[1]
    return msgs, hdr


class XLaunch:
    """One launch of the hook: configuration, bytes, clock, table; ``want(R, narrow)`` is the model's slot."""

    def __init__(self, name, cfg, rows, tab, prev=None, clock=0, seq=0):
        self.name, self.cfg, self.clock, self.seq = name, cfg, int(clock), int(seq)
        self.cur = np.ascontiguousarray(np.stack(rows), np.uint8)
        self.prev = None if prev is None else np.ascontiguousarray(np.stack(prev), np.uint8)
        assert self.cur.shape[1] == 2 * cfg.block_size and (self.prev is None or self.prev.shape == self.cur.shape)
        self.table = table(tab) if not isinstance(tab, np.ndarray) else tab
        assert 1 <= self.table.size <= MAX
        self.n_ch = self.cur.shape[0]
        self._want = {}

    def want(self, r, narrow):
        if (r, narrow) not in self._want:
            self._want[r, narrow] = slot_model(self, r, narrow)
        return self._want[r, narrow]

    def recs(self, r=0, narrow=False):
        msgs, hdr = self.want(r, narrow)
        live = hdr["chunk"] == (self.seq & 0xFFFFFFFF)
        return msgs[live & (hdr["n_msgs"] == 1)]

    def headers(self, r=0, narrow=False):
        return self.want(r, narrow)[1][: self.table.size]

    def forms(self):
        """The forms this launch's symbol length admits."""
        return ALL_FORMS if int(self.cfg.symbol_length) >= NB.MIN_SL else ALL_FORMS[:3]


def _quiet(seed, bs):
    return BC.quiet_bytes(np.random.default_rng(seed), bs)


def _data(r, n):
    return bytes(r["data"][: n // 8])


def best_tau(cfg, row, lo, hi, corr, prev=None, narrow=False, channel=0):
    """The model's tau for a window lo .. hi of one channel's bytes (clock 0), or None."""
    got = decode_expect(row, prev, table([expect_row(channel, lo, hi, corr)])[0], 0, cfg, prev is not None, 0, 0, narrow)
    return None if got is None or got[1] is None else got[1][2]


CARRIER = 0.11                                               # burst_decode_cases.fsk_burst's default


# ------------------------------------------------------------------------------------------ crafted bytes
@functools.lru_cache(maxsize=None)
def edges_launch():
    """Case 1.  SL 8, N 40, one packet whose best tau is T and whose valid taus are v0 .. v1: windows T .. T + 9 (the
    record at t_lo), T - 9 .. T (at t_hi), T .. T (one candidate), v0 - 5 .. v0 - 1 and v1 + 1 .. v1 + 5 (the window
    ends one output before the first valid tau / begins one after the last: candidates 5, no record)."""
    sl, n, bs = 8, 40, 1152
    cfg = DC.config(sl, n, bs)
    data = DC.packet(n, ident=2, seed=900)
    row = DC.put(_quiet(900, bs), 300, DC.fsk_burst(data, sl))
    c = corr_of(CARRIER)
    T = best_tau(cfg, row, 300, 500, c)
    assert T == 300 + 64 + sl - 1
    valid = [t for t in range(T - 12, T + 13) if best_tau(cfg, row, t, t, c) == t]
    v0, v1 = valid[0], valid[-1]
    assert valid == list(range(v0, v1 + 1)) and v0 <= T <= v1 and len(valid) >= 2
    X = XLaunch("window_edges", cfg, [row], [expect_row(0, T, T + 9, c), expect_row(0, T - 9, T, c), expect_row(0, T, T, c),
                                              expect_row(0, v0 - 5, v0 - 1, c), expect_row(0, v1 + 1, v1 + 5, c)], seq=3)
    h = X.headers()
    assert list(h["n_msgs"]) == [1, 1, 1, 0, 0] and list(h["candidates"]) == [10, 10, 1, 5, 5]
    assert [int(r["tau"]) for r in X.recs()] == [T, T, T] and all(_data(r, n) == data and int(r["flags"]) == EXPECTED for r in X.recs())
    assert [int(r["first"]) for r in X.recs()] == [0, 1, 2]
    return X, T


@functools.lru_cache(maxsize=None)
def seam_launches():
    """Case 2.  burst_decode_cases.seam_rows: the packet's last output at boundary + last for last in -SL .. SL, a
    channel per position, each under an expectation of +-40 outputs around its packet: (chunk 0, chunk 1)."""
    data, b0, b1 = DC.seam_rows()
    cfg = DC.config(DC.SEAM_SL, DC.SEAM_N, DC.SEAM_BS)
    c = corr_of(CARRIER)
    tab = [expect_row(j, DC.SEAM_BS + last - DC.SEAM_SL * (DC.SEAM_N - 1) - 40, DC.SEAM_BS + last - DC.SEAM_SL * (DC.SEAM_N - 1) + 40, c)
           for j, last in enumerate(DC.SEAM_LAST)]
    first = XLaunch("seam_chunk0", cfg, list(b0), tab, seq=0)
    back = XLaunch("seam_chunk1", cfg, list(b1), tab, prev=list(b0), clock=DC.SEAM_BS, seq=1)
    return first, back, data


def seam_survivors(first_recs, back_recs):
    """(records of chunk 0, records of chunk 1 after step 7')."""
    return first_recs, drop_repeats(back_recs, first_recs, DC.SEAM_SL)


@functools.lru_cache(maxsize=None)
def gap_window0_off():
    """Case 3a.  The packet's last 11 outputs reach into chunk 1, and nothing follows: window 0 of chunk 1 stays OFF, so
    there is no run in it, and chunk 0's run cannot report a packet that does not end in chunk 0.  Returns (the run
    launches of chunk 0 and 1, the expectation launch of chunk 1, data)."""
    sl, n, bs = 14, 80, 2048
    cfg = DC.config(sl, n, bs)
    data = DC.packet(n, ident=4, seed=910)
    both = DC.put(_quiet(910, 2 * bs), bs + 10 - (n * sl - 1) - 64, DC.fsk_burst(data, sl, lead=64, trail=0))
    b0, b1 = both[: 2 * bs], both[2 * bs:]
    r0 = DC.Launch("gap_off_chunk0", cfg, [b0], seq=0)
    r1 = DC.Launch("gap_off_chunk1", cfg, [b1], prev=[b0], clock=bs, seq=1)
    assert list(r0.n_msgs) == [0] and list(r1.n_runs) == [0] and list(r1.n_msgs) == [0]
    t = bs + 10 - sl * (n - 1)
    X = XLaunch("gap_window0_off", cfg, [b1], [expect_row(0, t - 30, t + 30, corr_of(CARRIER))], prev=[b0], clock=bs, seq=1)
    assert len(X.recs()) == 1 and _data(X.recs()[0], n) == data and int(X.recs()[0]["flags"]) == EXPECTED | 1
    return (r0, r1), X, data


@functools.lru_cache(maxsize=None)
def gap_long_run():
    """Case 3b.  burst_decode_cases.run_length_launch's channel 1: the packet inside a run of 33 windows, counted in
    long_runs and not decoded; the expectation gives it."""
    R = DC.run_length_launch()
    sl, n = 14, 80
    assert list(R.long_runs) == [0, 1] and int(R.n_msgs[1]) == 0
    t = W + 100 + sl - 1
    X = XLaunch("gap_long_run", R.cfg, [R.cur[1]], [expect_row(0, t - 30, t + 30, corr_of(CARRIER))])
    assert len(X.recs()) == 1 and _data(X.recs()[0], n) == bytes(R.msgs[0, 0]["data"][: n // 8])
    return R, X


@functools.lru_cache(maxsize=None)
def gap_trailing_only():
    """Case 3c.  The packet ends 8 outputs into chunk 1 and is followed by 8 trailing 0-symbols, then nothing: chunk 1's
    run holds the trailing symbols alone, its correlation sum lies a deviation below the carrier, and the packet is
    not decoded from it; chunk 0 cannot reach the packet's end."""
    sl, n, bs = 14, 80, 2048
    cfg = DC.config(sl, n, bs)
    data = DC.packet(n, ident=5, seed=920)
    dev = DC.deviation(sl)
    freqs = np.concatenate([RP.burst_freqs(data, sl, lead=64, trail=0), np.full(8 * sl, CARRIER - dev)])
    both = DC.put(_quiet(920, 2 * bs), bs + 7 - (n * sl - 1) - 64, DC.fsk_bytes(freqs))
    b0, b1 = both[: 2 * bs], both[2 * bs:]
    r0 = DC.Launch("gap_trailing_chunk0", cfg, [b0], seq=0)
    r1 = DC.Launch("gap_trailing_chunk1", cfg, [b1], prev=[b0], clock=bs, seq=1)
    assert list(r0.n_msgs) == [0] and list(r1.n_runs) == [1] and list(r1.n_msgs) == [0], (r0.n_msgs, r1.n_runs, r1.n_msgs)
    t = bs + 7 - sl * (n - 1)
    X = XLaunch("gap_trailing_only", cfg, [b1], [expect_row(0, t - 30, t + 30, corr_of(CARRIER))], prev=[b0], clock=bs, seq=1)
    assert len(X.recs()) == 1 and _data(X.recs()[0], n) == data
    return (r0, r1), X, data


@functools.lru_cache(maxsize=None)
def first_chunk_launches():
    """Case 4.  The packet's first symbol is outputs 0 .. SL - 1, tau = SL - 1 < SL: with no chunk before, that tau is
    no candidate (and SL - 1 outputs on, the packet no longer decodes); the same bytes behind a quiet chunk give the
    record."""
    sl, n, bs = 8, 40, 1152
    cfg = DC.config(sl, n, bs)
    data = DC.packet(n, ident=6, seed=930)
    row = DC.put(_quiet(930, bs), 0, DC.fsk_burst(data, sl, lead=0, trail=100))
    tab = [expect_row(0, 0, 5 * sl, corr_of(CARRIER))]
    alone = XLaunch("first_chunk_no_prev", cfg, [row], tab)
    behind = XLaunch("first_chunk_with_prev", cfg, [row], tab, prev=[_quiet(931, bs)])
    ha, hb = alone.headers()[0], behind.headers()[0]
    assert int(ha["candidates"]) == 5 * sl - sl + 1 and int(hb["candidates"]) == 5 * sl + 1
    assert int(hb["n_msgs"]) == 1 and int(behind.recs()[0]["tau"]) <= sl - 1 and _data(behind.recs()[0], n) == data
    assert int(ha["n_msgs"]) == 0 or int(alone.recs()[0]["tau"]) >= sl
    return alone, behind


@functools.lru_cache(maxsize=None)
def alignment_launch():
    """Case 5.  Eight windows T - r .. T + 3, r = 0 .. 7, over one packet inside a long stretch of full-amplitude carrier:
    t0 = T - r - SL takes every residue modulo 8 and none is a multiple of 128, and the bytes in front of t0 (of zf0) and
    behind t1 (zf1) that the rounded-down loads bring along are not quiet."""
    sl, n, bs = 8, 40, 1152
    cfg = DC.config(sl, n, bs)
    data = DC.packet(n, ident=7, seed=940)
    row = DC.put(_quiet(940, bs), 100, DC.fsk_burst(data, sl, lead=200, trail=300))
    c = corr_of(CARRIER)
    T = best_tau(cfg, row, 250, 400, c)
    assert T == 100 + 200 + sl - 1
    X = XLaunch("alignment", cfg, [row], [expect_row(0, T - r, T + 3, c) for r in range(8)], seq=9)
    assert sorted((T - r - sl) % 8 for r in range(8)) == list(range(8)) and all((T - r - sl) % 128 for r in range(8))
    for nb in (False, True):
        assert [int(r["tau"]) for r in X.recs(0, nb)] == [T] * 8
    a = 2 * row.astype(np.int64) - 255
    for t in (T - 7 - sl - (sl + 2) - 1, T + 3 + sl * (n - 1) + 1 + sl + 2):      # just outside the widest zf0 .. zf1
        assert abs(int(a[2 * t])) + abs(int(a[2 * t + 1])) > 40
    return X, T


@functools.lru_cache(maxsize=None)
def id_launches():
    """Case 6.  A packet of id 3 under expectations for id 3, 5 and any; and a packet of id 2 whose weak wrong symbol is
    17 - bit 1 of the id, lonely between symbols 16 and 18 - under expectations for id 2 (the corrected id), 0 (the id as
    received) and any."""
    sl, n, bs = 8, 80, 2048
    cfg = DC.config(sl, n, bs)
    c = corr_of(CARRIER)
    data = DC.packet(n, ident=3, seed=950)
    t = 300 + 64 + sl - 1
    plain = XLaunch("id_filter", cfg, [DC.put(_quiet(950, bs), 300, DC.fsk_burst(data, sl))],
                    [expect_row(0, t - 20, t + 20, c, i) for i in (3, 5, ANY)])
    assert list(plain.headers()["n_msgs"]) == [1, 0, 1] and all(int(r["id"]) == 3 for r in plain.recs())
    bad = RP.find_packet(n, lambda b: RP.lonely(b, 17) and (synth._swap_bits8(int("".join(map(str, b[16:24])), 2)) & 7) == 2, 5000)
    flip = XLaunch("id_filter_repaired", cfg, [DC.put(_quiet(951, bs), 300, RP.damaged(bad, sl, {17: RP.WEAK}))],
                   [expect_row(0, t - 20, t + 20, c, i) for i in (2, 0, ANY)])
    assert list(flip.headers(0)["n_msgs"]) == [0, 0, 0] and list(flip.headers(1)["n_msgs"]) == [1, 0, 1]
    m = flip.recs(1)[0]
    assert tuple(int(x) for x in m["pad"][:3]) == (1, 17, 0) and int(m["id"]) == 2 and _data(m, n) == bad
    return plain, flip


@functools.lru_cache(maxsize=None)
def largest_launch():
    """Case 7.  N 40, SL 51 (N SL + 1 = 2041), a window of 2048: 2049 candidates, a region of 4089 outputs that begins
    2040 outputs before the chunk, over a packet that straddles t = 0."""
    sl, n, bs = 51, 40, 2176
    cfg = DC.config(sl, n, bs)
    data = DC.packet(n, ident=1, seed=960)
    both = DC.put(_quiet(960, 2 * bs), bs - 1000 - 100, DC.fsk_burst(data, sl, carrier=-0.30, lead=100, trail=200))
    c = corr_of(-0.30)
    clock = 5 * bs
    X = XLaunch("largest_region", cfg, [both[2 * bs:]], [expect_row(0, clock - sl * (n - 1), clock - sl * (n - 1) + 2048, c)],
                prev=[both[: 2 * bs]], clock=clock, seq=5)
    for nb in (False, True):
        h = X.headers(0, nb)[0]
        assert int(h["candidates"]) == 2049 and int(h["n_msgs"]) == 1
        m = X.recs(0, nb)[0]
        assert _data(m, n) == data and abs(int(m["tau"]) - (-1000 + sl - 1)) <= sl // 2 and int(m["flags"]) & 1
    return X


@functools.lru_cache(maxsize=None)
def full_table_launch():
    """Case 8.  64 expectations over three channels with a packet each: every fourth is idle (its window lies in another
    chunk), the others overlap on their channel and each give their own record."""
    sl, n, bs = 8, 40, 1152
    cfg = DC.config(sl, n, bs)
    carriers = (0.11, -0.07, 0.31)
    datas = [DC.packet(n, ident=k, seed=970 + k) for k in range(3)]
    rows = [DC.put(_quiet(970 + k, bs), 200 + 150 * k, DC.fsk_burst(datas[k], sl, carrier=f)) for k, f in enumerate(carriers)]
    clock = 7 * bs
    tab = []
    for i in range(MAX):
        k = i % 3
        t = clock + 200 + 150 * k + 64 + sl - 1
        if i % 4 == 3:
            tab.append(expect_row(k, t + 3 * bs, t + 3 * bs + 10, corr_of(carriers[k])))
        else:
            tab.append(expect_row(k, t - 20 - i, t + 5 + i % 7, corr_of(carriers[k])))
    X = XLaunch("full_table", cfg, rows, tab, clock=clock, seq=7)
    h = X.headers()
    idle = np.arange(MAX) % 4 == 3
    assert np.all(h["candidates"][idle] == 0) and np.all(h["n_msgs"][idle] == 0) and np.all(h["n_msgs"][~idle] == 1)
    assert [int(r["first"]) for r in X.recs()] == [i for i in range(MAX) if i % 4 != 3]
    assert all(_data(r, n) == datas[int(r["channel"])] for r in X.recs())
    msgs, _ = X.want(0, False)
    assert all(msgs[i].tobytes() == bytes([FILL]) * BURST_MSG_DTYPE.itemsize for i in range(MAX) if i % 4 == 3)
    return X


@functools.lru_cache(maxsize=None)
def all_idle_launch():
    """Case 8, no expectation active: nothing is launched and the slot comes back as it was filled."""
    X0 = full_table_launch()
    tab = X0.table.copy()
    tab["t_lo"] += 10 * 1152
    tab["t_hi"] += 10 * 1152
    X = XLaunch("all_idle", X0.cfg, list(X0.cur), tab, clock=X0.clock, seq=7)
    assert X.want(0, False)[1].tobytes() == bytes([FILL]) * (MAX * HDR_DTYPE.itemsize)
    return X


@functools.lru_cache(maxsize=None)
def tie_launch():
    """Case 9a.  burst_decode_cases.tie_launch's rows (SL 2: the wide forms only) under one window over both copies: two
    candidates of equal margin, the smaller tau; and with the later copy one step louder, the later."""
    L = DC.tie_launch()
    c = corr_of(CARRIER)
    X = XLaunch("expect_ties", L.cfg, list(L.cur), [expect_row(ch, 128, 128 + 1700, c) for ch in range(L.n_ch)])
    want = [int(L.msgs[ch, 0]["tau"]) for ch in range(L.n_ch)]
    assert [int(r["tau"]) for r in X.recs()] == want
    return X


CORR_BOUNDS = ((-32768, 32767), (1, 0), (0, -1), (32767, -32768))


@functools.lru_cache(maxsize=None)
def bounds_launch():
    """Case 9b.  burst_narrow_cases.saturated_launch's bytes (0 and 255 only) under corr at the ends of its range."""
    L = NB.saturated_launch()
    X = XLaunch("expect_corr_bounds", L.cfg, [L.cur[0]], [expect_row(0, 3 * W, 3 * W + 400, c) for c in CORR_BOUNDS])
    for nb in (False, True):
        got = decode_chunk(X.cur, None, X.table, X.cfg, False, 0, 0, nb)
        assert all(g is not None for g in got)
    return X


@functools.lru_cache(maxsize=None)
def repair_launches():
    """Case 10.  The one-flip and two-flip launches of burst_repair_cases through an expectation per channel."""
    out = []
    c = corr_of(CARRIER)
    for L, at in ((RP.one_flip_launch(), lambda ch: 300 + 5 * ch), (RP.two_flips_launch(), lambda ch: 280 + 3 * ch)):
        sl = int(L.cfg.symbol_length)
        X = XLaunch("expect_" + L.name, L.cfg, list(L.cur), [expect_row(ch, at(ch) + 64 + sl - 1 - 12, at(ch) + 64 + sl - 1 + 12, c)
                                                            for ch in range(L.n_ch)])
        for r in range(3):
            assert [int(x) for x in X.headers(r)["n_msgs"]] == L.counts(r), (L.name, r)
            for ch, m in enumerate(X.recs(r)):
                assert tuple(int(v) for v in m["pad"][:3]) == tuple(int(v) for v in L.recs(r, ch)[0]["pad"][:3])
        out.append(X)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def grid_launch(n, sl):
    """Case 10, the grid: burst_narrow_cases.grid_launch's bytes for (N, SL), an expectation per channel at its carrier."""
    L = NB.grid_launch(n, sl)
    tab = [expect_row(ch, 200 + 17 * ch + 64 + sl - 1 - 2 * sl, 200 + 17 * ch + 64 + sl - 1 + 2 * sl, corr_of(f))
           for ch, f in enumerate(NB.grid_carriers(n, sl))]
    X = XLaunch(f"expect_grid_n{n}_sl{sl}", L.cfg, list(L.cur), tab, seq=L.seq)
    for nb in (False, True):
        assert [_data(r, n) for r in X.recs(0, nb)] == [_data(L.nrecs(0, ch)[0], n) for ch in range(2)], (n, sl, nb)
    return X


# ------------------------------------------------------------------------------------------ a station that hops
TRACK_PATTERN = (2, 0, 1)                                    # a made-up hop pattern over three channels
TRACK_PERIOD = 1500                                          # outputs between packets (shortened from the Davis dwell)


def track_plan(n_packets, first=400, omit=()):
    """[(packet index, channel, first output of its burst)] of a station that hops TRACK_PATTERN every TRACK_PERIOD
    outputs, without the packets in ``omit``."""
    return [(j, TRACK_PATTERN[j % len(TRACK_PATTERN)], first + j * TRACK_PERIOD) for j in range(n_packets) if j not in omit]
