"""Helpers shared by tests/test_burst_repair_cpu.py and tests/test_burst_repair.py (no tests in here): the NumPy / Python
integer model of the CRC-guided repair of k_chan_burst_decode (include/rtldavis_hip.h, BURST DECODE, steps 5a, 5b, 6'),
written from the definition - it flips the symbols of every subset in the defined order and runs the CRC gate on the
bytes, where the kernel XORs a table of single-symbol CRCs against the syndrome -; the slot model of the hook
rd_debug_burst_decode_repair; the stream model with step 7; and the crafted launches: FSK written straight into
channelized bytes with single symbols damaged through the per-output frequency array.  The builders of
burst_decode_cases.py are imported, not repeated.  Every case asserts the edge it is built for on the model of its own
bytes when it is built.  Nothing here touches a device."""
import functools
import itertools

import numpy as np

import burst_cases as BC
import burst_decode_cases as DC
import retune_cases as RC
from rtldavis_amd import synth
from rtldavis_amd.wideband import BURST_MSG_DTYPE, BurstMessages

W, MAX_W, FILL = DC.W, DC.MAX_W, DC.FILL
LIST = 8                                                     # RD_BD_REPAIR_L
REPAIRED = 2                                                 # RD_BURST_MSG_REPAIRED
SYNC = tuple(int(ch) for ch in RC.PREAMBLE)


# ------------------------------------------------------------------------------------------ the definition
def crc_bitwise(bits):
    """CRC-16-CCITT (x^16 + x^12 + x^5 + 1, init 0) of a bit sequence, one bit at a time, the first bit first."""
    crc = 0
    for b in bits:
        top = ((crc >> 15) & 1) ^ int(b)
        crc = (crc << 1) & 0xFFFF
        if top:
            crc ^= 0x1021
    return crc


def crc_bit_order(n):
    """The symbol indices 16 .. n-1 in the order the CRC of the bit-swapped bytes [2:] takes them in: byte by byte, and
    inside a byte the LAST symbol first (on-air symbol 8 j + i is bit 7 - i of byte j, bit i of the swapped byte)."""
    return [8 * j + i for j in range(2, n // 8) for i in range(7, -1, -1)]


def syndrome(bits):
    """S of N symbols: the CRC of step 5 (0: the packet passes the gate)."""
    return crc_bitwise([bits[k] for k in crc_bit_order(len(bits))])


@functools.lru_cache(maxsize=None)
def syndrome_table(n):
    """E[k] for a packet of n symbols, uint16 [n] (0 for k < 16): through the byte-wise CRC of the package."""
    e = np.zeros(n, np.uint16)
    for k in range(16, n):
        one = np.zeros(n, np.uint8)
        one[k] = 1
        e[k] = synth._crc16_ccitt(bytes(synth._swap_bits8(b) for b in bytes(np.packbits(one))[2:]))
    return e


def ranked(s_symbols):
    """r_0 .. r_7: the payload symbols by (|s|, k) ascending, the first LIST."""
    return sorted(range(16, len(s_symbols)), key=lambda k: (abs(int(s_symbols[k])), k))[:LIST]


def subsets(max_flips):
    """The index sets into r of 5b, in order."""
    out = [(a,) for a in range(LIST)] if max_flips >= 1 else []
    if max_flips >= 2:
        out += [(a, b) for a in range(LIST) for b in range(a + 1, LIST)]
    return out


def repair_model(s_symbols, max_flips, sync=SYNC):
    """Steps 5, 5a, 5b for one candidate's N symbol sums: None, or (flips, bits, margin) - the flipped symbol indices
    ascending (() for a candidate that passes as it is), the corrected symbols and the margin of step 6'."""
    s = [int(v) for v in s_symbols]
    n = len(s)
    bits = [1 if v > 0 else 0 for v in s]
    if tuple(bits[:16]) != tuple(sync):
        return None
    if DC._crc_ok(bytes(np.packbits(bits))):
        return (), bits, min(abs(v) for v in s)
    r = ranked(s)
    for sub in subsets(max_flips):
        ks = tuple(sorted(r[a] for a in sub))
        fixed = list(bits)
        for k in ks:
            fixed[k] ^= 1
        if DC._crc_ok(bytes(np.packbits(fixed))):
            return ks, fixed, min(abs(v) for k, v in enumerate(s) if k not in ks)
    return None


def repair_batch(s, max_flips, sync=SYNC):
    """repair_model for many candidates at once, int64 [M, N] -> int [M]: -1 (no record), else the number of flips.  Uses
    the linearity of the CRC (the syndrome table) - tests/test_burst_repair_cpu.py holds it against repair_model."""
    s = np.asarray(s, np.int64)
    m, n = s.shape
    e = syndrome_table(n).astype(np.int64)
    bits = s > 0
    syn = np.bitwise_xor.reduce(np.where(bits, e[None, :], 0), axis=1)
    mag = np.abs(s[:, 16:])
    idx = np.argsort(mag, axis=1, kind="stable")[:, :LIST] + 16          # (stable: ties to the smaller k)
    el = e[idx]
    out = np.full(m, -1, np.int64)
    hit = np.zeros(m, bool)
    if max_flips >= 1:
        hit = (el == syn[:, None]).any(axis=1)
        out[hit] = 1
    if max_flips >= 2:
        two = np.zeros(m, bool)
        for a, b in itertools.combinations(range(LIST), 2):
            two |= (el[:, a] ^ el[:, b]) == syn
        out[two & ~hit] = 2
    out[syn == 0] = 0
    out[~np.all(bits[:, :16] == np.asarray(sync, bool)[None, :], axis=1)] = -1
    return out


def symbol_sums(cur, prev, rec, cfg, have_prev):
    """Steps 2 .. 4 for one run: None, or (taus, s [candidates, N], back, p_re, p_im, t0): every candidate tau of step 5's
    range with its N symbol sums, and p over t0 < t < t1."""
    sl, n, _, look = DC.shape(cfg)
    cre, cim = int(rec["corr_re"]), int(rec["corr_im"])
    if cre == 0 and cim == 0:
        return None
    back = bool(int(rec["flags"]) & 1) and have_prev
    t0 = W * int(rec["first"]) - (look if back else 0)
    t1 = W * (int(rec["first"]) + int(rec["windows"]))
    if t1 - t0 < n * sl + 1:
        return None
    a = 2 * (np.concatenate([prev, cur]) if back else cur).astype(np.int64) - 255
    org = cur.size // 2 if back else 0
    zi, zq = a[0::2][org + t0: org + t1], a[1::2][org + t0: org + t1]
    p_re = zi[1:] * zi[:-1] + zq[1:] * zq[:-1]               # p[t0 + 1 + j] at j
    p_im = zq[1:] * zi[:-1] - zi[1:] * zq[:-1]
    d = p_im * cre - p_re * cim
    s_all = np.convolve(d, np.ones(sl, np.int64), "valid")   # s[t0 + sl + j] at j (int64, exact: |s| < 2^54)
    taus = np.arange(max(t0 + sl, -sl * (n - 1)), t1 - sl * (n - 1))
    if taus.size == 0:
        return None
    s = s_all[(taus - t0 - sl)[:, None] + sl * np.arange(n)[None, :]]
    return taus, s, back, p_re, p_im, t0


def decode_run(cur, prev, rec, cfg, have_prev, max_flips):
    """Steps 2 .. 6' for one channel's bytes and one burst record: None, or (tau, flags, margin, f_re, f_im, data, ones,
    id, pad)."""
    sl, n, sync, _ = DC.shape(cfg)
    got = symbol_sums(cur, prev, rec, cfg, have_prev)
    if got is None:
        return None
    taus, s, back, p_re, p_im, t0 = got
    best = None
    for j in np.flatnonzero(np.all((s[:, :16] > 0) == np.asarray(sync, bool)[None, :], axis=1)):
        r = repair_model(s[j], max_flips, tuple(sync))
        if r is None:
            continue
        key = (len(r[0]), -r[2], int(taus[j]))               # (flips ascending, margin descending, tau ascending)
        if best is None or key < best[0]:
            best = (key, r)
    if best is None:
        return None
    (n_flip, neg_margin, tau), (ks, bits, _) = best
    data = bytes(np.packbits(bits))
    tt = np.arange(tau - sl + 1, tau + sl * (n - 1) + 1) - (t0 + 1)
    assert tt.size == n * sl and tt[0] >= 0
    pad = [n_flip] + list(ks) + [0] * (3 - len(ks))
    flags = (1 if back else 0) | (REPAIRED if n_flip else 0)
    return tau, flags, -neg_margin, int(p_re[tt].sum()), int(p_im[tt].sum()), data, int(sum(bits)), synth._swap_bits8(data[2]) & 7, pad


def _row(c, first, clock, got):
    tau, flags, margin, f_re, f_im, data, ones, ident, pad = got
    return (c, first, tau, flags, (int(clock) + tau) % 2 ** 64, margin, f_re, f_im, list(data) + [0] * (10 - len(data)), ones, ident, pad)


def decode_model(cur, prev, bursts, cfg, have_prev, clock, max_flips):
    """The BurstMessages of one chunk at max_flips, as burst_decode_cases.decode_model gives them at 0."""
    cur = np.atleast_2d(cur)
    long_runs = np.zeros(cur.shape[0], np.uint32)
    rows = []
    for rec in bursts.records:
        c = int(rec["channel"])
        if int(rec["windows"]) > MAX_W:
            long_runs[c] += 1
            continue
        got = decode_run(cur[c], None if prev is None else np.atleast_2d(prev)[c], rec, cfg, have_prev, max_flips)
        if got is not None:
            rows.append(_row(c, int(rec["first"]), clock, got))
    return BurstMessages(np.asarray(rows, BURST_MSG_DTYPE).reshape(-1), long_runs, int(bursts.chunk))


def decode_stream(blocks, thr, cfg, max_flips, clock0=0, bursts=None):
    """A receiver in NumPy with repair: burst_decode_cases.decode_stream with decode_model above; step 7 is the same."""
    out, prev, delivered = [], None, ()
    for k, block in enumerate(blocks):
        block = np.atleast_2d(block)
        b = BC.model_bursts(block, thr, k) if bursts is None else bursts[k]
        m = decode_model(block, prev, b, cfg, k >= 1, clock0 + k * (block.shape[1] // 2), max_flips)
        m = DC.drop_repeats(m, delivered, int(cfg.symbol_length))
        out.append((b, m))
        prev, delivered = block, m.records
    return out


def slot_model(L, max_flips):
    """What rd_debug_burst_decode_repair must hand back for a Launch: burst_decode_cases.slot_decode_model with repair."""
    n_ch, n_win = L.cur.shape[0], L.cur.shape[1] // (2 * W)
    cap = BC.cap_of(n_win)
    msgs = np.frombuffer(bytes([FILL]) * (n_ch * cap * BURST_MSG_DTYPE.itemsize), BURST_MSG_DTYPE).reshape(n_ch, cap).copy()
    n_msgs, long_runs = np.zeros(n_ch, np.uint32), np.zeros(n_ch, np.uint32)
    for c in range(n_ch):
        for rec in L.runs[c, : min(int(L.n_runs[c]), cap)]:
            first, windows = int(rec["first"]), int(rec["windows"])
            if windows > MAX_W:
                long_runs[c] += 1
                continue
            if windows == 0 or first >= n_win or first + windows > n_win:
                continue
            got = decode_run(L.cur[c], None if L.prev is None else L.prev[c], rec, L.cfg, L.prev is not None, max_flips)
            if got is not None:
                msgs[c, n_msgs[c]] = _row(c, first, L.clock, got)
                n_msgs[c] += 1
    return msgs, n_msgs, long_runs, np.full(n_ch, L.seq & 0xFFFFFFFF, np.uint32)


class Launch(DC.Launch):
    """A launch of the hook with what the model expects back at max_flips = 0, 1, 2 (``want[R]``); at 0 it is what
    burst_decode_cases' own slot model gives, asserted here."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.want = tuple(slot_model(self, r) for r in range(3))
        assert self.want[0][0].tobytes() == self.msgs.tobytes() and np.array_equal(self.want[0][1], self.n_msgs)

    def recs(self, r, c):
        return self.want[r][0][c, : int(self.want[r][1][c])]

    def counts(self, r):
        return [int(x) for x in self.want[r][1]]

    def sums(self, c, run=0):
        return symbol_sums(self.cur[c], None if self.prev is None else self.prev[c], self.runs[c, run], self.cfg, self.prev is not None)


# ------------------------------------------------------------------------------------------ crafted bytes
def burst_freqs(data, sl, scale=None, carrier=0.11, lead=64, trail=32, dev=None):
    """The per-output frequencies (cycles per output) of burst_decode_cases.fsk_burst, with symbol k's deviation
    multiplied by scale[k]: a negative factor gives a WRONG symbol (-0.4: weak, -1: of full magnitude), a factor in 0 .. 1
    a correct but weaker one."""
    dev = DC.deviation(sl) if dev is None else dev
    bits = np.unpackbits(np.frombuffer(bytes(data), np.uint8)).astype(np.float64)
    sym = np.where(bits == 1, dev, -dev)
    for k, f in (scale or {}).items():
        sym[k] *= f
    return np.concatenate([np.zeros(lead), np.repeat(sym, sl), np.zeros(trail)]) + carrier


def damaged(data, sl, scale, amp=DC.AMP, phase0=0.0, **kw):
    return DC.fsk_bytes(burst_freqs(data, sl, scale, **kw), amp, phase0)


def _quiet(seed, bs):
    return BC.quiet_bytes(np.random.default_rng(seed), bs)


def _pad(r):
    return tuple(int(x) for x in r["pad"])


def _data(r, n):
    return bytes(r["data"][: n // 8])


WEAK = -0.4                                                   # a weak wrong symbol: 0.4 of the deviation, the wrong sign


def _bits(data):
    return [int(b) for b in np.unpackbits(np.frombuffer(bytes(data), np.uint8))]


def lonely(bits, k):
    """Symbol k differs from both neighbours (the carrier behind the last symbol counts as neither).  A weak wrong symbol
    that is lonely is sent on its neighbours' side, so a tau a few outputs off - which lets a neighbour leak into the
    symbol's sum - leaves it wrong; between two symbols of its own value it would come out right there, and the packet
    would have an exact candidate."""
    return bits[k - 1] != bits[k] and (k + 1 == len(bits) or bits[k + 1] != bits[k])


def lonely_pair(bits, k):
    """Symbols k, k + 1 equal each other and differ from k - 1 and k + 2: both stay wrong at every tau when both are weak."""
    return bits[k] == bits[k + 1] and bits[k - 1] != bits[k] and (k + 2 == len(bits) or bits[k + 2] != bits[k])


def find_packet(n, want, seed0):
    """The first packet of burst_decode_cases.packet (seeds from seed0 on, the eight ids) whose symbols meet ``want``."""
    for seed in range(seed0, seed0 + 4000):
        data = DC.packet(n, ident=seed % 8, seed=seed)
        if want(_bits(data)):
            return data
    raise AssertionError("no packet with the wanted symbols")


def lonely_ks(data, lo=17):
    b = _bits(data)
    return [k for k in range(lo, len(b) - 1) if lonely(b, k)]


@functools.lru_cache(maxsize=None)
def one_flip_launch():
    """One weak wrong symbol at k = 16 (the first payload symbol), N - 1 (the CRC's last bit) and 23 / 24 (a byte seam),
    a channel each, SL 8: pad = (1, k, 0, 0) and the planted data at R = 1 and 2, nothing at R = 0."""
    sl, n, bs = 8, 80, 2048
    cfg = DC.config(sl, n, bs)
    ks = (16, n - 1, 23, 24)
    data = find_packet(n, lambda b: all(lonely(b, k) for k in ks), 1100)
    L = Launch("one_flip", cfg, [DC.put(_quiet(200 + c, bs), 300 + 5 * c, damaged(data, sl, {k: WEAK})) for c, k in enumerate(ks)])
    assert L.counts(0) == [0] * 4 and L.counts(1) == [1] * 4 == L.counts(2)
    for c, k in enumerate(ks):
        for r in (1, 2):
            m = L.recs(r, c)[0]
            assert _pad(m) == (1, k, 0, 0) and _data(m, n) == data and int(m["flags"]) == REPAIRED
            assert int(m["tau"]) == 300 + 5 * c + 64 + sl - 1 and int(m["ones"]) == bin(int.from_bytes(data, "big")).count("1")
    return L


@functools.lru_cache(maxsize=None)
def two_flips_launch():
    """Two weak wrong symbols: (16, N - 1), (40, 41) and (23, 24): nothing at R = 0 and 1, the record at R = 2."""
    sl, n, bs = 8, 80, 2048
    cfg = DC.config(sl, n, bs)
    pairs = ((16, n - 1), (40, 41), (23, 24))
    data = find_packet(n, lambda b: lonely(b, 16) and lonely(b, n - 1) and lonely_pair(b, 40) and lonely_pair(b, 23), 1200)
    L = Launch("two_flips", cfg, [DC.put(_quiet(210 + c, bs), 280 + 3 * c, damaged(data, sl, {a: WEAK, b: WEAK}))
                                  for c, (a, b) in enumerate(pairs)])
    assert L.counts(0) == [0] * 3 == L.counts(1) and L.counts(2) == [1] * 3
    for c, (a, b) in enumerate(pairs):
        m = L.recs(2, c)[0]
        assert _pad(m) == (2, a, b, 0) and _data(m, n) == data and int(m["flags"]) == REPAIRED
    return L


def _weaker(data, n, count, avoid):
    """``count`` payload positions, spread, none in or next to ``avoid``."""
    free = [k for k in range(17, n - 1, 2) if all(abs(k - a) > 1 for a in avoid)]
    assert len(free) >= count
    return free[:count]


@functools.lru_cache(maxsize=None)
def rank_edge_launch():
    """SL 1 (a symbol is one output: no neighbour leaks into it): a wrong symbol of half the deviation beside 7, 8 and 9
    correct symbols of a fifth of it.  With seven the wrong symbol is r_7 and is repaired; with eight or nine it is not
    in the list and nothing is reported."""
    sl, n, bs = 1, 40, 2048
    cfg = DC.config(sl, n, bs)
    data = DC.packet(n, seed=13)
    k = 30
    rows = []
    for c, count in enumerate((7, 8, 9)):
        scale = {k: -0.5}
        scale.update({j: 0.2 for j in _weaker(data, n, count, (k,))})
        rows.append(DC.put(_quiet(220 + c, bs), 300, damaged(data, sl, scale)))
    L = Launch("rank_edge", cfg, rows)
    for r in (1, 2):
        assert L.counts(r) == [1, 0, 0], (r, L.counts(r))
        assert _pad(L.recs(r, 0)[0]) == (1, k, 0, 0) and _data(L.recs(r, 0)[0], n) == data
    assert L.counts(0) == [0, 0, 0]
    for c, count in enumerate((7, 8, 9)):                    # the wrong symbol's rank at the packet's tau
        taus, s, *_ = L.sums(c)
        j = int(np.flatnonzero(taus == 300 + 64)[0])
        order = sorted(range(16, n), key=lambda q: (abs(int(s[j, q])), q))
        assert order.index(k) == count, (c, order.index(k))
    return L


@functools.lru_cache(maxsize=None)
def strong_wrong_launch():
    """A wrong symbol of full magnitude (it is not among the 8 weakest), and a wrong symbol among the first 16 (sync
    symbols are never flipped), weak: no record at any R."""
    sl, n, bs = 8, 80, 2048
    cfg = DC.config(sl, n, bs)
    data = find_packet(n, lambda b: lonely(b, 37), 1400)
    assert lonely(SYNC, 5) and lonely(SYNC, 4)
    rows = [DC.put(_quiet(230, bs), 300, damaged(data, sl, {37: -1.0})),
            DC.put(_quiet(231, bs), 300, damaged(data, sl, {5: WEAK})),
            DC.put(_quiet(232, bs), 300, damaged(data, sl, {4: WEAK}))]
    L = Launch("strong_wrong_and_sync_damage", cfg, rows)
    assert all(L.counts(r) == [0, 0, 0] for r in range(3)) and list(L.n_runs) == [1, 1, 1]
    taus, s, *_ = L.sums(0)                                  # the strong symbol is wrong at the packet's tau, and not in the list
    j = int(np.flatnonzero(taus == 300 + 64 + sl - 1)[0])
    bits = np.unpackbits(np.frombuffer(data, np.uint8))
    assert [q for q in range(n) if (s[j, q] > 0) != bool(bits[q])] == [37] and 37 not in ranked(s[j])
    for c, k in ((1, 5), (2, 4)):
        taus, s, *_ = L.sums(c)
        assert [q for q in range(n) if (s[j, q] > 0) != bool(bits[q])] == [k]
    return L


@functools.lru_cache(maxsize=None)
def alias_quads(n):
    """Every (a, b, c, d), a < b, c < d, (a, b) < (c, d), all distinct payload symbols, with E[a] ^ E[b] = E[c] ^ E[d]:
    a codeword of weight 4 - by brute force over the table."""
    e = syndrome_table(n)
    by = {}
    for a, b in itertools.combinations(range(16, n), 2):
        by.setdefault(int(e[a] ^ e[b]), []).append((a, b))
    return [(p + q) for v in by.values() for p, q in itertools.combinations(v, 2) if len(set(p + q)) == 4]


@functools.lru_cache(maxsize=None)
def alias_pair_launch():
    """Two pairs inside the list with the same syndrome.  The wrong symbols are (c, d); (a, b) are correct.  Channel 0:
    (a, b) are the weaker pair, r_0 r_1, and are tried first: the record flips (a, b) - a valid packet, not the planted
    one.  Channel 1: (c, d) are the weaker pair and the planted packet comes back.  SL 1."""
    sl, n, bs = 1, 80, 2048
    cfg = DC.config(sl, n, bs)
    data = DC.packet(n, seed=15)
    quad = next(q for q in alias_quads(n) if all(abs(x - y) > 1 for x, y in itertools.combinations(q, 2)))
    a, b, c, d = quad
    rows = [DC.put(_quiet(240, bs), 300, damaged(data, sl, {a: 0.15, b: 0.2, c: -0.4, d: -0.5})),
            DC.put(_quiet(241, bs), 300, damaged(data, sl, {a: 0.4, b: 0.5, c: -0.15, d: -0.2}))]
    L = Launch("alias_pair", cfg, rows)
    assert L.counts(0) == [0, 0] == L.counts(1) and L.counts(2) == [1, 1]
    m0, m1 = L.recs(2, 0)[0], L.recs(2, 1)[0]
    assert _pad(m0) == (2, a, b, 0) and _data(m0, n) != data and DC._crc_ok(_data(m0, n))
    assert _pad(m1) == (2, c, d, 0) and _data(m1, n) == data
    taus, s, *_ = L.sums(0)
    r = ranked(s[int(np.flatnonzero(taus == 300 + 64)[0])])
    assert set(r[:4]) == {a, b, c, d} and set(r[:2]) == {a, b}
    return L, quad


TIE_GRID = 32                                                 # rank_tie: every frequency is a multiple of 1 / 32 cycle per output


@functools.lru_cache(maxsize=None)
def rank_tie_launch():
    """Carrier 8 / 32, deviation 4 / 32 cycles per output, SL 1, phase0 1 / 64 cycle: the phase moves on a grid of 32
    points none of which lies on an axis, so the bytes repeat and equal steps from equivalent phases give EQUAL 64-bit
    sums.  Seven correct symbols at a quarter of the deviation fill r_0 .. r_6; the wrong symbol x and a correct symbol
    y, both at half the deviation on the same side, have equal |s| and compete for r_7: the smaller k gets it.  Channel
    0, x < y: repaired.  Channel 1, the roles swapped (y' = x is correct, x' = y is wrong): not repaired."""
    sl, n, bs = 1, 40, 2048
    cfg = DC.config(sl, n, bs)
    kw = dict(carrier=8 / TIE_GRID, dev=4 / TIE_GRID, phase0=2 * np.pi / 64)
    for seed in range(40):
        data = DC.packet(n, seed=300 + seed)
        bits = np.unpackbits(np.frombuffer(data, np.uint8))
        for x, y in itertools.combinations(range(17, n - 1), 2):
            if bits[x] == bits[y] or y - x < 2:
                continue
            weak = {j: 0.25 for j in _weaker(data, n, 7, (x, y))}
            # x true bit b sent at -0.5 (wrong), y true bit 1 - b sent at +0.5 (correct): the same step
            rows = [DC.put(_quiet(250, bs), 300, damaged(data, sl, {**weak, x: -0.5, y: 0.5}, **kw)),
                    DC.put(_quiet(251, bs), 300, damaged(data, sl, {**weak, x: 0.5, y: -0.5}, **kw))]
            probe = DC.Launch("probe", cfg, rows)
            got = [symbol_sums(probe.cur[c], None, probe.runs[c, 0], cfg, False) for c in (0, 1)]
            if any(g is None for g in got):
                continue
            eq = []
            for taus, s, *_ in got:
                j = int(np.flatnonzero(taus == 300 + 64)[0])
                eq.append(abs(int(s[j, x])) == abs(int(s[j, y])) and set(ranked(s[j])[:7]) == set(weak) and
                          sorted(range(16, n), key=lambda q: (abs(int(s[j, q])), q))[7:9] == [x, y])
            if all(eq):
                L = Launch("rank_tie", cfg, rows)
                assert L.counts(0) == [0, 0] and L.counts(1) == [1, 0], L.counts(1)
                m = L.recs(1, 0)[0]
                assert _pad(m) == (1, x, 0, 0) and _data(m, n) == data
                return L, (x, y)
    raise AssertionError("rank_tie: no pair of symbols with equal sums found")


@functools.lru_cache(maxsize=None)
def winner_launch():
    """Step 6' inside one run (the stretch between the packets is carrier).  Channel 0, exact_beats_repaired: a damaged
    packet of amplitude 60 and, later, an exact one of amplitude 30: the exact one at every R.  Channel 1,
    fewer_flips_first: a two-flip packet of amplitude 60 earlier, a one-flip packet of amplitude 30 later: the one-flip
    packet at R = 1 and R = 2.  Channel 2, repaired_tie: two byte-identical one-flip copies 300 outputs apart: the
    smaller tau."""
    sl, n, bs = 2, 40, 2048
    cfg = DC.config(sl, n, bs)
    d1, d2 = DC.packet(n, ident=1, seed=16), DC.packet(n, ident=2, seed=17)
    kw = dict(lead=8, trail=4)

    def row(seed, first, second, gap=300):
        r = DC.put(_quiet(seed, bs), 128, DC.fsk_bytes(np.full(gap + 300, 0.11)))
        DC.put(r, 170, first)
        return DC.put(r, 170 + gap, second)

    rows = [row(260, damaged(d1, sl, {20: WEAK}, amp=60, **kw), damaged(d2, sl, None, amp=30, **kw)),
            row(261, damaged(d1, sl, {20: WEAK, 30: WEAK}, amp=60, **kw), damaged(d2, sl, {25: WEAK}, amp=30, **kw)),
            row(262, damaged(d1, sl, {20: WEAK}, **kw), damaged(d1, sl, {20: WEAK}, **kw))]
    L = Launch("winner", cfg, rows)
    assert list(L.n_runs) == [1, 1, 1]
    t_a, t_b = 170 + 8 + sl - 1, 170 + 300 + 8 + sl - 1
    assert L.counts(0) == [1, 0, 0] and L.counts(1) == [1, 1, 1] == L.counts(2)
    for r in range(3):                                       # the exact packet, although the damaged one is louder
        m = L.recs(r, 0)[0]
        assert int(m["tau"]) == t_b and _data(m, n) == d2 and _pad(m) == (0, 0, 0, 0) and int(m["flags"]) == 0
    alone = Launch("probe", cfg, [row(260, damaged(d1, sl, {20: WEAK}, amp=60, **kw), DC.fsk_bytes(np.full(100, 0.11)))])
    assert alone.counts(1) == [1] and int(alone.recs(1, 0)[0]["margin"]) > int(L.recs(1, 0)[0]["margin"])
    for r in (1, 2):
        m = L.recs(r, 1)[0]
        assert int(m["tau"]) == t_b and _data(m, n) == d2 and _pad(m) == (1, 25, 0, 0)
    two = Launch("probe", cfg, [row(261, damaged(d1, sl, {20: WEAK, 30: WEAK}, amp=60, **kw), DC.fsk_bytes(np.full(100, 0.11)))])
    assert two.counts(2) == [1] and _pad(two.recs(2, 0)[0]) == (2, 20, 30, 0) and int(two.recs(2, 0)[0]["margin"]) > int(L.recs(2, 1)[0]["margin"])
    for r in (1, 2):
        m = L.recs(r, 2)[0]
        assert int(m["tau"]) == t_a and _pad(m) == (1, 20, 0, 0) and _data(m, n) == d1
    taus, s, *_ = L.sums(2)                                  # the later copy is the same candidate, 300 outputs on
    ja, jb = (int(np.flatnonzero(taus == t)[0]) for t in (t_a, t_b))
    assert np.array_equal(s[ja], s[jb])
    return L


@functools.lru_cache(maxsize=None)
def seam_launches():
    """The damaged packet straddles the chunk boundary (its last output at boundary + 200) and is reached by the
    look-back of chunk 1: flags = 3 at R = 1; chunk 0 alone reports nothing."""
    sl, n, bs = 14, 80, 2048
    cfg = DC.config(sl, n, bs)
    data = find_packet(n, lambda b: lonely(b, 44), 1800)
    both = DC.put(_quiet(270, 2 * bs), bs + 200 - (n * sl - 1) - 56, damaged(data, sl, {44: WEAK}, lead=56, trail=300))
    b0, b1 = both[: 2 * bs], both[2 * bs:]
    first = Launch("repair_seam_chunk0", cfg, [b0], seq=0)
    back = Launch("repair_seam_chunk1", cfg, [b1], prev=[b0], clock=bs, seq=1)
    assert all(first.counts(r) == [0] for r in range(3))
    assert back.counts(0) == [0] and back.counts(1) == [1] == back.counts(2)
    m = back.recs(1, 0)[0]
    assert int(m["flags"]) == 3 and _pad(m) == (1, 44, 0, 0) and _data(m, n) == data and int(m["tau"]) < 0
    assert int(m["tau"]) + sl * (n - 1) >= 0
    return first, back, (b0, b1), cfg, data


def seam_stream(max_flips):
    """The seam's two chunks through the stream model: the packet is reported once, by chunk 1."""
    _, _, (b0, b1), cfg, data = seam_launches()
    out = decode_stream([b0[None, :], b1[None, :]], DC.THR, cfg, max_flips)
    return [m for _, m in out], data


@functools.lru_cache(maxsize=None)
def longest_launch():
    """burst_decode_cases.longest_launch with a weak wrong symbol: SL 25, a run of 32 windows and 16 of look-back, all
    of the kernel's LDS with the repair's table beside it."""
    sl, n, bs = 25, 80, 4096
    cfg = DC.config(sl, n, bs)
    data = find_packet(n, lambda b: lonely(b, 61), 1900)
    both = DC.put(_quiet(280, 2 * bs), bs - 1000 - 100, damaged(data, sl, {61: WEAK}, lead=100, trail=bs - 1000))
    L = Launch("repair_longest_region", cfg, [both[2 * bs:]], prev=[both[: 2 * bs]], clock=7 * bs, seq=7)
    assert list(L.n_runs) == [1] and int(L.runs[0, 0]["windows"]) == 32 and int(L.runs[0, 0]["flags"]) == 3
    assert L.counts(0) == [0] and L.counts(1) == [1] == L.counts(2)
    m = L.recs(2, 0)[0]
    assert int(m["tau"]) == -1000 + sl - 1 and int(m["flags"]) == 3 and _pad(m) == (1, 61, 0, 0) and _data(m, n) == data
    return L


GRID = tuple((n, sl) for n in (40, 64, 80) for sl in (1, 8, 14))


@functools.lru_cache(maxsize=None)
def grid_launch(n, sl):
    """One weak wrong symbol per channel (above and below the channel's centre) for N 40, 64, 80 x SL 1, 8, 14."""
    bs = 2048
    cfg = DC.config(sl, n, bs)
    data = find_packet(n, lambda b: sum(lonely(b, k) for k in range(17, n - 1)) >= 2, 2000 + 10 * (n + sl))
    ks = (lonely_ks(data)[0], lonely_ks(data)[-1])
    rows = [DC.put(_quiet(290 + c, bs), 200 + 17 * c, damaged(data, sl, {ks[c]: WEAK}, carrier=f)) for c, f in enumerate((0.11, -0.07))]
    L = Launch(f"repair_grid_n{n}_sl{sl}", cfg, rows, seq=2 ** 32 + n)
    assert L.counts(0) == [0, 0] and L.counts(1) == [1, 1] == L.counts(2), (n, sl, L.counts(1))
    for c in range(2):
        m = L.recs(1, c)[0]
        assert _pad(m) == (1, ks[c], 0, 0) and _data(m, n) == data and not m["data"][n // 8:].any() and int(m["id"]) == synth._swap_bits8(data[2]) & 7
    return L


def saturated_fsk(data, sl, turns, lead, trail):
    """Bytes 0 and 255 only, as burst_decode_cases._saturated_fsk, with the turning outputs given per symbol: symbol k
    steps by 90 degrees x sign(turns[k]) for |turns[k]| outputs and by 180 degrees for the rest."""
    step = np.concatenate([np.where(np.arange(sl) < abs(int(t)), 1 if t > 0 else -1, 2) for t in turns])
    quad = np.cumsum(np.concatenate([np.zeros(lead, np.int64), step, np.zeros(trail, np.int64)])) % 4
    out = np.empty(2 * quad.size, np.uint8)
    out[0::2], out[1::2] = 255 * np.isin(quad, (0, 3)), 255 * np.isin(quad, (0, 1))
    return out


@functools.lru_cache(maxsize=None)
def saturated_launch():
    """Saturated bytes and a correlation sum of (2^30 - 1000, 1000): |s| up to 2^51.  With u = 2 x 65025, a symbol sent with
    t turning outputs has |s| = u (corr_re t + corr_im (14 - t)) when it reads 1 and u (corr_re t - corr_im (14 - t)) when
    it reads 0: the same t, the same high word, another low word.  Six correct 0s of 9 turns are r_0 .. r_5; the wrong
    symbol x, a 1 sent with 10 turns the wrong way, reads 0 and is r_6, in front of all the correct 1s of 10 turns, which
    have its high word and larger low words (the other 0s have 11 turns).  Ranked by the high words alone x ties with
    the 1s and loses to the smaller k; ranked by the low words alone it is nowhere near: only all 64 bits repair it."""
    sl, n, bs = 14, 80, 2048
    cfg = DC.config(sl, n, bs)
    data = DC.packet(n, seed=20)
    bits = _bits(data)
    ones = [k for k in range(17, n) if bits[k] == 1]
    wrong = [k for k in ones if lonely(bits, k)][-1]         # (lonely: no tau lets a neighbour's turns put it right)
    assert sum(k < wrong for k in ones) >= 4
    zeros = [k for k in range(17, n) if bits[k] == 0 and abs(k - wrong) > 1]
    turns = np.where(np.asarray(bits) == 1, 10, -11)
    turns[wrong] = -10
    turns[zeros[1:12:2]] = -9
    row = DC.put(_quiet(295, bs), 3 * W, saturated_fsk(data, sl, turns, 40, 40))
    runs, n_runs = DC.runs_of(row[None, :], DC.THR)
    assert n_runs[0] == 1
    runs[0, 0]["corr_re"], runs[0, 0]["corr_im"] = 2 ** 30 - 1000, 1000   # (at 2^30 - 1 the classes straddle a multiple of 2^32)
    L = Launch("repair_saturated", cfg, [row], runs=runs, n_runs=n_runs)
    assert L.counts(0) == [0] and L.counts(1) == [1] == L.counts(2)
    m = L.recs(1, 0)[0]
    assert _pad(m) == (1, wrong, 0, 0) and _data(m, n) == data
    taus, s, *_ = L.sums(0)
    sj = s[int(np.flatnonzero(taus == int(m["tau"]))[0])]
    mags = [abs(int(sj[k])) for k in range(n)]
    full = ranked(sj)
    assert max(mags) > 2 ** 50 and min(mags[k] for k in full) > 2 ** 49 and full[6] == wrong
    low = sorted(range(16, n), key=lambda k: (mags[k] & 0xFFFFFFFF, k))[:LIST]
    high = sorted(range(16, n), key=lambda k: (mags[k] >> 32, k))[:LIST]
    assert wrong not in low and wrong not in high, (full, low, high)
    return L


def crafted_launches():
    """Every launch of the crafted repair cases, each with its conditions asserted."""
    first, back, *_ = seam_launches()
    return (one_flip_launch(), two_flips_launch(), rank_edge_launch(), strong_wrong_launch(), alias_pair_launch()[0],
            rank_tie_launch()[0], winner_launch(), first, back, longest_launch(), saturated_launch()) + tuple(
                grid_launch(n, sl) for n, sl in GRID)


# ------------------------------------------------------------------------------------------ noisy bursts (the gain)
GAIN_SL, GAIN_BS = 14, 2048
GAIN_PERIOD = 2 * GAIN_BS                                     # one burst per two chunks, inside the first of them


def gain_payloads(k):
    return [synth.make_packet(j % 8, bytes(np.random.default_rng(5000 + j).integers(0, 256, 6, dtype=np.uint8))) for j in range(k)]


def gain_blocks(k, noise, seed, cfo=1500.0):
    """K bursts of synth.synth_bursts, one every GAIN_PERIOD samples of one stream with noise ``noise``, as the chunks of
    one channel (the stream IS the channel's bytes: it lies at -Fs / 4 like a channelized one)."""
    datas = gain_payloads(k)
    bursts = [(d, j * GAIN_PERIOD + 200, cfo) for j, d in enumerate(datas)]
    raw = synth.synth_bursts(bursts, k * GAIN_PERIOD, seed, GAIN_SL, amplitude=0.3, noise=noise)
    return datas, [raw[None, 2 * GAIN_BS * j: 2 * GAIN_BS * (j + 1)] for j in range(2 * k)]


def gain_threshold(noise, amplitude=0.3):
    """Half way (geometrically) between a window of noise and a window of burst, in the units of p_w."""
    a2 = 4 * 127.6 ** 2 * W
    return int(a2 * np.sqrt((2 * noise ** 2) * (amplitude ** 2 + 2 * noise ** 2)))


def gain_run(k, noise, seed, flips=(0, 1, 2)):
    """{R: [records]} of the stream model over gain_blocks, and the planted payloads."""
    datas, blocks = gain_blocks(k, noise, seed)
    cfg = DC.config(GAIN_SL, 80, GAIN_BS)
    thr = gain_threshold(noise)
    bursts = [BC.model_bursts(b, thr, j) for j, b in enumerate(blocks)]
    out = {}
    for r in flips:
        out[r] = [rec for _, m in decode_stream(blocks, thr, cfg, r, bursts=bursts) for rec in m.records]
    return datas, out


# ------------------------------------------------------------------------------------------ the device capture
# burst_decode_cases' symbol_length 8 plan (device_receiver(bs, 8, offsets_hz=S8_OFFSETS_HZ), "s16", decim 4) with damaged
# bursts: (channel, first output, Hz off the channel's centre, {symbol: factor of its deviation}) - the packet of burst j
# is cap_packets()[j].  The channel filter smears a damaged symbol into its neighbours, so the symbols are lonely ones
# and several strengths are planted; what the device's bytes hold is for the model to say (tests/test_burst_repair.py).
CAP_BS = (1024, 2048)
CAP_OUTPUTS = 8 * 1024
CAP_BURSTS = ((1, 2048 + 300, 20000, {30: -0.5}),             # one flip, crosses 3072
              (2, 3072 + 500, -30000, {}),                    # undamaged, crosses 4096
              (0, 4096 + 200, 25000, {41: -0.5, 66: -0.6}),   # two flips, crosses 5120
              (1, 5120 + 400, 20000, {52: -1.0}),             # a strong wrong symbol
              (2, 6144 + 30, -30000, {27: -0.7}),             # one flip, inside 6144 .. 7167
              (0, 7168 + 40, 25000, {5: -0.5}))               # a wrong sync symbol (the last burst ends at 8168)


@functools.lru_cache(maxsize=None)
def cap_packets():
    out = []
    for j, (_, _, _, scale) in enumerate(CAP_BURSTS):
        ks = [k for k in scale if k >= 16]
        out.append(find_packet(80, lambda b: all(lonely(b, k) for k in ks), 3000 + 100 * j))
    return out


@functools.lru_cache(maxsize=None)
def cap_capture(sl=8, decim=DC.DEV_DECIM, amplitude=0.12, noise=0.004):
    """int16 I,Q of CAP_OUTPUTS x decim samples, made the way burst_decode_cases.s8_capture makes its own."""
    fw = decim * 19200 * sl
    n = CAP_OUTPUTS * decim
    rng = np.random.default_rng(909)
    x = noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for (c, start, hz, scale), data in zip(CAP_BURSTS, cap_packets()):
        bits = np.concatenate([np.tile(np.array([1, 0], np.uint8), 16), np.unpackbits(np.frombuffer(data, np.uint8)), np.zeros(8, np.uint8)])
        dev = np.where(bits == 1, 4800.0, -4800.0)
        for k, f in scale.items():
            dev[32 + k] *= f
        freq = float(DC.S8_OFFSETS_HZ[c] + hz) + np.repeat(dev, sl * decim)
        lo = start * decim
        x[lo: lo + freq.size] += amplitude * np.exp(2j * np.pi * np.cumsum(freq) / fw)
    out = np.empty(2 * n, np.int16)
    out[0::2] = np.clip(np.rint(x.real * 32768.0), -32768, 32767)
    out[1::2] = np.clip(np.rint(x.imag * 32768.0), -32768, 32767)
    return out
