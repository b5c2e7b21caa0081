"""Helpers shared by tests/test_burst_narrow_cpu.py, tests/test_burst_narrow.py and tools/burst_narrow_gain.py (no tests
in here): the NumPy / Python integer model of the narrow-band filter of k_chan_burst_decode (include/rtldavis_hip.h,
BURST DECODE, step 4n), written from the definition - the tables from the float64 formula, the grid choice in Python
integers, the filter as a convolution of the zero-extended region, a shift, a multiply - where the kernel looks the taps
up in a device table, pads the region in LDS and runs packed 16-bit dot products.  Steps 5 .. 7 are
burst_repair_cases' (repair_model, drop_repeats); with narrow off every function here hands the work to that module.
The crafted launches follow, each with the edge it is built for asserted on the model of its own bytes when it is
built.  Nothing here touches a device."""
import functools

import numpy as np

import burst_cases as BC
import burst_decode_cases as DC
import burst_repair_cases as RP
from rtldavis_amd import synth
from rtldavis_amd.wideband import BURST_MSG_DTYPE, BurstMessages

W, MAX_W, FILL = DC.W, DC.MAX_W, DC.FILL
GRID = 64                                                    # RD_BD_NB_GRID
SHIFT = 11                                                   # RD_BD_NB_SHIFT
NARROW = 4                                                   # RD_BURST_MSG_NARROW
MIN_SL = 4
Y_MAX = 3192                                                 # |y| per component (the header's bound)
SUM_ABS = {4: 25633, 8: 24727, 14: 23986, 25: 23471, 51: 23181}   # max over g of sum_k |H.re| + |H.im|


# ------------------------------------------------------------------------------------------ the definition
@functools.lru_cache(maxsize=None)
def table(sl):
    """(H, C) of step 4n from the formula: H int64 [64, T, 2] with H[g][k] at [g, k + M], C int64 [64, 2].  Every product
    and quotient in the order of the definition; the sum of the window runs over k ascending."""
    assert sl >= MIN_SL
    t, m = 2 * sl + 5, sl + 2
    k = np.arange(-m, m + 1)
    w = 0.54 + 0.46 * np.cos(2.0 * np.pi * k / (t - 1))
    x = 1.8 * k / sl
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(k == 0, 1.0, np.sin(np.pi * x) / (np.pi * x))
    raw = sinc * w
    total = 0.0
    for v in raw:
        total += float(v)
    h = raw / total
    g = np.arange(GRID)
    a = 2.0 * np.pi * ((g[:, None] * k[None, :]) % GRID) / GRID          # (reduced in integers; % is the floor's: 0 .. 63)
    hk = 16384.0 * h
    H = np.stack([np.rint(hk[None, :] * np.cos(a)), np.rint(hk[None, :] * np.sin(a))], axis=-1).astype(np.int64)
    ac = 2.0 * np.pi * g / GRID
    C = np.stack([np.rint(16384.0 * np.cos(ac)), np.rint(16384.0 * np.sin(ac))], axis=-1).astype(np.int64)
    return H, C


def library_table(sl):
    """The same from rd_bd_narrow_table (host code: no device), as int64 arrays."""
    from rtldavis_amd import _lib
    t = 2 * sl + 5
    taps, centres = np.zeros((GRID, t, 2), np.int16), np.zeros((GRID, 2), np.int16)
    _lib.check(_lib.lib().rd_bd_narrow_table(sl, taps.ctypes.data, centres.ctypes.data))
    return taps.astype(np.int64), centres.astype(np.int64)


def grid_choice(cre, cim, sl=MIN_SL):
    """(sh, ca, cb, g) of a run's correlation sum, in Python integers."""
    cre, cim = int(cre), int(cim)
    assert cre or cim
    sh = max(0, max(abs(cre), abs(cim)).bit_length() - 15)
    ca, cb = cre >> sh, cim >> sh                            # (floor)
    assert ca or cb
    C = table(sl)[1]                                         # (C does not depend on SL)
    score = [ca * int(C[g, 0]) + cb * int(C[g, 1]) for g in range(GRID)]
    assert max(abs(v) for v in score) < 2 ** 30
    return sh, ca, cb, score.index(max(score))               # the smallest g among the largest


def filter_region(zi, zq, hg):
    """acc and y over a region (int64 arrays of z's parts, zero outside): acc[t] = sum_k H[g][k] z[t - k], complex;
    y = (acc + 2^10) >> 11 per part."""
    m = (hg.shape[0] - 1) // 2
    hr, hi = hg[:, 0], hg[:, 1]
    full = lambda x, h: np.convolve(x, h)[m: m + x.size]     # sum_j h[j] x[t + M - j], j = k + M
    acc_re = full(zi, hr) - full(zq, hi)
    acc_im = full(zq, hr) + full(zi, hi)
    assert max(np.abs(acc_re).max(), np.abs(acc_im).max()) < 2 ** 23
    y_re, y_im = (acc_re + (1 << (SHIFT - 1))) >> SHIFT, (acc_im + (1 << (SHIFT - 1))) >> SHIFT
    assert max(np.abs(y_re).max(), np.abs(y_im).max()) <= Y_MAX
    return (acc_re, acc_im), (y_re, y_im)


def region_of(cur, prev, rec, cfg, have_prev):
    """Steps 2, 3: None, or (back, t0, t1, zi, zq) with z over t0 <= t < t1."""
    sl, n, _, look = DC.shape(cfg)
    if int(rec["corr_re"]) == 0 and int(rec["corr_im"]) == 0:
        return None
    back = bool(int(rec["flags"]) & 1) and have_prev
    t0 = W * int(rec["first"]) - (look if back else 0)
    t1 = W * (int(rec["first"]) + int(rec["windows"]))
    if t1 - t0 < n * sl + 1:
        return None
    a = 2 * (np.concatenate([prev, cur]) if back else cur).astype(np.int64) - 255
    org = cur.size // 2 if back else 0
    return back, t0, t1, a[0::2][org + t0: org + t1], a[1::2][org + t0: org + t1]


def symbol_sums(cur, prev, rec, cfg, have_prev, tab=None):
    """Steps 2, 3, 4n for one run: None, or (taus, s [candidates, N], back, p_re, p_im, t0, g) as burst_repair_cases'
    symbol_sums gives them for step 4, with p' for p and the grid point g."""
    sl, n, _, _ = DC.shape(cfg)
    got = region_of(cur, prev, rec, cfg, have_prev)
    if got is None:
        return None
    back, t0, t1, zi, zq = got
    H, _ = table(sl) if tab is None else tab
    _, ca, cb, g = grid_choice(rec["corr_re"], rec["corr_im"], sl)
    _, (y_re, y_im) = filter_region(zi, zq, H[g])
    p_re = y_re[1:] * y_re[:-1] + y_im[1:] * y_im[:-1]       # p'[t0 + 1 + j] at j
    p_im = y_im[1:] * y_re[:-1] - y_re[1:] * y_im[:-1]
    assert max(np.abs(p_re).max(), np.abs(p_im).max()) < 2 ** 25
    ones = np.ones(sl, np.int64)
    assert max(np.abs(np.convolve(p_re, ones, "valid")).max(), np.abs(np.convolve(p_im, ones, "valid")).max()) < 2 ** 31
    d = p_im * ca - p_re * cb
    s_all = np.convolve(d, ones, "valid")                    # s[t0 + sl + j] at j
    assert np.abs(s_all).max() < 2 ** 47
    taus = np.arange(max(t0 + sl, -sl * (n - 1)), t1 - sl * (n - 1))
    if taus.size == 0:
        return None
    s = s_all[(taus - t0 - sl)[:, None] + sl * np.arange(n)[None, :]]
    return taus, s, back, p_re, p_im, t0, g


def decode_run(cur, prev, rec, cfg, have_prev, max_flips, narrow=True, tab=None):
    """Steps 2 .. 6' for one run: None, or (tau, flags, margin, f_re, f_im, data, ones, id, pad).  narrow off:
    burst_repair_cases.decode_run."""
    if not narrow:
        return RP.decode_run(cur, prev, rec, cfg, have_prev, max_flips)
    sl, n, sync, _ = DC.shape(cfg)
    got = symbol_sums(cur, prev, rec, cfg, have_prev, tab)
    if got is None:
        return None
    taus, s, back, p_re, p_im, t0, g = got
    best = None
    for j in np.flatnonzero(np.all((s[:, :16] > 0) == np.asarray(sync, bool)[None, :], axis=1)):
        r = RP.repair_model(s[j], max_flips, tuple(sync))    # steps 5, 5a, 5b
        if r is None:
            continue
        key = (len(r[0]), -r[2], int(taus[j]))               # step 6'
        if best is None or key < best[0]:
            best = (key, r)
    if best is None:
        return None
    (n_flip, neg_margin, tau), (ks, bits, _) = best
    data = bytes(np.packbits(bits))
    tt = np.arange(tau - sl + 1, tau + sl * (n - 1) + 1) - (t0 + 1)
    assert tt.size == n * sl and tt[0] >= 0
    f_re, f_im = int(p_re[tt].sum()), int(p_im[tt].sum())
    assert max(abs(f_re), abs(f_im)) < 2 ** 36
    pad = [n_flip] + list(ks) + [0] * (2 - len(ks)) + [g]
    flags = (1 if back else 0) | (RP.REPAIRED if n_flip else 0) | NARROW
    return tau, flags, -neg_margin, f_re, f_im, data, int(sum(bits)), synth._swap_bits8(data[2]) & 7, pad


def decode_model(cur, prev, bursts, cfg, have_prev, clock, max_flips, narrow=True, tab=None):
    """The BurstMessages of one chunk."""
    if not narrow:
        return RP.decode_model(cur, prev, bursts, cfg, have_prev, clock, max_flips)
    cur = np.atleast_2d(cur)
    long_runs = np.zeros(cur.shape[0], np.uint32)
    rows = []
    for rec in bursts.records:
        c = int(rec["channel"])
        if int(rec["windows"]) > MAX_W:
            long_runs[c] += 1
            continue
        got = decode_run(cur[c], None if prev is None else np.atleast_2d(prev)[c], rec, cfg, have_prev, max_flips, True, tab)
        if got is not None:
            rows.append(RP._row(c, int(rec["first"]), clock, got))
    return BurstMessages(np.asarray(rows, BURST_MSG_DTYPE).reshape(-1), long_runs, int(bursts.chunk))


def decode_stream(blocks, thr, cfg, max_flips, narrow=True, clock0=0, bursts=None, tab=None):
    """A receiver in NumPy; step 7 is burst_decode_cases'.  narrow off: burst_repair_cases.decode_stream."""
    if not narrow:
        return RP.decode_stream(blocks, thr, cfg, max_flips, clock0=clock0, bursts=bursts)
    out, prev, delivered = [], None, ()
    for k, block in enumerate(blocks):
        block = np.atleast_2d(block)
        b = BC.model_bursts(block, thr, k) if bursts is None else bursts[k]
        m = decode_model(block, prev, b, cfg, k >= 1, clock0 + k * (block.shape[1] // 2), max_flips, True, tab)
        m = DC.drop_repeats(m, delivered, int(cfg.symbol_length))
        out.append((b, m))
        prev, delivered = block, m.records
    return out


def slot_model(L, max_flips, tab=None):
    """What rd_debug_burst_decode_narrow must hand back for a Launch at narrow = 1."""
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
            got = decode_run(L.cur[c], None if L.prev is None else L.prev[c], rec, L.cfg, L.prev is not None, max_flips, True, tab)
            if got is not None:
                msgs[c, n_msgs[c]] = RP._row(c, first, L.clock, got)
                n_msgs[c] += 1
    return msgs, n_msgs, long_runs, np.full(n_ch, L.seq & 0xFFFFFFFF, np.uint32)


class Launch(RP.Launch):
    """A launch of the hook with what the model expects back at narrow = 1 and max_flips = 0, 1, 2 (``narrow[R]``);
    ``want[R]`` stays what burst_repair_cases expects at narrow = 0."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.narrow = tuple(slot_model(self, r) for r in range(3))

    def nrecs(self, r, c):
        return self.narrow[r][0][c, : int(self.narrow[r][1][c])]

    def ncounts(self, r):
        return [int(x) for x in self.narrow[r][1]]

    def nsums(self, c, run=0):
        return symbol_sums(self.cur[c], None if self.prev is None else self.prev[c], self.runs[c, run], self.cfg, self.prev is not None)


# ------------------------------------------------------------------------------------------ crafted bytes
def _quiet(seed, bs):
    return BC.quiet_bytes(np.random.default_rng(seed), bs)


def _pad(r):
    return tuple(int(x) for x in r["pad"])


def _data(r, n):
    return bytes(r["data"][: n // 8])


NGRID = tuple((n, sl) for n in (40, 64, 80) for sl in (4, 8, 14, 25, 51) if n * sl + 1 <= 2048)


def grid_carriers(n, sl):
    """Two carriers (cycles per output) of a packet shape, spread over the band so that every channel of every shape
    meets another grid point."""
    j = NGRID.index((n, sl))
    return tuple(-0.45 + 0.9 * (2 * j + c) / (2 * len(NGRID)) for c in (0, 1))


@functools.lru_cache(maxsize=None)
def grid_launch(n, sl):
    """One decodable burst per channel, each at a carrier of its own, for every packet shape step 4n admits."""
    bs = 4096 if n * sl > 1500 else 2048
    cfg = DC.config(sl, n, bs)
    data = DC.packet(n, ident=(n + sl) % 8, seed=n + sl)
    rows = [DC.put(_quiet(400 + k, bs), 200 + 17 * k, DC.fsk_burst(data, sl, carrier=f)) for k, f in enumerate(grid_carriers(n, sl))]
    L = Launch(f"narrow_grid_n{n}_sl{sl}", cfg, rows, seq=2 ** 32 + n)
    for c, f in enumerate(grid_carriers(n, sl)):
        for r in range(3):
            assert L.ncounts(r)[c] == 1, (n, sl, c, r)
            m = L.nrecs(r, c)[0]
            g = _pad(m)[3]
            assert _pad(m)[:3] == (0, 0, 0) and int(m["flags"]) == NARROW and _data(m, n) == data and not m["data"][n // 8:].any()
            assert min((g - f * GRID) % GRID, (f * GRID - g) % GRID) <= 1.0, (n, sl, c, g, f * GRID)   # the grid point beside the carrier
            assert abs(int(m["tau"]) - (200 + 17 * c + 64 + sl - 1)) <= sl // 2
    return L


def grid_points():
    """g of every channel of every grid launch."""
    return [_pad(grid_launch(n, sl).nrecs(0, c)[0])[3] for n, sl in NGRID for c in (0, 1)]


CHOICE = (((1606, 79), 0),                                   # scores g = 0 and g = 1 alike: 1606 x 16384 = 1606 x 16305 + 79 x 1606
          ((5000, 0), 0), ((0, 5000), 16), ((-5000, 0), 32), ((0, -5000), 48),
          ((-1, 0), 32),                                     # sh = 0, ca = -1
          ((2 ** 30 + 12345, -(2 ** 29 + 777)), 59))         # bit length 31: sh = 16, ca = 16384, cb = -8193 (floor)


@functools.lru_cache(maxsize=None)
def choice_launch():
    """The grid choice through hand-written run records: per entry of CHOICE a channel whose burst lies at the angle of
    the written correlation sum, so that it decodes at the grid point the definition gives."""
    sl, n, bs = 8, 40, 2048
    cfg = DC.config(sl, n, bs)
    data = DC.packet(n, seed=31)
    rows = []
    for c, ((cre, cim), g) in enumerate(CHOICE):
        f = np.arctan2(cim, cre) / (2 * np.pi)
        rows.append(DC.put(_quiet(420 + c, bs), 300, DC.fsk_burst(data, sl, carrier=f)))
    runs, n_runs = DC.runs_of(np.stack(rows), DC.THR)
    for c, ((cre, cim), g) in enumerate(CHOICE):
        assert n_runs[c] == 1
        runs[c, 0]["corr_re"], runs[c, 0]["corr_im"] = cre, cim
    L = Launch("narrow_grid_choice", cfg, rows, runs=runs, n_runs=n_runs)
    C = table(sl)[1]
    assert 1606 * int(C[0, 0]) + 79 * int(C[0, 1]) == 1606 * int(C[1, 0]) + 79 * int(C[1, 1])
    assert grid_choice(*CHOICE[5][0])[:3] == (0, -1, 0) and grid_choice(*CHOICE[6][0])[:3] == (16, 16384, -8193)
    for c, ((cre, cim), g) in enumerate(CHOICE):
        assert grid_choice(cre, cim)[3] == g, (c, grid_choice(cre, cim))
        assert L.ncounts(0)[c] == 1 and _pad(L.nrecs(0, c)[0]) == (0, 0, 0, g) and _data(L.nrecs(0, c)[0], n) == data, (c, L.ncounts(0))
    return L


@functools.lru_cache(maxsize=None)
def edge_launch():
    """The region's ends, SL 4, inside a longer stretch of carrier whose run record is cut by hand to windows 3 .. 8: the
    filter must take zeros where bytes of full amplitude lie.  Channel 0: the packet's first symbol begins at t0 + 1 - the
    first output p' has - and its tau is t0 + SL; channel 1: the packet's last output is t1 - 1."""
    sl, n, bs = 4, 80, 2048
    cfg = DC.config(sl, n, bs)
    data = DC.packet(n, seed=32)
    t0, t1 = 128 * 3, 128 * 9
    rows = [DC.put(_quiet(430, bs), t0 - 199, DC.fsk_burst(data, sl, lead=200, trail=600)),
            DC.put(_quiet(431, bs), t1 - n * sl - 600, DC.fsk_burst(data, sl, lead=600, trail=600))]
    runs, n_runs = DC.runs_of(np.stack(rows), DC.THR)
    assert list(n_runs) == [1, 1]
    for c in (0, 1):
        assert int(runs[c, 0]["first"]) < 3 and int(runs[c, 0]["first"]) + int(runs[c, 0]["windows"]) > 9
        runs[c, 0]["first"], runs[c, 0]["windows"] = 3, 6
    L = Launch("narrow_zero_extension", cfg, rows, runs=runs, n_runs=n_runs)
    return L, (t0, t1)


def edge_taus(L):
    return [[int(r["tau"]) for r in L.nrecs(0, c)] for c in (0, 1)]


def y_with_neighbours(L, c):
    """(y of the model, y had the filter read the bytes that lie outside the region) at the region's first and last
    output of channel c's run."""
    rec, cfg = L.runs[c, 0], L.cfg
    sl = int(cfg.symbol_length)
    _, t0, t1, zi, zq = region_of(L.cur[c], None, rec, cfg, False)
    g = grid_choice(rec["corr_re"], rec["corr_im"])[3]
    hg = table(sl)[0][g]
    _, (yr, yi) = filter_region(zi, zq, hg)
    m = sl + 2
    a = 2 * L.cur[c].astype(np.int64) - 255
    _, (wr, wi) = filter_region(a[0::2][t0 - m: t1 + m], a[1::2][t0 - m: t1 + m], hg)
    return [(int(yr[j]), int(yi[j])) for j in (0, -1)], [(int(wr[m + j]), int(wi[m + j])) for j in (0, t1 - t0 - 1)]


@functools.lru_cache(maxsize=None)
def seam_launches():
    """A packet that straddles the chunk boundary (its last output at boundary + 200), reached by chunk 1's look-back:
    flags = 5; chunk 0 alone reports nothing."""
    sl, n, bs = 14, 80, 2048
    cfg = DC.config(sl, n, bs)
    data = DC.packet(n, seed=33)
    both = DC.put(_quiet(440, 2 * bs), bs + 200 - (n * sl - 1) - 56, DC.fsk_burst(data, sl, carrier=-0.21, lead=56, trail=300))
    b0, b1 = both[: 2 * bs], both[2 * bs:]
    first = Launch("narrow_seam_chunk0", cfg, [b0], seq=0)
    back = Launch("narrow_seam_chunk1", cfg, [b1], prev=[b0], clock=bs, seq=1)
    assert all(first.ncounts(r) == [0] for r in range(3)) and all(back.ncounts(r) == [1] for r in range(3))
    m = back.nrecs(0, 0)[0]
    assert int(m["flags"]) == 5 and _data(m, n) == data and int(m["tau"]) < 0 <= int(m["tau"]) + sl * (n - 1)
    assert int(m["time"]) == bs + int(m["tau"])
    return first, back, (b0, b1), cfg, data


def worst_region(sl, g):
    """z of bytes 0 and 255 only whose signs at the centre output follow the taps of H[g]: acc_re there is 255 times
    sum_k |H.re| + |H.im|, the largest any bytes can give; the rest alternates."""
    hg = table(sl)[0][g]
    m = sl + 2
    size = 4 * m + 1
    t = size // 2
    zi = np.where(np.arange(size) % 2 == 0, 255, -255).astype(np.int64)
    zq = zi.copy()
    for k in range(-m, m + 1):                               # acc_re = sum hr zi - hi zq
        zi[t - k] = 255 if hg[k + m, 0] >= 0 else -255
        zq[t - k] = -255 if hg[k + m, 1] >= 0 else 255
    return zi, zq, t


@functools.lru_cache(maxsize=None)
def saturated_launch():
    """Bytes 0 and 255 only: a hard-limited FSK burst (amplitude 10^9 before the clip), decodable, beside a correlation
    sum of bit length 30 - the largest a run of 32 windows gives.  y comes within a factor 1.3 of its bound."""
    sl, n, bs = 14, 80, 2048
    cfg = DC.config(sl, n, bs)
    data = DC.packet(n, seed=34)
    burst = np.where(DC.fsk_burst(data, sl, carrier=0.11, lead=80, trail=80, amp=1e9) >= 128, 255, 0).astype(np.uint8)
    row = DC.put(_quiet(450, bs), 3 * W, burst)
    runs, n_runs = DC.runs_of(row[None, :], DC.THR)
    assert n_runs[0] == 1
    big = 2 ** 30 - 1000
    ph = 2 * np.pi * 0.11
    runs[0, 0]["corr_re"], runs[0, 0]["corr_im"] = int(big * np.cos(ph)), int(big * np.sin(ph))
    L = Launch("narrow_saturated", cfg, [row], runs=runs, n_runs=n_runs)
    assert all(L.ncounts(r) == [1] for r in range(3)) and _data(L.nrecs(0, 0)[0], n) == data
    _, t0, t1, zi, zq = region_of(L.cur[0], None, L.runs[0, 0], cfg, False)
    sh, ca, cb, g = grid_choice(runs[0, 0]["corr_re"], runs[0, 0]["corr_im"])
    assert sh == 15 and g == 7 == _pad(L.nrecs(0, 0)[0])[3]
    _, (yr, yi) = filter_region(zi, zq, table(sl)[0][g])
    assert max(np.abs(yr).max(), np.abs(yi).max()) > Y_MAX / 1.3
    return L


@functools.lru_cache(maxsize=None)
def longest_launches():
    """SL 25 and SL 51 (107 taps) in a run of 32 windows with 16 of look-back over a packet that straddles t = 0: 6144
    outputs, all of the kernel's LDS, 24 outputs per lane."""
    out = []
    for sl, n, f in ((25, 80, 0.11), (51, 40, -0.30)):
        bs = 4096
        cfg = DC.config(sl, n, bs)
        assert DC.shape(cfg)[3] == 16 * W
        data = DC.packet(n, seed=35 + sl)
        both = DC.put(_quiet(460 + sl, 2 * bs), bs - 1000 - 100, DC.fsk_burst(data, sl, carrier=f, lead=100, trail=bs + 1000 - n * sl))
        L = Launch(f"narrow_longest_sl{sl}", cfg, [both[2 * bs:]], prev=[both[: 2 * bs]], clock=7 * bs, seq=7)
        assert list(L.n_runs) == [1] and int(L.runs[0, 0]["windows"]) == 32 and int(L.runs[0, 0]["flags"]) == 3
        assert all(L.ncounts(r) == [1] for r in range(3))
        m = L.nrecs(0, 0)[0]
        assert int(m["flags"]) == 5 and _data(m, n) == data and abs(int(m["tau"]) - (-1000 + sl - 1)) <= sl // 2
        out.append(L)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def repair_launch():
    """One wrong symbol behind the filter, SL 8: nothing at R = 0, pad = (1, k, 0, g) at R = 1 and 2.  The filter spreads
    a symbol over its neighbours, so the strength at which symbol k alone comes out wrong is searched on the model."""
    sl, n, bs = 8, 80, 2048
    cfg = DC.config(sl, n, bs)
    data = RP.find_packet(n, lambda b: RP.lonely(b, 37), 1400)
    for scale in (-0.4, -0.6, -0.8, -1.0):
        row = DC.put(_quiet(470, bs), 300, RP.damaged(data, sl, {37: scale}))
        L = Launch("narrow_one_flip", cfg, [row])
        if L.ncounts(0) == [0] and L.ncounts(1) == [1] == L.ncounts(2):
            m = L.nrecs(1, 0)[0]
            g = grid_choice(L.runs[0, 0]["corr_re"], L.runs[0, 0]["corr_im"])[3]
            assert _pad(m) == (1, 37, 0, g) and int(m["flags"]) == NARROW | RP.REPAIRED and _data(m, n) == data
            assert L.nrecs(2, 0)[0].tobytes() == m.tobytes()
            return L
    raise AssertionError("narrow_one_flip: no strength leaves symbol 37 alone wrong")


def crafted_launches():
    """Every crafted launch of the narrow-band cases, each with its conditions asserted."""
    first, back, *_ = seam_launches()
    return tuple(grid_launch(n, sl) for n, sl in NGRID) + (choice_launch(), edge_launch()[0], first, back, saturated_launch(),
                                                           repair_launch()) + longest_launches()


# ------------------------------------------------------------------------------------------ noisy bursts (the gain)
def gain_run(k, noise, seed, flips=(0, 2), cfo=1500.0):
    """({(narrow, R): [records]}, planted payloads) of the stream models over burst_repair_cases.gain_blocks."""
    datas, blocks = RP.gain_blocks(k, noise, seed, cfo)
    cfg = DC.config(RP.GAIN_SL, 80, RP.GAIN_BS)
    thr = RP.gain_threshold(noise)
    bursts = [BC.model_bursts(b, thr, j) for j, b in enumerate(blocks)]
    out = {}
    for narrow in (False, True):
        for r in flips:
            out[narrow, r] = [rec for _, m in decode_stream(blocks, thr, cfg, r, narrow, bursts=bursts) for rec in m.records]
    return out, datas


def tally(records, datas):
    """(bursts decoded, records with a payload that was not planted)."""
    planted = set(datas)
    return len({bytes(x["data"]) for x in records} & planted), sum(bytes(x["data"]) not in planted for x in records)


# ------------------------------------------------------------------------------------------ the device capture
# burst_decode_cases' symbol_length 8 plan (device_receiver(bs, 8, offsets_hz=S8_OFFSETS_HZ), "s16", decim 4) with
# undamaged bursts in noise: (channel, first output, Hz off the channel's centre); the packet of burst j is
# cap_packets()[j].  The first chunk is noise alone (it measures the floor).
CAP_BS = (1024, 2048)
CAP_OUTPUTS = 10 * 1024
CAP_AMPLITUDE, CAP_NOISE = 0.12, 0.09
CAP_FACTOR = 2                                               # thresholds at twice the floor of the quiet first chunk
CAP_BURSTS = ((1, 2048 + 300, 20000),                         # crosses 3072
              (2, 3072 + 500, -30000),                        # crosses 4096
              (0, 4096 + 200, 25000),                         # crosses 5120
              (1, 5120 + 400, -12000),                        # crosses 6144
              (2, 6144 + 30, 38000),                          # inside 6144 .. 7167
              (0, 7168 + 40, -25000),                         # crosses 8192 in chunks of 1024
              (1, 8192 + 1024 + 20, 5000))                    # inside the last chunk of either size


@functools.lru_cache(maxsize=None)
def cap_packets():
    return [DC.packet(80, ident=j % 8, seed=500 + j) for j in range(len(CAP_BURSTS))]


@functools.lru_cache(maxsize=None)
def cap_capture(sl=8, decim=DC.DEV_DECIM, amplitude=CAP_AMPLITUDE, noise=CAP_NOISE):
    """int16 I,Q of CAP_OUTPUTS x decim samples, made the way burst_decode_cases.s8_capture makes its own."""
    fw = decim * 19200 * sl
    n = CAP_OUTPUTS * decim
    rng = np.random.default_rng(919)
    x = noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for (c, start, hz), data in zip(CAP_BURSTS, cap_packets()):
        bits = np.concatenate([np.tile(np.array([1, 0], np.uint8), 16), np.unpackbits(np.frombuffer(data, np.uint8)), np.zeros(8, np.uint8)])
        freq = float(DC.S8_OFFSETS_HZ[c] + hz) + np.repeat(np.where(bits == 1, 4800.0, -4800.0), sl * decim)
        lo = start * decim
        x[lo: lo + freq.size] += amplitude * np.exp(2j * np.pi * np.cumsum(freq) / fw)
    out = np.empty(2 * n, np.int16)
    out[0::2] = np.clip(np.rint(x.real * 32768.0), -32768, 32767)
    out[1::2] = np.clip(np.rint(x.imag * 32768.0), -32768, 32767)
    return out
