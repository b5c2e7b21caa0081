"""Helpers shared by tests/test_burst_quality_cpu.py, tests/test_burst_quality.py, tests/test_wideband_quality.py and
tests/test_quality_sanitizers.py (no tests in here): the NumPy / Python integer model of k_chan_burst_quality, written
from the definition (include/rtldavis_hip.h, BURST QUALITY) - the windows in Python integers, z over both chunks as one
int64 array with zeros nowhere but outside it, the filter as burst_narrow_cases' convolution over that whole array where
the kernel pads a region in LDS, the sums as NumPy sums -; the slot model of the hook rd_debug_burst_quality; and the
crafted launches, whose bytes come from burst_decode_cases' builders.  Every case asserts the edge it is built for on the
model of its own bytes when it is built.  Nothing here touches a device."""
import functools

import numpy as np

import burst_cases as BC
import burst_decode_cases as DC
import burst_narrow_cases as NB
from rtldavis_amd.wideband import BURST_MSG_DTYPE, QUALITY_DTYPE

W, FILL = DC.W, DC.FILL
MAX_GAP = 1024                                               # RD_BQ_MAX_GAP
BX_MAX = 64                                                  # RD_BX_MAX: the expect part of the quality slot
INBAND, UNMEASURABLE = 1, 128                                # rd_burst_quality.flags
DEBUG_CHUNK = 0x51A7                                         # RD_BQ_DEBUG_CHUNK
Z2_MAX = 2 * 255 * 255                                       # |z|^2 at most: 130050
Y2_MAX = 2 * NB.Y_MAX * NB.Y_MAX                             # |y|^2 at most


# ------------------------------------------------------------------------------------------ the definition
def windows(sl, n, bs, have_prev, tau, gap):
    """None for a record that is not measurable, else (p0, p1, s1, n0, n1): packet [p0, p1), sync [p0, s1), noise
    [n0, n1) - n0 = n1 = p0 when nothing of the noise window is left."""
    lo_lim = -bs if have_prev else 0
    p0 = tau - sl + 1
    p1 = p0 + n * sl
    if p0 < lo_lim or p1 > bs:
        return None
    n1 = p0 - gap
    n0 = max(n1 - 16 * sl, lo_lim)
    if n1 <= n0:
        n0 = n1 = p0
    return p0, p1, p0 + 16 * sl, n0, n1


def naive_windows(sl, n, bs, have_prev, tau, gap):
    """The same by enumeration: the outputs of each window, one by one."""
    lo_lim = -bs if have_prev else 0
    p0 = tau - sl + 1
    pkt = [p0 + i for i in range(n * sl)]
    if min(pkt) < lo_lim or max(pkt) >= bs:
        return None
    noise = [t for t in range(p0 - gap - 16 * sl, p0 - gap) if t >= lo_lim]
    return pkt, pkt[: 16 * sl], noise


def z_of(cur, prev):
    """(zi, zq, org): z over lo_lim <= t < B as int64 arrays, output t at index org + t."""
    a = 2 * (cur if prev is None else np.concatenate([prev, cur])).astype(np.int64) - 255
    return a[0::2], a[1::2], 0 if prev is None else cur.size // 2


def measure(cur, prev, cfg, channel, tau, f_re, f_im, gap, n_ch, chunk=DEBUG_CHUNK):
    """The quality record of one message record, as a tuple in the order of QUALITY_DTYPE."""
    sl, n, bs = int(cfg.symbol_length), int(cfg.packet_symbols), int(cfg.block_size)
    channel, tau, f_re, f_im = int(channel), int(tau), int(f_re), int(f_im)
    win = windows(sl, n, bs, prev is not None, tau, gap) if 0 <= channel < n_ch else None
    if win is None:
        return (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, UNMEASURABLE, chunk)
    p0, p1, s1, n0, n1 = win
    zi, zq, org = z_of(cur[channel], None if prev is None else prev[channel])
    e = zi * zi + zq * zq
    cut = lambda x, a, b: x[org + a: org + b]
    pkt, sig, noise = int(cut(e, p0, p1).sum()), int(cut(e, p0, s1).sum()), int(cut(e, n0, n1).sum())
    assert max(pkt, sig, noise) < 2 ** 28
    peak = int(max(np.abs(cut(zi, p0, p1)).max(), np.abs(cut(zq, p0, p1)).max()))
    raw = cur[channel] if prev is None else np.concatenate([prev[channel], cur[channel]])
    b = raw[2 * (org + p0): 2 * (org + p1)]
    clipped = int(((b == 0) | (b == 255)).sum())
    if sl < NB.MIN_SL or (f_re == 0 and f_im == 0):
        return (pkt, sig, noise, 0, 0, 0, n1 - n0, clipped, peak, 0, 0, chunk)
    g = NB.grid_choice(f_re, f_im, sl)[3]
    _, (yr, yi) = NB.filter_region(zi, zq, NB.table(sl)[0][g])          # z = 0 outside lo_lim <= t < B: the array's ends
    e2 = yr * yr + yi * yi
    nb = tuple(int(cut(e2, a, b).sum()) for a, b in ((p0, p1), (p0, s1), (n0, n1)))
    assert max(nb) < 2 ** 36
    return (pkt, sig, noise) + nb + (n1 - n0, clipped, peak, g, INBAND, chunk)


def quality_rows(cur, prev, cfg, records, gap, chunk):
    """QUALITY_DTYPE rows parallel to message rows of one chunk (cur / prev: [n_ch, 2 B])."""
    cur = np.atleast_2d(cur)
    prev = None if prev is None else np.atleast_2d(prev)
    rows = [measure(cur, prev, cfg, r["channel"], r["tau"], r["f_re"], r["f_im"], gap, cur.shape[0], chunk & 0xFFFFFFFF) for r in records]
    return np.asarray(rows, QUALITY_DTYPE).reshape(-1)


def packet_sum(cur, prev, p0, length):
    """(f_re, f_im) as the decoders write them: the sum of z[t] conj(z[t-1]) over the packet's outputs."""
    zi, zq, org = z_of(cur, prev)
    t = np.arange(org + p0, org + p0 + length)
    t = t[t >= 1]
    return (int((zi[t] * zi[t - 1] + zq[t] * zq[t - 1]).sum()), int((zq[t] * zi[t - 1] - zi[t] * zq[t - 1]).sum()))


def message(channel, tau, f_re, f_im, flags=0):
    """A message record as far as the kernel reads it; the other fields hold what a decoder might have written."""
    return (channel, 0, tau, flags, tau % 2 ** 64, 1, f_re, f_im, [0] * 10, 0, 0, [0, 0, 0, 0])


class QLaunch:
    """One launch of the hook: configuration, bytes (rows: one uint8 [2 B] per channel; prev alike or None), the gap, the
    message records per channel ([(channel, tau, f_re, f_im)], or ready rows of BURST_MSG_DTYPE) and what the model
    expects back: the whole quality slot, FILL wherever the kernel must not write."""

    def __init__(self, name, cfg, rows, prev, gap, records):
        self.name, self.cfg, self.gap = name, cfg, gap
        self.cur = np.ascontiguousarray(np.stack(rows), np.uint8)
        self.prev = None if prev is None else np.ascontiguousarray(np.stack(prev), np.uint8)
        bs = int(cfg.block_size)
        # (any block_size rd_debug_burst_quality admits and any number of channels: the crafted cases use LOOK and at most 4)
        assert self.cur.shape[1] == 2 * bs and (self.prev is None or self.prev.shape == self.cur.shape) and bs % W == 0 and bs >= DC.shape(cfg)[3]
        self.n_ch = self.cur.shape[0]
        assert len(records) == self.n_ch
        self.cap = BC.cap_of(bs // W)
        self.msgs = np.frombuffer(bytes([FILL]) * (self.n_ch * self.cap * BURST_MSG_DTYPE.itemsize), BURST_MSG_DTYPE).reshape(self.n_ch, self.cap).copy()
        self.n_msgs = np.zeros(self.n_ch, np.uint32)
        for c, recs in enumerate(records):
            assert len(recs) <= self.cap
            for i, r in enumerate(recs):
                self.msgs[c, i] = r if isinstance(r, np.void) else message(*r)
            self.n_msgs[c] = len(recs)
        self.want = np.frombuffer(bytes([FILL]) * ((self.n_ch * self.cap + BX_MAX) * QUALITY_DTYPE.itemsize), QUALITY_DTYPE).copy()
        for c in range(self.n_ch):
            for i in range(int(self.n_msgs[c])):
                m = self.msgs[c, i]
                self.want[c * self.cap + i] = measure(self.cur, self.prev, cfg, m["channel"], m["tau"], m["f_re"], m["f_im"], gap, self.n_ch)

    def row(self, c, i=0):
        assert i < int(self.n_msgs[c])
        return self.want[c * self.cap + i]


# ------------------------------------------------------------------------------------------ crafted bytes
def smallest_block(sl, n):
    """The smallest multiple of 128 that holds LOOK."""
    return W * (-(-(n * sl + 1) // W))


def planted(name, sl, n, p0s, have_prev=True, gap=0, seed=0, extra=None, amp=DC.AMP):
    """One burst per channel whose packet's first output is p0s[c] (relative to the chunk; negative: in the chunk before),
    with carrier lead-in in front as far as the two chunks hold it, in quiet bytes; one record per channel at the packet's
    own place with the f a decoder would write, plus extra[c] records."""
    bs = smallest_block(sl, n)
    cfg = DC.config(sl, n, bs)
    cur, prev, records = [], [], []
    for c, p0 in enumerate(p0s):
        both = BC.quiet_bytes(np.random.default_rng(7000 + 10 * seed + c), 2 * bs)
        org = bs if have_prev else 0
        lead = min(64, org + p0)
        trail = min(32, bs - (p0 + n * sl))
        carrier = (-0.31, 0.11, 0.27, -0.06)[c]
        DC.put(both, org + p0 - lead, DC.fsk_burst(DC.packet(n, seed=seed + c), sl, carrier=carrier, lead=lead, trail=trail, amp=amp))
        row_prev, row_cur = (both[: 2 * bs], both[2 * bs:]) if have_prev else (None, both[: 2 * bs])
        cur.append(row_cur)
        prev.append(row_prev)
        f = packet_sum(row_cur, row_prev, p0, n * sl)
        records.append([(c, p0 + sl - 1) + f] + ([] if extra is None else [(c, q0 + sl - 1) + f for q0 in extra[c]]))
    return QLaunch(name, cfg, cur, prev if have_prev else None, gap, records)


@functools.lru_cache(maxsize=None)
def default_launch():
    """SL 14 / N 80 in 1152 outputs: a packet near the chunk's start (its noise window crosses into the chunk before), one
    that begins in the chunk before, and one whose last output is block_size - 1."""
    L = planted("quality_default", 14, 80, (10, -500, 32), seed=1)
    assert int(L.cfg.block_size) == 1152 and 32 + 80 * 14 == 1152
    for c in range(3):
        r = L.row(c)
        assert int(r["flags"]) == INBAND and int(r["n_noise"]) == 224 and 0 < int(r["noise"]) < int(r["sig"]) < int(r["pkt"])
        assert int(r["noise_nb"]) > 0 and int(r["clipped"]) == 0 and 2 * DC.AMP - 2 <= int(r["peak"]) <= 2 * DC.AMP + 2
    return L


@functools.lru_cache(maxsize=None)
def sl4_launch():
    """SL 4 / N 40: the smallest filter (13 taps), 256 outputs."""
    L = planted("quality_sl4", 4, 40, (70, -100), seed=2)
    assert int(L.cfg.block_size) == 256 and all(int(L.row(c)["flags"]) == INBAND and int(L.row(c)["n_noise"]) == 64 for c in (0, 1))
    return L


@functools.lru_cache(maxsize=None)
def sl3_launch():
    """SL 3: no filter - bit 0 clear, the in-band fields 0, the raw sums as ever."""
    L = planted("quality_sl3", 3, 40, (5, -60), seed=3)
    for c in (0, 1):
        r = L.row(c)
        assert int(r["flags"]) == 0 and int(r["g"]) == 0 and not (int(r["pkt_nb"]) or int(r["sig_nb"]) or int(r["noise_nb"])) and int(r["pkt"]) > 0
    return L


@functools.lru_cache(maxsize=None)
def sl51_launch():
    """SL 51 / N 40: the largest T (107 taps), 2048 outputs."""
    L = planted("quality_sl51", 51, 40, (3, -1000), seed=4)
    assert int(L.cfg.block_size) == 2048 and all(int(L.row(c)["flags"]) == INBAND and int(L.row(c)["n_noise"]) == 816 for c in (0, 1))
    return L


@functools.lru_cache(maxsize=None)
def largest_launch():
    """The largest region: SL 51 / N 40 - N SL + 1 = 2041, the most a configuration with N a multiple of 8 reaches below
    2048 - with noise_gap = 1024: 1024 + 816 + 2040 = 3880 outputs, the noise window whole and deep in the chunk before."""
    L = planted("quality_largest", 51, 40, (-200, 8), gap=MAX_GAP, seed=5)
    assert windows(51, 40, 2048, True, -200 + 50, MAX_GAP) == (-200, 1840, 616, -2040, -1224)
    assert int(L.row(0)["n_noise"]) == 816 and int(L.row(1)["n_noise"]) == 816 and 8 + 2040 == 2048
    return L


@functools.lru_cache(maxsize=None)
def placement_launches():
    """SL 8 / N 40 in 384 outputs.  Without a chunk before: P0 = 0 (n_noise = 0) and P0 = 50 (the window cut at t = 0:
    n_noise = 50).  With one: the same records (noise wholly in the chunk before; whole) and P0 = -300, whose window is
    cut by lo_lim = -384 (n_noise = 84)."""
    alone = planted("quality_placement_alone", 8, 40, (0, 50), have_prev=False, seed=6)
    assert [int(alone.row(c)["n_noise"]) for c in (0, 1)] == [0, 50] and int(alone.row(0)["noise"]) == 0 == int(alone.row(0)["noise_nb"])
    assert int(alone.row(0)["flags"]) == INBAND and int(alone.row(1)["noise"]) > 0
    both = planted("quality_placement_prev", 8, 40, (0, 50, -300), seed=6)
    assert [int(both.row(c)["n_noise"]) for c in (0, 1, 2)] == [128, 128, 84]
    assert windows(8, 40, 384, True, 7, 0)[3:] == (-128, 0) and windows(8, 40, 384, True, -293, 0)[3:] == (-384, -300)
    return alone, both


@functools.lru_cache(maxsize=None)
def residue_launch():
    """P0 at every residue mod 8, above and below t = 0, through extra records on the same bytes: the vector loads begin at
    a multiple of 8 below the filter's first output whatever P0 is."""
    L = planted("quality_residues", 14, 80, (16, 18, 20, 22), seed=7, extra=((17, -41), (19, -43), (21, -46), (23, -48)))
    res_pos = sorted(int(L.msgs[c, i]["tau"] - 13) % 8 for c in range(4) for i in (0, 1))
    res_neg = sorted(int(L.msgs[c, 2]["tau"] - 13) % 8 for c in range(4))
    assert res_pos == list(range(8)) and len(set(res_neg)) == 4 and all(int(L.msgs[c, 2]["tau"]) - 13 < 0 for c in range(4))
    assert all(int(L.row(c, i)["flags"]) == INBAND for c in range(4) for i in range(3))
    return L


@functools.lru_cache(maxsize=None)
def saturated_launch():
    """burst_decode_cases.overflow_launch's saturated bytes (0 and 255 only) and its own decoded records: the largest raw
    sums, every byte of the packet clipped, peak 255."""
    O = DC.overflow_launch()
    assert int(O.cfg.block_size) == 2048
    cfg = DC.config(14, 80, 2048)
    # (2048 is not the smallest block for SL 14: the builder's bytes are what they are, and QLaunch's rule is waived here)
    L = QLaunch.__new__(QLaunch)
    L.name, L.cfg, L.gap, L.cur, L.prev, L.n_ch = "quality_saturated", cfg, 0, O.cur, None, O.n_ch
    L.cap = BC.cap_of(2048 // W)
    L.msgs, L.n_msgs = O.msgs.copy(), O.n_msgs.copy()
    L.want = np.frombuffer(bytes([FILL]) * ((L.n_ch * L.cap + BX_MAX) * QUALITY_DTYPE.itemsize), QUALITY_DTYPE).copy()
    for c in range(L.n_ch):
        m = L.msgs[c, 0]
        L.want[c * L.cap] = measure(L.cur, None, cfg, m["channel"], m["tau"], m["f_re"], m["f_im"], 0, L.n_ch)
        r = L.row(c)
        assert int(r["pkt"]) == Z2_MAX * 1120 and int(r["sig"]) == Z2_MAX * 224 and int(r["clipped"]) == 2 * 1120 and int(r["peak"]) == 255
        assert int(r["flags"]) == INBAND and int(r["pkt_nb"]) > 0
    return L


@functools.lru_cache(maxsize=None)
def flat_launch():
    """Constant bytes 127, 128 (the smallest sums: |z|^2 = 2), 255 and 0 (the largest), with a chunk before alike."""
    sl, n = 14, 80
    bs = smallest_block(sl, n)
    cfg = DC.config(sl, n, bs)
    rows = [np.full(2 * bs, v, np.uint8) for v in (127, 128, 255, 0)]
    recs = [[(c, 16 + sl - 1) + packet_sum(rows[c], rows[c], 16, n * sl)] for c in range(4)]
    L = QLaunch("quality_flat", cfg, rows, rows, 0, recs)
    for c, z2 in enumerate((2, 2, Z2_MAX, Z2_MAX)):
        r = L.row(c)
        assert (int(r["pkt"]), int(r["sig"]), int(r["noise"]), int(r["n_noise"])) == (z2 * 1120, z2 * 224, z2 * 224, 224)
        assert int(r["clipped"]) == (0 if c < 2 else 2240) and int(r["peak"]) == (1 if c < 2 else 255) and int(r["flags"]) == INBAND
        assert int(r["g"]) == 0 and int(L.msgs[c, 0]["f_im"]) == 0 and int(L.msgs[c, 0]["f_re"]) == z2 * 1120
    return L


TIE_F = (1606, 79)                                           # scores g = 0 and g = 1 alike (burst_narrow_cases.CHOICE)


@functools.lru_cache(maxsize=None)
def record_launch():
    """Record extremes on ordinary bytes.  Channel 0: f = (0, 0) (bit 0 clear), f at +-2^36, and f on a tie between g = 0
    and g = 1 (the smallest wins).  Channel 1: a record with tau out of range (beyond the chunk, and INT32_MIN), one with a
    channel that does not exist (7, -1) - flags bit 7 and zeros - between good records, which are untouched by them."""
    P = planted("quality_records_bytes", 14, 80, (16, 16), seed=8)
    good = [tuple(int(P.msgs[c, 0][k]) for k in ("channel", "tau", "f_re", "f_im")) for c in (0, 1)]
    t = good[0][1]
    big = 2 ** 36
    ch0 = [(0, t, 0, 0), (0, t, big, -big), (0, t, -big, 5), (0, t) + TIE_F]
    ch1 = [good[1], (1, 40000, 5, 5), (7, good[1][1], 5, 5), (1, -2 ** 31, 5, 5), (-1, good[1][1], 5, 5)]
    assert P.cap == 5
    L = QLaunch("quality_records", P.cfg, list(P.cur), list(P.prev), 0, [ch0, ch1])
    C = NB.table(14)[1]
    assert TIE_F[0] * int(C[0, 0]) + TIE_F[1] * int(C[0, 1]) == TIE_F[0] * int(C[1, 0]) + TIE_F[1] * int(C[1, 1])
    assert NB.grid_choice(big, -big, 14)[:3] == (22, 2 ** 14, -2 ** 14) and NB.grid_choice(-big, 5, 14)[:3] == (22, -2 ** 14, 0)
    assert int(L.row(0, 0)["flags"]) == 0 and int(L.row(0, 0)["pkt"]) > 0 and int(L.row(0, 0)["pkt_nb"]) == 0
    assert [int(L.row(0, i)["g"]) for i in (1, 2, 3)] == [56, 32, 0] and all(int(L.row(0, i)["flags"]) == INBAND for i in (1, 2, 3))
    assert L.row(1, 0).tobytes() == P.row(1).tobytes()
    for i in (1, 2, 3, 4):
        assert L.row(1, i).tobytes() == np.asarray([(0,) * 10 + (UNMEASURABLE, DEBUG_CHUNK)], QUALITY_DTYPE).tobytes()
    return L


@functools.lru_cache(maxsize=None)
def occupancy_launch():
    """A channel with cap = 5 records between channels with none: every place of channels 0 and 2, and the expect part,
    keeps its FILL."""
    P = planted("quality_occupancy_bytes", 14, 80, (16, 20, 24), seed=9)
    f = tuple(int(P.msgs[1, 0][k]) for k in ("f_re", "f_im"))
    L = QLaunch("quality_occupancy", P.cfg, list(P.cur), list(P.prev), 7, [[], [(1, q0 + 13) + f for q0 in (20, -3, 1, 31, -900)], []])
    fill = bytes([FILL]) * QUALITY_DTYPE.itemsize
    assert L.cap == 5 and list(L.n_msgs) == [0, 5, 0]
    assert all(L.want[i].tobytes() == fill for i in list(range(5)) + list(range(10, 15 + BX_MAX)))
    assert all(int(L.row(1, i)["flags"]) == INBAND for i in range(5))
    return L


def crafted_launches():
    """Every crafted launch of the quality cases, each with its conditions asserted."""
    return (default_launch(), sl4_launch(), sl3_launch(), sl51_launch(), largest_launch()) + placement_launches() + (
        residue_launch(), saturated_launch(), flat_launch(), record_launch(), occupancy_launch())
