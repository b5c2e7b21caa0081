"""Helpers shared by tests/test_burst_clips_cpu.py, tests/test_burst_clips.py and tests/test_wideband_clips.py (no tests in
here): the NumPy / Python integer model of k_chan_burst_clips, written from the definition (include/rtldavis_hip.h, BURST
CLIPS) - the request list in its order, the clamp in Python integers, the allocation, owed; the image of the whole slot
that the hook rd_debug_burst_clips hands back, FILL wherever the kernel must leave it alone; a receiver in NumPy for
the streamed tests; and the crafted launches.  A clip is a copy, so the crafted bytes are random: any wrong index shows.
Every case asserts the edge it is built for on its own model when it is built.  Nothing here touches a device."""
import functools

import numpy as np

import burst_cases as BC
import burst_decode_cases as DC
from rtldavis_amd.wideband import BURST_DTYPE, BURST_MSG_DTYPE, CLIP_DTYPE, SEARCH_HDR_DTYPE

W, FILL = DC.W, DC.FILL
RUNS, MESSAGES = 1, 2                                        # RD_BC_RUNS, RD_BC_MESSAGES
MAX_ROLL, MAX_QUOTA, MAX_POOL, PER = 1024, 65536, 1 << 26, 16
CUT_START, CUT_END, FROM_PREV = 1, 2, 4
TAIL, RUN, DECODE, EXPECTED, SEARCHED = range(5)
BX_MAX, BS_MAX, BS_PER = 64, 8, 4
HDR_DTYPE = np.dtype([("n_clips", np.uint32), ("dropped", np.uint32), ("owed", np.uint32), ("used", np.uint32),
                      ("chunk", np.uint32), ("pad", np.uint32)])
X_HDR_DTYPE = np.dtype([("n_msgs", np.uint32), ("candidates", np.uint32), ("chunk", np.uint32), ("pad", np.uint32)])
assert CLIP_DTYPE.itemsize == 48 and HDR_DTYPE.itemsize == 24


# ------------------------------------------------------------------------------------------ the definition
def clamp(bs, have_prev, a, e):
    """None for a request that gives no clip, else (t0, n, flags)."""
    lo_lim = -bs if have_prev else 0
    if e <= a:
        return None
    t0 = max(a, lo_lim) // 8 * 8                             # (Python's // rounds towards minus infinity)
    t1 = -(-min(e, bs) // 8) * 8
    if t1 - t0 <= 0:
        return None
    return t0, t1 - t0, (CUT_START if a < lo_lim else 0) | (CUT_END if e > bs else 0) | (FROM_PREV if t0 < 0 else 0)


def naive_clamp(bs, have_prev, a, e):
    """The same by enumeration: the outputs of the request that the two chunks hold, one by one, then the 8-output groups
    they touch.  (For small |a|, |e| only.)"""
    lo_lim = -bs if have_prev else 0
    inside = [t for t in range(a, e) if lo_lim <= t < bs]
    if not inside:
        return None
    groups = sorted({t // 8 for t in inside})
    assert groups == list(range(groups[0], groups[-1] + 1))
    t0, n = 8 * groups[0], 8 * len(groups)
    return t0, n, (CUT_START if a < lo_lim else 0) | (CUT_END if e - 1 >= bs else 0) | (FROM_PREV if t0 < 0 else 0)


def row_request(row, c, source, sl, n_sym, bs, have_prev, pre, post):
    """The request of a message row, or None: its channel field is c and its packet lies inside the two chunks."""
    lo_lim = -bs if have_prev else 0
    p0 = int(row["tau"]) - sl + 1
    if int(row["channel"]) != c or p0 < lo_lim or p0 + n_sym * sl > bs:
        return None
    return source, p0 - pre, p0 + n_sym * sl + post, int(row["time"])


def requests(c, sl, n_sym, bs, have_prev, sources, pre, post, owed_prev, runs, decode_rows, expect_rows, search_rows):
    """Channel c's requests in the definition's order: [(source, a, e, ref)].  runs: the record places k_chan_bursts is said to
    have written; decode_rows: the rows of c's decode slot; expect_rows: the rows of the expect slot (any channel) by table
    index; search_rows: the rows of c's search places by (centre, place).  owed_prev: None or the previous header's owed."""
    out = []
    if owed_prev is not None and 0 < int(owed_prev) <= MAX_ROLL:
        out.append((TAIL, 0, int(owed_prev), 0))
    n_win = bs // W
    if sources & RUNS:
        for r in runs:
            first, windows = int(r["first"]), int(r["windows"])
            if windows == 0 or first >= n_win or first + windows > n_win:
                continue
            out.append((RUN, W * first - pre, W * (first + windows) + post, first))
    if sources & MESSAGES:
        for source, rows in ((DECODE, decode_rows), (EXPECTED, expect_rows), (SEARCHED, search_rows)):
            for row in rows:
                q = row_request(row, c, source, sl, n_sym, bs, have_prev, pre, post)
                if q is not None:
                    out.append(q)
    return out


def allocate(c, reqs, bs, have_prev, clock, seq, quota):
    """(records CLIP_DTYPE, header tuple in the order of HDR_DTYPE) of one channel."""
    recs, used, dropped, owed = [], 0, 0, 0
    for source, a, e, ref in reqs:
        w = clamp(bs, have_prev, a, e)
        if w is None:
            continue
        t0, n, flags = w
        if len(recs) >= PER or used + n > quota:
            dropped += 1
            continue
        recs.append((c, source, flags, t0, n, used, (int(clock) + t0) % 2 ** 64, ref % 2 ** 64, seq & 0xFFFFFFFF, 0))
        used += n
        if flags & CUT_END:
            owed = max(owed, e - bs)
    assert 0 <= owed <= MAX_ROLL
    return np.asarray(recs, CLIP_DTYPE).reshape(-1), (len(recs), dropped, owed, used, seq & 0xFFFFFFFF, 0)


def clip_bytes(cur_row, prev_row, t0, n):
    """Outputs t0 .. t0 + n - 1 of one channel as they lie: uint8 [2 n]."""
    bs = cur_row.size // 2
    both = cur_row if prev_row is None else np.concatenate([prev_row, cur_row])
    org = 0 if prev_row is None else bs
    assert org + t0 >= 0 and t0 + n <= bs
    return both[2 * (org + t0): 2 * (org + t0 + n)]


def header_offset(n_ch):
    return n_ch * PER * CLIP_DTYPE.itemsize


def pool_offset(n_ch):
    return (header_offset(n_ch) + n_ch * HDR_DTYPE.itemsize + 15) // 16 * 16


def slot_bytes(n_ch, quota):
    return pool_offset(n_ch) + n_ch * 2 * quota


def split_slot(slot, n_ch, quota):
    """(records [n_ch, PER], headers [n_ch], pool [n_ch, 2 quota]) as views of a slot image."""
    slot = np.asarray(slot, np.uint8)
    assert slot.size == slot_bytes(n_ch, quota)
    recs = slot[: header_offset(n_ch)].view(CLIP_DTYPE).reshape(n_ch, PER)
    hdr = slot[header_offset(n_ch): header_offset(n_ch) + n_ch * HDR_DTYPE.itemsize].view(HDR_DTYPE)
    pool = slot[pool_offset(n_ch):].reshape(n_ch, 2 * quota)
    return recs, hdr, pool


def chunk_model(cur, prev, sl, n_sym, clock, seq, sources, pre, post, quota, owed_prev, runs, decode_rows, expect_rows, search_rows):
    """One chunk, every channel: [(records, header, bytes)].  cur / prev: uint8 [n_ch, 2 B]; runs, decode_rows, search_rows:
    one list per channel; expect_rows: one list for all; owed_prev: None or one value per channel."""
    cur = np.atleast_2d(cur)
    n_ch, bs = cur.shape[0], cur.shape[1] // 2
    out = []
    for c in range(n_ch):
        reqs = requests(c, sl, n_sym, bs, prev is not None, sources, pre, post, None if owed_prev is None else owed_prev[c],
                        runs[c], decode_rows[c], expect_rows, search_rows[c])
        recs, hdr = allocate(c, reqs, bs, prev is not None, clock, seq, quota)
        data = [clip_bytes(cur[c], None if prev is None else np.atleast_2d(prev)[c], int(r["t0"]), int(r["n"])) for r in recs]
        out.append((recs, hdr, np.concatenate(data) if data else np.zeros(0, np.uint8)))
    return out


def slot_image(n_ch, quota, per_channel):
    """The whole slot from chunk_model's result: FILL wherever the kernel writes nothing."""
    slot = np.full(slot_bytes(n_ch, quota), FILL, np.uint8)
    recs, hdr, pool = split_slot(slot, n_ch, quota)
    for c, (r, h, data) in enumerate(per_channel):
        recs[c, : r.size] = r
        hdr[c] = h
        pool[c, : data.size] = data
        assert data.size == 2 * h[3]
    return slot


def packed(per_channel):
    """What the receiver's fetch keeps: (records with offset rewritten to the packed place, bytes, dropped per channel)."""
    recs, data, base = [], [], 0
    for r, h, b in per_channel:
        r = r.copy()
        r["offset"] += base
        recs.append(r)
        data.append(b)
        base += h[3]
    return (np.concatenate(recs) if recs else np.zeros(0, CLIP_DTYPE), np.concatenate(data) if data else np.zeros(0, np.uint8),
            np.asarray([h[1] for _, h, _ in per_channel], np.uint32))


# ------------------------------------------------------------------------------------------ crafted launches
def run(first, windows, channel=0):
    """A run record as far as the kernel reads it; the other fields hold what k_chan_bursts might have written."""
    return (channel, first, windows, (1 if first == 0 else 0), 1000 * windows, 1000, 0, 5, -7)


def msg(channel, tau, clock=0, flags=0):
    """A message row as far as the kernel reads it: channel, tau and time = clock + tau."""
    return (channel, 0, tau, flags, (int(clock) + tau) % 2 ** 64, 1, 3, 4, [0] * 10, 0, 0, [0, 0, 0, 0])


def _filled(shape, dtype):
    return np.frombuffer(bytes([FILL]) * (int(np.prod(shape)) * dtype.itemsize), dtype).reshape(shape).copy()


def random_bytes(seed, n_ch, bs):
    return np.random.default_rng(seed).integers(0, 256, (n_ch, 2 * bs), dtype=np.uint8)


class CLaunch:
    """One launch of the hook.  runs / msgs: one list of records per channel; expect: None or [(n_msgs, row or None)] per
    table entry; search: None or {(centre, channel): [rows]} with n_search; owed_prev: None or one value per channel.
    ``want`` is the model's image of the whole slot."""

    def __init__(self, name, sl, n_sym, bs, n_ch, sources, pre, post, quota, runs=None, msgs=None, expect=None, search=None,
                 n_search=0, owed_prev=None, prev=True, clock=0, seq=5, seed=0, cur=None, prev_bytes=None):
        self.name, self.sl, self.n_sym, self.bs, self.n_ch = name, sl, n_sym, bs, n_ch
        self.cfg = DC.config(sl, n_sym, bs)
        self.sources, self.pre, self.post, self.quota, self.clock, self.seq = sources, pre, post, quota, clock, seq
        self.cur = random_bytes(9000 + seed, n_ch, bs) if cur is None else np.ascontiguousarray(cur, np.uint8)
        self.prev = (random_bytes(9500 + seed, n_ch, bs) if prev_bytes is None else np.ascontiguousarray(prev_bytes, np.uint8)) if prev else None
        self.cap = BC.cap_of(bs // W)
        runs = [[] for _ in range(n_ch)] if runs is None else runs
        msgs = [[] for _ in range(n_ch)] if msgs is None else msgs
        assert len(runs) == n_ch == len(msgs)
        self.runs, self.n_runs = _filled((n_ch, self.cap), BURST_DTYPE), np.zeros(n_ch, np.uint32)
        self.msgs, self.n_msgs = _filled((n_ch, self.cap), BURST_MSG_DTYPE), np.zeros(n_ch, np.uint32)
        for c in range(n_ch):
            assert len(runs[c]) <= self.cap and len(msgs[c]) <= self.cap
            for i, r in enumerate(runs[c]):
                self.runs[c, i] = r
            for i, r in enumerate(msgs[c]):
                self.msgs[c, i] = r
            self.n_runs[c], self.n_msgs[c] = len(runs[c]), len(msgs[c])
        self.x_msgs = self.x_hdr = self.s_msgs = self.s_hdr = None
        self.n_expect, self.n_search = 0, 0
        expect_rows, search_rows = [], [[] for _ in range(n_ch)]
        if expect is not None:
            self.n_expect = len(expect)
            assert 1 <= self.n_expect <= BX_MAX
            self.x_msgs, self.x_hdr = _filled((BX_MAX,), BURST_MSG_DTYPE), _filled((BX_MAX,), X_HDR_DTYPE)
            for i, (n_msgs, row) in enumerate(expect):
                self.x_hdr[i] = (n_msgs, 1, seq & 0xFFFFFFFF, 0)
                if row is not None:
                    self.x_msgs[i] = row                     # (a row under n_msgs = 0 is a stale one: the kernel must not read it)
                if n_msgs == 1:
                    expect_rows.append(self.x_msgs[i])
        if search is not None:
            self.n_search = n_search
            assert 1 <= n_search <= BS_MAX
            self.s_msgs, self.s_hdr = _filled((BS_MAX, n_ch, BS_PER), BURST_MSG_DTYPE), _filled((BS_MAX, n_ch), SEARCH_HDR_DTYPE)
            for i in range(n_search):
                for c in range(n_ch):
                    rows = search.get((i, c), [])
                    self.s_hdr[i, c] = (len(rows), len(rows), seq & 0xFFFFFFFF, 0)
                    for p, r in enumerate(rows):
                        self.s_msgs[i, c, p] = r
                        search_rows[c].append(self.s_msgs[i, c, p])
        self.owed_prev = None if owed_prev is None else np.ascontiguousarray(owed_prev, np.uint32)
        assert self.owed_prev is None or self.owed_prev.size == n_ch
        self.model = chunk_model(self.cur, self.prev, sl, n_sym, clock, seq, sources, pre, post, quota, self.owed_prev,
                                 [self.runs[c, : int(self.n_runs[c])] for c in range(n_ch)],
                                 [self.msgs[c, : int(self.n_msgs[c])] for c in range(n_ch)], expect_rows, search_rows)
        self.want = slot_image(n_ch, quota, self.model)

    def records(self, c):
        return self.model[c][0]

    def header(self, c):
        return dict(zip(HDR_DTYPE.names, self.model[c][1]))

    def owed(self):
        return np.asarray([m[1][2] for m in self.model], np.uint32)


@functools.lru_cache(maxsize=None)
def chain_launches():
    """B = 128, one window, post = 1024: a run in launch 0 owes 1024 outputs, and the tails of the four launches behind it
    are each cut again at B - 896, 768, 640, 512 still owed.  Launch 0 has no chunk before: its pre-roll is cut."""
    out, owed, prev = [], None, None
    for k in range(5):
        L = CLaunch(f"clips_chain_{k}", 4, 40, 128, 2, RUNS, 64, 1024, 512, runs=[[run(0, 1)] if k == 0 else [], []], owed_prev=owed,
                    prev=k > 0, prev_bytes=prev, clock=128 * k, seq=k, seed=10 + k)
        out.append(L)
        owed, prev = L.owed(), L.cur
    assert [int(L.owed()[0]) for L in out] == [1024, 896, 768, 640, 512] and all(int(L.owed()[1]) == 0 for L in out)
    r0 = out[0].records(0)[0]
    assert (int(r0["source"]), int(r0["flags"]), int(r0["t0"]), int(r0["n"])) == (RUN, CUT_START | CUT_END, 0, 128)
    for L in out[1:]:
        r = L.records(0)
        assert r.size == 1 and (int(r[0]["source"]), int(r[0]["flags"]), int(r[0]["t0"]), int(r[0]["n"]), int(r[0]["ref"])) == (TAIL, CUT_END, 0, 128, 0)
        assert L.records(1).size == 0 and L.header(1)["used"] == 0
    return tuple(out)


@functools.lru_cache(maxsize=None)
def window0_launches():
    """A run at window 0, B = 256 with pre = 512 and B = 2048 with pre = 256, with and without a chunk before: the pre-roll
    comes from the chunk before (bit 2) as far as it reaches (B = 256: cut at -256, bit 0 too), or is cut at t = 0."""
    out = []
    for bs, pre in ((256, 512), (2048, 256)):
        for have_prev in (True, False):
            L = CLaunch(f"clips_window0_{bs}_{int(have_prev)}", 4, 40, bs, 1, RUNS, pre, 8, 4096, runs=[[run(0, 1)]], prev=have_prev, seed=20 + bs)
            r = L.records(0)[0]
            want = ((-256, CUT_START | FROM_PREV) if bs == 256 else (-256, FROM_PREV)) if have_prev else (0, CUT_START)
            assert (int(r["t0"]), int(r["flags"])) == want and int(r["n"]) == 128 + 8 - want[0]
            assert int(r["time"]) == want[0] % 2 ** 64
            out.append(L)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def end_launches():
    """A run that ends at window nW - 1 (bit 1, owed = post), and the launch behind it, whose list the tail leads in front of
    a run and a row of its own."""
    a = CLaunch("clips_end_0", 4, 40, 256, 2, RUNS, 16, 200, 1024, runs=[[run(1, 1)], [run(0, 2)]], seed=30)
    assert list(a.owed()) == [200, 200] and int(a.records(0)[0]["flags"]) == CUT_END and int(a.records(1)[0]["flags"]) == CUT_END | FROM_PREV
    b = CLaunch("clips_end_1", 4, 40, 256, 2, RUNS | MESSAGES, 16, 8, 1024, runs=[[run(0, 1)], []], msgs=[[msg(0, 50, 256)], []],
                owed_prev=a.owed(), prev_bytes=a.cur, clock=256, seq=6, seed=31)
    assert [int(s) for s in b.records(0)["source"]] == [TAIL, RUN, DECODE] and [int(s) for s in b.records(1)["source"]] == [TAIL]
    assert (int(b.records(0)[0]["t0"]), int(b.records(0)[0]["n"]), int(b.records(0)[0]["flags"])) == (0, 200, 0) and list(b.owed()) == [0, 0]
    assert [int(o) for o in b.records(0)["offset"]] == [0, 200, 200 + 152] and int(b.records(0)[2]["n"]) == 192
    return a, b


@functools.lru_cache(maxsize=None)
def no_roll_launch():
    """pre = post = 0: a run gives its windows alone, a row its packet rounded outwards to multiples of 8."""
    L = CLaunch("clips_no_roll", 14, 80, 1152, 1, RUNS | MESSAGES, 0, 0, 4096, runs=[[run(2, 3)]], msgs=[[msg(0, 13 + 21)]], seed=40)
    r = L.records(0)
    assert [(int(x["t0"]), int(x["n"]), int(x["flags"])) for x in r] == [(256, 384, 0), (16, 1128, 0)] and 21 + 1120 == 1141
    return L


@functools.lru_cache(maxsize=None)
def residue_launch():
    """Rows whose P0 - pre has every residue 0 .. 7 modulo 8, and one with a negative tau; no expect or search slot."""
    rows = [[msg(c, 13 + 16 + 4 * c + i) for i in range(4)] for c in range(2)]
    rows[1].append(msg(1, -100))
    L = CLaunch("clips_residues", 14, 80, 1152, 2, MESSAGES, 8, 8, 8192, msgs=rows, seed=50)
    a = [int(m["tau"]) - 13 - 8 for c in range(2) for m in L.msgs[c, :4]]
    assert sorted(x % 8 for x in a) == list(range(8)) and L.header(0)["n_clips"] == 4 and L.header(1)["n_clips"] == 5
    last = L.records(1)[4]
    assert (int(last["t0"]), int(last["flags"]), int(last["ref"])) == (-128, FROM_PREV, 2 ** 64 - 100) and int(last["time"]) == 2 ** 64 - 128
    assert all(L.header(c)["dropped"] == 0 for c in range(2))
    return L


@functools.lru_cache(maxsize=None)
def per_launch():
    """B = 4608, 17 runs on one channel: the 17th is dropped by RD_BC_PER, not by the quota."""
    L = CLaunch("clips_per", 4, 40, 4608, 2, RUNS, 0, 0, 4096, runs=[[run(2 * i, 1) for i in range(17)], [run(35, 1)]], seed=60)
    h = L.header(0)
    assert L.cap == 18 and (h["n_clips"], h["dropped"], h["used"]) == (16, 1, 2048) and h["used"] + 128 <= 4096
    assert L.header(1)["n_clips"] == 1 and int(L.records(1)[0]["t0"]) == 4480
    return L


@functools.lru_cache(maxsize=None)
def quota_launch():
    """A request too large for what is left of the quota is dropped whole; the smaller one behind it still fits."""
    L = CLaunch("clips_quota", 4, 40, 1152, 1, RUNS, 0, 0, 400, runs=[[run(0, 2), run(3, 5), run(8, 1)]], seed=70)
    h = L.header(0)
    assert (h["n_clips"], h["dropped"], h["used"]) == (2, 1, 384) and [int(x) for x in L.records(0)["ref"]] == [0, 8]
    return L


@functools.lru_cache(maxsize=None)
def sources_launch():
    """All five sources in one launch of three channels, their intervals overlapping: the tail, a run, a decode row, two
    rows of an expect table that also holds an idle entry over a stale row and an entry of another channel, and searched rows
    of two centres - each its own copy, in the definition's order."""
    t = 13 + 29
    ck = 5 * 1152
    expect = [(1, msg(1, t + 1, ck, 8)), (0, msg(1, t, ck, 8)), (1, msg(2, t + 2, ck, 8)), (1, msg(1, t + 3, ck, 8))]
    search = {(0, 1): [msg(1, t, ck, 20), msg(1, t + 2, ck, 20)], (1, 1): [msg(1, t - 1, ck, 20)], (1, 0): [msg(0, 700 - 1120, ck, 20)]}
    L = CLaunch("clips_sources", 14, 80, 1152, 3, RUNS | MESSAGES, 256, 128, 16384, runs=[[], [run(0, 9)], []],
                msgs=[[], [msg(1, t, ck)], []], expect=expect, search=search, n_search=2, owed_prev=[0, 200, 1024], clock=ck, seed=80)
    assert [int(s) for s in L.records(1)["source"]] == [TAIL, RUN, DECODE, EXPECTED, EXPECTED, SEARCHED, SEARCHED, SEARCHED]
    assert [int(r) for r in L.records(1)["ref"]] == [0, 0, ck + t, ck + t + 1, ck + t + 3, ck + t, ck + t + 2, ck + t - 1]
    assert [int(s) for s in L.records(2)["source"]] == [TAIL, EXPECTED] and [int(s) for s in L.records(0)["source"]] == [SEARCHED]
    assert int(L.records(0)[0]["flags"]) == FROM_PREV and int(L.records(2)[0]["n"]) == 1024
    assert all(L.header(c)["dropped"] == 0 for c in range(3))
    return L


@functools.lru_cache(maxsize=None)
def skipped_launch():
    """Records k_chan_bursts never writes, and rows with a channel or a tau out of range, between good ones: skipped, not
    counted as dropped, and the slot untouched where their clips would lie."""
    bs, t = 1152, 13 + 16
    runs = [[run(0, 0), run(9, 1), run(1, 1), run(8, 2), run(3, 2 ** 32 - 1)], [run(2 ** 31, 1)]]
    rows = [[msg(7, t), msg(-1, t), msg(1, t), msg(0, t), msg(0, 40000)], [msg(1, -2 ** 31), msg(1, 13 - 1153), msg(1, 13 + 33), msg(1, 13 + 32)]]
    L = CLaunch("clips_skipped", 14, 80, bs, 2, RUNS | MESSAGES, 8, 8, 8192, runs=runs, msgs=rows, seed=90)
    assert L.cap == 5
    assert [(int(r["source"]), int(r["ref"])) for r in L.records(0)] == [(RUN, 1), (DECODE, t)]
    assert [(int(r["source"]), int(r["ref"])) for r in L.records(1)] == [(DECODE, 13 + 32)]
    assert all(L.header(c)["dropped"] == 0 for c in range(2))
    return L


@functools.lru_cache(maxsize=None)
def shape_launches():
    """(SL, N) = (4, 40), (14, 80), (51, 40) in their smallest blocks: a row at the chunk's end and one that begins in the
    chunk before."""
    out = []
    for sl, n in ((4, 40), (14, 80), (51, 40)):
        bs = W * (-(-(n * sl + 1) // W))
        p_end = bs - n * sl
        L = CLaunch(f"clips_shape_{sl}_{n}", sl, n, bs, 2, MESSAGES, 256, 128, 8192, msgs=[[msg(0, p_end + sl - 1)], [msg(1, -40 + sl - 1)]], seed=100 + sl)
        a, b = L.records(0)[0], L.records(1)[0]
        assert int(a["flags"]) & CUT_END and int(a["t0"]) == (p_end - 256) // 8 * 8 and int(L.owed()[0]) == 128
        assert int(b["flags"]) & FROM_PREV and int(b["t0"]) == max(-296, -bs) and bool(int(b["flags"]) & CUT_START) == (bs < 296)
        out.append(L)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def channels_launch(n_ch):
    """n_ch channels with one or two runs each at places that differ from channel to channel, and a tail on every third."""
    bs = 512
    runs = [[run(c % 4, 1)] + ([run(3, 1)] if c % 4 < 2 and c % 3 == 0 else []) for c in range(n_ch)]
    owed = [8 * (c + 1) if c % 3 == 0 else 0 for c in range(n_ch)]
    L = CLaunch(f"clips_channels_{n_ch}", 4, 40, bs, n_ch, RUNS, 24, 40, 1024, runs=runs, owed_prev=owed, seed=110 + n_ch)
    assert all(L.header(c)["n_clips"] == len(runs[c]) + (1 if owed[c] else 0) for c in range(n_ch))
    return L


def crafted_launches():
    """Every crafted launch of the clip cases, each with its conditions asserted."""
    return chain_launches() + window0_launches() + end_launches() + (no_roll_launch(), residue_launch(), per_launch(), quota_launch(),
            sources_launch(), skipped_launch()) + shape_launches() + tuple(channels_launch(n) for n in (1, 3, 70))


# ------------------------------------------------------------------------------------------ a receiver in NumPy
def stream_model(blocks, cfg, settings, runs, decode_rows, expect_rows, search_rows, clock0=0):
    """Per chunk the packed (records, bytes, dropped) a fetch keeps and the per-channel model.  blocks: the channelized
    bytes [n_ch, 2 B] in order from a reset; settings: per chunk (sources, pre, post, quota), sources 0 = off (None in
    the result, and nothing owed to the next chunk); runs: per chunk the Bursts records; decode_rows / expect_rows /
    search_rows: per chunk the rows as the kernels wrote them (before the host's steps 7), in slot order."""
    sl, n_sym = int(cfg.symbol_length), int(cfg.packet_symbols)
    out, prev, owed = [], None, None
    for k, block in enumerate(blocks):
        block = np.atleast_2d(block)
        n_ch, bs = block.shape[0], block.shape[1] // 2
        sources, pre, post, quota = settings[k]
        if not sources:
            out.append(None)
            prev, owed = block, None
            continue
        per = chunk_model(block, prev, sl, n_sym, clock0 + k * bs, k, sources, pre, post, quota, owed,
                          [[r for r in runs[k] if int(r["channel"]) == c] for c in range(n_ch)],
                          [[r for r in decode_rows[k] if int(r["channel"]) == c] for c in range(n_ch)], list(expect_rows[k]),
                          [[r for r in search_rows[k] if int(r["channel"]) == c] for c in range(n_ch)])
        out.append(packed(per) + (per,))
        prev, owed = block, [p[1][2] for p in per]
    return out
