"""Helpers shared by tests/test_burst_sweep_cpu.py, tests/test_burst_sweep.py and tools/burst_sweep.py (no tests in here):
seeded random launches of the seven burst kernels.  scene(seed) draws one chunk - packet shape, block size, channels, row
stride, clock, the bytes of every channel and the inputs of every stage - as a pure function of the seed; chain(seed)
puts it in front of every family through the Launch classes the crafted cases already use (burst_cases.crafted,
burst_narrow_cases.Launch / burst_repair_cases.Launch, burst_track_cases.XLaunch, burst_search_cases.SLaunch,
burst_quality_cases.QLaunch, burst_clip_cases.CLaunch, clip_replay_cases.Case), each later stage fed with what the models
of the earlier ones wrote.  No model is written here: every expected slot is the existing integer model's.  Nothing here
touches a device.

The draw (scene): (N, SL) cycles through SHAPES, so every admissible shape comes up; block_size from BLOCKS >= LOOK; 1 - 5
channels, sometimes 17 or 65 (those with the two smallest blocks and at most two search centres, to bound the models'
time); in half of the scenes a row stride above 2 block_size with 0xA5 in the gap; prev present or absent; the clock
sometimes within a chunk of 2^64, seq sometimes above 2^32.  A channel is quiet noise, bytes within +-1 of 127.5, a
constant (0, 255, 127, 128, or the zigzag (255, 255), (0, 255), whose products sum to exactly 0 over an even count),
uniformly random bytes, or a background with 0 - 3 FSK bursts: carrier +-0.45 cycles per output, amplitude 2 .. 200 byte
steps (4 counts of a = 2 b - 255 up to hard saturation) or exact 0 / 255 bytes, lead-in and trailer of any length, valid
or the CRC-invalid twin, sometimes inverted, 0 - 3 symbols weakened or flipped; placed anywhere, across prev | cur, cut by
the chunk's end, with the packet against a window boundary, back to back, or as a train of packets.  Thresholds from 0
to 2^32 - 1, among them the energy of one of the channel's own windows.  In a quarter of the scenes run records are
rewritten by hand within what burst_decode_cases.slot_decode_model accepts.

Quality: QLaunch's limits (n_ch <= 4, block_size = LOOK) were limits of the class, not of rd_debug_burst_quality; they are
lifted there, and the quality stage takes every scene.  Narrow and search need SL >= 4: for the scenes below it those
families are skipped and counted (tally: "skipped_narrow", "skipped_search").

Counts over SEEDS on the models alone (tests/test_burst_sweep_cpu.py asserts the floors and prints these):
    every (N, SL) of SHAPES: 16 scenes
    block 'LOOK' 76
    block 'LOOK+128' 80
    block 1152 53
    block 2048 70
    block 2176 51
    block 4096 59
    n_ch 1 73
    n_ch 17 18
    n_ch 2 67
    n_ch 3 62
    n_ch 4 56
    n_ch 5 55
    n_ch 65 21
    clip_channels_dropped 941
    clip_channels_owed 988
    clips 2243
    clock_near_wrap 42
    decode_messages_R0 222
    expect_candidates_no_message 1552
    expect_decoded 264
    expect_nothing_launched 41
    expect_tables_of_64 18
    have_prev 232
    long_runs 355
    look_back_messages 112
    n_runs_above_cap 59
    narrow_rows 91
    narrow_rows_two_grid_points 51
    quality_noise_in_prev 316
    quality_rows 1454
    repair_refused 368
    repaired_only 35
    repaired_two_flips 14
    replay_decoded 312
    replay_jobs 1944
    replay_own_direction_jobs 977
    replay_own_direction_zero 11
    runs_in_bounds 3342
    search_dropped_headers 68
    search_rows 672
    seq_above_2^32 121
    short_regions 1645
    skipped_narrow 96
    skipped_replay 136
    skipped_search 96
    stride_gap 169
Building every chain of SEEDS with every form of expect and replay takes 13 to 23 s of one CPU here, by the machine's
load (tests/test_burst_sweep_cpu.py prints it); the device tests share the chains through cached_chain.
"""
import functools
from collections import Counter
from types import SimpleNamespace

import numpy as np

import burst_cases as BC
import burst_clip_cases as CC
import burst_decode_cases as DC
import burst_narrow_cases as NB
import burst_quality_cases as QC
import burst_repair_cases as RP
import burst_search_cases as SC
import burst_track_cases as TK
import clip_replay_cases as CR
from rtldavis_amd import acquire, synth
from rtldavis_amd.wideband import BURST_DTYPE

W, FILL = DC.W, DC.FILL
N_SET, SL_SET = (40, 64, 80), (1, 3, 4, 5, 8, 14, 25, 51)
SHAPES = tuple((n, sl) for n in N_SET for sl in SL_SET if n * sl + 1 <= 2048)
BLOCKS = ("LOOK", "LOOK+128", 1152, 2048, 2176, 4096)
BIG_CH = (17, 65)
GAP_BYTE = 0xA5
SEEDS = tuple(range(352))
CHAINED = SEEDS[::4]                                         # the seeds of the device test that chains the stages
FAMILIES = ("bursts", "decode", "expect", "search", "quality", "clips", "replay")
MAX_REPLAY_CLIPS = 10


def block_sizes(look):
    """{label: block_size} of the entries of BLOCKS that are >= LOOK."""
    out = {"LOOK": look, "LOOK+128": look + 128}
    out.update({b: b for b in BLOCKS[2:] if b >= look})
    return out


def _rng(seed, stage):
    return np.random.default_rng([20260, int(seed), int(stage)])


def _put_cut(both, at, piece):
    """burst_decode_cases.put for a piece that may reach over either end of the row: the part inside is written."""
    n_out = both.size // 2
    lo, hi = max(at, 0), min(at + piece.size // 2, n_out)
    if hi > lo:
        DC.put(both, lo, piece[2 * (lo - at): 2 * (hi - at)])


# ------------------------------------------------------------------------------------------ the bytes
CONSTANTS = ((0, 0), (255, 255), (127, 127), (128, 128))


def _constant_row(kind, n_out):
    row = np.empty(2 * n_out, np.uint8)
    if kind == "zigzag":
        row[0::2] = np.where(np.arange(n_out) % 2 == 0, 255, 0)
        row[1::2] = 255
    else:
        row[0::2], row[1::2] = kind
    return row


def _burst_piece(rng, sh, saturated, train=None):
    """One burst of the shape sh = (n, sl): (bytes, lead, info).  train: the carrier of a train of clean packets a few
    outputs apart, so that one search centre finds them all."""
    n, sl = sh
    if train is not None:
        data = DC.packet(n, ident=int(rng.integers(0, 8)), seed=int(rng.integers(0, 10 ** 6)))
        lead, amp = int(rng.integers(0, 9)), float(rng.uniform(20.0, 120.0))
        piece = RP.damaged(data, sl, None, amp=amp, phase0=float(rng.uniform(0, 2 * np.pi)), carrier=train, lead=lead, trail=int(rng.integers(0, 9)))
        return piece, lead, SimpleNamespace(data=data, carrier=train, twin=False, amp=amp)
    twin = rng.random() < 0.15
    data = DC.packet(n, ident=int(rng.integers(0, 8)), seed=int(rng.integers(0, 10 ** 6)),
                     flip_bit=int(rng.integers(0, n - 16)) if twin else None)
    lead, trail = int(rng.integers(0, 200)), int(rng.integers(0, 120))
    if rng.random() < 0.15:
        lead = int(rng.integers(0, 2))
    if rng.random() < 0.15:
        trail = 0
    carrier = float(rng.uniform(-0.45, 0.45))
    invert = rng.random() < 0.1
    if saturated:                                            # bytes 0 and 255 only: equal margins at neighbouring taus
        bits = np.unpackbits(np.frombuffer(data, np.uint8)).astype(np.int64)
        t = max(1, (2 * sl) // 3)
        turns = np.where(bits == 1, -t, t) * (-1 if invert else 1)   # (reads as sent under the run's own, negative real, corr)
        return RP.saturated_fsk(data, sl, turns, lead, trail), lead, SimpleNamespace(data=data, carrier=0.5, twin=twin, amp=255)
    scale = {k: -1.0 for k in range(n)} if invert else {}
    for _ in range(int(rng.choice((0, 0, 0, 1, 1, 2, 2, 2, 3)))):
        k = int(rng.integers(16, n)) if rng.random() < 0.9 else int(rng.integers(0, 16))
        scale[k] = scale.get(k, 1.0) * float(rng.choice((RP.WEAK, RP.WEAK, RP.WEAK, -0.6, 0.3, -1.0)))
    amp = float(np.exp(rng.uniform(np.log(2.0), np.log(200.0)))) if rng.random() < 0.5 else float(rng.uniform(20.0, 120.0))
    piece = RP.damaged(data, sl, scale, amp=amp, phase0=float(rng.uniform(0, 2 * np.pi)), carrier=carrier, lead=lead, trail=trail)
    return piece, lead, SimpleNamespace(data=data, carrier=carrier, twin=twin, amp=amp)


def _channel(rng, sh, bs, many):
    """(both: uint8 [4 bs], prev | cur of one channel; planted: [info with p0, the packet's first output relative to cur])."""
    n, sl = sh
    kind = rng.choice(("quiet", "bursts", "uniform", "const", "tiny", "mixed", "zigzag"),
                      p=(0.53, 0.25, 0.05, 0.05, 0.05, 0.05, 0.02) if many else (0.08, 0.58, 0.07, 0.07, 0.07, 0.07, 0.06))
    n_out = 2 * bs
    if kind == "uniform":
        return rng.integers(0, 256, 2 * n_out).astype(np.uint8), []
    if kind == "zigzag":
        return _constant_row("zigzag", n_out), []
    if kind == "const":
        return _constant_row(CONSTANTS[int(rng.integers(0, len(CONSTANTS)))], n_out), []
    if kind == "tiny":
        return rng.integers(127, 129, 2 * n_out).astype(np.uint8), []
    both = BC.quiet_bytes(rng, n_out) if rng.random() < 0.8 else rng.integers(127, 129, 2 * n_out).astype(np.uint8)
    if kind == "quiet":
        return both, []
    if kind == "mixed":                                      # a stretch of uniform bytes in the background
        a = int(rng.integers(0, n_out - 64))
        e = int(rng.integers(a + 1, min(n_out, a + 1500) + 1))
        both[2 * a: 2 * e] = rng.integers(0, 256, 2 * (e - a))
    planted, taken, end, shared = [], [], None, float(rng.uniform(-0.45, 0.45))
    train = n * sl <= 330 and rng.random() < 0.45            # several packets back to back: more than the search keeps
    for j in range(int(rng.integers(5, 8)) if train else int(rng.integers(0, 4))):
        piece, lead, info = _burst_piece(rng, sh, saturated=sl >= 3 and rng.random() < 0.12, train=shared if train else None)
        length = piece.size // 2
        mode = rng.choice(("in", "in", "in", "straddle", "cut", "edge_lo", "edge_hi", "abut"))
        if train:
            p0 = (int(rng.integers(0, 100)) if end is None else end) + lead
        elif mode == "abut" and end is not None:
            p0 = end + lead
        elif mode == "straddle":
            p0 = -int(rng.integers(1, n * sl))
        elif mode == "cut":
            p0 = bs - int(rng.integers(1, n * sl + 40))
        elif mode == "edge_lo":                              # the first symbol begins one output behind a window boundary
            p0 = W * int(rng.integers(0, bs // W)) + 1
        elif mode == "edge_hi":                              # the last symbol ends one output before one
            p0 = W * int(rng.integers(-(-(n * sl) // W), bs // W + 1)) - n * sl
        else:                                                # anywhere, beside the bursts already there if a few draws find room
            for _ in range(6):
                p0 = int(rng.integers(-bs // 2, bs))
                if all(p0 - lead >= e or p0 - lead + length <= a for a, e in taken):
                    break
        at = bs + p0 - lead                                  # index into both
        taken.append((p0 - lead, p0 - lead + length))
        _put_cut(both, at, piece)
        info.p0, end = p0, p0 - lead + length
        planted.append(info)
    return both, planted


def _threshold(rng, p_row, planted):
    kind = rng.choice(("between", "median", "window", "zero", "max", "strong"), p=(0.7, 0.06, 0.08, 0.04, 0.04, 0.08) if planted else
                      (0.3, 0.2, 0.2, 0.1, 0.1, 0.1))
    srt = np.sort(p_row)
    if kind == "between":
        return int(np.sqrt(float(max(1, srt[srt.size // 4])) * float(max(1, srt[-1]))))
    if kind == "median":
        return int(srt[srt.size // 2])
    if kind == "window":                                     # exactly one window's energy (the >=), or one above it
        return min(2 ** 32 - 1, int(p_row[int(rng.integers(0, p_row.size))]) + int(rng.integers(0, 2)))
    if kind == "strong":
        return int(0.9 * float(srt[-1])) + 1
    return 0 if kind == "zero" else 2 ** 32 - 1


def _perturb_runs(rng, runs, n_runs, n_win):
    """Records rewritten by hand within what slot_decode_model accepts: first / windows in and out of bounds with flags
    as k_chan_bursts would set them, corr random with (0, 0) and +-(2^30 - 1), n_runs above cap."""
    n_ch, cap = runs.shape
    big = 2 ** 30 - 1
    for c in rng.choice(n_ch, size=min(n_ch, int(rng.integers(1, 4))), replace=False):
        for _ in range(int(rng.integers(1, 4))):
            j = int(rng.integers(0, min(cap, int(n_runs[c]) + 2)))
            rec = runs[c, j].copy()
            if j >= int(n_runs[c]) or rng.random() < 0.5:
                first = int(rng.choice((0, int(rng.integers(0, n_win)), n_win - 1, n_win, n_win + 1, 2 ** 31, 2 ** 32 - 1)))
                windows = int(rng.choice((0, 1, int(rng.integers(1, 34)), 32, 33, max(1, n_win - min(first, n_win)), 2 ** 32 - 1)))
                flags = (1 if first == 0 else 0) | (2 if first + windows == n_win else 0)
                rec = np.asarray([(c, first, windows, flags, 1000 * (windows % 64), 1000, 0, 5, -7)], BURST_DTYPE)[0]
            pick = rng.random()
            if pick < 0.15:
                rec["corr_re"], rec["corr_im"] = 0, 0
            elif pick < 0.35:
                rec["corr_re"], rec["corr_im"] = (int(rng.choice((-big, big))), int(rng.choice((-big, 0, big))))
            elif pick < 0.6:
                rec["corr_re"], rec["corr_im"] = (int(rng.integers(-big, big + 1)), int(rng.integers(-big, big + 1)))
            elif pick < 0.7:
                rec["corr_re"], rec["corr_im"] = (int(rng.integers(-2, 3)), int(rng.integers(-2, 3)))
            runs[c, j] = rec
            n_runs[c] = max(int(n_runs[c]), j + 1)
        if rng.random() < 0.4:
            n_runs[c] = cap + int(rng.integers(1, 6))
    return runs, n_runs


def _abs_window(clock, lo, hi):
    """(t_lo, t_hi) of the window clock + lo .. clock + hi as the table holds it: a window that would wrap at 2^64 (or
    reach below 0) is cut at the wrap, for the table rule is t_lo <= t_hi."""
    a, b = int(clock) + lo, int(clock) + hi
    if a < 0 <= b:
        a = 0
    if a < 2 ** 64 <= b:
        b = 2 ** 64 - 1
    return a % 2 ** 64, b % 2 ** 64


def _random_corr(rng):
    while True:
        c = (int(rng.integers(-32768, 32768)), int(rng.integers(-32768, 32768)))
        if c != (0, 0):
            return c


def _expect_table(rng, sc):
    n, sl, bs = sc.n, sc.sl, sc.bs
    body = sl * (n - 1)
    bursts = [(c, b) for c in range(sc.n_ch) for b in sc.planted[c]]
    n_rows = 64 if rng.random() < 0.06 else int(rng.integers(1, 13))
    all_idle = rng.random() < 0.05
    rows = []
    for _ in range(n_rows):
        kind = "outside" if all_idle else rng.choice(("on", "on", "on", "beside", "seam", "outside", "random"))
        c, corr, ident = int(rng.integers(0, sc.n_ch)), _random_corr(rng), TK.ANY
        if kind in ("on", "beside") and bursts:
            c, b = bursts[int(rng.integers(0, len(bursts)))]
            tau = b.p0 + sl - 1
            if kind == "beside":
                tau += int(rng.choice((-1, 1))) * int(rng.integers(sl, 3 * sl + 2))
            lo, hi = tau - int(rng.choice((0, 0, int(rng.integers(0, 40))))), tau + int(rng.choice((0, 0, int(rng.integers(0, 40)))))
            if rng.random() < 0.7:
                corr = TK.corr_of(b.carrier)
            right = synth._swap_bits8(b.data[2]) & 7
            ident = int(rng.choice((right, right, (right + 1 + int(rng.integers(0, 7))) % 8, TK.ANY, TK.ANY)))
        elif kind == "seam":
            lo, hi = -int(rng.integers(0, body + 60)), int(rng.integers(0, 60))
        elif kind == "outside":
            lo = int(rng.choice((bs + int(rng.integers(0, 3000)), -body - 2 * bs - int(rng.integers(1, 3000)))))
            hi = lo + int(rng.integers(0, 200))
        else:
            lo = int(rng.integers(-bs, bs))
            hi = lo + int(rng.integers(0, TK.MAX_SPAN + 1))
        if hi - lo > TK.MAX_SPAN:
            hi = lo + TK.MAX_SPAN
        t_lo, t_hi = _abs_window(sc.clock, lo, hi)
        rows.append(TK.expect_row(c, t_lo, t_hi, corr, ident))
    return TK.table(rows)


def _search_centres(rng, sc):
    carriers = [b.carrier for c in range(sc.n_ch) for b in sc.planted[c]]
    rate = 19200 * sc.sl
    out = []
    if carriers:
        some = [carriers[int(i)] for i in rng.choice(len(carriers), size=min(len(carriers), 3), replace=False)]
        out += [int(g) for g in acquire.search_centres([f * rate for f in some], rate, if_hz=0, spread=int(rng.integers(0, 2)))]
    out += [int(g) for g in rng.integers(0, NB.GRID, int(rng.integers(1, 4)))]
    out = list(dict.fromkeys(out))                           # (no duplicates: the list's rule)
    rng.shuffle(out)
    return out[: 2 if sc.n_ch > 5 else int(rng.integers(1, SC.MAX_CENTRES + 1))]


@functools.lru_cache(maxsize=None)
def scene(seed):
    """One chunk and the inputs of every stage, a pure function of the seed."""
    rng = _rng(seed, 0)
    n, sl = SHAPES[seed % len(SHAPES)]
    cfg0 = DC.config(sl, n, 4096)
    look = DC.shape(cfg0)[3]
    r = rng.random()
    n_ch = BIG_CH[0] if r < 0.06 else BIG_CH[1] if r < 0.12 else int(rng.integers(1, 6))
    sizes = block_sizes(look)
    labels = [k for k in BLOCKS if k in sizes]
    if n_ch > 5:
        labels = labels[:2]
    label = labels[int(rng.integers(0, len(labels)))]
    bs = sizes[label]
    sc = SimpleNamespace(seed=seed, n=n, sl=sl, look=look, bs=bs, block_label=label, n_ch=n_ch, cfg=DC.config(sl, n, bs),
                         n_win=bs // W, cap=BC.cap_of(bs // W))
    sc.stride = 2 * bs + (16 * int(rng.integers(1, 5)) if rng.random() < 0.5 else 0)
    sc.have_prev = bool(rng.random() < 0.65)
    pick = rng.random()
    sc.clock = (2 ** 64 - int(rng.integers(1, bs)) if pick < 0.15 else int(rng.integers(1, 2 ** 40)) if pick < 0.5 else
                bs * int(rng.integers(1 if sc.have_prev else 0, 1000)))
    sc.seq = 2 ** 32 + int(rng.integers(0, 2 ** 33)) if rng.random() < 0.3 else int(rng.integers(0, 1000))
    rows = [_channel(rng, (n, sl), bs, n_ch > 5) for _ in range(n_ch)]
    both = np.stack([b for b, _ in rows])
    sc.planted = [p for _, p in rows]
    sc.cur = np.ascontiguousarray(both[:, 2 * bs:])
    sc.prev = np.ascontiguousarray(both[:, : 2 * bs]) if sc.have_prev else None
    p = BC.window_sums(sc.cur)[0]
    sc.thr = np.asarray([_threshold(rng, p[c], sc.planted[c]) for c in range(n_ch)], np.uint64)
    # ---- the later stages' own inputs, each from a generator of its own
    sc.perturb = bool(_rng(seed, 1).random() < 0.25)
    sc.table = _expect_table(_rng(seed, 2), sc)
    sc.centres = _search_centres(_rng(seed, 3), sc) if sl >= NB.MIN_SL else None
    q = _rng(seed, 4)
    forms = TK.ALL_FORMS if sl >= NB.MIN_SL else TK.ALL_FORMS[:3]
    sc.feed_form = forms[int(q.integers(0, len(forms)))]     # (max_flips, narrow) of the rows that quality and clips are fed
    sc.gap = int(q.choice((0, 0, int(q.integers(0, QC.MAX_GAP + 1)), QC.MAX_GAP)))
    sc.sources = int(q.integers(1, 4))
    sc.pre, sc.post = 8 * int(q.integers(0, 129)), 8 * int(q.integers(0, 129))
    sc.quota = 8 * int(q.choice((1, int(q.integers(1, 64)), int(q.integers(64, 1024)), int(q.integers(256, 2048)), 1024)))
    if q.random() < 0.7:
        sc.owed_prev = np.where(q.random(n_ch) < 0.5, q.integers(0, CC.MAX_ROLL + 1, n_ch), 0).astype(np.uint32)
        if q.random() < 0.2:
            sc.owed_prev[int(q.integers(0, n_ch))] = int(q.choice((CC.MAX_ROLL + 1, 2 ** 32 - 1)))
    else:
        sc.owed_prev = None
    return sc


def device_bytes(sc):
    """(cur, prev or None) as the hooks take them: [n_ch, stride] with GAP_BYTE behind every row's 2 block_size bytes."""
    def lay(a):
        if a is None:
            return None
        out = np.full((sc.n_ch, sc.stride), GAP_BYTE, np.uint8)
        out[:, : 2 * sc.bs] = a
        return out
    return lay(sc.cur), lay(sc.prev)


# ------------------------------------------------------------------------------------------ the stages
def make_bursts(sc):
    cs = BC.crafted(f"sweep{sc.seed}_bursts", list(sc.cur), sc.thr, seq=sc.seq, gap=sc.stride - 2 * sc.bs)
    cs.chan[:, 2 * sc.bs:] = GAP_BYTE
    return cs


def runs_of_slot(recs, floor):
    """(runs [n_ch][cap], n_runs) of a bursts slot - the model's or a device's - as the decode hook takes them."""
    return np.ascontiguousarray(recs), np.ascontiguousarray(floor["n_bursts"], np.uint32)


def scene_runs(sc, recs, floor):
    """The run table of the scene: the given bursts slot, rewritten by hand in the scenes drawn for it."""
    runs, n_runs = runs_of_slot(recs.copy(), floor)
    if sc.perturb:
        runs, n_runs = _perturb_runs(_rng(sc.seed, 1), runs, n_runs.copy(), sc.n_win)
    return runs, n_runs


def make_decode(sc, runs, n_runs):
    cls = NB.Launch if sc.sl >= NB.MIN_SL else RP.Launch
    return cls(f"sweep{sc.seed}_decode", sc.cfg, list(sc.cur), prev=None if sc.prev is None else list(sc.prev), runs=runs,
               n_runs=n_runs, clock=sc.clock, seq=sc.seq)


def decode_forms(sc):
    return TK.ALL_FORMS if sc.sl >= NB.MIN_SL else TK.ALL_FORMS[:3]


def decode_want(L, r, narrow):
    return L.narrow[r] if narrow else L.want[r]


def make_expect(sc):
    return TK.XLaunch(f"sweep{sc.seed}_expect", sc.cfg, list(sc.cur), sc.table, prev=None if sc.prev is None else list(sc.prev),
                      clock=sc.clock, seq=sc.seq)


def make_search(sc):
    if sc.centres is None:
        return None
    return SC.SLaunch(f"sweep{sc.seed}_search", sc.cfg, list(sc.cur), sc.centres, prev=None if sc.prev is None else list(sc.prev),
                      clock=sc.clock, seq=sc.seq)


def handwritten_rows(sc):
    """Per channel a few (channel, tau, f_re, f_im) no decoder wrote: any tau, f = (0, 0) and large, a wrong channel."""
    rng = _rng(sc.seed, 5)
    out = []
    for c in range(sc.n_ch):
        rows = []
        for _ in range(int(rng.integers(0, 3)) if sc.n_ch <= 5 else int(rng.random() < 0.2)):
            tau = int(rng.choice((int(rng.integers(-sc.bs, sc.bs)), int(rng.integers(0, sc.sl + 40)), sc.bs - sc.n * sc.sl + sc.sl - 1,
                                  int(rng.integers(-2 ** 31, 2 ** 31)))))
            f = (0, 0) if rng.random() < 0.2 else (int(rng.integers(-2 ** 36, 2 ** 36)), int(rng.integers(-2 ** 36, 2 ** 36)))
            ch = c if rng.random() < 0.85 else int(rng.choice((-1, sc.n_ch, 7 + sc.n_ch)))
            rows.append((ch, tau) + f)
        out.append(rows)
    return out


def make_quality(sc, msgs, n_msgs):
    """On the decode slot's rows (msgs [n_ch][cap], n_msgs) and handwritten rows behind them, as far as cap allows."""
    extra = handwritten_rows(sc)
    records = []
    for c in range(sc.n_ch):
        mine = [msgs[c, i] for i in range(int(n_msgs[c]))]
        records.append(mine + extra[c][: sc.cap - len(mine)])
    return QC.QLaunch(f"sweep{sc.seed}_quality", sc.cfg, list(sc.cur), None if sc.prev is None else list(sc.prev), sc.gap, records)


def expect_feed(sc, x_slot):
    """burst_clip_cases.CLaunch's ``expect`` of an expect slot (msgs, hdr); None when the kernel was not launched."""
    msgs, hdr = x_slot
    if hdr.tobytes() == bytes([FILL]) * hdr.nbytes:
        return None
    return [(int(hdr[i]["n_msgs"]), msgs[i].copy() if int(hdr[i]["n_msgs"]) == 1 else None) for i in range(sc.table.size)]


def search_feed(sc, s_slot):
    if s_slot is None:
        return None
    msgs, hdr = s_slot
    return {(i, c): [msgs[i, c, p].copy() for p in range(int(hdr[i, c]["n_msgs"]))] for i in range(len(sc.centres)) for c in range(sc.n_ch)}


def make_clips(sc, runs, n_runs, msgs, n_msgs, x_slot, s_slot):
    """Fed with the run table (the cap places the hook admits), the decode slot's rows, the expect slot and the search slot
    as they are; without RD_BC_MESSAGES the hook takes no expect or search slot."""
    want_msgs = bool(sc.sources & CC.MESSAGES)
    search = search_feed(sc, s_slot) if want_msgs else None
    return CC.CLaunch(f"sweep{sc.seed}_clips", sc.sl, sc.n, sc.bs, sc.n_ch, sc.sources, sc.pre, sc.post, sc.quota,
                   runs=[[runs[c, i] for i in range(min(int(n_runs[c]), sc.cap))] for c in range(sc.n_ch)],
                   msgs=[[msgs[c, i] for i in range(int(n_msgs[c]))] for c in range(sc.n_ch)],
                   expect=expect_feed(sc, x_slot) if want_msgs else None, search=search, n_search=0 if search is None else len(sc.centres),
                   owed_prev=sc.owed_prev, prev=sc.prev is not None, clock=sc.clock, seq=sc.seq, cur=sc.cur, prev_bytes=sc.prev)


def _signed64(x):
    x = int(x) % 2 ** 64
    return x - 2 ** 64 if x >= 2 ** 63 else x


def make_replay(sc, slot):
    """A clip_replay_cases.Case on the recordings of a clip slot image (the model's or a device's): None without a clip."""
    recs, hdr, pool = CC.split_slot(slot, sc.n_ch, sc.quota)
    found = [(c, recs[c, i]) for c in range(sc.n_ch) for i in range(int(hdr[c]["n_clips"]))]
    if not found:
        return None
    rng = _rng(sc.seed, 6)
    if len(found) > MAX_REPLAY_CLIPS:
        found = [found[int(i)] for i in sorted(rng.choice(len(found), size=MAX_REPLAY_CLIPS, replace=False))]
    clips = [pool[c, 2 * int(r["offset"]): 2 * (int(r["offset"]) + int(r["n"]))].copy() for c, r in found]
    span = CR.MAX_SPAN
    carriers = {c: [b.carrier for b in sc.planted[c]] for c in range(sc.n_ch)}
    jobs, clip_of = [], []

    def direction(c):
        pick = rng.random()
        if pick < 0.5:
            return (0, 0)                                    # the region's own
        if pick < 0.8 and carriers[c]:
            return TK.corr_of(carriers[c][int(rng.integers(0, len(carriers[c])))])
        return _random_corr(rng)

    for k, (c, r) in enumerate(found):
        n = int(r["n"])
        if int(r["source"]) in (CC.DECODE, CC.EXPECTED, CC.SEARCHED):   # the packet the clip was cut for
            tau = _signed64(int(r["ref"]) - int(r["time"]))
            lo, hi = tau - int(rng.integers(0, 30)), tau + int(rng.integers(0, 30))
        else:
            # (from SL + 1 to the clip's end the region holds an even number of products: a zigzag row's sum to exactly (0, 0))
            lo = int(rng.choice((0, sc.sl + 1)))
            hi = max(lo, min(n, span))
        jobs.append((k, n, lo, hi, direction(c), CR.ANY_ID, c, int(r["time"])))
        clip_of.append(k)
    for _ in range(int(rng.integers(2, 7))):
        k = int(rng.integers(0, len(found)))
        c, r = found[k]
        n = int(r["n"])
        lo = int(rng.integers(-50, n + 50))
        hi = lo + 2 * int(rng.integers(0, span // 2 + 1)) + int(rng.random() < 0.3)   # (mostly even: see the zigzag rows)
        ident = CR.ANY_ID if rng.random() < 0.8 else int(rng.integers(0, 8))
        jobs.append((k, n, lo, min(hi, lo + span), direction(c), ident, c, int(rng.integers(0, 2 ** 40))))
        clip_of.append(k)
    return CR.Case(f"sweep{sc.seed}_replay", sc.sl, sc.n, clips,
                   lambda off: [CR.job_row(off[k], n, lo, hi, corr, ident, channel=c, clock=clock) for k, n, lo, hi, corr, ident, c, clock in jobs],
                   clip_of)


class Chain:
    """The launches of every family for one scene, each built when first asked for; a family that does not apply to the
    scene is None (search below SL 4; replay when the clip model recorded nothing)."""

    def __init__(self, seed):
        self.seed, self.scene = seed, scene(seed)

    @functools.cached_property
    def bursts(self):
        return make_bursts(self.scene)

    @functools.cached_property
    def runs(self):
        return scene_runs(self.scene, *BC.slot_model(self.bursts))

    @functools.cached_property
    def decode(self):
        return make_decode(self.scene, *self.runs)

    @functools.cached_property
    def expect(self):
        return make_expect(self.scene)

    @functools.cached_property
    def search(self):
        return make_search(self.scene)

    @functools.cached_property
    def fed(self):
        """(msgs, n_msgs) of the decode model at the scene's feed form: the rows quality and clips are fed."""
        return decode_want(self.decode, *self.scene.feed_form)[:2]

    @functools.cached_property
    def quality(self):
        return make_quality(self.scene, *self.fed)

    @functools.cached_property
    def clips(self):
        sc = self.scene
        return make_clips(sc, *self.runs, *self.fed, self.expect.want(*sc.feed_form), None if self.search is None else self.search.want())

    @functools.cached_property
    def replay(self):
        return make_replay(self.scene, self.clips.want)

    def build(self, families=FAMILIES):
        for f in families:
            getattr(self, f)
        return self


def chain(seed):
    """Every family's launch of scene(seed), built: what a failure message's seed rebuilds."""
    return Chain(seed).build()


@functools.lru_cache(maxsize=None)
def cached_chain(seed):
    """A Chain shared by the tests of one process: families are built as the tests ask for them."""
    return Chain(seed)


# ------------------------------------------------------------------------------------------ what the models report
def tally(ch):
    """The counts of one chain that tests/test_burst_sweep_cpu.py sums over SEEDS and holds against its floors."""
    sc, t = ch.scene, Counter()
    t["shape", sc.n, sc.sl] += 1
    t["block", sc.block_label] += 1
    for label, b in block_sizes(sc.look).items():            # (a size two labels share counts for both)
        if b == sc.bs and label != sc.block_label:
            t["block", label] += 1
    t["n_ch", sc.n_ch] += 1
    t["stride_gap"] += sc.stride > 2 * sc.bs
    t["have_prev"] += sc.have_prev
    t["clock_near_wrap"] += sc.clock >= 2 ** 64 - sc.bs
    t["seq_above_2^32"] += sc.seq >= 2 ** 32
    L = ch.decode
    runs, n_runs = ch.runs
    t["decode_messages_R0"] += int(L.want[0][1].sum())
    two = L.want[2]
    for c in range(sc.n_ch):
        for m in two[0][c, : int(two[1][c])]:
            if int(m["flags"]) & RP.REPAIRED:
                t["repaired_only"] += 1
                t["repaired_two_flips"] += int(m["pad"][0]) == 2
        for m in L.want[0][0][c, : int(L.want[0][1][c])]:
            t["look_back_messages"] += int(m["flags"]) & 1
        t["n_runs_above_cap"] += int(n_runs[c]) > sc.cap
        for rec in runs[c, : min(int(n_runs[c]), sc.cap)]:
            first, windows = int(rec["first"]), int(rec["windows"])
            if windows > DC.MAX_W or windows == 0 or first >= sc.n_win or first + windows > sc.n_win:
                continue
            t["runs_in_bounds"] += 1
            back = bool(int(rec["flags"]) & 1) and sc.have_prev
            t["short_regions"] += W * windows + (sc.look if back else 0) < sc.n * sc.sl + 1
            if (int(rec["corr_re"]), int(rec["corr_im"])) != (0, 0):
                got = RP.symbol_sums(sc.cur[c], None if sc.prev is None else sc.prev[c], rec, sc.cfg, sc.have_prev)
                if got is not None:
                    sync = np.all((got[1][:, :16] > 0) == np.asarray(RP.SYNC, bool)[None, :], axis=1)
                    if sync.any():
                        t["repair_refused"] += int((RP.repair_batch(got[1][sync], 2) == -1).sum())
    t["long_runs"] += int(L.long_runs.sum())
    if sc.sl >= NB.MIN_SL:
        g = [int(m["pad"][3]) for c in range(sc.n_ch) for m in L.narrow[0][0][c, : int(L.narrow[0][1][c])]]
        t["narrow_rows"] += len(g)
        t["narrow_rows_two_grid_points"] += len(g) if len(set(g)) >= 2 else 0
    else:
        t["skipped_narrow"] += 1
        t["skipped_search"] += 1
    hdr = ch.expect.want(0, False)[1]
    if hdr.tobytes() == bytes([FILL]) * hdr.nbytes:
        t["expect_nothing_launched"] += 1
    else:
        live = hdr[: sc.table.size]
        t["expect_decoded"] += int((live["n_msgs"] == 1).sum())
        t["expect_candidates_no_message"] += int(((live["candidates"] > 0) & (live["n_msgs"] == 0)).sum())
    t["expect_tables_of_64"] += sc.table.size == TK.MAX
    if ch.search is not None:
        s_hdr = ch.search.want()[1][: len(sc.centres)]
        t["search_rows"] += int(s_hdr["n_msgs"].sum())
        t["search_dropped_headers"] += int((s_hdr["dropped"] > 0).sum())
    Q = ch.quality
    for c in range(sc.n_ch):
        for i in range(int(Q.n_msgs[c])):
            m = Q.msgs[c, i]
            win = QC.windows(sc.sl, sc.n, sc.bs, sc.have_prev, int(m["tau"]), sc.gap) if 0 <= int(m["channel"]) < sc.n_ch else None
            t["quality_rows"] += 1
            t["quality_noise_in_prev"] += win is not None and win[3] < 0 and win[4] > win[3]
    X = ch.clips
    for c in range(sc.n_ch):
        h = X.header(c)
        t["clips"] += h["n_clips"]
        t["clip_channels_dropped"] += h["dropped"] > 0
        t["clip_channels_owed"] += h["owed"] > 0
    R = ch.replay
    if R is None:
        t["skipped_replay"] += 1
    else:
        _, r_hdr, _ = R.want(0, False)
        t["replay_jobs"] += R.jobs.size
        t["replay_decoded"] += int(r_hdr["n_msgs"].sum())
        own = (R.jobs["corr_re"] == 0) & (R.jobs["corr_im"] == 0)
        t["replay_own_direction_jobs"] += int(own.sum())
        t["replay_own_direction_zero"] += int((own & (r_hdr["candidates"] > 0) & (r_hdr["ca"] == 0) & (r_hdr["cb"] == 0)).sum())
    return t
