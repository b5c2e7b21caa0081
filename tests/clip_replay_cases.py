"""Helpers shared by tests/test_clip_replay_cpu.py, tests/test_clip_replay.py and tools/clip_replay_rate.py (no tests in
here): the model of k_clip_decode (include/rtldavis_hip.h, CLIP DECODE) and its cases.  The model is a thin wrapper
around burst_track_cases.decode_expect - the integer model of BURST EXPECT, written from the definition - called with
the clip as a chunk of its own: the configuration with block_size = n, no chunk before, the job's clock.  The wrapper
maps the record's flags 8 -> 32, and adds in NumPy / Python integers what CLIP DECODE has and BURST EXPECT has not: the
own direction, the header's (ca, cb) and the soft values.  Every case asserts, on the model and when it is built, the
edge it is built for.  Nothing here touches a device."""
import functools

import numpy as np

import burst_cases as BC
import burst_decode_cases as DC
import burst_narrow_cases as NB
import burst_repair_cases as RP
import burst_track_cases as TC
from rtldavis_amd.replay import ANY_ID, CD_HEADER_DTYPE, CLIP_JOB_DTYPE, MAX_SPAN, REPLAYED
from rtldavis_amd.wideband import BURST_MSG_DTYPE

FORMS = TC.ALL_FORMS                                         # (max_flips, narrow): R = 0, 1, 2 without and with the filter
CARRIER = TC.CARRIER


def forms_for(sl):
    """The forms a symbol length admits."""
    return FORMS if sl >= NB.MIN_SL else FORMS[:3]


def job_row(offset, n, tau_lo, tau_hi, corr=(0, 0), ident=ANY_ID, channel=0, clock=0, pad=0):
    return (int(offset), int(clock) % 2 ** 64, int(n), int(ident), int(tau_lo), int(tau_hi), int(corr[0]), int(corr[1]), int(channel),
            int(pad))


def jobs_of(rows):
    return np.asarray(list(rows), CLIP_JOB_DTYPE).reshape(-1)


# ------------------------------------------------------------------------------------------ the definition
def job_range(n, tau_lo, tau_hi, sl, n_sym):
    """None (idle), or (tau_a, tau_b)."""
    a, b = max(int(tau_lo), sl), min(int(tau_hi), int(n) - 1 - sl * (n_sym - 1))
    return (a, b) if a <= b else None


def region_sum(clip, t0, t1):
    """F = the sum of p[t] = z[t] conj(z[t-1]) over t0 < t < t1, in Python integers."""
    a = 2 * np.asarray(clip, np.int64).reshape(-1) - 255
    zi, zq = a[0::2][t0:t1], a[1::2][t0:t1]
    return (int((zi[1:] * zi[:-1] + zq[1:] * zq[:-1]).sum()), int((zq[1:] * zi[:-1] - zi[1:] * zq[:-1]).sum()))


def direction_of(f):
    """(ca, cb) of a sum F by the rule of step 4n: floor shifts until both fit int16."""
    sh = max(0, max(abs(f[0]), abs(f[1])).bit_length() - 15)
    return f[0] >> sh, f[1] >> sh, sh


def own_direction(clip, rng, sl, n_sym, whole_clip=False):
    """(ca, cb, sh) of a job's region; ``whole_clip``: the mutant that sums over the clip instead."""
    t0, t1 = rng[0] - sl, rng[1] + sl * (n_sym - 1) + 1
    f = region_sum(clip, 0, np.asarray(clip).size // 2) if whole_clip else region_sum(clip, t0, t1)
    assert max(abs(f[0]), abs(f[1])) < 2 ** 30
    return direction_of(f)


def decode_job(clip, job, index, sl, n_sym, max_flips, narrow, whole_clip=False):
    """(record row or None, header row, soft [N]) of one job on its clip's bytes (uint8, 2 n)."""
    clip = np.ascontiguousarray(clip, np.uint8).reshape(-1)
    n = int(job["n"])
    assert clip.size == 2 * n
    zero = np.zeros(n_sym, np.int64)
    rng = job_range(n, job["tau_lo"], job["tau_hi"], sl, n_sym)
    if rng is None:
        return None, (0, 0, 0, 0), zero
    cand = rng[1] - rng[0] + 1
    ca, cb = int(job["corr_re"]), int(job["corr_im"])
    if ca == 0 and cb == 0:
        ca, cb, _ = own_direction(clip, rng, sl, n_sym, whole_clip)
        if ca == 0 and cb == 0:
            return None, (0, cand, 0, 0), zero
    assert -32768 <= ca <= 32767 and -32768 <= cb <= 32767
    cfg_n = DC.config(sl, n_sym, n)
    clock = int(job["clock"])
    # (a dict, so that t_lo and t_hi stay unreduced Python integers: the model takes their difference as it is)
    e = {"channel": int(job["channel"]), "id": int(job["id"]), "t_lo": clock + int(job["tau_lo"]), "t_hi": clock + int(job["tau_hi"]),
         "corr_re": ca, "corr_im": cb}
    got = TC.decode_expect(clip, None, e, index, cfg_n, False, clock, max_flips, narrow)
    assert got is not None and got[0] == cand
    if got[1] is None:
        return None, (0, cand, ca, cb), zero
    row = list(got[1])
    assert row[3] & TC.EXPECTED and not row[3] & 1
    row[3] = (row[3] & ~TC.EXPECTED) | REPLAYED
    taus, s, _, _, _, _ = TC.symbol_sums(clip, None, e, cfg_n, False, clock, narrow)
    return tuple(row), (1, cand, ca, cb), s[row[2] - int(taus[0])].astype(np.int64)


class Case:
    """Clips, the pool they lie in and jobs on it for one (SL, N); ``want(R, narrow)`` is the model's Replay: records,
    headers and soft values, row j for job j.  ``clip_of[j]`` names job j's clip."""

    def __init__(self, name, sl, n_sym, clips, jobs, clip_of, pool=None, offsets=None):
        self.name, self.sl, self.n_sym = name, int(sl), int(n_sym)
        self.cfg = DC.config(sl, n_sym, 2048)                # (block_size takes no part)
        self.clips = [np.ascontiguousarray(c, np.uint8).reshape(-1) for c in clips]
        if pool is None:
            pool, offsets = build_pool(self.clips)
        self.pool, self.offsets = pool, list(offsets)
        self.jobs = jobs_of(jobs(self.offsets) if callable(jobs) else jobs)
        self.clip_of = list(clip_of)
        assert len(self.clip_of) == self.jobs.size
        for j, k in zip(self.jobs, self.clip_of):
            assert int(j["offset"]) == self.offsets[k] and 2 * int(j["n"]) == self.clips[k].size and int(j["offset"]) % 8 == 0
        self._want, self._memo = {}, {}

    def forms(self):
        return forms_for(self.sl)

    def _one(self, j, r, narrow):
        job, k = self.jobs[j], self.clip_of[j]
        key = (k, r, narrow) + tuple(int(job[f]) for f in CLIP_JOB_DTYPE.names if f != "offset")
        if key not in self._memo:
            self._memo[key] = decode_job(self.clips[k], job, 0, self.sl, self.n_sym, r, narrow)
        return self._memo[key]

    def want(self, r=0, narrow=False):
        if (r, narrow) not in self._want:
            recs = np.zeros(self.jobs.size, BURST_MSG_DTYPE)
            hdr = np.zeros(self.jobs.size, CD_HEADER_DTYPE)
            soft = np.zeros((self.jobs.size, self.n_sym), np.int64)
            for j in range(self.jobs.size):
                row, h, s = self._one(j, r, narrow)
                hdr[j], soft[j] = h, s
                if row is not None:
                    recs[j] = row
                    recs[j]["first"] = j
            self._want[r, narrow] = (recs, hdr, soft)
        return self._want[r, narrow]

    def rec(self, j, r=0, narrow=False):
        recs, hdr, _ = self.want(r, narrow)
        return recs[j] if int(hdr[j]["n_msgs"]) else None


def build_pool(clips, order=None, fill=0x00):
    """(pool, offsets): the clips in ``order`` (indices; default as given), each at the next multiple of 8 outputs, the slack
    bytes between them - and behind the last, up to a multiple of 8 outputs - set to ``fill``.  offsets[k] is clip k's."""
    order = list(range(len(clips))) if order is None else list(order)
    offsets, at = [0] * len(clips), 0
    for k in order:
        offsets[k] = at
        at = (at + clips[k].size // 2 + 7) // 8 * 8
    pool = np.full(2 * at, fill, np.uint8)
    for k in order:
        pool[2 * offsets[k]: 2 * offsets[k] + clips[k].size] = clips[k]
    return pool, offsets


def _quiet(seed, n):
    return BC.quiet_bytes(np.random.default_rng(seed), n)


def _data(r, n_sym):
    return bytes(r["data"][: n_sym // 8])


def burst_clip(data, sl, n, at, seed, **kw):
    """A clip of n outputs of quiet bytes with fsk_burst(data) whose first output is ``at``."""
    return DC.put(_quiet(seed, n), at, DC.fsk_burst(data, sl, **kw))


# ------------------------------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def edges_case():
    """SL 14, N 80.  Clip 0: exactly N SL + 1 outputs - one candidate, tau = SL.  Clips 1 .. 3: the first symbol ends at
    tau = SL, n % 8 = 0, 1, 7; clips 4 .. 6: the last symbol ends at n - 1, n % 8 = 0, 1, 7 - the narrow form sits on the
    zero extension at that edge.  Jobs 7, 8: ranges wholly outside clip 1 (before SL, past the end): idle.  Clip 7 with
    job 9: the widest range, tau_hi - tau_lo = 2048."""
    sl, n_sym = 14, 80
    body = sl * (n_sym - 1)
    datas = [DC.packet(n_sym, ident=k % 8, seed=3000 + k) for k in range(8)]
    clips = [DC.fsk_burst(datas[0], sl, lead=1, trail=0)]
    clips += [DC.fsk_burst(datas[1 + i], sl, lead=1, trail=t) for i, t in enumerate((31, 32, 38))]
    clips += [DC.fsk_burst(datas[4 + i], sl, lead=ld, trail=0) for i, ld in enumerate((64, 65, 71))]
    clips.append(burst_clip(datas[7], sl, 3301, 1500, 3007))
    ns = [c.size // 2 for c in clips]
    assert ns[0] == n_sym * sl + 1 and [n % 8 for n in ns[1:7]] == [0, 1, 7, 0, 1, 7]

    def jobs(off):
        rows = [job_row(off[k], ns[k], -100, 1900, channel=k, clock=1000 * k) for k in range(7)]
        rows += [job_row(off[1], ns[1], -50, sl - 1), job_row(off[1], ns[1], ns[1] - body, ns[1] + 500)]
        rows.append(job_row(off[7], ns[7], sl, sl + MAX_SPAN, channel=7, clock=2 ** 64 - 1000))
        return rows
    X = Case("edges", sl, n_sym, clips, jobs, list(range(7)) + [1, 1, 7])
    _, hdr, _ = X.want()
    assert list(hdr["candidates"][:1]) == [1] and int(X.rec(0)["tau"]) == sl and _data(X.rec(0), n_sym) == datas[0]
    for k in (1, 2, 3):
        assert int(X.rec(k)["tau"]) == sl and _data(X.rec(k), n_sym) == datas[k]
    for k in (4, 5, 6):
        assert int(X.rec(k)["tau"]) == ns[k] - 1 - body == int(hdr[k]["candidates"]) + sl - 1 and _data(X.rec(k), n_sym) == datas[k]
    for j in (7, 8):
        assert hdr[j].tobytes() == bytes(16) and X.rec(j) is None
    assert int(hdr[9]["candidates"]) == MAX_SPAN + 1 and _data(X.rec(9), n_sym) == datas[7]
    assert int(X.rec(9)["time"]) == (2 ** 64 - 1000 + int(X.rec(9)["tau"])) % 2 ** 64 < 3000     # the clock wraps inside the clip
    for r, nb in FORMS:                                      # the wrapper's flags: REPLAYED, never bit 0 or bit 3
        recs, hdr, _ = X.want(r, nb)
        live = recs[hdr["n_msgs"] == 1]
        assert np.all(live["flags"] & REPLAYED) and not np.any(live["flags"] & 9) and np.all((live["flags"] & 4 != 0) == nb)
    return X


ISO_ORDERS = ((0, 1, 2, 3, 4, 5, 6, 7), (5, 2, 7, 0, 3, 6, 1, 4))


@functools.lru_cache(maxsize=None)
def isolation_case():
    """SL 8, N 40: eight clips with every n % 8, and their jobs - own direction, and for clips 0 and 1 a given one too.  Clip 0
    ends with its packet's last symbol (n % 8 = 1: seven outputs of slack) and is followed directly, in the first order,
    by clip 1, which begins with a stronger copy of the same packet.  Returns (clips, per-order (pool, offsets, Case))."""
    sl, n_sym = 8, 40
    datas = [DC.packet(n_sym, ident=k % 8, seed=3100 + k) for k in range(8)]
    datas[1] = datas[0]
    clips = [DC.fsk_burst(datas[0], sl, lead=64 + 1, trail=0, amp=30),
             DC.fsk_burst(datas[1], sl, lead=1, trail=66, amp=90)]
    clips += [burst_clip(datas[k], sl, n, 60 + 3 * k, 3100 + k, carrier=(0.11, -0.2, 0.31)[k % 3])
              for k, n in zip(range(2, 8), (504, 514, 524, 533, 542, 551))]
    ns = [c.size // 2 for c in clips]
    assert ns[0] % 8 == 1 and sorted(n % 8 for n in ns) == list(range(8))
    clip_of = list(range(8)) + [0, 1]

    def jobs(off):
        rows = [job_row(off[k], ns[k], 0, 1000, channel=k, clock=77 * k) for k in range(8)]
        rows += [job_row(off[k], ns[k], 0, 1000, TC.corr_of(CARRIER), channel=k) for k in (0, 1)]
        return rows
    out = []
    for order, fill in zip(ISO_ORDERS, (0x00, 0xA5)):
        pool, off = build_pool(clips, order, fill)
        out.append(Case(f"isolation_{fill:02x}", sl, n_sym, clips, jobs, clip_of, pool, off))
    A, B = out
    assert A.offsets[1] == A.offsets[0] + ns[0] + 7 and np.all(A.pool[2 * (A.offsets[0] + ns[0]): 2 * A.offsets[1]] == 0x00)
    assert np.all(B.pool[2 * (B.offsets[0] + ns[0]): 2 * (B.offsets[0] + ns[0] + 7)] == 0xA5)
    for X in out:
        for k in range(8):
            assert X.rec(k) is not None and _data(X.rec(k), n_sym) == datas[k], k
    m0, m1 = A.rec(0), A.rec(1)
    assert int(m0["tau"]) == ns[0] - 1 - sl * (n_sym - 1) and int(m1["tau"]) == sl and int(m1["margin"]) > 4 * int(m0["margin"])
    return clips, out


def zero_sum_clip(sl, n_sym, n, tau):
    """A clip whose outputs turn by +90 and -90 degrees in alternation from tau - SL on - the region of the one candidate tau
    then sums to exactly (0, 0) - and by +90 degrees at every output in front of it."""
    c = 41
    z = complex(c, c)
    turn = [1j if t < tau - sl or (t - (tau - sl)) % 2 == 1 else -1j for t in range(n)]
    out = np.empty(2 * n, np.uint8)
    for t in range(n):
        z = z * turn[t] if t else z
        out[2 * t], out[2 * t + 1] = (255 + int(z.real)) // 2, (255 + int(z.imag)) // 2
    return out


@functools.lru_cache(maxsize=None)
def own_direction_case():
    """SL 14, N 80.  Clips 0, 1: bursts at +0.11 and -0.2 cycles per output under corr = (0, 0) (jobs 0, 1: sh > 0).  Clip 2,
    job 2: the region of its one candidate sums to exactly (0, 0) - candidates 1, no record, ca = cb = 0 - while the clip as
    a whole does not.  Clip 3, job 3: quiet bytes, |F| < 2^15: sh = 0.  Job 4: clip 0 with its direction given."""
    sl, n_sym = 14, 80
    datas = [DC.packet(n_sym, ident=2 + k, seed=3200 + k) for k in range(2)]
    clips = [burst_clip(datas[0], sl, 1400, 100, 3200, carrier=0.11), burst_clip(datas[1], sl, 1403, 90, 3201, carrier=-0.2),
             zero_sum_clip(sl, n_sym, 1500, 200), _quiet(3203, 1300)]
    ns = [c.size // 2 for c in clips]

    def jobs(off):
        return [job_row(off[0], ns[0], 0, 400), job_row(off[1], ns[1], 0, 400, channel=1), job_row(off[2], ns[2], 200, 200),
                job_row(off[3], ns[3], 20, 120), job_row(off[0], ns[0], 0, 400, TC.corr_of(0.11))]
    X = Case("own_direction", sl, n_sym, clips, jobs, [0, 1, 2, 3, 0])
    _, hdr, _ = X.want()
    for j, f in ((0, 0.11), (1, -0.2)):
        rng = job_range(ns[j], 0, 400, sl, n_sym)
        ca, cb, sh = own_direction(clips[j], rng, sl, n_sym)
        assert sh > 0 and (int(hdr[j]["ca"]), int(hdr[j]["cb"])) == (ca, cb) and _data(X.rec(j), n_sym) == datas[j]
        assert abs(np.angle(complex(ca, cb) * np.exp(-2j * np.pi * f))) < 0.2
    assert region_sum(clips[2], 200 - sl, 200 + sl * (n_sym - 1) + 1) == (0, 0) and region_sum(clips[2], 0, ns[2]) != (0, 0)
    for r, nb in FORMS:
        assert X.want(r, nb)[1][2].tobytes() == np.asarray([(0, 1, 0, 0)], CD_HEADER_DTYPE).tobytes() and X.rec(2, r, nb) is None
    rng = job_range(ns[3], 20, 120, sl, n_sym)
    ca, cb, sh = own_direction(clips[3], rng, sl, n_sym)
    assert sh == 0 and (ca, cb) != (0, 0) and (int(hdr[3]["ca"]), int(hdr[3]["cb"])) == (ca, cb) and int(hdr[3]["candidates"]) == 101
    assert _data(X.rec(4), n_sym) == datas[0] and (int(hdr[4]["ca"]), int(hdr[4]["cb"])) == TC.corr_of(0.11)
    return X


@functools.lru_cache(maxsize=None)
def repair_case():
    """SL 8, N 80, burst_repair_cases' builders.  Clips 0, 1: one weak wrong symbol (k = 16, N - 1); clips 2, 3: two ((16, N - 1),
    (40, 41)) - nothing at R = 0 (and 1), the planted data from R = 1 (2) on.  Clip 4: a damaged copy and, later and at half
    the amplitude, an exact copy of the same packet: job 4 over both gives the exact one at every R, job 5 over the first
    alone the repaired one from R = 1.  Clip 5: packets of ids 3 and 5, the second louder: jobs 6, 7, 8 for id 3, 5 and any."""
    sl, n_sym = 8, 80
    c = TC.corr_of(CARRIER)
    one = RP.find_packet(n_sym, lambda b: all(RP.lonely(b, k) for k in (16, n_sym - 1)), 1100)
    two = RP.find_packet(n_sym, lambda b: RP.lonely(b, 16) and RP.lonely(b, n_sym - 1) and RP.lonely_pair(b, 40), 1200)
    scales = ({16: RP.WEAK}, {n_sym - 1: RP.WEAK}, {16: RP.WEAK, n_sym - 1: RP.WEAK}, {40: RP.WEAK, 41: RP.WEAK})
    clips = [DC.put(_quiet(3300 + i, 901 + i), 100 + i, RP.damaged(one if i < 2 else two, sl, sc)) for i, sc in enumerate(scales)]
    both = DC.put(_quiet(3304, 1900), 50, RP.damaged(one, sl, {16: RP.WEAK}))
    clips.append(DC.put(both, 1000, RP.damaged(one, sl, {}, amp=20)))
    ids = [DC.packet(n_sym, ident=i, seed=3310 + i) for i in (3, 5)]
    pair = DC.put(_quiet(3305, 1900), 40, DC.fsk_burst(ids[0], sl, amp=30))
    clips.append(DC.put(pair, 1000, DC.fsk_burst(ids[1], sl, amp=60)))
    ns = [x.size // 2 for x in clips]

    def jobs(off):
        rows = [job_row(off[k], ns[k], 100, 300, c, channel=k) for k in range(4)]
        rows += [job_row(off[4], ns[4], 0, 1300, c), job_row(off[4], ns[4], 0, 400, c)]
        rows += [job_row(off[5], ns[5], 0, 1300, c, ident=i) for i in (3, 5, ANY_ID)]
        return rows
    X = Case("repair_and_id", sl, n_sym, clips, jobs, [0, 1, 2, 3, 4, 4, 5, 5, 5])
    for j, (need, data) in enumerate(((1, one), (1, one), (2, two), (2, two))):
        for r in range(3):
            m = X.rec(j, r)
            assert (m is not None) == (r >= need), (j, r)
            if m is not None:
                ks = sorted(scales[j])
                assert _data(m, n_sym) == data and int(m["flags"]) == REPLAYED | RP.REPAIRED
                assert tuple(int(v) for v in m["pad"][:3]) == (len(ks), ks[0], ks[1] if len(ks) == 2 else 0)
    exact = [X.rec(4, r) for r in range(3)]
    assert all(m is not None and int(m["pad"][0]) == 0 and int(m["tau"]) > 1000 and _data(m, n_sym) == one for m in exact)
    assert exact[0].tobytes() == exact[1].tobytes() == exact[2].tobytes()
    assert X.rec(5, 0) is None and int(X.rec(5, 1)["pad"][0]) == 1 and int(X.rec(5, 1)["tau"]) < 400
    assert int(X.rec(5, 1)["margin"]) > int(exact[0]["margin"])          # the repaired copy is the louder one, and still loses
    assert [int(X.rec(j)["id"]) for j in (6, 7, 8)] == [3, 5, 5] and int(X.rec(6)["tau"]) < 400 < int(X.rec(7)["tau"])
    return X


SHAPES = ((4, 40), (51, 40), (3, 40))


@functools.lru_cache(maxsize=None)
def shape_case(sl, n_sym):
    """One burst at -0.07 cycles per output in a clip with n % 8 = 5, under its own direction and a given one, and a range
    that misses the packet."""
    data = DC.packet(n_sym, ident=6, seed=3400 + sl)
    n = n_sym * sl + 1 + 8 * 40 + 5 - (n_sym * sl + 1) % 8
    clip = burst_clip(data, sl, n, 37, 3400 + sl, carrier=-0.07, lead=48, trail=24)
    T = 37 + 48 + sl - 1

    def jobs(off):
        return [job_row(off[0], n, 0, 400), job_row(off[0], n, T - 20, T + 20, TC.corr_of(-0.07)),
                job_row(off[0], n, T + 2 * sl, T + 2 * sl + 30, TC.corr_of(-0.07))]
    X = Case(f"shape_sl{sl}_n{n_sym}", sl, n_sym, [clip], jobs, [0, 0, 0])
    assert n % 8 == 5
    for r, nb in X.forms():
        assert all(X.rec(j, r, nb) is not None and _data(X.rec(j, r, nb), n_sym) == data for j in (0, 1)), (sl, r, nb)
    assert X.rec(2) is None and int(X.want()[1][2]["candidates"]) == 31
    return X


@functools.lru_cache(maxsize=None)
def many_jobs_case(n_jobs=600):
    """SL 8, N 40: 600 jobs drawn from 12 clips (eight with a packet at one of three carriers, four of quiet bytes, every
    n % 8 among them) and 48 templates that differ in range, id and direction, idle ones among them - more workgroups
    than the chip has compute units."""
    sl, n_sym = 8, 40
    carriers = (0.11, -0.2, 0.31)
    datas = [DC.packet(n_sym, ident=k % 8, seed=3500 + k) for k in range(8)]
    clips = [burst_clip(datas[k], sl, 600 + 9 * k, 80 + 11 * k, 3500 + k, carrier=carriers[k % 3]) for k in range(8)]
    clips += [_quiet(3510 + k, 400 + 3 * k) for k in range(4)]
    ns = [c.size // 2 for c in clips]
    rng = np.random.default_rng(3500)
    templates = []
    for t in range(48):
        k = t % 12
        kind = t // 12
        lo = int(rng.integers(-40, 120))
        corr = (0, 0) if kind % 2 == 0 else TC.corr_of(carriers[k % 3])
        ident = ANY_ID if kind < 2 else (k % 8 if kind == 2 else (k + 1) % 8)
        hi = lo + int(rng.integers(0, 400))
        if t % 8 == 7:
            lo, hi = ns[k] + 5, ns[k] + 50                   # idle
        templates.append((k, lo, hi, corr, ident))
    pick = rng.integers(0, len(templates), n_jobs)
    pick[: len(templates)] = np.arange(len(templates))       # each at least once

    def jobs(off):
        return [job_row(off[templates[p][0]], ns[templates[p][0]], templates[p][1], templates[p][2], templates[p][3], templates[p][4],
                        channel=int(p), clock=1000 * i) for i, p in enumerate(pick)]
    X = Case("many_jobs", sl, n_sym, clips, jobs, [templates[p][0] for p in pick])
    return X, templates, pick


def check_many_jobs(X):
    _, hdr, _ = X.want()
    assert X.jobs.size == 600 and np.count_nonzero(hdr["candidates"] == 0) >= 50 and np.count_nonzero(hdr["n_msgs"]) >= 100
    assert np.count_nonzero((hdr["candidates"] > 0) & (hdr["n_msgs"] == 0)) >= 50


# ------------------------------------------------------------------------------------------ the argument rule, restated
def check_jobs(jobs, pool_outputs):
    """rd_cd_check_jobs in Python: (0, -1), or (-1, the first offending job; -1 for the count itself)."""
    jobs = np.asarray(jobs, CLIP_JOB_DTYPE).reshape(-1)
    if not 1 <= jobs.size <= 2 ** 20:
        return -1, -1
    for i, j in enumerate(jobs):
        off, n, lo, hi = int(j["offset"]), int(j["n"]), int(j["tau_lo"]), int(j["tau_hi"])
        bad = (off % 8 != 0 or n < 1 or off + n > pool_outputs or lo > hi or hi - lo > MAX_SPAN or abs(lo) > 2 ** 30 or abs(hi) > 2 ** 30
               or not (int(j["id"]) < 8 or int(j["id"]) == ANY_ID) or not -32768 <= int(j["corr_re"]) <= 32767
               or not -32768 <= int(j["corr_im"]) <= 32767 or int(j["pad"]) != 0)
        if bad:
            return -1, i
    return 0, -1


def assert_replay_equals(got, want, what=""):
    """A Replay against the model's (records, headers, soft): every field of every row."""
    recs, hdr, soft = want
    assert got.records.dtype == BURST_MSG_DTYPE and got.headers.dtype == CD_HEADER_DTYPE
    for f in CD_HEADER_DTYPE.names:
        assert np.array_equal(got.headers[f], hdr[f]), (what, f, np.flatnonzero(got.headers[f] != hdr[f])[:8])
    for f in BURST_MSG_DTYPE.names:
        assert np.array_equal(got.records[f], recs[f]), (what, f, got.records[f], recs[f])
    if got.soft is not None:
        assert got.soft.dtype == np.int64 and np.array_equal(got.soft, soft), (what, "soft", np.argwhere(got.soft != soft)[:8])
