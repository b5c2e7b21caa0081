"""Helpers shared by tests/test_wideband_bursts_cpu.py and tests/test_wideband_bursts.py (no tests in here): the model
of k_chan_bursts in NumPy int64, written from the definition (include/rtldavis_hip.h, BURSTS) and not from the kernel's
byte arithmetic; the acquisition captures - retune_cases.loop_capture's recipe with the planted offset as a parameter -
and the order in which the closed-loop tests feed them.  Nothing here touches a device."""
import functools
from types import SimpleNamespace

import numpy as np

import retune_cases as RC
from rtldavis_amd import acquire
from rtldavis_amd import channelizer as CZ
from rtldavis_amd import synth
from rtldavis_amd.wideband import BURST_DTYPE, BURST_FLOOR_DTYPE, BURST_THRESHOLD_OFF, Bursts

W = 128
PLANTED = (20000, -20000, 38000)     # Hz off the channel's centre: far outside the +-4.8 kHz the demodulator reaches
ESTIMATE_TOL_HZ = 1500               # the issue's bound on |estimate - planted|


def window_sums(block):
    """(p, re r, im r) per channel and window, int64 [n_channels, nW], of channelized bytes uint8 [n_channels, 2 B]."""
    b = np.atleast_2d(np.asarray(block, np.uint8)).astype(np.int64)
    n_ch, n2 = b.shape
    assert n2 % (2 * W) == 0 and n2 > 0
    ai = (2 * b[:, 0::2] - 255).reshape(n_ch, -1, W)
    aq = (2 * b[:, 1::2] - 255).reshape(n_ch, -1, W)
    p = (ai * ai + aq * aq).sum(axis=2)
    # z[t] conj(z[t-1]) over the 127 pairs inside a window
    re = (ai[:, :, 1:] * ai[:, :, :-1] + aq[:, :, 1:] * aq[:, :, :-1]).sum(axis=2)
    im = (aq[:, :, 1:] * ai[:, :, :-1] - ai[:, :, 1:] * aq[:, :, :-1]).sum(axis=2)
    return p, re, im


def burst_model(block, thr, chunk=0):
    """(records, floor) of one channelized chunk under the thresholds ``thr`` (one integer or one per channel):
    structured arrays of BURST_DTYPE / BURST_FLOOR_DTYPE, from the definition, in Python integers."""
    p, re, im = window_sums(block)
    n_ch, n_win = p.shape
    thr = np.broadcast_to(np.asarray(thr, np.uint64), (n_ch,))
    recs, floor = [], np.zeros(n_ch, BURST_FLOOR_DTYPE)
    for c in range(n_ch):
        on = [int(p[c, w]) >= int(thr[c]) for w in range(n_win)]
        runs, w = [], 0
        while w < n_win:
            if not on[w]:
                w += 1
                continue
            e = w
            while e + 1 < n_win and on[e + 1]:
                e += 1
            runs.append((w, e))
            w = e + 1
        for a, e in runs:
            sl = slice(a, e + 1)
            recs.append((c, a, e - a + 1, (1 if a == 0 else 0) | (2 if e == n_win - 1 else 0), int(p[c, sl].sum()),
                         int(p[c, sl].max()), 0, int(re[c, sl].sum()), int(im[c, sl].sum())))
        off = np.asarray([not o for o in on])
        floor[c] = (int(thr[c]), int(off.sum()), len(runs), chunk, int(p[c, off].sum()), int(re[c, off].sum()),
                    int(im[c, off].sum()))
    return np.asarray(recs, BURST_DTYPE).reshape(-1), floor


def model_bursts(block, thr, chunk=0):
    """burst_model as the ``Bursts`` a receiver returns."""
    recs, floor = burst_model(block, thr, chunk)
    return Bursts(recs, floor, chunk)


def median_thresholds(block):
    """Per channel, the median of its window energies (the upper one of an even count): about half the windows ON."""
    p = window_sums(block)[0]
    return np.sort(p, axis=1)[:, p.shape[1] // 2].astype(np.uint64)


def assert_equals_model(got, block, thr, chunk):
    """A receiver's Bursts against the model of the same bytes: every field of every record and floor row."""
    recs, floor = burst_model(block, thr, chunk)
    assert got.chunk == chunk
    assert got.floor.dtype == BURST_FLOOR_DTYPE and got.records.dtype == BURST_DTYPE
    for f in BURST_FLOOR_DTYPE.names:
        assert np.array_equal(got.floor[f], floor[f]), (chunk, f, got.floor[f], floor[f])
    assert got.records.shape == recs.shape, (chunk, got.records.shape, recs.shape)
    for f in BURST_DTYPE.names:
        assert np.array_equal(got.records[f], recs[f]), (chunk, f)


# ------------------------------------------------------------------------------------------ crafted bytes
# Inputs for k_chan_bursts alone (the hook rd_debug_bursts): exact bytes, exact thresholds.  Every case names the edge it
# is built for as a condition on the model of its own bytes, asserted when the case is built - an input that misses its
# edge fails instead of passing quietly.
FILL = 0xA5                                                  # what the hook leaves in a place the kernel did not write
P_MAX = 256 * 65025                                          # p_w of saturated bytes (the kernel's header comment)
R_MAX = 254 * 65025                                          # |re r_w| or |im r_w| at most
GAP = 16                                                     # bytes between channels in the cases with a wider stride


def cap_of(n_win):
    return (n_win + 1) // 2


def quiet_bytes(rng, n_out):
    """Noise near 127: bytes 126 .. 129 (a = -3 .. 3), p_w <= 128 x 18."""
    return rng.integers(126, 130, 2 * n_out).astype(np.uint8)


def saturated(kind, n_out):
    """2 n_out bytes of 0 and 255 only: "zeros", "ones" (all 255), "flip" (outputs (255, 255), (0, 0) alternating: every
    pair gives -2 x 65025), "rot+" / "rot-" (z turns by +-90 degrees per output: every pair gives +-2 x 65025 j)."""
    t = np.arange(n_out)
    if kind == "zeros":
        i = q = np.zeros(n_out, np.int64)
    elif kind == "ones":
        i = q = np.full(n_out, 255)
    elif kind == "flip":
        i = q = 255 * (1 - t % 2)
    else:
        quad = t % 4 if kind == "rot+" else (-t) % 4         # (a, a), (-a, a), (-a, -a), (a, -a)
        i, q = 255 * np.isin(quad, (0, 3)), 255 * np.isin(quad, (0, 1))
    out = np.empty(2 * n_out, np.uint8)
    out[0::2], out[1::2] = i, q
    return out


def crafted(name, rows, thr, seq=3, gap=0, check=None):
    """One launch: ``rows`` (one uint8 [2 n_out] per channel) laid out with ``gap`` bytes of 255 behind every channel."""
    rows = np.stack([np.asarray(r, np.uint8) for r in rows])
    n_ch, n2 = rows.shape
    chan = np.full((n_ch, n2 + gap), 255, np.uint8)
    chan[:, :n2] = rows
    thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thr, np.uint64), (n_ch,)).astype(np.uint32))
    cs = SimpleNamespace(name=name, rows=rows, chan=chan, stride=n2 + gap, n_ch=n_ch, n_out=n2 // 2, n_win=n2 // (2 * W),
                         thr=thr, seq=seq)
    cs.records, cs.floor = burst_model(rows, thr, seq & 0xFFFFFFFF)
    if check is not None:
        check(cs)
    return cs


def slot_model(cs):
    """The whole slot the hook hands back: [n_ch][cap] record places - the channel's runs first, FILL behind them - and
    the floor rows."""
    cap = cap_of(cs.n_win)
    recs = np.frombuffer(bytes([FILL]) * (cs.n_ch * cap * BURST_DTYPE.itemsize), BURST_DTYPE).reshape(cs.n_ch, cap).copy()
    for c in range(cs.n_ch):
        mine = cs.records[cs.records["channel"] == c]
        assert mine.size == cs.floor["n_bursts"][c] <= cap
        recs[c, : mine.size] = mine
    return recs, cs.floor


def _groups_between(rec):
    """Whole groups of 64 windows inside the run that are neither its first nor its last."""
    a, e = int(rec["first"]), int(rec["first"]) + int(rec["windows"]) - 1
    return [g for g in range(a // 64 + 1, e // 64) if 64 * g >= a and 64 * g + 63 <= e]


@functools.lru_cache(maxsize=None)
def crafted_small():
    """Every crafted case but the largest chunk (which the GPU test alone launches; crafted_largest)."""
    rng = np.random.default_rng(20260)
    uni = lambda n_out: rng.integers(0, 256, 2 * n_out).astype(np.uint8)
    out = []
    # window counts around the 16 windows of a pass, the 64 of a group and the carried run: uniform bytes, median thresholds
    for n_win in (1, 15, 16, 17, 63, 64, 65, 129, 192, 193):
        rows = [uni(W * n_win) for _ in range(3)]
        out.append(crafted(f"uniform_w{n_win}", rows, median_thresholds(np.stack(rows)), seq=n_win,
                           gap=GAP if n_win in (17, 65, 193) else 0))
    # designed runs: a carried run is carried again (c_win, c_pow, c_re, c_im accumulate)
    def long_check(cs):
        for c in range(cs.n_ch):
            mine = cs.records[cs.records["channel"] == c]
            assert mine.size == 1 and _groups_between(mine[0]), (cs.name, c, mine)
    for n_win in (193, 256):
        rows = []
        for a, e in ((10, 140), (0, 192), (63, 128)):
            r = quiet_bytes(rng, W * n_win)
            r[2 * W * a: 2 * W * (e + 1)] = uni(W * (e + 1 - a))
            rows.append(r)
        cs = crafted(f"long_runs_w{n_win}", rows, 100000, gap=GAP if n_win == 193 else 0, check=long_check)
        assert [(int(r["first"]), int(r["windows"])) for r in cs.records] == [(10, 131), (0, 193), (63, 66)]
        out.append(cs)
    # alternating ON / OFF: every record place of the channel that starts ON is filled
    def alt_check(cs):
        assert cs.floor["n_bursts"][0] == cap_of(cs.n_win) and cs.floor["n_bursts"][1] == cs.n_win // 2
        assert np.all(cs.records["windows"] == 1)
    for n_win in (64, 65, 129):
        rows = []
        for start_on in (1, 0):
            r = quiet_bytes(rng, W * n_win).reshape(n_win, 2 * W)
            on = (np.arange(n_win) % 2) != start_on
            r[on] = rng.integers(0, 256, (int(on.sum()), 2 * W))
            rows.append(r.reshape(-1))
        out.append(crafted(f"alternating_w{n_win}", rows, 100000, check=alt_check))
    # saturated bytes: the int32 / uint32 bounds of the kernel's header comment, per window and per lane
    def sat_check(want):
        def check(cs):
            p, re, im = window_sums(cs.rows)
            assert np.all(p == P_MAX), cs.name
            for c, (wr, wi) in enumerate(want):
                assert np.all(re[c] == wr * R_MAX) and np.all(im[c] == wi * R_MAX), (cs.name, c)
                assert cs.records[c]["windows"] == cs.n_win and cs.records[c]["flags"] == 3
        return check
    out.append(crafted("saturated_re", [saturated(k, 64 * W) for k in ("zeros", "ones", "flip")], 0,
                       check=sat_check([(1, 0), (1, 0), (-1, 0)])))
    out.append(crafted("saturated_im", [saturated(k, 64 * W) for k in ("rot+", "rot-")], 0, gap=GAP,
                       check=sat_check([(0, 1), (0, -1)])))
    # the threshold at exactly p_w (the >=), one above it, 0 and 2^32 - 1, on the same bytes
    def thr_check(cs):
        on = [set(w for r in cs.records[cs.records["channel"] == c] for w in range(int(r["first"]), int(r["first"]) + int(r["windows"])))
              for c in range(cs.n_ch)]
        assert 5 in on[0] and 5 not in on[1] and on[0] - on[1] == {5}
        assert on[2] == set(range(cs.n_win)) and on[3] == set() and cs.floor["windows_off"][3] == cs.n_win
    row = uni(17 * W)
    p5 = int(window_sums(row)[0][0, 5])
    out.append(crafted("threshold_at_p_w", [row] * 4, [p5, p5 + 1, 0, 2 ** 32 - 1], check=thr_check))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def crafted_largest():
    """nW = 4096, the most rd_bursts_check admits: all of the kernel's LDS, one run of 4096 windows per channel, 64-bit
    sums of 4096 saturated windows."""
    def check(cs):
        assert cs.records.size == 3 and np.all(cs.records["windows"] == 4096) and np.all(cs.records["flags"] == 3)
        assert [int(x) for x in cs.records["power"]] == [68183654400] * 3 == [4096 * P_MAX] * 3
        assert [int(x) for x in cs.records["corr_re"]] == [67650969600, -67650969600, 0]
        assert [int(x) for x in cs.records["corr_im"]] == [0, 0, 4096 * R_MAX]
    return crafted("largest_w4096", [saturated(k, 4096 * W) for k in ("ones", "flip", "rot+")], 0, seq=2 ** 32 + 9, check=check)


BAD_N_OUT = (0, 127, 129, 4097 * W)                          # what rd_bursts_check refuses


# ------------------------------------------------------------------------------------------ acquisition
@functools.lru_cache(maxsize=None)
def acq_capture(planted):
    """retune_cases.loop_capture with both bursts ``planted`` Hz off the channel's centre instead of LOOP_CFO."""
    f = CZ.US_CHANNELS_HZ[RC.LOOP_CHANNEL] - RC.CENTRE
    payload = synth.payload_of(RC.LOOP_SEEDS[0])
    raw, info = synth.synth_wideband(RC.LOOP_SEEDS, [f + planted, f + planted], RC.LOOP_NK * RC.LOOP_B, payloads=[payload, payload])
    plan = SimpleNamespace()
    CZ.plan_channels(plan, [CZ.US_CHANNELS_HZ[RC.LOOP_CHANNEL]], RC.CENTRE, CZ.DEFAULT_DECIM, None, 3.0, CZ.OUT_RATE)
    return SimpleNamespace(raw=raw, info=info, payload=payload, plan=plan, chans=[CZ.US_CHANNELS_HZ[RC.LOOP_CHANNEL]],
                           step=2 * RC.LOOP_B * CZ.DEFAULT_DECIM, planted=planted)


def new_acquisition(need=1):
    return acquire.Acquisition(1, RC.packet_config(RC.LOOP_B), need=need)


def run_loop(n_chunks, submit, fetch, acq, retune):
    """The order of the closed-loop tests, two chunks in flight: chunk k - 2 is fetched and handed to ``acq`` before
    chunk k is submitted.  ``fetch()`` returns (Bursts, parsed rows) of the oldest chunk in flight; a proposal goes to
    ``retune(offset)`` at once.  Returns [(chunks submitted when proposed, offset)]."""
    asked, submitted = [], 0

    def take():
        b, rows = fetch()
        new = acq.update(b, rows, submitted)
        if new is not None:
            retune(new)
            asked.append((submitted, new))

    for k in range(n_chunks):
        if k >= 2:
            take()
        submit(k)
        submitted += 1
    take()
    take()
    return asked
