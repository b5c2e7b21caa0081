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
