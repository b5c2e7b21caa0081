"""k_clip_decode / rd_clips_* on the device (include/rtldavis_hip.h, CLIP DECODE) against the model of
tests/clip_replay_cases.py - burst_track_cases.decode_expect with the clip as a chunk of its own -: every field of every
record, every header and every soft value, under every form the symbol length admits.  The cases assert their own edges on
the model when they are built; here the device has to equal the model."""
import ctypes as C

import numpy as np
import pytest

import burst_decode_cases as DC
import clip_replay_cases as RC
from rtldavis_amd import _lib, acquire, clips, replay
from rtldavis_amd.replay import CD_HEADER_DTYPE, CLIP_JOB_DTYPE, ClipDecoder
from rtldavis_amd.wideband import BURST_MSG_DTYPE

pytestmark = pytest.mark.gpu


def _decoder(X):
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    dec = ClipDecoder(X.cfg)
    dec.upload(X.pool)
    return dec


def _assert_case(X, dec=None):
    """Every form on one upload; returns the device's Replays by form."""
    dec = _decoder(X) if dec is None else dec
    out = {}
    for r, nb in X.forms():
        got = dec.decode_jobs(X.jobs, r, nb, soft=True)
        RC.assert_replay_equals(got, X.want(r, nb), (X.name, r, nb))
        out[r, nb] = got
    return out


def test_edges():
    X = RC.edges_case()
    got = _assert_case(X)
    for g in got.values():                                        # an idle job's places read 0
        for j in (7, 8):
            assert g.records[j].tobytes() == bytes(BURST_MSG_DTYPE.itemsize) and g.headers[j].tobytes() == bytes(16) and not g.soft[j].any()
    assert np.all(acquire.replayed(got[0, False].records[got[0, False].headers["n_msgs"] == 1]))


def test_isolation():
    _, (A, B) = RC.isolation_case()
    ga, gb = _assert_case(A), _assert_case(B)
    assert A.pool.tobytes() != B.pool.tobytes() and A.offsets != B.offsets
    for form in A.forms():                                        # job for job, whatever the order and the slack hold
        for f in BURST_MSG_DTYPE.names:
            assert np.array_equal(ga[form].records[f], gb[form].records[f]), (form, f)
        assert ga[form].headers.tobytes() == gb[form].headers.tobytes() and np.array_equal(ga[form].soft, gb[form].soft)


def test_own_direction():
    X = RC.own_direction_case()
    got = _assert_case(X)
    for g in got.values():
        assert tuple(g.headers[2]) == (0, 1, 0, 0) and not g.records[2].tobytes().strip(b"\0")
        assert (int(g.headers[0]["ca"]), int(g.headers[0]["cb"])) == (int(X.want()[1][0]["ca"]), int(X.want()[1][0]["cb"]))


def test_repair_and_id():
    _assert_case(RC.repair_case())


@pytest.mark.parametrize("sl,n_sym", RC.SHAPES, ids=lambda v: str(v))
def test_shapes(sl, n_sym):
    X = RC.shape_case(sl, n_sym)
    dec = _decoder(X)
    _assert_case(X, dec)
    if sl < 4:                                                    # narrow needs SL >= 4: refused, nothing launched
        assert _call(dec, X.jobs, nb=1) == (_lib.RD_ERR_ARG, True)
        with pytest.raises(ValueError, match="symbol_length"):
            dec.decode_jobs(X.jobs, 0, True)


def test_many_jobs():
    X, _, _ = RC.many_jobs_case()
    RC.check_many_jobs(X)
    dec = _decoder(X)
    first = _assert_case(X, dec)
    again = _assert_case(X, dec)                                  # a second call on the same upload
    for form in X.forms():
        assert first[form].records.tobytes() == again[form].records.tobytes()
        assert first[form].headers.tobytes() == again[form].headers.tobytes() and np.array_equal(first[form].soft, again[form].soft)
    # the order of the jobs changes nothing: the same jobs backwards
    back = dec.decode_jobs(X.jobs[::-1].copy(), 2, True, soft=True)
    want = first[2, True]
    for f in BURST_MSG_DTYPE.names:
        if f != "first":
            assert np.array_equal(back.records[f][::-1], want.records[f]), f
    assert back.headers[::-1].tobytes() == want.headers.tobytes() and np.array_equal(back.soft[::-1], want.soft)


# ------------------------------------------------------------------------------------------ a live receiver's rows, replayed
LIVE_BS = 2048
LIVE_CLIPS = (3, 64, 64, 8192)                                   # runs and messages, 64 outputs before and behind


@pytest.mark.parametrize("narrow", (False, True), ids=("wide", "narrow"))
def test_live_equivalence(narrow):
    """The small receiver of tests/test_wideband_quality.py with its expectation table and clips on: every expected row,
    replayed from the stitched recordings with the row's own direction at the row's tau, gives the row again."""
    import test_wideband_quality as WQ
    sl, n_sym = 14, 80
    body, m = sl * (n_sym - 1), sl + 2
    _, stream = DC.device_capture()
    rx = WQ._receiver(LIVE_BS, narrow=narrow)
    rx.set_burst_clips(*LIVE_CLIPS)
    tab = WQ._table()
    st = clips.ClipStitcher(LIVE_BS)
    rows, recordings = [], []
    for chunk in DC.chunks_of(stream, LIVE_BS):
        rx.set_burst_expect(tab)
        rx.demodulate(chunk)
        x = rx.expected_messages()
        rows += [(r.copy(), x.chunk) for r in x.records]
        c = rx.burst_clips()
        assert not c.dropped.any()
        recordings += st.add(c, c.chunk * LIVE_BS)
    recordings += st.flush()
    assert len(rows) >= 4 and all(bool(int(r["flags"]) & 4) == narrow for r, _ in rows)
    pool, offsets = replay.pack(recordings)
    jobs, live = [], []
    for r, chunk in rows:
        t, e = int(r["time"]), tab[int(r["first"])]
        hold = [k for k, rec in enumerate(recordings) if rec.channel == int(r["channel"]) and rec.time + m <= t - sl
                and t + body + 1 + m <= rec.time + len(rec.iq)]
        assert len(hold) == 1, (r, [(rec.channel, rec.time, len(rec.iq)) for rec in recordings])     # none is left out
        # the live filter saw real samples on both sides too: the row's region lies M outputs inside its two chunks
        tau_live = t - chunk * LIVE_BS
        assert tau_live + body + 1 + m <= LIVE_BS and tau_live - sl - m >= (-1152 if chunk else 0)
        rec = recordings[hold[0]]
        tau = t - rec.time
        jobs.append(RC.job_row(offsets[hold[0]], len(rec.iq), tau, tau, (int(e["corr_re"]), int(e["corr_im"])), int(e["id"]),
                               rec.channel, rec.time))
        live.append(r)
    dec = ClipDecoder(rx.cfg)
    dec.upload(pool)
    got = dec.decode_jobs(RC.jobs_of(jobs), 0, narrow)
    assert np.all(got.headers["n_msgs"] == 1) and np.all(got.headers["candidates"] == 1)
    for j, r in enumerate(live):
        for f in ("time", "data", "margin", "f_re", "f_im", "ones", "id", "pad"):
            assert np.array_equal(got.records[j][f], r[f]), (j, f, got.records[j][f], r[f])
        assert int(got.records[j]["flags"]) == replay.REPLAYED | (4 if narrow else 0) and int(got.records[j]["first"]) == j


# ------------------------------------------------------------------------------------------ arguments
def _call(dec, jobs, n=None, r=0, nb=0, fill=0x5A):
    """rd_clips_decode on buffers filled with ``fill``: (rc, the buffers are untouched)."""
    jobs = np.ascontiguousarray(jobs, CLIP_JOB_DTYPE)
    k = max(jobs.size, 1)
    recs = np.frombuffer(bytes([fill]) * (BURST_MSG_DTYPE.itemsize * k), BURST_MSG_DTYPE).copy()
    hdr = np.frombuffer(bytes([fill]) * (16 * k), CD_HEADER_DTYPE).copy()
    rc = _lib.lib().rd_clips_decode(dec._h, jobs.ctypes.data, jobs.size if n is None else n, r, nb, recs.ctypes.data, hdr.ctypes.data, None)
    return rc, recs.tobytes() == bytes([fill]) * recs.nbytes and hdr.tobytes() == bytes([fill]) * hdr.nbytes


def test_arguments():
    L = _lib.lib()
    X = RC.shape_case(4, 40)
    n = int(X.jobs[0]["n"])
    good = X.jobs[:1].copy()
    fresh = ClipDecoder(X.cfg)
    assert _call(fresh, good) == (_lib.RD_ERR_STATE, True)        # a decode before any upload
    with pytest.raises(RuntimeError, match="upload"):
        fresh.decode_jobs(good)
    dec = _decoder(X)
    assert _call(dec, good)[0] == _lib.RD_OK
    for r, nb in ((-1, 0), (3, 0), (0, 2), (0, -1)):
        assert _call(dec, good, r=r, nb=nb) == (_lib.RD_ERR_ARG, True), (r, nb)
    for count in (0, -1, 2 ** 20 + 1):
        assert _call(dec, good, n=count) == (_lib.RD_ERR_ARG, True), count
    pool_outputs = X.pool.size // 2
    bad = {"offset": (4, 8 * 10 ** 6), "n": (0, pool_outputs + 1), "tau_lo": (int(good[0]["tau_hi"]) + 1, -2 ** 30 - 1),
           "tau_hi": (int(good[0]["tau_lo"]) + 2049, 2 ** 30 + 1), "id": (8, 0xFE, 0x100), "corr_re": (32768, -32769),
           "corr_im": (32768, -32769), "pad": (1,)}
    for field, values in bad.items():
        for v in values:
            j = np.concatenate([good, good])
            j[1][field] = v
            if field == "tau_hi" and v > 2 ** 30:
                j[1]["tau_lo"] = v - 5
            if field == "tau_lo" and v < -2 ** 30:
                j[1]["tau_hi"] = v + 5
            assert RC.check_jobs(j, pool_outputs) == (-1, 1), (field, v)
            assert _call(dec, j) == (_lib.RD_ERR_ARG, True), (field, v)
            assert "job 1" in _lib.last_error()
    assert L.rd_clips_decode(dec._h, None, 1, 0, 0, None, None, None) == _lib.RD_ERR_ARG
    assert L.rd_clips_decode(None, good.ctypes.data, 1, 0, 0, None, None, None) == _lib.RD_ERR_ARG
    assert L.rd_clips_upload(dec._h, None, 16) == _lib.RD_ERR_ARG and L.rd_clips_upload(dec._h, X.pool.ctypes.data, 0) == _lib.RD_ERR_ARG
    assert L.rd_clips_upload(dec._h, X.pool.ctypes.data, 3) == _lib.RD_ERR_ARG
    # a job that merely has no candidate is legal and idle
    idle = good.copy()
    idle[0]["tau_lo"], idle[0]["tau_hi"] = n, n + 10
    got = dec.decode_jobs(idle)
    assert got.headers[0].tobytes() == bytes(16) and got.records[0].tobytes() == bytes(BURST_MSG_DTYPE.itemsize)
    # the last clip may end at the pool's last output, n % 8 = 5: the last vector's three outputs of slack lie past the pool
    assert n % 8 == 5 and X.offsets == [0]
    dec.upload(X.pool[: 2 * n].copy())
    RC.assert_replay_equals(dec.decode_jobs(X.jobs, 2, True, soft=True), X.want(2, True), "a pool that ends with its clip")
    # the configurations burst decode refuses are refused at create - but for block_size, which takes no part
    h = C.c_void_p()
    for sl, pre, n_sym, bs in ((14, 16, 80, 100), (14, 16, 80, 0)):
        assert L.rd_clips_create(C.byref(_lib.make_config(19200, sl, pre, n_sym, "1100101110001001", bs)), C.byref(h)) == _lib.RD_OK
        L.rd_clips_destroy(h)
    for sl, pre, n_sym, sync in ((14, 8, 80, "11001011"), (14, 16, 36, "1100101110001001"), (14, 16, 88, "1100101110001001"),
                                 (52, 16, 40, "1100101110001001"), (0, 16, 80, "1100101110001001")):
        assert L.rd_clips_create(C.byref(_lib.make_config(19200, sl, pre, n_sym, sync, 2048)), C.byref(h)) == _lib.RD_ERR_ARG
    assert L.rd_clips_create(None, C.byref(h)) == _lib.RD_ERR_ARG


def test_decode_packs_plans_and_drops_repeats():
    """ClipDecoder.decode on recordings: one long recording that plan() cuts into two ranges with the packet's adjacent valid
    positions on both sides of the cut, and two short ones - every packet once, under every form."""
    sl, n_sym = 14, 80
    datas = [DC.packet(n_sym, ident=k, seed=3600 + k) for k in range(3)]
    cut = sl + replay.MAX_SPAN                                    # the last tau of the first range
    long_clip = RC.burst_clip(datas[0], sl, 4000, cut - 64 - sl + 1 + 2, 3600)        # the first symbol ends 2 past the cut
    recs = [clips.Recording(5, 2 ** 64 - 700, long_clip.reshape(-1, 2), ()),
            clips.Recording(1, 10 ** 6, RC.burst_clip(datas[1], sl, 1403, 100, 3601, carrier=-0.2).reshape(-1, 2), ()),
            clips.Recording(2, 555, RC.burst_clip(datas[2], sl, 1500, 200, 3602).reshape(-1, 2), ())]
    dec = ClipDecoder(DC.config(sl, n_sym, 2048))
    jobs, owner = dec.jobs_for(recs, replay.pack(recs)[1])
    assert list(owner) == [0, 0, 1, 2] and int(jobs[0]["tau_hi"]) == cut == int(jobs[1]["tau_lo"]) - 1
    dec.upload(replay.pack(recs)[0])
    both = dec.decode_jobs(jobs)
    assert list(both.headers["n_msgs"]) == [1, 1, 1, 1]           # both ranges report the long recording's packet ...
    out = dec.decode(recs, forms=RC.FORMS)
    assert [o.form for o in out] == [tuple(f) for f in RC.FORMS]
    for o in out:                                                 # ... and decode() hands it out once, the earlier job's
        assert list(o.recording) == [0, 1, 2] and [bytes(r["data"]) for r in o.records] == datas, o.form
        assert int(o.records[0]["first"]) == 0 and int(o.records[0]["tau"]) <= cut and np.all(acquire.replayed(o.records))
        assert int(o.records[0]["time"]) == (2 ** 64 - 700 + int(o.records[0]["tau"])) % 2 ** 64 and list(o.records["channel"]) == [5, 1, 2]
    f = acquire.burst_message_offset_hz(out[0].records[1], dec.out_rate, dec.if_hz)
    assert abs(f - (-0.2 * dec.out_rate - dec.if_hz)) < 1500
    given = dec.decode(recs, offset_hz=[0.11 * dec.out_rate - dec.if_hz, f, 0.11 * dec.out_rate - dec.if_hz], ident=[0, 1, 7])
    assert [bytes(r["data"]) for r in given[0].records] == datas[:2] and list(given[0].recording) == [0, 1]
