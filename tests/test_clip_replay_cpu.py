"""The host's share of the clip decoder (rtldavis_amd/replay.py, rd_cd_check_jobs in rd_host.cpp) and the model wrapper of
tests/clip_replay_cases.py.  No device is touched."""
import ctypes as C

import numpy as np
import pytest

import burst_decode_cases as DC
import clip_replay_cases as RC
from rtldavis_amd import _lib, acquire, clips, replay
from rtldavis_amd.replay import CD_HEADER_DTYPE, CLIP_JOB_DTYPE
from rtldavis_amd.wideband import BURST_MSG_DTYPE


def test_layouts_and_exports():
    import rtldavis_amd
    assert CLIP_JOB_DTYPE.itemsize == 48 and CD_HEADER_DTYPE.itemsize == 16 and replay.REPLAYED == 32 == acquire.MSG_REPLAYED
    assert [CLIP_JOB_DTYPE.fields[f][1] for f in CLIP_JOB_DTYPE.names] == [0, 8, 16, 20, 24, 28, 32, 36, 40, 44]
    assert rtldavis_amd.ClipDecoder is replay.ClipDecoder and "ClipDecoder" in rtldavis_amd.__all__
    rows = np.zeros(3, BURST_MSG_DTYPE)
    rows["flags"] = (32, 8, 32 | 2 | 4)
    assert list(acquire.replayed(rows)) == [True, False, True] and list(acquire.expected(rows)) == [False, True, False]
    for name in ("rd_clips_create", "rd_clips_destroy", "rd_clips_upload", "rd_clips_decode", "rd_clips_kernel_ms", "rd_cd_check_jobs"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)


@pytest.mark.parametrize("sl,n_sym", ((14, 80), (4, 40), (51, 40), (1, 40)))
def test_plan_tiles_every_tau_exactly_once(sl, n_sym):
    need = n_sym * sl + 1
    for span in (0, 1, 7, 100, 2048):
        for n in (1, sl, need - 1, need, need + 1, need + span, need + span + 1, need + 2 * span + 2, need + 5000):
            if span < 7 and n > need + 300:
                continue                                      # (thousands of one-tau ranges show nothing more)
            got = replay.plan(n, sl, n_sym, span)
            taus = [t for lo, hi in got for t in range(lo, hi + 1)]
            assert taus == list(range(sl, n - sl * (n_sym - 1))), (n, span)
            assert all(lo <= hi and hi - lo <= span for lo, hi in got) and (n >= need) == bool(got)
    with pytest.raises(ValueError):
        replay.plan(5000, sl, n_sym, 2049)


def test_pack_aligns_every_clip():
    rng = np.random.default_rng(5)
    recs = [rng.integers(1, 256, (n, 2), dtype=np.uint8) for n in (1, 8, 9, 15, 16, 1121, 7)]
    recs[2] = clips.Recording(3, 99, recs[2], ())
    recs[3] = recs[3].reshape(-1)
    pool, off = replay.pack(recs)
    assert pool.dtype == np.uint8 and pool.ndim == 1 and off.dtype == np.int64 and list(off) == [0, 8, 16, 32, 48, 64, 1192]
    assert pool.size == 2 * (1192 + 7)
    used = np.zeros(pool.size, bool)
    for r, o in zip(recs, off):
        a = np.asarray(getattr(r, "iq", r)).reshape(-1)
        assert o % 8 == 0 and np.array_equal(pool[2 * o: 2 * o + a.size], a)
        used[2 * o: 2 * o + a.size] = True
    assert not pool[~used].any() and pool[used].all()
    for bad in ([], [np.zeros((0, 2), np.uint8)], [np.zeros(3, np.uint8)], [np.zeros((4, 2), np.int8)]):
        with pytest.raises(ValueError):
            replay.pack(bad)


def _row(channel, time, data, first=0):
    r = np.zeros(1, BURST_MSG_DTYPE)[0]
    r["channel"], r["time"], r["first"], r["flags"] = channel, time % 2 ** 64, first, replay.REPLAYED
    r["data"][: len(data)] = list(data)
    return r


def test_drop_repeats_on_handmade_rows():
    sl = 14
    a, b = bytes(range(10)), bytes(range(1, 11))
    rows = np.asarray([_row(0, 1000, a), _row(0, 1013, a),      # 13 < SL apart: the later job's row goes
                       _row(0, 1027, a),                        # 27 from the first KEPT row: stays (the dropped one is no anchor)
                       _row(0, 1030, b),                        # other data
                       _row(1, 1030, b),                        # other channel
                       _row(0, 1000, a),                        # the same packet in ANOTHER recording
                       _row(2, 2 ** 64 - 5, a), _row(2, 8, a),  # 13 apart across the wrap of the 64-bit clock
                       _row(2, 2 ** 64 - 5 + 14, a)],           # exactly SL from the kept one: stays
                      BURST_MSG_DTYPE)
    owner = np.asarray([0, 0, 0, 0, 0, 1, 2, 2, 2])
    assert list(replay.drop_repeats(rows, owner, sl)) == [0, 2, 3, 4, 5, 6, 8]
    assert list(replay.drop_repeats(rows[:0], owner[:0], sl)) == []
    assert list(replay.drop_repeats(rows[[1, 0]], owner[:2], sl)) == [0]       # the earlier job wins, whatever its time


def _check(cfg, jobs, pool_outputs, n=None):
    bad, why = C.c_int(7), C.c_char_p()
    jobs = np.ascontiguousarray(jobs, CLIP_JOB_DTYPE)
    rc = _lib.lib().rd_cd_check_jobs(C.byref(cfg), jobs.ctypes.data, jobs.size if n is None else n, pool_outputs, C.byref(bad), C.byref(why))
    assert (rc == 0) == (why.value == b"")
    return rc, bad.value


def test_check_jobs_equals_its_restatement_on_random_jobs():
    cfg = _lib.make_config(19200, 14, 16, 80, "1100101110001001", 2048)
    rng = np.random.default_rng(11)
    pool_outputs = 100000
    edge = {"offset": (0, 8, 4, 99992, 100000, 100008, 2 ** 63, 2 ** 64 - 8), "n": (0, 1, 8, 100000, 100001, 2 ** 32 - 1),
            "tau_lo": (-2 ** 30 - 1, -2 ** 30, -1, 0, 2 ** 30, 2 ** 30 + 1, -2 ** 31), "tau_hi": (-2 ** 30, 0, 2048, 2049, 2 ** 30, 2 ** 30 + 1, 2 ** 31 - 1),
            "id": (0, 7, 8, 0xFE, 0xFF, 0x100, 2 ** 32 - 1), "corr_re": (-32769, -32768, 0, 32767, 32768), "corr_im": (-32769, -32768, 0, 32767, 32768),
            "pad": (0, 0, 0, 1, 2 ** 31)}
    refused = accepted = 0
    for it in range(400):
        k = int(rng.integers(1, 6))
        jobs = RC.jobs_of([RC.job_row(8 * int(rng.integers(0, 1000)), int(rng.integers(1, 2000)), lo, lo + int(rng.integers(0, 2049)))
                           for lo in rng.integers(-3000, 3000, k)])
        for _ in range(int(rng.integers(0, 3))):                   # zero, one or two fields at an edge value
            f = list(edge)[int(rng.integers(0, len(edge)))]
            jobs[int(rng.integers(0, k))][f] = edge[f][int(rng.integers(0, len(edge[f])))]
        want = RC.check_jobs(jobs, pool_outputs)
        assert _check(cfg, jobs, pool_outputs) == want, jobs
        refused += want[0] != 0
        accepted += want[0] == 0
    assert refused >= 100 and accepted >= 100
    one = RC.jobs_of([RC.job_row(0, 10, 0, 0)])
    assert _check(cfg, one, 10) == (0, -1) and _check(cfg, one, 9) == (-1, 0)
    for n in (0, -1, 2 ** 20 + 1):
        assert _check(cfg, one, 10, n) == (-1, -1)
    L = _lib.lib()
    assert L.rd_cd_check_jobs(C.byref(cfg), None, 1, 10, None, None) == _lib.RD_ERR_ARG
    assert L.rd_cd_check_jobs(None, one.ctypes.data, 1, 10, None, None) == _lib.RD_ERR_ARG
    assert L.rd_cd_check_jobs(C.byref(cfg), one.ctypes.data, 1, 10, None, None) == _lib.RD_OK


def test_create_and_refusals_touch_no_device():
    cfg = DC.config(14, 80, 77)                                   # block_size takes no part
    dec = replay.ClipDecoder(cfg)
    assert dec.corr(0.0) == (0, -16384) and dec.if_hz == -67200
    with pytest.raises(ValueError):
        replay.ClipDecoder(DC.config(14, 88, 2048))
    with pytest.raises(ValueError):
        dec.decode_jobs(RC.jobs_of([RC.job_row(0, 10, 0, 0)]), 3)      # max_flips is checked before the pool
    with pytest.raises(ValueError):
        dec.decode(np.zeros((0, 2), np.uint8)[None])


def test_the_wrapper_tells_a_mutant_from_the_definition():
    X = RC.own_direction_case()
    sl, n_sym = X.sl, X.n_sym
    # the own direction over the whole clip instead of the region: the crafted clip no longer sums to (0, 0)
    job = X.jobs[2]
    right = RC.decode_job(X.clips[2], job, 2, sl, n_sym, 0, False)
    wrong = RC.decode_job(X.clips[2], job, 2, sl, n_sym, 0, False, whole_clip=True)
    assert right[1] == (0, 1, 0, 0) and wrong[1][2:] != (0, 0)
    # ... and a burst's direction moves with what lies beside its region
    job = X.jobs[0].copy()
    job["tau_lo"], job["tau_hi"] = 150, 200
    a = RC.decode_job(X.clips[0], job, 0, sl, n_sym, 0, False)
    b = RC.decode_job(X.clips[0], job, 0, sl, n_sym, 0, False, whole_clip=True)
    assert a[1][2:] != b[1][2:] and a[0] is not None
    # bytes outside the clip's n outputs are not the wrapper's to see; bytes outside the region do not move the result
    clip = X.clips[0].copy()
    clip[: 2 * (150 - sl)] ^= 0xFF
    clip[2 * (200 + sl * (n_sym - 1) + 1):] ^= 0xFF
    c = RC.decode_job(clip, job, 0, sl, n_sym, 0, False)
    assert c[0] == a[0] and c[1] == a[1] and np.array_equal(c[2], a[2])
    # the soft values are the winner's symbol sums: their signs are the record's bits, their least magnitude its margin
    row, _, soft = a
    assert bytes(np.packbits(soft > 0)) == bytes(row[8][: n_sym // 8]) and int(np.abs(soft).min()) == row[5]
    # a repaired record's soft values are those BEFORE the flip
    R = RC.repair_case()
    recs, hdr, soft = R.want(1, False)
    m = recs[0]
    k = int(m["pad"][1])
    bits = np.unpackbits(np.asarray(m["data"][: R.n_sym // 8], np.uint8))
    assert int(m["pad"][0]) == 1 and (soft[0][k] > 0) != bool(bits[k]) and np.array_equal(np.delete(soft[0] > 0, k), np.delete(bits, k).astype(bool))


def test_every_case_holds_its_edges_on_the_model():
    RC.edges_case()
    RC.isolation_case()
    RC.repair_case()
    for sl, n_sym in RC.SHAPES:
        RC.shape_case(sl, n_sym)
    RC.check_many_jobs(RC.many_jobs_case()[0])
