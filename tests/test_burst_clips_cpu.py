"""BURST CLIPS without a device: rd_bc_window through the C ABI against the model of tests/burst_clip_cases.py and against a
naive per-output enumeration; every crafted launch's edge, asserted when the case is built; rtldavis_amd.clips - the
stitcher on random overlapping, abutting and disjoint clips cut from a known random stream, and a SigMF round trip."""
import json

import numpy as np
import pytest

import burst_clip_cases as CC
from rtldavis_amd import clips
from rtldavis_amd.wideband import BURST_MSG_DTYPE, CLIP_DTYPE, BurstClips


@pytest.fixture(scope="module")
def L():
    from rtldavis_amd import _lib
    return _lib.lib()


def _window(L, bs, have_prev, a, e):
    out = np.full(3, 77, np.int32)
    ok = L.rd_bc_window(int(bs), int(have_prev), int(a), int(e), out.ctypes.data)
    assert ok in (0, 1) and (ok or not out.any())
    return tuple(int(v) for v in out) if ok else None


def test_window_equals_the_model_and_a_naive_enumeration(L):
    rng = np.random.default_rng(31)
    seen = {"clip": 0, "none": 0, CC.CUT_START: 0, CC.CUT_END: 0, CC.FROM_PREV: 0}
    for _ in range(6000):
        bs = int(rng.choice([8, 16, 128, 256, 1152]))
        have_prev = bool(rng.integers(0, 2))
        a = int(rng.integers(-2 * bs - 20, 2 * bs + 20))
        e = a + int(rng.integers(-4, 3 * bs))
        got = _window(L, bs, have_prev, a, e)
        assert got == CC.clamp(bs, have_prev, a, e) == CC.naive_clamp(bs, have_prev, a, e), (bs, have_prev, a, e, got)
        if got is None:
            seen["none"] += 1
            continue
        seen["clip"] += 1
        for bit in (CC.CUT_START, CC.CUT_END, CC.FROM_PREV):
            seen[bit] += 1 if got[2] & bit else 0
        t0, n, _ = got
        assert t0 % 8 == 0 and n % 8 == 0 and n >= 8 and (-bs if have_prev else 0) <= t0 and t0 + n <= bs
    assert all(v > 300 for v in seen.values()), seen


def test_window_on_64_bit_requests_and_bad_blocks(L):
    big = 2 ** 63 - 1
    assert _window(L, 128, True, -big - 1, big) == (-128, 256, CC.CUT_START | CC.CUT_END | CC.FROM_PREV)
    assert _window(L, 128, False, -big - 1, big) == (0, 128, CC.CUT_START | CC.CUT_END)
    assert _window(L, 128, True, big, -big - 1) is None and _window(L, 128, True, big - 5, big) is None
    assert _window(L, 128, True, -big - 1, -big + 5) is None
    assert _window(L, 128, True, 127, big) == (120, 8, CC.CUT_END) and _window(L, 128, True, -big, -127) == (-128, 8, CC.CUT_START | CC.FROM_PREV)
    for bs in (0, -8, 4, 12, 129):
        assert _window(L, bs, True, 0, 8) is None
    assert L.rd_bc_window(128, 1, 0, 8, None) == 0


def test_every_crafted_launch_builds_with_its_conditions():
    launches = CC.crafted_launches()
    assert len(launches) == 23 and len({X.name for X in launches}) == 23
    for X in launches:
        recs, hdr, pool = CC.split_slot(X.want, X.n_ch, X.quota)
        for c in range(X.n_ch):
            h = X.header(c)
            assert int(hdr[c]["n_clips"]) == h["n_clips"] <= CC.PER and int(hdr[c]["used"]) == h["used"] <= X.quota
            assert recs[c, h["n_clips"]:].tobytes() == bytes([CC.FILL]) * ((CC.PER - h["n_clips"]) * CLIP_DTYPE.itemsize)
            assert pool[c, 2 * h["used"]:].tobytes() == bytes([CC.FILL]) * (2 * (X.quota - h["used"]))
            assert int(X.records(c)["n"].sum()) == h["used"]
    assert any(X.header(c)["dropped"] for X in launches for c in range(X.n_ch))


# ------------------------------------------------------------------------------------------ the stitcher
def _stream_clips(rng, stream, bs, k, intervals):
    """BurstClips of chunk k holding the given (channel, start, end) intervals of ``stream`` [n_ch, n, 2], clamped to the
    chunk's reach K - bs .. K + bs and rounded outwards to 8 as the device does."""
    K = k * bs
    recs, data, off = [], [], 0
    for c, a, e in intervals:
        a, e = max(a, K - bs, 0), min(e, K + bs)
        a, e = a // 8 * 8, -(-e // 8) * 8
        if e <= a:
            continue
        recs.append((c, int(rng.integers(1, 5)), 0, a - K, e - a, off, a, int(rng.integers(0, 1 << 40)), k, 0))
        data.append(stream[c, a:e])
        off += e - a
    iq = np.concatenate(data) if data else np.zeros((0, 2), np.uint8)
    return BurstClips(np.asarray(recs, CLIP_DTYPE).reshape(-1), iq, np.zeros(stream.shape[0], np.uint32), k)


def _random_plan(seed, bs, n_chunks, n_ch):
    """Per chunk a list of (channel, start, end): bursts of random length, each requested several times with other rolls
    (overlapping copies), some abutting the one before, some crossing a chunk boundary (their rest requested again by
    the next chunk, as a tail is)."""
    rng = np.random.default_rng(seed)
    plan = [[] for _ in range(n_chunks)]
    for c in range(n_ch):
        t = int(rng.integers(0, bs))
        while t < n_chunks * bs - 8:
            length = int(rng.integers(8, bs // 2))
            e = min(t + length, n_chunks * bs)
            k0 = e // bs if e % bs and e // bs < n_chunks else max(e // bs - 1, 0)     # the chunk in which it ends
            for _ in range(int(rng.integers(1, 4))):
                plan[k0].append((c, t - int(rng.integers(0, 40)), e + int(rng.integers(0, 40))))
            if e + 40 > (k0 + 1) * bs and k0 + 1 < n_chunks:
                plan[k0 + 1].append((c, (k0 + 1) * bs, e + 40))              # what chunk k0 could not deliver
            gap = int(rng.choice([0, 0, 8, 100, 700]))                        # 0: the next abuts (after rounding) or overlaps
            t = e + 40 + gap
    return plan


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_stitched_recordings_equal_the_stream_and_come_out_on_time(seed):
    bs, n_chunks, n_ch = 512, 12, 3
    rng = np.random.default_rng(100 + seed)
    stream = rng.integers(0, 256, (n_ch, n_chunks * bs + 64, 2), dtype=np.uint8)
    plan = _random_plan(seed, bs, n_chunks, n_ch)
    st = clips.ClipStitcher(bs)
    covered = np.zeros((n_ch, stream.shape[1]), bool)
    got, merged, n_clips = [], 0, 0
    for k in range(n_chunks):
        bc = _stream_clips(rng, stream, bs, k, plan[k])
        n_clips += bc.records.size
        for r in bc.records:
            covered[int(r["channel"]), int(r["time"]): int(r["time"]) + int(r["n"])] = True
        out = st.add(bc, k * bs)
        # handed out no later than the rule says: nothing that ends before this chunk's clock is still held back ...
        for ch, segs in st._open.items():
            assert all(s[0] + len(s[1]) >= k * bs for s in segs), (k, ch)
        # ... and nothing that a later chunk could still extend has left
        assert all(r.time + len(r.iq) < k * bs for r in out)
        got += out
    got += st.flush()
    assert not any(st._open.values())
    # every recording is the stream's slice; together they are exactly what the clips covered, in maximal stretches
    again = np.zeros_like(covered)
    for r in got:
        assert r.iq.dtype == np.uint8 and r.iq.shape == (len(r.iq), 2)
        assert np.array_equal(r.iq, stream[r.channel, r.time: r.time + len(r.iq)])
        assert not again[r.channel, r.time: r.time + len(r.iq)].any()
        again[r.channel, r.time: r.time + len(r.iq)] = True
        assert r.time == 0 or not covered[r.channel, r.time - 1]
        assert not covered[r.channel, r.time + len(r.iq)]
        merged += len(r.refs) > 1
    assert np.array_equal(again, covered)
    assert len(got) >= 10 and merged >= 5
    assert sum(len(r.refs) for r in got) == n_clips


def test_a_planted_disagreement_raises():
    bs = 256
    rng = np.random.default_rng(5)
    stream = rng.integers(0, 256, (1, 4 * bs, 2), dtype=np.uint8)
    good = _stream_clips(rng, stream, bs, 1, [(0, 200, 400), (0, 304, 504)])
    assert len(clips.ClipStitcher(bs).add(good, bs)) == 0
    bad = BurstClips(good.records, good.iq.copy(), good.dropped, good.chunk)
    at = int(bad.records[1]["offset"]) + 10                       # output 314 of the second copy: inside the overlap
    bad.iq[at, 1] ^= 1
    with pytest.raises(ValueError, match="disagree at output 314"):
        clips.ClipStitcher(bs).add(bad, bs)
    # outside the overlap the same flip is just other data
    far = BurstClips(good.records, good.iq.copy(), good.dropped, good.chunk)
    far.iq[int(far.records[1]["offset"]) + 150, 1] ^= 1
    st = clips.ClipStitcher(bs)
    st.add(far, bs)
    (rec,) = st.flush()
    assert rec.time == 200 and len(rec.iq) == 304
    with pytest.raises(ValueError, match="more than a chunk before"):
        clips.ClipStitcher(bs).add(good, 3 * bs)


def test_abutting_clips_merge_and_disjoint_ones_do_not():
    bs = 128
    stream = np.arange(2 * 4 * bs, dtype=np.uint32).astype(np.uint8).reshape(1, -1, 2)
    rng = np.random.default_rng(0)
    st = clips.ClipStitcher(bs)
    assert st.add(_stream_clips(rng, stream, bs, 0, [(0, 0, 64), (0, 64, 128), (0, 8, 16)]), 0) == []
    out = st.add(_stream_clips(rng, stream, bs, 1, [(0, 128, 136), (0, 200, 256)]), bs)
    assert out == []                                              # 0 .. 136 ends at the clock or later: the next chunk may extend it
    out = st.add(_stream_clips(rng, stream, bs, 2, [(0, 136, 144)]), 2 * bs)
    assert [(r.time, len(r.iq), len(r.refs)) for r in out] == [(0, 144, 5)]
    assert [(r.time, len(r.iq)) for r in st.flush()] == [(200, 56)]


# ------------------------------------------------------------------------------------------ SigMF
def test_sigmf_round_trip(tmp_path):
    rng = np.random.default_rng(9)
    rec = clips.Recording(17, 123456789012, rng.integers(0, 256, (3000, 2), dtype=np.uint8), ((1, 4), (2, 123456789500)))
    rows = np.zeros(3, BURST_MSG_DTYPE)
    rows["time"] = [123456789500, 123456789012 + 2990, 5]        # inside, cut at the end, not in the recording
    rows["data"][0] = list(bytes.fromhex("cb890520ac8bd4000e5c"))
    base = str(tmp_path / "burst")
    clips.write_sigmf(base, rec, 268800, 902_419_338 + 67200, messages=rows)
    with open(base + ".sigmf-data", "rb") as f:
        assert f.read() == rec.iq.tobytes()
    with open(base + ".sigmf-meta", encoding="utf-8") as f:
        meta = json.load(f)
    g = meta["global"]
    assert g["core:datatype"] == "cu8" and g["core:sample_rate"] == 268800.0 and g["core:version"]
    assert g["rtldavis:channel"] == 17 and g["rtldavis:time"] == 123456789012
    assert meta["captures"] == [{"core:sample_start": 0, "core:frequency": 902_419_338.0 + 67200}]
    ann = meta["annotations"]
    assert len(ann) == 2
    assert ann[0] == {"core:sample_start": 500 - 12 - 13, "core:sample_count": 1120, "core:comment": "cb890520ac8bd4000e5c"}
    assert ann[1]["core:sample_start"] == 2990 - 13 and ann[1]["core:sample_count"] == 3000 - 2977
    back, meta2 = clips.read_sigmf(base)
    assert meta2 == meta and back.channel == 17 and back.time == rec.time and back.refs == rec.refs
    assert back.iq.dtype == np.uint8 and np.array_equal(back.iq, rec.iq)
    # (time, data) pairs serve as messages too, and another packet shape moves the annotation
    clips.write_sigmf(base, rec, 268800, 1.0, messages=[(123456789500, b"\x01\x02")], symbol_length=4, packet_symbols=40)
    assert clips.read_sigmf(base)[1]["annotations"] == [{"core:sample_start": 500 - 12 - 3, "core:sample_count": 160, "core:comment": "0102"}]
    g["core:datatype"] = "cf32_le"
    with open(base + ".sigmf-meta", "w", encoding="utf-8") as f:
        json.dump(meta, f)
    with pytest.raises(ValueError, match="cu8"):
        clips.read_sigmf(base)


def test_the_package_exports_the_clip_tools():
    import rtldavis_amd
    assert rtldavis_amd.ClipStitcher is clips.ClipStitcher and rtldavis_amd.write_sigmf is clips.write_sigmf
    assert rtldavis_amd.read_sigmf is clips.read_sigmf and rtldavis_amd.Recording is clips.Recording
