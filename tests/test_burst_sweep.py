"""The seven burst kernels on seeded random launches (tests/burst_sweep_cases.py), through their test hooks: for every
seed of SEEDS and every family the scene applies to, the device's whole slot - every field of every record and header,
and 0xA5 wherever the kernel must not write - equals the integer model's, byte for byte.  The launching and comparing code
is that of the crafted device tests (test_burst_kernels_crafted.py, test_burst_narrow.py, test_burst_track.py,
test_burst_search.py, test_burst_quality.py, test_burst_clips.py, test_clip_replay.py), imported, not copied; a scene
whose row stride is above 2 block_size goes to the hooks in that layout, 0xA5 in the gaps.  Then the stages chained on
the device's own outputs, and ten scenes launched twice.  Equality throughout; a failure names the launch
"sweep<seed>_<family>", and burst_sweep_cases.chain(<seed>) rebuilds it.  tests/test_burst_sweep_cpu.py holds the draw
against its coverage floors and shows that it tells mutated models from the right ones, without a device."""
import copy

import pytest

import burst_sweep_cases as S
import clip_replay_cases as CR
import test_burst_clips as T_CLIPS
import test_burst_kernels_crafted as T_BURSTS
import test_burst_narrow as T_DECODE
import test_burst_quality as T_QUALITY
import test_burst_search as T_SEARCH
import test_burst_track as T_EXPECT
from rtldavis_amd.replay import ClipDecoder

pytestmark = pytest.mark.gpu

TWICE = S.SEEDS[5:45:4]                                       # the ten scenes launched twice


def _lib_with_device():
    from rtldavis_amd import _lib
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    return _lib


def _laid_out(L, sc):
    """The launch as the hooks are to see it: its bytes in the scene's row stride (the model keeps the rows alone)."""
    D = copy.copy(L)
    D.cur, D.prev = S.device_bytes(sc)
    return D


# ------------------------------------------------------------------------------------------ one family on the device
def _bursts(lib, sc, cs):
    return T_BURSTS._run_bursts(lib, cs)


def _decode(lib, sc, L):
    """{(max_flips, narrow): slot} of every form the scene admits, and the plain hook's slot under "plain"."""
    D = _laid_out(L, sc)
    out = {(r, nb): T_DECODE._run(lib, D, r, 1 if nb else 0) for r, nb in S.decode_forms(sc)}
    out["plain"] = T_BURSTS._run_decode(lib, D)
    return out


def _assert_decode(L, got):
    T_BURSTS._assert_decode(L, got["plain"])
    for form, slot in got.items():
        if form != "plain":
            T_DECODE._assert_slot(L.name, form, slot, S.decode_want(L, *form))


def _expect(lib, sc, X):
    D = _laid_out(X, sc)
    return {form: T_EXPECT._run(lib, D, *form) for form in X.forms()}


def _assert_expect(X, got):
    for (r, nb), slot in got.items():
        T_EXPECT._assert_slot(X, r, nb, slot)


def _search(lib, sc, L):
    return T_SEARCH._run(lib, _laid_out(L, sc))


def _quality(lib, sc, Q):
    return T_QUALITY._run(lib, _laid_out(Q, sc))


def _clips(lib, sc, X):
    return T_CLIPS._run(lib, _laid_out(X, sc))


def _replay(lib, sc, R):
    dec = ClipDecoder(R.cfg)
    dec.upload(R.pool)
    return {form: dec.decode_jobs(R.jobs, form[0], form[1], soft=True) for form in R.forms()}


def _assert_replay(R, got):
    for (r, nb), g in got.items():
        CR.assert_replay_equals(g, R.want(r, nb), (R.name, r, nb))


def _replay_bytes(got):
    return [(g.records.tobytes(), g.headers.tobytes(), g.soft.tobytes()) for _, g in sorted(got.items())]


# ------------------------------------------------------------------------------------------ every seed, family by family
def test_bursts():
    lib = _lib_with_device()
    for seed in S.SEEDS:
        ch = S.cached_chain(seed)
        T_BURSTS._assert_bursts(ch.bursts, *_bursts(lib, ch.scene, ch.bursts))


def test_decode_all_forms():
    """rd_debug_burst_decode, and rd_debug_burst_decode_narrow at max_flips 0, 1, 2 without and (SL >= 4) with the filter,
    on the scene's run table - in a quarter of the scenes rewritten by hand."""
    lib = _lib_with_device()
    for seed in S.SEEDS:
        ch = S.cached_chain(seed)
        _assert_decode(ch.decode, _decode(lib, ch.scene, ch.decode))


def test_expect_all_forms():
    lib = _lib_with_device()
    for seed in S.SEEDS:
        ch = S.cached_chain(seed)
        _assert_expect(ch.expect, _expect(lib, ch.scene, ch.expect))


def test_search():
    lib = _lib_with_device()
    ran = 0
    for seed in S.SEEDS:
        ch = S.cached_chain(seed)
        if ch.search is not None:
            T_SEARCH._assert_slot(ch.search, _search(lib, ch.scene, ch.search))
            ran += 1
    assert ran == sum(sl >= 4 for _, sl in (S.SHAPES[s % len(S.SHAPES)] for s in S.SEEDS))


def test_quality():
    lib = _lib_with_device()
    for seed in S.SEEDS:
        ch = S.cached_chain(seed)
        T_QUALITY._assert_slot(ch.quality, _quality(lib, ch.scene, ch.quality))


def test_clips():
    lib = _lib_with_device()
    for seed in S.SEEDS:
        ch = S.cached_chain(seed)
        T_CLIPS._assert_slot(ch.clips, _clips(lib, ch.scene, ch.clips))


def test_replay():
    lib = _lib_with_device()
    ran = 0
    for seed in S.SEEDS:
        ch = S.cached_chain(seed)
        if ch.replay is not None:
            _assert_replay(ch.replay, _replay(lib, ch.scene, ch.replay))
            ran += 1
    assert ran >= len(S.SEEDS) // 2


# ------------------------------------------------------------------------------------------ the stages chained
def _stage(seed, name, check, *a):
    try:
        check(*a)
    except AssertionError as e:
        raise AssertionError(f"seed {seed}: chained on the device's own outputs, {name} is the first stage that differs from the model: {e}") from e


def test_stages_chained_on_the_devices_own_outputs():
    """A quarter of the seeds: the device's burst records go to the device's decode; the device's decode, expect and search
    rows to the device's quality and clips; the device's clip pool to the replay decoder.  Every stage equals the model run
    on what the device handed to it."""
    lib = _lib_with_device()
    for seed in S.CHAINED:
        sc = S.scene(seed)
        cs = S.make_bursts(sc)
        recs, floor = _bursts(lib, sc, cs)
        _stage(seed, "bursts", T_BURSTS._assert_bursts, cs, recs, floor)
        runs, n_runs = S.scene_runs(sc, recs, floor)
        L = S.make_decode(sc, runs, n_runs)
        d_got = _decode(lib, sc, L)
        _stage(seed, "decode", _assert_decode, L, d_got)
        X = S.make_expect(sc)
        x_got = _expect(lib, sc, X)
        _stage(seed, "expect", _assert_expect, X, x_got)
        F = S.make_search(sc)
        s_got = None
        if F is not None:
            s_got = _search(lib, sc, F)
            _stage(seed, "search", T_SEARCH._assert_slot, F, s_got)
        msgs, n_msgs = d_got[sc.feed_form][:2]
        Q = S.make_quality(sc, msgs, n_msgs)
        _stage(seed, "quality", T_QUALITY._assert_slot, Q, _quality(lib, sc, Q))
        K = S.make_clips(sc, runs, n_runs, msgs, n_msgs, x_got[sc.feed_form], s_got)
        slot = _clips(lib, sc, K)
        _stage(seed, "clips", T_CLIPS._assert_slot, K, slot)
        R = S.make_replay(sc, slot)
        if R is not None:
            _stage(seed, "replay", _assert_replay, R, _replay(lib, sc, R))


def test_the_same_scene_twice_gives_the_same_bytes():
    lib = _lib_with_device()
    for seed in TWICE:
        ch = S.cached_chain(seed)
        sc = ch.scene
        runs = []
        for _ in range(2):
            got = [a.tobytes() for a in _bursts(lib, sc, ch.bursts)]
            got += [a.tobytes() for _, slot in sorted(_decode(lib, sc, ch.decode).items(), key=str) for a in slot]
            got += [a.tobytes() for _, slot in sorted(_expect(lib, sc, ch.expect).items()) for a in slot]
            if ch.search is not None:
                got += [a.tobytes() for a in _search(lib, sc, ch.search)]
            got += [_quality(lib, sc, ch.quality).tobytes(), _clips(lib, sc, ch.clips).tobytes()]
            if ch.replay is not None:
                got += _replay_bytes(_replay(lib, sc, ch.replay))
            runs.append(got)
        assert len(runs[0]) == len(runs[1])
        for i, (a, b) in enumerate(zip(*runs)):
            assert a == b, f"seed {seed}: output {i} of the second launch differs from the first"
