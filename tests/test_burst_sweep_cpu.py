"""The seeded sweep of the burst kernels (tests/burst_sweep_cases.py) on the models alone, no device.  Three things:
the draw covers what it is meant to cover - counts of what the models report over SEEDS, each against a floor that is a
condition on the draw, not a measurement (a missed floor means the draw has to change); the sweep tells a wrong kernel
from a right one - single-deviation mutants of the models, made here by wrapping or patching and never in the case
modules, each change the expected slot of at least one scene; and the chain is consistent - quality and clips are fed the
very rows the earlier models wrote, and every clip's bytes are the slice of prev | cur its record names.

Building every chain of SEEDS (352 scenes, every family, every form of expect and replay) takes 13 to 23 s of one
CPU here, by the machine's load (measured by the fixture below, which prints it);
the counts are printed by test_coverage_floors and copied into the case module's docstring.

One listed mutant cannot be told apart by any input: the region threshold t1 - t0 < N SL + 1 off by one.  t1 - t0 is a
multiple of 128 and N SL + 1 is odd, so t1 - t0 = N SL + 1 never occurs; and a region of exactly N SL outputs has an
empty candidate range.  test_region_threshold_off_by_one_changes_nothing shows both for every shape; the nearest deviation
that can be seen - the threshold one window too high - is among the mutants."""
import time
from collections import Counter

import numpy as np
import pytest

import burst_clip_cases as CC
import burst_decode_cases as DC
import burst_narrow_cases as NB
import burst_quality_cases as QC
import burst_repair_cases as RP
import burst_search_cases as SC
import burst_sweep_cases as S
import burst_track_cases as TK
import clip_replay_cases as CR
from rtldavis_amd import synth

W = DC.W


@pytest.fixture(scope="module")
def chains():
    t0 = time.process_time()
    out = [S.cached_chain(seed).build() for seed in S.SEEDS]
    for ch in out:
        for form in ch.expect.forms():
            ch.expect.want(*form)
        if ch.replay is not None:
            for form in ch.replay.forms():
                ch.replay.want(*form)
    print(f"\n[burst sweep] {len(out)} chains built in {time.process_time() - t0:.1f} s of CPU")
    return out


# ------------------------------------------------------------------------------------------ coverage
FLOORS = {"decode_messages_R0": 100, "repaired_only": 10, "repaired_two_flips": 3, "repair_refused": 5, "look_back_messages": 10,
          "long_runs": 5, "short_regions": 10, "n_runs_above_cap": 3, "narrow_rows_two_grid_points": 20, "expect_decoded": 30,
          "expect_candidates_no_message": 30, "expect_tables_of_64": 1, "expect_nothing_launched": 1, "search_rows": 20,
          "search_dropped_headers": 2, "quality_noise_in_prev": 20, "clips": 50, "clip_channels_dropped": 5, "clip_channels_owed": 5,
          "replay_decoded": 30,
          # "jobs whose own direction is (0, 0)", in both readings: asked with corr = (0, 0), the region's own direction; and
          # jobs among those whose region sums to exactly (0, 0) - candidates counted, no record
          "replay_own_direction_jobs": 5, "replay_own_direction_zero": 5}


def test_coverage_floors(chains):
    total = Counter()
    for ch in chains:
        total.update(S.tally(ch))
    print("\n[burst sweep] counts over SEEDS:")
    for k in sorted(total, key=str):
        print(f"    {k}: {total[k]}")
    for sh in S.SHAPES:
        assert total[("shape",) + sh] >= 2, sh
    for label in S.BLOCKS:
        assert total["block", label] >= 2, label
    for n_ch in S.BIG_CH:
        assert total["n_ch", n_ch] >= 3, n_ch
    for k, floor in FLOORS.items():
        assert total[k] >= floor, (k, total[k], floor)
    assert total["stride_gap"] >= len(S.SEEDS) // 3 and total["clock_near_wrap"] >= 5 and total["seq_above_2^32"] >= 5
    assert 0 < total["have_prev"] < len(S.SEEDS)
    assert total["skipped_narrow"] == total["skipped_search"] == sum(S.SHAPES[s % len(S.SHAPES)][1] < NB.MIN_SL for s in S.SEEDS)


def test_scene_is_a_pure_function_of_the_seed():
    for seed in S.SEEDS[:12]:
        a = S.scene(seed)
        b = S.scene.__wrapped__(seed)
        assert a is not b and a.cur.tobytes() == b.cur.tobytes() and a.table.tobytes() == b.table.tobytes() and a.centres == b.centres
        assert (a.bs, a.n_ch, a.stride, a.clock, a.seq, a.quota, a.feed_form) == (b.bs, b.n_ch, b.stride, b.clock, b.seq, b.quota, b.feed_form)
        assert np.array_equal(a.thr, b.thr) and (a.prev is None) == (b.prev is None)


def test_every_input_is_one_the_hooks_admit(chains):
    """The rules the hooks check before any device work, restated on every scene: a launch the device tests make is never
    refused for its arguments."""
    for ch in chains:
        sc = ch.scene
        assert sc.bs % W == 0 and sc.bs >= sc.look and sc.stride % 16 == 0 and sc.stride >= 2 * sc.bs
        cur, prev = S.device_bytes(sc)
        assert cur.shape == (sc.n_ch, sc.stride) and np.all(cur[:, 2 * sc.bs:] == S.GAP_BYTE) and (prev is None) == (sc.prev is None)
        runs, n_runs = ch.runs
        assert runs.shape == (sc.n_ch, sc.cap)
        t = sc.table
        assert 1 <= t.size <= TK.MAX and np.all((0 <= t["channel"]) & (t["channel"] < sc.n_ch)) and np.all((t["id"] < 8) | (t["id"] == TK.ANY))
        assert np.all(t["t_lo"] <= t["t_hi"]) and np.all(t["t_hi"] - t["t_lo"] <= TK.MAX_SPAN)
        assert np.all((t["corr_re"] != 0) | (t["corr_im"] != 0)) and np.all(np.abs(t["corr_re"].astype(np.int64)) <= 32768)
        if sc.centres is not None:
            assert 1 <= len(sc.centres) <= SC.MAX_CENTRES and len(set(sc.centres)) == len(sc.centres) and all(0 <= g < 64 for g in sc.centres)
        assert 0 <= sc.gap <= QC.MAX_GAP and np.all(ch.quality.n_msgs <= sc.cap)
        assert sc.sources in (1, 2, 3) and sc.pre % 8 == sc.post % 8 == sc.quota % 8 == 0 and 8 <= sc.quota <= CC.MAX_QUOTA
        assert 0 <= sc.pre <= CC.MAX_ROLL and 0 <= sc.post <= CC.MAX_ROLL and np.all(ch.clips.n_runs <= sc.cap)
        if not sc.sources & CC.MESSAGES:
            assert ch.clips.x_msgs is None and ch.clips.s_msgs is None
        if ch.replay is not None:
            assert CR.check_jobs(ch.replay.jobs, ch.replay.pool.size // 2) == (0, -1)


# ------------------------------------------------------------------------------------------ consistency of the chain
def test_later_stages_are_fed_the_earlier_models_rows(chains):
    for ch in chains:
        sc = ch.scene
        msgs, n_msgs = S.decode_want(ch.decode, *sc.feed_form)[:2]
        runs, n_runs = ch.runs
        x_msgs, x_hdr = ch.expect.want(*sc.feed_form)
        for c in range(sc.n_ch):
            n = int(n_msgs[c])
            assert ch.quality.msgs[c, :n].tobytes() == msgs[c, :n].tobytes() and int(ch.quality.n_msgs[c]) >= n, (sc.seed, c)
            assert ch.clips.msgs[c, :n].tobytes() == msgs[c, :n].tobytes() and int(ch.clips.n_msgs[c]) == n, (sc.seed, c)
            k = min(int(n_runs[c]), sc.cap)
            assert ch.clips.runs[c, :k].tobytes() == runs[c, :k].tobytes() and int(ch.clips.n_runs[c]) == k, (sc.seed, c)
        if not sc.sources & CC.MESSAGES:
            continue
        launched = x_hdr.tobytes() != bytes([S.FILL]) * x_hdr.nbytes
        assert (ch.clips.x_msgs is not None) == launched, sc.seed
        if launched:
            live = np.flatnonzero(x_hdr[: sc.table.size]["n_msgs"] == 1)
            assert ch.clips.x_msgs[live].tobytes() == x_msgs[live].tobytes(), sc.seed
            assert np.array_equal(ch.clips.x_hdr["n_msgs"][: sc.table.size], x_hdr["n_msgs"][: sc.table.size]), sc.seed
        if ch.search is not None:
            s_msgs, s_hdr = ch.search.want()
            k = len(sc.centres)
            assert np.array_equal(ch.clips.s_hdr["n_msgs"][:k], s_hdr["n_msgs"][:k]), sc.seed
            for i in range(k):
                for c in range(sc.n_ch):
                    n = int(s_hdr[i, c]["n_msgs"])
                    assert ch.clips.s_msgs[i, c, :n].tobytes() == s_msgs[i, c, :n].tobytes(), (sc.seed, i, c)


def test_every_clip_is_the_slice_its_record_names(chains):
    seen = 0
    for ch in chains:
        sc = ch.scene
        recs, hdr, pool = CC.split_slot(ch.clips.want, sc.n_ch, sc.quota)
        both = sc.cur if sc.prev is None else np.concatenate([sc.prev, sc.cur], axis=1)
        org = 0 if sc.prev is None else sc.bs
        for c in range(sc.n_ch):
            for r in recs[c, : int(hdr[c]["n_clips"])]:
                t0, n, off = int(r["t0"]), int(r["n"]), int(r["offset"])
                assert org + t0 >= 0 and t0 + n <= sc.bs and off + n <= sc.quota, (sc.seed, c)
                assert pool[c, 2 * off: 2 * (off + n)].tobytes() == both[c, 2 * (org + t0): 2 * (org + t0 + n)].tobytes(), (sc.seed, c, t0, n)
                seen += 1
        if ch.replay is not None:                            # and the replay's clips are those recordings
            for k, clip in enumerate(ch.replay.clips):
                o = ch.replay.offsets[k]
                assert ch.replay.pool[2 * o: 2 * o + clip.size].tobytes() == clip.tobytes()
    assert seen >= FLOORS["clips"]


# ------------------------------------------------------------------------------------------ mutants
def _variant_decode_run(sums, narrow, cur, prev, rec, cfg, have_prev, max_flips, tie_larger=False):
    """burst_repair_cases.decode_run / burst_narrow_cases.decode_run restated over their own symbol_sums, with the one
    deviation a mutant needs: an equal (flips, margin) goes to the larger tau."""
    sl, n, sync, _ = DC.shape(cfg)
    got = sums(cur, prev, rec, cfg, have_prev)
    if got is None:
        return None
    taus, s, back, p_re, p_im, t0 = got[:6]
    best = None
    for j in np.flatnonzero(np.all((s[:, :16] > 0) == np.asarray(sync, bool)[None, :], axis=1)):
        r = RP.repair_model(s[j], max_flips, tuple(sync))
        if r is None:
            continue
        key = (len(r[0]), -r[2], -int(taus[j]) if tie_larger else int(taus[j]))
        if best is None or key < best[0]:
            best = (key, r, int(taus[j]))
    if best is None:
        return None
    (n_flip, neg_margin, _), (ks, bits, _), tau = best
    data = bytes(np.packbits(bits))
    tt = np.arange(tau - sl + 1, tau + sl * (n - 1) + 1) - (t0 + 1)
    pad = [n_flip] + list(ks) + [0] * (2 - len(ks)) + [got[6] if narrow else 0]
    flags = (1 if back else 0) | (RP.REPAIRED if n_flip else 0) | (NB.NARROW if narrow else 0)
    return tau, flags, -neg_margin, int(p_re[tt].sum()), int(p_im[tt].sum()), data, int(sum(bits)), synth._swap_bits8(data[2]) & 7, pad


def _patch_decode_run(mp, **kw):
    wide_sums, narrow_sums = RP.symbol_sums, NB.symbol_sums
    mp.setattr(RP, "decode_run", lambda cur, prev, rec, cfg, hp, r: _variant_decode_run(wide_sums, False, cur, prev, rec, cfg, hp, r, **kw))
    mp.setattr(NB, "decode_run", lambda cur, prev, rec, cfg, hp, r, narrow=True, tab=None: (
        _variant_decode_run(narrow_sums, True, cur, prev, rec, cfg, hp, r, **kw) if narrow else RP.decode_run(cur, prev, rec, cfg, hp, r)))


def _wrap_sums(mp, change):
    """Both symbol_sums through ``change(got, rec, cfg)`` -> got or None."""
    for mod in (RP, NB):
        orig = mod.symbol_sums
        mp.setattr(mod, "symbol_sums", lambda cur, prev, rec, cfg, hp, *a, _o=orig: (
            lambda got: None if got is None else change(got, rec, cfg))(_o(cur, prev, rec, cfg, hp, *a)))


def _drop(got, sl):
    taus, s = got[0][sl], got[1][sl]
    return None if taus.size == 0 else (taus, s) + tuple(got[2:])


def _wrap_runs(mp, change):
    """Both decode_run through ``change(orig, cur, prev, rec, cfg, have_prev, *rest)``."""
    for mod in (RP, NB):
        orig = mod.decode_run
        mp.setattr(mod, "decode_run", lambda cur, prev, rec, cfg, hp, *a, _o=orig, **k: change(_o, cur, prev, rec, cfg, hp, *a, **k))


def _m_tie(mp):
    _patch_decode_run(mp, tie_larger=True)


def _m_range_lo(mp):
    _wrap_sums(mp, lambda got, rec, cfg: _drop(got, slice(1, None)))


def _m_range_hi(mp):
    _wrap_sums(mp, lambda got, rec, cfg: _drop(got, slice(None, -1)))


def _m_no_look_back(mp):
    _wrap_runs(mp, lambda o, cur, prev, rec, cfg, hp, *a, **k: o(cur, prev, rec, cfg, False, *a, **k))


def _m_look_back_without_prev(mp):
    def change(o, cur, prev, rec, cfg, hp, *a, **k):
        if prev is None and int(rec["flags"]) & 1:
            return o(cur, np.full(cur.size, 128, np.uint8), rec, cfg, True, *a, **k)
        return o(cur, prev, rec, cfg, hp, *a, **k)
    _wrap_runs(mp, change)


def _m_need_one_window_more(mp):
    def change(got, rec, cfg):
        sl, n, _, _ = DC.shape(cfg)
        return None if W * (int(rec["first"]) + int(rec["windows"])) - got[5] < n * sl + 1 + W else got
    _wrap_sums(mp, change)


def _m_long_runs_at_max(mp):
    for mod in (DC, RP, NB):
        mp.setattr(mod, "MAX_W", DC.MAX_W - 1)               # windows > 31: >= MAX_W


def _m_rank_wrong_end(mp):
    mp.setattr(RP, "ranked", lambda s: sorted(range(16, len(s)), key=lambda k: (-abs(int(s[k])), k))[: RP.LIST])


def _m_grid_other_way(mp):
    orig = NB.grid_choice

    def other(cre, cim, sl=NB.MIN_SL):
        sh, ca, cb, g = orig(cre, cim, sl)
        C = NB.table(sl)[1]
        score = lambda q: ca * int(C[q % NB.GRID, 0]) + cb * int(C[q % NB.GRID, 1])
        return sh, ca, cb, ((g + 1) if score(g + 1) >= score(g - 1) else (g - 1)) % NB.GRID
    mp.setattr(NB, "grid_choice", other)


def _m_expect_t_hi(mp):
    orig = TK.candidate_range
    mp.setattr(TK, "candidate_range", lambda cfg, hp, clock, t_lo, t_hi: orig(cfg, hp, clock, t_lo, int(t_hi) - (int(t_hi) > int(t_lo))))


def _m_search_last_four(mp):
    orig = SC.search_channel

    def last(*a):
        hits, rows = orig(*a)
        return hits, rows[-SC.PER:] + rows[: -SC.PER] if len(rows) > SC.PER else rows
    mp.setattr(SC, "search_channel", last)


def _m_quality_noise_shift(mp):
    orig = QC.windows

    def shifted(sl, n, bs, have_prev, tau, gap):
        w = orig(sl, n, bs, have_prev, tau, gap)
        if w is None or w[4] <= w[3] or w[3] - 1 < (-bs if have_prev else 0):
            return w
        return w[:3] + (w[3] - 1, w[4] - 1)
    mp.setattr(QC, "windows", shifted)


def _m_clip_pre_unclamped(mp):
    clamp, take = CC.clamp, CC.clip_bytes

    def unclamped(bs, have_prev, a, e):
        if not have_prev or a >= -bs or e <= a:
            return clamp(bs, have_prev, a, e)
        t0, t1 = a // 8 * 8, -(-min(e, bs) // 8) * 8
        return (t0, t1 - t0, CC.CUT_START | (CC.CUT_END if e > bs else 0) | CC.FROM_PREV) if t1 > t0 else None

    def padded(cur_row, prev_row, t0, n):
        bs = cur_row.size // 2
        if prev_row is None or t0 >= -bs:
            return take(cur_row, prev_row, t0, n)
        return np.concatenate([np.zeros(2 * (-bs - t0), np.uint8), take(cur_row, prev_row, -bs, n - (-bs - t0))])
    mp.setattr(CC, "clamp", unclamped)
    mp.setattr(CC, "clip_bytes", padded)


def _m_owed_not_carried(mp):
    orig = CC.requests
    mp.setattr(CC, "requests", lambda *a: orig(*a[:8], None, *a[9:]))


def _m_replay_whole_clip(mp):
    orig = CR.own_direction
    mp.setattr(CR, "own_direction", lambda clip, rng, sl, n_sym, whole_clip=False: orig(clip, rng, sl, n_sym, True))


MUTANTS = {
    "a margin tie goes to the larger tau": ("decode", _m_tie),
    "the candidate range is one output short at its lower end": ("decode", _m_range_lo),
    "the candidate range is one output short at its upper end": ("decode", _m_range_hi),
    "look-back is ignored": ("decode", _m_no_look_back),
    "look-back is taken without a prev": ("decode", _m_look_back_without_prev),
    "the region threshold is one window too high": ("decode", _m_need_one_window_more),
    "long_runs counts at >= MAX_W": ("decode", _m_long_runs_at_max),
    "repair ranks by the wrong end of |s|": ("decode", _m_rank_wrong_end),
    "the narrow grid point is rounded the other way": ("decode", _m_grid_other_way),
    "an expectation's window is clipped at t_hi - 1": ("expect", _m_expect_t_hi),
    "the search keeps the last 4 rows": ("search", _m_search_last_four),
    "the quality noise window is shifted by one output": ("quality", _m_quality_noise_shift),
    "clip pre is not clamped at the start of prev": ("clips", _m_clip_pre_unclamped),
    "owed is not carried": ("clips", _m_owed_not_carried),
    "the replay region is summed over the whole clip": ("replay", _m_replay_whole_clip),
}


def _expected(ch, family):
    """The bytes of every expected slot of one family of a scene, rebuilt now - under whatever patch is in force - from
    the scene and the baseline's upstream rows; None where the family does not apply."""
    sc = ch.scene
    if family == "decode":
        L = ch.decode
        out = [a for r in range(3) for a in RP.slot_model(L, r)]
        if sc.sl >= NB.MIN_SL:
            out += [a for r in range(3) for a in NB.slot_model(L, r)]
        return b"".join(a.tobytes() for a in out)
    if family == "expect":
        X = S.make_expect(sc)
        return b"".join(a.tobytes() for form in X.forms() for a in X.want(*form))
    if family == "search":
        F = S.make_search(sc)
        return None if F is None else b"".join(a.tobytes() for a in F.want())
    if family == "quality":
        return S.make_quality(sc, *ch.fed).want.tobytes()
    if family == "clips":
        return S.make_clips(sc, *ch.runs, *ch.fed, ch.expect.want(*sc.feed_form), None if ch.search is None else ch.search.want()).want.tobytes()
    R = S.make_replay(sc, ch.clips.want)
    return None if R is None else b"".join(a.tobytes() for form in R.forms() for a in R.want(*form))


def _own(ch, family):
    """The same bytes from the chain's own launches: what the device tests compare with."""
    sc = ch.scene
    if family == "decode":
        L = ch.decode
        return b"".join(a.tobytes() for a in [a for r in range(3) for a in L.want[r]] + ([a for r in range(3) for a in L.narrow[r]] if sc.sl >= NB.MIN_SL else []))
    if family == "expect":
        return b"".join(a.tobytes() for form in ch.expect.forms() for a in ch.expect.want(*form))
    if family == "search":
        return None if ch.search is None else b"".join(a.tobytes() for a in ch.search.want())
    if family in ("quality", "clips"):
        return getattr(ch, family).want.tobytes()
    return None if ch.replay is None else b"".join(a.tobytes() for form in ch.replay.forms() for a in ch.replay.want(*form))


def test_the_rebuilt_slots_are_the_chains_own(chains):
    """_expected with no patch in force gives the slots the device tests compare with (a third of the seeds, every family);
    so does the restated decode_run with no deviation switched on."""
    for ch in chains[::3]:
        for family in S.FAMILIES[1:]:
            assert _expected(ch, family) == _own(ch, family), (ch.seed, family)
    with pytest.MonkeyPatch.context() as mp:
        _patch_decode_run(mp)
        for ch in chains[::3]:
            assert _expected(ch, "decode") == _own(ch, "decode"), (ch.seed, "restated decode_run")


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_mutant_changes_a_scene(chains, name):
    family, apply = MUTANTS[name]
    with pytest.MonkeyPatch.context() as mp:
        apply(mp)
        for ch in chains:
            if _expected(ch, family) != _own(ch, family):
                print(f"\n[burst sweep] mutant '{name}': seed {ch.seed} is the first scene whose {family} slot changes")
                return
    raise AssertionError(f"no scene of SEEDS tells the mutant '{name}' from the model: the draw is too tame")


def test_region_threshold_off_by_one_changes_nothing():
    """t1 - t0 is a multiple of 128 (with or without the look-back, itself a multiple of 128).  N SL + 1 is odd, so the
    threshold one higher rejects nothing more; one lower admits t1 - t0 = N SL, whose candidate range t0 + SL <= tau <
    t1 - SL (N - 1) = t0 + SL is empty."""
    for n, sl in S.SHAPES:
        need = n * sl + 1
        assert need % 2 == 1 and need % W != 0 and DC.shape(DC.config(sl, n, 4096))[3] % W == 0
        t0, t1 = 0, n * sl
        assert len(range(t0 + sl, t1 - sl * (n - 1))) == 0
