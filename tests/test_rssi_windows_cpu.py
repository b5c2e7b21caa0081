"""CPU side of the RSSI / SNR window cases (tests/rssi_window_cases.py): the oracle reports exactly the planted records,
every position class and residue is there, every power step sits at the window index it is meant for (from the oracle's
own filter output), both routes' NumPy models agree with the oracle within half the documented tolerance on every
record, and every way to be wrong listed in MUTANTS is told apart from the oracle by more than the tolerance on a named
case - or is proved unable to change any value.  pytest -s prints the figures profiles/rssi_windows.txt records."""
import collections
import math

import numpy as np
import pytest

import rssi_window_cases as RW
import tail_dense_cases as TD
from oracle import c_oracle as CO

B, PL = RW.B, RW.PL
MODEL_TOL = 5e-4        # half of the 1e-3 dB the device is held to: the rest is the wave sum's order and v_log_f32
KILL = 1e-3


@pytest.fixture(scope="module")
def cs():
    return RW.cases()


def _want(cs, k):
    return float(cs.recs[k]["rssi"]), float(cs.recs[k]["snr"])


def _power(raw):
    """|filtered|^2 per call of the oracle: p[c][j] = |f[c B + j - 1]|^2, j in [0, B]."""
    filt, _, _ = CO.stages(raw)                       # filt[i] = f[i - 1]
    p = np.abs(filt) ** 2
    return [p[c * B: c * B + B + 1] for c in range(RW.N_BLOCKS)]


# ------------------------------------------------------------------------------------------------ the plants
def test_oracle_reports_exactly_the_planted_records(cs):
    assert 100 <= cs.n_streams <= 170 and cs.raw.shape == (cs.n_streams, 2 * RW.N_SAMPLES)
    for s in range(cs.n_streams):
        got = sorted((p.call, p.index) for p in cs.pk[s])
        assert got == cs.planted[s], (cs.order[s], got, cs.planted[s])
    assert [(int(r["stream"]), int(r["call"]), int(r["index"])) for r in cs.recs] == [(r.stream, r.call, r.q) for r in cs.records]
    assert all(int(r["nbytes"]) == 10 for r in cs.recs)
    # the usual inputs put every expected value near -31 dB and 0 dB; these span the whole range
    assert cs.recs["rssi"].min() < -81 and cs.recs["rssi"].max() > -2
    assert cs.recs["snr"].min() < -70 and cs.recs["snr"].max() > 70


def test_generic_configuration_reports_the_same_positions(cs):
    """packet_symbols = 72 slices nine bytes at the same positions: the same (stream, call, q), other bytes."""
    g = RW.generic_recs()
    assert [(int(r["stream"]), int(r["call"]), int(r["index"])) for r in g] == [(r.stream, r.call, r.q) for r in cs.records]
    assert all(int(r["nbytes"]) == 9 for r in g)
    assert np.array_equal(g["rssi"], cs.recs["rssi"]) and np.array_equal(g["snr"], cs.recs["snr"], equal_nan=True)


def test_call_0_holds_no_record(cs):
    """Position 0 is the only one call 0 could report (as q = B), and bit 0 of a stream is never the preamble's 1."""
    assert TD.PRE[0] == 1 and _buffer_length() == 2 * B
    assert not (cs.bits[:, 0] & 1).any()
    loud = np.random.default_rng(5).integers(0, 256, (4, 2 * RW.N_SAMPLES), dtype=np.uint8)
    _, bits = CO.demod_batch(loud, CO.make_cfg(block_size=B), threads=2, want_bits=True)
    assert not (bits[:, 0] & 1).any()
    assert cs.recs["call"].min() == 1 and (1, 2) in {(r.call, r.q) for r in cs.records}


def _buffer_length():
    return TD.oracle_cfg().buffer_length


def test_every_position_class_and_residue(cs):
    planted = [r for r in cs.records if r.planted]
    by_cls = collections.defaultdict(set)
    for r in cs.records:
        by_cls[r.cls].add((r.call, r.q))
    assert set(by_cls) == set(RW.CLASSES)
    res = lambda call, q: RW.window(call, q)["t_lo"] % 4
    interior = {res(c, q) for c, q in by_cls["interior"]}
    assert interior == {0, 1, 2, 3} and all(c == 1 and PL < q < B - PL for c, q in by_cls["interior"])
    # lower clip: ns = 0; a noise window of one sample, an empty one, the last clipped and the first unclipped q
    low = by_cls["lower"]
    assert all(RW.window(c, q)["ns"] == 0 or q == PL + 1 for c, q in low)
    assert {(2, 0), (2, 1), (1, PL), (1, PL + 1)} <= low and (1, B) in by_cls["upper"]
    # upper clip in a middle call: pe = B + 1, the signal window down to one sample
    up = by_cls["upper"]
    assert all(c == 1 for c, _ in up) and sum(1 for c, q in up if q + PL > B + 1) >= 3
    assert any(q + PL == B + 1 for _, q in up) and any(q + PL < B + 1 for _, q in up)
    # the end of the stream, both sides of A + 512 <= n, in the LAST call
    last = RW.N_BLOCKS - 1
    mat, fp = by_cls["end_matrix"], by_cls["end_fp32"]
    assert all(c == last and RW.route(c, q) == "matrix" and q > RW.FIRST_FP32_Q - 32 for c, q in mat)
    assert all(c == last and RW.route(c, q) == "fp32" for c, q in fp) and (last, RW.FIRST_FP32_Q) in fp and (last, B) in fp
    assert RW.route(last, RW.FIRST_FP32_Q - 1) == "matrix" and RW.route(last, RW.FIRST_FP32_Q) == "fp32"
    res_mat = sorted({res(c, q) for c, q in mat})
    res_fp = sorted({res(c, q) for c, q in fp if q < RW.FIRST_FP32_Q + 4})
    assert len(res_mat) >= 2 and len(res_fp) >= 2
    # both parities of the oracle's choice of phase
    assert any(r.q % 14 == 0 for r in planted) and any(r.q % 14 == 1 for r in planted)
    # every content in every class
    have = {(r.cls, r.content) for r in planted}
    assert have == {(c, k) for c in RW.CLASSES for k in RW.CONTENTS}, {(c, k) for c in RW.CLASSES for k in RW.CONTENTS} - have
    routes = collections.Counter(RW.route(r.call, r.q) for r in cs.records)
    print(f"\n{cs.n_streams} streams, {len(cs.records)} records: {dict(routes)}; t_lo mod 4 interior {sorted(interior)}, last "
          f"matrix-route positions {sorted(mat)} -> {res_mat}, first fp32-route positions "
          f"{sorted(p for p in fp if p[1] < RW.FIRST_FP32_Q + 4)} -> {res_fp}")


def test_which_ok_conditions_the_batch_path_reaches():
    """Of rd_rssi_prepare's four conditions only the one on the stream's end can fail: every (call, q) of every call
    that can hold a record.  The same sweep bounds the outputs a window needs: at most A + 451 of the 512 a block has, and
    no sample past n - 2."""
    n = RW.N_SAMPLES
    reach, fails = 0, collections.Counter()
    for call in range(1, RW.N_BLOCKS):
        for q in range(B + 1):
            w = RW.window(call, q)
            fails["t_lo"] += not w["t_lo"] >= 1
            fails["valid_from"] += not w["A"] - 8 >= 0
            fails["t_hi"] += not w["t_hi"] <= w["A"] + 512
            fails["end"] += not w["A"] + 520 <= n + 8
            reach = max(reach, w["t_hi"] - w["A"])
            assert w["A"] % 4 == 0 and w["A"] + 1 <= w["t_lo"] <= w["A"] + 4 and w["t_hi"] - 1 <= n - 2
            if call == RW.N_BLOCKS - 1:
                assert w["ok"] == (q < RW.FIRST_FP32_Q)
            else:
                assert w["ok"]
    assert fails == {"t_lo": 0, "valid_from": 0, "t_hi": 0, "end": B + 1 - RW.FIRST_FP32_Q} and reach == 451
    # what rd_rssi_fetch loads on the matrix route: samples A - 8 .. A + 511, inside the stream exactly when ok
    assert RW.window(RW.N_BLOCKS - 1, RW.FIRST_FP32_Q - 1)["A"] + 511 == n - 1
    print(f"\nok: t_lo, valid_from and t_hi never fail; the stream's end fails for q >= {RW.FIRST_FP32_Q} of the last call; "
          f"t_hi - A <= {reach}")


def test_k_tail_group_alternates_routes(cs):
    """The first group of four streams: more records than k_tail has waves, and record r and r + 4 - one wave's
    consecutive jobs - on different routes, in both orders."""
    g = [r for r in cs.records if r.stream < TD.GROUP]
    routes = [RW.route(r.call, r.q) for r in g]
    assert len(g) > 4 and all(routes[k] != routes[k + 4] for k in range(len(g) - 4))
    firsts = {routes[k] for k in range(len(g) - 4)}
    assert firsts == {"matrix", "fp32"}
    # and the windows of one wave's two jobs hold different contents: stale bytes would show
    assert all(g[k].content != g[k + 4].content for k in range(len(g) - 4))
    # the other streams: routes in turn, so that any assignment of consecutive tasks to a wave changes route often
    rest = [RW.route(r.call, r.q) for r in cs.records if r.stream >= TD.GROUP]
    changes = sum(1 for a, b in zip(rest, rest[1:]) if a != b)
    assert changes >= 60, changes
    print(f"\ngroup 0: {routes}; route changes between consecutive records of the other streams: {changes}")


# ------------------------------------------------------------------------------------------------ the steps
def test_steps_sit_at_their_index(cs):
    """From the oracle's f: below / above the stated window index the two sides differ by at least 40 dB, the output at
    the index itself included - the first loud output (or the first quiet one) is exactly that index."""
    seen = collections.Counter()
    for r in cs.records:
        if not r.planted or r.content not in RW.STEPS:
            continue
        p = _power(cs.raw[r.stream])[r.call]
        idx, loud_above = RW.step_index(r.content, r.call, r.q)
        w = RW.window(r.call, r.q)
        lo, hi = max(w["ns"] - 8, 0), min(w["pe"] + 8, B + 1)
        below, above = p[lo: idx], p[idx: hi]
        if r.content == "step_ns":            # the loud side lies before the block for ns = 0: the previous call's output
            if idx == 0:
                below = _power(cs.raw[r.stream])[r.call - 1][B - 8: B]     # filtered[B] of call c - 1 is filtered[0] of c
                below = below[:-1] if len(below) else below
            lo = idx - len(below)
        quiet, loud = (below, above) if loud_above else (above, below)
        if not len(loud) or not len(quiet):
            seen[(r.content, "one side outside the block")] += 1
            continue
        db = lambda x: 10 * math.log10(x)
        edge_loud = loud[0] if loud_above else loud[-1]
        assert db(edge_loud) - db(quiet.max()) >= 40, (r.name, db(edge_loud), db(quiet.max()))
        assert db(loud.mean()) - db(quiet.max()) >= 40, r.name
        assert db(quiet.max()) < -81, (r.name, db(quiet.max()))
        seen[(r.content, r.cls)] += 1
    for c in RW.STEPS:
        assert sum(v for (k, cl), v in seen.items() if k == c and cl in RW.CLASSES) >= 5, (c, seen)
    print(f"\nsteps proved at their index: {dict(seen)}")


# ------------------------------------------------------------------------------------------------ the models
def test_models_agree_with_the_oracle(cs):
    worst = {}
    for k, r in enumerate(cs.records):
        rt = RW.route(r.call, r.q)
        got, want = RW.model(cs.raw[r.stream], r.call, r.q), _want(cs, k)
        d_r = abs(got[0] - want[0])
        d_s = 0.0 if math.isnan(got[1]) and math.isnan(want[1]) else abs(got[1] - want[1])
        assert RW.db_diff(got, want) <= MODEL_TOL, (r.name, rt, got, want)
        # the other route's arithmetic on the same record (the matrix model needs real bytes only)
        other = (RW.model_fp32 if rt == "matrix" else RW.model_matrix)(cs.raw[r.stream], r.call, r.q)
        assert RW.db_diff(other, want) <= MODEL_TOL, (r.name, "other route", other, want)
        key = (rt, r.content)
        w = worst.setdefault(key, [0.0, "", 0.0, ""])
        if d_r >= w[0]:
            w[0], w[1] = d_r, r.name
        if d_s >= w[2]:
            w[2], w[3] = d_s, r.name
    print("\n|model - oracle| in dB: route content  rssi (case)  snr (case)")
    for (rt, c), w in sorted(worst.items()):
        print(f"  {rt:6s} {c:10s}  {w[0]:.3e} ({w[1]})  {w[2]:.3e} ({w[3]})")
    assert {rt for rt, _ in worst} == {"matrix", "fp32"}
    # the weakest level: a constant-127 window costs the quantised taps a fifth of the tolerance, the fp32 route a thirtieth
    assert 1e-4 < worst[("matrix", "quiet")][0] < 3e-4 and worst[("fp32", "quiet")][0] < 1e-4


EQUIVALENT = {
    "511 outputs": "a window's outputs end at A + 451 (test_which_ok_conditions_the_batch_path_reaches): output A + 512 "
                   "is never inside a window",
    "ok off by one": "the outputs of a window use samples up to n - 2 on either route: the four samples of the next "
                     "stream that the last column would load feed masked outputs only; the condition guards the loads",
}


def _mutant_values(cs, mutant):
    """[(record, figures)] of the mutated model over every record it applies to."""
    out = []
    if mutant == "stale prefetch":
        # one wave of k_tail takes records r and r + 4 of a group: the second job computed from the first one's bytes
        g = [(k, r) for k, r in enumerate(cs.records) if r.stream < TD.GROUP]
        rest = [(k, r) for k, r in enumerate(cs.records) if r.stream >= TD.GROUP]
        # (the other streams: consecutive records, as a wave of k_rssi_u8 on a short grid would take them)
        for (_, a), (k, b) in list(zip(g, g[4:])) + list(zip(rest, rest[1:])):
            if RW.route(b.call, b.q) == "matrix" and RW.route(a.call, a.q) == "fp32":
                out.append((k, b, RW.model_matrix(cs.raw[b.stream], b.call, b.q, stale=(cs.raw[a.stream], a.call, a.q))))
        return out
    for k, r in enumerate(cs.records):
        if mutant == "A not rounded" and RW.route(r.call, r.q) != "matrix":
            continue
        nxt = cs.raw[(r.stream + 1) % cs.n_streams]
        out.append((k, r, RW.model(cs.raw[r.stream], r.call, r.q, mutant, next_raw=nxt)))
    return out


@pytest.mark.parametrize("mutant", RW.MUTANTS)
def test_every_mutant_is_told_apart(cs, mutant):
    vals = _mutant_values(cs, mutant)
    assert vals
    diffs = [(RW.db_diff(v, _want(cs, k)), r.name) for k, r, v in vals]
    worst = max(diffs)
    if mutant in EQUIVALENT:
        assert worst[0] <= MODEL_TOL
        if mutant == "511 outputs":
            assert all(v == RW.model(cs.raw[r.stream], r.call, r.q) for _, r, v in vals)
        else:   # the first fp32-side positions move to the matrix route, whose figures do not depend on the bytes past n
            moved = [(r, v) for _, r, v in vals if RW.route(r.call, r.q) == "fp32" and RW.route(r.call, r.q, RW.N_SAMPLES + 4) == "matrix"]
            assert len(moved) >= 8 and {RW.window(r.call, r.q)["t_lo"] % 4 for r, _ in moved} == {0, 1, 2, 3}
            assert all(v == RW.model(cs.raw[r.stream], r.call, r.q, mutant) for r, v in moved)     # (zeros past n)
        how = ("the unmutated model's figures bit for bit on every case" if mutant == "511 outputs" else
               f"{len(moved)} records move to the matrix route, none further than {worst[0]:.2e} dB from the oracle, whatever lies past the stream")
        print(f"\n{mutant}: cannot be told apart - {how} ({EQUIVALENT[mutant]})")
        return
    killed = [(d, n) for d, n in diffs if d > KILL]
    assert killed, (mutant, worst)
    by_route = collections.defaultdict(list)
    for (d, n), (_, r, _) in zip(diffs, vals):
        if d > KILL:
            by_route[RW.route(r.call, r.q)].append((d, n))
    print(f"\n{mutant}: told apart on {len(killed)} of {len(vals)} records; " +
          "; ".join(f"{rt}: {max(v)[1]} by {max(v)[0]:.3g} dB" for rt, v in sorted(by_route.items())))
    # (the floor and the divide are rd_rssi_finish's, one copy for both routes; A and the prefetch are the matrix route's)
    if mutant not in ("A not rounded", "stale prefetch", "floor 0", "divide by PL"):
        assert set(by_route) == {"matrix", "fp32"}, (mutant, "one route's copy of this line is not covered", dict(by_route))


def test_a_not_rounded_needs_the_residues(cs):
    """The unrounded A is told apart at every residue but the one where rounding changes nothing."""
    per = collections.defaultdict(float)
    for k, r, v in _mutant_values(cs, "A not rounded"):
        per[(RW.window(r.call, r.q)["t_lo"] - 1) % 4] = max(per[(RW.window(r.call, r.q)["t_lo"] - 1) % 4], RW.db_diff(v, _want(cs, k)))
    assert per[0] <= MODEL_TOL and all(per[m] > KILL for m in (1, 2, 3)), dict(per)


def test_streamed_oracle_gives_the_batch_records(cs):
    """OracleDemodulator block by block over the streams the device test feeds block by block: the batch oracle's
    records (the whole-stream formulation is the same computation), every class and content among them."""
    subset = RW.streamed_subset()
    assert 30 <= len(subset) <= 60
    seen = set()
    for s in subset:
        calls = RW.streamed_calls(s)
        flat = [(c, p) for c, pk in enumerate(calls) for p in pk]
        want = cs.recs[cs.recs["stream"] == s]
        assert [(c, p[0], p[1]) for c, p in flat] == [(int(r["call"]), int(r["index"]), bytes(r["data"][:10]).hex()) for r in want]
        for (c, p), r in zip(flat, want):
            assert RW.db_diff(p[2:], (float(r["rssi"]), float(r["snr"]))) <= 1e-9, (cs.order[s], p, r)
        seen |= {(r.cls, r.content) for r in cs.records if r.stream == s}
    assert seen == {(c, k) for c in RW.CLASSES for k in RW.CONTENTS}


def test_rssi_u8_grid_has_a_wave_per_record_below_its_clamp(cs):
    """Why the device test reaches k_rssi_u8's second and third job per wave with a large batch and not with a short
    match list: the grid is min(ceil(match_cap / 4), 1024) workgroups of four waves (rd_launch_slice, rd_slice_grid) - at
    least match_cap waves below the clamp -, a run that keeps its results has matches <= match_cap, and its tasks are the
    surviving matches and one more per match on a block boundary.  With about 13 raw matches per burst, records stay
    far below matches; only the clamp's 4096 waves can be outnumbered."""
    waves = lambda cap: 4 * min(max((cap + 3) // 4, 1), 1024)
    assert all(waves(c) >= min(c, 4096) for c in range(1, 20000)) and waves(10 ** 6) == 4096
    raw_matches = sum(int((TD.positions(np.unpackbits(b, bitorder="little")[: RW.N_SAMPLES]) <= 2 * B).sum()) for b in cs.bits)
    assert raw_matches >= 5 * len(cs.recs)
    import test_rssi_windows as GT
    assert GT.RSSI_WAVES == waves(10 ** 6) and GT.TILES * len(cs.recs) > 2 * GT.RSSI_WAVES
    print(f"\n{raw_matches} raw matches for {len(cs.recs)} records; {GT.TILES} copies: {GT.TILES * len(cs.recs)} records on {GT.RSSI_WAVES} waves")
