"""CPU side of the dense tail cases (tests/tail_dense_cases.py): every condition under which the device test's batches
work k_tail's lists, lane rounds, twins and record loop - on the oracle's evidence alone - and the comparison's teeth: a
NumPy re-slicer of the oracle's bits (search -> calls -> bytes -> order -> dedupe) that equals the C oracle's records
on every batch, and whose mutants - each one a way for the kernel to be wrong - each differ on a named batch.  The
figures DESIGN section 5.2 quotes are printed (pytest -s)."""
import collections

import numpy as np
import pytest

import tail_dense_cases as TD

B, NB, S = TD.B, TD.N_BLOCKS, TD.S
HI = TD.last_position()


@pytest.fixture(scope="module", params=TD.NAMES)
def any_batch(request):
    return TD.batch(request.param)


# ------------------------------------------------------------------------------------------------ the re-slicer
def tasks_of(bits, mutant=None, nb=NB):
    """[(call, q, position, slot)] of one stream: slot = the match's rank by position (the order in which one search
    wave fills a list); raw = matches up to last_position()."""
    hi = TD.last_position(nb)
    pos = TD.positions(bits)
    raw = pos[pos <= (hi + S if mutant == "beyond p_hi" else hi)]
    out = []
    for slot, p in enumerate(raw.tolist()):
        if mutant == "slot 32 lost" and slot == TD.LIST_MIN - 1:
            continue
        if mutant == "slots >= 64 lost" and slot >= TD.LANES:
            continue
        b, q = p // B + 1, p % B
        if b < nb:
            if not (q == 0 and mutant == "q = 0 twin dropped"):
                out.append((b, q, p, slot))
        elif p > hi:                                  # (only the mutant gets here)
            out.append((nb - 1, p - (nb - 2) * B, p, slot))
        if q == 0 and b - 1 < nb and mutant != "q = B twin dropped":
            out.append((b - 1, B, p, slot))
    return out, len(raw)


def reslice(bits, mutant=None, nb=NB):
    """[(call, index, bytes)] of one stream in the reference's order, and the raw match count."""
    tasks, raw = tasks_of(bits, mutant, nb)
    key = (lambda t: (t[0], t[1])) if mutant == "position-major" else (lambda t: (t[0], t[1] % S, t[1]))
    tasks.sort(key=key)
    out, seen = [], set()
    if mutant == "lowest position wins":
        low = {}
        for b, q, p, _ in tasks:
            k = (b, TD.bytes_at(bits, p))
            low[k] = min(low.get(k, q), q)
        return [(b, q, TD.bytes_at(bits, p)) for b, q, p, _ in tasks if low[(b, TD.bytes_at(bits, p))] == q], raw
    for b, q, p, _ in tasks:
        data = TD.bytes_at(bits, p)
        k = data if mutant == "dedupe across calls" else (b, data)
        if k in seen:
            continue
        seen.add(k)
        out.append((b, q, data))
    return out, raw


def reslice_batch(bt, mutant=None):
    recs, raws = [], []
    for s in range(bt.n_streams):
        r, raw = reslice(bt.unpacked(s), mutant, bt.n_blocks)
        recs += [(s,) + x for x in r]
        raws.append(raw)
    if mutant == "records >= 256 of a group lost":
        per = collections.Counter()
        kept = []
        for r in recs:
            per[r[0] // TD.GROUP] += 1
            if per[r[0] // TD.GROUP] <= 256:
                kept.append(r)
        recs = kept
    return recs, raws


def oracle_tuples(bt):
    return [(int(r["stream"]), int(r["call"]), int(r["index"]), bytes(r["data"][: int(r["nbytes"])])) for r in bt.recs]


def test_reslicer_equals_the_oracle(any_batch):
    recs, raws = reslice_batch(any_batch)
    assert recs == oracle_tuples(any_batch)
    assert raws == any_batch.raw_matches.tolist()       # (dsp_oracle.search over the whole stream: another search)
    assert any_batch.raw.shape == (any_batch.n_streams, 2 * any_batch.n_samples) and 4 <= any_batch.n_streams <= 16
    assert (any_batch.counts < 1100).all()               # the oracle's per-stream array was never full
    per = collections.Counter((int(r["stream"]), int(r["call"])) for r in any_batch.recs)
    print(f"\n{any_batch.name}: raw matches {any_batch.raw_matches.tolist()}, records {any_batch.counts.tolist()}, "
          f"most records in one call {max(per.values())}, list size {any_batch.list_size()}")


MUTANTS = {   # mutant: the batch on which it must differ from the oracle
    "position-major": "rounds",
    "lowest position wins": "rounds",
    "dedupe across calls": "twins",
    "q = B twin dropped": "twins",
    "q = 0 twin dropped": "twins",
    "beyond p_hi": "geometry",
    "slot 32 lost": "full_list_a",
    "slots >= 64 lost": "rounds",
    "records >= 256 of a group lost": "many_records",
}


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_differs_on_its_batch(mutant):
    bt = TD.batch(MUTANTS[mutant])
    recs, raws = reslice_batch(bt, mutant)
    assert recs != oracle_tuples(bt), mutant
    if mutant == "beyond p_hi":
        assert raws != bt.raw_matches.tolist()           # the match count the device test compares differs as well
    if mutant == "slots >= 64 lost":   # on both of the batch's long streams
        for s in (1, 3):
            assert reslice(bt.unpacked(s), mutant)[0] != reslice(bt.unpacked(s))[0], s


# ------------------------------------------------------------------------------------------------ the conditions
def test_shape_is_one_k_tail_accepts():
    """rd_launch_tail_fused: the bits' stride a multiple of four words, the last reported position's 16-word window
    inside the stream; rd_ord_bucket_cap (rd_host.cpp) gives these streams the shortest lists."""
    stride = (TD.N_SAMPLES + 31) // 32
    assert stride % 4 == 0 and HI == (NB - 1) * B and HI // 32 + 16 <= stride
    want = (4 * TD.N_SAMPLES + 65535) // 65536 + 12
    assert max(((want + 31) // 32) * 32, TD.LIST_MIN) == TD.LIST_MIN
    assert TD.list_from_length(TD.N_SAMPLES) == TD.LIST_MIN and TD.list_from_length(33 * B) == 32 and TD.list_from_length(330 * B) == 192
    for name in TD.NAMES:
        if not name.startswith("long_"):
            assert TD.batch(name).n_blocks == NB and TD.batch(name).raw.nbytes <= 16 * NB * B * 2


def test_long_96():
    """The route to a long list without growth: rd_ord_bucket_cap gives 105 blocks 96 entries."""
    bt = TD.batch("long_96")
    n = bt.n_samples
    assert TD.list_from_length(n) == 96 == bt.list_size()
    hi = TD.last_position(bt.n_blocks)
    assert ((n + 31) // 32) % 4 == 0 and hi // 32 + 16 <= (n + 31) // 32
    assert 65 <= bt.raw_matches[1] <= 96 and 65 <= bt.raw_matches[3] <= 96
    calls = {int(r["call"]) for r in bt.stream_recs(3)}
    assert len(calls) >= 5 and min(calls) <= 2 and max(calls) >= 100     # records from one end of the stream to the other
    print(f"\nlong_96: raw matches {bt.raw_matches.tolist()}, records {bt.counts.tolist()}")


def test_full_list():
    a, b = TD.batch("full_list_a"), TD.batch("full_list_b")
    assert a.raw_matches[:4].tolist() == [32, 0, 31, 32] and b.raw_matches[:4].tolist() == [32, 0, 33, 32]
    assert a.counts[1] == 0 and b.counts[1] == 0
    assert a.raw_matches.max() == 32 and a.list_size() == 32 and b.list_size() == 64
    keep = [s for s in range(a.n_streams) if s != 2]
    assert np.array_equal(a.raw[keep], b.raw[keep]) and not np.array_equal(a.raw[2], b.raw[2])
    for bt in (a, b):
        assert bt.n_streams == 10 and bt.n_streams % TD.GROUP == 2      # a ragged last group ...
        assert (bt.counts[8:] > 0).all() and (bt.counts[4:8] > 0).all()  # ... that holds records, behind a full one
        assert (bt.counts[[0, 2, 3]] >= 8).all()
        assert any(r[2] for calls in bt.calls() for rows in calls for r in rows)      # a CRC-valid message
        assert all(abs(r[5] - round(r[5])) >= 1e-6 for calls in bt.calls() for rows in calls for r in rows if r[2])
    # the 32nd match of a full list is one whose loss shows: a record of its own in at least one of the full streams
    shows = []
    for s in (0, 3, 9):
        p = int(TD.positions(a.unpacked(s))[31])
        shows.append(any((int(r["call"]) - 1) * B + int(r["index"]) == p for r in a.stream_recs(s)))
    assert any(shows), shows
    print(f"\nfull_list: a {a.raw_matches.tolist()} -> {a.counts.tolist()} records, b {b.raw_matches.tolist()} -> {b.counts.tolist()}")


def test_ladder():
    lo = {64: 33, 128: 65, 256: 129, 512: 257}
    fig = {}
    for key in (64, 128, 256, 512, "over"):
        bt = TD.batch(f"ladder_{key}")
        n = int(bt.raw_matches[1])
        fig[key] = (n, int(bt.counts[1]))
        assert bt.raw_matches.argmax() == 1 and np.delete(bt.raw_matches, 1).max() <= 16 and bt.raw_matches[3] == 0
        if key == "over":
            assert n > TD.LIST_MAX
        else:
            assert lo[key] <= n <= key and bt.list_size() == key
    assert TD.batch("ordinary").raw_matches.max() <= 16 and TD.batch("ordinary").counts.sum() > 0
    print(f"\nladder (raw matches, records) of the train: {fig}")


def _dedupe_facts(bits):
    """Over the calls of one stream: duplicates whose surviving first occurrence sits in another round of 64 slots
    (slots by position), and duplicates beaten by a first occurrence at a higher position."""
    tasks, _ = tasks_of(bits)
    tasks.sort(key=lambda t: (t[0], t[1] % S, t[1]))
    first, other_round, higher = {}, 0, 0
    for b, q, p, slot in tasks:
        k = (b, TD.bytes_at(bits, p))
        if k not in first:
            first[k] = (p, slot)
            continue
        fp, fslot = first[k]
        other_round += fslot // TD.LANES != slot // TD.LANES
        higher += fp > p
    return other_round, higher


def test_rounds():
    bt = TD.batch("rounds")
    n1, n3 = int(bt.raw_matches[1]), int(bt.raw_matches[3])
    assert 65 <= n1 <= 128 and 257 <= n3 <= 512 and bt.list_size() == 512
    assert TD.list_size(n1) == 128 and -(-n3 // TD.LANES) >= 5
    facts = {s: _dedupe_facts(bt.unpacked(s)) for s in (1, 3)}
    for s in (1, 3):
        assert facts[s][0] >= 1 and facts[s][1] >= 1, (s, facts)
    per = collections.Counter((int(r["stream"]), int(r["call"])) for r in bt.recs)
    assert max(per.values()) >= 12
    print(f"\nrounds: {n1} and {n3} raw matches; duplicates with their first occurrence in another round of 64 slots "
          f"{facts[1][0]} and {facts[3][0]}, beaten by a higher position {facts[1][1]} and {facts[3][1]}; "
          f"most records in one call {max(per.values())}")


def twin_classes(bt, s):
    """Per match position p = k B of stream s: (p, class) with class 'both' ((k, B) and (k + 1, 0) are records), 'B
    deduped' ((k, B) lost to an earlier same-bytes match of call k), 'last' (p = last_position(): no call k + 1);
    and whether the (k + 1, 0) record beats a later same-bytes match of call k + 1."""
    bits = bt.unpacked(s)
    pos = TD.positions(bits)
    pos = pos[pos <= HI]
    rec = {(int(r["call"]), int(r["index"])) for r in bt.stream_recs(s)}
    out = []
    for p in pos[pos % B == 0].tolist():
        k = p // B
        data = TD.bytes_at(bits, p)
        earlier = any(TD.bytes_at(bits, x) == data for x in pos[(pos >= p - B) & (pos < p)].tolist())
        later = any(TD.bytes_at(bits, x) == data for x in pos[(pos > p) & (pos <= p + B)].tolist())
        has_b, has_0 = (k, B) in rec, (k + 1, 0) in rec
        assert has_0 == (k + 1 < NB)                    # (phase 0, q 0) is the first task of its call: never a duplicate
        assert has_b == (not earlier) or not has_b      # the q = B record can only be lost to an earlier match
        out.append((p, "both" if has_b and has_0 else "B kept, last call" if has_b else "B deduped", has_0 and later))
    return out


def test_twins():
    bt = TD.batch("twins")
    found = {s: twin_classes(bt, s) for s in range(bt.n_streams)}
    flat = [c for cs in found.values() for c in cs]
    assert sum(1 for c in flat if c[1] == "both") >= 2
    assert sum(1 for c in flat if c[1] == "B deduped" and c[0] < HI) >= 2
    assert sum(1 for c in flat if c[2]) >= 2
    assert {c[0] for c in flat} == {B, 2 * B, 3 * B}     # every boundary a call starts at, the last reported position too
    assert any(c[0] == HI and c[1] == "B kept, last call" for c in flat) and any(c[0] == HI and c[1] == "B deduped" for c in flat)
    assert bt.list_size() == 128
    assert any(r[2] for calls in bt.calls() for rows in calls for r in rows)
    assert all(abs(r[5] - round(r[5])) >= 1e-6 for calls in bt.calls() for rows in calls for r in rows if r[2])
    print(f"\ntwins: raw matches {bt.raw_matches.tolist()}, (position, class, q = 0 beats a later match) per stream {found}")


def fp32_rssi(call, q):
    """Whether k_tail evaluates this record's RSSI window on its fp32 route: rd_rssi_prepare's `ok` (rd_device.h,
    the line `j.ok = t_lo >= 1 && ...`) is false when the 32 columns of the matrix form would reach outside the stream."""
    pl = TD.REP
    ns, pe = max(q - pl, 0), min(q + pl, B + 1)
    t_lo, t_hi = call * B + ns - 1, call * B + pe - 2
    a = (t_lo - 1) & ~3
    return not (t_lo >= 1 and a - 8 >= 0 and a + 16 * 31 + 24 <= TD.N_SAMPLES + 8 and t_hi <= a + 512)


def test_geometry():
    bt = TD.batch("geometry")
    def pairs(s, m, not_m=None):
        pos = TD.positions(bt.unpacked(s))
        pos = set(pos[pos <= HI].tolist())
        return [p for p in pos if p + 1 in pos and (p + 1) % m == 0 and (not_m is None or (p + 1) % not_m)]
    assert pairs(0, 8192), "no run of adjacent matches across a multiple of 8192 (two search waves on one list)"
    assert pairs(1, 128, 8192), "no run across a multiple of 128 (two lanes)"
    assert pairs(3, 32, 128), "no run across a multiple of 32 (two words of a lane)"
    pos = TD.positions(bt.unpacked(4))
    assert {HI - 1, HI, HI + 1} <= set(pos.tolist()), "the last-words mask has nothing to cut"
    beyond = int((pos > HI).sum())
    assert bt.raw_matches[4] == int((pos <= HI).sum()) and beyond >= 3
    last = bt.stream_recs(4)
    assert int(last["call"].max()) == NB - 1 and int(last[last["call"] == NB - 1]["index"].max()) <= B
    # from sample 0: matches below position 225, reported by call 1 with a noise window cut at the block's start
    early = TD.positions(bt.unpacked(5))
    early = early[early < 225]
    first = bt.stream_recs(5)
    assert len(early) >= 8 and any(r["call"] == 1 and r["index"] < 225 for r in first)
    # the fp32 RSSI route: the last call's records near the end of the stream (not the first samples' records: their
    # windows lie in block 1, inside the stream)
    routes = [fp32_rssi(int(r["call"]), int(r["index"])) for r in bt.recs]
    assert sum(routes) >= 2 and not all(routes)
    assert all(fp32_rssi(int(r["call"]), int(r["index"])) for r in last if r["call"] == NB - 1 and r["index"] > B - 64)
    assert not any(fp32_rssi(int(r["call"]), int(r["index"])) for r in first if r["call"] == 1 and r["index"] < 225)
    assert bt.list_size() == 128
    print(f"\ngeometry: raw matches {bt.raw_matches.tolist()}, {beyond} matches beyond the last position in stream 4, "
          f"matches below 225 in stream 5: {early.tolist()}, records on the fp32 RSSI route {sum(routes)} of {len(routes)}")


def test_many_records():
    bt = TD.batch("many_records")
    assert (bt.counts[:4] > 64).all() and bt.counts[:4].sum() > 256
    assert (bt.raw_matches[:4] > 64).all() and bt.raw_matches.max() <= 128 and bt.list_size() == 128
    assert (bt.counts[4:] > 0).all()                    # a group behind the long one: its first record number is > 256
    print(f"\nmany_records: raw matches {bt.raw_matches.tolist()}, records {bt.counts.tolist()}")


# ------------------------------------------------------------------------------------------------ teeth of the comparison
def _streams_swapped(want):
    """A wrong `off` inside a group: streams 1 and 2 of the first group change places."""
    a, b = want[want["stream"] == 1], want[want["stream"] == 2]
    assert len(a) and len(b)
    return np.concatenate([want[want["stream"] == 0], b, a, want[want["stream"] > 2]])


def _groups_swapped(want):
    """A wrong `first`: the second group's records in front of the first group's."""
    g = want["stream"] // TD.GROUP
    assert (g == 0).any() and (g == 1).any()
    return np.concatenate([want[g == 1], want[g == 0], want[g > 1]])


@pytest.mark.parametrize("wrong", (_streams_swapped, _groups_swapped))
@pytest.mark.parametrize("name", ("many_records", "twins"))
def test_comparison_rejects_wrong_order(name, wrong):
    want = TD.batch(name).recs
    TD.assert_records_equal(want.copy(), want, "itself", db_tol=0.0)
    got = wrong(want)
    assert got.dtype == want.dtype and len(got) == len(want)
    with pytest.raises(AssertionError):
        TD.assert_records_equal(got, want, wrong.__name__)
