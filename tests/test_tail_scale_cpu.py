"""CPU side of the tail-scale cases (tests/tail_scale_cases.py): the conditions under which the device test's batches
work k_tail's prefix loop past its first round - on the oracle's evidence alone - and the whole-array comparison the
device test uses shown to reject records that sit at wrong positions."""
import hashlib

import numpy as np
import pytest

import tail_scale_cases as TS
from oracle import dsp_oracle as O

RAW_SHA256 = "3280ac71fc3aaea8768a010c3eb03356c924c037bc922d55600e06a0ce168189"


@pytest.fixture(scope="module")
def cases():
    return TS.cases()


def test_generator_is_pinned(cases):
    assert cases.raw.shape == (TS.U + len(TS.QUIET), 2 * TS.N_SAMPLES)
    assert hashlib.sha256(cases.raw[: TS.U].tobytes()).hexdigest() == RAW_SHA256
    for u in range(TS.U):
        bursts = TS.bursts_of(u)
        assert len(bursts) == u % 4
        starts = [s for _, s, _ in bursts]
        assert all(b - a >= TS.BURST_SAMPLES for a, b in zip(starts, starts[1:]))
        assert all(s + 32 * 14 <= TS.last_position() for s in starts)   # every sync word starts at a reported position
    everything = [b for u in range(TS.U) for b in TS.bursts_of(u)]
    for k in range(3):   # payloads, starts and frequency offsets are all distinct
        assert len({bytes(b[k]) if k == 0 else b[k] for b in everything}) == len(everything)
    assert TS.U % TS.GROUP and np.gcd(TS.U, TS.GROUP) == 1


def test_the_shape_is_one_k_tail_accepts():
    """rd_launch_tail_fused: the bits' stride a multiple of four words, the last reported position's 16-word window
    inside the stream."""
    stride = (TS.N_SAMPLES + 31) // 32
    assert stride == 192 and stride % 4 == 0
    assert TS.last_position() == 13 * 512 - 2048 and TS.last_position() // 32 + 16 <= stride
    assert (2 * TS.N_SAMPLES) % 16 == 0


def test_stream_and_group_conditions(cases):
    per_stream = cases.counts[: TS.U]
    assert per_stream.min() == 0 and per_stream.max() >= 4
    # half of RD_BUCKET_MIN = 32: the first pass cannot overflow a stream's match list
    assert cases.raw_matches.max() <= 16, cases.raw_matches
    assert np.all(cases.raw_matches[TS.U:] == 0) and np.all(cases.counts[TS.U:] == 0)   # the quiet streams: no match at all
    assert np.all(cases.raw_matches[: TS.U] >= per_stream)
    for n in TS.N_STREAMS:
        totals = TS.group_totals(n)
        assert len(totals) == (n + TS.GROUP - 1) // TS.GROUP > TS.ROUND
        assert len(set(totals.tolist())) >= 5
        empty = np.flatnonzero(totals == 0)
        assert len(empty) >= 3 and TS.ROUND in empty and TS.ROUND - 1 in empty, empty
        assert totals[: TS.ROUND - 2].min() > 0   # ... and nowhere else in the first round: a stalled chain has work behind it
        assert totals.sum() == len(TS.expected_records(n))
    assert len(TS.group_totals(8197)) == 2050 and TS.group_totals(8197)[-1] == cases.counts[8196 % TS.U] > 0
    # more than one record in one call of one stream: the order inside a call is part of what is compared
    assert max(np.unique(r["call"], return_counts=True)[1].max() for r in cases.recs if len(r)) >= 3


def test_messages(cases):
    rows = [r for calls in cases.calls[: TS.U] for rs in calls for r in rs]
    assert sum(1 for r in rows if r[2]) >= 1 and sum(1 for r in rows if not r[2]) >= 1
    planted = {bytes(o).hex(): u for u in range(TS.U) if u % 4 == 1 for o, _, _ in TS.bursts_of(u)}
    seen_ok = {r[1] for r in rows if r[2]}
    seen_bad = {r[1] for r in rows if not r[2]}
    for hx, u in planted.items():   # the strong bursts arrive as planted: a message, or a packet the CRC gate refuses
        assert hx in (seen_bad if u % 3 == 0 else seen_ok), u
    # parsed() is compared exactly: no message's frequency error lies within 1e-6 Hz of an integer
    assert all(abs(r[5] - round(r[5])) >= 1e-6 for r in rows if r[2])
    # the two oracles agree on every packet (records come from the C oracle, parsed rows from parse_calls)
    for k, calls in enumerate(cases.calls):
        assert [(b, r[0], r[1]) for b, rs in enumerate(calls) for r in rs] == \
               [(p.call, p.index, bytes(p.data).hex()) for p in cases.pk[k]], k
    assert len(TS.expected_rows(4100)) == sum(sum(1 for rs in cases.calls[k] for r in rs if r[2]) for k in TS.sources(4100))


def test_raw_matches_are_the_whole_stream_search(cases):
    """raw_matches counts positions 0 .. last_position() of the whole stream; every packet of every call sits at one."""
    cfg = TS.oracle_cfg()
    for k in (1, 2, 3, 10, 35):
        bits = np.unpackbits(cases.bits[k], bitorder="little")[: TS.N_SAMPLES]
        pos = {p for p in O.search(bits, cfg) if p <= TS.last_position()}
        assert len(pos) == cases.raw_matches[k]
        at = {(p.call + 1) * TS.B - cfg.buffer_length + p.index for p in cases.pk[k]}
        assert at <= pos, k


def test_expected_records_are_the_streams_records_in_stream_order(cases):
    n = 4100
    want = TS.expected_records(n)
    parts = []
    for s, k in enumerate(TS.sources(n)):
        r = cases.recs[k].copy()
        r["stream"] = s
        parts.append(r)
    naive = np.concatenate(parts)
    assert want.dtype == naive.dtype and np.array_equal(want, naive)
    assert np.all(np.diff(want["stream"]) >= 0)
    assert TS.expected_matches(n) == sum(int(cases.raw_matches[k]) for k in TS.sources(n))
    from rtldavis_amd import batch
    assert batch.RD_PACKET_DTYPE == TS.PACKET_DTYPE
    picked = TS.bits_streams(8197)
    assert {0, 3, 4092, 4095, 4096, 4099, 4100, 4103, 8196, 97, 8148} <= set(picked) and len(picked) < 120


# ------------------------------------------------------------------------------------------------ teeth
def _group_span(want, g):
    lo = int(np.searchsorted(want["stream"], TS.GROUP * g))
    hi = int(np.searchsorted(want["stream"], TS.GROUP * (g + 1)))
    return lo, hi


def _swapped(want):
    (a0, a1), (b0, b1) = _group_span(want, 1030), _group_span(want, 1031)
    assert a1 == b0 and a1 - a0 != b1 - b0 and a1 > a0 and b1 > b0
    return np.concatenate([want[:a0], want[b0:b1], want[a0:a1], want[b1:]])


def _shifted(want):
    lo, _ = _group_span(want, TS.ROUND)
    out = want.copy()
    out[lo + 1:] = want[lo:-1]
    out[lo] = np.zeros((), dtype=want.dtype)
    return out


def _dropped(want):
    """Group 1024 itself is empty by design: the first group behind it that has records."""
    g = TS.ROUND + int(np.flatnonzero(TS.group_totals(8197)[TS.ROUND:])[0])
    lo, hi = _group_span(want, g)
    assert hi > lo
    return np.concatenate([want[:lo], want[hi:]])


def _stream_off(want):
    out = want.copy()
    out["stream"][len(out) // 2] += 4
    return out


def _rssi_off(want):
    out = want.copy()
    out["rssi"][len(out) // 3] += 2e-3
    return out


MUTATIONS = {
    "two adjacent groups' record blocks swapped": _swapped,
    "every record from group 1024 on one position late": _shifted,
    "the records of the first non-empty group of the second round dropped": _dropped,
    "one record's stream id off by 4": _stream_off,
    "an RSSI off by 2e-3 dB": _rssi_off,
}


def test_comparison_accepts_what_it_should():
    want = TS.expected_records(8197)
    near = want.copy()
    near["rssi"] += 5e-4
    near["snr"] -= 5e-4
    TS.assert_records_equal(near, want, "within the tolerance")
    TS.assert_records_equal(want.copy(), want, "itself", db_tol=0.0)


@pytest.mark.parametrize("name", MUTATIONS)
def test_comparison_rejects_misplaced_records(name):
    want = TS.expected_records(8197)
    got = MUTATIONS[name](want)
    assert got.dtype == want.dtype
    with pytest.raises(AssertionError):
        TS.assert_records_equal(got, want, name)
