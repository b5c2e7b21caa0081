"""The batch tail past 1024 stream groups (MI355X).  k_tail's workgroups wait for each other: a group of four streams
adds up the record counts of every group in front of it, 1024 per round of its prefix loop, and 1024 workgroups are
resident at once.  The batches of tests/tail_scale_cases.py have 1025 and 2050 groups: a second and a third round, a
grid that is not resident as a whole, empty groups on both sides of the round boundary.  Everything is compared with
the oracle as a whole and in order - a group's records at another group's position are what a wrong prefix gives - and
every run must stay in its first pass: a chain of waiting groups that stalls ends in overflow bit 16 and a quiet
second pass through the separate kernels, with the right records.  The conditions the inputs meet and the comparison's
teeth are checked on the CPU (tests/test_tail_scale_cpu.py)."""
import collections
import types

import numpy as np
import pytest

import parse_gate_cases as PG
import tail_scale_cases as TS

pytestmark = pytest.mark.gpu

STALLED = ("a second pass behind the one-launch tail: RD_CNT_OVF bit 16 (a group gave up waiting for the groups in front "
           "of it: k_tail's spin limit), 8 (a group's fix-up bucket) or 1 (a stream's match list)")


@pytest.fixture(scope="module")
def mods():
    from rtldavis_amd import _lib, batch, dsp
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    return batch, dsp


@pytest.fixture(scope="module")
def cases():
    return TS.cases()


@pytest.fixture(scope="module")
def want():
    """Per stream count: the batch's input, its records and its parsed rows (built once, never changed)."""
    out = {}
    for n in TS.N_STREAMS:
        raw, recs = TS.batch_input(n), TS.expected_records(n)
        raw.setflags(write=False)
        recs.setflags(write=False)
        out[n] = types.SimpleNamespace(raw=raw, recs=recs, rows=TS.expected_rows(n), matches=TS.expected_matches(n))
    return out


def _handle(mods, n_streams, parse=False):
    batch, dsp = mods
    bd = batch.BatchDemodulator(dsp.PacketConfig(19200, 14, 16, 80, PG.PREAMBLE, TS.B), n_streams, TS.N_BLOCKS)
    bd.set_parse(parse)
    return bd


def _packets_by_stream(recs):
    by = collections.defaultdict(list)
    for s, i, r, q in zip(recs["stream"].tolist(), recs["index"].tolist(), recs["rssi"].tolist(), recs["snr"].tolist()):
        by[s].append(types.SimpleNamespace(index=i, rssi=r, snr=q))
    return by


def _assert_bits(bd, cases, n_streams, what):
    src = TS.sources(n_streams)
    for s in TS.bits_streams(n_streams):
        assert np.array_equal(bd.bits(s), cases.bits[src[s]]), f"{what}: bits of stream {s} (group {s // TS.GROUP})"


@pytest.mark.parametrize("n_streams", TS.N_STREAMS)
def test_one_launch_tail_past_1024_groups(mods, cases, want, n_streams):
    """4098: 1025 groups, the last with two streams; 4100: 1025 full groups; 8197: 2050 groups, the last with one
    stream - two rounds and a lane mask that ends inside the third, twice the resident grid, and the last group's
    totals over 2050 words.  One upload, three runs (both counter sets, three sequence numbers); after every run the
    forms, the records, the bits of the groups around the boundary and the parsed rows."""
    w = want[n_streams]
    bd = _handle(mods, n_streams, parse=True)
    bd.upload(w.raw)
    for run in range(3):
        what = f"{n_streams} streams, run {run}"
        bd.run()
        forms = bd.last_run_forms()
        assert not forms["second_pass"], f"{what}: {STALLED}; {forms} {bd.counters()}"
        assert forms["one_launch_tail"] and forms["ordered_tail"], (what, forms)
        recs = bd.results().copy()
        TS.assert_records_equal(recs, w.recs, what)
        _assert_bits(bd, cases, n_streams, what)
        arr = bd.parsed()
        got = PG.parsed_rows(arr)
        assert got == w.rows, f"{what}: {[(g, e) for g, e in zip(got, w.rows) if g != e][:4]} {len(got)} {len(w.rows)}"
        PG.assert_parsed_carry_their_packets(arr, _packets_by_stream(recs), what)
        assert bd.counters()["matches"] == w.matches, what
    print(f"\n{n_streams} streams: forms {forms}, counters {bd.counters()}, {len(recs)} records, {len(arr)} messages")
    bd.close()


@pytest.mark.parametrize("n_streams", TS.N_STREAMS)
def test_separate_kernels_at_the_same_size(mods, cases, want, monkeypatch, n_streams):
    """RD_TAIL_IMPL=legacy - the fallback of every overflow and the path of every other shape - on the same batches:
    the slice kernel's grid is capped at 4096 workgroups (16384 matches) and strides over 28 k and 56 k of them, the host
    orders and dedupes them, k_parse_select takes more than one grid pass.  The records equal the one-launch tail's
    field for field (RSSI / SNR within 1e-4 dB) and the oracle's; the counters are equal, and the match count is the
    oracle's raw preamble matches - the last group's sum over all groups' words."""
    w = want[n_streams]
    out = {}
    for impl in (None, "legacy"):
        if impl is None:
            monkeypatch.delenv("RD_TAIL_IMPL", raising=False)
        else:
            monkeypatch.setenv("RD_TAIL_IMPL", impl)
        what = f"{n_streams} streams, {impl or 'default'}"
        bd = _handle(mods, n_streams, parse=True)
        bd.upload(w.raw)
        bd.run()
        forms = bd.last_run_forms()
        assert not forms["second_pass"], f"{what}: {STALLED}; {forms}"
        assert forms["one_launch_tail"] == (impl is None) and forms["ordered_tail"] == (impl is None), (what, forms)
        recs = bd.results().copy()
        TS.assert_records_equal(recs, w.recs, what)
        arr = bd.parsed()
        assert PG.parsed_rows(arr) == w.rows, what
        PG.assert_parsed_carry_their_packets(arr, _packets_by_stream(recs), what)
        if impl:
            _assert_bits(bd, cases, n_streams, what)
        out[impl] = (recs, bd.counters())
        bd.close()
    TS.assert_records_equal(out["legacy"][0], out[None][0], f"{n_streams} streams, legacy against default", db_tol=1e-4)
    assert out[None][1] == out["legacy"][1], "fix-up and match counts differ between the forms"
    assert out[None][1]["matches"] == w.matches
    print(f"\n{n_streams} streams: counters default {out[None][1]}, legacy {out['legacy'][1]}")


def test_match_list_overflow_in_every_group_falls_back(mods, cases, want, monkeypatch):
    """RD_TEST_BUCKET_CAP=2 at 4098 streams: every group with a burst overflows its streams' lists, and the separate
    kernels finish the run on the bits k_tail made exact - the fallback behind more than 1024 groups."""
    monkeypatch.setenv("RD_TEST_BUCKET_CAP", "2")
    n = 4098
    bd = _handle(mods, n)
    bd.upload(want[n].raw)
    bd.run()
    forms = bd.last_run_forms()
    assert forms["second_pass"] and not forms["ordered_tail"], forms
    TS.assert_records_equal(bd.results(), want[n].recs, "4098 streams, lists of two matches")
    _assert_bits(bd, cases, n, "lists of two matches")
    bd.close()


def test_sequence_number_wraps(mods, cases):
    """A group's words carry the run's sequence number, 1 .. 4095 and round again: 4100 runs of one handle (the first
    eight unique streams: two groups, the second waits for the first).  No run may need a second pass; the records of
    the runs around the wrap are the first run's, bit for bit, and the first run's are the oracle's."""
    n = 8
    raw = cases.raw[:n]
    bd = _handle(mods, n)
    bd.upload(raw)
    first = None
    for run in range(1, 4101):
        bd.run()
        forms = bd.last_run_forms()
        assert forms["one_launch_tail"] and not forms["second_pass"], f"run {run}: {STALLED}; {forms}"
        if run == 1:
            first = bd.results().copy()
            exp = np.concatenate([cases.recs[k] for k in range(n)])
            exp["stream"] = np.repeat(np.arange(n), cases.counts[:n])
            TS.assert_records_equal(first, exp, "run 1")
            assert len(np.unique(first["stream"] // TS.GROUP)) == 2
        elif run in (2, 4094, 4095, 4096, 4097, 4100):
            assert np.array_equal(bd.results(), first), f"run {run} differs from run 1"
    assert bd.counters()["matches"] == int(cases.raw_matches[:n].sum())
    bd.close()
