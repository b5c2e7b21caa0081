"""The batch tail on dense match lists (MI355X): the batches of tests/tail_dense_cases.py through BatchDemodulator.
k_tail keeps a stream's matches in a list in LDS, 32 entries for these four-block streams; an upload whose run
overflowed a list is finished by the separate kernels and the next upload gets lists twice as long, up to 512 (61 and
120 KiB of LDS for the last two sizes), beyond which the handle stays on the separate kernels.  Here: lists exactly
full and over by one, every list size with a stream that needs it, two to five lane rounds of slice, dedupe and rank,
block-boundary twins, two search waves on one list, the last reported position, more than 256 records in a group.
Everything is compared with the oracle as a whole and in order after every run, whichever form the run took.  The
conditions the inputs meet and the comparison's teeth are checked on the CPU (tests/test_tail_dense_cpu.py)."""
import collections
import types

import numpy as np
import pytest

import parse_gate_cases as PG
import tail_dense_cases as TD

pytestmark = pytest.mark.gpu

STALLED = ("RD_CNT_OVF bit 16 (a group gave up waiting for the groups in front of it: k_tail's spin limit) or 8 (a "
           "group's fix-up bucket): every run of every stream was re-evaluated")


@pytest.fixture(scope="module")
def mods():
    from rtldavis_amd import _lib, batch, dsp
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    return batch, dsp


def _handle(mods, n_streams, parse=False, n_blocks=TD.N_BLOCKS):
    batch, dsp = mods
    bd = batch.BatchDemodulator(dsp.PacketConfig(19200, 14, 16, 80, PG.PREAMBLE, TD.B), n_streams, n_blocks)
    bd.set_parse(parse)
    return bd


def _packets_by_stream(recs):
    by = collections.defaultdict(list)
    for s, i, r, q in zip(recs["stream"].tolist(), recs["index"].tolist(), recs["rssi"].tolist(), recs["snr"].tolist()):
        by[s].append(types.SimpleNamespace(index=i, rssi=r, snr=q))
    return by


def _check(bd, bt, what, parse=False):
    """Everything that is compared after every run; returns the forms and a copy of the records."""
    forms = bd.last_run_forms()
    cnt = bd.counters()
    # the spin limit and the fix-up buckets answer with an exact re-evaluation of every run: the fix-up count says so
    assert cnt["fixup_runs"] < bt.n_streams * (bt.n_samples // 32), f"{what}: {STALLED}; {forms} {cnt}"
    recs = bd.results().copy()
    TD.assert_records_equal(recs, bt.recs, what)
    for s in range(bt.n_streams):
        assert np.array_equal(bd.bits(s), bt.bits[s]), f"{what}: bits of stream {s}"
    assert cnt["matches"] == int(bt.raw_matches.sum()), f"{what}: {cnt}, the oracle has {bt.raw_matches.tolist()}"
    if parse:
        arr = bd.parsed()
        got, want = PG.parsed_rows(arr), bt.rows()
        assert got == want, f"{what}: {[(g, e) for g, e in zip(got, want) if g != e][:4]} {len(got)} {len(want)}"
        PG.assert_parsed_carry_their_packets(arr, _packets_by_stream(recs), what)
    return forms, recs


def _first_pass(forms, what):
    assert forms["one_launch_tail"] and forms["ordered_tail"] and not forms["second_pass"], (what, forms)


def _overflowed(forms, what):
    assert forms["second_pass"] and not forms["ordered_tail"] and not forms["one_launch_tail"], (what, forms)


def _separate(forms, what):
    assert not forms["second_pass"] and not forms["ordered_tail"] and not forms["one_launch_tail"], (what, forms)


def _run(bd, bt, what, parse=False, upload=True):
    if upload:
        bd.upload(bt.raw)
    bd.run()
    return _check(bd, bt, what, parse)


def _grow(bd, bt, parse=False):
    """Upload and run the batch until a run stays in its first pass: one overflowing upload per doubling of the lists
    from 32 to what the batch needs, each finished by the separate kernels with the right records."""
    doublings = bt.list_size().bit_length() - TD.LIST_MIN.bit_length()
    for k in range(doublings):
        forms, _ = _run(bd, bt, f"{bt.name}, lists of {TD.LIST_MIN << k}", parse)
        _overflowed(forms, f"{bt.name}, lists of {TD.LIST_MIN << k}")
    forms, recs = _run(bd, bt, f"{bt.name}, lists of {bt.list_size()}", parse)
    _first_pass(forms, f"{bt.name}, lists of {bt.list_size()}")
    return recs


def test_full_list(mods):
    """Lists of 32 with 32, 0, 31 and 32 matches hold; with 33 in one stream the run overflows and the separate kernels
    finish it, the full and the ragged group behind the overflowing one included; the first batch on that handle, whose
    lists are 64 by then, gives the records of the fresh handle bit for bit."""
    a, b = TD.batch("full_list_a"), TD.batch("full_list_b")
    bd = _handle(mods, a.n_streams, parse=True)
    forms, fresh = _run(bd, a, "full_list_a, fresh handle", parse=True)
    _first_pass(forms, "full_list_a: lists exactly full")
    bd.close()
    bd = _handle(mods, b.n_streams, parse=True)
    forms, _ = _run(bd, b, "full_list_b, fresh handle", parse=True)
    _overflowed(forms, "full_list_b: a list over by one")
    forms, again = _run(bd, a, "full_list_a behind full_list_b", parse=True)
    _first_pass(forms, "full_list_a at lists of 64")
    assert np.array_equal(again, fresh), "lists of 64 and of 32 give different records"
    forms, _ = _run(bd, b, "full_list_b at lists of 64", parse=True)
    _first_pass(forms, "full_list_b at lists of 64")
    bd.close()


def test_ladder(mods):
    """One handle from lists of 32 to 512 and past them.  The 65..128 batch three times: 32 -> 64 -> 128, the third
    run stays in its first pass; a run repeated without an upload after an overflow stays on the separate kernels;
    then 256 and 512 entries (61 and 120 KiB of LDS); then a stream with more than 512 matches, after which no upload
    brings the one-launch tail back on this handle - and a fresh handle is not affected."""
    bd = _handle(mods, 8)
    b128 = TD.batch("ladder_128")
    seen = []
    for k in range(3):
        forms, _ = _run(bd, b128, f"ladder_128, upload {k}")
        seen.append(forms["second_pass"])
        if k == 0:
            _overflowed(forms, "ladder_128 at lists of 32")
            forms, _ = _run(bd, b128, "ladder_128 run again without an upload", upload=False)
            _separate(forms, "a run without an upload after an overflow")
    assert seen == [True, True, False], f"second passes of three uploads of a {b128.raw_matches.max()}-match stream: {seen}"
    _first_pass(forms, "ladder_128 at lists of 128")
    for name in ("ladder_256", "ladder_512"):
        bt = TD.batch(name)
        forms, _ = _run(bd, bt, f"{name}, first upload")
        _overflowed(forms, f"{name}, first upload")
        forms, _ = _run(bd, bt, f"{name}, second upload")
        _first_pass(forms, f"{name}, second upload")
        forms, _ = _run(bd, bt, f"{name}, run again", upload=False)
        _first_pass(forms, f"{name}, run again")
    forms, _ = _run(bd, b128, "ladder_128 at lists of 512")
    _first_pass(forms, "ladder_128 at lists of 512")
    over, plain = TD.batch("ladder_over"), TD.batch("ordinary")
    forms, _ = _run(bd, over, "ladder_over")
    _overflowed(forms, "ladder_over: more matches than the longest list")
    forms, _ = _run(bd, over, "ladder_over, second upload")
    _separate(forms, "ladder_over, second upload")
    forms, _ = _run(bd, plain, "ordinary behind ladder_over")
    _separate(forms, "ordinary behind ladder_over")
    bd.close()
    bd = _handle(mods, 8)
    forms, _ = _run(bd, plain, "ordinary, fresh handle")
    _first_pass(forms, "ordinary, fresh handle")
    bd.close()


def test_ladder_first_doubling(mods):
    """A 33..64-match stream: one overflow, then lists of 64."""
    bd = _handle(mods, 8)
    _grow(bd, TD.batch("ladder_64"))
    bd.close()


def test_rounds_are_the_same_every_run(mods):
    """Two and five lane rounds of slice, dedupe and rank at lists of 512; three runs: the search waves' atomics give
    the matches other slots every time, the records are the same bit for bit."""
    bt = TD.batch("rounds")
    bd = _handle(mods, bt.n_streams)
    first = _grow(bd, bt)
    for run in (1, 2):
        forms, recs = _run(bd, bt, f"rounds, run {run}", upload=False)
        _first_pass(forms, f"rounds, run {run}")
        assert np.array_equal(recs, first), f"rounds: run {run} differs from run 0"
    bd.close()


@pytest.mark.parametrize("name", ("twins", "geometry", "many_records"))
def test_one_launch_tail_at_lists_of_128(mods, name):
    bt = TD.batch(name)
    assert bt.list_size() == 128
    bd = _handle(mods, bt.n_streams, parse=name in TD.PARSED)
    _grow(bd, bt, parse=name in TD.PARSED)
    bd.close()


def test_long_streams_start_with_lists_of_96(mods):
    """Four streams of 105 blocks: lists of 96 from the streams' length (rd_ord_bucket_cap), no growth; 91 and 85
    matches - two lane rounds - in the first pass of a fresh handle."""
    bt = TD.batch("long_96")
    bd = _handle(mods, bt.n_streams, n_blocks=bt.n_blocks)
    for run in range(2):
        forms, _ = _run(bd, bt, f"long_96, run {run}", upload=run == 0)
        _first_pass(forms, f"long_96, run {run}")
    bd.close()


@pytest.mark.parametrize("name", ("full_list_b", "rounds", "twins", "geometry"))
def test_separate_kernels_agree(mods, monkeypatch, name):
    """RD_TAIL_IMPL=legacy - what every overflow falls back to - on a handle of its own: the oracle's records, and the
    one-launch tail's field for field, RSSI / SNR within 1e-4 dB."""
    bt = TD.batch(name)
    monkeypatch.delenv("RD_TAIL_IMPL", raising=False)
    bd = _handle(mods, bt.n_streams)
    one = _grow(bd, bt)
    bd.close()
    monkeypatch.setenv("RD_TAIL_IMPL", "legacy")
    bd = _handle(mods, bt.n_streams)
    forms, sep = _run(bd, bt, f"{name}, separate kernels")
    _separate(forms, f"{name}, separate kernels")
    bd.close()
    TD.assert_records_equal(sep, one, f"{name}, separate kernels against the one-launch tail", db_tol=1e-4)
