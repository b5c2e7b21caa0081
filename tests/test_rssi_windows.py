"""RSSI / SNR windows of the uint8 paths on the device (MI355X): the streams of tests/rssi_window_cases.py - one planted
burst each and a chosen content under the windows its record reads - through every form that evaluates them:

  k_tail                      BatchDemodulator's one-launch tail: the matrix route, fp32 where rd_rssi_job::ok is false
  k_classify + k_rssi_u8      RD_TAIL_IMPL=legacy: the same two routes behind another pipeline
  k_slice_rssi<rd_u8_src>     packet_symbols = 72 (rd_davis_slice false): fp32 at every position
  k_stream_block              Demodulator / MultiDemodulator block by block: fp32 at every position
  RD_STREAM_IMPL=legacy       the multi-launch streaming form: k_slice_rssi again, one block at a time

Packets, call, index and bytes exactly, RSSI and SNR within 1e-3 dB of the oracle for every record; two forms that
take a record down the same route agree within 1e-4 dB.  What the inputs are proved to be, the models of both routes and
the mutants this comparison would catch: tests/test_rssi_windows_cpu.py.  ``python tests/test_rssi_windows.py`` prints
the largest errors per form, route and content (profiles/rssi_windows.txt)."""
import collections
import math
import os

import numpy as np
import pytest

import rssi_window_cases as RW
import tail_dense_cases as TD
from parse_gate_cases import PREAMBLE

pytestmark = pytest.mark.gpu

DB_TOL = 1e-3
SAME_ROUTE_TOL = 1e-4       # between two forms on the same route (tests/test_tail_dense.py's bound between the tails)
# k_rssi_u8's grid is min(rd_slice_grid(match_cap), 1024) workgroups of four waves, rd_slice_grid(c) = ceil(c / 4): at
# least match_cap waves below the clamp.  A run that keeps its results has matches <= match_cap, and its tasks are the
# matches that survive plus one per match on a block boundary - so no RD_TEST_MATCH_CAP gives the grid fewer waves than
# there are records: a smaller list overflows and the lists grow past the match count again.  The clamp does: 1024
# workgroups are 4096 waves, and a batch of more than 8192 records makes the first waves take a second and a third job
# through the prefetch pipeline (t_cur / t_nxt two steps ahead, the bytes one step ahead).  TILES copies of the streams
# are 7314 streams and 8234 records.  Which wave gets which task is k_classify's atomics' business; the streams
# alternate routes (Cases.order), so any assignment mixes them.
RSSI_WAVES = 4 * 1024
TILES = 46


@pytest.fixture(scope="module")
def dsp():
    from rtldavis_amd import _lib, dsp as d
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    return d


@pytest.fixture(scope="module")
def batchmod():
    from rtldavis_amd import batch
    return batch


@pytest.fixture(scope="module")
def cs():
    return RW.cases()


def _cfg(dsp, packet_symbols=80):
    return dsp.PacketConfig(19200, TD.S, TD.P, packet_symbols, PREAMBLE, RW.B)


def _batch(dsp, batchmod, raw, packet_symbols=80):
    bd = batchmod.BatchDemodulator(_cfg(dsp, packet_symbols), len(raw), RW.N_BLOCKS)
    bd.upload(raw)
    bd.run()
    forms, recs = bd.last_run_forms(), bd.results().copy()
    bits = [bd.bits(s) for s in (0, len(raw) // 2, len(raw) - 1)]
    bd.close()
    return forms, recs, bits


def _check_bits(cs, bits, n):
    for s, b in zip((0, n // 2, n - 1), bits):
        assert np.array_equal(b, cs.bits[s % cs.n_streams]), f"bits of stream {s}"


@pytest.fixture(scope="module")
def one_launch(dsp, batchmod, cs):
    os.environ.pop("RD_TAIL_IMPL", None)
    return _batch(dsp, batchmod, cs.raw)


@pytest.fixture(scope="module")
def separate(dsp, batchmod, cs):
    old = os.environ.get("RD_TAIL_IMPL")
    os.environ["RD_TAIL_IMPL"] = "legacy"
    try:
        return _batch(dsp, batchmod, cs.raw)
    finally:
        os.environ.pop("RD_TAIL_IMPL", None)
        if old is not None:
            os.environ["RD_TAIL_IMPL"] = old


@pytest.fixture(scope="module")
def generic(dsp, batchmod, cs):
    os.environ.pop("RD_TAIL_IMPL", None)
    return _batch(dsp, batchmod, cs.raw, RW.K_GENERIC)


def test_one_launch_tail(cs, one_launch):
    forms, recs, bits = one_launch
    assert forms["one_launch_tail"] and forms["ordered_tail"] and not forms["second_pass"], forms
    TD.assert_records_equal(recs, cs.recs, "k_tail", db_tol=DB_TOL)
    _check_bits(cs, bits, cs.n_streams)


def test_separate_kernels(cs, separate, one_launch):
    forms, recs, bits = separate
    assert not forms["one_launch_tail"] and not forms["ordered_tail"] and not forms["second_pass"], forms
    TD.assert_records_equal(recs, cs.recs, "k_classify + k_rssi_u8", db_tol=DB_TOL)
    _check_bits(cs, bits, cs.n_streams)
    TD.assert_records_equal(recs, one_launch[1], "k_rssi_u8 against k_tail: the same route for every record", db_tol=SAME_ROUTE_TOL)


def test_generic_tail(cs, generic, one_launch):
    forms, recs, _ = generic
    assert not forms["one_launch_tail"] and not forms["second_pass"], forms
    want = RW.generic_recs()
    TD.assert_records_equal(recs, want, "k_slice_rssi<rd_u8_src>", db_tol=DB_TOL)
    # against k_tail where k_tail is on the fp32 route too
    fp = np.array([RW.route(r.call, r.q) == "fp32" for r in cs.records])
    assert fp.sum() >= 40
    for f in ("rssi", "snr"):
        d = np.abs(recs[f][fp] - one_launch[1][f][fp])
        assert (d <= SAME_ROUTE_TOL).all(), (f, float(d.max()), cs.records[int(np.flatnonzero(fp)[int(d.argmax())])].name)


def test_rssi_u8_prefetch_pipeline(dsp, batchmod, cs, monkeypatch):
    """More records than k_rssi_u8 has waves, twice over (see RSSI_WAVES above): waves take three jobs in a row."""
    monkeypatch.setenv("RD_TAIL_IMPL", "legacy")
    n_rec = len(cs.recs)
    assert TILES * n_rec > 2 * RSSI_WAVES and TILES * cs.n_streams * (8 + RW.N_BLOCKS) + 1024 >= 4 * RSSI_WAVES
    raw = np.tile(cs.raw, (TILES, 1))
    want = np.tile(cs.recs, TILES)
    want["stream"] += np.repeat(np.arange(TILES, dtype=np.int32) * cs.n_streams, n_rec)
    forms, recs, bits = _batch(dsp, batchmod, raw)
    # (about 13 raw matches per burst are more than the first lists hold: the lists grow and the run is repeated, its
    # k_rssi_u8 on the clamped grid like the first one's)
    assert not forms["one_launch_tail"] and not forms["ordered_tail"], forms
    TD.assert_records_equal(recs, want, f"k_rssi_u8, {len(want)} records on {RSSI_WAVES} waves", db_tol=DB_TOL)
    _check_bits(cs, bits, len(raw))
    # every copy of a record gets the same bits whichever wave took it and whatever that wave did before
    for f in ("rssi", "snr"):
        a = recs[f].reshape(TILES, n_rec)
        assert np.array_equal(a, np.tile(a[0], (TILES, 1)), equal_nan=True), f


# ------------------------------------------------------------------------------------------------ block by block
def _streamed(dsp, cs, subset, legacy, packet_symbols=80):
    """[[(index, hex, rssi, snr)] per call] per stream of the subset, all streams in lock step (MultiDemodulator)."""
    if legacy:
        os.environ["RD_STREAM_IMPL"] = "legacy"
    else:
        os.environ.pop("RD_STREAM_IMPL", None)
    try:
        md = dsp.MultiDemodulator(_cfg(dsp, packet_symbols), len(subset))
        out = [[] for _ in subset]
        for b in range(RW.N_BLOCKS):
            blocks = np.ascontiguousarray(cs.raw[subset][:, 2 * RW.B * b: 2 * RW.B * (b + 1)])
            for k, pk in enumerate(md.demodulate(blocks)):
                out[k].append([(int(p.index), bytes(p.data).hex(), float(p.rssi), float(p.snr)) for p in pk])
        del md
        return out
    finally:
        os.environ.pop("RD_STREAM_IMPL", None)


def _compare_calls(got, want, what, tol=DB_TOL, worst=None):
    assert [[p[:2] for p in c] for c in got] == [[p[:2] for p in c] for c in want], what
    for c, (gc, wc) in enumerate(zip(got, want)):
        for g, w in zip(gc, wc):
            d = RW.db_diff(g[2:], w[2:])
            assert d <= tol, (what, c, g, w)
            if worst is not None:
                worst.append((abs(g[2] - w[2]), abs(g[3] - w[3]) if not math.isnan(w[3]) else 0.0))


@pytest.fixture(scope="module")
def streamed(dsp, cs):
    subset = RW.streamed_subset()
    return subset, {legacy: _streamed(dsp, cs, subset, legacy) for legacy in (False, True)}


@pytest.mark.parametrize("legacy", (False, True), ids=("k_stream_block", "multi-launch"))
def test_streamed(cs, streamed, legacy):
    subset, got = streamed
    seen = set()
    for k, s in enumerate(subset):
        _compare_calls(got[legacy][k], RW.streamed_calls(s), (cs.order[s], "legacy" if legacy else "one launch"))
        seen |= {(r.cls, r.content) for r in cs.records if r.stream == s}
    assert seen >= {(c, k) for c in RW.CLASSES for k in RW.CONTENTS}
    assert sum(len(c) for k in range(len(subset)) for c in got[legacy][k]) >= len(subset)


def test_single_demodulator(dsp, cs):
    """One plain Demodulator, a pair stream and the twin: the lists MultiDemodulator's stream gave."""
    os.environ.pop("RD_STREAM_IMPL", None)
    for name in ("pairA", "twin0/step_q"):
        s = cs.order.index(name)
        dem = dsp.Demodulator(_cfg(dsp))
        got = [[(int(p.index), bytes(p.data).hex(), float(p.rssi), float(p.snr))
                for p in dem.demodulate(cs.raw[s][2 * RW.B * b: 2 * RW.B * (b + 1)])] for b in range(RW.N_BLOCKS)]
        _compare_calls(got, RW.streamed_calls(s), name)
        assert sum(map(len, got)) == 2


def test_forms_on_the_fp32_route_agree(cs, streamed, generic, one_launch):
    """k_stream_block, the multi-launch form, the generic tail and - for its fp32-route records - k_tail: one arithmetic."""
    subset, got = streamed
    n = 0
    for k, s in enumerate(subset):
        _compare_calls(got[True][k], got[False][k], (cs.order[s], "multi-launch against k_stream_block"), SAME_ROUTE_TOL)
        idx = [i for i, r in enumerate(cs.records) if r.stream == s]
        flat = [p for c in got[False][k] for p in c]
        assert [(r.q) for r in (cs.records[i] for i in idx)] == [p[0] for p in flat], cs.order[s]
        for i, p in zip(idx, flat):
            r = cs.records[i]
            g = (float(generic[1]["rssi"][i]), float(generic[1]["snr"][i]))
            assert RW.db_diff(p[2:], g) <= SAME_ROUTE_TOL, (r.name, "k_stream_block against the generic tail", p, g)
            if RW.route(r.call, r.q) == "fp32":
                t = (float(one_launch[1]["rssi"][i]), float(one_launch[1]["snr"][i]))
                assert RW.db_diff(p[2:], t) <= SAME_ROUTE_TOL, (r.name, "k_stream_block against k_tail", p, t)
                n += 1
    assert n >= 10


# ------------------------------------------------------------------------------------------------ the record
def measure():
    from rtldavis_amd import batch as batchmod, dsp
    cs = RW.cases()
    rows = collections.defaultdict(lambda: [0.0, "", 0.0, ""])

    def note(form, r, got, want):
        w = rows[(form, RW.route(r.call, r.q) if form in ("k_tail", "k_rssi_u8") else "fp32", r.content)]
        d_r = abs(got[0] - want[0])
        d_s = 0.0 if math.isnan(want[1]) else abs(got[1] - want[1])
        if d_r >= w[0]:
            w[0], w[1] = d_r, r.name
        if d_s >= w[2]:
            w[2], w[3] = d_s, r.name

    for form, env, k in (("k_tail", None, 80), ("k_rssi_u8", "legacy", 80), ("k_slice_rssi", None, RW.K_GENERIC)):
        os.environ.pop("RD_TAIL_IMPL", None)
        if env:
            os.environ["RD_TAIL_IMPL"] = env
        _, recs, _ = _batch(dsp, batchmod, cs.raw, k)
        os.environ.pop("RD_TAIL_IMPL", None)
        for i, r in enumerate(cs.records):
            note(form, r, (recs["rssi"][i], recs["snr"][i]), (cs.recs["rssi"][i], cs.recs["snr"][i]))
    subset = RW.streamed_subset()
    for form, legacy in (("k_stream_block", False), ("stream legacy", True)):
        got = _streamed(dsp, cs, subset, legacy)
        for k, s in enumerate(subset):
            recs = [r for r in cs.records if r.stream == s]
            flat_g = [p for c in got[k] for p in c]
            flat_w = [p for c in RW.streamed_calls(s) for p in c]
            for r, g, w in zip(recs, flat_g, flat_w):
                note(form, r, g[2:], w[2:])
    print("|device - oracle| in dB, the largest per form, route and content (case)")
    print(f"{'form':15s} {'route':6s} {'content':10s}  rssi                          snr")
    for (form, rt, c), w in sorted(rows.items()):
        print(f"{form:15s} {rt:6s} {c:10s}  {w[0]:.3e} ({w[1]:24s})  {w[2]:.3e} ({w[3]})")


if __name__ == "__main__":
    measure()
