"""WidebandReceiver.retune on the device (rd_wb_retune -> k_chan_retune, rd_channelizer.hip): every chunk of a receiver
retuned between chunks, with chunks in flight, against the float64 model of its segment's tuning (s', P') and its
a-priori bound (tests/retune_cases.py); channels that are not retuned, a retune before the first chunk, a retune to the
tuning in force, reset() after a retune - byte for byte against receivers that were never retuned or were constructed
with the new channels; a clock past 2^40; and the frequency loop closed through parsed().  PARITY UNPINNED, as for the
channelizer: the reference retunes its dongle (runners/rtlsdr.py:51,72)."""
import functools

import numpy as np
import pytest

import chan_bound as CB
import retune_cases as RC
from stream_parse_helpers import _oracle_expected, _rows, assert_rows_match

pytestmark = pytest.mark.gpu
NAMES = list(RC.CASES)


def _tuning(w):
    s, p = w.tuning()
    return tuple(int(v) for v in s), tuple(int(v) for v in p)


@functools.lru_cache(maxsize=None)
def _twin(name):
    """The chunks of a receiver that is never retuned."""
    from rtldavis_amd import _lib
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    cs = RC.case(name)
    w = RC.receiver(cs)
    out = []
    for chunk in cs.chunks:
        w.demodulate(chunk)
        out.append(w.channelized())
    return out


@functools.lru_cache(maxsize=None)
def _retuned(name):
    """The case's schedule with two chunks in flight: submit, submit, retune, fetch, submit, ... - a subset of the
    channels before chunk 2, all of them before chunk 3.  Returns (chunks' bytes, the tuning() seen before each submit)."""
    cs = RC.case(name)
    _twin(name)
    w = RC.receiver(cs)
    got, seen = [], []

    def take():
        w.fetch()
        got.append(w.channelized())

    for k, chunk in enumerate(cs.chunks):
        if k in cs.schedule:
            assert w.inflight == 2
            w.retune(cs.schedule[k])
        if k >= 2:
            take()
        seen.append(_tuning(w))
        w.submit(chunk)
    take()
    take()
    return got, seen


@pytest.mark.parametrize("name", NAMES)
def test_every_chunk_matches_the_model_of_its_tuning(name):
    cs = RC.case(name)
    got, seen = _retuned(name)
    want = RC.tunings(cs)
    assert seen == want
    assert want[1] == want[0] and want[2] != want[1] and want[3] != want[2] and any(want[3][1])
    assert min(want[3][0]) == -(cs.fw // 2) and max(want[3][0]) == cs.fw // 2
    for k in range(cs.nk):
        Z, delta = RC.segment_model(cs, k, *want[k])
        s = CB.assert_matches_model(got[k], Z, delta)
        print(f"\n[chan-retune] {name} chunk {k}: exempt {s['exempt']:.2%}, mismatches {s['mismatches']}/{got[k].size}, "
              f"worst distance {s['worst_dist']:.2e} ({s['worst_ratio']:.2f} of delta)")


@pytest.mark.parametrize("name", NAMES)
def test_channels_not_retuned_are_untouched(name):
    cs = RC.case(name)
    got, _ = _retuned(name)
    twin = _twin(name)
    for k in (0, 1):
        assert np.array_equal(got[k], twin[k]), k
    keep = ~cs.subset
    assert keep.any() and cs.subset.any()
    assert np.array_equal(got[2][keep], twin[2][keep])
    for c in np.flatnonzero(cs.subset):
        assert not np.array_equal(got[2][c], twin[2][c]), c
    for c in range(cs.n_ch):
        assert not np.array_equal(got[3][c], twin[3][c]), c


@pytest.mark.parametrize("name", NAMES)
def test_retune_before_the_first_chunk_equals_construction(name):
    """The tables are still the host's then: the receiver is the one constructed with the new channels, early DC
    entries included."""
    cs = RC.case(name)
    off = cs.schedule[3]
    w = RC.receiver(cs)
    w.retune(off)
    built = RC.receiver(cs, [int(f) + int(o) for f, o in zip(cs.chans, off)])
    assert _tuning(w) == _tuning(built) == (tuple(int(s) + int(o) for s, o in zip(cs.plan_shift, off)), (0,) * cs.n_ch)
    for k in range(3):
        w.demodulate(cs.chunks[k])
        built.demodulate(cs.chunks[k])
        assert np.array_equal(w.channelized(), built.channelized()), k
    assert not np.array_equal(w.channelized(), _twin(name)[2])


@pytest.mark.parametrize("name", NAMES)
def test_retune_to_the_tuning_in_force_changes_nothing(name):
    cs = RC.case(name)
    twin = _twin(name)
    off = cs.schedule[2]
    w, once = RC.receiver(cs), RC.receiver(cs)
    w.retune(0)                                         # before the first chunk, host tables
    for k in range(cs.nk):
        if k == 2:
            w.retune(off)
            once.retune(off)
        elif k == 1:
            w.retune(np.zeros(cs.n_ch, np.int64))       # device tables, the plan in force
        elif k > 2:
            w.retune(-off)
            w.retune(off)                               # collapses into the tuning in force
        before = _tuning(w)
        w.demodulate(cs.chunks[k])
        once.demodulate(cs.chunks[k])
        assert _tuning(w) == before == _tuning(once)
        assert np.array_equal(w.channelized(), once.channelized()), k
        if k < 2:
            assert np.array_equal(w.channelized(), twin[k]), k


@pytest.mark.parametrize("name", NAMES)
def test_reset_after_a_retune(name):
    """reset() returns to the constructed plan with P = 0: the chunks that follow equal a fresh receiver's (the device
    tables are rebuilt at clock 0, early DC entries and all), and a retune pending at the reset is dropped."""
    cs = RC.case(name)
    twin = _twin(name)
    w = RC.receiver(cs)
    w.demodulate(cs.chunks[0])
    w.retune(cs.schedule[3])
    w.demodulate(cs.chunks[1])
    assert not np.array_equal(w.channelized(), twin[1])
    w.retune(cs.schedule[2])                            # pending at the reset
    w.reset()
    assert _tuning(w) == (tuple(int(s) for s in cs.plan_shift), (0,) * cs.n_ch)
    assert np.array_equal(w.shift_hz, cs.plan_shift)
    for k in range(3):
        w.demodulate(cs.chunks[k])
        assert np.array_equal(w.channelized(), twin[k]), k


def test_large_clock():
    """The clock starts at 2^40 + 128 x 77 and every channel is retuned at the first boundary behind it: the model's
    rotation constant is (s' t_off + P') mod Fo.  (Chunk 0 has zero history at a clock that is not 0, where the uint8
    kernel's DC term is the steady one: its first n_early outputs are the test hook's, not the model's.)"""
    cs = RC.case(RC.LARGE_CLOCK_CASE)
    t_off = RC.LARGE_CLOCK
    sched = RC.large_clock_schedule(cs)
    want = RC.tunings(cs, sched, t_off)
    assert any(want[1][1]) and t_off > 2 ** 40
    w = RC.receiver(cs)
    w._debug_advance_clock(t_off)
    n_early = -(-(cs.taps.size - 1) // cs.decim)
    assert n_early == 64 and cs.fmt == "u8"
    for k in range(cs.nk):
        if k in sched:
            w.retune(sched[k])
        assert _tuning(w) == want[k]
        w.demodulate(cs.chunks[k])
        got = w.channelized()
        Z, delta = RC.segment_model(cs, k, *want[k], t_off=t_off)
        skip = n_early if k == 0 else 0
        s = CB.assert_matches_model(got[:, 2 * skip:], Z[:, skip:], delta[:, skip:])
        print(f"\n[chan-retune] large clock chunk {k}: exempt {s['exempt']:.2%}, mismatches {s['mismatches']}, "
              f"worst distance {s['worst_dist']:.2e} ({s['worst_ratio']:.2f} of delta)")


def test_closed_loop_through_parsed():
    """parsed() of burst A -> retune(offset = freq_err) -> burst B, two chunks in flight: the capture and seeds of the
    CPU test.  The device's rows equal the dsp oracle's on the device's own channelized bytes, and the error of burst
    B is at most a quarter of burst A's - the sign convention is the reference's channel_freq + freq_corr."""
    from rtldavis_amd import wideband
    lc = RC.loop_capture()
    w = wideband.WidebandReceiver(RC.packet_config(RC.LOOP_B), lc.chans)
    w.set_parse(True)
    rows, blocks, retuned_at = [], [], []

    def take(k_next):
        w.fetch()
        r = _rows(w.parsed())
        rows.append(r)
        blocks.append(w.channelized()[0])
        if r and not retuned_at:
            w.retune(r[0][4])                           # offset = freq_err, as it comes
            retuned_at.append(k_next)

    for k in range(RC.LOOP_NK):
        if k >= 2:
            take(k)
        w.submit(lc.raw[lc.step * k: lc.step * (k + 1)])
    take(RC.LOOP_NK)
    take(RC.LOOP_NK)
    assert retuned_at == [RC.LOOP_RETUNE_CHUNK]
    orc = _oracle_expected([blocks], RC.LOOP_B)
    for k in range(RC.LOOP_NK):
        assert_rows_match(rows[k], orc[k], ("oracle", k))
    msgs = [r for rs in rows for r in rs]
    assert [(r[1], r[5]) for r in msgs] == [(2, lc.payload), (5, lc.payload)]
    e_a, e_b = msgs[0][4], msgs[1][4]
    print(f"\n[retune-loop] e_A {e_a} Hz, e_B {e_b} Hz")
    assert abs(e_a - RC.LOOP_CFO) < 500
    assert abs(e_b) <= abs(e_a) / 4
    assert [int(s) for s in w.shift_hz] == [int(lc.plan.shift_hz[0]) + e_a]
