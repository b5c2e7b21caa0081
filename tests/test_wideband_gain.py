"""WidebandReceiver.set_gain / levels() on the device (rd_wb_set_gain -> the gains[ch] load of k_channelize, rd_wb_set_levels
-> k_chan_levels; rd_channelizer.hip, rd_chan_levels.hip): every chunk of a receiver whose per-channel gains change between chunks, with
chunks in flight and a retune beside them, against the float64 model at each channel's gain and its a-priori bound
(tests/gain_cases.py); receivers that never call set_gain, are constructed with the gain or are reset - byte for byte;
the level records against NumPy integers of the same bytes, exactly; and the gain loop closed through levels() and
agc.GainControl on the weak-and-strong capture.  PARITY UNPINNED, as for the channelizer."""
import functools

import numpy as np
import pytest

import chan_bound as CB
import gain_cases as GC
import retune_cases as RC
from stream_parse_helpers import _pkey, _rows

pytestmark = pytest.mark.gpu
NAMES = list(RC.CASES)


def _device():
    from rtldavis_amd import _lib
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"


@functools.lru_cache(maxsize=None)
def _twin(name):
    """(bytes, packets) per chunk of a receiver that never calls set_gain, set_levels or retune, one chunk at a time."""
    _device()
    cs = RC.case(name)
    w = RC.receiver(cs)
    out = []
    for chunk in cs.chunks:
        pk = w.demodulate(chunk)
        out.append((w.channelized(), _pkey(pk)))
    return out


@functools.lru_cache(maxsize=None)
def _base(name):
    """The same receiver at the case's first gain set (gains A), never changed afterwards: bytes per chunk."""
    _device()
    gc = GC.case(name)
    w = RC.receiver(gc.cs)
    w.set_gain(gc.gain_schedule[0])
    out = []
    for chunk in gc.cs.chunks:
        w.demodulate(chunk)
        out.append(w.channelized())
    return out


@functools.lru_cache(maxsize=None)
def _scheduled(name):
    """The case's gain schedule with two chunks in flight and levels on: gains A before chunk 0, a subset before chunk 2,
    all (and a retune of all) before chunk 3 - submit, submit, set_gain, fetch, submit, ...  Per chunk, taken after its
    fetch with the next chunk already submitted: (bytes, levels, packets); and the gains() seen before each submit."""
    _device()
    gc = GC.case(name)
    cs = gc.cs
    w = RC.receiver(cs)
    w.set_levels(True)
    got, seen = [], []

    def take():
        pk = w.fetch()
        got.append((w.channelized(), w.levels(), _pkey(pk)))

    for k, chunk in enumerate(cs.chunks):
        if k in gc.gain_schedule:
            assert w.inflight == (2 if k else 0)
            w.set_gain(gc.gain_schedule[k])
        if k in gc.retune_schedule:
            assert w.inflight == 2
            w.retune(gc.retune_schedule[k])
        if k >= 2:
            take()                                      # chunk k - 2, chunk k - 1 in flight
        seen.append(w.gains())
        w.submit(chunk)
    take()
    take()
    return got, seen, w


@pytest.mark.parametrize("name", NAMES)
def test_equal_gains_through_set_gain_change_nothing(name):
    cs = RC.case(name)
    twin = _twin(name)
    w = RC.receiver(cs)
    for k, chunk in enumerate(cs.chunks):
        w.set_gain(cs.gain if k % 2 else [cs.gain] * cs.n_ch)
        pk = w.demodulate(chunk)
        assert np.array_equal(w.channelized(), twin[k][0]), k
        assert _pkey(pk) == twin[k][1], k
    assert w.gains().tolist() == [cs.gain] * cs.n_ch


@pytest.mark.parametrize("name", NAMES)
def test_every_chunk_matches_the_model_at_its_channels_gains(name):
    """Distinct per-channel gains 0.25 .. 300, changed for a subset before chunk 2 and for all - with a retune of all -
    before chunk 3, both with two chunks in flight: every chunk's bytes against the model at the gains (and tuning) in
    force at its submit."""
    gc = GC.case(name)
    got, seen, _ = _scheduled(name)
    want = GC.gains_per_chunk(gc)
    assert [s.tolist() for s in seen] == [g.tolist() for g in want]
    assert want[0].min() == 0.25 and want[0].max() == 300.0 and len(set(want[0].tolist())) >= min(gc.n_ch, 3)
    for k, (Z, delta, g, _) in enumerate(GC.schedule_models(gc)):
        s = CB.check_against_model(got[k][0], Z, delta)
        print(f"\n[chan-gain] {name} chunk {k}: exempt {s['exempt']:.2%}, mismatches {s['mismatches']}/{got[k][0].size}, "
              f"worst distance {s['worst_dist']:.2e} ({s['worst_ratio']:.2f} of delta)")
        assert s["bad_lsb"] == 0 and s["bad_exact"] == 0, (k, s)
        assert s["exempt"] <= GC.GPU_EXEMPT_CAP, (k, s)


@pytest.mark.parametrize("name", NAMES)
def test_channels_whose_gain_stays_are_untouched(name):
    gc = GC.case(name)
    cs = gc.cs
    got, _, _ = _scheduled(name)
    base = _base(name)
    for k in (0, 1):
        assert np.array_equal(got[k][0], base[k]), k
    keep = ~cs.subset
    assert keep.any() and cs.subset.any()
    assert np.array_equal(got[2][0][keep], base[2][keep])
    for c in np.flatnonzero(cs.subset):
        assert not np.array_equal(got[2][0][c], base[2][c]), c
    # chunk 3: a new gain and a new frequency for every channel - neither the base receiver's bytes nor, scaled, a
    # gain change alone (the retune test's receiver at gains A would be the base's bytes at another frequency)
    for c in range(cs.n_ch):
        assert not np.array_equal(got[3][0][c], base[3][c]), c
    s, p = _scheduled(name)[2].tuning()
    assert (tuple(int(v) for v in s), tuple(int(v) for v in p)) == RC.tunings(cs, gc.retune_schedule)[-1]


@pytest.mark.parametrize("name", NAMES)
def test_set_gain_before_the_first_chunk_equals_construction(name):
    from rtldavis_amd import wideband
    cs = RC.case(name)
    w = RC.receiver(cs)
    w.set_gain(0.75)
    built = wideband.WidebandReceiver(cs.cfg, cs.chans, RC.CENTRE, decim=cs.decim, taps=cs.user_taps, gain=0.75,
                                      sample_format=cs.fmt)
    assert w.gains().tolist() == built.gains().tolist() == [0.75] * cs.n_ch
    for k in range(3):
        a, b = w.demodulate(cs.chunks[k]), built.demodulate(cs.chunks[k])
        assert np.array_equal(w.channelized(), built.channelized()), k
        assert _pkey(a) == _pkey(b), k
    assert not np.array_equal(w.channelized(), _twin(name)[2][0])


@pytest.mark.parametrize("name", NAMES)
def test_reset_after_set_gain_reproduces_the_first_run(name):
    gc = GC.case(name)
    cs = gc.cs
    twin = _twin(name)
    w = RC.receiver(cs)
    w.set_levels(True)
    w.demodulate(cs.chunks[0])
    w.set_gain(gc.gain_schedule[3])
    w.demodulate(cs.chunks[1])
    assert not np.array_equal(w.channelized(), twin[1][0]) and w.levels().chunk == 1
    w.set_gain(gc.gain_schedule[0])                     # pending at the reset
    w.reset()
    assert w.gains().tolist() == [cs.gain] * cs.n_ch
    with pytest.raises(RuntimeError):
        w.levels()
    for k in range(3):
        pk = w.demodulate(cs.chunks[k])
        assert np.array_equal(w.channelized(), twin[k][0]), k
        assert _pkey(pk) == twin[k][1], k
        assert w.levels().chunk == k                    # the sequence restarts


@pytest.mark.parametrize("name", NAMES)
def test_levels_are_the_numpy_integers(name):
    """For every chunk, read after its fetch with the next chunk submitted: the channel records are exactly the integers
    NumPy computes from channelized(), the gain the float32 in force, the input record exactly those of the submitted
    chunk, and `chunk` counts 0, 1, 2, ..."""
    gc = GC.case(name)
    cs = gc.cs
    got, _, _ = _scheduled(name)
    gains = GC.gains_per_chunk(gc)
    for k, (block, lv, _) in enumerate(got):
        assert lv.chunk == k
        want = GC.channel_levels(block)
        have = [(int(r["peak"]), int(r["clipped"]), int(r["power"])) for r in lv.channels]
        assert have == want, k
        assert lv.channels["gain"].dtype == np.float32
        assert lv.channels["gain"].tolist() == gains[k].astype(np.float32).tolist(), k
        assert tuple(lv.input) == GC.input_levels(cs.chunks[k], cs.fmt), k
    if cs.fmt != "u8":
        assert got[0][1].input.clipped >= 2             # capture_fmt plants both ends of the range in chunk 0
        assert got[0][1].input.peak == {"s8": 128, "s16": 32768}[cs.fmt]
    assert any(r["clipped"] for r in got[0][1].channels) and max(int(r["peak"]) for r in got[0][1].channels) == 255


@pytest.mark.parametrize("name", NAMES)
def test_levels_off_is_the_plain_receiver(name):
    cs = RC.case(name)
    twin = _twin(name)
    on, off = RC.receiver(cs), RC.receiver(cs)
    on.set_levels(True)
    for k in range(3):
        a, b = on.demodulate(cs.chunks[k]), off.demodulate(cs.chunks[k])
        with pytest.raises(RuntimeError):
            off.levels()
        assert on.levels().chunk == k
        assert np.array_equal(on.channelized(), twin[k][0]) and np.array_equal(off.channelized(), twin[k][0]), k
        assert _pkey(a) == _pkey(b) == twin[k][1], k
    on.submit(cs.chunks[3])
    with pytest.raises(RuntimeError):
        on.set_levels(False)                            # a chunk in flight
    on.fetch()
    on.set_levels(False)
    on.demodulate(cs.chunks[4 % cs.nk])
    with pytest.raises(RuntimeError):
        on.levels()                                     # that chunk was submitted with levels off


def test_closed_loop_through_levels():
    """levels() -> GainControl.update() -> set_gain() every chunk, two chunks in flight, on the weak-and-strong capture
    of the CPU test: the CRC-valid messages are the model's - both packets - and so are the gains chunk by chunk."""
    from rtldavis_amd import agc, wideband
    _device()
    lc = GC.loop_capture()
    _, model_used = GC.loop_run_model()
    w = wideband.WidebandReceiver(RC.packet_config(GC.LOOP_B), lc.chans, gain=GC.LOOP_SCALAR_GAIN, sample_format="s16")
    w.set_parse(True)
    w.set_levels(True)
    ctl = agc.GainControl(len(lc.chans), GC.LOOP_B, **GC.LOOP_AGC)
    w.set_gain(ctl.gains())
    msgs, used = [], []

    def take():
        w.fetch()
        msgs.extend((r[0], r[1], r[5]) for r in _rows(w.parsed()))
        lv = w.levels()
        used.append(lv.channels["gain"].astype(np.float64).tolist())
        new = ctl.update(lv)
        if new is not None:
            w.set_gain(new)

    for k in range(GC.LOOP_NK):
        if k >= 2:
            take()
        w.submit(lc.raw[lc.step * k: lc.step * (k + 1)])
    take()
    take()
    print(f"\n[gain-loop] gains per chunk {used}")
    assert used == [u.tolist() for u in model_used]
    strong, weak = lc.info
    assert sorted(msgs) == [(0, 3, strong[0]), (1, 10, weak[0])]
    plain = wideband.WidebandReceiver(RC.packet_config(GC.LOOP_B), lc.chans, gain=GC.LOOP_SCALAR_GAIN, sample_format="s16")
    plain.set_parse(True)
    lost = []
    for k in range(GC.LOOP_NK):
        plain.demodulate(lc.raw[lc.step * k: lc.step * (k + 1)])
        lost.extend((r[0], r[1], r[5]) for r in _rows(plain.parsed()))
    assert lost == [(0, 3, strong[0])]                  # the scalar gain loses the weak packet on the device too


@pytest.mark.parametrize("name", NAMES)
def test_channelizer_set_gain_is_the_same_table(name):
    """The one-shot form: set_gain before the first run (host table) and after one (device table) - the whole capture's
    bytes are the streamed chunks' of a receiver at the same gains."""
    from rtldavis_amd import channelizer
    gc = GC.case(name)
    cs = gc.cs
    ch = channelizer.Channelizer(cs.chans, RC.CENTRE, decim=cs.decim, taps=cs.user_taps, gain=cs.gain, out_rate=cs.fo,
                                 sample_format=cs.fmt)
    ch.upload(cs.raw)
    assert np.array_equal(ch.run_host(), np.concatenate([t[0] for t in _twin(name)], axis=1))
    ch.set_gain(gc.gain_schedule[0])
    assert np.array_equal(ch.run_host(), np.concatenate(_base(name), axis=1))
    first = channelizer.Channelizer(cs.chans, RC.CENTRE, decim=cs.decim, taps=cs.user_taps, gain=cs.gain, out_rate=cs.fo,
                                    sample_format=cs.fmt)
    first.set_gain(gc.gain_schedule[0])
    first.upload(cs.raw)
    assert np.array_equal(first.run_host(), np.concatenate(_base(name), axis=1))
