"""k_chan_levels (rd_chan_levels.hip) on the crafted captures of tests/level_cases.py, through WidebandReceiver.set_levels /
levels(): the input record equals the NumPy integers exactly on chunks drawn from each format's edge alphabet, on
all-min, all-max and all-quiet chunks, with a single extreme at every position of the first and the last 16-byte vector,
and with peaks that come from the negative side alone; over 2 and 7 workgroups and past the cap of 256 with the
extremes where only the last round of the grid-stride loop reads them; the five device words clean between launches
with two chunks in flight; and the channel records at gains of 300 and 0.25 against the bytes channelized() returns."""
import numpy as np
import pytest

import gain_cases as GC
import level_cases as LC
import retune_cases as RC

pytestmark = pytest.mark.gpu
CHANS = [RC.CENTRE - 100000, RC.CENTRE + 100000]
TAPS = np.hanning(10)[1:-1] / np.hanning(10).sum()
GAINS = (300.0, 0.25)                                                      # the loud channel, the faint one


def _receiver(fmt, decim, bs):
    from rtldavis_amd import _lib, wideband
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    w = wideband.WidebandReceiver(RC.packet_config(bs), CHANS, RC.CENTRE, decim=decim, taps=TAPS, sample_format=fmt)
    w.set_levels(True)
    return w


def _channel_records(lv):
    return [(int(r["peak"]), int(r["clipped"]), int(r["power"])) for r in lv.channels]


@pytest.mark.parametrize("fmt", LC.FORMATS)
def test_edge_captures_on_the_smallest_chunk(fmt):
    """Every small case in turn on one receiver at gains (300, 0.25): the input record is the NumPy integers', the
    channel records those of the bytes channelized() returns with the float32 gains in force, and the alphabet captures
    drive the loud channel to both ends of the byte range."""
    w = _receiver(fmt, *LC.SMALL)
    w.set_gain(GAINS)
    for k, (name, raw) in enumerate(LC.small_cases(fmt).items()):
        w.demodulate(raw)
        lv = w.levels()
        assert lv.chunk == k, name
        assert tuple(lv.input) == LC.want(raw, fmt), (fmt, name, tuple(lv.input), LC.want(raw, fmt))
        block = w.channelized()
        assert block.shape == (2, 2 * LC.SMALL[1])
        if name.startswith("alphabet"):
            assert (block[0] == 0).any() and (block[0] == 255).any(), (fmt, name)
        assert _channel_records(lv) == GC.channel_levels(block), (fmt, name)
        assert lv.channels["gain"].dtype == np.float32 and lv.channels["gain"].tolist() == [np.float32(g) for g in GAINS]


@pytest.mark.parametrize("fmt", LC.FORMATS)
def test_extremes_in_the_last_vector_of_several_workgroups(fmt):
    for which, count in ((0, 2), (1, 7)):
        decim, bs, raw = LC.sliced_case(fmt, which)
        assert LC.slices(fmt, decim * bs) == count
        w = _receiver(fmt, decim, bs)
        for k in range(2):                                                 # twice: the second launch finds the words clean
            w.demodulate(raw)
            lv = w.levels()
            assert lv.chunk == k and tuple(lv.input) == LC.want(raw, fmt), (fmt, count, k, tuple(lv.input), LC.want(raw, fmt))
            assert _channel_records(lv) == GC.channel_levels(w.channelized()), (fmt, count, k)


def test_past_the_cap_of_workgroups():
    """More than 256 * 2048 vectors: 256 workgroups, nine rounds of the grid-stride loop; the negative end sits in the
    first vector of the ninth round, a NaN and the positive end in the last vector."""
    fmt, decim, bs, raw = LC.big_case()
    assert LC.slices(fmt, decim * bs) == 256 and LC.passes(fmt, decim * bs) == 9
    w = _receiver(fmt, decim, bs)
    for k in range(2):
        w.demodulate(raw)
        lv = w.levels()
        assert lv.chunk == k and tuple(lv.input) == LC.want(raw, fmt), (k, tuple(lv.input), LC.want(raw, fmt))
    assert lv.input.peak == 32768 and lv.input.clipped == 3


@pytest.mark.parametrize("fmt", LC.FORMATS)
def test_accumulators_are_clean_between_chunks_in_flight(fmt):
    """Two chunks in flight, all-max and all-quiet in turn for six chunks on seven workgroups: every record is exactly its
    own chunk's - nothing of a loud chunk stays in the five device words."""
    decim, bs, loud, quiet = LC.sliced_pair(fmt)
    chunks = [loud, quiet, loud, quiet, quiet, loud]
    w = _receiver(fmt, decim, bs)
    got = []
    for k, c in enumerate(chunks):
        if k >= 2:
            w.fetch()
            got.append(w.levels())
        w.submit(c)
    for _ in range(2):
        w.fetch()
        got.append(w.levels())
    for k, (c, lv) in enumerate(zip(chunks, got)):
        assert lv.chunk == k and tuple(lv.input) == LC.want(c, fmt), (fmt, k, tuple(lv.input), LC.want(c, fmt))
    assert tuple(got[1].input) == tuple(got[3].input) == tuple(got[4].input) == ((1, 0, quiet.size) if fmt == "u8" else (0, 0, 0))
