"""WidebandReceiver.set_parse / parsed() (rd_wb_set_parse, rd_wb_parsed): the CRC-valid messages of every channel with
their frequency errors, chunk k's while chunk k+1 is in flight - which discriminated(channel), the state after the
NEWEST chunk, cannot give.  Expected values: a synchronous receiver with parse off, parse_packet on its packets and the
reference's formula (protocol.py:304-311) on its discriminated(channel) mirror."""
import numpy as np
import pytest

from rtldavis_amd import synth
from stream_parse_helpers import _cfg, _host_expected, _oracle_expected, _pkey, _rows, assert_rows_match

B = 8192
SIX = [0, 7, 24, 25, 26, 50]   # both band edges, the centre and its neighbours
SEEDS = [21, 22, 23, 24, 25, 26]
NK = 5


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["u8", "s16"])
def test_wideband_parsed_with_two_chunks_in_flight(fmt):
    from rtldavis_amd import _lib, dsp, wideband
    from rtldavis_amd import channelizer as CZ
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    cfg = _cfg()
    chans = [CZ.US_CHANNELS_HZ[c] for c in SIX]
    raw, _ = synth.synth_wideband(SEEDS, [f - CZ.DEFAULT_CENTRE_HZ for f in chans], NK * B, sample_format=fmt)
    quiet = wideband.WidebandReceiver(cfg, chans, sample_format=fmt)
    n_el = quiet.chunk_bytes // raw.itemsize
    chunks = [raw[n_el * k: n_el * (k + 1)] for k in range(NK)]
    want, want_pk, want_bytes = [], [], []
    for k in range(NK):
        per = quiet.demodulate(chunks[k])
        want_pk.append(_pkey(per))
        want_bytes.append(quiet.channelized())
        rows = []
        for c, ps in enumerate(per):
            rows += _host_expected(dsp, cfg, ps, lambda c=c: quiet.discriminated(c), c, k)
        want.append(rows)
    with pytest.raises(RuntimeError, match="parse off"):
        quiet.parsed()

    w = wideband.WidebandReceiver(cfg, chans, sample_format=fmt)
    w.set_parse(True)
    got, got_pk, got_bytes = [], [], []

    def take():
        got_pk.append(_pkey(w.fetch()))
        got.append(_rows(w.parsed()))
        got_bytes.append(w.channelized())

    w.submit(chunks[0])
    for k in range(1, NK):
        w.submit(chunks[k])            # chunk k's copy runs beside chunk k-1's kernels
        assert w.inflight == 2
        if k == 1:
            with pytest.raises(RuntimeError, match="in flight"):
                w.set_parse(False)     # refused with chunks in flight, nothing consumed
            assert w.inflight == 2
        take()
        assert w.inflight == 1         # chunk k is still in flight while chunk k-1's messages are read
    take()
    strict = sum(assert_rows_match(got[k], want[k], (fmt, k)) for k in range(NK))
    assert strict >= 1
    # ... and the independent oracle on the channelized bytes of every chunk
    orc = _oracle_expected([[got_bytes[k][c] for k in range(NK)] for c in range(len(SIX))], B)
    assert sum(assert_rows_match(got[k], orc[k], ("oracle", fmt, k)) for k in range(NK)) >= 1
    msgs = [r for rows in got for r in rows]
    assert {r[0] for r in msgs} == set(range(len(SIX)))            # every channel yields at least one message
    for r in msgs:
        assert r[5] == synth.payload_of(SEEDS[r[0]]), r            # ... and it is the burst that channel carries
    # the flag changes neither the packets nor the channelized bytes
    assert got_pk == want_pk
    for k in range(NK):
        assert np.array_equal(got_bytes[k], want_bytes[k]), k
