"""The device-side parse (bit swap, CRC-16-CCITT gate, transmitter id, frequency error) in its five device forms against
oracle.dsp_oracle.parse_calls on inputs that work the gate (tests/parse_gate_cases.py; their conditions, the oracle's
agreement with the real Parser and the comparison's teeth are checked on the CPU in tests/test_parse_gate_cpu.py).
Every test compares parsed() row for row (stream, call, index, id, freq_err, on-air hex - exactly, no frequency error
is exempt), the packets of fetch() / demodulate() (index, bytes, order, rssi and snr within 1e-3 dB) and requires that a
parsed row carries its packet's rssi and snr."""
import numpy as np
import pytest

import parse_gate_cases as PG
from oracle import dsp_oracle as O
from rtldavis_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dsp():
    from rtldavis_amd import _lib, dsp as d
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    return d


def _want(cases):
    """Per call, the expected rows of all streams (stream-major), and per stream the oracle's states."""
    nb = cases[0].n_blocks
    per = [PG.message_rows(c.calls, i) for i, c in enumerate(cases)]
    return [[r for rows in per for r in rows[b]] for b in range(nb)]


def _stream_run(handle, cases, kind, multi):
    """Two blocks in flight; returns (parsed rows per call, packets per stream per call)."""
    nb = cases[0].n_blocks
    if multi:
        blocks = [np.stack([c.blocks()[b] for c in cases]) for b in range(nb)]
    else:
        blocks = cases[0].blocks(kind)
    handle.set_parse(True)
    rows, pk = [], [[] for _ in cases]

    def take():
        got = handle.fetch()
        per = got if multi else [got]
        arr = handle.parsed()
        rows.append(PG.parsed_rows(arr))
        PG.assert_parsed_carry_their_packets(arr, per, cases[0].name)
        for i, ps in enumerate(per):
            pk[i].append(ps)

    handle.submit(blocks[0])
    for b in range(1, nb):
        handle.submit(blocks[b])
        assert handle.inflight == 2
        take()
    take()
    return rows, pk


def _check_stream(handle, cases, kind="u8", multi=False):
    rows, pk = _stream_run(handle, cases, kind, multi)
    what = f"{cases[0].name} {kind}"
    PG.assert_messages_equal(rows, _want(cases), what)
    for i, c in enumerate(cases):
        PG.assert_packets_equal(pk[i], c.states, f"{what} stream {i}")
    return rows


# ------------------------------------------------------------------------------------------------ batch
def _check_batch(dsp, cases, what):
    from rtldavis_amd import batch
    nb = cases[0].n_blocks
    bd = batch.BatchDemodulator(cases[0].product_cfg(), len(cases), nb)
    bd.set_parse(True)
    bd.upload(np.stack([c.raw for c in cases]))
    bd.run()
    arr = bd.parsed()
    want = [r for i, c in enumerate(cases) for rows in PG.message_rows(c.calls, i) for r in rows]
    got = PG.parsed_rows(arr)
    assert got == want, f"{what}: {[(g, w) for g, w in zip(got, want) if g != w][:4]} {len(got)} {len(want)}"
    res = bd.packets()
    for i, c in enumerate(cases):
        PG.assert_packets_equal(res[i], c.states, f"{what} stream {i}")
    pk = {(s, cl, p.index): p for s, cl, p in bd.records()}
    for r in arr:
        p = pk[(int(r["stream"]), int(r["call"]), int(r["index"]))]
        assert r["rssi"] == p.rssi and r["snr"] == p.snr
    forms = bd.last_run_forms()
    bd.close()
    return forms


@pytest.mark.parametrize("tail", [None, "legacy"])
@pytest.mark.parametrize("B,n_streams", [(8192, 4), (2048, 4), (2048, 72), (1024, 4), (1000, 4), (1000, 72)])
def test_batch(dsp, monkeypatch, B, n_streams, tail):
    """The stacked streams of one block size through k_parse_select + k_freq_err: behind the default one-launch tail and
    behind the separate kernels (RD_TAIL_IMPL=legacy: k_classify + k_rssi_u8, the dense record layout).  72 streams:
    the survivors span more than one wave and more than one workgroup of k_parse_select."""
    if tail is None:
        monkeypatch.delenv("RD_TAIL_IMPL", raising=False)
    else:
        monkeypatch.setenv("RD_TAIL_IMPL", tail)
    cases = [PG.prod_case(B, "u8", k % 3) for k in range(n_streams)]
    assert sum(len(r) for c in cases for r in PG.message_rows(c.calls)) > (256 if n_streams > 64 else 8)
    forms = _check_batch(dsp, cases, f"batch B={B} x{n_streams} {tail}")
    if tail == "legacy":
        assert not forms["one_launch_tail"]


@pytest.mark.parametrize("name", PG.OTHER_NAMES)
def test_batch_other_packet_lengths(dsp, name):
    """3, 25, 32 and 9.5-byte packets and symbol_length 8 (the sparse record layout of k_slice_rssi); 2 bytes: no
    message and no error, where the reference itself would index an empty msg_data (protocol.py:315)."""
    _check_batch(dsp, [PG.other_case(name)], f"batch {name}")


# ------------------------------------------------------------------------------------------------ one-launch blocks
@pytest.mark.parametrize("kind", ["u8", "c128"])
@pytest.mark.parametrize("B", [8192, 2048])
def test_one_launch_block(dsp, B, kind):
    """Demodulator, two blocks in flight: uint8 blocks (rd_wave_parse in the one-launch block) and the same stream as
    complex128 blocks (the block shared by four workgroups), the oracle run on the complex blocks."""
    case = PG.prod_case(B, kind)
    rows = _check_stream(dsp.Demodulator(case.product_cfg()), [case], kind)
    assert {r[3] for rs in rows for r in rs} == set(range(8))


def test_one_launch_block_three_streams(dsp):
    """MultiDemodulator, three different streams at B = 2048: the gather is stream-major, kept[] non-trivial."""
    cases = [PG.prod_case(2048, "u8", v) for v in range(3)]
    _check_stream(dsp.MultiDemodulator(cases[0].product_cfg(), 3), cases, multi=True)


# ------------------------------------------------------------------------------------------------ multi-launch form
@pytest.mark.parametrize("B", [1024, 1000])
def test_multi_launch_form(dsp, B):
    """k_stream_parse behind the slice kernel: uint8 single, uint8 three streams, complex128 single."""
    case = PG.prod_case(B)
    _check_stream(dsp.Demodulator(case.product_cfg()), [case])
    cases = [PG.prod_case(B, "u8", v) for v in range(3)]
    _check_stream(dsp.MultiDemodulator(case.product_cfg(), 3), cases, multi=True)
    cc = PG.prod_case(B, "c128")
    _check_stream(dsp.Demodulator(cc.product_cfg()), [cc], "c128")


@pytest.mark.parametrize("name", PG.OTHER_NAMES)
def test_multi_launch_form_other_packet_lengths(dsp, name):
    """As test_batch_other_packet_lengths, on the streaming handle (block_size 512: the multi-launch form)."""
    case = PG.other_case(name)
    rows = _check_stream(dsp.Demodulator(case.product_cfg()), [case])
    if name == "k16":
        assert not any(rows)


# ------------------------------------------------------------------------------------------------ wideband
WB_CHANNELS = [0, 25, 26]          # a band edge, the centre, the centre + 1
WB_SEEDS = [41, 42, 43, 44, 48, 53]   # the valid bursts start in chunk 2, the CRC-invalid ones in chunk 1


def _wb_payloads():
    good = [synth.make_packet(i, PG._body(i)).hex() for i in (2, 5, 7)]
    bad = [synth.make_packet(i, PG._body(8 + i), flip_bit=f).hex() for i, f in ((3, 0), (4, 63), (6, 6))]
    return good + bad


@pytest.mark.parametrize("fmt", ["u8", "s16"])
def test_wideband(fmt):
    """Three channels, per channel one valid burst (ids 2, 5, 7) and one CRC-invalid one, four chunks, two in flight.
    Expected: parse_calls on the bytes channelized() returns for each chunk (those bytes are pinned to the float64
    model in tests/test_channelizer*.py; nothing of the channelizer is restated here)."""
    from rtldavis_amd import _lib, dsp, wideband
    from rtldavis_amd import channelizer as CZ
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    B, NK = 8192, 4
    cfg = dsp.PacketConfig(19200, 14, 16, 80, PG.PREAMBLE, B)
    chans = [CZ.US_CHANNELS_HZ[c] for c in WB_CHANNELS]
    shifts = [f - CZ.DEFAULT_CENTRE_HZ for f in chans] * 2
    payloads = _wb_payloads()
    raw, info = synth.synth_wideband(WB_SEEDS, shifts, NK * B, sample_format=fmt, payloads=payloads)
    for c in range(3):   # the two bursts of a channel do not overlap
        assert abs(info[c][1] - info[c + 3][1]) > 1680 + 64, info
    w = wideband.WidebandReceiver(cfg, chans, sample_format=fmt)
    w.set_parse(True)
    n_el = w.chunk_bytes // raw.itemsize
    chunks = [raw[n_el * k: n_el * (k + 1)] for k in range(NK)]
    got, got_pk, got_bytes = [], [], []

    def take():
        per = w.fetch()
        arr = w.parsed()
        PG.assert_parsed_carry_their_packets(arr, per, fmt)
        got_pk.append(per)
        got.append(PG.parsed_rows(arr))
        got_bytes.append(w.channelized())

    w.submit(chunks[0])
    for k in range(1, NK):
        w.submit(chunks[k])
        take()
    take()
    ocfg = O.OracleConfig(19200, 14, 16, 80, PG.PREAMBLE, B)
    want = [[] for _ in range(NK)]
    seen_ok, seen_bad = set(), set()
    for c in range(3):
        calls, states = O.parse_calls([got_bytes[k][c] for k in range(NK)], ocfg, states=True)
        for k, rows in enumerate(PG.message_rows(calls, c)):
            want[k] += rows
        PG.assert_packets_equal([got_pk[k][c] for k in range(NK)], states, f"{fmt} channel {c}")
        for rows in calls:
            for r in rows:
                assert abs(r[5] - round(r[5])) >= 1e-6 or not r[2], r
                (seen_ok if r[2] else seen_bad).add((c, r[1]))
    PG.assert_messages_equal(got, want, fmt)
    for c in range(3):   # every channel's valid burst is a message, its CRC-invalid one a packet the gate refused
        assert (c, payloads[c]) in seen_ok and (c, payloads[c + 3]) in seen_bad, (c, seen_ok, seen_bad)
