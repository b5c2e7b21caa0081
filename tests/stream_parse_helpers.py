"""Helpers shared by tests/test_stream_parse.py and tests/test_wideband_parse.py (no tests in here): the production
packet configuration, a bitwise CRC and bit swap written independently of the code under test, row keys of parsed()
arrays and of the fixtures, and the expected values a quiet synchronous handle gives through the reference's formula
(protocol.py:290-318) with the comparison rule that goes with them."""
import math

import numpy as np

PREAMBLE = "1100101110001001"


def _cfg(block_size=8192):
    from rtldavis_amd import dsp
    return dsp.PacketConfig(19200, 14, 16, 80, PREAMBLE, block_size)


def _swap(b):
    return int(f"{b:08b}"[::-1], 2)


def _crc16_bitwise(data):
    """CRC-16-CCITT, poly 0x1021, init 0, one bit at a time."""
    crc = 0
    for byte in data:
        for bit in range(7, -1, -1):
            top = (crc >> 15) & 1
            crc = ((crc << 1) & 0xFFFF) | 0
            if top ^ ((byte >> bit) & 1):
                crc ^= 0x1021
    return crc


def _ota(row):
    """on-air packet hex of a parsed() row (un-swap, sync word back in front)"""
    return (bytes([0xCB, 0x89]) + bytes(_swap(int(b)) for b in row["data"][: int(row["nbytes"])])).hex()


def _rows(arr):
    return [(int(r["stream"]), int(r["call"]), int(r["index"]), int(r["id"]), int(r["freq_err"]), _ota(r)) for r in arr]


def _want_rows(golden_streams, seeds, call):
    out = []
    for i, seed in enumerate(seeds):
        for m in golden_streams[str(seed)]["parse"].get(str(call), []):
            out.append((i, call, m["index"], m["id"], m["freq_err"], m["data"]))
    return out


def _pkey(per_stream):
    return [[(p.index, bytes(p.data), p.rssi, p.snr) for p in ps] for ps in per_stream]


def _host_expected(dsp, cfg, packets, disc, stream, call):
    """The reference's formula (protocol.py:290-318) on a quiet handle's packets and discriminated() mirror:
    [(row, x)] with x = mean * fs / 2 pi before int()."""
    out = []
    for p in packets:
        r = dsp.parse_packet(p.data)
        if r is None:
            continue
        ident, msg = r
        mean = np.mean(disc()[p.index: p.index + cfg.preamble_length])
        x = (mean * float(cfg.sample_rate)) / (2 * math.pi)
        ota = (bytes([0xCB, 0x89]) + bytes(_swap(b) for b in msg)).hex()
        out.append(((stream, call, int(p.index), ident, -int(x), ota), x))
    return out


def _oracle_expected(blocks_per_stream, block_size):
    """The same, from the independent oracle (oracle.dsp_oracle.parse_calls: OracleDemodulator, crc16_ccitt,
    swap_bit_order, freq_error) on the input blocks themselves: per call, [(row, x)] of all streams, stream-major."""
    from oracle import dsp_oracle as O
    cfg = O.OracleConfig(19200, 14, 16, 80, PREAMBLE, block_size)
    per = [O.parse_calls(blocks, cfg) for blocks in blocks_per_stream]
    return [[((s, b, r[0], r[3], r[4], r[1]), r[5]) for s, calls in enumerate(per) for r in calls[b] if r[2]]
            for b in range(len(per[0]))]


def assert_rows_match(got, want_x, what):
    """Equality; where mean * fs / 2 pi lies within 1e-6 of an integer (the two sides sum the same float64 values in a
    different order) the frequency error may differ by 1 Hz.  Returns how many messages did not need the exception."""
    assert [g[:4] + g[5:] for g in got] == [w[:4] + w[5:] for w, _ in want_x], what
    strict = 0
    for g, (w, x) in zip(got, want_x):
        if abs(x - round(x)) < 1e-6:
            assert abs(g[4] - w[4]) <= 1, (what, g, w, x)
        else:
            assert g[4] == w[4], (what, g, w, x)
            strict += 1
    return strict
