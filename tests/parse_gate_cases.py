"""Inputs that work the device-side parse's gate (no tests in here; tests/test_parse_gate_cpu.py checks the conditions
below on the CPU, tests/test_parse_gate.py runs the cases on every device form).  Each case is one stream of bursts
with chosen payloads built by synth.synth_bursts; what is expected of it is oracle.dsp_oracle.parse_calls, which
tests/golden/parse_gate.json (tools/gen_golden_parse.py) pins to the real Parser for the production-config cases.

Production config, one case per block size (8192 x 5, 2048 x 12, 1024 x 24, 1000 x 24 blocks).  In time order:
  V0   a CRC-valid burst, transmitter 0, that starts at sample 20 (the zero state before block 0 lies next to it)
  V1   valid, placed so that the first sample at which its sync word matches is a block boundary: two consecutive
       calls report it, at index B and at index 0
  I0 I63 I6 I30 I17   one message bit flipped (numbered as the CRC takes them in): the first checked bit, the last bit
       of the CRC's low byte, a bit of the transmitter id, two others.  Sync-valid, CRC-invalid.
  S    a bit of the sync word flipped: no packet at all
  V4a V4b   byte-identical, in one call's window, at +1500 and -1500 Hz: one message (B >= 2048 only: a window reports
       positions 0 .. B and two whole packets of 1120 samples do not start inside 1024 of them)
  V6   its cfo tuned until mean * fs / 2 pi lies inside (-1, 1): int(), floor() and round() disagree there
  V2 V3 V5 V7   the remaining transmitter ids
5 of 15 (5 of 14) bursts are CRC-invalid.  At 2048 x 12 fifteen whole bursts do not fit in front of the last reported
position: there a burst starts inside its predecessor's trailing zero symbols and lead-in (synth_bursts: the earlier
burst keeps its samples), which costs it 11 of its 32 lead-in symbols.  Starts and cfos were tuned with the oracle.

Other packet lengths (block_size 512, 16 blocks): packet_symbols 24, 200, 256, 76, 16 at symbol_length 14 and 80 at
symbol_length 8; a valid and a CRC-invalid burst each.  packet_symbols 256 is two cases (k256_ok, k256_bad): the last
reported position is 8 blocks in front of the stream's end and a second 3584-sample packet does not start before it.
"""
import functools

import numpy as np

from oracle import dsp_oracle as O
from rtldavis_amd import synth

PREAMBLE = "1100101110001001"

_ROLES15 = ["V0", "V1", "I0", "I63", "V2", "I6", "V3", "S", "V4a", "V4b", "I30", "V5", "I17", "V6", "V7"]
_ROLES14 = [r for r in _ROLES15 if r != "V4b"]
_CFOS15 = [700.0, -450.0, -1200.0, 900.0, 1300.0, -800.0, -1700.0, 600.0, 1500.0, -1500.0, 400.0, -950.0, -300.0, None,
           1100.0]
_CFOS14 = [2400.0, -450.0, -1200.0, 900.0, 1500.0, -800.0, -1700.0, 600.0, 2300.0, 400.0, -950.0, -300.0, None, 1100.0]

# block size -> (blocks, noise seed, roles, burst starts, cfos with V6's tuned value filled in)
_PROD = {
    8192: (5, 9192, _ROLES15, [20, 7738] + [9424 + 1680 * k for k in range(13)], _CFOS15, 60.2),
    2048: (12, 3048, _ROLES15, [20, 1594] + [3132 + 1532 * k for k in range(13)], _CFOS15, 470.6),
    1024: (24, 2024, _ROLES14, [20, 1594] + [3280 + 1680 * k for k in range(12)], _CFOS14, 2096.0),
    1000: (24, 2000, _ROLES14, [20, 1546] + [3216 + 1664 * k for k in range(12)], _CFOS14, 2421.0),
}
PROD_BLOCK_SIZES = tuple(_PROD)
_HEAD = [0x88, 0x50, 0xE8, 0xA0, 0x28, 0x90, 0x70, 0x38]   # message byte 0 without the id: bit 3 set in half of them


def _body(k, n=6):
    return bytes([_HEAD[k % 8]] + [(k * 37 + j * 11 + 5) & 0xFF for j in range(1, n)])


def role_packet(role):
    """On-air bytes of a production-config burst."""
    if role[0] == "V":
        ident = int(role[1])
        return synth.make_packet(ident, _body(ident))
    if role[0] == "I":
        flip = int(role[1:])
        return synth.make_packet((flip + 2) % 8, _body(8 + flip % 5), flip_bit=flip)
    p = bytearray(synth.make_packet(5, _body(13)))
    p[1] ^= 0x08                                         # the sync word cb 89 -> cb 81
    return bytes(p)


class Case:
    """One stream: bursts [(on-air bytes, start, cfo)], roles, raw uint8 IQ, the oracle's config, per-call rows
    (parse_calls) and per-call (packets, discriminated, quantized)."""

    def __init__(self, name, cfg, n_blocks, seed, bursts, roles):
        self.name, self.cfg, self.n_blocks, self.seed, self.bursts, self.roles = name, cfg, n_blocks, seed, bursts, roles
        self.B = cfg.block_size
        self.raw = synth.synth_bursts(bursts, n_blocks * self.B, seed, symbol_length=cfg.symbol_length)
        self.raw.setflags(write=False)
        self.calls, self.states = O.parse_calls(self.blocks(), cfg, states=True)

    def blocks(self, kind="u8"):
        B = self.B
        if kind == "u8":
            return [self.raw[2 * B * b: 2 * B * (b + 1)] for b in range(self.n_blocks)]
        c = self.cplx()
        return [c[B * b: B * (b + 1)] for b in range(self.n_blocks)]

    def cplx(self):
        return ((self.raw.astype(np.float64) - 127.4) / 127.6).view(np.complex128)   # dsp.py:26,38-39

    def product_cfg(self):
        from rtldavis_amd import dsp
        c = self.cfg
        return dsp.PacketConfig(c.bit_rate, c.symbol_length, c.preamble_symbols, c.packet_symbols, c.preamble, c.block_size)


@functools.lru_cache(maxsize=None)
def prod_case(B, kind="u8", variant=0):
    """variant 0 is the case that meets every condition; variants 1 and 2 are further streams of the same block size
    for the handles that take several (other noise, every burst a few samples later, variant 2 with the cfos negated)."""
    nb, seed, roles, starts, cfos, tuned = _PROD[B]
    cfos = [tuned if c is None else c for c in cfos]
    if variant:
        starts = [s + (0, 5, 9)[variant] for s in starts]
        cfos = [-c if variant == 2 else c for c in cfos]
    bursts = [(role_packet(r), s, c) for r, s, c in zip(roles, starts, cfos)]
    case = Case(f"prod_b{B}_v{variant}", O.OracleConfig(19200, 14, 16, 80, PREAMBLE, B), nb, seed + variant, bursts,
                list(roles))
    if kind == "c128":   # the oracle on the complex blocks
        case.calls, case.states = O.parse_calls(case.blocks("c128"), case.cfg, states=True)
    return case


def _k76_packets():
    """76 symbols: the tenth byte holds 4 bits, shifted in from the right (dsp.py:197-200).  A valid message's CRC low
    byte, bit-reversed, must therefore be 0000xxxx; on air those four bits follow the ninth byte directly."""
    for k in range(1, 4096):
        body = bytes([0x50, k & 0xFF, k >> 8, 0x21, 0x43, 0x65])
        ota = synth.make_packet(3, body)
        if ota[9] < 16:
            bad = synth.make_packet(3, body, flip_bit=20)
            return [ota[:9] + bytes([ota[9] << 4]), bad[:9] + bytes([bad[9] << 4])]
    raise AssertionError("no such body")


def _other_specs():
    long25 = bytes((7 * j + 3) & 0xFF for j in range(21))
    long32 = bytes((13 * j + 1) & 0xFF for j in range(28))
    # name, packet_symbols, symbol_length, [(on-air bytes, start, cfo)]
    return [
        ("k24", 24, 14, [(bytes([0xCB, 0x89, 0x00]), 300, 500.0), (bytes([0xCB, 0x89, 0x20]), 2400, -700.0),
                         (bytes([0xCB, 0x89, 0x00]), 4500, -900.0)]),
        ("k200", 200, 14, [(synth.make_packet(2, long25, 25), 20, 800.0),
                           (synth.make_packet(5, long25, 25, flip_bit=183), 3400, -600.0)]),
        ("k256_ok", 256, 14, [(synth.make_packet(7, long32, 32), 40, -1100.0)]),
        ("k256_bad", 256, 14, [(synth.make_packet(4, long32, 32, flip_bit=0), 40, 900.0)]),
        ("k76", 76, 14, [(p, s, c) for p, (s, c) in zip(_k76_packets(), [(100, 650.0), (2300, -1250.0)])]),
        ("k16", 16, 14, [(bytes([0xCB, 0x89]), 200, 300.0), (bytes([0xCB, 0x89]), 3000, -400.0)]),
        ("s8", 80, 8, [(synth.make_packet(6, _body(6)), 64, 1000.0), (synth.make_packet(1, _body(9), flip_bit=63), 1200, -800.0),
                       (synth.make_packet(2, _body(2)), 2300, -1400.0)]),
    ]


OTHER_NAMES = ("k24", "k200", "k256_ok", "k256_bad", "k76", "k16", "s8")


@functools.lru_cache(maxsize=None)
def other_case(name):
    for n, K, S, bursts in _other_specs():
        if n == name:
            return Case(n, O.OracleConfig(19200, S, 16, K, PREAMBLE, 512), 16, 500 + K + S, bursts, None)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------- the comparison
def message_rows(calls, stream=0):
    """What parsed() must hold after each call: (stream, call, index, id, freq_err, on-air hex) of the CRC-valid rows."""
    return [[(stream, b, r[0], r[3], r[4], r[1]) for r in rows if r[2]] for b, rows in enumerate(calls)]


def assert_messages_equal(got, want, what=""):
    """got / want: per call, lists of (stream, call, index, id, freq_err, on-air hex).  Exact: no message of any case
    lies within 1e-6 of an integer Hz (checked on the CPU), so no frequency error is exempt."""
    assert len(got) == len(want), what
    for b, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{what} call {b}: got {g} want {w}"


def assert_packets_equal(got_calls, want_states, what="", db_tol=1e-3):
    """Packets of every call: index, bytes and order equal, rssi and snr within the project's 1e-3 dB."""
    assert len(got_calls) == len(want_states), what
    for b, (g, st) in enumerate(zip(got_calls, want_states)):
        w = st[0]
        assert [(int(p.index), bytes(p.data).hex()) for p in g] == [(int(p.index), bytes(p.data).hex()) for p in w], \
            f"{what} call {b}"
        for p, q in zip(g, w):
            for key in ("rssi", "snr"):
                a, e = float(getattr(p, key)), float(getattr(q, key))
                assert (a != a and e != e) or abs(a - e) <= db_tol, f"{what} call {b} {key}: {a} vs {e}"


def parsed_rows(arr):
    """parsed() array -> [(stream, call, index, id, freq_err, on-air hex)]"""
    out = []
    for r in arr:
        ota = bytes([0xCB, 0x89]) + bytes(O.swap_bit_order(int(b)) for b in r["data"][: int(r["nbytes"])])
        out.append((int(r["stream"]), int(r["call"]), int(r["index"]), int(r["id"]), int(r["freq_err"]), ota.hex()))
    return out


def assert_parsed_carry_their_packets(arr, packets_by_stream, what=""):
    """A parsed row's rssi and snr are its packet's, exactly."""
    for r in arr:
        ps = [p for p in packets_by_stream[int(r["stream"])] if p.index == int(r["index"])]
        assert ps, (what, r)
        assert any(r["rssi"] == p.rssi and r["snr"] == p.snr for p in ps), (what, r)
