"""CPU side of the parse-gate cases (tests/parse_gate_cases.py): the conditions every case must meet, the oracle's
parse_calls pinned to the real Parser (tests/golden/parse_gate.json, tools/gen_golden_parse.py), and the comparison the
GPU tests use shown to reject a catalogue of subtly wrong parsers."""
import copy
import hashlib
import math
import re

import numpy as np
import pytest

import parse_gate_cases as PG
from conftest import load_json
from oracle import dsp_oracle as O
from rtldavis_amd import synth


def _msgs(case):
    return [(b, r) for b, rows in enumerate(case.calls) for r in rows if r[2]]


def _twin_of(case, b, row):
    """Index of the same bytes elsewhere (> 1000 samples away) in call b's window, or None."""
    q = case.states[b][2]
    for i in O.search(q, case.cfg):
        if i <= case.B and abs(i - row[0]) > 1000 and O.slice_bytes(q, i, case.cfg).hex() == row[1]:
            return i
    return None


def test_make_packet_and_synth_bursts():
    for hexp in synth.OTA_PACKETS:   # the five packets of the reference's own tests are what make_packet builds
        b = bytes.fromhex(hexp)
        msg = bytes(O.swap_bit_order(x) for x in b[2:])
        assert synth.make_packet(msg[0] & 7, msg[:6]) == b
    for n in (5, 10, 25, 32):
        body = bytes(range(n - 4))
        for ident in range(8):
            p = synth.make_packet(ident, body, n)
            m = bytes(O.swap_bit_order(x) for x in p[2:])
            assert len(p) == n and p[:2] == b"\xcb\x89" and O.crc16_ccitt(m) == 0 and m[0] & 7 == ident
        for flip in range(8 * (n - 2)):
            q = synth.make_packet(3, body, n, flip_bit=flip)
            m = bytes(O.swap_bit_order(x) for x in q[2:])
            assert q[:2] == b"\xcb\x89" and O.crc16_ccitt(m) != 0
    # one burst where synth_stream puts it, same cfo: the same chips (the noise differs: other draws come first)
    rng = np.random.default_rng(3)
    payload = synth.OTA_PACKETS[int(rng.integers(0, 5))]
    start = int(rng.integers(8192, 4 * 8192 - 1680 - 8192))
    cfo = float(rng.uniform(-2000.0, 2000.0))
    a = synth.synth_stream(3, n_samples=4 * 8192, noise=0.0)
    b = synth.synth_bursts([(bytes.fromhex(payload), start, cfo)], 4 * 8192, 3, noise=0.0)
    on = slice(2 * start, 2 * (start + 1680))
    # synth_stream carries the cfo's phase from sample 0, synth_bursts from the burst's start: a constant rotation
    za = (a[on][0::2] - 127.4) + 1j * (a[on][1::2] - 127.4)
    zb = (b[on][0::2] - 127.4) + 1j * (b[on][1::2] - 127.4)
    rot = za * np.conj(zb)
    assert np.all(np.abs(np.angle(rot * np.conj(rot[0]))) < 0.05)
    assert np.all(a[: 2 * start] == b[: 2 * start]) and np.all(a[2 * (start + 1680):] == b[2 * (start + 1680):])


def test_existing_generators_are_unchanged(golden_streams):
    for seed in (0, 1, 63):
        raw = synth.synth_stream(seed)
        assert hashlib.sha256(raw.tobytes()).hexdigest() == golden_streams[str(seed)]["raw_sha256"]
    two = load_json("two_bursts.json")
    for seed, g in two.items():
        assert hashlib.sha256(synth.synth_two_bursts(int(seed), g["gap"]).tobytes()).hexdigest() == g["raw_sha256"]
    a, ia = synth.synth_wideband([21, 22], [-3e5, 2e5], 3 * 8192)
    b, ib = synth.synth_wideband([21, 22], [-3e5, 2e5], 3 * 8192, payloads=[synth.payload_of(21), synth.payload_of(22)])
    assert np.array_equal(a, b) and ia == ib
    c, ic = synth.synth_wideband([21, 22], [-3e5, 2e5], 3 * 8192, payloads=["cb89" + "00" * 8, synth.payload_of(22)])
    assert not np.array_equal(a, c) and ic[0] == ("cb89" + "00" * 8, ia[0][1]) and ic[1] == ia[1]


@pytest.mark.parametrize("B", PG.PROD_BLOCK_SIZES)
def test_production_case_conditions(B):
    case = PG.prod_case(B)
    roles, bursts = case.roles, case.bursts
    hexes = {r: bytes(o).hex() for r, (o, _, _) in zip(roles, bursts)}
    msgs = _msgs(case)
    rows = [(b, r) for b, rs in enumerate(case.calls) for r in rs]
    # the parser's own dedupe never drops a packet the demodulator kept (rd_parse.h)
    for b, rs in enumerate(case.calls):
        assert len(rs) == len(case.states[b][0])
    # all eight ids; every planted valid burst is a message, every CRC-invalid one a packet that fails the gate
    assert {r[3] for _, r in msgs} == set(range(8))
    for role, hx in hexes.items():
        got = [r for _, r in rows if r[1] == hx]
        if role[0] == "V":
            assert got and all(r[2] for r in got), role
        elif role[0] == "I":
            assert got and not any(r[2] for r in got), role
    n_bad = sum(r[0] == "I" for r in roles)
    assert 3 * n_bad >= len(roles)
    assert {"I0", "I63", "I6"} <= set(roles)   # first checked bit, last bit of the CRC's low byte, an id bit
    m0 = bytes(O.swap_bit_order(x) for x in bytes.fromhex(hexes["I6"])[2:])
    good = synth.make_packet((6 + 2) % 8, PG._body(8 + 6 % 5))
    assert (m0[0] ^ O.swap_bit_order(good[2])) == 0x02   # ... and it is inside the three id bits
    # the burst with the broken sync word: no packet anywhere near it, in any call
    k = roles.index("S")
    p_s = bursts[k][1] + 32 * 14
    nbk = case.cfg.buffer_length // B
    for b, r in rows:
        p_abs = (b + 1 - nbk) * B + r[0]
        assert not (p_s - 200 <= p_abs < p_s + 80 * 14), (b, r)
    assert bytes(bursts[k][0])[:2] != b"\xcb\x89"
    if B == 8192:   # >= 3 messages in one call with CRC-invalid packets between them in index order
        ok = False
        for rs in case.calls:
            srt = sorted(rs, key=lambda r: r[0])
            pat = "".join("V" if r[2] else "I" for r in srt)
            ok = ok or re.search(r"VI+VI+V", pat) is not None
        assert ok
        assert max(sum(1 for r in rs if r[2]) for rs in case.calls) >= 3
    # the twins
    if B >= 2048:
        ka, kb = roles.index("V4a"), roles.index("V4b")
        assert bytes(bursts[ka][0]) == bytes(bursts[kb][0]) and {bursts[ka][2], bursts[kb][2]} == {1500.0, -1500.0}
        tw = [(b, r) for b, r in msgs if r[1] == hexes["V4a"]]
        assert len(tw) == 1
        b, r = tw[0]
        other = _twin_of(case, b, r)
        assert other is not None, "the twins are not in one call's window"
        x_other = O.freq_error_x(case.states[b][1], other, case.cfg)
        assert abs(-int(x_other) - r[4]) > 1000
    else:
        assert B < 80 * 14   # two 1120-sample packets cannot both start inside one reported span of B samples
    # the boundary message: index B, then index 0
    bd = [(b, r[0]) for b, r in msgs if r[1] == hexes["V1"]]
    assert len(bd) == 2 and bd[0][1] == B and bd[1] == (bd[0][0] + 1, 0)
    # a burst inside the first 64 samples
    assert min(s for _, s, _ in bursts) < 64
    # both signs, one |x| < 1, nobody within 1e-6 of an integer
    xs = [r[5] for _, r in msgs]
    assert min(xs) < -100 and max(xs) > 100 and any(abs(x) < 1 for x in xs)
    assert all(abs(x - round(x)) >= 1e-6 for x in xs)


@pytest.mark.parametrize("name", PG.OTHER_NAMES)
def test_other_length_case_conditions(name):
    """packet_symbols 16 (2 bytes): no message bytes at all; the reference itself would index an empty msg_data
    (protocol.py:315), the project reports no message and no error (nbytes <= 2)."""
    case = PG.other_case(name)
    K = case.cfg.packet_symbols
    rows = [r for rs in case.calls for r in rs]
    planted = {}
    for ota, _, _ in case.bursts:
        bits = np.unpackbits(np.frombuffer(bytes(ota), np.uint8))[:K]
        pk = bytearray((K + 7) // 8)
        for i, v in enumerate(bits):
            pk[i >> 3] = ((pk[i >> 3] << 1) | int(v)) & 0xFF
        m = bytes(O.swap_bit_order(x) for x in pk[2:])
        planted[bytes(pk).hex()] = len(m) > 0 and O.crc16_ccitt(m) == 0
    for hx, ok in planted.items():
        got = [r for r in rows if r[1] == hx]
        assert got and all(r[2] == ok for r in got), (hx, ok)
    if name == "k16":
        assert not any(planted.values()) and not any(r[2] for r in rows)
    elif name.startswith("k256"):
        assert sum(planted.values()) == (name == "k256_ok")
        assert case.cfg.packet_symbols // 8 == 32
    else:
        assert any(planted.values()) and not all(planted.values())
    if name == "k24":
        assert [bytes.fromhex(h)[2] for h in planted] == [0x00, 0x20]
    for r in rows:
        if r[2]:
            assert abs(r[5] - round(r[5])) >= 1e-6


@pytest.mark.parametrize("B", PG.PROD_BLOCK_SIZES)
def test_no_message_of_any_stream_is_near_an_integer(B):
    """The exemption cap is zero: the GPU comparison is exact for every message, of the further streams and of the
    complex blocks too."""
    n = 0
    for kind, variant in (("u8", 0), ("u8", 1), ("u8", 2), ("c128", 0)):
        case = PG.prod_case(B, kind, variant)
        for _, r in _msgs(case):
            assert abs(r[5] - round(r[5])) >= 1e-6, (kind, variant, r)
            n += 1
    assert n >= 4 * 8


# ------------------------------------------------------------------------------------------------ the real parser
def test_parse_calls_equals_the_real_parser():
    fx = load_json("parse_gate.json")
    assert set(fx["cases"]) == {str(B) for B in PG.PROD_BLOCK_SIZES}
    for key, g in fx["cases"].items():
        case = PG.prod_case(int(key))
        assert hashlib.sha256(case.raw.tobytes()).hexdigest() == g["raw_sha256"]
        assert [(bytes(o).hex(), s, c) for o, s, c in case.bursts] == [(b["data"], b["start"], b["cfo"]) for b in g["bursts"]]
        assert g["seed"] == case.seed and len(g["calls"]) == case.n_blocks
        n_msg = 0
        for b, (rows, want) in enumerate(zip(case.calls, g["calls"])):
            assert [(r[0], r[1], r[2], r[3], r[4]) for r in rows] == \
                   [(w["index"], w["data"], w["crc_ok"], w["id"], w["freq_err"]) for w in want], (key, b)
            for w in want:
                assert w["crc_ok"] or not w["message"]   # every message the real parser returned is CRC-valid here
                n_msg += w["message"]
        assert n_msg >= 8


# ------------------------------------------------------------------------------------------------ teeth
def _crc(data, init=0):
    crc = init
    for byte in data:
        crc ^= byte << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def _model_rows(case, gate=None, ident=None, to_int=None, window=None):
    """parsed() of a parser that differs from the reference in one respect."""
    cfg = case.cfg
    out = []
    for b, (pk, disc, _) in enumerate(case.states):
        rows = []
        for p in pk:
            ota = bytes(p.data)
            data = bytes(O.swap_bit_order(x) for x in ota)
            if not (gate(data) if gate else _crc(data[2:]) == 0):
                continue
            lo, n = window(p.index, cfg.preamble_length) if window else (p.index, cfg.preamble_length)
            x = float(np.mean(disc[lo: lo + n]) * float(cfg.sample_rate) / (2 * math.pi))
            fe = -(to_int(x) if to_int else int(x))
            rows.append((0, b, int(p.index), ident(data, ota) if ident else data[2] & 7, fe, ota.hex()))
        out.append(rows)
    return out


def _rotate_fe(want):
    out = copy.deepcopy(want)
    for rows in out:
        if len(rows) >= 2:
            fes = [r[4] for r in rows]
            fes = fes[1:] + fes[:1]
            rows[:] = [r[:4] + (f,) + r[5:] for r, f in zip(rows, fes)]
    return out


def _dropped_twin(case, want):
    out = copy.deepcopy(want)
    hx = bytes(case.bursts[case.roles.index("V4a")][0]).hex()
    for b, rows in enumerate(out):
        for i, r in enumerate(rows):
            if r[5] == hx:
                q = _twin_of(case, b, (r[2], r[5]))
                x = O.freq_error_x(case.states[b][1], q, case.cfg)
                rows[i] = (r[0], r[1], q, r[3], -int(x), r[5])
    return out


def _boundary_once(want):
    out = copy.deepcopy(want)
    for rows in out:
        rows[:] = [r for r in rows if r[2] != 0]
    return out


WRONG = {
    "crc init 0xFFFF": dict(gate=lambda d: _crc(d[2:], 0xFFFF) == 0),
    "crc over data[0:]": dict(gate=lambda d: _crc(d) == 0),
    "crc skips the last byte": dict(gate=lambda d: _crc(d[2:-1]) == 0),
    "no gate": dict(gate=lambda d: True),
    "id = byte & 0xF": dict(ident=lambda d, ota: d[2] & 0xF),
    "id before the bit swap": dict(ident=lambda d, ota: ota[2] & 7),
    "floor for int": dict(to_int=math.floor),
    "round for int": dict(to_int=round),
    "window one sample early": dict(window=lambda i, n: (max(i - 1, 0), n)),
    "window of preamble_length - 1": dict(window=lambda i, n: (i, n - 1)),
}


@pytest.mark.parametrize("B", PG.PROD_BLOCK_SIZES)
def test_comparison_rejects_wrong_parsers(B):
    case = PG.prod_case(B)
    want = PG.message_rows(case.calls)
    PG.assert_messages_equal(_model_rows(case), want, "the right model")   # the harness itself
    models = {k: _model_rows(case, **kw) for k, kw in WRONG.items()}
    if B >= 2048:   # (a call of a smaller block reports one span of B < 1120 samples: never two whole packets)
        models["frequency errors of a call rotated"] = _rotate_fe(want)
    else:
        assert max(len(rows) for rows in want) == 1 and B < 80 * 14
    models["the boundary message in one call only"] = _boundary_once(want)
    if B >= 2048:
        models["the dropped twin's index and frequency error"] = _dropped_twin(case, want)
    for name, got in models.items():
        with pytest.raises(AssertionError):
            PG.assert_messages_equal(got, want, name)
        assert got != want, name
