"""protocol.Parser.parse's front half inside the STREAMING kernels (Demodulator / MultiDemodulator.set_parse, parsed();
rd_demod_set_parse, rd_demod_parsed, rd_parse_packet; rtldavis_amd/csrc/rd_parse.h): bit swap, CRC-16-CCITT gate,
transmitter id and the frequency error from the discriminator state right after each block - with later blocks in
flight - and the worker loop built on it (worker.pipelined_worker_loop).  The wideband receiver's side is in
tests/test_wideband_parse.py.  Expected values: tests/golden/streams.json (the real Parser's output per stream and call),
and, where no fixture exists, a quiet synchronous handle's packets and discriminated() mirror through the reference's
formula."""
import ctypes as C
import os
import queue
import re
import threading

import numpy as np
import pytest

from conftest import dense_calls
from rtldavis_amd import synth
from stream_parse_helpers import (_cfg, _crc16_bitwise, _host_expected, _oracle_expected, _pkey, _rows, _swap,
                                  _want_rows, assert_rows_match)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ CPU
def test_parse_packet_agrees_with_the_fixtures(golden_streams):
    """Every packet recorded in streams.json: valid exactly for those listed under `parse`, equal id and bytes."""
    from rtldavis_amd import parse_packet
    n_valid = 0
    for seed, g in golden_streams.items():
        for call, pkts in g["calls"].items():
            want = {m["index"]: m for m in g["parse"].get(call, [])}
            got = {}
            for p in pkts:
                r = parse_packet(bytes.fromhex(p["data"]))
                if r is not None:
                    ident, msg = r
                    ota = bytes([0xCB, 0x89]) + bytes(_swap(b) for b in msg)
                    got[p["index"]] = (ident, ota.hex())
            assert got == {i: (m["id"], m["data"]) for i, m in want.items()}, (seed, call)
            n_valid += len(got)
        assert set(g["parse"]) <= set(g["calls"])
    assert n_valid >= len(golden_streams)


def test_parse_packet_crc_gate():
    from rtldavis_amd import dsp, parse_packet
    for hexp in synth.OTA_PACKETS:
        data = bytes.fromhex(hexp)
        ident, msg = parse_packet(data)
        assert msg == bytes(_swap(b) for b in data[2:]) and ident == msg[0] & 7
        assert parse_packet(np.frombuffer(data, np.uint8)) == (ident, msg)
        for bit in range(16, 80):   # any single bit of the checked bytes flipped: invalid
            bad = bytearray(data)
            bad[bit // 8] ^= 1 << (bit % 8)
            assert parse_packet(bytes(bad)) is None, (hexp, bit)
        for bit in range(16):       # the sync word is not under the CRC (protocol.py:297 checks data[2:])
            same = bytearray(data)
            same[bit // 8] ^= 1 << (bit % 8)
            assert parse_packet(bytes(same)) == (ident, msg)
    for n in (0, 1, 2):
        assert parse_packet(bytes(n)) is None   # nbytes <= 2
    assert dsp.parse_packet is parse_packet
    with pytest.raises(ValueError):
        parse_packet(bytes(33))
    rng = np.random.default_rng(20)
    n_ok = 0
    for k in range(2000):
        data = rng.integers(0, 256, 10, dtype=np.uint8)
        if k % 50 == 0:   # a share of valid ones: random payload, the CRC appended
            body = bytes(int(b) for b in data[2:8])
            crc = _crc16_bitwise(body)
            sw = body + bytes([crc >> 8, crc & 0xFF])
            data[2:] = [_swap(b) for b in sw]
        want = _crc16_bitwise(bytes(_swap(int(b)) for b in data[2:])) == 0
        got = parse_packet(data)
        assert (got is not None) == want, k
        n_ok += want
    assert n_ok >= 40


def test_parse_packet_under_sanitizers():
    """rd_parse_packet lives in the pure-host translation unit: built here with ASan + UBSan (the GPU pool allows no
    sanitizer runs) and driven with exactly sized buffers of every length (tests/parse_asan.cpp)."""
    import subprocess
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "parse_asan")
    srcs = [os.path.join(ROOT, "tests", "parse_asan.cpp"), os.path.join(ROOT, "rtldavis_amd", "csrc", "rd_host.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Wextra", "-o", exe] + srcs)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for seed in (1, 2):
        r = subprocess.run([exe, str(seed)], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "parse ok" in r.stdout, f"{r.stdout}\n{r.stderr[-3000:]}"
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_new_symbols_declared_exported_and_in_the_ctypes_table():
    from rtldavis_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtldavis_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rd_[a-z0-9_]+)\s*\(", src))
    L = _lib.lib()
    for n in ("rd_parse_packet", "rd_demod_set_parse", "rd_demod_parsed", "rd_wb_set_parse", "rd_wb_parsed"):
        assert n in declared and n in _lib.SIGNATURES and hasattr(L, n), n
    # the records' layouts are what they were
    assert C.sizeof(_lib.RdParsed) == 6 * 4 + 32 + 2 * 8 and C.sizeof(_lib.RdPacket) == 4 * 4 + 32 + 2 * 8


def test_call_order_without_a_device():
    """set_parse is host state only (safe before fork, like construction); parsed() before any fetch is a state
    error, not a crash and not a device call."""
    from rtldavis_amd import _lib, dsp, wideband
    dem = dsp.Demodulator(_cfg())
    n = C.c_int(-1)
    buf = (_lib.RdParsed * 4)()
    assert _lib.lib().rd_demod_parsed(dem._h, buf, 4, C.byref(n)) == _lib.RD_ERR_STATE
    dem.set_parse(True)
    assert _lib.lib().rd_demod_parsed(dem._h, buf, 4, C.byref(n)) == _lib.RD_ERR_STATE
    with pytest.raises(RuntimeError):
        dem.parsed()
    dem.set_parse(False)
    md = dsp.MultiDemodulator(_cfg(), 3)
    md.set_parse(True)
    with pytest.raises(RuntimeError):
        md.parsed()
    w = wideband.WidebandReceiver(_cfg(), channels_hz=[914963100])
    w.set_parse(True)
    with pytest.raises(RuntimeError):
        w.parsed()
    assert _lib.lib().rd_demod_set_parse(None, 1) == _lib.RD_ERR_ARG
    assert _lib.lib().rd_wb_parsed(None, buf, 4, C.byref(n)) == _lib.RD_ERR_ARG


# ---- the pipelined worker loop on a fake demodulator and a stand-in parser ----
ROW = np.dtype([("stream", "<i4"), ("call", "<i4"), ("index", "<i4"), ("freq_err", "<i4"), ("id", "<i4"), ("nbytes", "<i4"),
                ("data", "u1", (32,)), ("rssi", "<f8"), ("snr", "<f8")])


class Pkt:
    def __init__(self, index, data):
        self.index, self.data, self.rssi, self.snr = index, data, -30.0, 10.0


class FakeDem:
    """Records its calls.  Block v (the first byte of the block) carries one packet at index 100 + v whose message is
    from transmitter v % 3 with frequency error 10 v; block 5's fetch fails on the device side and drops the block."""

    def __init__(self):
        self.flight, self.log, self.max_flight, self.parse_on, self.last = [], [], 0, False, None

    def set_parse(self, on):
        self.parse_on = bool(on)
        self.log.append(("set_parse", on))

    def submit(self, block):
        if block.size != 4:
            raise ValueError("Incompatible array sizes")
        assert len(self.flight) < 2, "a third block in flight"
        self.flight.append(int(block[0]))
        self.max_flight = max(self.max_flight, len(self.flight))
        self.log.append(("submit", int(block[0])))

    @property
    def inflight(self):
        return len(self.flight)

    def fetch(self):
        v = self.flight.pop(0)
        self.log.append(("fetch", v, len(self.flight)))
        if v == 5:
            self.last = None
            raise RuntimeError("device lost")
        self.last = v
        return [Pkt(100 + v, bytes([0xCB, 0x89, v]))]

    def parsed(self):
        assert self.parse_on and self.last is not None
        r = np.zeros(1, ROW)
        v = self.last
        r["index"], r["freq_err"], r["id"], r["nbytes"] = 100 + v, 10 * v, v % 3, 8
        r["data"][0, :8] = [v % 3 | 0x20, v, 0, 0, 0, 0, 0, 0]
        return r


class StandInParser:
    """The attributes and the one method of protocol.Parser the back half of parse() touches (protocol.py:318-337)."""
    max_tr_ch_list = 4

    def __init__(self, station_id=None):
        self.cfg = None
        self.demodulator = FakeDem()
        self.station_id = station_id
        self.hop_pattern = [3, 1, 2]
        self.hop_idx = 1
        self.transmitter = 0
        self.freq_err_tr_ch_list = [[[0] * self.max_tr_ch_list for _ in range(5)] for _ in range(8)]
        self.freq_err_tr_ch_ptr = [[0] * 5 for _ in range(8)]
        self.seen = []

    def _parse_sensor_data(self, pkt, msg_id, msg_data):
        self.seen.append((pkt.index, bytes(pkt.data), msg_id, msg_data))
        if msg_data[1] == 7:
            raise RuntimeError("decoder blew up")   # logged, block dropped, loop goes on
        if msg_data[1] == 8:
            return None                              # a message the parser does not decode
        return ("msg", msg_id, msg_data[1])


def _run_pipelined(parser, values, **kw):
    from rtldavis_amd import worker
    dq, rq = queue.Queue(), queue.Queue()
    for v in values:
        dq.put(None if v is None else np.zeros(3, np.uint8) if v == "bad" else np.full(4, v, np.uint8))
    t = threading.Thread(target=worker.pipelined_worker_loop, args=(dq, rq, lambda: parser), kwargs=dict(poll_s=0.02, **kw))
    t.start(); t.join(20)
    assert not t.is_alive()
    got = []
    while not rq.empty():
        got.append(rq.get())
    return got


def test_pipelined_worker_loop_two_in_flight_order_errors_and_drain():
    p = StandInParser()
    got = _run_pipelined(p, [0, 1, 2, 3, 4, 5, 6, "bad", 7, 8, 9, 10, None, 11])
    dem = p.demodulator
    assert dem.log[0] == ("set_parse", True)
    # two blocks really are in flight: from the third block on, every fetch leaves one behind
    assert dem.max_flight == 2
    assert [e for e in dem.log if e[0] == "fetch" and e[1] in (0, 1, 2, 3)] == [("fetch", v, 1) for v in (0, 1, 2, 3)]
    # block order; 5: fetch raised (dropped), "bad": submit raised, 7: the decoder raised, 8: not decoded
    assert got == [("msg", v % 3, v) for v in (0, 1, 2, 3, 4, 6, 9, 10)]
    # the stop sentinel drains what is in flight and nothing behind it is taken
    assert dem.flight == [] and ("submit", 11) not in dem.log
    assert [e[1] for e in dem.log if e[0] == "submit"] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
    assert [e[1] for e in dem.log if e[0] == "fetch"] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
    # the decoder was handed the packet with the on-air bytes, the id and the swapped message bytes
    assert p.seen[1] == (101, bytes([0xCB, 0x89, 1]), 1, bytes([0x21, 1, 0, 0, 0, 0, 0, 0]))


def test_pipelined_worker_loop_filter_and_frequency_error_ring():
    """protocol.py:318-337: every CRC-valid message feeds the ring of (its transmitter, the current hop channel) and
    moves `transmitter`, whether or not the station filter then drops it."""
    p = StandInParser(station_id=1)
    got = _run_pipelined(p, list(range(12)) + [None])
    fetched = [v for v in range(12) if v != 5]
    assert got == [("msg", 1, v) for v in fetched if v % 3 == 1 and v not in (7,)]
    ch = p.hop_pattern[p.hop_idx]
    for tr in range(3):
        errs = [10 * v for v in fetched if v % 3 == tr]
        ring = [0] * p.max_tr_ch_list
        for k, e in enumerate(errs):
            ring[k % p.max_tr_ch_list] = e      # a ring: the oldest entry is overwritten
        assert p.freq_err_tr_ch_list[tr][ch] == ring, tr
        assert p.freq_err_tr_ch_ptr[tr][ch] == len(errs) % p.max_tr_ch_list
        for other in range(5):
            if other != ch:
                assert p.freq_err_tr_ch_list[tr][other] == [0] * p.max_tr_ch_list
    assert p.transmitter == 11 % 3
    assert all(s[2] == 1 for s in p.seen)   # the decoder only ever saw station 1


def test_pipelined_worker_loop_failing_factory_idle_polls_and_main_signature():
    import inspect
    import time
    from rtldavis_amd import worker

    def bad():
        raise RuntimeError("no parser")

    worker.pipelined_worker_loop(queue.Queue(), queue.Queue(), bad, poll_s=0.01)   # returns, like worker.py:30-32
    assert list(inspect.signature(worker.pipelined_worker_main).parameters) == \
        list(inspect.signature(worker.worker_main).parameters)
    assert list(inspect.signature(worker.pipelined_worker_loop).parameters) == \
        list(inspect.signature(worker.worker_loop).parameters)
    p = StandInParser()
    dq, rq = queue.Queue(), queue.Queue()
    t = threading.Thread(target=worker.pipelined_worker_loop, args=(dq, rq, lambda: p), kwargs=dict(poll_s=0.01))
    t.start()
    time.sleep(0.1)
    dq.put(np.full(4, 4, np.uint8))
    assert rq.get(timeout=2) == ("msg", 1, 4)   # delivered without waiting for a further block
    dq.put(None)
    t.join(10)
    assert not t.is_alive()


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def dsp():
    from rtldavis_amd import _lib, dsp as d
    assert _lib.lib().rd_device_count() > 0, "no HIP device: the GPU tests need an MI355X"
    return d


@pytest.mark.gpu
def test_multi_demodulator_parsed_with_two_blocks_in_flight(dsp, golden_streams):
    """Five receivers in lock step, parse on, two blocks in flight: parsed() after each fetch - the next block still in
    flight - equals the real Parser's output for that block; the packets are those of a run with parse off."""
    seeds = [0, 1, 2, 3, 17]
    raws = synth.synth_streams(seeds)
    nb, B = synth.BLOCKS_PER_STREAM, 8192
    cfg = _cfg()
    plain = dsp.MultiDemodulator(cfg, len(seeds))
    want_pk = [_pkey(plain.demodulate(raws[:, 2 * B * b: 2 * B * (b + 1)])) for b in range(nb)]
    with pytest.raises(RuntimeError):
        plain.parsed()   # fetched, but with parse off
    md = dsp.MultiDemodulator(cfg, len(seeds))
    md.set_parse(True)
    got_pk, got_rows = [], []

    def take():
        got_pk.append(_pkey(md.fetch()))
        got_rows.append(_rows(md.parsed()))
        assert _rows(md.parsed()) == got_rows[-1]   # any number of times

    md.submit(raws[:, : 2 * B])
    for b in range(1, nb):
        md.submit(raws[:, 2 * B * b: 2 * B * (b + 1)])
        assert md.inflight == 2
        take()
        assert md.inflight == 1   # block b is still in flight while block b-1's messages are read
    take()
    n_msgs = 0
    for b in range(nb):
        assert got_rows[b] == _want_rows(golden_streams, seeds, b), f"block {b}"
        assert got_pk[b] == want_pk[b], f"block {b}"
        n_msgs += len(got_rows[b])
    assert n_msgs == len(seeds)
    # rssi / snr are the packet's
    md.reset()
    with pytest.raises(RuntimeError):
        md.parsed()   # nothing fetched since reset


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 5])
def test_single_demodulator_parsed_uint8_and_complex128(dsp, golden_streams, seed):
    """The same stream as uint8 blocks (k_stream_block) and as complex128 blocks (k_stream_block_cplx), two in flight:
    both give the fixture's messages."""
    raw = synth.synth_stream(seed)
    B, nb = 8192, synth.BLOCKS_PER_STREAM
    cplx = ((raw.astype(np.float64) - 127.4) / 127.6).view(np.complex128)   # dsp.py:26,38-39
    want = [_want_rows(golden_streams, [seed], b) for b in range(nb)]
    assert sum(len(w) for w in want) == 1
    want_calls = dense_calls(golden_streams[str(seed)]["calls"], nb)
    for kind in ("u8", "c128"):
        dem = dsp.Demodulator(_cfg())
        dem.set_parse(True)
        blocks = [raw[2 * B * b: 2 * B * (b + 1)] if kind == "u8" else cplx[B * b: B * (b + 1)] for b in range(nb)]
        rows, pk = [], []
        dem.submit(blocks[0])
        for b in range(1, nb):
            dem.submit(blocks[b])
            pk.append(dem.fetch())
            rows.append(_rows(dem.parsed()))
        pk.append(dem.fetch())
        rows.append(_rows(dem.parsed()))
        assert rows == want, kind
        assert [[(p.index, bytes(p.data).hex()) for p in c] for c in pk] == \
               [[(p["index"], p["data"]) for p in c] for c in want_calls], kind
        # rssi / snr of a message are its packet's
        dem2 = dsp.Demodulator(_cfg())
        dem2.set_parse(True)
        for b in range(nb):
            ps = dem2.demodulate(blocks[b])
            for r in dem2.parsed():
                p = {q.index: q for q in ps}[int(r["index"])]
                assert r["rssi"] == p.rssi and r["snr"] == p.snr


@pytest.mark.gpu
def test_parsed_in_the_multi_launch_form(dsp):
    """block_size 1024: the one-launch block declines (it needs 2048 .. 16384), k_stream_parse runs behind the slice.
    Expected: a second, quiet, synchronous handle with parse off - parse_packet on its packets and the reference's
    formula on its discriminated() mirror."""
    B, nb = 1024, 32
    cfg = _cfg(B)
    for seeds in ([31, 32, 33], [34]):
        raws = np.stack([synth.synth_stream(s, n_samples=nb * B) for s in seeds])
        quiet = dsp.MultiDemodulator(cfg, len(seeds))
        want, want_pk = [], []
        for b in range(nb):
            per = quiet.demodulate(raws[:, 2 * B * b: 2 * B * (b + 1)])
            want_pk.append(_pkey(per))
            rows = []
            for i, ps in enumerate(per):
                rows += _host_expected(dsp, cfg, ps, lambda i=i: quiet.discriminated(i), i, b)
            want.append(rows)
        md = dsp.MultiDemodulator(cfg, len(seeds))
        md.set_parse(True)
        got, got_pk = [], []
        md.submit(raws[:, : 2 * B])
        for b in range(1, nb):
            md.submit(raws[:, 2 * B * b: 2 * B * (b + 1)])
            got_pk.append(_pkey(md.fetch()))
            got.append(_rows(md.parsed()))
        got_pk.append(_pkey(md.fetch()))
        got.append(_rows(md.parsed()))
        strict = sum(assert_rows_match(got[b], want[b], (seeds, b)) for b in range(nb))
        assert got_pk == want_pk
        # ... and the independent oracle on the same blocks
        orc = _oracle_expected([[r[2 * B * b: 2 * B * (b + 1)] for b in range(nb)] for r in raws], B)
        assert sum(assert_rows_match(got[b], orc[b], ("oracle", seeds, b)) for b in range(nb)) >= 1
        assert strict >= 1, "the input holds no message that is compared exactly"
        assert {r[0] for rows in got for r in rows} == set(range(len(seeds)))   # every stream's burst is CRC-valid
    # a complex128 block on the multi-launch form (the complex ring's view)
    raw = synth.synth_stream(34, n_samples=nb * B)
    cplx = ((raw.astype(np.float64) - 127.4) / 127.6).view(np.complex128)
    quiet, dem = dsp.Demodulator(cfg), dsp.Demodulator(cfg)
    dem.set_parse(True)
    strict = strict_o = 0
    orc = _oracle_expected([[cplx[B * b: B * (b + 1)] for b in range(nb)]], B)
    for b in range(nb):
        ps = quiet.demodulate(cplx[B * b: B * (b + 1)])
        want = _host_expected(dsp, cfg, ps, lambda: quiet.discriminated, 0, b)
        ps2 = dem.demodulate(cplx[B * b: B * (b + 1)])
        assert _pkey([ps2]) == _pkey([ps])
        strict += assert_rows_match(_rows(dem.parsed()), want, ("c128", b))
        strict_o += assert_rows_match(_rows(dem.parsed()), orc[b], ("c128 oracle", b))
    assert strict >= 1 and strict_o >= 1


@pytest.mark.gpu
def test_parse_off_and_toggling_in_flight(dsp):
    raw = synth.synth_stream(0)
    B = 8192
    dem = dsp.Demodulator(_cfg())
    dem.demodulate(raw[: 2 * B])
    with pytest.raises(RuntimeError, match="parse off"):
        dem.parsed()
    dem.submit(raw[2 * B: 4 * B])
    with pytest.raises(RuntimeError, match="in flight"):
        dem.set_parse(True)            # refused, nothing consumed
    assert dem.inflight == 1
    dem.fetch()
    with pytest.raises(RuntimeError, match="parse off"):
        dem.parsed()
    dem.set_parse(True)
    dem.demodulate(raw[4 * B: 6 * B])
    from rtldavis_amd import batch
    assert dem.parsed().dtype == batch.RD_PARSED_DTYPE
    dem.set_parse(False)
    dem.demodulate(raw[6 * B: 8 * B])
    with pytest.raises(RuntimeError, match="parse off"):
        dem.parsed()
