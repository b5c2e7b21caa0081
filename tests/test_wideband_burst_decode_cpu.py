"""Burst decode, the part that needs no GPU: the integer model (tests/burst_decode_cases.py) on synthetic streams and on
the float64 channelizer model's bytes, the one-burst acquisition on made-up rows and closed through the model, and the
argument and state errors through the C ABI (host bookkeeping: no device is touched).  The device's records are compared
with the same model in tests/test_wideband_burst_decode.py."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import burst_cases as BC
import burst_decode_cases as DC
import retune_cases as RC
from rtldavis_amd import acquire, synth
from rtldavis_amd.wideband import BURST_FLOOR_DTYPE, BURST_MSG_DTYPE, BURST_THRESHOLD_OFF, BurstMessages, Bursts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_RATE, IF_HZ = 268800, -67200
BS = 2048
CFG = RC.packet_config(BS)


# ------------------------------------------------------------------------------------------ the model on synthetic streams
def _stream_messages(bursts, n_blocks=4, seed=7, thr=None):
    """One channel of plain synth_bursts bytes in chunks of 2048, thresholds at 4 x the floor of chunk 0 (noise):
    [(chunk, record)] of the model."""
    raw = synth.synth_bursts(bursts, n_blocks * BS, seed)
    blocks = DC.rechunk([raw[None, :]], BS)
    if thr is None:
        thr = BC.new_acquisition().thresholds(BC.burst_model(blocks[0], BURST_THRESHOLD_OFF)[1])
    return [(k, r) for k, (_, m) in enumerate(DC.decode_stream(blocks, thr, CFG)) for r in m.records]


@pytest.mark.parametrize("payload", synth.OTA_PACKETS[:3])
def test_model_recovers_the_payload_at_any_offset(payload):
    """A burst 60 kHz below to 100 kHz above the channel's centre - the demodulator reaches 4.8 kHz -: one record, the
    planted bytes, where the burst lies, with an estimate of its carrier (printed; held to the project's 1500 Hz)."""
    start = BS + 300                                         # the packet: outputs 748 .. 1868 of chunk 1
    for cfo in (-60000, -20000, 0, 38000, 100000):
        rows = _stream_messages([(bytes.fromhex(payload), start, cfo)])
        assert len(rows) == 1, (cfo, rows)
        k, r = rows[0]
        est = acquire.burst_message_offset_hz(r, OUT_RATE, IF_HZ)
        print(f"\n[decode model] {payload[:8]} at {cfo:+d} Hz: tau {int(r['tau'])}, estimate {est - cfo:+.0f} Hz off")
        assert k == 1 and bytes(r["data"]).hex() == payload and r["channel"] == 0 and r["flags"] == 0
        assert abs(int(r["tau"]) - (300 + 32 * 14 + 13)) <= 3          # the end of the first symbol, within the filter's lag
        assert r["time"] == BS + int(r["tau"]) and r["margin"] > 0
        assert r["ones"] == int(synth.packet_bits(payload).sum()) and r["id"] == synth._swap_bits8(bytes.fromhex(payload)[2]) & 7
        assert abs(est - cfo) <= BC.ESTIMATE_TOL_HZ


def test_model_reports_a_packet_across_the_boundary_once():
    payload = synth.OTA_PACKETS[3]
    rows = _stream_messages([(bytes.fromhex(payload), 2 * BS - 700, 25000)])
    assert [(k, bytes(r["data"]).hex(), int(r["flags"])) for k, r in rows] == [(2, payload, 1)]
    assert int(rows[0][1]["tau"]) < 0 and rows[0][1]["time"] == 2 * BS + int(rows[0][1]["tau"])


def test_model_wants_the_crc():
    """make_packet(..., flip_bit=k) is sync-valid and CRC-invalid: a run, no record; unflipped, the record."""
    body = bytes([0xA8, 0x11, 0x22, 0x33, 0x44, 0x55])
    good = synth.make_packet(5, body)
    rows = _stream_messages([(good, BS + 300, 30000)])
    assert [(k, bytes(r["data"]), int(r["id"])) for k, r in rows] == [(1, good, 5)]
    for k in (0, 17, 40, 63):
        assert _stream_messages([(synth.make_packet(5, body, flip_bit=k), BS + 300, 30000)]) == []


def test_model_finds_nothing_in_noise():
    raw = synth.synth_bursts([], 8 * BS, 11)
    blocks = DC.rechunk([raw[None, :]], BS)
    thr = BC.median_thresholds(raw[None, :])
    out = DC.decode_stream(blocks, thr, CFG)
    assert sum(int(b.records.size) for b, _ in out) > 8      # runs there are
    assert all(m.records.size == 0 and m.long_runs[0] == 0 for _, m in out)


def test_model_counts_long_runs_and_skips_short_ones():
    raw = synth.synth_bursts([(bytes.fromhex(synth.OTA_PACKETS[0]), 300, 30000)], 40 * 128, 3)[None, :]
    out = DC.decode_stream([raw], 0, RC.packet_config(40 * 128))       # one run of 40 windows
    assert out[0][0].records.size == 1 and out[0][1].records.size == 0 and list(out[0][1].long_runs) == [1]
    out = DC.decode_stream([raw[:, : 2 * 8 * 128]], 0, RC.packet_config(8 * 128))   # 1024 outputs: shorter than a packet
    assert out[0][0].records.size == 1 and out[0][1].records.size == 0 and list(out[0][1].long_runs) == [0]


# ------------------------------------------------------------------------------------------ the float64 channelizer model
@functools.lru_cache(maxsize=None)
def _open_loop(planted):
    lc, want = DC.acq_plan(planted)
    blocks = RC.loop_model_blocks(lc, {})
    thr = BC.new_acquisition().thresholds(BC.burst_model(blocks[0], BURST_THRESHOLD_OFF)[1])
    return lc, want, blocks, thr


@pytest.mark.parametrize("bs", [RC.LOOP_B, 2048])
@pytest.mark.parametrize("planted", BC.PLANTED)
def test_decode_on_the_channelizer_model(planted, bs):
    """Both bursts of the acquisition capture - 20 and 38 kHz off, where the demodulator hears nothing - decode to the
    planted payload, each once, with an estimate within 1500 Hz of planted + drawn cfo.  In chunks of 2048 both cross a
    boundary and are found through the look-back, with the same estimates."""
    lc, want, blocks, thr = _open_loop(planted)
    out = DC.decode_stream(DC.rechunk(blocks, bs), thr, RC.packet_config(bs))
    rows = [(k, r) for k, (_, m) in enumerate(out) for r in m.records]
    est = [acquire.burst_message_offset_hz(r, OUT_RATE, IF_HZ) for _, r in rows]
    print(f"\n[decode chan model] planted {planted} Hz, chunks of {bs}: " +
          ", ".join(f"chunk {k} tau {int(r['tau'])}: {e:.0f} Hz ({e - w:+.0f})" for (k, r), e, w in zip(rows, est, want)))
    assert [bytes(r["data"]).hex() for _, r in rows] == [lc.payload, lc.payload]
    ends = [(s + 32 * 14 + 80 * 14) // bs for _, s in lc.info]      # the chunk in which each packet ends
    assert [k for k, _ in rows] == ends
    for (k, r), e, w in zip(rows, est, want):
        assert abs(e - w) <= BC.ESTIMATE_TOL_HZ
        assert r["time"] == k * bs + int(r["tau"])
    if bs == 2048:
        assert all(int(r["flags"]) & 1 and int(r["tau"]) < 0 for _, r in rows)
        whole = DC.decode_stream(blocks, thr, RC.packet_config(RC.LOOP_B))
        same = [acquire.burst_message_offset_hz(r, OUT_RATE, IF_HZ) for _, m in whole for r in m.records]
        assert same == est                                   # the same packets' samples, whichever way they were found


# ------------------------------------------------------------------------------------------ acquisition
def _row(channel, hz, ones=40, mag=10 ** 7, n=80):
    """A message row whose packet lies `hz` off the channel centre: the mean frequency carries the imbalance."""
    ph = 2 * np.pi * (hz + IF_HZ + 4800.0 * (2 * ones - n) / n) / OUT_RATE
    return (channel, 3, 500, 0, 500, 1000, int(round(mag * np.cos(ph))), int(round(mag * np.sin(ph))), [0] * 10, ones, 1, [0] * 4)


def _msgs(k, *rows):
    return BurstMessages(np.asarray(list(rows), BURST_MSG_DTYPE).reshape(-1), np.zeros(3, np.uint32), k)


def _bursts(k, n_ch=3):
    floor = np.zeros(n_ch, BURST_FLOOR_DTYPE)
    floor["windows_off"], floor["chunk"] = 64, k
    return Bursts(np.zeros(0, BC.BURST_DTYPE), floor, k)


def _valid(*channels):
    return np.asarray([(c,) for c in channels], np.dtype([("stream", np.int32)]))


def test_burst_message_offset_hz_takes_the_imbalance_off():
    for hz in (0, 4000, -20000, 38000, 100000):
        for ones in (40, 31, 52):
            r = np.asarray([_row(0, hz, ones)], BURST_MSG_DTYPE)[0]
            assert abs(acquire.burst_message_offset_hz(r, OUT_RATE, IF_HZ) - hz) < 0.5
    r = np.asarray([_row(0, 1000, 30)], BURST_MSG_DTYPE)[0]
    assert abs(acquire.burst_message_offset_hz(r, OUT_RATE, IF_HZ, deviation_hz=0.0) - (1000 - 1200)) < 0.5
    r = np.asarray([_row(0, 1000, 30, n=40)], BURST_MSG_DTYPE)[0]
    assert abs(acquire.burst_message_offset_hz(r, OUT_RATE, IF_HZ, packet_symbols=40) - 1000) < 0.5


def test_acquisition_proposes_from_one_message_at_once():
    acq = acquire.Acquisition(3, RC.packet_config(8192))      # need = 3: the messages do not wait for it
    assert acq.update(_bursts(0), _valid(), 2, _msgs(0)) is None
    assert acq.update(_bursts(1), _valid(), 3, None) is None
    new = acq.update(_bursts(2), _valid(), 4, _msgs(2, _row(1, 20100), _row(2, 19900), _row(0, 20000)))
    assert new == 20000 and acq.offset == 20000 and acq.valid_from == 4 and not acq.locked and acq.estimates == []
    # chunks submitted under the old tuning are ignored, rows or not
    assert acq.update(_bursts(3), _valid(), 5, _msgs(3, _row(0, 20000))) is None and acq.offset == 20000
    # a plain array of rows serves as well; the proposal is relative to the plan: offset + median
    rows = np.asarray([_row(0, -150)], BURST_MSG_DTYPE)
    assert acq.update(_bursts(4), _valid(), 6, rows) == 19850 and acq.valid_from == 6
    # locked by parsed rows only, and then silent
    assert acq.update(_bursts(6), _valid(1), 8, _msgs(6, _row(0, 300))) is None and acq.locked
    assert acq.update(_bursts(7), _valid(), 9, _msgs(7, _row(0, 300))) is None
    acq.reset()
    assert acq.update(_bursts(0), _valid(), 2, _msgs(0, _row(0, 300))) == 300
    # messages of another chunk than the bursts are refused, whatever the state
    for a in (acq, acquire.Acquisition(3, RC.packet_config(8192))):
        with pytest.raises(ValueError):
            a.update(_bursts(5), _valid(), 7, _msgs(4, _row(0, 300)))


def test_closed_loop_on_the_model_with_one_burst():
    """Two chunks in flight, burst_cases.run_loop's order.  Burst A (chunk 1) is read while chunk 2 is in flight: its
    one row gives the retune that holds from chunk 3 - a chunk earlier than three bursts' median could (need = 3 would
    never get there: the capture holds two) -, and with it the dsp oracle receives burst B, CRC-valid."""
    from oracle import dsp_oracle as O
    planted = BC.PLANTED[0]
    lc, want, blocks, thr = _open_loop(planted)
    assert RC.loop_messages(blocks) == []
    cfg = RC.packet_config(RC.LOOP_B)
    ocfg = O.OracleConfig(19200, 14, 16, 80, RC.PREAMBLE, RC.LOOP_B)
    acq = acquire.Acquisition(1, cfg)                        # the default need = 3
    st = dict(blocks=blocks, rows=[[]] * RC.LOOP_NK, submitted=0, fetched=0, sched={}, msgs=None)

    def submit(k):
        st["submitted"] += 1

    def fetch():
        k = st["fetched"]
        st["fetched"] += 1
        b = BC.model_bursts(st["blocks"][k], thr, k)
        st["msgs"] = DC.decode_model(st["blocks"][k], st["blocks"][k - 1] if k else None, b, cfg, k >= 1, k * RC.LOOP_B)
        return b, st["rows"][k]

    def retune(off):
        st["sched"][st["submitted"]] = off
        st["blocks"] = RC.loop_model_blocks(lc, st["sched"])
        st["rows"] = [[r for r in call if r[2]] for call in O.parse_calls(st["blocks"], ocfg)]

    class WithMessages:
        def update(self, b, rows, submitted):
            return acq.update(b, rows, submitted, st["msgs"])

    asked = BC.run_loop(RC.LOOP_NK, submit, fetch, WithMessages(), retune)
    print(f"\n[decode loop model] planted {planted} Hz (+ cfo {want[0] - planted:.0f}): asked {asked}")
    assert asked[0][0] == 3 and abs(asked[0][1] - want[0]) <= BC.ESTIMATE_TOL_HZ
    assert all(abs(off - w) <= BC.ESTIMATE_TOL_HZ for (_, off), w in zip(asked, want))
    assert all(np.array_equal(x, y) for x, y in zip(st["blocks"][:3], blocks))
    got = [(k, r[1]) for k, call in enumerate(st["rows"]) for r in call]
    assert got and all(p == lc.payload for _, p in got) and got[0][0] in (4, 5)
    assert acq.locked


# ------------------------------------------------------------------------------------------ C ABI without a device
def _receiver(bs=2048, decim=100, n_ch=2, sl=14, cfg=None):
    from rtldavis_amd import wideband
    chans = [RC.CENTRE - 100000 + 50000 * c for c in range(n_ch)]
    return wideband.WidebandReceiver(cfg or RC.packet_config(bs, sl), chans, RC.CENTRE, decim=decim, taps=np.ones(8) / 8)


def test_set_burst_decode_states_and_shapes():
    from rtldavis_amd import _lib, dsp
    L = _lib.lib()
    w = _receiver()
    with pytest.raises(RuntimeError):
        w.set_burst_decode(True)                             # bursts are off
    assert "bursts" in _lib.last_error()
    assert L.rd_wb_set_burst_decode(w._h, 1) == _lib.RD_ERR_STATE
    assert L.rd_wb_set_burst_decode(None, 1) == _lib.RD_ERR_ARG
    w.set_burst_decode(False)                                # off is always possible
    w.set_bursts(True)
    w.set_burst_decode(True)
    w.set_burst_decode(False)
    w.set_burst_decode(True)
    w.set_bursts(False)                                      # ... and takes decode with it
    with pytest.raises(RuntimeError):
        w.set_burst_decode(True)
    # the shape: 16 sync symbols, N a multiple of 8 in 40 .. 80, N SL + 1 <= 2048, block_size >= LOOK
    P = RC.PREAMBLE
    bad = [dsp.PacketConfig(19200, 14, 8, 80, P[:8], 2048), dsp.PacketConfig(19200, 14, 16, 76, P, 2048),
           dsp.PacketConfig(19200, 14, 16, 32, P, 2048), dsp.PacketConfig(19200, 14, 16, 88, P, 2048),
           dsp.PacketConfig(19200, 26, 16, 80, P, 4096), RC.packet_config(1024), RC.packet_config(640, 8)]
    for cfg in bad:
        r = _receiver(cfg=cfg)
        r.set_bursts(True)
        with pytest.raises(ValueError):
            r.set_burst_decode(True)
        assert L.rd_wb_set_burst_decode(r._h, 1) == _lib.RD_ERR_ARG and L.rd_wb_set_burst_decode(r._h, 0) == _lib.RD_OK
    for cfg in (RC.packet_config(1152), RC.packet_config(768, 8), dsp.PacketConfig(19200, 25, 16, 80, P, 2048),
                dsp.PacketConfig(19200, 14, 16, 40, P, 640)):
        r = _receiver(cfg=cfg)
        r.set_bursts(True)
        r.set_burst_decode(True)


def test_burst_messages_before_any_fetch():
    from rtldavis_amd import _lib
    L = _lib.lib()
    w = _receiver()
    with pytest.raises(RuntimeError):
        w.burst_messages()                                   # off, nothing fetched
    w.set_bursts(True)
    w.set_burst_decode(True)
    with pytest.raises(RuntimeError):
        w.burst_messages()                                   # on, nothing fetched
    assert "no chunk fetched" in _lib.last_error()
    n = C.c_int(-1)
    recs = np.empty(4, BURST_MSG_DTYPE)
    lr = np.empty(2, np.uint32)
    assert L.rd_wb_burst_messages(w._h, recs.ctypes.data, 4, C.byref(n), lr.ctypes.data, 2) == _lib.RD_ERR_STATE
    assert L.rd_wb_burst_messages(w._h, recs.ctypes.data, 4, C.byref(n), lr.ctypes.data, 3) == _lib.RD_ERR_ARG
    assert L.rd_wb_burst_messages(w._h, None, 4, C.byref(n), None, 0) == _lib.RD_ERR_ARG
    assert L.rd_wb_burst_messages(w._h, recs.ctypes.data, -1, C.byref(n), None, 0) == _lib.RD_ERR_ARG
    assert L.rd_wb_burst_messages(w._h, recs.ctypes.data, 4, None, None, 0) == _lib.RD_ERR_ARG
    assert L.rd_wb_burst_messages(None, recs.ctypes.data, 4, C.byref(n), None, 0) == _lib.RD_ERR_ARG
    w.reset()                                                # the setting stays, no device needed
    with pytest.raises(RuntimeError):
        w.burst_messages()
    chunk = C.c_uint64(7)
    assert L.rd_wb_fetched_chunk(w._h, C.byref(chunk)) == _lib.RD_ERR_STATE and "no chunk fetched" in _lib.last_error()
    assert L.rd_wb_fetched_chunk(w._h, None) == _lib.RD_ERR_ARG and L.rd_wb_fetched_chunk(None, C.byref(chunk)) == _lib.RD_ERR_ARG
    assert chunk.value == 7


def test_symbols_layouts_and_the_ctypes_table():
    from rtldavis_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtldavis_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    protos = {
        "rd_wb_set_burst_decode": r"int\s+rd_wb_set_burst_decode\s*\(\s*rd_wideband\s*\*\s*w\s*,\s*int\s+enabled\s*\)",
        "rd_wb_burst_messages": r"int\s+rd_wb_burst_messages\s*\(\s*rd_wideband\s*\*\s*w\s*,\s*rd_burst_msg\s*\*\s*out\s*,\s*int\s+cap\s*,\s*int\s*\*\s*n\s*,\s*uint32_t\s*\*\s*long_runs\s*,\s*int\s+n_channels\s*\)",
    }
    protos["rd_wb_fetched_chunk"] = r"int\s+rd_wb_fetched_chunk\s*\(\s*rd_wideband\s*\*\s*w\s*,\s*uint64_t\s*\*\s*chunk\s*\)"
    for name, proto in protos.items():
        assert re.search(proto, src), name
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert re.search(r"#define\s+RD_BURST_MSG_BYTES\s+10\b", src) and _lib.RD_BURST_MSG_BYTES == 10
    body = re.search(r"typedef\s+struct\s+rd_burst_msg\s*\{(.*?)\}", src, flags=re.S).group(1)
    names = [re.sub(r"\[.*?\]", "", n) for decl in body.split(";")
             for n in re.sub(r"^\s*\w+\s+", "", decl.strip()).replace(" ", "").split(",") if n]
    ctype, dtype = _lib.RdBurstMsg, BURST_MSG_DTYPE
    assert names == [f for f, _ in ctype._fields_] == list(dtype.names)
    assert C.sizeof(ctype) == dtype.itemsize == 64
    assert [getattr(ctype, f).offset for f in names] == [dtype.fields[f][1] for f in names]
    assert [C.sizeof(t) for _, t in ctype._fields_] == [dtype.fields[f][0].itemsize for f in names]
    assert dtype.fields["data"][1] == 48 and dtype.fields["ones"][1] == 58 and dtype.fields["id"][1] == 59


# ------------------------------------------------------------------------------------------ crafted bytes and the seam
def test_crafted_launches_reach_their_edges():
    """burst_decode_cases builds every launch of the hook tests with its condition asserted on the model; here what spans
    launches, and the second implementation of steps 4 .. 6 (candidates(), sample by sample in Python integers) against
    decode_run on every run that gave a record."""
    launches = DC.hook_launches()
    assert len({L.name for L in launches}) == len(launches) == 11 + len(DC.GRID) and len(DC.GRID) == 13
    assert {(L.cfg.packet_symbols, L.cfg.symbol_length) for L in launches} >= set(DC.GRID)
    for L in launches:
        cap = BC.cap_of(L.cfg.block_size // 128)
        assert L.msgs.shape == (L.n_ch, cap) and L.runs.shape == (L.n_ch, cap)
        for c in range(L.n_ch):
            n = int(L.n_msgs[c])
            assert L.msgs[c, n:].tobytes() == bytes([DC.FILL]) * ((cap - n) * BURST_MSG_DTYPE.itemsize)
            assert np.all(L.msgs[c, :n]["channel"] == c) and not L.msgs[c, :n]["pad"].any()
    for L in (DC.tie_launch(), DC.range_launch(), DC.need_launch(), DC.several_launch(), DC.overflow_launch(), DC.grid_launch(40, 1)):
        for c in range(L.n_ch):
            got = []
            for r in range(min(int(L.n_runs[c]), L.runs.shape[1])):
                cand = L.candidates(c, r)
                if cand:
                    best = max(m for _, m in cand)
                    got.append((min(t for t, m in cand if m == best), best))
            assert got == [(int(r["tau"]), int(r["margin"])) for r in L.records(c)], (L.name, c)
    # the longest region, and both sides of MAX_W and of need
    L = DC.longest_launch()
    assert 128 * int(L.runs[0, 0]["windows"]) + DC.shape(L.cfg)[3] == 6144


def test_the_seam_reports_a_packet_once_with_step_7_and_twice_without():
    """A noise-free burst whose last output lies at boundary - SL .. boundary + SL: decode_model per chunk - the kernel's
    definition, steps 1 .. 6 - reports the packet in both chunks for some positions; decode_stream, with the host's
    step 7, exactly once for every position."""
    data, b0, b1 = DC.seam_rows()
    cfg = DC.config(DC.SEAM_SL, DC.SEAM_N, DC.SEAM_BS)
    first, back, _ = DC.seam_launches()
    twice = [last for c, last in enumerate(DC.SEAM_LAST) if first.n_msgs[c] and back.n_msgs[c]]
    print(f"\n[seam model] reported by both chunks without step 7 at last = {twice}: {len(twice)} of {len(DC.SEAM_LAST)} positions")
    assert len(twice) >= 1
    for c in twice:                                          # (the same packet, a few outputs apart)
        j = DC.SEAM_LAST.index(c)
        a, b = first.msgs[j, 0], back.msgs[j, 0]
        assert bytes(a["data"]) == bytes(b["data"]) == data and 0 < int(b["time"]) - int(a["time"]) < DC.SEAM_SL
    out = DC.decode_stream([b0, b1], DC.THR, cfg)
    for c, last in enumerate(DC.SEAM_LAST):
        rows = [(k, r) for k, (_, m) in enumerate(out) for r in m.records if r["channel"] == c]
        assert [bytes(r["data"]) for _, r in rows] == [data], (last, rows)
        assert rows[0][0] == (0 if first.n_msgs[c] else 1)   # the chunk that found it first keeps it
    # without flags & 1, or SL or more away, or after other data, nothing is dropped
    m = out[1][1]
    keep = DC.decode_model(b1, b0, out[1][0], cfg, True, DC.SEAM_BS)
    far = keep.records.copy()
    far["time"] += DC.SEAM_SL
    assert DC.drop_repeats(keep, far, DC.SEAM_SL).records.size == keep.records.size > m.records.size
    assert DC.drop_repeats(keep, out[0][1].records, 1).records.size == keep.records.size


def test_debug_burst_decode_refuses_what_the_check_refuses():
    """The hook's argument rule is rd_burst_decode_check's, before any device work: no GPU needed."""
    from rtldavis_amd import _lib, dsp
    L = _lib.lib()
    cur = np.full(2 * 2048, 127, np.uint8)
    runs, n_runs = np.zeros(8, BC.BURST_DTYPE), np.zeros(1, np.uint32)
    msgs, out = np.zeros(8, BURST_MSG_DTYPE), np.zeros(3, np.uint32)

    def call(cfg, stride=4096, cur_p=cur.ctypes.data):
        rc = _lib.make_config(cfg.bit_rate, cfg.symbol_length, cfg.preamble_symbols, cfg.packet_symbols, cfg.preamble, cfg.block_size)
        return L.rd_debug_burst_decode(C.byref(rc), cur_p, None, stride, 1, 0, 0, runs.ctypes.data, n_runs.ctypes.data,
                                       msgs.ctypes.data, out[0:].ctypes.data, out[1:].ctypes.data, out[2:].ctypes.data)

    P = RC.PREAMBLE
    for cfg in (dsp.PacketConfig(19200, 14, 16, 88, P, 2048), dsp.PacketConfig(19200, 26, 16, 80, P, 4096), RC.packet_config(1024),
                dsp.PacketConfig(19200, 51, 16, 64, P, 4096), dsp.PacketConfig(19200, 14, 16, 32, P, 2048)):
        assert call(cfg) == _lib.RD_ERR_ARG and "burst decode" in _lib.last_error()
    assert call(RC.packet_config(2048), stride=4096 - 16) == _lib.RD_ERR_ARG
    assert call(RC.packet_config(2048), cur_p=None) == _lib.RD_ERR_ARG
    assert not msgs.tobytes().strip(b"\0") and not out.any()


def test_hook_prototypes_and_the_ctypes_table():
    from rtldavis_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rtldavis_hip.h")).read(), flags=re.S)
    for name, n_args in (("rd_debug_bursts", 8), ("rd_debug_burst_decode", 13)):
        m = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert m and len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]) and hasattr(_lib.lib(), name)
