"""The CRC-guided repair of k_chan_burst_decode (include/rtldavis_hip.h, BURST DECODE, steps 5a, 5b, 6') without a device:
the model of tests/burst_repair_cases.py against the definition's own pieces - the syndrome table against a bitwise CRC,
single flips at every payload position, the model at max_flips = 0 against burst_decode_cases.decode_model -, the edge of
every crafted case, the argument rule of the hook, the derived bound on false accepts, and the gain on noisy bursts; and
the kernels' own candidate test (rtldavis_amd/csrc/rd_burst_candidate.h), compiled for the CPU by tests/host_harness.cpp,
against the model."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import burst_decode_cases as DC
import burst_repair_cases as RP
from rtldavis_amd import _lib, acquire, wideband
from rtldavis_amd.wideband import BURST_MSG_DTYPE


@pytest.mark.parametrize("n", [40, 64, 80])
def test_syndrome_table_equals_a_bitwise_crc_of_single_symbol_packets(n):
    """E[k], 16 <= k < N, against the CRC taken one bit at a time in the order the bit-swapped bytes [2:] give the symbols;
    and the CRC is linear: the syndrome of a random packet is the XOR of the E of its set symbols."""
    e = RP.syndrome_table(n)
    for k in range(16, n):
        one = [0] * n
        one[k] = 1
        assert int(e[k]) == RP.syndrome(one) != 0, k
    assert not e[:16].any() and len(set(int(x) for x in e[16:])) == n - 16
    rng = np.random.default_rng(n)
    for _ in range(20):
        bits = [int(b) for b in rng.integers(0, 2, n)]
        want = 0
        for k in range(16, n):
            want ^= int(e[k]) if bits[k] else 0
        assert RP.syndrome(bits) == want
        assert (want == 0) == DC._crc_ok(bytes(np.packbits(bits)))
    # the reason for a fixed order: pairs that share a syndrome exist (the generator has weight 4)
    assert RP.alias_quads(n)


@pytest.mark.parametrize("n", [40, 64, 80])
def test_repair_model_repairs_a_single_flip_at_every_payload_position(n):
    data = DC.packet(n, seed=n)
    bits = np.unpackbits(np.frombuffer(data, np.uint8)).astype(np.int64)
    rng = np.random.default_rng(100 + n)
    for k in range(16, n):
        s = (2 * bits - 1) * rng.integers(1000, 2000, n)
        s[k] = -s[k] // 100                                   # wrong, and the weakest
        assert RP.repair_model(s, 0) is None
        for r in (1, 2):
            flips, fixed, margin = RP.repair_model(s, r)
            assert flips == (k,) and bytes(np.packbits(fixed)) == data
            assert margin == min(abs(int(v)) for j, v in enumerate(s) if j != k)
        s[3] = -s[3]                                          # a wrong sync symbol: never
        assert RP.repair_model(s, 2) is None
    s = (2 * bits - 1) * rng.integers(1000, 2000, n)
    assert RP.repair_model(s, 2) == ((), [int(b) for b in bits], int(np.abs(s).min()))


def test_repair_batch_equals_repair_model():
    """The vectorised form the false-accept count uses, candidate by candidate - ties in |s| included."""
    rng = np.random.default_rng(5)
    m = 3000
    s = rng.integers(1, 40, (m, 80)) * np.where(rng.integers(0, 2, (m, 80)) == 1, 1, -1)   # small magnitudes: many ties
    s[:, :16] = np.abs(s[:, :16]) * np.where(np.asarray(RP.SYNC) == 1, 1, -1)
    s[: m // 2, 16:] = s[m // 2:, 16:]
    data = DC.packet(80, seed=1)
    good = 2 * np.unpackbits(np.frombuffer(data, np.uint8)).astype(np.int64) - 1
    for j in range(0, m // 2):                               # half of them: a packet with 0, 1 or 2 flips, somewhere
        s[j] = np.abs(s[j]) * good
        for k in rng.integers(0, 80, j % 3):
            s[j, k] = -s[j, k]
    for r in range(3):
        got = RP.repair_batch(s, r)
        want = [(-1 if x is None else len(x[0])) for x in (RP.repair_model(row, r) for row in s)]
        assert np.array_equal(got, want), r
    assert {0, 1, 2, -1} <= set(int(x) for x in RP.repair_batch(s, 2))


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def candidate():
    """hh_bd_candidate of tests/host_harness.cpp: rd_burst_candidate.h, the text both decoders compile, built for the CPU."""
    so = os.path.join(ROOT, "tests", "_build", "libhostharness.so")
    src = [os.path.join(ROOT, "tests", "host_harness.cpp")] + [os.path.join(ROOT, "rtldavis_amd", "csrc", h)
                                                               for h in ("rd_burst_candidate.h", "rd_parse.h", "rd_math.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in src):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-march=x86-64-v3", "-shared", "-fPIC", "-o", so, src[0]])
    fn = C.CDLL(so).hh_bd_candidate
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]

    def run(s, max_flips, sync=RP.SYNC, sl=1):
        """int64 [rows, 6]: pass, flips, k1, k2, margin, id; and E.  sl > 1: the rows are read with that stride."""
        s = np.ascontiguousarray(s, np.int64)
        rows, n = s.shape
        wide = np.full((rows, n, sl), 1 - 2 ** 62, np.int64)   # what lies between the symbols must not be read
        wide[:, :, 0] = s
        e, out = np.full(n, 0xFFFF, np.uint16), np.full((rows, 6), -7, np.int64)
        word = int("".join(str(int(b)) for b in sync), 2)
        fn(wide.ctypes.data, rows, sl, n, word, max_flips, e.ctypes.data, out.ctypes.data)
        return out, e
    return run


def _model_rows(s, max_flips, sync=RP.SYNC):
    """RP.repair_model for every row in the form of hh_bd_candidate; rows whose first 16 symbols are not the sync word are
    None by the model's first test and are not handed to it."""
    s = np.asarray(s, np.int64)
    want = np.zeros((s.shape[0], 6), np.int64)
    want[:, 2:4] = -1
    for j in np.flatnonzero(np.all((s[:, :16] > 0) == np.asarray(sync, bool)[None, :], axis=1)):
        r = RP.repair_model(s[j], max_flips, tuple(sync))
        if r is not None:
            ks, bits, margin = r
            ident = bits[16] | bits[17] << 1 | bits[18] << 2     # rd_swap_bits8(byte 2) & 7
            want[j] = (1, len(ks), ks[0] if ks else -1, ks[1] if len(ks) == 2 else -1, margin, ident)
    return want


def test_candidate_function_of_the_kernels_equals_repair_model(candidate):
    """rd_bd_candidate, compiled for the CPU, on the symbol sums of every candidate tau of every run of the crafted repair
    launches (the grid at N = 40, 64, 80 among them) and on seeded random rows with the sync word forced and many |s|
    ties, at max_flips 0, 1, 2: (pass, flips, k1, k2, margin, id) are the model's; E is the model's table."""
    for n in (40, 64, 80):
        e = candidate(np.ones((1, n), np.int64), 2)[1]
        assert np.array_equal(e, RP.syndrome_table(n)), n
    seen = {0: 0, 1: 0, 2: 0}
    launches = RP.crafted_launches()
    assert {(40, 1), (40, 14), (80, 1), (80, 14)} <= set(RP.GRID) and all(RP.grid_launch(n, sl) in launches for n, sl in RP.GRID)
    for L in launches:
        n_win = L.cur.shape[1] // (2 * RP.W)
        sync = DC.shape(L.cfg)[2]
        for c in range(L.n_ch):
            for run in range(min(int(L.n_runs[c]), L.runs.shape[1])):
                first, windows = int(L.runs[c, run]["first"]), int(L.runs[c, run]["windows"])
                if windows > RP.MAX_W or windows == 0 or first >= n_win or first + windows > n_win:
                    continue
                got = L.sums(c, run)
                if got is None:
                    continue
                s = got[1]
                for r in (0, 1, 2):
                    out = candidate(s, r, sync, sl=1 if r else 3)[0]
                    assert np.array_equal(out, _model_rows(s, r, sync)), (L.name, c, run, r)
                    for k in seen:
                        seen[k] += int(((out[:, 0] == 1) & (out[:, 1] == k)).sum()) if r == 2 else 0
    assert min(seen.values()) > 0, seen
    rng = np.random.default_rng(23)
    for n in (40, 80):
        m = 3000
        s = rng.integers(1, 12, (m, n)) * np.where(rng.integers(0, 2, (m, n)) == 1, 1, -1)   # small magnitudes: ties everywhere
        s[:, :16] = np.abs(s[:, :16]) * np.where(np.asarray(RP.SYNC) == 1, 1, -1)
        good = 2 * np.unpackbits(np.frombuffer(DC.packet(n, seed=n + 1), np.uint8)).astype(np.int64) - 1
        for j in range(m // 2):                              # half of them: a packet with 0 .. 3 flips, the id symbols among them
            s[j] = np.abs(s[j]) * good
            for k in rng.integers(16, 16 + (4 if j % 2 else n - 16), j % 4):
                s[j, k] = -s[j, k]
        s[m // 2: m // 2 + 50, 5] *= -1                      # a wrong sync symbol
        s[-50:] *= 2 ** 40                                   # 64-bit magnitudes
        for r in (0, 1, 2):
            out = candidate(s, r)[0]
            assert np.array_equal(out, _model_rows(s, r)), (n, r)
        assert {0, 1, 2} <= set(int(x) for x in out[out[:, 0] == 1, 1]) and (out[:, 0] == 0).sum() > 50


def test_model_without_repair_is_the_decode_model():
    """max_flips = 0 on every launch of the crafted decode cases: the slot burst_decode_cases' own model gives, byte for
    byte (Launch asserts it); at max_flips = 2 every record of the off model is there unchanged - an exact candidate
    always wins -, pad 0, bit 1 clear."""
    n_recs = 0
    for L0 in DC.hook_launches():
        for r in range(3):
            msgs, n_msgs, long_runs, chunk = RP.slot_model(L0, r)
            if r == 0:
                assert msgs.tobytes() == L0.msgs.tobytes(), L0.name
                assert np.array_equal(n_msgs, L0.n_msgs) and np.array_equal(long_runs, L0.long_runs) and np.array_equal(chunk, L0.chunk)
                continue
            for c in range(L0.n_ch):
                mine = msgs[c, : int(n_msgs[c])]
                exact = [m for m in mine if not int(m["flags"]) & 2]
                assert [m.tobytes() for m in exact] == [rec.tobytes() for rec in L0.records(c)], (L0.name, r, c)
                assert not any(m["pad"].any() for m in exact)
                n_recs += len(exact)
    assert n_recs > 40


CASES = ("one_flip_launch", "two_flips_launch", "rank_edge_launch", "strong_wrong_launch", "alias_pair_launch", "rank_tie_launch",
         "winner_launch", "seam_launches", "longest_launch", "saturated_launch")


@pytest.mark.parametrize("name", CASES)
def test_every_crafted_case_reaches_its_edge(name):
    getattr(RP, name)()


@pytest.mark.parametrize("n,sl", RP.GRID)
def test_grid_cases_reach_their_edge(n, sl):
    RP.grid_launch(n, sl)


def test_seam_is_reported_once_by_the_stream_model():
    for r, want in ((0, 0), (1, 1), (2, 1)):
        msgs, data = RP.seam_stream(r)
        rows = [rec for m in msgs for rec in m.records]
        assert len(rows) == want
        if want:
            assert msgs[0].records.size == 0 and int(rows[0]["flags"]) == 3 and bytes(rows[0]["data"]) == data


def test_prototypes_and_the_argument_rule_of_the_hook():
    """max_flips = -1 and 3: RD_ERR_ARG before any device work (no device is needed to get it), nothing written."""
    for name in ("rd_wb_set_burst_repair", "rd_wb_burst_repair", "rd_debug_burst_decode_repair"):
        assert name in _lib.SIGNATURES and getattr(_lib.lib(), name)
    assert len(_lib.SIGNATURES["rd_debug_burst_decode_repair"][1]) == len(_lib.SIGNATURES["rd_debug_burst_decode"][1]) + 1
    assert wideband.BURST_MSG_REPAIRED == RP.REPAIRED == acquire.MSG_REPAIRED == 2 and wideband.BURST_REPAIR_LIST == RP.LIST
    assert BURST_MSG_DTYPE.itemsize == 64 and BURST_MSG_DTYPE.fields["pad"][1] == 60
    L = RP.one_flip_launch()
    cfg = _lib.make_config(L.cfg.bit_rate, L.cfg.symbol_length, L.cfg.preamble_symbols, L.cfg.packet_symbols, L.cfg.preamble,
                           L.cfg.block_size)
    msgs = np.zeros(L.msgs.shape, BURST_MSG_DTYPE)
    n_msgs, long_runs, chunk = (np.zeros(L.n_ch, np.uint32) for _ in range(3))
    for bad in (-1, 3):
        rc = _lib.lib().rd_debug_burst_decode_repair(C.byref(cfg), L.cur.ctypes.data, None, L.cur.shape[1], L.n_ch, L.clock, L.seq,
                                                     L.runs.ctypes.data, L.n_runs.ctypes.data, bad, msgs.ctypes.data,
                                                     n_msgs.ctypes.data, long_runs.ctypes.data, chunk.ctypes.data)
        assert rc == _lib.RD_ERR_ARG and "max_flips" in _lib.last_error()
    assert not msgs.tobytes().strip(b"\0") and not n_msgs.any()


def test_acquire_helpers_on_model_rows():
    L = RP.two_flips_launch()
    rows = np.concatenate([L.recs(2, 0), RP.one_flip_launch().recs(1, 1), DC.grid_launch(80, 14).records(0)])
    assert list(acquire.repaired(rows)) == [True, True, False]
    assert [acquire.flipped_symbols(r) for r in rows] == [(16, 79), (79,), ()]
    assert acquire.repaired(wideband.BurstMessages(rows, np.zeros(1, np.uint32), 0)).sum() == 2


def test_false_accepts_stay_under_the_derived_bound():
    """2^20 random candidates of 80 symbols - random signs and magnitudes in the payload, the sync word right - through
    the model at R = 2.  A random syndrome equals one of at most 36 subset syndromes with probability at most 36 / 65535,
    so at most 2^20 x 36 / 65536 = 576 are expected to be accepted with a non-empty flip set; six standard deviations
    (sqrt(576) = 24) on top: 720.  At least 400 shows that the repair acts (36 distinct syndromes are the rule: pairs
    that alias are rare).  Measured with this seed: 583 (110 with one flip, 473 with two; 15 exact)."""
    rng = np.random.default_rng(1)
    count = {-1: 0, 0: 0, 1: 0, 2: 0}
    for _ in range(16):
        m = 2 ** 16
        s = rng.integers(1, 2 ** 40, (m, 80)) * np.where(rng.integers(0, 2, (m, 80)) == 1, 1, -1)
        s[:, :16] = np.abs(s[:, :16]) * np.where(np.asarray(RP.SYNC) == 1, 1, -1)
        r = RP.repair_batch(s, 2)
        for k in count:
            count[k] += int((r == k).sum())
    print(f"\n[false accepts of 2^20 at R = 2] {count}")
    assert sum(count.values()) == 2 ** 20
    assert 400 <= count[1] + count[2] <= 720, count
    assert count[1] <= 2 ** 20 * 8 / 65536 + 6 * np.sqrt(2 ** 20 * 8 / 65536), count     # R = 1's share: 128 + 68


GAIN_K, GAIN_NOISE, GAIN_SEED = 24, 0.09, 7


def test_repair_gains_bursts_and_invents_none():
    """24 bursts of synth.synth_bursts at one noise level, chosen on the model so that R = 0 decodes some but not all
    (14 of 24 with this seed; 19 at R = 1, 22 at R = 2).  R = 0 misses at least one; R = 2 recovers at least one of those
    with the planted payload; no record at any R carries a payload that was not planted; every record without bit 1
    equals R = 0's."""
    datas, out = RP.gain_run(GAIN_K, GAIN_NOISE, GAIN_SEED)
    got = {r: [bytes(x["data"]) for x in v] for r, v in out.items()}
    print(f"\n[gain, noise {GAIN_NOISE}] decoded of {GAIN_K}: " + ", ".join(f"R={r}: {len(set(got[r]))}" for r in got))
    assert 0 < len(got[0]) and set(got[0]) < set(datas)
    assert set(got[2]) - set(got[0]) and set(got[0]) <= set(got[1]) <= set(got[2])
    for r in (0, 1, 2):
        assert all(d in datas for d in got[r]) and len(set(got[r])) == len(got[r]), r
        exact = [x.tobytes() for x in out[r] if not int(x["flags"]) & RP.REPAIRED]
        assert exact == [x.tobytes() for x in out[0]], r
        for x in out[r]:
            flips = acquire.flipped_symbols(x)
            assert len(flips) <= r and all(16 <= k < 80 for k in flips) and (len(flips) > 0) == bool(int(x["flags"]) & RP.REPAIRED)


def test_python_argument_rules_need_no_device():
    """set_burst_repair refuses bools and values outside 0 .. 2 before it calls into the library."""
    rx = wideband.WidebandReceiver.__new__(wideband.WidebandReceiver)
    for bad in (True, False, -1, 3, 1.0, "1", None):
        with pytest.raises(ValueError):
            wideband.WidebandReceiver.set_burst_repair(rx, bad)


def test_state_rules_without_a_device():
    """The C rule on a receiver that never touches a device: RD_ERR_ARG outside 0 .. 2, RD_ERR_STATE unless decode is on,
    decode or bursts off put it back to 0, reset() keeps it."""
    import retune_cases as RC
    L = _lib.lib()
    w = wideband.WidebandReceiver(RC.packet_config(2048), [RC.CENTRE - 100000, RC.CENTRE + 50000], RC.CENTRE, decim=100, taps=np.ones(8) / 8)
    r = C.c_int(-7)
    assert L.rd_wb_burst_repair(w._h, C.byref(r)) == _lib.RD_OK and r.value == 0 == w.burst_repair()
    assert L.rd_wb_burst_repair(w._h, None) == _lib.RD_ERR_ARG and L.rd_wb_set_burst_repair(None, 1) == _lib.RD_ERR_ARG
    assert L.rd_wb_set_burst_repair(w._h, 3) == _lib.RD_ERR_ARG and L.rd_wb_set_burst_repair(w._h, -1) == _lib.RD_ERR_ARG
    for v in (0, 1, 2):
        assert L.rd_wb_set_burst_repair(w._h, v) == _lib.RD_ERR_STATE       # decode is off (0 included: the rule is the state's)
    w.set_bursts(True)
    with pytest.raises(RuntimeError):
        w.set_burst_repair(1)
    w.set_burst_decode(True)
    for v in (1, 2, 0, 2):
        w.set_burst_repair(v)
        assert w.burst_repair() == v
    w.reset()
    assert w.burst_repair() == 2
    w.set_burst_decode(False)
    assert w.burst_repair() == 0
    w.set_burst_decode(True)
    w.set_burst_repair(1)
    w.set_bursts(False)
    assert w.burst_repair() == 0
    with pytest.raises(RuntimeError):
        w.set_burst_repair(1)


def test_acquisition_ignores_repaired_rows_unless_asked():
    import retune_cases as RC
    from rtldavis_amd.wideband import BURST_FLOOR_DTYPE, Bursts
    import burst_cases as BC
    cfg = RC.packet_config(2048)
    floor = np.zeros(3, BURST_FLOOR_DTYPE)
    floor["windows_off"], floor["chunk"] = 16, 4
    b = Bursts(np.zeros(0, BC.BURST_DTYPE), floor, 4)
    rep = RP.one_flip_launch().recs(1, 0)[:1].copy()
    exact = DC.grid_launch(80, 14).records(0)[:1].copy()
    both = np.concatenate([rep, exact])
    msgs = lambda rows: wideband.BurstMessages(rows, np.zeros(3, np.uint32), 4)
    assert acquire.Acquisition(3, cfg).update(b, [], 5, msgs(rep)) is None
    a = acquire.Acquisition(3, cfg, use_repaired=True)
    assert isinstance(a.update(b, [], 5, msgs(rep)), int) and a.valid_from == 5
    # a repaired row beside an exact one: only the exact one counts by default
    assert acquire.Acquisition(3, cfg).update(b, [], 5, msgs(both)) == acquire.Acquisition(3, cfg).update(b, [], 5, msgs(exact))
    assert acquire.Acquisition(3, cfg, use_repaired=True).update(b, [], 5, msgs(both)) != acquire.Acquisition(3, cfg).update(b, [], 5, msgs(exact))
