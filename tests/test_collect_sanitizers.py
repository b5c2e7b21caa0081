"""The receiver's fetch (rtldavis_amd/csrc/rd_host.cpp: rd_collect_*, rd_delivered, rd_msg_repeats) in a stand-alone
program, tests/collect_asan.cpp, built with -fsanitize=address,undefined and run here on the CPU.  These functions are all
that stands between a slot the device wrote and the copies that trust its counts, and no GPU test may provoke their
refusals.  Every slot is handed over in a heap block of exactly its size: well-formed slots of the integer models, held
against what this file derives from the same slot; every refusal, with the fault at the first and at the last channel or
entry, by its message; the delivered history across fetched, skipped, forgotten and failed chunks; and the one repeat
rule against the three loops it replaced.  The library compiles the same rd_host.cpp (csrc/Makefile)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import burst_cases as BC
import burst_clip_cases as CC
import burst_decode_cases as DC
import burst_sweep_cases as SW
from rtldavis_amd.wideband import (BURST_DTYPE, BURST_FLOOR_DTYPE, BURST_MSG_DTYPE, CLIP_DTYPE, QUALITY_DTYPE, SEARCH_HDR_DTYPE,
                                   BurstMessages)

BUILD = os.path.join(ROOT, "tests", "_build")
EXE = os.path.join(BUILD, "collect_asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
CSRC = os.path.join(ROOT, "rtldavis_amd", "csrc")

OK, ERR_DEVICE = 0, -2                                   # RD_OK, RD_ERR_DEVICE
LEVELS, SPECTRUM, BURSTS, DECODE, EXPECT, SEARCH, CLIPS, FORGET = range(8)
FILL, W = 0xA5, 128
BX_MAX, BS_MAX, BS_PER, BC_PER, NO_ENTRY = 64, 8, 4, 16, 0xFFFFFFFF
LEVEL = np.dtype([("power", np.uint64), ("peak", np.uint32), ("clipped", np.uint32), ("gain", np.float32), ("chunk", np.uint32)])
INPUT = np.dtype([("power", np.uint64), ("chunk", np.uint64), ("peak", np.uint32), ("clipped", np.uint32)])
SPEC = np.dtype([("chunk", np.uint64), ("segments", np.uint32), ("n_bins", np.uint32)])
BD_HDR = np.dtype([("n_msgs", np.uint32), ("long_runs", np.uint32), ("chunk", np.uint32), ("pad", np.uint32)])
BX_HDR, BC_HDR, BS_HDR, MSG, Q = CC.X_HDR_DTYPE, CC.HDR_DTYPE, SEARCH_HDR_DTYPE, BURST_MSG_DTYPE, QUALITY_DTYPE
BX_ENTRY_BYTES = 32
assert (MSG.itemsize, Q.itemsize, BURST_DTYPE.itemsize, BURST_FLOOR_DTYPE.itemsize, CLIP_DTYPE.itemsize) == (64, 64, 48, 40, 48)
SHAPES = [(n_ch, n_win) for n_ch in (1, 3, 70) for n_win in (1, 4)]      # block sizes 128 and 512
K = 5                                                                    # the chunk the crafted slots belong to


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "collect_asan.cpp"), os.path.join(CSRC, "rd_host.cpp")]
    deps = srcs + [os.path.join(CSRC, "rd_host.h"), os.path.join(CSRC, "rd_slots.h"), os.path.join(ROOT, "include", "rtldavis_hip.h")]
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-Wall", "-Wextra", "-o", EXE] + srcs)
    return EXE


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{args}: rc {r.returncode}\n{r.stdout}\n{r.stderr[-3000:]}"
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout


# ------------------------------------------------------------------------------------------ the program's file protocol
def op(kind, n_ch=0, a=0, chunk=0, sl=14, n=0, slot=None, q=None, cand=None):
    blobs = [None if b is None else np.ascontiguousarray(b).tobytes() for b in (slot, q)]
    cand = None if cand is None else np.ascontiguousarray(cand, np.uint32).tobytes()
    head = struct.pack("<10q", kind, n_ch, a, chunk, sl, n, *(-1 if b is None else len(b) for b in blobs),
                       -1 if cand is None else len(cand) // 4, 0)
    return head + b"".join(b for b in blobs + [cand] if b is not None)


def collect(exe, tmp_path, ops):
    """[(rc, history chunk, message, [array bytes])] of the operations, run in order by one process."""
    src, dst = tmp_path / "ops.bin", tmp_path / "results.bin"
    src.write_bytes(b"".join(ops))
    assert f"run ok: {len(ops)} operations" in run(exe, "run", src, dst)
    raw, at, out = dst.read_bytes(), 0, []
    for _ in ops:
        rc, hist, n_msg, n_arr = struct.unpack_from("<4q", raw, at)
        at += 32
        msg = raw[at: at + n_msg].decode()
        at += n_msg
        arrays = []
        for _ in range(n_arr):
            nb, = struct.unpack_from("<q", raw, at)
            arrays.append(raw[at + 8: at + 8 + nb])
            at += 8 + nb
        out.append((rc, hist, msg, arrays))
    assert at == len(raw)
    return out


def as_rows(b, dtype):
    return np.frombuffer(b, dtype)


# ------------------------------------------------------------------------------------------ slots, as rd_slots.h lays them out
def cap_of(n_win):
    return (n_win + 1) // 2


class Slot:
    """A slot image and named views of its parts; everything nothing wrote is FILL."""

    def __init__(self, parts):
        at, self.at = 0, {}
        for name, dtype, shape, align in parts:
            at = (at + align - 1) // align * align
            self.at[name] = (at, np.dtype(dtype), shape)
            at += np.dtype(dtype).itemsize * int(np.prod(shape))
        self.buf = np.full(at, FILL, np.uint8)

    def __getitem__(self, name):
        at, dtype, shape = self.at[name]
        return self.buf[at: at + dtype.itemsize * int(np.prod(shape))].view(dtype).reshape(shape)

    def copy(self):
        other = Slot([])
        other.at, other.buf = self.at, self.buf.copy()
        return other


def noise(rng, dtype, shape):
    return rng.integers(0, 256, int(np.prod(shape)) * np.dtype(dtype).itemsize, dtype=np.uint8).view(dtype).reshape(shape)


def bursts_slot(n_ch, n_win):
    return Slot([("recs", BURST_DTYPE, (n_ch, cap_of(n_win)), 1), ("floor", BURST_FLOOR_DTYPE, (n_ch,), 1), ("thr", np.uint32, (n_ch,), 1)])


def decode_slot(n_ch, n_win):
    return Slot([("recs", MSG, (n_ch, cap_of(n_win)), 1), ("hdr", BD_HDR, (n_ch,), 1)])


def quality_slot(n_ch, n_win):
    return Slot([("rows", Q, (n_ch, cap_of(n_win)), 1), ("xrows", Q, (BX_MAX,), 1)])


def expect_slot():
    return Slot([("recs", MSG, (BX_MAX,), 1), ("hdr", BX_HDR, (BX_MAX,), 1), ("entries", np.uint8, (BX_MAX * BX_ENTRY_BYTES,), 1)])


def search_slot(n_ch):
    return Slot([("recs", MSG, (BS_MAX, n_ch, BS_PER), 1), ("hdr", BS_HDR, (BS_MAX, n_ch), 1)])


def clips_slot(n_ch, quota):
    s = Slot([("recs", CLIP_DTYPE, (n_ch, BC_PER), 1), ("hdr", BC_HDR, (n_ch,), 1), ("pool", np.uint8, (n_ch, 2 * quota), 16)])
    assert s.buf.size == CC.slot_bytes(n_ch, quota)
    return s


# what a collection must hand back, derived from the slot itself
def repeats(m, delivered, sl, look_back, same_centre):
    if look_back and not int(m["flags"]) & 1:
        return False
    for q in delivered:
        d = (int(m["time"]) - int(q["time"])) % 2 ** 64
        if (q["channel"] == m["channel"] and bytes(q["data"]) == bytes(m["data"]) and min(d, 2 ** 64 - d) < sl
                and (not same_centre or q["pad"][3] == m["pad"][3])):
            return True
    return False


def want_bursts(s):
    n = s["floor"]["n_bursts"]
    return np.concatenate([s["recs"][c, : int(n[c])] for c in range(n.size)]).tobytes(), s["floor"].tobytes()


def want_decode(s, qs, delivered=(), sl=14):
    """(messages, long_runs, quality rows): the first n_msgs records of each channel in channel order, less step 7's
    repeats (burst_decode_cases.drop_repeats), each kept message's quality row beside it."""
    n = s["hdr"]["n_msgs"]
    where = np.asarray([(c, i) for c in range(n.size) for i in range(int(n[c]))], np.int64).reshape(-1, 2)
    rows = s["recs"][where[:, 0], where[:, 1]]
    kept = DC.drop_repeats(BurstMessages(rows, s["hdr"]["long_runs"], 0), list(delivered), sl).records
    keep = np.asarray([j for j, r in enumerate(rows) if not repeats(r, delivered, sl, True, False)], np.int64)
    assert kept.tobytes() == rows[keep].tobytes()            # (this file's rule and the model's agree)
    qual = b"" if qs is None else qs["rows"][where[keep, 0], where[keep, 1]].tobytes()
    return kept.tobytes(), s["hdr"]["long_runs"].astype(np.uint32).tobytes(), qual


def want_expect(s, qs, n, delivered=(), sl=14):
    counts = np.full(BX_MAX, NO_ENTRY, np.uint32)
    counts[:n] = 0
    keep = []
    if s is not None:
        counts[:n] = s["hdr"]["candidates"][:n]
        keep = [i for i in range(n) if s["hdr"]["n_msgs"][i] == 1 and not repeats(s["recs"][i], delivered, sl, False, False)]
    msgs = b"" if s is None else s["recs"][keep].tobytes()
    return msgs, counts.tobytes(), b"" if qs is None or s is None else qs["xrows"][keep].tobytes()


def want_search(s, n, delivered=(), sl=14):
    if not n:
        return b"", b""
    where = [(i, c, r) for i in range(n) for c in range(s["hdr"].shape[1]) for r in range(int(s["hdr"][i, c]["n_msgs"]))]
    kept = [s["recs"][p].tobytes() for p in where if not repeats(s["recs"][p], delivered, sl, False, True)]
    return b"".join(kept), s["hdr"][:n].tobytes()


def want_clips(s):
    """The clip bytes packed channel after channel with `offset` rewritten, and the drop counts."""
    recs, data, base = [], [], 0
    for c, h in enumerate(s["hdr"]):
        r = s["recs"][c, : int(h["n_clips"])].copy()
        r["offset"] += base
        recs.append(r)
        data.append(s["pool"][c, : 2 * int(h["used"])])
        base += int(h["used"])
    return np.concatenate(recs).tobytes(), np.concatenate(data).tobytes(), s["hdr"]["dropped"].astype(np.uint32).tobytes()


# crafted slots: random records under headers of chunk K
def crafted_bursts(rng, n_ch, n_win):
    s = bursts_slot(n_ch, n_win)
    s["recs"][:] = noise(rng, BURST_DTYPE, s["recs"].shape)
    s["floor"][:] = noise(rng, BURST_FLOOR_DTYPE, (n_ch,))
    s["floor"]["chunk"] = K
    s["floor"]["n_bursts"] = rng.integers(0, cap_of(n_win) + 1, n_ch)
    s["floor"]["n_bursts"][[0, -1]] = cap_of(n_win)
    return s


def crafted_decode(rng, n_ch, n_win, chunk=K):
    s, qs = decode_slot(n_ch, n_win), quality_slot(n_ch, n_win)
    s["recs"][:] = noise(rng, MSG, s["recs"].shape)
    s["hdr"]["n_msgs"] = rng.integers(0, cap_of(n_win) + 1, n_ch)
    s["hdr"]["n_msgs"][[0, -1]] = cap_of(n_win)
    s["hdr"]["long_runs"] = rng.integers(0, 2 ** 32, n_ch)
    s["hdr"]["chunk"], s["hdr"]["pad"] = chunk, 0
    qs["rows"][:], qs["xrows"][:] = noise(rng, Q, qs["rows"].shape), noise(rng, Q, (BX_MAX,))
    qs["rows"]["chunk"], qs["xrows"]["chunk"] = chunk, chunk
    return s, qs


def crafted_expect(rng, n, chunk=K):
    s = expect_slot()
    s["recs"][:n] = noise(rng, MSG, (n,))
    s["hdr"][:n] = noise(rng, BX_HDR, (n,))
    s["hdr"]["n_msgs"][:n] = rng.integers(0, 2, n)
    if n:
        s["hdr"]["n_msgs"][[0, n - 1]] = 1
    s["hdr"]["chunk"][:n] = chunk
    return s, s["hdr"]["candidates"][:n].copy()


def crafted_search(rng, n_ch, n, chunk=K):
    s = search_slot(n_ch)
    s["recs"][:n] = noise(rng, MSG, (n, n_ch, BS_PER))
    s["hdr"][:n] = noise(rng, BS_HDR, (n, n_ch))
    s["hdr"]["n_msgs"][:n] = rng.integers(0, BS_PER + 1, (n, n_ch))
    if n:
        s["hdr"]["n_msgs"][0, 0] = s["hdr"]["n_msgs"][n - 1, -1] = BS_PER
    s["hdr"]["chunk"][:n] = chunk
    return s


def crafted_clips(rng, n_ch, quota):
    s = clips_slot(n_ch, quota)
    s["pool"][:] = noise(rng, np.uint8, s["pool"].shape)
    s["recs"][:] = noise(rng, CLIP_DTYPE, s["recs"].shape)
    s["hdr"][:] = noise(rng, BC_HDR, (n_ch,))
    s["hdr"]["chunk"] = K
    s["hdr"]["n_clips"] = rng.integers(0, BC_PER + 1, n_ch)
    s["hdr"]["n_clips"][[0, -1]] = BC_PER
    s["hdr"]["used"] = rng.integers(0, quota + 1, n_ch)
    s["hdr"]["used"][[0, -1]] = quota
    for c in range(n_ch):
        used = int(s["hdr"]["used"][c])
        s["recs"]["offset"][c] = rng.integers(0, used + 1, BC_PER)
        s["recs"]["n"][c] = used - s["recs"]["offset"][c]        # (every clip ends with the pool's used part: the limit itself)
    return s


def crafted_levels(rng, n_ch):
    s = Slot([("lv", LEVEL, (n_ch,), 1), ("in", INPUT, (1,), 1)])
    s["lv"][:], s["in"][:] = noise(rng, LEVEL, (n_ch,)), noise(rng, INPUT, (1,))
    s["lv"]["chunk"], s["in"]["chunk"] = K, K
    return s


def crafted_spectrum(rng, n_bins):
    s = Slot([("info", SPEC, (1,), 1), ("power", np.float64, (n_bins,), 1)])
    s["info"][0] = (K, 3, n_bins)
    s["power"][:] = rng.random(n_bins)
    return s


# ------------------------------------------------------------------------------------------ 1. well-formed slots
def _ok(results, wants):
    assert len(results) == len(wants)
    for j, ((rc, _, msg, arrays), want) in enumerate(zip(results, wants)):
        assert rc == OK and msg == "", (j, rc, msg)
        assert len(arrays) == len(want), j
        for i, (a, b) in enumerate(zip(arrays, want)):
            assert a == b, f"operation {j}, array {i}: {len(a)} bytes against {len(b)}"


def test_model_slots_are_collected_as_the_slot_itself_says(exe, tmp_path):
    rng = np.random.default_rng(1)
    ops, wants = [], []
    # k_chan_bursts' model: uniform bytes under median thresholds, at every small shape
    for n_ch, n_win in SHAPES:
        rows = [rng.integers(0, 256, 2 * W * n_win).astype(np.uint8) for _ in range(n_ch)]
        cs = BC.crafted(f"collect_{n_ch}_{n_win}", rows, BC.median_thresholds(np.stack(rows)), seq=K)
        recs, floor = BC.slot_model(cs)
        s = bursts_slot(n_ch, n_win)
        s["recs"][:], s["floor"][:], s["thr"][:] = recs, floor, cs.thr
        assert cs.records.size == floor["n_bursts"].sum()
        ops.append(op(BURSTS, n_ch, n_win, K, slot=s.buf))
        wants.append(want_bursts(s))
        assert wants[-1][0] == cs.records.tobytes()          # (the model's own list: channel order, a channel's runs ascending)
    assert sum(len(w[0]) for w in wants) > 0
    # k_chan_burst_decode's model (slot_decode_model), with and without a quality slot beside it
    n_msgs = 0
    for L in (DC.several_launch(), DC.handwritten_launch(), DC.overflow_launch(), DC.tie_launch()):
        n_win = L.cfg.block_size // W
        s, qs = decode_slot(L.n_ch, n_win), quality_slot(L.n_ch, n_win)
        s["recs"][:] = L.msgs
        s["hdr"]["n_msgs"], s["hdr"]["long_runs"], s["hdr"]["chunk"], s["hdr"]["pad"] = L.n_msgs, L.long_runs, L.chunk, 0
        qs["rows"][:] = noise(rng, Q, qs["rows"].shape)
        qs["rows"]["chunk"] = L.chunk[:, None]
        for q in (None, qs):
            ops.append(op(DECODE, L.n_ch, n_win, L.seq, L.cfg.symbol_length, slot=s.buf, q=None if q is None else q.buf))
            ops.append(op(FORGET))
            wants += [want_decode(s, q), ()]
        assert wants[-2][0] == b"".join(L.records(c).tobytes() for c in range(L.n_ch))
        n_msgs += int(L.n_msgs.sum())
    assert n_msgs >= 4
    # k_chan_burst_clips' model: the slot image, through split_slot
    n_clips = 0
    for L in tuple(CC.channels_launch(n) for n in (1, 3, 70)) + (CC.quota_launch(), CC.per_launch(), CC.residue_launch()):
        recs, hdr, pool = CC.split_slot(L.want, L.n_ch, L.quota)
        s = clips_slot(L.n_ch, L.quota)
        s.buf[:] = L.want
        assert s["hdr"].tobytes() == hdr.tobytes() and s["pool"].tobytes() == pool.tobytes() and s["recs"].tobytes() == recs.tobytes()
        ops.append(op(CLIPS, L.n_ch, L.quota, L.seq, slot=s.buf))
        wants.append(want_clips(s))
        packed = CC.packed(L.model)
        assert wants[-1] == tuple(p.tobytes() for p in packed)
        n_clips += packed[0].size
    assert n_clips >= 10
    # the expect and search slots of the seeded chains
    launched = found = searched = 0
    for seed in (0, 2, 3, 8, 13, 22, 41):
        ch = SW.cached_chain(seed)
        sc = ch.scene
        msgs, hdr = ch.expect.want(*sc.feed_form)
        n = int(sc.table.size)
        s = None
        if hdr.tobytes() != bytes([FILL]) * hdr.nbytes:      # (else: no expectation has a candidate, nothing was launched)
            s = expect_slot()
            s["recs"][:], s["hdr"][:] = msgs, hdr
            launched += 1
        ops += [op(EXPECT, sc.n_ch, sc.n_win, sc.seq, sc.sl, n, slot=None if s is None else s.buf,
                   cand=np.zeros(n, np.uint32) if s is None else s["hdr"]["candidates"][:n]), op(FORGET)]
        wants += [want_expect(s, None, n), ()]
        found += len(wants[-2][0]) // MSG.itemsize
        if ch.search is not None:
            s = search_slot(sc.n_ch)
            s["recs"][:], s["hdr"][:] = ch.search.want()
            ops += [op(SEARCH, sc.n_ch, 0, sc.seq, sc.sl, len(sc.centres), slot=s.buf), op(FORGET)]
            wants += [want_search(s, len(sc.centres)), ()]
            assert wants[-2][1] == ch.search.want()[1][: len(sc.centres)].tobytes()       # the search headers
            searched += len(wants[-2][0]) // MSG.itemsize
    assert launched >= 4 and found >= 2 and searched >= 2, (launched, found, searched)
    _ok(collect(exe, tmp_path, ops), wants)


def test_crafted_slots_at_every_small_shape(exe, tmp_path):
    """Random records under full and empty counts: n_ch 1, 3, 70, blocks of 128 and 512, quota 8 and 4096, 0, 1 and 64
    expectations, 0, 1 and 8 centres; levels and the spectrum beside them."""
    rng = np.random.default_rng(2)
    ops, wants = [], []
    for n_ch, n_win in SHAPES:
        s = crafted_bursts(rng, n_ch, n_win)
        ops.append(op(BURSTS, n_ch, n_win, K, slot=s.buf))
        wants.append(want_bursts(s))
        s, qs = crafted_decode(rng, n_ch, n_win)
        for q in (None, qs):
            ops += [op(DECODE, n_ch, n_win, K, slot=s.buf, q=None if q is None else q.buf), op(FORGET)]
            wants += [want_decode(s, q), ()]
        for n in (0, 1, 64):
            x, cand = crafted_expect(rng, n)
            for q in (None, qs):
                ops += [op(EXPECT, n_ch, n_win, K, n=n, slot=x.buf, q=None if q is None else q.buf, cand=cand), op(FORGET)]
                wants += [want_expect(x, q, n), ()]
            ops += [op(EXPECT, n_ch, n_win, K, n=n, slot=None, q=qs.buf, cand=cand), op(FORGET)]   # nothing launched
            wants += [want_expect(None, qs, n), ()]
        for n in (0, 1, 8):
            x = crafted_search(rng, n_ch, n)
            ops += [op(SEARCH, n_ch, 0, K, n=n, slot=x.buf), op(FORGET)]
            wants += [want_search(x, n), ()]
        ops += [op(SEARCH, n_ch, 0, K, n=0, slot=None), op(FORGET)]                                # never allocated
        wants += [(b"", b""), ()]
        for quota in (8, 4096):
            s = crafted_clips(rng, n_ch, quota)
            ops.append(op(CLIPS, n_ch, quota, K, slot=s.buf))
            wants.append(want_clips(s))
        s = crafted_levels(rng, n_ch)
        ops.append(op(LEVELS, n_ch, 0, K, slot=s.buf))
        wants.append((s["lv"].tobytes(), s["in"].tobytes()))
    for n_bins in (64, 4096):
        s = crafted_spectrum(rng, n_bins)
        ops.append(op(SPECTRUM, 0, n_bins, K, slot=s.buf))
        wants.append((s["info"].tobytes(), s["power"].tobytes()))
    _ok(collect(exe, tmp_path, ops), wants)


# ------------------------------------------------------------------------------------------ 2. every refusal
def _refusals():
    """[(name, operation, message)]: a slot that is well-formed but for one fault, at the first or the last channel / entry."""
    rng = np.random.default_rng(3)
    out = []
    for n_ch, n_win in SHAPES:
        cap = cap_of(n_win)
        for c in sorted({0, n_ch - 1}):
            tag = f"{n_ch}ch_{n_win}w_at{c}"
            # bursts
            base = crafted_bursts(rng, n_ch, n_win)
            for what, (chunk, n) in dict(fresh=(NO_ENTRY, NO_ENTRY), before=(K - 1, 0), after=(K + 1, 0), over=(K, cap + 1), huge=(K, NO_ENTRY)).items():
                s = base.copy()
                if what == "fresh":
                    s["floor"].view(np.uint8).reshape(n_ch, -1)[c] = 0xFF
                else:
                    s["floor"]["chunk"][c], s["floor"]["n_bursts"][c] = chunk, n
                out.append((f"bursts_{what}_{tag}", op(BURSTS, n_ch, n_win, K, slot=s.buf),
                            f"burst floor record of channel {c} belongs to chunk {chunk} ({n} runs), not {K}"))
            # decode and its quality rows
            base, qs = crafted_decode(rng, n_ch, n_win)
            for what, (chunk, n) in dict(fresh=(NO_ENTRY, NO_ENTRY), before=(K - 1, 1), after=(K + 1, 1), over=(K, cap + 1), huge=(K, NO_ENTRY)).items():
                s = base.copy()
                if what == "fresh":
                    s["hdr"].view(np.uint8).reshape(n_ch, -1)[c] = 0xFF
                else:
                    s["hdr"]["chunk"][c], s["hdr"]["n_msgs"][c] = chunk, n
                out.append((f"decode_{what}_{tag}", op(DECODE, n_ch, n_win, K, slot=s.buf, q=qs.buf),
                            f"burst message header of channel {c} belongs to chunk {chunk} ({n} messages), not {K}"))
            for i in sorted({0, cap - 1}):
                for other in (K - 1, K + 1, NO_ENTRY):
                    q = qs.copy()
                    q["rows"]["chunk"][c, i] = other
                    out.append((f"decode_quality_{other}_{tag}_{i}", op(DECODE, n_ch, n_win, K, slot=base.buf, q=q.buf),
                                f"quality record {i} of channel {c} belongs to chunk {other}, not {K}"))
            # search: centre c of 8 would not do - the fault at the first and the last (centre, channel)
            n = 8
            base = crafted_search(rng, n_ch, n)
            i = 0 if c == 0 else n - 1
            for what, (chunk, m) in dict(fresh=(NO_ENTRY, NO_ENTRY), before=(K - 1, 1), after=(K + 1, 1), over=(K, BS_PER + 1), huge=(K, NO_ENTRY)).items():
                s = base.copy()
                if what == "fresh":
                    s["hdr"].view(np.uint8).reshape(BS_MAX, n_ch, -1)[i, c] = 0xFF
                else:
                    s["hdr"]["chunk"][i, c], s["hdr"]["n_msgs"][i, c] = chunk, m
                out.append((f"search_{what}_{tag}", op(SEARCH, n_ch, 0, K, n=n, slot=s.buf),
                            f"search header of centre {i}, channel {c} belongs to chunk {chunk} ({m} messages), not {K}"))
            # clips
            for quota in (8, 4096) if n_win == 1 else ():       # (the clip slot does not depend on the windows)
                base = crafted_clips(rng, n_ch, quota)
                h0 = base["hdr"][c]
                faults = dict(fresh=(NO_ENTRY, NO_ENTRY, NO_ENTRY), before=(K - 1, int(h0["n_clips"]), int(h0["used"])),
                              after=(K + 1, int(h0["n_clips"]), int(h0["used"])), over=(K, BC_PER + 1, int(h0["used"])),
                              huge=(K, NO_ENTRY, int(h0["used"])), used=(K, int(h0["n_clips"]), quota + 1), used_huge=(K, 0, NO_ENTRY))
                for what, (chunk, m, used) in faults.items():
                    s = base.copy()
                    if what == "fresh":
                        s["hdr"].view(np.uint8).reshape(n_ch, -1)[c] = 0xFF
                    else:
                        s["hdr"]["chunk"][c], s["hdr"]["n_clips"][c], s["hdr"]["used"][c] = chunk, m, used
                    out.append((f"clips_{what}_{quota}_{tag}", op(CLIPS, n_ch, quota, K, slot=s.buf),
                                f"clip header of channel {c} belongs to chunk {chunk} ({m} clips, {used} outputs), not {K}"))
                used = int(h0["used"])
                for i in (0, BC_PER - 1):                    # (channels 0 and n_ch - 1 hold BC_PER clips)
                    for off, m in ((used, 1), (0, used + 1), (NO_ENTRY, 1), (1, NO_ENTRY), (NO_ENTRY, NO_ENTRY)):
                        s = base.copy()
                        s["recs"]["offset"][c, i], s["recs"]["n"][c, i] = off, m
                        out.append((f"clips_clip_{off}_{m}_{quota}_{tag}_{i}", op(CLIPS, n_ch, quota, K, slot=s.buf),
                                    f"clip {i} of channel {c} lies at {off} + {m} of {used} outputs"))
            # levels
            base = crafted_levels(rng, n_ch)
            for other in (K - 1, K + 1, NO_ENTRY):
                s = base.copy()
                s["lv"]["chunk"][c] = other
                out.append((f"levels_{other}_{tag}", op(LEVELS, n_ch, 0, K, slot=s.buf), f"level record of channel {c} belongs to chunk {other}, not {K}"))
        if n_win != 1:
            continue
        s = crafted_levels(rng, n_ch)
        s.buf[:] = 0xFF
        out.append((f"levels_fresh_{n_ch}", op(LEVELS, n_ch, 0, K, slot=s.buf), f"level record of channel 0 belongs to chunk {NO_ENTRY}, not {K}"))
        s = crafted_levels(rng, n_ch)
        s["in"]["chunk"] = K + 1
        out.append((f"levels_input_{n_ch}", op(LEVELS, n_ch, 0, K, slot=s.buf), f"the input level record belongs to chunk {K + 1}, not {K}"))
    # expect: the fault at the first and the last entry of a table of 1 and of 64
    _, qs = crafted_decode(rng, 3, 4)
    for n in (1, 64):
        for i in sorted({0, n - 1}):
            base, cand = crafted_expect(rng, n)
            note = int(cand[i])
            faults = dict(fresh=(NO_ENTRY, NO_ENTRY, NO_ENTRY), before=(K - 1, 1, note), after=(K + 1, 1, note), two=(K, 2, note),
                          huge=(K, NO_ENTRY, note), more=(K, 1, (note + 1) % 2 ** 32), fewer=(K, 0, (note - 1) % 2 ** 32))
            for what, (chunk, m, got) in faults.items():
                s = base.copy()
                s["hdr"]["chunk"][i], s["hdr"]["n_msgs"][i], s["hdr"]["candidates"][i] = chunk, m, got
                if what == "fresh":
                    s.buf[:] = 0xFF
                    if i:
                        continue                             # (a fresh slot fails at its first entry)
                out.append((f"expect_{what}_{n}_at{i}", op(EXPECT, 3, 4, K, n=n, slot=s.buf, q=qs.buf, cand=cand),
                            f"expectation {i}: header of chunk {chunk} ({m} messages, {got} candidates), not of chunk {K} with {note} candidates"))
            for other in (K - 1, K + 1, NO_ENTRY):
                q = qs.copy()
                q["xrows"]["chunk"][i] = other
                out.append((f"expect_quality_{other}_{n}_at{i}", op(EXPECT, 3, 4, K, n=n, slot=base.buf, q=q.buf, cand=cand),
                            f"quality record of expectation {i} belongs to chunk {other}, not {K}"))
    for n_bins in (64, 4096):
        for what, (chunk, bins) in dict(fresh=(2 ** 64 - 1, NO_ENTRY), before=(K - 1, n_bins), after=(K + 1, n_bins), bins=(K, 2 * n_bins)).items():
            s = crafted_spectrum(rng, n_bins)
            s["info"][0] = (chunk, 3, bins)
            out.append((f"spectrum_{what}_{n_bins}", op(SPECTRUM, 0, n_bins, K, slot=s.buf),
                        f"the spectrum record belongs to chunk {chunk} ({bins} bins), not {K} ({n_bins} bins)"))
    return out


def test_every_refusal_names_its_channel_and_reads_nothing_beyond_the_slot(exe, tmp_path):
    cases = _refusals()
    assert len({name for name, _, _ in cases}) == len(cases) > 400
    ops = []
    for _, o, _ in cases:
        ops += [o, op(FORGET)]
    got = collect(exe, tmp_path, ops)[::2]
    for (name, _, want), (rc, hist, msg, arrays) in zip(cases, got):
        assert (rc, msg, arrays) == (ERR_DEVICE, want, []), name
        assert hist in (0, -1), name                         # a history is left unfinished: what it delivered is unknown


# ------------------------------------------------------------------------------------------ 3. the delivered history
SL = 14


def _message(channel, time, byte, flags=1, g=0):
    m = np.zeros(1, MSG)[0]
    m["channel"], m["time"], m["flags"], m["data"], m["pad"] = channel, time % 2 ** 64, flags, [byte] * 10, [0, 0, 0, g]
    return m


def _seam_pair(n_ch, n_win):
    """(before, after): chunk k - 1 delivers one packet per channel, near 0, 2^64 and in between; chunk k reports each again
    at every offset around SL, with and without the look-back flag, and something else behind it."""
    before, after = decode_slot(n_ch, n_win), decode_slot(n_ch, n_win)
    for s in (before, after):
        s["hdr"]["n_msgs"], s["hdr"]["long_runs"], s["hdr"]["pad"] = 0, 0, 0
    offs = list(range(-SL - 1, SL + 2))
    for c in range(n_ch):
        t = (5000, 0, 2 ** 64 - 3)[c % 3]
        before["recs"][c, 0], before["hdr"]["n_msgs"][c] = _message(c, t, 16 + c), 1
        after["recs"][c, 0] = _message(c, t + offs[c % len(offs)], 16 + c, flags=0 if c % 11 == 10 else 1)
        after["recs"][c, 1] = _message(c, t, 17 + c) if c % 2 else _message((c + 1) % n_ch, t, 16 + c, flags=0)
        after["hdr"]["n_msgs"][c] = 2
    return before, after


def _as(slot, chunk):
    s = slot.copy()
    s["hdr"]["chunk"] = chunk
    return s


def test_delivered_history_of_the_decoder(exe, tmp_path):
    n_ch, n_win = 70, 4
    before, after = _seam_pair(n_ch, n_win)
    d = lambda s, k: op(DECODE, n_ch, n_win, k, SL, slot=_as(s, k).buf)
    bad = _as(after, 11)
    bad["hdr"]["n_msgs"][n_ch - 1] = 3
    ops = [d(before, 4), d(after, 5),                        # k - 1 collected, then k: the seam repeats are dropped
           d(after, 7),                                      # 6 was skipped: nothing is dropped
           d(after, 8),                                      # ... and 8 repeats what 7 delivered, where it looked back
           op(FORGET), d(after, 0),                          # after forget(): nothing is dropped, chunk 0 has no chunk -1
           d(before, 10), op(DECODE, n_ch, n_win, 11, SL, slot=bad.buf), d(after, 12)]   # 11 failed: 12 drops nothing
    got = collect(exe, tmp_path, ops)
    delivered = lambda r: list(as_rows(r[3][0], MSG))
    everything = want_decode(after, None)
    dropped = want_decode(after, None, delivered(got[0]), SL)
    n_all, n_kept = len(everything[0]) // 64, len(dropped[0]) // 64
    offs = list(range(-SL - 1, SL + 2))
    assert n_all == 2 * n_ch and n_all - n_kept == sum(abs(offs[c % len(offs)]) < SL and c % 11 != 10 for c in range(n_ch)) > 50
    assert [r[:3] for r in got[:4]] == [(OK, 4, ""), (OK, 5, ""), (OK, 7, ""), (OK, 8, "")]
    assert tuple(got[0][3]) == want_decode(before, None)
    assert tuple(got[1][3]) == dropped
    assert tuple(got[2][3]) == everything
    again = want_decode(after, None, delivered(got[2]), SL)
    assert tuple(got[3][3]) == again and len(again[0]) // 64 == n_ch // 2 + n_ch // 11   # only the records that did not look back
    assert got[4][:2] == (OK, -2) and got[5][:2] == (OK, 0) and tuple(got[5][3]) == everything
    assert got[6][:2] == (OK, 10) and got[7][:2] == (ERR_DEVICE, -1) and f"channel {n_ch - 1}" in got[7][2]
    assert got[8][:2] == (OK, 12) and tuple(got[8][3]) == everything


def test_delivered_history_of_expect_and_search(exe, tmp_path):
    """Steps 7' and 7s: no flag is asked for; the search also compares the centre."""
    n, n_ch = 64, 3
    offs = list(range(-SL - 1, SL + 2))
    xa, xb = expect_slot(), expect_slot()
    for s in (xa, xb):
        s["hdr"][:n] = [(1, 7, 0, 0)] * n
    for i in range(n):
        t = (5000, 0, 2 ** 64 - 3)[i % 3]
        xa["recs"][i] = _message(i % n_ch, t + 100 * i, i)
        xb["recs"][i] = _message(i % n_ch, t + 100 * i + offs[i % len(offs)], i, flags=8)
    cand = np.full(n, 7, np.uint32)
    sa, sb = search_slot(n_ch), search_slot(n_ch)
    for s in (sa, sb):
        s["hdr"][:] = (BS_PER, 9, 0, 0)
    j = 0
    for i in range(BS_MAX):
        for c in range(n_ch):
            for r in range(BS_PER):
                t = (5000, 0, 2 ** 64 - 3)[j % 3] + 100 * j
                sa["recs"][i, c, r] = _message(c, t, j % 256, 16, g=i)
                sb["recs"][i, c, r] = _message(c, t + offs[j % len(offs)], j % 256, 16, g=i if j % 5 else i + 1)
                j += 1
    x = lambda s, k: op(EXPECT, n_ch, 4, k, SL, n, slot=_as(s, k).buf, cand=cand)
    y = lambda s, k: op(SEARCH, n_ch, 0, k, SL, BS_MAX, slot=_as(s, k).buf)
    ops = [x(xa, 4), x(xb, 5), x(xb, 7), op(FORGET), x(xb, 0), y(sa, 0), y(sb, 1), y(sb, 3), op(FORGET), y(sb, 0)]
    got = collect(exe, tmp_path, ops)
    assert [r[:2] for r in got] == [(OK, 4), (OK, 5), (OK, 7), (OK, -2), (OK, 0), (OK, 0), (OK, 1), (OK, 3), (OK, -2), (OK, 0)]
    all_x, all_s = want_expect(xb, None, n), want_search(sb, BS_MAX)
    kept_x = want_expect(xb, None, n, list(as_rows(got[0][3][0], MSG)), SL)
    kept_s = want_search(_as(sb, 1), BS_MAX, list(as_rows(got[5][3][0], MSG)), SL)
    assert len(all_x[0]) // 64 == n and 20 <= n - len(kept_x[0]) // 64 <= n - 2
    assert 0 < len(kept_s[0]) < len(all_s[0]) and len(kept_s[0]) // 64 > len(all_s[0]) // 64 * 7 // 31   # another centre: kept
    assert tuple(got[1][3][:2]) == kept_x[:2] and tuple(got[2][3][:2]) == all_x[:2] and tuple(got[4][3][:2]) == all_x[:2]
    assert tuple(got[6][3]) == kept_s and got[7][3][0] == all_s[0] and tuple(got[9][3]) == all_s


# ------------------------------------------------------------------------------------------ 4. the repeat rule
def test_one_repeat_rule_equals_the_three_it_replaced(exe):
    out = run(exe, "rule")
    assert "rule ok: 6000 cases" in out
    a, b, c = (int(v) for v in out.split()[-3:])
    assert 100 < a < b and 100 < c < b, out                  # each form said yes and no often, and the three differ
