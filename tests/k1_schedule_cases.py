"""The work-queue schedule of k_demod_mfma (rtldavis_amd/csrc/rd_demod_mfma.hip) at small shapes.  TEST INFRASTRUCTURE ONLY:
no tests in here; tests/test_k1_schedule_cpu.py checks the model and the inputs on the CPU, tests/test_k1_schedule.py runs the
cases on the device.

A wave of the persistent grid takes chunk number wave_id first and draws every further chunk from work queue
wave_id % RD_NQUEUE (an atomic add; queue q owns the chunks nwaves + q + RD_NQUEUE k).  On the product's grid that happens
only past 16384 tiles; the test hook RD_TEST_K1_WGS caps the grid at 8 workgroups (32 waves), so that a few hundred tiles
already give every wave several chunks.  This module restates

  the launch arithmetic   `launch`: tiles per chunk, chunks, waves (rd_mf_launch_variant);
  a wave's walk           `walk`: rd_mf_chunk_at / rd_mf_next, and per tile `carry`, `follows`, the 4-tile store group with
                          `st_flush`, the forced bits of `gmask`, the pending row (k_demod_mfma's loop);
  draw orders             `simulate`: which wave draws which chunk is not deterministic - waves are picked at random, each
                          draws at the start of every chunk it enters;
  what the grid fixes     `forced_groups`: the fix-up entries that do not depend on the data - the first group of every
                          chunk's first tile, all four groups of word 0 of a stream without history, the first group of a
                          tile with ti == 0 inside a chunk - and exactly-once coverage of every (stream, tile);
  the kernel's outputs    `kernel_outputs`: the words it stores, the list it writes and the g it dumps, from the walk and
                          the fp32 model of tests/near_tie_cases.py; with a MUTANT, what a kernel with that fault would write;
  the check               `check_outputs`: what the GPU test asserts of the kernel's outputs and the CPU test of the model's.

Inputs: synth bursts (packets for the batch path) with near-ties planted by near_tie_cases.plant at every tile boundary -
t mod 2048 in 0..3 or the last 8 samples of the tile before - in the classes "deep inside the band" and "guard value at
1.5 c0", and two dense tiles (a flagged plant in every 32-sample word) that are the last tile of a drawn chunk at every
chunk length used, so that the pending row carries 64 entries into the next chunk.  Every shape comes in three data sets:
bits left in place by an earlier run never pass for a run that skipped a chunk.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import near_tie_cases as NT
from rtldavis_amd import synth

TILE = NT.TILE
BLOCK = 8192
RD_NQUEUE = 32          # rd_internal.h
WAVES_PER_WG = 4        # RD_MF_WAVES
STAGE_TILES = 4         # RD_MF_STAGE_TILES
PEND = 64               # RD_MF_PEND
TEST_WGS = 8            # RD_TEST_K1_WGS of every case but real_grid
AMP = (64, 192)         # bytes of the planted windows
N_SETS = 3
MUTANTS = ("queue1", "carry", "halo", "flush", "pend")


# ---------------------------------------------------------------------------------------------------------------------
# launch arithmetic (rd_mf_launch_variant)
@dataclass(frozen=True)
class Sched:
    total: int      # tiles
    tps: int        # tiles per stream
    chunk: int      # tiles per chunk
    chunks: int
    waves: int
    dynamic: bool   # work queues (chunks of at least four tiles), else equal shares: cur_chunk += nwaves


def launch(ns, n, n_cu=256, per_cu=4, chunk_env=0, test_wgs=0) -> Sched:
    tps = (n + TILE - 1) // TILE
    total = ns * tps
    chunk = max(chunk_env, 2) if chunk_env > 0 else 8     # (RD_K1_CHUNK=1 is raised to 2: see `simulate`, one_tile_chunks)
    if chunk_env <= 0:
        waves = n_cu * per_cu * WAVES_PER_WG
        while chunk > STAGE_TILES and total // chunk < waves:
            chunk -= STAGE_TILES
    chunk = min(chunk, total)
    chunks = (total + chunk - 1) // chunk
    wgs = (chunks + WAVES_PER_WG - 1) // WAVES_PER_WG
    max_wgs = n_cu * per_cu
    if test_wgs > 0:
        max_wgs = min(max_wgs, max(test_wgs, RD_NQUEUE // WAVES_PER_WG))
    wgs = min(wgs, max_wgs)
    nwaves = wgs * WAVES_PER_WG
    dynamic = chunk >= 4
    assert not dynamic or nwaves >= RD_NQUEUE or chunks <= nwaves, "the launch code refuses this grid"
    return Sched(total, tps, chunk, chunks, nwaves, dynamic)


# ---------------------------------------------------------------------------------------------------------------------
# a wave's walk
@dataclass(frozen=True)
class Step:
    tile: int
    s: int
    ti: int
    inchunk: int
    prev: tuple | None    # (s, ti) of the tile this wave processed before (None: the wave's first)

    @property
    def transition(self):   # entered by a jump to another chunk
        return self.inchunk == 0 and self.prev is not None

    @property
    def follows(self):      # rd: nx1.s == s && nx1.ti == ti + 1, seen from the tile that was fetched
        return self.prev is not None and self.prev == (self.s, self.ti - 1)


def walk(sc: Sched, chunk_ids):
    """the tiles of a wave that takes these chunks in turn (rd_mf_chunk_at for a chunk's first tile, rd_mf_next inside);
    the kernel's loop ends at the first tile >= total"""
    out, prev = [], None
    for c in chunk_ids:
        assert 0 <= c < sc.chunks
        for k in range(sc.chunk):
            g = c * sc.chunk + k
            if g >= sc.total:
                return out
            s, ti = divmod(g, sc.tps)
            out.append(Step(g, s, ti, k, prev))
            prev = (s, ti)
    return out


def simulate(sc: Sched, rng, queue_init=0, check=True):
    """One draw order: {wave: [chunk ids]}.  queue_init: the value the queue words hold at launch (0; 1 is the MUTANT of a
    counter set nobody cleared).  check: exactly-once coverage, and no drawn chunk is the successor of the chunk before it
    (`follows` is unreachable at a transition).
    Equal shares with ONE tile per chunk (a Sched built by hand: `launch` raises RD_K1_CHUNK=1 to 2, as the launch code
    does) walk as the kernel would: it works out the tile after next (nx2) from `nextc` before the iteration that notes
    that nx1 entered a new chunk has advanced `nextc`, so chunk w + nwaves is taken twice - what the device showed at
    RD_K1_CHUNK=1 before the launch code raised it (41 words listed twice on short40)."""
    seqs = {w: [w] for w in range(sc.waves) if w < sc.chunks}
    if not sc.dynamic:
        seqs = {w: list(range(w, sc.chunks, sc.waves)) for w in seqs}
        if sc.chunk == 1:
            seqs = {w: ids[:2] + ids[1:] if len(ids) > 1 else ids for w, ids in seqs.items()}
    else:
        counters = [queue_init] * RD_NQUEUE
        active = sorted(seqs)
        while active:
            w = active[int(rng.integers(len(active)))]     # this wave enters the last chunk of its list and draws
            q = w % RD_NQUEUE
            nid = sc.waves + q + RD_NQUEUE * counters[q]
            counters[q] += 1
            ends = (seqs[w][-1] + 1) * sc.chunk >= sc.total   # the launch's last chunk: the loop leaves at `total`
            if nid < sc.chunks and not ends:
                seqs[w].append(nid)
            else:
                assert not (nid < sc.chunks) or not check, "a drawn chunk is lost behind the last tile"
                active.remove(w)
    if check:
        seen = np.zeros(sc.total, dtype=np.int64)
        for w, ids in seqs.items():
            for st in walk(sc, ids):
                seen[st.tile] += 1
                assert not (st.transition and st.follows), "a drawn chunk follows the chunk before it"
        assert (seen == 1).all(), f"tiles processed {np.unique(seen)} times"
    return seqs


def queue_loads(sc: Sched):
    """chunks each queue hands out (beyond the waves' first ones)"""
    return [len(range(sc.waves + q, sc.chunks, RD_NQUEUE)) for q in range(RD_NQUEUE)] if sc.dynamic else []


def forced_groups(sc: Sched, ns, n, hist: bool):
    """[ns, ceil(n / 32) * 4] bool: the groups the kernel lists whatever the data, by the chunk grid alone"""
    words = (n + 31) // 32
    out = np.zeros((ns, words * 4), dtype=bool)
    for g in range(sc.total):
        s, ti = divmod(g, sc.tps)
        if g % sc.chunk == 0 or ti == 0:
            if ti == 0 and not hist:
                out[s, :4] = True
            else:
                out[s, 4 * 64 * ti] = True
    return out


def tile_kinds(sc: Sched):
    """{kind: [tile]}: the tiles the plants are placed around.  drawn_first / drawn_second: first and second tile of a chunk
    taken from a queue; chunk_last: the last tile of a chunk that another chunk's tile follows in the stream;
    after_boundary: a stream's first tile inside a chunk."""
    first_drawn = sc.waves if sc.dynamic else sc.chunks     # chunk ids from here on come from a queue
    k = {"drawn_first": [], "drawn_second": [], "chunk_last": [], "after_boundary": []}
    for g in range(sc.total):
        c, inch = divmod(g, sc.chunk)
        ti = g % sc.tps
        if c >= first_drawn and inch == 0:
            k["drawn_first"].append(g)
        if c >= first_drawn and inch == 1:
            k["drawn_second"].append(g)
        if (inch == sc.chunk - 1) and g + 1 < sc.total and (g + 1) % sc.tps != 0:
            k["chunk_last"].append(g)
        if inch > 0 and ti == 0:
            k["after_boundary"].append(g)
    return k


# ---------------------------------------------------------------------------------------------------------------------
# inputs
@dataclass(frozen=True)
class Shape:
    name: str
    ns: int
    n: int
    hist: bool = False
    dense: tuple = ()       # (s, ti): tiles with a flagged plant in every word
    burst_margin: int = BLOCK


SHAPES = {
    # 132 tiles per stream, 396 tiles.  The dense tiles 199 and 239 (39 mod 40) are the last of their chunk at 4, 5 and 8
    # tiles per chunk.  With 32 waves every queue has one wave: wave w takes the chunks w, 32 + w, 64 + w, ...  At 4 and 5
    # tiles per chunk both lie in a drawn chunk with another chunk of its queue behind it (at 8 no queue holds more than
    # one chunk: nothing follows a drawn chunk there).  Two, not more: the three streams share one fix-up bucket of the
    # one-launch tail (FIX_BCAP), which this content must fit for the batch runs to stay in their first pass
    "long3": Shape("long3", 3, 33 * BLOCK, dense=((1, 67), (1, 107))),
    # 4 tiles per stream: streams 3 and 5 are the first chunks of waves 3 and 5 at 4 tiles per chunk (chunks 35 and 37 follow)
    "short40": Shape("short40", 40, BLOCK, dense=((3, 3), (5, 3)), burst_margin=1024),
    "hist": Shape("hist", 3, 33 * BLOCK, hist=True, dense=((1, 67), (1, 107))),
    # 21 tiles per stream, the last ragged: tile 146 (stream 6's last) is the third of drawn chunk 36, the wave goes on with
    # stream 7's first tile.  Dense: tile 23, the last of wave 5's first chunk
    "ragged": Shape("ragged", 9, 20 * TILE + 1000, dense=((1, 2),), burst_margin=2048),
}


def _slots(sh: Shape, rng):
    """(s, t, kind) for one data set: one plant at every tile boundary - `start`: t mod 2048 in 0..3, or `end`: the last 8
    samples of the tile before - and around every stream boundary; the dense tiles"""
    tps = (sh.n + TILE - 1) // TILE
    dense = set(sh.dense)
    slots = []
    # (one in eight inside the band: the listed words of a group of four streams must fit the one-launch tail's bucket,
    # fix_bcap, also where real_grid puts a stream with dense tiles beside three others)
    kinds = ("deep+", "deep-") + ("out1.5",) * 14
    for s in range(sh.ns):
        for ti in range(1, tps):
            kind = kinds[int(rng.integers(16))]
            start = bool(rng.integers(2)) or (s, ti - 1) in dense or (s, ti) in dense
            t = ti * TILE + (int(rng.integers(4)) if start else -8 + int(rng.integers(8)))
            slots.append((s, t, kind))
        # a stream's last samples (the window reaches t + 2), and the first word behind the stream's first run
        if (s, tps - 1) not in dense:
            slots.append((s, sh.n - 8 + int(rng.integers(6)), ("deep+", "deep-", "out1.5", "out1.5")[int(rng.integers(4))]))
        slots.append((s, (12 if sh.hist else 32) + int(rng.integers(4)), kinds[int(rng.integers(16))]))
    for s, ti in sh.dense:
        for wd in range(64):
            # (offsets that keep 16 samples to the plants at the tile's two boundaries)
            off = 20 if wd == 0 else 12 if wd == 63 else 16
            slots.append((s, ti * TILE + 32 * wd + off + int(rng.integers(4)), ("deep", "band")[int(rng.integers(2))]))
    return slots


def _build(sh: Shape, k: int) -> NT.Case:
    for attempt in range(8):
        seed = [4100 + sorted(SHAPES).index(sh.name), k, attempt]
        rng = np.random.default_rng(seed)
        streams = np.stack([synth.synth_stream(int(rng.integers(1 << 30)), n_samples=sh.n, margin=sh.burst_margin)
                            for _ in range(sh.ns)])
        hist = rng.integers(AMP[0], AMP[1] + 1, size=(sh.ns, 64), dtype=np.uint8) if sh.hist else None
        slots = _slots(sh, rng)
        for s in range(sh.ns):
            ts = sorted(t for s_, t, _ in slots if s_ == s)
            assert all(b - a >= 16 for a, b in zip(ts, ts[1:])) and ts[0] >= 10 and ts[-1] + 2 < sh.n, sh.name
        plants = NT.plant(streams, slots, rng, AMP[0], AMP[1], reuse=4)
        c = NT.evaluate(NT.Case(f"{sh.name}/{k}", streams, hist, plants))
        if NT.margin_ok(c) and not c.zeros:
            c.streams.setflags(write=False)
            return c
    raise AssertionError(f"{sh.name}/{k}: no draw met its conditions")


@functools.lru_cache(maxsize=None)
def data(shape: str, k: int) -> NT.Case:
    """data set k (0 .. N_SETS - 1) of a shape, evaluated: exact bits, fp32 model, flagged groups (near_tie_cases.Case)"""
    return _build(SHAPES[shape], k)


# the kernel-hook and batch cases: (name, shape, RD_K1_CHUNK); the grid is RD_TEST_K1_WGS = 8 workgroups
CASES = (("long3", 4), ("long3", 5), ("long3", 8), ("short40", 4), ("short40", 8), ("hist", 4), ("ragged", 4),
         ("short40", 1), ("short40", 3))
BATCH_SHAPES = ("long3", "short40")     # whole blocks without history: also through BatchDemodulator


def sched_of(shape: str, chunk_env: int) -> Sched:
    sh = SHAPES[shape]
    return launch(sh.ns, sh.n, chunk_env=chunk_env, test_wgs=TEST_WGS)


def fix_bcap(n):
    """entries a group's fix-up bucket holds (rd_batch_plan.cpp: rd_batch_sizes_of), a group being RD_FT_STREAMS = 4 consecutive streams"""
    tps = (n + TILE - 1) // TILE
    return min((2 * 4 * (tps // 4 + 8) + 63) & ~63, 1 << 20)


def bucket_loads(c: NT.Case, sc: Sched):
    """entries per group of four streams: what the demod kernel puts into the one-launch tail's buckets"""
    w = expected_groups(c, sc)
    ns = w.shape[0]
    per = np.array([int(np.pad(w[s], (0, (-w.shape[1]) % 4)).reshape(-1, 4).any(axis=1).sum()) for s in range(ns)])
    return np.add.reduceat(per, np.arange(0, ns, 4))


# real_grid: no RD_TEST_K1_WGS; RD_K1_WGS_PER_CU = 1 and RD_K1_CHUNK = 4: 40 streams x 33 blocks, 5280 tiles, 1320 chunks
# against 1024 waves on 256 CUs.  Stream i of data set k is one of the nine long3 streams.
REAL_NS, REAL_CHUNK = 40, 4


def real_grid_sources(k: int):
    """-> long3 data set j // 3, stream j % 3.  Every group of four streams (a bucket of the one-launch tail) gets exactly
    one stream with dense tiles (stream 1 of a data set), as its second"""
    plain, dense = (0, 2, 3, 5, 6, 8), (1, 4, 7)
    return [dense[(i // 4 + k) % 3] if i % 4 == 1 else plain[(3 * (i // 4) + i % 4 + 2 * k) % 6] for i in range(REAL_NS)]


def real_grid_input(k: int):
    return np.stack([data("long3", j // 3).streams[j % 3] for j in real_grid_sources(k)])


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's outputs from the walk
def _pack(bits01):
    ns, n = bits01.shape
    words = (n + 31) // 32
    pad = np.zeros((ns, words * 32), dtype=np.uint8)
    pad[:, :n] = bits01
    return np.packbits(pad, axis=1, bitorder="little").view(np.uint32).reshape(ns, words)


def _group_masks(c: NT.Case, flagged):
    ns, ng = flagged.shape
    words = (c.n + 31) // 32
    pad = np.zeros((ns, 4 * words), dtype=np.int64)
    pad[:, :ng] = flagged
    return (pad.reshape(ns, words, 4) << np.arange(4)).sum(axis=-1)


def kernel_outputs(c: NT.Case, sc: Sched, seqs, mutant=None):
    """(words [ns, ceil(n / 32)] uint32 as stored before any fix-up, entries of the list, samples of g that differ from
    the integer model, notes) for the draw order `seqs`.  The stored signs are the fp32 model's; inside a forced group the
    kernel's are arbitrary, and nothing may depend on them.  mutant: None, or the fault to apply -
      carry   carry = ti > 0, without the inchunk term: a chunk's first tile trusts a predecessor it never saw
      halo    the 16 halo bytes come from the wave's registers at a transition too: the last 8 samples of the tile the wave
              processed before stand in front of the new tile
      flush   st_flush ignored: staged tiles are stored four at a time at the first one's address
      pend    the pending row is reset, not flushed, when a wave enters a drawn chunk
    (queue1 is simulate's queue_init = 1.)  notes: counts of what the mutant touched."""
    ns, n = c.streams.shape[0], c.n
    words = (n + 31) // 32
    hist = c.hist is not None
    ragged_n = n % TILE != 0
    fast = c.fast.copy()
    flagged = c.flagged.copy()
    g_bad = 0
    notes = {"transitions": 0, "entries_lost": 0, "tiles_misplaced": 0, "forced_missing": 0, "signs_changed": 0}
    walks = {w: walk(sc, ids) for w, ids in seqs.items()}
    if mutant == "halo":
        for steps in walks.values():
            for st in steps:
                if not st.transition or (st.ti == 0 and not hist):
                    continue     # (no history: the first run's g is never looked at and its word is listed whole)
                ps, pti = st.prev
                if (pti + 1) * TILE > n:
                    continue     # (behind a ragged tile the registers hold padding: left alone)
                t0 = st.ti * TILE
                win = np.concatenate([c.streams[ps, 2 * ((pti + 1) * TILE - 8): 2 * (pti + 1) * TILE],
                                      c.streams[st.s, 2 * t0: 2 * (t0 + 12)]])
                gw = NT.kernel_g32(win, None)           # index (window sample) + 1; g[local k] = window k + 8
                loc = gw[10: 21]                        # g[local 1 .. 11]
                true = c.g32[st.s, t0 + 2: t0 + 13]
                diff = (loc[:8] != true[:8]).any(axis=-1)
                g_bad += int(diff.sum())
                lm = NT.lane_model(loc[None, 6: 11])    # lane 2 of the tile: g[local 7 .. 11]
                fast[st.s, t0 + 8: t0 + 12] = lm.fast_bits[0]
                flagged[st.s, t0 // 8 + 1] = bool(lm.lane_flag[0, 0]) or bool(c.lane.lane_flag[st.s, t0 // 4 + 3])
                notes["signs_changed"] += int((lm.fast_bits[0] != c.fast[st.s, t0 + 8: t0 + 12]).sum())
    fastw = _pack(fast)
    masks = _group_masks(c, flagged)
    flat = np.zeros(ns * words, dtype=np.uint32)
    written = np.zeros(ns * words, dtype=bool)       # holds its own tile's data
    entries = []
    for w in sorted(walks):
        steps = walks[w]
        staged, base, st_flush = [], 0, False
        pend = []

        def store():
            for q, (ds, dti) in enumerate(staged):
                a = base + 64 * q
                src = fastw[ds, 64 * dti: 64 * dti + 64]
                if a + 64 <= flat.size:
                    flat[a: a + 64] = src
                    written[a: a + 64] = a == ds * words + 64 * dti
            staged.clear()

        for i, st in enumerate(steps):
            nxt = steps[i + 1] if i + 1 < len(steps) else None
            notes["transitions"] += st.transition
            if mutant == "pend" and st.transition:
                notes["entries_lost"] += len(pend)
                pend = []
            if len(staged) == STAGE_TILES or (staged and st_flush and mutant != "flush"):
                store()
            carry = st.ti > 0 if mutant == "carry" else (st.inchunk > 0 and st.ti > 0)
            nw = min(64, words - 64 * st.ti)
            m = masks[st.s, 64 * st.ti: 64 * st.ti + nw].copy()
            if not carry:
                m[0] = 0xF if (st.ti == 0 and not hist) else (m[0] | 1)
            elif st.inchunk == 0:
                notes["forced_missing"] += 1
            ragged = ragged_n and st.ti + 1 == sc.tps
            if not ragged:
                if not staged:
                    base = st.s * words + 64 * st.ti
                staged.append((st.s, st.ti))
                next_ragged = nxt is not None and ragged_n and nxt.ti + 1 == sc.tps
                st_flush = not (nxt is not None and nxt.s == st.s and nxt.ti == st.ti + 1 and not next_ragged)
            else:
                a = st.s * words + 64 * st.ti
                flat[a: a + nw] = fastw[st.s, 64 * st.ti: 64 * st.ti + nw]
                written[a: a + nw] = True
            new = [(int(st.s * words + 64 * st.ti + j) << 4) | int(m[j]) for j in range(nw) if m[j]]
            if len(pend) + len(new) > PEND:
                entries += pend
                pend = []
            pend += new
        if staged:
            store()
        entries += pend
    notes["tiles_misplaced"] = int((~written).reshape(ns, words)[:, : (n // 32)].sum()) // 64
    return flat.reshape(ns, words), np.array(entries, dtype=np.uint32), g_bad, notes


def pend_at_transitions(c: NT.Case, sc: Sched, seqs):
    """entries in the pending row when a wave enters a drawn chunk: [(wave, tile entered, entries)]"""
    words = (c.n + 31) // 32
    masks = _group_masks(c, c.flagged)
    hist = c.hist is not None
    out = []
    for w, ids in seqs.items():
        npend = 0
        for st in walk(sc, ids):
            if st.transition:
                out.append((w, st.tile, npend))
            nw = min(64, words - 64 * st.ti)
            m = masks[st.s, 64 * st.ti: 64 * st.ti + nw].copy()
            if not (st.inchunk > 0 and st.ti > 0):
                m[0] = 0xF if (st.ti == 0 and not hist) else (m[0] | 1)
            nf = int((m != 0).sum())
            if npend + nf > PEND:
                npend = 0
            npend += nf
    return out


def expected_groups(c: NT.Case, sc: Sched):
    """[ns, n / 8] bool: exactly the groups on the kernel's list - the model's flagged groups and the grid's forced ones"""
    ng = c.flagged.shape[1]
    return c.flagged | forced_groups(sc, c.streams.shape[0], c.n, c.hist is not None)[:, :ng]


def check_outputs(c: NT.Case, sc: Sched, words, entries, g_bad, what=""):
    """What the kernel's outputs must satisfy under schedule `sc` (shared by the GPU test and the CPU module's mutants):
    g is the integer model's; every entry names a word of the launch, once, with a mask; the list is exactly the model's
    flagged groups and the grid's forced ones; outside it every stored sign is the exact one; past a ragged end the words
    are zero."""
    what = what or c.name
    ns, n = c.streams.shape[0], c.n
    nw = (n + 31) // 32
    assert g_bad == 0, f"{what}: g differs from the integer model at {g_bad} samples"
    entries = np.asarray(entries, dtype=np.uint32)
    assert (entries & 15 != 0).all(), f"{what}: an entry with an empty group mask"
    listed, dup = NT.listed_groups(entries, ns, nw)
    assert dup == 0, f"{what}: {dup} words listed twice"
    ng = c.flagged.shape[1]
    assert not listed[:, ng:].any(), f"{what}: a group past the end of a stream is listed"
    listed = listed[:, :ng]
    want = expected_groups(c, sc)
    missing, extra = want & ~listed, listed & ~want
    assert not missing.any(), f"{what}: {int(missing.sum())} groups missing from the list, first (stream, group) {np.argwhere(missing)[:4].tolist()}"
    assert not extra.any(), f"{what}: {int(extra.sum())} groups listed without cause, first (stream, group) {np.argwhere(extra)[:4].tolist()}"
    allbits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(ns, -1), axis=1, bitorder="little")
    assert not allbits[:, n:].any(), f"{what}: bits past the end of a stream"
    bad = (allbits[:, :n] != c.bits) & ~np.repeat(listed, 8, axis=1)
    assert not bad.any(), (f"{what}: {int(bad.sum())} wrong signs outside the list in {int(bad.reshape(ns, -1, 32).any(axis=-1).sum())} "
                           f"words, first (stream, sample) {np.argwhere(bad)[:4].tolist()}")


# ---------------------------------------------------------------------------------------------------------------------
# the batch path's expected values: the C oracle (packets with call, index, bytes, RSSI, SNR; the packed bits)
PACKET_DTYPE = np.dtype([("stream", "<i4"), ("call", "<i4"), ("index", "<i4"), ("nbytes", "<i4"),
                         ("data", "u1", (32,)), ("rssi", "<f8"), ("snr", "<f8")])   # rd_packet (batch.RD_PACKET_DTYPE)


def _records(pk_per_stream):
    out = []
    for pk in pk_per_stream:
        r = np.zeros(len(pk), dtype=PACKET_DTYPE)
        for i, p in enumerate(pk):
            r[i]["call"], r[i]["index"], r[i]["nbytes"] = p.call, p.index, p.data.size
            r[i]["data"][: p.data.size] = p.data
            r[i]["rssi"], r[i]["snr"] = p.rssi, p.snr
        out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(shape: str, k: int):
    from oracle import c_oracle as CO
    pk, bits = CO.demod_batch(np.ascontiguousarray(data(shape, k).streams), CO.make_cfg(), threads=4, want_bits=True)
    return _records(pk), bits


def _join(recs):
    out = np.concatenate([r.copy() for r in recs]) if recs else np.zeros(0, dtype=PACKET_DTYPE)
    out["stream"] = np.repeat(np.arange(len(recs), dtype=np.int32), [len(r) for r in recs])
    return out


def batch_expected(shape: str, k: int):
    """(records of the whole batch in results()' order: stream-major, the oracle's order inside a stream; bits [ns, words])"""
    recs, bits = _oracle(shape, k)
    return _join(recs), bits


def real_grid_expected(k: int):
    src = real_grid_sources(k)
    per = [_oracle("long3", j // 3) for j in src]
    return _join([per[i][0][j % 3] for i, j in enumerate(src)]), np.stack([per[i][1][j % 3] for i, j in enumerate(src)])
