"""The schedule model and the inputs of tests/k1_schedule_cases.py, judged on the CPU alone: the edges every case is there
for, exactly-once coverage under random draw orders, the planted samples against the oracle and the fp32 flag model, and five
mutants of the kernel's chunk transition that the check shared with the GPU test (k1_schedule_cases.check_outputs) must
refuse.  The printed figures are the ones DESIGN.md quotes (pytest -s)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import k1_schedule_cases as K  # noqa: E402
import near_tie_cases as NT  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from oracle import dsp_oracle as O  # noqa: E402

TILE = K.TILE
ORDERS = 12   # random draw orders per case


def test_launch_arithmetic_and_the_edge_of_every_case():
    # the product's formula, no hook: small launches get 4-tile chunks and one wave per chunk, rounded up to a workgroup
    assert K.launch(4, 3 * 8192) == K.Sched(48, 12, 4, 12, 12, True)
    assert K.launch(3, 33 * 8192) == K.Sched(396, 132, 4, 99, 100, True)
    big = K.launch(4096, 33 * 8192)
    assert (big.chunk, big.waves) == (8, 4096) and big.chunks == 67584
    assert K.launch(128, 33 * 8192).chunk == 4 and K.launch(249, 33 * 8192).chunk == 8   # 32868 tiles / 8 >= 4096 waves
    # the hook: never fewer than RD_NQUEUE waves
    for wgs in (1, 7, 8):
        assert K.launch(3, 33 * 8192, chunk_env=4, test_wgs=wgs).waves == 32
    assert K.launch(3, 33 * 8192, chunk_env=4, test_wgs=9).waves == 36

    sc = K.sched_of("long3", 4)
    loads = K.queue_loads(sc)
    assert (sc.chunks, sc.waves, sum(loads)) == (99, 32, 67) and set(loads) == {2, 3}
    def straddling(sc):
        return [c for c in range(sc.chunks) if (c * sc.chunk) // sc.tps != min(c * sc.chunk + sc.chunk - 1, sc.total - 1) // sc.tps]

    sc = K.sched_of("long3", 5)
    assert sc.chunks == 80 and {(c * 5) % sc.tps % 4 for c in range(32, 80)} == {0, 1, 2, 3}, "drawn chunks start at every ti mod 4"
    assert straddling(sc) == [26, 52] and 52 >= sc.waves, "a drawn chunk straddles a stream boundary"
    # 8 tiles per chunk: the stream boundaries are tiles 132 and 264 = 33 * 8, so ONE chunk straddles a boundary (chunk 16,
    # a wave's first chunk: the drawn straddling chunk is the one at 5 tiles above); the last chunk has 4 tiles
    sc = K.sched_of("long3", 8)
    assert sc.chunks == 50 and straddling(sc) == [16] and sc.total - 49 * 8 == 4 and set(K.queue_loads(sc)) == {0, 1}
    sc = K.sched_of("short40", 4)
    assert sc.chunks == 40 and sc.tps == sc.chunk and sum(K.queue_loads(sc)) == 8, "every chunk is a whole stream"
    sc = K.sched_of("short40", 8)
    assert sc.chunks == 20 and len(K.tile_kinds(sc)["after_boundary"]) == 20, "two streams per chunk: inchunk > 0 && ti == 0"
    sc = K.sched_of("ragged", 4)
    assert K.SHAPES["ragged"].n % TILE and K.SHAPES["ragged"].n % 8 == 0
    g = 6 * sc.tps + sc.tps - 1   # stream 6's ragged tile
    assert g // 4 >= sc.waves and g % 4 == 2 and (g + 1) % sc.tps == 0, "the ragged tile inside a drawn chunk, the next stream behind it"
    for ch in (1, 3):
        sc = K.sched_of("short40", ch)
        assert not sc.dynamic and sc.chunks > 1.5 * sc.waves
    assert K.sched_of("short40", 1).chunk == 2 and K.sched_of("short40", 1) == K.sched_of("short40", 2), "RD_K1_CHUNK=1 is raised to 2"
    sc = K.launch(K.REAL_NS, 33 * 8192, n_cu=256, per_cu=1, chunk_env=K.REAL_CHUNK)
    assert (sc.total, sc.chunks, sc.waves) == (5280, 1320, 1024)
    for shape, ch in K.CASES:
        sc = K.sched_of(shape, ch)
        print(f"{shape} chunk {ch}: {sc.total} tiles, {sc.chunks} chunks, {sc.waves} waves, drawn per queue "
              f"{sorted(set(K.queue_loads(sc))) if sc.dynamic else 'equal shares'}")


@pytest.mark.parametrize("shape,chunk", K.CASES)
def test_every_draw_order_covers_every_tile_once_and_writes_the_same(shape, chunk):
    """simulate asserts the coverage and that no transition `follows`; the outputs the model derives from a wave's walk -
    stored words and the set of entries - are the same for every order and pass the shared check, so the forced entries are
    what forced_groups states from the grid alone."""
    sc, c = K.sched_of(shape, chunk), K.data(shape, 0)
    rng = np.random.default_rng(31)
    first = None
    for _ in range(ORDERS if sc.dynamic else 1):
        seqs = K.simulate(sc, rng)
        words, entries, g_bad, _ = K.kernel_outputs(c, sc, seqs)
        K.check_outputs(c, sc, words, entries, g_bad)
        cur = (words.tobytes(), np.sort(entries).tobytes())
        assert first is None or cur == first
        first = cur
    if sc.dynamic and sc.chunks > sc.waves:
        longest = max(len(v) for v in seqs.values())
        assert longest >= 2


@pytest.mark.parametrize("shape", sorted(K.SHAPES))
@pytest.mark.parametrize("k", range(K.N_SETS))
def test_exact_reference_is_the_oracles(shape, k):
    """the checks of test_near_tie_cpu.py at the new positions: the exact integers agree with the oracle everywhere, no
    numerator is zero, the planted ones are far above float64 rounding; the data sets differ from each other"""
    c = K.data(shape, k)
    ns = c.streams.shape[0]
    assert c.zeros == 0 and NT.margin_ok(c)
    if shape in K.BATCH_SHAPES:
        pk, wbits = CO.demod_batch(np.ascontiguousarray(c.streams), CO.make_cfg(), threads=4, want_bits=True)
        for s in range(ns):
            assert np.array_equal(np.unpackbits(wbits[s].view(np.uint8), bitorder="little")[: c.n], c.bits[s]), (shape, k, s)
        # (a batch of ONE block reports positions up to (n_blocks + 1) B - buffer_length = 0 only: short40 has no packet to
        # report by construction, its batch runs are judged by their bits)
        assert sum(len(p) for p in pk) >= (3 if shape == "long3" else 0), "packets for the batch path"
    else:
        for s in range(ns):
            if c.hist is None:
                ob = O.demod_stream_oneshot(c.streams[s])[2]
            else:
                ob = O.demod_stream_oneshot(np.concatenate([c.hist[s], c.streams[s]]))[2][c.hist.shape[1] // 2:]
            assert np.array_equal(ob, c.bits[s]), (shape, k, s)
    G = [NT.exact_G(c.streams[s], None if c.hist is None else c.hist[s]) for s in range(ns)]
    for p in c.plants:
        Gr, Gi = G[p.s]
        N = NT.exact_N_int(Gr, Gi, p.t)
        F2 = max(abs(int(Gr[p.t])), abs(int(Gi[p.t])), abs(int(Gr[p.t + 1])), abs(int(Gi[p.t + 1]))) ** 2
        assert N != 0 and abs(N) >= 1e-10 * F2, (shape, k, p)
        assert c.bits[p.s, p.t] == (N < 0)
    if k:
        assert (K.data(shape, 0).bits != c.bits).mean() > 0.2, "another data set: other bits nearly everywhere"


@pytest.mark.parametrize("shape", sorted(K.SHAPES))
def test_fp32_model_classifies_the_plants_as_intended(shape):
    """deep / band / in-band plants are flagged, the out1.5 ones are trusted with a guard value within (1, 2] c0, and the
    model's guard value of every planted lane is the rational one rounded where fp32 rounds"""
    wrong = 0
    for k in range(K.N_SETS):
        c = K.data(shape, k)
        lm = c.lane
        assert (lm.thr <= NT.C0_MAX).all()
        for i, p in enumerate(c.plants):
            lane = p.t // 4
            if not c.valid[p.s, p.t // 8]:
                continue
            if p.kind == "out1.5":
                assert not lm.lane_flag[p.s, lane] and lm.thr[p.s, lane] < lm.nm[p.s, lane] <= 2 * lm.thr[p.s, lane], (shape, k, p)
            else:
                assert lm.lane_flag[p.s, lane] and c.flagged[p.s, p.t // 8], (shape, k, p)
                wrong += int(c.fast[p.s, p.t] != c.bits[p.s, p.t])
            if i % 7 == 0:
                want = NT.lane_nm_fraction(c.g32[p.s, 4 * lane: 4 * lane + 5])
                assert np.float32(want) == lm.nm[p.s, lane], (shape, k, p)
        w = (c.fast != c.bits) & np.repeat(c.valid, 8, axis=1)
        assert not (w & ~np.repeat(c.flagged, 8, axis=1)).any(), "a wrong fast sign outside the model's band"
    assert wrong >= 20, "the deep plants are where the fast sign is wrong"
    print(f"{shape}: {sum(len(K.data(shape, k).plants) for k in range(K.N_SETS))} plants in {K.N_SETS} data sets, "
          f"{wrong} of the flagged ones with a wrong fast sign")


def _plants_by_tile(c):
    """(s, tile) -> [(where, kind)]: 'start' for t mod 2048 in 0..3, 'end' for the tile's last 8 samples"""
    out = {}
    for p in c.plants:
        r = p.t % TILE
        if r < 4:
            out.setdefault((p.s, p.t // TILE), []).append(("start", p.kind, r))
        elif r >= TILE - 8 or p.t >= c.n - 8:
            out.setdefault((p.s, p.t // TILE), []).append(("end", p.kind, r))
    return out


def test_plants_sit_at_every_kind_of_transition():
    """Around the tiles of every kind (tile_kinds) - at the tile's own start and at the end of the tile in front of it - there
    are plants of both classes, flagged and trusted; over all cases every t mod 2048 in 0..3 occurs in both classes at the
    first and the second tile of a drawn chunk."""
    seen_p = {}
    for shape, ch in K.CASES:
        sc = K.sched_of(shape, ch)
        kinds = K.tile_kinds(sc)
        line = []
        for kind, tiles in kinds.items():
            got = set()
            n_pl = 0
            for k in range(K.N_SETS):
                c = K.data(shape, k)
                by = _plants_by_tile(c)
                for g in tiles:
                    s, ti = divmod(g, sc.tps)
                    here = by.get((s, ti), [])
                    if kind == "chunk_last":     # the end of this tile and the start of the next
                        here = [x for x in here if x[0] == "end"] + [x for x in by.get((s, ti + 1), []) if x[0] == "start"]
                    elif kind == "after_boundary":   # the end of the stream in front (the new stream's first word is forced)
                        here = [x for x in by.get((s - 1, sc.tps - 1), []) if x[0] == "end"]
                    else:                        # the start of this tile and the end of the one in front
                        here = [x for x in here if x[0] == "start"] + ([x for x in by.get((s, ti - 1), []) if x[0] == "end"] if ti else [])
                    for where, pk, r in here:
                        cls = "trusted" if pk == "out1.5" else "flagged"
                        got.add((where, cls))
                        n_pl += 1
                        if where == "start":
                            seen_p.setdefault(kind, set()).add((r, cls))
            inside = [g for g in tiles if g % sc.tps]     # (a stream's first word is forced whole: nothing to plant there)
            if inside and kind != "after_boundary":
                assert got == {(w, cl) for w in ("start", "end") for cl in ("flagged", "trusted")}, (shape, ch, kind, got)
            elif tiles and kind == "after_boundary":
                assert {cl for _, cl in got} == {"flagged", "trusted"}, (shape, ch, kind, got)
            line.append(f"{kind} {len(tiles)} tiles / {n_pl} plants")
        print(f"{shape} chunk {ch}: " + ", ".join(line))
    for kind in ("drawn_first", "drawn_second"):
        assert seen_p[kind] == {(r, cl) for r in range(4) for cl in ("flagged", "trusted")}, (kind, seen_p[kind])


# transitions a wave enters with more than half a row pending, = dense tiles with a transition behind them
DENSE_CARRIES = {("long3", 4): 2, ("long3", 5): 2, ("hist", 4): 2, ("short40", 4): 2, ("ragged", 4): 1}


@pytest.mark.parametrize("shape,chunk", sorted(DENSE_CARRIES))
def test_dense_tiles_fill_the_pending_row_in_front_of_a_transition(shape, chunk):
    """every dense tile is the last of its chunk; the wave enters its next chunk with 33..64 entries pending.  At 4 and 5
    tiles per chunk two of long3's dense tiles end a DRAWN chunk."""
    sc = K.sched_of(shape, chunk)
    drawn = 0
    for s, ti in K.SHAPES[shape].dense:
        g = s * sc.tps + ti
        if DENSE_CARRIES[shape, chunk] == len(K.SHAPES[shape].dense):
            assert g % sc.chunk == sc.chunk - 1, (shape, chunk, s, ti)
        drawn += g // sc.chunk >= sc.waves
    if shape in ("long3", "hist") and chunk in (4, 5):
        assert drawn == 2
    rng = np.random.default_rng(33)
    for k in range(K.N_SETS):
        c = K.data(shape, k)
        assert all(c.flagged_words()[s, 64 * ti: 64 * ti + 64].all() for s, ti in K.SHAPES[shape].dense)
        carried = [n for _, _, n in K.pend_at_transitions(c, sc, K.simulate(sc, rng)) if n > K.PEND // 2]
        assert len(carried) == DENSE_CARRIES[shape, chunk] and max(carried) <= K.PEND, (shape, chunk, k, carried)
    print(f"{shape} chunk {chunk}: pending rows of {carried} entries carried into the next chunk")


def test_more_waves_than_queues_any_order_same_outputs():
    """With 8 workgroups a queue has one wave and the schedule is fixed.  The model at 16 workgroups (two waves per queue,
    as on the product's grid, where it is 32): the draw order changes which wave takes which chunk, not one stored word
    and not the set of entries."""
    sh = K.SHAPES["long3"]
    c = K.data("long3", 0)
    for ch in (4, 5, 8):
        sc = K.launch(sh.ns, sh.n, chunk_env=ch, test_wgs=16)
        assert sc.waves == 64 if ch < 8 else sc.waves == 52
        rng = np.random.default_rng(37)
        outs, shapes = set(), set()
        for _ in range(ORDERS):
            seqs = K.simulate(sc, rng)
            words, entries, g_bad, _ = K.kernel_outputs(c, sc, seqs)
            K.check_outputs(c, sc, words, entries, g_bad)
            outs.add((words.tobytes(), np.sort(entries).tobytes()))
            shapes.add(tuple(len(seqs[w]) for w in sorted(seqs)))
        assert len(outs) == 1 and (len(shapes) > 1 or ch == 8), (ch, len(shapes))


# which cases must refuse which mutant (the others cannot: at 4 and 8 tiles per chunk a store group is always full at a
# transition; short40 at 4 has ti == 0 at every chunk start; equal shares draw from no queue)
KILLS = {
    "queue1": [("long3", 4), ("long3", 5), ("long3", 8), ("short40", 4), ("hist", 4), ("ragged", 4)],
    "carry": [("long3", 4), ("long3", 5), ("long3", 8), ("hist", 4), ("ragged", 4), ("short40", 1), ("short40", 3)],
    "halo": [("long3", 4), ("long3", 5), ("long3", 8), ("hist", 4), ("ragged", 4), ("short40", 1), ("short40", 3)],
    "flush": [("long3", 5), ("ragged", 4), ("short40", 1), ("short40", 3)],
    "pend": [("long3", 4), ("long3", 5), ("long3", 8), ("short40", 4), ("hist", 4), ("ragged", 4), ("short40", 1), ("short40", 3)],
}


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_mutants_of_the_transition_fail_the_shared_check(mutant):
    """queue1: the queue words start at 1 (a counter set nobody cleared) - the first chunk of every queue is never
    processed; carry: carry = ti > 0 - the forced entry of a chunk's first tile is missing; halo: the halo from registers at
    a transition - g differs at the tile's first 8 outputs; flush: st_flush ignored - tiles stored at another tile's address;
    pend: the pending row reset at a transition - its entries are lost.  Each is applied in the model and must fail
    check_outputs - the assertions of the GPU test - in every data set of every case listed for it."""
    rng = np.random.default_rng(35)
    for shape, ch in KILLS[mutant]:
        sc = K.sched_of(shape, ch)
        for k in range(K.N_SETS):
            c = K.data(shape, k)
            if mutant == "queue1":
                seqs = K.simulate(sc, rng, queue_init=1, check=False)
                out = K.kernel_outputs(c, sc, seqs)
            else:
                out = K.kernel_outputs(c, sc, K.simulate(sc, rng), mutant)
            with pytest.raises(AssertionError) as ei:
                K.check_outputs(c, sc, *out[:3])
            if k == 0:
                notes = {a: b for a, b in out[3].items() if b and a != "transitions"}
                print(f"{mutant} on {shape} chunk {ch}: {notes}; {str(ei.value)[len(c.name) + 2:][:90]}")


def test_batch_cases_fit_the_one_launch_tails_buckets():
    """The demod kernel lists the forced and flagged words of four consecutive streams in one bucket of the one-launch tail;
    a bucket that overflows sends the run through the separate kernels.  The batch cases stay below its capacity (restated:
    fix_bcap) at every chunk length, so their default runs are first-pass runs of k_tail; RD_TEST_FIX_BCAP=16 of the overflow
    child is below the load of long3's group in every data set.  real_grid: every stream position holds another stream in every data set."""
    for shape, ch in K.CASES:
        if shape in K.BATCH_SHAPES:
            sc = K.sched_of(shape, ch)
            loads = np.concatenate([K.bucket_loads(K.data(shape, k), sc) for k in range(K.N_SETS)])
            assert loads.max() <= K.fix_bcap(K.SHAPES[shape].n), (shape, ch, loads)
            assert shape != "long3" or loads.min() > 16, (shape, ch, loads)   # (the overflow child runs long3)
    sc = K.sched_of("long3", K.REAL_CHUNK)
    per = {}
    for k in range(K.N_SETS):
        w = K.expected_groups(K.data("long3", k), sc)
        for s in range(3):
            per[3 * k + s] = int(w[s].reshape(-1, 4).any(axis=1).sum())
    for k in range(K.N_SETS):
        src = K.real_grid_sources(k)
        loads = np.add.reduceat(np.array([per[j] for j in src]), np.arange(0, K.REAL_NS, 4))
        assert loads.max() <= K.fix_bcap(33 * K.BLOCK), (k, loads)
        assert all(a != b for a, b in zip(src, K.real_grid_sources((k + 1) % K.N_SETS)))
    print(f"real_grid: up to {loads.max()} entries per bucket of {K.fix_bcap(33 * K.BLOCK)}")


def test_one_tile_per_chunk_would_take_a_chunk_twice():
    """Why the launch code raises RD_K1_CHUNK=1 to 2 (found on the device by tests/test_k1_schedule.py): with one tile per
    chunk the equal-share walk takes chunk w + nwaves twice.  The stored words are the same, but every entry of those 32
    tiles is listed twice - the shared check refuses it, as it did on the device (41 words)."""
    sh = K.SHAPES["short40"]
    sc = K.Sched(sh.ns * 4, 4, 1, sh.ns * 4, 32, False)
    seqs = K.simulate(sc, np.random.default_rng(1), check=False)
    assert all(ids[1] == ids[2] == w + 32 and len(set(ids)) == len(ids) - 1 for w, ids in seqs.items())
    c = K.data("short40", 0)
    words, entries, g_bad, _ = K.kernel_outputs(c, sc, seqs)
    with pytest.raises(AssertionError, match="words listed twice"):
        K.check_outputs(c, sc, words, entries, g_bad)
    dup = entries.size - np.unique(entries >> 4).size
    assert dup >= 32
    print(f"one tile per chunk on short40: {dup} words listed twice, stored words unchanged")
