"""The planted near-tie cases of tests/near_tie_cases.py, judged on the CPU alone: the exact reference against the oracle,
the fp32 flag model against rational arithmetic, the coverage the GPU tests (tests/test_gpu_near_ties.py) rely on, and
four mutants of the kernel's list logic that the shared list check must refuse on these very cases."""
import ctypes as C
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import near_tie_cases as NT  # noqa: E402
from oracle import dsp_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = NT.TILE


def wrong_samples(c):
    """[ns, n] bool: the modelled fast sign differs from the exact one (where the model speaks)"""
    return (c.fast != c.bits) & np.repeat(c.valid, 8, axis=1)


def word_rank(c):
    """[ns, words]: rank of a word among its tile's model-flagged words, lane order (-1: not flagged)"""
    fw = c.flagged_words()
    ns, words = fw.shape
    rank = -np.ones((ns, words), dtype=np.int64)
    for ti in range((words + 63) // 64):
        seg = fw[:, 64 * ti: 64 * ti + 64]
        rank[:, 64 * ti: 64 * ti + 64] = np.where(seg, np.cumsum(seg, axis=1) - 1, -1)
    return rank


@pytest.mark.parametrize("name", NT.NAMES)
def test_exact_reference_is_the_oracles_and_has_no_zero(name):
    c = NT.case(name)
    assert c.zeros == 0
    for s in range(c.streams.shape[0]):
        if c.hist is None:
            ob = O.demod_stream_oneshot(c.streams[s])[2]
        else:
            ob = O.demod_stream_oneshot(np.concatenate([c.hist[s], c.streams[s]]))[2][c.hist.shape[1] // 2:]
        assert np.array_equal(ob, c.bits[s]), f"{name} stream {s}"
    # the planted numerators are far above float64 rounding, relative to the products they are the difference of
    G = [NT.exact_G(c.streams[s], None if c.hist is None else c.hist[s]) for s in range(c.streams.shape[0])]
    for p in c.plants:
        Gr, Gi = G[p.s]
        N = NT.exact_N_int(Gr, Gi, p.t)
        F2 = max(abs(int(Gr[p.t])), abs(int(Gi[p.t])), abs(int(Gr[p.t + 1])), abs(int(Gi[p.t + 1]))) ** 2
        assert N != 0 and abs(N) >= 1e-10 * F2, (name, p, N / F2)


@pytest.mark.parametrize("name", NT.NAMES)
def test_model_is_bit_exact_where_it_decides(name):
    """Every lane whose guard value is within reach of a threshold (nm <= C0_MAX), and a sample of the others, through
    rational arithmetic with one rounding per fp32 operation; c0(F) <= C0_MAX for every F met, so the kernel's first step
    (the constant threshold) never changes an outcome; no lane sits within the margin of its threshold."""
    c = NT.case(name)
    lm = c.lane
    assert (lm.thr <= NT.C0_MAX).all() and lm.F.max() < 138.9
    assert NT.margin_ok(c)
    near = np.argwhere(lm.nm <= NT.C0_MAX)
    rng = np.random.default_rng(5)
    far = np.argwhere(lm.nm > NT.C0_MAX)
    far = far[rng.permutation(far.shape[0])[:200]]
    if near.shape[0] > 1500:
        near = near[rng.permutation(near.shape[0])[:1500]]
    for s, l in np.concatenate([near, far]):
        if c.hist is None and l < 8:
            continue
        want = NT.lane_nm_fraction(c.g32[s, 4 * l: 4 * l + 5])
        assert np.float32(want) == lm.nm[s, l], (name, s, l, want, lm.nm[s, l])


def test_round_f32_helper():
    rng = np.random.default_rng(6)
    for v in rng.standard_normal(200) * 10.0 ** rng.integers(-20, 20, 200):
        assert NT.round_f32(Fraction(float(v))) == float(np.float32(v))
    one = Fraction(1)
    assert NT.round_f32(one + Fraction(1, 2 ** 24)) == 1.0                       # tie -> even
    assert NT.round_f32(one + Fraction(3, 2 ** 24)) == 1.0 + 2.0 ** -22          # tie -> even, upwards
    assert NT.round_f32(one + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)) == 1.0 + 2.0 ** -23


def test_fma32_rounds_once():
    # x y + z with a sum that float64 would round first: 1 + 2^-24 + 2^-60 -> must round UP in fp32
    x = np.array([1.0 + 2.0 ** -12], dtype=np.float32)
    y = np.array([1.0 + 2.0 ** -12], dtype=np.float32)       # x y = 1 + 2^-11 + 2^-24
    z = np.array([2.0 ** -70], dtype=np.float32)
    assert NT.fma32(x, y, z)[0] == np.float32(1.0 + 2.0 ** -11 + 2.0 ** -23)
    assert NT.fma32(x, y, -z)[0] == np.float32(1.0 + 2.0 ** -11)
    rng = np.random.default_rng(7)
    a, b, cc = (rng.standard_normal(300).astype(np.float32) for _ in range(3))
    got = NT.fma32(a, b, cc)
    for i in range(300):
        assert got[i] == np.float32(NT.round_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(cc[i]))))


@pytest.mark.parametrize("amp", list(NT.AMPS))
def test_positions_cover_every_lane_route(amp):
    c = NT.case(f"positions_{amp}")
    assert c.n % TILE != 0 and c.n % 32 != 0, "the last tile is ragged, the last word partial"
    flagged_at, trusted_at = set(), set()
    carry = {(par, kind): set() for par in (0, 1) for kind in ("f", "t")}
    ragged = 0
    for p in c.plants:
        lane_f = bool(c.lane.lane_flag[p.s, p.t // 4])
        grp_f = bool(c.flagged[p.s, p.t // 8])
        just_out = p.kind in ("out1.5", "out3") and not grp_f and c.lane.nm[p.s, p.t // 4] <= 4 * c.lane.thr[p.s, p.t // 4]
        if lane_f:
            flagged_at.add(p.t % 64)
        if just_out:
            trusted_at.add(p.t % 64)
        if p.t % TILE < 4 and p.t >= TILE:
            if lane_f:
                carry[((p.t // TILE) & 1, "f")].add(p.t % TILE)
            if just_out:
                carry[((p.t // TILE) & 1, "t")].add(p.t % TILE)
        ragged += p.t >= (c.n // TILE) * TILE
    assert flagged_at == set(range(64)) and trusted_at == set(range(64))
    for k, v in carry.items():
        assert v == {0, 1, 2, 3}, (k, v)
    assert ragged >= 24
    print(f"positions_{amp}: {len(c.plants)} plants, {int(c.flagged.sum())} flagged groups, "
          f"{int(wrong_samples(c).sum())} wrong fast signs, {ragged} plants on the ragged tile")


def test_with_history_plants_in_the_first_word():
    c = NT.case("with_history")
    assert c.hist is not None and c.hist.shape[1] == 64
    assert any(p.t < 32 and c.flagged[p.s, p.t // 8] for p in c.plants)
    assert c.valid.all()


def test_wrong_fast_signs_are_many_and_everywhere():
    total, classes, deep_rank = 0, set(), 0
    for c in NT.cases():
        w = wrong_samples(c)
        total += int(w.sum())
        for s, t in np.argwhere(w):
            classes.add(((t % 64) // 8, (t % 8) // 4))
        assert not (w & ~np.repeat(c.flagged, 8, axis=1)).any(), "a wrong fast sign outside the model's band: the bound of rd_mfma.h"
        if c.name.startswith("dense_"):
            rank = word_rank(c)
            deep_rank += int((w.reshape(w.shape[0], -1, 32).any(axis=-1) & (rank >= 32)).sum())
    print(f"wrong fast signs: {total} samples, {len(classes)} of 16 (block, half) classes, {deep_rank} dense words of rank >= 32")
    assert total >= 64
    assert classes == {(b, h) for b in range(8) for h in range(2)}
    assert deep_rank >= 8


def test_dense_tiles_are_dense():
    for name in ("dense_full", "dense_low"):
        c = NT.case(name)
        assert c.streams.shape == (8, 2 * 4 * TILE)
        per_tile = c.flagged_words().reshape(8, 4, 64).sum(axis=-1)
        print(f"{name}: flagged words per tile min {per_tile.min()} max {per_tile.max()}, tiles with 64: {(per_tile == 64).sum()} of 32")
        assert per_tile.min() >= 33 and (per_tile == 64).sum() > 16
    c = NT.case("dense_partial")
    assert np.array_equal(c.flagged_words().reshape(2, 5, 64).sum(axis=-1), np.array(NT.PARTIAL_COUNTS))
    assert sorted(NT.PARTIAL_COUNTS[0][1:]) == [31, 32, 33, 64]


def test_launch_sizes():
    for c in NT.cases():
        tiles = (c.n + TILE - 1) // TILE
        assert c.streams.shape[0] <= 8 and tiles <= 8 and c.streams.shape[1] % 16 == 0
        assert c.streams.min() >= 0 and c.streams.dtype == np.uint8
    for amp, (lo, hi) in NT.AMPS.items():
        c = NT.case(f"positions_{amp}")
        assert c.streams.min() >= lo and c.streams.max() <= hi


# ---------------------------------------------------------------------------------------------------------------------
# mutants: each is a kernel that is subtly wrong in its list logic; the check the GPU tests apply must refuse it
def _ideal(c, flagged=None):
    ents = [e for tile in NT.model_entries(c, flagged) for e in tile]
    words = (c.n + 31) // 32
    return NT.listed_groups(ents, c.streams.shape[0], words)


def _refused(mutant) -> list:
    names = []
    for c in NT.cases():
        listed, dup = mutant(c)
        try:
            NT.check_list(c, listed, c.fast, dup)
        except AssertionError:
            names.append(c.name)
    return names


def test_the_model_itself_passes_the_list_check():
    for c in NT.cases():
        listed, dup = _ideal(c)
        NT.check_list(c, listed, c.fast, dup)


def _pad4(f):
    ns, ng = f.shape
    out = np.zeros((ns, (ng + 3) // 4 * 4), dtype=bool)
    out[:, :ng] = f
    return out


def test_mutants_are_refused():
    def no_t1_term(c):
        return _ideal(c, NT._evaluate(c, drop_t1=True))

    def f_from_own_outputs(c):
        return _ideal(c, NT._evaluate(c, f_own_only=True))

    def byte_to_next_bit(c):
        f = _pad4(c.flagged).reshape(c.flagged.shape[0], -1, 4)
        g = np.zeros_like(f)
        g[:, :, 1:] = f[:, :, :-1]
        return g.reshape(f.shape[0], -1), 0

    def byte_to_previous_bit(c):
        f = _pad4(c.flagged).reshape(c.flagged.shape[0], -1, 4)
        g = np.zeros_like(f)
        g[:, :, :-1] = f[:, :, 1:]
        return g.reshape(f.shape[0], -1), 0

    def rank_32_and_up_lost(c):
        ents = [e for tile in NT.model_entries(c) for e in tile[:32]]
        return NT.listed_groups(ents, c.streams.shape[0], (c.n + 31) // 32)

    for m in (no_t1_term, f_from_own_outputs, byte_to_next_bit, byte_to_previous_bit, rank_32_and_up_lost):
        r = _refused(m)
        print(f"{m.__name__}: refused on {r}")
        assert r, f"mutant {m.__name__} passes the list check on every case"
    # the overrun in particular must show as WRONG SIGNS, not only as missing entries: drop the ranks, look at signs alone
    hits = 0
    for name in ("dense_full", "dense_low", "dense_partial"):
        c = NT.case(name)
        listed, _ = rank_32_and_up_lost(c)
        hits += int(((c.fast != c.bits) & ~np.repeat(listed[:, : c.flagged.shape[1]], 8, axis=1) & np.repeat(c.valid, 8, axis=1)).sum())
    assert hits >= 8


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hh():
    so = os.path.join(ROOT, "tests", "_build", "libhostharness.so")
    src = os.path.join(ROOT, "tests", "host_harness.cpp")
    hdr = os.path.join(ROOT, "rtldavis_amd", "csrc", "rd_math.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-march=x86-64-v3", "-shared", "-fPIC", "-o", so, src])
    L = C.CDLL(so)
    L.hh_exact_bit_f64.restype = C.c_uint32
    L.hh_exact_bit_f64.argtypes = [C.c_double] * 4
    return L


def _ref_bit(nx, ny, px, py):
    num = ny * px - nx * py          # Python integers
    if num != 0:
        return int(num < 0)
    return int(nx == 0 and ny == 0 and px < 0 and py > 0)


def test_exact_bit_f64_int128_branch(hh):
    """rd_exact_bit_f64 where float64 cannot decide: the largest FIR outputs (|F| ~ 6.4e14) with p1 - p2 in
    {0, +-1, +-2, +-2^40} - the __int128 branch with a non-zero numerator - and the zero-history rule."""
    big = 638 * sum(NT.C12[m if m <= 4 else 8 - m] for m in range(9))
    assert 6.3e14 < big < 6.5e14
    seen = set()
    for delta in (0, 1, -1, 2, -2, 2 ** 40, -2 ** 40):
        for a in (big - 2 ** 41, big - 2 ** 41 - 12345, big // 3):
            b = a + delta - 1
            # ny px - nx py = a b - (a - 1)(b + 1) = b - a + 1 = delta
            for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
                nx, ny, px, py = sx * (a - 1), sy * a, sy * b, sx * (b + 1)
                assert max(abs(v) for v in (nx, ny, px, py)) <= big
                assert ny * px - nx * py == delta
                assert float(nx) == nx and float(px) == px
                assert abs(float(ny) * float(px) - float(nx) * float(py)) <= 2.0 ** -51 * 2 * float(a) * float(b), "float64 must be undecided"
                assert hh.hh_exact_bit_f64(nx, ny, px, py) == _ref_bit(nx, ny, px, py), (delta, a, sx, sy)
                seen.add((delta, _ref_bit(nx, ny, px, py)))
    assert {(d, int(d < 0)) for d in (1, -1, 2, -2, 2 ** 40, -2 ** 40)} <= seen
    # decided by float64 (sanity), then the zero-history rule: n = 0 gives 1 exactly for Re np < 0 < Im np
    assert hh.hh_exact_bit_f64(3, big, big, -5) == _ref_bit(3, big, big, -5) == 0
    assert hh.hh_exact_bit_f64(3, -big, big, -5) == 1
    for px in (-big, -1, 0, 1, big):
        for py in (-big, -1, 0, 1, big):
            assert hh.hh_exact_bit_f64(0, 0, px, py) == int(px < 0 and py > 0), (px, py)
    # an exact zero with n != 0: +0.0
    assert hh.hh_exact_bit_f64(2, 4, 3, 6) == 0 and hh.hh_exact_bit_f64(-2, -4, 3, 6) == 0
