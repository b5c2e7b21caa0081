"""The crafted captures of tests/level_cases.py reach what they claim (no device): the workgroup counts from the launch
arithmetic restated, every alphabet value present, the single extremes where they are said to be, the int16 word whose
squares sum to 2^31, the negative-only peaks, and the models' answers on the cases whose answer is plain."""
import numpy as np
import pytest

import level_cases as LC


def _bits(a):
    a = np.asarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def test_launch_arithmetic():
    for fmt in LC.FORMATS:
        n = LC.SMALL[0] * LC.SMALL[1]
        assert LC.slices(fmt, n) == 1 and LC.passes(fmt, n) == 1
        assert LC.in_vectors(fmt, n) == {"u8": 64, "s8": 64, "s16": 128, "cf32": 256}[fmt]
        for which, count in ((0, 2), (1, 7)):
            decim, bs, raw = LC.sliced_case(fmt, which)
            assert decim % 4 == 0 and decim <= 160 and bs % 128 == 0 and raw.size == 2 * decim * bs
            assert LC.slices(fmt, decim * bs) == count
            assert (count - 1) * 2048 < LC.in_vectors(fmt, decim * bs) <= count * 2048
    fmt, decim, bs, raw = LC.big_case()
    n = decim * bs
    assert decim % 4 == 0 and decim <= 160 and bs % 128 == 0
    assert LC.in_vectors(fmt, n) == 532480 > 256 * 2048 == LC.BIG_FIRST_OF_NEXT_ROUND and raw.nbytes > 8 << 20
    assert LC.slices(fmt, n) == 256 and LC.passes(fmt, n) == 9            # eight full rounds and a part of a ninth
    # the same rule as rd_chan_stream_levels, spelled the kernel's way: workgroup `slice` starts at vector slice * 256 + lane
    stride = LC.slices(fmt, n) * LC.LV_THREADS
    assert LC.BIG_FIRST_OF_NEXT_ROUND % stride == 0 and LC.BIG_FIRST_OF_NEXT_ROUND // stride == 8


@pytest.mark.parametrize("fmt", LC.FORMATS)
def test_small_cases_are_what_they_claim(fmt):
    cases = LC.small_cases(fmt)
    n = 2 * LC.SMALL[0] * LC.SMALL[1]
    vc = LC.vector_components(fmt)
    assert vc * np.dtype(LC.DTYPE[fmt]).itemsize == 16
    assert len(cases) == 5 + 2 * vc + (2 if fmt == "u8" else 1)
    for name, raw in cases.items():
        assert raw.dtype == LC.DTYPE[fmt] and raw.shape == (n,) and not raw.flags.writeable, name
    for seed in (0, 1):
        raw = cases[f"alphabet{seed}"]
        have = set(_bits(raw).tolist())
        assert have == set(_bits(LC.ALPHABET[fmt]).tolist())               # every value, and nothing else (bit patterns: NaN, -0.0)
    assert not np.array_equal(_bits(cases["alphabet0"]), _bits(cases["alphabet1"]))
    quiet = np.asarray(LC.QUIET[fmt], LC.DTYPE[fmt])
    for where, base in (("first", 0), ("last", n - vc)):
        for p in range(vc):
            raw = cases[f"one_{where}_{p}"]
            odd = np.flatnonzero(_bits(raw) != _bits(quiet))
            assert odd.tolist() == [base + p]
            assert _bits(raw[base + p: base + p + 1])[0] == _bits(np.asarray([LC.HIGH[fmt] if p & 1 else LC.LOW[fmt]], LC.DTYPE[fmt]))[0]
    # plain answers
    full = {"u8": 255, "s8": 128, "s16": 32768, "cf32": 32768}[fmt]
    top = {"u8": 255, "s8": 127, "s16": 32767, "cf32": 32767}[fmt]
    assert LC.want(cases["all_min"], fmt) == (full, n, n * full * full)
    assert LC.want(cases["all_max"], fmt) == (top, n, n * top * top)
    assert LC.want(cases["all_quiet"], fmt) == ((1, 0, n) if fmt == "u8" else (0, 0, 0))
    q = 1 if fmt == "u8" else 0
    assert LC.want(cases["one_last_0"], fmt) == (full, 1, full * full + (n - 1) * q)
    assert LC.want(cases["one_first_1"], fmt) == (top, 1, top * top + (n - 1) * q)
    # the peak comes from the negative side alone
    raw = cases["negative_only"]
    peak, clipped, _ = LC.want(raw, fmt)
    if fmt == "u8":
        assert raw.max() <= 127 and peak == 255 - 2 * 3 and clipped == 0
        zero = cases["negative_only_zero"]
        assert zero.max() <= 127 and LC.want(zero, fmt)[:2] == (255, 1) and int(zero[-1]) == 0
    elif fmt == "s8":
        assert raw.max() < 100 and peak == 128 and clipped == 1
    else:
        assert peak == 32768 and clipped == 2
        pairs = np.asarray(raw).reshape(-1, 2)
        k = np.asarray([LC.want(np.asarray([v, 0], raw.dtype), fmt)[0] for v in pairs[len(pairs) // 3]], np.int64)
        assert int((k * k).sum()) == 2 ** 31                               # one 32-bit word: m0 m0 + m1 m1 = 2^31
        assert (len(pairs) // 3 * 2 * raw.dtype.itemsize) % 4 == 0


def test_float_alphabet_meets_every_branch():
    """What each float32 value is for, by the model: the ties of rint, the clamp, the top count clipped, NaN counted."""
    a = LC.ALPHABET["cf32"]
    k = {i: LC.want(np.asarray([a[i], 0.0], np.float32), "cf32") for i in range(a.size)}
    peaks = [k[i][0] for i in range(a.size)]
    clipped = [k[i][1] for i in range(a.size)]
    #        1.0    -1.0   <1     8      -8     9      -9     NaN inf    -inf   -0 sub 0.5 1.5 32766.5 32767.5
    assert peaks == [32767, 32768, 32767, 32767, 32768, 32767, 32768, 0, 32767, 32768, 0, 0, 0, 2, 32766, 32767]
    assert clipped == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1]
    assert float(LC.BELOW_ONE) * 32768.0 == 32767.998046875                # rounds to 32768 and is clipped to 32767


@pytest.mark.parametrize("fmt", LC.FORMATS)
def test_sliced_and_paired_cases(fmt):
    vc = LC.vector_components(fmt)
    full = {"u8": 255, "s8": 128, "s16": 32768, "cf32": 32768}[fmt]
    for which in (0, 1):
        _, _, raw = LC.sliced_case(fmt, which)
        peak, clipped, _ = LC.want(raw, fmt)
        assert (peak, clipped) == (full, 2)
        assert LC.want(raw[:-vc], fmt)[0] < 300 and LC.want(raw[:-vc], fmt)[1] == 0     # nothing before the last vector
    decim, bs, loud, quiet = LC.sliced_pair(fmt)
    assert (decim, bs) == LC.SLICED[fmt][1] and loud.size == quiet.size == 2 * decim * bs
    assert LC.want(loud, fmt)[1] == loud.size and LC.want(quiet, fmt)[1] == 0


def test_big_case():
    fmt, decim, bs, raw = LC.big_case()
    v = np.asarray(raw).reshape(-1, 4)
    assert v.shape[0] == LC.in_vectors(fmt, decim * bs)
    edge = np.flatnonzero((np.abs(v) > 0.01).any(axis=1) | np.isnan(v).any(axis=1))
    assert edge.tolist() == [LC.BIG_FIRST_OF_NEXT_ROUND, v.shape[0] - 1]
    peak, clipped, power = LC.want(raw, fmt)
    assert (peak, clipped) == (32768, 3)
    rest = np.delete(v, edge, axis=0).reshape(-1)
    planted = 32768 ** 2 + 32767 ** 2                                      # (the NaN is the value 0)
    assert planted <= power - LC.want(rest, fmt)[2] <= planted + 6 * 100 ** 2
