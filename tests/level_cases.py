"""Helpers shared by tests/test_level_cases_cpu.py and tests/test_wideband_levels.py (no tests in here): crafted capture
chunks for k_chan_levels (rd_chan_levels.hip), each aimed at one piece of its arithmetic - the carry-free zero-byte count,
the packed 16-bit maxima, the int8 bit flip, the int16 word whose squares sum to 2^31, the grid-stride loop beyond
RD_LV_MAX_SLICES workgroups - and the launch arithmetic restated.  The models are the suite's own: gain_cases.input_levels
and channel_levels, chan_bound_cf32.input_levels for float32.  Nothing here touches a device.

A chunk is a flat I,Q array of the format's dtype, read-only, 2 * decim * block_size components.  Vectors are the 16
bytes one lane loads: 16 components of uint8 / int8, 8 of int16, 4 of float32."""
import functools

import numpy as np

import chan_bound_cf32 as CC
import gain_cases as GC

FORMATS = ("u8", "s8", "s16", "cf32")
DTYPE = {"u8": np.uint8, "s8": np.int8, "s16": np.int16, "cf32": np.float32}
PAIR_BYTES = {"u8": 2, "s8": 2, "s16": 4, "cf32": 8}          # bytes per IQ pair
LV_THREADS, LV_MAX_SLICES, LV_VEC_PER_LANE = 256, 256, 8
F32 = np.float32
BELOW_ONE = np.nextafter(F32(1.0), F32(0.0))

# the edge alphabets: both ends of every range, their neighbours, the values about zero; float32: full scale and the
# value just under it, the clamp (+-8) and beyond it, NaN, the infinities, -0.0, a subnormal, the two ties of rint about
# one count (0.5 -> 0, 1.5 -> 2) and the ties about the top count (32766.5 -> 32766, 32767.5 -> 32768, clipped to 32767)
ALPHABET = {
    "u8": np.asarray([0, 1, 127, 128, 254, 255], np.uint8),
    "s8": np.asarray([-128, -127, -1, 0, 1, 126, 127], np.int8),
    "s16": np.asarray([-32768, -32767, -1, 0, 1, 32766, 32767], np.int16),
    "cf32": np.asarray([1.0, -1.0, BELOW_ONE, 8.0, -8.0, 9.0, -9.0, np.nan, np.inf, -np.inf, -0.0, 1e-40, 0.5 / 32768,
                        1.5 / 32768, (32767 - 0.5) / 32768, (32767 + 0.5) / 32768], np.float32),
}
QUIET = {"u8": 128, "s8": 0, "s16": 0, "cf32": 0.0}            # a = +1 for uint8, 0 for the others
LOW = {"u8": 0, "s8": -128, "s16": -32768, "cf32": -9.0}       # the negative end (float32: past the clamp, k = -32768)
HIGH = {"u8": 255, "s8": 127, "s16": 32767, "cf32": np.inf}    # the positive end (float32: k = 32767)

SMALL = (4, 128)                                               # (decim, block_size): 512 IQ pairs, one workgroup
# (decim, block_size) whose capture chunk takes 2 and 7 workgroups, per format
SLICED = {"u8": ((8, 2176), (8, 12416)), "s8": ((8, 2176), (8, 12416)), "s16": ((8, 1152), (8, 6272)),
          "cf32": ((8, 640), (8, 3200))}
# past the cap: float32, more than 256 * 2048 vectors (8.1 MiB), the only large chunk
BIG = ("cf32", 160, 6656)
BIG_FIRST_OF_NEXT_ROUND = LV_MAX_SLICES * LV_THREADS * LV_VEC_PER_LANE      # vector 524288


def vector_components(fmt):
    return 16 // np.dtype(DTYPE[fmt]).itemsize


def in_vectors(fmt, n_samples):
    assert (PAIR_BYTES[fmt] * n_samples) % 16 == 0
    return PAIR_BYTES[fmt] * n_samples // 16


def slices(fmt, n_samples):
    """rd_chan_stream_levels' launch arithmetic: the workgroups over the capture chunk, 8 vectors per lane up to the cap."""
    per = LV_THREADS * LV_VEC_PER_LANE
    return min(LV_MAX_SLICES, (in_vectors(fmt, n_samples) + per - 1) // per)


def passes(fmt, n_samples):
    """Rounds of the grid-stride loop the busiest lane makes."""
    stride = slices(fmt, n_samples) * LV_THREADS
    return (in_vectors(fmt, n_samples) + stride - 1) // stride


def want(raw, fmt):
    """(peak, clipped, power) of a chunk by the suite's models."""
    return CC.input_levels(raw) if fmt == "cf32" else GC.input_levels(raw, fmt)


def _done(raw):
    raw.setflags(write=False)
    return raw


def _full(fmt, n_samples, value):
    return np.full(2 * n_samples, value, DTYPE[fmt])


def _background(fmt, n_samples, seed):
    """Small values away from every edge: the sums are not trivial, the peak and the clip count come from what is planted."""
    rng = np.random.default_rng(seed)
    n = 2 * n_samples
    if fmt == "u8":
        return rng.integers(120, 136, n).astype(np.uint8)
    if fmt == "s8":
        return rng.integers(-8, 9, n).astype(np.int8)
    if fmt == "s16":
        return rng.integers(-100, 101, n).astype(np.int16)
    return (rng.integers(-100, 101, n) / 32768.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def small_cases(fmt):
    """name -> chunk on the smallest shape (SMALL), in a fixed order."""
    n_samples = SMALL[0] * SMALL[1]
    n, vc = 2 * n_samples, vector_components(fmt)
    out = {}
    for seed in (0, 1):                                        # drawn from the alphabet, every value present
        rng = np.random.default_rng(50 + seed + 10 * FORMATS.index(fmt))
        raw = ALPHABET[fmt][rng.integers(0, ALPHABET[fmt].size, n)]
        raw[rng.permutation(n)[: ALPHABET[fmt].size]] = ALPHABET[fmt]
        out[f"alphabet{seed}"] = raw
    out["all_min"], out["all_max"], out["all_quiet"] = (_full(fmt, n_samples, v) for v in (LOW[fmt], HIGH[fmt], QUIET[fmt]))
    # one extreme component in a quiet chunk, at every position of a vector (so every byte of it), first vector and last;
    # the negative end at even positions, the positive end at odd ones
    for where, base in (("first", 0), ("last", n - vc)):
        for p in range(vc):
            raw = _full(fmt, n_samples, QUIET[fmt])
            raw[base + p] = HIGH[fmt] if p & 1 else LOW[fmt]
            out[f"one_{where}_{p}"] = raw
    # the peak from the negative side alone
    raw = _background(fmt, n_samples, 7)
    if fmt == "u8":
        raw = np.minimum(raw, 127).astype(np.uint8)            # all <= 127
        raw[n // 3] = 3
    elif fmt == "s8":
        raw[n // 3] = -128
    else:
        i = 2 * (n_samples // 3)                               # I and Q of one sample: one 32-bit word of int16
        raw[i] = raw[i + 1] = LOW[fmt]
    out["negative_only"] = raw
    if fmt == "u8":
        raw = np.minimum(_background(fmt, n_samples, 8), 127).astype(np.uint8)
        raw[n - 1] = 0
        out["negative_only_zero"] = raw
    return {k: _done(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def sliced_case(fmt, which):
    """(decim, block_size, chunk): 2 (which = 0) or 7 (which = 1) workgroups over the capture, a small background and the
    only extremes in the last vector - its first component the negative end, its last the positive end."""
    decim, bs = SLICED[fmt][which]
    raw = _background(fmt, decim * bs, 20 + which)
    raw[-vector_components(fmt)] = LOW[fmt]
    raw[-1] = HIGH[fmt]
    return decim, bs, _done(raw)


@functools.lru_cache(maxsize=None)
def sliced_pair(fmt):
    """(decim, block_size, all-max chunk, all-quiet chunk) on the 7-workgroup shape."""
    decim, bs = SLICED[fmt][1]
    return decim, bs, _done(_full(fmt, decim * bs, HIGH[fmt])), _done(_full(fmt, decim * bs, QUIET[fmt]))


@functools.lru_cache(maxsize=None)
def big_case():
    """(fmt, decim, block_size, chunk) past the cap: the negative end at the first vector of the round after 256 * 2048
    vectors, a NaN and the positive end in the last vector, a small background."""
    fmt, decim, bs = BIG
    raw = _background(fmt, decim * bs, 30)
    raw[4 * BIG_FIRST_OF_NEXT_ROUND + 1] = LOW[fmt]
    raw[-3] = np.nan
    raw[-1] = HIGH[fmt]
    return fmt, decim, bs, _done(raw)
