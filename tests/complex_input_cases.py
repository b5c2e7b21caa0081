"""Inputs and expected values for the complex-input branch of ``Demodulator`` (tests/test_complex_input_cpu.py checks
the cases themselves, tests/test_complex_input.py runs them on the device).  No tests here.

Expected values: ``oracle.dsp_oracle.OracleDemodulator`` block by block, which takes complex blocks and any config.

SHAPES is the only place where it is written down which shape takes which kernels.  The rule it restates
(``takes_one_launch``) is rd_stream.hip's ``one_ok`` / ``one_cplx`` and ``rd_launch_stream_block_cplx``'s own check:

* one launch (``k_stream_block_cplx``): the Davis search (14 samples per symbol, 16-symbol preamble 1100101110001001,
  80 symbols), buffer_length == 2 * block_size, block_size a multiple of 32 in [2048, 8192], RD_STREAM_IMPL not
  "legacy";
* everything else: the multi-launch form (``roll_cplx``, ``k_cplx_bits``, ``k_window_update``, ``k_search``,
  ``k_slice_rssi<complex ring>``, the ``k_disc`` / ``k_filt`` mirrors).

Input classes (``CLASSES_DAVIS``; the non-Davis shapes take ``float`` and ``pyrtlsdr``):

* ``pyrtlsdr``   synth_bursts' bytes through ``b / 127.5`` then ``- (1 + 1j)``, pyrtlsdr's own arithmetic
* ``float``      the same modulation and noise without the byte quantisation, amplitude 0.5, noise 0.05
* ``x2^-20`` ``x2^13`` ``x2^-17`` ``x1e-5`` ``x32768``   ``float`` times that factor (2^-17 is here because amplitude 0.5 times
                 2^-20 puts |f|^2 at 2.3e-13, a factor 440 under the discriminator's 1e-10; 2^-17 and 1e-5 lie within 100)
* ``c64`` ``c64s``   ``float`` as complex64, contiguous and as every second element of a longer array
* ``edges``      ``float`` with one preamble at window index 0 (noise power = the constant 1e-9) and one whose signal
                 window is clipped at block_size + 1
* ``raise0`` ``raise1``   the block of the report all zeros, the preamble so early that the noise window holds the filter's
                 transient: signal power 0 over noise > 0, ValueError("math domain error") out of that call
* ``fall0`` ``fall1``     the same with the preamble later: both windows zero, a record with exactly (-120.0, 50.0)
* ``runs``       zero runs of 1, 8, 9, 17 and 40 samples inside the first burst and inside noise; one crosses a block
                 boundary, one sample 2048 of a block (where there is one)
* ``runs-0``     the same runs made of -0.0 (both components)
* ``zero-first`` an all-zero first block
* ``zero-gap``   an all-zero block between two bursts
"""
from __future__ import annotations

import functools
import math
import os
import sys
from typing import List, NamedTuple, Optional

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import dsp_oracle as O  # noqa: E402
from rtldavis_amd import synth  # noqa: E402

DAVIS_PRE = "1100101110001001"
PIECE = 2048   # samples one workgroup of k_stream_block_cplx takes (8 * RD_SBC_THREADS)
TAPS = O.FIR9_COEFFS


class Shape(NamedTuple):
    name: str
    S: int
    P: int
    K: int
    B: int
    form: str        # "one" or "multi": what the table claims; takes_one_launch() is the rule
    legacy: bool     # RD_STREAM_IMPL=legacy set before the handle's first block
    nb: int          # blocks per stream

    @property
    def davis(self) -> bool:
        return (self.S, self.P, self.K) == (14, 16, 80)

    @property
    def preamble(self) -> str:
        if self.davis:
            return DAVIS_PRE
        rng = np.random.default_rng(1000 * self.S + self.P)   # test_random_configs_against_c_oracle's preambles
        return "".join(str(int(b)) for b in rng.integers(0, 2, size=self.P))

    def ocfg(self) -> O.OracleConfig:
        return O.OracleConfig(19200, self.S, self.P, self.K, self.preamble, self.B)

    def cfg_args(self):
        return (19200, self.S, self.P, self.K, self.preamble, self.B)


SHAPES = (
    Shape("davis-2048", 14, 16, 80, 2048, "one", False, 4),        # one piece
    Shape("davis-2144", 14, 16, 80, 2144, "one", False, 4),        # ragged second piece
    Shape("davis-8192", 14, 16, 80, 8192, "one", False, 4),        # four pieces, the product's block size
    Shape("davis-512", 14, 16, 80, 512, "multi", False, 12),       # the reference's default block size (L = 4 B)
    Shape("davis-1024", 14, 16, 80, 1024, "multi", False, 7),      # L = 3 B
    Shape("davis-16384", 14, 16, 80, 16384, "multi", False, 4),    # the uint8 one-launch form accepts it, the complex one declines
    Shape("s8-1024", 8, 16, 80, 1024, "multi", False, 4),
    Shape("s4-64", 4, 4, 12, 64, "multi", False, 8),
    Shape("s3-96", 3, 6, 200, 96, "multi", False, 24),
    Shape("davis-8192-legacy", 14, 16, 80, 8192, "multi", True, 4),
)
SHAPE = {s.name: s for s in SHAPES}

SCALES = {"x2^-20": 2.0 ** -20, "x2^13": 2.0 ** 13, "x2^-17": 2.0 ** -17, "x1e-5": 1e-5, "x32768": 32768.0}
TWINS = {"x2^-20": -20, "x2^13": 13, "x2^-17": -17, "x32768": 15}     # class -> k of 2^k
NEAR_EPSILON = ("x2^-17", "x1e-5")
CLASSES_ANY = ("pyrtlsdr", "float")
CLASSES_DAVIS = CLASSES_ANY + tuple(SCALES) + ("c64", "c64s", "edges", "raise0", "raise1", "fall0", "fall1",
                                               "runs", "runs-0", "zero-first", "zero-gap")
RUN_LENGTHS = (1, 8, 9, 17, 40)


def takes_one_launch(S: int, P: int, K: int, preamble: str, B: int, legacy: bool) -> bool:
    """rd_stream.hip one_ok and one_cplx (single stream, complex input) and rd_launch_stream_block_cplx's check."""
    L = (K * S // B + 2) * B
    davis = (S, P, K, preamble) == (14, 16, 80, DAVIS_PRE)
    return (not legacy) and B % 8 == 0 and davis and L == 2 * B and B % 32 == 0 and 2048 <= B <= 8192


def classes_of(shape: Shape):
    return CLASSES_DAVIS if shape.davis else CLASSES_ANY


# ------------------------------------------------------------------------------------------------ synthesis
def packet_bytes(shape: Shape, k: int) -> bytes:
    """On-air bytes of burst k: an OTA packet on the Davis shapes; elsewhere the shape's preamble followed by the OTA
    packet's bits behind its sync word (repeated to length), whole bytes."""
    ota = bytes.fromhex(synth.OTA_PACKETS[(k + shape.B) % len(synth.OTA_PACKETS)])
    if shape.davis:
        return ota
    bits = np.concatenate([np.array([int(c) for c in shape.preamble], dtype=np.uint8), np.tile(np.unpackbits(np.frombuffer(ota[2:], np.uint8)), 4)])
    return np.packbits(bits[: 8 * ((shape.K + 7) // 8)]).tobytes()


def lead_in(shape: Shape) -> int:
    return 32 * shape.S   # samples of alternating symbols in front of a burst's packet (synth_bursts)


def burst_len(shape: Shape) -> int:
    return (32 + 8 * len(packet_bytes(shape, 0)) + 8) * shape.S


def synth_float(bursts, n_samples: int, seed: int, symbol_length: int, amplitude: float = 0.5, noise: float = 0.05) -> np.ndarray:
    """``synth.synth_bursts`` without its last step: the same bursts, phase and noise draws, as complex128."""
    sample_rate = 19200 * symbol_length
    rng = np.random.default_rng(seed)
    freq = np.full(n_samples, -sample_rate / 4.0)
    on = np.zeros(n_samples)
    for ota, start, cfo in reversed(list(bursts)):
        sym = np.concatenate([np.tile(np.array([1, 0], dtype=np.uint8), 16), np.unpackbits(np.frombuffer(bytes(ota), dtype=np.uint8)),
                              np.zeros(8, dtype=np.uint8)])
        chips = np.repeat(sym, symbol_length)
        start = int(start)
        if start < 0 or start + chips.size > n_samples:
            raise ValueError("synth_float: a burst does not fit the stream")
        on[start:start + chips.size] = 1.0
        freq[start:start + chips.size] = -sample_rate / 4.0 + float(cfo) + np.where(chips == 1, 4800.0, -4800.0)
    phase = np.cumsum(freq) * (2.0 * np.pi / sample_rate)
    x = amplitude * on * np.exp(1j * phase)
    return x + noise * (rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples))


def pyrtlsdr_convert(raw: np.ndarray) -> np.ndarray:
    """pyrtlsdr's packed_bytes_to_iq: bytes to float64, pairs viewed as complex128, ``/= 127.5``, ``-= (1 + 1j)``."""
    iq = raw.astype(np.float64).view(np.complex128)
    iq /= 127.5
    iq -= (1 + 1j)
    return iq


def report_delay(shape: Shape) -> int:
    """Blocks between the block a preamble starts in and the call that reports it (window index <= B)."""
    return shape.ocfg().buffer_length // shape.B - 1


def _seed(shape: Shape, cls: str) -> int:
    return 7000 + 97 * SHAPES.index(shape) + 7 * CLASSES_DAVIS.index(cls)


def default_starts(shape: Shape):
    """Two bursts: the first from block 1 on (block 0 on the small shapes), the second behind it, both reported before the
    stream ends."""
    B, bl = shape.B, burst_len(shape)
    if B >= bl + 400:
        return (B + 300, 2 * B + 100)
    first = 3 * shape.S + 20
    return (first, first + bl + 5 * shape.S + 3)


def _bursts(shape: Shape, starts):
    cfos = (350.0, -900.0)
    return [(packet_bytes(shape, k), s, cfos[k % 2]) for k, s in enumerate(starts)]


@functools.lru_cache(maxsize=None)
def _align(shape: Shape) -> int:
    """Samples by which the reported window index lags the preamble's first sample (filter and discriminator delay),
    measured with the oracle on a clean burst."""
    B, n = shape.B, shape.B * shape.nb
    start = default_starts(shape)[0]
    x = synth_float(_bursts(shape, [start]), n, 1, shape.S, noise=0.0)
    dem = O.OracleDemodulator(shape.ocfg())
    want = packet_bytes(shape, 0)[: (shape.K + 7) // 8]
    for b in range(shape.nb):
        dem.demodulate(x[b * B:(b + 1) * B])
        # every adjacent sample position that slices the same packet; the middle one is the least sensitive to noise
        hits = sorted(q for q in O.search(dem.quantized, dem.cfg) if q <= B and _same_packet(O.slice_bytes(dem.quantized, q, dem.cfg), want, shape.K))
        if hits:
            base = (b + 1) * B - dem.cfg.buffer_length
            return base + hits[len(hits) // 2] - (start + lead_in(shape))
    raise AssertionError("the clean burst was not reported")


def _same_packet(got: bytes, want: bytes, K: int) -> bool:
    """_slice packs K symbols MSB first into whole bytes, the last byte right-aligned when K % 8 != 0."""
    bits = np.unpackbits(np.frombuffer(want, np.uint8))[:K]
    return O.slice_bytes(bits, 0, O.OracleConfig(19200, 1, 1, K, "1", 8)) == got


def _start_for(shape: Shape, block: int, q: int) -> int:
    """Burst start that puts the preamble at window index q of the call reporting block `block`'s preambles."""
    return block * shape.B + q - _align(shape) - lead_in(shape)


def _zero_runs(shape: Shape, starts):
    """[(first sample, length)]: RUN_LENGTHS inside the first burst's packet, then inside noise; the 17-run of the noise
    set crosses a block boundary, the 40-run sample PIECE of a block where a block has one."""
    B = shape.B
    p0 = starts[0] + lead_in(shape) + 16 * shape.S      # behind the preamble
    runs = [(p0 + 150 * k + 3, n) for k, n in enumerate(RUN_LENGTHS)]
    end = starts[-1] + burst_len(shape)                 # behind the last burst
    boundary = ((end + 200) // B + 1) * B
    noise = [(end + 20, 1), (end + 60, 8), (end + 120, 9), (boundary - 8, 17)]
    noise.append((3 * B + PIECE - 20, 40) if B > PIECE else (boundary + 60, 40))
    return runs + noise


@functools.lru_cache(maxsize=None)
def stream(shape_name: str, cls: str):
    """(blocks, meta): the case's blocks as the caller passes them (complex128 [B], or complex64 for c64 / c64s, c64s a
    strided view), and a dict of what the case was built from."""
    shape = SHAPE[shape_name]
    B, n = shape.B, shape.B * shape.nb
    meta = {}
    if cls in SCALES or cls in ("c64", "c64s"):
        base, meta = stream(shape_name, "float")
        x = np.concatenate(base)
        if cls in SCALES:
            x = x * SCALES[cls]
        elif cls == "c64":
            x = x.astype(np.complex64)
        else:
            wide = np.zeros(2 * n, dtype=np.complex64)
            wide[1::2] = 1e30   # (what a contiguous read would pick up)
            wide[0::2] = x.astype(np.complex64)
            x = wide[0::2]
        return _blocks(x, B), dict(meta)
    seed = _seed(shape, cls)
    starts = default_starts(shape)
    zero_blocks, runs, neg = [], [], False
    rb = report_delay(shape)
    if cls == "edges":
        starts = (_start_for(shape, 1, 0), _start_for(shape, 1 + max(1, -(-burst_len(shape) // B)), B - 100))
    elif cls in ("raise0", "raise1", "fall0", "fall1"):
        q = {"raise0": 13, "raise1": 154, "fall0": 300, "fall1": 400}[cls]
        k = 1 if B >= 2048 else -(-(lead_in(shape) + 5) // B)
        starts = (_start_for(shape, k, q),)
        zero_blocks = [k + rb]
        meta["report_call"] = k + rb
    elif cls in ("runs", "runs-0"):
        runs, neg = _zero_runs(shape, starts), cls == "runs-0"
    elif cls == "zero-first":
        zero_blocks = [0]
    elif cls == "zero-gap":
        s0 = 3 * shape.S + 20
        gap = (s0 + burst_len(shape)) // B + 1
        starts = (s0, (gap + 1) * B + 100)
        zero_blocks = [gap]
    if cls == "pyrtlsdr":
        x = pyrtlsdr_convert(synth.synth_bursts(_bursts(shape, starts), n, seed, symbol_length=shape.S))
    else:
        x = synth_float(_bursts(shape, starts), n, seed, shape.S)
    for b in zero_blocks:
        x[b * B:(b + 1) * B] = 0.0
    z = complex(-0.0, -0.0) if neg else 0.0
    for s, ln in runs:
        x[s:s + ln] = z
    meta.update(starts=starts, zero_blocks=zero_blocks, runs=runs, seed=seed)
    return _blocks(x, B), meta


def _blocks(x: np.ndarray, B: int):
    out = [x[b * B:(b + 1) * B] for b in range(x.size // B)]
    for blk in out:
        blk.flags.writeable = False
    return tuple(out)


def widened(blocks) -> np.ndarray:
    """The whole stream as complex128 (exact for complex64)."""
    return np.concatenate([np.asarray(b, dtype=np.complex128) for b in blocks])


# ------------------------------------------------------------------------------------------------ expected values
class Call(NamedTuple):
    packets: Optional[list]      # [(index, hex, rssi, snr)], None where the call raises ValueError("math domain error")
    quantized: np.ndarray        # after the call
    filtered: np.ndarray
    discriminated: np.ndarray
    fbound: np.ndarray           # per element of filtered: sum_m |c_m| |y_m| per component (max of the two)


def _abs_tap_sum(v: np.ndarray, n_out: int) -> np.ndarray:
    return np.convolve(np.abs(v), np.abs(TAPS), mode="valid")[:n_out]


def oracle_calls(ocfg: O.OracleConfig, blocks) -> List[Call]:
    """OracleDemodulator over the blocks (uint8 [2B] or complex); the state after every call, the raise as None."""
    dem = O.OracleDemodulator(ocfg)
    out = []
    fb = np.zeros(ocfg.block_size + 1)
    for blk in blocks:
        try:
            pk = [(int(p.index), bytes(p.data).hex(), float(p.rssi), float(p.snr)) for p in dem.demodulate(np.asarray(blk))]
        except ValueError as e:
            assert str(e) == "math domain error", e
            pk = None
        fb = np.concatenate([fb[-1:], np.maximum(_abs_tap_sum(dem.iq.real, ocfg.block_size), _abs_tap_sum(dem.iq.imag, ocfg.block_size))])
        out.append(Call(pk, dem.quantized.copy(), dem.filtered.copy(), dem.discriminated.copy(), fb))
    return out


@functools.lru_cache(maxsize=None)
def expected(shape_name: str, cls: str) -> tuple:
    blocks, _ = stream(shape_name, cls)
    return tuple(oracle_calls(SHAPE[shape_name].ocfg(), blocks))


FILT_ULPS = 18 * 2.0 ** -53
DB_TOL = 1e-3


class Errors:
    """Largest errors seen by ``compare`` (records for profiles/complex_input.txt, not thresholds)."""

    def __init__(self):
        self.db = 0.0
        self.filt = 0.0     # in units of the bound
        self.disc = 0.0     # in units of max(1, |ref|)


def compare(got: List[Call], want: List[Call], err: Optional[Errors] = None) -> List[str]:
    """What differs between two runs of one case, at the tolerances the device is held to: quantized, packet index,
    bytes, order and dedupe exactly; the raise; -120 / 50 with ==; RSSI / SNR within 1e-3 dB; filtered per component
    within 18 * 2^-53 * sum |c_m| |y_m|; discriminated within 1e-9 * max(1, |ref|).  A mirror that is None is skipped."""
    bad = []
    if len(got) != len(want):
        return [f"{len(got)} calls, expected {len(want)}"]
    for c, (g, w) in enumerate(zip(got, want)):
        if g.quantized is not None and not np.array_equal(g.quantized, w.quantized):
            d = np.flatnonzero(g.quantized != w.quantized)
            bad.append(f"call {c}: quantized differs at {d.size} positions, first {int(d[0])}")
        if (g.packets is None) != (w.packets is None):
            bad.append(f"call {c}: raise {g.packets is None}, expected {w.packets is None}")
        elif w.packets is not None:
            if [p[:2] for p in g.packets] != [p[:2] for p in w.packets]:
                bad.append(f"call {c}: packets {[p[:2] for p in g.packets]} expected {[p[:2] for p in w.packets]}")
            else:
                for a, e in zip(g.packets, w.packets):
                    for k, name in ((2, "rssi"), (3, "snr")):
                        if (k == 2 and e[k] == -120.0) or (k == 3 and e[k] == 50.0) or e[k] != e[k]:
                            ok = a[k] == e[k] or (e[k] != e[k] and a[k] != a[k])
                        else:
                            ok = abs(a[k] - e[k]) <= DB_TOL
                            if err is not None and ok:
                                err.db = max(err.db, abs(a[k] - e[k]))
                        if not ok:
                            bad.append(f"call {c} index {e[0]}: {name} {a[k]!r} expected {e[k]!r}")
        if g.filtered is not None:
            lim = FILT_ULPS * w.fbound
            dr, di = np.abs(g.filtered.real - w.filtered.real), np.abs(g.filtered.imag - w.filtered.imag)
            worst = np.maximum(dr, di)
            if not (worst <= lim).all():
                j = int(np.argmax(worst - lim))
                bad.append(f"call {c}: filtered[{j}] off by {worst[j]:.3e}, bound {lim[j]:.3e}")
            elif err is not None and (lim > 0).any():
                err.filt = max(err.filt, float(np.max(worst[lim > 0] / lim[lim > 0])))
        if g.discriminated is not None:
            tol = 1e-9 * np.maximum(1.0, np.abs(w.discriminated))
            dd = np.abs(g.discriminated - w.discriminated)
            if not (dd <= tol).all():
                j = int(np.argmax(~(dd <= tol)))
                bad.append(f"call {c}: discriminated[{j}] {g.discriminated[j]!r} expected {w.discriminated[j]!r}")
            elif err is not None:
                err.disc = max(err.disc, float(np.max(dd / tol)) * 1e-9)
    return bad


# ------------------------------------------------------------------------------------------------ certainty condition
def certainty(x: np.ndarray):
    """For every t of the stream x (complex128): is the oracle's sign at t certain?  Returns (ok, exact_zero, margin):
    exact_zero where f[t] or f[t-1] is exactly 0 + 0j (the numerator is an exact signed zero), else
    margin = |num_t| / E_t with E_t = 2^-49 A_{t-1} A_t, A_t = sum_m |c_m| (|Re y| + |Im y|) over the nine samples under
    the taps; ok = exact_zero or margin >= 1024.  E_t: nine products and eight sums on either side, a product of two
    such sums on top."""
    n = x.size
    f, _, _ = O.demod_stream_oneshot(x)
    y = O.rotate_fs4(x)
    ypad = np.concatenate([np.zeros(9), np.abs(y.real) + np.abs(y.imag)])
    A = np.convolve(ypad, np.abs(TAPS), mode="valid")[:n]
    fp = np.concatenate([np.zeros(1, dtype=np.complex128), f])
    Ap = np.concatenate([np.zeros(1), A])
    num = fp.imag[:-1] * fp.real[1:] - fp.real[:-1] * fp.imag[1:]
    zero = (fp[:-1] == 0) | (fp[1:] == 0)
    E = 2.0 ** -49 * Ap[:-1] * Ap[1:]
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.where(zero, np.inf, np.abs(num) / E)
    return zero | (margin >= 1024.0), zero, margin


# ------------------------------------------------------------------------------------------------ mode changes
def mode_change_blocks(shape_name: str):
    """uint8 blocks, then complex blocks, then a uint8 block of one byte stream (the complex ones through pyrtlsdr's
    arithmetic, so the bursts carry across the changes): [(block, is_complex)], and the stream as the oracle's LUT and
    the conversion see it, for the certainty condition."""
    shape = SHAPE[shape_name]
    B, n = shape.B, shape.B * shape.nb
    raw = synth.synth_bursts(_bursts(shape, default_starts(shape)), n, 4242 + shape.B, symbol_length=shape.S)
    n_u8 = 2 if shape.nb <= 4 else shape.nb // 3
    seq, parts = [], []
    for b in range(shape.nb):
        r = raw[2 * B * b: 2 * B * (b + 1)]
        if b < n_u8 or b == shape.nb - 1:
            seq.append((r, False))
            parts.append(O.byte_to_cmplx(r))
        else:
            seq.append((pyrtlsdr_convert(r), True))
            parts.append(seq[-1][0])
    return seq, np.concatenate(parts)


# ------------------------------------------------------------------------------------------------ the path restated
MUTANTS = {
    "no_epsilon": "epsilon omitted from discriminated",
    "piece_phase": "rotation phase counted from the first sample a piece reads instead of from the block",
    "no_block_history": "nine-sample history not carried across a block",
    "no_seam_history": "nine-sample history not carried across the 2048 seam",
    "zero_is_plus": "a zero numerator always read as +0",
    "clip_at_B": "signal window clipped at B instead of B + 1",
    "noise_fallback_0": "noise fallback 0 instead of 1e-9",
    "never_raise": "snr = 50 whenever signal_power == 0 (no raise)",
    "c64_rounded_again": "complex64 input rounded again (the filter's output to complex64) instead of only widened",
}


def _rot_signs(x: np.ndarray, phase: np.ndarray):
    """x * j^phase on the signs alone (a negation flips the sign bit, of a zero too): (re, im)."""
    a, b = x.real, x.imag
    re = np.choose(phase, [a, -b, -a, b])
    im = np.choose(phase, [b, a, -b, -a])
    return re, im


def _taps_in_order(v: np.ndarray, n_out: int) -> np.ndarray:
    acc = np.zeros(n_out)          # +0.0
    for m in range(9):
        acc = acc + TAPS[m] * v[m:m + n_out]
    return acc


def model_calls(ocfg: O.OracleConfig, blocks, mutant: Optional[str] = None) -> List[Call]:
    """The float64 arithmetic of the complex path as the kernels spell it, block by block: rotation on signs with the
    phase of the sample's index in the block; per piece of PIECE samples the nine rotated samples in front of it; the
    taps in order m = 0..8 from +0.0; the sign of prev.im * f.re - prev.re * f.im; discriminated = that over
    |prev|^2 + 1e-10; the window rolled by B; the oracle's search, slice and dedupe on it; RSSI / SNR from the sums
    over [max(0, q - PL), q) and [q, min(B + 1, q + PL)) of the newest block's filtered with the three fallbacks
    (noise 1e-9 for an empty window, -120 for signal 0, 50 for noise 0) and the raise for signal 0 over noise > 0."""
    assert mutant is None or mutant in MUTANTS
    B, L, PL = ocfg.block_size, ocfg.buffer_length, ocfg.preamble_length
    hist_re, hist_im = np.zeros(9), np.zeros(9)
    f_last = 0j
    quant = np.zeros(L, dtype=np.uint8)
    disc = np.zeros(2 * B)
    out = []
    for blk in blocks:
        is_c64 = np.asarray(blk).dtype == np.complex64
        x = np.asarray(blk, dtype=np.complex128) if np.iscomplexobj(blk) else O.byte_to_cmplx(np.asarray(blk))
        idx = np.arange(B)
        re, im = _rot_signs(x, idx & 3)
        if mutant == "no_block_history":
            hist_re, hist_im = np.zeros(9), np.zeros(9)
        fre, fim = np.empty(B), np.empty(B)
        for s0 in range(0, B, PIECE):
            n = min(PIECE, B - s0)
            if mutant == "piece_phase":
                pre_, pim_ = _rot_signs(x[s0:s0 + n], (idx[:n] + 9) & 3)
            else:
                pre_, pim_ = re[s0:s0 + n], im[s0:s0 + n]
            if s0 == 0:
                hr, hi = hist_re, hist_im
            elif mutant == "no_seam_history":
                hr, hi = np.zeros(9), np.zeros(9)
            else:
                hr, hi = re[s0 - 9:s0], im[s0 - 9:s0]
            fre[s0:s0 + n] = _taps_in_order(np.concatenate([hr, pre_]), n)
            fim[s0:s0 + n] = _taps_in_order(np.concatenate([hi, pim_]), n)
        if mutant == "c64_rounded_again" and is_c64:
            fre, fim = fre.astype(np.float32).astype(np.float64), fim.astype(np.float32).astype(np.float64)
        hist_re, hist_im = re[B - 9:], im[B - 9:]
        filt = np.concatenate([[f_last], fre + 1j * fim])
        f_last = filt[-1]
        pr, pi_, cr, ci = filt.real[:-1], filt.imag[:-1], filt.real[1:], filt.imag[1:]
        num = pi_ * cr - pr * ci
        bits = np.signbit(num).astype(np.uint8)
        if mutant == "zero_is_plus":
            bits[num == 0] = 0
        den = pr * pr + pi_ * pi_
        if mutant == "no_epsilon":      # (0 / 0 read as 0: the magnitudes have to tell it apart, not a NaN)
            d = np.where(den == 0, 0.0, num / np.where(den == 0, 1.0, den))
        else:
            d = num / (den + O.DISC_EPSILON)
        disc = np.concatenate([disc[B:], d])
        quant = np.concatenate([quant[B:], bits])
        p2 = filt.real ** 2 + filt.imag ** 2
        seen, pk = set(), []
        for q in O.search(quant, ocfg):
            if q > B:
                continue
            data = O.slice_bytes(quant, q, ocfg)
            if data in seen:
                continue
            seen.add(data)
            ns, pe = max(0, q - PL), min(B if mutant == "clip_at_B" else B + 1, q + PL)
            noise = float(np.sum(p2[ns:q])) / (q - ns) if q > ns else (0.0 if mutant == "noise_fallback_0" else 1e-9)
            sig = float(np.sum(p2[q:pe])) / (pe - q) if pe > q else float("nan")
            rssi = 10.0 * math.log10(sig) if sig > 0 else -120.0
            if mutant == "never_raise" and sig == 0:
                snr = 50.0
            elif noise > 0:
                if sig == 0:
                    pk = None    # log10(0): the reference raises out of the call, the device reports -inf
                    break
                snr = 10.0 * math.log10(sig / noise)
            else:
                snr = 50.0
            pk.append((int(q), data.hex(), rssi, snr))
        out.append(Call(pk, quant.copy(), filt.copy(), disc.copy(), None))
    return out
