"""Inputs and expected values for the batch tail on dense match lists (no tests in here; tests/test_tail_dense_cpu.py
checks every condition named below on the CPU, tests/test_tail_dense.py runs the batches on the device).

k_tail (rd_tail.hip) searches, slices, dedupes, ranks and writes the records of four streams per workgroup, with a
match list per stream in LDS: 32 entries for these short streams, doubled by the host after every upload that
overflowed it, up to 512.  The other tail tests give a stream at most 16 raw preamble matches, or about a hundred spread
over hundreds of blocks; here a stream of four blocks of 8192 holds up to 530.

The input that makes this cheap is a preamble TRAIN: an FSK burst whose symbols are the 16-symbol preamble repeated R
times, then a payload.  Every repetition matches at about 13 adjacent sample phases, and matches 224 samples (16
symbols) apart slice the same 80 symbols as long as five repetitions follow: a train is a run of duplicates with a few
distinct packets at its end.  fsk() is synth.synth_bursts' modulation, noise and quantisation for any symbol string,
without the lead-in a transmitter sends (unless the symbols hold one).

Batches (Davis config, block_size 8192, four blocks per stream; seeds and starts chosen with the oracle):
  full_list_a / _b   streams with exactly 32, 0, 31 and 32 raw matches in the first group (b: 33 instead of 31), a
                     second group of ordinary bursts and a ragged third group of two streams that hold records
  ladder_N           one train with a count in 33..64, 65..128, 129..256, 257..512 and above 512 (N = 64, 128, 256, 512,
                     over) between ordinary and quiet neighbours
  rounds             a stream of two identical trains (65..128 matches: two lane rounds of 64) and a 24-repetition
                     train (257..512: five rounds)
  twins              trains across block boundaries with a match at a position p = k 8192: the records (k, 8192) and
                     (k + 1, 0)
  geometry           runs of adjacent matches across a multiple of 8192, of 128 and of 32 positions, around the last
                     reported position, and from sample 0
  many_records       four streams of 17 weak bursts each: more than 64 records per stream, more than 256 in the group
  ordinary           eight streams with at most one burst each
  long_96            four streams of 105 blocks, whose lists are 96 entries from their length alone: a train with 65..96
                     matches, and a stream of five one-repetition trains along its length

Expected: oracle.c_oracle.demod_batch (packets with call, index, bytes, RSSI, SNR, and the packed bits), the raw match
count of a stream from oracle.dsp_oracle.search over its bits up to last_position(), parsed rows from
oracle.dsp_oracle.parse_calls through parse_gate_cases.message_rows.
"""
import functools

import numpy as np

from oracle import c_oracle as CO
from oracle import dsp_oracle as O
from parse_gate_cases import PREAMBLE, message_rows
from rtldavis_amd import synth
from tail_scale_cases import GROUP, PACKET_DTYPE, assert_records_equal   # noqa: F401  (re-exported)

B, N_BLOCKS = 8192, 4
N_SAMPLES = B * N_BLOCKS
S, P, K = 14, 16, 80                    # samples per symbol, preamble symbols, packet symbols
REP = P * S                             # 224: samples per repetition of the preamble
PRE = np.array([int(c) for c in PREAMBLE], dtype=np.uint8)
SAMPLE_RATE = 19200 * S
LIST_MIN, LIST_MAX = 32, 512            # RD_BUCKET_MIN, RD_BUCKET_MAX
LANES = 64
DELAY = 12                              # a train that starts at sample s matches around s + DELAY + 224 r (+- 6)


def oracle_cfg():
    return O.OracleConfig(19200, S, P, K, PREAMBLE, B)


def last_position(n_blocks=N_BLOCKS):
    """The last stream position a call reports (index B of the last call): p_hi of the device's search."""
    return (n_blocks + 1) * B - oracle_cfg().buffer_length


def list_from_length(n_samples):
    """rd_ord_bucket_cap (rd_host.cpp): the list a fresh handle gives a stream of this length."""
    want = (4 * n_samples + 65535) // 65536 + 12
    return min(max((want + 31) // 32 * 32, LIST_MIN), LIST_MAX)


def list_size(count):
    """The shortest match list (a power of two times 32) that holds `count` matches."""
    size = LIST_MIN
    while size < count:
        size *= 2
    return size


# ------------------------------------------------------------------------------------------------ generator
def train(reps, tail_hex="", trailing=8):
    """Symbols of a preamble train: the preamble `reps` times, the bits of `tail_hex` MSB first, `trailing` zeros."""
    tail = np.unpackbits(np.frombuffer(bytes.fromhex(tail_hex), dtype=np.uint8))
    return np.concatenate([np.tile(PRE, reps), tail, np.zeros(trailing, dtype=np.uint8)])


def fsk(parts, seed, amplitude=0.5, noise=0.05, n_samples=N_SAMPLES):
    """One stream of uint8 interleaved IQ: ``parts`` is a list of (start sample, symbol array).  Modulation, noise and
    quantisation are synth.synth_bursts' (a tone at -Fs/4 +- 4800 Hz with continuous phase, symbol 1 the upper one;
    the generator draws the noise, real then imaginary); nothing is put in front of the symbols.  Where two parts
    overlap the one listed first keeps its samples; a part may reach past either end of the stream and is cut there."""
    rng = np.random.default_rng(seed)
    freq = np.full(n_samples, -SAMPLE_RATE / 4.0)
    on = np.zeros(n_samples)
    for start, sym in reversed(list(parts)):
        chips = np.repeat(np.asarray(sym, dtype=np.uint8), S)
        lo, hi = max(int(start), 0), min(int(start) + chips.size, n_samples)
        chips = chips[lo - int(start): hi - int(start)]
        on[lo:hi] = 1.0
        freq[lo:hi] = -SAMPLE_RATE / 4.0 + np.where(chips == 1, 4800.0, -4800.0)
    phase = np.cumsum(freq) * (2.0 * np.pi / SAMPLE_RATE)
    x = amplitude * on * np.exp(1j * phase)
    x = x + noise * (rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples))
    out = np.empty(2 * n_samples, dtype=np.uint8)
    out[0::2] = np.clip(np.rint(x.real * 127.6 + 127.4), 0, 255).astype(np.uint8)
    out[1::2] = np.clip(np.rint(x.imag * 127.6 + 127.4), 0, 255).astype(np.uint8)
    return out


TAILS = tuple(p[4:] for p in synth.OTA_PACKETS)   # the last repetition of a train and its tail: a CRC-valid packet


def ordinary(k, n_samples=N_SAMPLES):
    """One burst as a transmitter sends it (lead-in, a CRC-valid packet, trailing zeros) at synth's usual amplitude."""
    ota = bytes.fromhex(synth.OTA_PACKETS[k % len(synth.OTA_PACKETS)])
    return synth.synth_bursts([(ota, 1500 + 3911 * k, 300.0 * (k - 3))], n_samples, 81000 + k)


def quiet(k):
    """Noise alone; k = 1 and 3 are without a single preamble match."""
    return synth.synth_bursts([], N_SAMPLES, 82000 + k)


def exact(seed):
    """A three-repetition train at amplitude 0.2: 30 to 34 raw matches, by the seed."""
    return fsk([(3000 + 17 * seed, train(3, TAILS[0]))], 9000 + seed, amplitude=0.2)


EXACT_SEEDS = {31: 1, 32: (10, 11, 12), 33: 4}
LADDER_REPS = {64: 4, 128: 6, 256: 12, 512: 24, "over": 40}


def ladder_train(reps):
    return fsk([(5000, train(reps, TAILS[0]))], 9100)


def boundary_train(k, reps_before, reps, delta, seed):
    """A train whose repetition `reps_before` matches around position k B + delta (+- 6)."""
    return fsk([(k * B - DELAY + delta - REP * reps_before, train(reps, TAILS[1]))], 9300 + seed)


def weak_bursts(seed, n_bursts=17, gap=1800, first=200):
    """17 bursts with payloads of their own (a short lead-in, the preamble, 64 random bits) at amplitude 0.14: every
    burst matches at five or six phases and nearly every phase slices other bytes."""
    rng = np.random.default_rng(100 + seed)
    parts = []
    for k in range(n_bursts):
        body = rng.integers(0, 256, 8, dtype=np.uint8)
        sym = np.concatenate([np.tile([1, 0], 8).astype(np.uint8), PRE, np.unpackbits(body), np.zeros(4, dtype=np.uint8)])
        parts.append((first + gap * k, sym))
    return fsk(parts, 9500 + seed, amplitude=0.14)


TWINS = ((2, 3, 8, 7, 0), (2, 3, 8, 7, 1), (1, 0, 1, 7, 0), (1, 0, 8, 7, 0), (1, 3, 8, -5, 0), (3, 3, 8, 0, 0), (3, 0, 1, 6, 0))
MANY_SEEDS = (1, 2, 6, 7)


def _streams(name):
    if name in ("full_list_a", "full_list_b"):
        third = exact(EXACT_SEEDS[31]) if name == "full_list_a" else exact(EXACT_SEEDS[33])
        return [exact(EXACT_SEEDS[32][0]), quiet(1), third, exact(EXACT_SEEDS[32][1]),
                ordinary(0), ordinary(1), ordinary(2), ordinary(3), ordinary(4), exact(EXACT_SEEDS[32][2])]
    if name.startswith("ladder_"):
        key = name[len("ladder_"):]
        return [ordinary(0), ladder_train(LADDER_REPS[int(key) if key.isdigit() else key]), ordinary(1), quiet(1),
                ordinary(2), ordinary(3), ordinary(4), ordinary(5)]
    if name == "rounds":
        two = fsk([(9000, train(3, TAILS[2])), (12000, train(3, TAILS[2]))], 9600)
        return [ordinary(0), two, ordinary(1), fsk([(5000, train(24, TAILS[0]))], 9101),
                ordinary(2), quiet(1), ordinary(3), ordinary(4)]
    if name == "twins":
        return [boundary_train(*t) for t in TWINS] + [ordinary(0)]
    if name == "geometry":
        return [boundary_train(1, 3, 8, 0, 2),                                   # across position 8192
                fsk([(128 * 39 - DELAY, train(2, TAILS[3]))], 9401),              # across a multiple of 128
                ordinary(0),
                fsk([(32 * 157 - DELAY, train(2, TAILS[3]))], 9402),              # across a multiple of 32, not of 128
                boundary_train(3, 3, 8, 4, 3),                                   # around the last reported position
                fsk([(0, train(3, TAILS[4]))], 9403),                             # from sample 0
                ordinary(1), ordinary(2)]
    if name == "many_records":
        return [weak_bursts(s) for s in MANY_SEEDS] + [ordinary(0), ordinary(1)]
    if name == "long_96":
        n = LONG_BLOCKS * B
        return [ordinary(0, n), fsk([(70 * B - 1000, train(5, TAILS[0]))], 9700, n_samples=n), ordinary(1, n),
                fsk([(5000 + 25 * B * k + 977 * k, train(1, TAILS[k])) for k in range(5)], 9701, n_samples=n)]
    if name == "ordinary":
        return [ordinary(k) for k in range(7)] + [quiet(3)]
    raise KeyError(name)


LONG_BLOCKS = 105     # rd_ord_bucket_cap gives a stream of 105 blocks a list of 96: a long list without any growth
NAMES = ("full_list_a", "full_list_b", "ladder_64", "ladder_128", "ladder_256", "ladder_512", "ladder_over", "rounds",
         "twins", "geometry", "many_records", "ordinary", "long_96")
PARSED = ("full_list_a", "full_list_b", "twins")     # the batches whose parsed rows the device test compares


def positions(bits):
    """Every position of the unpacked `bits` at which the preamble matches, ascending (beyond last_position() too)."""
    m = np.ones(bits.size - (P - 1) * S, dtype=bool)
    for k, c in enumerate(PRE):
        m &= bits[S * k: S * k + m.size] == c
    return np.flatnonzero(m)


def bytes_at(bits, p):
    """The packet's bytes sliced at position p: 80 symbols 14 samples apart, the first one the MSB of byte 0."""
    return np.packbits(bits[p: p + K * S: S]).tobytes()


class Batch:
    """raw [n, 2 N_SAMPLES] uint8; recs: the whole batch's rd_packet records in the order results() must have; counts:
    records per stream; bits [n, N_SAMPLES / 8] packed LSB first; raw_matches: a stream's preamble matches up to
    last_position(); rows(): parsed() of the whole batch as parse_gate_cases.parsed_rows gives it."""

    def __init__(self, name):
        self.name = name
        self.n_blocks = LONG_BLOCKS if name.startswith("long_") else N_BLOCKS
        self.n_samples = self.n_blocks * B
        self.raw = np.stack(_streams(name))
        self.raw.setflags(write=False)
        self.n_streams = len(self.raw)
        self.pk, self.bits = CO.demod_batch(self.raw, CO.make_cfg(block_size=B), threads=4, want_bits=True, cap_per_stream=1100)
        self.bits.setflags(write=False)
        self.counts = np.array([len(p) for p in self.pk], dtype=np.int64)
        self.recs = np.zeros(int(self.counts.sum()), dtype=PACKET_DTYPE)
        k = 0
        for s, pk in enumerate(self.pk):
            for p in pk:
                r = self.recs[k]
                r["stream"], r["call"], r["index"], r["nbytes"] = s, p.call, p.index, p.data.size
                r["data"][: p.data.size] = p.data
                r["rssi"], r["snr"] = p.rssi, p.snr
                k += 1
        self.recs.setflags(write=False)
        cfg, hi = oracle_cfg(), last_position(self.n_blocks)
        self.raw_matches = np.array([sum(1 for p in O.search(self.unpacked(s), cfg) if p <= hi) for s in range(self.n_streams)],
                                    dtype=np.int64)

    def unpacked(self, s):
        return np.unpackbits(self.bits[s], bitorder="little")[: self.n_samples]

    def stream_recs(self, s):
        return self.recs[self.recs["stream"] == s]

    @functools.lru_cache(maxsize=None)
    def calls(self):
        cfg = oracle_cfg()
        return [O.parse_calls([s[2 * B * b: 2 * B * (b + 1)] for b in range(self.n_blocks)], cfg) for s in self.raw]

    def rows(self):
        return [r for s, calls in enumerate(self.calls()) for rows in message_rows(calls, stream=s) for r in rows]

    def list_size(self):
        """The match lists this batch needs for its first pass: a fresh handle's, doubled until they hold."""
        size = list_from_length(self.n_samples)
        while size < int(self.raw_matches.max()):
            size *= 2
        return size


@functools.lru_cache(maxsize=None)
def batch(name):
    return Batch(name)
