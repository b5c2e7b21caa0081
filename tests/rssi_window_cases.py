"""Inputs, expected values and NumPy models for the RSSI / SNR windows of the uint8 paths (no tests in here;
tests/test_rssi_windows_cpu.py proves every condition named below on the CPU, tests/test_rssi_windows.py runs the streams
on the device).

A record (call, q) takes its two windows from the NEWEST block's filter output, filtered[j] = f[call B + j - 1]: noise
over j in [ns, q), signal over j in [q, pe), ns = max(q - 224, 0), pe = min(q + 224, B + 1) - one block AFTER the packet
whose position selects them.  So the window content can be chosen independently of the packet: a stream here (Davis
config, B = 8192, three blocks, no noise: every byte outside a burst is exactly 127) holds one planted burst - one
repetition of the preamble and a CRC-valid tail through tail_dense_cases.fsk - and a CONTENT laid over the samples its
record's windows read.  Start sample and amplitude of every burst were found with the oracle (find() below); at
amplitude 0.5 a burst matches at 14 adjacent phases and the oracle reports the lowest phase, q = 14 k; at amplitudes of
two or three LSB the run is shorter and q = 14 k + 1 (or + 3, + 8 ...) is reported, which gives the odd residues.

Positions (POSITIONS: class, call, q):
  interior    call 1 mid-block, t_lo mod 4 = 3, 0, 1, 2 (q = 4004, 4005, 4018, 4019), and 4007
  lower       ns = 0: (2, 1) with a noise window of one sample, (1, 2), (1, 14), (1, 98), (1, 210), the last clipped and
              the first unclipped q (224 is unclipped with ns = 0, 225 has ns = 1), and the twin (1, B) / (2, 0) of a
              match at position B, whose second record has an EMPTY noise window (the 1e-9 floor)
  upper       call 1, pe = B + 1: q = 7966 (pe = 8190, not clipped), 7969 (the last unclipped one), 7980, 8190, and
              q = B of the twin, where the signal window is one sample
  end_matrix  the last call, the last positions whose 32 columns end inside the stream: q = 7882, 7883, 7896, 7897
              (t_lo mod 4 = 1, 2, 3, 0; the oracle reports nothing at 7906 .. 7909)
  end_fp32    the last call, from the first q on the fp32 side: 7910, 7911, 7912, 7913 (t_lo mod 4 = 1, 2, 3, 0), 7924,
              7925, 8050 (pe clipped), 8190, 8191 and q = B

Which of rd_rssi_prepare's four `ok` conditions the batch path can make false (Davis, PL = 224, valid_from = 0):
  t_lo >= 1             never false: t_lo = call B + ns - 1 is at least B - 1 for call >= 1, and call 0 holds no record
                        at all (below)
  A - 8 >= valid_from   never false: A >= t_lo - 4 >= B - 5
  t_hi <= A + 512       never false: the two windows are at most 448 outputs and A >= t_lo - 4, so t_hi <= A + 451.  For
                        the same reason a column block of 511 outputs instead of 512 cannot change any value
  A + 520 <= n + 8      false in the last call from q = B - 282 = 7910 on (A + 512 <= n with A = (2 B + q - 226) & ~3):
                        the only reachable boundary, covered from both sides at every residue.  The samples a window's
                        outputs USE end at t_hi - 1 <= n - 2 whatever the route, so this condition guards the loads, not
                        the values: a test on values cannot see it off by one aligned load
Start of the stream: call 0 sees positions q - B, so only q = B (position 0) could be a record - and it never is: f[0]
uses y[-9 .. -1] = 0, so d[0] = disc(0, 0) = +0.0 and bit 0 of every stream is 0, while the preamble starts with a 1.
The earliest record of a stream is (1, 2).  (test_call_0_holds_no_record.)

Contents (CONTENTS), laid over the samples call B + ns - 10 .. call B + pe - 3 and a margin:
  noise       synth's noise of 0.05            quiet        nothing: bytes 127, |f|^2 = -81.4 dB from cancellation alone
  clipped     random bytes from {0, 255}       full         uniform random bytes
  step_q      quiet below window index q, full from q on      step_q_rev   full below q, quiet from q on
  step_ns     full up to index ns - 1, quiet from ns          step_pe      quiet up to pe - 1, full from pe
A byte is smeared over nine outputs (f[t] uses y[t-9 .. t-1]): output j is loud from the first loud sample call B + j - 2
on and until the last loud sample call B + j - 10, and the sample at an edge is full scale so that its single outer tap
(c0 = 0.0177) stands 40 dB above the quiet side.

PAIRS are streams of two bursts (call 1 interior: matrix route; last call, q >= 7910: fp32 route) and ORDER puts three of
them and a single fp32 stream in one group of four, so that k_tail's four waves each take two records of different
routes, in both orders.

Expected: oracle.c_oracle.demod_batch (Davis) and with packet_symbols = 72 (the generic tail); OracleDemodulator block
by block for the streamed forms.

Models of the two uint8 routes, restated from rd_device.h: model_matrix (exact integers from mfma_model.T / DHI, one
float32 combine of the two digits, float32 |g|^2, A and ok as rd_rssi_prepare) and model_fp32 (float32 with 127.4f,
1 / 127.6f, the fma chain, eight outputs per lane).  Both sum a lane's outputs in float32 in the kernel's order, the 64
lanes in float64 (the kernel: a DPP tree in float32), and take the logarithm in float64 (the kernel: v_log_f32).
route(call, q, n_samples) says which of the two k_tail / k_rssi_u8 use.  MUTANTS lists the ways to be wrong that
tests/test_rssi_windows_cpu.py tells apart from the oracle.
"""
import functools
import math
from typing import NamedTuple

import numpy as np

import mfma_model as MM
import tail_dense_cases as TD
from oracle import c_oracle as CO
from oracle import dsp_oracle as O
from parse_gate_cases import PREAMBLE
from tail_scale_cases import PACKET_DTYPE

B, N_BLOCKS = 8192, 3
N_SAMPLES = B * N_BLOCKS
PL = TD.REP                             # 224: preamble_length, the length of an unclipped window
K_GENERIC = 72                          # packet_symbols of the configuration that takes the generic tail
PAD = 24                                # margin of a content around the samples the windows read
CONTENTS = ("noise", "quiet", "clipped", "full", "step_q", "step_q_rev", "step_ns", "step_pe")
STEPS = ("step_q", "step_q_rev", "step_ns", "step_pe")
CLASSES = ("interior", "lower", "upper", "end_matrix", "end_fp32")
FIRST_FP32_Q = B - 282                  # in the last call


class Pos(NamedTuple):
    cls: str
    call: int
    q: int
    start: int          # the burst's first sample
    amp: float
    twin: tuple = ()    # the other record of a match on a block boundary


ALL = CONTENTS
POSITIONS = {   # name: (position, contents)
    "i4004": (Pos("interior", 1, 4004, 3986, 0.5), ALL),
    "i4005": (Pos("interior", 1, 4005, 3999, 0.02), ("noise", "step_q", "step_ns", "full")),
    "i4018": (Pos("interior", 1, 4018, 4000, 0.5), ("quiet", "step_q_rev", "step_pe", "step_q")),
    "i4019": (Pos("interior", 1, 4019, 4011, 0.015), ("full", "clipped", "step_q", "step_ns")),
    "i4007": (Pos("interior", 1, 4007, 3999, 0.015), ("step_q", "step_pe")),
    "l1": (Pos("lower", 2, 1, 8187, 0.02), ALL),
    "l2": (Pos("lower", 1, 2, -16, 0.5), ("noise", "step_q", "full")),
    "l14": (Pos("lower", 1, 14, -4, 0.5), ("noise", "quiet", "step_q", "step_q_rev")),
    "l98": (Pos("lower", 1, 98, 80, 0.5), ("noise", "full", "step_q", "step_q_rev", "clipped")),
    "l210": (Pos("lower", 1, 210, 192, 0.5), ("step_q", "clipped", "step_pe")),
    "l224": (Pos("lower", 1, 224, 206, 0.5), ("noise", "step_ns", "step_q")),
    "l225": (Pos("lower", 1, 225, 219, 0.02), ("quiet", "full", "step_ns", "step_q_rev")),
    "twin0": (Pos("lower", 2, 0, 8187, 0.5, twin=(1, B)), ALL),
    "twinB": (Pos("upper", 1, B, 8187, 0.5, twin=(2, 0)), ALL),
    "u7966": (Pos("upper", 1, 7966, 7948, 0.5), ("noise", "step_pe", "step_q")),
    "u7969": (Pos("upper", 1, 7969, 7962, 0.0125), ("quiet", "full", "step_pe", "step_q_rev")),
    "u7980": (Pos("upper", 1, 7980, 7962, 0.5), ALL),
    "u8190": (Pos("upper", 1, 8190, 8172, 0.5), ("noise", "quiet", "clipped", "step_q", "step_q_rev")),
    "m7882": (Pos("end_matrix", 2, 7882, 16056, 0.5), ("noise", "quiet", "full", "step_q", "step_ns")),
    "m7883": (Pos("end_matrix", 2, 7883, 16067, 0.015), ("noise", "quiet", "clipped", "step_q_rev", "step_pe")),
    "m7896": (Pos("end_matrix", 2, 7896, 16070, 0.5), ALL),
    "m7897": (Pos("end_matrix", 2, 7897, 16083, 0.02), ("noise", "quiet", "full", "step_q", "step_pe")),
    "f7910": (Pos("end_fp32", 2, 7910, 16084, 0.5), ALL),
    "f7911": (Pos("end_fp32", 2, 7911, 16095, 0.015), ("noise", "quiet", "full", "step_q", "step_ns")),
    "f7912": (Pos("end_fp32", 2, 7912, 16098, 0.025), ("noise", "quiet", "clipped", "step_q_rev", "step_pe")),
    "f7913": (Pos("end_fp32", 2, 7913, 16098, 0.0125), ("noise", "quiet", "full", "step_q", "step_pe")),
    "f7924": (Pos("end_fp32", 2, 7924, 16098, 0.5), ("noise", "step_q_rev")),
    "f7925": (Pos("end_fp32", 2, 7925, 16111, 0.02), ("quiet", "step_q")),
    "f8050": (Pos("end_fp32", 2, 8050, 16224, 0.5), ("noise", "step_q", "step_pe", "clipped")),
    "f8190": (Pos("end_fp32", 2, 8190, 16364, 0.5), ("noise", "quiet", "step_q", "step_q_rev")),
    "f8191": (Pos("end_fp32", 2, 8191, 16378, 0.5), ("full", "step_q")),
    "fB": (Pos("end_fp32", 2, B, 16379, 0.5), ("noise", "quiet", "clipped", "full", "step_q", "step_q_rev", "step_ns")),
}
PAIRS = {   # name: ((position, content) of the matrix-route record, of the fp32-route record)
    "pairA": (("i4004", "full"), ("f7910", "quiet")),
    "pairB": (("i4018", "quiet"), ("f7924", "clipped")),
    "pairC": (("i4005", "step_q"), ("f7913", "noise")),
    "pairD": (("i4019", "noise"), ("f7911", "step_q_rev")),
}


def find(want, amps=(0.5, 0.02, 0.015, 0.025, 0.0125, 0.01), span=22):
    """How POSITIONS was made: the first (start, amplitude) for which the oracle's records of the stream are exactly
    `want`, a sorted list of (call, q)."""
    c, q = want[0]
    p = (c - 1) * B + q
    cands = [(s, a) for a in amps for s in range(p - span, p - 1)]
    raw = np.stack([_burst_stream([(s, a)]) for s, a in cands])
    pk, _ = CO.demod_batch(raw, CO.make_cfg(block_size=B), threads=4)
    for cand, recs in zip(cands, pk):
        if sorted((r.call, r.index) for r in recs) == list(want):
            return cand
    return None


# ------------------------------------------------------------------------------------------------ geometry
def window(call, q, n_samples=N_SAMPLES):
    """rd_rssi_prepare for the batch path (origin = call B, valid_from = 0)."""
    ns, pe = max(q - PL, 0), min(q + PL, B + 1)
    origin = call * B
    t_lo, t_hi = origin + ns - 1, origin + pe - 2
    a = (t_lo - 1) & ~3
    ok = t_lo >= 1 and a - 8 >= 0 and a + 16 * 31 + 24 <= n_samples + 8 and t_hi <= a + 512
    return dict(ns=ns, pe=pe, origin=origin, t_lo=t_lo, t_hi=t_hi, A=a, ok=ok)


def route(call, q, n_samples=N_SAMPLES):
    """The arithmetic k_tail and k_rssi_u8 give the record (call, q) of a stream of n_samples."""
    return "matrix" if window(call, q, n_samples)["ok"] else "fp32"


def loud_samples(content, call, q):
    """[lo, hi) of the samples a content overwrites (before clipping at the stream) and, for a step, the sample at the
    edge: the first loud one of step_q / step_pe, the last loud one of step_q_rev / step_ns."""
    w = window(call, q)
    o, lo, hi = w["origin"], w["origin"] + w["ns"] - 10, w["origin"] + w["pe"] - 2
    if content == "quiet":
        return None
    if content == "step_q":
        return o + q - 2, hi + PAD, o + q - 2
    if content == "step_q_rev":
        return lo - PAD, o + q - 10, o + q - 11
    if content == "step_ns":
        return lo - PAD - 16, lo, lo - 1
    if content == "step_pe":
        return hi, hi + PAD, hi
    return lo - PAD, hi + PAD, None


def step_index(content, call, q):
    """The window index at which a step's |f|^2 changes, and whether the loud side is the upper one."""
    w = window(call, q)
    return {"step_q": (q, True), "step_q_rev": (q, False), "step_ns": (w["ns"], False), "step_pe": (w["pe"], True)}[content]


# ------------------------------------------------------------------------------------------------ generator
def _burst_stream(bursts):
    """[(start, amplitude)] -> a stream without noise.  Each burst's samples come from a stream of its own (they are 127
    elsewhere), so that a burst is the same bytes whatever else its stream holds."""
    out = np.full(2 * N_SAMPLES, 127, dtype=np.uint8)
    for s, a in bursts:
        one = TD.fsk([(s, TD.train(1, TD.TAILS[0]))], 1, amplitude=a, noise=0.0, n_samples=N_SAMPLES)
        lo, hi = max(s, 0), min(s + 88 * TD.S, N_SAMPLES)
        out[2 * lo: 2 * hi] = one[2 * lo: 2 * hi]
    return out


def _lay(raw, content, call, q, seed):
    span = loud_samples(content, call, q)
    if span is None:
        return
    lo, hi, edge = span
    lo, hi = max(lo, 0), min(hi, N_SAMPLES)
    rng = np.random.default_rng(seed)
    n = hi - lo
    if content == "noise":
        x = 0.05 * rng.standard_normal(2 * n)
        new = np.clip(np.rint(x * 127.6 + 127.4), 0, 255).astype(np.uint8)
    elif content == "clipped":
        new = (255 * rng.integers(0, 2, 2 * n)).astype(np.uint8)
    else:
        new = rng.integers(0, 256, 2 * n, dtype=np.uint8)
    raw[2 * lo: 2 * hi] = new
    if edge is not None and lo <= edge < hi:
        raw[2 * edge: 2 * edge + 2] = (255, 0)


class Record(NamedTuple):
    name: str           # "<position>/<content>" (a pair: "<pair>:<position>/<content>")
    stream: int
    pos: str
    content: str
    cls: str
    call: int
    q: int
    planted: bool       # False for the other record of a twin: its windows hold whatever the planted one's content is


def _plan():
    """[(stream name, [(position name, content)])]: the single-burst streams, then the pairs."""
    out = [(f"{p}/{c}", [(p, c)]) for p, (_, cs) in POSITIONS.items() for c in cs]
    out += [(name, list(parts)) for name, parts in PAIRS.items()]
    return out


class Cases:
    """raw [n, 2 N_SAMPLES] uint8 in ORDER; records: one Record per expected rd_packet, in the order results() must
    have; recs: the same as rd_packet records (the oracle's rssi / snr); bits; per-stream oracle packets pk."""

    def __init__(self):
        plan = _plan()
        names = [n for n, _ in plan]
        # one group of four whose records alternate routes along every wave of k_tail (r, r + 4): MF MF F MF
        group = ["pairA", "pairB", "f7910/noise", "pairC"]
        rest = [n for n in names if n not in group]
        # the other streams: matrix-route and fp32-route records in turn as far as they go
        mat = [n for n in rest if n not in PAIRS and POSITIONS[n.split("/")[0]][0].cls != "end_fp32"]
        fp = [n for n in rest if n not in mat]
        mixed = []
        for k in range(max(len(mat), len(fp))):
            mixed += mat[k: k + 1] + fp[k: k + 1]
        self.order = group + mixed
        parts_of = dict(plan)
        streams = []
        for k, name in enumerate(self.order):
            parts = parts_of[name]
            raw = _burst_stream([(POSITIONS[p][0].start, POSITIONS[p][0].amp) for p, _ in parts]).copy()
            for m, (p, c) in enumerate(parts):
                pos = POSITIONS[p][0]
                _lay(raw, c, pos.call, pos.q, 7000 + 10 * names.index(name) + m)
            streams.append(raw)
        self.raw = np.stack(streams)
        self.raw.setflags(write=False)
        self.n_streams = len(streams)
        self.pk, self.bits = CO.demod_batch(self.raw, CO.make_cfg(block_size=B), threads=4, want_bits=True)
        self.recs = records_of(self.pk)
        self.planted = []           # per stream: the sorted (call, q) the plan promises
        self.records = []
        for s, name in enumerate(self.order):
            want = {}
            for p, c in parts_of[name]:
                pos = POSITIONS[p][0]
                tag = f"{name}:{p}/{c}" if name in PAIRS else name
                want[(pos.call, pos.q)] = Record(tag, s, p, c, pos.cls, pos.call, pos.q, True)
                if pos.twin:
                    cls = "lower" if pos.twin[1] == 0 else "upper"
                    want[pos.twin] = Record(tag + "+twin", s, p, c, cls, pos.twin[0], pos.twin[1], False)
            self.planted.append(sorted(want))
            self.records += [want[k] for k in sorted(want)]

    def by_name(self, name):
        return next(r for r in self.records if r.name == name)


def records_of(pk):
    n = sum(len(p) for p in pk)
    recs = np.zeros(n, dtype=PACKET_DTYPE)
    k = 0
    for s, plist in enumerate(pk):
        for p in plist:
            r = recs[k]
            r["stream"], r["call"], r["index"], r["nbytes"] = s, p.call, p.index, p.data.size
            r["data"][: p.data.size] = p.data
            r["rssi"], r["snr"] = p.rssi, p.snr
            k += 1
    recs.setflags(write=False)
    return recs


@functools.lru_cache(maxsize=None)
def cases():
    return Cases()


@functools.lru_cache(maxsize=None)
def generic_recs():
    """The same streams under packet_symbols = 72 (rd_davis_slice false: k_slice_rssi<rd_u8_src>, fp32 everywhere)."""
    pk, _ = CO.demod_batch(cases().raw, CO.make_cfg(packet_symbols=K_GENERIC, block_size=B), threads=4)
    return records_of(pk)


def streamed_subset():
    """Streams for the block-by-block forms: every (class, content) pair once, and the pairs."""
    cs = cases()
    seen, pick = set(), []
    for r in cs.records:
        if r.planted and (r.cls, r.content) not in seen:
            seen.add((r.cls, r.content))
            if r.stream not in pick:
                pick.append(r.stream)
    return sorted(set(pick) | {cs.order.index(n) for n in PAIRS})


@functools.lru_cache(maxsize=None)
def streamed_calls(s, packet_symbols=80):
    """OracleDemodulator over stream s block by block: [[(index, hex, rssi, snr)] per call]."""
    dem = O.OracleDemodulator(O.OracleConfig(19200, TD.S, TD.P, packet_symbols, PREAMBLE, B))
    raw = cases().raw[s]
    return [[(int(p.index), bytes(p.data).hex(), float(p.rssi), float(p.snr)) for p in dem.demodulate(raw[2 * B * b: 2 * B * (b + 1)])]
            for b in range(N_BLOCKS)]


# ------------------------------------------------------------------------------------------------ the models
MUTANTS = ("split jj <= q", "ns off by one", "pe clipped at B", "A not rounded", "511 outputs", "origin off by one",
           "floor 0", "divide by PL", "ok off by one", "stale prefetch")
F32 = np.float32
_C32 = O.FIR9_COEFFS.astype(np.float32)
_INV = F32(1.0 / (127.6 * (MM.SCALE / 16777216.0) * 127.6 * (MM.SCALE / 16777216.0)))


def _fma32(a, b, c):
    """fmaf on float32 arrays (the product of two float32 is exact in float64)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _limits(call, q, mutant):
    w = window(call, q)
    ns, pe = w["ns"], w["pe"]
    if mutant == "ns off by one":
        ns = max(q - PL - 1, 0)
    if mutant == "pe clipped at B":
        pe = min(q + PL, B)
    return w, ns, pe


def finish(noise, sig, ns, pe, q, mutant=None):
    """rd_rssi_finish behind the wave sum: float32 divides, the reference's floor and fallbacks; log in float64."""
    dn, ds = (PL, PL) if mutant == "divide by PL" else (q - ns, pe - q)
    floor = F32(0.0) if mutant == "floor 0" else F32(1e-9)
    noise_power = F32(noise) / F32(dn) if q > ns else floor
    signal_power = F32(sig) / F32(ds) if pe > q else F32("nan")
    rssi = 10.0 * math.log10(float(signal_power)) if signal_power > 0 else -120.0
    if noise_power > 0:
        ratio = float(F32(signal_power) / F32(noise_power))
        snr = 10.0 * math.log10(ratio) if ratio > 0 else float("nan")
    else:
        snr = 50.0
    return rssi, snr


def _lane_sums(pw, jj, ns, pe, q, mutant):
    """pw, jj [64, 8]: a lane's eight outputs added in float32 in register order, split at q."""
    below = jj <= q if mutant == "split jj <= q" else jj < q
    inside = (jj >= ns) & (jj < pe)
    sn, ss = np.zeros(64, dtype=np.float32), np.zeros(64, dtype=np.float32)
    for r in range(8):
        sn = sn + np.where(inside[:, r] & below[:, r], pw[:, r], F32(0))
        ss = ss + np.where(inside[:, r] & ~below[:, r], pw[:, r], F32(0))
    return sn, ss


def _bytes_at(raw, first, count):
    """`count` samples from sample `first` as [count, 2] float64, zero outside the stream."""
    out = np.zeros((count, 2))
    lo, hi = max(first, 0), min(first + count, raw.size // 2)
    if hi > lo:
        out[lo - first: hi - first] = raw[2 * lo: 2 * hi].reshape(-1, 2)
    return out


def model_matrix(raw, call, q, mutant=None, stale=None):
    """rd_rssi_block + rd_rssi_finish.  `stale` = (raw, call, q) of the job whose bytes a broken pipeline would use."""
    w, ns, pe = _limits(call, q, mutant)
    a = w["A"]
    src_raw, src_a = (stale[0], window(stale[1], stale[2])["A"]) if stale else (raw, a)
    u = _bytes_at(src_raw, src_a + 1 - 9, 512 + 8)            # samples A - 8 .. A + 511: what rd_rssi_fetch loads
    z = u[:, 0] + 1j * u[:, 1]
    taps = [MM.T[m if m <= 4 else 8 - m] * (1j ** m) for m in range(9)]
    g = sum(taps[m] * z[m: m + 512] for m in range(9)) - 2048.0 * MM.DHI * (1 + 1j)   # exact integers: t = A+1 .. A+512
    lane = np.arange(64)
    k = (16 * (lane & 31) + 8 * (lane >> 5))[:, None] + np.arange(8)[None, :]         # t - (A + 1)
    gr = (g.real[k] * MM.UNIT).astype(np.float32)             # fmaf(ah, 2048, al): one rounding of the exact sum
    gi = (g.imag[k] * MM.UNIT).astype(np.float32)
    pw = _fma32(gr, gr, gi * gi)
    a_idx = w["t_lo"] - 1 if mutant == "A not rounded" else a
    origin = w["origin"] + (1 if mutant == "origin off by one" else 0)
    jj = a_idx + k + 1 - origin + 1
    if mutant == "511 outputs":
        jj = np.where(k >= 511, -1, jj)
    sn, ss = _lane_sums(pw, jj, ns, pe, q, mutant)
    return finish((sn * _INV).astype(np.float64).sum(), (ss * _INV).astype(np.float64).sum(), ns, pe, q, mutant)


def model_fp32(raw, call, q, mutant=None):
    """rd_rssi_u8: one pass of 512 outputs from window index ns, lane l the outputs ns + 8 l .. ns + 8 l + 7."""
    w, ns, pe = _limits(call, q, mutant)
    assert pe - ns <= 512
    origin = w["origin"] + (1 if mutant == "origin off by one" else 0)
    n0 = origin + ns - 10                                     # lane 0's first sample
    u = _bytes_at(raw, n0, 512 + 8).astype(np.float32)
    inside = ((np.arange(n0, n0 + 520) >= 0))[:, None]
    x = np.where(inside, (u - F32(127.4)) * (F32(1.0) / F32(127.6)), F32(0))
    ph = np.arange(n0, n0 + 520) & 3
    a, b = x[:, 0], x[:, 1]
    yr = np.select([ph == 0, ph == 1, ph == 2], [a, -b, -a], b)
    yi = np.select([ph == 0, ph == 1, ph == 2], [b, a, -b], -a)
    fr, fi = np.zeros(512, dtype=np.float32), np.zeros(512, dtype=np.float32)
    for m in range(9):
        c = np.full(512, _C32[m], dtype=np.float32)
        fr, fi = _fma32(c, yr[m: m + 512], fr), _fma32(c, yi[m: m + 512], fi)
    pw = (fr * fr + fi * fi).reshape(64, 8)
    jj = ns + np.arange(512).reshape(64, 8)
    sn, ss = _lane_sums(pw, jj, ns, pe, q, mutant)
    return finish(sn.astype(np.float64).sum(), ss.astype(np.float64).sum(), ns, pe, q, mutant)


def model(raw, call, q, mutant=None, next_raw=None):
    """The record's figures by the route k_tail / k_rssi_u8 give it.  "ok off by one" lets the matrix route go one
    aligned load (four samples) past the end of the stream, into the next stream's bytes."""
    n = N_SAMPLES + (4 if mutant == "ok off by one" else 0)
    if n > N_SAMPLES:
        raw = np.concatenate([raw, next_raw[:64] if next_raw is not None else np.zeros(64, dtype=np.uint8)])
    return (model_matrix if route(call, q, n) == "matrix" else model_fp32)(raw, call, q, mutant)


def db_diff(got, want):
    """|got - want| of an (rssi, snr) pair in dB; a NaN or a fallback constant on one side only counts as infinite."""
    out = 0.0
    for g, e in zip(got, want):
        if math.isnan(g) and math.isnan(e):
            continue
        d = abs(g - e)
        out = max(out, float("inf") if math.isnan(d) else d)
    return out
