"""Inputs and expected values for the batch tail past 1024 stream groups (no tests in here; tests/test_tail_scale_cpu.py
checks the conditions below on the CPU, tests/test_tail_scale.py runs the batches on the device).

k_tail gives a workgroup RD_FT_STREAMS = 4 consecutive streams; a group publishes its record count and adds up the counts
of every group in front of it, 1024 per round of its prefix loop, and 1024 workgroups are resident at once.  The batches
here are 4098, 4100 and 8197 streams: 1025 groups (the last with two streams, and full) and 2050 groups (the last with
one stream).  Streams are short so that thousands cost nothing: the Davis config at block_size 512, 12 blocks (6144
samples, three 2048-sample tiles of the demod kernel, whose chunks therefore cross stream boundaries everywhere).

U = 37 unique streams (coprime to 4: no two neighbouring groups hold the same four streams).  Stream u carries u % 4
bursts with payloads, starts and frequency offsets of its own, over noise of its own seed.  A burst at synth's usual
amplitude matches the preamble at 11 to 15 of its 14-sample phases and three of them would overflow a 32-entry match
list, so a stream's amplitude goes by its burst count (AMPLITUDE): one burst at 0.5 (a third of these CRC-invalid by a
flipped bit), two at 0.14, three at 0.12 - weak bursts match at fewer phases and nearly every phase slices other bytes,
which gives up to 13 records per stream from at most 16 raw matches, several of them in one call.  Batch stream s is
unique stream s % 37, except the QUIET stretch - streams 4088 .. 4099, the whole groups 1022, 1023 and 1024 - which is
noise-only streams without a single preamble match: whole groups with zero records on both sides of the 1024-group
boundary, among them the first group of the second prefix round.  Amplitudes and seeds were chosen with the oracle.

Expected: oracle.c_oracle.demod_batch on the 37 + 12 source streams (packets with call, index, bytes, RSSI, SNR, and the
packed bits); the batch's records are the sources' records concatenated in stream order.  Parsed rows:
oracle.dsp_oracle.parse_calls through parse_gate_cases.message_rows.
"""
import functools

import numpy as np

from oracle import c_oracle as CO
from oracle import dsp_oracle as O
from parse_gate_cases import PREAMBLE, message_rows
from rtldavis_amd import synth

B, N_BLOCKS = 512, 12
N_SAMPLES = B * N_BLOCKS
U = 37
GROUP = 4                       # RD_FT_STREAMS
ROUND = 1024                    # groups per round of k_tail's prefix loop = workgroups resident on 256 CUs
QUIET = range(4088, 4100)       # groups 1022, 1023, 1024
N_STREAMS = (4098, 4100, 8197)
BURST_SAMPLES = (32 + 80 + 8) * 14   # lead-in, packet, trailing zero symbols

PACKET_DTYPE = np.dtype([("stream", "<i4"), ("call", "<i4"), ("index", "<i4"), ("nbytes", "<i4"),
                         ("data", "u1", (32,)), ("rssi", "<f8"), ("snr", "<f8")])   # rd_packet (batch.RD_PACKET_DTYPE)


def oracle_cfg():
    return O.OracleConfig(19200, 14, 16, 80, PREAMBLE, B)


def last_position():
    """The last stream position a call reports (index B of the last call): what the device's search covers."""
    return (N_BLOCKS + 1) * B - oracle_cfg().buffer_length


AMPLITUDE = {0: 0.5, 1: 0.5, 2: 0.14, 3: 0.12}   # by bursts in the stream


def bursts_of(u):
    """[(on-air bytes, start, cfo)] of unique stream u: u % 4 bursts; a third of the strong ones CRC-invalid."""
    out = []
    for i in range(u % 4):
        body = bytes([(u * 8) & 0xF8, u, 0x31 * (i + 1), (u * 29 + 5) & 0xFF, (i * 53 + 7) & 0xFF, 0xA5])
        flip = (u * 5 + i) % 64 if (u + i) % 3 == 0 else None
        ota = synth.make_packet((u + i) % 8, body, flip_bit=flip)
        cfo = (1000.0 + 23.0 * u + 170.0 * i) * (-1 if (u // 4 + i) % 2 else 1)
        out.append((ota, 20 + 1900 * i + 5 * u, cfo))
    return out


class Cases:
    """raw [49, 2 N] uint8: the 37 unique streams, then the 12 quiet ones.  Per source stream: pk (the C oracle's
    packets), recs (the same as rd_packet records with stream 0), bits (packed, LSB first), raw_matches (preamble
    matches of the whole stream's bits up to last_position()), calls (parse_calls' rows per call)."""

    def __init__(self):
        cfg = oracle_cfg()
        streams = [synth.synth_bursts(bursts_of(u), N_SAMPLES, 70000 + u, amplitude=AMPLITUDE[u % 4]) for u in range(U)]
        streams += [synth.synth_bursts([], N_SAMPLES, 71000 + k) for k in range(len(QUIET))]
        self.raw = np.stack(streams)
        self.raw.setflags(write=False)
        self.pk, self.bits = CO.demod_batch(self.raw, CO.make_cfg(block_size=B), threads=4, want_bits=True)
        self.bits.setflags(write=False)
        self.recs = []
        for pk in self.pk:
            r = np.zeros(len(pk), dtype=PACKET_DTYPE)
            for k, p in enumerate(pk):
                r[k]["call"], r[k]["index"], r[k]["nbytes"] = p.call, p.index, p.data.size
                r[k]["data"][: p.data.size] = p.data
                r[k]["rssi"], r[k]["snr"] = p.rssi, p.snr
            self.recs.append(r)
        self.counts = np.array([len(r) for r in self.recs], dtype=np.int64)
        self.all_recs = np.concatenate(self.recs)
        self.all_recs.setflags(write=False)
        hi = last_position()
        self.raw_matches = np.array(
            [sum(1 for p in O.search(np.unpackbits(b, bitorder="little")[:N_SAMPLES], cfg) if p <= hi) for b in self.bits],
            dtype=np.int64)
        self.calls = [O.parse_calls([s[2 * B * b: 2 * B * (b + 1)] for b in range(N_BLOCKS)], cfg) for s in self.raw]


@functools.lru_cache(maxsize=None)
def cases():
    return Cases()


def sources(n_streams):
    """Row of Cases.raw that batch stream s holds."""
    s = np.arange(n_streams)
    src = s % U
    quiet = (s >= QUIET.start) & (s < QUIET.stop)
    src[quiet] = U + s[quiet] - QUIET.start
    return src


def batch_input(n_streams):
    return cases().raw[sources(n_streams)]


def expected_records(n_streams):
    """The whole batch's records in the order results() must have: stream-major, the oracle's order inside a stream."""
    c = cases()
    src = sources(n_streams)
    cnt = c.counts[src]
    first_src = np.concatenate([[0], np.cumsum(c.counts)])[:-1]     # a source's first record in all_recs
    first_out = np.concatenate([[0], np.cumsum(cnt)])[:-1]          # a stream's first record in the batch
    idx = np.repeat(first_src[src] - first_out, cnt) + np.arange(int(cnt.sum()))
    out = c.all_recs[idx]
    out["stream"] = np.repeat(np.arange(n_streams, dtype=np.int32), cnt)
    return out


def expected_rows(n_streams):
    """parsed() of the whole batch as parse_gate_cases.parsed_rows gives it."""
    per = [[r[1:] for rows in message_rows(calls) for r in rows] for calls in cases().calls]
    return [(int(s),) + r for s, k in enumerate(sources(n_streams)) for r in per[k]]


def expected_matches(n_streams):
    return int(cases().raw_matches[sources(n_streams)].sum())


def group_totals(n_streams):
    """Records per group of four streams."""
    cnt = cases().counts[sources(n_streams)]
    pad = (-n_streams) % GROUP
    return np.concatenate([cnt, np.zeros(pad, dtype=cnt.dtype)]).reshape(-1, GROUP).sum(axis=1)


def bits_streams(n_streams):
    """Streams whose bits the device test reads back: groups 0, 1023, 1024, 1025 and the last, and every 97th."""
    last = (n_streams - 1) // GROUP
    pick = set(range(0, n_streams, 97))
    for g in (0, ROUND - 1, ROUND, ROUND + 1, last):
        pick.update(s for s in range(GROUP * g, GROUP * g + GROUP) if s < n_streams)
    return sorted(pick)


# ---------------------------------------------------------------------------------------------- the comparison
def assert_records_equal(got, want, what="", db_tol=1e-3):
    """Two rd_packet arrays as a whole and in order: stream, call, index, nbytes and bytes equal, rssi and snr within
    db_tol.  The message names the first record that differs and the groups involved."""
    def where(bad):
        i = int(np.flatnonzero(bad)[0])
        g, w = got[i], want[i]
        return (f"{what}: {int(bad.sum())} records differ, the first is record {i}: got stream {g['stream']} (group "
                f"{g['stream'] // GROUP}) call {g['call']} index {g['index']}, want stream {w['stream']} (group "
                f"{w['stream'] // GROUP}) call {w['call']} index {w['index']}")

    n = min(len(got), len(want))
    for f in ("stream", "call", "index", "nbytes"):
        bad = got[f][:n] != want[f][:n]
        assert not bad.any(), f"{f}: " + where(bad)
    bad = (got["data"][:n] != want["data"][:n]).any(axis=1)
    assert not bad.any(), "data: " + where(bad)
    assert len(got) == len(want), f"{what}: {len(got)} records, want {len(want)} (the first {n} agree)"
    for f in ("rssi", "snr"):
        a, e = got[f], want[f]
        bad = ~((np.abs(a - e) <= db_tol) | (np.isnan(a) & np.isnan(e)))
        assert not bad.any(), f"{f}: " + where(bad) + f", worst {np.nanmax(np.abs(a - e))}"
