"""Decode recorded burst clips on the device: the batch replay decoder (include/rtldavis_hip.h, CLIP DECODE).

``WidebandReceiver.set_burst_clips`` and ``rtldavis_amd.clips`` bring the channelized IQ of every burst home as
``Recording``s.  ``ClipDecoder`` asks of such bytes what a live chunk can be asked only once: would this burst have decoded
with the narrow-band filter on, with one or two flips, around another direction?  It takes channel-rate bytes directly -
no receiver, no channelizer - and decodes thousands of clips per launch with the kernels' own steps: the off-frequency
slicer, the CRC repair and the narrow-band filter of the burst decoders.

    dec = ClipDecoder(cfg)
    recs = [read_sigmf(base)[0] for base in bases]
    plain, best = dec.decode(recs, forms=((0, False), (2, True)))     # own direction: each clip's mean frequency
    for row, k in zip(best.records, best.recording): ...

A *pool* is a flat byte array of clips, a *job* (``CLIP_JOB_DTYPE``) names one clip in it - ``n`` outputs from output
``offset``, a multiple of 8 - and the range ``tau_lo .. tau_hi`` of candidate positions to test (at most ``MAX_SPAN`` wide,
relative to the clip's output 0), the direction ``corr`` to slice around ((0, 0): the clip's own, the sum of
``z[t] conj(z[t-1])`` over the job's region) and the transmitter id to accept.  A job gives at most one row; ``plan``
tiles a long recording with jobs instead.

``ClipDecoder.synthesize`` fills the pool on the device instead (CLIP SYNTH): one *spec* (``SPEC_DTYPE``) per clip - a burst
of up to 192 symbols at an integer carrier and deviation, an amplitude, a noise level and a 64-bit seed - and no host
bytes; ``burst_specs`` writes the specs of Davis bursts in the units of ``synth.synth_bursts``.  The same specs give the
same pool on every machine: tests/clip_synth_cases.py holds the NumPy model, bit for bit.

    specs, tau = burst_specs(payloads, n=2048, at=300, seed=1, amplitude=0.3, noise=0.2)
    dec.synthesize(specs)
    jobs = centred_jobs(specs, tau, span=64)
    got = dec.decode_jobs(jobs, max_flips=2, narrow=True)"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .dsp import _cfg_struct
from .wideband import BURST_MSG_DTYPE

CLIP_JOB_DTYPE = np.dtype([("offset", np.uint64), ("clock", np.uint64), ("n", np.uint32), ("id", np.uint32),
                           ("tau_lo", np.int32), ("tau_hi", np.int32), ("corr_re", np.int32), ("corr_im", np.int32),
                           ("channel", np.int32), ("pad", np.uint32)])
CD_HEADER_DTYPE = np.dtype([("n_msgs", np.uint32), ("candidates", np.uint32), ("ca", np.int32), ("cb", np.int32)])
SPEC_DTYPE = np.dtype([("offset", np.uint64), ("seed", np.uint64), ("n", np.uint32), ("at", np.int32), ("phase0", np.uint32),
                       ("f_c", np.int32), ("f_d", np.uint32), ("amp_q", np.uint32), ("noise_q", np.uint32), ("n_sym", np.uint32),
                       ("pre", np.uint16), ("post", np.uint16), ("pad", np.uint32), ("bits", np.uint8, (24,))])
assert SPEC_DTYPE.itemsize == 80
MAX_SYM = 192                          # symbols of a spec at most
MAX_PRE = 4096                         # ``pre``, ``post`` at most
MAX_N = 1 << 24                        # outputs of a synthesised clip at most
MAX_SPECS = 1 << 20                    # specs per call of ``synthesize``
MAX_AMP_Q = 1 << 16                    # ``amp_q`` at most: 256 bytes
MAX_NOISE_Q = 1 << 20                  # ``noise_q`` at most: sigma of 73.9 bytes
FULL_SCALE = 127.6                     # bytes per unit of ``synth.synth_bursts``' amplitude and noise
NOISE_SIGMA = math.sqrt(16 * 65535 / 12.0) / 2 ** 22     # sigma in bytes per unit of ``noise_q``
REPLAYED = 32                          # ``flags`` bit 5: a row of the clip decoder, ``first`` is the job's index
MAX_SPAN = 2048                        # ``tau_hi - tau_lo`` at most
MAX_JOBS = 1 << 20                     # jobs per call of ``decode_jobs``
ANY_ID = 0xFF
FORMS = tuple((r, nb) for nb in (False, True) for r in (0, 1, 2))     # (max_flips, narrow): the six forms


class Replay(NamedTuple):
    """``ClipDecoder.decode_jobs``: row ``j`` of each is job ``j``.  ``records`` (``BURST_MSG_DTYPE``; all zero where the job
    gave no message), ``headers`` (``CD_HEADER_DTYPE``: ``n_msgs`` 0 / 1, ``candidates`` - 0 for an idle job -, ``ca, cb``
    the direction that was used) and ``soft`` (int64 [jobs, packet_symbols]: the winner's symbol sums before any flip,
    zeros without a message; ``None`` unless asked for)."""
    records: np.ndarray
    headers: np.ndarray
    soft: Optional[np.ndarray]


class ReplayedMessages(NamedTuple):
    """One form's result of ``ClipDecoder.decode``: ``records`` (``BURST_MSG_DTYPE``, the rows with a message after the
    drop of repeats, in job order), ``recording`` (for each row the index of its recording in the list given) and
    ``form`` = ``(max_flips, narrow)``."""
    records: np.ndarray
    recording: np.ndarray
    form: Tuple[int, bool]


def _iq(rec) -> np.ndarray:
    a = np.asarray(getattr(rec, "iq", rec))
    if a.dtype != np.uint8 or a.size == 0 or a.size % 2:
        raise ValueError("a clip is a non-empty uint8 array of I, Q pairs")
    return np.ascontiguousarray(a).reshape(-1)


def pack(recordings) -> Tuple[np.ndarray, np.ndarray]:
    """``(pool, offsets)``: the recordings' bytes (``Recording``s, or uint8 arrays ``[n, 2]`` / flat) one behind the other
    in a flat uint8 pool, each clip beginning at the next multiple of 8 outputs; ``offsets`` (int64) in outputs.  The
    slack between two clips is zero - and takes no part in any result."""
    clips = [_iq(r) for r in recordings]
    if not clips:
        raise ValueError("no recordings")
    offsets = np.zeros(len(clips), np.int64)
    at = 0
    for k, c in enumerate(clips):
        offsets[k] = at
        at = (at + c.size // 2 + 7) // 8 * 8
    pool = np.zeros(2 * int(offsets[-1]) + clips[-1].size, np.uint8)
    for o, c in zip(offsets, clips):
        pool[2 * int(o): 2 * int(o) + c.size] = c
    return pool, offsets


def plan(n: int, symbol_length: int, packet_symbols: int, span: int = MAX_SPAN) -> List[Tuple[int, int]]:
    """The ranges ``(tau_lo, tau_hi)``, inclusive and ascending, that tile the candidate positions of a clip of ``n``
    outputs - ``symbol_length .. n - 1 - symbol_length * (packet_symbols - 1)`` - exactly once each, every range at most
    ``span`` wide (``tau_hi - tau_lo <= span``).  Empty for a clip shorter than ``packet_symbols * symbol_length + 1``."""
    n, sl, ns, span = int(n), int(symbol_length), int(packet_symbols), int(span)
    if sl < 1 or ns < 1 or not 0 <= span <= MAX_SPAN:
        raise ValueError(f"symbol_length and packet_symbols must be positive and span in 0 .. {MAX_SPAN}")
    last = n - 1 - sl * (ns - 1)
    return [(lo, min(lo + span, last)) for lo in range(sl, last + 1, span + 1)]


def drop_repeats(records: np.ndarray, recording: np.ndarray, symbol_length: int) -> np.ndarray:
    """Step 7' for replayed rows, which arrive in job order: the indices of the rows to keep.  A row is dropped when an
    earlier kept row of the same recording has its channel and data and a time less than ``symbol_length`` away on the
    64-bit clock - two adjacent ranges of ``plan`` can each report one of a packet's adjacent valid positions."""
    keep: List[int] = []
    sl = int(symbol_length)
    for i, r in enumerate(records):
        again = False
        for k in keep:
            q = records[k]
            if int(recording[k]) != int(recording[i]) or int(q["channel"]) != int(r["channel"]):
                continue
            d = (int(r["time"]) - int(q["time"])) % 2 ** 64
            if min(d, 2 ** 64 - d) < sl and bytes(q["data"]) == bytes(r["data"]):
                again = True
                break
        if not again:
            keep.append(i)
    return np.asarray(keep, np.int64)


def _per_clip(value, n, what, dtype=np.float64):
    a = np.asarray(value, dtype)
    if a.ndim > 1 or (a.ndim == 1 and a.size != n):
        raise ValueError(f"{what}: one value, or one per clip")
    return np.broadcast_to(a, (n,))


def burst_specs(payloads, *, n, at, seed, amplitude, noise, offset_hz=0.0, lead_symbols=32, trail_symbols=8, pre=0, post=0,
                phase0=None, count=None, symbol_length=14, bit_rate=19200, if_hz=None):
    """``(specs, tau)``: one spec (``SPEC_DTYPE``) per payload - on-air bytes, as ``synth.make_packet`` gives them (a list of
    bytes or hex strings, or a uint8 array [clips, bytes]) - for clips
    of ``n`` outputs at consecutive multiples of 8 of a pool, each with ``synth.synth_bursts``' burst: ``lead_symbols``
    alternating symbols 1 0 1 0 .., the payload's bits MSB first, ``trail_symbols`` zeros, at ``if_hz + offset_hz`` +- a
    quarter of the bit rate, with ``pre`` / ``post`` outputs of plain carrier around them.  The lead-in begins at output
    ``at`` of the clip (may lie outside it); ``tau`` (int64) is where the decoder reports the packet: the last output of the
    payload's first symbol, ``at + (lead_symbols + 1) symbol_length - 1``.  ``amplitude`` and ``noise`` (sigma per
    component) are in ``synth_bursts``' units, full scale ``FULL_SCALE`` bytes.  ``seed``: an integer - the clips' 64-bit
    noise seeds and, with ``phase0=None``, their start phases are drawn from ``numpy.random.default_rng(seed)`` - or an
    array of one seed per clip.  ``at``, ``offset_hz``, ``amplitude``, ``noise``, ``phase0``: one value, or one per clip.
    ``payloads=None``: ``count`` noise-only clips (no burst, amplitude 0).  ``if_hz``: default ``-out_rate // 4``, the
    channelizer's.  ValueError for what ``rd_cs_check_specs`` would refuse."""
    sl = int(symbol_length)
    out_rate = int(bit_rate) * sl
    if payloads is None:
        if count is None or int(count) < 1:
            raise ValueError("noise-only clips: give their count")
        k, rows = int(count), None
        lead_symbols = trail_symbols = 0
        amplitude = 0.0
    else:
        if isinstance(payloads, np.ndarray) and payloads.dtype == np.uint8 and payloads.ndim == 2:
            rows = payloads                                   # [clips, bytes]
        else:
            rows = [bytes.fromhex(p) if isinstance(p, str) else bytes(p) for p in payloads]
            if not rows or not rows[0] or any(len(r) != len(rows[0]) for r in rows):
                raise ValueError("payloads: at least one, all of one length")
            rows = np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1)
        k = int(rows.shape[0])
    if not 1 <= k <= MAX_SPECS:
        raise ValueError(f"{k} clips, not 1 .. {MAX_SPECS}")
    n, pre, post = int(n), int(pre), int(post)
    n_sym = 0 if rows is None else int(lead_symbols) + 8 * int(rows.shape[1]) + int(trail_symbols)
    if not 1 <= n <= MAX_N or not 0 <= pre <= MAX_PRE or not 0 <= post <= MAX_PRE or sl < 1:
        raise ValueError(f"n in 1 .. {MAX_N}, pre and post in 0 .. {MAX_PRE}, symbol_length >= 1")
    if int(lead_symbols) < 0 or int(trail_symbols) < 0 or n_sym > MAX_SYM:
        raise ValueError(f"a burst of {n_sym} symbols, at most {MAX_SYM}")
    at_a = _per_clip(at, k, "at", np.int64)
    if np.any(np.abs(at_a) > 2 ** 30):
        raise ValueError("at: -2**30 .. 2**30")
    amp_q = np.rint(_per_clip(amplitude, k, "amplitude") * (FULL_SCALE * 256.0))
    noise_q = np.rint(_per_clip(noise, k, "noise") * (FULL_SCALE / NOISE_SIGMA))
    if np.any(amp_q < 0) or np.any(amp_q > MAX_AMP_Q) or np.any(noise_q < 0) or np.any(noise_q > MAX_NOISE_Q):
        raise ValueError(f"amplitude in 0 .. {MAX_AMP_Q / 256 / FULL_SCALE:.3f}, noise in 0 .. {MAX_NOISE_Q * NOISE_SIGMA / FULL_SCALE:.3f}")
    centre = float(-out_rate // 4 if if_hz is None else if_hz)
    f_c = np.rint((centre + _per_clip(offset_hz, k, "offset_hz")) / out_rate * 2.0 ** 32).astype(np.int64)
    seeds = np.asarray(seed)
    rng = None
    if seeds.ndim == 0:
        rng = np.random.default_rng(int(seed))
        seeds = rng.integers(0, 2 ** 64, k, dtype=np.uint64)
    elif seeds.shape != (k,):
        raise ValueError("seed: an integer, or one seed per clip")
    if phase0 is None:
        ph = (rng or np.random.default_rng(0)).integers(0, 2 ** 32, k, dtype=np.uint64)
    else:
        ph = _per_clip(phase0, k, "phase0", np.int64) % 2 ** 32
    specs = np.zeros(k, SPEC_DTYPE)
    specs["offset"] = np.arange(k, dtype=np.uint64) * np.uint64((n + 7) // 8 * 8)
    specs["seed"] = seeds.astype(np.uint64)
    specs["n"], specs["at"], specs["phase0"] = n, at_a, ph.astype(np.uint32)
    specs["f_c"] = ((f_c + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)
    specs["f_d"] = int(round(2.0 ** 32 / (4 * sl))) if rows is not None else 0
    specs["amp_q"], specs["noise_q"] = amp_q.astype(np.uint32), noise_q.astype(np.uint32)
    specs["n_sym"], specs["pre"], specs["post"] = n_sym, pre, post
    if rows is not None:
        sym = np.zeros((k, MAX_SYM), np.uint8)
        sym[:, 0:int(lead_symbols):2] = 1
        sym[:, int(lead_symbols): int(lead_symbols) + 8 * int(rows.shape[1])] = np.unpackbits(rows, axis=1)
        specs["bits"] = np.packbits(sym, axis=1)
    return specs, at_a + (int(lead_symbols) + 1) * sl - 1


def centred_jobs(specs, tau, span: int = 64, corr=(0, 0), ident: int = ANY_ID) -> np.ndarray:
    """One job (``CLIP_JOB_DTYPE``) per spec over ``tau - span // 2 .. tau - span // 2 + span``, the planted position in the
    middle; ``corr``: one direction for all, or one ``(re, im)`` per spec; ``channel`` is the spec's index modulo 2**31."""
    specs = np.asarray(specs, SPEC_DTYPE).reshape(-1)
    span = int(span)
    if not 0 <= span <= MAX_SPAN:
        raise ValueError(f"span in 0 .. {MAX_SPAN}")
    c = np.broadcast_to(np.asarray(corr, np.int64), (specs.size, 2))
    jobs = np.zeros(specs.size, CLIP_JOB_DTYPE)
    jobs["offset"], jobs["n"], jobs["id"] = specs["offset"], specs["n"], int(ident)
    jobs["tau_lo"] = np.asarray(tau, np.int64) - span // 2
    jobs["tau_hi"] = jobs["tau_lo"] + span
    jobs["corr_re"], jobs["corr_im"] = c[:, 0], c[:, 1]
    jobs["channel"] = np.arange(specs.size) % 2 ** 31
    return jobs


def _per_recording(value, n, what):
    if value is None:
        return [None] * n
    a = np.asarray(value)
    if a.ndim == (1 if what == "corr" else 0):
        return [value] * n
    if len(value) != n:
        raise ValueError(f"{what}: one value, or one per recording")
    return list(value)


class ClipDecoder:
    """``ClipDecoder(cfg)``: the batch decoder for clips of a packet configuration ``cfg`` (``block_size`` is ignored).
    ``if_hz``: where a channel's centre lies in its bytes, for ``offset_hz``; default ``-out_rate // 4``, the
    channelizer's.  Creating one touches no device; the first ``upload`` does."""

    def __init__(self, cfg, if_hz: Optional[int] = None) -> None:
        self.cfg = cfg
        self._h = C.c_void_p()
        self.symbol_length = int(cfg.symbol_length)
        self.packet_symbols = int(cfg.packet_symbols)
        self.out_rate = int(cfg.bit_rate) * self.symbol_length
        self.if_hz = -self.out_rate // 4 if if_hz is None else int(if_hz)
        self.pool_outputs = 0
        _lib.check(_lib.lib().rd_clips_create(C.byref(_cfg_struct(cfg)), C.byref(self._h)))

    def __del__(self):
        try:
            if self._h:
                _lib.lib().rd_clips_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def corr(self, offset_hz: float) -> Tuple[int, int]:
        """``round(2**14 e^{j 2 pi (if_hz + offset) / out_rate})`` as ``(re, im)``, as ``track.Tracker.corr``."""
        a = 2.0 * math.pi * (float(self.if_hz) + float(offset_hz)) / float(self.out_rate)
        return int(round(16384.0 * math.cos(a))), int(round(16384.0 * math.sin(a)))

    def upload(self, pool) -> None:
        """Copy a pool (uint8, I, Q per output) to the device; it stays there until the next ``upload``."""
        a = np.asarray(pool)
        if a.dtype != np.uint8:
            raise ValueError("a pool is a uint8 array of I, Q pairs")
        a = np.ascontiguousarray(a).reshape(-1)
        self.pool_outputs = 0
        _lib.check(_lib.lib().rd_clips_upload(self._h, a.ctypes.data, a.nbytes))
        self.pool_outputs = a.size // 2

    def synthesize(self, specs, pool_outputs: Optional[int] = None) -> None:
        """Fill the device pool from ``specs`` (``SPEC_DTYPE``, ascending and apart) with no host bytes: a pool of
        ``pool_outputs`` outputs - default: the last clip's end rounded up to 8 - in which every byte outside a clip is 0.
        It takes the place of an uploaded pool.  ValueError for what the library refuses; the pool before stays then."""
        s = np.ascontiguousarray(specs, SPEC_DTYPE).reshape(-1)
        if pool_outputs is None:
            pool_outputs = (int(s["offset"][-1]) + int(s["n"][-1]) + 7) // 8 * 8 if s.size else 0
        pool_outputs = int(pool_outputs)
        if not 0 <= pool_outputs < 2 ** 64:
            raise ValueError("pool_outputs: 0 .. 2**64 - 1")
        rc = _lib.lib().rd_clips_synth(self._h, s.ctypes.data, int(s.size), pool_outputs)
        if rc != _lib.RD_OK and rc != _lib.RD_ERR_ARG:
            self.pool_outputs = 0                             # (a refusal touched nothing; a device error leaves no pool)
        _lib.check(rc)
        self.pool_outputs = pool_outputs

    def download(self) -> np.ndarray:
        """The pool as the device holds it (uint8, 2 pool_outputs), uploaded or synthesised.  RuntimeError without one."""
        out = np.empty(2 * max(int(self.pool_outputs), 1), np.uint8)
        _lib.check(_lib.lib().rd_clips_download(self._h, out.ctypes.data, 2 * int(self.pool_outputs)))
        return out

    def synth_ms(self) -> float:
        """The device time of the last ``synthesize`` - the zeroing of the pool and the kernel -, by device events, in ms."""
        ms = C.c_float()
        _lib.check(_lib.lib().rd_clips_synth_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def decode_jobs(self, jobs, max_flips: int = 0, narrow: bool = False, soft: bool = False) -> Replay:
        """One launch over ``jobs`` (``CLIP_JOB_DTYPE``) on the uploaded pool, under one form.  ValueError for a job or a
        form the library refuses (nothing is launched then), RuntimeError before any ``upload``."""
        j = np.ascontiguousarray(jobs, CLIP_JOB_DTYPE).reshape(-1)
        n = max(int(j.size), 1)
        recs = np.zeros(n, BURST_MSG_DTYPE)
        hdr = np.zeros(n, CD_HEADER_DTYPE)
        sv = np.zeros((n, self.packet_symbols), np.int64) if soft else None
        _lib.check(_lib.lib().rd_clips_decode(self._h, j.ctypes.data, int(j.size), int(max_flips), int(bool(narrow)),
                                              recs.ctypes.data, hdr.ctypes.data, sv.ctypes.data if soft else None))
        return Replay(recs, hdr, sv)

    def kernel_ms(self) -> float:
        """The kernel time of the last ``decode_jobs``, by device events, in milliseconds."""
        ms = C.c_float()
        _lib.check(_lib.lib().rd_clips_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def jobs_for(self, recordings, offsets, corr=None, ident=None, span: int = MAX_SPAN):
        """``(jobs, recording)``: the jobs that tile every recording by ``plan`` - ``recording[j]`` is job ``j``'s index in
        the list -, each recording's ``channel`` and ``time`` (0 for a bare array) in its jobs."""
        recordings = list(recordings)
        corrs = _per_recording(corr, len(recordings), "corr")
        ids = _per_recording(ident, len(recordings), "ident")
        rows, owner = [], []
        for k, rec in enumerate(recordings):
            n = _iq(rec).size // 2
            c = (0, 0) if corrs[k] is None else (int(corrs[k][0]), int(corrs[k][1]))
            i = ANY_ID if ids[k] is None else int(ids[k])
            for lo, hi in plan(n, self.symbol_length, self.packet_symbols, span):
                rows.append((int(offsets[k]), int(getattr(rec, "time", 0)) % 2 ** 64, n, i, lo, hi, c[0], c[1],
                             int(getattr(rec, "channel", 0)), 0))
                owner.append(k)
        return np.asarray(rows, CLIP_JOB_DTYPE).reshape(-1), np.asarray(owner, np.int64)

    def decode(self, recordings, *, offset_hz=None, corr=None, ident=None,
               forms: Sequence[Tuple[int, bool]] = ((0, False),)) -> List[ReplayedMessages]:
        """Pack the recordings, tile each with ``plan`` and run every form of ``forms`` - ``(max_flips, narrow)`` pairs - on
        one upload; per form the rows with a message, after ``drop_repeats``.  ``offset_hz`` (the carrier's offset from the
        channel's centre, turned into a direction by ``corr()``) or ``corr`` ``(re, im)``, one for all or one per recording;
        neither: each job slices around its own region's direction.  ``ident``: only messages of this transmitter.  The rows
        go as they are into ``acquire.burst_message_offset_hz``, ``acquire.repaired``, ``acquire.flipped_symbols`` and
        ``write_sigmf(messages=...)``."""
        recordings = list(recordings)
        if offset_hz is not None and corr is not None:
            raise ValueError("offset_hz or corr, not both")
        if offset_hz is not None:
            corr = [self.corr(f) for f in _per_recording(offset_hz, len(recordings), "offset_hz")]
        pool, offsets = pack(recordings)
        jobs, owner = self.jobs_for(recordings, offsets, corr, ident)
        out = []
        if jobs.size:
            self.upload(pool)
        for r, nb in forms:
            if not jobs.size:
                out.append(ReplayedMessages(np.zeros(0, BURST_MSG_DTYPE), np.zeros(0, np.int64), (int(r), bool(nb))))
                continue
            rows = []
            for a in range(0, jobs.size, MAX_JOBS):
                got = self.decode_jobs(jobs[a: a + MAX_JOBS], r, nb)
                hit = np.flatnonzero(got.headers["n_msgs"] == 1)
                part = got.records[hit]
                part["first"] += np.uint32(a)             # the job's index in the whole list
                rows.append((part, owner[a + hit]))
            recs = np.concatenate([p for p, _ in rows])
            own = np.concatenate([o for _, o in rows])
            keep = drop_repeats(recs, own, self.symbol_length)
            out.append(ReplayedMessages(recs[keep], own[keep], (int(r), bool(nb))))
        return out
