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
tiles a long recording with jobs instead."""
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
