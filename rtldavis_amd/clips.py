"""From the receiver's burst clips to recordings every SDR tool reads.  Pure Python and NumPy: nothing here touches the
library or a device.

``WidebandReceiver.set_burst_clips`` makes the device cut the channelized IQ of every burst out of each chunk.  The
clips of one burst overlap (its run, its decoded row, a searched row of the same packet each get their own copy) and a
burst that crosses a chunk boundary continues in the next chunk's tail clip.  ``ClipStitcher`` merges the clips of a
channel whose output ranges overlap or abut into one ``Recording``; ``write_sigmf`` stores a recording as SigMF ``cu8``,
which is exactly the channelized bytes, and ``read_sigmf`` reads it back.

    st = ClipStitcher(rx.block_size)
    while ...:
        rx.submit(chunk); rx.fetch()
        c = rx.burst_clips()
        for rec in st.add(c, c.chunk * rx.block_size):
            write_sigmf(f"burst_{rec.channel}_{rec.time}", rec, rx.out_rate, centre_hz + shift_hz[rec.channel])
    for rec in st.flush(): ...
"""
from __future__ import annotations

import json
from typing import List, NamedTuple, Tuple

import numpy as np

SIGMF_VERSION = "1.0.0"


class Recording(NamedTuple):
    """One stretch of one channel's output stream: ``iq`` (uint8 [n, 2]) holds outputs ``time .. time + n - 1`` on the
    receiver's absolute output clock; ``refs`` lists ``(source, ref)`` of every clip merged into it, in the order they
    came - ``ref`` is a message row's ``time`` (sources 2, 3, 4), a run's ``first`` (1) or 0 (a tail)."""
    channel: int
    time: int
    iq: np.ndarray
    refs: Tuple[Tuple[int, int], ...]


def _merge(pieces):
    """[(time, iq, refs)] that form one connected stretch -> (time, iq, refs); ValueError where two copies differ."""
    t0 = min(p[0] for p in pieces)
    t1 = max(p[0] + len(p[1]) for p in pieces)
    iq = np.zeros((t1 - t0, 2), np.uint8)
    filled = np.zeros(t1 - t0, bool)
    refs = []
    for t, a, r in pieces:
        lo, hi = t - t0, t - t0 + len(a)
        both = filled[lo:hi]
        if both.any() and not np.array_equal(iq[lo:hi][both], a[both]):
            at = t + int(np.flatnonzero(both & (iq[lo:hi] != a).any(axis=1))[0])
            raise ValueError(f"two clips disagree at output {at}: they are not copies of the same stream")
        iq[lo:hi] = a
        filled[lo:hi] = True
        refs.extend(r)
    return t0, iq, refs


class ClipStitcher:
    """Merges the clips of successive chunks into recordings.  ``add(clips, clock)`` takes one chunk's ``BurstClips`` (or
    anything with ``records`` of ``CLIP_DTYPE`` and ``iq``) and ``clock``, the absolute output clock of that chunk's
    first output (``chunk * block_size`` for a receiver that was never reset mid-run), and returns the recordings that
    are complete.  Chunk j's clips begin at or after ``K_j - block_size`` and every later chunk's at or after ``K_j``, so
    after chunk j a recording that ends before ``K_j`` can no longer grow and is handed out; one that ends at ``K_j`` or
    later waits.  ``flush()`` hands out the rest.  Clips of one channel whose ranges ``[time, time + n)`` overlap or abut
    become one recording; where they overlap they are copies of the same stream and must be identical - a difference is a
    ``ValueError``."""

    def __init__(self, block_size: int):
        if int(block_size) < 1:
            raise ValueError("block_size must be positive")
        self.block_size = int(block_size)
        self._open = {}                       # channel -> [(time, iq, refs)], disjoint and not abutting, by time

    def add(self, clips, clock: int) -> List[Recording]:
        clock = int(clock)
        recs, iq = clips.records, np.asarray(clips.iq).reshape(-1, 2)
        for r in recs:
            ch, t, n, off = int(r["channel"]), int(r["time"]), int(r["n"]), int(r["offset"])
            if t < clock - self.block_size:
                raise ValueError(f"a clip of channel {ch} begins at {t}, more than a chunk before the clock {clock}")
            piece = (t, iq[off: off + n], [(int(r["source"]), int(r["ref"]))])
            if len(piece[1]) != n:
                raise ValueError(f"clip at offset {off} with {n} outputs lies outside the {len(iq)} outputs given")
            segs = self._open.setdefault(ch, [])
            touch = [s for s in segs if s[0] <= t + n and t <= s[0] + len(s[1])]
            rest = [s for s in segs if not (s[0] <= t + n and t <= s[0] + len(s[1]))]
            rest.append(_merge(touch + [piece]))
            rest.sort(key=lambda s: s[0])
            self._open[ch] = rest
        return self._hand_out(lambda s: s[0] + len(s[1]) < clock)

    def flush(self) -> List[Recording]:
        return self._hand_out(lambda s: True)

    def _hand_out(self, done) -> List[Recording]:
        out = []
        for ch in sorted(self._open):
            keep = []
            for s in self._open[ch]:
                if done(s):
                    out.append(Recording(ch, s[0], s[1], tuple(s[2])))
                else:
                    keep.append(s)
            self._open[ch] = keep
        return out


def _message_fields(m):
    try:
        return int(m["time"]), bytes(bytearray(np.asarray(m["data"], np.uint8).tolist()))
    except (KeyError, IndexError, ValueError, TypeError):
        t, d = m
        return int(t), bytes(d)


def write_sigmf(base: str, recording: Recording, sample_rate: float, frequency_hz: float, messages=(),
                symbol_length: int = 14, packet_symbols: int = 80) -> None:
    """``base.sigmf-data``: the recording's bytes as they are (``cu8``: I, Q per output).  ``base.sigmf-meta``: the
    global object (``core:datatype``, ``core:sample_rate``, ``core:version``, ``rtldavis:channel``, ``rtldavis:time`` - the
    absolute output clock of sample 0), one capture (``core:sample_start`` 0, ``core:frequency``) and one annotation per
    message that lies in the recording: ``core:sample_start`` / ``core:sample_count`` are the packet's first output
    ``time - symbol_length + 1`` relative to the recording and its ``packet_symbols * symbol_length`` outputs (cut to the
    recording), ``core:comment`` the on-air bytes as hex.  ``messages``: rows of ``BURST_MSG_DTYPE`` (or ``(time, data)``
    pairs) of the recording's channel.

    ``frequency_hz`` is the caller's: ``centre_hz + shift_hz[c]`` of the tuning in force when the chunk was submitted,
    the RF frequency the channelizer moved to 0 Hz of the bytes.  The channel's nominal frequency is NOT at 0 Hz there:
    the carrier sits at the receiver's intermediate frequency ``if_hz`` (``WidebandReceiver.if_hz``, ``-out_rate // 4``
    by default) plus the station's own offset, so a viewer shows the burst ``if_hz`` away from ``core:frequency``."""
    iq = np.ascontiguousarray(recording.iq, np.uint8).reshape(-1, 2)
    n = len(iq)
    ann = []
    for m in messages:
        t, data = _message_fields(m)
        a = t - int(symbol_length) + 1 - int(recording.time)
        e = a + int(packet_symbols) * int(symbol_length)
        a, e = max(a, 0), min(e, n)
        if e > a:
            ann.append({"core:sample_start": a, "core:sample_count": e - a, "core:comment": data.hex()})
    meta = {"global": {"core:datatype": "cu8", "core:sample_rate": float(sample_rate), "core:version": SIGMF_VERSION,
                       "rtldavis:channel": int(recording.channel), "rtldavis:time": int(recording.time),
                       "rtldavis:refs": [[int(s), int(r)] for s, r in recording.refs]},
            "captures": [{"core:sample_start": 0, "core:frequency": float(frequency_hz)}],
            "annotations": ann}
    with open(base + ".sigmf-data", "wb") as f:
        f.write(iq.tobytes())
    with open(base + ".sigmf-meta", "w", encoding="utf-8") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


def read_sigmf(base: str):
    """``(Recording, meta)`` of a pair written by ``write_sigmf``: the bytes back as uint8 [n, 2] and the metadata as a dict.
    ValueError for another datatype."""
    with open(base + ".sigmf-meta", encoding="utf-8") as f:
        meta = json.load(f)
    g = meta["global"]
    if g.get("core:datatype") != "cu8":
        raise ValueError(f"{base}.sigmf-meta: datatype {g.get('core:datatype')!r}, not 'cu8'")
    iq = np.fromfile(base + ".sigmf-data", np.uint8)
    if iq.size % 2:
        raise ValueError(f"{base}.sigmf-data: an odd number of bytes")
    refs = tuple((int(s), int(r)) for s, r in g.get("rtldavis:refs", []))
    return Recording(int(g.get("rtldavis:channel", 0)), int(g.get("rtldavis:time", 0)), iq.reshape(-1, 2), refs), meta
