"""Station tracking for ``wideband.WidebandReceiver``: the host policy on top of ``set_burst_expect``.

A Davis station is predictable once it has been heard: its next channel follows from its hop pattern, its next packet
comes one dwell period later to within tens of outputs, and its carrier offset - a property of the transmitter and the
receiver's reference - does not change from hop to hop.  The reference's ``Hopper`` uses this to retune a narrow-band
SDR; a wideband receiver sees every channel already and uses the same facts to decode at the expected place with no
energy gate (include/rtldavis_hip.h, BURST EXPECT), and to say which packets of a station were MISSED::

    rx.set_bursts(True); rx.set_burst_decode(True)
    trk = Tracker(rx.cfg, hop_pattern)              # channel indices of the receiver, in the station's hop order
    clock = 0
    for chunk in chunks:
        rx.set_burst_expect(trk.table(clock, rx.block_size))
        rx.demodulate(chunk)                        # submit + fetch
        clock += rx.block_size
        trk.observe(rx.burst_messages().records)
        trk.observe(rx.expected_messages().records)

A station never yet heard and too weak for a run is found by the blind search (``set_burst_search``, BURST SEARCH), whose
rows prove less than any other: with every position of every channel tested, sync word and CRC pass by chance every few
minutes per centre.  The acquisition loop is therefore ``search -> provisional -> expectation -> promoted``: feed
``rx.searched_messages()`` to ``observe`` as well; a searched row of an unknown id seeds a PROVISIONAL station, which gets
expectations like any other, is promoted by the first row of another path that ``observe`` accepts for it, and is dropped
quietly after ``provisional_missed`` misses in a row.

``hop_pattern`` is the caller's: this package holds no station's table.  Rows of ``parsed()`` carry no clock, so a
tracker cannot be fed from them alone; that is out of scope here.

Pure Python on the records' integers: the same rows give the same tables, on any machine; nothing here touches a device.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import numpy as np

from . import acquire

EXPECT_MAX = 64                  # wideband.BURST_EXPECT_MAX
EXPECT_MAX_SPAN = 2048           # wideband.BURST_EXPECT_MAX_SPAN
# the layout of rd_expect (wideband.EXPECT_DTYPE; kept here so that this module imports no library)
EXPECT_DTYPE = np.dtype([("channel", np.int32), ("id", np.uint32), ("t_lo", np.uint64), ("t_hi", np.uint64),
                         ("corr_re", np.int32), ("corr_im", np.int32)])
MAX_MISSED = 50                  # the reference Hopper's MAX_MISSED


class _Station:
    __slots__ = ("hop", "last", "missed", "offset_hz")

    def __init__(self, hop: int, last: int, offset_hz: float) -> None:
        self.hop, self.last, self.missed, self.offset_hz = hop, last, 0, offset_hz


class Tracker:
    """Where and when each station heard so far transmits next.

    ``hop_pattern``: the sequence of channel indices (of the receiver's channel list) a station visits, one per dwell.
    ``period_outputs``: outputs between two packets of a station; default ``(41 + id) * out_rate // 16``, the Davis dwell
    of 2.5625 s + id / 16 s.  The reference uses 2.5625 s, which is id 0; the id term is taken from the protocol's
    published description and has not been checked against a station here.
    ``guard_outputs``: half the window's width; default ``2 * symbol_length + ceil(drift_ppm * 1e-6 * period * (missed +
    1))``, widening with every miss.  Either is capped at ``EXPECT_MAX_SPAN // 2`` so that ``t_hi - t_lo <= 2048``.  The
    default has not been measured on real stations, which is why it is a parameter.
    ``max_missed``: a station that misses this many expectations in a row is dropped (``lost``).
    ``if_hz``: where the channel's centre lies in its channelized bytes; default ``-out_rate // 4``, the channelizer's.
    ``use_repaired``: also learn from repaired rows (``acquire.repaired``), which are not CRC-proven.
    ``provisional_missed``: a provisional station (seeded by a searched row, ``acquire.searched``) that misses this many
    expectations in a row is dropped; it appears in ``provisional()``, not in ``stations()`` or ``stats()``, until a
    row of another path promotes it.
    """

    def __init__(self, cfg, hop_pattern: Sequence[int], *, period_outputs: Optional[int] = None,
                 guard_outputs: Optional[int] = None, drift_ppm: float = 100, max_missed: int = MAX_MISSED,
                 if_hz: Optional[int] = None, use_repaired: bool = False, provisional_missed: int = 2) -> None:
        self.hop_pattern = [int(c) for c in hop_pattern]
        if not self.hop_pattern or min(self.hop_pattern) < 0:
            raise ValueError("hop_pattern: a non-empty sequence of channel indices")
        if period_outputs is not None and int(period_outputs) < 1:
            raise ValueError("period_outputs must be positive")
        if guard_outputs is not None and int(guard_outputs) < 0:
            raise ValueError("guard_outputs must not be negative")
        if int(max_missed) < 1 or float(drift_ppm) < 0:
            raise ValueError("max_missed must be positive and drift_ppm not negative")
        if int(provisional_missed) < 1:
            raise ValueError("provisional_missed must be positive")
        self.symbol_length = int(cfg.symbol_length)
        self.packet_symbols = int(cfg.packet_symbols)
        self.out_rate = int(cfg.bit_rate) * self.symbol_length
        self.deviation_hz = 4800.0
        self.if_hz = -self.out_rate // 4 if if_hz is None else int(if_hz)
        self.period_outputs = None if period_outputs is None else int(period_outputs)
        self.guard_outputs = None if guard_outputs is None else int(guard_outputs)
        self.drift_ppm = float(drift_ppm)
        self.max_missed = int(max_missed)
        self.use_repaired = bool(use_repaired)
        self._stations: Dict[int, _Station] = {}
        self._stats: Dict[int, Dict[str, int]] = {}
        self.provisional_missed = int(provisional_missed)
        self._provisional: Dict[int, _Station] = {}
        self._search_stats = {"seeded": 0, "promoted": 0, "expired": 0, "ignored": 0}

    # ------------------------------------------------------------------------------------ the policy's numbers
    def period(self, ident: int) -> int:
        return self.period_outputs if self.period_outputs is not None else (41 + int(ident)) * self.out_rate // 16

    def guard(self, ident: int, missed: int = 0) -> int:
        if self.guard_outputs is not None:
            g = self.guard_outputs
        else:
            g = 2 * self.symbol_length + int(math.ceil(self.drift_ppm * self.period(ident) * (int(missed) + 1) / 1e6))
        return min(g, EXPECT_MAX_SPAN // 2)

    def corr(self, offset_hz: float):
        """``round(2**14 e^{j 2 pi (if_hz + offset) / out_rate})`` as ``(re, im)``."""
        a = 2.0 * math.pi * (float(self.if_hz) + float(offset_hz)) / float(self.out_rate)
        return int(round(16384.0 * math.cos(a))), int(round(16384.0 * math.sin(a)))

    # ------------------------------------------------------------------------------------ what was heard
    def observe_at(self, channel: int, ident: int, time: int, offset_hz: float) -> None:
        """A CRC-proven message of station ``ident`` on ``channel`` whose first symbol ended at ``time`` (the receiver's
        absolute output clock), its carrier ``offset_hz`` from the channel's centre: seeds the station or re-anchors it.
        A channel outside the hop pattern is ignored; a second report of the packet already counted (another path, the
        other side of a chunk boundary) only refreshes the carrier."""
        channel, ident, time = int(channel), int(ident), int(time)
        if channel not in self.hop_pattern:
            return
        hop = self.hop_pattern.index(channel)
        if self._provisional.pop(ident, None) is not None:    # confirmed: from here on a station like any other
            self._search_stats["promoted"] += 1
        st = self._stations.get(ident)
        stats = self._stats.setdefault(ident, {"received": 0, "missed": 0, "lost": 0})
        if st is not None and abs(time - st.last) < self.period(ident) // 2:
            st.offset_hz = float(offset_hz)
            return
        self._stations[ident] = _Station(hop, time, float(offset_hz))
        stats["received"] += 1

    def observe(self, rows) -> None:
        """Rows of ``burst_messages()`` / ``expected_messages()`` / ``searched_messages()`` (the records, or the named
        tuple), in order.  A searched row (``acquire.searched``) never re-anchors anything: of an id already known,
        provisional or not, or on a channel outside the hop pattern, it is ignored; of an unknown id it seeds a
        provisional station."""
        recs = np.asarray(getattr(rows, "records", rows))
        if recs.size and not self.use_repaired:
            recs = recs[~acquire.repaired(recs)]
        for r in recs:
            hz = acquire.burst_message_offset_hz(r, self.out_rate, self.if_hz, self.deviation_hz, self.packet_symbols)
            if int(r["flags"]) & acquire.MSG_SEARCHED:
                self._observe_searched(int(r["channel"]), int(r["id"]), int(r["time"]), hz)
            else:
                self.observe_at(int(r["channel"]), int(r["id"]), int(r["time"]), hz)

    def _observe_searched(self, channel: int, ident: int, time: int, offset_hz: float) -> None:
        if ident in self._stations or ident in self._provisional or channel not in self.hop_pattern:
            self._search_stats["ignored"] += 1
            return
        self._provisional[ident] = _Station(self.hop_pattern.index(channel), time, float(offset_hz))
        self._search_stats["seeded"] += 1

    def retuned(self, delta_hz: float) -> None:
        """Every channel's centre has moved by ``delta_hz`` (a ``retune`` to ``old + delta_hz``): the stored carriers,
        which are relative to the centres, move the other way."""
        for st in list(self._stations.values()) + list(self._provisional.values()):
            st.offset_hz -= float(delta_hz)

    # ------------------------------------------------------------------------------------ what to expect
    def _window(self, ident: int, st: _Station, missed: int):
        centre = st.last + (missed + 1) * self.period(ident)
        g = self.guard(ident, missed)
        return max(centre - g, 0), centre + g

    def table(self, clock: int, horizon_outputs: int) -> np.ndarray:
        """The ``EXPECT_DTYPE`` table for the chunks that cover outputs ``clock .. clock + horizon_outputs - 1``, every
        chunk before ``clock`` having been observed.  Per station: the next channel by the hop pattern, ``t_lo .. t_hi``
        around ``last + (missed + 1) * period``, the stored carrier as ``corr``.  An expectation all of whose packets
        would have ended before ``clock`` with nothing observed counts one miss and moves one hop on; after
        ``max_missed`` in a row the station is dropped.  A provisional station gets its rows in the same way, counts its
        misses apart from ``stats()`` and is dropped after ``provisional_missed`` of them."""
        clock, horizon = int(clock), int(horizon_outputs)
        body = self.symbol_length * (self.packet_symbols - 1)
        rows = []
        for ident in sorted(set(self._stations) | set(self._provisional)):   # (an id is in one of the two)
            prov = ident in self._provisional
            st = self._provisional[ident] if prov else self._stations[ident]
            limit = self.provisional_missed if prov else self.max_missed
            while True:
                _, t_hi = self._window(ident, st, st.missed)
                if t_hi + body >= clock:
                    break
                st.missed += 1
                if not prov:
                    self._stats[ident]["missed"] += 1
                if st.missed >= limit:
                    break
            if st.missed >= limit:
                if prov:
                    del self._provisional[ident]
                    self._search_stats["expired"] += 1
                else:
                    del self._stations[ident]
                    self._stats[ident]["lost"] += 1
                continue
            cre, cim = self.corr(st.offset_hz)
            m = st.missed
            while True:                                   # every window that begins inside the horizon
                t_lo, t_hi = self._window(ident, st, m)
                if t_lo - self.symbol_length >= clock + horizon or m - st.missed >= limit:
                    break
                ch = self.hop_pattern[(st.hop + m + 1) % len(self.hop_pattern)]
                rows.append((ch, ident, t_lo, t_hi, cre, cim))
                m += 1
        rows.sort(key=lambda r: (r[2], r[1]))
        return np.asarray(rows[:EXPECT_MAX], EXPECT_DTYPE).reshape(-1)

    def stations(self):
        """{id: (channel of the last message, its time, expectations missed since, carrier offset in Hz)}."""
        return {i: (self.hop_pattern[s.hop], s.last, s.missed, s.offset_hz) for i, s in sorted(self._stations.items())}

    def stats(self):
        """{id: {"received": messages counted, "missed": expectations that passed with nothing observed, "lost": times
        the station was dropped after ``max_missed`` misses in a row}}."""
        return {i: dict(v) for i, v in sorted(self._stats.items())}

    def provisional(self):
        """The ids of the provisional stations (seeded by a searched row, not yet confirmed), ascending."""
        return sorted(self._provisional)

    def search_stats(self):
        """{"seeded": searched rows that made a provisional station, "promoted": provisional stations confirmed by a row of
        another path, "expired": provisional stations dropped after ``provisional_missed`` misses, "ignored": searched rows
        of an id already known or of a channel outside the hop pattern}."""
        return dict(self._search_stats)
