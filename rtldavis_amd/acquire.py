"""Coarse frequency acquisition for ``wideband.WidebandReceiver``: the host policy on top of the device mechanism.

``retune`` learns from ``parsed()``: from messages that already passed the CRC.  A receiver whose reference is further
off than the +-4.8 kHz deviation decodes nothing and never gets such a number.  The energy of the bursts it cannot decode
still carries their carrier frequency: the receiver finds them in every chunk (``set_bursts`` / ``bursts()``), and what to
do with them is decided here, between chunks, as ``agc.GainControl`` decides the gains::

    rx.set_parse(True)
    rx.set_bursts(True)
    acq = Acquisition(rx.n_channels, rx.cfg)
    ...
    packets = rx.fetch()
    b = rx.bursts()
    rx.set_burst_threshold(acq.thresholds(b.floor))
    new = acq.update(b, rx.parsed(), rx.submitted)
    if new is not None:
        rx.retune(new)

With ``set_burst_decode`` the receiver also decodes every burst around the burst's own mean frequency
(``burst_messages()``): one burst then gives a CRC-proven message and, the bits being known, a carrier estimate without
the payload's 0/1 imbalance in it (``burst_message_offset_hz``).  Handed to ``update`` as ``messages``, one such row is
enough for a proposal - no ``need``, no waiting chunk, and a burst of any other device never enters::

    rx.set_burst_decode(True)
    ...
    new = acq.update(b, rx.parsed(), rx.submitted, rx.burst_messages())

With ``set_burst_repair`` some rows of ``burst_messages()`` are repaired ones (``repaired``, ``flipped_symbols``): the CRC
was made to pass by flipping one or two weak symbols, which a random candidate survives up to 36 times as often as the
CRC alone.  ``update`` ignores those rows unless the ``Acquisition`` was built with ``use_repaired=True``.

With ``set_burst_narrow`` the rows are decoded behind a narrow-band filter at the burst's own frequency (``narrowband``):
far more bursts decode in noise, and the rows are used like any others - the carrier estimate needs only the angle of
``(f_re, f_im)``.

Pure Python on the records' exact integers: the same records give the same decisions, on any machine; nothing here
touches a device.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import numpy as np

WINDOW = 128                 # outputs per window of a burst record (wideband.BURST_WINDOW)
THRESHOLD_OFF = 2 ** 32 - 1  # wideband.BURST_THRESHOLD_OFF
FLAG_FIRST, FLAG_LAST = 1, 2
MSG_REPAIRED = 2             # wideband.BURST_MSG_REPAIRED: bit 1 of a burst message's flags
MSG_NARROW = 4               # wideband.BURST_MSG_NARROW: bit 2
MSG_EXPECTED = 8             # wideband.BURST_MSG_EXPECTED: bit 3
MSG_SEARCHED = 16            # wideband.BURST_MSG_SEARCHED: bit 4
MSG_REPLAYED = 32            # replay.REPLAYED: bit 5
SEARCH_GRID = 64             # wideband.BURST_NARROW_GRID: a centre is g / 64 cycles per output


def burst_offset_hz(rec, floor_row, out_rate: int, if_hz: int) -> float:
    """The mean frequency of one burst record relative to the channel centre tuned at present, in Hz - what ``retune``
    adds.  ``R = (corr_re + j corr_im) - windows * (corr_off / windows_off)`` takes off what the channel's own noise
    contributes to the correlation (the channel filter colours it; no correction when the chunk has no OFF window), and
    ``angle(R) * out_rate / 2 pi`` is the frequency of the channelized samples, which carry the channel at ``if_hz``
    (``WidebandReceiver.if_hz``).  Unambiguous within +-out_rate / 2 of the channelized band's centre."""
    r = complex(int(rec["corr_re"]), int(rec["corr_im"]))
    n_off = int(floor_row["windows_off"])
    if n_off:
        r -= int(rec["windows"]) * complex(int(floor_row["corr_re_off"]), int(floor_row["corr_im_off"])) / n_off
    return math.atan2(r.imag, r.real) * float(out_rate) / (2.0 * math.pi) - float(if_hz)


def burst_message_offset_hz(row, out_rate: int, if_hz: int, deviation_hz: float = 4800.0, packet_symbols: int = 80) -> float:
    """The carrier of one decoded burst (a row of ``burst_messages().records``) relative to the channel centre tuned at
    present, in Hz.  ``angle(f_re + j f_im) * out_rate / 2 pi`` is the mean frequency of the packet's samples, which
    carry the channel at ``if_hz``; a packet with ``ones`` 1 symbols of ``packet_symbols`` lies
    ``deviation_hz * (2 ones - packet_symbols) / packet_symbols`` above its carrier on average, and the bits are known."""
    f = math.atan2(int(row["f_im"]), int(row["f_re"])) * float(out_rate) / (2.0 * math.pi) - float(if_hz)
    return f - float(deviation_hz) * (2 * int(row["ones"]) - int(packet_symbols)) / float(packet_symbols)


def repaired(records) -> np.ndarray:
    """Boolean mask over ``burst_messages().records`` (or a ``BurstMessages``): the rows whose CRC passes only after the
    flips in ``pad`` (``flags`` bit 1).  With ``set_burst_repair`` never called it is all False."""
    recs = np.asarray(getattr(records, "records", records))
    return (recs["flags"] & MSG_REPAIRED) != 0


def narrowband(records) -> np.ndarray:
    """Boolean mask over ``burst_messages().records`` (or a ``BurstMessages``): the rows decoded behind the narrow-band
    filter (``flags`` bit 2; ``pad[3]`` is the filter's centre in 64ths of a cycle per output).  Their ``margin``, ``f_re``
    and ``f_im`` are in the filter's units: ``burst_message_offset_hz`` uses only the angle of ``(f_re, f_im)`` and holds
    for both kinds, and nothing in this module compares ``margin``.  With ``set_burst_narrow`` never called it is all
    False."""
    recs = np.asarray(getattr(records, "records", records))
    return (recs["flags"] & MSG_NARROW) != 0


def expected(records) -> np.ndarray:
    """Boolean mask over message rows (or a ``BurstMessages`` / ``ExpectedMessages``): the rows decoded at an expectation
    (``flags`` bit 3; ``first`` is the expectation's index in its table) - all of ``expected_messages()``, none of
    ``burst_messages()``."""
    recs = np.asarray(getattr(records, "records", records))
    return (recs["flags"] & MSG_EXPECTED) != 0


def searched(records) -> np.ndarray:
    """Boolean mask over message rows (or a ``SearchedMessages`` / ``BurstMessages`` / ``ExpectedMessages``): the rows the
    blind search found (``flags`` bit 4; ``first`` is the centre's index in its list) - all of ``searched_messages()``,
    none of the others.  Such a row proves less than any other (``WidebandReceiver.searched_messages``)."""
    recs = np.asarray(getattr(records, "records", records))
    return (recs["flags"] & MSG_SEARCHED) != 0


def replayed(records) -> np.ndarray:
    """Boolean mask over message rows (or anything with ``records``): the rows that ``replay.ClipDecoder`` decoded from a
    recording (``flags`` bit 5; ``first`` is the job's index) - all of a ``Replay``'s rows with a message, none of a
    receiver's."""
    recs = np.asarray(getattr(records, "records", records))
    return (recs["flags"] & MSG_REPLAYED) != 0


def search_hits(records) -> np.ndarray:
    """uint8 per searched row: the adjacent positions (less than ``symbol_length`` away, the row's own included) that
    passed sync word and CRC - ``pad[0]``.  About ``symbol_length - 2`` for a real packet and 1 for a chance hit; the
    library gates on neither this nor ``margin``, the policy is the caller's.  0 for a row that is not a searched one."""
    recs = np.asarray(getattr(records, "records", records))
    return np.where((recs["flags"] & MSG_SEARCHED) != 0, recs["pad"][..., 0], 0).astype(np.uint8)


def search_centres(offsets_hz, out_rate: int, if_hz: Optional[int] = None, spread: int = 0) -> np.ndarray:
    """The list for ``WidebandReceiver.set_burst_search``: sorted unique grid points
    ``g = round(64 (if_hz + off) / out_rate) mod 64`` for every carrier offset ``off`` (Hz from the channel centre, as
    ``burst_message_offset_hz`` gives it) and the ``spread`` grid steps to either side of each.  ``if_hz`` None is the
    receiver's default, ``-out_rate // 4``.  One centre covers about +-2 steps at moderate noise and +-1 near the limit
    (profiles/burst_search_gain.txt); the library takes at most eight."""
    if int(spread) < 0:
        raise ValueError("spread: a non-negative number of grid steps")
    i_f = -int(out_rate) // 4 if if_hz is None else int(if_hz)
    out = set()
    for off in np.asarray(offsets_hz, np.float64).reshape(-1):
        g = int(round(SEARCH_GRID * (i_f + float(off)) / float(out_rate)))
        out.update((g + d) % SEARCH_GRID for d in range(-int(spread), int(spread) + 1))
    return np.asarray(sorted(out), np.uint8)


# Signal quality of a message row (``WidebandReceiver.burst_message_quality()`` / ``expected_message_quality()``, rows of
# ``wideband.QUALITY_DTYPE``), by the reference's formulas (rtldavis dsp.py: the mean power of the 16 sync symbols for
# the signal, of the 16 symbols' worth of samples in front of the packet for the noise).  The sums are in the units of the
# channelized bytes, a = 2 b - 255, so full scale is 255; behind the narrow-band filter the pass-band gain is 2^14 / 2^11.
FULL_SCALE = 255.0
INBAND_GAIN = 8.0            # 2^14 (the taps sum to it) / 2^11 (RD_BD_NB_SHIFT)
QUALITY_INBAND = 1           # wideband.QUALITY_INBAND: bit 0 of a quality row's flags
NO_NOISE_POWER = 1e-9        # the reference's noise power when there is no noise region, in full-scale^2
NO_SIGNAL_DB = -120.0        # the reference's rssi at zero power
ZERO_NOISE_SNR_DB = 50.0     # the reference's snr at zero noise power


def _snr_db(sig: int, n_sig: int, noise: int, n_noise: int, full_scale: float) -> float:
    if sig <= 0:
        return float("nan")  # (no measurable row has it: every |z|^2 is at least 2)
    signal_power = sig / (n_sig * full_scale * full_scale)
    noise_power = noise / (n_noise * full_scale * full_scale) if n_noise > 0 else NO_NOISE_POWER
    return 10.0 * math.log10(signal_power / noise_power) if noise_power > 0 else ZERO_NOISE_SNR_DB


def rssi_db(q, symbol_length: int) -> float:
    """``10 log10`` of the mean power of the packet's 16 sync symbols, 1.0 = a full-scale component (|a| = 255): the
    reference's ``rssi`` on the channelized bytes.  -120 at zero power (a row with ``flags`` bit 7)."""
    sig = int(q["sig"])
    return 10.0 * math.log10(sig / (16 * int(symbol_length) * FULL_SCALE * FULL_SCALE)) if sig > 0 else NO_SIGNAL_DB


def snr_db(q, symbol_length: int) -> float:
    """The reference's ``snr``: sync power over the mean power of the ``n_noise`` outputs in front of the packet; with its
    fallbacks - a noise power of 1e-9 full-scale^2 when ``n_noise`` = 0, and 50 when the noise sum is 0.  What lies in that
    window is whatever the transmitter sends before its sync word: see ``snr_floor_db``.  NaN for a row without signal."""
    return _snr_db(int(q["sig"]), 16 * int(symbol_length), int(q["noise"]), int(q["n_noise"]), FULL_SCALE)


def snr_inband_db(q, symbol_length: int) -> float:
    """The same on the sums behind the narrow-band filter (``sig_nb``, ``noise_nb``): the ratio in the +-0.9 symbol rates
    the narrow decoder sees.  NaN without ``flags`` bit 0."""
    if not int(q["flags"]) & QUALITY_INBAND:
        return float("nan")
    return _snr_db(int(q["sig_nb"]), 16 * int(symbol_length), int(q["noise_nb"]), int(q["n_noise"]), FULL_SCALE * INBAND_GAIN)


def snr_floor_db(q, floor_row, symbol_length: int) -> float:
    """Sync power over the channel's noise floor, ``power_off / (128 windows_off)`` of the chunk's ``bursts().floor`` row -
    for the case where the window in front of the packet is not noise (a lead-in).  The reference's fallbacks apply to a
    chunk without OFF windows and to a floor of 0."""
    return _snr_db(int(q["sig"]), 16 * int(symbol_length), int(floor_row["power_off"]), WINDOW * int(floor_row["windows_off"]), FULL_SCALE)


def flipped_symbols(row) -> Tuple[int, ...]:
    """The symbol indices (0 = the first sync symbol) a repaired row had flipped, ascending: a tuple of 0, 1 or 2."""
    if not int(row["flags"]) & MSG_REPAIRED:
        return ()
    return tuple(int(k) for k in row["pad"][1: 1 + int(row["pad"][0])])


def merge(tail, bursts) -> Tuple[np.ndarray, np.ndarray]:
    """Join the runs a chunk boundary cut.  ``tail``: the records of the chunk before that end with it (flag bit 1), or
    None; ``bursts``: the next chunk's records.  Returns ``(complete, new_tail)``: ``new_tail`` are the runs that end with
    this chunk - they may go on - and ``complete`` all others, a run of ``tail`` joined with the run that begins this
    chunk on the same channel (the sums add, ``peak`` is the larger, ``first`` and flag bit 0 are the earlier half's) or,
    when there is none, as it was."""
    recs = np.asarray(getattr(bursts, "records", bursts))
    out = recs.copy()
    heads = {int(r["channel"]): i for i, r in enumerate(out) if int(r["flags"]) & FLAG_FIRST}
    alone = []
    for t in ([] if tail is None else tail):
        i = heads.get(int(t["channel"]))
        if i is None:
            alone.append(t)
            continue
        r = out[i]
        for f in ("windows", "power", "corr_re", "corr_im"):
            r[f] += t[f]
        r["peak"] = max(int(r["peak"]), int(t["peak"]))
        r["first"] = t["first"]
        r["flags"] = (int(r["flags"]) & FLAG_LAST) | (int(t["flags"]) & FLAG_FIRST)
    goes_on = (out["flags"] & FLAG_LAST) != 0
    complete = out[~goes_on]
    if alone:
        complete = np.concatenate([np.asarray(alone, dtype=out.dtype), complete])
    return complete, out[goes_on]


class Acquisition:
    """One frequency offset for all channels - a wrong reference moves every channel alike - found from bursts that
    bring no message.

    ``thresholds(floor)``: per channel ``factor * power_off // windows_off``, ``factor`` times the mean energy of the
    windows that were OFF; a channel without an OFF window keeps its value.  With the default table every window is OFF,
    so the first chunk measures the floor.

    ``update(bursts, parsed_rows, submitted)`` takes one fetched chunk: its ``bursts()``, its ``parsed()`` rows and
    ``WidebandReceiver.submitted`` at that moment.  It returns None, or the offset to ``retune`` to before the next
    submit: one integer, relative to the constructed plan like every ``retune`` argument.

    - A run is a candidate when it is complete (``merge``: a run that ends with its chunk waits for the next one) and
      ``min_windows <= windows <= max_windows``: a packet lasts ``packet_symbols * symbol_length`` outputs plus its lead-in,
      so anything shorter is a fragment or a spike and anything over twice that is no single packet.
    - A candidate waits one chunk before it counts as an estimate: the message of a burst is reported with the chunk in
      which the packet ends, which may be the next, and a burst the receiver decodes needs no acquisition.
    - Chunks submitted before the last proposed retune took effect are ignored: their estimates refer to the old tuning.
    - After ``need`` estimates the proposal is ``offset + median`` of them, rounded; the estimates start anew.
    - With ``messages`` (``burst_messages()`` of the same chunk - a ``BurstMessages`` of another chunk is a ValueError;
      optional - without it everything is as above): while not
      locked, a chunk ``>= valid_from`` that brings rows is proposed from at once, ``offset + round(median of
      burst_message_offset_hz over its rows)``; the CRC is the proof, so there is no ``need`` and no waiting chunk.
      ``valid_from`` becomes ``submitted``, candidates and estimates are forgotten.  Repaired rows (``repaired``) are
      left out unless ``use_repaired`` is set: they are not CRC-proven.
    - Once a CRC-valid message arrives, on any channel, the receiver is within reach of the AFC (``parsed()`` ->
      ``retune``): ``locked`` is set, the candidates and estimates are dropped - that channel's own burst among them - and
      nothing is proposed any more, until ``reset()``.
    """

    def __init__(self, n_channels: int, cfg, factor: int = 4, need: int = 3, min_windows: Optional[int] = None,
                 max_windows: Optional[int] = None, if_hz: Optional[int] = None, use_repaired: bool = False) -> None:
        if int(n_channels) < 1 or int(factor) < 1 or int(need) < 1:
            raise ValueError("n_channels, factor and need must be positive")
        self.n_channels = int(n_channels)
        self.out_rate = int(cfg.bit_rate) * int(cfg.symbol_length)
        self.packet_symbols = int(cfg.packet_symbols)
        self.deviation_hz = 4800.0                                           # the Davis link's (synth.py)
        self.if_hz = -self.out_rate // 4 if if_hz is None else int(if_hz)     # (channelizer.plan_channels' default)
        self.factor = int(factor)
        self.need = int(need)
        self.use_repaired = bool(use_repaired)
        self.min_windows = int(cfg.packet_symbols) * int(cfg.symbol_length) // WINDOW if min_windows is None else int(min_windows)
        self.max_windows = 2 * self.min_windows + 2 if max_windows is None else int(max_windows)
        if not 1 <= self.min_windows <= self.max_windows:
            raise ValueError("1 <= min_windows <= max_windows")
        self.reset()

    def reset(self) -> None:
        """Back to the state after construction: offset 0, no estimates, not locked, the default thresholds."""
        self.offset = 0                  # the offset last proposed
        self.valid_from = 0              # the first chunk that offset holds for
        self.locked = False
        self.estimates: List[float] = []
        self._thr = np.full(self.n_channels, THRESHOLD_OFF, np.uint64)
        self._forget()

    def _forget(self) -> None:
        self._chunk = None               # the chunk of the last update
        self._tail = None                # its runs that may go on
        self._waiting: List[Tuple[int, float]] = []   # its candidates (channel, Hz)

    def thresholds(self, floor) -> np.ndarray:
        """uint32 per channel for ``set_burst_threshold``, from one chunk's floor records."""
        floor = np.asarray(getattr(floor, "floor", floor))
        if floor.shape != (self.n_channels,):
            raise ValueError(f"{floor.size} floor records for {self.n_channels} channels")
        n_off = floor["windows_off"].astype(np.uint64)
        some = n_off > 0
        self._thr[some] = np.minimum(self.factor * floor["power_off"][some].astype(np.uint64) // n_off[some], THRESHOLD_OFF)
        return self._thr.astype(np.uint32)

    def candidates(self, bursts) -> List[Tuple[int, float]]:
        """``(channel, offset in Hz)`` of the chunk's complete runs of plausible length; keeps the runs that may go on
        for the next chunk (a gap in the chunk numbers drops the ones kept before)."""
        k = int(bursts.chunk)
        tail = self._tail if self._chunk is not None and k == self._chunk + 1 else None
        complete, self._tail = merge(tail, bursts.records)
        return [(int(r["channel"]), burst_offset_hz(r, bursts.floor[int(r["channel"])], self.out_rate, self.if_hz))
                for r in complete if self.min_windows <= int(r["windows"]) <= self.max_windows]

    def update(self, bursts, parsed_rows, submitted: int, messages=None) -> Optional[int]:
        k = int(bursts.chunk)
        if messages is not None and int(getattr(messages, "chunk", k)) != k:
            raise ValueError(f"messages of chunk {int(messages.chunk)} with the bursts of chunk {k}")
        if len(parsed_rows):
            self.locked = True
        if self.locked:
            self.estimates = []
            self._forget()
            return None
        if k < self.valid_from:
            self._forget()
            return None
        rows = [] if messages is None else np.asarray(getattr(messages, "records", messages))
        if len(rows) and not self.use_repaired:
            rows = rows[~repaired(rows)]
        if len(rows):
            est = [burst_message_offset_hz(r, self.out_rate, self.if_hz, self.deviation_hz, self.packet_symbols) for r in rows]
            self.offset += int(round(float(np.median(est))))
            self.valid_from = int(submitted)
            self.estimates = []
            self._forget()
            return self.offset
        if self._chunk is not None and k == self._chunk + 1:
            self.estimates += [hz for _, hz in self._waiting]
        self._waiting = self.candidates(bursts)
        self._chunk = k
        if len(self.estimates) < self.need:
            return None
        self.offset += int(round(float(np.median(self.estimates))))
        self.valid_from = int(submitted)
        self.estimates = []
        self._forget()
        return self.offset
