"""Live wideband receiver: one capture that never ends, fed chunk by chunk, channelized into every hop
channel and demodulated on the GPU with the state of both carried from chunk to chunk
(csrc/rd_wideband.hip).

``Channelizer`` + ``BatchDemodulator`` handle one self-contained capture: zero history before it, output
time counted from its start.  Fed a live SDR's chunks one at a time they would restart the filter history
and the mixer phase at every boundary and damage every packet that crosses one.  ``WidebandReceiver``
carries both: its channelized bytes equal ``Channelizer.run_host()`` on the whole capture, byte for byte,
and its packets equal ``BatchDemodulator`` on those bytes.  Parity with the reference is unpinned, as for
the channelizer (rtldavis retunes one narrow-band dongle per hop).
"""
from __future__ import annotations

import ctypes as C
import logging
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import _lib
from .channelizer import DEFAULT_CENTRE_HZ, DEFAULT_DECIM, US_CHANNELS_HZ, chan_config, plan_channels
from .dsp import Packet, _cfg_struct, _packets_per_stream

logger = logging.getLogger(__name__)

# levels(): one row per channel
LEVEL_DTYPE = np.dtype([("gain", np.float32), ("peak", np.uint32), ("clipped", np.uint32), ("power", np.uint64)])


class InputLevel(NamedTuple):
    """The capture chunk's own levels (``Levels.input``): over its ``2 * chunk_samples`` components k, with a = 2 k - 255
    for "u8" and a = k for "s8" / "s16": ``peak`` = max |a|, ``clipped`` = components at either end of the format's
    range, ``power`` = sum a^2."""
    peak: int
    clipped: int
    power: int


class Levels(NamedTuple):
    """``WidebandReceiver.levels()``: ``channels`` (structured array of ``LEVEL_DTYPE``, one row per channel), ``input``
    (``InputLevel``) and ``chunk``, the chunk's number since construction / ``reset()`` (its packets' ``call``)."""
    channels: np.ndarray
    input: InputLevel
    chunk: int


# bursts(): one row per run of ON windows / one row per channel - the layouts of rd_burst and rd_burst_floor
BURST_DTYPE = np.dtype([("channel", np.int32), ("first", np.uint32), ("windows", np.uint32), ("flags", np.uint32),
                        ("power", np.uint64), ("peak", np.uint32), ("pad", np.uint32), ("corr_re", np.int64),
                        ("corr_im", np.int64)])
BURST_FLOOR_DTYPE = np.dtype([("threshold", np.uint32), ("windows_off", np.uint32), ("n_bursts", np.uint32),
                              ("chunk", np.uint32), ("power_off", np.uint64), ("corr_re_off", np.int64),
                              ("corr_im_off", np.int64)])
BURST_WINDOW = 128                     # outputs per window
BURST_THRESHOLD_OFF = 2 ** 32 - 1      # the default threshold: no window's energy reaches it


class Bursts(NamedTuple):
    """``WidebandReceiver.bursts()``: ``records`` (structured array of ``BURST_DTYPE``, one row per run of ON windows,
    channels ascending, a channel's runs in ascending ``first``), ``floor`` (``BURST_FLOOR_DTYPE``, one row per channel:
    the OFF windows and the threshold in force) and ``chunk``, the chunk's number since construction / ``reset()``."""
    records: np.ndarray
    floor: np.ndarray
    chunk: int


# burst_messages(): one row per decoded burst - the layout of rd_burst_msg
BURST_MSG_DTYPE = np.dtype([("channel", np.int32), ("first", np.uint32), ("tau", np.int32), ("flags", np.uint32),
                            ("time", np.uint64), ("margin", np.uint64), ("f_re", np.int64), ("f_im", np.int64),
                            ("data", np.uint8, (_lib.RD_BURST_MSG_BYTES,)), ("ones", np.uint8), ("id", np.uint8),
                            ("pad", np.uint8, (4,))])
BURST_DECODE_MAX_WINDOWS = 32          # a longer run is counted in ``long_runs``, not decoded
BURST_MSG_REPAIRED = 2                 # ``flags`` bit 1: ``pad[1]`` (and ``pad[2]``) were flipped to satisfy the CRC
BURST_REPAIR_LIST = 8                  # the least reliable payload symbols a repair may flip
BURST_REPAIR_MAX_FLIPS = 2
BURST_MSG_NARROW = 4                   # ``flags`` bit 2: decoded behind the narrow-band filter, ``pad[3]`` its centre g
BURST_NARROW_GRID = 64                 # the filter's centre is g / 64 cycles per output
BURST_NARROW_MIN_SL = 4
BURST_MSG_EXPECTED = 8                 # ``flags`` bit 3: decoded at an expectation, ``first`` is its index in the table
BURST_EXPECT_MAX = 64                  # expectations per table
BURST_EXPECT_MAX_SPAN = 2048           # ``t_hi - t_lo`` at most
BURST_EXPECT_ANY_ID = 0xFF
# set_burst_expect(): one row per expectation - the layout of rd_expect
EXPECT_DTYPE = np.dtype([("channel", np.int32), ("id", np.uint32), ("t_lo", np.uint64), ("t_hi", np.uint64),
                         ("corr_re", np.int32), ("corr_im", np.int32)])
BURST_MSG_SEARCHED = 16                # ``flags`` bit 4: found by the blind search, ``first`` is the centre's index in the list
BURST_SEARCH_MAX_CENTRES = 8           # centres per list
BURST_SEARCH_PER = 4                   # rows per (centre, channel) and chunk
BURST_SEARCH_TILE = 1024               # candidates per tile of the search kernel
# searched_messages(): the layout of rd_bs_header, one per (centre, channel)
SEARCH_HDR_DTYPE = np.dtype([("n_msgs", np.uint32), ("sync_hits", np.uint32), ("chunk", np.uint32), ("dropped", np.uint32)])


# burst_message_quality() / expected_message_quality(): one row per message row - the layout of rd_burst_quality
QUALITY_DTYPE = np.dtype([("pkt", np.uint64), ("sig", np.uint64), ("noise", np.uint64), ("pkt_nb", np.uint64),
                          ("sig_nb", np.uint64), ("noise_nb", np.uint64), ("n_noise", np.uint32), ("clipped", np.uint32),
                          ("peak", np.uint16), ("g", np.uint8), ("flags", np.uint8), ("chunk", np.uint32)])
QUALITY_INBAND = 1                     # ``flags`` bit 0: ``g`` and the ``_nb`` sums are valid
QUALITY_UNMEASURABLE = 128             # ``flags`` bit 7: the message's channel or tau was out of range, every sum is 0
QUALITY_MAX_GAP = 1024                 # ``noise_gap`` at most


# burst_clips(): one row per clip - the layout of rd_burst_clip
CLIP_DTYPE = np.dtype([("channel", np.int32), ("source", np.uint32), ("flags", np.uint32), ("t0", np.int32), ("n", np.uint32),
                       ("offset", np.uint32), ("time", np.uint64), ("ref", np.uint64), ("chunk", np.uint32), ("pad", np.uint32)])
CLIP_RUNS = 1                          # ``sources`` bit 0: every run of ``bursts()``
CLIP_MESSAGES = 2                      # ``sources`` bit 1: every row the decode, expect and search kernels wrote
CLIP_MAX_ROLL = 1024                   # ``pre`` and ``post`` at most
CLIP_MAX_QUOTA = 65536
CLIP_PER = 16                          # clips per channel and chunk
CLIP_SOURCE_TAIL, CLIP_SOURCE_RUN, CLIP_SOURCE_DECODE, CLIP_SOURCE_EXPECTED, CLIP_SOURCE_SEARCHED = range(5)
CLIP_CUT_START = 1                     # ``flags`` bit 0: the request began before the chunk before (or, without one, the chunk)
CLIP_CUT_END = 2                       # ``flags`` bit 1: the request ends in the next chunk, whose first clip is its tail
CLIP_FROM_PREV = 4                     # ``flags`` bit 2: the clip begins in the chunk before


class BurstClips(NamedTuple):
    """``WidebandReceiver.burst_clips()``: ``records`` (``CLIP_DTYPE``, channels ascending, a channel's clips in the order
    tail, runs, decode rows, expected rows, searched rows), ``iq`` (uint8 [total_outputs, 2]: the clips' channelized bytes,
    I and Q per output, one clip behind the other - row ``records["offset"][i]`` is clip i's first output), ``dropped``
    (uint32 per channel: requests that did not fit the quota or the ``CLIP_PER`` records) and ``chunk``."""
    records: np.ndarray
    iq: np.ndarray
    dropped: np.ndarray
    chunk: int

    def clip(self, i: int) -> np.ndarray:
        """uint8 [n, 2]: a view of clip ``i``'s outputs ``time .. time + n - 1`` of its channel."""
        r = self.records[i]
        return self.iq[int(r["offset"]): int(r["offset"]) + int(r["n"])]


class BurstMessages(NamedTuple):
    """``WidebandReceiver.burst_messages()``: ``records`` (structured array of ``BURST_MSG_DTYPE``, one row per burst that
    carried a CRC-valid message, channels ascending, a channel's runs ascending), ``long_runs`` (uint32 per channel: runs
    of more than 32 windows, which are not decoded) and ``chunk``, the chunk's number since construction / ``reset()``."""
    records: np.ndarray
    long_runs: np.ndarray
    chunk: int


class ExpectedMessages(NamedTuple):
    """``WidebandReceiver.expected_messages()``: ``records`` (``BURST_MSG_DTYPE``, at most one row per expectation of the
    table the chunk was submitted with, in table order; ``first`` is the expectation's index and ``flags`` has
    ``BURST_MSG_EXPECTED`` set), ``candidates`` (uint32, one per expectation of that table: the number of candidate
    positions it had in the chunk, 0 when it was idle there) and ``chunk``."""
    records: np.ndarray
    candidates: np.ndarray
    chunk: int


class SearchedMessages(NamedTuple):
    """``WidebandReceiver.searched_messages()``: ``records`` (``BURST_MSG_DTYPE``, centres in list order, channels
    ascending, at most ``BURST_SEARCH_PER`` rows per centre and channel by ``tau``; ``flags`` has ``BURST_MSG_SEARCHED`` and
    ``BURST_MSG_NARROW`` set, ``first`` is the centre's index in the list the chunk was submitted with, ``pad`` is
    ``(hits, 0, 0, g)``), ``sync_hits`` and ``dropped`` (uint32 [centres, channels]: the positions whose first 16 symbols
    equalled the sync word, and the reported positions beyond the fourth) and ``chunk``."""
    records: np.ndarray
    sync_hits: np.ndarray
    dropped: np.ndarray
    chunk: int


class Spectrum(NamedTuple):
    """``WidebandReceiver.spectrum()`` / ``Channelizer.spectrum()``: ``power`` (float64 [n_bins], ascending frequency,
    1.0 = a full-scale complex tone on a bin centre), ``freqs_hz`` (float64 [n_bins], the bins' absolute RF centres:
    ``centre_hz + (j - n_bins / 2) * wide_rate / n_bins``), ``segments`` (windows of ``n_bins`` samples averaged) and
    ``chunk`` (the chunk's number since construction / ``reset()``; 0 for a ``Channelizer``)."""
    power: np.ndarray
    freqs_hz: np.ndarray
    segments: int
    chunk: int

    def db(self) -> np.ndarray:
        """``10 log10(power)`` in dBFS, an empty bin as the smallest positive float64's."""
        return 10.0 * np.log10(np.maximum(self.power, np.finfo(np.float64).tiny))

    def band_power(self, lo_hz: float, hi_hz: float) -> float:
        """The sum of the bins whose centres lie in [lo_hz, hi_hz] - e.g. the occupancy of one hop channel."""
        sel = (self.freqs_hz >= lo_hz) & (self.freqs_hz <= hi_hz)
        return float(self.power[sel].sum())


def spectrum_freqs(centre_hz: int, wide_rate: int, n_bins: int) -> np.ndarray:
    """The bin centres of an ``n_bins`` spectrum in Hz, ascending; entry ``n_bins // 2`` is ``centre_hz``."""
    return float(centre_hz) + (np.arange(n_bins, dtype=np.float64) - n_bins // 2) * (float(wide_rate) / n_bins)


def burst_packets(records, quality, n_channels: int, symbol_length: int, inband: bool = False,
                  use_repaired: bool = False, packet_symbols: int = 80) -> List[List[Packet]]:
    """One ``List[Packet]`` per channel from message rows (``burst_messages().records`` or ``expected_messages().records``)
    and their quality rows: ``Packet(index=-1, data, rssi, snr)`` with ``acquire.rssi_db`` and ``acquire.snr_db``
    (``snr_inband_db`` with ``inband``).  ``index = -1`` selects the branch of the reference's ``Parser.parse`` for packets
    demodulated in hardware (no frequency error from the discriminator), so the rows go through the unmodified parser.
    Repaired rows (``flags`` bit 1) are left out unless ``use_repaired``; ``data`` is the row's first
    ``packet_symbols / 8`` on-air bytes."""
    from . import acquire
    recs = np.asarray(getattr(records, "records", records))
    quality = np.asarray(quality)
    if recs.shape != quality.shape:
        raise ValueError(f"Incompatible array sizes: {recs.size} message rows, {quality.size} quality rows")
    out: List[List[Packet]] = [[] for _ in range(int(n_channels))]
    for m, q in zip(recs.reshape(-1), quality.reshape(-1)):
        if int(m["flags"]) & BURST_MSG_REPAIRED and not use_repaired:
            continue
        snr = acquire.snr_inband_db(q, symbol_length) if inband else acquire.snr_db(q, symbol_length)
        out[int(m["channel"])].append(Packet(-1, np.array(m["data"][: int(packet_symbols) // 8], dtype=np.uint8), acquire.rssi_db(q, symbol_length), snr))
    return out


class WidebandReceiver:
    """``WidebandReceiver(cfg, channels_hz, centre_hz)``: chunks of ``chunk_bytes`` (I,Q of ``chunk_samples`` =
    ``decim * cfg.block_size`` wideband samples at ``decim * cfg.bit_rate * cfg.symbol_length``, in ``sample_format``:
    ``"u8"`` offset bytes, ``"s8"`` int8, ``"s16"`` int16 or ``"cf32"`` float32 / ``complex64``, see ``Channelizer``) in,
    one ``List[Packet]`` per channel and chunk out - each channel behaves like its own ``Demodulator``
    fed the channel's stream.  ``submit`` / ``fetch`` keep up to two chunks in flight (the copy of
    one beside the kernels of the other); ``demodulate`` is both in one call."""

    def __init__(self, cfg, channels_hz: Sequence[int] = US_CHANNELS_HZ, centre_hz: int = DEFAULT_CENTRE_HZ,
                 decim: int = DEFAULT_DECIM, taps: Optional[np.ndarray] = None, gain: float = 3.0,
                 sample_format: str = "u8") -> None:
        self.cfg = cfg
        self._h = C.c_void_p()
        self.sample_format = sample_format
        self._fmt, self.dtype = _lib.sample_format(sample_format)
        if int(cfg.block_size) % 128 or int(cfg.block_size) < 128:
            raise ValueError(f"block_size {cfg.block_size} is not a positive multiple of 128")
        plan_channels(self, channels_hz, centre_hz, decim, taps, gain, int(cfg.bit_rate) * int(cfg.symbol_length))
        self._plan_shift_hz = self.shift_hz.copy()                  # the constructed plan: retune() offsets, reset()
        self.centre_hz = int(centre_hz)                             # spectrum(): the bins' absolute frequencies
        self.block_size = int(cfg.block_size)
        self.chunk_samples = self.decim * self.block_size           # IQ pairs per chunk
        self.chunk_bytes = 2 * np.dtype(self.dtype).itemsize * self.chunk_samples
        _lib.check(_lib.lib().rd_wb_create_fmt(C.byref(_cfg_struct(cfg)), C.byref(chan_config(self)), self._fmt,
                                               self.taps.ctypes.data, self.shift_hz.ctypes.data, C.byref(self._h)))
        self._spectrum_bins = self._fetched_bins = 0                # set_spectrum(); the setting at the last fetch
        self._submitted = 0
        self._burst_cap = 64
        self._cap = 64 * max(1, self.n_channels)
        self._recs = (_lib.RdPacket * self._cap)()

    def __del__(self):
        try:
            if self._h:
                _lib.lib().rd_wideband_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def _check_chunk(self, chunk: np.ndarray) -> np.ndarray:
        a = _lib.iq_array(chunk, self.dtype)
        if a.nbytes != self.chunk_bytes:
            logger.error(f"Incompatible array sizes: chunk.size={a.size}")
            raise ValueError("Incompatible array sizes")
        return a

    def _take(self, rc: int, n: "C.c_int") -> List[List[Packet]]:
        if rc == _lib.RD_ERR_CAPACITY:  # nothing is lost: the handle keeps the chunk's packets
            self._cap = max(2 * self._cap, n.value)
            self._recs = (_lib.RdPacket * self._cap)()
            rc = _lib.lib().rd_wideband_refetch(self._h, self._recs, self._cap, C.byref(n))
        _lib.check(rc)
        return _packets_per_stream(self._recs, n.value, self.n_channels)

    def submit(self, chunk: np.ndarray) -> None:
        """Queue one chunk (asynchronous copy, channelizer and demodulator; at most two chunks in flight)."""
        a = self._check_chunk(chunk)
        _lib.check(_lib.lib().rd_wideband_submit(self._h, a.ctypes.data, a.nbytes))
        self._submitted += 1

    @property
    def submitted(self) -> int:
        """Chunks submitted since construction / ``reset()``: the number the next submitted chunk will carry, i.e. the
        chunk from which a ``retune``, ``set_gain`` or ``set_burst_threshold`` made now holds."""
        return self._submitted

    def fetch(self) -> List[List[Packet]]:
        """Packets of the oldest chunk in flight, one list per channel."""
        n = C.c_int(0)
        rc = _lib.lib().rd_wideband_fetch(self._h, self._recs, self._cap, C.byref(n))
        out = self._take(rc, n)
        self._fetched_bins = self._spectrum_bins
        return out

    def demodulate(self, chunk: np.ndarray) -> List[List[Packet]]:
        """submit + fetch of one chunk on a quiet receiver."""
        a = self._check_chunk(chunk)
        if self.inflight:
            raise RuntimeError(f"{self.inflight} chunk(s) in flight: fetch them first")
        self.submit(a)
        return self.fetch()

    @property
    def inflight(self) -> int:
        return int(_lib.lib().rd_wideband_inflight(self._h))

    def set_parse(self, on: bool = True) -> None:
        """From the next chunk on, the demodulator's kernels also run ``protocol.Parser.parse``'s front half for every
        channel's packets (``Demodulator.set_parse``).  Needs a receiver with nothing in flight."""
        _lib.check(_lib.lib().rd_wb_set_parse(self._h, 1 if on else 0))

    def parsed(self) -> np.ndarray:
        """CRC-valid messages of the chunk the last ``fetch()`` returned, with their frequency errors (structured array
        of ``batch.RD_PARSED_DTYPE``; ``stream`` = channel, ``call`` = chunk) - the next chunk may be in flight, which
        ``discriminated(channel)`` does not allow."""
        from .dsp import _parsed_array
        return _parsed_array(_lib.lib().rd_wb_parsed, self._h)

    def retune(self, offset_hz) -> None:
        """From the next submitted chunk on, receive channel c as if its centre were ``channels_hz[c] + offset_hz[c]`` -
        the reference's ``channel_freq + freq_corr`` (runners/rtlsdr.py:51,72), so the ``freq_err`` values of ``parsed()``,
        averaged the caller's way (protocol.py:258-271), go in as they are.  ``offset_hz``: one integer for all channels or
        one per channel, relative to the constructed plan (not cumulative).  Phase-continuous at the chunk boundary, legal
        with chunks in flight, nothing else disturbed (filter history, clock, demodulators); only the tables of the
        channels that change are rebuilt, by a kernel in front of that chunk's channelizer.  ValueError for a wrong
        length or a channel pushed outside the captured band."""
        off = np.asarray(offset_hz)
        if off.dtype.kind not in "iu" or off.ndim > 1 or (off.ndim == 1 and off.size != self.n_channels):
            raise ValueError(f"offset_hz: one integer or {self.n_channels} of them")
        shift = np.ascontiguousarray(self._plan_shift_hz + off.astype(np.int64), np.int64)
        if shift.size and np.abs(shift).max() > self.wide_rate // 2:
            raise ValueError("a channel lies outside the captured band")
        _lib.check(_lib.lib().rd_wb_retune(self._h, shift.ctypes.data, shift.size))
        self.shift_hz = shift

    def tuning(self):
        """``(shift_hz, phase)``, int64 per channel: the mixer frequencies the next submitted chunk will use and the
        integer phase accumulators P_c that keep the phase continuous across retunes - the output phase of channel c at
        the absolute output time t is ``frac((shift_hz[c] * t + phase[c]) / out_rate)``."""
        shift = np.empty(self.n_channels, np.int64)
        phase = np.empty(self.n_channels, np.int64)
        _lib.check(_lib.lib().rd_wb_tuning(self._h, shift.ctypes.data, phase.ctypes.data, shift.size))
        return shift, phase

    def set_gain(self, gain) -> None:
        """From the next submitted chunk on, re-quantise channel c with ``gain[c]``: one positive number for all channels
        or one per channel - absolute values (not relative to the constructed ``gain``), stored as float32.  The change
        takes effect exactly at that chunk boundary, is legal with chunks in flight and disturbs nothing else (filter
        history, clock, tuning, demodulators); with every entry equal to the constructed gain the bytes are those of a
        receiver that never called it.  ValueError for a wrong length or a gain that is not finite and > 0.
        ``Packet.rssi`` is measured on the channel's bytes: referred to the input it is ``rssi - 20 log10(gain)``."""
        g = _lib.gain_array(gain, self.n_channels)
        _lib.check(_lib.lib().rd_wb_set_gain(self._h, g.ctypes.data, g.size))

    def gains(self) -> np.ndarray:
        """float64 per channel: the gains the next submitted chunk will use (exactly the float32 values in the table)."""
        g = np.empty(self.n_channels, np.float64)
        _lib.check(_lib.lib().rd_wb_gains(self._h, g.ctypes.data, g.size))
        return g

    def set_levels(self, on: bool = True) -> None:
        """From the next chunk on, meter every chunk on the device (one more kernel behind its channelizer); ``levels()``
        returns the records.  Needs a receiver with nothing in flight.  Off (the default): nothing is launched."""
        _lib.check(_lib.lib().rd_wb_set_levels(self._h, 1 if on else 0))

    def levels(self) -> "Levels":
        """Levels of the chunk the last ``fetch()`` returned - later chunks may be in flight - as exact integers:
        per channel, over the ``2 * block_size`` bytes b of its channelized chunk with a = 2 b - 255, ``peak`` = max |a|,
        ``clipped`` = bytes equal to 0 or 255, ``power`` = sum a^2, and ``gain``, the float32 in force for that chunk;
        the capture chunk's own record (``InputLevel``: how hard the ADC is driven); and the chunk's number.
        Conversions: a channel's RMS as a fraction of full scale is ``sqrt(power / (2 * block_size)) / 255``; the input's
        likewise with its component count (``2 * chunk_samples``) and 255 ("u8"), 128 ("s8") or 32768 ("s16", and "cf32",
        whose components are metered in int16 units: k = clip(rint(32768 v), -32768, 32767) of the value clamped to
        [-8, 8], a NaN counted as clipped and as the value 0).  ``agc.GainControl.update`` takes
        the result as it is.  RuntimeError before any fetch and when levels were off for that chunk."""
        recs = (_lib.RdChanLevel * self.n_channels)()
        inp = _lib.RdInputLevel()
        _lib.check(_lib.lib().rd_wb_levels(self._h, recs, self.n_channels, C.byref(inp)))
        raw = np.frombuffer(recs, dtype=np.dtype([("power", np.uint64), ("peak", np.uint32), ("clipped", np.uint32),
                                                  ("gain", np.float32), ("chunk", np.uint32)]))
        out = np.empty(self.n_channels, LEVEL_DTYPE)
        for f in LEVEL_DTYPE.names:
            out[f] = raw[f]
        return Levels(out, InputLevel(int(inp.peak), int(inp.clipped), int(inp.power)), int(inp.chunk))

    def set_spectrum(self, n_bins: Optional[int]) -> None:
        """From the next chunk on, compute every chunk's power spectrum on the device (one more kernel behind its
        channelizer; ``spectrum()`` returns it): ``n_bins`` a power of two in 64 .. 4096 and at most ``chunk_samples``;
        ``0`` or ``None`` switches it off (the default: nothing is launched).  Needs a receiver with nothing in flight
        (RuntimeError); ValueError for another value."""
        n = 0 if n_bins is None else n_bins
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
            raise ValueError("n_bins: 0 / None, or a power of two in 64 .. 4096")
        if not -2 ** 31 <= int(n) < 2 ** 31:
            raise ValueError("n_bins: 0 / None, or a power of two in 64 .. 4096")
        _lib.check(_lib.lib().rd_wb_set_spectrum(self._h, int(n)))
        self._spectrum_bins = int(n)

    def spectrum(self) -> "Spectrum":
        """Power spectrum of the chunk the last ``fetch()`` returned - later chunks may be in flight: Welch's method over
        the chunk's ``chunk_samples // n_bins`` whole windows of ``n_bins`` samples (periodic Hann, no overlap, the
        samples left over at the chunk's end unused), float32 per window, float64 across windows, scaled so that a
        full-scale complex tone on a bin centre reads 1.0 (0 dBFS); bit-identical from run to run.  RuntimeError before
        any fetch and when the spectrum was off for that chunk."""
        n = self._fetched_bins or 64                     # (the record's size: the setting when its chunk was fetched)
        power = np.empty(n, np.float64)
        info = _lib.RdSpectrumInfo()
        _lib.check(_lib.lib().rd_wb_spectrum(self._h, power.ctypes.data, n, C.byref(info)))
        return Spectrum(power, spectrum_freqs(self.centre_hz, self.wide_rate, n), int(info.segments), int(info.chunk))

    def set_bursts(self, on: bool = True) -> None:
        """From the next chunk on, look for bursts in every channel's channelized chunk on the device (one more kernel
        behind its channelizer); ``bursts()`` returns the records.  Needs a receiver with nothing in flight
        (RuntimeError); ValueError when ``block_size`` exceeds 4096 windows of 128 outputs.  Off (the default): nothing is
        launched."""
        _lib.check(_lib.lib().rd_wb_set_bursts(self._h, 1 if on else 0))

    def set_burst_threshold(self, thr) -> None:
        """From the next submitted chunk on, a window of channel c is ON when its energy reaches ``thr[c]``: one integer
        for all channels or one per channel, ``0 .. 2**32 - 1`` (the default, ``BURST_THRESHOLD_OFF``: never).  Takes
        effect exactly at that chunk boundary and is legal with chunks in flight; the table in force is echoed in
        ``bursts().floor["threshold"]``; ``reset()`` returns to the default.  ValueError for a wrong length or value."""
        t = np.asarray(thr)
        if t.dtype.kind not in "iu" or t.ndim > 1 or (t.ndim == 1 and t.size != self.n_channels):
            raise ValueError(f"thr: one integer or {self.n_channels} of them")
        if t.size and (int(t.min()) < 0 or int(t.max()) > BURST_THRESHOLD_OFF):
            raise ValueError("every threshold must lie in 0 .. 2**32 - 1")
        t = np.ascontiguousarray(np.broadcast_to(t, (self.n_channels,)), np.uint32)
        _lib.check(_lib.lib().rd_wb_set_burst_threshold(self._h, t.ctypes.data, t.size))

    def burst_thresholds(self) -> np.ndarray:
        """uint32 per channel: the thresholds the next submitted chunk will use."""
        t = np.empty(self.n_channels, np.uint32)
        _lib.check(_lib.lib().rd_wb_burst_thresholds(self._h, t.ctypes.data, t.size))
        return t

    def bursts(self) -> "Bursts":
        """Bursts of the chunk the last ``fetch()`` returned - later chunks may be in flight - as exact integers.  Per
        channel, over windows of 128 outputs of its channelized chunk (z = aI + j aQ, a = 2 b - 255): the window's energy
        ``p = sum |z|^2`` and lag-1 correlation ``r = sum z[t] conj(z[t-1])`` over the 127 pairs inside it.  A record is a
        maximal run of windows with ``p >= threshold``: ``channel``, ``first``, ``windows``, ``flags`` (bit 0: the run
        begins with the chunk, bit 1: it ends with it - ``acquire.merge`` joins the halves), ``power`` = sum p, ``peak`` =
        max p, ``corr_re`` / ``corr_im`` = sum r.  ``floor``: per channel the same sums over the other windows
        (``windows_off``, ``power_off``, ``corr_re_off``, ``corr_im_off``), the ``threshold`` in force and ``n_bursts``.
        ``acquire.burst_offset_hz`` turns a record into a frequency.  RuntimeError before any fetch and when bursts were
        off for that chunk."""
        L = _lib.lib()
        floor = np.empty(self.n_channels, BURST_FLOOR_DTYPE)
        n = C.c_int(0)
        recs = np.empty(self._burst_cap, BURST_DTYPE)
        rc = L.rd_wb_bursts(self._h, recs.ctypes.data, recs.size, C.byref(n), floor.ctypes.data, floor.size)
        if rc == _lib.RD_ERR_CAPACITY:  # nothing is lost: the handle keeps the records
            self._burst_cap = max(2 * self._burst_cap, n.value)
            recs = np.empty(self._burst_cap, BURST_DTYPE)
            rc = L.rd_wb_bursts(self._h, recs.ctypes.data, recs.size, C.byref(n), floor.ctypes.data, floor.size)
        _lib.check(rc)
        return Bursts(recs[: n.value].copy(), floor, int(floor["chunk"][0]))

    def set_burst_decode(self, on: bool = True) -> None:
        """From the next chunk on, decode every burst ``bursts()`` reports on the device (one more kernel behind the
        burst kernel): the discriminator is sliced around the burst's own mean frequency, so a packet decodes at any
        offset the channel filter passes, and sync word plus CRC prove that it is a message; ``burst_messages()``
        returns the records.  Needs a receiver with nothing in flight and ``set_bursts(True)`` (RuntimeError;
        ``set_bursts(False)`` switches it off too); ValueError unless the configuration has 16 preamble symbols,
        ``packet_symbols`` a multiple of 8 in 40 .. 80, ``packet_symbols * symbol_length + 1 <= 2048`` and ``block_size``
        at least that, rounded up to whole windows of 128.  Off (the default): nothing is launched."""
        _lib.check(_lib.lib().rd_wb_set_burst_decode(self._h, 1 if on else 0))

    def set_burst_repair(self, max_flips: int) -> None:
        """From the next chunk on, a burst whose sync word is right and whose CRC fails is repaired when flipping one
        (``max_flips`` 1) or up to two (2) of its 8 least reliable payload symbols - those with the smallest |matched
        filter output| - makes the CRC pass: singles first, then pairs, weakest first.  0 (the default) is the receiver
        without repair, byte for byte.  A repaired row of ``burst_messages()`` has ``flags`` bit 1 set
        (``BURST_MSG_REPAIRED``), ``pad[0]`` flips, ``pad[1] < pad[2]`` the flipped symbols, and ``data``, ``ones`` and
        ``id`` corrected; ``acquire.repaired`` and ``acquire.flipped_symbols`` read them.  An exact candidate of a run
        always wins over a repaired one, so every row without bit 1 is the row ``max_flips = 0`` gives.  A repaired row
        proves less than a CRC-proven one: a random candidate passes with up to 8 / 65535 (one flip) or 36 / 65535 (two)
        instead of 1 / 65536 - keep the two classes apart.  Needs a receiver with nothing in flight and
        ``set_burst_decode(True)`` (RuntimeError; switching decode or bursts off puts it back to 0, ``reset()`` keeps
        it); ValueError outside 0 .. 2 and for a bool."""
        if isinstance(max_flips, (bool, np.bool_)) or not isinstance(max_flips, (int, np.integer)):
            raise ValueError("max_flips: an integer in 0 .. 2")
        if not 0 <= int(max_flips) <= BURST_REPAIR_MAX_FLIPS:
            raise ValueError(f"max_flips {int(max_flips)}: 0 .. {BURST_REPAIR_MAX_FLIPS}")
        _lib.check(_lib.lib().rd_wb_set_burst_repair(self._h, int(max_flips)))

    def burst_repair(self) -> int:
        """``max_flips`` the next submitted chunk will use (0: repair off)."""
        r = C.c_int(0)
        _lib.check(_lib.lib().rd_wb_burst_repair(self._h, C.byref(r)))
        return int(r.value)

    def set_burst_narrow(self, on: bool = True) -> None:
        """From the next chunk on, every burst is band-passed at its own frequency before the discriminator: a filter
        of ``2 * symbol_length + 5`` integer taps, 0.9 symbol rates wide, centred on the nearest of 64 frequencies to the
        run's correlation sum (the kernel chooses, the row's ``pad[3]`` says which).  The channel filter passes +-110 kHz
        and a burst occupies +-15 kHz; without the filter the discriminator multiplies all of that noise with itself.  On
        the project's model of noisy bursts the noise level at which half of them decode rises from about 0.09 to about
        0.25 (profiles/burst_narrow_gain.txt).  Rows decoded this way have ``flags`` bit 2 set (``BURST_MSG_NARROW``;
        ``acquire.narrowband``); their ``margin`` and ``f_re`` / ``f_im`` are in the filter's units - do not compare a
        ``margin`` across the two kinds; ``acquire.burst_message_offset_hz`` uses the angle alone and holds for both.
        Repair composes with it.  Off (the default) is the receiver without it, byte for byte.  Needs a receiver with
        nothing in flight and ``set_burst_decode(True)`` (RuntimeError; switching decode or bursts off switches it off,
        ``reset()`` keeps it); ValueError for ``symbol_length`` below 4."""
        _lib.check(_lib.lib().rd_wb_set_burst_narrow(self._h, 1 if on else 0))

    def burst_narrow(self) -> bool:
        """Whether the next submitted chunk will be decoded behind the narrow-band filter."""
        r = C.c_int(0)
        _lib.check(_lib.lib().rd_wb_burst_narrow(self._h, C.byref(r)))
        return bool(r.value)

    def burst_messages(self) -> "BurstMessages":
        """Messages of the chunk the last ``fetch()`` returned - later chunks may be in flight - as exact integers.  Per
        run of ``bursts()`` of at most 32 windows (a run that begins with the chunk is extended LOOK_W windows back - a packet's
        length + 1 in whole windows, 9 for 14 samples per symbol, 6 for 8 - into the
        chunk before), at most one row: ``channel``, ``first`` (the run's), ``tau`` (the output at which the first symbol
        ends, relative to the chunk's first output - negative when the packet began in the chunk before; the packet ends
        in this chunk), ``flags`` (bit 0: the region reached into the previous chunk), ``time`` (``tau`` on the receiver's
        absolute output clock), ``margin`` (the least |matched filter output| among the symbols), ``f_re`` / ``f_im`` (the
        lag-1 correlation summed over the packet: ``acquire.burst_message_offset_hz`` turns it into a frequency),
        ``data`` (the on-air bytes, as ``Packet.data``: ``dsp.parse_packet`` takes them), ``ones`` and ``id``; ``pad`` is
        zero unless ``set_burst_repair`` is on and the row was repaired (``flags`` bit 1) or ``set_burst_narrow`` is on
        (``flags`` bit 2, ``pad[3]`` the filter's centre).  A burst
        the demodulator decodes as well is reported here and in ``parsed()``: dedupe by channel, chunk and data.
        A packet that ends within ``symbol_length`` outputs of a chunk boundary can be found by both chunks; the fetch
        drops the later chunk's look-back row when the fetch before it delivered the same ``channel`` and ``data`` less
        than ``symbol_length`` outputs away in ``time``, so the rows here hold every packet once.
        RuntimeError before any fetch and when decode was off for that chunk."""
        L = _lib.lib()
        long_runs = np.empty(self.n_channels, np.uint32)
        n = C.c_int(0)
        recs = np.empty(self._burst_cap, BURST_MSG_DTYPE)
        rc = L.rd_wb_burst_messages(self._h, recs.ctypes.data, recs.size, C.byref(n), long_runs.ctypes.data, long_runs.size)
        if rc == _lib.RD_ERR_CAPACITY:  # nothing is lost: the handle keeps the records
            self._burst_cap = max(2 * self._burst_cap, n.value)
            recs = np.empty(self._burst_cap, BURST_MSG_DTYPE)
            rc = L.rd_wb_burst_messages(self._h, recs.ctypes.data, recs.size, C.byref(n), long_runs.ctypes.data, long_runs.size)
        _lib.check(rc)
        chunk = C.c_uint64(0)                            # the chunk whose headers the fetch checked
        _lib.check(L.rd_wb_fetched_chunk(self._h, C.byref(chunk)))
        return BurstMessages(recs[: n.value].copy(), long_runs, int(chunk.value))

    def set_burst_expect(self, table) -> None:
        """From the next submitted chunk on, exactly at that boundary, also decode at the places ``table`` names, with no
        energy gate: rows of ``EXPECT_DTYPE`` (at most ``BURST_EXPECT_MAX``; an empty table clears it) - ``channel``,
        ``id`` (0 .. 7: only that transmitter's message; ``BURST_EXPECT_ANY_ID``), ``t_lo .. t_hi`` (the window, inclusive,
        on the receiver's absolute output clock, for the END of the packet's first symbol - ``time`` of a message row;
        at most ``BURST_EXPECT_MAX_SPAN`` wide) and ``corr_re, corr_im`` (the direction to slice around, each in
        ``-2**15 .. 2**15 - 1``: ``round(2**14 e^{j 2 pi f / out_rate})`` for a carrier at f Hz in the channel's bytes).
        ``track.Tracker`` makes such tables from the messages already received.  Legal with chunks in flight; calls before
        a submit collapse into the last.  ``set_burst_repair`` and ``set_burst_narrow`` apply to expectations too.
        ValueError for a table that breaks a rule (nothing changes); RuntimeError unless ``set_burst_decode(True)``;
        switching decode or bursts off and ``reset()`` clear the table."""
        t = np.ascontiguousarray(np.asarray(table, EXPECT_DTYPE).reshape(-1))
        _lib.check(_lib.lib().rd_wb_set_burst_expect(self._h, t.ctypes.data if t.size else None, t.size))

    def burst_expect(self) -> np.ndarray:
        """The table the next submitted chunk will use (``EXPECT_DTYPE``)."""
        t = np.empty(BURST_EXPECT_MAX, EXPECT_DTYPE)
        n = C.c_int(0)
        _lib.check(_lib.lib().rd_wb_burst_expect(self._h, t.ctypes.data, t.size, C.byref(n)))
        return t[: n.value].copy()

    def expected_messages(self) -> "ExpectedMessages":
        """The messages found at the expectations in the chunk the last ``fetch()`` returned - rows like those of
        ``burst_messages()`` with ``flags`` bit 3 (``BURST_MSG_EXPECTED``) set, ``first`` the expectation's index in the
        table that chunk was submitted with and ``flags`` bit 0 meaning that the searched region began before the
        chunk - and per expectation the number of candidate positions it had in the chunk.  A packet whose window
        straddles a chunk boundary can be found from both sides; the fetch drops the later chunk's row when the fetch
        before it delivered the same ``channel`` and ``data`` less than ``symbol_length`` outputs away.  The same packet
        may also appear in ``parsed()`` and ``burst_messages()``: dedupe by channel, time and data.  A chunk submitted
        with an empty table gives no rows.  RuntimeError before any fetch and when decode was off for that chunk."""
        L = _lib.lib()
        cand = np.empty(BURST_EXPECT_MAX, np.uint32)
        recs = np.empty(BURST_EXPECT_MAX, BURST_MSG_DTYPE)
        n = C.c_int(0)
        _lib.check(L.rd_wb_expected_messages(self._h, recs.ctypes.data, recs.size, C.byref(n), cand.ctypes.data, cand.size))
        chunk = C.c_uint64(0)
        _lib.check(L.rd_wb_fetched_chunk(self._h, C.byref(chunk)))
        return ExpectedMessages(recs[: n.value].copy(), cand[cand != 0xFFFFFFFF].copy(), int(chunk.value))

    def set_burst_search(self, centres) -> None:
        """From the next submitted chunk on, also search EVERY output position of every channel for the sync word and a
        valid CRC behind the narrow-band filter, once per centre of ``centres`` (at most ``BURST_SEARCH_MAX_CENTRES``
        distinct grid points 0 .. 63, g / 64 cycles per output; ``acquire.search_centres`` makes the list; an empty list,
        the default, switches the search off and nothing is launched).  No energy threshold and no earlier message is
        needed: this is how a station never yet heard is found when it is too weak for ``burst_messages()``.  It costs one
        filter pass over every channel per centre and chunk.  Legal with chunks in flight.  ValueError for a centre above
        63, a duplicate, more than eight, or ``symbol_length < 4`` (nothing changes); RuntimeError unless
        ``set_burst_decode(True)``; switching decode or bursts off clears the list, ``reset()`` keeps it."""
        t = np.asarray(centres).reshape(-1)
        if t.size and (np.any(t < 0) or np.any(t > 255) or np.any(t != np.floor(t))):
            raise ValueError("burst search: centres are grid points 0 .. 63")
        t = np.ascontiguousarray(t.astype(np.uint8))
        _lib.check(_lib.lib().rd_wb_set_burst_search(self._h, t.ctypes.data if t.size else None, t.size))

    def burst_search(self) -> np.ndarray:
        """The centres the next submitted chunk will use (uint8)."""
        t = np.empty(BURST_SEARCH_MAX_CENTRES, np.uint8)
        n = C.c_int(0)
        _lib.check(_lib.lib().rd_wb_burst_search(self._h, t.ctypes.data, t.size, C.byref(n)))
        return t[: n.value].copy()

    def searched_messages(self) -> "SearchedMessages":
        """The messages the blind search found in the chunk the last ``fetch()`` returned - rows like those of
        ``burst_messages()`` with ``flags`` bit 4 (``BURST_MSG_SEARCHED``) and bit 2 set, ``first`` the centre's index in
        the list that chunk was submitted with, ``pad[0]`` the number of adjacent positions that passed (about
        ``symbol_length - 2`` for a real packet, 1 for a chance hit) and ``pad[3]`` the centre.  A searched row proves less
        than any other: with every position tested, sync word and CRC pass by chance every few minutes per centre -
        ``track.Tracker`` holds a station seeded by one as provisional until an expectation confirms it.  A packet found
        from both sides of a chunk boundary is dropped from the later chunk; two centres that both decode a packet each
        give their row: dedupe by channel, time and data.  A chunk submitted with an empty list gives no rows.
        RuntimeError before any fetch and when decode was off for that chunk."""
        L = _lib.lib()
        n_ch = self.n_channels
        hdr = np.empty(BURST_SEARCH_MAX_CENTRES * n_ch, SEARCH_HDR_DTYPE)
        recs = np.empty(BURST_SEARCH_MAX_CENTRES * n_ch * BURST_SEARCH_PER, BURST_MSG_DTYPE)
        n = C.c_int(0)
        _lib.check(L.rd_wb_searched_messages(self._h, recs.ctypes.data, recs.size, C.byref(n), hdr.ctypes.data, hdr.size))
        chunk = C.c_uint64(0)
        _lib.check(L.rd_wb_fetched_chunk(self._h, C.byref(chunk)))
        hdr = hdr.reshape(BURST_SEARCH_MAX_CENTRES, n_ch)
        hdr = hdr[hdr["n_msgs"][:, 0] != 0xFFFFFFFF]
        return SearchedMessages(recs[: n.value].copy(), hdr["sync_hits"].copy(), hdr["dropped"].copy(), int(chunk.value))

    def set_burst_quality(self, on: bool = True, noise_gap: int = 0) -> None:
        """From the next chunk on, every row of ``burst_messages()`` and ``expected_messages()`` gets a row of
        ``QUALITY_DTYPE``, exact integers in the units of the channelized bytes (a = 2 b - 255): ``pkt`` / ``sig`` /
        ``noise`` are the sums of |z|^2 over the packet, its 16 sync symbols and the ``n_noise`` outputs that end
        ``noise_gap`` outputs in front of the packet (the reference's noise window at ``noise_gap = 0``; cut at the start
        of the chunk before, possibly to nothing); ``peak`` and ``clipped`` are the largest component and the bytes at 0
        or 255 inside the packet; ``pkt_nb`` / ``sig_nb`` / ``noise_nb`` (``flags`` bit 0) are the same sums behind the
        narrow-band filter of ``set_burst_narrow`` centred at ``g`` / 64 cycles per output, chosen from the row's own
        ``f_re, f_im`` - whether or not the row was decoded behind that filter.  ``acquire.rssi_db``, ``snr_db``,
        ``snr_inband_db`` and ``snr_floor_db`` turn a row into decibels, ``burst_packets`` into ``Packet``s.  What a
        transmitter sends in front of its sync word has not been measured in this project: ``noise_gap`` (0 .. 1024) moves
        the window further out, and ``snr_floor_db`` does without it.  Off (the default) is the receiver without it, byte
        for byte.  Needs a receiver with nothing in flight and ``set_burst_decode(True)`` (RuntimeError; switching decode
        or bursts off switches it off, ``reset()`` keeps it); ValueError for a ``noise_gap`` out of range."""
        _lib.check(_lib.lib().rd_wb_set_burst_quality(self._h, 1 if on else 0, int(noise_gap)))

    def burst_quality(self):
        """``(on, noise_gap)`` the next submitted chunk will use."""
        on, gap = C.c_int(0), C.c_int(0)
        _lib.check(_lib.lib().rd_wb_burst_quality(self._h, C.byref(on), C.byref(gap)))
        return bool(on.value), int(gap.value)

    def _quality_rows(self, fn) -> np.ndarray:
        n = C.c_int(0)
        rc = fn(self._h, None, 0, C.byref(n))
        if rc != _lib.RD_ERR_CAPACITY:
            _lib.check(rc)
        out = np.empty(n.value, QUALITY_DTYPE)
        if out.size:
            _lib.check(fn(self._h, out.ctypes.data, out.size, C.byref(n)))
        return out

    def burst_message_quality(self) -> np.ndarray:
        """``QUALITY_DTYPE`` rows parallel to ``burst_messages().records`` of the same fetch (a row the fetch dropped as a
        repeat took its quality with it).  RuntimeError before any fetch and when quality was off for that chunk."""
        return self._quality_rows(_lib.lib().rd_wb_burst_message_quality)

    def expected_message_quality(self) -> np.ndarray:
        """``QUALITY_DTYPE`` rows parallel to ``expected_messages().records`` of the same fetch."""
        return self._quality_rows(_lib.lib().rd_wb_expected_message_quality)

    def set_burst_clips(self, sources: int = CLIP_RUNS | CLIP_MESSAGES, pre: int = 256, post: int = 128,
                        quota: int = 4096) -> None:
        """From the next chunk on, the device cuts the channelized IQ of every burst out of the chunk and ``burst_clips()``
        hands it over: with ``CLIP_RUNS`` the outputs of every run of ``bursts()``, with ``CLIP_MESSAGES`` the packet of
        every row the decode, expect and search kernels wrote (before the fetch drops repeats), each with ``pre`` outputs
        in front and ``post`` behind (multiples of 8, 0 .. 1024).  A request that begins before the chunk takes the bytes
        from the chunk before; one that ends behind it is completed by the first clip (source 0, the tail) of the next
        chunk.  ``quota`` (a multiple of 8, 8 .. 65536, ``n_channels * quota * 2 <= 2**26``) is the room per channel and
        chunk in outputs; a request that does not fit is dropped whole and counted.  Overlapping requests each get their
        own copy - ``clips.ClipStitcher`` merges them into recordings.  ``sources = 0`` (the default) is the receiver
        without it, byte for byte.  ValueError for a value out of range; RuntimeError unless nothing is in flight and
        ``set_bursts(True)``, and for ``CLIP_MESSAGES`` unless ``set_burst_decode(True)``.  Switching bursts off switches
        clips off, switching decode off clears ``CLIP_MESSAGES``; ``reset()`` keeps the settings."""
        _lib.check(_lib.lib().rd_wb_set_burst_clips(self._h, int(sources), int(pre), int(post), int(quota)))

    def burst_clips_config(self):
        """``(sources, pre, post, quota)`` the next submitted chunk will use."""
        v = [C.c_int(0) for _ in range(4)]
        _lib.check(_lib.lib().rd_wb_burst_clips_config(self._h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def burst_clips(self) -> BurstClips:
        """The clips of the chunk the last fetch returned (``BurstClips``), kept by that fetch: valid with later chunks in
        flight, until the next fetch.  A clip is matched to a message row by ``(channel, ref == row["time"])``, to a run by
        ``(channel, source == CLIP_SOURCE_RUN, ref == first)``.  RuntimeError before any fetch and when that chunk was
        submitted with clips off."""
        L = _lib.lib()
        n, nb = C.c_int(0), C.c_size_t(0)
        dropped = np.zeros(self.n_channels, np.uint32)
        rc = L.rd_wb_burst_clips(self._h, None, 0, C.byref(n), None, 0, C.byref(nb), dropped.ctypes.data, dropped.size)
        if rc != _lib.RD_ERR_CAPACITY:
            _lib.check(rc)
        recs = np.zeros(max(n.value, 1), CLIP_DTYPE)
        iq = np.zeros(max(nb.value, 2), np.uint8)
        _lib.check(L.rd_wb_burst_clips(self._h, recs.ctypes.data, recs.size, C.byref(n), iq.ctypes.data, iq.size, C.byref(nb),
                                       dropped.ctypes.data, dropped.size))
        chunk = C.c_uint64(0)
        _lib.check(L.rd_wb_fetched_chunk(self._h, C.byref(chunk)))
        return BurstClips(recs[: n.value].copy(), iq[: nb.value].reshape(-1, 2).copy(), dropped, int(chunk.value))

    def reset(self) -> None:
        """Back to the state after construction: clock at 0, zero history, demodulators reset, the constructed channel
        plan (a pending or earlier ``retune`` is dropped), the constructed gain (``set_gain`` likewise) and the default
        burst thresholds."""
        _lib.check(_lib.lib().rd_wideband_reset(self._h))
        self._fetched_bins = 0
        self._submitted = 0
        self.shift_hz = self._plan_shift_hz.copy()

    def channelized(self) -> np.ndarray:
        """uint8 [n_channels, 2*block_size]: the channelized chunk the last fetch returned (until the next submit)."""
        out = np.empty((self.n_channels, 2 * self.block_size), np.uint8)
        _lib.check(_lib.lib().rd_wideband_copy_channelized(self._h, out.ctypes.data, out.size))
        return out

    def discriminated(self, channel: int) -> np.ndarray:
        """``Demodulator.discriminated`` of one channel (for the reference's frequency-error step)."""
        out = np.empty(2 * self.block_size, dtype=np.float64)
        _lib.check(_lib.lib().rd_wideband_copy_discriminated(self._h, int(channel), out.ctypes.data, out.size))
        return out

    def _debug_advance_clock(self, n_out: int) -> None:
        """Test hook (quiet receiver): move the output clock on by n_out (a multiple of 128), history kept."""
        _lib.check(_lib.lib().rd_wideband_debug_advance_clock(self._h, int(n_out)))
