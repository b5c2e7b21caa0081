"""Wideband front end: one IQ capture (uint8, int8, int16 or float32) -> one 268.8 kSPS uint8 IQ stream
per hop channel, channelized on the GPU straight into a BatchDemodulator's input buffer.

rtldavis itself has no channelizer: it retunes one narrow-band dongle per hop
(/root/reference/src/rtldavis/runners/rtlsdr.py:51,72), so parity is unpinned.  The arithmetic is
defined in csrc/rd_channelizer.hip; oracle/channelizer_oracle.py restates it in float64 for the tests.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib

# protocol.py:119-171 (US band): 51 hop channels, 501.75 kHz apart
US_CHANNELS_HZ = (
    902419338, 902921088, 903422839, 903924589, 904426340, 904928090, 905429841, 905931591, 906433342,
    906935092, 907436843, 907938593, 908440344, 908942094, 909443845, 909945595, 910447346, 910949096,
    911450847, 911952597, 912454348, 912956099, 913457849, 913959599, 914461350, 914963100, 915464850,
    915966601, 916468351, 916970102, 917471852, 917973603, 918475353, 918977104, 919478854, 919980605,
    920482355, 920984106, 921485856, 921987607, 922489357, 922991108, 923492858, 923994609, 924496359,
    924998110, 925499860, 926001611, 926503361, 927005112, 927506862,
)
OUT_RATE = 268800          # 19200 bit/s x 14 samples per symbol (protocol.py:68-76, :309)
DEFAULT_DECIM = 100        # 26.88 MS/s covers the 25.1 MHz the 51 channels span
DEFAULT_CENTRE_HZ = 914963100


def design_taps(n_taps: int = 512, cutoff_hz: float = 110e3, wide_rate: float = OUT_RATE * DEFAULT_DECIM,
                beta: float = 7.0) -> np.ndarray:
    """Kaiser-windowed sinc low-pass, unit DC gain (float64).  The defaults pass the channel
    (carrier at -67.2 kHz +- deviation and data) and stop the neighbours 501.75 kHz away (~-70 dB),
    whose aliases would otherwise land beside it after the decimation."""
    n = np.arange(n_taps) - (n_taps - 1) / 2.0
    h = np.sinc(2.0 * cutoff_hz / wide_rate * n) * np.kaiser(n_taps, beta)
    return h / h.sum()


def plan_channels(obj, channels_hz: Sequence[int], centre_hz: int, decim: int, taps: Optional[np.ndarray], gain: float,
                  out_rate: int, if_hz: Optional[int] = None) -> None:
    """The channel plan shared by Channelizer and wideband.WidebandReceiver: sets out_rate, decim, wide_rate, if_hz,
    taps (float64), gain, shift_hz (int64: the wideband frequency that lands on 0 Hz of each channel's output) and
    n_channels on ``obj``; ValueError for a decimation or rate below 1 and for a channel outside the captured band."""
    obj.out_rate = int(out_rate)
    obj.decim = int(decim)
    if obj.decim < 1 or obj.out_rate < 1:
        raise ValueError("decim and out_rate must be positive")
    obj.wide_rate = obj.out_rate * obj.decim
    obj.if_hz = -obj.out_rate // 4 if if_hz is None else int(if_hz)
    obj.taps = np.ascontiguousarray(design_taps(wide_rate=obj.wide_rate) if taps is None else taps, np.float64)
    obj.gain = float(gain)
    # the wideband frequency that lands on 0 Hz of the output: channel offset minus the IF
    obj.shift_hz = np.ascontiguousarray([int(f) - int(centre_hz) - obj.if_hz for f in channels_hz], np.int64)
    obj.n_channels = obj.shift_hz.size
    if obj.n_channels and np.abs(obj.shift_hz).max() > obj.wide_rate // 2:
        raise ValueError("a channel lies outside the captured band")


def chan_config(plan) -> _lib.RdChanConfig:
    """rd_chan_config of a plan made by plan_channels."""
    return _lib.RdChanConfig(plan.out_rate, plan.decim, int(plan.taps.size), int(plan.n_channels), plan.gain)


class Channelizer:
    """``Channelizer(channels_hz, centre_hz)`` moves each channel's centre to -out_rate/4, where the
    demodulator's Fs/4 rotation (dsp.py:42-49) expects the carrier, low-passes, decimates by
    ``decim`` and re-quantises to uint8 with ``gain``.  ``sample_format`` is the capture's: ``"u8"`` (RTL-SDR offset
    bytes, x = (k - 127.4) / 127.6), ``"s8"`` (int8, x = k / 128), ``"s16"`` (int16, x = k / 32768) or ``"cf32"``
    (float32 I,Q or ``complex64``, nominal full scale 1.0: x = the value itself, clamped to [-8, 8], a NaN taken as 0)."""

    def __init__(self, channels_hz: Sequence[int] = US_CHANNELS_HZ, centre_hz: int = DEFAULT_CENTRE_HZ,
                 decim: int = DEFAULT_DECIM, taps: Optional[np.ndarray] = None, gain: float = 3.0,
                 out_rate: int = OUT_RATE, if_hz: Optional[int] = None, sample_format: str = "u8") -> None:
        self._h = C.c_void_p()
        self.sample_format = sample_format
        self._fmt, self.dtype = _lib.sample_format(sample_format)
        plan_channels(self, channels_hz, centre_hz, decim, taps, gain, out_rate, if_hz)
        self.centre_hz = int(centre_hz)
        _lib.check(_lib.lib().rd_chan_create_fmt(C.byref(chan_config(self)), self._fmt, self.taps.ctypes.data,
                                                 self.shift_hz.ctypes.data, C.byref(self._h)))
        self.n_wide = 0

    def __del__(self):
        try:
            if self._h:
                _lib.lib().rd_chan_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def set_gain(self, gain) -> None:
        """Re-quantise channel c with ``gain[c]`` in the runs that follow: one positive number for all channels or one
        per channel, absolute values that replace the constructed ``gain`` (stored as float32).  With every entry equal
        to the constructed gain the bytes do not change.  ValueError for a wrong length or a gain that is not finite and
        > 0.  Call it between runs whose results have been taken (``run_host``, or a synchronised ``run_into``)."""
        g = _lib.gain_array(gain, self.n_channels)
        _lib.check(_lib.lib().rd_chan_set_gain(self._h, g.ctypes.data, g.size))

    def upload(self, wide_iq: np.ndarray) -> None:
        """Copy a capture (``self.dtype``, I,Q interleaved: flat or [n, 2]; ``"cf32"`` also ``complex64`` [n]) to the
        device."""
        a = _lib.iq_array(wide_iq, self.dtype)
        _lib.check(_lib.lib().rd_chan_upload(self._h, a.ctypes.data, a.nbytes))
        self.n_wide = a.size // 2

    def run_host(self, n_out: Optional[int] = None) -> np.ndarray:
        """Channelized streams as a host array uint8 [n_channels, 2*n_out]."""
        n_out = self.n_wide // self.decim if n_out is None else int(n_out)
        out = np.empty((self.n_channels, 2 * n_out), np.uint8)
        _lib.check(_lib.lib().rd_chan_run_host(self._h, n_out, out.ctypes.data, out.size))
        return out

    def spectrum(self, n_bins: int):
        """Power spectrum of the uploaded capture as ``wideband.Spectrum`` (``chunk`` = 0): what
        ``WidebandReceiver.spectrum()`` gives for a chunk, over the capture's ``n_wide // n_bins`` whole windows - for a
        chunk uploaded alone the same bits.  ``n_bins``: a power of two in 64 .. 4096, at most ``n_wide`` (ValueError);
        RuntimeError without an uploaded capture."""
        from .wideband import Spectrum, spectrum_freqs
        if isinstance(n_bins, bool) or not isinstance(n_bins, (int, np.integer)) or not 64 <= int(n_bins) <= 4096 \
                or int(n_bins) & (int(n_bins) - 1):
            raise ValueError("n_bins: a power of two in 64 .. 4096")
        n = int(n_bins)
        power = np.empty(n, np.float64)
        seg = C.c_uint32(0)
        _lib.check(_lib.lib().rd_chan_spectrum(self._h, n, power.ctypes.data, C.byref(seg)))
        return Spectrum(power, spectrum_freqs(self.centre_hz, self.wide_rate, n), int(seg.value), 0)

    def run_into(self, bd, hip_stream: int = 0) -> None:
        """Channelize straight into a BatchDemodulator's resident input (n_streams == n_channels)."""
        if bd.n_streams != self.n_channels:
            raise ValueError("Incompatible array sizes")
        ptr, nbytes = bd.input_ptr()
        _lib.check(_lib.lib().rd_chan_run(self._h, bd.n_samples, ptr, 2 * bd.n_samples, hip_stream))
