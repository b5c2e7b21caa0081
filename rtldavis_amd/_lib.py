"""ctypes binding of librtldavis_hip.so (include/rtldavis_hip.h).

There is no CPU fallback: if the shared library is missing this module raises at import
of the symbol table, and every compute call raises ``HipError`` when no MI355X is usable.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# RTLDAVIS_HIP_LIB overrides the path (A/B builds of the kernels); the default is the in-tree build
LIB_PATH = os.environ.get("RTLDAVIS_HIP_LIB") or os.path.join(HERE, "librtldavis_hip.so")

RD_MAX_PREAMBLE = 64
RD_MAX_PKT_BYTES = 32
RD_OK, RD_ERR_ARG, RD_ERR_DEVICE, RD_ERR_CAPACITY, RD_ERR_STATE = 0, -1, -2, -3, -4


class HipError(RuntimeError):
    """A HIP/device failure reported by librtldavis_hip (never swallowed, never retried on CPU)."""


class RdConfig(C.Structure):
    _fields_ = [("bit_rate", C.c_int32), ("symbol_length", C.c_int32), ("preamble_symbols", C.c_int32),
                ("packet_symbols", C.c_int32), ("block_size", C.c_int32), ("preamble", C.c_uint8 * RD_MAX_PREAMBLE)]


class RdPacket(C.Structure):
    _fields_ = [("stream", C.c_int32), ("call", C.c_int32), ("index", C.c_int32), ("nbytes", C.c_int32),
                ("data", C.c_uint8 * RD_MAX_PKT_BYTES), ("rssi", C.c_double), ("snr", C.c_double)]


class RdParsed(C.Structure):
    _fields_ = [("stream", C.c_int32), ("call", C.c_int32), ("index", C.c_int32), ("freq_err", C.c_int32),
                ("id", C.c_int32), ("nbytes", C.c_int32), ("data", C.c_uint8 * RD_MAX_PKT_BYTES),
                ("rssi", C.c_double), ("snr", C.c_double)]


class RdTiming(C.Structure):
    _fields_ = [("demod_ms", C.c_float), ("fixup_ms", C.c_float), ("search_ms", C.c_float),
                ("slice_ms", C.c_float), ("total_ms", C.c_float), ("runs", C.c_int32)]


class RdChanConfig(C.Structure):
    _fields_ = [("out_rate", C.c_int32), ("decim", C.c_int32), ("n_taps", C.c_int32), ("n_channels", C.c_int32),
                ("gain", C.c_double)]


class RdChanLevel(C.Structure):
    _fields_ = [("power", C.c_uint64), ("peak", C.c_uint32), ("clipped", C.c_uint32), ("gain", C.c_float),
                ("chunk", C.c_uint32)]


class RdInputLevel(C.Structure):
    _fields_ = [("power", C.c_uint64), ("chunk", C.c_uint64), ("peak", C.c_uint32), ("clipped", C.c_uint32)]


class RdSpectrumInfo(C.Structure):
    _fields_ = [("chunk", C.c_uint64), ("segments", C.c_uint32), ("n_bins", C.c_uint32)]


class RdBurst(C.Structure):
    _fields_ = [("channel", C.c_int32), ("first", C.c_uint32), ("windows", C.c_uint32), ("flags", C.c_uint32),
                ("power", C.c_uint64), ("peak", C.c_uint32), ("pad", C.c_uint32), ("corr_re", C.c_int64),
                ("corr_im", C.c_int64)]


class RdBurstFloor(C.Structure):
    _fields_ = [("threshold", C.c_uint32), ("windows_off", C.c_uint32), ("n_bursts", C.c_uint32), ("chunk", C.c_uint32),
                ("power_off", C.c_uint64), ("corr_re_off", C.c_int64), ("corr_im_off", C.c_int64)]


RD_BURST_MSG_BYTES = 10


class RdBurstMsg(C.Structure):
    _fields_ = [("channel", C.c_int32), ("first", C.c_uint32), ("tau", C.c_int32), ("flags", C.c_uint32),
                ("time", C.c_uint64), ("margin", C.c_uint64), ("f_re", C.c_int64), ("f_im", C.c_int64),
                ("data", C.c_uint8 * RD_BURST_MSG_BYTES), ("ones", C.c_uint8), ("id", C.c_uint8), ("pad", C.c_uint8 * 4)]


class RdBurstClip(C.Structure):
    _fields_ = [("channel", C.c_int32), ("source", C.c_uint32), ("flags", C.c_uint32), ("t0", C.c_int32), ("n", C.c_uint32),
                ("offset", C.c_uint32), ("time", C.c_uint64), ("ref", C.c_uint64), ("chunk", C.c_uint32), ("pad", C.c_uint32)]


# rtldavis_hip.h RD_IQ_*: the sample formats of a wideband capture, name -> (code, numpy dtype of one component)
# (code 3 is unassigned and there is no "f32": float32 I/Q is "cf32", code 4)
RD_IQ_U8, RD_IQ_S8, RD_IQ_S16, RD_IQ_CF32 = 0, 1, 2, 4
SAMPLE_FORMATS = {"u8": (RD_IQ_U8, np.uint8), "s8": (RD_IQ_S8, np.int8), "s16": (RD_IQ_S16, np.int16),
                  "cf32": (RD_IQ_CF32, np.float32)}


def sample_format(name):
    """(code, dtype) of a sample format name; ValueError for an unknown one."""
    try:
        return SAMPLE_FORMATS[name]
    except (KeyError, TypeError):
        raise ValueError(f"unknown sample format {name!r}: one of {sorted(SAMPLE_FORMATS)}") from None


def iq_array(a, dtype):
    """A capture as a flat contiguous array of ``dtype`` (I,Q interleaved; [n, 2] or flat in).  Integer arrays of
    another width whose values fit are converted; anything else (complex, float, out of range) is a ValueError -
    never a silent cast.  (uint8 keeps the conversion it always had: numpy's cast.)  A float32 capture ("cf32") is
    complex64 of shape [n], viewed as its float32 pairs without a copy, or float32, flat or [n, 2]; nothing else -
    complex128, float64 and integers included."""
    if np.dtype(dtype) == np.uint8:
        return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
    a = np.asarray(a)
    if np.dtype(dtype) == np.float32:
        if a.dtype == np.complex64 and a.ndim == 1:
            return np.ascontiguousarray(a).view(np.float32)
        if a.dtype == np.float32 and (a.ndim == 1 or (a.ndim == 2 and a.shape[1] == 2)):
            return np.ascontiguousarray(a).reshape(-1)
        raise ValueError(f"a {a.dtype} array of shape {a.shape} is not a capture of float32 I,Q samples "
                         "(complex64 [n], or float32 flat or [n, 2])")
    if a.dtype != dtype:
        info = np.iinfo(dtype)
        if a.dtype.kind not in "iu" or (a.size and (a.min() < info.min or a.max() > info.max)):
            raise ValueError(f"a {a.dtype} array is not a capture of {np.dtype(dtype).name} samples")
        a = a.astype(dtype)
    return np.ascontiguousarray(a).reshape(-1)


# name -> (restype, argtypes); exactly the functions include/rtldavis_hip.h declares
_P = C.c_void_p
SIGNATURES = {
    "rd_last_error": (C.c_char_p, []),
    "rd_device_count": (C.c_int, []),
    "rd_set_device": (C.c_int, [C.c_int]),
    "rd_set_wait_timeout_ms": (C.c_int, [C.c_int]),
    "rd_set_input_push": (C.c_int, [C.c_int]),
    "rd_demod_input_mode": (C.c_int, [C.c_void_p]),
    "rd_create": (C.c_int, [C.POINTER(RdConfig), C.POINTER(_P)]),
    "rd_create_multi": (C.c_int, [C.POINTER(RdConfig), C.c_int, C.POINTER(_P)]),
    "rd_demod_blocks": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(RdPacket), C.c_int, C.POINTER(C.c_int)]),
    "rd_copy_discriminated_stream": (C.c_int, [_P, C.c_int, _P, C.c_size_t]),
    "rd_demod_submit": (C.c_int, [_P, _P, C.c_size_t, C.c_int]),
    "rd_demod_register_input": (C.c_int, [_P, _P, C.c_size_t]),
    "rd_demod_submit_from": (C.c_int, [_P, C.c_size_t, C.c_size_t, C.c_int]),
    "rd_demod_fetch": (C.c_int, [_P, C.POINTER(RdPacket), C.c_int, C.POINTER(C.c_int)]),
    "rd_demod_refetch": (C.c_int, [_P, C.POINTER(RdPacket), C.c_int, C.POINTER(C.c_int)]),
    "rd_demod_inflight": (C.c_int, [_P]),
    "rd_demod_set_parse": (C.c_int, [_P, C.c_int]),
    "rd_demod_parsed": (C.c_int, [_P, C.POINTER(RdParsed), C.c_int, C.POINTER(C.c_int)]),
    "rd_parse_packet": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int)]),
    "rd_destroy": (None, [_P]),
    "rd_reset": (C.c_int, [_P]),
    "rd_demod_block": (C.c_int, [_P, _P, C.c_size_t, C.c_int, C.POINTER(RdPacket), C.c_int, C.POINTER(C.c_int)]),
    "rd_copy_discriminated": (C.c_int, [_P, _P, C.c_size_t]),
    "rd_copy_filtered": (C.c_int, [_P, _P, C.c_size_t]),
    "rd_copy_quantized": (C.c_int, [_P, _P, C.c_size_t]),
    "rd_batch_create": (C.c_int, [C.POINTER(RdConfig), C.c_int, C.c_int, C.POINTER(_P)]),
    "rd_batch_destroy": (None, [_P]),
    "rd_batch_input_ptr": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "rd_batch_upload": (C.c_int, [_P, _P, C.c_size_t]),
    "rd_batch_upload_async": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "rd_batch_run": (C.c_int, [_P, _P]),
    "rd_batch_results": (C.c_int, [_P, C.POINTER(RdPacket), C.c_int, C.POINTER(C.c_int)]),
    "rd_batch_copy_bits": (C.c_int, [_P, C.c_int, _P, C.c_size_t]),
    "rd_batch_copy_discriminated": (C.c_int, [_P, C.c_int, C.c_size_t, _P, C.c_size_t]),
    "rd_batch_set_parse": (C.c_int, [_P, C.c_int]),
    "rd_batch_parsed": (C.c_int, [_P, C.POINTER(RdParsed), C.c_int, C.POINTER(C.c_int)]),
    "rd_batch_set_timing": (C.c_int, [_P, C.c_int]),
    "rd_batch_set_pipelined": (C.c_int, [_P, C.c_int]),
    "rd_batch_last_run_forms": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "rd_batch_get_timing": (C.c_int, [_P, C.POINTER(RdTiming)]),
    "rd_batch_get_counters": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rd_k1_schedule": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rd_lut_execute": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t]),
    "rd_rotate_fs4": (C.c_int, [_P, _P, C.c_size_t]),
    "rd_fir9": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t]),
    "rd_discriminate": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t]),
    "rd_quantize": (C.c_int, [_P, _P, C.c_size_t]),
    "rd_search": (C.c_int, [C.POINTER(RdConfig), _P, C.c_size_t, _P, C.c_int, C.POINTER(C.c_int)]),
    "rd_chan_create": (C.c_int, [C.POINTER(RdChanConfig), _P, _P, C.POINTER(_P)]),
    "rd_chan_create_fmt": (C.c_int, [C.POINTER(RdChanConfig), C.c_int, _P, _P, C.POINTER(_P)]),
    "rd_chan_destroy": (None, [_P]),
    "rd_chan_upload": (C.c_int, [_P, _P, C.c_size_t]),
    "rd_chan_input_ptr": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "rd_chan_run": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, _P]),
    "rd_chan_run_host": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t]),
    "rd_chan_set_gain": (C.c_int, [_P, _P, C.c_int]),
    "rd_chan_spectrum": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_uint32)]),
    "rd_chan_spectrum_dev": (C.c_int, [_P, C.c_int, _P, _P]),
    "rd_wideband_create": (C.c_int, [C.POINTER(RdConfig), C.POINTER(RdChanConfig), _P, _P, C.POINTER(_P)]),
    "rd_wb_create_fmt": (C.c_int, [C.POINTER(RdConfig), C.POINTER(RdChanConfig), C.c_int, _P, _P, C.POINTER(_P)]),
    "rd_wideband_destroy": (None, [_P]),
    "rd_wideband_reset": (C.c_int, [_P]),
    "rd_wideband_submit": (C.c_int, [_P, _P, C.c_size_t]),
    "rd_wideband_fetch": (C.c_int, [_P, C.POINTER(RdPacket), C.c_int, C.POINTER(C.c_int)]),
    "rd_wideband_refetch": (C.c_int, [_P, C.POINTER(RdPacket), C.c_int, C.POINTER(C.c_int)]),
    "rd_wideband_inflight": (C.c_int, [_P]),
    "rd_wideband_copy_channelized": (C.c_int, [_P, _P, C.c_size_t]),
    "rd_wideband_copy_discriminated": (C.c_int, [_P, C.c_int, _P, C.c_size_t]),
    "rd_wb_set_parse": (C.c_int, [_P, C.c_int]),
    "rd_wb_parsed": (C.c_int, [_P, C.POINTER(RdParsed), C.c_int, C.POINTER(C.c_int)]),
    "rd_wb_retune": (C.c_int, [_P, _P, C.c_int]),
    "rd_wb_tuning": (C.c_int, [_P, _P, _P, C.c_int]),
    "rd_wb_set_gain": (C.c_int, [_P, _P, C.c_int]),
    "rd_wb_gains": (C.c_int, [_P, _P, C.c_int]),
    "rd_wb_set_levels": (C.c_int, [_P, C.c_int]),
    "rd_wb_levels": (C.c_int, [_P, _P, C.c_int, C.POINTER(RdInputLevel)]),
    "rd_wb_set_spectrum": (C.c_int, [_P, C.c_int]),
    "rd_wb_spectrum": (C.c_int, [_P, _P, C.c_int, C.POINTER(RdSpectrumInfo)]),
    "rd_wb_set_bursts": (C.c_int, [_P, C.c_int]),
    "rd_wb_set_burst_threshold": (C.c_int, [_P, _P, C.c_int]),
    "rd_wb_burst_thresholds": (C.c_int, [_P, _P, C.c_int]),
    "rd_wb_bursts": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), _P, C.c_int]),
    "rd_wb_set_burst_decode": (C.c_int, [_P, C.c_int]),
    "rd_wb_burst_messages": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), _P, C.c_int]),
    "rd_wb_set_burst_repair": (C.c_int, [_P, C.c_int]),
    "rd_wb_burst_repair": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "rd_wb_set_burst_narrow": (C.c_int, [_P, C.c_int]),
    "rd_wb_burst_narrow": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "rd_bd_narrow_table": (C.c_int, [C.c_int, _P, _P]),
    "rd_wb_set_burst_expect": (C.c_int, [_P, _P, C.c_int]),
    "rd_wb_burst_expect": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int)]),
    "rd_wb_expected_messages": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), _P, C.c_int]),
    "rd_wb_set_burst_search": (C.c_int, [_P, _P, C.c_int]),
    "rd_wb_burst_search": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int)]),
    "rd_wb_searched_messages": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), _P, C.c_int]),
    "rd_wb_set_burst_quality": (C.c_int, [_P, C.c_int, C.c_int]),
    "rd_wb_burst_quality": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rd_wb_burst_message_quality": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int)]),
    "rd_wb_expected_message_quality": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int)]),
    "rd_bq_window": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, _P]),
    "rd_wb_set_burst_clips": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "rd_wb_burst_clips_config": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rd_wb_burst_clips": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), _P, C.c_size_t, C.POINTER(C.c_size_t), _P, C.c_int]),
    "rd_bc_window": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int64, _P]),
    "rd_clips_create": (C.c_int, [C.POINTER(RdConfig), C.POINTER(_P)]),
    "rd_clips_destroy": (None, [_P]),
    "rd_clips_upload": (C.c_int, [_P, _P, C.c_size_t]),
    "rd_clips_decode": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    "rd_clips_kernel_ms": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "rd_cd_check_jobs": (C.c_int, [C.POINTER(RdConfig), _P, C.c_int, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_char_p)]),
    "rd_clips_synth": (C.c_int, [_P, _P, C.c_int, C.c_uint64]),
    "rd_clips_download": (C.c_int, [_P, _P, C.c_size_t]),
    "rd_clips_synth_ms": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "rd_cs_check_specs": (C.c_int, [_P, C.c_int, C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_char_p)]),
    "rd_cs_table": (None, [_P]),
    "rd_wb_fetched_chunk": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "rd_wideband_debug_advance_clock": (C.c_int, [_P, C.c_uint64]),
    "rd_debug_mfma_taps": (None, [_P]),
    "rd_debug_mfma_taps8": (None, [_P]),
    "rd_debug_mfma_taps8s": (None, [_P, _P]),
    "rd_debug_demod_mfma": (C.c_int, [_P, C.c_int, C.c_uint32, C.c_int, C.c_uint32, _P, _P, _P, C.c_uint32,
                                      C.POINTER(C.c_uint32)]),
    "rd_debug_bursts": (C.c_int, [_P, C.c_size_t, C.c_int, C.c_size_t, _P, C.c_uint64, _P, _P]),
    "rd_debug_burst_decode": (C.c_int, [C.POINTER(RdConfig), _P, _P, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, _P, _P,
                                        _P, _P, _P, _P]),
    "rd_debug_burst_decode_repair": (C.c_int, [C.POINTER(RdConfig), _P, _P, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, _P, _P,
                                               C.c_int, _P, _P, _P, _P]),
    "rd_debug_burst_decode_narrow": (C.c_int, [C.POINTER(RdConfig), _P, _P, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, _P, _P,
                                               C.c_int, C.c_int, _P, _P, _P, _P]),
    "rd_debug_burst_expect": (C.c_int, [C.POINTER(RdConfig), _P, _P, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, _P, C.c_int,
                                        C.c_int, C.c_int, _P, _P]),
    "rd_debug_burst_search": (C.c_int, [C.POINTER(RdConfig), _P, _P, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, _P, C.c_int,
                                        _P, _P]),
    "rd_debug_burst_quality": (C.c_int, [C.POINTER(RdConfig), _P, _P, C.c_size_t, C.c_int, C.c_int, _P, _P, _P]),
    "rd_bc_slot_size": (C.c_size_t, [C.c_int, C.c_int]),
    "rd_debug_burst_clips": (C.c_int, [C.POINTER(RdConfig), _P, _P, C.c_size_t, C.c_int, C.c_uint64, C.c_uint64, _P, _P, _P, _P,
                                       _P, _P, C.c_int, _P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
}

_lib = None


def lib():
    """The loaded library.  Raises ImportError (loudly) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C rtldavis_amd/csrc`.  rtldavis_amd has no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    return (lib().rd_last_error() or b"").decode("utf-8", "replace")


def check(rc: int) -> None:
    """Map rd_status to the exceptions the reference raises (dsp.py:32-36,145-149 -> ValueError)."""
    if rc == RD_OK:
        return
    msg = last_error()
    if rc == RD_ERR_ARG:
        raise ValueError(msg)
    if rc == RD_ERR_CAPACITY:
        raise BufferError(msg)
    if rc == RD_ERR_STATE:
        raise RuntimeError(msg)
    raise HipError(msg)


def gain_array(gain, n_channels):
    """``gain`` - one positive finite number for all channels or one per channel - as float64 [n_channels];
    ValueError otherwise (the library checks again, float32 range included)."""
    try:
        g = np.asarray(gain, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"gain: one positive number or {n_channels} of them") from None
    if g.ndim > 1 or (g.ndim == 1 and g.size != n_channels):
        raise ValueError(f"gain: one positive number or {n_channels} of them")
    g = np.ascontiguousarray(np.broadcast_to(g, (n_channels,)), np.float64)
    if not (np.all(np.isfinite(g)) and np.all(g > 0)):
        raise ValueError("every gain must be finite and > 0")
    return g


def make_config(bit_rate, symbol_length, preamble_symbols, packet_symbols, preamble, block_size) -> RdConfig:
    if len(preamble) > RD_MAX_PREAMBLE:
        raise ValueError("preamble longer than 64 symbols is not supported")
    c = RdConfig(int(bit_rate), int(symbol_length), int(preamble_symbols), int(packet_symbols), int(block_size))
    for i, ch in enumerate(preamble):
        c.preamble[i] = int(ch)
    return c
