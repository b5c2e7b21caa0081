#!/usr/bin/env python3
"""k_channelize by sample format: HIP-event times of the one-shot kernel on the default plan (51 channels, decim 100,
512 taps) over one second of capture - random samples at a fifth of full scale, the capture resident on the device -
for the formats named, interleaved in one process.  Prints min / median / mean / max per format in microseconds.

    python tools/chan_format_times.py --formats s16 cf32 --launches 21
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtldavis_amd import _lib  # noqa: E402
from rtldavis_amd import channelizer as CZ  # noqa: E402


def capture(fmt, n, rng):
    x = 0.2 / 3 * rng.standard_normal(2 * n)
    if fmt == "cf32":
        return x.astype(np.float32)
    dtype, scale, offset = {"u8": (np.uint8, 127.6, 127.4), "s8": (np.int8, 128.0, 0.0), "s16": (np.int16, 32768.0, 0.0)}[fmt]
    lim = np.iinfo(dtype)
    return np.clip(np.rint(x * scale + offset), lim.min, lim.max).astype(dtype)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--formats", nargs="+", default=["u8", "s16", "cf32"], choices=sorted(_lib.SAMPLE_FORMATS))
    ap.add_argument("--launches", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    hip = C.CDLL("libamdhip64.so")
    P = C.c_void_p
    hip.hipMalloc.argtypes = [C.POINTER(P), C.c_size_t]
    hip.hipFree.argtypes = [P]
    hip.hipEventCreate.argtypes = [C.POINTER(P)]
    hip.hipEventRecord.argtypes = [P, P]
    hip.hipEventSynchronize.argtypes = [P]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), P, P]
    hip.hipEventDestroy.argtypes = [P]
    n_out = CZ.OUT_RATE
    n = n_out * CZ.DEFAULT_DECIM
    rng = np.random.default_rng(1)
    cz = {}
    for fmt in args.formats:
        cz[fmt] = CZ.Channelizer(sample_format=fmt)
        cz[fmt].upload(capture(fmt, n, rng))
    dst = P()
    size = 51 * 2 * n_out
    assert hip.hipMalloc(C.byref(dst), size) == 0
    e0, e1 = P(), P()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    times = {fmt: [] for fmt in args.formats}
    try:
        for it in range(args.warmup + args.launches):
            for fmt in args.formats:
                assert hip.hipEventRecord(e0, None) == 0
                _lib.check(_lib.lib().rd_chan_run(cz[fmt]._h, n_out, dst, 2 * n_out, None))
                assert hip.hipEventRecord(e1, None) == 0
                assert hip.hipEventSynchronize(e1) == 0
                ms = C.c_float()
                assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
                if it >= args.warmup:
                    times[fmt].append(1e3 * ms.value)
    finally:
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
        hip.hipFree(dst)
    print(f"k_channelize, one second of default-plan capture ({n} samples -> 51 x {n_out}), HIP events, {args.launches} launches, us")
    print("format   min      median   mean     max")
    for fmt in args.formats:
        t = np.asarray(times[fmt])
        print(f"{fmt:<8} {t.min():<8.1f} {np.median(t):<8.1f} {t.mean():<8.1f} {t.max():<8.1f}")


if __name__ == "__main__":
    main()
