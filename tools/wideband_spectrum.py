#!/usr/bin/env python3
"""k_chan_spectrum at the default plan (51 channels, decim 100, 512 taps, chunks of 8192 outputs = 819200 samples), per
sample format and n_bins, in one process:
  kernel    HIP-event times of k_chan_spectrum (rd_chan_spectrum_dev) and of k_channelize (rd_chan_run) on one resident
            chunk, interleaved launch by launch; medians in microseconds and their ratio
  rate      chunks per second of a WidebandReceiver fed with two chunks in flight, the spectrum on and off in
            alternating rounds; medians and the on / off ratio
  error     the largest |P_dev - P_ref| / tol over the inputs of tests/spectrum_model.py at that n_bins (must be < 1)

    python tools/wideband_spectrum.py --formats u8 s16 --launches 21
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rtldavis_amd import _lib  # noqa: E402
from rtldavis_amd import channelizer as CZ  # noqa: E402
from rtldavis_amd import dsp, wideband  # noqa: E402
import spectrum_model as SM  # noqa: E402

BLOCK = 8192


def capture(fmt, n, rng):
    x = 0.2 / 3 * rng.standard_normal(2 * n)
    if fmt == "cf32":
        return x.astype(np.float32)
    dtype, scale, offset = {"u8": (np.uint8, 127.6, 127.4), "s8": (np.int8, 128.0, 0.0), "s16": (np.int16, 32768.0, 0.0)}[fmt]
    lim = np.iinfo(dtype)
    return np.clip(np.rint(x * scale + offset), lim.min, lim.max).astype(dtype)


def error_ratio(fmt, n_bins):
    worst = 0.0
    for decim, bs, n in SM.SHAPES:
        if n != n_bins:
            continue
        ch = CZ.Channelizer([CZ.DEFAULT_CENTRE_HZ], decim=decim, taps=np.ones(8) / 8, sample_format=fmt)
        ch.upload(SM.chunk_input(fmt, decim * bs, n))
        ref, _, tol = SM.reference(fmt, decim * bs, n)
        worst = max(worst, float(np.abs(ch.spectrum(n).power - ref).max()) / tol)
    return worst


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--formats", nargs="+", default=list(SM.FORMATS), choices=sorted(_lib.SAMPLE_FORMATS))
    ap.add_argument("--bins", nargs="+", type=int, default=[1024, 4096])
    ap.add_argument("--launches", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunks", type=int, default=24, help="chunks per streaming round")
    ap.add_argument("--rounds", type=int, default=5, help="streaming rounds per setting")
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
    L = _lib.lib()
    n = BLOCK * CZ.DEFAULT_DECIM
    rng = np.random.default_rng(1)
    cfg = dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", BLOCK)
    dst, rec = P(), P()
    assert hip.hipMalloc(C.byref(dst), 51 * 2 * BLOCK) == 0 and hip.hipMalloc(C.byref(rec), 16 + 8 * 4096) == 0
    e0, e1 = P(), P()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

    def timed(call):
        assert hip.hipEventRecord(e0, None) == 0
        _lib.check(call())
        assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return 1e3 * ms.value

    print(f"k_chan_spectrum, default plan, one chunk = {n} samples -> 51 x {BLOCK}; HIP events, {args.launches} launches (medians, us);")
    print(f"streaming: {args.rounds} rounds of {args.chunks} chunks per setting, two in flight (median chunks/s)")
    print("format n_bins  spectrum_us channelize_us  ratio   rate_off  rate_on   on/off  err/tol")
    try:
        for fmt in args.formats:
            chunk = capture(fmt, n, rng)
            cz = CZ.Channelizer(sample_format=fmt)
            cz.upload(chunk)
            w = wideband.WidebandReceiver(cfg, sample_format=fmt)
            for n_bins in args.bins:
                t_sp, t_ch = [], []
                for it in range(args.warmup + args.launches):
                    a = timed(lambda: L.rd_chan_spectrum_dev(cz._h, n_bins, rec, None))
                    b = timed(lambda: L.rd_chan_run(cz._h, BLOCK, dst, 2 * BLOCK, None))
                    if it >= args.warmup:
                        t_sp.append(a)
                        t_ch.append(b)
                rates = {0: [], n_bins: []}
                for rnd in range(2 * args.rounds + 2):
                    setting = n_bins if rnd % 2 else 0
                    w.reset()
                    w.set_spectrum(setting)
                    t0 = time.perf_counter()
                    w.submit(chunk)
                    for _ in range(args.chunks - 1):
                        w.submit(chunk)
                        w.fetch()
                    w.fetch()
                    dt = time.perf_counter() - t0
                    if rnd >= 2:                            # (the first round of each setting allocates)
                        rates[setting].append(args.chunks / dt)
                sp, ch = float(np.median(t_sp)), float(np.median(t_ch))
                off, on = float(np.median(rates[0])), float(np.median(rates[n_bins]))
                print(f"{fmt:<6} {n_bins:<6} {sp:<11.1f} {ch:<14.1f} {sp / ch:<7.2f} {off:<9.1f} {on:<9.1f} {on / off:<7.3f} "
                      f"{error_ratio(fmt, n_bins):.4f}")
    finally:
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
        hip.hipFree(dst)
        hip.hipFree(rec)


if __name__ == "__main__":
    main()
