#!/usr/bin/env python3
"""What the burst-quality estimators give against a planted signal-to-noise ratio, on the model alone (no device:
tests/burst_quality_cases.py is the NumPy model of include/rtldavis_hip.h, BURST QUALITY, which tests/test_burst_quality.py
holds the kernel to bit for bit).  The bursts and noise levels of tools/burst_narrow_gain.py: K bursts of
synth.synth_bursts per level (amplitude 0.3, SL 14, N 80, one burst every two chunks of 2048 outputs, white noise over the
whole stream), each measured at the place it was planted with the f a decoder would write there - the estimators are
judged, not the decoders, so a burst too weak to decode is measured all the same.

Planted: SNR in the channel band = 10 log10(0.3^2 / (2 noise^2)) (the stream is the channel's bytes: its noise is white
over all 14 symbol rates), and in +-0.9 symbol rates = that + 10 log10(14 / 1.8), the noise a brick-wall filter of the
narrow decoder's width would leave.  Both derived from the synthesiser's parameters, not measured.

Estimators (rtldavis_amd.acquire), per burst: snr_db at noise_gap 0 - the reference's window, which on these bursts holds
the 32 alternating lead-in symbols, that is signal -; snr_db and snr_inband_db at noise_gap 512, which steps over the
lead-in into noise; snr_floor_db from the chunk's OFF windows.  Every estimator divides signal + noise by noise, so it
cannot fall below 0 dB however weak the burst.

Per level and estimator: the mean over seeds x bursts, the standard deviation over bursts (pooled), and the spread
(max - min) of the per-seed means.  tests/test_burst_quality_cpu.py runs a seed that is not in this file and holds its
mean to  |mean - recorded mean| <= 3 sd / sqrt(bursts of the test) + seed spread :  three standard errors of a mean of
that many bursts, plus what the recorded seeds already differ by among themselves.

    python tools/burst_quality_model.py [--bursts 40] [--seeds 7 8 9] > profiles/burst_quality_model.txt
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import burst_cases as BC  # noqa: E402
import burst_decode_cases as DC  # noqa: E402
import burst_quality_cases as QC  # noqa: E402
import burst_repair_cases as RP  # noqa: E402
from rtldavis_amd import acquire  # noqa: E402
from rtldavis_amd.wideband import QUALITY_DTYPE  # noqa: E402

NOISE = (0.06, 0.08, 0.09, 0.10, 0.12, 0.15, 0.18, 0.20, 0.22, 0.24, 0.26, 0.28, 0.30)
ESTIMATORS = ("snr_db gap 0", "snr_db gap 512", "snr_inband_db gap 512", "snr_floor_db")
GAP = 512                                                     # past the 32 x 14 = 448 outputs of lead-in
P0 = 200 + 32 * RP.GAIN_SL                                    # the packet's first output in its chunk (gain_blocks)


def planted_db(noise):
    ch = 10 * np.log10(0.3 ** 2 / (2 * noise ** 2))
    return ch, ch + 10 * np.log10(RP.GAIN_SL / 1.8)


def estimates(k, noise, seed):
    """[k, 4]: the four estimators of every burst of gain_blocks(k, noise, seed)."""
    sl = RP.GAIN_SL
    cfg = DC.config(sl, 80, RP.GAIN_BS)
    _, blocks = RP.gain_blocks(k, noise, seed)
    thr = RP.gain_threshold(noise)
    out = np.empty((k, len(ESTIMATORS)))
    for j in range(k):
        cur, prev = blocks[2 * j], blocks[2 * j - 1] if j else None
        f = QC.packet_sum(cur[0], None if prev is None else prev[0], P0, 80 * sl)
        q0, q1 = (np.asarray([QC.measure(cur, prev, cfg, 0, P0 + sl - 1, f[0], f[1], gap, 1)], QUALITY_DTYPE)[0] for gap in (0, GAP))
        floor = BC.model_bursts(cur, thr, 2 * j).floor[0]
        out[j] = (acquire.snr_db(q0, sl), acquire.snr_db(q1, sl), acquire.snr_inband_db(q1, sl), acquire.snr_floor_db(q0, floor, sl))
    return out


def level(k, noise, seeds):
    """Per estimator (mean, pooled sd over bursts, spread of the seeds' means)."""
    runs = [estimates(k, noise, s) for s in seeds]
    means = np.array([r.mean(axis=0) for r in runs])
    sd = np.sqrt(np.mean([r.var(axis=0, ddof=1) for r in runs], axis=0))
    return means.mean(axis=0), sd, means.max(axis=0) - means.min(axis=0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bursts", type=int, default=40, help="bursts per noise level and seed")
    ap.add_argument("--seeds", type=int, nargs="+", default=[7, 8, 9], help="seeds of the noise (the payloads are fixed)")
    a = ap.parse_args()
    print(f"# tools/burst_quality_model.py --bursts {a.bursts} --seeds {' '.join(map(str, a.seeds))}")
    print("# CPU, model only (tests/burst_quality_cases.py): nothing here was run on a device, nothing here is a timing.")
    print("# synth.synth_bursts, amplitude 0.3, SL 14, N 80, chunks of 2048; every burst measured where it was planted.")
    print("# planted: SNR per sample in the channel band and in +-0.9 symbol rates (derived from the synthesiser's parameters).")
    print("# per estimator: mean dB, sd over bursts (pooled over the seeds), spread of the seeds' means.  The first burst of a")
    print("# stream has no chunk before it: at gap 512 its noise window is cut to what chunk 0 holds in front of it.")
    print("# margin of tests/test_burst_quality_cpu.py for a seed not listed here: 3 sd / sqrt(its bursts) + the seed spread.")
    print(f"# {'noise':>5} {'ch dB':>6} {'nb dB':>6} | " + " | ".join(f"{e:>21}" for e in ESTIMATORS))
    for noise in NOISE:
        mean, sd, spread = level(a.bursts, noise, a.seeds)
        ch, nb = planted_db(noise)
        print(f"{noise:7.3f} {ch:6.1f} {nb:6.1f} | " + " | ".join(f"{m:7.2f} {s:6.2f} {p:6.2f}" for m, s, p in zip(mean, sd, spread)))


if __name__ == "__main__":
    main()
