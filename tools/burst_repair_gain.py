#!/usr/bin/env python3
"""What the CRC-guided repair of the burst decoder gains, on the model alone (no device: tests/burst_repair_cases.py is
the NumPy model of include/rtldavis_hip.h, BURST DECODE, steps 5a / 5b / 6', which tests/test_burst_repair.py holds the
kernel to bit for bit).  Over a sweep of noise levels, K bursts of synth.synth_bursts per level (known payloads, fixed
seeds, amplitude 0.3, one burst every two chunks of 2048 outputs, SL 14, N 80) go through the stream model at
max_flips = 0, 1 and 2 - the SAME bursts at every R.  Per level: the bursts decoded (a record with the planted payload),
the records with a payload that was NOT planted (false accepts), and the repaired records by number of flips.

    python tools/burst_repair_gain.py [--bursts 300] [--seed 7] > profiles/burst_repair_gain.txt
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import burst_repair_cases as RP  # noqa: E402

NOISE = (0.06, 0.07, 0.075, 0.08, 0.085, 0.09, 0.095, 0.10, 0.11, 0.12)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bursts", type=int, default=300, help="bursts per noise level")
    ap.add_argument("--seed", type=int, default=7, help="seed of the noise (the payloads are fixed)")
    a = ap.parse_args()
    print(f"# tools/burst_repair_gain.py --bursts {a.bursts} --seed {a.seed}")
    print("# CPU, model only (tests/burst_repair_cases.py): nothing here was run on a device, nothing here is a timing.")
    print("# synth.synth_bursts, amplitude 0.3, cfo 1500 Hz, SL 14, N 80, chunks of 2048, threshold between floor and burst.")
    print("# SNR = 10 log10(0.3^2 / (2 noise^2)) dB per sample at 14 samples per symbol, before the 8-bit quantiser (derived")
    print("# from the synthesiser's parameters, not measured).")
    print("# decoded: bursts with a record carrying the planted payload; wrong: records whose payload was not planted;")
    print("# 1f / 2f: repaired records with one / two flips.  Every row: the same bursts at R = 0, 1, 2.")
    print(f"{'noise':>6} {'SNR':>6} {'bursts':>6} | {'R=0':>5} {'wrong':>5} | {'R=1':>5} {'gain':>5} {'wrong':>5} {'1f':>4} | "
          f"{'R=2':>5} {'gain':>5} {'wrong':>5} {'1f':>4} {'2f':>4}")
    for noise in NOISE:
        datas, out = RP.gain_run(a.bursts, noise, a.seed)
        planted = set(datas)
        dec = {r: len({bytes(x["data"]) for x in out[r]} & planted) for r in out}
        wrong = {r: sum(bytes(x["data"]) not in planted for x in out[r]) for r in out}
        nf = {r: [sum(int(x["pad"][0]) == f for x in out[r]) for f in (1, 2)] for r in out}
        for r in (1, 2):                                     # an exact record is R = 0's, bit for bit
            assert [x.tobytes() for x in out[r] if not int(x["flags"]) & RP.REPAIRED] == [x.tobytes() for x in out[0]]
        esn0 = 10 * np.log10(0.3 ** 2 / (2 * noise ** 2))
        print(f"{noise:6.3f} {esn0:6.1f} {a.bursts:6d} | {dec[0]:5d} {wrong[0]:5d} | {dec[1]:5d} {dec[1] - dec[0]:+5d} {wrong[1]:5d} "
              f"{nf[1][0]:4d} | {dec[2]:5d} {dec[2] - dec[0]:+5d} {wrong[2]:5d} {nf[2][0]:4d} {nf[2][1]:4d}")


if __name__ == "__main__":
    main()
