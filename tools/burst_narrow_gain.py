#!/usr/bin/env python3
"""What the narrow-band filter of the burst decoder gains, on the model alone (no device: tests/burst_narrow_cases.py is
the NumPy model of include/rtldavis_hip.h, BURST DECODE, step 4n, which tests/test_burst_narrow.py holds the kernel to
bit for bit).  The sweep of tools/burst_repair_gain.py, extended to noise 0.30: K bursts of synth.synth_bursts per level
(known payloads, fixed seeds, amplitude 0.3, one burst every two chunks of 2048 outputs, SL 14, N 80) go through the
stream model wide and narrow, at max_flips = 0 and 2 - the SAME bursts in all four.  Per level: the bursts decoded (a
record with the planted payload) and the records with a payload that was NOT planted.  Then one line per carrier offset
at noise 0.20.

    python tools/burst_narrow_gain.py [--bursts 60] [--seed 7] > profiles/burst_narrow_gain.txt
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import burst_narrow_cases as NB  # noqa: E402

NOISE = (0.06, 0.08, 0.09, 0.10, 0.12, 0.15, 0.18, 0.20, 0.22, 0.24, 0.26, 0.28, 0.30)
CFO = (1500.0, 22100.0, -38000.0)
KEYS = ((False, 0), (False, 2), (True, 0), (True, 2))


def row(bursts, noise, seed, cfo):
    out, datas = NB.gain_run(bursts, noise, seed, flips=(0, 2), cfo=cfo)
    t = [NB.tally(out[k], datas) for k in KEYS]
    assert all(int(x["flags"]) & NB.NARROW for x in out[True, 0] + out[True, 2])
    assert not any(int(x["flags"]) & NB.NARROW for x in out[False, 0] + out[False, 2])
    return " | ".join(f"{d:5d} {w:5d}" for d, w in t)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bursts", type=int, default=60, help="bursts per noise level")
    ap.add_argument("--seed", type=int, default=7, help="seed of the noise (the payloads are fixed)")
    a = ap.parse_args()
    print(f"# tools/burst_narrow_gain.py --bursts {a.bursts} --seed {a.seed}")
    print("# CPU, model only (tests/burst_narrow_cases.py): nothing here was run on a device, nothing here is a timing.")
    print("# synth.synth_bursts, amplitude 0.3, SL 14, N 80, chunks of 2048, threshold between floor and burst (gain_threshold).")
    print("# SNR = 10 log10(0.3^2 / (2 noise^2)) dB per sample at 14 samples per symbol, before the 8-bit quantiser (derived")
    print("# from the synthesiser's parameters, not measured).")
    print("# dec: bursts with a record carrying the planted payload; wrong: records whose payload was not planted.")
    print("# Every row: the same bursts through the wide and the narrow decoder at R = 0 and R = 2.")
    head = f"{'noise':>6} {'SNR':>6} {'cfo Hz':>7} {'bursts':>6} | " + " | ".join(f"{'dec':>5} {'wrong':>5}" for _ in KEYS)
    print(f"{'':>29}| " + " | ".join(f"{('narrow' if n else 'wide') + ' R=' + str(r):>11}" for n, r in KEYS))
    print(head)
    for noise in NOISE:
        snr = 10 * np.log10(0.3 ** 2 / (2 * noise ** 2))
        print(f"{noise:6.3f} {snr:6.1f} {CFO[0]:7.0f} {a.bursts:6d} | " + row(a.bursts, noise, a.seed, CFO[0]))
    print("# other carrier offsets at noise 0.20 (the grid point and the part of the pass band change):")
    for cfo in CFO:
        snr = 10 * np.log10(0.3 ** 2 / (2 * 0.20 ** 2))
        print(f"{0.20:6.3f} {snr:6.1f} {cfo:7.0f} {a.bursts:6d} | " + row(a.bursts, 0.20, a.seed, cfo))


if __name__ == "__main__":
    main()
