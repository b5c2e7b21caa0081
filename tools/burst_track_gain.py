#!/usr/bin/env python3
"""What decoding at expectations gains over decoding at runs, on the model alone (no device: tests/burst_track_cases.py
is the NumPy model of include/rtldavis_hip.h, BURST EXPECT, which tests/test_burst_track.py holds the kernel to bit for
bit).  The bursts of tools/burst_narrow_gain.py - K bursts of synth.synth_bursts per level, known payloads, fixed seeds,
amplitude 0.3, one burst every two chunks of 2048 outputs, SL 14, N 80, carrier 1500 Hz off - go through three decoders,
all behind the narrow-band filter, at max_flips = 0 and 2, the SAME bursts in all:

  policy   runs of ON windows at the product's policy threshold: Acquisition(factor=4) from the floor measured on the
           stream's first noise-only chunk
  oracle   runs at gain_threshold(noise), a threshold that knows the burst's amplitude
  expect   no runs: one expectation per burst with the TRUE carrier and a window of +- the Tracker's default guard
           around the true end of the first symbol

Per level: the bursts decoded (a record with the planted payload) and the records with a payload that was NOT planted.

    python tools/burst_track_gain.py [--bursts 60] [--seed 7] > profiles/burst_track_gain.txt
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import burst_cases as BC  # noqa: E402
import burst_decode_cases as DC  # noqa: E402
import burst_narrow_cases as NB  # noqa: E402
import burst_repair_cases as RP  # noqa: E402
import burst_track_cases as TK  # noqa: E402
from rtldavis_amd import acquire, track  # noqa: E402

NOISE = (0.06, 0.09, 0.12, 0.15, 0.18, 0.20, 0.22, 0.24, 0.26, 0.28, 0.30, 0.32, 0.36)
CFO = 1500.0
FLIPS = (0, 2)


def row(k, noise, seed):
    datas, blocks = RP.gain_blocks(k, noise, seed, CFO)
    cfg = DC.config(RP.GAIN_SL, 80, RP.GAIN_BS)
    out_rate = 19200 * RP.GAIN_SL
    floor = BC.model_bursts(blocks[1], 2 ** 32 - 1, 1).floor           # chunk 1 holds noise alone
    policy = acquire.Acquisition(1, cfg, factor=4).thresholds(floor)
    oracle = RP.gain_threshold(noise)
    guard = track.Tracker(cfg, (0,)).guard(0)
    corr = TK.corr_of(-0.25 + CFO / out_rate)
    tables = []
    for j in range(len(blocks)):
        if j % 2:
            tables.append(TK.table([]))
            continue
        t = (j // 2) * RP.GAIN_PERIOD + 200 + 32 * RP.GAIN_SL + RP.GAIN_SL - 1
        tables.append(TK.table([TK.expect_row(0, t - guard, t + guard, corr)]))
    cells, frag = [], 0
    for name, thr in (("policy", policy), ("oracle", oracle)):
        bursts = [BC.model_bursts(b, thr, j) for j, b in enumerate(blocks)]
        if name == "policy":
            frag = sum(len(b.records) for b in bursts)
        for r in FLIPS:
            recs = [rec for _, m in NB.decode_stream(blocks, thr, cfg, r, True, bursts=bursts) for rec in m.records]
            cells.append(NB.tally(recs, datas))
    for r in FLIPS:
        recs = [rec for m in TK.expect_stream(blocks, tables, cfg, r, True) for rec in m.records]
        assert all(int(x["flags"]) & TK.EXPECTED for x in recs)
        cells.append(NB.tally(recs, datas))
    return frag, guard, " | ".join(f"{d:5d} {w:5d}" for d, w in cells)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bursts", type=int, default=60, help="bursts per noise level")
    ap.add_argument("--seed", type=int, default=7, help="seed of the noise (the payloads are fixed)")
    a = ap.parse_args()
    print(f"# tools/burst_track_gain.py --bursts {a.bursts} --seed {a.seed}")
    print("# CPU, model only (tests/burst_track_cases.py, tests/burst_narrow_cases.py): nothing here was run on a device, nothing here is a timing.")
    print("# synth.synth_bursts, amplitude 0.3, SL 14, N 80, chunks of 2048, carrier 1500 Hz off, narrow-band filter on in every column.")
    print("# SNR = 10 log10(0.3^2 / (2 noise^2)) dB per sample at 14 samples per symbol, before the 8-bit quantiser (derived")
    print("# from the synthesiser's parameters, not measured).")
    print("# policy: runs at Acquisition(factor=4) x the floor of the first noise-only chunk; oracle: runs at gain_threshold(noise);")
    print("# expect: one expectation per burst, the true carrier, +- guard outputs around the true end of the first symbol.")
    print("# runs: the run records the policy threshold gives over the whole stream (fragments included).")
    print("# dec: bursts with a record carrying the planted payload; wrong: records whose payload was not planted.")
    cols = [f"{n} R={r}" for n in ("policy", "oracle", "expect") for r in FLIPS]
    print(f"{'':>34}| " + " | ".join(f"{c:>11}" for c in cols))
    print(f"{'noise':>6} {'SNR':>6} {'bursts':>6} {'runs':>6} {'guard':>5} | " + " | ".join(f"{'dec':>5} {'wrong':>5}" for _ in cols))
    for noise in NOISE:
        snr = 10 * np.log10(0.3 ** 2 / (2 * noise ** 2))
        frag, guard, cells = row(a.bursts, noise, a.seed)
        print(f"{noise:6.3f} {snr:6.1f} {a.bursts:6d} {frag:6d} {guard:5d} | " + cells, flush=True)


if __name__ == "__main__":
    main()
