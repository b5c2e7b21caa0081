#!/usr/bin/env python3
"""What the blind sync-word search gains over decoding at runs, and how it compares with an expectation that knows the
carrier and the time, on the model alone (no device: tests/burst_search_cases.py is the NumPy model of
include/rtldavis_hip.h, BURST SEARCH, which tests/test_burst_search.py holds the kernel to bit for bit).  The bursts of
tools/burst_track_gain.py - K bursts of synth.synth_bursts per level, known payloads, fixed seeds, amplitude 0.3, one
burst every two chunks of 2048 outputs, SL 14, N 80, carrier 1500 Hz off - go through, all behind the narrow-band filter
and without repair, the SAME bursts in all:

  policy    runs of ON windows at the product's policy threshold: Acquisition(factor=4) from the floor measured on the
            stream's first noise-only chunk
  expect    no runs: one expectation per burst with the TRUE carrier and a window of +- the Tracker's default guard
            around the true end of the first symbol
  search    no runs, no expectation: every position of every chunk at the grid point nearest the carrier
            (acquire.search_centres), at that point and its neighbours (+-1), and at +-2

Per level: the bursts decoded (a record with the planted payload; for several centres by any of them) and the records
with a payload that was NOT planted.  Every second chunk holds noise alone: on those, at the nearest centre, the
positions whose 16 sync symbols matched (sync_hits) and the rows reported, per 10^6 positions tested.

    python tools/burst_search_gain.py [--bursts 60] [--seed 7] > profiles/burst_search_gain.txt
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
import burst_search_cases as SC  # noqa: E402
import burst_track_cases as TK  # noqa: E402
from rtldavis_amd import acquire, track  # noqa: E402

NOISE = (0.06, 0.09, 0.12, 0.15, 0.18, 0.20, 0.22, 0.24, 0.26, 0.28, 0.30, 0.32, 0.36)
CFO = 1500.0


def row(k, noise, seed):
    datas, blocks = RP.gain_blocks(k, noise, seed, CFO)
    cfg = DC.config(RP.GAIN_SL, 80, RP.GAIN_BS)
    out_rate = 19200 * RP.GAIN_SL
    floor = BC.model_bursts(blocks[1], 2 ** 32 - 1, 1).floor           # chunk 1 holds noise alone
    policy = acquire.Acquisition(1, cfg, factor=4).thresholds(floor)
    bursts = [BC.model_bursts(b, policy, j) for j, b in enumerate(blocks)]
    cells = [NB.tally([rec for _, m in NB.decode_stream(blocks, policy, cfg, 0, True, bursts=bursts) for rec in m.records], datas)]
    guard = track.Tracker(cfg, (0,)).guard(0)
    corr = TK.corr_of(-0.25 + CFO / out_rate)
    tables = []
    for j in range(len(blocks)):
        t = (j // 2) * RP.GAIN_PERIOD + 200 + 32 * RP.GAIN_SL + RP.GAIN_SL - 1
        tables.append(TK.table([] if j % 2 else [TK.expect_row(0, t - guard, t + guard, corr)]))
    cells.append(NB.tally([rec for m in TK.expect_stream(blocks, tables, cfg, 0, True) for rec in m.records], datas))
    centres = [int(g) for g in acquire.search_centres([CFO], out_rate, spread=2)]
    mid = centres[2]
    found = SC.search_stream(blocks, [centres] * len(blocks), cfg)
    recs = [r for m in found for r in m.records]
    assert all(int(r["flags"]) & SC.SEARCHED for r in recs) and not any(int(m.dropped.sum()) for m in found)
    for spread in (0, 1, 2):
        cells.append(NB.tally([r for r in recs if min((int(r["pad"][3]) - mid) % 64, (mid - int(r["pad"][3])) % 64) <= spread], datas))
    quiet = [m for j, m in enumerate(found) if j % 2]                  # the chunks of noise alone
    positions = len(quiet) * RP.GAIN_BS                                # (behind a chunk every chunk has B candidates)
    hits = sum(int(m.sync_hits[2, 0]) for m in quiet)
    rows = sum(int(r["pad"][3]) == mid for m in quiet for r in m.records)
    return mid, " | ".join(f"{d:5d} {w:5d}" for d, w in cells), positions, hits, rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bursts", type=int, default=60, help="bursts per noise level")
    ap.add_argument("--seed", type=int, default=7, help="seed of the noise (the payloads are fixed)")
    a = ap.parse_args()
    print(f"# tools/burst_search_gain.py --bursts {a.bursts} --seed {a.seed}")
    print("# CPU, model only (tests/burst_search_cases.py, tests/burst_track_cases.py, tests/burst_narrow_cases.py): nothing here was run on a device,")
    print("# nothing here is a timing.")
    print("# synth.synth_bursts, amplitude 0.3, SL 14, N 80, chunks of 2048, carrier 1500 Hz off, narrow-band filter in every column, no repair.")
    print("# SNR = 10 log10(0.3^2 / (2 noise^2)) dB per sample at 14 samples per symbol, before the 8-bit quantiser (derived")
    print("# from the synthesiser's parameters, not measured).")
    print("# policy: runs at Acquisition(factor=4) x the floor of the first noise-only chunk; expect: one expectation per burst, the true")
    print("# carrier, +- guard outputs around the true end of the first symbol; search: every position, at the grid point g nearest the")
    print("# carrier, at g and g +- 1 (by any of the three), at g .. g +- 2 (by any of the five).")
    print("# dec: bursts with a record carrying the planted payload; wrong: records whose payload was not planted.")
    print("# noise-only chunks (every second one), centre g: positions tested, sync_hits, rows reported, and both per 10^6 positions.")
    cols = ("policy", "expect", "search g", "search +-1", "search +-2")
    print(f"{'':>24}| " + " | ".join(f"{c:>11}" for c in cols) + " | noise-only chunks at g")
    print(f"{'noise':>6} {'SNR':>6} {'bursts':>6} {'g':>3} | " + " | ".join(f"{'dec':>5} {'wrong':>5}" for _ in cols)
          + f" | {'positions':>9} {'sync':>5} {'rows':>4} {'sync/1e6':>9} {'rows/1e6':>9}")
    for noise in NOISE:
        snr = 10 * np.log10(0.3 ** 2 / (2 * noise ** 2))
        g, cells, positions, hits, rows = row(a.bursts, noise, a.seed)
        print(f"{noise:6.3f} {snr:6.1f} {a.bursts:6d} {g:3d} | " + cells
              + f" | {positions:9d} {hits:5d} {rows:4d} {1e6 * hits / positions:9.1f} {1e6 * rows / positions:9.1f}", flush=True)


if __name__ == "__main__":
    main()
