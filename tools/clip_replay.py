#!/usr/bin/env python3
"""Decode every recording under a directory again, on the device, under all six forms of the burst decoder.

Reads every ``*.sigmf-meta`` under DIR (``rtldavis_amd.clips.write_sigmf`` wrote them), decodes each recording with
``rtldavis_amd.replay.ClipDecoder`` around its own direction with max_flips 0, 1, 2, without and with the narrow-band
filter, and prints one line per recording, form and message: time, id, data, flips, g, margin and the carrier estimate.
Needs a device.

    python tools/clip_replay.py DIR [--symbol-length 14] [--packet-symbols 80] [--bit-rate 19200]
"""
import argparse
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from rtldavis_amd import acquire, clips, dsp, replay  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--symbol-length", type=int, default=14)
    ap.add_argument("--packet-symbols", type=int, default=80)
    ap.add_argument("--bit-rate", type=int, default=19200)
    a = ap.parse_args()
    bases = sorted(p[: -len(".sigmf-meta")] for p in glob.glob(os.path.join(a.dir, "**", "*.sigmf-meta"), recursive=True))
    if not bases:
        raise SystemExit(f"clip_replay: no *.sigmf-meta under {a.dir}")
    recs = [clips.read_sigmf(b)[0] for b in bases]
    cfg = dsp.PacketConfig(a.bit_rate, a.symbol_length, 16, a.packet_symbols, "1100101110001001", 2048)
    dec = replay.ClipDecoder(cfg)
    for out in dec.decode(recs, forms=replay.FORMS):
        r, nb = out.form
        hit = set(int(k) for k in out.recording)
        for row, k in zip(out.records, out.recording):
            f = acquire.burst_message_offset_hz(row, dec.out_rate, dec.if_hz, packet_symbols=a.packet_symbols)
            flips = ",".join(str(s) for s in acquire.flipped_symbols(row)) or "-"
            print(f"{os.path.relpath(bases[int(k)], a.dir)}  max_flips {r} narrow {int(nb)}  time {int(row['time'])}  id {int(row['id'])}  "
                  f"data {bytes(row['data'][: a.packet_symbols // 8]).hex()}  flips {flips}  g {int(row['pad'][3])}  "
                  f"margin {int(row['margin'])}  carrier {f:+.0f} Hz")
        for k, b in enumerate(bases):
            if k not in hit:
                print(f"{os.path.relpath(b, a.dir)}  max_flips {r} narrow {int(nb)}  no message")


if __name__ == "__main__":
    main()
