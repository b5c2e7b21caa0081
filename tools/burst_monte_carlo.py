#!/usr/bin/env python3
"""Monte-Carlo sensitivity and false-accept figures of the burst decoders: clips synthesised on the device
(rtldavis_amd/replay.py: burst_specs, ClipDecoder.synthesize - k_clip_synth) and decoded where they lie (k_clip_decode).

Per noise level, --bursts clips of --clip outputs (batches of at most 2^16), each with one Davis burst in synth_bursts'
layout - 32 alternating lead-in symbols, a CRC-valid packet of 80 symbols with a random id and body, 8 zeros - at
amplitude --amplitude and --offset-hz off the channel's centre, its first symbol at a random output; payloads, positions,
seeds and start phases are drawn from --seed.  Every clip is one job over --span candidate positions centred on the
planted one, decoded under the clip's own direction (corr = (0, 0)) and under the true carrier, in four forms: max_flips
0 / 2, without and with the narrow-band filter.  Counted per form and direction: decoded (the planted payload), wrong (a
record with another payload), and the decoded ones by their number of flips; each rate with its 95 % Wilson interval.
A noise-only leg follows: --noise-clips clips of noise alone, id = any, the widest span, own direction; the rows and the
candidate positions per form, and the false-accept rate per position beside the derived one.
--cpu-check K downloads the first K clips of every level and holds them to the NumPy model of the synthesiser
(tests/clip_synth_cases.py), and their rows to the decoder's model (tests/clip_replay_cases.decode_job), before any count
of that level is printed.

The noise is white at the channel rate: synth_bursts' model - NOT the wideband model behind profiles/burst_track_gain.txt,
where the noise passes the channelizer's filter first.  SNR per sample is amplitude^2 / (2 noise^2).  The columns of the
earlier CPU sweeps (60 bursts per level, README) are not reproduced or asserted against here.

--rate: the synthesiser against the path it replaces, for --rate-clips clips (default 10^4 and 10^6) of --clip outputs at
noise 0.2: (a) synth_ms by device events and the whole rd_clips_synth call by host clock, median of --reps after one
warm-up call; (b) the NumPy model (timed on 100 clips, scaled - said so in the output) plus rd_clips_upload of as many
bytes, for the smallest count; (c) kernel_ms of the four decode forms on the synthesised pool.
Needs a device; there is no fall-back.

    python tools/burst_monte_carlo.py > profiles/burst_monte_carlo.txt
    python tools/burst_monte_carlo.py --rate > profiles/clip_synth.txt
"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import burst_decode_cases as DC  # noqa: E402
import clip_replay_cases as RC  # noqa: E402
import clip_synth_cases as SC  # noqa: E402
from rtldavis_amd import _lib, replay, synth  # noqa: E402
from rtldavis_amd.wideband import BURST_MSG_DTYPE  # noqa: E402

SL, N = 14, 80
FORMS = ((0, False), (2, False), (0, True), (2, True))
BATCH = 1 << 16
MULS_PER_OUTPUT = 2 * 10 * 2           # k_clip_synth: two Philox4x32-10 per output, two 32 x 32 -> 64 products per round
MUL_RATE = 37.3e12                     # lane-multiplies per second the chip sustains (profiles/r01_ubench_valu_rates.txt, 8 waves/SIMD)
_REV = np.array([int(f"{b:08b}"[::-1], 2) for b in range(256)], np.uint8)


def wilson(k, n, z=1.959964):
    """The 95 % Wilson score interval of k successes in n trials."""
    if n == 0:
        return 0.0, 1.0
    p = k / n
    d = 1.0 + z * z / n
    c = (p + z * z / (2 * n)) / d
    h = z * math.sqrt(p * (1 - p) / n + z * z / (4.0 * n * n)) / d
    return max(0.0, c - h), min(1.0, c + h)


def rate(k, n):
    lo, hi = wilson(k, n)
    return f"{k:>8d} / {n:<8d} {k / max(n, 1):9.3e} [{lo:9.3e}, {hi:9.3e}]"


def random_payloads(rng, k):
    """[k, 10] uint8: synth.make_packet(ident, body, 10) for a random id and a random body of 6 bytes, all rows at once."""
    ident = rng.integers(0, 8, k, dtype=np.uint8)
    body = rng.integers(0, 256, (k, 6), dtype=np.uint8)
    msg = np.zeros((k, 8), np.uint8)
    msg[:, 0] = (body[:, 0] & 0xF8) | ident
    msg[:, 1:6] = body[:, 1:]
    crc = np.zeros(k, np.uint32)
    for col in range(6):
        crc ^= msg[:, col].astype(np.uint32) << 8
        for _ in range(8):
            top = (crc & 0x8000) != 0
            crc = (crc << 1) & 0xFFFF
            crc[top] ^= 0x1021
    msg[:, 6], msg[:, 7] = crc >> 8, crc & 0xFF
    ota = np.empty((k, 10), np.uint8)
    ota[:, 0], ota[:, 1] = 0xCB, 0x89
    ota[:, 2:] = _REV[msg]
    for j in range(min(k, 4)):
        assert ota[j].tobytes() == synth.make_packet(int(ident[j]), body[j].tobytes(), 10)
    return ota


def check_on_cpu(dec, specs, jobs_by_dir, got_by, k):
    """The first k clips against the synthesiser's model, their rows against the decoder's model."""
    end = int(specs[k - 1]["offset"]) + int(specs[k - 1]["n"])
    model = SC.pool_of(specs[:k], SL, end)
    if not np.array_equal(dec.download()[: 2 * end], model):
        raise SystemExit("burst_monte_carlo: the device's clips differ from the NumPy model of the synthesiser")
    for (dirn, form), got in got_by.items():
        jobs = jobs_by_dir[dirn]
        for j in range(k):
            clip = model[2 * int(specs[j]["offset"]): 2 * (int(specs[j]["offset"]) + int(specs[j]["n"]))]
            row, hdr, _ = RC.decode_job(clip, jobs[j], j, SL, N, form[0], form[1])
            want = np.zeros(1, BURST_MSG_DTYPE)
            if row is not None:
                want[0] = row
                want[0]["first"] = j
            if got.records[j].tobytes() != want[0].tobytes() or tuple(int(v) for v in got.headers[j]) != tuple(int(v) for v in hdr):
                raise SystemExit(f"burst_monte_carlo: job {j} ({dirn}, {form}) differs from the decoder's model")


def sweep(dec, a):
    rng = np.random.default_rng(a.seed)
    corr_true = dec.corr(a.offset_hz)
    for noise in a.noise_levels:
        snr = 10 * math.log10(a.amplitude ** 2 / (2 * noise ** 2)) if noise > 0 else float("inf")
        tally = {(d, f): [0, 0, [0, 0, 0]] for d in ("own", "true") for f in FORMS}      # decoded, wrong, decoded by flips
        synth_ms, kernel_ms = [], {key: [] for key in tally}
        done, lines = 0, []
        while done < a.bursts:
            k = min(BATCH, a.bursts - done)
            ota = random_payloads(rng, k)
            at = rng.integers(40, a.clip - (32 + N + 8) * SL - 40, k)
            specs, tau = replay.burst_specs(ota, n=a.clip, at=at, seed=int(rng.integers(0, 2 ** 63)), amplitude=a.amplitude, noise=noise,
                                            offset_hz=a.offset_hz, symbol_length=SL)
            dec.synthesize(specs)
            synth_ms.append(dec.synth_ms())
            jobs_by_dir = {"own": replay.centred_jobs(specs, tau, a.span), "true": replay.centred_jobs(specs, tau, a.span, corr_true)}
            got_by = {}
            for dirn, jobs in jobs_by_dir.items():
                for form in FORMS:
                    got = dec.decode_jobs(jobs, form[0], form[1])
                    kernel_ms[dirn, form].append(dec.kernel_ms())
                    got_by[dirn, form] = got
                    hit = got.headers["n_msgs"] == 1
                    same = hit & np.all(got.records["data"][:, :10] == ota, axis=1)
                    t = tally[dirn, form]
                    t[0] += int(same.sum())
                    t[1] += int((hit & ~same).sum())
                    flips = got.records["pad"][same, 0]
                    for r in range(3):
                        t[2][r] += int((flips == r).sum())
            if done == 0 and a.cpu_check:
                check_on_cpu(dec, specs, jobs_by_dir, got_by, min(a.cpu_check, k))
                lines.append(f"  cpu check: the first {min(a.cpu_check, k)} clips equal the synthesiser's model byte for byte, and their "
                             f"{len(got_by)} x {min(a.cpu_check, k)} rows and headers the decoder's model")
            done += k
        print(f"\nnoise {noise:.3f} (sigma {noise * replay.FULL_SCALE:.1f} bytes), amplitude {a.amplitude:.3f}: SNR per sample {snr:.1f} dB; "
              f"{a.bursts} bursts, {a.span + 1} candidates per job")
        for ln in lines:
            print(ln)
        print(f"  synth_ms per batch (median of {len(synth_ms)}): {statistics.median(synth_ms):.3f} for {min(BATCH, a.bursts)} clips")
        print(f"  {'direction':<6} {'form':<14} {'decoded: count / bursts, rate [95 % Wilson]':<52} {'wrong':<52} flips 0 / 1 / 2   kernel_ms")
        for (dirn, form), t in tally.items():
            print(f"  {dirn:<6} R={form[0]} narrow={int(form[1])}   {rate(t[0], a.bursts)}   {rate(t[1], a.bursts)}   "
                  f"{t[2][0]} / {t[2][1]} / {t[2][2]}   {statistics.median(kernel_ms[dirn, form]):.3f}")
        sys.stdout.flush()


def noise_leg(dec, a):
    rng = np.random.default_rng(a.seed + 1)
    rows = {f: 0 for f in FORMS}
    cand = {f: 0 for f in FORMS}
    synth_ms, kernel_ms = [], {f: [] for f in FORMS}
    done = 0
    while done < a.noise_clips:
        k = min(BATCH, a.noise_clips - done)
        specs, _ = replay.burst_specs(None, count=k, n=a.clip, at=0, seed=int(rng.integers(0, 2 ** 63)), amplitude=0.0, noise=a.noise_only_level,
                                      symbol_length=SL)
        dec.synthesize(specs)
        synth_ms.append(dec.synth_ms())
        jobs = replay.centred_jobs(specs, np.full(k, replay.MAX_SPAN // 2), replay.MAX_SPAN)      # tau 0 .. 2048: every candidate of the clip
        for form in FORMS:
            got = dec.decode_jobs(jobs, form[0], form[1])
            kernel_ms[form].append(dec.kernel_ms())
            rows[form] += int(got.headers["n_msgs"].sum())
            cand[form] += int(got.headers["candidates"].astype(np.int64).sum())
        done += k
    print(f"\nnoise only: {a.noise_clips} clips of {a.clip} outputs at noise {a.noise_only_level:.3f}, id = any, own direction, "
          f"tau 0 .. {replay.MAX_SPAN}; synth_ms per batch (median) {statistics.median(synth_ms):.3f}")
    print("  derived per position: 2^-32 = 2.33e-10 at R = 0 (16 sync symbols and a 16-bit CRC); at most (1 + 36) x 2^-32 = 8.6e-09 at R = 2 "
          "(8 x 2^-32 of it from one flip, 28 x 2^-32 from two)")
    for form in FORMS:
        print(f"  R={form[0]} narrow={int(form[1])}   rows / positions, rate [95 % Wilson]: {rate(rows[form], cand[form])}   "
              f"kernel_ms {statistics.median(kernel_ms[form]):.3f}")


def rate_mode(dec, a):
    print(f"clip synthesiser (k_clip_synth behind rd_clips_synth): tools/burst_monte_carlo.py --rate --reps {a.reps}")
    print(f"clips of {a.clip} outputs, one burst each (32 + {N} + 8 symbols, SL {SL}), amplitude {a.amplitude}, noise 0.2; profiler off; "
          "every figure the median of the calls after one warm-up call")
    rng = np.random.default_rng(a.seed)
    for count in a.rate_clips:
        parts = []
        for lo in range(0, count, BATCH):                       # the payloads batch by batch, the specs as one list
            parts.append(random_payloads(rng, min(BATCH, count - lo)))
        ota = np.concatenate(parts)
        at = rng.integers(40, a.clip - (32 + N + 8) * SL - 40, count)
        t = time.perf_counter()
        specs, tau = replay.burst_specs(ota, n=a.clip, at=at, seed=a.seed, amplitude=a.amplitude, noise=0.2, offset_hz=a.offset_hz, symbol_length=SL)
        host_specs = time.perf_counter() - t
        outputs = count * a.clip
        ms, wall = [], []
        for rep in range(a.reps + 1):
            t = time.perf_counter()
            dec.synthesize(specs)
            w = time.perf_counter() - t
            if rep:
                ms.append(dec.synth_ms())
                wall.append(w * 1e3)
        m, w = statistics.median(ms), statistics.median(wall)
        print(f"\n{count} clips ({outputs} outputs, pool {2 * outputs / 1e6:.1f} MB, specs {specs.nbytes / 1e6:.1f} MB built on the host in {host_specs:.2f} s)")
        print(f"  (a) synth_ms (device events: zeroing + kernel)  {m:9.3f} ms   {count / m * 1e3:12.4g} clips/s  {2 * outputs / m / 1e6:9.2f} GB/s of clip bytes written")
        print(f"      rd_clips_synth, whole call (host clock)      {w:9.3f} ms   {count / w * 1e3:12.4g} clips/s   (min {min(wall):.3f}, max {max(wall):.3f})")
        mul_ms, store_ms = outputs * MULS_PER_OUTPUT / MUL_RATE * 1e3, outputs * 4 / 8e12 * 1e3
        print(f"      derived floors (DESIGN.md 5.3): {mul_ms:.3f} ms for the {MULS_PER_OUTPUT} 32 x 32 -> 64 products per output (2 Philox x 10 "
              f"rounds x 2; one v_mad_u64_u32 each as compiled) if one costs no less than a v_mul_lo_u32, {MUL_RATE / 1e12:.1f} T lane-ops/s "
              f"(profiles/r01_ubench_valu_rates.txt; v_mad_u64_u32's own rate is not measured); {store_ms:.3f} ms for 4 bytes stored per "
              f"output (2 zeroed, 2 written) at the 8 TB/s peak: integer throughput bounds the kernel (that floor is {mul_ms / m * 100:.0f} % of "
              f"synth_ms), not the stores ({store_ms / m * 100:.0f} %)")
        if count == min(a.rate_clips):
            t = time.perf_counter()
            SC.pool_of(specs[:100], SL)
            model = (time.perf_counter() - t) / 100 * count
            pool = dec.download()
            up = []
            for rep in range(a.reps + 1):
                t = time.perf_counter()
                dec.upload(pool)
                if rep:
                    up.append((time.perf_counter() - t) * 1e3)
            dec.synthesize(specs)
            print(f"  (b) NumPy model on one core, timed on 100 clips and SCALED to {count}: {model * 1e3:9.1f} ms; rd_clips_upload of the "
                  f"same {pool.nbytes / 1e6:.1f} MB: {statistics.median(up):9.3f} ms (host clock)")
        jobs = replay.centred_jobs(specs, tau, a.span)
        slowest = 0.0
        for form in FORMS:
            km = []
            for rep in range(a.reps + 1):
                for lo in range(0, count, replay.MAX_JOBS):
                    dec.decode_jobs(jobs[lo: lo + replay.MAX_JOBS], form[0], form[1])
                if rep:
                    km.append(dec.kernel_ms())
            slowest = max(slowest, statistics.median(km))
            print(f"  (c) kernel_ms R={form[0]} narrow={int(form[1])}, {a.span + 1} candidates per job, own direction: {statistics.median(km):9.3f} ms")
        print(f"      synth_ms / slowest decode form's kernel_ms = {m / slowest:.2f}")
        sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bursts", type=int, default=100000)
    ap.add_argument("--noise-levels", type=lambda s: [float(v) for v in s.split(",")], default=[0.10, 0.15, 0.20, 0.24, 0.28])
    ap.add_argument("--amplitude", type=float, default=0.3)
    ap.add_argument("--offset-hz", type=float, default=2688.0, help="carrier off the channel's centre (0.01 cycles per output)")
    ap.add_argument("--clip", type=int, default=2048)
    ap.add_argument("--span", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--noise-clips", type=int, default=100000)
    ap.add_argument("--noise-only-level", type=float, default=0.2)
    ap.add_argument("--cpu-check", type=int, default=32)
    ap.add_argument("--rate", action="store_true")
    ap.add_argument("--rate-clips", type=lambda s: [int(v) for v in s.split(",")], default=[10000, 1000000])
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.clip < (32 + N + 8) * SL + 100 or not 0 <= a.span <= replay.MAX_SPAN:
        raise SystemExit("burst_monte_carlo: --clip holds the burst and 100 outputs, --span is 0 .. 2048")
    if _lib.lib().rd_device_count() <= 0:
        raise SystemExit("burst_monte_carlo: no HIP device; the clips are synthesised and decoded on the GPU or not at all")
    dec = replay.ClipDecoder(DC.config(SL, N, 2048))
    if a.rate:
        rate_mode(dec, a)
        return
    print(f"burst decoders, Monte-Carlo: tools/burst_monte_carlo.py --bursts {a.bursts} --noise-clips {a.noise_clips} --span {a.span} "
          f"--seed {a.seed} --cpu-check {a.cpu_check}")
    print(f"clips of {a.clip} outputs synthesised on the device (k_clip_synth), SL {SL}, N {N}, carrier {a.offset_hz:.0f} Hz off the centre; "
          "white noise at the channel rate (synth_bursts' model, not the wideband model of burst_track_gain.txt); "
          "SNR per sample = amplitude^2 / (2 noise^2)")
    sweep(dec, a)
    noise_leg(dec, a)


if __name__ == "__main__":
    main()
