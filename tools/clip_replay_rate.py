#!/usr/bin/env python3
"""The rate of the batch replay decoder (rtldavis_amd/replay.py, k_clip_decode) on the device, and of the NumPy model
(tests/burst_track_cases.decode_expect through tests/clip_replay_cases.py) on one core.

10 000 jobs of one 1400-output synthetic burst clip each - tests/burst_decode_cases.fsk_burst, SL 14, N 80, every clip
its own payload, quiet bytes around the burst -, every job over all of its clip's candidates (280) under the clip's own
direction, for each of the kernel's four instantiations (max_flips 0 / 2, without / with the narrow-band filter):
  whole calls   jobs/s of rd_clips_decode, host clock around calls that end in the library's wait (the copy of the jobs
                in, the launch, the copies of records and headers out), the median of --reps calls after one warm-up call
  kernel        jobs/s of k_clip_decode alone, by the device events the library records around the launch, the median of
                the same calls
  model         seconds the model needs for 100 of the same jobs on one core, per form
Needs a device; there is no fall-back.

    python tools/clip_replay_rate.py [--jobs 10000] [--reps 7] > profiles/clip_replay.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import burst_decode_cases as DC  # noqa: E402
import clip_replay_cases as RC  # noqa: E402
from rtldavis_amd import _lib, replay  # noqa: E402

SL, N, CLIP = 14, 80, 1400
FORMS = ((0, False), (2, False), (0, True), (2, True))


def build(n_jobs, distinct=64):
    """``distinct`` different clips, repeated to ``n_jobs`` - each copy lies in the pool as a clip of its own."""
    base = [RC.burst_clip(DC.packet(N, ident=k % 8, seed=7000 + k), SL, CLIP, 100 + k % 37, 7000 + k, carrier=(0.11, -0.2, 0.31)[k % 3])
            for k in range(distinct)]
    clips = [base[j % distinct] for j in range(n_jobs)]
    pool, offsets = replay.pack(clips)
    jobs = RC.jobs_of([RC.job_row(offsets[j], CLIP, 0, replay.MAX_SPAN, channel=j % 51, clock=CLIP * j) for j in range(n_jobs)])
    return base, clips, pool, jobs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--model-jobs", type=int, default=100)
    a = ap.parse_args()
    if _lib.lib().rd_device_count() <= 0:
        raise SystemExit("clip_replay_rate: no HIP device; the rates are measured on the GPU or not at all")
    base, clips, pool, jobs = build(a.jobs)
    dec = replay.ClipDecoder(DC.config(SL, N, 2048))
    t = time.perf_counter()
    dec.upload(pool)
    up = time.perf_counter() - t
    cand = CLIP - 1 - SL * (N - 1) - SL + 1
    print(f"batch replay decoder (k_clip_decode behind rd_clips_decode): tools/clip_replay_rate.py --jobs {a.jobs} --reps {a.reps}")
    print(f"{a.jobs} jobs of one {CLIP}-output clip each (fsk_burst, SL {SL}, N {N}, {len(base)} distinct clips), {cand} candidates per job, "
          f"own direction; pool {pool.nbytes} bytes, uploaded once in {up * 1e3:.1f} ms (host clock, first use of the device included)")
    decoded = {}
    for r, nb in FORMS:
        dec.decode_jobs(jobs, r, nb)                              # warm-up: code object, buffers, the filter's table
        wall, kern = [], []
        for _ in range(a.reps):
            t = time.perf_counter()
            got = dec.decode_jobs(jobs, r, nb)
            wall.append(time.perf_counter() - t)
            kern.append(dec.kernel_ms() * 1e-3)
        decoded[r, nb] = got
        w, k = statistics.median(wall), statistics.median(kern)
        print(f"  max_flips {r}, narrow {int(nb)}: whole calls {a.jobs / w:10.0f} jobs/s (median {w * 1e3:7.2f} ms, all: "
              f"{' '.join(f'{x * 1e3:.2f}' for x in wall)}); kernel alone {a.jobs / k:10.0f} jobs/s (median {k * 1e3:7.2f} ms, all: "
              f"{' '.join(f'{x * 1e3:.2f}' for x in kern)}); {int(got.headers['n_msgs'].sum())} of {a.jobs} jobs gave a message")
    print(f"NumPy model (burst_track_cases.decode_expect), {a.model_jobs} of the same jobs, one core:")
    for r, nb in FORMS:
        t = time.perf_counter()
        rows = [RC.decode_job(clips[j], jobs[j], j, SL, N, r, nb) for j in range(a.model_jobs)]
        dt = time.perf_counter() - t
        same = all((row is None and not int(decoded[r, nb].headers[j]["n_msgs"])) or
                   (row is not None and bytes(decoded[r, nb].records[j]["data"]) == bytes(row[8]) and int(decoded[r, nb].records[j]["tau"]) == row[2])
                   for j, (row, _, _) in enumerate(rows))
        print(f"  max_flips {r}, narrow {int(nb)}: {dt:7.2f} s = {a.model_jobs / dt:8.1f} jobs/s; tau and data equal the device's: {same}")
    print("measured: host clock (time.perf_counter) around whole calls, which end in the library's wait; the kernel by device events "
          "recorded around its launch; this run.  Not measured: the kernel under a profiler, its share of any peak")


if __name__ == "__main__":
    main()
