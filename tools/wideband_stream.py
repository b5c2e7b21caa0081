"""Sustained rate of the live wideband receiver (rtldavis_amd.WidebandReceiver): 51 hop channels out of one
capture, fed chunk by chunk through submit / fetch with two chunks in flight.

A capture of a few chunks is synthesised once (one burst per channel; synth_wideband over hundreds of chunks would
need gigabytes of host memory) and its chunks are fed round and round, after a warm-up.  Reports, from a host clock
around work that ends in a fetch:
  - per-chunk latency (submit call to the return of its fetch) and sustained chunks per second,
  - wideband MS/s and the real-time factor (air time of the chunks over wall time),
  - how many injected packets came back on the first pass over the capture.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own.

    python tools/wideband_stream.py [--chunks 2000] [--repeats 3] [--capture-chunks 6] [--warmup 20] [--parse]
                                    [--retune {none,one,all}] [--levels] [--bursts [--bursts-out FILE]]
                                    [--burst-decode [--burst-decode-out FILE]]
                                    [--burst-repair N [--burst-repair-out FILE]]
                                    [--burst-narrow [--burst-narrow-out FILE]] [--track [--track-out FILE]]
                                    [--burst-quality [--burst-quality-out FILE]]
                                    [--burst-clips [--burst-clips-out FILE]] [--json OUT]

--parse: the receiver runs Parser.parse's front half in its kernels (WidebandReceiver.set_parse) and parsed() is read
after every fetch, the next chunk in flight; one more window measures the route without it - a quiet receiver per chunk,
the CRC gate on the host, discriminated(channel) per CRC-valid packet.
--retune one | all: WidebandReceiver.retune before every submit - channel 25, or all 51 channels, alternately 1 Hz up and
back on the plan - so every chunk carries the rebuild of those channels' tables (k_chan_retune) in front of its
channelizer; 1 Hz keeps every burst where it was.
--levels: level metering on (WidebandReceiver.set_levels: k_chan_levels behind every chunk's channelizer), levels() read
after every fetch and handed to agc.GainControl.update, whose gains go into set_gain when a channel moves.
--bursts: every repeat times two windows, burst detection off and on (WidebandReceiver.set_bursts: k_chan_bursts behind
every chunk's channelizer; bursts() read after every fetch, its floor turned into the next thresholds and its records handed
to acquire.Acquisition.update - a proposed retune is counted, not applied).  "Off" is the baseline of the same run; both go
into --bursts-out (default profiles/wideband_bursts.txt).  The kernel's own time: the rocprofv3 run above.
--burst-decode: as --bursts, but the two windows of every repeat are burst detection on, and burst detection plus burst
decode on (WidebandReceiver.set_burst_decode: k_chan_burst_decode behind k_chan_bursts; burst_messages() read after
every fetch and handed to Acquisition.update with the rest).  Both go into --burst-decode-out (default
profiles/wideband_burst_decode.txt); the comparison outside this run is the commit before with --bursts.
--burst-repair N (1 or 2): as --burst-decode, but the two windows of every repeat are bursts + decode on, and bursts +
decode + WidebandReceiver.set_burst_repair(N) on, and every channel's burst is DAMAGED: its payload is the CRC-invalid
twin of a packet (synth.make_packet(..., flip_bit=...): one payload symbol wrong at full strength), so that every tau that
passes the sync word runs the whole search of the repair - the list, the 8 singles, the 28 pairs - and, the wrong symbol
being a strong one, mostly finds nothing.  Both go into --burst-repair-out (default profiles/wideband_burst_repair.txt),
with the spread of the windows beside the difference.  The kernel's own time is not measured here.
--burst-quality: as --burst-narrow, but the second window of every repeat has WidebandReceiver.set_burst_quality(True) on
(k_chan_burst_quality behind k_chan_burst_decode) and reads burst_message_quality() per chunk; written to
--burst-quality-out (default profiles/wideband_burst_quality.txt).
--burst-clips: the same windows, but the second of every repeat has WidebandReceiver.set_burst_clips() on (both sources, the
default rolls and quota: k_chan_burst_clips behind k_chan_burst_decode) and reads burst_clips() per chunk; written to
--burst-clips-out (default profiles/wideband_burst_clips.txt).
--burst-narrow: as --burst-decode, but the two windows of every repeat are bursts + decode on, and bursts + decode +
WidebandReceiver.set_burst_narrow(True) on (k_chan_burst_decode<false, true>: the narrow-band filter in front of the
discriminator, in every chunk that holds a run); the capture is --burst-decode's, an undamaged burst on every channel.
Both go into --burst-narrow-out (default profiles/wideband_burst_narrow.txt), with the spread of the windows beside the
difference and whether the windows of the two settings overlap.  The kernel's own time is not measured here.
--track: as --burst-decode, but the two windows of every repeat are bursts + decode on, and bursts + decode on with a table
of 8 expectations set before every submit (WidebandReceiver.set_burst_expect: k_chan_burst_expect behind
k_chan_burst_decode, 8 workgroups, 201 candidates each, all inside the chunk) and expected_messages() read after every
fetch.  Both go into --track-out (default profiles/wideband_burst_track.txt), with the spread of the windows beside the
difference.  The kernel's own time is not measured here.
--burst-search N (1 .. 8): as --burst-decode, but the two windows of every repeat are bursts + decode on, and bursts +
decode on with the blind search at N centres (WidebandReceiver.set_burst_search: k_chan_burst_search behind
k_chan_burst_decode, one workgroup per channel and centre, every output position tested) and searched_messages() read
after every fetch.  The centres are the grid point of the channels' centre and its neighbours; the capture's bursts lie
there.  Both go into --burst-search-out (default profiles/wideband_burst_search.txt), with the rate against that of the
air.  The kernel's own time is not measured here.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import rtldavis_amd  # noqa: E402,F401  (sets the environment before HIP initialises)
from rtldavis_amd import channelizer as CZ  # noqa: E402
from rtldavis_amd import dsp, synth, wideband  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--chunks", type=int, default=2000, help="timed chunks per repeat (>= 200)")
    ap.add_argument("--repeats", type=int, default=3, help="timed windows (each after a reset); the median is reported")
    ap.add_argument("--capture-chunks", type=int, default=6, help="chunks in the synthesised capture")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sample-format", default="u8", choices=["u8", "s8", "s16", "cf32"], help="the capture's sample format")
    ap.add_argument("--parse", action="store_true", help="device parse on, parsed() read per chunk; also time the route without it")
    ap.add_argument("--retune", default="none", choices=["none", "one", "all"],
                    help="retune one channel or all of them before every chunk")
    ap.add_argument("--levels", action="store_true", help="metering on; levels() -> GainControl.update -> set_gain per chunk")
    ap.add_argument("--bursts", action="store_true", help="time every window with burst detection off and on; write --bursts-out")
    ap.add_argument("--bursts-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                         "wideband_bursts.txt"))
    ap.add_argument("--burst-decode", action="store_true",
                    help="time every window with bursts on, and with bursts and burst decode on; write --burst-decode-out")
    ap.add_argument("--burst-decode-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                               "wideband_burst_decode.txt"))
    ap.add_argument("--burst-repair", type=int, default=0, choices=[0, 1, 2],
                    help="time every window with bursts + decode on, and with repair of N flips on top, on damaged bursts; write --burst-repair-out")
    ap.add_argument("--burst-repair-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                               "wideband_burst_repair.txt"))
    ap.add_argument("--burst-narrow", action="store_true",
                    help="time every window with bursts + decode on, and with the narrow-band filter on top; write --burst-narrow-out")
    ap.add_argument("--burst-narrow-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                               "wideband_burst_narrow.txt"))
    ap.add_argument("--burst-quality", action="store_true",
                    help="time every window with bursts + decode on, and with burst quality on top; write --burst-quality-out")
    ap.add_argument("--burst-quality-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                                "wideband_burst_quality.txt"))
    ap.add_argument("--burst-clips", action="store_true",
                    help="time every window with bursts + decode on, and with burst clips (both sources) on top; write --burst-clips-out")
    ap.add_argument("--burst-clips-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                              "wideband_burst_clips.txt"))
    ap.add_argument("--track", action="store_true",
                    help="time every window with bursts + decode on, and with 8 expectations active in every chunk on top; write --track-out")
    ap.add_argument("--track-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                        "wideband_burst_track.txt"))
    ap.add_argument("--burst-search", type=int, default=0, choices=range(0, 9), metavar="N",
                    help="time every window with bursts + decode on, and with the blind search at N centres on top; write --burst-search-out")
    ap.add_argument("--burst-search-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                               "wideband_burst_search.txt"))
    ap.add_argument("--json", default=None, help="also write the result as JSON here")
    args = ap.parse_args()
    if args.chunks < 1 or args.repeats < 1 or args.capture_chunks < 3:
        raise SystemExit("--chunks >= 1, --repeats >= 1 and --capture-chunks >= 3")
    if args.bursts and args.burst_decode:
        raise SystemExit("--bursts or --burst-decode: each run compares two windows")
    repair = args.burst_repair
    if repair and (args.bursts or args.burst_decode):
        raise SystemExit("--burst-repair alone: each run compares two windows")
    narrow = args.burst_narrow
    if narrow and (args.bursts or args.burst_decode or repair):
        raise SystemExit("--burst-narrow alone: each run compares two windows")
    track = args.track
    if track and (args.bursts or args.burst_decode or repair or narrow):
        raise SystemExit("--track alone: each run compares two windows")
    quality = args.burst_quality
    if quality and (args.bursts or args.burst_decode or repair or narrow or track):
        raise SystemExit("--burst-quality alone: each run compares two windows")
    search = args.burst_search
    if search and (args.bursts or args.burst_decode or repair or narrow or track or quality):
        raise SystemExit("--burst-search alone: each run compares two windows")
    clips = args.burst_clips
    if clips and (args.bursts or args.burst_decode or repair or narrow or track or quality or search):
        raise SystemExit("--burst-clips alone: each run compares two windows")
    decode = args.burst_decode or repair > 0 or narrow or track or quality or search > 0 or clips
    args.bursts = args.bursts or decode       # (everything --bursts does; the baseline window keeps bursts on)
    cfg = dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", 8192)
    B, nk = cfg.block_size, args.capture_chunks
    off = [f - CZ.DEFAULT_CENTRE_HZ for f in CZ.US_CHANNELS_HZ]
    damaged = whole = None
    if repair:                        # a CRC-invalid twin per channel: sync-valid, one payload symbol wrong
        body = [bytes([(37 * c + j) & 0xFF for j in range(6)]) for c in range(len(off))]
        damaged = [synth.make_packet(c % 8, body[c], flip_bit=(7 * c) % 64).hex() for c in range(len(off))]
        whole = [synth.make_packet(c % 8, body[c]) for c in range(len(off))]     # what a right repair gives back
    raw, info = synth.synth_wideband(range(200, 200 + len(off)), off, nk * B, amplitude=0.05,
                                     sample_format=args.sample_format, **({"payloads": damaged} if repair else {}))
    rx = wideband.WidebandReceiver(cfg, sample_format=args.sample_format)
    rx.set_parse(args.parse)
    ctl = None
    if args.levels:
        from rtldavis_amd import agc
        rx.set_levels(True)
        ctl = agc.GainControl(rx.n_channels, B)
    n_msgs = [0]
    step = 2 * rx.chunk_samples      # array elements per chunk
    chunks = [np.ascontiguousarray(raw[step * k: step * (k + 1)]) for k in range(nk)]
    acq, thr0, n_bursts, n_asked = None, None, [0], [0]
    if args.bursts:
        from rtldavis_amd import acquire
        acq = acquire.Acquisition(rx.n_channels, cfg)
        rx.set_bursts(True)
        rx.demodulate(chunks[0])     # (no burst starts inside the first chunk: its floor gives the first thresholds)
        thr0 = acq.thresholds(rx.bursts().floor)
        rx.set_bursts(False)
    moved = np.zeros(rx.n_channels, np.int64)
    moved[[25] if args.retune == "one" else slice(None)] = 1

    bursts_on, decode_on, n_dmsgs, n_repaired, n_right, base_msgs = [False], [False], [0], [0], [0], [0]
    n_narrow = [0]
    track_on, n_xmsgs, n_xcand = [False], [0], [0]
    quality_on, n_qrows, q_snr = [False], [0], []
    clips_on, n_clips, n_clip_out, n_clip_drop, clip_kinds = [False], [0], [0], [0], [0] * 5
    # the capture's bursts lie on their channels' centres: the nearest grid point first, then its neighbours
    search_on, n_smsgs, n_shits = [False], [0], [0]
    centres = [(48 + d) % 64 for d in (0, -1, 1, -2, 2, -3, 3, -4)][:search]

    def track_table(clock):
        """8 expectations, every one with 201 candidates inside the chunk that begins at `clock`, spread over the channels."""
        t = np.zeros(8, wideband.EXPECT_DTYPE)
        for i in range(8):
            t[i] = ((6 * i) % rx.n_channels, 0xFF, clock + 1000 + 100 * i, clock + 1200 + 100 * i, 0, -16384)
        return t

    def meter():
        if ctl is not None:
            g = ctl.update(rx.levels())
            if g is not None:
                rx.set_gain(g)
        if bursts_on[0]:
            b = rx.bursts()
            n_bursts[0] += len(b.records)
            rx.set_burst_threshold(acq.thresholds(b.floor))
            msgs = None
            if decode_on[0]:
                msgs = rx.burst_messages()
                n_dmsgs[0] += len(msgs.records)
                if narrow:
                    n_narrow[0] += int(acquire.narrowband(msgs.records).sum())
                if quality_on[0]:
                    q = rx.burst_message_quality()
                    n_qrows[0] += len(q)
                    if len(q):
                        q_snr[:] = [q]                       # (turned into decibels after the window, outside the timing)
                if clips_on[0]:
                    bc = rx.burst_clips()
                    n_clips[0] += len(bc.records)
                    n_clip_out[0] += len(bc.iq)
                    n_clip_drop[0] += int(bc.dropped.astype(np.int64).sum())
                    for s_ in bc.records["source"]:
                        clip_kinds[int(s_)] += 1
                if search_on[0]:
                    sm = rx.searched_messages()
                    n_smsgs[0] += len(sm.records)
                    n_shits[0] += int(sm.sync_hits.astype(np.int64).sum())
                if track_on[0]:
                    x = rx.expected_messages()
                    n_xmsgs[0] += len(x.records)
                    n_xcand[0] += int(x.candidates.astype(np.int64).sum())
                if repair:
                    rep = msgs.records[acquire.repaired(msgs.records)]
                    n_repaired[0] += len(rep)
                    n_right[0] += sum(bytes(r["data"]) == whole[int(r["channel"])] for r in rep)
            n_asked[0] += acq.update(b, rx.parsed() if args.parse else (), rx.submitted, msgs) is not None

    def run(n):
        """n chunks round and round through submit / fetch, two in flight; per-chunk latency and packets."""
        lat, pk = [], []
        t_sub = []
        t0 = time.perf_counter()
        for k in range(n):
            if rx.inflight == 2:
                pk.append(rx.fetch())
                if args.parse:
                    n_msgs[0] += len(rx.parsed())
                meter()
                lat.append(time.perf_counter() - t_sub[len(pk) - 1])
            t_sub.append(time.perf_counter())
            if args.retune != "none":
                rx.retune(moved * ((k + 1) & 1))
            if track_on[0]:
                rx.set_burst_expect(track_table(rx.submitted * B))
            rx.submit(chunks[k % nk])
        while rx.inflight:
            pk.append(rx.fetch())
            if args.parse:
                n_msgs[0] += len(rx.parsed())
            meter()
            lat.append(time.perf_counter() - t_sub[len(pk) - 1])
        return time.perf_counter() - t0, np.array(lat), pk

    run(args.warmup)
    runs, runs_off = [], []
    for _ in range(args.repeats):
        for on in ((False, True) if args.bursts else (False,)):
            rx.reset()
            if args.bursts:
                rx.set_bursts(on or decode)
                rx.set_burst_decode((on and decode) or repair > 0 or narrow or track or quality or search > 0 or clips)
                if search:
                    rx.set_burst_search(centres if on else [])
                search_on[0] = on and search > 0
                n_smsgs[0] = n_shits[0] = 0
                if repair:
                    rx.set_burst_repair(repair if on else 0)
                if narrow:
                    rx.set_burst_narrow(on)
                if quality:
                    rx.set_burst_quality(on)
                quality_on[0] = on and quality
                if clips:
                    rx.set_burst_clips(*((wideband.CLIP_RUNS | wideband.CLIP_MESSAGES,) if on else (0,)))
                clips_on[0] = on and clips
                n_clips[0] = n_clip_out[0] = n_clip_drop[0] = 0
                clip_kinds[:] = [0] * 5
                n_qrows[0] = 0
                del q_snr[:]
                bursts_on[0], decode_on[0] = on or decode, (on and decode) or repair > 0 or narrow or track or quality or search > 0 or clips
                track_on[0] = on and track
                n_dmsgs[0] = n_repaired[0] = n_right[0] = n_narrow[0] = n_xmsgs[0] = n_xcand[0] = 0
                acq.reset()
                rx.set_burst_threshold(thr0)
                n_bursts[0] = n_asked[0] = 0
            n_msgs[0] = 0
            (runs if on or not args.bursts else runs_off).append(run(args.chunks))
            if not on:
                base_msgs[0] = n_dmsgs[0]
    walls = [r[0] for r in runs]
    wall, lat, pk = sorted(runs, key=lambda r: r[0])[len(runs) // 2]   # the median window
    # the first pass over the capture (chunks 0 .. nk-1 after the reset): every channel's burst where it was injected
    found = 0
    for c, (payload, start) in enumerate(info):
        hits = [(k, p.index) for k in range(min(nk, len(pk))) for p in pk[k][c] if bytes(p.data).hex() == payload]
        found += any(0 <= (k - 1) * B + i - (start + 32 * 14) <= 30 for k, i in hits)
    out_rate = rx.out_rate
    air = args.chunks * B / out_rate
    res = {
        "chunks": args.chunks, "capture_chunks": nk, "warmup": args.warmup, "channels": rx.n_channels,
        "block_size": B, "decim": rx.decim, "chunk_bytes": rx.chunk_bytes,
        "sample_format": args.sample_format, "chunk_air_ms": 1e3 * B / out_rate,
        "repeats": args.repeats, "wall_s": wall, "wall_s_all": walls, "chunks_per_s": args.chunks / wall,
        "latency_ms": {"median": float(np.median(lat) * 1e3), "p99": float(np.percentile(lat, 99) * 1e3),
                       "max": float(lat.max() * 1e3), "min": float(lat.min() * 1e3)},
        "wideband_msps": args.chunks * rx.decim * B / wall / 1e6,
        "realtime_factor": air / wall,
        "injected_packets": len(info), "recovered_first_pass": int(found),
        "packets_total": int(sum(len(x) for ch in pk for x in ch)),
        "parse": bool(args.parse), "retune": args.retune, "levels": bool(args.levels), "bursts_on": bool(args.bursts),
    }
    if args.bursts:
        w_off, l_off, _ = sorted(runs_off, key=lambda r: r[0])[len(runs_off) // 2]
        res["bursts"] = {"records_last_window": n_bursts[0], "retunes_proposed_last_window": n_asked[0],
                         "off": {"wall_s": w_off, "wall_s_all": [r[0] for r in runs_off], "chunks_per_s": args.chunks / w_off,
                                 "latency_ms_median": float(np.median(l_off) * 1e3)}}
        lines = [
            "WidebandReceiver burst detection (k_chan_bursts), on against off in the same run: tools/wideband_stream.py --bursts"
            + (" --parse" if args.parse else ""),
            f"{rx.n_channels} channels, chunks of {B} outputs ({1e3 * B / out_rate:.1f} ms air, {rx.chunk_bytes} bytes, {args.sample_format}), "
            f"{args.chunks} chunks per window, {args.repeats} windows each, alternating; the median window is reported",
            f"  bursts off: {args.chunks / w_off:8.1f} chunks/s, submit -> fetch median {np.median(l_off) * 1e3:.3f} ms",
            f"  bursts on:  {res['chunks_per_s']:8.1f} chunks/s, submit -> fetch median {res['latency_ms']['median']:.3f} ms "
            f"(bursts() read, thresholds set and Acquisition.update run per chunk)",
            f"  all windows, wall s: off {' '.join(f'{r[0]:.3f}' for r in runs_off)}; on {' '.join(f'{w:.3f}' for w in walls)}",
            f"  last window on: {n_bursts[0]} burst records, {n_asked[0]} retunes proposed",
        ]
        if decode:
            res["burst_decode"] = {"messages_last_window": n_dmsgs[0]}
            lines = [
                "WidebandReceiver burst decode (k_chan_burst_decode), bursts + decode on against bursts on in the same run: "
                "tools/wideband_stream.py --burst-decode" + (" --parse" if args.parse else ""),
                lines[1],
                f"  bursts on:           {args.chunks / w_off:8.1f} chunks/s, submit -> fetch median {np.median(l_off) * 1e3:.3f} ms",
                f"  bursts + decode on:  {res['chunks_per_s']:8.1f} chunks/s, submit -> fetch median {res['latency_ms']['median']:.3f} ms "
                f"(burst_messages() read and handed to Acquisition.update per chunk)",
                f"  all windows, wall s: bursts {' '.join(f'{r[0]:.3f}' for r in runs_off)}; bursts + decode {' '.join(f'{w:.3f}' for w in walls)}",
                f"  last window with decode: {n_bursts[0]} burst records, {n_dmsgs[0]} burst messages, {n_asked[0]} retunes proposed",
            ]
        if repair:
            res["burst_repair"] = {"max_flips": repair, "messages_last_window": n_dmsgs[0], "repaired_last_window": n_repaired[0],
                                   "repaired_right_last_window": n_right[0], "messages_last_window_without": base_msgs[0]}
            w_all_off, w_all_on = [r[0] for r in runs_off], walls
            spread = max(max(w_all_off) - min(w_all_off), max(w_all_on) - min(w_all_on))
            diff = wall - w_off
            overlap = min(w_all_on) <= max(w_all_off) and min(w_all_off) <= max(w_all_on)
            lines = [
                f"WidebandReceiver burst repair (k_chan_burst_decode<true>, max_flips {repair}), bursts + decode + repair on against bursts + "
                f"decode on in the same run: tools/wideband_stream.py --burst-repair {repair}" + (" --parse" if args.parse else ""),
                lines[1] + "; every channel's burst is a CRC-invalid twin (one payload symbol wrong, full strength)",
                f"  bursts + decode on:           {args.chunks / w_off:8.1f} chunks/s, submit -> fetch median {np.median(l_off) * 1e3:.3f} ms",
                f"  bursts + decode + repair on:  {res['chunks_per_s']:8.1f} chunks/s, submit -> fetch median {res['latency_ms']['median']:.3f} ms "
                f"(burst_messages() read and handed to Acquisition.update per chunk)",
                f"  all windows, wall s: decode {' '.join(f'{w:.3f}' for w in w_all_off)}; decode + repair {' '.join(f'{w:.3f}' for w in w_all_on)}",
                f"  median window: repair {diff * 1e3:+.1f} ms of wall ({100 * diff / w_off:+.1f} %); the windows of one setting spread over "
                f"{spread * 1e3:.1f} ms, and the windows of the two settings {'overlap: the difference lies inside' if overlap else 'do NOT overlap: the difference lies outside'} their spread",
                f"  last window with repair: {n_bursts[0]} burst records, {n_dmsgs[0]} burst messages of which {n_repaired[0]} repaired "
                f"({n_right[0]} of those with the channel's undamaged payload), {n_asked[0]} retunes proposed; last window without: "
                f"{base_msgs[0]} burst messages - the difference includes the host's handling of the additional rows",
                "  measured: wall time per window on the host (time.perf_counter around submit / fetch), this run; the kernel's own time: not measured",
            ]
        if narrow:
            res["burst_narrow"] = {"messages_last_window": n_dmsgs[0], "narrow_rows_last_window": n_narrow[0],
                                   "messages_last_window_without": base_msgs[0]}
            w_all_off, w_all_on = [r[0] for r in runs_off], walls
            spread = max(max(w_all_off) - min(w_all_off), max(w_all_on) - min(w_all_on))
            diff = wall - w_off
            overlap = min(w_all_on) <= max(w_all_off) and min(w_all_off) <= max(w_all_on)
            lines = [
                "WidebandReceiver narrow-band burst filter (k_chan_burst_decode<false, true>), bursts + decode + narrow on against bursts + "
                "decode on in the same run: tools/wideband_stream.py --burst-narrow" + (" --parse" if args.parse else ""),
                lines[1] + "; a burst on every channel",
                f"  bursts + decode on:           {args.chunks / w_off:8.1f} chunks/s, submit -> fetch median {np.median(l_off) * 1e3:.3f} ms",
                f"  bursts + decode + narrow on:  {res['chunks_per_s']:8.1f} chunks/s, submit -> fetch median {res['latency_ms']['median']:.3f} ms "
                f"(burst_messages() read and handed to Acquisition.update per chunk)",
                f"  all windows, wall s: decode {' '.join(f'{w:.3f}' for w in w_all_off)}; decode + narrow {' '.join(f'{w:.3f}' for w in w_all_on)}",
                f"  median window: narrow {diff * 1e3:+.1f} ms of wall ({100 * diff / w_off:+.1f} %); the windows of one setting spread over "
                f"{spread * 1e3:.1f} ms, and the windows of the two settings {'overlap: the difference lies inside' if overlap else 'do NOT overlap: the difference lies outside'} their spread",
                f"  last window with narrow: {n_bursts[0]} burst records, {n_dmsgs[0]} burst messages, all {n_narrow[0]} of them narrow rows, "
                f"{n_asked[0]} retunes proposed; last window without: {base_msgs[0]} burst messages",
                "  measured: wall time per window on the host (time.perf_counter around submit / fetch), this run; the kernel's own time: not measured",
            ]
        if track:
            res["burst_track"] = {"expectations_per_chunk": 8, "candidates_last_window": n_xcand[0], "expected_messages_last_window": n_xmsgs[0]}
            w_all_off, w_all_on = [r[0] for r in runs_off], walls
            spread = max(max(w_all_off) - min(w_all_off), max(w_all_on) - min(w_all_on))
            diff = wall - w_off
            overlap = min(w_all_on) <= max(w_all_off) and min(w_all_off) <= max(w_all_on)
            lines = [
                "WidebandReceiver burst expect (k_chan_burst_expect<false, false>), bursts + decode + 8 expectations active in every chunk "
                "against bursts + decode on in the same run: tools/wideband_stream.py --track" + (" --parse" if args.parse else ""),
                lines[1] + "; a burst on every channel; per chunk set_burst_expect with 8 windows of 201 candidates inside the chunk",
                f"  bursts + decode on:                   {args.chunks / w_off:8.1f} chunks/s, submit -> fetch median {np.median(l_off) * 1e3:.3f} ms",
                f"  bursts + decode + 8 expectations on:  {res['chunks_per_s']:8.1f} chunks/s, submit -> fetch median {res['latency_ms']['median']:.3f} ms "
                f"(set_burst_expect per submit, expected_messages() read per fetch)",
                f"  all windows, wall s: decode {' '.join(f'{w:.3f}' for w in w_all_off)}; decode + expectations {' '.join(f'{w:.3f}' for w in w_all_on)}",
                f"  median window: expectations {diff * 1e3:+.1f} ms of wall ({100 * diff / w_off:+.1f} %); the windows of one setting spread over "
                f"{spread * 1e3:.1f} ms, and the windows of the two settings {'overlap: the difference lies inside' if overlap else 'do NOT overlap: the difference lies outside'} their spread",
                f"  last window with expectations: {n_xcand[0]} candidates tested ({n_xcand[0] / max(args.chunks, 1):.0f} per chunk), {n_xmsgs[0]} expected messages, "
                f"{n_dmsgs[0]} burst messages; last window without: {base_msgs[0]} burst messages",
                "  measured: wall time per window on the host (time.perf_counter around submit / fetch), this run; the kernel's own time: not measured",
            ]
        if quality:
            res["burst_quality"] = {"messages_last_window": n_dmsgs[0], "quality_rows_last_window": n_qrows[0],
                                    "messages_last_window_without": base_msgs[0]}
            w_all_off, w_all_on = [r[0] for r in runs_off], walls
            spread = max(max(w_all_off) - min(w_all_off), max(w_all_on) - min(w_all_on))
            diff = wall - w_off
            overlap = min(w_all_on) <= max(w_all_off) and min(w_all_off) <= max(w_all_on)
            snr_txt = "no rows"
            if q_snr:
                db = [(acquire.rssi_db(r, cfg.symbol_length), acquire.snr_db(r, cfg.symbol_length), acquire.snr_inband_db(r, cfg.symbol_length)) for r in q_snr[0]]
                snr_txt = "the last chunk's rows: median rssi_db %.1f, snr_db %.1f, snr_inband_db %.1f" % tuple(np.median(np.array(db), axis=0))
            lines = [
                "WidebandReceiver burst quality (k_chan_burst_quality behind k_chan_burst_decode), bursts + decode + quality on against bursts + "
                "decode on in the same run: tools/wideband_stream.py --burst-quality" + (" --parse" if args.parse else ""),
                lines[1] + "; a burst on every channel",
                f"  bursts + decode on:            {args.chunks / w_off:8.1f} chunks/s, submit -> fetch median {np.median(l_off) * 1e3:.3f} ms",
                f"  bursts + decode + quality on:  {res['chunks_per_s']:8.1f} chunks/s, submit -> fetch median {res['latency_ms']['median']:.3f} ms "
                f"(burst_messages() and burst_message_quality() read per chunk, the messages handed to Acquisition.update)",
                f"  all windows, wall s: decode {' '.join(f'{w:.3f}' for w in w_all_off)}; decode + quality {' '.join(f'{w:.3f}' for w in w_all_on)}",
                f"  median window: quality {diff * 1e3:+.1f} ms of wall ({100 * diff / w_off:+.1f} %); the windows of one setting spread over "
                f"{spread * 1e3:.1f} ms, and the windows of the two settings {'overlap: the difference lies inside' if overlap else 'do NOT overlap: the difference lies outside'} their spread",
                f"  last window with quality: {n_bursts[0]} burst records, {n_dmsgs[0]} burst messages, {n_qrows[0]} quality rows ({snr_txt}), "
                f"{n_asked[0]} retunes proposed; last window without: {base_msgs[0]} burst messages",
                "  measured: wall time per window on the host (time.perf_counter around submit / fetch), this run; the kernel's own time: not measured",
            ]
        if clips:
            res["burst_clips"] = {"clips_last_window": n_clips[0], "outputs_last_window": n_clip_out[0], "dropped_last_window": n_clip_drop[0],
                                  "by_source_last_window": list(clip_kinds), "settings": list(rx.burst_clips_config()),
                                  "messages_last_window": n_dmsgs[0], "messages_last_window_without": base_msgs[0]}
            w_all_off, w_all_on = [r[0] for r in runs_off], walls
            spread = max(max(w_all_off) - min(w_all_off), max(w_all_on) - min(w_all_on))
            diff = wall - w_off
            overlap = min(w_all_on) <= max(w_all_off) and min(w_all_off) <= max(w_all_on)
            _, c_pre, c_post, c_quota = rx.burst_clips_config()
            per_chunk = 2.0 * n_clip_out[0] / max(args.chunks, 1)
            lines = [
                "WidebandReceiver burst clips (k_chan_burst_clips behind k_chan_burst_decode), bursts + decode + clips on against bursts + "
                "decode on in the same run: tools/wideband_stream.py --burst-clips" + (" --parse" if args.parse else ""),
                lines[1] + f"; a burst on every channel; clips of runs and messages, pre {c_pre}, post {c_post}, quota {c_quota} outputs",
                f"  bursts + decode on:          {args.chunks / w_off:8.1f} chunks/s, submit -> fetch median {np.median(l_off) * 1e3:.3f} ms",
                f"  bursts + decode + clips on:  {res['chunks_per_s']:8.1f} chunks/s, submit -> fetch median {res['latency_ms']['median']:.3f} ms "
                f"(burst_messages() and burst_clips() read per chunk, the messages handed to Acquisition.update)",
                f"  all windows, wall s: decode {' '.join(f'{w:.3f}' for w in w_all_off)}; decode + clips {' '.join(f'{w:.3f}' for w in w_all_on)}",
                f"  median window: clips {diff * 1e3:+.1f} ms of wall ({100 * diff / w_off:+.1f} %); the windows of one setting spread over "
                f"{spread * 1e3:.1f} ms, and the windows of the two settings {'overlap: the difference lies inside' if overlap else 'do NOT overlap: the difference lies outside'} their spread",
                f"  last window with clips: {n_clips[0]} clips (tail / run / decode / expected / searched: {' / '.join(str(v) for v in clip_kinds)}), "
                f"{n_clip_out[0]} outputs = {per_chunk / 1024:.1f} KiB per chunk of the {rx.n_channels * 2 * B / 1024:.0f} KiB channelized "
                f"(counted: the bytes burst_clips() handed over), {n_clip_drop[0]} requests dropped, {n_bursts[0]} burst records, {n_dmsgs[0]} burst messages; "
                f"last window without: {base_msgs[0]} burst messages",
                "  measured: wall time per window on the host (time.perf_counter around submit / fetch), this run; the kernel's own time: not measured",
            ]
        if search:
            res["burst_search"] = {"centres": centres, "searched_messages_last_window": n_smsgs[0], "sync_hits_last_window": n_shits[0]}
            w_all_off, w_all_on = [r[0] for r in runs_off], walls
            spread = max(max(w_all_off) - min(w_all_off), max(w_all_on) - min(w_all_on))
            diff = wall - w_off
            overlap = min(w_all_on) <= max(w_all_off) and min(w_all_off) <= max(w_all_on)
            air_rate = out_rate / B
            lines = [
                f"WidebandReceiver burst search (k_chan_burst_search, {search} centre{'s' if search > 1 else ''} {centres}), bursts + decode + search on "
                f"against bursts + decode on in the same run: tools/wideband_stream.py --burst-search {search}" + (" --parse" if args.parse else ""),
                lines[1] + "; a burst on every channel, on its centre",
                f"  bursts + decode on:           {args.chunks / w_off:8.1f} chunks/s, submit -> fetch median {np.median(l_off) * 1e3:.3f} ms",
                f"  bursts + decode + search on:  {res['chunks_per_s']:8.1f} chunks/s, submit -> fetch median {res['latency_ms']['median']:.3f} ms "
                f"(searched_messages() read per fetch)",
                f"  the air delivers {air_rate:.1f} chunks/s: search on runs at {res['chunks_per_s'] / air_rate:.1f} x real time",
                f"  all windows, wall s: decode {' '.join(f'{w:.3f}' for w in w_all_off)}; decode + search {' '.join(f'{w:.3f}' for w in w_all_on)}",
                f"  median window: search {diff * 1e3:+.1f} ms of wall ({100 * diff / w_off:+.1f} %); the windows of one setting spread over "
                f"{spread * 1e3:.1f} ms, and the windows of the two settings {'overlap: the difference lies inside' if overlap else 'do NOT overlap: the difference lies outside'} their spread",
                f"  last window with search: {n_smsgs[0]} searched messages, {n_shits[0]} sync hits over {search * rx.n_channels} (centre, channel) pairs, "
                f"{n_dmsgs[0]} burst messages; last window without: {base_msgs[0]} burst messages",
                "  measured: wall time per window on the host (time.perf_counter around submit / fetch), this run; the kernel's own time: not measured",
            ]
        with open(args.burst_clips_out if clips else args.burst_search_out if search else args.burst_quality_out if quality else args.track_out if track else args.burst_narrow_out if narrow else args.burst_repair_out if repair else args.burst_decode_out if decode else args.bursts_out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        print("\n".join(lines))
    if args.parse:
        import math
        res["messages_last_window"] = n_msgs[0]
        # the route without device parse: one chunk at a time, the receiver quiet when its state is read
        rq = wideband.WidebandReceiver(cfg, sample_format=args.sample_format)
        rq.demodulate(chunks[0])
        rq.reset()
        n, nm, t0 = max(args.chunks // 4, nk), 0, time.perf_counter()
        for k in range(n):
            for c, ps in enumerate(rq.demodulate(chunks[k % nk])):
                for p in ps:
                    if dsp.parse_packet(p.data) is not None:
                        mean = np.mean(rq.discriminated(c)[p.index: p.index + cfg.preamble_length])
                        nm += isinstance(-int((mean * float(cfg.sample_rate)) / (2 * math.pi)), int)
        dt = time.perf_counter() - t0
        res["host_route"] = {"chunks": n, "chunks_per_s": n / dt, "messages": nm}
        print(f"parsed() per chunk: {n_msgs[0]} messages in the last window; without device parse (quiet receiver, "
              f"discriminated(channel) per CRC-valid packet): {n / dt:.0f} chunks/s over {n} chunks, {nm} messages")
    print(f"{args.chunks} chunks of {1e3 * B / out_rate:.1f} ms air x {rx.n_channels} channels in {wall:.3f} s: "
          f"{res['chunks_per_s']:.0f} chunks/s, {res['wideband_msps']:.0f} wideband MS/s, real-time factor "
          f"{res['realtime_factor']:.0f}x")
    print(f"latency submit -> fetch: median {res['latency_ms']['median']:.3f} ms, p99 {res['latency_ms']['p99']:.3f} ms, "
          f"max {res['latency_ms']['max']:.3f} ms")
    print(f"first pass: {found} of {len(info)} injected packets recovered")
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)
    if found != len(info):
        raise SystemExit(f"only {found} of {len(info)} injected packets recovered")


if __name__ == "__main__":
    main()
