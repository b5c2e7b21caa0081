"""What the HIP runtime is asked to do by the batch demodulator's host code (rtldavis_amd/csrc/rd_batch.hip), for comparing two
builds of the library (profiles/batch_host_refactor.txt).

  python3 tools/batch_api_session.py run
      Twelve scripted sessions of 6 streams x synth.BLOCKS_PER_STREAM blocks in this process, one after the other: plain;
      pipelined, three runs queued on one stream; pipelined and rerun on another stream; timing 1; timing 2; parse on;
      upload_async on a copy stream; a run left unfetched before the next upload; RD_TAIL_IMPL=legacy; legacy with lists
      that really grow (RD_TEST_MATCH_CAP); RD_TEST_BUCKET_CAP=2; RD_TEST_FIX_BCAP=8 on a quiet input.  Every session
      asserts, through last_run_forms() and the counters, that the form it is about really ran, and prints a digest of its
      records.  Three rd_device_count() calls in a row mark the borders create | first run .. last fetch | destroy.
      Run it under HIP API tracing alone (python3 straight after `--`), once per library (RTLDAVIS_HIP_LIB).
  python3 tools/batch_api_session.py compare A_hip_api_trace.csv B_hip_api_trace.csv
      The two traces, session by session: the ordered list of API names from first run to last fetch (a run of one polling
      query, hipEventQuery or hipStreamQuery, counts as one call), the multiset of names at create and at destroy.
      Exit status 1 when any of them differs."""
import collections
import csv
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HOOKS = ("RD_TAIL_IMPL", "RD_TEST_MATCH_CAP", "RD_TEST_BUCKET_CAP", "RD_TEST_FIX_BCAP")
NAMES = ["plain", "pipelined, three runs queued", "pipelined, rerun on another stream", "timing 1", "timing 2", "parse on",
         "upload_async on a copy stream", "a run left unfetched before an upload", "RD_TAIL_IMPL=legacy",
         "legacy, RD_TEST_MATCH_CAP=7", "RD_TEST_BUCKET_CAP=2", "RD_TEST_FIX_BCAP=8, quiet input"]
ONE_LAUNCH = {"ordered_tail": True, "second_pass": False, "one_launch_tail": True}
SEPARATE = {"ordered_tail": False, "second_pass": False, "one_launch_tail": False}
FELL_BACK = {"ordered_tail": False, "second_pass": True, "one_launch_tail": False}


def run():
    import numpy as np
    from rtldavis_amd import _lib, batch, dsp, synth
    L = _lib.lib()
    cfg = dsp.PacketConfig(19200, 14, 16, 80, "1100101110001001", 8192)
    NS, NB = 6, synth.BLOCKS_PER_STREAM
    raw = np.ascontiguousarray(synth.synth_streams(range(NS)))
    other = np.ascontiguousarray(synth.synth_streams(range(NS, 2 * NS)))
    rng = np.random.default_rng(3)
    quiet = np.stack([rng.integers(126, 130, size=raw.shape[1], dtype=np.uint8) for _ in range(NS - 1)] + [synth.synth_stream(9)])
    hip = C.CDLL("libamdhip64.so")
    digest = hashlib.sha256()

    def mark():
        for _ in range(3):
            L.rd_device_count()

    def stream():
        st = C.c_void_p()
        assert hip.hipStreamCreate(C.byref(st)) == 0
        return st.value

    def handles(n, env, data=raw):
        for k in HOOKS:
            os.environ.pop(k, None)
        os.environ.update(env)
        hs = [batch.BatchDemodulator(cfg, NS, NB) for _ in range(n)]
        for h in hs:
            h.upload(data)   # (the first device call: the hooks are read here)
        return hs

    def fetch(h, forms):
        digest.update(h.results().tobytes())
        f = h.last_run_forms()
        assert f == forms, (f, forms)

    def session(name, n, env, body, data=raw, prepare=None):
        assert name == NAMES[session.count], name
        session.count += 1
        mark()
        hs = handles(n, env, data)
        extra = prepare(hs) if prepare else None
        mark()
        body(hs, extra)
        mark()
        for h in hs:
            h.close()
        print("session %-40s %s" % (name, digest.hexdigest()[:16]), flush=True)
    session.count = 0

    def plain(hs, _):
        for _ in range(2):
            hs[0].run()
            fetch(hs[0], ONE_LAUNCH)
    session(NAMES[0], 1, {}, plain)

    def queued(hs, _):
        for _ in range(2):
            for h in hs:
                h.run()
            for h in hs:
                fetch(h, ONE_LAUNCH)
    session(NAMES[1], 3, {}, queued, prepare=lambda hs: [h.set_pipelined(True) for h in hs])

    def rerun(hs, st2):
        for _ in range(2):
            hs[0].run(0)
            hs[0].run(st2)
            fetch(hs[0], ONE_LAUNCH)
            hs[0].run(st2)
            hs[0].run(0)
            fetch(hs[0], ONE_LAUNCH)

    def rerun_prepare(hs):
        hs[0].set_pipelined(True)
        return stream()
    session(NAMES[2], 1, {}, rerun, prepare=rerun_prepare)

    def timed(level):
        def body(hs, _):
            for _ in range(3):
                hs[0].run()
                fetch(hs[0], ONE_LAUNCH if level == 1 else SEPARATE)
            t = hs[0].timing()
            assert t["runs"] == 3 and t["demod_ms"] > 0 and t["total_ms"] > 0 and (t["search_ms"] > 0) == (level == 2), t
        return body
    session(NAMES[3], 1, {}, timed(1), prepare=lambda hs: hs[0].set_timing(1))
    session(NAMES[4], 1, {}, timed(2), prepare=lambda hs: hs[0].set_timing(2))

    def parse(hs, _):
        for _ in range(2):
            hs[0].run()
            fetch(hs[0], ONE_LAUNCH)
            assert len(hs[0].parsed()) == NS   # one CRC-valid message per stream
    session(NAMES[5], 1, {}, parse, prepare=lambda hs: hs[0].set_parse(True))

    def async_upload(hs, cs):
        for data in (other, raw, other):
            hs[0].upload_async(data, cs)
            hs[0].run()
            fetch(hs[0], ONE_LAUNCH)
        hs[0].upload_async(raw, cs)
        hs[0].run()
        hs[0].upload_async(other, cs)   # queues behind the run that still reads the input
        hs[0].run()
        fetch(hs[0], ONE_LAUNCH)
    session(NAMES[6], 1, {}, async_upload, prepare=lambda hs: stream())

    def unfetched(hs, _):
        hs[0].run()
        hs[0].upload(other)   # the host waits for the run nobody fetched
        hs[0].run()
        fetch(hs[0], ONE_LAUNCH)
        hs[0].set_pipelined(True)
        hs[0].run()
        hs[0].upload(raw)     # ... which is flushed first when it is parked
        hs[0].run()
        fetch(hs[0], ONE_LAUNCH)
    session(NAMES[7], 1, {}, unfetched)

    def legacy(hs, _):
        for _ in range(2):
            hs[0].run()
            fetch(hs[0], SEPARATE)
    session(NAMES[8], 1, {"RD_TAIL_IMPL": "legacy"}, legacy)

    def grow(hs, _):
        hs[0].run()
        fetch(hs[0], FELL_BACK)          # the lists grew: search and slice ran again
        assert hs[0].counters()["matches"] > 7
        hs[0].run()
        fetch(hs[0], SEPARATE)           # ... and are long enough now
    session(NAMES[9], 1, {"RD_TAIL_IMPL": "legacy", "RD_TEST_MATCH_CAP": "7"}, grow)

    def lds_list(hs, _):
        hs[0].run()
        fetch(hs[0], FELL_BACK)
        hs[0].run()
        fetch(hs[0], SEPARATE)           # remembered until the next upload
        hs[0].upload(raw)
        hs[0].run()
        fetch(hs[0], FELL_BACK)
    session(NAMES[10], 1, {"RD_TEST_BUCKET_CAP": "2"}, lds_list)

    def buckets(hs, _):
        hs[0].run()
        # every run was re-evaluated exactly: the fix-up count is the number of 32-sample runs (asked first: a later call
        # that completes the run again reports the device's counter instead)
        assert hs[0].counters()["fixup_runs"] == NS * NB * 8192 // 32, hs[0].counters()
        fetch(hs[0], FELL_BACK)
        hs[0].run()
        fetch(hs[0], SEPARATE)
        hs[0].upload(quiet)
        hs[0].run()
        fetch(hs[0], FELL_BACK)
    session(NAMES[11], 1, {"RD_TEST_FIX_BCAP": "8"}, buckets, data=quiet)
    mark()
    print("sessions ok %d records digest %s library %s" % (session.count, digest.hexdigest(), os.path.basename(os.path.dirname(_lib.LIB_PATH))))


POLLS = ("hipEventQuery", "hipStreamQuery")


def segments(path):
    """The trace's API names in start order, split at the marks (three or more hipGetDeviceCount in a row); the process's
    start-up in front of the first mark is dropped."""
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Function"] for r in rows]
    segs, cur, i = [], [], 0
    while i < len(names):
        j = i
        while j < len(names) and names[j] == "hipGetDeviceCount":
            j += 1
        if j - i >= 3:
            segs.append(cur)
            cur = []
            i = j
        else:
            cur.append(names[i])
            i += 1
    return segs[1:], sum(n in POLLS for n in names)


def squeeze(names):
    out = []
    for n in names:
        if not (out and out[-1] == n and n in POLLS):
            out.append(n)
    return out


def compare(a_path, b_path):
    (a, a_polls), (b, b_polls) = segments(a_path), segments(b_path)
    assert len(a) == len(b) == 3 * len(NAMES), (len(a), len(b))
    print("polling queries in all: %d / %d" % (a_polls, b_polls))
    bad = 0
    for k, name in enumerate(NAMES):
        ca, cb = collections.Counter(a[3 * k]), collections.Counter(b[3 * k])
        sa, sb = squeeze(a[3 * k + 1]), squeeze(b[3 * k + 1])
        da, db = collections.Counter(squeeze(a[3 * k + 2])), collections.Counter(squeeze(b[3 * k + 2]))
        same = (ca == cb, sa == sb, da == db)
        bad += not all(same)
        print("  %-40s create %3d / %3d calls, multiset %s; session %4d / %4d calls, sequence %s; destroy %2d / %2d calls, multiset %s"
              % (name, sum(ca.values()), sum(cb.values()), "identical" if same[0] else "DIFFERENT", len(sa), len(sb),
                 "identical" if same[1] else "DIFFERENT", sum(da.values()), sum(db.values()), "identical" if same[2] else "DIFFERENT"))
        if not same[1]:
            at = next((i for i, (x, y) in enumerate(zip(sa, sb)) if x != y), min(len(sa), len(sb)))
            print("    first difference at call %d: %s | %s" % (at, sa[at - 2: at + 3], sb[at - 2: at + 3]))
        for what, x, y, ok in (("create", ca, cb, same[0]), ("destroy", da, db, same[2])):
            if not ok:
                print("    %s: only in A %s, only in B %s" % (what, dict(x - y), dict(y - x)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
