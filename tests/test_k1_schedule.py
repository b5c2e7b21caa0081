"""k_demod_mfma's work-queue schedule on the device (MI355X), at the small shapes of tests/k1_schedule_cases.py: the grid
capped at 8 workgroups by the test hook RD_TEST_K1_WGS, RD_K1_CHUNK at 4, 5, 8 (queues) and 1, 3 (equal shares), and the
uncapped grid at one workgroup per CU on a batch large enough for it.  What the model says a correct kernel writes, and that
five faults of the chunk transition would be noticed, is checked on the CPU (tests/test_k1_schedule_cpu.py).

The knobs are read once per process, so every setting is ONE child process that runs all its cases; inputs and outputs
travel through tmp_path and every assertion is made here.  The children run one after the other, each under a timeout
sized to its jobs; a child that fails, dies or times out fails its test there (no retry), and no later child of this
module starts: every later test fails at once, without touching the device.

Through the kernel hook (both instantiations): g = the integer model bit for bit, the words outside the list = the exact
bits, the list EXACTLY the model's flagged groups and the forced entries of the chunk grid that the launch reports, no
duplicate, zero bits past a ragged end.  Through BatchDemodulator: bits, packets, RSSI / SNR against the C oracle, the
reported schedule against the restated launch arithmetic, three data sets on one handle and the first again, the same
through pipelined handles; then RD_TAIL_IMPL=legacy and the overflow fallbacks with further runs on the same handle -
RD_TEST_BUCKET_CAP (a second pass whose bits are still the demod kernel's: the one that would show a queue word left
non-zero) and RD_TEST_FIX_BCAP / RD_TEST_MATCH_CAP (every run re-evaluated exactly: results only)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import k1_schedule_cases as K  # noqa: E402
import tail_scale_cases as TS  # noqa: E402  (assert_records_equal)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREAMBLE = "1100101110001001"
KNOBS = ("RD_TEST_K1_WGS", "RD_K1_CHUNK", "RD_K1_WGS_PER_CU", "RD_TAIL_IMPL", "RD_TEST_MATCH_CAP", "RD_TEST_FIX_BCAP",
         "RD_TEST_BUCKET_CAP")

CHILD = r'''
import json, os, sys
import numpy as np
spec = json.load(open(sys.argv[1]))
sys.path.insert(0, os.path.join(spec["root"], "tests"))
from rtldavis_amd import batch, dsp
import test_gpu_mfma as TM
z = np.load(spec["in"])
out = {}
for j in spec["hook"]:
    g, bits, fix, sched = TM.run_kernel(z[j["streams"]], z[j["hist"]] if j["hist"] else None, want_g=j["want_g"])
    out[j["tag"] + "/bits"], out[j["tag"] + "/fix"] = bits, fix
    out[j["tag"] + "/sched"] = np.array([sched["k1_chunk"], sched["k1_waves"]])
    if j["want_g"]:
        out[j["tag"] + "/g"] = g
for j in spec["batch"]:
    cfg = dsp.PacketConfig(19200, 14, 16, 80, spec["preamble"], 8192)
    hs = [batch.BatchDemodulator(cfg, j["ns"], j["nb"]) for _ in range(j["handles"])]
    for h in hs:
        h.set_pipelined(bool(j["pipelined"]))
    for op in j["ops"]:
        h = hs[op[1]]
        if op[0] == "upload":
            h.upload(z[op[2]])
        elif op[0] == "run":
            h.run()
        else:
            tag = j["tag"] + "/" + op[2]
            out[tag + "/recs"] = h.results().copy()
            out[tag + "/bits"] = np.stack([np.asarray(h.bits(i)) for i in range(j["ns"])])
            c, f = h.counters(), h.last_run_forms()
            out[tag + "/info"] = np.array([c["k1_chunk"], c["k1_waves"], c["fixup_runs"], c["matches"],
                                           int(f["one_launch_tail"]), int(f["second_pass"])], dtype=np.int64)
    for h in hs:
        h.close()
np.savez(spec["out"], **out)
'''


_DEAD = []   # the first child that failed, died or timed out: no later child is started


def _child(tmp_path, name, env, arrays, hook=(), batch=()):
    """one child process for one setting of the knobs; returns its outputs.  Timeout: 60 s for the start of the process
    and of the device, 5 s per hook launch, 3 s per run of a batch job (a job is a few hundred milliseconds; the limit is
    for a hang, it is never waited for)"""
    if _DEAD:
        pytest.fail(f"not started: child {_DEAD[0]} of this module failed, died or timed out before")
    timeout = 60 + 5 * len(hook) + 3 * sum(sum(op[0] == "run" for op in j["ops"]) for j in batch)
    d = tmp_path / name
    d.mkdir()
    np.savez(d / "in.npz", **arrays)
    spec = {"root": ROOT, "in": str(d / "in.npz"), "out": str(d / "out.npz"), "preamble": PREAMBLE, "hook": list(hook), "batch": list(batch)}
    (d / "spec.json").write_text(json.dumps(spec))
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(env)
    try:
        r = subprocess.run([sys.executable, "-c", CHILD, str(d / "spec.json")], env=e, cwd=ROOT, capture_output=True, text=True,
                           timeout=timeout)
    except subprocess.TimeoutExpired:
        _DEAD.append(f"{name} {env}")
        pytest.fail(f"child {name} {env}: no end after {timeout} s")
    if r.returncode != 0:
        _DEAD.append(f"{name} {env}")
    assert r.returncode == 0, f"child {name} {env}: exit {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
    return np.load(d / "out.npz")


def _reported(shape_ns, n, sched):
    chunk, waves = int(sched[0]), int(sched[1])
    tps = (n + K.TILE - 1) // K.TILE
    total = shape_ns * tps
    return K.Sched(total, tps, chunk, (total + chunk - 1) // chunk, waves, chunk >= 4)


def _hook_jobs(shape, arrays):
    """both instantiations, each on a data set of its own"""
    jobs = []
    for k, want_g in ((0, True), (1, False)):
        c = K.data(shape, k)
        arrays[f"{shape}/{k}"] = c.streams
        if c.hist is not None:
            arrays[f"{shape}/{k}/hist"] = c.hist
        jobs.append({"tag": f"hook/{shape}/{k}", "streams": f"{shape}/{k}", "hist": f"{shape}/{k}/hist" if c.hist is not None else "",
                     "want_g": want_g})
    return jobs


def _check_hook(z, shape, chunk_env, must_draw=True):
    want_sc = K.sched_of(shape, chunk_env)
    for k, want_g in ((0, True), (1, False)):
        c = K.data(shape, k)
        tag = f"hook/{shape}/{k}"
        what = f"{shape} chunk {chunk_env} data set {k} ({'with g' if want_g else 'product instantiation'})"
        sc = _reported(c.streams.shape[0], c.n, z[tag + "/sched"])
        assert sc == want_sc, f"{what}: the launch reports {sc}, the restated arithmetic gives {want_sc}"
        if must_draw:   # waves took further chunks: asserted from the reported values
            assert sc.chunks > sc.waves >= K.RD_NQUEUE, f"{what}: {sc}"
        g_bad = 0
        if want_g:
            g = z[tag + "/g"]
            t = np.arange(g.shape[1])
            ok = (t % K.TILE >= 1) & (t < c.n) & (t >= (9 if c.hist is None else 1))
            g_bad = int((g[:, ok] != c.g32[:, t[ok] + 1]).any(axis=-1).sum())
        K.check_outputs(c, sc, z[tag + "/bits"], z[tag + "/fix"], g_bad, what)
        print(f"{what}: {sc.chunks} chunks on {sc.waves} waves, {z[tag + '/fix'].size} entries = flagged + forced, g and signs exact")


SEQ = (0, 1, 2, 0)
MATCHLIST_CAP = 4   # RD_TEST_BUCKET_CAP of the matchlist child


def _batch_jobs(shape, arrays, tail_twice=False):
    """three data sets on one handle and the first again; then two pipelined handles with runs queued behind each other.
    tail_twice: a run without a new upload behind the second one (after an overflow that is the separate kernels' path)"""
    sh = K.SHAPES[shape]
    for k in range(K.N_SETS):
        arrays[f"{shape}/{k}"] = K.data(shape, k).streams
    ops = []
    for i, k in enumerate(SEQ):
        ops += [["upload", 0, f"{shape}/{k}"], ["run", 0], ["fetch", 0, f"seq{i}"]]
        if tail_twice and i == 1:
            ops += [["run", 0], ["fetch", 0, "again1"]]
    one = {"tag": f"batch/{shape}", "ns": sh.ns, "nb": sh.n // K.BLOCK, "handles": 1, "pipelined": False, "ops": ops}
    ops = [["upload", 0, f"{shape}/0"], ["upload", 1, f"{shape}/1"], ["run", 0], ["run", 1], ["fetch", 0, "p0"],
           ["upload", 0, f"{shape}/2"], ["run", 0], ["fetch", 1, "p1"], ["upload", 1, f"{shape}/0"], ["run", 1],
           ["fetch", 0, "p2"], ["fetch", 1, "p3"], ["run", 0], ["run", 1], ["fetch", 0, "p4"], ["fetch", 1, "p5"]]
    two = {"tag": f"pipe/{shape}", "ns": sh.ns, "nb": sh.n // K.BLOCK, "handles": 2, "pipelined": True, "ops": ops}
    return [one, two]


PIPE_SETS = {"p0": 0, "p1": 1, "p2": 2, "p3": 0, "p4": 2, "p5": 0}


def _check_run(z, tag, shape, k, want_sc, what, one_launch=None, second=None):
    c = K.data(shape, k)
    recs_want, bits_want = K.batch_expected(shape, k)
    info = z[tag + "/info"]
    sc = _reported(c.streams.shape[0], c.n, info[:2])
    assert sc == want_sc, f"{what}: counters() report {sc}, the restated arithmetic gives {want_sc}"
    bits = z[tag + "/bits"]
    for s in range(bits.shape[0]):
        assert np.array_equal(bits[s], bits_want[s]), f"{what} stream {s}: bits differ from the C oracle in {int((bits[s] != bits_want[s]).sum())} bytes"
        got = np.unpackbits(bits[s].view(np.uint8), bitorder="little")[: c.n]
        assert np.array_equal(got, c.bits[s]), f"{what} stream {s}: bits differ from the exact integers"
    TS.assert_records_equal(z[tag + "/recs"], recs_want, what, db_tol=1e-3)
    if one_launch is not None:
        assert bool(info[4]) == one_launch, f"{what}: one_launch_tail {bool(info[4])}"
    if second is not None:
        assert bool(info[5]) == second, f"{what}: second_pass {bool(info[5])}"
    return info


def _check_batch(z, shape, chunk_env, one_launch=True, second=False, tail_twice=False):
    want_sc = K.sched_of(shape, chunk_env)
    for i, k in enumerate(SEQ):
        info = _check_run(z, f"batch/{shape}/seq{i}", shape, k, want_sc, f"{shape} chunk {chunk_env}, run {i} (data set {k})",
                          one_launch and not second, second)
    if tail_twice:   # the overflowed input again: the separate kernels from the start, no second pass
        _check_run(z, f"batch/{shape}/again1", shape, SEQ[1], want_sc, f"{shape} chunk {chunk_env}, run 1 again", False, False)
    for tag, k in PIPE_SETS.items():
        _check_run(z, f"pipe/{shape}/{tag}", shape, k, want_sc, f"{shape} chunk {chunk_env}, pipelined {tag} (data set {k})",
                   None if second else one_launch, None)
    print(f"{shape} chunk {chunk_env}: {len(SEQ)} runs on one handle and {len(PIPE_SETS)} pipelined ones exact; "
          f"{want_sc.chunks} chunks on {want_sc.waves} waves; last counters {info.tolist()}")


# ---------------------------------------------------------------------------------------------------------------------
def test_without_the_hook_the_launch_arithmetic_is_unchanged(tmp_path):
    """No knob set: a small launch through the hook and through BatchDemodulator reports what the restated formula of the
    launch code gives - 4-tile chunks, one wave per chunk rounded up to a workgroup - whatever the number of CUs."""
    assert K.launch(4, 3 * K.BLOCK, n_cu=64, per_cu=1) == K.launch(4, 3 * K.BLOCK, n_cu=256, per_cu=8)
    arrays = {}
    c = K.data("ragged", 2)
    arrays["r"] = c.streams
    arrays["b"] = K.data("short40", 2).streams
    hook = [{"tag": "hook/r", "streams": "r", "hist": "", "want_g": False}]
    ops = [["upload", 0, "b"], ["run", 0], ["fetch", 0, "x"]]
    z = _child(tmp_path, "plain", {}, arrays, hook, [{"tag": "batch/b", "ns": 40, "nb": 1, "handles": 1, "pipelined": False, "ops": ops}])
    want = K.launch(c.streams.shape[0], c.n)
    assert (want.chunk, want.waves) == (4, 48)
    sc = _reported(c.streams.shape[0], c.n, z["hook/r/sched"])
    assert sc == want, (sc, want)
    K.check_outputs(c, sc, z["hook/r/bits"], z["hook/r/fix"], 0, "ragged, no hook")
    want = K.launch(40, K.BLOCK)
    assert (want.chunk, want.waves) == (4, 40)
    _check_run(z, "batch/b/x", "short40", 2, want, "short40, no hook", True, False)


@pytest.mark.parametrize("chunk_env", [4, 5, 8])
def test_work_queues_on_a_capped_grid(tmp_path, chunk_env):
    """RD_TEST_K1_WGS=8: 32 waves, one per queue.  4 tiles per chunk: long3 (99 chunks, two or three per queue), short40
    (every chunk a whole stream), 64 bytes of history, a ragged stream whose last tile lies inside a drawn chunk.  5: chunk
    starts at every ti mod 4, partly filled store groups, a drawn chunk across a stream boundary.  8: a partial last chunk;
    short40 with two streams per chunk (20 chunks: no wave takes a second one, the edge is inchunk > 0 && ti == 0)."""
    shapes = {4: ("long3", "short40", "hist", "ragged"), 5: ("long3",), 8: ("long3", "short40")}[chunk_env]
    arrays, hook, batch = {}, [], []
    for sh in shapes:
        hook += _hook_jobs(sh, arrays)
        if sh in K.BATCH_SHAPES:
            batch += _batch_jobs(sh, arrays)
    z = _child(tmp_path, f"chunk{chunk_env}", {"RD_TEST_K1_WGS": str(K.TEST_WGS), "RD_K1_CHUNK": str(chunk_env)}, arrays, hook, batch)
    for sh in shapes:
        _check_hook(z, sh, chunk_env, must_draw=(sh, chunk_env) != ("short40", 8))
        if sh in K.BATCH_SHAPES:
            _check_batch(z, sh, chunk_env)


@pytest.mark.parametrize("chunk_env", [1, 3])
def test_equal_shares_on_a_capped_grid(tmp_path, chunk_env):
    """chunks of fewer than four tiles: no queue, cur_chunk += nwaves.  RD_K1_CHUNK=3: 54 chunks on 32 waves.  RD_K1_CHUNK=1:
    the launch code raises it to 2 (80 chunks) - with one tile per chunk every wave took its second chunk twice and this
    test found 41 words listed twice (the walk is restated in k1_schedule_cases.simulate)."""
    arrays = {}
    hook, batch = _hook_jobs("short40", arrays), _batch_jobs("short40", arrays)
    z = _child(tmp_path, f"chunk{chunk_env}", {"RD_TEST_K1_WGS": str(K.TEST_WGS), "RD_K1_CHUNK": str(chunk_env)}, arrays, hook, batch)
    _check_hook(z, "short40", chunk_env)
    _check_batch(z, "short40", chunk_env)


def test_real_grid_one_workgroup_per_cu(tmp_path):
    """No cap: RD_K1_WGS_PER_CU=1 and RD_K1_CHUNK=4 on 40 streams x 33 blocks - 1320 chunks against 1024 waves on 256 CUs,
    32 waves per queue, so which wave takes which chunk is up to the device.  Fails (does not skip) on a device where that
    shape gives every chunk a wave of its own."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 33 * K.BLOCK
    want_sc = K.launch(K.REAL_NS, n, n_cu=n_cu, per_cu=1, chunk_env=K.REAL_CHUNK)
    arrays = {f"real/{k}": K.real_grid_input(k) for k in range(K.N_SETS)}
    ops = []
    for i, k in enumerate(SEQ):
        ops += [["upload", 0, f"real/{k}"], ["run", 0], ["fetch", 0, f"seq{i}"]]
    z = _child(tmp_path, "real", {"RD_K1_WGS_PER_CU": "1", "RD_K1_CHUNK": str(K.REAL_CHUNK)}, arrays, (),
               [{"tag": "batch/real", "ns": K.REAL_NS, "nb": 33, "handles": 1, "pipelined": False, "ops": ops}])
    for i, k in enumerate(SEQ):
        tag, what = f"batch/real/seq{i}", f"real_grid run {i} (data set {k})"
        info = z[tag + "/info"]
        sc = _reported(K.REAL_NS, n, info[:2])
        assert sc == want_sc, f"{what}: counters() report {sc}, the restated arithmetic gives {want_sc} on {n_cu} CUs"
        assert sc.chunks > sc.waves, (f"{what}: {K.REAL_NS} streams x 33 blocks are {sc.chunks} chunks of {sc.chunk} tiles for "
                                      f"{sc.waves} waves on {n_cu} CUs: no wave takes a second chunk on this device")
        recs_want, bits_want = K.real_grid_expected(k)
        bits = z[tag + "/bits"]
        for s in range(K.REAL_NS):
            assert np.array_equal(bits[s], bits_want[s]), f"{what} stream {s}: bits differ from the C oracle in {int((bits[s] != bits_want[s]).sum())} bytes"
        TS.assert_records_equal(z[tag + "/recs"], recs_want, what, db_tol=1e-3)
        assert info[4] == 1 and info[5] == 0, (what, info.tolist())
    print(f"real_grid on {n_cu} CUs: {want_sc.chunks} chunks on {want_sc.waves} waves, {len(SEQ)} runs exact, counters {info.tolist()}")


def test_fallbacks_clear_the_queue_words_too(tmp_path):
    """Who clears the other counter set's queue words when k_tail did not finish the job?  A queue word left non-zero makes
    the next run's demod kernel skip the first chunk of that queue; every run here has other data than the one before, so
    the skipped words would hold the wrong bits - PROVIDED the run's bits are still the demod kernel's.  Three children:
    legacy      RD_TAIL_IMPL=legacy: k_fixup re-evaluates the listed groups only and clears the other set.  Seen.
    matchlist   RD_TEST_BUCKET_CAP=4: every long3 data set has a stream with more than 4 preamble matches, so k_tail
                reports overflow bit 1 and the host runs a second search / slice pass through the separate kernels, with NO
                further fix-up: the bits stay what the demod kernel stored and k_tail's list fix-up repaired.  second_pass is
                asserted for every run, and three more data sets follow on the same handle.  Seen: this is the child that
                answers the question for a run that k_tail began and did not finish (k_tail clears the other set at its
                start, before any overflow is known).
    overflow    RD_TEST_FIX_BCAP=16 (+ RD_TEST_MATCH_CAP=7): a fix-up bucket overflows (bit 8) and the host re-evaluates
                EVERY run exactly from the input, so these bits no longer depend on what the demod kernel stored or skipped:
                this child checks the records, bits and forms of that fallback and of the run without an upload behind it
                (the separate kernels from the start), NOT the queue words - a skipped chunk would be repaired silently."""
    base = {"RD_TEST_K1_WGS": str(K.TEST_WGS), "RD_K1_CHUNK": "4"}
    arrays = {}
    batch = _batch_jobs("long3", arrays) + _batch_jobs("short40", arrays)
    z = _child(tmp_path, "legacy", dict(base, RD_TAIL_IMPL="legacy"), arrays, (), batch)
    _check_batch(z, "long3", 4, one_launch=False)
    _check_batch(z, "short40", 4, one_launch=False)
    arrays = {}
    for k in range(K.N_SETS):
        per_stream = np.bincount(K.batch_expected("long3", k)[0]["stream"], minlength=3)
        assert per_stream.max() > MATCHLIST_CAP, "records <= matches: a stream of every data set overflows the short list"
    z = _child(tmp_path, "matchlist", dict(base, RD_TEST_BUCKET_CAP=str(MATCHLIST_CAP)), arrays, (), _batch_jobs("long3", arrays))
    _check_batch(z, "long3", 4, second=True)
    arrays = {}
    batch = _batch_jobs("long3", arrays, tail_twice=True)
    z = _child(tmp_path, "overflow", dict(base, RD_TEST_FIX_BCAP="16", RD_TEST_MATCH_CAP="7"), arrays, (), batch)
    _check_batch(z, "long3", 4, second=True, tail_twice=True)
