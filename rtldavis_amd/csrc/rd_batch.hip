// rd_batch.hip - the batch demodulator of the C ABI (include/rtldavis_hip.h: rd_batch_*).
//
// Host-side orchestration only: buffer management, kernel sequencing, and the per-call ordering/dedupe of
// Demodulator._slice (py:190-205) where the device has not done it.  All arithmetic of the path runs in the kernels of
// rd_tail.hip, rd_tail_kernels.hip, rd_parse_kernels.hip and rd_demod_mfma.hip.  py = /root/reference/src/rtldavis/dsp.py
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "rd_internal.h"
#include "rd_math.h"

// RD_DEBUG_HOST=1: print host-side phase times of rd_batch_results to stderr (diagnostic)
static bool dbg_host() {
    static int v = -1;
    if (v < 0) v = getenv("RD_DEBUG_HOST") ? 1 : 0;
    return v == 1;
}
static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct rd_batch {
    rd_config cfg;
    rd_devcfg dc;
    int n_streams, n_blocks;
    long n_samples;      // per stream
    size_t bits_stride;  // words per stream
    bool dev_ready = false, fast_ok = false, ran = false, timing = false, timing_detail = false;
    bool run_timing = false, run_detail = false;  // the timing mode latched by the run in flight
    int device = -1;      // the device the buffers live on (set by the first device call)
    bool fetched = false;  // batch_finish has seen the last run complete
    uint8_t *d_iq = nullptr;
    size_t iq_bytes = 0;
    uint32_t *d_bits = nullptr, *d_fix = nullptr, *d_cnt = nullptr;
    rd_match *d_matches = nullptr;
    void *d_tasks = nullptr;         // rec_cap entries of RD_TASK_BYTES (two-kernel slice)
    int dense = 0;                   // the last run's records are dense (one per task from index 0)
    rd_order_scratch order;          // host ordering scratch
    rd_packet *d_recs = nullptr;     // rec_cap = 2 * match_cap entries (layout: rd_launch_slice)
    int cnt_set = 0;                 // d_cnt holds two counter sets; a run's fixup kernel clears the other one
    bool parse = false;              // Parser.parse front half on the device (rd_batch_set_parse)
    rd_parsed *d_parsed = nullptr;   // rec_cap entries
    uint32_t fix_cap = 0, match_cap = 0, rec_cap = 0;
    hipStream_t stream = nullptr;
    std::vector<hipEvent_t> evs;  // 5 events per timed run, read back in rd_batch_get_timing
    size_t ev_runs = 0;           // timed runs recorded since the last rd_batch_get_timing
    hipEvent_t *ev = nullptr;     // the current run's five events
    hipEvent_t done = nullptr;    // recorded after the run's readback copies: results wait on it,
                                  // not on the stream, so another batch may already be queued behind
    hipEvent_t kdone = nullptr;   // recorded after the run's last kernel
    hipEvent_t uploaded = nullptr;  // recorded behind an rd_batch_upload_async copy: the next run's kernels wait for it
    bool upload_pending = false;
    hipStream_t copy_stream = nullptr;  // readback runs here, beside the next batch's kernels
    uint32_t h_cnt[RD_CNT_SLOTS] = {};
    uint32_t *h_cnt_pin = nullptr;   // pinned: counters of the run in flight
    rd_packet *h_recs_pin = nullptr; // pinned: records of the run in flight (rec_cap entries)
    uint32_t rec_pin_cap = 0;
    uint32_t spec_recs = 1024;       // records copied back speculatively with the counters
    uint64_t last_fix = 0, last_match = 0;
    rd_timing last_timing = {};
    // dev_order: the run in flight left its records in the reference's order with the per-call duplicates dropped
    // (k_tail), and rd_batch_results only copies them.  tail_off: an input overflowed k_tail's lists - the separate
    // kernels + host ordering until the next upload.
    bool dev_order = false, tail_off = false;
    size_t cnt_stride = RD_CNT_TOTAL;  // words per counter set (k_tail's per-group fix-up counters live behind the counters)
    // The one-launch tail (round 4, rd_launch_tail_fused: k_tail): fix-up, search, slice with order and dedupe, RSSI and
    // the final records in ONE kernel, a workgroup per RD_FT_STREAMS streams; the demod kernel's waves put their fix-up
    // entries into per-group buckets (RD_DEMOD_FIX_BUCKETS) and no k_fixup is launched.  ft_ok: the buffers exist
    // (Davis shape, RD_TAIL_IMPL unset); ft_run: the run in flight used it; its overflows (a stream's match list, a
    // group's fix-up bucket) send this input through the separate kernels (tail_off) and the next upload gets lists
    // twice as long.
    rd_ft_bufs ft;
    bool ft_ok = false, ft_run = false;
    uint32_t ft_seq = 0, ft_limit = 0;   // ft_limit: test hook RD_TEST_BUCKET_CAP (0: none)
    bool ft_sticky = false;              // an input overflowed the longest match lists: uploads no longer re-enable k_tail
    size_t ft_cnt_off = 0;               // the groups' fix-up counters inside a counter set (words)
    // Pipelined completion (rd_batch_set_pipelined): the run's last kernel carries no event; the readback is hung on
    // the stop event of the NEXT demod kernel launched on the same stream (any handle's), see batch_adopt below.
    bool second_pass = false;   // the run in flight needed a second search / slice pass (a list or bucket overflowed)
    uint32_t last_launch[2] = {0, 0};  // tiles per chunk and waves of the last demod launch
    bool pipelined = false;
    bool deferred = false;          // the run in flight has no completion event yet (guarded by g_tail_mx)
    hipEvent_t kfirst = nullptr;    // stop event of this handle's demod launch when it adopts another run untimed
    std::vector<uint8_t> ev_end;    // per timed run: its end-of-run event (ev[4]) was recorded
};

// pipelined completion: launch stream -> the handle whose last run waits there for an adopter (see batch_adopt)
static std::mutex g_tail_mx;
// (keyed by device AND stream: the null stream of one device is not the null stream of another)
typedef std::pair<int, hipStream_t> rd_tail_key;
static std::map<rd_tail_key, rd_batch *> g_tail;

static rd_layout batch_layout(const rd_batch *b) {
    rd_layout l;
    l.iq = b->d_iq;
    l.stream_stride = (size_t)b->n_samples * 2;
    l.n_streams = b->n_streams;
    l.n_samples = (uint32_t)b->n_samples;
    l.hist_mode = 0;
    l.valid_from = 0;
    l.bits = b->d_bits;
    l.bits_stride = b->bits_stride;
    return l;
}

extern "C" int rd_batch_create(const rd_config *cfg, int n_streams, int n_blocks, rd_batch **out) {
    if (!out) return rd_fail_msg(RD_ERR_ARG, "null out");
    rd_devcfg dc;
    int rc = rd_devcfg_checked(cfg, &dc);
    if (rc) return rc;
    if (n_streams < 1 || n_blocks < 1) return rd_fail_msg(RD_ERR_ARG, "n_streams and n_blocks must be >= 1");
    const long n = (long)n_blocks * cfg->block_size;
    const uint64_t runs = (uint64_t)n_streams * ((n + RD_RUN - 1) / RD_RUN);
    if (n > 0x7FFFFFF0L || runs > 0x0FFFFFFFull)
        return rd_fail_msg(RD_ERR_ARG, "batch too large: at most 2^28 32-sample runs (8.6e9 samples) per batch");
    rd_batch *b = new rd_batch();
    b->cfg = *cfg;
    b->dc = dc;
    b->n_streams = n_streams;
    b->n_blocks = n_blocks;
    b->n_samples = n;
    b->bits_stride = (size_t)((n + 31) / 32);
    b->fast_ok = ((size_t)n * 2) % 16 == 0;  // 16-byte aligned streams for the LDS-DMA loads
    *out = b;
    return RD_OK;
}

static uint32_t *batch_cnt(const rd_batch *b) { return b->d_cnt + (size_t)b->cnt_set * b->cnt_stride; }

// The record lists for `match_cap` matches: matches, records (two per match: rd_launch_slice), tasks, and the pinned
// records.  Lists that exist are freed first, every pointer cleared as it is freed: should one of the allocations
// fail, rd_batch_destroy must not free anything twice (and the handle reports the failure on every later call).
// ran = false until the new lists exist: a failed re-allocation leaves a handle that must be run again.
static int batch_alloc_lists(rd_batch *b, uint32_t match_cap) {
    const bool ran = b->ran;
    if (b->match_cap) {
        hipFree(b->d_matches); b->d_matches = nullptr;
        hipFree(b->d_recs); b->d_recs = nullptr;
        hipHostFree(b->h_recs_pin); b->h_recs_pin = nullptr;
        hipFree(b->d_tasks); b->d_tasks = nullptr;
        hipFree(b->d_parsed); b->d_parsed = nullptr;
    }
    b->match_cap = b->rec_cap = b->rec_pin_cap = 0;
    b->ran = false;
    const uint32_t rec_cap = 2 * match_cap;
    HIPCHK(hipMalloc(&b->d_matches, (size_t)match_cap * sizeof(rd_match)));
    HIPCHK(hipMalloc(&b->d_recs, (size_t)rec_cap * sizeof(rd_packet)));
    HIPCHK(hipMalloc(&b->d_tasks, (size_t)rec_cap * RD_TASK_BYTES));
    HIPCHK(hipHostMalloc((void **)&b->h_recs_pin, (size_t)rec_cap * sizeof(rd_packet), hipHostMallocDefault));
    b->match_cap = match_cap;
    b->rec_cap = b->rec_pin_cap = rec_cap;
    b->ran = ran;
    return RD_OK;
}

static int batch_alloc(rd_batch *b) {
    if (b->dev_ready) return rd_use_device(b->device);
    int rc = rd_ensure_device();
    if (rc) return rc;
    HIPCHK(hipGetDevice(&b->device));
    const uint64_t runs = (uint64_t)b->n_streams * b->bits_stride;
    b->iq_bytes = (size_t)b->n_streams * b->n_samples * 2;
    // guard-band list: one entry per flagged 32-sample run (~1.5 % of the runs on noise)
    b->fix_cap = (uint32_t)std::min<uint64_t>(runs, std::max<uint64_t>(4096, runs / 8));
    // ~16 raw matches per 33-block stream on noise + one burst; the lists grow on overflow
    uint32_t match_cap = (uint32_t)std::min<uint64_t>((uint64_t)b->n_streams * (8 + 1ull * b->n_blocks) + 1024, 1u << 26);
    // test hook: a deliberately small first list so that the overflow path (grow, search and slice again) runs on
    // ordinary inputs (tests/test_gpu_parity.py::test_match_list_overflow_is_transparent)
    if (const char *e = getenv("RD_TEST_MATCH_CAP")) {
        const long v = atol(e);
        if (v >= 1 && v < (long)match_cap) match_cap = (uint32_t)v;
    }
    HIPCHK(hipMalloc(&b->d_iq, b->iq_bytes + RD_INPUT_PAD));
    HIPCHK(hipMemset(b->d_iq + b->iq_bytes, 127, RD_INPUT_PAD));
    HIPCHK(hipMalloc(&b->d_bits, runs * sizeof(uint32_t)));
    HIPCHK(hipMalloc(&b->d_fix, (size_t)b->fix_cap * sizeof(uint32_t)));
    {
        // RD_TAIL_IMPL=legacy: the separate kernels (k_fixup, k_search, k_classify + k_rssi_u8) + host ordering instead
        // of the one-launch tail (A/B; also what every shape other than the Davis one takes).  RD_TEST_BUCKET_CAP makes
        // the per-stream match lists short so that the fallback runs on ordinary inputs (test hook)
        const char *ti = getenv("RD_TAIL_IMPL");
        const bool legacy = ti && ti[0] == 'l';
        b->ft_ok = !legacy && b->fast_ok && rd_davis_shape(b->dc) &&
                   b->n_samples < (1l << 30) && b->dc.B < (1 << 24) && b->bits_stride % 4 == 0 && b->dc.L >= b->dc.B &&
                   (long)(b->n_blocks + 1) * b->dc.B - b->dc.L >= 0 &&   // (a batch shorter than a packet has no position to report)
                   ((long)(b->n_blocks + 1) * b->dc.B - b->dc.L) / 32 + 16 <= (long)b->bits_stride;
        if (const char *e = getenv("RD_TEST_BUCKET_CAP")) {
            const long v = atol(e);
            if (v >= 1 && v < RD_BUCKET_MIN) b->ft_limit = (uint32_t)v;
        }
    }
    b->cnt_stride = RD_CNT_TOTAL;
    if (b->ft_ok) {  // the groups' fix-up counters live behind the per-stream match counters: cleared with the set
        const size_t groups = ((size_t)b->n_streams + RD_FT_STREAMS - 1) / RD_FT_STREAMS;
        b->ft_cnt_off = b->cnt_stride;
        b->cnt_stride += (groups + 3) & ~(size_t)3;
        // a group's bucket: the first group of every chunk of tiles (chunks of four tiles at the least) and the first
        // run of each of its streams are always listed; twice that, plus room for the groups inside the guard band
        const uint64_t tps = ((uint64_t)b->n_samples + RD_TILE_SAMPLES - 1) / RD_TILE_SAMPLES;
        b->ft.fix_bcap = (uint32_t)std::min<uint64_t>((2 * RD_FT_STREAMS * (tps / 4 + 8) + 63) & ~63ull, 1u << 20);
        if (const char *e = getenv("RD_TEST_FIX_BCAP")) {  // test hook: small buckets, so that their overflow path runs on ordinary inputs
            const long v = atol(e);
            if (v >= 1 && v < (long)b->ft.fix_bcap) b->ft.fix_bcap = (uint32_t)v;
        }
        b->ft.bcap = rd_ord_bucket_cap(b->n_samples);
        HIPCHK(hipMalloc(&b->ft.fixb, groups * b->ft.fix_bcap * sizeof(uint32_t)));
        HIPCHK(hipMalloc(&b->ft.gstate, 3 * groups * sizeof(uint32_t)));
        HIPCHK(hipMemset(b->ft.gstate, 0, 3 * groups * sizeof(uint32_t)));
    }
    HIPCHK(hipMalloc(&b->d_cnt, 2 * b->cnt_stride * sizeof(uint32_t)));
    HIPCHK(hipMemset(b->d_cnt, 0, 2 * b->cnt_stride * sizeof(uint32_t)));
    if ((rc = batch_alloc_lists(b, match_cap))) return rc;
    HIPCHK(hipHostMalloc((void **)&b->h_cnt_pin, RD_CNT_SLOTS * sizeof(uint32_t), hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(&b->done, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&b->kdone, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&b->kfirst, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&b->uploaded, hipEventDisableTiming));
    HIPCHK(hipStreamCreateWithFlags(&b->copy_stream, hipStreamNonBlocking));
    b->dev_ready = true;
    return RD_OK;
}

extern "C" void rd_batch_destroy(rd_batch *b) {
    if (!b) return;
    {
        std::lock_guard<std::mutex> g(g_tail_mx);  // a run still waiting to be adopted dies with its handle
        auto it = g_tail.find(rd_tail_key(b->device, b->stream));
        if (it != g_tail.end() && it->second == b) g_tail.erase(it);
        b->deferred = false;
    }
    if (b->dev_ready && rd_owns_device_state()) {
        if (b->device >= 0) hipSetDevice(b->device);
        if (b->ran && !b->fetched) hipDeviceSynchronize();  // kernels of a run nobody fetched may still use the buffers
        hipFree(b->d_iq); hipFree(b->d_bits); hipFree(b->d_fix); hipFree(b->d_cnt);
        hipFree(b->d_matches); hipFree(b->d_recs); hipFree(b->d_tasks);
        hipFree(b->d_parsed);
        hipFree(b->ft.fixb); hipFree(b->ft.gstate);
        hipHostFree(b->h_cnt_pin); hipHostFree(b->h_recs_pin);
        if (b->done) hipEventDestroy(b->done);
        if (b->kdone) hipEventDestroy(b->kdone);
        if (b->kfirst) hipEventDestroy(b->kfirst);
        if (b->uploaded) hipEventDestroy(b->uploaded);
        if (b->copy_stream) hipStreamDestroy(b->copy_stream);
        for (auto &e : b->evs) if (e) hipEventDestroy(e);
    }
    delete b;
}

extern "C" int rd_batch_input_ptr(rd_batch *b, void **dev_ptr, size_t *nbytes) {
    if (!b || !dev_ptr) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = batch_alloc(b);
    if (rc) return rc;
    *dev_ptr = b->d_iq;
    if (nbytes) *nbytes = b->iq_bytes;
    return RD_OK;
}

static int batch_flush(rd_batch *b);

extern "C" int rd_batch_upload(rd_batch *b, const uint8_t *iq_host, size_t nbytes) {
    if (!b || !iq_host) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = batch_alloc(b);
    if (rc) return rc;
    if (nbytes != b->iq_bytes) {
        return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: got %zu bytes, expected %zu", nbytes, b->iq_bytes);
    }
    if (b->ran && !b->fetched) {  // a run nobody fetched (e.g. its wait timed out) still reads the input
        rc = batch_flush(b);
        if (rc) return rc;
        rc = rd_wait_event(b->done, "the previous run before an upload");
        if (rc) return rc;
    }
    HIPCHK(hipMemcpy(b->d_iq, iq_host, nbytes, hipMemcpyHostToDevice));
    if (!b->ft_sticky) b->tail_off = false;  // a new input: the one-launch tail gets its chance again
    return RD_OK;
}

// Host-fed batches without the serial upload (SURVEY section 7 "PCIe vs HBM"): the copy goes to `hip_stream` (a copy
// stream of the caller's) and returns at once; the handle's next rd_batch_run waits for it ON THE DEVICE, so the upload
// of one resident batch runs beside the kernels of another.  `iq_host` should be pinned (a pageable buffer makes the
// runtime stage the copy and the call block) and must stay untouched until that run has been launched and the copy
// has completed (rd_batch_results of that run is late enough).  The copy itself waits for the handle's previous run.
extern "C" int rd_batch_upload_async(rd_batch *b, const uint8_t *iq_host, size_t nbytes, void *hip_stream) {
    if (!b || !iq_host) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = batch_alloc(b);
    if (rc) return rc;
    if (nbytes != b->iq_bytes) return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: got %zu bytes, expected %zu", nbytes, b->iq_bytes);
    hipStream_t cs = (hipStream_t)hip_stream;
    if (b->ran && !b->fetched) {  // the previous run still reads the input: the copy queues behind its completion
        rc = batch_flush(b);
        if (rc) return rc;
        HIPCHK(hipStreamWaitEvent(cs, b->done, 0));
    }
    HIPCHK(hipMemcpyAsync(b->d_iq, iq_host, nbytes, hipMemcpyHostToDevice, cs));
    HIPCHK(hipEventRecord(b->uploaded, cs));
    b->upload_pending = true;
    if (!b->ft_sticky) b->tail_off = false;
    return RD_OK;
}

// results come back with the run: counters plus as many records as the last run produced
// (+25 %); rd_batch_results fetches the remainder if this run produced more.
// The copies run on their own stream so that another batch's kernels queued on `st` need
// not wait for them.
static int batch_readback(rd_batch *b, hipEvent_t after) {
    HIPCHK(hipStreamWaitEvent(b->copy_stream, after, 0));
    HIPCHK(hipMemcpyAsync(b->h_cnt_pin, batch_cnt(b), RD_CNT_SLOTS * sizeof(uint32_t), hipMemcpyDeviceToHost,
                          b->copy_stream));
    const uint32_t spec = std::min(b->dev_order ? b->rec_cap : b->match_cap, b->spec_recs);
    if (spec)
        HIPCHK(hipMemcpyAsync(b->h_recs_pin, b->d_recs, (size_t)spec * sizeof(rd_packet), hipMemcpyDeviceToHost,
                              b->copy_stream));
    HIPCHK(hipEventRecord(b->done, b->copy_stream));
    return RD_OK;
}

// Pipelined completion.  An event on a run's last kernel leaves the GPU idle for 6-11 us before the next kernel
// starts (profiles/r02_event_gap.txt); an event on the demod kernel costs nothing measurable (the fix-up kernel
// starts as it ends).  A pipelined handle therefore launches its tail without an event and waits to be ADOPTED: the
// next run launched on the same stream - this handle's or another's - gives its demod kernel a stop event and the
// adopted run's readback waits for that one (kernels of a stream run in order: when the next demod kernel has ended,
// the adopted run's tail has).  The records arrive one demod kernel later; the stream never idles.  If nothing is
// launched behind it, the first call that needs the results records an event on the stream as before.
// g_tail: launch stream -> the handle waiting there; every transition of `deferred` happens under g_tail_mx (the
// adopter may be another thread's handle).

static int batch_flush_locked(rd_batch *p) {  // nobody adopted it: an event of its own
    if (!p->deferred) return RD_OK;
    auto it = g_tail.find(rd_tail_key(p->device, p->stream));
    if (it != g_tail.end() && it->second == p) g_tail.erase(it);
    p->deferred = false;
    int rc = rd_use_device(p->device);
    if (rc) return rc;
    HIPCHK(hipEventRecord(p->kdone, p->stream));
    return batch_readback(p, p->kdone);
}
static int batch_flush(rd_batch *b) {
    std::lock_guard<std::mutex> g(g_tail_mx);
    return batch_flush_locked(b);
}
static bool batch_stream_has_tail(int device, hipStream_t st) {
    std::lock_guard<std::mutex> g(g_tail_mx);
    return g_tail.find(rd_tail_key(device, st)) != g_tail.end();
}
// `carrier`: recorded when a kernel launched on `st` after the waiting run's tail has ended
static int batch_adopt(int device, hipStream_t st, hipEvent_t carrier) {
    std::lock_guard<std::mutex> g(g_tail_mx);
    auto it = g_tail.find(rd_tail_key(device, st));
    if (it == g_tail.end()) return RD_OK;
    rd_batch *p = it->second;
    g_tail.erase(it);
    p->deferred = false;
    return batch_readback(p, carrier);
}

// search + slice part of a run (re-issued on list overflow: then with an event of its own, may_defer = false)
static int batch_search_slice(rd_batch *b, hipStream_t st, bool may_defer = false, uint32_t *zero_next = nullptr) {
    const rd_layout lay = batch_layout(b);
    const long B = b->dc.B, L = b->dc.L;
    const bool last_on_slice = !b->parse;
    const bool defer = may_defer && b->pipelined && last_on_slice && !(b->run_timing && b->run_detail);
    // the run's last kernel carries the end-of-run event itself when nothing follows it
    hipEvent_t last = defer ? nullptr : b->run_timing ? b->ev[4] : b->kdone;
    if (b->run_timing && may_defer) b->ev_end.push_back(defer ? 0 : 1);
    b->dev_order = false;
    if (b->ft_run && may_defer) {  // the run's first pass: everything behind the demod kernel in one launch
        rd_ft_bufs fb = b->ft;
        fb.fixcnt = batch_cnt(b) + b->ft_cnt_off;
        b->ft_seq = b->ft_seq % 4095u + 1u;
        const int ok = rd_launch_tail_fused(lay, b->dc, b->n_blocks, B - L, (long)(b->n_blocks + 1) * B - L, fb,
                                            b->ft_limit ? b->ft_limit : fb.bcap, b->ft_seq, 0, b->d_recs, b->rec_cap, batch_cnt(b), st,
                                            last_on_slice ? last : nullptr, zero_next, (uint32_t)b->cnt_stride);
        if (!ok) return rd_fail_msg(RD_ERR_STATE, "the one-launch tail refused a shape its buffers were allocated for");
        b->dev_order = true;   // (the records are final: order and dedupe happened on the device)
        b->dense = 1;
    }
    if (!b->dev_order) {
        rd_launch_search(b->d_bits, b->bits_stride, b->n_streams, b->n_samples, B - L, (long)(b->n_blocks + 1) * B - L,
                         b->dc, b->d_matches, b->match_cap, batch_cnt(b), st);
        if (b->run_timing && b->run_detail) HIPCHK(hipEventRecord(b->ev[3], st));
        b->dense = rd_launch_slice(lay, b->d_bits, b->bits_stride, b->n_samples, b->dc, b->d_matches, b->match_cap, 1,
                                   b->n_blocks, 0, b->d_recs, nullptr, batch_cnt(b), st, last_on_slice ? last : nullptr,
                                   b->d_tasks);
    }
    if (b->parse) {
        if (!b->d_parsed) HIPCHK(hipMalloc(&b->d_parsed, (size_t)b->rec_cap * sizeof(rd_parsed)));
        rd_launch_parse(lay, b->dc, b->d_recs, b->match_cap, b->d_parsed, batch_cnt(b), st, b->dense);
    }
    if (defer) {  // the readback is enqueued by whoever launches next on this stream (batch_adopt) or by batch_flush
        std::lock_guard<std::mutex> g(g_tail_mx);
        auto it = g_tail.find(rd_tail_key(b->device, st));
        if (it != g_tail.end() && it->second != b) {  // (cannot happen after rd_batch_run's adoption; kept safe)
            int rc = batch_flush_locked(it->second);
            if (rc) return rc;
        }
        g_tail[rd_tail_key(b->device, st)] = b;
        b->deferred = true;
        HIPCHK(hipGetLastError());
        return RD_OK;
    }
    // Every event recorded between two kernels idles the GPU for a few microseconds, so a timed run's end-of-run
    // event doubles as the copy stream's trigger.
    if (!last_on_slice) HIPCHK(hipEventRecord(last, st));
    int rc = batch_readback(b, last);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return RD_OK;
}

extern "C" int rd_batch_run(rd_batch *b, void *hip_stream) {
    if (!b) return rd_fail_msg(RD_ERR_ARG, "null batch");
    int rc = batch_alloc(b);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    const rd_layout lay = batch_layout(b);
    // the previous run's readback of d_cnt / d_recs must be over before they are rewritten: the host
    // has already waited for it if the results were fetched (the normal order), else the stream waits
    if (b->ran && !b->fetched) {
        // (a pipelined run nobody adopted: its readback is not even enqueued yet.  b->stream is still the stream THAT
        // run was launched on - the key of its g_tail entry and where its completion event belongs - and `done`, recorded
        // behind its readback, orders this run's kernels on `st` after it whichever stream that was)
        rc = batch_flush(b);
        if (rc) return rc;
        HIPCHK(hipStreamWaitEvent(st, b->done, 0));
    }
    b->stream = st;
    const bool had_upload = b->upload_pending;
    if (b->upload_pending) {  // rd_batch_upload_async: the input is on its way
        HIPCHK(hipStreamWaitEvent(st, b->uploaded, 0));
        b->upload_pending = false;
    }
    b->fetched = false;
    // counters: this run uses the set the previous run's fixup kernel cleared (both start at zero)
    b->cnt_set ^= 1;
    uint32_t *cnt = batch_cnt(b), *cnt_next = b->d_cnt + (size_t)(b->cnt_set ^ 1) * b->cnt_stride;
    b->run_timing = b->timing;  // set_timing between run() and results() does not touch the run in flight
    b->run_detail = b->timing_detail;
    if (b->timing) {
        if (b->evs.size() < 5 * (b->ev_runs + 1)) {
            const size_t old = b->evs.size();
            b->evs.resize(old + 5, nullptr);
            for (size_t i = old; i < b->evs.size(); i++) HIPCHK(hipEventCreate(&b->evs[i]));
        }
        b->ev = &b->evs[5 * b->ev_runs];
        b->ev_runs++;
    }
    // a pipelined run waiting on this stream is adopted by this run's demod kernel (its stop event)
    const bool adopt = batch_stream_has_tail(b->device, st);
    // the one-launch tail: the fix-up entries go to its workgroups' buckets
    const bool want_ft = b->ft_ok && b->fast_ok && !b->tail_off && !(b->timing && b->timing_detail);
    const uint32_t dflags = want_ft ? RD_DEMOD_FIX_BUCKETS : 0u;
    uint32_t *fixl = want_ft ? b->ft.fixb : b->d_fix, *bcnt = want_ft ? cnt + b->ft_cnt_off : nullptr;
    const uint32_t fixc = want_ft ? b->ft.fix_bcap : b->fix_cap;
    uint32_t honoured = 0;
    // The launch code refused the grid (rd_demod_mfma.hip: fewer waves than work queues, more chunks than waves): nothing
    // ran, so the handle goes back to where it was - the counter set, the pending upload, the timed-run slot - and holds
    // no run: results() reports an error instead of an earlier run's records.  Checked before any adoption: a run waiting
    // on this stream keeps waiting for a launch that really happens (or for its own flush).
    auto refused = [&]() {
        b->cnt_set ^= 1;
        b->upload_pending = had_upload;
        if (b->timing) b->ev_runs--;
        b->ran = false;
        b->fetched = true;
        return rd_fail_msg(RD_ERR_STATE, "the demod kernel's grid has fewer waves than work queues and more chunks than waves: not launched");
    };
    if (b->timing && b->fast_ok) {
        // the demod kernel's dispatch carries its own start / stop events (no marker packets)
        honoured = rd_launch_demod(lay, fixl, fixc, cnt, st, b->ev[0], b->ev[1], dflags, b->last_launch, bcnt);
        if (honoured & RD_DEMOD_REFUSED) return refused();
        if (adopt && (rc = batch_adopt(b->device, st, b->ev[1]))) return rc;
    } else if (b->fast_ok && adopt) {
        honoured = rd_launch_demod(lay, fixl, fixc, cnt, st, nullptr, b->kfirst, dflags, b->last_launch, bcnt);
        if (honoured & RD_DEMOD_REFUSED) return refused();
        if ((rc = batch_adopt(b->device, st, b->kfirst))) return rc;
    } else {
        if (b->timing) HIPCHK(hipEventRecord(b->ev[0], st));   // (timed and no fast kernel: the launch below does not happen)
        if (b->fast_ok) {
            honoured = rd_launch_demod(lay, fixl, fixc, cnt, st, nullptr, nullptr, dflags, b->last_launch, bcnt);
            if (honoured & RD_DEMOD_REFUSED) return refused();
        }
        if (b->timing) HIPCHK(hipEventRecord(b->ev[1], st));
        if (adopt) {  // (an event of THIS run: b->ev is null - or a finished run's - when the handle is untimed)
            hipEvent_t carrier = b->timing ? b->ev[1] : b->kfirst;
            if (!b->timing) HIPCHK(hipEventRecord(carrier, st));
            if ((rc = batch_adopt(b->device, st, carrier))) return rc;
        }
    }
    b->second_pass = false;
    b->ft_run = b->fast_ok && (honoured & RD_DEMOD_FIX_BUCKETS);   // (k_tail does the fix-up and clears the next counter set)
    if (!b->ft_run)   // (fixl / fixc: where this run's demod kernel put its list - the groups' bucket space when an ablated kernel
                      // of the diagnostic library declined the buckets; bounded by fixc either way)
        rd_launch_fixup(lay, fixl, fixc, cnt, b->fast_ok ? 0 : 1, cnt_next, st, (uint32_t)b->cnt_stride, b->last_fix);
    if (b->timing && b->timing_detail) HIPCHK(hipEventRecord(b->ev[2], st));
    rc = batch_search_slice(b, st, true, b->ft_run ? cnt_next : nullptr);
    if (rc) return rc;
    b->ran = true;
    return RD_OK;
}

// a second search / slice pass of the run in flight, with an event of its own, over cleared lists
static int batch_second_pass(rd_batch *b, hipStream_t st) {
    const uint32_t zero[5] = {0, 0, 0, 0, 0};  // matches, boundary records, tasks, parsed, overflow flags
    HIPCHK(hipMemcpyAsync(batch_cnt(b) + RD_CNT_MATCH, zero, sizeof zero, hipMemcpyHostToDevice, st));
    b->second_pass = true;
    return batch_search_slice(b, st);
}

// Synchronise, handle list overflows (re-running what is needed), fetch the counters.
static int batch_finish(rd_batch *b) {
    if (!b->ran) return rd_fail_msg(RD_ERR_STATE, "rd_batch_run has not been called");
    hipStream_t st = b->stream;
    {
        int frc = batch_flush(b);  // pipelined and not adopted: nothing was launched behind this run
        if (frc) return frc;
    }
    for (int attempt = 0; attempt < 8; attempt++) {
        const double ta = now_ms();
        int wrc = rd_wait_event(b->done, "the batch run's results");
        if (wrc) return wrc;
        memcpy(b->h_cnt, b->h_cnt_pin, sizeof b->h_cnt);
        if (dbg_host()) fprintf(stderr, "[rd] finish: wait %.3f ms\n", now_ms() - ta);
        bool redo_search = false;
        if (b->ft_run && !b->second_pass && (b->h_cnt[RD_CNT_OVF] & (8u | 16u))) {
            // a group's fix-up bucket overflowed (quiet or degenerate input), or a workgroup gave up waiting for the
            // groups in front of it: every run is re-evaluated exactly, then the separate kernels
            const rd_layout lay = batch_layout(b);
            rd_launch_fixup(lay, b->d_fix, b->fix_cap, batch_cnt(b), 1, nullptr, st);
            b->last_fix = (uint64_t)b->n_streams * b->bits_stride;
            b->tail_off = true;
            b->h_cnt[RD_CNT_OVF] = 0;
            b->h_cnt[RD_CNT_FIX] = 0;
            redo_search = true;
        } else if (b->ft_run && !b->second_pass && (b->h_cnt[RD_CNT_OVF] & 1u)) {
            // a stream with more matches than its list in LDS holds: this input takes the separate kernels, the next
            // upload gets lists twice as long
            if (!b->ft_limit && b->ft.bcap < RD_BUCKET_MAX) b->ft.bcap = std::min<uint32_t>(2 * b->ft.bcap, RD_BUCKET_MAX);
            else if (!b->ft_limit) b->ft_sticky = true;  // (the longest lists there are: inputs like this one keep the separate kernels)
        }
        if (redo_search) {
        } else if (b->fast_ok && !b->ft_run && b->h_cnt[RD_CNT_FIX] > b->fix_cap) {
            // guard list overflowed (degenerate input): re-evaluate every run exactly
            const rd_layout lay = batch_layout(b);
            rd_launch_fixup(lay, b->d_fix, b->fix_cap, batch_cnt(b), 1, nullptr, st);
            // mark handled: this branch must not see the count again
            uint32_t cap = b->fix_cap;
            HIPCHK(hipMemcpyAsync(batch_cnt(b) + RD_CNT_FIX, &cap, sizeof cap, hipMemcpyHostToDevice, st));
            b->last_fix = (uint64_t)b->n_streams * b->bits_stride;
            redo_search = true;
        } else if (attempt == 0) {
            b->last_fix = (uint64_t)b->h_cnt[RD_CNT_FIX];
        }
        if (redo_search && b->tail_off) b->dev_order = false;  // (the bucket-overflow branch above: not the record-overflow one below)
        if (b->dev_order && b->h_cnt[RD_CNT_OVF]) {
            // a stream with more matches than its list holds (or more records than the output array): this input goes
            // through the separate kernels and the host-side ordering, now and until the next upload
            b->tail_off = true;
            if (dbg_host())
                fprintf(stderr, "[rd] one-launch tail overflow: flags %u (1 a stream's match list, 2 records), matches %u\n",
                        b->h_cnt[RD_CNT_OVF], b->h_cnt[RD_CNT_MATCH]);
            int rc2 = batch_second_pass(b, st);
            if (rc2) return rc2;
            continue;
        }
        if (!b->dev_order && b->h_cnt[RD_CNT_MATCH] > b->match_cap) {
            int rc2 = batch_alloc_lists(b, b->h_cnt[RD_CNT_MATCH] + b->h_cnt[RD_CNT_MATCH] / 4 + 1024);   // longer lists
            if (rc2) return rc2;
            redo_search = true;
        }
        if (!redo_search) {
            b->last_match = b->h_cnt[RD_CNT_MATCH];
            b->fetched = true;
            return RD_OK;
        }
        int rc2 = batch_second_pass(b, st);
        if (rc2) return rc2;
    }
    return rd_fail_msg(RD_ERR_DEVICE, "result lists kept overflowing");
}

extern "C" int rd_batch_results(rd_batch *b, rd_packet *out, int cap, int *n) {
    if (!b || !n) return rd_fail_msg(RD_ERR_ARG, "null argument");
    const double t0 = now_ms();
    int rc = batch_finish(b);
    if (rc) return rc;
    const double t1 = now_ms();
    // one record per match, plus the second records of block-boundary positions (kept apart on
    // the device, appended here)
    // sparse layout: one slot per match + the block-boundary twins behind match_cap; dense: one record per task
    const uint32_t nprim = b->dense ? std::min(b->h_cnt[RD_CNT_TASKS], b->rec_cap) : std::min(b->h_cnt[RD_CNT_MATCH], b->match_cap);
    const uint32_t nextra = b->dense ? 0u : std::min(b->h_cnt[RD_CNT_REC], b->match_cap);
    const uint32_t have = std::min(b->dev_order ? b->rec_cap : b->match_cap, b->spec_recs);
    // Late copies go to the copy stream: it has already waited for this run's last kernel, whereas the
    // launch stream may hold the NEXT batch's run by now (two resident batches alternate in bench.py) and a
    // copy queued there would wait for it.
    if (nprim > have) {  // more records than were copied back with the run: fetch the rest
        rc = rd_copy_d2h(b->h_recs_pin + have, b->d_recs + have, (size_t)(nprim - have) * sizeof(rd_packet), b->copy_stream);
        if (rc) return rc;
    }
    if (nextra) {  // second records of block-boundary positions (q == B in one call, q == 0 in the next)
        rc = rd_copy_d2h(b->h_recs_pin + nprim, b->d_recs + b->match_cap, (size_t)nextra * sizeof(rd_packet), b->copy_stream);
        if (rc) return rc;
    }
    const uint32_t nrec = nprim + nextra;
    b->spec_recs = std::max<uint32_t>(1024, nprim + nprim / 4);
    const double t2 = now_ms();
    // the device wrote them in the reference's order, duplicates dropped (copy, nothing else) - or the host orders them
    if (!b->dev_order) rd_order_and_dedupe(b->h_recs_pin, nrec, b->dc.S, b->order);
    const size_t count = b->dev_order ? nrec : b->order.kept.size();
    *n = (int)count;
    if ((int)count > cap) return rd_fail_msg(RD_ERR_CAPACITY, "need room for %zu packets", count);
    if (count && !out) return rd_fail_msg(RD_ERR_ARG, "null out");
    if (b->dev_order && count) memcpy(out, b->h_recs_pin, count * sizeof(rd_packet));
    if (!b->dev_order)
        for (size_t i = 0; i < count; i++) out[i] = b->h_recs_pin[b->order.kept[i]];  // straight into the caller's array
    if (dbg_host())
        fprintf(stderr, "[rd] results%s: finish %.3f ms, D2H %u recs %.3f ms, %s %.3f ms\n", b->dev_order ? " (k_tail)" : "", t1 - t0,
                nrec, t2 - t1, b->dev_order ? "copy" : "order+dedupe+copy", now_ms() - t2);
    return RD_OK;
}

extern "C" int rd_batch_copy_bits(rd_batch *b, int stream, uint8_t *out, size_t nbytes) {
    if (!b || !out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (stream < 0 || stream >= b->n_streams) return rd_fail_msg(RD_ERR_ARG, "stream out of range");
    const size_t need = (size_t)((b->n_samples + 7) / 8);
    if (nbytes < need) return rd_fail_msg(RD_ERR_ARG, "bit buffer too small: %zu < %zu", nbytes, need);
    int rc = batch_finish(b);
    if (rc) return rc;
    return rd_copy_d2h(out, (const uint8_t *)(b->d_bits + (size_t)stream * b->bits_stride), need, b->stream);
}

extern "C" int rd_batch_copy_discriminated(rd_batch *b, int stream, size_t t0, double *out, size_t n) {
    if (!b || !out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (stream < 0 || stream >= b->n_streams || t0 + n > (size_t)b->n_samples)
        return rd_fail_msg(RD_ERR_ARG, "range out of bounds");
    int rc = batch_alloc(b);
    if (rc) return rc;
    if (n == 0) return RD_OK;
    double *d = nullptr;
    HIPCHK(hipMalloc(&d, n * sizeof(double)));
    rd_launch_disc(batch_layout(b), stream, (long)t0, (long)n, d, b->stream);
    rc = rd_copy_d2h(out, d, n * sizeof(double), b->stream);
    hipFree(d);
    return rc;
}

extern "C" int rd_batch_set_parse(rd_batch *b, int enabled) {
    if (!b) return rd_fail_msg(RD_ERR_ARG, "null batch");
    b->parse = enabled != 0;
    return RD_OK;
}

extern "C" int rd_batch_parsed(rd_batch *b, rd_parsed *out, int cap, int *n) {
    if (!b || !n) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (!b->parse) return rd_fail_msg(RD_ERR_STATE, "rd_batch_set_parse(b, 1) must precede rd_batch_run");
    int rc = batch_finish(b);
    if (rc) return rc;
    const uint32_t np = std::min(b->h_cnt[RD_CNT_PARSED], b->rec_cap);
    std::vector<rd_parsed> recs(np);
    if (np) {
        rc = rd_copy_d2h(recs.data(), b->d_parsed, (size_t)np * sizeof(rd_parsed), b->stream);
        if (rc) return rc;
    }
    const size_t kept = rd_order_parsed(recs.data(), recs.size(), b->dc.S);
    *n = (int)kept;
    if ((int)kept > cap) return rd_fail_msg(RD_ERR_CAPACITY, "need room for %zu messages", kept);
    if (kept) {
        if (!out) return rd_fail_msg(RD_ERR_ARG, "null out");
        memcpy(out, recs.data(), kept * sizeof(rd_parsed));
    }
    return RD_OK;
}

// 1: pipelined completion (see batch_adopt): for callers that keep several runs queued on one stream and want the
// stream never to idle; a run's results then become available one demod kernel later.  0 (default): every run ends
// with an event of its own.
extern "C" int rd_batch_set_pipelined(rd_batch *b, int enabled) {
    if (!b) return rd_fail_msg(RD_ERR_ARG, "null batch");
    b->pipelined = enabled != 0;
    return RD_OK;
}

extern "C" int rd_batch_set_timing(rd_batch *b, int enabled) {
    if (!b) return rd_fail_msg(RD_ERR_ARG, "null batch");
    b->timing = enabled != 0;
    b->timing_detail = enabled >= 2;  // 1: demod kernel and total only (3 events per run); 2: every stage
    b->ev_runs = 0;
    b->ev_end.clear();
    // events for the first 64 timed runs exist before the first of them is launched (creating them one run at a
    // time showed as a stall of several milliseconds inside a 60 ms timed region)
    if (b->timing && b->dev_ready && rd_use_device(b->device) == RD_OK) {
        const size_t want = 5 * 64;
        const size_t old = b->evs.size();
        if (old < want) {
            b->evs.resize(want, nullptr);
            for (size_t i = old; i < want; i++) HIPCHK(hipEventCreate(&b->evs[i]));
        }
    }
    return RD_OK;
}

extern "C" int rd_batch_get_timing(rd_batch *b, rd_timing *out) {
    if (!b || !out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (!b->timing) return rd_fail_msg(RD_ERR_STATE, "timing not enabled");
    int rc = batch_finish(b);
    if (rc) return rc;
    // mean over the runs recorded since the last call (events are only read here, after the
    // timed region: hipEventElapsedTime costs milliseconds on ROCm 7.2)
    rd_timing t = {};
    size_t n_end = 0;
    for (size_t r = 0; r < b->ev_runs; r++) {
        hipEvent_t *e = &b->evs[5 * r];
        float v[5] = {0, 0, 0, 0, 0};
        HIPCHK(hipEventElapsedTime(&v[0], e[0], e[1]));
        if (b->timing_detail) {
            HIPCHK(hipEventElapsedTime(&v[1], e[1], e[2]));
            HIPCHK(hipEventElapsedTime(&v[2], e[2], e[3]));
            HIPCHK(hipEventElapsedTime(&v[3], e[3], e[4]));
        }
        // (a pipelined run has no end-of-run event: total_ms is the mean over the runs that have one, 0 if none)
        const bool has_end = r >= b->ev_end.size() || b->ev_end[r];
        if (has_end) { HIPCHK(hipEventElapsedTime(&v[4], e[0], e[4])); n_end++; }
        t.demod_ms += v[0]; t.fixup_ms += v[1]; t.search_ms += v[2]; t.slice_ms += v[3]; t.total_ms += v[4];
    }
    if (b->ev_runs) {
        const float k = 1.0f / (float)b->ev_runs;
        t.demod_ms *= k; t.fixup_ms *= k; t.search_ms *= k; t.slice_ms *= k;
        t.total_ms = n_end ? t.total_ms / (float)n_end : 0.0f;
    }
    t.runs = (int32_t)b->ev_runs;
    b->ev_runs = 0;
    b->ev_end.clear();
    b->last_timing = t;
    *out = t;
    return RD_OK;
}

// Which forms the last run took (after it has completed): RD_FORM_* bits.
extern "C" int rd_batch_last_run_forms(rd_batch *b, uint32_t *forms) {
    if (!b || !forms) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = batch_finish(b);
    if (rc) return rc;
    *forms = (b->dev_order ? RD_FORM_ORDERED_TAIL | RD_FORM_ONE_LAUNCH_TAIL : 0u) | (b->second_pass ? RD_FORM_SECOND_PASS : 0u);
    return RD_OK;
}

extern "C" int rd_k1_schedule(rd_batch *b, uint32_t *tiles_per_chunk, uint32_t *waves) {
    uint32_t v[2] = {0, 0};
    if (b) {
        if (!b->ran) return rd_fail_msg(RD_ERR_STATE, "rd_batch_run has not been called");
        v[0] = b->last_launch[0]; v[1] = b->last_launch[1];
    } else {
        rd_debug_last_launch(v);
    }
    if (tiles_per_chunk) *tiles_per_chunk = v[0];
    if (waves) *waves = v[1];
    return RD_OK;
}

extern "C" int rd_batch_get_counters(rd_batch *b, uint64_t *fixup_runs, uint64_t *matches) {
    if (!b) return rd_fail_msg(RD_ERR_ARG, "null batch");
    int rc = batch_finish(b);
    if (rc) return rc;
    if (fixup_runs) *fixup_runs = b->last_fix;
    if (matches) *matches = b->last_match;
    return RD_OK;
}
