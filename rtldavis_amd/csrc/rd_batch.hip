// rd_batch.hip - the batch demodulator of the C ABI (include/rtldavis_hip.h: rd_batch_*).
//
// Host-side orchestration only: buffer management, kernel sequencing, and the per-call ordering/dedupe of
// Demodulator._slice (py:190-205) where the device has not done it.  All arithmetic of the path runs in the kernels of
// rd_tail.hip, rd_tail_kernels.hip, rd_parse_kernels.hip and rd_demod_mfma.hip.  py = /root/reference/src/rtldavis/dsp.py
// What is decided here without the device - a handle's sizes, the launch plan of a run, the overflow ladder, what results()
// copies - is decided in rd_batch_plan.cpp (pure host code, CPU-tested); this file carries it out.
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

static_assert(RD_BATCH_RUN == RD_RUN, "rd_batch_plan.h sizes the bit arrays by the kernels' run length");

// RD_DEBUG_HOST=1: print host-side phase times of rd_batch_results to stderr (diagnostic)
static bool dbg_host() {
    static int v = -1;
    if (v < 0) v = getenv("RD_DEBUG_HOST") ? 1 : 0;
    return v == 1;
}
static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The handle's state, grouped by lifetime.  Shape and sizes (dc, n_streams, n_blocks, sz) are constant after create, the
// sizes that depend on the hooks after the first device call; the caller's switches change between runs only.
struct rd_batch_bufs {  // device memory, pinned memory, streams and the long-lived events: batch_alloc makes them, batch_free frees them
    int device = -1;    // the device the buffers live on (set by the first device call)
    uint8_t *d_iq = nullptr;
    uint32_t *d_bits = nullptr, *d_fix = nullptr;
    uint32_t *d_cnt = nullptr;       // two counter sets; a run's fixup kernel (or k_tail) clears the other one
    uint32_t *fixb = nullptr, *gstate = nullptr;  // k_tail's fix-up buckets and group states (rd_ft_bufs), with sz.ft_ok
    // the record lists (batch_alloc_lists): they grow when an input overflows them
    uint32_t match_cap = 0, rec_cap = 0;
    rd_match *d_matches = nullptr;
    rd_packet *d_recs = nullptr;     // rec_cap = 2 * match_cap entries (layout: rd_launch_slice)
    void *d_tasks = nullptr;         // rec_cap entries of RD_TASK_BYTES (two-kernel slice)
    rd_parsed *d_parsed = nullptr;   // rec_cap entries, from the first run with parse on
    uint32_t *h_cnt_pin = nullptr;   // pinned: counters of the run in flight
    rd_packet *h_recs_pin = nullptr; // pinned: records of the run in flight (rec_cap entries)
    hipStream_t copy_stream = nullptr;  // readback runs here, beside the next batch's kernels
    hipEvent_t done = nullptr;     // recorded after the run's readback copies: results wait on it,
                                   // not on the stream, so another batch may already be queued behind
    hipEvent_t kdone = nullptr;    // recorded after the run's last kernel
    hipEvent_t kfirst = nullptr;   // stop event of this handle's demod launch when it adopts another run untimed
    hipEvent_t uploaded = nullptr; // recorded behind an rd_batch_upload_async copy: the next run's kernels wait for it
};
struct rd_batch_run_state {  // the run in flight (or the last one)
    bool ran = false;        // there is one; false again while its lists are being re-allocated
    bool fetched = false;    // batch_finish has seen it complete
    bool upload_pending = false;  // an rd_batch_upload_async copy the next run has to wait for
    hipStream_t stream = nullptr;
    int cnt_set = 0;         // which of d_cnt's two counter sets it counts in
    bool timing = false, detail = false;  // the timing mode it latched: set_timing between run() and results() does not touch it
    hipEvent_t *ev = nullptr;             // its five events when timed
    rd_run_plan plan;
    bool ft_run = false;      // it used the one-launch tail (k_tail did the fix-up and cleared the next counter set)
    bool dev_order = false;   // k_tail left its records in the reference's order with the per-call duplicates dropped:
                              // rd_batch_results only copies them
    int dense = 0;            // its records are dense (one per task from index 0)
    bool second_pass = false; // it needed a second search / slice pass (a list or bucket overflowed)
    bool deferred = false;    // pipelined completion: it has no completion event yet (guarded by g_tail_mx)
    uint32_t ft_seq = 0;      // k_tail's launch number on gstate
    uint32_t last_launch[2] = {0, 0};  // tiles per chunk and waves of the demod launch
    uint32_t have = 0;        // records copied back speculatively with the counters (batch_readback)
    uint32_t h_cnt[RD_CNT_SLOTS] = {};
};
struct rd_batch_timer {           // rd_batch_set_timing / rd_batch_get_timing
    std::vector<hipEvent_t> evs;  // 5 events per timed run
    size_t ev_runs = 0;           // timed runs recorded since the last rd_batch_get_timing
    std::vector<uint8_t> ev_end;  // per timed run: its end-of-run event (ev[4]) was recorded
};
struct rd_batch {
    rd_devcfg dc;
    int n_streams, n_blocks;
    rd_batch_sizes sz;       // from create: n_samples, bits_stride, fast_ok; the rest with the hooks, at the first device call
    bool dev_ready = false;
    // the caller's switches: timing 1 / 2, Parser.parse's front half on the device, pipelined completion (see batch_adopt)
    bool timing = false, timing_detail = false, parse = false, pipelined = false;
    rd_batch_bufs m;
    rd_batch_run_state run;
    rd_batch_learned learned;  // what inputs have taught the handle (rd_batch_plan.h)
    rd_batch_timer timer;
    rd_order_scratch order;    // host ordering scratch
};

static rd_layout batch_layout(const rd_batch *b) {
    rd_layout l;
    l.iq = b->m.d_iq;
    l.stream_stride = (size_t)b->sz.n_samples * 2;
    l.n_streams = b->n_streams;
    l.n_samples = (uint32_t)b->sz.n_samples;
    l.hist_mode = 0;
    l.valid_from = 0;
    l.bits = b->m.d_bits;
    l.bits_stride = b->sz.bits_stride;
    return l;
}

extern "C" int rd_batch_create(const rd_config *cfg, int n_streams, int n_blocks, rd_batch **out) {
    if (!out) return rd_fail_msg(RD_ERR_ARG, "null out");
    rd_devcfg dc;
    int rc = rd_devcfg_checked(cfg, &dc);
    if (rc) return rc;
    const char *why = "";
    if ((rc = rd_batch_check_size(n_streams, n_blocks, cfg->block_size, &why))) return rd_fail_msg(rc, "%s", why);
    rd_batch *b = new rd_batch();
    b->dc = dc;
    b->n_streams = n_streams;
    b->n_blocks = n_blocks;
    b->sz = rd_batch_sizes_of(n_streams, n_blocks, dc, rd_batch_hooks());
    *out = b;
    return RD_OK;
}

static uint32_t *batch_cnt(const rd_batch *b) { return b->m.d_cnt + (size_t)b->run.cnt_set * b->sz.cnt_stride; }

// The record lists for `match_cap` matches: matches, records (two per match: rd_launch_slice), tasks, and the pinned
// records.  Lists that exist are freed first, every pointer cleared as it is freed: should one of the allocations
// fail, rd_batch_destroy must not free anything twice (and the handle reports the failure on every later call).
// ran = false until the new lists exist: a failed re-allocation leaves a handle that must be run again.
static int batch_alloc_lists(rd_batch *b, uint32_t match_cap) {
    rd_batch_bufs &m = b->m;
    const bool ran = b->run.ran;
    if (m.match_cap) {
        hipFree(m.d_matches); m.d_matches = nullptr;
        hipFree(m.d_recs); m.d_recs = nullptr;
        hipHostFree(m.h_recs_pin); m.h_recs_pin = nullptr;
        hipFree(m.d_tasks); m.d_tasks = nullptr;
        hipFree(m.d_parsed); m.d_parsed = nullptr;
    }
    m.match_cap = m.rec_cap = 0;
    b->run.ran = false;
    const uint32_t rec_cap = 2 * match_cap;
    HIPCHK(hipMalloc(&m.d_matches, (size_t)match_cap * sizeof(rd_match)));
    HIPCHK(hipMalloc(&m.d_recs, (size_t)rec_cap * sizeof(rd_packet)));
    HIPCHK(hipMalloc(&m.d_tasks, (size_t)rec_cap * RD_TASK_BYTES));
    HIPCHK(hipHostMalloc((void **)&m.h_recs_pin, (size_t)rec_cap * sizeof(rd_packet), hipHostMallocDefault));
    m.match_cap = match_cap;
    m.rec_cap = rec_cap;
    b->run.ran = ran;
    return RD_OK;
}

// The handle's first device call: the hooks are read (tests set them per handle), the sizes follow (rd_batch_sizes_of)
// and everything is allocated by them.
static int batch_alloc(rd_batch *b) {
    rd_batch_bufs &m = b->m;
    if (b->dev_ready) return rd_use_device(m.device);
    int rc = rd_ensure_device();
    if (rc) return rc;
    HIPCHK(hipGetDevice(&m.device));
    const rd_batch_sizes z = b->sz = rd_batch_sizes_of(b->n_streams, b->n_blocks, b->dc, rd_batch_hooks_env());
    b->learned.bcap = z.bcap;
    HIPCHK(hipMalloc(&m.d_iq, z.iq_bytes + RD_INPUT_PAD));
    HIPCHK(hipMemset(m.d_iq + z.iq_bytes, 127, RD_INPUT_PAD));
    HIPCHK(hipMalloc(&m.d_bits, (uint64_t)b->n_streams * z.bits_stride * sizeof(uint32_t)));
    HIPCHK(hipMalloc(&m.d_fix, (size_t)z.fix_cap * sizeof(uint32_t)));
    if (z.ft_ok) {
        HIPCHK(hipMalloc(&m.fixb, z.groups * z.fix_bcap * sizeof(uint32_t)));
        HIPCHK(hipMalloc(&m.gstate, 3 * z.groups * sizeof(uint32_t)));
        HIPCHK(hipMemset(m.gstate, 0, 3 * z.groups * sizeof(uint32_t)));
    }
    HIPCHK(hipMalloc(&m.d_cnt, 2 * z.cnt_stride * sizeof(uint32_t)));
    HIPCHK(hipMemset(m.d_cnt, 0, 2 * z.cnt_stride * sizeof(uint32_t)));
    if ((rc = batch_alloc_lists(b, z.match_cap))) return rc;
    HIPCHK(hipHostMalloc((void **)&m.h_cnt_pin, RD_CNT_SLOTS * sizeof(uint32_t), hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(&m.done, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&m.kdone, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&m.kfirst, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&m.uploaded, hipEventDisableTiming));
    HIPCHK(hipStreamCreateWithFlags(&m.copy_stream, hipStreamNonBlocking));
    b->dev_ready = true;
    return RD_OK;
}

static void batch_free(rd_batch_bufs &m) {
    hipFree(m.d_iq); hipFree(m.d_bits); hipFree(m.d_fix); hipFree(m.d_cnt);
    hipFree(m.d_matches); hipFree(m.d_recs); hipFree(m.d_tasks);
    hipFree(m.d_parsed);
    hipFree(m.fixb); hipFree(m.gstate);
    hipHostFree(m.h_cnt_pin); hipHostFree(m.h_recs_pin);
    if (m.done) hipEventDestroy(m.done);
    if (m.kdone) hipEventDestroy(m.kdone);
    if (m.kfirst) hipEventDestroy(m.kfirst);
    if (m.uploaded) hipEventDestroy(m.uploaded);
    if (m.copy_stream) hipStreamDestroy(m.copy_stream);
}

// the timer's pool holds at least n events
static int timer_reserve(rd_batch_timer &t, size_t n) {
    const size_t old = t.evs.size();
    if (old >= n) return RD_OK;
    t.evs.resize(n, nullptr);
    for (size_t i = old; i < n; i++) HIPCHK(hipEventCreate(&t.evs[i]));
    return RD_OK;
}

// results come back with the run: counters plus as many records as the last run produced
// (+25 %); rd_batch_results fetches the remainder if this run produced more.
// The copies run on their own stream so that another batch's kernels queued on `st` need
// not wait for them.
static int batch_readback(rd_batch *b, hipEvent_t after) {
    rd_batch_bufs &m = b->m;
    HIPCHK(hipStreamWaitEvent(m.copy_stream, after, 0));
    HIPCHK(hipMemcpyAsync(m.h_cnt_pin, batch_cnt(b), RD_CNT_SLOTS * sizeof(uint32_t), hipMemcpyDeviceToHost, m.copy_stream));
    b->run.have = rd_batch_spec_count(b->run.dev_order, m.match_cap, m.rec_cap, b->learned.spec_recs);
    if (b->run.have)
        HIPCHK(hipMemcpyAsync(m.h_recs_pin, m.d_recs, (size_t)b->run.have * sizeof(rd_packet), hipMemcpyDeviceToHost, m.copy_stream));
    HIPCHK(hipEventRecord(m.done, m.copy_stream));
    return RD_OK;
}

// Pipelined completion.  An event on a run's last kernel leaves the GPU idle for 6-11 us before the next kernel
// starts (profiles/r02_event_gap.txt); an event on the demod kernel costs nothing measurable (the fix-up kernel
// starts as it ends).  A pipelined handle therefore launches its tail without an event and waits to be ADOPTED: the
// next run launched on the same stream - this handle's or another's - gives its demod kernel a stop event and the
// adopted run's readback waits for that one (kernels of a stream run in order: when the next demod kernel has ended,
// the adopted run's tail has).  The records arrive one demod kernel later; the stream never idles.  If nothing is
// launched behind it, the first call that needs the results records an event on the stream as before.
// g_tail: launch stream -> the handle whose run is parked there; every transition of `deferred` happens under g_tail_mx
// (the adopter may be another thread's handle), in one of tail_park / tail_take / tail_drop.
static std::mutex g_tail_mx;
// (keyed by device AND stream: the null stream of one device is not the null stream of another)
typedef std::pair<int, hipStream_t> rd_tail_key;
static std::map<rd_tail_key, rd_batch *> g_tail;

static void tail_park(rd_batch *b) {  // (g_tail_mx held)
    g_tail[rd_tail_key(b->m.device, b->run.stream)] = b;
    b->run.deferred = true;
}
static rd_batch *tail_take(int device, hipStream_t st) {  // (g_tail_mx held) the handle parked there, or null
    auto it = g_tail.find(rd_tail_key(device, st));
    if (it == g_tail.end()) return nullptr;
    rd_batch *p = it->second;
    g_tail.erase(it);
    p->run.deferred = false;
    return p;
}
static void tail_drop(rd_batch *p) {  // (g_tail_mx held) p's run is parked no longer, wherever it was
    auto it = g_tail.find(rd_tail_key(p->m.device, p->run.stream));
    if (it != g_tail.end() && it->second == p) g_tail.erase(it);
    p->run.deferred = false;
}

static int batch_flush_locked(rd_batch *p) {  // nobody adopted it: an event of its own
    if (!p->run.deferred) return RD_OK;
    tail_drop(p);
    int rc = rd_use_device(p->m.device);
    if (rc) return rc;
    HIPCHK(hipEventRecord(p->m.kdone, p->run.stream));
    return batch_readback(p, p->m.kdone);
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
    rd_batch *p = tail_take(device, st);
    return p ? batch_readback(p, carrier) : RD_OK;
}

// A run nobody fetched (e.g. its wait timed out) still uses the buffers - it reads the input, its readback reads d_cnt and
// d_recs: it is flushed (a pipelined run nobody adopted has its readback not even enqueued yet) and then whoever is about
// to overwrite them waits for `done`, recorded behind its readback: stream *st, or the host (st null; `what` names the wait).
static int batch_settle(rd_batch *b, const hipStream_t *st, const char *what = nullptr) {
    if (!b->run.ran || b->run.fetched) return RD_OK;
    int rc = batch_flush(b);
    if (rc) return rc;
    if (!st) return rd_wait_event(b->m.done, what);
    HIPCHK(hipStreamWaitEvent(*st, b->m.done, 0));
    return RD_OK;
}

extern "C" void rd_batch_destroy(rd_batch *b) {
    if (!b) return;
    {
        std::lock_guard<std::mutex> g(g_tail_mx);  // a run still waiting to be adopted dies with its handle
        tail_drop(b);
    }
    if (b->dev_ready && rd_owns_device_state()) {
        if (b->m.device >= 0) hipSetDevice(b->m.device);
        if (b->run.ran && !b->run.fetched) hipDeviceSynchronize();  // kernels of a run nobody fetched may still use the buffers
        batch_free(b->m);
        for (auto &e : b->timer.evs) if (e) hipEventDestroy(e);
    }
    delete b;
}

extern "C" int rd_batch_input_ptr(rd_batch *b, void **dev_ptr, size_t *nbytes) {
    if (!b || !dev_ptr) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = batch_alloc(b);
    if (rc) return rc;
    *dev_ptr = b->m.d_iq;
    if (nbytes) *nbytes = b->sz.iq_bytes;
    return RD_OK;
}

extern "C" int rd_batch_upload(rd_batch *b, const uint8_t *iq_host, size_t nbytes) {
    if (!b || !iq_host) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = batch_alloc(b);
    if (rc) return rc;
    if (nbytes != b->sz.iq_bytes) {
        return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: got %zu bytes, expected %zu", nbytes, b->sz.iq_bytes);
    }
    if ((rc = batch_settle(b, nullptr, "the previous run before an upload"))) return rc;
    HIPCHK(hipMemcpy(b->m.d_iq, iq_host, nbytes, hipMemcpyHostToDevice));
    if (!b->learned.ft_sticky) b->learned.tail_off = false;  // a new input: the one-launch tail gets its chance again
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
    if (nbytes != b->sz.iq_bytes) return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: got %zu bytes, expected %zu", nbytes, b->sz.iq_bytes);
    hipStream_t cs = (hipStream_t)hip_stream;
    if ((rc = batch_settle(b, &cs))) return rc;
    HIPCHK(hipMemcpyAsync(b->m.d_iq, iq_host, nbytes, hipMemcpyHostToDevice, cs));
    HIPCHK(hipEventRecord(b->m.uploaded, cs));
    b->run.upload_pending = true;
    if (!b->learned.ft_sticky) b->learned.tail_off = false;
    return RD_OK;
}

static hipEvent_t batch_event(const rd_batch *b, rd_run_event which) {
    switch (which) {
    case RD_RUN_EV0: return b->run.ev[0];
    case RD_RUN_EV1: return b->run.ev[1];
    case RD_RUN_EV4: return b->run.ev[4];
    case RD_RUN_KFIRST: return b->m.kfirst;
    case RD_RUN_KDONE: return b->m.kdone;
    default: return nullptr;
    }
}

// The tail of the run in flight: everything behind the demod kernel (and k_fixup).  first: the run's first pass - k_tail
// if the demod kernel filled its buckets, and the completion may be deferred (run.plan); else a second pass after an
// overflow, with the separate kernels and an event of its own.
static int batch_tail(rd_batch *b, bool first, uint32_t *zero_next = nullptr) {
    rd_batch_bufs &m = b->m;
    rd_batch_run_state &r = b->run;
    hipStream_t st = r.stream;
    const rd_layout lay = batch_layout(b);
    const long B = b->dc.B, L = b->dc.L, p_lo = B - L, p_hi = (long)(b->n_blocks + 1) * B - L;
    const bool last_on_slice = !b->parse, defer = first && r.plan.defer;
    // the run's last kernel carries the end-of-run event itself when nothing follows it
    hipEvent_t last = batch_event(b, first ? r.plan.end : r.plan.end_again);
    if (r.timing && first) b->timer.ev_end.push_back(defer ? 0 : 1);
    r.dev_order = false;
    if (r.ft_run && first) {  // everything behind the demod kernel in one launch
        rd_ft_bufs fb;
        fb.fixb = m.fixb; fb.gstate = m.gstate; fb.fix_bcap = b->sz.fix_bcap; fb.bcap = b->learned.bcap;
        fb.fixcnt = batch_cnt(b) + b->sz.ft_cnt_off;
        r.ft_seq = r.ft_seq % 4095u + 1u;
        const int ok = rd_launch_tail_fused(lay, b->dc, b->n_blocks, p_lo, p_hi, fb, b->sz.ft_limit ? b->sz.ft_limit : fb.bcap, r.ft_seq, 0,
                                            m.d_recs, m.rec_cap, batch_cnt(b), st, last_on_slice ? last : nullptr, zero_next,
                                            (uint32_t)b->sz.cnt_stride);
        if (!ok) return rd_fail_msg(RD_ERR_STATE, "the one-launch tail refused a shape its buffers were allocated for");
        r.dev_order = true;   // (the records are final: order and dedupe happened on the device)
        r.dense = 1;
    } else {
        rd_launch_search(m.d_bits, b->sz.bits_stride, b->n_streams, b->sz.n_samples, p_lo, p_hi, b->dc, m.d_matches, m.match_cap,
                         batch_cnt(b), st);
        if (r.timing && r.detail) HIPCHK(hipEventRecord(r.ev[3], st));
        r.dense = rd_launch_slice(lay, m.d_bits, b->sz.bits_stride, b->sz.n_samples, b->dc, m.d_matches, m.match_cap, 1, b->n_blocks, 0,
                                  m.d_recs, nullptr, batch_cnt(b), st, last_on_slice ? last : nullptr, m.d_tasks);
    }
    if (b->parse) {
        if (!m.d_parsed) HIPCHK(hipMalloc(&m.d_parsed, (size_t)m.rec_cap * sizeof(rd_parsed)));
        rd_launch_parse(lay, b->dc, m.d_recs, m.match_cap, m.d_parsed, batch_cnt(b), st, r.dense);
    }
    if (defer) {  // the readback is enqueued by whoever launches next on this stream (batch_adopt) or by batch_flush
        std::lock_guard<std::mutex> g(g_tail_mx);
        auto it = g_tail.find(rd_tail_key(m.device, st));
        if (it != g_tail.end() && it->second != b) {  // (cannot happen after rd_batch_run's adoption; kept safe)
            int rc = batch_flush_locked(it->second);
            if (rc) return rc;
        }
        tail_park(b);
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

// The launch code refused the grid (rd_demod_mfma.hip: fewer waves than work queues, more chunks than waves): nothing
// ran, so the handle goes back to where it was - the counter set, the pending upload, the timed-run slot - and holds
// no run: results() reports an error instead of an earlier run's records.  Checked before any adoption: a run waiting
// on this stream keeps waiting for a launch that really happens (or for its own flush).
static int batch_refused(rd_batch *b, bool had_upload) {
    b->run.cnt_set ^= 1;
    b->run.upload_pending = had_upload;
    if (b->timing) b->timer.ev_runs--;
    b->run.ran = false;
    b->run.fetched = true;
    return rd_fail_msg(RD_ERR_STATE, "the demod kernel's grid has fewer waves than work queues and more chunks than waves: not launched");
}

// The state of a new run on `st`: the previous run settled, the pending upload waited for, the other counter set, the run's
// timing mode and its slot in the timer's pool.  *had_upload: what batch_refused puts back.
static int batch_begin_run(rd_batch *b, hipStream_t st, bool *had_upload) {
    rd_batch_run_state &r = b->run;
    // the previous run's readback of d_cnt / d_recs must be over before they are rewritten: the host has already waited
    // for it if the results were fetched (the normal order), else the stream waits.  (r.stream is still the stream THAT run
    // was launched on - the key of its g_tail entry and where its completion event belongs)
    int rc = batch_settle(b, &st);
    if (rc) return rc;
    r.stream = st;
    *had_upload = r.upload_pending;
    if (r.upload_pending) {  // rd_batch_upload_async: the input is on its way
        HIPCHK(hipStreamWaitEvent(st, b->m.uploaded, 0));
        r.upload_pending = false;
    }
    r.fetched = false;
    r.cnt_set ^= 1;  // counters: this run uses the set the previous run's fixup kernel cleared (both start at zero)
    r.timing = b->timing;
    r.detail = b->timing_detail;
    if (r.timing) {
        if ((rc = timer_reserve(b->timer, 5 * (b->timer.ev_runs + 1)))) return rc;
        r.ev = &b->timer.evs[5 * b->timer.ev_runs++];
    }
    return RD_OK;
}

// Settle the previous run, take the plan, launch the demod kernel by it (one launch, one refusal check, one adoption), then
// k_fixup unless the one-launch tail does the fix-up, then the tail.
extern "C" int rd_batch_run(rd_batch *b, void *hip_stream) {
    if (!b) return rd_fail_msg(RD_ERR_ARG, "null batch");
    int rc = batch_alloc(b);
    if (rc) return rc;
    rd_batch_run_state &r = b->run;
    hipStream_t st = (hipStream_t)hip_stream;
    bool had_upload = false;
    if ((rc = batch_begin_run(b, st, &had_upload))) return rc;
    uint32_t *cnt = batch_cnt(b), *cnt_next = b->m.d_cnt + (size_t)(r.cnt_set ^ 1) * b->sz.cnt_stride;
    // (parked: a pipelined run waiting on this stream is adopted by this run's demod kernel, through its stop event)
    const rd_run_plan p = r.plan = rd_batch_plan_run({b->sz.fast_ok, b->sz.ft_ok, b->learned.tail_off, r.timing, r.detail, b->pipelined,
                                                      b->parse, batch_stream_has_tail(b->m.device, st)});
    // the one-launch tail: the fix-up entries go to its workgroups' buckets
    uint32_t *fixl = p.buckets ? b->m.fixb : b->m.d_fix, *bcnt = p.buckets ? cnt + b->sz.ft_cnt_off : nullptr;
    const uint32_t fixc = p.buckets ? b->sz.fix_bcap : b->sz.fix_cap;
    const rd_layout lay = batch_layout(b);
    uint32_t honoured = 0;
    if (p.record_around) HIPCHK(hipEventRecord(r.ev[0], st));
    if (p.demod) {  // the dispatch carries its own start / stop events (no marker packets)
        honoured = rd_launch_demod(lay, fixl, fixc, cnt, st, batch_event(b, p.ride_start), batch_event(b, p.ride_stop),
                                   p.buckets ? RD_DEMOD_FIX_BUCKETS : 0u, r.last_launch, bcnt);
        if (honoured & RD_DEMOD_REFUSED) return batch_refused(b, had_upload);
    }
    if (p.record_around) HIPCHK(hipEventRecord(r.ev[1], st));
    if (p.record_carrier) HIPCHK(hipEventRecord(batch_event(b, p.carrier), st));
    if (p.carrier && (rc = batch_adopt(b->m.device, st, batch_event(b, p.carrier)))) return rc;
    r.second_pass = false;
    r.ft_run = p.demod && (honoured & RD_DEMOD_FIX_BUCKETS);
    if (!r.ft_run)   // (fixl / fixc: where this run's demod kernel put its list - the groups' bucket space when an ablated kernel
                     // of the diagnostic library declined the buckets; bounded by fixc either way)
        rd_launch_fixup(lay, fixl, fixc, cnt, p.demod ? 0 : 1, cnt_next, st, (uint32_t)b->sz.cnt_stride, b->learned.last_fix);
    if (r.timing && r.detail) HIPCHK(hipEventRecord(r.ev[2], st));
    if ((rc = batch_tail(b, true, r.ft_run ? cnt_next : nullptr))) return rc;
    r.ran = true;
    return RD_OK;
}

// a second search / slice pass of the run in flight, with an event of its own, over cleared lists
static int batch_second_pass(rd_batch *b) {
    const uint32_t zero[5] = {0, 0, 0, 0, 0};  // matches, boundary records, tasks, parsed, overflow flags
    HIPCHK(hipMemcpyAsync(batch_cnt(b) + RD_CNT_MATCH, zero, sizeof zero, hipMemcpyHostToDevice, b->run.stream));
    b->run.second_pass = true;
    return batch_tail(b, false);
}

// The overflow ladder's hands (rd_batch_plan.h: rd_batch_ladder_run decides, this carries out).
struct batch_ladder {
    rd_batch *b;
    int read(rd_ladder_in &in) {  // synchronise, fetch the counters
        rd_batch_run_state &r = b->run;
        const double ta = now_ms();
        int rc = rd_wait_event(b->m.done, "the batch run's results");
        if (rc) return rc;
        memcpy(r.h_cnt, b->m.h_cnt_pin, sizeof r.h_cnt);
        if (dbg_host()) fprintf(stderr, "[rd] finish: wait %.3f ms\n", now_ms() - ta);
        in = {r.h_cnt[RD_CNT_FIX], r.h_cnt[RD_CNT_MATCH], r.h_cnt[RD_CNT_OVF], r.ft_run, r.second_pass, r.dev_order, b->sz.fast_ok, 0,
              b->sz.fix_cap, b->m.match_cap, b->sz.ft_limit, (uint64_t)b->n_streams * b->sz.bits_stride};
        return RD_OK;
    }
    int carry_out(const rd_ladder_action &a) {  // (rd_ladder_action: in the order of its fields)
        rd_batch_run_state &r = b->run;
        int rc = RD_OK;
        r.dev_order = a.dev_order;
        if (a.exact_fixup) rd_launch_fixup(batch_layout(b), b->m.d_fix, b->sz.fix_cap, batch_cnt(b), 1, nullptr, r.stream);
        const uint32_t cap = b->sz.fix_cap;
        if (a.stamp_fix) HIPCHK(hipMemcpyAsync(batch_cnt(b) + RD_CNT_FIX, &cap, sizeof cap, hipMemcpyHostToDevice, r.stream));
        if (a.tail_overflow && dbg_host())
            fprintf(stderr, "[rd] one-launch tail overflow: flags %u (1 a stream's match list, 2 records), matches %u\n",
                    r.h_cnt[RD_CNT_OVF], r.h_cnt[RD_CNT_MATCH]);
        if (a.grow_to && (rc = batch_alloc_lists(b, a.grow_to))) return rc;   // longer lists
        if (a.second_pass && (rc = batch_second_pass(b))) return rc;
        if (a.done) r.fetched = true;
        return RD_OK;
    }
    int gave_up() { return rd_fail_msg(RD_ERR_DEVICE, "result lists kept overflowing"); }
};

// Synchronise, handle list overflows (re-running what is needed), fetch the counters.
static int batch_finish(rd_batch *b) {
    if (!b->run.ran) return rd_fail_msg(RD_ERR_STATE, "rd_batch_run has not been called");
    int rc = batch_flush(b);  // pipelined and not adopted: nothing was launched behind this run
    if (rc) return rc;
    batch_ladder hands = {b};
    return rd_batch_ladder_run(hands, b->learned);
}

extern "C" int rd_batch_results(rd_batch *b, rd_packet *out, int cap, int *n) {
    if (!b || !n) return rd_fail_msg(RD_ERR_ARG, "null argument");
    const double t0 = now_ms();
    int rc = batch_finish(b);
    if (rc) return rc;
    const double t1 = now_ms();
    rd_batch_bufs &m = b->m;
    rd_batch_run_state &r = b->run;
    // one record per match, plus the second records of block-boundary positions (kept apart on
    // the device, appended here)
    const rd_result_counts c = rd_batch_result_counts(r.h_cnt, r.dense != 0, m.match_cap, m.rec_cap);
    // Late copies go to the copy stream: it has already waited for this run's last kernel, whereas the
    // launch stream may hold the NEXT batch's run by now (two resident batches alternate in bench.py) and a
    // copy queued there would wait for it.
    if (c.nprim > r.have) {  // more records than were copied back with the run: fetch the rest
        rc = rd_copy_d2h(m.h_recs_pin + r.have, m.d_recs + r.have, (size_t)(c.nprim - r.have) * sizeof(rd_packet), m.copy_stream);
        if (rc) return rc;
    }
    if (c.nextra) {  // second records of block-boundary positions (q == B in one call, q == 0 in the next)
        rc = rd_copy_d2h(m.h_recs_pin + c.nprim, m.d_recs + m.match_cap, (size_t)c.nextra * sizeof(rd_packet), m.copy_stream);
        if (rc) return rc;
    }
    const uint32_t nrec = c.nprim + c.nextra;
    b->learned.spec_recs = std::max<uint32_t>(1024, c.nprim + c.nprim / 4);
    // (what a repeated call for this run takes as copied: the new speculative count, which covers the nprim just fetched
    // wherever the lists are long enough for it)
    r.have = rd_batch_spec_count(r.dev_order, m.match_cap, m.rec_cap, b->learned.spec_recs);
    const double t2 = now_ms();
    // the device wrote them in the reference's order, duplicates dropped (copy, nothing else) - or the host orders them
    if (!r.dev_order) rd_order_and_dedupe(m.h_recs_pin, nrec, b->dc.S, b->order);
    const size_t count = r.dev_order ? nrec : b->order.kept.size();
    *n = (int)count;
    if ((int)count > cap) return rd_fail_msg(RD_ERR_CAPACITY, "need room for %zu packets", count);
    if (count && !out) return rd_fail_msg(RD_ERR_ARG, "null out");
    if (r.dev_order && count) memcpy(out, m.h_recs_pin, count * sizeof(rd_packet));
    if (!r.dev_order)
        for (size_t i = 0; i < count; i++) out[i] = m.h_recs_pin[b->order.kept[i]];  // straight into the caller's array
    if (dbg_host())
        fprintf(stderr, "[rd] results%s: finish %.3f ms, D2H %u recs %.3f ms, %s %.3f ms\n", r.dev_order ? " (k_tail)" : "", t1 - t0,
                nrec, t2 - t1, r.dev_order ? "copy" : "order+dedupe+copy", now_ms() - t2);
    return RD_OK;
}

extern "C" int rd_batch_copy_bits(rd_batch *b, int stream, uint8_t *out, size_t nbytes) {
    if (!b || !out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (stream < 0 || stream >= b->n_streams) return rd_fail_msg(RD_ERR_ARG, "stream out of range");
    const size_t need = (size_t)((b->sz.n_samples + 7) / 8);
    if (nbytes < need) return rd_fail_msg(RD_ERR_ARG, "bit buffer too small: %zu < %zu", nbytes, need);
    int rc = batch_finish(b);
    if (rc) return rc;
    return rd_copy_d2h(out, (const uint8_t *)(b->m.d_bits + (size_t)stream * b->sz.bits_stride), need, b->run.stream);
}

extern "C" int rd_batch_copy_discriminated(rd_batch *b, int stream, size_t t0, double *out, size_t n) {
    if (!b || !out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (stream < 0 || stream >= b->n_streams || t0 + n > (size_t)b->sz.n_samples)
        return rd_fail_msg(RD_ERR_ARG, "range out of bounds");
    int rc = batch_alloc(b);
    if (rc) return rc;
    if (n == 0) return RD_OK;
    double *d = nullptr;
    HIPCHK(hipMalloc(&d, n * sizeof(double)));
    rd_launch_disc(batch_layout(b), stream, (long)t0, (long)n, d, b->run.stream);
    rc = rd_copy_d2h(out, d, n * sizeof(double), b->run.stream);
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
    const uint32_t np = std::min(b->run.h_cnt[RD_CNT_PARSED], b->m.rec_cap);
    std::vector<rd_parsed> recs(np);
    if (np) {
        rc = rd_copy_d2h(recs.data(), b->m.d_parsed, (size_t)np * sizeof(rd_parsed), b->run.stream);
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
    b->timer.ev_runs = 0;
    b->timer.ev_end.clear();
    // events for the first 64 timed runs exist before the first of them is launched (creating them one run at a
    // time showed as a stall of several milliseconds inside a 60 ms timed region)
    if (b->timing && b->dev_ready && rd_use_device(b->m.device) == RD_OK) return timer_reserve(b->timer, 5 * 64);
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
    for (size_t r = 0; r < b->timer.ev_runs; r++) {
        hipEvent_t *e = &b->timer.evs[5 * r];
        float v[5] = {0, 0, 0, 0, 0};
        HIPCHK(hipEventElapsedTime(&v[0], e[0], e[1]));
        if (b->timing_detail) {
            HIPCHK(hipEventElapsedTime(&v[1], e[1], e[2]));
            HIPCHK(hipEventElapsedTime(&v[2], e[2], e[3]));
            HIPCHK(hipEventElapsedTime(&v[3], e[3], e[4]));
        }
        // (a pipelined run has no end-of-run event: total_ms is the mean over the runs that have one, 0 if none)
        const bool has_end = r >= b->timer.ev_end.size() || b->timer.ev_end[r];
        if (has_end) { HIPCHK(hipEventElapsedTime(&v[4], e[0], e[4])); n_end++; }
        t.demod_ms += v[0]; t.fixup_ms += v[1]; t.search_ms += v[2]; t.slice_ms += v[3]; t.total_ms += v[4];
    }
    if (b->timer.ev_runs) {
        const float k = 1.0f / (float)b->timer.ev_runs;
        t.demod_ms *= k; t.fixup_ms *= k; t.search_ms *= k; t.slice_ms *= k;
        t.total_ms = n_end ? t.total_ms / (float)n_end : 0.0f;
    }
    t.runs = (int32_t)b->timer.ev_runs;
    b->timer.ev_runs = 0;
    b->timer.ev_end.clear();
    *out = t;
    return RD_OK;
}

// Which forms the last run took (after it has completed): RD_FORM_* bits.
extern "C" int rd_batch_last_run_forms(rd_batch *b, uint32_t *forms) {
    if (!b || !forms) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = batch_finish(b);
    if (rc) return rc;
    *forms = (b->run.dev_order ? RD_FORM_ORDERED_TAIL | RD_FORM_ONE_LAUNCH_TAIL : 0u) | (b->run.second_pass ? RD_FORM_SECOND_PASS : 0u);
    return RD_OK;
}

extern "C" int rd_k1_schedule(rd_batch *b, uint32_t *tiles_per_chunk, uint32_t *waves) {
    uint32_t v[2] = {0, 0};
    if (b) {
        if (!b->run.ran) return rd_fail_msg(RD_ERR_STATE, "rd_batch_run has not been called");
        v[0] = b->run.last_launch[0]; v[1] = b->run.last_launch[1];
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
    if (fixup_runs) *fixup_runs = b->learned.last_fix;
    if (matches) *matches = b->learned.last_match;
    return RD_OK;
}
