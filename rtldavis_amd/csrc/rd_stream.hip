// rd_stream.hip - the streaming demodulator of the C ABI (include/rtldavis_hip.h: rd_create .. rd_copy_quantized;
// py:128-253) and the entry points the wideband receiver reaches it through (rd_internal.h: rd_demod_prepare ..).
//
// Host-side orchestration only: the slots of the two blocks in flight, which launch form a block takes, the waits.  The
// arithmetic runs in the kernels of rd_stream_kernels.hip and rd_tail_kernels.hip, the fetch from a slot's device-written counts to host copies in
// rd_host.cpp (rd_collect_block).  py = /root/reference/src/rtldavis/dsp.py
#include <immintrin.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rd_internal.h"

// One block in flight: its input where the host or the device put it, and what its kernels report.
// A slot's mapped pinned buffers - m[k].h the host's address, m[k].d the device's of the same memory, taken once:
enum {
    SL_IN,     // NS x 2B bytes (or B complex128): the block, where the one-launch kernel reads it
    SL_RECS,   // rec_cap rd_packet: written by the slice kernel
    SL_SB,     // the one-launch block (k_stream_block): [NS] matches found, [NS] sequence numbers that say "done"
    SL_FE,     // Parser.parse's front half on the device (rd_demod_set_parse): per record place of SL_RECS, RD_FE_NONE or the
               // packet's frequency error, written by the kernel that writes the record (or by k_stream_parse behind the slice)
    SL_MAPPED
};
struct rd_mapped {
    uint8_t *h = nullptr, *d = nullptr;
};
struct rd_slot {
    rd_mapped m[SL_MAPPED];
    uint8_t *d_in = nullptr;         // device staging: the H2D copy lands here on the copy stream
    uint8_t *d_push = nullptr;       // uncached device memory the HOST writes the block into (large BAR), or null
    uint32_t *h_cnt = nullptr;       // pinned: the multi-launch form's counters
    uint32_t seq = 0;                // what the flags read once this slot's block is done
    bool one = false;                // this slot's block went through k_stream_block
    bool parse = false;              // this slot's block was submitted with parse on
    hipEvent_t e_in = nullptr, e_done = nullptr;
    template <class T> T *host(int k) const { return (T *)m[k].h; }
    template <class T> T *dev(int k) const { return (T *)m[k].d; }
};

struct rd_demod {
    rd_config cfg;
    rd_devcfg dc;
    bool dev_ready = false;
    bool cplx_mode = false;  // switched on by the first complex128 block, until reset
    long seen = 0;           // blocks submitted since reset
    int NS = 1;              // independent streams fed in lock step (rd_create_multi)
    int device = -1;         // the device the buffers live on
    size_t ring_stride = 0;  // bytes between the streams' rings
    // per stream, byte ring: [hdr 32 B][prev 2B][cur 2B]; complex ring (NS == 1 only):
    // [hdr 16][prev B][cur B] complex128
    uint8_t *d_ring = nullptr;
    double *d_cring = nullptr;
    uint32_t *d_sync = nullptr;   // k_stream_block_cplx's arrival counter (zero between launches)
    uint32_t *d_blockbits = nullptr, *d_win[2] = {nullptr, nullptr}, *d_fix = nullptr, *d_cnt = nullptr;
    int cur_win = 0;
    rd_match *d_matches = nullptr;
    double *d_tmp = nullptr;  // 2*(B+1) doubles for the state mirrors
    double *h_tmp = nullptr;        // pinned mirror of d_tmp (state accessors)
    // Two slots: block i+1's host-to-device copy (copy stream) runs beside block i's kernels (compute
    // stream).  rd_demod_block = submit + fetch of one block; rd_demod_submit / rd_demod_fetch expose the
    // pipeline (runners/rtlsdr.py:100-103 -> worker.py:34-58 without the pickled-queue hop).
    rd_slot slot[2];
    int head = 0, nflight = 0;      // oldest block in flight, blocks in flight (0..2)
    hipStream_t st = nullptr, st_copy = nullptr;
    volatile uint32_t *hdp_flush = nullptr;  // host push (rd_hiphost.h: rd_push_flush_reg) where the slots have a d_push
    std::vector<rd_packet> last;    // ordered, deduplicated records of the last fetched block
    rd_block_scratch collect;       // the fetch's scratch
    uint32_t fix_cap = 0, match_cap = 0, rec_cap = 0;
    bool fast_ok = false;
    bool one_ok = false;            // the configuration is one k_stream_block is built for (and RD_STREAM_IMPL != legacy)
    uint32_t seq = 0;               // blocks sent through k_stream_block
    // A producer's buffer registered with the device (rd_demod_register_input): rd_demod_submit_from launches on blocks
    // that already lie there - a shared-memory ring an SDR process fills - without copying them anywhere
    uint8_t *ext_host = nullptr, *ext_dev = nullptr;
    size_t ext_bytes = 0;
    bool parse = false;             // rd_demod_set_parse: blocks submitted from now on are parsed on the device
    bool fetched = false;           // a block has been fetched since create / reset ...
    bool last_parse = false;        // ... and it had been submitted with parse on: last_parsed holds its messages
    std::vector<rd_parsed> last_parsed;  // CRC-valid messages of the last fetched block, in the order of `last`
    int stale = 0;                  // blocks in flight whose fetch timed out: dropped (waited for, results discarded) by
                                    // the next submit / reset - the caller has already been told (worker.py:56-58)
};

extern "C" int rd_create_multi(const rd_config *cfg, int n_streams, rd_demod **out) {
    if (!out) return rd_fail_msg(RD_ERR_ARG, "null out");
    rd_devcfg dc;
    int rc = rd_devcfg_checked(cfg, &dc);
    if (rc) return rc;
    if (n_streams < 1 || (uint64_t)n_streams * ((uint64_t)dc.B + 1) > 0x7FFFFFFFull)
        return rd_fail_msg(RD_ERR_ARG, "n_streams out of range");
    rd_demod *h = new rd_demod();
    h->cfg = *cfg;
    h->dc = dc;
    h->NS = n_streams;
    h->ring_stride = ((32 + 4 * (size_t)dc.B) + 15) & ~(size_t)15;
    h->fast_ok = (dc.B % 8) == 0;
    *out = h;
    return RD_OK;
}

extern "C" int rd_create(const rd_config *cfg, rd_demod **out) { return rd_create_multi(cfg, 1, out); }

static size_t ring_cur_off(const rd_demod *h) { return 32 + 2 * (size_t)h->dc.B; }

// the two slots: every mapped pair, the staging and push buffers, the pinned counters, the events
static int demod_alloc_slots(rd_demod *h) {
    const size_t B = (size_t)h->dc.B, NS = (size_t)h->NS;
    size_t bytes[SL_MAPPED];
    bytes[SL_IN] = std::max(16 * B, NS * 2 * B);
    bytes[SL_RECS] = (size_t)h->rec_cap * sizeof(rd_packet);
    bytes[SL_SB] = 2 * NS * sizeof(uint32_t);
    bytes[SL_FE] = (size_t)h->rec_cap * sizeof(int32_t);
    h->hdp_flush = rd_push_flush_reg(h->device);
    for (rd_slot &sl : h->slot) {
        for (int k = 0; k < SL_MAPPED; k++) {
            HIPCHK(hipHostMalloc((void **)&sl.m[k].h, bytes[k], hipHostMallocMapped));
            HIPCHK(hipHostGetDevicePointer((void **)&sl.m[k].d, sl.m[k].h, 0));
        }
        memset(sl.m[SL_SB].h, 0, bytes[SL_SB]);
        HIPCHK(hipMalloc(&sl.d_in, bytes[SL_IN]));
        if (h->hdp_flush && hipExtMallocWithFlags((void **)&sl.d_push, bytes[SL_IN], hipDeviceMallocUncached) != hipSuccess) {
            (void)hipGetLastError();
            sl.d_push = nullptr;   // (the pinned slot serves)
        }
        HIPCHK(hipHostMalloc((void **)&sl.h_cnt, RD_CNT_SLOTS * 4, hipHostMallocDefault));
        HIPCHK(hipEventCreateWithFlags(&sl.e_in, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&sl.e_done, hipEventDisableTiming));
    }
    return RD_OK;
}

// Nothing is allocated inside a demodulate() call: the complex ring of a single-stream handle exists from the start
// (pyrtlsdr feeds complex blocks), and the state mirrors' float64 kernels run once here - the first launch of a
// kernel that needs scratch memory costs milliseconds, which `.discriminated` (read by protocol.py:307-309 for the
// first CRC-valid packet) used to pay inside a 30 ms block budget.
static int demod_warm_up(rd_demod *h) {
    const size_t B = (size_t)h->dc.B;
    if (h->NS == 1) {
        HIPCHK(hipMalloc(&h->d_cring, 2 * (16 + 2 * B) * sizeof(double)));
        HIPCHK(hipMemset(h->d_cring, 0, 2 * (16 + 2 * B) * sizeof(double)));
        HIPCHK(hipMalloc(&h->d_sync, 64));
        HIPCHK(hipMemset(h->d_sync, 0, 64));
    }
    HIPCHK(hipDeviceSynchronize());  // the memsets of demod_alloc ran on the null stream
    rd_layout wl;
    wl.iq = h->d_ring + 32 + 2 * B; wl.stream_stride = h->ring_stride; wl.n_streams = h->NS; wl.n_samples = (uint32_t)B;
    wl.hist_mode = 0; wl.valid_from = 0; wl.bits = h->d_blockbits; wl.bits_stride = (B + 31) / 32;
    rd_launch_disc(wl, 0, 0, 8, h->d_tmp, h->st);
    rd_launch_filtered(wl, 0, 0, 8, h->d_tmp, h->st);
    if (h->d_cring) {
        rd_cplx_layout cl;
        cl.x = h->d_cring + 2 * (16 + B); cl.valid_from = 0; cl.n = (long)B;
        rd_launch_cplx_disc(cl, 0, 8, h->d_tmp, h->st);
        rd_launch_cplx_filtered(cl, 0, 8, h->d_tmp, h->st);
    }
    HIPCHK(hipMemcpyAsync(h->h_tmp, h->d_tmp, 64, hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipStreamSynchronize(h->st));
    return RD_OK;
}

static int demod_alloc(rd_demod *h) {
    if (h->dev_ready) return rd_use_device(h->device);
    int rc = rd_ensure_device();
    if (rc) return rc;
    HIPCHK(hipGetDevice(&h->device));
    const size_t B = (size_t)h->dc.B, L = (size_t)h->dc.L, NS = (size_t)h->NS;
    const size_t ring_bytes = NS * h->ring_stride + RD_INPUT_PAD;
    HIPCHK(hipMalloc(&h->d_ring, ring_bytes));
    HIPCHK(hipMemset(h->d_ring, 127, ring_bytes));
    h->fix_cap = (uint32_t)(NS * ((B + 31) / 32));  // every run of a block
    h->match_cap = (uint32_t)(NS * (B + 1));        // every position of every window: cannot overflow
    h->rec_cap = h->match_cap;
    HIPCHK(hipMalloc(&h->d_blockbits, NS * ((B + 31) / 32) * 4));
    for (int i = 0; i < 2; i++) {
        HIPCHK(hipMalloc(&h->d_win[i], NS * ((L + 31) / 32) * 4));
        HIPCHK(hipMemset(h->d_win[i], 0, NS * ((L + 31) / 32) * 4));
    }
    HIPCHK(hipMalloc(&h->d_fix, (size_t)h->fix_cap * 4));
    HIPCHK(hipMalloc(&h->d_cnt, RD_CNT_TOTAL * 4));
    HIPCHK(hipMalloc(&h->d_matches, (size_t)h->match_cap * sizeof(rd_match)));
    HIPCHK(hipMalloc(&h->d_tmp, 2 * (2 * B + 2) * sizeof(double)));
    HIPCHK(hipHostMalloc((void **)&h->h_tmp, 2 * (2 * B + 2) * sizeof(double), hipHostMallocDefault));
    if ((rc = demod_alloc_slots(h))) return rc;
    HIPCHK(hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&h->st_copy, hipStreamNonBlocking));
    if ((rc = demod_warm_up(h))) return rc;
    // one launch per block where the kernel exists for the configuration; RD_STREAM_IMPL=legacy: the multi-launch form (A/B)
    const char *e = getenv("RD_STREAM_IMPL");
    const rd_devcfg &c = h->dc;
    h->one_ok = !(e && e[0] == 'l') && h->fast_ok && rd_davis_shape(c) &&
                c.L == 2 * c.B && c.B % 32 == 0 && c.B >= 2048 && c.B <= 16384;
    h->dev_ready = true;
    return RD_OK;
}

extern "C" void rd_destroy(rd_demod *h) {
    if (!h) return;
    if (h->dev_ready && rd_owns_device_state()) {
        if (h->device >= 0) hipSetDevice(h->device);
        if (h->st) hipStreamSynchronize(h->st);
        if (h->st_copy) hipStreamSynchronize(h->st_copy);
        if (h->ext_host) hipHostUnregister(h->ext_host);
        hipFree(h->d_ring); hipFree(h->d_cring); hipFree(h->d_sync); hipFree(h->d_blockbits);
        hipFree(h->d_win[0]); hipFree(h->d_win[1]); hipFree(h->d_fix); hipFree(h->d_cnt);
        hipFree(h->d_matches); hipFree(h->d_tmp);
        hipHostFree(h->h_tmp);
        for (rd_slot &sl : h->slot) {
            for (rd_mapped &m : sl.m) hipHostFree(m.h);
            hipFree(sl.d_in); hipFree(sl.d_push); hipHostFree(sl.h_cnt);
            if (sl.e_in) hipEventDestroy(sl.e_in);
            if (sl.e_done) hipEventDestroy(sl.e_done);
        }
        if (h->st) hipStreamDestroy(h->st);
        if (h->st_copy) hipStreamDestroy(h->st_copy);
    }
    delete h;
}

// Wait (polling, with the deadline of every host wait) until the block in `sl` has completed.
static int demod_wait_slot(rd_demod *h, rd_slot &sl) {
    if (!sl.one) return rd_wait_event(sl.e_done, "the block's kernels");
    // one-launch block: the streams' sequence numbers in pinned memory (an event query costs microseconds; a kernel
    // that died would never write them, so the stream is asked now and then)
    const size_t NS = (size_t)h->NS;
    volatile uint32_t *flag = sl.host<uint32_t>(SL_SB) + NS;
    rd_waiter w(rd_wait_timeout_ms());
    uint32_t spins = 0;
    for (size_t s = 0; s < NS; s++) {
        while (flag[s] != sl.seq) {
            if (!w.relax())
                return rd_fail_msg(RD_ERR_DEVICE, "timed out after %.0f ms waiting for the block's kernel (stream %zu of %zu)",
                                   w.waited_ms(), s, NS);
            if ((++spins & 0xFFF) == 0xFFF || w.polls >= 1024) {  // (>= 1024 polls: past the 50 us of spinning)
                const hipError_t e = hipStreamQuery(h->st);
                if (e != hipSuccess && e != hipErrorNotReady)
                    return rd_fail_msg(RD_ERR_DEVICE, "hipStreamQuery: %s", hipGetErrorString(e));
                if (e == hipSuccess && flag[s] != sl.seq)
                    return rd_fail_msg(RD_ERR_DEVICE, "the block's kernel finished without reporting stream %zu", s);
            }
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return RD_OK;
}

// Blocks whose fetch timed out are still in flight: wait for them (deadline again) and discard what they found - the
// streams' state (ring, window) has advanced by them as the reference's would have, only their packets are lost.
static int demod_drop_stale(rd_demod *h) {
    while (h->stale > 0 && h->nflight > 0) {
        int rc = demod_wait_slot(h, h->slot[h->head]);
        if (rc) return rc;
        h->head ^= 1;
        h->nflight--;
        h->stale--;
    }
    h->stale = 0;
    return RD_OK;
}

// every block in flight has been fetched (state accessors and reset need a quiet handle)
static int demod_quiet(rd_demod *h) {
    if (h->stale) {
        int rc = demod_drop_stale(h);
        if (rc) return rc;
    }
    if (h->nflight) return rd_fail_msg(RD_ERR_STATE, "%d block(s) in flight: rd_demod_fetch them first", h->nflight);
    return RD_OK;
}

extern "C" int rd_reset(rd_demod *h) {
    if (!h) return rd_fail_msg(RD_ERR_ARG, "null handle");
    if (h->dev_ready) {
        // blocks still in flight are dropped: wait for them, then clear
        // (on a timeout the handle is left as it was: reset() may be called again once the device has caught up)
        for (int i = 0; i < h->nflight; i++) {
            int rc = demod_wait_slot(h, h->slot[(h->head + i) & 1]);
            if (rc) return rc;
        }
        const size_t L = (size_t)h->dc.L;
        for (int i = 0; i < 2; i++)
            HIPCHK(hipMemsetAsync(h->d_win[i], 0, (size_t)h->NS * ((L + 31) / 32) * 4, h->st));
        if (h->d_sync) HIPCHK(hipMemsetAsync(h->d_sync, 0, 64, h->st));   // (a launch that never finished may have left a count)
        int rc = rd_wait_stream(h->st, "reset()'s clears");
        if (rc) return rc;
    }
    h->stale = 0;
    h->nflight = 0;
    h->head = 0;
    h->seen = 0;
    h->cplx_mode = false;
    h->last.clear();
    h->last_parsed.clear();
    h->fetched = h->last_parse = false;
    return RD_OK;
}

// first readable sample relative to the newest block's sample 0
static long demod_valid_from(const rd_demod *h, long seen_before) {
    const long B = h->dc.B;
    if (seen_before <= 0) return 0;
    if (seen_before == 1) return -B;
    return -(B + 16);
}

static rd_layout demod_layout(const rd_demod *h, long seen_before) {
    rd_layout l;
    l.iq = h->d_ring + ring_cur_off(h);
    l.stream_stride = h->ring_stride;
    l.n_streams = h->NS;
    l.n_samples = (uint32_t)h->dc.B;
    l.hist_mode = seen_before > 0 ? 1 : 0;
    l.valid_from = demod_valid_from(h, seen_before);
    l.bits = h->d_blockbits;
    l.bits_stride = (size_t)((h->dc.B + 31) / 32);
    return l;
}

static rd_cplx_layout demod_clayout(const rd_demod *h, long seen_before) {
    rd_cplx_layout l;
    l.x = h->d_cring + 2 * (16 + (size_t)h->dc.B);
    l.valid_from = demod_valid_from(h, seen_before);
    l.n = h->dc.B;
    return l;
}

// Switch to the complex ring: LUT-convert the byte ring (py:26,38-39 - what the reference
// keeps in raw_samples) so history carries over exactly.
static int demod_enter_cplx(rd_demod *h) {
    const size_t B = (size_t)h->dc.B;
    if (!h->d_cring) HIPCHK(hipMalloc(&h->d_cring, 2 * (16 + 2 * B) * sizeof(double)));  // (single-stream handles have it from demod_alloc)
    rd_launch_lut(h->d_ring, h->d_cring, 16 + 2 * B, h->st);
    HIPCHK(hipGetLastError());
    h->cplx_mode = true;
    return RD_OK;
}

// ------------------------------------------------------------------------------------------
// submit: three forms of one block
// ------------------------------------------------------------------------------------------
// What rd_sb_args and rd_sbc_args share: the block at device address `in`, the windows, the slot's mapped buffers, the
// sequence number this launch will report
template <class A> static void one_launch_args(A &a, const rd_demod *h, const rd_slot &sl, const uint8_t *in) {
    a.cfg = h->dc;
    a.in = in;
    a.win_in = h->d_win[h->cur_win];
    a.win_out = h->d_win[h->cur_win ^ 1];
    a.recs_host = sl.dev<rd_packet>(SL_RECS);
    a.cnt_host = sl.dev<uint32_t>(SL_SB);
    a.flag_host = sl.dev<uint32_t>(SL_SB) + h->NS;
    a.seq = h->seq + 1;
    a.seen_before = h->seen;
    a.stamps = nullptr;
    a.parse = sl.parse ? 1 : 0;
    a.fe_host = sl.dev<int32_t>(SL_FE);
}

// a one-launch block is queued: its window is the current one, the slot waits for its sequence number
static int one_launched(rd_demod *h, rd_slot &sl, uint32_t seq) {
    h->seq = seq;
    HIPCHK(hipGetLastError());
    h->cur_win ^= 1;
    sl.seq = seq;
    sl.one = true;
    h->seen++;
    h->nflight++;
    return RD_OK;
}

// ONE launch: the kernel takes the block from `in`, rolls the ring, decides the bits exactly, searches, slices and leaves
// records, counts and a per-stream sequence number in mapped host memory.  sl.one says whether it was launched: the
// kernel declines a configuration it is not built for.
static int submit_one_u8(rd_demod *h, rd_slot &sl, const uint8_t *in) {
    rd_sb_args a;
    one_launch_args(a, h, sl, in);
    a.ring = h->d_ring;
    a.ring_stride = h->ring_stride;
    return rd_launch_stream_block(a, h->NS, h->st) ? one_launched(h, sl, a.seq) : RD_OK;
}

// ONE launch for the complex-input branch as well (py:144-150: what pyrtlsdr's stream() feeds the live receiver,
// /root/reference/src/rtldavis/runners/rtlsdr.py:100-103); a uint8 block on a handle in complex mode goes through
// the LUT inside the kernel.  The first complex block converts the byte ring once (py:26,38-39: history carries over)
static int submit_one_cplx(rd_demod *h, rd_slot &sl, const uint8_t *in, int is_complex) {
    if (!h->cplx_mode) {
        int rc = demod_enter_cplx(h);
        if (rc) return rc;
    }
    rd_sbc_args a;
    one_launch_args(a, h, sl, in);
    a.ring = h->d_cring;
    a.in_is_u8 = is_complex ? 0 : 1;
    a.sync = h->d_sync;
    return rd_launch_stream_block_cplx(a, h->st) ? one_launched(h, sl, a.seq) : RD_OK;
}

// The multi-launch form's steps that differ between the byte rings and the complex ring.  roll: the raw rings left by one
// block (py:140,154) - hdr <- tail of prev, prev <- cur, cur <- the new block in sl.d_in.  bits: the block's exact bits
// into d_blockbits.  slice: records of the matches into the slot, and their fe entries when the block is parsed.
struct multi_form {
    int (*roll)(rd_demod *h, const rd_slot &sl, int is_complex, long seen_before);
    int (*bits)(rd_demod *h, long seen_before);
    void (*slice)(rd_demod *h, const rd_slot &sl, long seen_before);
};

static int roll_u8(rd_demod *h, const rd_slot &sl, int, long seen_before) {
    const size_t B = (size_t)h->dc.B, NS = (size_t)h->NS, rs = h->ring_stride;
    uint8_t *r = h->d_ring;
    if (seen_before > 0) {
        HIPCHK(hipMemcpy2DAsync(r, rs, r + 2 * B, rs, 32, NS, hipMemcpyDeviceToDevice, h->st));
        HIPCHK(hipMemcpy2DAsync(r + 32, rs, r + 32 + 2 * B, rs, 2 * B, NS, hipMemcpyDeviceToDevice, h->st));
    }
    HIPCHK(hipMemcpy2DAsync(r + 32 + 2 * B, rs, sl.d_in, 2 * B, 2 * B, NS, hipMemcpyDeviceToDevice, h->st));
    return RD_OK;
}
static int roll_cplx(rd_demod *h, const rd_slot &sl, int is_complex, long seen_before) {
    const size_t B = (size_t)h->dc.B;
    double *r = h->d_cring;
    if (seen_before > 0) {
        HIPCHK(hipMemcpyAsync(r, r + 2 * B, 32 * sizeof(double), hipMemcpyDeviceToDevice, h->st));
        HIPCHK(hipMemcpyAsync(r + 32, r + 32 + 2 * B, 2 * B * sizeof(double), hipMemcpyDeviceToDevice, h->st));
    }
    if (is_complex) HIPCHK(hipMemcpyAsync(r + 32 + 2 * B, sl.d_in, 2 * B * sizeof(double), hipMemcpyDeviceToDevice, h->st));
    else rd_launch_lut(sl.d_in, r + 32 + 2 * B, B, h->st);
    return RD_OK;
}
static int bits_u8(rd_demod *h, long seen_before) {
    const rd_layout lay = demod_layout(h, seen_before);
    if (h->fast_ok && (rd_launch_demod(lay, h->d_fix, h->fix_cap, h->d_cnt, h->st) & RD_DEMOD_REFUSED))
        return rd_fail_msg(RD_ERR_STATE, "the demod kernel's grid has fewer waves than work queues and more chunks than waves: not launched");
    rd_launch_fixup(lay, h->d_fix, h->fix_cap, h->d_cnt, h->fast_ok ? 0 : 1, nullptr, h->st);
    return RD_OK;
}
static int bits_cplx(rd_demod *h, long seen_before) {
    rd_launch_cplx_bits(demod_clayout(h, seen_before), h->d_blockbits, h->st);
    return RD_OK;
}
static void slice_u8(rd_demod *h, const rd_slot &sl, long seen_before) {
    const rd_layout lay = demod_layout(h, seen_before);
    rd_launch_slice(lay, h->d_win[h->cur_win], ((size_t)h->dc.L + 31) / 32, (long)h->dc.L, h->dc, h->d_matches, h->match_cap, 0, 0,
                    (int)seen_before, nullptr, sl.dev<rd_packet>(SL_RECS), h->d_cnt, h->st);
    if (sl.parse) rd_launch_stream_parse(lay, h->dc, sl.dev<rd_packet>(SL_RECS), h->match_cap, sl.dev<int32_t>(SL_FE), h->d_cnt, h->st);
}
static void slice_cplx(rd_demod *h, const rd_slot &sl, long seen_before) {
    const rd_cplx_layout lay = demod_clayout(h, seen_before);
    rd_launch_cplx_slice(lay, h->d_win[h->cur_win], (long)h->dc.L, h->dc, h->d_matches, h->match_cap, (int)seen_before, nullptr,
                         sl.dev<rd_packet>(SL_RECS), h->d_cnt, h->st);
    if (sl.parse) rd_launch_cplx_stream_parse(lay, h->dc, sl.dev<rd_packet>(SL_RECS), h->match_cap, sl.dev<int32_t>(SL_FE), h->d_cnt, h->st);
}
static const multi_form k_multi_u8 = {roll_u8, bits_u8, slice_u8}, k_multi_cplx = {roll_cplx, bits_cplx, slice_cplx};

// The multi-launch form: the block into the slot's staging buffer - from `dev_block` (device memory, its producer ran on
// the compute stream) or from `in_host` on the copy stream - and everything else behind it on the compute stream.
static int submit_multi(rd_demod *h, rd_slot &sl, const uint8_t *in_host, const uint8_t *dev_block, size_t nbytes, int is_complex) {
    const size_t B = (size_t)h->dc.B, L = (size_t)h->dc.L;
    hipStream_t st = h->st;
    if (dev_block) {
        HIPCHK(hipMemcpyAsync(sl.d_in, dev_block, nbytes, hipMemcpyDeviceToDevice, st));
    } else {
        HIPCHK(hipMemcpyAsync(sl.d_in, in_host, nbytes, hipMemcpyHostToDevice, h->st_copy));
        HIPCHK(hipEventRecord(sl.e_in, h->st_copy));
        HIPCHK(hipStreamWaitEvent(st, sl.e_in, 0));
    }
    if (is_complex && !h->cplx_mode) {
        int rc = demod_enter_cplx(h);
        if (rc) return rc;
    }
    const multi_form &form = h->cplx_mode ? k_multi_cplx : k_multi_u8;
    const long seen_before = h->seen;
    int rc = form.roll(h, sl, is_complex, seen_before);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(h->d_cnt, 0, RD_CNT_TOTAL * 4, st));
    if ((rc = form.bits(h, seen_before))) return rc;
    // quantized <- roll(quantized, -B) with the new bits at the end (py:157,163-166)
    const int nw = h->cur_win ^ 1;
    rd_launch_window_update(h->d_win[nw], h->d_win[h->cur_win], (long)L, h->d_blockbits, (long)B, h->NS, (L + 31) / 32, (B + 31) / 32, st);
    h->cur_win = nw;
    // whole-buffer search, keep q <= B (py:171-188,194)
    rd_launch_search(h->d_win[nw], (L + 31) / 32, h->NS, (long)L, 0, (long)B, h->dc, h->d_matches, h->match_cap, h->d_cnt, st);
    form.slice(h, sl, seen_before);
    HIPCHK(hipGetLastError());
    // The counters come back with the block; the few records of a block are written by the slice
    // kernel straight into pinned host memory (no copy to wait for; for the thousands of records of
    // a batch run the same was measured slower than a device buffer + one copy).
    HIPCHK(hipMemcpyAsync(sl.h_cnt, h->d_cnt, RD_CNT_SLOTS * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(sl.e_done, st));
    h->seen = seen_before + 1;
    h->nflight++;
    return RD_OK;
}

// Queue one block per stream (uint8: NS x 2B bytes, stream-major; complex128: single stream only).  Returns at once; at
// most two blocks may be in flight.  Decide where the block's bytes are, then try the launch forms:
// `ext_off` >= 0: the block lies at that offset of the registered producer buffer (no copy: the kernels read it there)
// `dev_block`: the block lies in device memory, written by work queued on h->st before this call (rd_demod_submit_device)
// else `samples` goes into device memory by the host's own stores (see rd_api.hip: host push) where a one-launch form
// will read it, and into the pinned slot otherwise.
static int demod_submit(rd_demod *h, const void *samples, int is_complex, long ext_off = -1,
                        const uint8_t *dev_block = nullptr) {
    const size_t B = (size_t)h->dc.B, NS = (size_t)h->NS;
    int rc = demod_alloc(h);
    if (rc) return rc;
    if (h->stale && (rc = demod_drop_stale(h))) return rc;
    if (h->nflight >= 2) return rd_fail_msg(RD_ERR_STATE, "two blocks in flight: rd_demod_fetch one first");
    rd_slot &sl = h->slot[(h->head + h->nflight) & 1];
    const size_t nbytes = is_complex ? 2 * B * sizeof(double) : NS * 2 * B;
    const bool cplx = is_complex || h->cplx_mode;
    const bool one_cplx = h->one_ok && cplx && NS == 1 && h->dc.B <= 8192, one_u8 = h->one_ok && !cplx;
    const uint8_t *in_host = sl.m[SL_IN].h, *in_dev = sl.m[SL_IN].d;   // where this block's bytes are, host and device address
    bool pushed = false;
    if (dev_block) {
        in_dev = dev_block;
    } else if (ext_off >= 0) {
        in_host = h->ext_host + ext_off;
        in_dev = h->ext_dev + ext_off;
    } else if ((one_cplx || one_u8) && sl.d_push) {
        // stores out of the write-combining buffers, then the HDP flush, then - in posted order behind both - the
        // launch's doorbell
        memcpy(sl.d_push, samples, nbytes);
        _mm_sfence();
        *h->hdp_flush = 1u;
        in_dev = sl.d_push;
        pushed = true;
    } else {
        memcpy(sl.m[SL_IN].h, samples, nbytes);
    }
    sl.one = false;
    sl.parse = h->parse;
    if (one_cplx && ((rc = submit_one_cplx(h, sl, in_dev, is_complex)) || sl.one)) return rc;
    if (one_u8 && ((rc = submit_one_u8(h, sl, in_dev)) || sl.one)) return rc;
    if (pushed) memcpy(sl.m[SL_IN].h, samples, nbytes);   // (the one-launch form declined: the multi-launch form copies from the pinned slot)
    return submit_multi(h, sl, in_host, dev_block, nbytes, is_complex);
}

// what the last fetch kept, into the caller's array: the count always, RD_ERR_CAPACITY (`room`) when cap is too small
template <class T> static int demod_give(const std::vector<T> &kept, const char *room, T *out, int cap, int *n) {
    *n = (int)kept.size();
    if ((int)kept.size() > cap) return rd_fail_msg(RD_ERR_CAPACITY, room, kept.size());
    if (!kept.empty()) {
        if (!out) return rd_fail_msg(RD_ERR_ARG, "null out");
        memcpy(out, kept.data(), kept.size() * sizeof(T));
    }
    return RD_OK;
}
static int demod_give(rd_demod *h, rd_packet *out, int cap, int *n) {
    return demod_give(h->last, "need room for %zu packets (rd_demod_refetch returns them)", out, cap, n);
}

// Wait (polling) for the oldest block in flight and return its packets in the reference's order; its messages
// (rd_demod_parsed) are kept beside them.
static int demod_fetch(rd_demod *h, rd_packet *out, int cap, int *n) {
    if (h->nflight == 0) return rd_fail_msg(RD_ERR_STATE, "no block in flight");
    rd_slot &sl = h->slot[h->head];
    if (h->stale) return rd_fail_msg(RD_ERR_STATE, "the blocks in flight were given up on (their fetch timed out): submit the next block or reset()");
    int rc = demod_wait_slot(h, sl);
    if (rc) {  // every block in flight is dropped: the next submit / reset waits for them and discards their packets
        if (rc == RD_ERR_DEVICE) h->stale = h->nflight;
        return rc;
    }
    h->head ^= 1;
    h->nflight--;
    // one-launch form: a count and B + 1 record places per stream; multi-launch form: one record per match (no call
    // overlap here), match_cap places
    const int32_t *fe = sl.parse ? sl.host<int32_t>(SL_FE) : nullptr;
    if (sl.one) rd_collect_block(sl.host<uint32_t>(SL_SB), (size_t)h->NS, (size_t)h->dc.B + 1, sl.host<rd_packet>(SL_RECS), fe, h->dc.S,
                                 h->collect, h->last, h->last_parsed);
    else rd_collect_block(&sl.h_cnt[RD_CNT_MATCH], 1, h->match_cap, sl.host<rd_packet>(SL_RECS), fe, h->dc.S, h->collect, h->last, h->last_parsed);
    h->fetched = true;
    h->last_parse = sl.parse;
    return demod_give(h, out, cap, n);
}

// "Is this block the right size for this handle" (py:32-36 / py:145-149), what every entry point refuses before any device
// work, in this order.  blocks_call: rd_demod_blocks, which says "bytes" and takes no handle in complex mode - the other
// entry points refuse only a multi-stream one.
static int demod_check_block(const rd_demod *h, int is_complex, size_t count, bool blocks_call = false) {
    const size_t NS = (size_t)h->NS;
    size_t want = 0;
    if (is_complex && NS != 1) return rd_fail_msg(RD_ERR_STATE, "complex input needs a single-stream handle");
    if (rd_check_block_count(is_complex, count, (size_t)h->dc.B, NS, &want) != RD_OK)
        return rd_fail_msg(RD_ERR_ARG, blocks_call ? "Incompatible array sizes: got %zu bytes, expected %zu" : "Incompatible array sizes: got %zu, expected %zu",
                           count, want);
    if (!is_complex && h->cplx_mode && (NS != 1 || blocks_call)) return rd_fail_msg(RD_ERR_STATE, "handle is in complex mode: reset() first");
    return RD_OK;
}

extern "C" int rd_demod_submit(rd_demod *h, const void *samples, size_t count, int is_complex) {
    if (!h || !samples) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = demod_check_block(h, is_complex, count);
    return rc ? rc : demod_submit(h, samples, is_complex);
}

// Zero-copy input (the pinned ring that replaces the pickled-ndarray queue hop,
// /root/reference/src/rtldavis/runners/rtlsdr.py:100-103 -> /root/reference/src/rtldavis/worker.py:37).
extern "C" int rd_demod_register_input(rd_demod *h, void *host, size_t nbytes) {
    if (!h) return rd_fail_msg(RD_ERR_ARG, "null handle");
    int rc = demod_alloc(h);
    if (rc) return rc;
    if (h->nflight) return rd_fail_msg(RD_ERR_STATE, "%d block(s) in flight: fetch them before the input buffer changes", h->nflight);
    if (h->ext_host) {
        HIPCHK(hipHostUnregister(h->ext_host));
        h->ext_host = h->ext_dev = nullptr;
        h->ext_bytes = 0;
    }
    if (!host || nbytes == 0) return RD_OK;  // (unregister only)
    if ((uintptr_t)host % 16) return rd_fail_msg(RD_ERR_ARG, "the input buffer must be 16-byte aligned");
    HIPCHK(hipHostRegister(host, nbytes, hipHostRegisterMapped | hipHostRegisterPortable));
    void *dev = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&dev, host, 0);
    if (e != hipSuccess) {
        hipHostUnregister(host);
        return rd_fail_msg(RD_ERR_DEVICE, "hipHostGetDevicePointer: %s", hipGetErrorString(e));
    }
    h->ext_host = (uint8_t *)host;
    h->ext_dev = (uint8_t *)dev;
    h->ext_bytes = nbytes;
    return RD_OK;
}

extern "C" int rd_demod_input_mode(rd_demod *h) {
    if (!h) return rd_fail_msg(RD_ERR_ARG, "null handle");
    int rc = demod_alloc(h);
    if (rc) return rc;
    return h->slot[0].d_push && h->slot[1].d_push ? 1 : 0;
}

extern "C" int rd_demod_submit_from(rd_demod *h, size_t offset, size_t count, int is_complex) {
    if (!h) return rd_fail_msg(RD_ERR_ARG, "null handle");
    if (!h->ext_host) return rd_fail_msg(RD_ERR_STATE, "no input buffer registered (rd_demod_register_input)");
    int rc = demod_check_block(h, is_complex, count);
    if (rc) return rc;
    const size_t B = (size_t)h->dc.B, nbytes = is_complex ? 2 * B * sizeof(double) : (size_t)h->NS * 2 * B;
    if (offset % 16 || offset > h->ext_bytes || nbytes > h->ext_bytes - offset)
        return rd_fail_msg(RD_ERR_ARG, "block at offset %zu (%zu bytes) does not lie 16-byte aligned inside the registered buffer (%zu bytes)",
                           offset, nbytes, h->ext_bytes);
    return demod_submit(h, nullptr, is_complex, (long)offset);
}

extern "C" int rd_demod_fetch(rd_demod *h, rd_packet *out, int cap, int *n) {
    if (!h || !n) return rd_fail_msg(RD_ERR_ARG, "null argument");
    return demod_fetch(h, out, cap, n);
}

extern "C" int rd_demod_refetch(rd_demod *h, rd_packet *out, int cap, int *n) {
    if (!h || !n) return rd_fail_msg(RD_ERR_ARG, "null argument");
    return demod_give(h, out, cap, n);
}

extern "C" int rd_demod_inflight(rd_demod *h) { return h ? h->nflight : 0; }

// Parser.parse's front half inside the streaming kernels (no device work here: safe before fork)
extern "C" int rd_demod_set_parse(rd_demod *h, int enabled) {
    if (!h) return rd_fail_msg(RD_ERR_ARG, "null handle");
    if (h->nflight) return rd_fail_msg(RD_ERR_STATE, "%d block(s) in flight: rd_demod_fetch them before parse is switched", h->nflight);
    h->parse = enabled != 0;
    return RD_OK;
}

extern "C" int rd_demod_parsed(rd_demod *h, rd_parsed *out, int cap, int *n) {
    if (!h || !n) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (!h->fetched) return rd_fail_msg(RD_ERR_STATE, "no block fetched since create / reset");
    if (!h->last_parse) return rd_fail_msg(RD_ERR_STATE, "the last fetched block was submitted with parse off (rd_demod_set_parse)");
    return demod_give(h->last_parsed, "need room for %zu messages", out, cap, n);
}

// ------------------------------------------------------------------------------------------
// internal entry points of the wideband receiver (rd_internal.h, rd_wideband.hip)
// ------------------------------------------------------------------------------------------
int rd_demod_prepare(rd_demod *h, hipStream_t *st, hipStream_t *st_copy) {
    if (!h || !st || !st_copy) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = demod_alloc(h);
    if (rc) return rc;
    *st = h->st;
    *st_copy = h->st_copy;
    return RD_OK;
}

int rd_demod_check_room(rd_demod *h) {
    if (!h) return rd_fail_msg(RD_ERR_ARG, "null handle");
    int rc = demod_alloc(h);
    if (rc) return rc;
    if (h->stale && (rc = demod_drop_stale(h))) return rc;
    if (h->nflight >= 2) return rd_fail_msg(RD_ERR_STATE, "two blocks in flight: fetch one first");
    return RD_OK;
}

int rd_demod_submit_device(rd_demod *h, const uint8_t *dev_block) {
    if (!h || !dev_block) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (h->cplx_mode) return rd_fail_msg(RD_ERR_STATE, "handle is in complex mode: reset() first");
    return demod_submit(h, nullptr, 0, -1, dev_block);
}

int rd_demod_pending(const rd_demod *h) { return h ? h->nflight - h->stale : 0; }

// ------------------------------------------------------------------------------------------
// synchronous calls and state accessors
// ------------------------------------------------------------------------------------------
static int demod_blocks(rd_demod *h, const void *samples, int is_complex, rd_packet *out, int cap, int *n) {
    int rc = demod_quiet(h);
    if (rc) return rc;
    rc = demod_submit(h, samples, is_complex);
    if (rc) return rc;
    return demod_fetch(h, out, cap, n);
}

extern "C" int rd_demod_block(rd_demod *h, const void *samples, size_t count, int is_complex, rd_packet *out, int cap,
                              int *n) {
    if (!h || !samples || !n) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (h->NS != 1) return rd_fail_msg(RD_ERR_STATE, "handle holds %d streams: use rd_demod_blocks", h->NS);
    int rc = demod_check_block(h, is_complex, count);
    return rc ? rc : demod_blocks(h, samples, is_complex, out, cap, n);
}

extern "C" int rd_demod_blocks(rd_demod *h, const uint8_t *iq, size_t nbytes, rd_packet *out, int cap, int *n) {
    if (!h || !iq || !n) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = demod_check_block(h, 0, nbytes, true);
    return rc ? rc : demod_blocks(h, iq, 0, out, cap, n);
}

// nbytes at device address `src` through the pinned mirror (no staging, polling wait) to `out`
static int demod_mirror_out(rd_demod *h, const void *src, void *out, size_t nbytes) {
    int rc = rd_copy_d2h(h->h_tmp, src, nbytes, h->st);
    if (rc) return rc;
    memcpy(out, h->h_tmp, nbytes);
    return RD_OK;
}

// A state mirror of a quiet handle: `launch` computes it into d_tmp on the compute stream.  All zeros before the first
// block (py:134).
template <class Launch> static int demod_state_out(rd_demod *h, void *out, size_t nbytes, Launch launch) {
    if (h->seen == 0) {
        memset(out, 0, nbytes);
        return RD_OK;
    }
    int rc = demod_quiet(h);
    if (rc) return rc;
    launch(h->seen - 1);
    HIPCHK(hipGetLastError());
    return demod_mirror_out(h, h->d_tmp, out, nbytes);
}

extern "C" int rd_copy_discriminated_stream(rd_demod *h, int stream, double *out, size_t n) {
    if (!h || !out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (stream < 0 || stream >= h->NS) return rd_fail_msg(RD_ERR_ARG, "stream out of range");
    const long B = h->dc.B;
    if (n != 2 * (size_t)B) return rd_fail_msg(RD_ERR_ARG, "discriminated has %zu elements", 2 * (size_t)B);
    // discriminated = d over [-B, B) relative to the newest block (py:156,162)
    return demod_state_out(h, out, n * sizeof(double), [=](long seen_before) {
        if (!h->cplx_mode) rd_launch_disc(demod_layout(h, seen_before), stream, -B, 2 * B, h->d_tmp, h->st);
        else rd_launch_cplx_disc(demod_clayout(h, seen_before), -B, 2 * B, h->d_tmp, h->st);
    });
}

extern "C" int rd_copy_discriminated(rd_demod *h, double *out, size_t n) { return rd_copy_discriminated_stream(h, 0, out, n); }

extern "C" int rd_copy_filtered(rd_demod *h, double *out_interleaved, size_t n_complex) {
    if (!h || !out_interleaved) return rd_fail_msg(RD_ERR_ARG, "null argument");
    const long B = h->dc.B;
    if (n_complex != (size_t)B + 1) return rd_fail_msg(RD_ERR_ARG, "filtered has %zu elements", (size_t)B + 1);
    // filtered[j] = f[j-1] relative to the newest block (py:155,161)
    return demod_state_out(h, out_interleaved, 2 * n_complex * sizeof(double), [=](long seen_before) {
        if (!h->cplx_mode) rd_launch_filtered(demod_layout(h, seen_before), 0, -1, B + 1, h->d_tmp, h->st);
        else rd_launch_cplx_filtered(demod_clayout(h, seen_before), -1, B + 1, h->d_tmp, h->st);
    });
}

extern "C" int rd_copy_quantized(rd_demod *h, uint8_t *out, size_t n) {
    if (!h || !out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    const size_t L = (size_t)h->dc.L;
    if (n != L) return rd_fail_msg(RD_ERR_ARG, "quantized has %zu elements", L);
    if (!h->dev_ready) {  // py:135 zeros
        memset(out, 0, n);
        return RD_OK;
    }
    std::vector<uint32_t> words((L + 31) / 32);
    if (words.size() * 4 > 2 * (2 * (size_t)h->dc.B + 2) * sizeof(double)) return rd_fail_msg(RD_ERR_ARG, "window too large");
    int rc = demod_quiet(h);
    if (rc) return rc;
    rc = demod_mirror_out(h, h->d_win[h->cur_win], words.data(), words.size() * 4);
    if (rc) return rc;
    for (size_t t = 0; t < L; t++) out[t] = (uint8_t)((words[t >> 5] >> (t & 31)) & 1u);  // unpack only
    return RD_OK;
}
