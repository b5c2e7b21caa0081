// rd_burst_clips.hip - the channelized IQ bytes of every burst, cut out on the device (include/rtldavis_hip.h, BURST CLIPS).
// k_chan_bursts, k_chan_burst_decode, k_chan_burst_expect and k_chan_burst_search write their records into mapped slots;
// this kernel is launched behind the last of them on the same stream, reads the records back the way k_chan_burst_decode
// reads the slot k_chan_bursts filled, and copies the outputs each record names - with a pre- and a post-roll - out of the
// two channelized chunks into a mapped slot of its own.  The kernels in front stay what they were.  Used by rd_wideband.hip
// per streamed chunk (rd_wb_set_burst_clips).
//
// Kernel.  One workgroup of 256 threads per channel c; nothing crosses workgroups, no atomics.
//   1. counts.  Thread 0 fetches the channel's run count (the floor record), its decode header, the previous chunk's owed;
//      threads 0 .. n_search - 1 the search headers of (centre, c).  System-scope loads into LDS.
//   2. the list.  The channel's possible requests have fixed places: 0 the tail, then the runs, the decode rows, the expect
//      table's entries, the search places (centre, place).  They are taken RD_BURST_THREADS at a time: lane j evaluates
//      place base + j - loads the record's few words, applies the skip rules and rd_bc_window_of (rd_host.h) - and leaves
//      (valid, source, t0, n, flags, ref, e - B) in LDS; then thread 0 walks the batch in order and allocates: a request is
//      written as a record at offset = used, or dropped whole when used + n > Q or RD_BC_PER records are written.  The
//      order is the definition's, whatever the grid: the same bits on every run.
//   3. thread 0 writes the header; the records' (t0, n, offset) stay in LDS.
//   4. the copy.  All lanes copy the clips' 16-byte vectors from cur (t >= 0) or prev (t < 0: output t + B of the chunk
//      before) into the pool.  t0 and n are multiples of 8 and so are lo_lim and B: a vector lies in one chunk and inside
//      it; lo_lim <= t0, t0 + n <= B and offset + n <= Q by steps 2 and rd_bc_window_of, whatever the records say.
// LDS: 7 words per lane of a batch and 3 per record: under 10 KiB.
#include <cstddef>

#include <hip/hip_runtime.h>

#include "rd_burst_common.h"

static_assert(sizeof(rd_burst_clip) == 48 && sizeof(rd_bc_header) == 24, "the record and header layouts of the slot");
static_assert(RD_BC_MAX_ROLL % 8 == 0 && RD_BC_MAX_QUOTA % 8 == 0 && RD_BU_WINDOW % 8 == 0, "whole 16-byte vectors");
static_assert(RD_BS_MAX_CENTRES <= RD_BURST_THREADS && RD_BC_PER <= RD_BURST_THREADS, "one thread per search header");

struct rd_bc_params {
    int sl, n_sym;             // SL, N (read with RD_BC_MESSAGES only)
    int block;                 // B
    int n_ch;
    int sources, pre, post, quota;
    int n_expect, n_search;    // 0: that kernel was not launched
    uint32_t cap;              // record places per channel of the burst and decode slots
    uint32_t chunk;
    uint64_t clock;            // K
};

struct rd_bc_request {
    int32_t valid, source;
    int64_t a, e;
    uint64_t ref;
};

// the request of a message row, or none: its channel field is c and its packet lies inside the two chunks
__device__ __forceinline__ void rd_bc_row_request(const rd_burst_msg *m, int c, const rd_bc_params &P, int have_prev, int source,
                                                  rd_bc_request &q) {
    const int32_t ch = rd_bd_sys_load(&m->channel);
    const int64_t tau = (int64_t)rd_bd_sys_load(&m->tau);
    rd_bq_windows w;
    if (ch != c || !rd_bq_windows_of(P.sl, P.n_sym, P.block, have_prev, tau, 0, &w)) return;
    q.valid = 1;
    q.source = source;
    q.a = (int64_t)w.p0 - P.pre;
    q.e = (int64_t)w.p1 + P.post;
    q.ref = rd_bd_sys_load(&m->time);
}

__global__ __launch_bounds__(RD_BURST_THREADS) void k_chan_burst_clips(const uint8_t *__restrict__ cur, const uint8_t *__restrict__ prev,
                                                                    size_t ch_stride, rd_bc_params P, const rd_burst *runs,
                                                                    const rd_burst_floor *floor, const rd_burst_msg *d_recs,
                                                                    const rd_bd_header *d_hdr, const rd_burst_msg *x_recs,
                                                                    const rd_bx_header *x_hdr, const rd_burst_msg *s_recs,
                                                                    const rd_bs_header *s_hdr, const rd_bc_header *prev_hdr,
                                                                    rd_burst_clip *clips, rd_bc_header *hdr, uint8_t *pool) {
    __shared__ int32_t s_valid[RD_BURST_THREADS], s_src[RD_BURST_THREADS], s_t0[RD_BURST_THREADS], s_n[RD_BURST_THREADS];
    __shared__ int32_t s_fl[RD_BURST_THREADS], s_over[RD_BURST_THREADS];
    __shared__ uint64_t s_ref[RD_BURST_THREADS];
    __shared__ int32_t s_ct0[RD_BC_PER], s_cn[RD_BC_PER], s_coff[RD_BC_PER];   // the records written
    __shared__ uint32_t s_cnt[4 + RD_BS_MAX_CENTRES];     // runs, decode rows, owed of the chunk before, records; search rows
    const int c = (int)blockIdx.x;
    const unsigned tid = threadIdx.x;
    const int have_prev = prev ? 1 : 0;
    const bool want_runs = (P.sources & (int)RD_BC_RUNS) != 0, want_msgs = (P.sources & (int)RD_BC_MESSAGES) != 0;
    // ---- 1. counts
    if (tid == 0u) {
        uint32_t nr = want_runs && floor ? rd_bd_sys_load(&floor[c].n_bursts) : 0u;
        uint32_t nd = want_msgs && d_hdr ? rd_bd_sys_load(&d_hdr[c].n_msgs) : 0u;
        uint32_t ow = prev_hdr ? rd_bd_sys_load(&prev_hdr[c].owed) : 0u;
        s_cnt[0] = nr < P.cap ? nr : P.cap;               // (a place past the channel's ceil(nW / 2) is never written)
        s_cnt[1] = nd < P.cap ? nd : P.cap;
        s_cnt[2] = ow <= (uint32_t)RD_BC_MAX_ROLL ? ow : 0u;
        s_cnt[3] = 0u;
    }
    if (tid < (unsigned)RD_BS_MAX_CENTRES) {
        uint32_t ns = 0u;
        if (want_msgs && s_hdr && (int)tid < P.n_search) ns = rd_bd_sys_load(&s_hdr[(size_t)tid * (size_t)P.n_ch + (size_t)c].n_msgs);
        s_cnt[4 + tid] = ns < (uint32_t)RD_BS_PER ? ns : (uint32_t)RD_BS_PER;
    }
    __syncthreads();
    const int n_runs = (int)s_cnt[0], n_dec = (int)s_cnt[1], owed_in = (int)s_cnt[2];
    const int n_exp = want_msgs && x_hdr ? P.n_expect : 0, n_sea = want_msgs && s_hdr ? P.n_search * RD_BS_PER : 0;
    const int i_run = 1, i_dec = i_run + n_runs, i_exp = i_dec + n_dec, i_sea = i_exp + n_exp, total = i_sea + n_sea;
    const int nW = P.block / RD_BU_WINDOW;
    // ---- 2. the list, a batch at a time (every bound is workgroup-uniform)
    uint32_t n_clips = 0u, dropped = 0u, used = 0u, owed = 0u;   // (thread 0's)
    for (int base = 0; base < total; base += RD_BURST_THREADS) {
        const int i = base + (int)tid;
        rd_bc_request q;
        q.valid = 0;
        q.source = 0;
        q.a = q.e = 0;
        q.ref = 0ull;
        if (i == 0) {
            if (owed_in > 0) {
                q.valid = 1;
                q.e = owed_in;
            }
        } else if (i < i_dec) {
            const rd_burst *r = &runs[(size_t)c * P.cap + (size_t)(i - i_run)];
            const uint32_t first = rd_bd_sys_load(&r->first), windows = rd_bd_sys_load(&r->windows);
            if (windows != 0u && first < (uint32_t)nW && windows <= (uint32_t)nW - first) {   // (else k_chan_bursts never writes it)
                q.valid = 1;
                q.source = 1;
                q.a = (int64_t)RD_BU_WINDOW * first - P.pre;
                q.e = (int64_t)RD_BU_WINDOW * ((int64_t)first + windows) + P.post;
                q.ref = first;
            }
        } else if (i < i_exp) {
            rd_bc_row_request(&d_recs[(size_t)c * P.cap + (size_t)(i - i_dec)], c, P, have_prev, 2, q);
        } else if (i < i_sea) {
            const int x = i - i_exp;
            if (rd_bd_sys_load(&x_hdr[x].n_msgs) == 1u) rd_bc_row_request(&x_recs[x], c, P, have_prev, 3, q);
        } else if (i < total) {
            const int ci = (i - i_sea) / RD_BS_PER, place = (i - i_sea) % RD_BS_PER;
            if ((uint32_t)place < s_cnt[4 + ci])
                rd_bc_row_request(&s_recs[((size_t)ci * (size_t)P.n_ch + (size_t)c) * RD_BS_PER + (size_t)place], c, P, have_prev, 4, q);
        }
        rd_bc_clamped w = {0, 0, 0};
        const bool ok = q.valid && rd_bc_window_of(P.block, have_prev, q.a, q.e, &w);
        __syncthreads();                                  // the batch before has been read out of LDS
        s_valid[tid] = ok ? 1 : 0;
        s_src[tid] = q.source;
        s_t0[tid] = w.t0;
        s_n[tid] = w.n;
        s_fl[tid] = w.flags;
        s_over[tid] = ok && (w.flags & RD_BC_CUT_END) ? (int32_t)(q.e - (int64_t)P.block) : 0;   // (1 .. RD_BC_MAX_ROLL by the rules above)
        s_ref[tid] = q.ref;
        __syncthreads();
        if (tid == 0u) {
            const int m = min(RD_BURST_THREADS, total - base);
            for (int j = 0; j < m; j++) {
                if (!s_valid[j]) continue;
                const uint32_t n = (uint32_t)s_n[j];
                if (n_clips >= (uint32_t)RD_BC_PER || used + n > (uint32_t)P.quota) {
                    dropped++;
                    continue;
                }
                rd_burst_clip *k = &clips[(size_t)c * RD_BC_PER + n_clips];   // field by field: no private copy of the record
                k->channel = c;
                k->source = (uint32_t)s_src[j];
                k->flags = (uint32_t)s_fl[j];
                k->t0 = s_t0[j];
                k->n = n;
                k->offset = used;
                k->time = P.clock + (uint64_t)(int64_t)s_t0[j];
                k->ref = s_ref[j];
                k->chunk = P.chunk;
                k->pad = 0u;
                s_ct0[n_clips] = s_t0[j];
                s_cn[n_clips] = (int32_t)n;
                s_coff[n_clips] = (int32_t)used;
                n_clips++;
                used += n;
                if ((uint32_t)s_over[j] > owed) owed = (uint32_t)s_over[j];
            }
        }
    }
    // ---- 3. the header
    if (tid == 0u) {
        rd_bc_header *h = &hdr[c];
        h->n_clips = n_clips;
        h->dropped = dropped;
        h->owed = owed < (uint32_t)RD_BC_MAX_ROLL ? owed : (uint32_t)RD_BC_MAX_ROLL;
        h->used = used;
        h->chunk = P.chunk;
        h->pad = 0u;
        s_cnt[3] = n_clips;
    }
    __syncthreads();
    // ---- 4. the copy: clip k's vector v is outputs t0 + 8 v .. t0 + 8 v + 7
    const uint8_t *src = cur + (size_t)c * ch_stride;
    const uint8_t *src_prev = prev ? prev + (size_t)c * ch_stride : nullptr;
    uint4 *dst = (uint4 *)(pool + (size_t)c * 2 * (size_t)P.quota);
    const int nk = (int)s_cnt[3];
    for (int k = 0; k < nk; k++) {
        const int t0 = s_ct0[k], nv = s_cn[k] / 8, ov = s_coff[k] / 8;
        for (int v = (int)tid; v < nv; v += RD_BURST_THREADS) {
            const int t = t0 + 8 * v;
            const uint8_t *g = t < 0 ? src_prev + 2 * ((long)t + (long)P.block) : src + 2 * (long)t;   // (t < 0 only with prev: lo_lim)
            dst[ov + v] = *(const uint4 *)g;
        }
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
int rd_burst_clips_check(int n_ch, int sources, int pre, int post, int quota) {
    if (sources < 0 || (sources & ~(int)(RD_BC_RUNS | RD_BC_MESSAGES)))
        return rd_fail_msg(RD_ERR_ARG, "burst clips: sources %d, not a mask of RD_BC_RUNS | RD_BC_MESSAGES", sources);
    if (pre < 0 || pre > RD_BC_MAX_ROLL || (pre & 7) || post < 0 || post > RD_BC_MAX_ROLL || (post & 7))
        return rd_fail_msg(RD_ERR_ARG, "burst clips: pre %d, post %d, not multiples of 8 in 0 .. %d", pre, post, RD_BC_MAX_ROLL);
    if (quota < 8 || quota > RD_BC_MAX_QUOTA || (quota & 7))
        return rd_fail_msg(RD_ERR_ARG, "burst clips: quota %d, not a multiple of 8 in 8 .. %d", quota, RD_BC_MAX_QUOTA);
    if (n_ch < 1 || (uint64_t)n_ch * (uint64_t)quota * 2ull > (uint64_t)RD_BC_MAX_POOL)
        return rd_fail_msg(RD_ERR_ARG, "burst clips: %d channels x quota %d x 2 bytes, more than %u", n_ch, quota, RD_BC_MAX_POOL);
    return RD_OK;
}

int rd_burst_clips_launch(const rd_config *cfg, const uint8_t *chan_out, const uint8_t *chan_prev, size_t out_stride, int n_ch,
                          size_t n_out, uint64_t clock, uint64_t seq, int sources, int pre, int post, int quota,
                          const void *burst_slot, const void *decode_slot, const void *expect_slot, int n_expect,
                          const void *search_slot, int n_search, const rd_bc_header *prev_hdr, void *slot, hipStream_t st) {
    int rc = rd_burst_clips_check(n_ch, sources, pre, post, quota);
    if (rc) return rc;
    if (!sources) return rd_fail_msg(RD_ERR_ARG, "burst clips: no source");
    if (!cfg || !chan_out || !burst_slot || !slot) return rd_fail_msg(RD_ERR_ARG, "burst clips: null argument");
    if ((rc = rd_bursts_check(n_out))) return rc;
    const bool msgs = (sources & (int)RD_BC_MESSAGES) != 0;
    if (msgs && (rc = rd_burst_decode_check(cfg))) return rc;
    if (n_expect < 0 || n_expect > RD_BX_MAX || n_search < 0 || n_search > RD_BS_MAX_CENTRES || (n_expect > 0 && !expect_slot) ||
        (n_search > 0 && !search_slot))
        return rd_fail_msg(RD_ERR_ARG, "burst clips: %d expectations, %d centres, or a slot missing", n_expect, n_search);
    if (n_out != (size_t)cfg->block_size || out_stride < 2 * n_out || (out_stride & 15) || ((uintptr_t)chan_out & 15) ||
        ((uintptr_t)chan_prev & 15) || ((uintptr_t)slot & 15))
        return rd_fail_msg(RD_ERR_ARG, "burst clips: stride %zu for %zu outputs, or a misaligned buffer", out_stride, n_out);
    const size_t n_win = n_out / RD_BU_WINDOW;
    rd_bc_params P;
    P.sl = msgs ? cfg->symbol_length : 1;
    P.n_sym = msgs ? cfg->packet_symbols : 16;
    P.block = (int)n_out;
    P.n_ch = n_ch;
    P.sources = sources;
    P.pre = pre;
    P.post = post;
    P.quota = quota;
    P.n_expect = expect_slot ? n_expect : 0;
    P.n_search = search_slot ? n_search : 0;
    P.cap = (uint32_t)rd_bu_cap(n_win);
    P.chunk = (uint32_t)seq;
    P.clock = clock;
    const uint8_t *bu = (const uint8_t *)burst_slot, *bd = (const uint8_t *)decode_slot, *bx = P.n_expect ? (const uint8_t *)expect_slot : nullptr,
                  *bs = P.n_search ? (const uint8_t *)search_slot : nullptr;
    uint8_t *out = (uint8_t *)slot;
    hipLaunchKernelGGL(k_chan_burst_clips, dim3((unsigned)n_ch), dim3(RD_BURST_THREADS), 0, st, chan_out, chan_prev, out_stride, P,
                       (const rd_burst *)bu, (const rd_burst_floor *)(bu + rd_bu_floor_offset(n_ch, n_win)), (const rd_burst_msg *)bd,
                       bd ? (const rd_bd_header *)(bd + rd_bd_header_offset(n_ch, n_win)) : nullptr, (const rd_burst_msg *)bx,
                       bx ? (const rd_bx_header *)(bx + RD_BX_HEADER_OFFSET) : nullptr, (const rd_burst_msg *)bs,
                       bs ? (const rd_bs_header *)(bs + rd_bs_header_offset(n_ch)) : nullptr, prev_hdr, (rd_burst_clip *)out,
                       (rd_bc_header *)(out + rd_bc_header_offset(n_ch)), out + rd_bc_pool_offset(n_ch));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "k_chan_burst_clips: %s", hipGetErrorString(e));
    return RD_OK;
}

extern "C" size_t rd_bc_slot_size(int n_ch, int quota) { return n_ch < 1 || quota < 0 ? 0 : rd_bc_slot_bytes(n_ch, quota); }

// Test hook (tests/test_burst_clips.py): k_chan_burst_clips alone on host bytes and on the records the caller supplies,
// through rd_burst_clips_launch and mapped host slots as the receiver allocates them.  Slot 0 holds what the kernels in
// front would have written, one part behind the other (burst slot | decode slot | expect slot | search slot | the headers of
// the chunk before), each part on a multiple of 64 bytes; slot 1 is the clip slot, filled with 0xA5 and copied out whole.
extern "C" int rd_debug_burst_clips(const rd_config *cfg, const uint8_t *cur, const uint8_t *prev, size_t stride, int n_ch, uint64_t clock,
                                    uint64_t seq, const rd_burst *runs, const uint32_t *n_runs, const rd_burst_msg *msgs,
                                    const uint32_t *n_msgs, const rd_burst_msg *x_msgs, const uint32_t *x_hdr, int n_expect,
                                    const rd_burst_msg *s_msgs, const rd_bs_header *s_hdr, int n_search, const uint32_t *owed_prev,
                                    int sources, int pre, int post, int quota, uint8_t *out) {
    int rc = rd_burst_clips_check(n_ch < 1 ? 1 : n_ch, sources, pre, post, quota);
    if (rc) return rc;
    if (!sources) return rd_fail_msg(RD_ERR_ARG, "burst clips: no source");
    const bool want_msgs = (sources & (int)RD_BC_MESSAGES) != 0;
    if (!cfg || !cur || !out || n_ch < 1 || !runs || !n_runs || (want_msgs && (!msgs || !n_msgs)) || ((x_msgs || x_hdr) && !want_msgs) ||
        ((s_msgs || s_hdr) && !want_msgs))
        return rd_fail_msg(RD_ERR_ARG, "null argument");
    if ((n_expect != 0) != (x_msgs != nullptr) || (x_msgs != nullptr) != (x_hdr != nullptr) || n_expect < 0 || n_expect > RD_BX_MAX ||
        (n_search != 0) != (s_msgs != nullptr) || (s_msgs != nullptr) != (s_hdr != nullptr) || n_search < 0 || n_search > RD_BS_MAX_CENTRES)
        return rd_fail_msg(RD_ERR_ARG, "burst clips: %d expectations or %d centres without their rows and headers", n_expect, n_search);
    if (cfg->block_size < RD_BU_WINDOW || cfg->block_size % RD_BU_WINDOW)
        return rd_fail_msg(RD_ERR_ARG, "block_size %d is not a positive multiple of 128", cfg->block_size);
    const size_t n_out = (size_t)cfg->block_size, n_win = n_out / RD_BU_WINDOW, cap = rd_bu_cap(n_win);
    if ((rc = rd_bursts_check(n_out))) return rc;
    if (want_msgs && (rc = rd_burst_decode_check(cfg))) return rc;
    for (int c = 0; c < n_ch; c++)
        if (n_runs[c] > cap || (want_msgs && n_msgs[c] > cap))
            return rd_fail_msg(RD_ERR_ARG, "burst clips: more records in channel %d than its %zu places", c, cap);
    if (stride < 2 * n_out || (stride & 15)) return rd_fail_msg(RD_ERR_ARG, "burst clips: stride %zu for %zu outputs", stride, n_out);
    if ((rc = rd_ensure_device())) return rc;    // (no device work for a wrong argument)
    auto up = [](size_t v) { return (v + 63) & ~(size_t)63; };
    const size_t o_bu = 0, o_bd = up(o_bu + rd_bu_slot_bytes(n_ch, n_win)), o_bx = up(o_bd + rd_bd_slot_bytes(n_ch, n_win)),
                 o_bs = up(o_bx + RD_BX_SLOT_BYTES), o_ph = up(o_bs + rd_bs_slot_bytes(n_ch)),
                 in_bytes = o_ph + (size_t)n_ch * sizeof(rd_bc_header), bc_bytes = rd_bc_slot_bytes(n_ch, quota);
    rd_burst_dbg D;                                     // slot 0: what the kernels in front wrote, slot 1: the clip slot
    if ((rc = D.upload(cur, prev, (size_t)n_ch * stride)) || (rc = D.map(0, in_bytes)) || (rc = D.map(1, bc_bytes))) return rc;
    memcpy(D.slot[0] + o_bu, runs, (size_t)n_ch * cap * sizeof(rd_burst));
    rd_burst_floor *fl = (rd_burst_floor *)(D.slot[0] + o_bu + rd_bu_floor_offset(n_ch, n_win));
    for (int c = 0; c < n_ch; c++) {
        memset(&fl[c], 0, sizeof(rd_burst_floor));
        fl[c].n_bursts = n_runs[c];
        fl[c].chunk = (uint32_t)seq;
    }
    if (want_msgs) {
        memcpy(D.slot[0] + o_bd, msgs, (size_t)n_ch * cap * sizeof(rd_burst_msg));
        rd_bd_header *h = (rd_bd_header *)(D.slot[0] + o_bd + rd_bd_header_offset(n_ch, n_win));
        for (int c = 0; c < n_ch; c++) {
            h[c].n_msgs = n_msgs[c];
            h[c].long_runs = 0u;
            h[c].chunk = (uint32_t)seq;
            h[c].pad = 0u;
        }
    }
    if (x_msgs) {
        memcpy(D.slot[0] + o_bx, x_msgs, (size_t)RD_BX_MAX * sizeof(rd_burst_msg));
        memcpy(D.slot[0] + o_bx + RD_BX_HEADER_OFFSET, x_hdr, (size_t)RD_BX_MAX * sizeof(rd_bx_header));
    }
    if (s_msgs) {
        memcpy(D.slot[0] + o_bs, s_msgs, rd_bs_header_offset(n_ch));
        memcpy(D.slot[0] + o_bs + rd_bs_header_offset(n_ch), s_hdr, (size_t)RD_BS_MAX_CENTRES * (size_t)n_ch * sizeof(rd_bs_header));
    }
    if (owed_prev) {
        rd_bc_header *ph = (rd_bc_header *)(D.slot[0] + o_ph);
        for (int c = 0; c < n_ch; c++) {
            memset(&ph[c], 0, sizeof(rd_bc_header));
            ph[c].owed = owed_prev[c];
        }
    }
    const uint8_t *in = (const uint8_t *)D.d_slot[0];
    if ((rc = rd_burst_clips_launch(cfg, D.d_cur, D.d_prev, stride, n_ch, n_out, clock, seq, sources, pre, post, quota, in + o_bu,
                                    want_msgs ? in + o_bd : nullptr, x_msgs ? in + o_bx : nullptr, n_expect, s_msgs ? in + o_bs : nullptr,
                                    n_search, owed_prev ? (const rd_bc_header *)(in + o_ph) : nullptr, D.d_slot[1], nullptr)) ||
        (rc = D.sync()))
        return rc;
    memcpy(out, D.slot[1], bc_bytes);
    return RD_OK;
}
