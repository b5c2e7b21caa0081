// rd_burst_expect.hip - decode at the places the host expects a packet (include/rtldavis_hip.h, BURST EXPECT).
// k_chan_burst_decode needs a run of ON windows and slices around the run's own correlation sum; this kernel gets, per
// expectation, a channel, a range of candidate taus, the direction to slice around and the id to accept, and decodes there
// with no energy gate.  Used by rd_wideband.hip per streamed chunk (rd_wb_set_burst_expect), behind k_chan_burst_decode on
// the same stream.
//
// The host turns every rd_expect into an rd_bx_entry for the chunk's clock (rd_bx_range, rd_host.cpp): tau_a .. tau_b, or
// tau_a > tau_b for an expectation with no candidate in this chunk.  The entries travel in the mapped slot, behind the
// records and the headers; a launch is made only when one of them is active.
//
// Kernel.  One workgroup of 256 threads per expectation.  Region t0 = tau_a - SL, t1 = tau_b + SL (N - 1) + 1, at most
// 4096 outputs; t0 is no multiple of 8, so the bytes are loaded from L0 = the filter's first output (t0 without the
// filter) rounded DOWN to 8 up to its last rounded up - a 16-byte vector still lies in one chunk -, and everything
// behind the load indexes from t0: the outputs loaded in front of it enter neither p nor, beyond zf0 .. zf1, the
// filter, which gets the real samples of zf0 .. zf1 where a run of k_chan_burst_decode has zeros.  Then the region
// decoder of rd_burst_common.h, one lane per tau over tau_a .. tau_b only, and the winner's record.
// LDS: s (int64, 32 KiB), the bytes (8.25 KiB), y (16 KiB, narrow only) - less than the decode kernel's.  Plain vector
// stores into the mapped slot, no atomics.
#include <type_traits>

#include <hip/hip_runtime.h>

#include "rd_burst_common.h"

#define RD_BX_LEN (RD_BX_MAX_SPAN + RD_BD_MAX_LOOK_W * RD_BU_WINDOW)   // t1 - t0 at most: the span + N SL + 1
#define RD_BX_LOAD (RD_BX_LEN + 128)                                    // outputs loaded at most
static_assert(RD_BX_LEN + 2 * (RD_BD_NB_MAX_SL + 2) + 14 <= RD_BX_LOAD && RD_BX_LOAD % 8 == 0, "the filter's margins and the rounding to 8");
static_assert((RD_BX_LEN + RD_BD_NB_MAX_T - 1) * 4 <= RD_BX_LEN * 8, "the padded int16 region lies in s's place");
static_assert(sizeof(rd_bx_header) == 16 && sizeof(rd_bx_entry) == 32, "the slot layout of rd_bx_* (rd_internal.h)");

struct rd_bx_params {
    rd_bd_shape shape;
    int look;                  // LOOK
    int have_prev;
    int n_ch;
    uint64_t clock, seq;
};

template <bool REPAIR, bool NARROW>
__global__ __launch_bounds__(RD_BURST_THREADS) void k_chan_burst_expect(const uint8_t *__restrict__ cur, const uint8_t *__restrict__ prev,
                                                                        size_t ch_stride, size_t n_out, rd_bx_params P,
                                                                        const rd_bx_entry *tab, rd_burst_msg *recs, rd_bx_header *hdr,
                                                                        const uint32_t *__restrict__ nb_tab) {
    using f_t = std::conditional_t<NARROW, int64_t, int>;
    __shared__ int64_t s_s[RD_BX_LEN];                   // s[t0 + i] at i (i >= SL)
    __shared__ uint4 s_z[RD_BX_LOAD / 8];                // the loaded bytes: output L0 + i at bytes 2 i, 2 i + 1
    __shared__ uint64_t s_m[RD_BURST_THREADS / 64];
    __shared__ int s_t[RD_BURST_THREADS / 64];
    __shared__ f_t s_fr[RD_BURST_THREADS / 64], s_fi[RD_BURST_THREADS / 64];
    __shared__ int32_t s_ent[6];                         // the entry: channel, id, tau_a, tau_b, corr_re, corr_im
    __shared__ uint16_t s_E[8 * RD_BD_DATA_BYTES];       // (REPAIR) E[k], 16 <= k < N
    __shared__ uint32_t s_f[RD_BURST_THREADS / 64];      // (REPAIR) the waves' flips
    __shared__ uint32_t s_y[RD_BX_LEN];                  // (NARROW) y[t0 + i] at i: re in the low half, im in the high one
    __shared__ uint32_t s_hA[RD_BD_NB_MAX_T], s_hB[RD_BD_NB_MAX_T];   // (NARROW) H[g][kk - M] as (re, -im) and (im, re)
    const rd_bd_work W = {s_s, s_m, s_t, s_E, s_f, s_y, s_hA, s_hB};
    const int x = (int)blockIdx.x;
    const unsigned tid = threadIdx.x;
    if (tid == 0u) {                                     // one thread crosses the bus, the workgroup takes it from LDS
        s_ent[0] = rd_bd_sys_load(&tab[x].channel);
        s_ent[1] = (int32_t)rd_bd_sys_load(&tab[x].id);
        s_ent[2] = rd_bd_sys_load(&tab[x].tau_a);
        s_ent[3] = rd_bd_sys_load(&tab[x].tau_b);
        s_ent[4] = rd_bd_sys_load(&tab[x].corr_re);
        s_ent[5] = rd_bd_sys_load(&tab[x].corr_im);
    }
    if constexpr (REPAIR) rd_bd_syndrome_table(s_E, P.shape.n_sym, tid);
    __syncthreads();
    const int c = s_ent[0], tau_a = s_ent[2], tau_b = s_ent[3];   // (workgroup-uniform from here on)
    const uint32_t want_id = (uint32_t)s_ent[1];
    const int32_t cr = s_ent[4], ci = s_ent[5];
    const int SL = P.shape.sl, N = P.shape.n_sym, body = SL * (N - 1), M = SL + 2;
    const int lo_lim = P.have_prev && prev ? -P.look : 0;
    const int t0 = tau_a - SL, t1 = tau_b + body + 1, len = t1 - t0;
    const int zf0 = NARROW ? max(t0 - M, lo_lim) : t0, zf1 = NARROW ? min(t1 + M, (int)n_out) : t1;
    const int L0 = zf0 & ~7, L1 = (zf1 + 7) & ~7;         // (floor and ceiling: lo_lim and n_out are multiples of 8)
    // What the host's range guarantees, checked again before anything is indexed by it: an entry that fails is idle.
    const bool active = tau_a <= tau_b && tau_b - tau_a <= RD_BX_MAX_SPAN && c >= 0 && c < P.n_ch && (cr != 0 || ci != 0) &&
                        cr >= -32768 && cr <= 32767 && ci >= -32768 && ci <= 32767 && tau_a + body >= 0 && t0 >= lo_lim &&
                        t1 <= (int)n_out && len <= RD_BX_LEN && L1 - L0 <= RD_BX_LOAD;
    bool found = false;
    if (active) {
        const uint8_t *src = cur + (size_t)c * ch_stride;
        const uint8_t *src_prev = prev ? prev + (size_t)c * ch_stride : nullptr;
        const uint16_t *zl = (const uint16_t *)s_z;      // output L0 + i: I in the low byte, Q in the high one
        const uint16_t *zw = zl + (t0 - L0);             // output t0 + i
        rd_bd_load_bytes(s_z, src, src_prev, L0, L1, (long)n_out, tid);   // (L0 < 0 only with lo_lim < 0: there is a chunk before)
        __syncthreads();
        // ---- the region decoder: one lane per tau = t0 + i, tau_a <= tau <= tau_b, under the entry's id
        uint64_t best_m;
        int best_t;
        uint32_t best_f;
        const int nb_g = rd_bd_best_in_region<REPAIR, NARROW>(zl, L0, t0, len, zf0, zf1, cr, ci, P.shape, want_id, INT32_MIN, nb_tab, W, tid,
                                                              best_f, best_m, best_t);
        found = best_t != INT32_MAX;                      // (uniform: every thread read the same four)
        if (found) {
            // ---- the record: sum of p over the packet's N SL samples tau - SL + 1 .. tau + SL (N - 1)
            const int i0 = best_t - t0;                   // (>= SL: the first pair lies in the region)
            rd_bd_packet_f<NARROW>(zw, s_y, i0 - SL + 1, i0 + body, s_fr, s_fi, tid);
            if (tid == 0u)
                rd_bd_write_record<REPAIR, NARROW>(&recs[x], c, (uint32_t)x, RD_BURST_MSG_EXPECTED | (t0 < 0 ? 1u : 0u), best_t, P.clock,
                                                   best_m, best_f, s_fr, s_fi, s_s + i0, SL, N, nb_g);
        }
    }
    if (tid == 0u) {
        rd_bx_header h;
        h.n_msgs = found ? 1u : 0u;
        h.candidates = active ? (uint32_t)(tau_b - tau_a + 1) : 0u;
        h.chunk = (uint32_t)P.seq;
        h.pad = 0u;
        hdr[x] = h;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
int rd_burst_expect_stage(const rd_config *cfg, int have_prev, uint64_t clock, const rd_expect *e, int n, void *slot_host,
                          uint32_t *cand) {
    rd_bx_entry *ent = (rd_bx_entry *)((uint8_t *)slot_host + RD_BX_ENTRY_OFFSET);
    int active = 0;
    for (int i = 0; i < n; i++) {
        rd_bx_entry x = {};
        x.channel = e[i].channel;
        x.id = e[i].id;
        x.corr_re = e[i].corr_re;
        x.corr_im = e[i].corr_im;
        x.tau_a = 0;
        x.tau_b = -1;
        uint32_t k = 0u;
        if (rd_bx_range(cfg->symbol_length, cfg->packet_symbols, cfg->block_size, have_prev, clock, e[i].t_lo, e[i].t_hi, &x.tau_a, &x.tau_b)) {
            k = (uint32_t)(x.tau_b - x.tau_a + 1);
            active++;
        } else {
            x.tau_a = 0;
            x.tau_b = -1;
        }
        ent[i] = x;
        if (cand) cand[i] = k;
    }
    return active;
}

int rd_burst_expect_launch(const rd_config *cfg, const uint8_t *chan_out, const uint8_t *chan_prev, size_t out_stride, int n_ch,
                           size_t n_out, uint64_t clock, uint64_t seq, int n, int max_flips, const uint32_t *narrow_tab,
                           void *slot_dev, hipStream_t st) {
    int rc = rd_burst_launch_check(cfg, chan_out, chan_prev, out_stride, n_ch, n_out, slot_dev, max_flips, narrow_tab, "burst expect");
    if (rc) return rc;
    if (n < 1 || n > RD_BX_MAX) return rd_fail_msg(RD_ERR_ARG, "burst expect: %d expectations, not 1 .. %d", n, RD_BX_MAX);
    rd_bx_params P;
    P.shape = rd_bd_shape_of(cfg, max_flips);
    P.look = RD_BU_WINDOW * rd_bd_look_windows(cfg);
    P.have_prev = chan_prev ? 1 : 0;
    P.n_ch = n_ch;
    P.clock = clock;
    P.seq = seq;
    uint8_t *base = (uint8_t *)slot_dev;
    rd_burst_msg *recs = (rd_burst_msg *)base;
    rd_bx_header *hdr = (rd_bx_header *)(base + RD_BX_HEADER_OFFSET);
    const rd_bx_entry *tab = (const rd_bx_entry *)(base + RD_BX_ENTRY_OFFSET);
    rd_bd_with_form(max_flips != 0, narrow_tab != nullptr, [&](auto repair, auto narrow) {
        hipLaunchKernelGGL((k_chan_burst_expect<decltype(repair)::value, decltype(narrow)::value>), dim3((unsigned)n),
                           dim3(RD_BURST_THREADS), 0, st, chan_out, chan_prev, out_stride, n_out, P, tab, recs, hdr, narrow_tab);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "k_chan_burst_expect: %s", hipGetErrorString(e));
    return RD_OK;
}

// Test hook (tests/test_burst_track.py): k_chan_burst_expect alone on host bytes, through rd_burst_expect_stage and
// rd_burst_expect_launch and a mapped host slot as the receiver allocates it, filled with 0xA5 and copied out whole.
extern "C" int rd_debug_burst_expect(const rd_config *cfg, const uint8_t *cur, const uint8_t *prev, size_t stride, int n_ch,
                                     uint64_t clock, uint64_t seq, const rd_expect *e, int n_e, int max_flips, int narrow,
                                     rd_burst_msg *msgs_out, uint32_t *hdr_out) {
    int rc = rd_burst_hook_modes(cfg, max_flips, narrow);
    if (rc) return rc;
    if (!cfg || !cur || !e || !msgs_out || !hdr_out || n_ch < 1 || n_e < 1) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int bad = -1;
    const char *why = "";
    if (rd_bx_check_table(e, n_e, n_ch, &bad, &why)) return rd_fail_msg(RD_ERR_ARG, "burst expect: entry %d: %s", bad, why);
    if ((rc = rd_burst_dbg::check(cfg, stride, "burst expect"))) return rc;   // (nothing allocated, nothing launched)
    rd_burst_dbg D;
    if ((rc = D.upload(cur, prev, (size_t)n_ch * stride)) || (rc = D.map(0, RD_BX_SLOT_BYTES))) return rc;
    if (rd_burst_expect_stage(cfg, prev ? 1 : 0, clock, e, n_e, D.slot[0], nullptr) > 0) {
        if ((narrow && (rc = D.narrow(cfg->symbol_length))) ||
            (rc = rd_burst_expect_launch(cfg, D.d_cur, D.d_prev, stride, n_ch, (size_t)cfg->block_size, clock, seq, n_e, max_flips, D.d_nb,
                                         D.d_slot[0], nullptr)) ||
            (rc = D.sync()))
            return rc;
    }
    memcpy(msgs_out, D.slot[0], RD_BX_HEADER_OFFSET);
    memcpy(hdr_out, D.slot[0] + RD_BX_HEADER_OFFSET, (size_t)RD_BX_MAX * sizeof(rd_bx_header));
    return RD_OK;
}
