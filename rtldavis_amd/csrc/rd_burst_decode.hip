// rd_burst_decode.hip - decode the bursts k_chan_bursts found, wherever in the channel filter's pass band their carrier
// lies (include/rtldavis_hip.h, BURST DECODE).  The demodulator slices the discriminator around 0 Hz, so a burst further
// off than the deviation gives it no message; here the discriminator is sliced around the burst's OWN mean frequency -
// the run's lag-1 correlation sum, which its rd_burst record carries - and sync word plus CRC-16 prove the message.
// Used by rd_wideband.hip per streamed chunk (rd_wb_set_burst_decode), behind k_chan_bursts on the same stream.
//
// Definition (exact integers throughout; SL = symbol_length, N = packet_symbols, sync = the 16 preamble bits,
// LOOK_W = ceil((N SL + 1) / 128), LOOK = 128 LOOK_W, MAX_W = 32).  Channel c of chunk k: b = its channelized bytes,
// continued to t < 0 by chunk k-1's (t + block_size); a = 2 b - 255, z[t] = aI[t] + j aQ[t], p[t] = z[t] conj(z[t-1])
// (|re p|, |im p| <= 2 x 255^2 < 2^18).  For every rd_burst (first, windows, flags, corr) of the channel, in order:
//   windows > MAX_W: counted in long_runs, not decoded.  corr = 0: skipped.  A record k_chan_bursts never writes
//   (windows = 0, first >= nW, first + windows > nW; places past cap) is skipped.
//   region  t0 = 128 first - (LOOK if (flags & 1) and have_prev), t1 = 128 (first + windows); t1 - t0 < N SL + 1: skipped
//   d[t] = im p[t] corr_re - re p[t] corr_im   (t0 < t < t1)      Im(p conj(corr)); |corr| < 2^30 at MAX_W: |d| < 2^48
//   s[t] = sum_{i < SL} d[t - i]               (t0 + SL <= t < t1), bit[t] = s[t] > 0
//   candidate tau (the end of the first symbol): t0 + SL <= tau, tau + SL (N - 1) < t1, tau + SL (N - 1) >= 0 (the packet
//   ends in this chunk.  A packet has about SL - 2 adjacent valid taus, so one that ends within SL outputs of the chunk
//   boundary can still be reported on both sides of it: the host drops the second report when it copies the records
//   out, step 7 of the header, rd_wideband.hip); symbols bit[tau + SL i]; the first 16 equal sync; the
//   N symbols packed MSB first into N / 8 bytes whose bit-swapped bytes [2:] have CRC-16-CCITT 0 (rd_parse.h)
//   one record per run at most: the candidate with the largest margin = min_i |s[tau + SL i]|, ties to the smallest tau.
//
// Kernel.  One workgroup of 256 threads per channel, the channel's runs one after the other (the loop is bounded by the
// record places, every inner loop by the region); thread 0 fetches a run's record with system-scope loads from the burst
// slot where k_chan_bursts, earlier on the same stream, wrote it.  Per run: the region's bytes (t0 and the chunk boundary
// are multiples of 128; 12 KiB for the longest region, 32 + 16 windows), the region decoder of rd_burst_common.h (s is
// int64, 48 KiB; one lane per tau - all but a few leave at the sync word), and the winner's record, completed by the whole
// workgroup and written by thread 0.
// Output: channel c owns cap = rd_bu_cap(nW) record places, as in the burst slot, and one header (n_msgs, long_runs,
// chunk): a run gives at most one record, so there is no overflow and no ticket; the channel's records are its first
// n_msgs places, in run order.  All stores are plain vector stores into the mapped host slot of the chunk's parity.  With
// the default thresholds there are no runs: the header is written and that is all.
//
// The kernel is a template on the repair (steps 5a, 5b, 6'; rd_wb_set_burst_repair: max_flips > 0 launches <true, *>, whose
// candidate test goes on behind a failed CRC - rd_burst_candidate.h - and whose reduction carries the flips) and on the
// narrow-band filter (step 4n; rd_wb_set_burst_narrow: a table launches <*, true>).  The <*, true> forms put, between the
// bytes and the sliding sums: the grid choice from (ca, cb), the taps, the region as int16 pairs with SL + 2 zeros on
// both sides in the place of s, which is not yet live, and y, 24 KiB of its own for the longest region, because p' reads
// y while s is written and the record's f sum reads it again.  That takes them to 85 KiB of static LDS (87024 and 87200
// bytes) - one workgroup per CU where the others fit two; the grid is one workgroup per channel, far fewer than the chip
// has CUs, so nothing waits for the second.  The rest then runs on p' = y conj(y[-1]) with (ca, cb) for the correlation
// sum, |s| < 2^47.
#include <type_traits>
#include <vector>

#include <hip/hip_runtime.h>

#include "rd_burst_common.h"

#define RD_BD_MAX_REGION ((RD_BD_MAX_W + RD_BD_MAX_LOOK_W) * RD_BU_WINDOW)   // outputs of the longest region

static_assert(sizeof(rd_burst_msg) == 64 && sizeof(rd_bd_header) == 16, "the slot layout of rd_bd_* (rd_internal.h)");
static_assert(RD_BD_MAX_REGION * 10 + 2 * 8 * RD_BD_DATA_BYTES + 256 <= 64 * 1024,
              "s (int64) and the bytes of the longest region, 60 KiB; the E table of the repair; 256 bytes of per-wave slots: under 64 KiB of LDS");
static_assert((RD_BD_MAX_REGION + RD_BD_NB_MAX_T - 1) * 4 <= RD_BD_MAX_REGION * 8, "the padded int16 region lies in s's place");
static_assert(RD_BD_MAX_REGION * 14 + 2 * 8 * RD_BD_DATA_BYTES + 2 * 4 * RD_BD_NB_MAX_T + 512 <= 160 * 1024,
              "narrow: y (4 bytes per output) and the taps beside the rest, under gfx950's 160 KiB of LDS");

struct rd_bd_params {
    rd_bd_shape shape;
    int look;                  // LOOK
    int have_prev;
    unsigned n_win, cap;
    uint64_t clock, seq;
};

template <bool REPAIR, bool NARROW>
__global__ __launch_bounds__(RD_BURST_THREADS) void k_chan_burst_decode(const uint8_t *__restrict__ cur, const uint8_t *__restrict__ prev,
                                                                        size_t ch_stride, size_t n_out, rd_bd_params P,
                                                                        const rd_burst *runs, const rd_burst_floor *floor,
                                                                        rd_burst_msg *recs, rd_bd_header *hdr,
                                                                        const uint32_t *__restrict__ nb_tab) {
    using f_t = std::conditional_t<NARROW, int64_t, int>;
    __shared__ int64_t s_s[RD_BD_MAX_REGION];            // s[t0 + i] at i (i >= SL)
    __shared__ uint4 s_z[RD_BD_MAX_REGION / 8];          // the region's bytes: output t0 + i at bytes 2 i, 2 i + 1
    __shared__ uint64_t s_m[RD_BURST_THREADS / 64];
    __shared__ int s_t[RD_BURST_THREADS / 64];
    __shared__ f_t s_fr[RD_BURST_THREADS / 64], s_fi[RD_BURST_THREADS / 64];
    __shared__ uint32_t s_run[4];                        // n_bursts; first, windows, flags of the run in hand
    __shared__ int64_t s_corr[2];
    __shared__ uint16_t s_E[8 * RD_BD_DATA_BYTES];       // (REPAIR) E[k], 16 <= k < N
    __shared__ uint32_t s_f[RD_BURST_THREADS / 64];      // (REPAIR) the waves' flips
    __shared__ uint32_t s_y[RD_BD_MAX_REGION];           // (NARROW) y[t0 + i] at i: re in the low half, im in the high one
    __shared__ uint32_t s_hA[RD_BD_NB_MAX_T], s_hB[RD_BD_NB_MAX_T];   // (NARROW) H[g][kk - M] as (re, -im) and (im, re)
    const rd_bd_work W = {s_s, s_m, s_t, s_E, s_f, s_y, s_hA, s_hB};
    const int c = (int)blockIdx.x;
    const unsigned tid = threadIdx.x;
    const uint8_t *src = cur + (size_t)c * ch_stride;
    const uint8_t *src_prev = prev ? prev + (size_t)c * ch_stride : nullptr;
    const rd_burst *mine = runs + (size_t)c * P.cap;
    rd_burst_msg *out = recs + (size_t)c * P.cap;
    const uint16_t *zw = (const uint16_t *)s_z;           // output t0 + i: I in the low byte, Q in the high one
    if (tid == 0u) s_run[0] = rd_bd_sys_load(&floor[c].n_bursts);
    if constexpr (REPAIR) rd_bd_syndrome_table(s_E, P.shape.n_sym, tid);
    __syncthreads();
    uint32_t n_runs = s_run[0];
    if (n_runs > P.cap) n_runs = P.cap;                   // (k_chan_bursts never writes more)
    const int SL = P.shape.sl, N = P.shape.n_sym, need = N * SL + 1;
    uint32_t n_msgs = 0u, n_long = 0u;
    for (uint32_t r = 0; r < n_runs; r++) {
        __syncthreads();                                  // the run before has been read out of LDS
        if (tid == 0u) {                                  // one thread crosses the bus, the workgroup takes it from LDS
            s_run[1] = rd_bd_sys_load(&mine[r].first);
            s_run[2] = rd_bd_sys_load(&mine[r].windows);
            s_run[3] = rd_bd_sys_load(&mine[r].flags);
            s_corr[0] = rd_bd_sys_load(&mine[r].corr_re);
            s_corr[1] = rd_bd_sys_load(&mine[r].corr_im);
        }
        __syncthreads();
        const uint32_t first = s_run[1], windows = s_run[2], rflags = s_run[3];   // (workgroup-uniform from here on)
        const int64_t cr64 = s_corr[0], ci64 = s_corr[1];
        if (windows > RD_BD_MAX_W) {
            n_long++;
            continue;
        }
        if (windows == 0u || first >= P.n_win || first + windows > P.n_win) continue;   // (no record of k_chan_bursts)
        if (cr64 == 0 && ci64 == 0) continue;
        const bool back = (rflags & 1u) && P.have_prev && src_prev && first == 0u;
        const int t0 = RD_BU_WINDOW * (int)first - (back ? P.look : 0);
        const int t1 = RD_BU_WINDOW * (int)(first + windows);
        const int len = t1 - t0;                          // a multiple of 128, <= RD_BD_MAX_REGION
        if (len < need || len > RD_BD_MAX_REGION) continue;
        int nb_sh = 0;                                    // (NARROW) sh of step 4n
        if constexpr (NARROW) {
            const int64_t mr = cr64 < 0 ? -cr64 : cr64, mi = ci64 < 0 ? -ci64 : ci64;
            const int bl = 64 - __clzll((long long)(mr > mi ? mr : mi));   // (not both 0: at least 1)
            nb_sh = bl > 15 ? bl - 15 : 0;
        }
        // |corr| <= 32 x 254 x 65025 < 2^30; NARROW: (ca, cb), in -2^15 .. 2^15 - 1
        const int32_t cr = NARROW ? (int32_t)(cr64 >> nb_sh) : (int32_t)cr64, ci = NARROW ? (int32_t)(ci64 >> nb_sh) : (int32_t)ci64;
        rd_bd_load_bytes(s_z, src, src_prev, t0, t1, (long)n_out, tid);
        __syncthreads();
        // ---- the region decoder: the filter sees zeros outside the region; any id; tau + SL (N - 1) >= 0 - a packet that
        // ended in the chunk before was reported there
        uint64_t best_m;
        int best_t;
        uint32_t best_f;
        const int nb_g = rd_bd_best_in_region<REPAIR, NARROW>(zw, t0, t0, len, t0, t1, cr, ci, P.shape, 8u, -SL * (N - 1), nb_tab, W, tid,
                                                              best_f, best_m, best_t);
        if (best_t == INT32_MAX) continue;                // (uniform: every thread read the same four)
        // ---- the record: sum of p over the packet's N SL samples tau - SL + 1 .. tau + SL (N - 1)
        const int i0 = best_t - t0;
        rd_bd_packet_f<NARROW>(zw, s_y, i0 - SL + 1, i0 + SL * (N - 1), s_fr, s_fi, tid);
        if (tid == 0u)
            rd_bd_write_record<REPAIR, NARROW>(&out[n_msgs], c, first, back ? 1u : 0u, best_t, P.clock, best_m, best_f, s_fr, s_fi,
                                               s_s + i0, SL, N, nb_g);
        n_msgs++;
    }
    if (tid == 0u) {
        rd_bd_header h;
        h.n_msgs = n_msgs;
        h.long_runs = n_long;
        h.chunk = (uint32_t)P.seq;
        h.pad = 0u;
        hdr[c] = h;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
int rd_bd_look_windows(const rd_config *cfg) {
    return (cfg->packet_symbols * cfg->symbol_length + 1 + RD_BU_WINDOW - 1) / RD_BU_WINDOW;
}

int rd_burst_decode_check(const rd_config *cfg) {
    if (!cfg) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (cfg->preamble_symbols != 16)
        return rd_fail_msg(RD_ERR_ARG, "burst decode: a sync word of %d symbols, not 16", cfg->preamble_symbols);
    if (cfg->symbol_length < 1 || cfg->packet_symbols % 8 || cfg->packet_symbols < 40 || cfg->packet_symbols > 8 * RD_BD_DATA_BYTES)
        return rd_fail_msg(RD_ERR_ARG, "burst decode: packets of %d symbols (a multiple of 8 in 40 .. %d)", cfg->packet_symbols,
                           8 * RD_BD_DATA_BYTES);
    if ((long)cfg->packet_symbols * cfg->symbol_length + 1 > RD_BD_MAX_LOOK_W * RD_BU_WINDOW)
        return rd_fail_msg(RD_ERR_ARG, "burst decode: a packet of %d x %d + 1 outputs, at most %d", cfg->packet_symbols,
                           cfg->symbol_length, RD_BD_MAX_LOOK_W * RD_BU_WINDOW);
    if (cfg->block_size < RD_BU_WINDOW * rd_bd_look_windows(cfg))
        return rd_fail_msg(RD_ERR_ARG, "burst decode: block_size %d is shorter than the look-back of %d outputs", cfg->block_size,
                           RD_BU_WINDOW * rd_bd_look_windows(cfg));
    return rd_bursts_check((size_t)cfg->block_size);
}

int rd_bd_narrow_upload(int sl, uint32_t **d_tab) {
    if (!d_tab) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (sl < RD_BD_NB_MIN_SL || sl > RD_BD_NB_MAX_SL)
        return rd_fail_msg(RD_ERR_ARG, "narrow-band filter: symbol_length %d, not %d .. %d", sl, RD_BD_NB_MIN_SL, RD_BD_NB_MAX_SL);
    const size_t T = 2 * (size_t)sl + 5, n = RD_BD_NB_GRID * T + RD_BD_NB_GRID;
    std::vector<int16_t> tab(2 * n);                    // taps, then centres: (re, im) is one little-endian word
    int rc = rd_bd_narrow_table(sl, tab.data(), tab.data() + 2 * RD_BD_NB_GRID * T);
    if (rc) return rd_fail_msg(rc, "narrow-band filter: no table for symbol_length %d", sl);
    uint32_t *d = nullptr;
    if (hipMalloc(&d, n * sizeof(uint32_t)) != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "hipMalloc of the narrow-band table failed");
    if (hipMemcpy(d, tab.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return rd_fail_msg(RD_ERR_DEVICE, "hipMemcpy of the narrow-band table failed");
    }
    *d_tab = d;
    return RD_OK;
}

int rd_burst_decode_launch(const rd_config *cfg, const uint8_t *chan_out, const uint8_t *chan_prev, size_t out_stride, int n_ch,
                           size_t n_out, uint64_t clock, uint64_t seq, int max_flips, const uint32_t *narrow_tab,
                           const void *burst_slot, void *slot, hipStream_t st) {
    // (a missing burst slot is refused where a missing message slot is)
    int rc = rd_burst_launch_check(cfg, chan_out, chan_prev, out_stride, n_ch, n_out, burst_slot ? slot : nullptr, max_flips, narrow_tab,
                                   "burst decode");
    if (rc) return rc;
    const size_t n_win = n_out / RD_BU_WINDOW;
    rd_bd_params P;
    P.shape = rd_bd_shape_of(cfg, max_flips);
    P.look = RD_BU_WINDOW * rd_bd_look_windows(cfg);
    P.have_prev = chan_prev ? 1 : 0;
    P.n_win = (unsigned)n_win;
    P.cap = (unsigned)rd_bu_cap(n_win);
    P.clock = clock;
    P.seq = seq;
    const uint8_t *bs = (const uint8_t *)burst_slot;
    uint8_t *base = (uint8_t *)slot;
    const rd_burst *runs = (const rd_burst *)bs;
    const rd_burst_floor *floor = (const rd_burst_floor *)(bs + rd_bu_floor_offset(n_ch, n_win));
    rd_burst_msg *recs = (rd_burst_msg *)base;
    rd_bd_header *hdr = (rd_bd_header *)(base + rd_bd_header_offset(n_ch, n_win));
    rd_bd_with_form(max_flips != 0, narrow_tab != nullptr, [&](auto repair, auto narrow) {
        hipLaunchKernelGGL((k_chan_burst_decode<decltype(repair)::value, decltype(narrow)::value>), dim3((unsigned)n_ch),
                           dim3(RD_BURST_THREADS), 0, st, chan_out, chan_prev, out_stride, n_out, P, runs, floor, recs, hdr, narrow_tab);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "k_chan_burst_decode: %s", hipGetErrorString(e));
    return RD_OK;
}

// Test hook (tests/test_burst_kernels_crafted.py): k_chan_burst_decode alone on host bytes, through
// rd_burst_decode_launch and mapped host slots as the receiver allocates them.  The caller's runs ([n_ch][cap]) and
// n_runs go into a burst slot of the product's layout - records k_chan_bursts never writes included -; the message slot
// is filled with 0xA5 before the launch and copied out whole, so the caller sees which places the kernel left alone.
// rd_debug_burst_decode_repair (tests/test_burst_repair.py) is the same with max_flips; rd_debug_burst_decode is it at 0.
// rd_debug_burst_decode_narrow (tests/test_burst_narrow.py) is the same with `narrow`: 1 uploads the table of step 4n for
// the launch; rd_debug_burst_decode_repair is it at 0.
extern "C" int rd_debug_burst_decode_narrow(const rd_config *cfg, const uint8_t *cur, const uint8_t *prev, size_t stride, int n_ch,
                                            uint64_t clock, uint64_t seq, const rd_burst *runs, const uint32_t *n_runs, int max_flips,
                                            int narrow, rd_burst_msg *msgs_out, uint32_t *n_msgs, uint32_t *long_runs,
                                            uint32_t *chunk) {
    int rc = rd_burst_hook_modes(cfg, max_flips, narrow);
    if (rc) return rc;
    if (!cfg || !cur || !runs || !n_runs || !msgs_out || !n_msgs || !long_runs || !chunk || n_ch < 1)
        return rd_fail_msg(RD_ERR_ARG, "null argument");
    if ((rc = rd_burst_dbg::check(cfg, stride, "burst decode"))) return rc;   // (nothing allocated, nothing launched)
    const size_t n_out = (size_t)cfg->block_size, n_win = n_out / RD_BU_WINDOW;
    rd_burst_dbg D;                                     // slot 0: the burst slot, slot 1: the message slot
    if ((rc = D.upload(cur, prev, (size_t)n_ch * stride)) || (rc = D.map(0, rd_bu_slot_bytes(n_ch, n_win))) ||
        (rc = D.map(1, rd_bd_slot_bytes(n_ch, n_win))) || (narrow && (rc = D.narrow(cfg->symbol_length))))
        return rc;
    uint8_t *bu = D.slot[0], *bd = D.slot[1];
    memcpy(bu, runs, rd_bu_floor_offset(n_ch, n_win));
    for (int c = 0; c < n_ch; c++) {
        rd_burst_floor f = {};
        f.n_bursts = n_runs[c];
        f.chunk = (uint32_t)seq;
        memcpy(bu + rd_bu_floor_offset(n_ch, n_win) + (size_t)c * sizeof f, &f, sizeof f);
    }
    if ((rc = rd_burst_decode_launch(cfg, D.d_cur, D.d_prev, stride, n_ch, n_out, clock, seq, max_flips, D.d_nb, D.d_slot[0], D.d_slot[1],
                                     nullptr)) ||
        (rc = D.sync()))
        return rc;
    memcpy(msgs_out, bd, rd_bd_header_offset(n_ch, n_win));
    for (int c = 0; c < n_ch; c++) {
        rd_bd_header h;
        memcpy(&h, bd + rd_bd_header_offset(n_ch, n_win) + (size_t)c * sizeof h, sizeof h);
        n_msgs[c] = h.n_msgs;
        long_runs[c] = h.long_runs;
        chunk[c] = h.chunk;
    }
    return RD_OK;
}

extern "C" int rd_debug_burst_decode_repair(const rd_config *cfg, const uint8_t *cur, const uint8_t *prev, size_t stride, int n_ch,
                                            uint64_t clock, uint64_t seq, const rd_burst *runs, const uint32_t *n_runs, int max_flips,
                                            rd_burst_msg *msgs_out, uint32_t *n_msgs, uint32_t *long_runs, uint32_t *chunk) {
    return rd_debug_burst_decode_narrow(cfg, cur, prev, stride, n_ch, clock, seq, runs, n_runs, max_flips, 0, msgs_out, n_msgs,
                                        long_runs, chunk);
}

extern "C" int rd_debug_burst_decode(const rd_config *cfg, const uint8_t *cur, const uint8_t *prev, size_t stride, int n_ch,
                                     uint64_t clock, uint64_t seq, const rd_burst *runs, const uint32_t *n_runs,
                                     rd_burst_msg *msgs_out, uint32_t *n_msgs, uint32_t *long_runs, uint32_t *chunk) {
    return rd_debug_burst_decode_repair(cfg, cur, prev, stride, n_ch, clock, seq, runs, n_runs, 0, msgs_out, n_msgs, long_runs, chunk);
}
