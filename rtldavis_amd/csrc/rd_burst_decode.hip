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
// record places, every inner loop by the region).  Per run: the region's bytes go to LDS as they lie (16-byte vectors;
// t0 and the chunk boundary are multiples of 128); s is linear in p, so with SI, SR the sums of im p, re p over the SL
// samples (< 2^24: int32; a lane takes a stretch of consecutive outputs and slides both sums along it, one p in and one
// out per output) s[t] = corr_re SI[t] - corr_im SR[t] - two 32 x 32 -> 64-bit multiplies per sample, exact -
// goes to LDS as int64 (48 KiB for the longest region, 32 + 16 windows; the bytes 12 KiB); then one lane per tau: the
// sync word first - all but a few lanes leave there -, the rest of the symbols with byte packing, CRC and margin.  The
// candidates are reduced by a max over (margin, -tau): a total order, so the fixed tree of shuffles and the four waves'
// results in LDS give the same record whatever the order - no atomics.  The winner's record is completed by the whole
// workgroup (sum of p over the packet's N SL samples) and written by thread 0.
// Output: channel c owns cap = rd_bu_cap(nW) record places, as in the burst slot, and one header (n_msgs, long_runs,
// chunk): a run gives at most one record, so there is no overflow and no ticket; the channel's records are its first
// n_msgs places, in run order.  All stores are plain vector stores into the mapped host slot of the chunk's parity.  The
// burst records and the floor row are read from the burst slot where k_chan_bursts, earlier on the same stream, wrote
// them (system-scope loads).  With the default thresholds there are no runs: the header is written and that is all.
//
// Repair (steps 5a, 5b, 6' of the header; rd_wb_set_burst_repair).  The kernel is a template on it: k_chan_burst_decode<false>
// is the code above and is what max_flips = 0 launches; k_chan_burst_decode<true> adds, behind the sync test and the CRC
// of a tau - where all but a few lanes have left -, for a candidate with syndrome S != 0: the L = 8 smallest (|s|, k) of
// the payload symbols, kept sorted in registers by an unrolled insertion (64-bit magnitudes, ties to the smaller k); the
// singles, then the pairs in (a, b) order against S through E[k], the CRC of the packet whose only set symbol is k - the
// CRC has init 0 and is linear -, which the workgroup builds once into LDS (N x 16 bits); and the margin again without
// the flipped symbols.  The reduction carries (flips, k1, k2) in one word beside (margin, tau) and orders by
// (flips ascending, margin descending, tau ascending): still a total order, the same tree, the same four slots.  Thread 0
// writes the corrected symbols.
//
// Narrow-band filter (step 4n of the header; rd_wb_set_burst_narrow).  The second template argument: the two <*, false>
// forms are the code above, the two <*, true> forms put, between the region's bytes and the sliding sums: the grid choice
// - every wave scores the 64 centres, lane g its own, against (ca, cb) and reduces over (score, -g) by the fixed tree of
// shuffles: a max over a total order, the same g in all four waves, no LDS, no atomics -; the T = 2 SL + 5 taps of H[g]
// from the device table into LDS, as the two int16 pairs (re, -im) and (im, re) a complex product wants; the region as
// int16 pairs (zi, zq) with SL + 2 zeros on both sides (the zero extension: no bounds test per tap) in the place of s,
// which is not yet live; then y: a lane takes outputs tid + 256 j, four at a time in registers, per tap two LDS
// broadcasts of the tap and, per output, one LDS word and two packed 16-bit dot products (v_dot2_i32_i16) - 4 T integer
// multiply-adds per output, |acc| < 2^23 -; y = (acc + 2^10) >> 11 goes to LDS as a packed int16 pair, 24 KiB of its own
// for the longest region, because p' reads y while s is written and the record's f sum reads it again.  That takes the
// <*, true> forms to 85 KiB of static LDS (87024 and 87200 bytes) - one workgroup per CU where the others fit two; the grid is one workgroup per
// channel, far fewer than the chip has CUs, so nothing waits for the second.  The sliding sums, the candidates and the
// reduction then run as they are on p' = y conj(y[-1]) (components < 2^25, SL-sums < 2^31: int32) with (ca, cb) for the
// correlation sum, |s| < 2^47; the record's f sum is widened to 64 bits before the lanes are added (< 2^36).
#include <cstring>
#include <type_traits>
#include <vector>

#include <hip/hip_runtime.h>

#include "rd_burst_common.h"
#include "rd_internal.h"
#include "rd_parse.h"

extern int rd_fail_msg(int code, const char *fmt, ...);  // rd_api.hip: sets rd_last_error

#define RD_BD_THREADS 256
#define RD_BD_MAX_REGION ((RD_BD_MAX_W + RD_BD_MAX_LOOK_W) * RD_BU_WINDOW)   // outputs of the longest region

static_assert(sizeof(rd_burst_msg) == 64 && sizeof(rd_bd_header) == 16, "the slot layout of rd_bd_* (rd_internal.h)");
static_assert(RD_BD_MAX_REGION * 10 + 2 * 8 * RD_BD_DATA_BYTES + 256 <= 64 * 1024,
              "s (int64) and the bytes of the longest region, 60 KiB; the E table of the repair; 256 bytes of per-wave slots: under 64 KiB of LDS");
static_assert(RD_BD_REPAIR_L == 8, "the pair loop and the record's pad[] are written for a list of 8");
#define RD_BD_NB_MAX_T (2 * RD_BD_NB_MAX_SL + 5)
static_assert(RD_BD_NB_GRID == 64, "one lane of a wave per centre");
static_assert((RD_BD_MAX_REGION + RD_BD_NB_MAX_T - 1) * 4 <= RD_BD_MAX_REGION * 8, "the padded int16 region lies in s's place");
static_assert(RD_BD_MAX_REGION * 14 + 2 * 8 * RD_BD_DATA_BYTES + 2 * 4 * RD_BD_NB_MAX_T + 512 <= 160 * 1024,
              "narrow: y (4 bytes per output) and the taps beside the rest, under gfx950's 160 KiB of LDS");

struct rd_bd_params {
    int sl, n_sym;             // SL, N
    uint32_t sync;             // the 16 sync symbols, the first in bit 15
    int look;                  // LOOK
    int have_prev;
    unsigned n_win, cap;
    int max_flips;             // R (k_chan_burst_decode<true> alone reads it)
    uint64_t clock, seq;
};

template <bool REPAIR, bool NARROW>
__global__ __launch_bounds__(RD_BD_THREADS) void k_chan_burst_decode(const uint8_t *__restrict__ cur, const uint8_t *__restrict__ prev,
                                                                     size_t ch_stride, size_t n_out, rd_bd_params P,
                                                                     const rd_burst *runs, const rd_burst_floor *floor,
                                                                     rd_burst_msg *recs, rd_bd_header *hdr,
                                                                     const uint32_t *__restrict__ nb_tab) {
    __shared__ int64_t s_s[RD_BD_MAX_REGION];            // s[t0 + i] at i (i >= SL)
    __shared__ uint4 s_z[RD_BD_MAX_REGION / 8];          // the region's bytes: output t0 + i at bytes 2 i, 2 i + 1
    __shared__ uint64_t s_m[RD_BD_THREADS / 64];
    __shared__ int s_t[RD_BD_THREADS / 64];
    __shared__ int s_fr[RD_BD_THREADS / 64], s_fi[RD_BD_THREADS / 64];
    __shared__ uint32_t s_run[4];                        // n_bursts; first, windows, flags of the run in hand
    __shared__ int64_t s_corr[2];
    __shared__ uint16_t s_E[8 * RD_BD_DATA_BYTES];       // (REPAIR) E[k], 16 <= k < N
    __shared__ uint32_t s_f[RD_BD_THREADS / 64];         // (REPAIR) the waves' flips
    __shared__ uint32_t s_y[RD_BD_MAX_REGION];           // (NARROW) y[t0 + i] at i: re in the low half, im in the high one
    __shared__ uint32_t s_hA[RD_BD_NB_MAX_T], s_hB[RD_BD_NB_MAX_T];   // (NARROW) H[g][kk - M] as (re, -im) and (im, re)
    __shared__ int64_t s_fr64[RD_BD_THREADS / 64], s_fi64[RD_BD_THREADS / 64];   // (NARROW) in the place of s_fr, s_fi
    const int c = (int)blockIdx.x;
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint8_t *src = cur + (size_t)c * ch_stride;
    const uint8_t *src_prev = prev ? prev + (size_t)c * ch_stride : nullptr;
    const rd_burst *mine = runs + (size_t)c * P.cap;
    rd_burst_msg *out = recs + (size_t)c * P.cap;
    const uint16_t *zw = (const uint16_t *)s_z;           // output t0 + i: I in the low byte, Q in the high one
    if (tid == 0u) s_run[0] = rd_bd_sys_load(&floor[c].n_bursts);
    if constexpr (REPAIR) {
        // E[k]: symbol k is bit 7 - (k & 7) of on-air byte k >> 3, bit k & 7 of the bit-swapped byte
        if ((int)tid >= 16 && (int)tid < P.n_sym) {
            uint32_t crc = 0u;
            for (int b = 2; b < P.n_sym >> 3; b++) crc = rd_crc16_step(crc, b == (int)(tid >> 3) ? 1u << (tid & 7u) : 0u);
            s_E[tid] = (uint16_t)crc;
        }
    }
    __syncthreads();
    uint32_t n_runs = s_run[0];
    if (n_runs > P.cap) n_runs = P.cap;                   // (k_chan_bursts never writes more)
    const int SL = P.sl, N = P.n_sym, need = N * SL + 1;
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
        int nb_sh = 0, nb_g = 0;                          // (NARROW) sh and g of step 4n
        if constexpr (NARROW) {
            const int64_t mr = cr64 < 0 ? -cr64 : cr64, mi = ci64 < 0 ? -ci64 : ci64;
            const int bl = 64 - __clzll((long long)(mr > mi ? mr : mi));   // (not both 0: at least 1)
            nb_sh = bl > 15 ? bl - 15 : 0;
        }
        // |corr| <= 32 x 254 x 65025 < 2^30; NARROW: (ca, cb), in -2^15 .. 2^15 - 1
        const int32_t cr = NARROW ? (int32_t)(cr64 >> nb_sh) : (int32_t)cr64, ci = NARROW ? (int32_t)(ci64 >> nb_sh) : (int32_t)ci64;
        // ---- the region's bytes
        for (int v = (int)tid; v < len / 8; v += RD_BD_THREADS) {
            const int t = t0 + 8 * v;                     // (t0 and 0 are multiples of 8: a vector lies in one chunk)
            const uint8_t *g = t < 0 ? src_prev + 2 * ((long)t + (long)n_out) : src + 2 * (long)t;
            s_z[v] = *(const uint4 *)g;
        }
        __syncthreads();
        if constexpr (NARROW) {
            const int T = 2 * SL + 5, M = SL + 2;
            // ---- g: the smallest centre with the largest ca C.re + cb C.im (|score| < 2^30), the same in every wave
            {
                const uint32_t cw = nb_tab[RD_BD_NB_GRID * T + (int)lane];
                int sc = cr * (int)(int16_t)(cw & 0xFFFFu) + ci * ((int)cw >> 16);
                nb_g = (int)lane;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const int os = __shfl_xor(sc, off), og = __shfl_xor(nb_g, off);
                    if (os > sc || (os == sc && og < nb_g)) {
                        sc = os;
                        nb_g = og;
                    }
                }
            }
            if ((int)tid < T) {
                const uint32_t hw = nb_tab[nb_g * T + (int)tid];
                const int hr = (int)(int16_t)(hw & 0xFFFFu), hi = (int)hw >> 16;
                s_hA[tid] = rd_bd_pack16(hr, -hi);
                s_hB[tid] = rd_bd_pack16(hi, hr);
            }
            // ---- z as int16 pairs, output t0 + i at word i + M, zeros in front of the region and behind it
            uint32_t *z16 = (uint32_t *)s_s;
            for (int i = (int)tid; i < len + 2 * M; i += RD_BD_THREADS) {
                const int j = i - M;
                uint32_t zv = 0u;
                if (j >= 0 && j < len) {
                    const uint32_t a = zw[j];
                    zv = rd_bd_pack16(2 * (int)(a & 0xFFu) - 255, 2 * (int)(a >> 8) - 255);
                }
                z16[i] = zv;
            }
            __syncthreads();
            // ---- y[t0 + i] = (sum_kk H[g][kk - M] z[t0 + i - (kk - M)] + 2^10) >> 11: z[..] lies at word i + T - 1 - kk
            for (int base = (int)tid; base < len; base += 4 * RD_BD_THREADS) {
                int at[4], ar[4], ai[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int i = base + q * RD_BD_THREADS;
                    at[q] = (i < len ? i : base) + T - 1;    // (an output past the region repeats the lane's first and is not stored)
                    ar[q] = 0;
                    ai[q] = 0;
                }
                for (int kk = 0; kk < T; kk++) {
                    const uint32_t hA = s_hA[kk], hB = s_hB[kk];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const uint32_t zv = z16[at[q] - kk];
                        ar[q] = rd_bd_dot2(hA, zv, ar[q]);
                        ai[q] = rd_bd_dot2(hB, zv, ai[q]);
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int i = base + q * RD_BD_THREADS;
                    if (i < len)
                        s_y[i] = rd_bd_pack16((ar[q] + (1 << (RD_BD_NB_SHIFT - 1))) >> RD_BD_NB_SHIFT,
                                              (ai[q] + (1 << (RD_BD_NB_SHIFT - 1))) >> RD_BD_NB_SHIFT);
                }
            }
            __syncthreads();                              // y is whole, and z16 has been read: s may be written
        }
        // ---- s[t0 + i], SL <= i < len: a lane takes a stretch of outputs and slides the two window sums along it
        const int per = (len - SL + RD_BD_THREADS - 1) / RD_BD_THREADS;
        const int ia = SL + (int)tid * per, ib = min(ia + per, len);
        if (ia < ib) {
            int sr = 0, si = 0, re, im;
            for (int j = ia - SL + 1; j <= ia; j++) {
                rd_bd_pp<NARROW>(zw, s_y, j, re, im);
                sr += re;
                si += im;
            }
            s_s[ia] = (int64_t)cr * (int64_t)si - (int64_t)ci * (int64_t)sr;
            for (int i = ia + 1; i < ib; i++) {
                rd_bd_pp<NARROW>(zw, s_y, i, re, im);
                sr += re;
                si += im;
                rd_bd_pp<NARROW>(zw, s_y, i - SL, re, im);          // (i - SL >= 1: its pair lies in the region)
                sr -= re;
                si -= im;
                s_s[i] = (int64_t)cr * (int64_t)si - (int64_t)ci * (int64_t)sr;
            }
        }
        __syncthreads();
        // ---- one lane per tau = t0 + i
        uint64_t best_m = 0ull;
        int best_t = INT32_MAX;
        uint32_t best_f = 0u;
        const int i_hi = len - SL * (N - 1);              // i + SL (N - 1) < len
        for (int i = SL + (int)tid; i < i_hi; i += RD_BD_THREADS) {
            const int tau = t0 + i;
            if (tau + SL * (N - 1) < 0) continue;         // the packet ended in the chunk before: reported there
            uint64_t margin = ~0ull;
            uint32_t word = 0u, crc = 0u;
            bool ok = true;
            for (int k = 0; k < N; k++) {
                const int64_t v = s_s[i + SL * k];
                const uint32_t bit = v > 0 ? 1u : 0u;
                if (k < 16 && bit != ((P.sync >> (15 - k)) & 1u)) {
                    ok = false;
                    break;
                }
                const uint64_t mag = (uint64_t)(v > 0 ? v : -v);
                margin = mag < margin ? mag : margin;
                word = ((word << 1) | bit) & 0xFFu;
                if ((k & 7) == 7 && k >= 16) crc = rd_crc16_step(crc, rd_swap_bits8(word));
            }
            if constexpr (!REPAIR) {
                if (ok && crc == 0u && rd_bd_better(margin, tau, best_m, best_t)) {
                    best_m = margin;
                    best_t = tau;
                }
            } else {
                if (!ok) continue;
                uint32_t fl = 0u;
                if (crc != 0u) {                          // steps 5a, 5b: the syndrome S = crc
                    uint64_t lm[RD_BD_REPAIR_L];          // the list, ascending in (|s|, k)
                    int lk[RD_BD_REPAIR_L];
#pragma unroll
                    for (int a = 0; a < RD_BD_REPAIR_L; a++) {
                        lm[a] = ~0ull;
                        lk[a] = INT32_MAX;
                    }
                    for (int k = 16; k < N; k++) {
                        const int64_t v = s_s[i + SL * k];
                        uint64_t cm = (uint64_t)(v > 0 ? v : -v);
                        int ck = k;
#pragma unroll
                        for (int a = 0; a < RD_BD_REPAIR_L; a++)
                            if (cm < lm[a] || (cm == lm[a] && ck < lk[a])) {   // the entry moves in, the one it displaces goes on
                                const uint64_t tm = lm[a];
                                const int tk = lk[a];
                                lm[a] = cm;
                                lk[a] = ck;
                                cm = tm;
                                ck = tk;
                            }
                    }
                    uint32_t e[RD_BD_REPAIR_L];
#pragma unroll
                    for (int a = 0; a < RD_BD_REPAIR_L; a++) e[a] = s_E[lk[a]];   // (N >= 40: 24 payload symbols, the list is full)
#pragma unroll
                    for (int a = 0; a < RD_BD_REPAIR_L; a++)
                        if (fl == 0u && e[a] == crc) fl = 1u | ((uint32_t)lk[a] << 8);
                    if (P.max_flips >= 2) {
#pragma unroll
                        for (int a = 0; a < RD_BD_REPAIR_L; a++)
#pragma unroll
                            for (int b = a + 1; b < RD_BD_REPAIR_L; b++)
                                if (fl == 0u && (e[a] ^ e[b]) == crc) {
                                    const uint32_t ka = (uint32_t)lk[a], kb = (uint32_t)lk[b];
                                    fl = 2u | ((ka < kb ? ka : kb) << 8) | ((ka < kb ? kb : ka) << 16);
                                }
                    }
                    if (fl == 0u) continue;
                    const int k1 = (int)((fl >> 8) & 0xFFu), k2 = (fl & 0xFFu) == 2u ? (int)(fl >> 16) : -1;
                    margin = ~0ull;                       // step 6': over the symbols that were not flipped
                    for (int k = 0; k < N; k++) {
                        if (k == k1 || k == k2) continue;
                        const int64_t v = s_s[i + SL * k];
                        const uint64_t mag = (uint64_t)(v > 0 ? v : -v);
                        margin = mag < margin ? mag : margin;
                    }
                }
                if (rd_bd_better_r(fl, margin, tau, best_f, best_m, best_t)) {
                    best_f = fl;
                    best_m = margin;
                    best_t = tau;
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t om = (uint64_t)__shfl_xor((unsigned long long)best_m, off);
            const int ot = __shfl_xor(best_t, off);
            if constexpr (!REPAIR) {
                if (rd_bd_better(om, ot, best_m, best_t)) {
                    best_m = om;
                    best_t = ot;
                }
            } else {
                const uint32_t of = (uint32_t)__shfl_xor((int)best_f, off);
                if (rd_bd_better_r(of, om, ot, best_f, best_m, best_t)) {
                    best_f = of;
                    best_m = om;
                    best_t = ot;
                }
            }
        }
        if (lane == 0u) {
            s_m[wave] = best_m;
            s_t[wave] = best_t;
            if constexpr (REPAIR) s_f[wave] = best_f;
        }
        __syncthreads();
        best_m = s_m[0];
        best_t = s_t[0];
        if constexpr (REPAIR) best_f = s_f[0];
#pragma unroll
        for (int wv = 1; wv < RD_BD_THREADS / 64; wv++) {
            if constexpr (!REPAIR) {
                if (rd_bd_better(s_m[wv], s_t[wv], best_m, best_t)) {
                    best_m = s_m[wv];
                    best_t = s_t[wv];
                }
            } else {
                if (rd_bd_better_r(s_f[wv], s_m[wv], s_t[wv], best_f, best_m, best_t)) {
                    best_f = s_f[wv];
                    best_m = s_m[wv];
                    best_t = s_t[wv];
                }
            }
        }
        if (best_t == INT32_MAX) continue;                // (uniform: every thread read the same four)
        // ---- the record: sum of p over the packet's N SL samples tau - SL + 1 .. tau + SL (N - 1)
        const int i0 = best_t - t0;
        // |.| <= 2048 x 2 x 255^2 < 2^29; NARROW: a lane's 8 terms of p' < 2^28, the packet's 2047 < 2^36
        std::conditional_t<NARROW, long long, int> fr = 0, fi = 0;
        for (int j = i0 - SL + 1 + (int)tid; j <= i0 + SL * (N - 1); j += RD_BD_THREADS) {
            int re, im;
            rd_bd_pp<NARROW>(zw, s_y, j, re, im);
            fr += re;
            fi += im;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            fr += __shfl_xor(fr, off);
            fi += __shfl_xor(fi, off);
        }
        if (lane == 0u) {
            if constexpr (NARROW) {
                s_fr64[wave] = fr;
                s_fi64[wave] = fi;
            } else {
                s_fr[wave] = fr;
                s_fi[wave] = fi;
            }
        }
        __syncthreads();
        if (tid == 0u) {                                  // field by field into the slot: no private copy of the record
            rd_burst_msg *m = &out[n_msgs];
            m->channel = c;
            m->first = first;
            m->tau = best_t;
            uint32_t n_flip = 0u;
            int k1 = -1, k2 = -1;                         // the flipped symbols (REPAIR; none: -1)
            if constexpr (REPAIR) {
                n_flip = best_f & 0xFFu;
                if (n_flip >= 1u) k1 = (int)((best_f >> 8) & 0xFFu);
                if (n_flip == 2u) k2 = (int)((best_f >> 16) & 0xFFu);
            }
            m->flags = (back ? 1u : 0u) | (n_flip ? RD_BURST_MSG_REPAIRED : 0u) | (NARROW ? RD_BURST_MSG_NARROW : 0u);
            m->time = P.clock + (uint64_t)(int64_t)best_t;
            m->margin = best_m;
            int64_t sfr = 0, sfi = 0;
            for (int wv = 0; wv < RD_BD_THREADS / 64; wv++) {
                if constexpr (NARROW) {
                    sfr += s_fr64[wv];
                    sfi += s_fi64[wv];
                } else {
                    sfr += s_fr[wv];
                    sfi += s_fi[wv];
                }
            }
            m->f_re = sfr;
            m->f_im = sfi;
            uint32_t word = 0u, ones = 0u, id = 0u;
            for (int k = 0; k < N; k++) {
                uint32_t bit = s_s[i0 + SL * k] > 0 ? 1u : 0u;
                if constexpr (REPAIR) bit ^= (k == k1 || k == k2) ? 1u : 0u;
                ones += bit;
                word = ((word << 1) | bit) & 0xFFu;
                if ((k & 7) == 7) m->data[k >> 3] = (uint8_t)word;
                if (k == 23) id = rd_swap_bits8(word) & 7u;
            }
            for (int k = N >> 3; k < RD_BD_DATA_BYTES; k++) m->data[k] = 0;
            m->ones = (uint8_t)ones;
            m->id = (uint8_t)id;
            m->pad[0] = (uint8_t)n_flip;
            m->pad[1] = (uint8_t)(n_flip >= 1u ? k1 : 0);
            m->pad[2] = (uint8_t)(n_flip == 2u ? k2 : 0);
            m->pad[3] = (uint8_t)nb_g;                     // (0 without NARROW)
        }
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
    if (max_flips < 0 || max_flips > RD_BD_MAX_FLIPS)
        return rd_fail_msg(RD_ERR_ARG, "burst repair: max_flips %d, not 0 .. %d", max_flips, RD_BD_MAX_FLIPS);
    if (!chan_out || !burst_slot || !slot || n_ch < 1) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = rd_burst_decode_check(cfg);
    if (rc) return rc;
    if (narrow_tab && cfg->symbol_length < RD_BD_NB_MIN_SL)   // (at most RD_BD_NB_MAX_SL by the check above)
        return rd_fail_msg(RD_ERR_ARG, "narrow-band filter: symbol_length %d, at least %d", cfg->symbol_length, RD_BD_NB_MIN_SL);
    if (n_out != (size_t)cfg->block_size || out_stride < 2 * n_out || (out_stride & 15) || ((uintptr_t)chan_out & 15) ||
        ((uintptr_t)chan_prev & 15) || ((uintptr_t)slot & 15))
        return rd_fail_msg(RD_ERR_ARG, "burst decode: stride %zu for %zu outputs, or a misaligned buffer", out_stride, n_out);
    const size_t n_win = n_out / RD_BU_WINDOW;
    rd_bd_params P;
    P.sl = cfg->symbol_length;
    P.n_sym = cfg->packet_symbols;
    P.sync = 0u;
    for (int i = 0; i < 16; i++) P.sync = (P.sync << 1) | (cfg->preamble[i] ? 1u : 0u);
    P.look = RD_BU_WINDOW * rd_bd_look_windows(cfg);
    P.have_prev = chan_prev ? 1 : 0;
    P.n_win = (unsigned)n_win;
    P.cap = (unsigned)rd_bu_cap(n_win);
    P.clock = clock;
    P.seq = seq;
    P.max_flips = max_flips;
    const uint8_t *bs = (const uint8_t *)burst_slot;
    uint8_t *base = (uint8_t *)slot;
    const rd_burst *runs = (const rd_burst *)bs;
    const rd_burst_floor *floor = (const rd_burst_floor *)(bs + rd_bu_floor_offset(n_ch, n_win));
    rd_burst_msg *recs = (rd_burst_msg *)base;
    rd_bd_header *hdr = (rd_bd_header *)(base + rd_bd_header_offset(n_ch, n_win));
#define RD_BD_LAUNCH(REPAIR, NARROW)                                                                                          \
    hipLaunchKernelGGL((k_chan_burst_decode<REPAIR, NARROW>), dim3((unsigned)n_ch), dim3(RD_BD_THREADS), 0, st, chan_out, chan_prev, \
                       out_stride, n_out, P, runs, floor, recs, hdr, narrow_tab)
    if (!narrow_tab) {
        if (max_flips == 0) RD_BD_LAUNCH(false, false);   // the kernels from before step 4n, instruction for instruction
        else RD_BD_LAUNCH(true, false);
    } else {
        if (max_flips == 0) RD_BD_LAUNCH(false, true);
        else RD_BD_LAUNCH(true, true);
    }
#undef RD_BD_LAUNCH
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
    if (max_flips < 0 || max_flips > RD_BD_MAX_FLIPS)
        return rd_fail_msg(RD_ERR_ARG, "burst repair: max_flips %d, not 0 .. %d", max_flips, RD_BD_MAX_FLIPS);
    if (narrow != 0 && narrow != 1) return rd_fail_msg(RD_ERR_ARG, "narrow-band filter: narrow %d, not 0 or 1", narrow);
    if (narrow && cfg && cfg->symbol_length < RD_BD_NB_MIN_SL)
        return rd_fail_msg(RD_ERR_ARG, "narrow-band filter: symbol_length %d, at least %d", cfg->symbol_length, RD_BD_NB_MIN_SL);
    if (!cfg || !cur || !runs || !n_runs || !msgs_out || !n_msgs || !long_runs || !chunk || n_ch < 1)
        return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = rd_burst_decode_check(cfg);
    if (rc) return rc;                               // (nothing allocated, nothing launched)
    const size_t n_out = (size_t)cfg->block_size;
    if (stride < 2 * n_out || (stride & 15)) return rd_fail_msg(RD_ERR_ARG, "burst decode: stride %zu for %zu outputs", stride, n_out);
    rc = rd_ensure_device_public();
    if (rc) return rc;
    const size_t n_win = n_out / RD_BU_WINDOW, bu_bytes = rd_bu_slot_bytes(n_ch, n_win), bd_bytes = rd_bd_slot_bytes(n_ch, n_win);
    uint8_t *d_cur = nullptr, *d_prev = nullptr, *bu = nullptr, *bd = nullptr;
    uint32_t *d_nb = nullptr;
    void *d_bu = nullptr, *d_bd = nullptr;
#define RD_DBG_CHK(x) do { if ((x) != hipSuccess) { rc = rd_fail_msg(RD_ERR_DEVICE, "%s failed", #x); goto out; } } while (0)
    RD_DBG_CHK(hipMalloc(&d_cur, (size_t)n_ch * stride));
    RD_DBG_CHK(hipMemcpy(d_cur, cur, (size_t)n_ch * stride, hipMemcpyHostToDevice));
    if (prev) {
        RD_DBG_CHK(hipMalloc(&d_prev, (size_t)n_ch * stride));
        RD_DBG_CHK(hipMemcpy(d_prev, prev, (size_t)n_ch * stride, hipMemcpyHostToDevice));
    }
    RD_DBG_CHK(hipHostMalloc((void **)&bu, bu_bytes, hipHostMallocMapped));
    RD_DBG_CHK(hipHostMalloc((void **)&bd, bd_bytes, hipHostMallocMapped));
    memset(bu, 0xA5, bu_bytes);
    memset(bd, 0xA5, bd_bytes);
    memcpy(bu, runs, rd_bu_floor_offset(n_ch, n_win));
    for (int c = 0; c < n_ch; c++) {
        rd_burst_floor f = {};
        f.n_bursts = n_runs[c];
        f.chunk = (uint32_t)seq;
        memcpy(bu + rd_bu_floor_offset(n_ch, n_win) + (size_t)c * sizeof f, &f, sizeof f);
    }
    RD_DBG_CHK(hipHostGetDevicePointer(&d_bu, bu, 0));
    RD_DBG_CHK(hipHostGetDevicePointer(&d_bd, bd, 0));
    if (narrow && (rc = rd_bd_narrow_upload(cfg->symbol_length, &d_nb))) goto out;
    rc = rd_burst_decode_launch(cfg, d_cur, d_prev, stride, n_ch, n_out, clock, seq, max_flips, d_nb, d_bu, d_bd, nullptr);
    if (rc) goto out;
    RD_DBG_CHK(hipDeviceSynchronize());
    memcpy(msgs_out, bd, rd_bd_header_offset(n_ch, n_win));
    for (int c = 0; c < n_ch; c++) {
        rd_bd_header h;
        memcpy(&h, bd + rd_bd_header_offset(n_ch, n_win) + (size_t)c * sizeof h, sizeof h);
        n_msgs[c] = h.n_msgs;
        long_runs[c] = h.long_runs;
        chunk[c] = h.chunk;
    }
out:
#undef RD_DBG_CHK
    if (bu) hipHostFree(bu);
    if (bd) hipHostFree(bd);
    if (d_cur) hipFree(d_cur);
    if (d_prev) hipFree(d_prev);
    if (d_nb) hipFree(d_nb);
    return rc;
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
