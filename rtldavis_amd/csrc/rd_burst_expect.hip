// rd_burst_expect.hip - decode at the places the host expects a packet (include/rtldavis_hip.h, BURST EXPECT).
// k_chan_burst_decode needs a run of ON windows and slices around the run's own correlation sum; this kernel gets, per
// expectation, a channel, a range of candidate taus and the direction to slice around, and decodes there with no energy
// gate.  Used by rd_wideband.hip per streamed chunk (rd_wb_set_burst_expect), behind k_chan_burst_decode on the same stream.
//
// The host turns every rd_expect into an rd_bx_entry for the chunk's clock (rd_bx_range, rd_host.cpp): tau_a .. tau_b, or
// tau_a > tau_b for an expectation with no candidate in this chunk.  The entries travel in the mapped slot, behind the
// records and the headers; a launch is made only when one of them is active.
//
// Kernel.  One workgroup of 256 threads per expectation.  Region t0 = tau_a - SL, t1 = tau_b + SL (N - 1) + 1, at most
// 4096 outputs; t0 is no multiple of 8, so the bytes are loaded from L0 = the filter's first output (t0 without the
// filter) rounded DOWN to 8 up to its last rounded up - a 16-byte vector still lies in one chunk -, and everything
// behind the load indexes from t0: the outputs loaded in front of it enter neither p nor, beyond zf0 .. zf1, the
// filter.  From there the body is k_chan_burst_decode's (rd_burst_decode.hip), written out again because that kernel's
// loop over runs, its look-back rule and its candidate range SL .. len - SL (N - 1) are not this kernel's, and its four
// instantiations had to stay what they were: the narrow-band filter with the real samples of zf0 .. zf1 in the padded
// int16 region where a run has zeros, the sliding sums, one lane per tau over tau_a .. tau_b only, the id filter behind
// the repair, the same fixed tree of shuffles over the same total order, thread 0 writing the record field by field.
// LDS: s (int64, 32 KiB), the bytes (8.25 KiB), y (16 KiB, narrow only) - less than the decode kernel's.  Plain vector
// stores into the mapped slot, no atomics.
#include <cstring>
#include <type_traits>
#include <vector>

#include <hip/hip_runtime.h>

#include "rd_burst_common.h"
#include "rd_internal.h"
#include "rd_parse.h"

extern int rd_fail_msg(int code, const char *fmt, ...);  // rd_api.hip: sets rd_last_error

#define RD_BX_THREADS 256
#define RD_BX_LEN (RD_BX_MAX_SPAN + RD_BD_MAX_LOOK_W * RD_BU_WINDOW)   // t1 - t0 at most: the span + N SL + 1
#define RD_BX_NB_MAX_T (2 * RD_BD_NB_MAX_SL + 5)
#define RD_BX_LOAD (RD_BX_LEN + 128)                                    // outputs loaded at most
static_assert(RD_BX_LEN + 2 * (RD_BD_NB_MAX_SL + 2) + 14 <= RD_BX_LOAD && RD_BX_LOAD % 8 == 0, "the filter's margins and the rounding to 8");
static_assert((RD_BX_LEN + RD_BX_NB_MAX_T - 1) * 4 <= RD_BX_LEN * 8, "the padded int16 region lies in s's place");
static_assert(sizeof(rd_bx_header) == 16 && sizeof(rd_bx_entry) == 32, "the slot layout of rd_bx_* (rd_internal.h)");
static_assert(RD_BD_REPAIR_L == 8 && RD_BD_NB_GRID == 64, "the pair loop is written for a list of 8, the grid for one lane per centre");

struct rd_bx_params {
    int sl, n_sym;             // SL, N
    uint32_t sync;             // the 16 sync symbols, the first in bit 15
    int look;                  // LOOK
    int have_prev;
    int n_ch;
    int max_flips;             // R (the <true, *> forms alone read it)
    uint64_t clock, seq;
};

template <bool REPAIR, bool NARROW>
__global__ __launch_bounds__(RD_BX_THREADS) void k_chan_burst_expect(const uint8_t *__restrict__ cur, const uint8_t *__restrict__ prev,
                                                                     size_t ch_stride, size_t n_out, rd_bx_params P,
                                                                     const rd_bx_entry *tab, rd_burst_msg *recs, rd_bx_header *hdr,
                                                                     const uint32_t *__restrict__ nb_tab) {
    __shared__ int64_t s_s[RD_BX_LEN];                   // s[t0 + i] at i (i >= SL)
    __shared__ uint4 s_z[RD_BX_LOAD / 8];                // the loaded bytes: output L0 + i at bytes 2 i, 2 i + 1
    __shared__ uint64_t s_m[RD_BX_THREADS / 64];
    __shared__ int s_t[RD_BX_THREADS / 64];
    __shared__ int s_fr[RD_BX_THREADS / 64], s_fi[RD_BX_THREADS / 64];
    __shared__ int32_t s_ent[6];                         // the entry: channel, id, tau_a, tau_b, corr_re, corr_im
    __shared__ uint16_t s_E[8 * RD_BD_DATA_BYTES];       // (REPAIR) E[k], 16 <= k < N
    __shared__ uint32_t s_f[RD_BX_THREADS / 64];         // (REPAIR) the waves' flips
    __shared__ uint32_t s_y[RD_BX_LEN];                  // (NARROW) y[t0 + i] at i: re in the low half, im in the high one
    __shared__ uint32_t s_hA[RD_BX_NB_MAX_T], s_hB[RD_BX_NB_MAX_T];   // (NARROW) H[g][kk - M] as (re, -im) and (im, re)
    __shared__ int64_t s_fr64[RD_BX_THREADS / 64], s_fi64[RD_BX_THREADS / 64];   // (NARROW) in the place of s_fr, s_fi
    const int x = (int)blockIdx.x;
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0u) {                                     // one thread crosses the bus, the workgroup takes it from LDS
        s_ent[0] = rd_bd_sys_load(&tab[x].channel);
        s_ent[1] = (int32_t)rd_bd_sys_load(&tab[x].id);
        s_ent[2] = rd_bd_sys_load(&tab[x].tau_a);
        s_ent[3] = rd_bd_sys_load(&tab[x].tau_b);
        s_ent[4] = rd_bd_sys_load(&tab[x].corr_re);
        s_ent[5] = rd_bd_sys_load(&tab[x].corr_im);
    }
    if constexpr (REPAIR) {
        // E[k]: symbol k is bit 7 - (k & 7) of on-air byte k >> 3, bit k & 7 of the bit-swapped byte
        if ((int)tid >= 16 && (int)tid < P.n_sym) {
            uint32_t crc = 0u;
            for (int b = 2; b < P.n_sym >> 3; b++) crc = rd_crc16_step(crc, b == (int)(tid >> 3) ? 1u << (tid & 7u) : 0u);
            s_E[tid] = (uint16_t)crc;
        }
    }
    __syncthreads();
    const int c = s_ent[0], tau_a = s_ent[2], tau_b = s_ent[3];   // (workgroup-uniform from here on)
    const uint32_t want_id = (uint32_t)s_ent[1];
    const int32_t cr = s_ent[4], ci = s_ent[5];
    const int SL = P.sl, N = P.n_sym, body = SL * (N - 1), M = SL + 2;
    const int lo_lim = P.have_prev && prev ? -P.look : 0;
    const int t0 = tau_a - SL, t1 = tau_b + body + 1, len = t1 - t0;
    const int zf0 = NARROW ? max(t0 - M, lo_lim) : t0, zf1 = NARROW ? min(t1 + M, (int)n_out) : t1;
    const int L0 = zf0 & ~7, L1 = (zf1 + 7) & ~7;         // (floor and ceiling: lo_lim and n_out are multiples of 8)
    // What the host's range guarantees, checked again before anything is indexed by it: an entry that fails is idle.
    const bool active = tau_a <= tau_b && tau_b - tau_a <= RD_BX_MAX_SPAN && c >= 0 && c < P.n_ch && (cr != 0 || ci != 0) &&
                        cr >= -32768 && cr <= 32767 && ci >= -32768 && ci <= 32767 && tau_a + body >= 0 && t0 >= lo_lim &&
                        t1 <= (int)n_out && len <= RD_BX_LEN && L1 - L0 <= RD_BX_LOAD;
    if (!active) {
        if (tid == 0u) {
            rd_bx_header h;
            h.n_msgs = 0u;
            h.candidates = 0u;
            h.chunk = (uint32_t)P.seq;
            h.pad = 0u;
            hdr[x] = h;
        }
        return;
    }
    const uint8_t *src = cur + (size_t)c * ch_stride;
    const uint8_t *src_prev = prev ? prev + (size_t)c * ch_stride : nullptr;
    const uint16_t *zl = (const uint16_t *)s_z;          // output L0 + i: I in the low byte, Q in the high one
    const uint16_t *zw = zl + (t0 - L0);                 // output t0 + i
    // ---- the bytes of L0 .. L1 (L0 < 0 only with lo_lim < 0: there is a chunk before)
    for (int v = (int)tid; v < (L1 - L0) / 8; v += RD_BX_THREADS) {
        const int t = L0 + 8 * v;                         // (L0 and 0 are multiples of 8: a vector lies in one chunk)
        const uint8_t *g = t < 0 ? src_prev + 2 * ((long)t + (long)n_out) : src + 2 * (long)t;
        s_z[v] = *(const uint4 *)g;
    }
    __syncthreads();
    int nb_g = 0;                                         // (NARROW) g of step 4n
    if constexpr (NARROW) {
        const int T = 2 * SL + 5;
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
        // ---- z as int16 pairs, output t0 - M + i at word i: the samples of zf0 .. zf1, zeros outside
        uint32_t *z16 = (uint32_t *)s_s;
        for (int i = (int)tid; i < len + 2 * M; i += RD_BX_THREADS) {
            const int t = t0 - M + i;
            uint32_t zv = 0u;
            if (t >= zf0 && t < zf1) {
                const uint32_t a = zl[t - L0];
                zv = rd_bd_pack16(2 * (int)(a & 0xFFu) - 255, 2 * (int)(a >> 8) - 255);
            }
            z16[i] = zv;
        }
        __syncthreads();
        // ---- y[t0 + i] = (sum_kk H[g][kk - M] z[t0 + i - (kk - M)] + 2^10) >> 11: z[..] lies at word i + T - 1 - kk
        for (int base = (int)tid; base < len; base += 4 * RD_BX_THREADS) {
            int at[4], ar[4], ai[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int i = base + q * RD_BX_THREADS;
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
                const int i = base + q * RD_BX_THREADS;
                if (i < len)
                    s_y[i] = rd_bd_pack16((ar[q] + (1 << (RD_BD_NB_SHIFT - 1))) >> RD_BD_NB_SHIFT,
                                          (ai[q] + (1 << (RD_BD_NB_SHIFT - 1))) >> RD_BD_NB_SHIFT);
            }
        }
        __syncthreads();                                  // y is whole, and z16 has been read: s may be written
    }
    // ---- s[t0 + i], SL <= i < len: a lane takes a stretch of outputs and slides the two window sums along it
    const int per = (len - SL + RD_BX_THREADS - 1) / RD_BX_THREADS;
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
    // ---- one lane per tau = t0 + i, tau_a <= tau <= tau_b
    uint64_t best_m = 0ull;
    int best_t = INT32_MAX;
    uint32_t best_f = 0u;
    const int i_hi = len - body;                          // = SL + (tau_b - tau_a) + 1
    for (int i = SL + (int)tid; i < i_hi; i += RD_BX_THREADS) {
        const int tau = t0 + i;
        uint64_t margin = ~0ull;
        uint32_t word = 0u, crc = 0u, id = 0u;
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
            if (k == 23) id = rd_swap_bits8(word) & 7u;   // symbols 16, 17, 18 are its bits 0, 1, 2
        }
        if (!ok) continue;
        if constexpr (!REPAIR) {
            if (crc == 0u && (want_id >= 8u || id == want_id) && rd_bd_better(margin, tau, best_m, best_t)) {
                best_m = margin;
                best_t = tau;
            }
        } else {
            uint32_t fl = 0u;
            if (crc != 0u) {                              // steps 5a, 5b: the syndrome S = crc
                uint64_t lm[RD_BD_REPAIR_L];              // the list, ascending in (|s|, k)
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
                margin = ~0ull;                           // step 6': over the symbols that were not flipped
                for (int k = 0; k < N; k++) {
                    if (k == k1 || k == k2) continue;
                    const int64_t v = s_s[i + SL * k];
                    const uint64_t mag = (uint64_t)(v > 0 ? v : -v);
                    margin = mag < margin ? mag : margin;
                }
                if (k1 >= 16 && k1 <= 18) id ^= 1u << (k1 - 16);   // the id of the corrected symbols
                if (k2 >= 16 && k2 <= 18) id ^= 1u << (k2 - 16);
            }
            if (want_id < 8u && id != want_id) continue;
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
    for (int wv = 1; wv < RD_BX_THREADS / 64; wv++) {
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
    const bool found = best_t != INT32_MAX;               // (uniform: every thread read the same four)
    if (found) {
        // ---- the record: sum of p over the packet's N SL samples tau - SL + 1 .. tau + SL (N - 1)
        const int i0 = best_t - t0;                       // (>= SL: the first pair lies in the region)
        std::conditional_t<NARROW, long long, int> fr = 0, fi = 0;
        for (int j = i0 - SL + 1 + (int)tid; j <= i0 + body; j += RD_BX_THREADS) {
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
            rd_burst_msg *m = &recs[x];
            m->channel = c;
            m->first = (uint32_t)x;
            m->tau = best_t;
            uint32_t n_flip = 0u;
            int k1 = -1, k2 = -1;                         // the flipped symbols (REPAIR; none: -1)
            if constexpr (REPAIR) {
                n_flip = best_f & 0xFFu;
                if (n_flip >= 1u) k1 = (int)((best_f >> 8) & 0xFFu);
                if (n_flip == 2u) k2 = (int)((best_f >> 16) & 0xFFu);
            }
            m->flags = RD_BURST_MSG_EXPECTED | (t0 < 0 ? 1u : 0u) | (n_flip ? RD_BURST_MSG_REPAIRED : 0u) | (NARROW ? RD_BURST_MSG_NARROW : 0u);
            m->time = P.clock + (uint64_t)(int64_t)best_t;
            m->margin = best_m;
            int64_t sfr = 0, sfi = 0;
            for (int wv = 0; wv < RD_BX_THREADS / 64; wv++) {
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
    }
    if (tid == 0u) {
        rd_bx_header h;
        h.n_msgs = found ? 1u : 0u;
        h.candidates = (uint32_t)(tau_b - tau_a + 1);
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
    if (max_flips < 0 || max_flips > RD_BD_MAX_FLIPS)
        return rd_fail_msg(RD_ERR_ARG, "burst repair: max_flips %d, not 0 .. %d", max_flips, RD_BD_MAX_FLIPS);
    if (!chan_out || !slot_dev || n_ch < 1 || n < 1 || n > RD_BX_MAX) return rd_fail_msg(RD_ERR_ARG, "burst expect: null argument or %d expectations", n);
    int rc = rd_burst_decode_check(cfg);
    if (rc) return rc;
    if (narrow_tab && cfg->symbol_length < RD_BD_NB_MIN_SL)   // (at most RD_BD_NB_MAX_SL by the check above)
        return rd_fail_msg(RD_ERR_ARG, "narrow-band filter: symbol_length %d, at least %d", cfg->symbol_length, RD_BD_NB_MIN_SL);
    if (n_out != (size_t)cfg->block_size || out_stride < 2 * n_out || (out_stride & 15) || ((uintptr_t)chan_out & 15) ||
        ((uintptr_t)chan_prev & 15) || ((uintptr_t)slot_dev & 15))
        return rd_fail_msg(RD_ERR_ARG, "burst expect: stride %zu for %zu outputs, or a misaligned buffer", out_stride, n_out);
    rd_bx_params P;
    P.sl = cfg->symbol_length;
    P.n_sym = cfg->packet_symbols;
    P.sync = 0u;
    for (int i = 0; i < 16; i++) P.sync = (P.sync << 1) | (cfg->preamble[i] ? 1u : 0u);
    P.look = RD_BU_WINDOW * rd_bd_look_windows(cfg);
    P.have_prev = chan_prev ? 1 : 0;
    P.n_ch = n_ch;
    P.max_flips = max_flips;
    P.clock = clock;
    P.seq = seq;
    uint8_t *base = (uint8_t *)slot_dev;
    rd_burst_msg *recs = (rd_burst_msg *)base;
    rd_bx_header *hdr = (rd_bx_header *)(base + RD_BX_HEADER_OFFSET);
    const rd_bx_entry *tab = (const rd_bx_entry *)(base + RD_BX_ENTRY_OFFSET);
#define RD_BX_LAUNCH(REPAIR, NARROW)                                                                                          \
    hipLaunchKernelGGL((k_chan_burst_expect<REPAIR, NARROW>), dim3((unsigned)n), dim3(RD_BX_THREADS), 0, st, chan_out, chan_prev, \
                       out_stride, n_out, P, tab, recs, hdr, narrow_tab)
    if (!narrow_tab) {
        if (max_flips == 0) RD_BX_LAUNCH(false, false);
        else RD_BX_LAUNCH(true, false);
    } else {
        if (max_flips == 0) RD_BX_LAUNCH(false, true);
        else RD_BX_LAUNCH(true, true);
    }
#undef RD_BX_LAUNCH
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "k_chan_burst_expect: %s", hipGetErrorString(e));
    return RD_OK;
}

// Test hook (tests/test_burst_track.py): k_chan_burst_expect alone on host bytes, through rd_burst_expect_stage and
// rd_burst_expect_launch and a mapped host slot as the receiver allocates it, filled with 0xA5 and copied out whole.
extern "C" int rd_debug_burst_expect(const rd_config *cfg, const uint8_t *cur, const uint8_t *prev, size_t stride, int n_ch,
                                     uint64_t clock, uint64_t seq, const rd_expect *e, int n_e, int max_flips, int narrow,
                                     rd_burst_msg *msgs_out, uint32_t *hdr_out) {
    if (max_flips < 0 || max_flips > RD_BD_MAX_FLIPS)
        return rd_fail_msg(RD_ERR_ARG, "burst repair: max_flips %d, not 0 .. %d", max_flips, RD_BD_MAX_FLIPS);
    if (narrow != 0 && narrow != 1) return rd_fail_msg(RD_ERR_ARG, "narrow-band filter: narrow %d, not 0 or 1", narrow);
    if (narrow && cfg && cfg->symbol_length < RD_BD_NB_MIN_SL)
        return rd_fail_msg(RD_ERR_ARG, "narrow-band filter: symbol_length %d, at least %d", cfg->symbol_length, RD_BD_NB_MIN_SL);
    if (!cfg || !cur || !e || !msgs_out || !hdr_out || n_ch < 1 || n_e < 1) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int bad = -1;
    const char *why = "";
    if (rd_bx_check_table(e, n_e, n_ch, &bad, &why)) return rd_fail_msg(RD_ERR_ARG, "burst expect: entry %d: %s", bad, why);
    int rc = rd_burst_decode_check(cfg);
    if (rc) return rc;                               // (nothing allocated, nothing launched)
    const size_t n_out = (size_t)cfg->block_size;
    if (stride < 2 * n_out || (stride & 15)) return rd_fail_msg(RD_ERR_ARG, "burst expect: stride %zu for %zu outputs", stride, n_out);
    rc = rd_ensure_device_public();
    if (rc) return rc;
    uint8_t *d_cur = nullptr, *d_prev = nullptr, *bx = nullptr;
    uint32_t *d_nb = nullptr;
    void *d_bx = nullptr;
#define RD_DBG_CHK(x) do { if ((x) != hipSuccess) { rc = rd_fail_msg(RD_ERR_DEVICE, "%s failed", #x); goto out; } } while (0)
    RD_DBG_CHK(hipMalloc(&d_cur, (size_t)n_ch * stride));
    RD_DBG_CHK(hipMemcpy(d_cur, cur, (size_t)n_ch * stride, hipMemcpyHostToDevice));
    if (prev) {
        RD_DBG_CHK(hipMalloc(&d_prev, (size_t)n_ch * stride));
        RD_DBG_CHK(hipMemcpy(d_prev, prev, (size_t)n_ch * stride, hipMemcpyHostToDevice));
    }
    RD_DBG_CHK(hipHostMalloc((void **)&bx, RD_BX_SLOT_BYTES, hipHostMallocMapped));
    memset(bx, 0xA5, RD_BX_SLOT_BYTES);
    RD_DBG_CHK(hipHostGetDevicePointer(&d_bx, bx, 0));
    if (rd_burst_expect_stage(cfg, prev ? 1 : 0, clock, e, n_e, bx, nullptr) > 0) {
        if (narrow && (rc = rd_bd_narrow_upload(cfg->symbol_length, &d_nb))) goto out;
        rc = rd_burst_expect_launch(cfg, d_cur, d_prev, stride, n_ch, n_out, clock, seq, n_e, max_flips, d_nb, d_bx, nullptr);
        if (rc) goto out;
        RD_DBG_CHK(hipDeviceSynchronize());
    }
    memcpy(msgs_out, bx, RD_BX_HEADER_OFFSET);
    memcpy(hdr_out, bx + RD_BX_HEADER_OFFSET, (size_t)RD_BX_MAX * sizeof(rd_bx_header));
out:
#undef RD_DBG_CHK
    if (bx) hipHostFree(bx);
    if (d_cur) hipFree(d_cur);
    if (d_prev) hipFree(d_prev);
    if (d_nb) hipFree(d_nb);
    return rc;
}
