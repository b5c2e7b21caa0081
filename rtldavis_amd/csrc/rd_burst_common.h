// rd_burst_common.h - what the burst kernels share: k_chan_burst_decode (rd_burst_decode.hip, "decode"),
// k_chan_burst_expect (rd_burst_expect.hip, "expect"), k_chan_burst_search (rd_burst_search.hip, "search"),
// k_chan_burst_quality (rd_burst_quality.hip, "quality") and k_clip_decode (rd_clip_decode.hip, "clip decode").  The
// definition of every step: include/rtldavis_hip.h, BURST DECODE.
//
// Device phases.  Each is one step of a kernel for a whole workgroup of RD_BURST_THREADS; it takes the LDS arrays it works
// on as pointers and its geometry as plain values - ranges, pointers, an id to match, never which kernel calls it.  The
// __shared__ arrays are declared by the kernels, which keep their own LDS budgets.  All forced inline: a kernel is
// compiled as if it held the phases itself, and the pointers keep their LDS address space.  No phase ends in a barrier
// unless it says so.
//   rd_bd_syndrome_table   E[k] of the repair into LDS                                  decode, expect, clip decode
//   rd_bd_load_bytes       region bytes -> LDS, 16-byte vectors, seam into chunk k-1    decode, expect, quality, clip decode
//   rd_bd_grid_choice      g of step 4n: 64 centres, a fixed tree of shuffles           decode, expect, clip decode, quality
//   rd_bd_load_taps        the taps of H[g] as the two int16 pairs a product wants      decode, expect, clip decode, search, quality
//   rd_bd_fill_z16         z as int16 pairs, zeros outside zf0 .. zf1                   decode, expect, clip decode, quality
//   rd_bd_filter           y, four outputs per lane, packed 16-bit dot products         decode, expect, clip decode, search
//   rd_bd_symbol_sums      the sliding sums s[t]                                        decode, expect, clip decode
//   rd_bd_consider         one candidate tau against the lane's best so far             decode, expect, clip decode
//   rd_bd_reduce_best      the workgroup's best candidate (ends behind a barrier)       decode, expect, clip decode
//   rd_bd_best_in_region   the region decoder: the seven rows above in their order, with their barriers, on a region
//                          that lies in LDS (ends behind a barrier)                     decode, expect
//   rd_bd_packet_f         the sum of p over the winner's packet (ends behind a barrier) decode, expect, clip decode
//   rd_bd_write_record     the winner's rd_burst_msg, field by field (one thread)       decode, expect, clip decode
// Decode and expect reach the rows from rd_bd_grid_choice to rd_bd_reduce_best through rd_bd_best_in_region alone.  Clip
// decode holds the same sequence itself, barriers included, for its speed's sake (its head comment says why): a change
// to rd_bd_best_in_region is a change to k_clip_decode too.
// The candidate test itself (steps 5, 5a, 5b, 6') is host + device code of its own: rd_burst_candidate.h.
// The search kernel's int32-pair sums, per-position slicing and ballot ranking and the quality kernel's one-output-per-lane
// sums are other algorithms and stay in their files.
//
// Host side (below the phases): the sync word, the packet's shape as the three decoders' params carry it (rd_bd_shape),
// the ladder from (max_flips, narrow) to a kernel's <REPAIR, NARROW> form, the argument checks every *_launch and every
// rd_debug_burst_* hook makes, and rd_burst_dbg, which owns what a hook allocates.
#pragma once
#include <cstring>
#include <type_traits>

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rd_burst_candidate.h"
#include "rd_internal.h"

#define RD_BURST_THREADS 256
#define RD_BD_NB_MAX_T (2 * RD_BD_NB_MAX_SL + 5)          // the taps of the narrow-band filter at most
static_assert(RD_BD_NB_GRID == 64 && RD_BD_NB_MAX_T <= RD_BURST_THREADS, "one lane of a wave per centre, one thread per tap");
static_assert(8 * RD_BD_DATA_BYTES <= RD_BURST_THREADS, "one thread per entry of the syndrome table");

template <typename T>
__device__ __forceinline__ T rd_bd_sys_load(const T *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// p[t0 + j] = z[t0 + j] conj(z[t0 + j - 1]) from the region's bytes in LDS (j >= 1)
__device__ __forceinline__ void rd_bd_p(const uint16_t *zw, int j, int &re, int &im) {
    const uint32_t a = zw[j], b = zw[j - 1];
    const int ai = 2 * (int)(a & 0xFFu) - 255, aq = 2 * (int)(a >> 8) - 255;
    const int pi = 2 * (int)(b & 0xFFu) - 255, pq = 2 * (int)(b >> 8) - 255;
    re = ai * pi + aq * pq;
    im = aq * pi - ai * pq;
}

// p'[t0 + j] = y[t0 + j] conj(y[t0 + j - 1]) from y in LDS, an int16 pair per word (j >= 1); |y| <= 3192: below 2^25
__device__ __forceinline__ void rd_bd_pn(const uint32_t *y, int j, int &re, int &im) {
    const uint32_t a = y[j], b = y[j - 1];
    const int ar = (int)(int16_t)(a & 0xFFFFu), ai = (int)a >> 16;
    const int br = (int)(int16_t)(b & 0xFFFFu), bi = (int)b >> 16;
    re = ar * br + ai * bi;
    im = ai * br - ar * bi;
}

// p at t0 + j, or p' behind the filter
template <bool NARROW>
__device__ __forceinline__ void rd_bd_pp(const uint16_t *zw, const uint32_t *y, int j, int &re, int &im) {
    if constexpr (NARROW) rd_bd_pn(y, j, re, im);
    else rd_bd_p(zw, j, re, im);
}

__device__ __forceinline__ uint32_t rd_bd_pack16(int lo, int hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }

// c + a.lo b.lo + a.hi b.hi over int16 pairs, exact in int32
typedef short rd_short2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int rd_bd_dot2(uint32_t a, uint32_t b, int c) {
#if __has_builtin(__builtin_amdgcn_sdot2)
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(rd_short2, a), __builtin_bit_cast(rd_short2, b), c, false);
#else
    return c + (int)(int16_t)(a & 0xFFFFu) * (int)(int16_t)(b & 0xFFFFu) + ((int)a >> 16) * ((int)b >> 16);
#endif
}

// y of one output from the filter's accumulator
__device__ __forceinline__ int rd_bd_round(int acc) { return (acc + (1 << (RD_BD_NB_SHIFT - 1))) >> RD_BD_NB_SHIFT; }

// Candidate (flips, margin, tau) of a is better than that of b; tau = INT32_MAX: none.  flips = count | k1 << 8 | k2 << 16
// of step 6', 0 for an exact candidate and without repair: flips ascending, margin descending, tau ascending - a total order.
__device__ __forceinline__ bool rd_bd_better(uint32_t fa, uint64_t ma, int ta, uint32_t fb, uint64_t mb, int tb) {
    if (tb == INT32_MAX) return true;
    if (ta == INT32_MAX) return false;
    const uint32_t na = fa & 0xFFu, nb = fb & 0xFFu;
    if (na != nb) return na < nb;
    return ma > mb || (ma == mb && ta < tb);
}

// The packet's shape and the repair's reach: what the params of decode, expect and clip decode have in common, filled by
// rd_bd_shape_of (host side, below)
struct rd_bd_shape {
    int sl, n_sym;             // SL, N
    uint32_t sync;             // the 16 sync symbols, the first in bit 15
    int max_flips;             // R (the <true, *> forms alone read it)
};

// The work arrays of rd_bd_best_in_region, declared by the kernel: s (and z16 in its place before s is live), the waves'
// slots of the reduction and, for the forms that read them, E and the waves' flips (REPAIR), y and the taps (NARROW)
struct rd_bd_work {
    int64_t *s_s;
    uint64_t *s_m;
    int *s_t;
    const uint16_t *s_E;
    uint32_t *s_f, *s_y, *s_hA, *s_hB;
};

// ------------------------------------------------------------------------------------------
// phases
// ------------------------------------------------------------------------------------------
// E[k], 16 <= k < N, one thread each
__device__ __forceinline__ void rd_bd_syndrome_table(uint16_t *s_E, int n_sym, unsigned tid) {
    if ((int)tid >= 16 && (int)tid < n_sym) s_E[tid] = (uint16_t)rd_bd_syndrome((int)tid, n_sym);
}

// The bytes of outputs L0 .. L1 - 1 as they lie, output L0 + i at bytes 2 i, 2 i + 1 of s_z; t < 0 is output t + n_out of
// the chunk before.  L0, L1 and n_out are multiples of 8: a 16-byte vector lies in one chunk.  SEAM = false is the form
// for bytes that have no chunk before (L0 >= 0; the clip decoder's): src_prev and n_out are not looked at.
template <bool SEAM = true>
__device__ __forceinline__ void rd_bd_load_bytes(uint4 *s_z, const uint8_t *src, const uint8_t *src_prev, int L0, int L1, long n_out,
                                                 unsigned tid) {
    for (int v = (int)tid; v < (L1 - L0) / 8; v += RD_BURST_THREADS) {
        const int t = L0 + 8 * v;
        const uint8_t *g = SEAM && t < 0 ? src_prev + 2 * ((long)t + n_out) : src + 2 * (long)t;
        s_z[v] = *(const uint4 *)g;
    }
}

// g: the smallest centre with the largest ca C.re + cb C.im (|score| < 2^30).  Every wave scores the 64 centres, lane g its
// own, and reduces over (score, -g): a max over a total order, so the same g in every wave - no LDS, no atomics.
__device__ __forceinline__ int rd_bd_grid_choice(const uint32_t *__restrict__ nb_tab, int T, int ca, int cb, unsigned lane) {
    const uint32_t cw = nb_tab[RD_BD_NB_GRID * T + (int)lane];
    int sc = ca * (int)(int16_t)(cw & 0xFFFFu) + cb * ((int)cw >> 16);
    int g = (int)lane;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int os = __shfl_xor(sc, off), og = __shfl_xor(g, off);
        if (os > sc || (os == sc && og < g)) {
            sc = os;
            g = og;
        }
    }
    return g;
}

// The T taps of H[g] from the device table: H[g][kk - M] as (re, -im) in s_hA[kk] and (im, re) in s_hB[kk]
__device__ __forceinline__ void rd_bd_load_taps(const uint32_t *__restrict__ nb_tab, int g, int T, uint32_t *s_hA, uint32_t *s_hB,
                                                unsigned tid) {
    if ((int)tid < T) {
        const uint32_t hw = nb_tab[g * T + (int)tid];
        const int hr = (int)(int16_t)(hw & 0xFFFFu), hi = (int)hw >> 16;
        s_hA[tid] = rd_bd_pack16(hr, -hi);
        s_hB[tid] = rd_bd_pack16(hi, hr);
    }
}

// z as int16 pairs (zi, zq): output t_first + i at word i, i < count - the samples of zf0 .. zf1 - 1 from the loaded bytes
// (output L0 + j at zl[j]), zeros outside: the filter's zero extension, no bounds test per tap.
__device__ __forceinline__ void rd_bd_fill_z16(uint32_t *z16, const uint16_t *zl, int L0, int t_first, int count, int zf0, int zf1,
                                               unsigned tid) {
    for (int i = (int)tid; i < count; i += RD_BURST_THREADS) {
        const int t = t_first + i;
        uint32_t zv = 0u;
        if (t >= zf0 && t < zf1) {
            const uint32_t a = zl[t - L0];
            zv = rd_bd_pack16(2 * (int)(a & 0xFFu) - 255, 2 * (int)(a >> 8) - 255);
        }
        z16[i] = zv;
    }
}

// y[i] = (sum_kk H[g][kk - M] z[i - (kk - M)] + 2^10) >> 11, i < n_y, z[i - (kk - M)] at word i + T - 1 - kk of z16: a lane
// takes outputs tid + 256 j, four at a time in registers; per tap two LDS broadcasts of the tap and, per output, one LDS
// word and two packed dot products - 4 T integer multiply-adds per output, |acc| < 2^23.  y goes to s_y as an int16 pair.
__device__ __forceinline__ void rd_bd_filter(const uint32_t *z16, int n_y, int T, const uint32_t *s_hA, const uint32_t *s_hB,
                                             uint32_t *s_y, unsigned tid) {
    for (int base = (int)tid; base < n_y; base += 4 * RD_BURST_THREADS) {
        int at[4], ar[4], ai[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int i = base + q * RD_BURST_THREADS;
            at[q] = (i < n_y ? i : base) + T - 1;         // (an output past the region repeats the lane's first and is not stored)
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
            const int i = base + q * RD_BURST_THREADS;
            if (i < n_y) s_y[i] = rd_bd_pack16(rd_bd_round(ar[q]), rd_bd_round(ai[q]));
        }
    }
}

// s[t0 + i] = cr SI - ci SR at s_s[i], SL <= i < len, SI and SR the sums of im p, re p (p' with NARROW) over the SL samples
// that end at i: a lane takes a stretch of consecutive outputs and slides both sums along it, one p in and one out per
// output (int32: < 2^24, p' < 2^31), then two 32 x 32 -> 64-bit multiplies, exact.
template <bool NARROW>
__device__ __forceinline__ void rd_bd_symbol_sums(const uint16_t *zw, const uint32_t *s_y, int64_t *s_s, int SL, int len, int32_t cr,
                                                  int32_t ci, unsigned tid) {
    const int per = (len - SL + RD_BURST_THREADS - 1) / RD_BURST_THREADS;
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
            rd_bd_pp<NARROW>(zw, s_y, i - SL, re, im);    // (i - SL >= 1: its pair lies in the region)
            sr -= re;
            si -= im;
            s_s[i] = (int64_t)cr * (int64_t)si - (int64_t)ci * (int64_t)sr;
        }
    }
}

// Candidate tau, whose symbol sums are s[SL k]: if it passes (rd_burst_candidate.h) and carries the wanted id (want_id >= 8:
// any) and is better than the lane's best so far, it becomes that.
template <bool REPAIR>
__device__ __forceinline__ void rd_bd_consider(const int64_t *s, int SL, int N, uint32_t sync, int max_flips, const uint16_t *s_E,
                                               uint32_t want_id, int tau, uint32_t &best_f, uint64_t &best_m, int &best_t) {
    rd_bd_cand cand;
    if (!rd_bd_candidate<REPAIR>(s, SL, N, sync, max_flips, s_E, cand)) return;
    if (want_id < 8u && cand.id != want_id) return;
    if (rd_bd_better(cand.flips, cand.margin, tau, best_f, best_m, best_t)) {
        best_f = cand.flips;
        best_m = cand.margin;
        best_t = tau;
    }
}

// The best of the lanes' candidates into every thread: the fixed tree of shuffles, then the four waves' results through
// LDS - a max over a total order, so the same winner whatever the order; no atomics.  Ends behind a barrier.
template <bool REPAIR>
__device__ __forceinline__ void rd_bd_reduce_best(uint32_t &best_f, uint64_t &best_m, int &best_t, uint32_t *s_f, uint64_t *s_m,
                                                  int *s_t, unsigned lane, unsigned wave) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t om = (uint64_t)__shfl_xor((unsigned long long)best_m, off);
        const int ot = __shfl_xor(best_t, off);
        uint32_t of = 0u;                                 // (without repair every flips word is 0 and travels nowhere)
        if constexpr (REPAIR) of = (uint32_t)__shfl_xor((int)best_f, off);
        if (rd_bd_better(of, om, ot, best_f, best_m, best_t)) {
            best_f = of;
            best_m = om;
            best_t = ot;
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
    best_f = REPAIR ? s_f[0] : 0u;
#pragma unroll
    for (int wv = 1; wv < RD_BURST_THREADS / 64; wv++) {
        const uint32_t of = REPAIR ? s_f[wv] : 0u;
        if (rd_bd_better(of, s_m[wv], s_t[wv], best_f, best_m, best_t)) {
            best_f = of;
            best_m = s_m[wv];
            best_t = s_t[wv];
        }
    }
}

// The region decoder.  The region t0 .. t0 + len - 1 lies in LDS, output L0 + j at zl[j] (L0 <= t0, behind a barrier): the
// workgroup's best candidate among tau = t0 + i, SL <= i < len - SL (N - 1), tau >= tau_min (INT32_MIN: no such rule),
// that carries want_id (>= 8: any), sliced around (cr, ci), into every thread's best_f, best_m, best_t (INT32_MAX:
// none).  NARROW puts step 4n in front - the filter gets the samples of zf0 .. zf1 - 1 and zeros beyond, its input lies
// in s's place, so s is written only after z16 has been read - and returns its g (0 otherwise).  Afterwards s[t0 + i] is
// at W.s_s[i], y at W.s_y[i].  Ends behind a barrier.
template <bool REPAIR, bool NARROW>
__device__ __forceinline__ int rd_bd_best_in_region(const uint16_t *zl, int L0, int t0, int len, int zf0, int zf1, int32_t cr, int32_t ci,
                                                    const rd_bd_shape &S, uint32_t want_id, int tau_min,
                                                    const uint32_t *__restrict__ nb_tab, const rd_bd_work &W, unsigned tid,
                                                    uint32_t &best_f, uint64_t &best_m, int &best_t) {
    const int SL = S.sl, N = S.n_sym;
    const unsigned lane = tid & 63u, wave = tid >> 6;
    int g = 0;
    if constexpr (NARROW) {
        const int T = 2 * SL + 5, M = SL + 2;
        uint32_t *z16 = (uint32_t *)W.s_s;                // output t0 - M + i at word i: zeros in front of zf0 and behind zf1
        g = rd_bd_grid_choice(nb_tab, T, cr, ci, lane);
        rd_bd_load_taps(nb_tab, g, T, W.s_hA, W.s_hB, tid);
        rd_bd_fill_z16(z16, zl, L0, t0 - M, len + 2 * M, zf0, zf1, tid);
        __syncthreads();
        rd_bd_filter(z16, len, T, W.s_hA, W.s_hB, W.s_y, tid);
        __syncthreads();                                  // y is whole, and z16 has been read: s may be written
    }
    rd_bd_symbol_sums<NARROW>(zl + (t0 - L0), W.s_y, W.s_s, SL, len, cr, ci, tid);
    __syncthreads();
    // ---- one lane per tau = t0 + i
    best_m = 0ull;
    best_t = INT32_MAX;
    best_f = 0u;
    const int i_hi = len - SL * (N - 1);                  // i + SL (N - 1) < len
    for (int i = SL + (int)tid; i < i_hi; i += RD_BURST_THREADS) {
        const int tau = t0 + i;
        if (tau < tau_min) continue;
        rd_bd_consider<REPAIR>(W.s_s + i, SL, N, S.sync, S.max_flips, W.s_E, want_id, tau, best_f, best_m, best_t);
    }
    rd_bd_reduce_best<REPAIR>(best_f, best_m, best_t, W.s_f, W.s_m, W.s_t, lane, wave);
    return g;
}

// The sum of p (p' with NARROW) over j0 <= j <= j1, the packet's N SL samples, as the four waves' partial sums in s_fr,
// s_fi.  |.| <= 2048 x 2 x 255^2 < 2^29: int; NARROW: a lane's 8 terms of p' < 2^28, the packet's 2047 < 2^36: 64 bits
// before the lanes are added.  Ends behind a barrier.
template <bool NARROW, typename F>
__device__ __forceinline__ void rd_bd_packet_f(const uint16_t *zw, const uint32_t *s_y, int j0, int j1, F *s_fr, F *s_fi, unsigned tid) {
    std::conditional_t<NARROW, long long, int> fr = 0, fi = 0;
    for (int j = j0 + (int)tid; j <= j1; j += RD_BURST_THREADS) {
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
    if ((tid & 63u) == 0u) {
        s_fr[tid >> 6] = fr;
        s_fi[tid >> 6] = fi;
    }
    __syncthreads();
}

// The winner's record, field by field into the slot (one thread; no private copy of the record): its symbols are
// s[SL k] > 0 with those of `flips` corrected; `flags` is the caller's share, bits 1 and 2 are added here.
template <bool REPAIR, bool NARROW, typename F>
__device__ __forceinline__ void rd_bd_write_record(rd_burst_msg *m, int channel, uint32_t first, uint32_t flags, int tau, uint64_t clock,
                                                   uint64_t margin, uint32_t flips, const F *s_fr, const F *s_fi, const int64_t *s,
                                                   int SL, int N, int nb_g) {
    m->channel = channel;
    m->first = first;
    m->tau = tau;
    uint32_t n_flip = 0u;
    int k1 = -1, k2 = -1;                                 // the flipped symbols (REPAIR; none: -1)
    if constexpr (REPAIR) {
        n_flip = flips & 0xFFu;
        if (n_flip >= 1u) k1 = (int)((flips >> 8) & 0xFFu);
        if (n_flip == 2u) k2 = (int)((flips >> 16) & 0xFFu);
    }
    m->flags = flags | (n_flip ? RD_BURST_MSG_REPAIRED : 0u) | (NARROW ? RD_BURST_MSG_NARROW : 0u);
    m->time = clock + (uint64_t)(int64_t)tau;
    m->margin = margin;
    int64_t sfr = 0, sfi = 0;
    for (int wv = 0; wv < RD_BURST_THREADS / 64; wv++) {
        sfr += s_fr[wv];
        sfi += s_fi[wv];
    }
    m->f_re = sfr;
    m->f_im = sfi;
    uint32_t word = 0u, ones = 0u, id = 0u;
    for (int k = 0; k < N; k++) {
        uint32_t bit = s[SL * k] > 0 ? 1u : 0u;
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
    m->pad[3] = (uint8_t)nb_g;                            // (0 without NARROW)
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// the 16 sync symbols, the first in bit 15
static inline uint32_t rd_bd_sync_word(const rd_config *cfg) {
    uint32_t sync = 0u;
    for (int i = 0; i < 16; i++) sync = (sync << 1) | (cfg->preamble[i] ? 1u : 0u);
    return sync;
}

static inline rd_bd_shape rd_bd_shape_of(const rd_config *cfg, int max_flips) {
    return {cfg->symbol_length, cfg->packet_symbols, rd_bd_sync_word(cfg), max_flips};
}

// The form ladder: f(std::bool_constant<REPAIR>(), std::bool_constant<NARROW>()) for the form the two switches ask for -
// f launches its kernel's <REPAIR, NARROW> instantiation and the site checks hipGetLastError behind it
template <typename F>
static inline void rd_bd_with_form(bool repair, bool narrow, F &&f) {
    if (!narrow) {
        if (!repair) f(std::false_type(), std::false_type());
        else f(std::true_type(), std::false_type());
    } else {
        if (!repair) f(std::false_type(), std::true_type());
        else f(std::true_type(), std::true_type());
    }
}

// The argument rule of a launch on a channelized chunk, in this order: max_flips, the pointers, the configuration
// (rd_burst_decode_check), the narrow-band table's symbol_length, stride and alignment.  `what` names the feature.
static inline int rd_burst_launch_check(const rd_config *cfg, const uint8_t *chan_out, const uint8_t *chan_prev, size_t out_stride,
                                        int n_ch, size_t n_out, const void *slot, int max_flips, const uint32_t *narrow_tab,
                                        const char *what) {
    if (max_flips < 0 || max_flips > RD_BD_MAX_FLIPS)
        return rd_fail_msg(RD_ERR_ARG, "burst repair: max_flips %d, not 0 .. %d", max_flips, RD_BD_MAX_FLIPS);
    if (!chan_out || !slot || n_ch < 1) return rd_fail_msg(RD_ERR_ARG, "%s: null argument", what);
    int rc = rd_burst_decode_check(cfg);
    if (rc) return rc;
    if (narrow_tab && cfg->symbol_length < RD_BD_NB_MIN_SL)   // (at most RD_BD_NB_MAX_SL by the check above)
        return rd_fail_msg(RD_ERR_ARG, "%s: narrow-band filter: symbol_length %d, at least %d", what, cfg->symbol_length, RD_BD_NB_MIN_SL);
    if (n_out != (size_t)cfg->block_size || out_stride < 2 * n_out || (out_stride & 15) || ((uintptr_t)chan_out & 15) ||
        ((uintptr_t)chan_prev & 15) || ((uintptr_t)slot & 15))
        return rd_fail_msg(RD_ERR_ARG, "%s: stride %zu for %zu outputs, or a misaligned buffer", what, out_stride, n_out);
    return RD_OK;
}

// The first argument rules of a hook with max_flips and narrow, before its null test
static inline int rd_burst_hook_modes(const rd_config *cfg, int max_flips, int narrow) {
    if (max_flips < 0 || max_flips > RD_BD_MAX_FLIPS)
        return rd_fail_msg(RD_ERR_ARG, "burst repair: max_flips %d, not 0 .. %d", max_flips, RD_BD_MAX_FLIPS);
    if (narrow != 0 && narrow != 1) return rd_fail_msg(RD_ERR_ARG, "narrow-band filter: narrow %d, not 0 or 1", narrow);
    if (narrow && cfg && cfg->symbol_length < RD_BD_NB_MIN_SL)
        return rd_fail_msg(RD_ERR_ARG, "narrow-band filter: symbol_length %d, at least %d", cfg->symbol_length, RD_BD_NB_MIN_SL);
    return RD_OK;
}

// What a rd_debug_burst_* hook holds while its kernel runs alone on host bytes: device copies of cur and prev, up to two
// mapped host slots as the receiver allocates them - filled with 0xA5, so the caller sees which places the kernel left
// alone - and the narrow-band table.  Every step returns RD_OK or the code rd_fail_msg set; the destructor frees all.
struct rd_burst_dbg {
    uint8_t *d_cur = nullptr, *d_prev = nullptr;
    uint8_t *slot[2] = {nullptr, nullptr};               // the host addresses
    void *d_slot[2] = {nullptr, nullptr};                // and the device's
    uint32_t *d_nb = nullptr;

    rd_burst_dbg() = default;
    rd_burst_dbg(const rd_burst_dbg &) = delete;
    rd_burst_dbg &operator=(const rd_burst_dbg &) = delete;
    ~rd_burst_dbg() {
        for (uint8_t *s : slot)
            if (s) hipHostFree(s);
        if (d_cur) hipFree(d_cur);
        if (d_prev) hipFree(d_prev);
        if (d_nb) hipFree(d_nb);
    }
    // the configuration, the symbol_length the feature needs and the stride of the hook's bytes (nothing allocated yet),
    // then the device
    static int check(const rd_config *cfg, size_t stride, const char *what, int min_sl = 1) {
        int rc = rd_burst_decode_check(cfg);
        if (rc) return rc;
        if (cfg->symbol_length < min_sl) return rd_fail_msg(RD_ERR_ARG, "%s: symbol_length %d, at least %d", what, cfg->symbol_length, min_sl);
        const size_t n_out = (size_t)cfg->block_size;
        if (stride < 2 * n_out || (stride & 15)) return rd_fail_msg(RD_ERR_ARG, "%s: stride %zu for %zu outputs", what, stride, n_out);
        return rd_ensure_device();
    }
    int upload(const uint8_t *cur, const uint8_t *prev, size_t bytes) {
        if (hipMalloc(&d_cur, bytes) != hipSuccess || hipMemcpy(d_cur, cur, bytes, hipMemcpyHostToDevice) != hipSuccess)
            return rd_fail_msg(RD_ERR_DEVICE, "the device copy of the chunk failed");
        if (prev && (hipMalloc(&d_prev, bytes) != hipSuccess || hipMemcpy(d_prev, prev, bytes, hipMemcpyHostToDevice) != hipSuccess))
            return rd_fail_msg(RD_ERR_DEVICE, "the device copy of the chunk before failed");
        return RD_OK;
    }
    int map(int i, size_t bytes) {
        if (hipHostMalloc((void **)&slot[i], bytes, hipHostMallocMapped) != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "hipHostMalloc of a slot failed");
        memset(slot[i], 0xA5, bytes);
        if (hipHostGetDevicePointer(&d_slot[i], slot[i], 0) != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "hipHostGetDevicePointer of a slot failed");
        return RD_OK;
    }
    int narrow(int sl) { return rd_bd_narrow_upload(sl, &d_nb); }
    int sync() { return hipDeviceSynchronize() == hipSuccess ? RD_OK : rd_fail_msg(RD_ERR_DEVICE, "hipDeviceSynchronize failed"); }
};
