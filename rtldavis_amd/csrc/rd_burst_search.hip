// rd_burst_search.hip - blind sync-word search behind the narrow-band filter (include/rtldavis_hip.h, BURST SEARCH).
// k_chan_burst_decode needs a run of ON windows, k_chan_burst_expect a station heard before; this kernel needs neither:
// for every channel and every centre g of a short list it filters the whole chunk (and the look-back into the chunk
// before) around g, and tests EVERY output position for the sync word and the CRC, slicing each position around the sum of
// its own 16 sync symbols.  Used by rd_wideband.hip per streamed chunk (rd_wb_set_burst_search), behind
// k_chan_burst_expect on the same stream.
//
// Kernel.  One workgroup of 256 threads per (channel, centre); grid (n_ch, n_centres).  It walks the candidates
// tau_min .. tau_max in tiles of RD_BS_TILE.  A tile with own candidates a .. b evaluates e0 .. e1 = a - (SL - 1) ..
// b + (SL - 1), cut to the candidate range (the rule of step 4s looks SL - 1 positions to either side), and for them needs
//     S[t], e0 <= t <= e1 + SL (N - 1)         (the packet body)
//     y[t], e0 - SL <= t <= e1 + SL (N - 1)    (S[t] sums p'[t - SL + 1 .. t], and p'[u] reads y[u - 1])
//     z[t], M further to either side           (the filter)
// all inside lo .. B - 1 by the candidate range, except z, which is 0 outside it.  Every tile computes its halos again
// from the bytes: what a position gives is a function of the bytes alone, so the result does not depend on the tile size.
// The taps and the filter are the phases of rd_burst_common.h; the z16 load straight from global memory, the int32-pair
// sums, the per-position slicing and the ranking are this kernel's own.
// LDS: S (int32 pair per output, 24.8 KiB; the int16 z of the filter lies in its place before S exists), y (12.6 KiB),
// the candidates' margins (8.8 KiB), the taps: 47.0 KiB, three workgroups per CU.  One lane works per tau; most leave after the sync
// test.  The records of a (centre, channel) are written in tau order by its one workgroup: the reported positions of a
// pass over 256 taus are ranked by ballot and prefix count, no atomics; plain vector stores into the mapped slot.
#include <hip/hip_runtime.h>

#include "rd_burst_common.h"
#include "rd_host.h"

#define RD_BS_MAX_BODY 2048                                           // SL (N - 1) < N SL + 1 <= 2048
#define RD_BS_E_LEN (RD_BS_TILE + 2 * (RD_BD_NB_MAX_SL - 1))          // positions a tile evaluates at most
#define RD_BS_S_LEN (RD_BS_E_LEN + RD_BS_MAX_BODY)
#define RD_BS_Y_LEN (RD_BS_S_LEN + RD_BD_NB_MAX_SL + 1)
static_assert(RD_BS_Y_LEN + 2 * (RD_BD_NB_MAX_SL + 2) <= 2 * RD_BS_S_LEN, "the int16 z of the filter lies in S's place");
static_assert(RD_BS_TILE % RD_BURST_THREADS == 0, "a tile is a whole number of passes");
static_assert(sizeof(rd_bs_header) == 16 && sizeof(rd_burst_msg) == 64, "the slot layout of rd_bs_* (rd_internal.h)");
static_assert(2 * RD_BD_NB_MAX_SL - 1 <= 255, "hits fits a byte");

struct rd_bs_params {
    int sl, n_sym;             // SL, N
    uint32_t sync;             // the 16 sync symbols, the first in bit 15
    int look;                  // LOOK
    int n_ch, n_centres;
    uint8_t centre[RD_BS_MAX_CENTRES];
    uint64_t clock, seq;
};

__global__ __launch_bounds__(RD_BURST_THREADS) void k_chan_burst_search(const uint8_t *__restrict__ cur, const uint8_t *__restrict__ prev,
                                                                     size_t ch_stride, size_t n_out, rd_bs_params P, rd_burst_msg *recs,
                                                                     rd_bs_header *hdr, const uint32_t *__restrict__ nb_tab) {
    __shared__ int2 s_S[RD_BS_S_LEN];                    // S[e0 + i] at i: (re, im)
    __shared__ uint32_t s_y[RD_BS_Y_LEN];                // y[e0 - SL + j] at j: re in the low half, im in the high one
    __shared__ uint64_t s_m[RD_BS_E_LEN];                // margin + 1 of a passing position e0 + i, 0 of any other
    __shared__ uint32_t s_hA[RD_BD_NB_MAX_T], s_hB[RD_BD_NB_MAX_T];   // H[g][kk - M] as (re, -im) and (im, re)
    __shared__ uint32_t s_cnt[RD_BURST_THREADS / 64];
    const int c = (int)blockIdx.x, ci = (int)blockIdx.y;
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const int SL = P.sl, N = P.n_sym, body = SL * (N - 1), M = SL + 2, T = 2 * SL + 5;
    const int B = (int)n_out;
    const int lo = prev ? -P.look : 0;
    const int g = ci < RD_BS_MAX_CENTRES ? (int)P.centre[ci] : RD_BD_NB_GRID;
    rd_bs_header *const my_hdr = hdr + ((size_t)ci * (size_t)P.n_ch + (size_t)c);
    rd_burst_msg *const my_recs = recs + ((size_t)ci * (size_t)P.n_ch + (size_t)c) * RD_BS_PER;
    // What the host's checks guarantee, checked again before anything is indexed by it: a launch that fails is empty.
    const bool sane = c < P.n_ch && ci < P.n_centres && ci < RD_BS_MAX_CENTRES && g < RD_BD_NB_GRID && SL >= RD_BD_NB_MIN_SL &&
                      SL <= RD_BD_NB_MAX_SL && N >= 40 && N <= 8 * RD_BD_DATA_BYTES && (N & 7) == 0 && N * SL + 1 <= RD_BS_MAX_BODY &&
                      n_out <= (size_t)INT32_MAX / 4 && (B & 7) == 0 && (P.look & 7) == 0 && P.look >= N * SL + 1 && P.look <= B &&
                      ch_stride >= 2 * n_out;
    int32_t tau_min = 0, tau_max = -1;                   // step 2s (rd_host.h)
    if (!sane || !rd_bs_range(SL, N, B, P.look, prev != nullptr, &tau_min, &tau_max)) {
        if (tid == 0u && c < P.n_ch && ci < P.n_centres) {
            rd_bs_header h;
            h.n_msgs = 0u;
            h.sync_hits = 0u;
            h.chunk = (uint32_t)P.seq;
            h.dropped = 0u;
            *my_hdr = h;
        }
        return;
    }
    const uint8_t *src = cur + (size_t)c * ch_stride;
    const uint8_t *src_prev = prev ? prev + (size_t)c * ch_stride : nullptr;
    rd_bd_load_taps(nb_tab, g, T, s_hA, s_hB, tid);
    uint32_t my_sync = 0u;                               // this thread's positions whose first 16 symbols equal sync
    uint32_t n_rep = 0u;                                 // reported positions so far (uniform)
    for (int a = tau_min; a <= tau_max; a += RD_BS_TILE) {
        const int b = min(a + RD_BS_TILE - 1, tau_max);
        const int e0 = max(a - (SL - 1), tau_min), e1 = min(b + (SL - 1), tau_max);
        const int nE = e1 - e0 + 1, nS = nE + body, nY = nS + SL, nZ = nY + 2 * M;
        const int zt0 = e0 - SL - M;                     // z16 word i holds output zt0 + i; y word j output e0 - SL + j
        __syncthreads();                                 // the tile before has been read (and the taps are written)
        // ---- z as int16 pairs: groups of 8 outputs, each wholly inside lo .. B - 1 of one chunk or wholly outside
        uint32_t *z16 = (uint32_t *)s_S;
        {
            const int g0 = zt0 & ~7, g1 = (zt0 + nZ + 7) & ~7;
            for (int t = g0 + 8 * (int)tid; t < g1; t += 8 * RD_BURST_THREADS) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                const bool in = t >= lo && t < B;
                if (in) v = *(const uint4 *)(t < 0 ? src_prev + 2 * ((long)t + (long)n_out) : src + 2 * (long)t);
                const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    const int i = t + q - zt0;
                    if (i < 0 || i >= nZ) continue;
                    const uint32_t h = (w4[q >> 1] >> (16 * (q & 1))) & 0xFFFFu;
                    z16[i] = in ? rd_bd_pack16(2 * (int)(h & 0xFFu) - 255, 2 * (int)(h >> 8) - 255) : 0u;
                }
            }
        }
        __syncthreads();
        rd_bd_filter(z16, nY, T, s_hA, s_hB, s_y, tid);   // y[e0 - SL + j] at word j
        __syncthreads();                                 // y is whole, and z16 has been read: S may be written
        // ---- S[e0 + i] = sum of p' at y words i + 1 .. i + SL: a lane takes a stretch and slides the window along it
        {
            const int per = (nS + RD_BURST_THREADS - 1) / RD_BURST_THREADS;
            const int ia = (int)tid * per, ib = min(ia + per, nS);
            if (ia < ib) {
                int sr = 0, si = 0, re, im;
                for (int j = ia + 1; j <= ia + SL; j++) {
                    rd_bd_pn(s_y, j, re, im);
                    sr += re;
                    si += im;
                }
                s_S[ia] = make_int2(sr, si);
                for (int i = ia + 1; i < ib; i++) {
                    rd_bd_pn(s_y, i + SL, re, im);
                    sr += re;
                    si += im;
                    rd_bd_pn(s_y, i, re, im);
                    sr -= re;
                    si -= im;
                    s_S[i] = make_int2(sr, si);
                }
            }
        }
        __syncthreads();
        // ---- one lane per position e0 + i: step 3s
        for (int i = (int)tid; i < nE; i += RD_BURST_THREADS) {
            int sr[16], si[16];
            long long dr = 0, di = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int2 v = s_S[i + SL * k];
                sr[k] = v.x;
                si[k] = v.y;
                dr += v.x;
                di += v.y;
            }
            uint64_t m1 = 0ull;
            const unsigned long long adr = (unsigned long long)(dr < 0 ? -dr : dr), adi = (unsigned long long)(di < 0 ? -di : di);
            const unsigned long long big = adr > adi ? adr : adi;
            if (big != 0ull) {
                const int sh = max(0, 64 - __clzll((long long)big) - 15);
                const long long ca = dr >> sh, cb = di >> sh;   // (floor; each in -2^15 .. 2^15 - 1)
                if (ca != 0 || cb != 0) {
                    uint32_t word = 0u;
                    uint64_t margin = ~0ull;
#pragma unroll
                    for (int k = 0; k < 16; k++) {
                        const long long v = (long long)si[k] * ca - (long long)sr[k] * cb;
                        word = (word << 1) | (v > 0 ? 1u : 0u);
                        const uint64_t mag = (uint64_t)(v > 0 ? v : -v);
                        margin = mag < margin ? mag : margin;
                    }
                    if (word == P.sync) {
                        const int tau = e0 + i;
                        if (tau >= a && tau <= b) my_sync++;     // (a halo position is another tile's own)
                        uint32_t crc = 0u;
                        word = 0u;
                        for (int k = 16; k < N; k++) {
                            const int2 sv = s_S[i + SL * k];
                            const long long v = (long long)sv.y * ca - (long long)sv.x * cb;
                            const uint64_t mag = (uint64_t)(v > 0 ? v : -v);
                            margin = mag < margin ? mag : margin;
                            word = ((word << 1) | (v > 0 ? 1u : 0u)) & 0xFFu;
                            if ((k & 7) == 7) crc = rd_crc16_step(crc, rd_swap_bits8(word));
                        }
                        if (crc == 0u) m1 = margin + 1ull;        // (|s| < 2^47)
                    }
                }
            }
            s_m[i] = m1;
        }
        __syncthreads();
        // ---- step 4s over the tile's own positions a .. b, in passes of 256 ascending taus; step 5s
        for (int p0 = a; p0 <= b; p0 += RD_BURST_THREADS) {  // (uniform: every thread makes every pass)
            const int tau = p0 + (int)tid, i = tau - e0;
            bool rep = false;
            uint32_t hits = 0u;
            uint64_t mine = 0ull;
            if (tau <= b && (mine = s_m[i]) != 0ull) {
                rep = true;
                const int j0 = max(i - (SL - 1), 0), j1 = min(i + (SL - 1), nE - 1);
                for (int j = j0; j <= j1; j++) {
                    const uint64_t o = s_m[j];
                    if (o == 0ull) continue;
                    hits++;
                    if (o > mine || (o == mine && j < i)) rep = false;
                }
            }
            const unsigned long long mask = __ballot(rep);
            if (lane == 0u) s_cnt[wave] = (uint32_t)__popcll(mask);
            __syncthreads();
            uint32_t rank = n_rep, total = 0u;
#pragma unroll
            for (unsigned wv = 0; wv < RD_BURST_THREADS / 64; wv++) {
                const uint32_t n = s_cnt[wv];
                if (wv < wave) rank += n;
                total += n;
            }
            rank += (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            n_rep += total;
            if (rep && rank < (uint32_t)RD_BS_PER) {      // field by field into the slot: no private copy of the record
                rd_burst_msg *m = my_recs + rank;
                long long dr = 0, di = 0;
                for (int k = 0; k < 16; k++) {
                    const int2 v = s_S[i + SL * k];
                    dr += v.x;
                    di += v.y;
                }
                const unsigned long long adr = (unsigned long long)(dr < 0 ? -dr : dr), adi = (unsigned long long)(di < 0 ? -di : di);
                const int sh = max(0, 64 - __clzll((long long)(adr > adi ? adr : adi)) - 15);
                const long long ca = dr >> sh, cb = di >> sh;
                long long fr = 0, fi = 0;
                uint32_t word = 0u, ones = 0u, id = 0u;
                for (int k = 0; k < N; k++) {
                    const int2 sv = s_S[i + SL * k];
                    fr += sv.x;
                    fi += sv.y;
                    const uint32_t bit = (long long)sv.y * ca - (long long)sv.x * cb > 0 ? 1u : 0u;
                    ones += bit;
                    word = ((word << 1) | bit) & 0xFFu;
                    if ((k & 7) == 7) m->data[k >> 3] = (uint8_t)word;
                    if (k == 23) id = rd_swap_bits8(word) & 7u;   // symbols 16, 17, 18 are its bits 0, 1, 2
                }
                for (int k = N >> 3; k < RD_BD_DATA_BYTES; k++) m->data[k] = 0;
                m->channel = c;
                m->first = (uint32_t)ci;
                m->tau = tau;
                m->flags = RD_BURST_MSG_SEARCHED | RD_BURST_MSG_NARROW | (tau - SL < 0 ? 1u : 0u);
                m->time = P.clock + (uint64_t)(int64_t)tau;
                m->margin = mine - 1ull;
                m->f_re = fr;
                m->f_im = fi;
                m->ones = (uint8_t)ones;
                m->id = (uint8_t)id;
                m->pad[0] = (uint8_t)hits;
                m->pad[1] = 0;
                m->pad[2] = 0;
                m->pad[3] = (uint8_t)g;
            }
            __syncthreads();                              // s_cnt is read: the next pass may write it
        }
    }
    // ---- the header: the threads' sync counts, summed in a fixed tree
    uint32_t sy = my_sync;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sy += (uint32_t)__shfl_xor((int)sy, off);
    __syncthreads();
    if (lane == 0u) s_cnt[wave] = sy;
    __syncthreads();
    if (tid == 0u) {
        rd_bs_header h;
        h.n_msgs = n_rep < (uint32_t)RD_BS_PER ? n_rep : (uint32_t)RD_BS_PER;
        h.sync_hits = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        h.chunk = (uint32_t)P.seq;
        h.dropped = n_rep > (uint32_t)RD_BS_PER ? n_rep - (uint32_t)RD_BS_PER : 0u;
        *my_hdr = h;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// what the launch and the hook test first: the configuration pointer, the channels, the centres
static int rd_bs_check_args(const rd_config *cfg, int n_ch, const uint8_t *centres, int n) {
    if (!cfg || !centres || n_ch < 1 || n_ch > RD_BS_MAX_CHANNELS)
        return rd_fail_msg(RD_ERR_ARG, "burst search: null argument or %d channels", n_ch);
    int bad = -1;
    const char *why = "";
    if (n < 1 || rd_bs_check_centres(centres, n, &bad, &why)) {
        if (bad < 0) return rd_fail_msg(RD_ERR_ARG, "burst search: %d centres, not 1 .. %d", n, RD_BS_MAX_CENTRES);
        return rd_fail_msg(RD_ERR_ARG, "burst search: centre %d: %s", bad, why);
    }
    return RD_OK;
}

int rd_burst_search_launch(const rd_config *cfg, const uint8_t *chan_out, const uint8_t *chan_prev, size_t out_stride, int n_ch,
                           size_t n_out, uint64_t clock, uint64_t seq, const uint8_t *centres, int n, const uint32_t *narrow_tab,
                           void *slot_dev, hipStream_t st) {
    int rc = rd_bs_check_args(cfg, n_ch, centres, n);
    if (rc) return rc;
    if (!narrow_tab) return rd_fail_msg(RD_ERR_ARG, "burst search: null argument");
    if ((rc = rd_burst_launch_check(cfg, chan_out, chan_prev, out_stride, n_ch, n_out, slot_dev, 0, narrow_tab, "burst search"))) return rc;
    rd_bs_params P;
    P.sl = cfg->symbol_length;
    P.n_sym = cfg->packet_symbols;
    P.sync = rd_bd_sync_word(cfg);
    P.look = RD_BU_WINDOW * rd_bd_look_windows(cfg);
    P.n_ch = n_ch;
    P.n_centres = n;
    for (int i = 0; i < RD_BS_MAX_CENTRES; i++) P.centre[i] = i < n ? centres[i] : (uint8_t)RD_BD_NB_GRID;
    P.clock = clock;
    P.seq = seq;
    uint8_t *base = (uint8_t *)slot_dev;
    hipLaunchKernelGGL(k_chan_burst_search, dim3((unsigned)n_ch, (unsigned)n), dim3(RD_BURST_THREADS), 0, st, chan_out, chan_prev, out_stride,
                       n_out, P, (rd_burst_msg *)base, (rd_bs_header *)(base + rd_bs_header_offset(n_ch)), narrow_tab);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "k_chan_burst_search: %s", hipGetErrorString(e));
    return RD_OK;
}

// Test hook (tests/test_burst_search.py): k_chan_burst_search alone on host bytes, through rd_burst_search_launch and a
// mapped host slot as the receiver allocates it, filled with 0xA5 and copied out whole.
extern "C" int rd_debug_burst_search(const rd_config *cfg, const uint8_t *cur, const uint8_t *prev, size_t stride, int n_ch,
                                     uint64_t clock, uint64_t seq, const uint8_t *centres, int n, rd_burst_msg *msgs_out,
                                     rd_bs_header *hdr_out) {
    if (!cur || !msgs_out || !hdr_out) return rd_fail_msg(RD_ERR_ARG, "burst search: null argument or %d channels", n_ch);
    int rc = rd_bs_check_args(cfg, n_ch, centres, n);
    if (rc || (rc = rd_burst_dbg::check(cfg, stride, "burst search", RD_BD_NB_MIN_SL))) return rc;   // (nothing allocated, nothing launched)
    rd_burst_dbg D;
    if ((rc = D.upload(cur, prev, (size_t)n_ch * stride)) || (rc = D.map(0, rd_bs_slot_bytes(n_ch))) || (rc = D.narrow(cfg->symbol_length)) ||
        (rc = rd_burst_search_launch(cfg, D.d_cur, D.d_prev, stride, n_ch, (size_t)cfg->block_size, clock, seq, centres, n, D.d_nb, D.d_slot[0],
                                     nullptr)) ||
        (rc = D.sync()))
        return rc;
    memcpy(msgs_out, D.slot[0], rd_bs_header_offset(n_ch));
    memcpy(hdr_out, D.slot[0] + rd_bs_header_offset(n_ch), (size_t)RD_BS_MAX_CENTRES * (size_t)n_ch * sizeof(rd_bs_header));
    return RD_OK;
}
