// rd_burst_quality.hip - power, noise and clipping of every burst record (include/rtldavis_hip.h, BURST QUALITY).
// k_chan_burst_decode and k_chan_burst_expect write rd_burst_msg records into mapped slots; this kernel is launched
// behind each of them on the same stream, reads the records back the way k_chan_burst_decode reads the slot k_chan_bursts
// filled, and writes one rd_burst_quality per record into a mapped slot of its own.  The kernels in front stay what they
// were.  Used by rd_wideband.hip per streamed chunk (rd_wb_set_burst_quality).
//
// One kernel, two launches.  Both slots are "groups of `cap` record places with a 16-byte header per group whose first
// word is n_msgs and whose third is the chunk number": the decode slot has n_ch groups of cap = rd_bu_cap(n_win) places,
// the expect slot RD_BX_MAX groups of one place.  The kernel takes (recs, cap, hdr, n_groups, qual) and walks the first
// min(n_msgs, cap) places of its group; quality record [group][place] lies where the message record does.
//
// Kernel.  One workgroup of 256 threads per group, one record after the other.  Thread 0 fetches channel, tau, f_re and
// f_im with system-scope loads into LDS.  The windows are rd_bq_windows_of's (rd_host.h), evaluated again here: a record
// whose channel or packet lies outside the two chunks gets flags bit 7 and zeros, and nothing is indexed by it.  Region
// R0 = the noise window's first output (the packet's when n_noise = 0) .. R1 = the packet's end: at most 1024 + 16 x 51 +
// 2047 = 3887 <= RD_BQ_LEN = 4096 outputs.  The filter needs M = SL + 2 outputs more on either side where the two
// chunks hold them (zf0 .. zf1); the bytes are loaded as 16-byte vectors from L0 = zf0 rounded DOWN to 8 up to zf1
// rounded up - lo_lim and block_size are multiples of 8, so a vector lies in one chunk and inside it.  z goes to LDS as
// int16 pairs, output R0 - M + i at word i, zeros outside zf0 .. zf1.  Bytes, grid choice, taps and z are the phases of
// rd_burst_common.h; the sums are this kernel's own: a lane takes the outputs R0 + tid + 256 j; one in
// the gap between noise and packet is skipped; y is 2 T packed 16-bit dot products (rd_bd_dot2); the eight sums are
// per-lane partials, a fixed tree of shuffles, then LDS across the four waves - integer sums, the same bits on every run.
// Thread 0 writes the record field by field with plain vector stores; no atomics.
// LDS: the bytes (RD_BQ_LOAD x 2 = 8.25 KiB), z16 ((RD_BQ_LEN + 2 x 53) x 4 = 16.4 KiB), the taps (2 x 107 x 4), the
// waves' partials: under 27 KiB.
#include <cstddef>

#include <hip/hip_runtime.h>

#include "rd_burst_common.h"

#define RD_BQ_LEN 4096                                    // outputs of a region at most
#define RD_BQ_NB_MAX_M (RD_BD_NB_MAX_SL + 2)
#define RD_BQ_LOAD (RD_BQ_LEN + 128)                      // outputs loaded at most
#define RD_BQ_SUMS 8                                      // pkt, sig, noise, pkt_nb, sig_nb, noise_nb, clipped, peak
static_assert(RD_BQ_MAX_GAP + 16 * RD_BD_NB_MAX_SL + RD_BD_MAX_LOOK_W * RD_BU_WINDOW <= RD_BQ_LEN, "gap + noise + packet fit the region");
static_assert(RD_BQ_LEN + 2 * RD_BQ_NB_MAX_M + 14 <= RD_BQ_LOAD && RD_BQ_LOAD % 8 == 0, "the filter's margins and the rounding to 8");
static_assert(RD_BQ_LOAD * 2 + (RD_BQ_LEN + 2 * RD_BQ_NB_MAX_M) * 4 + 2 * RD_BD_NB_MAX_T * 4 + (RD_BURST_THREADS / 64) * RD_BQ_SUMS * 8 + 64 <= 32768,
              "the LDS budget of the file header");
static_assert(sizeof(rd_burst_quality) == 64 && sizeof(rd_bq_header) == 16 && sizeof(rd_bd_header) == 16 && sizeof(rd_bx_header) == 16,
              "one header shape for both slots, one record layout");
static_assert(offsetof(rd_bd_header, n_msgs) == 0 && offsetof(rd_bd_header, chunk) == 8 && offsetof(rd_bx_header, n_msgs) == 0 &&
                  offsetof(rd_bx_header, chunk) == 8 && offsetof(rd_bq_header, chunk) == 8, "n_msgs first, the chunk number third");
static_assert(2047ull * 130050ull < (1ull << 28) && 2ull * 3192ull * 3192ull < (1ull << 25), "the bounds of the header");

struct rd_bq_params {
    int sl, n_sym;             // SL, N
    int block;                 // B
    int have_prev;
    int n_ch;
    int gap;
    int inband;                // SL >= 4 and the tables are there
};

__global__ __launch_bounds__(RD_BURST_THREADS) void k_chan_burst_quality(const uint8_t *__restrict__ cur, const uint8_t *__restrict__ prev,
                                                                      size_t ch_stride, rd_bq_params P, const rd_burst_msg *recs,
                                                                      uint32_t cap, const rd_bq_header *hdr, rd_burst_quality *qual,
                                                                      const uint32_t *__restrict__ nb_tab) {
    __shared__ uint4 s_z[RD_BQ_LOAD / 8];                 // the loaded bytes: output L0 + i at bytes 2 i, 2 i + 1
    __shared__ uint32_t s_z16[RD_BQ_LEN + 2 * RD_BQ_NB_MAX_M];   // z as int16 pairs: output R0 - M + i at word i
    __shared__ uint32_t s_hA[RD_BD_NB_MAX_T], s_hB[RD_BD_NB_MAX_T];   // H[g][kk - M] as (re, -im) and (im, re)
    __shared__ unsigned long long s_red[RD_BURST_THREADS / 64][RD_BQ_SUMS];
    __shared__ int64_t s_rec[4];                          // the record: channel, tau, f_re, f_im
    __shared__ uint32_t s_hd[2];                          // the header: n_msgs, chunk
    const unsigned grp = blockIdx.x;
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0u) {                                      // one thread crosses the bus, the workgroup takes it from LDS
        s_hd[0] = rd_bd_sys_load(&hdr[grp].n_msgs);
        s_hd[1] = rd_bd_sys_load(&hdr[grp].chunk);
    }
    __syncthreads();
    const uint32_t n_rec = s_hd[0] < cap ? s_hd[0] : cap, chunk = s_hd[1];   // (workgroup-uniform)
    const int SL = P.sl, N = P.n_sym;
    const int lo_lim = P.have_prev && prev ? -P.block : 0;
    const uint16_t *zl = (const uint16_t *)s_z;           // output L0 + i: I in the low byte, Q in the high one
    for (uint32_t r = 0; r < n_rec; r++) {
        const rd_burst_msg *m = &recs[(size_t)grp * cap + r];
        rd_burst_quality *q = &qual[(size_t)grp * cap + r];
        __syncthreads();                                  // the record before has been read out of LDS
        if (tid == 0u) {
            s_rec[0] = (int64_t)rd_bd_sys_load(&m->channel);
            s_rec[1] = (int64_t)rd_bd_sys_load(&m->tau);
            s_rec[2] = rd_bd_sys_load(&m->f_re);
            s_rec[3] = rd_bd_sys_load(&m->f_im);
        }
        __syncthreads();
        const int64_t c64 = s_rec[0], tau = s_rec[1], fr = s_rec[2], fi = s_rec[3];   // (uniform from here on)
        rd_bq_windows w;
        // What the decoders guarantee, checked again before anything is indexed by it
        bool ok = rd_bq_windows_of(SL, N, P.block, lo_lim < 0 ? 1 : 0, tau, P.gap, &w) && c64 >= 0 && c64 < (int64_t)P.n_ch;
        const bool inband = P.inband && (fr != 0 || fi != 0);
        const int M = inband ? SL + 2 : 0, T = 2 * SL + 5;
        const int n_noise = ok ? w.n1 - w.n0 : 0;
        const int R0 = n_noise > 0 ? w.n0 : w.p0, R1 = w.p1, len = R1 - R0;
        const int zf0 = max(R0 - M, lo_lim), zf1 = min(R1 + M, P.block);
        const int L0 = zf0 & ~7, L1 = (zf1 + 7) & ~7;       // (floor and ceiling: lo_lim and B are multiples of 8)
        ok = ok && len >= 1 && len <= RD_BQ_LEN && L1 - L0 <= RD_BQ_LOAD && L0 >= lo_lim && L1 <= P.block;
        if (!ok) {
            if (tid == 0u) {
                q->pkt = 0ull; q->sig = 0ull; q->noise = 0ull;
                q->pkt_nb = 0ull; q->sig_nb = 0ull; q->noise_nb = 0ull;
                q->n_noise = 0u; q->clipped = 0u;
                q->peak = 0; q->g = 0; q->flags = (uint8_t)RD_BQ_UNMEASURABLE;
                q->chunk = chunk;
            }
            continue;
        }
        const uint8_t *src = cur + (size_t)c64 * ch_stride;
        const uint8_t *src_prev = prev ? prev + (size_t)c64 * ch_stride : nullptr;
        rd_bd_load_bytes(s_z, src, src_prev, L0, L1, (long)P.block, tid);   // (L0 < 0 only with lo_lim < 0: there is a chunk before)
        int nb_g = 0;
        if (inband) {
            // ---- sh, ca, cb and g of step 4n from the record's own f: the same in every wave
            const uint64_t mr = fr < 0 ? 0ull - (uint64_t)fr : (uint64_t)fr, mi = fi < 0 ? 0ull - (uint64_t)fi : (uint64_t)fi;
            const int bl = 64 - __clzll((long long)(mr > mi ? mr : mi));   // (not both 0: at least 1)
            const int sh = bl > 15 ? bl - 15 : 0;
            const int ca = (int)(fr >> sh), cb = (int)(fi >> sh);          // each in -2^15 .. 2^15 - 1
            nb_g = rd_bd_grid_choice(nb_tab, T, ca, cb, lane);
            rd_bd_load_taps(nb_tab, nb_g, T, s_hA, s_hB, tid);
        }
        __syncthreads();
        rd_bd_fill_z16(s_z16, zl, L0, R0 - M, len + 2 * M, zf0, zf1, tid);
        __syncthreads();
        // ---- the sums: output R0 + i, i = tid + 256 j
        unsigned long long a_pkt = 0ull, a_sig = 0ull, a_noise = 0ull, a_pkt_nb = 0ull, a_sig_nb = 0ull, a_noise_nb = 0ull;
        uint32_t a_clip = 0u, a_peak = 0u;
        for (int i = (int)tid; i < len; i += RD_BURST_THREADS) {
            const int t = R0 + i;
            const bool in_pkt = t >= w.p0, in_sig = in_pkt && t < w.s1, in_noise = n_noise > 0 && t < w.n1;
            if (!in_pkt && !in_noise) continue;           // the gap
            const uint32_t zv = s_z16[i + M];
            const int zr = (int)(int16_t)(zv & 0xFFFFu), zi = (int)zv >> 16;
            const uint32_t e = (uint32_t)(zr * zr + zi * zi);
            uint32_t e_nb = 0u;
            if (inband) {
                // y[t] = (sum_kk H[g][kk - M] z[t - (kk - M)] + 2^10) >> 11: z[..] lies at word i + 2 M - kk
                int ar = 0, ai = 0;
                const uint32_t *zp = &s_z16[i + 2 * M];
                for (int kk = 0; kk < T; kk++) {
                    const uint32_t x = zp[-kk];
                    ar = rd_bd_dot2(s_hA[kk], x, ar);
                    ai = rd_bd_dot2(s_hB[kk], x, ai);
                }
                const int yr = rd_bd_round(ar), yi = rd_bd_round(ai);
                e_nb = (uint32_t)(yr * yr + yi * yi);     // < 2^25
            }
            if (in_noise) {
                a_noise += e;
                a_noise_nb += e_nb;
            } else {
                const uint32_t mr = (uint32_t)(zr < 0 ? -zr : zr), mi = (uint32_t)(zi < 0 ? -zi : zi), mx = mr > mi ? mr : mi;
                a_pkt += e;
                a_pkt_nb += e_nb;
                a_peak = mx > a_peak ? mx : a_peak;
                a_clip += (mr == 255u ? 1u : 0u) + (mi == 255u ? 1u : 0u);   // a = +-255: the byte is 255 or 0
                if (in_sig) {
                    a_sig += e;
                    a_sig_nb += e_nb;
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            a_pkt += __shfl_xor(a_pkt, off);
            a_sig += __shfl_xor(a_sig, off);
            a_noise += __shfl_xor(a_noise, off);
            a_pkt_nb += __shfl_xor(a_pkt_nb, off);
            a_sig_nb += __shfl_xor(a_sig_nb, off);
            a_noise_nb += __shfl_xor(a_noise_nb, off);
            a_clip += (uint32_t)__shfl_xor((int)a_clip, off);
            const uint32_t op = (uint32_t)__shfl_xor((int)a_peak, off);
            a_peak = op > a_peak ? op : a_peak;
        }
        if (lane == 0u) {
            s_red[wave][0] = a_pkt;
            s_red[wave][1] = a_sig;
            s_red[wave][2] = a_noise;
            s_red[wave][3] = a_pkt_nb;
            s_red[wave][4] = a_sig_nb;
            s_red[wave][5] = a_noise_nb;
            s_red[wave][6] = a_clip;
            s_red[wave][7] = a_peak;
        }
        __syncthreads();
        if (tid == 0u) {                                  // field by field into the slot: no private copy of the record
            unsigned long long t[RD_BQ_SUMS];
#pragma unroll
            for (int k = 0; k < RD_BQ_SUMS; k++) t[k] = s_red[0][k];
#pragma unroll
            for (int wv = 1; wv < RD_BURST_THREADS / 64; wv++) {
#pragma unroll
                for (int k = 0; k < RD_BQ_SUMS - 1; k++) t[k] += s_red[wv][k];
                t[7] = s_red[wv][7] > t[7] ? s_red[wv][7] : t[7];
            }
            q->pkt = t[0];
            q->sig = t[1];
            q->noise = t[2];
            q->pkt_nb = t[3];
            q->sig_nb = t[4];
            q->noise_nb = t[5];
            q->n_noise = (uint32_t)n_noise;
            q->clipped = (uint32_t)t[6];
            q->peak = (uint16_t)t[7];
            q->g = (uint8_t)nb_g;
            q->flags = (uint8_t)(inband ? RD_BQ_INBAND : 0u);
            q->chunk = chunk;
        }
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
int rd_burst_quality_launch(const rd_config *cfg, const uint8_t *chan_out, const uint8_t *chan_prev, size_t out_stride, int n_ch,
                            size_t n_out, int noise_gap, const uint32_t *narrow_tab, const rd_burst_msg *recs, size_t cap,
                            const rd_bq_header *hdr, int n_groups, rd_burst_quality *qual, hipStream_t st) {
    if (noise_gap < 0 || noise_gap > RD_BQ_MAX_GAP)
        return rd_fail_msg(RD_ERR_ARG, "burst quality: noise_gap %d, not 0 .. %d", noise_gap, RD_BQ_MAX_GAP);
    if (!chan_out || !recs || !hdr || !qual || n_ch < 1 || n_groups < 1 || cap < 1 || cap > RD_BU_MAX_WINDOWS)
        return rd_fail_msg(RD_ERR_ARG, "burst quality: null argument, %d groups or %zu places", n_groups, cap);
    int rc = rd_burst_decode_check(cfg);
    if (rc) return rc;
    if (!narrow_tab && cfg->symbol_length >= RD_BD_NB_MIN_SL)
        return rd_fail_msg(RD_ERR_ARG, "burst quality: symbol_length %d needs the narrow-band tables", cfg->symbol_length);
    if (n_out != (size_t)cfg->block_size || (n_out & 7) || out_stride < 2 * n_out || (out_stride & 15) || ((uintptr_t)chan_out & 15) ||
        ((uintptr_t)chan_prev & 15) || ((uintptr_t)qual & 7))
        return rd_fail_msg(RD_ERR_ARG, "burst quality: stride %zu for %zu outputs, or a misaligned buffer", out_stride, n_out);
    rd_bq_params P;
    P.sl = cfg->symbol_length;
    P.n_sym = cfg->packet_symbols;
    P.block = cfg->block_size;
    P.have_prev = chan_prev ? 1 : 0;
    P.n_ch = n_ch;
    P.gap = noise_gap;
    P.inband = cfg->symbol_length >= RD_BD_NB_MIN_SL ? 1 : 0;   // (at most RD_BD_NB_MAX_SL by the check above)
    hipLaunchKernelGGL(k_chan_burst_quality, dim3((unsigned)n_groups), dim3(RD_BURST_THREADS), 0, st, chan_out, chan_prev, out_stride, P,
                       recs, (uint32_t)cap, hdr, qual, narrow_tab);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "k_chan_burst_quality: %s", hipGetErrorString(e));
    return RD_OK;
}

// Test hook (tests/test_burst_quality.py): k_chan_burst_quality alone on host bytes and on the records the caller
// supplies, through rd_burst_quality_launch and mapped host slots as the receiver allocates them; the quality slot is
// filled with 0xA5 and copied out whole.
extern "C" int rd_debug_burst_quality(const rd_config *cfg, const uint8_t *cur, const uint8_t *prev, size_t stride, int n_ch,
                                      int noise_gap, const rd_burst_msg *msgs, const uint32_t *n_msgs_per_channel,
                                      rd_burst_quality *out) {
    if (noise_gap < 0 || noise_gap > RD_BQ_MAX_GAP)
        return rd_fail_msg(RD_ERR_ARG, "burst quality: noise_gap %d, not 0 .. %d", noise_gap, RD_BQ_MAX_GAP);
    if (!cfg || !cur || !msgs || !n_msgs_per_channel || !out || n_ch < 1) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = rd_burst_decode_check(cfg);
    if (rc) return rc;                               // (nothing allocated, nothing launched)
    const size_t n_out = (size_t)cfg->block_size, n_win = n_out / RD_BU_WINDOW, cap = rd_bu_cap(n_win);
    for (int c = 0; c < n_ch; c++)
        if (n_msgs_per_channel[c] > cap) return rd_fail_msg(RD_ERR_ARG, "burst quality: %u records in channel %d, room for %zu", n_msgs_per_channel[c], c, cap);
    if ((rc = rd_burst_dbg::check(cfg, stride, "burst quality"))) return rc;   // (the stride, then the device: no device work for a wrong argument)
    const size_t bq_bytes = rd_bq_slot_bytes(n_ch, n_win);
    rd_burst_dbg D;                                     // slot 0: the decode slot, slot 1: the quality slot
    if ((rc = D.upload(cur, prev, (size_t)n_ch * stride)) || (rc = D.map(0, rd_bd_slot_bytes(n_ch, n_win))) || (rc = D.map(1, bq_bytes)) ||
        (cfg->symbol_length >= RD_BD_NB_MIN_SL && (rc = D.narrow(cfg->symbol_length))))
        return rc;
    memcpy(D.slot[0], msgs, (size_t)n_ch * cap * sizeof(rd_burst_msg));
    rd_bd_header *h = (rd_bd_header *)(D.slot[0] + rd_bd_header_offset(n_ch, n_win));
    for (int c = 0; c < n_ch; c++) {
        h[c].n_msgs = n_msgs_per_channel[c];
        h[c].long_runs = 0u;
        h[c].chunk = RD_BQ_DEBUG_CHUNK;
        h[c].pad = 0u;
    }
    if ((rc = rd_burst_quality_launch(cfg, D.d_cur, D.d_prev, stride, n_ch, n_out, noise_gap, D.d_nb, (const rd_burst_msg *)D.d_slot[0], cap,
                                      (const rd_bq_header *)((uint8_t *)D.d_slot[0] + rd_bd_header_offset(n_ch, n_win)), n_ch,
                                      (rd_burst_quality *)D.d_slot[1], nullptr)) ||
        (rc = D.sync()))
        return rc;
    memcpy(out, D.slot[1], bq_bytes);
    return RD_OK;
}
