// rd_device.h - what the kernel files of the IQ -> bits -> packets path share (rd_tail.hip, rd_tail_kernels.hip,
// rd_stream_kernels.hip, rd_parse_kernels.hip, rd_stage_kernels.hip): the views of a layout, the launch helpers, the bit
// fetches, the wave sums, the RSSI family, rd_wave_parse and the record stores.  py = the reference's src/rtldavis/dsp.py
#pragma once
#include <algorithm>
#include <cstdlib>

#include <hip/hip_ext.h>

#include "rd_internal.h"
#include "rd_math.h"
#include "rd_mfma.h"
#include "rd_parse.h"

// ---- views: one stream of a layout (the index widened as its own type is), the complex ring of a layout ----
template <class Index>
RD_HD rd_stream_view rd_view_of(const rd_layout &lay, Index stream) {
    rd_stream_view v;
    v.base = lay.iq + (size_t)stream * lay.stream_stride;
    v.valid_from = lay.valid_from;
    v.n = lay.n_samples;
    return v;
}
static inline rd_cplx_view rd_cplx_view_of(const rd_cplx_layout &lay) { return rd_cplx_view{lay.x, lay.valid_from, lay.n}; }

// ---- launches ----
// One launch whose end is stamped into ev_stop when there is one: the dispatch records the event itself (no marker
// packet behind the kernel).
template <class... P, class... A>
static inline void rd_launch_ev(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, hipEvent_t ev_stop, A... args) {
    if (ev_stop)
        hipExtLaunchKernelGGL(kernel, grid, block, (unsigned)lds, st, nullptr, ev_stop, 0, args...);
    else
        hipLaunchKernelGGL(kernel, grid, block, (unsigned)lds, st, args...);
}
// the grid of a launch with one thread of a 256-thread workgroup per item
static inline dim3 rd_grid256(size_t n) { return dim3((unsigned)((n + 255) / 256)); }
// raises a kernel's limit of dynamic LDS, once per process (`done`: the caller's static flag)
static inline void rd_allow_lds(const void *kernel, int bytes, bool &done) {
    if (done) return;
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    done = true;
}

// ---- diagnostic library: a phase stamp (s_memrealtime, 100 MHz) into `slot` from the lanes for which `who` holds ----
#ifdef RD_DIAG
#define RD_STAMP(who, slot) do { if (who) { uint64_t t_; asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) : : "memory"); \
                                            (slot) = t_; } } while (0)
uint64_t *rd_sb_stamp_buffer();   // the streaming blocks' eight stamps, RD_SB_STAMPS=1 (rd_stream_kernels.hip)
#else
#define RD_STAMP(who, slot) do { } while (0)
#endif
// the streaming blocks' phases: stream 0's workgroup / whichever workgroup gets there (k_stream_block_cplx's last one)
#define RD_SB_STAMP(k) RD_STAMP(a.stamps && threadIdx.x == 0 && blockIdx.x == 0, a.stamps[(k)])
#define RD_SBL_STAMP(k) RD_STAMP(a.stamps && threadIdx.x == 0, a.stamps[(k)])

// A streaming block's view of its ring (sample 0 = the newest block's first sample): the first readable sample after
// seen_before blocks since reset - none in front of the first block, the previous block in front of the second, from
// then on the 16 samples of the header as well
// (a macro, as RD_RSSI_OF_SUMS_F64 below is: through a function the two one-launch kernels come out of the compiler with
// other registers and another instruction order)
#define RD_SB_VALID_FROM(seen_before, B) ((seen_before) <= 0 ? 0 : (seen_before) == 1 ? -(long)(B) : -(long)((B) + 16))

// ---- bit fetches ----
__device__ __forceinline__ uint32_t rd_word_at(const uint32_t *w, long nwords, long i) {
    return (i >= 0 && i < nwords) ? w[i] : 0u;
}

// 32 bits starting at bit offset o (may be negative / past the end: zeros there)
__device__ __forceinline__ uint32_t rd_bits32_at(const uint32_t *w, long nwords, long o) {
    const long wi = o >> 5;  // floor
    const uint32_t sh = (uint32_t)(o & 31);
    const uint32_t lo = rd_word_at(w, nwords, wi);
    const uint32_t hi = rd_word_at(w, nwords, wi + 1);
    return __builtin_amdgcn_alignbit(hi, lo, sh);
}

// 32-bit variant (bit offsets inside one stream's array always fit)
__device__ __forceinline__ uint32_t rd_bits32_at_i(const uint32_t *w, int nwords, int o) {
    const int wi = o >> 5;  // arithmetic shift: floor
    const uint32_t lo = (wi >= 0 && wi < nwords) ? w[wi] : 0u;
    const uint32_t hi = (wi + 1 >= 0 && wi + 1 < nwords) ? w[wi + 1] : 0u;
    return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)(o & 31));
}

// the same from a window in LDS (the streaming kernels): bits o .. o+31, zeros outside
__device__ __forceinline__ uint32_t rd_lds_bits32(const uint32_t *w, int nwords, int o) {
    if (o < 0) return o <= -32 ? 0u : (w[0] << (-o));
    const int wi = o >> 5;
    const uint32_t lo = wi < nwords ? w[wi] : 0u, hi = wi + 1 < nwords ? w[wi + 1] : 0u;
    return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)(o & 31));
}

// Preamble search over a streaming window in LDS (py:171-188), one 32-position word per thread; positions 0 .. B
// (q <= B: py:194).  The matches go to s_match, counted by *s_nm (at most B + 1 of them).
template <int S_, int P_, uint64_t PRE_>
__device__ __forceinline__ void rd_window_search(const uint32_t *s_win, int nwin, int nbw, int tid, int nthreads,
                                                 uint32_t *s_nm, int32_t *s_match) {
    for (int o = tid; o <= nbw; o += nthreads) {
        uint32_t m = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < P_; k++) {
            const uint32_t v = rd_lds_bits32(s_win, nwin, 32 * o + k * S_);
            m &= ((PRE_ >> k) & 1) ? v : ~v;
        }
        if (o == nbw) m &= 1u;  // position B only
        while (m) {
            const int bpos = __builtin_ctz(m);
            m &= m - 1;
            const uint32_t slot = atomicAdd(s_nm, 1u);
            s_match[slot] = 32 * o + bpos;
        }
    }
}

#ifndef RD_SEARCH_OUT
#define RD_SEARCH_OUT 4     // output words (32 positions each) per lane (a multiple of 4: 16-byte loads)
#endif

__device__ __forceinline__ double rd_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;  // valid in lane 0
}

__device__ __forceinline__ uint32_t rd_wave_incl_scan_u32(uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    return v;
}

// The parse of ONE packet by ONE wave, inside the streaming kernels: `byte` is the packet as the slice holds it (lane k
// = on-air byte k, k < cfg.nbytes), `pos` its window index q, `v` a view whose sample 0 is the newest block's first
// sample (rd_stream_view, rd_cplx_view or the coherent view of k_stream_block_cplx): discriminated[j] = d[j - B],
// j in [0, 2 B) (dsp.py:156,162 - the mapping of rd_copy_discriminated_stream), the window clamped at 2 B as k_freq_err
// does, history before the stream's first block the zero state (the view's valid_from).  The CRC is computed by every
// lane from the same bytes (readlane), so the decision is wave-uniform and the float64 loop over the preamble window
// runs for the survivors only, lane-strided and summed like k_freq_err's: the same bits as the batch path.
// Returns RD_FE_NONE or the frequency error; valid in lane 0.
template <class View>
__device__ __forceinline__ int32_t rd_wave_parse(const View &v, const rd_devcfg &cfg, long pos, uint32_t byte, int lane) {
    const int sw = (int)rd_swap_bits8(byte);
    uint32_t crc = 0;
    for (int k = 2; k < cfg.nbytes; k++) crc = rd_crc16_step(crc, (uint32_t)__builtin_amdgcn_readlane(sw, k));
    if (cfg.nbytes <= 2 || crc != 0) return RD_FE_NONE;
    const long j0 = pos;
    long j1 = j0 + cfg.PL;
    if (j1 > 2L * cfg.B) j1 = 2L * cfg.B;
    double sum = 0.0;
    for (long j = j0 + lane; j < j1; j += 64) {
        const long t = j - cfg.B;
        sum += rd_disc_f64(rd_f_f64(v, t - 1), rd_f_f64(v, t));
    }
    sum = rd_wave_sum(sum);
    return rd_freq_err_hz(sum, j1 - j0, cfg.fs);
}

// py:216-236 in float64: the window sums of |f|^2 over [ns, q) and [q, pe) -> rssi, snr
#define RD_RSSI_OF_SUMS_F64(noise, sig, ns, pe, q, rssi, snr) do {                                            \
        const double noise_power = ((q) > (ns)) ? (noise) / (double)((q) - (ns)) : 1e-9;                       \
        const double signal_power = ((pe) > (q)) ? (sig) / (double)((pe) - (q)) : __builtin_nan("");           \
        (rssi) = signal_power > 0 ? 10.0 * log10(signal_power) : -120.0;                                       \
        (snr) = noise_power > 0 ? 10.0 * log10(signal_power / noise_power) : 50.0;                             \
    } while (0)

// filtered[j] = f[origin + j - 1], j in [0, B] (py:133,161: newest block only); origin is
// call*B in batch mode and 0 (the newest block's first sample) in streaming mode.
// rssi / snr of the packet at window index q: valid in lane 0.
template <class View>
__device__ __forceinline__ void rd_rssi_f64(const View &v, long origin, const rd_devcfg &cfg, long q, int lane,
                                            double &rssi, double &snr) {
    const long ns = q - cfg.PL < 0 ? 0 : q - cfg.PL;
    const long pe = q + cfg.PL > cfg.B + 1 ? cfg.B + 1 : q + cfg.PL;
    double noise = 0.0, sig = 0.0;
    for (long j = ns + lane; j < pe; j += 64) {
        const rd_d2 f = rd_f_f64(v, origin + j - 1);
        const double p = f.x * f.x + f.y * f.y;
        if (j < q) noise += p; else sig += p;
    }
    noise = rd_wave_sum(noise);
    sig = rd_wave_sum(sig);
    if (lane == 0) RD_RSSI_OF_SUMS_F64(noise, sig, ns, pe, q, rssi, snr);
}

// uint8 input: the window means are evaluated in fp32; the tolerance on RSSI/SNR is 1e-3 dB.  Measured against
// the float64 oracle (profiles/rssi_windows.txt): at most 1e-5 dB on noise, random and clipped bytes, and 2.7e-5 dB on a
// window of constant bytes 127, where |f|^2 = -81.4 dB is what remains of 2 c0 - 2 c2 + c4 after cancellation and the
// float32 taps' own rounding shows.  Each lane takes a contiguous slice of the window so the
// nine-sample FIR history slides through registers (15 conversions for 7 outputs).
// One pass of the RSSI window for a wave: lane handles PER outputs from window index j0.
// PH0 = phase (index mod 4) of the first sample it reads - wave-uniform because every lane's
// start differs by 8 samples - so the Fs/4 rotation and the dword/half selection are static.
template <int PH0, int PER>
__device__ __forceinline__ void rd_rssi_pass(const rd_stream_view &v, int n0, int j0, int q, int pe,
                                             float &noise, float &sig) {
    // (32-bit indices: samples of one stream; 64-bit index arithmetic doubled this kernel's instructions)
    const int vfrom = (int)v.valid_from, vn = (int)v.n;
    const float c[9] = RD_TAPS9;
    constexpr int ODD = PH0 & 1;
    constexpr int ND = (PER + 8 + ODD + 1) / 2;  // aligned dwords (two samples each) covering PER+8 samples
    const int ne = n0 - ODD;
    const uint32_t *src = (const uint32_t *)(v.base + 2 * (long)ne);
    uint32_t dw[ND];
#pragma unroll
    for (int d = 0; d < ND; d++) {
        const int n = ne + 2 * d;
        dw[d] = (n + 1 >= vfrom && n < vn + 8) ? src[d] : 0u;
    }
    float yr[PER + 8], yi[PER + 8];
#pragma unroll
    for (int k = 0; k < PER + 8; k++) {
        constexpr int dummy = 0; (void)dummy;
        const int i = k + ODD;
        const uint32_t h = dw[i >> 1] >> (16 * (i & 1));
        float a = ((float)(h & 0xFF) - 127.4f) * (1.0f / 127.6f);
        float b = ((float)((h >> 8) & 0xFF) - 127.4f) * (1.0f / 127.6f);
        if (n0 + k < vfrom) { a = 0.0f; b = 0.0f; }
        const int ph = (PH0 + k) & 3;  // static
        yr[k] = ph == 0 ? a : ph == 1 ? -b : ph == 2 ? -a : b;
        yi[k] = ph == 0 ? b : ph == 1 ? a : ph == 2 ? -b : -a;
    }
#pragma unroll
    for (int r = 0; r < PER; r++) {
        float fr = 0.0f, fi = 0.0f;
#pragma unroll
        for (int m = 0; m < 9; m++) {  // f[t] = sum_m c_m y[t-9+m]; y[t-9+m] is window index r+m
            fr = __builtin_fmaf(c[m], yr[r + m], fr);
            fi = __builtin_fmaf(c[m], yi[r + m], fi);
        }
        const float pw = fr * fr + fi * fi;
        const int j = j0 + r;
        if (j < pe) { if (j < q) noise += pw; else sig += pw; }
    }
}

// The RSSI windows on the matrix pipe: the 448 filter outputs of a packet's two windows are ONE 16-output block of
// 32 columns in rd_mfma.h's formulation (six MFMAs, exact; rd_demod_mfma.hip: rd_mf_block) instead of 144 fp32
// fma per lane.  Column n covers outputs A + 16 n + 1 .. A + 16 n + 16, lane (n, h) its half h; A is the
// window's first output rounded down to a multiple of four samples (8-byte aligned loads).  Applies when every
// sample the 32 columns touch is a real byte of the stream; otherwise the caller's fp32 path runs.  The arithmetic is
// exact for the QUANTISED taps, which costs 2.3e-4 dB on a window of constant bytes 127 (the quantised DC response
// differs from 2 c0 - 2 c2 + c4 by that much; a quarter of the 1e-3 dB tolerance, the worst legal input) and at most
// 6e-6 dB on anything else (profiles/rssi_windows.txt).  In the batch path only the condition on the stream's end can
// fail (Davis: the last call from q = B - 282 on): tests/rssi_window_cases.py.
typedef _Float16 rd_k_h8 __attribute__((ext_vector_type(8)));
typedef float rd_k_f16v __attribute__((ext_vector_type(16)));
// (static: k_rssi_u8 and k_tail live in different files and the library has no relocatable device code - 6 KiB in each)
static __device__ const rd_mf_taps g_rssi_taps = rd_mf_make_taps();

__device__ __forceinline__ rd_k_h8 rd_k_frag(uint2 d) {  // as rd_mf_frag: a byte read as an f16 pattern is k * 2^-24
    uint4 v;
    v.x = d.x & 0x00FF00FFu;
    v.y = __builtin_amdgcn_perm(0u, d.x, 0x0c030c01u);
    v.z = d.y & 0x00FF00FFu;
    v.w = __builtin_amdgcn_perm(0u, d.y, 0x0c030c01u);
    return __builtin_bit_cast(rd_k_h8, v);
}

// One RSSI job prepared for the matrix pipe: ok = every sample the 32 columns touch is a real byte of the stream
// (wave-uniform); p = this lane's first 8 window bytes.
struct rd_rssi_job {
    bool ok;
    int A, ns, pe, q, origin;
    const uint8_t *p;
};
__device__ __forceinline__ rd_rssi_job rd_rssi_prepare(const rd_stream_view &v, int origin, const rd_devcfg &cfg, int q, int lane) {
    rd_rssi_job j;
    j.origin = origin; j.q = q;
    j.ns = q - cfg.PL < 0 ? 0 : q - cfg.PL;
    j.pe = q + cfg.PL > cfg.B + 1 ? cfg.B + 1 : q + cfg.PL;
    const int t_lo = origin + j.ns - 1, t_hi = origin + j.pe - 2;  // filter outputs f[t] of the window
    j.A = (t_lo - 1) & ~3;
    j.ok = t_lo >= 1 && j.A - 8 >= (int)v.valid_from && j.A + 16 * 31 + 24 <= (int)v.n + 8 && t_hi <= j.A + 512;
    j.p = v.base + 2 * (long)(j.A - 8) + 32 * (lane & 31) + 8 * (lane >> 5);
    return j;
}
struct rd_rssi_data {
    uint2 d0, d1, d2;
};
__device__ __forceinline__ rd_rssi_data rd_rssi_fetch(const rd_rssi_job &j) {
    rd_rssi_data d;
    d.d0 = *(const uint2 *)j.p; d.d1 = *(const uint2 *)(j.p + 16); d.d2 = *(const uint2 *)(j.p + 32);
    return d;
}
// window sums of |f|^2 (noise: window index < q, signal: the rest) from the fetched bytes
__device__ __forceinline__ void rd_rssi_block(const rd_rssi_job &j, const rd_rssi_data &d, const rd_k_h8 (&Ahi)[3],
                                              const rd_k_h8 (&Alo)[3], int lane, float &noise, float &sig) {
    const int n = lane & 31, h = lane >> 5;
    const float dcv = -(float)RD_MF_DHI / 16777216.0f;
    const rd_k_f16v dc = {dcv, dcv, dcv, dcv, dcv, dcv, dcv, dcv, dcv, dcv, dcv, dcv, dcv, dcv, dcv, dcv};
    const rd_k_f16v zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const rd_k_h8 b0 = rd_k_frag(d.d0), b1 = rd_k_frag(d.d1), b2 = rd_k_frag(d.d2);
    rd_k_f16v ah = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ahi[0], b0, dc, 0, 0, 0);
    rd_k_f16v al = __builtin_amdgcn_mfma_f32_32x32x16_f16(Alo[0], b0, zero, 0, 0, 0);
    ah = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ahi[1], b1, ah, 0, 0, 0);
    al = __builtin_amdgcn_mfma_f32_32x32x16_f16(Alo[1], b1, al, 0, 0, 0);
    ah = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ahi[2], b2, ah, 0, 0, 0);
    al = __builtin_amdgcn_mfma_f32_32x32x16_f16(Alo[2], b2, al, 0, 0, 0);
    // |f|^2 = |g|^2 / (127.6 * 2^-24 S)^2: g is the filter output in rd_mfma.h's units, the rotation has modulus 1
    const float inv = (float)(1.0 / (127.6 * RD_MF_G_PER_BYTE * 127.6 * RD_MF_G_PER_BYTE));
    float sn = 0.0f, ss = 0.0f;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const float gr = __builtin_fmaf(ah[2 * r], 2048.0f, al[2 * r]), gi = __builtin_fmaf(ah[2 * r + 1], 2048.0f, al[2 * r + 1]);
        const float pw = __builtin_fmaf(gr, gr, gi * gi);
        const int jj = j.A + 16 * n + 8 * h + 1 + r - j.origin + 1;  // window index of output t
        if (jj >= j.ns && jj < j.pe) { if (jj < j.q) sn += pw; else ss += pw; }
    }
    noise = sn * inv;
    sig = ss * inv;
}

// Sum over the wave without the LDS crossbar: four rotations inside the rows of 16 lanes (DPP), then the four row
// sums through scalar registers - a dozen short-latency instructions instead of six dependent ds_bpermute.
__device__ __forceinline__ float rd_wave_sum_dpp(float v) {
#define RD_ROR(x, n) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (x)), 0x120 + (n), 0xF, 0xF, false))
    v += RD_ROR(v, 1);
    v += RD_ROR(v, 2);
    v += RD_ROR(v, 4);
    v += RD_ROR(v, 8);
#undef RD_ROR
    const int vi = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 0)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 16)) +
           __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 32)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 48));
}

// per-lane partial sums -> py:207-236's two figures (valid in lane 0)
__device__ __forceinline__ void rd_rssi_finish(float noise, float sig, int ns, int pe, int q, int lane, double &rssi, double &snr) {
    noise = rd_wave_sum_dpp(noise);
    sig = rd_wave_sum_dpp(sig);
    if (lane == 0) {
        const float noise_power = (q > ns) ? noise / (float)(q - ns) : 1e-9f;
        const float signal_power = (pe > q) ? sig / (float)(pe - q) : __builtin_nanf("");
        // 10*log10(x) = 3.0102999566 * log2(x)
        rssi = signal_power > 0 ? (double)(3.0102999566f * __builtin_amdgcn_logf(signal_power)) : -120.0;
        snr = noise_power > 0 ? (double)(3.0102999566f * __builtin_amdgcn_logf(signal_power / noise_power)) : 50.0;
    }
}

// uint8 input: the window means are evaluated in fp32 and 10*log10 goes through v_log_f32; the tolerance on
// RSSI/SNR is 1e-3 dB.  Measured: 1e-5 dB at the most where the window holds a signal of any kind (the wave sum and
// v_log_f32 together; the NumPy model without them is within 1e-6 dB), 2.7e-5 dB on constant bytes 127 (rd_rssi_pass).
__device__ __forceinline__ void rd_rssi_u8(const rd_stream_view &v, long origin64, const rd_devcfg &cfg, long q64,
                                           int lane, double &rssi, double &snr) {
    const int origin = (int)origin64, q = (int)q64;
    const int ns = q - cfg.PL < 0 ? 0 : q - cfg.PL;
    const int pe = q + cfg.PL > cfg.B + 1 ? cfg.B + 1 : q + cfg.PL;
    constexpr int PER = 8;  // outputs per lane per pass: 64 * 8 = 512 window positions per pass
    float noise = 0.0f, sig = 0.0f;
    for (int jb = ns; jb < pe; jb += 64 * PER) {
        const int j0 = jb + PER * lane;
        // outputs j0 .. j0+PER-1 are f[t], t = origin + j - 1, each using y[t-9 .. t-1]:
        // samples n0 .. n0 + PER + 7 with n0 = origin + j0 - 10
        const int n0 = origin + j0 - 10;
        const int ph0 = __builtin_amdgcn_readfirstlane(n0 & 3);
        if (j0 < pe) {
            switch (ph0) {
                case 0: rd_rssi_pass<0, PER>(v, n0, j0, q, pe, noise, sig); break;
                case 1: rd_rssi_pass<1, PER>(v, n0, j0, q, pe, noise, sig); break;
                case 2: rd_rssi_pass<2, PER>(v, n0, j0, q, pe, noise, sig); break;
                default: rd_rssi_pass<3, PER>(v, n0, j0, q, pe, noise, sig); break;
            }
        }
    }
    rd_rssi_finish(noise, sig, ns, pe, q, lane, rssi, snr);
}

// Lanes 0..31 hold data[lane] in `byte`, lane 0 holds rssi / snr.  Destinations: `dev` (device
// memory) and/or `host` (pinned host memory mapped into the device, used by the streaming handle:
// a block's few records need no copy afterwards).  Plain byte + header stores: assembling the 64
// bytes across 16 lanes for one coalesced store (four ds_bpermute + readfirstlanes) was measured
// 7 us slower per launch.
__device__ __forceinline__ void rd_store_record(rd_packet *dev, rd_packet *host, int lane, int stream, long call, long q,
                                                int nbytes, uint32_t byte, double rssi, double snr) {
#pragma unroll
    for (int dst = 0; dst < 2; dst++) {
        rd_packet *o = dst ? host : dev;
        if (!o) continue;
        if (lane < RD_MAX_PKT_BYTES) o->data[lane] = lane < nbytes ? (uint8_t)byte : (uint8_t)0;
        if (lane == 0) {
            o->stream = stream; o->call = (int32_t)call; o->index = (int32_t)q; o->nbytes = nbytes;
            o->rssi = rssi; o->snr = snr;
        }
    }
}

// a match that no call reports, or that the per-call dedupe is certain to drop: stream = -1
__device__ __forceinline__ void rd_store_void(rd_packet *dev, rd_packet *host, int lane) {
    if (lane == 0) {
        if (dev) dev->stream = -1;
        if (host) host->stream = -1;
    }
}

// a workgroup barrier that orders LDS traffic only: __syncthreads() also waits for every global store in flight
// (s_waitcnt vmcnt(0)) - here the stores that publish a group's totals, whose acknowledgement nobody in the
// workgroup needs
__device__ __forceinline__ void rd_barrier_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

static inline uint32_t rd_slice_grid(uint32_t match_cap) {
    uint32_t wgs = (match_cap + 3) / 4;
    if (wgs > 4096) wgs = 4096;
    return wgs ? wgs : 1;
}

// ---- the slice of one match by one wave ----
// (Macros both: as functions - plain, or templates on the position's type and the fetch - they change the register
// allocation of k_classify, k_slice_rssi and the one-launch streaming kernels.)
// RD_WAVE_BYTES: symbols 64 r + lane of the packet at `pos`; byte bi = symbols 8 bi .. 8 bi + 7, first symbol = MSB; a
// last partial byte is right-aligned (the bits are shifted in one by one, py:197-200).  BITS3(o) = the bits from bit
// offset o on, of which three are used: the same fetch yields the symbols of the packets one position earlier and later.
// Lane k < 8 gets byte k into `byte`; same_prev / same_next (true before): cleared unless that neighbour carries the same
// bits (an oversampled burst matches at 2-4 adjacent positions).
#define RD_WAVE_BYTES(K, S, pos, lane, BITS3, byte, same_prev, same_next) do {                                              \
        for (int r = 0; r * 64 < (K); r++) {                                                                                \
            const int k = 64 * r + (lane);                                                                                  \
            const uint32_t tri = k < (K) ? BITS3((pos) - 1 + k * (S)) : 0u;                                                  \
            const uint64_t mp = __ballot((tri & 1u) != 0), mm = __ballot((tri & 2u) != 0), mn = __ballot((tri & 4u) != 0);  \
            (same_prev) &= mp == mm;                                                                                        \
            (same_next) &= mn == mm;                                                                                        \
            const int bi = (lane) - 8 * r;                                                                                  \
            if (bi >= 0 && bi < 8) {                                                                                        \
                const int have = (K) - 8 * (lane);  /* symbols in this byte */                                              \
                const uint32_t rev = __builtin_bitreverse32((uint32_t)((mm >> (8 * bi)) & 0xFF)) >> 24;                     \
                (byte) = have >= 8 ? rev : have > 0 ? rev >> (8 - have) : 0u;                                               \
            }                                                                                                               \
        }                                                                                                                   \
    } while (0)
// RD_SUPERSEDED: a neighbour position with the same bits comes first, so the record at window index q is certain to be
// dropped by the per-call dedupe (py:203-205) and is skipped before its RSSI windows are read.  The reference's order
// inside a call is by (q % S, q) (py:171-188, phase-major search): q-1 precedes q unless its phase is larger (it wraps to
// S-1 when q % S == 0, S > 1); q+1 precedes q only when its phase is smaller (it wraps to 0 when q % S == S-1, S > 1).
#define RD_SUPERSEDED(sym_len, q, B, same_prev, same_next) ({                                               \
        const uint32_t S = (uint32_t)(sym_len), ph = (uint32_t)(q) % S;                                     \
        const bool prev_first = S == 1 || ph != 0;                                                          \
        const bool next_first = S > 1 && ph == S - 1;                                                       \
        ((same_prev) && (q) >= 1 && prev_first) || ((same_next) && (q) + 1 <= (B) && next_first);           \
    })

#ifndef RD_SLICE_MIN_WGS
#define RD_SLICE_MIN_WGS 1  // (8 = 64 VGPRs was tried: 14 spills, 73 us instead of 58)
#endif
// where the RSSI windows read their samples from: the uint8 streams or the complex128 ring
struct rd_u8_src {
    rd_layout lay;
    __device__ __forceinline__ void rssi(int stream, long origin, const rd_devcfg &cfg, long q, int lane, double &r,
                                         double &s) const {
        rd_rssi_u8(rd_view_of(lay, stream), origin, cfg, q, lane, r, s);
    }
};
struct rd_cplx_src {
    rd_cplx_view v;
    __device__ __forceinline__ void rssi(int, long origin, const rd_devcfg &cfg, long q, int lane, double &r,
                                         double &s) const {
        rd_rssi_f64(v, origin, cfg, q, lane, r, s);
    }
};

// ------------------------------------------------------------------------------------------
// k_slice_rssi: one WAVE per match.  Decides which call(s) report it (py:194), packs
// packet_symbols bits at stride S (py:197-200: lane k reads symbol k, a ballot packs them) and
// evaluates the reference's RSSI/SNR windows (py:207-236) with all 64 lanes.
// Record i belongs to match i.  A position on a block boundary is reported by two calls (q = B in
// call b, q = 0 in call b+1): its second record is appended at recs[match_cap + k], k counted by
// RD_CNT_REC.  A match that no call reports leaves stream = -1.  Per-call duplicates (py:203-205)
// are dropped by the host when it puts the records in the reference's order.
// ------------------------------------------------------------------------------------------
template <class Src>
__global__ __launch_bounds__(256, RD_SLICE_MIN_WGS) void k_slice_rssi(Src src, const uint32_t *bits, size_t bits_stride, long nwords,
                                                    rd_devcfg cfg, const rd_match *matches, uint32_t match_cap,
                                                    int batch_mode, int n_calls, int call, rd_packet *recs,
                                                    rd_packet *recs_host, uint32_t *counters) {
    const int lane = threadIdx.x & 63;
    uint32_t count = counters[RD_CNT_MATCH];
    if (count > match_cap) count = match_cap;
    const uint32_t nw = gridDim.x * (blockDim.x >> 6);
    for (uint32_t i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < count; i += nw) {
        const int stream = __builtin_amdgcn_readfirstlane(matches[i].stream);
        const long pos = __builtin_amdgcn_readfirstlane(matches[i].pos);
        // Which call(s) report this position (py:194, q <= B): in batch mode call b sees absolute
        // positions w_b <= p <= w_b + B with w_b = (b+1)B - L, so p is reported by one call, or by
        // two when it falls on a block boundary (q = B in call b, q = 0 in call b+1).
        long b0 = call, b1 = -1, q0 = pos, q1 = 0;
        bool ok0 = true, ok1 = false;
        if (batch_mode) {
            // p + L >= B because p >= B - L, and < 2^32 (n_samples < 2^31): 32-bit division
            const uint32_t pl = (uint32_t)(pos + cfg.L), bq = pl / (uint32_t)cfg.B, br = pl - bq * (uint32_t)cfg.B;
            b0 = (long)bq - 1;
            q0 = pos - ((b0 + 1) * (long)cfg.B - cfg.L);
            ok0 = b0 >= 0 && b0 < n_calls;
            b1 = b0 - 1;
            q1 = q0 + cfg.B;
            ok1 = br == 0 && b1 >= 0 && b1 < n_calls;
        }
        const uint32_t *w = bits + (size_t)stream * bits_stride;
        uint32_t byte = 0;
        bool same_prev = true, same_next = true;
#define RD_BITS3(o) rd_bits32_at_i(w, (int)nwords, (o))
        RD_WAVE_BYTES(cfg.K, cfg.S, (int)pos, lane, RD_BITS3, byte, same_prev, same_next);
#undef RD_BITS3
        auto superseded = [&](long q) { return RD_SUPERSEDED(cfg.S, q, cfg.B, same_prev, same_next); };
        rd_packet *o = recs ? &recs[i] : nullptr, *oh = recs_host ? &recs_host[i] : nullptr;
        const bool use0 = ok0 && !superseded(q0), use1 = ok1 && !superseded(q1);
        if (!(use0 || use1)) {
            rd_store_void(o, oh, lane);
            continue;
        }
        const long pb = use0 ? b0 : b1, pq = use0 ? q0 : q1;
        double rssi = 0.0, snr = 0.0;
        src.rssi(stream, batch_mode ? pb * cfg.B : 0, cfg, pq, lane, rssi, snr);
        rd_store_record(o, oh, lane, stream, pb, pq, cfg.nbytes, byte, rssi, snr);
        if (use0 && use1) {
            uint32_t slot = 0;
            if (lane == 0) slot = atomicAdd(&counters[RD_CNT_REC], 1u);
            slot = __builtin_amdgcn_readfirstlane(slot);  // < match_cap: at most one per match
            src.rssi(stream, b1 * cfg.B, cfg, q1, lane, rssi, snr);
            const size_t xi = (size_t)match_cap + slot;
            rd_store_record(recs ? &recs[xi] : nullptr, recs_host ? &recs_host[xi] : nullptr, lane, stream, b1, q1,
                            cfg.nbytes, byte, rssi, snr);
        }
    }
}
