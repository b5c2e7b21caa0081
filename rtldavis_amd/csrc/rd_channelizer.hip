// rd_channelizer.hip - wideband front end: one IQ capture (uint8, int8, int16 or float32) at
// decim x 268.8 kSPS -> one 268.8 kSPS uint8 IQ stream per hop channel, written straight into a
// batch demodulator's resident input buffer.
//
// rtldavis has no channelizer (it retunes one narrow-band dongle per hop, runners/rtlsdr.py:51,72),
// so there is no reference implementation and parity is UNPINNED: the definition below is this
// repo's own, restated in float64 by oracle/channelizer_oracle.py, and the tests tie it to the
// reference through the packets the reference demodulator recovers from its output.
//
//   x[n]   = lut(I[n]) + j lut(Q[n]),  lut(k) = (k - 127.4) / 127.6        (RD_IQ_U8: uint8, dsp.py:20-39)
//                                       lut(k) = k / 128                    (RD_IQ_S8: int8)
//                                       lut(k) = k / 32768                  (RD_IQ_S16: int16, host byte order)
//                                       lut(v) = adm(v)                     (RD_IQ_CF32: float32, host byte order; below)
//   z_c[t] = sum_{k<T} h[k] x[D t - k] e^{-j 2 pi shift_c (D t - k) / Fw}    (x[n<0] = 0)
//          = e^{-j 2 pi frac(shift_c t / Fo)} sum_k g_c[k] x[D t - k],   g_c[k] = h[k] e^{+j 2 pi shift_c k / Fw}
//   out_c[t] = clip(rint(gain z 127.6 + 127.4), 0, 255) per component       (the synth's quantiser)
// with Fw the wideband rate, D the decimation, Fo = Fw / D; shift_c an integer number of Hz, so the
// output phasor's phase is an exact integer remainder.
// Contract against the model's Z = gain z 127.6 + 127.4 (oracle/channelizer_oracle.py:channelize_z): a byte is never
// more than one step from clip(rint(Z), 0, 255) and equals it wherever Z is more than delta from every rounding
// boundary k + 1/2.  delta (tests/chan_bound.py:error_bound) bounds every rounding below - fp32 taps, the f16 split,
// the fp32 accumulation from this capture's partial sums, the DC table, the phasor (v_sin/v_cos assumed within 2^-16),
// the final scale - and is 0.002-0.05 steps at 8..512 taps, ~0.2 at 8192.  Measured on the test sweep (decim 4..644,
// 8..8192 taps, 2..4096 channels): every byte that differs lies within 1/50 of delta of a boundary.
//
// Kernel: f16 MFMA (v_mfma_f32_32x32x16_f16) - the one dense contraction in this repo.  As a real
// GEMM, C[m][n] = sum_kappa A[m][kappa] B[kappa][n] with
//   m     = 2 c + part  (part 0 = re, 1 = im of channel c; rows 2c, 2c+1 land in one lane's registers)
//   kappa = 2 i + comp  (comp 0 = I, 1 = Q of window sample i, ascending in memory; inside a lane's four samples the
//           fragment's elements are ordered I0 I1 Q0 Q1 | I2 I3 Q2 Q3, which is what one v_and + one v_perm per dword give)
//   A[2c][2i] = g_r, A[2c][2i+1] = -g_i, A[2c+1][2i] = g_i, A[2c+1][2i+1] = g_r    (g = g_c[T-i], zero outside 0..T-1)
//   B[2i + comp][n] = b_comp[D (t0 + n) - T + i] 2^-24
// The samples are bytes: read as an f16 bit pattern, a byte in the low half of a 16-bit lane IS the subnormal
// b 2^-24 (round 3; the matrix pipe takes subnormal inputs at face value and at full rate,
// profiles/r02_ubench_mfma_subnormal.txt), and lut(b) = (b - 127.4) / 127.6, so
// z = (sum - 127.4 (1 + j) sum_k g_c[k]) / 127.6 with the second term a per-channel constant (a short
// table for the first outputs of a capture, whose history is zero).  The taps, scaled by a power of two
// so that the largest sits just below 2^15, are split into TWO f16 terms (hi + lo: 22 bits; round 1 used
// three bf16 terms for 24), i.e. two MFMAs per tile and K step into the same fp32 accumulator: products
// are exact, sums are fp32, the tap error 2^-22 relative - two orders below the fp32 accumulation's.
// 8 T flops per output: 113 GFLOP for one second of 51 channels; HBM traffic is 81 MB.
// A workgroup = 4 waves = 128 output times x a group of 4 row blocks (64 channels); wave w owns row
// block w and the four 32-time blocks (4 accumulator tiles).  The 127 D + T + 8 input samples are staged
// once in LDS as they are, two bytes each - 26 KiB (round 2: f16 pairs, 52 KiB and three workgroups per CU) - so a B
// fragment is one aligned ds_read_b64 (D = 100: lane stride 50 dwords, conflict-free) and four v_perm.  A wave only
// needs its own row block's A fragments (2 terms x 16 bytes per lane and K step): they come straight from L2
// into registers two K steps ahead; the main loop has no barrier.
// Measured (one second of capture, 27 M samples -> 51 x 270 k): 0.25 ms = 4000x real time.
// On the way: fp32 VALU kernel 0.88 ms (64 TFLOP/s, bound by the CU's LDS pipe: every fma needed
// 2.5 bytes from LDS), fp32 MFMA 0.84 ms, bf16 MFMA with the B bytes converted per fragment in
// each wave 0.55 ms (one wave per SIMD cannot hide ~25 VALU instructions per three MFMAs), A
// through a shared LDS chunk two steps ahead instead of one 0.55 -> 0.46, samples pre-converted in
// LDS 0.36, 128 instead of 256 output times per workgroup 0.27, A per wave from L2 without LDS or
// barriers 0.25 (three bf16 tap terms); two f16 tap terms: see DESIGN.
//
// The signed formats (template parameter FMT).  RD_IQ_S8: bit 7 of every byte is flipped while the window is staged (one
// v_xor per dword of the 16-byte vectors), which makes it offset-binary uint8; the loop is the uint8 one, the DC term
// -128 (1 + j) sum g, the scale 1/128.  A sample outside the capture is staged as 0x80, the value 0, so the table of early
// DC terms holds the steady one throughout.  Measured equal to uint8 (0.151 ms both, profiles/channelizer_formats.txt).
// RD_IQ_S16 stays an f16 MFMA GEMM on exact operands: an int16 is no f16, so a component s = sg (256 mh + ml) enters as
// two SIGN-MAGNITUDE digits, the f16 patterns sg | ml and sg | mh - the subnormals -+ m 2^-24, so the raw-pattern trick
// survives - and K doubles: kappa = 4 i + 2 comp + digit, four window samples per K = 16 step.  The conversion happens
// once per staged sample (abs, and, shift, or); LDS holds the four 16-bit lanes Ilo Ihi Qlo Qhi of a sample, 8 bytes, in
// fragment order, so a B fragment is one aligned ds_read_b128 and no VALU work at all.  The low digit's taps are scaled
// 2^-8 against the high digit's (a second power-of-two scale; 256 x the taps would overflow f16), both in two f16 terms.
// There is no DC term: zero history is the digit 0.  -32768 is mh = 128, ml = 0.
// Why signed digits: with offset binary (s + 32768 = 256 (hi ^ 0x80) + lo, both bytes subnormals as for uint8) the fp32
// accumulator carries 32768 sum g while a real signal is a few hundred counts, and the accumulation term of the bound
// scales with full scale: on the weak default-plan capture (437 counts, gain 300) it exempts a third of the bytes;
// signed digits keep every partial sum at signal size (derived bound there: median 2e-4, max 7e-3 LSB, 0.13 % exempt,
// tests/chan_bound_fmt.py).  Rejected: offset binary (above); two's-complement bytes (hi signed, lo unsigned: the low
// digit alone swings by 255 per sample, and a signed byte needs a conversion per fragment); balanced signed bytes
// converted per fragment (32767 = 256 x 128 - 1 does not fit a signed hi byte, and the per-fragment VALU work is what
// round 3 removed from the uint8 loop); sign-magnitude kept as 4 bytes with the lanes rebuilt per fragment (three VALU
// ops per dword, and -32768 has no 16-bit sign-magnitude form).  The price of 8 bytes per sample: the default plan's
// window is 106 KiB, one workgroup per CU, and decim <= 160.  Lane stride 2 D dwords (D = 100: 200 = 8 mod 64): the
// b128 reads are 2-way bank conflicted by the bank rule (not measured).  Measured: 0.40 ms per second of capture,
// 2.66 x uint8 - twice the MFMAs on twice the bytes, the rest at one wave per SIMD; 2480 x real time.  Not tried: a
// 64-output tile (two workgroups per CU, but twice the A traffic from L2).
//
// RD_IQ_CF32: interleaved float32 I, Q in host byte order, 8 bytes per IQ pair, nominal full scale +-1.0.  The admitted
// value of a component v is adm(v) = 0 if v is NaN, otherwise v clamped to [-8, +8] (so +-Inf is +-8), and
// x[n] = adm(I[n]) + j adm(Q[n]); everything behind x is the definition above.  No DC term; a sample outside the capture
// is exactly 0.  (Why 8: 18 dB over nominal keeps every digit far inside f16 and every fp32 partial sum far from
// overflow; one NaN would otherwise poison every channel's window.)  The kernel is the int16 one with other digits: a
// component enters as s = 2^12 adm(v) - an exact power-of-two pre-scale, |s| <= 2^15, undone in tap_unscale - split as
// hi = f16(s), lo = f16(s - hi), both round-to-nearest-even conversions, s - hi exact in fp32.  |s - hi - lo| <=
// max(2^-22 |s|, 2^-25); the pre-scale moves the f16 subnormal floor 2^-25 to 2^-37 in x's units, below the last bit
// of any float32 that matters (without it a capture at 1 % of full scale would lose its low digit to the floor).  The
// conversion must PRODUCE f16 subnormals (lo is one whenever |s| < 2^-3): the kernel relies on the default float
// mode, f16 denormals enabled (FP_DENORM of f16/f64 = 3), the same mode under which the matrix pipe takes them.  The
// staged sample is the four 16-bit lanes Ilo Ihi Qlo Qhi in int16's fragment order - one aligned ds_read_b128 per B
// fragment, no VALU work in the loop; both digits meet the SAME tap (no 2^-8), the epilogue's scale is gains[ch].
// Products stay exact: 11 x 11 bits, the smallest non-zero one 2^-24 2^-24 = 2^-48.  Bound: tests/chan_bound_cf32.py.
// Levels: k = clip(rint(2^15 adm(v)), -32768, 32767) per component, i.e. int16 units (rd_chan_levels.hip: k_chan_levels).
//
// RETUNE (streaming form only; rd_wideband.hip: rd_wb_retune).  With a phase accumulator P_c, an integer in [0, Fo) that is
// 0 after create and reset, and t the absolute output time,
//   z_c[t] = e^{-j 2 pi frac((shift_c t + P_c) / Fo)} sum_k g_c[k] x[D t - k],   g_c[k] = h[k] e^{+j 2 pi shift_c k / Fw}
// - the definition above when P_c = 0.  A retune shift -> shift' at a chunk boundary t_b replaces shift, g and
// P -> P' = (P + (shift - shift') t_b) mod Fo, exact integer arithmetic: the phase is continuous at t_b.  Every output
// from t_b on is filtered with the NEW band-pass g', the few whose window reaches back into the previous chunk included:
// the history is not re-mixed at the old frequency (the samples are kept, not the old mixer's products).  The tables of
// the channels that change are rebuilt in place by k_chan_retune, queued between the two chunks' k_channelize.
//
// GAIN.  `gain` above is per channel: the epilogue reads gains[ch], a float32 table that holds (float)cfg.gain in every
// entry after create - with which every byte is the scalar form's, the scale being the same fp32 product.  One load per
// lane and channel beside shifts[ch] and phase[ch]; the bound of a channel is error_bound at that channel's gain.
// rd_chan_set_gain rewrites the table for the one-shot form; the streaming form's updates are rd_chan_stream_gains
// (rd_wideband.hip: rd_wb_set_gain), a copy queued between two chunks' k_channelize as the retune kernel is.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/rtldavis_hip.h"
#include "rd_chan_tables.h"
#include "rd_internal.h"

#ifndef RD_CHAN_NPF
#define RD_CHAN_NPF 2                       // A chunks in flight in registers
#endif
#ifndef RD_CHAN_MINWAVES
#define RD_CHAN_MINWAVES 4                  // waves per SIMD the register allocation aims at (26 KiB of LDS admit 6)
#endif

typedef float rd_f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 rd_f16x8 __attribute__((ext_vector_type(8)));

// The handle: the host's state (rd_chan_tables.h) and what lives on the device
struct rd_chan : rd_chan_tables {
    uint16_t *d_amat = nullptr;
    float *d_dc = nullptr;
    int64_t *d_shifts = nullptr;
    int64_t *d_phase = nullptr;
    // GAIN: the device table, and two pinned slots of [n_channels] for the streaming form's updates (rd_chan_stream_gains)
    float *d_gains = nullptr;
    float *h_gains = nullptr;
    double *d_taps = nullptr;      // streaming form only: k_chan_retune's input, uploaded once
    int64_t *h_rt = nullptr;       // pinned: two slots of [n_channels][4] retune records (channel, shift, shift mod Fo, P)
    int64_t *d_rt = nullptr;       // one slot on the device (its copies and kernels are ordered by the stream)
    uint8_t *d_wide = nullptr;     // resident capture, rd_fmt_in_bps bytes per sample
    size_t wide_cap = 0, wide_n = 0;
    rd_spec *spec = nullptr;       // rd_chan_spectrum's tables and scratch (rd_spectrum.hip), made on first use
    bool dev_ready = false;
    int device = -1;               // the device the buffers live on
};

// T is the padded tap count (multiple of RD_CHAN_KC, zero taps appended), D a multiple of 4.
// Round 3: the window is staged as the RAW bytes - a byte in the low half of a 16-bit lane IS the f16 subnormal
// k 2^-24, which the matrix pipe takes at face value and at full rate (the demod kernel's operands, rd_mfma.h) - 2
// bytes per sample in LDS instead of an f16 pair's 4 (26 KiB per workgroup instead of 52), no conversion arithmetic in
// the staging, and the 127.4 offset of the LUT as a per-channel constant (-127.4 sum of the taps an output sees).  The
// window starts one sample early, at n0 = D t0 - T, a multiple of 8 samples: 16-byte loads, 16-byte LDS writes and
// 8-byte fragment reads are all aligned; the price is one more K step (the leading tap of it is zero).
//
// STREAM (rd_wideband.hip): `wide` is one chunk of a capture that never ends, `prev` the chunk before it (null for the
// first chunk after create / reset: zero history, as the one-shot form stages for n < 0), and output time 0 of the launch
// is the absolute time t_base; the kernel gets t_base mod out_rate (reduced exactly on the host) and an n_early of 0
// unless t_base is 0.  A chunk is a whole number of workgroups (block_size % RD_CHAN_TT == 0, so n_wide and every window
// start are multiples of 8 samples): an 8-sample vector lies wholly in `prev`, in `wide` or past the chunk, where the
// taps are zero - the streamed bytes equal the one-shot form's on the whole capture.
//
// FMT (header: the formats): RD_IQ_S8 flips bit 7 of every byte while staging - the window is then offset-binary uint8
// (a sample outside the capture becomes 0x80 = the value 0, so the DC table holds the steady term throughout) and the
// main loop is the uint8 one.  RD_IQ_S16 stages a sample as four 16-bit lanes Ilo Ihi Qlo Qhi, each the f16 pattern
// sign | digit of the component's sign-magnitude form, converted once per staged sample: a B fragment is then one
// aligned ds_read_b128 (two samples) and nothing else, a K step covers 4 window samples, there is no DC term.
// The sample dword of an int16 pair -> the two LDS dwords (lo | hi << 16 of I, of Q)
__device__ __forceinline__ uint2 rd_chan_sm16(uint32_t w) {
    const int si = (int)(int16_t)(w & 0xFFFFu), sq = (int)w >> 16;
    const uint32_t mi = (uint32_t)(si < 0 ? -si : si), mq = (uint32_t)(sq < 0 ? -sq : sq);   // 0 .. 32768
    return uint2{(si < 0 ? 0x80008000u : 0u) | (mi & 0xFFu) | ((mi >> 8) << 16),
                 (sq < 0 ? 0x80008000u : 0u) | (mq & 0xFFu) | ((mq >> 8) << 16)};
}

// One float32 component -> its LDS dword lo | hi << 16: s = 2^12 adm(v), hi = f16(s), lo = f16(s - hi), both
// round-to-nearest-even with subnormal results kept (the default float mode); s - hi is exact in fp32
__device__ __forceinline__ uint32_t rd_chan_f32_digits(uint32_t bits) {
    const float s = rd_chan_adm(bits) * (float)(1 << RD_CF32_PRESCALE_LOG2);
    const _Float16 hi = (_Float16)s;
    const _Float16 lo = (_Float16)(s - (float)hi);
    return (uint32_t)__builtin_bit_cast(uint16_t, lo) | ((uint32_t)__builtin_bit_cast(uint16_t, hi) << 16);
}

template <bool STREAM, int FMT>
__global__ __launch_bounds__(256, RD_CHAN_MINWAVES) void k_channelize(const uint8_t *__restrict__ wide, long n_wide,
                                                    const uint4 *__restrict__ amat, const float2 *__restrict__ dc,
                                                    const int64_t *shifts, int T, int D, int n_ch, int n_early,
                                                    long out_rate, const float *gains, float tap_unscale, long n_out,
                                                    uint8_t *out, size_t out_stride, int xs_bytes,
                                                    const uint8_t *__restrict__ prev, long t_base_mod,
                                                    const int64_t *phase) {
    extern __shared__ uint8_t lds[];
    uint8_t *xs = lds;                            // window samples 0 .. span-1, LB bytes each
    constexpr int IB = rd_fmt_in_bps(FMT), LB = rd_fmt_lds_bps(FMT), KC = rd_fmt_kc(FMT);
    constexpr int VS = 16 / IB;                   // samples per 16-byte vector of the capture
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // = row block
    const int r = lane & 31, h = lane >> 5;
    const long t0 = (long)blockIdx.x * RD_CHAN_TT;
    const int grp = blockIdx.y;
    // stage samples n0 .. n0 + span - 1; a sample before the capture (or after it) is the byte 0 = no contribution
    const long n0 = (long)D * t0 - T;
    const int span = (RD_CHAN_TT - 1) * D + T + KC;
    const int n_vec = (span + VS - 1) / VS;
    for (int q0 = threadIdx.x; q0 < n_vec; q0 += 4 * blockDim.x) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int q = q0 + u * blockDim.x;
            const long n = n0 + (long)VS * q;
            v[u] = uint4{0u, 0u, 0u, 0u};
            if constexpr (STREAM) {
                const uint8_t *src = n >= 0 ? wide + IB * n : (prev ? prev + IB * (n + n_wide) : nullptr);
                if (q < n_vec && src && n >= -n_wide && n + VS <= n_wide) v[u] = *(const uint4 *)src;
            } else if (q < n_vec) {
                if (n >= 0 && n + VS <= n_wide) {
                    v[u] = *(const uint4 *)(wide + IB * n);
                } else if constexpr (FMT == RD_IQ_S16) {
                    uint32_t e[4];
#pragma unroll
                    for (int w = 0; w < 4; w++) e[w] = (n + w >= 0 && n + w < n_wide) ? *(const uint32_t *)(wide + 4 * (n + w)) : 0u;
                    v[u] = uint4{e[0], e[1], e[2], e[3]};
                } else if constexpr (FMT == RD_IQ_CF32) {
                    uint2 e[2];
#pragma unroll
                    for (int w = 0; w < 2; w++) e[w] = (n + w >= 0 && n + w < n_wide) ? *(const uint2 *)(wide + 8 * (n + w)) : uint2{0u, 0u};
                    v[u] = uint4{e[0].x, e[0].y, e[1].x, e[1].y};
                } else {
                    uint16_t e[8];
#pragma unroll
                    for (int w = 0; w < 8; w++) e[w] = (n + w >= 0 && n + w < n_wide) ? *(const uint16_t *)(wide + 2 * (n + w)) : (uint16_t)0;
                    v[u] = uint4{(uint32_t)e[0] | ((uint32_t)e[1] << 16), (uint32_t)e[2] | ((uint32_t)e[3] << 16),
                                 (uint32_t)e[4] | ((uint32_t)e[5] << 16), (uint32_t)e[6] | ((uint32_t)e[7] << 16)};
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int q = q0 + u * blockDim.x;
            if (q >= n_vec) continue;
            if constexpr (FMT == RD_IQ_S16) {
                const uint2 a = rd_chan_sm16(v[u].x), b = rd_chan_sm16(v[u].y), c = rd_chan_sm16(v[u].z), d = rd_chan_sm16(v[u].w);
                *(uint4 *)(xs + 32 * q) = uint4{a.x, a.y, b.x, b.y};
                *(uint4 *)(xs + 32 * q + 16) = uint4{c.x, c.y, d.x, d.y};
            } else if constexpr (FMT == RD_IQ_CF32) {
                // two samples (I0 Q0 I1 Q1 as float32) -> their eight lanes Ilo Ihi Qlo Qhi | the same of the second
                *(uint4 *)(xs + 16 * q) = uint4{rd_chan_f32_digits(v[u].x), rd_chan_f32_digits(v[u].y),
                                                rd_chan_f32_digits(v[u].z), rd_chan_f32_digits(v[u].w)};
            } else {
                if constexpr (FMT == RD_IQ_S8) {
                    v[u].x ^= 0x80808080u; v[u].y ^= 0x80808080u; v[u].z ^= 0x80808080u; v[u].w ^= 0x80808080u;
                }
                *(uint4 *)(xs + 16 * q) = v[u];
            }
        }
    }
    const int n_chunks = T / KC + 1;
    const uint4 *asrc = amat + (size_t)grp * n_chunks * (RD_CHAN_Q_BYTES / 16);
    // A wave only ever needs ITS row block's A fragments (RD_CHAN_TERMS x 16 bytes per lane and K step):
    // they come straight from L2 into registers, NPF steps ahead - no LDS, no barrier in the loop.
    constexpr int NPF = RD_CHAN_NPF;
    const uint4 *amine = asrc + wave * 64 + lane;   // + (q * RD_CHAN_TERMS + term) * RD_CHAN_RBG * 64
    uint4 pre[NPF][RD_CHAN_TERMS];
#pragma unroll
    for (int s = 0; s < NPF; s++)
#pragma unroll
        for (int term = 0; term < RD_CHAN_TERMS; term++)
            pre[s][term] = amine[(size_t)((s < n_chunks ? s : n_chunks - 1) * RD_CHAN_TERMS + term) * (RD_CHAN_RBG * 64)];
    __syncthreads();  // the staged samples

    rd_f32x16 acc[RD_CHAN_TB];
#pragma unroll
    for (int b = 0; b < RD_CHAN_TB; b++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[b][e] = 0.0f;
    // B fragment of (time block tb, K step q): window samples 8q + 4h .. +3 of column 32 tb + r = eight bytes
    // (I0 Q0 I1 Q1 | I2 Q2 I3 Q3) -> eight 16-bit lanes
    // (RD_IQ_S16, RD_IQ_CF32: window samples 4q + 2h, + 1 = sixteen bytes = the eight 16-bit lanes as they are)
    const uint8_t *xl = xs + LB * (D * r + (KC / 2) * h);
    for (int c0 = 0; c0 < n_chunks; c0 += NPF) {
#pragma unroll
        for (int s = 0; s < NPF; s++) {
            const int q = c0 + s;
            if (q >= n_chunks) break;  // uniform
            rd_f16x8 a[RD_CHAN_TERMS];
#pragma unroll
            for (int term = 0; term < RD_CHAN_TERMS; term++) a[term] = __builtin_bit_cast(rd_f16x8, pre[s][term]);
            {   // refill this slot with step q + NPF (the last steps refetch the final one: a static
                // number of loads in flight)
                const int qn = (q + NPF < n_chunks) ? q + NPF : n_chunks - 1;
#pragma unroll
                for (int term = 0; term < RD_CHAN_TERMS; term++)
                    pre[s][term] = amine[(size_t)(qn * RD_CHAN_TERMS + term) * (RD_CHAN_RBG * 64)];
            }
            using raw_t = typename std::conditional<rd_fmt_digits(FMT), uint4, uint2>::type;
            raw_t raw[RD_CHAN_TB];
#pragma unroll
            for (int tb = 0; tb < RD_CHAN_TB; tb++) raw[tb] = *(const raw_t *)(xl + LB * (D * 32 * tb + KC * q));
#pragma unroll
            for (int tb = 0; tb < RD_CHAN_TB; tb++) {
                uint4 f;
                if constexpr (rd_fmt_digits(FMT)) {
                    f = raw[tb];
                } else {
                    // element order (I0 I1 Q0 Q1 | I2 I3 Q2 Q3) - the A fragments are laid out to match: the even bytes of
                    // a dword by one v_and, the odd ones by one v_perm (selector 0x0c = a zero byte), as in rd_mf_frag
                    f.x = raw[tb].x & 0x00FF00FFu;
                    f.y = __builtin_amdgcn_perm(0u, raw[tb].x, 0x0c030c01u);
                    f.z = raw[tb].y & 0x00FF00FFu;
                    f.w = __builtin_amdgcn_perm(0u, raw[tb].y, 0x0c030c01u);
                }
                const rd_f16x8 bfrag = __builtin_bit_cast(rd_f16x8, f);
#pragma unroll
                for (int term = 0; term < RD_CHAN_TERMS; term++)
                    acc[tb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[term], bfrag, acc[tb], 0, 0, 0);
            }
        }
    }
    // epilogue: register e of tile tb holds row (e & 3) + 8 (e >> 2) + 4 h, column r; rows 2i, 2i+1 =
    // (re, im) of channel 16 (4 grp + wave) + i
    // The output phasor e^{-j 2 pi frac(shift t / Fo)}: the exact remainder once per channel and lane, for the lane's
    // first time block (one float64 product, a quotient by multiplication, the hardware sine and cosine); the three
    // blocks behind it are 32 output times further on each - a rotation by the channel's constant from the table.
    // (Round 3, from the counters: the kernel's vector work - two float64 divisions and a sincospif per OUTPUT - took
    // as long as its MFMAs, and the two do not overlap.)
    const double fo = (double)out_rate, inv_fo = 1.0 / fo;
    // (t0 + r) mod Fo once per lane: a float estimate of the quotient is off by one at most
    long tm = t0 + r;
    if constexpr (STREAM) tm += t_base_mod;
    {
        const long qe = (long)floorf((float)tm * (float)inv_fo);
        tm -= qe * out_rate;
        if (tm < 0) tm += out_rate;
        if (tm >= out_rate) tm -= out_rate;
    }
#pragma unroll
    for (int e = 0; e < 16; e += 2) {
        const int row = (e & 3) + 8 * (e >> 2) + 4 * h;
        const int ch = 16 * (RD_CHAN_RBG * grp + wave) + (row >> 1);
        if (ch >= n_ch) continue;
        // frac((shift t + P) / Fo) exactly: shift, tm, P < Fo < 2^26, product and sum are exact in float64 (< 2^53; P is 0
        // until a retune, rd_chan_retune); the quotient from a multiplication by 1 / Fo is off by one at most
        const double x = (double)shifts[ch] * (double)tm + (double)phase[ch];
        // the channel's gain (GAIN: a table, rd_chan_set_gain / rd_wb_set_gain; every entry (float)cfg.gain until then)
        const float scale = gains[ch] * (FMT == RD_IQ_U8 ? 1.0f / 127.6f : FMT == RD_IQ_S8 ? 1.0f / 128.0f : FMT == RD_IQ_S16 ? 1.0f / 32768.0f : 1.0f);
        double rm = __builtin_fma(-floor(x * inv_fo), fo, x);
        if (rm < 0.0) rm += fo;
        if (rm >= fo) rm -= fo;
        // v_sin_f32 / v_cos_f32 take their argument in revolutions
        const float turns = -(float)(rm * inv_fo);
        float sn = __builtin_amdgcn_sinf(turns), cs = __builtin_amdgcn_cosf(turns);
        const float2 *dcc = dc + (size_t)ch * RD_CHAN_DCN;
        const float2 rot = dcc[RD_CHAN_EARLY + 1];
        const float ci = rot.x, si = rot.y;
#pragma unroll
        for (int tb = 0; tb < RD_CHAN_TB; tb++) {
            const long t = t0 + 32 * tb + r;
            if (t < n_out) {
                float2 d0 = float2{0.0f, 0.0f};   // (RD_IQ_S16, RD_IQ_CF32: signed digits, no DC term)
                if constexpr (!rd_fmt_digits(FMT)) d0 = dcc[t < n_early ? (int)t : RD_CHAN_EARLY];
                const float re = __builtin_fmaf(acc[tb][e], tap_unscale, d0.x), im = __builtin_fmaf(acc[tb][e + 1], tap_unscale, d0.y);
                const float zr = (re * cs - im * sn) * scale, zi = (re * sn + im * cs) * scale;
                const float qr = fminf(fmaxf(rintf(zr * 127.6f + 127.4f), 0.0f), 255.0f);
                const float qi = fminf(fmaxf(rintf(zi * 127.6f + 127.4f), 0.0f), 255.0f);
                *(uint16_t *)(out + (size_t)ch * out_stride + 2 * t) = (uint16_t)((uint32_t)qr | ((uint32_t)qi << 8));
            }
            const float c2 = cs * ci - sn * si, s2 = sn * ci + cs * si;
            cs = c2; sn = s2;
        }
    }
}

// RETUNE (rd_chan_retune; rd_wideband.hip: rd_wb_retune): the tables of the channels whose tuning changes, rebuilt in
// place between two chunks of a stream.  One workgroup per record (channel, shift, shift mod Fo, P); it writes what
// rd_chan_tables_build writes for that channel, through the same functions (rd_chan_tables.h) - the fp32 taps g through
// the exact 64-bit remainder (shift k) mod Fw and float64 sine / cosine, their two-term f16 split in the A operand's fragment
// order (every K step, both lane halves, both terms, the zero taps included: one 16-byte store per fragment), the DC entries summed in
// float64 in the host's order (one lane: t_pad dependent additions while the rest of its wave idles, beside the other
// waves' stores; not measured yet), the 32-output rotation, shift mod Fo and P.
// Equal to the host's tables UP TO LIBM: the device's float64 sin / cos need not equal glibc's in the last bit.  Every
// value is rounded to fp32 before anything else uses it, which absorbs a last-bit difference unless the product lies
// within a float64 ulp or two of an fp32 rounding boundary (about 2^-28 per tap), so the tests that compare a receiver
// reset after a retune with a fresh one byte for byte (tests/test_wideband_retune.py) rely on that, not on a guarantee.
// Should one fail on a new ROCm with a single differing table entry: the definition holds either way (both are the
// correctly-derived fp32 taps within half an ulp + libm's error, inside term 1 of tests/chan_bound.py) - change that test's
// seed or compare it through the model's bound, do not loosen the kernel.  (The f16 values: rd_chan_tables.h.)  The stream
// orders it behind the previous chunk's k_channelize and in front of the next one's: no second copy of the tables.
__global__ __launch_bounds__(256) void k_chan_retune(const int64_t *__restrict__ rec, const double *__restrict__ taps,
                                                     int fmt, int T, int t_pad, int D, long out_rate, double tap_scale,
                                                     uint4 *amat, float2 *dc, int64_t *shifts, int64_t *phase) {
    extern __shared__ uint8_t lds[];
    rd_chan_g *g = (rd_chan_g *)lds;              // the channel's fp32 taps (g_r, g_i), k < t_pad
    const int c = (int)rec[4 * blockIdx.x];
    const long shift = rec[4 * blockIdx.x + 1], smod = rec[4 * blockIdx.x + 2];
    const long fw = out_rate * D;
    for (int k = threadIdx.x; k < t_pad; k += blockDim.x) g[k] = k < T ? rd_chan_tap(taps[k], shift, k, fw) : rd_chan_g{0.0f, 0.0f};
    __syncthreads();
    float *dcc = (float *)(dc + (size_t)c * RD_CHAN_DCN);
    if (threadIdx.x == 0) {
        shifts[c] = smod;
        phase[c] = rec[4 * blockIdx.x + 3];
        rd_chan_rotation(smod, out_rate, dcc + 2 * (RD_CHAN_EARLY + 1));
    }
    // (a lane of the second wave: the first one's has the rotation)
    if (threadIdx.x == 64 && !rd_fmt_digits(fmt)) rd_chan_dc_entries(fmt, g, t_pad, D, dcc);
    const int n_q = t_pad / rd_fmt_kc(fmt) + 1;
    // one fragment (8 f16 = 16 bytes) per item: K step q, term, lane half hh, part
    for (int it = threadIdx.x; it < 8 * n_q; it += blockDim.x) {
        const int part = it & 1, hh = (it >> 1) & 1, tm = (it >> 2) & 1, q = it >> 3;
        uint32_t w[4];
        rd_chan_fragment(fmt, g, t_pad, tap_scale, q, tm, hh, part, w);
        amat[rd_chan_amat_index(c, n_q, q, tm, hh, part)] = uint4{w[0], w[1], w[2], w[3]};
    }
}

// ------------------------------------------------------------------------------------------
// C ABI (include/rtldavis_hip.h)
// ------------------------------------------------------------------------------------------

extern "C" int rd_chan_create(const rd_chan_config *cfg, const double *taps, const int64_t *shift_hz, rd_chan **out) {
    return rd_chan_create_fmt(cfg, RD_IQ_U8, taps, shift_hz, out);
}

extern "C" int rd_chan_create_fmt(const rd_chan_config *cfg, int fmt, const double *taps, const int64_t *shift_hz,
                                  rd_chan **out) {
    if (!out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    rd_chan *h = new rd_chan();
    const int rc = rd_chan_tables_create(h, cfg, fmt, taps, shift_hz);   // (the argument rules; no device)
    if (rc) delete h;
    else *out = h;
    return rc;
}

extern "C" void rd_chan_destroy(rd_chan *h) {
    if (!h) return;
    // device memory belongs to the process that allocated it: a forked copy only drops its host state
    if (h->dev_ready && rd_owns_device_state()) {
        if (h->device >= 0) hipSetDevice(h->device);
        hipFree(h->d_amat); hipFree(h->d_dc); hipFree(h->d_shifts); hipFree(h->d_wide);
        hipFree(h->d_phase); hipFree(h->d_taps); hipFree(h->d_rt); hipHostFree(h->h_rt);
        hipFree(h->d_gains); hipHostFree(h->h_gains);
    }
    rd_spec_destroy(h->spec);      // (checks the owning process itself)
    delete h;
}

static int chan_alloc(rd_chan *h, size_t n_wide) {
    int rc = rd_ensure_device();
    if (rc) return rc;
    if (h->dev_ready && h->device >= 0) HIPCHK(hipSetDevice(h->device));
    if (!h->dev_ready) {
        HIPCHK(hipGetDevice(&h->device));
        HIPCHK(hipMalloc(&h->d_amat, h->h_amat.size() * sizeof(uint16_t)));
        HIPCHK(hipMemcpy(h->d_amat, h->h_amat.data(), h->h_amat.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        HIPCHK(hipMalloc(&h->d_dc, h->h_dc.size() * sizeof(float)));
        HIPCHK(hipMemcpy(h->d_dc, h->h_dc.data(), h->h_dc.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(hipMalloc(&h->d_shifts, h->shifts.size() * sizeof(int64_t)));
        HIPCHK(hipMemcpy(h->d_shifts, h->shifts.data(), h->shifts.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(hipMalloc(&h->d_phase, h->phase.size() * sizeof(int64_t)));
        HIPCHK(hipMemcpy(h->d_phase, h->phase.data(), h->phase.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(hipMalloc(&h->d_gains, h->gains.size() * sizeof(float)));
        HIPCHK(hipMemcpy(h->d_gains, h->gains.data(), h->gains.size() * sizeof(float), hipMemcpyHostToDevice));
        h->dev_ready = true;
    }
    if (n_wide > h->wide_cap) {
        if (h->d_wide) hipFree(h->d_wide);
        h->d_wide = nullptr;
        HIPCHK(hipMalloc(&h->d_wide, rd_fmt_in_bps(h->fmt) * n_wide + 16));
        h->wide_cap = n_wide;
    }
    return RD_OK;
}

extern "C" int rd_chan_input_ptr(rd_chan *h, size_t n_wide_samples, void **dev_ptr) {
    if (!h || !dev_ptr) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = chan_alloc(h, n_wide_samples);
    if (rc) return rc;
    h->wide_n = n_wide_samples;
    *dev_ptr = h->d_wide;
    return RD_OK;
}

extern "C" int rd_chan_upload(rd_chan *h, const void *wide_iq, size_t nbytes) {
    if (!h || !wide_iq) return rd_fail_msg(RD_ERR_ARG, "null argument");
    const size_t bps = (size_t)rd_fmt_in_bps(h->fmt);
    if (nbytes % bps)
        return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: %zu bytes is not a whole number of %zu-byte IQ pairs", nbytes, bps);
    int rc = chan_alloc(h, nbytes / bps);
    if (rc) return rc;
    HIPCHK(hipMemcpy(h->d_wide, wide_iq, nbytes, hipMemcpyHostToDevice));
    h->wide_n = nbytes / bps;
    return RD_OK;
}

// the instantiation of a form and a format
static const void *chan_kernel(bool stream, int fmt) {
    switch (fmt) {
    case RD_IQ_S8: return stream ? (const void *)k_channelize<true, RD_IQ_S8> : (const void *)k_channelize<false, RD_IQ_S8>;
    case RD_IQ_S16: return stream ? (const void *)k_channelize<true, RD_IQ_S16> : (const void *)k_channelize<false, RD_IQ_S16>;
    case RD_IQ_CF32: return stream ? (const void *)k_channelize<true, RD_IQ_CF32> : (const void *)k_channelize<false, RD_IQ_CF32>;
    default: return stream ? (const void *)k_channelize<true, RD_IQ_U8> : (const void *)k_channelize<false, RD_IQ_U8>;
    }
}

static int chan_launch(rd_chan *h, bool stream, const uint8_t *wide, long n_wide, const uint8_t *prev, int n_early,
                       long t_base_mod, long n_out, unsigned gx, void *dst, size_t dst_stride, hipStream_t st) {
    int T = h->t_pad, D = h->cfg.decim, n_ch = h->cfg.n_channels;
    const size_t lds = rd_chan_lds_bytes(h->fmt, D, T);
    const uint4 *amat = (const uint4 *)h->d_amat;
    const float2 *dc = (const float2 *)h->d_dc;
    const int64_t *shifts = h->d_shifts, *phase = h->d_phase;
    long out_rate = (long)h->cfg.out_rate;
    const float *gains = h->d_gains;
    float tap_unscale = h->tap_unscale;
    uint8_t *out = (uint8_t *)dst;
    int xs_bytes = (int)lds;
    void *args[] = {&wide, &n_wide, &amat, &dc, &shifts, &T, &D, &n_ch, &n_early, &out_rate, &gains, &tap_unscale, &n_out,
                    &out, &dst_stride, &xs_bytes, &prev, &t_base_mod, &phase};   // k_channelize's parameters, in order
    HIPCHK(hipLaunchKernel(chan_kernel(stream, h->fmt), dim3(gx, (unsigned)h->n_groups), dim3(256), args, lds, st));
    HIPCHK(hipGetLastError());
    return RD_OK;
}

extern "C" int rd_chan_run(rd_chan *h, size_t n_out, void *dst_dev, size_t dst_stream_stride, void *hip_stream) {
    if (!h || !dst_dev) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (!h->dev_ready || !h->d_wide) return rd_fail_msg(RD_ERR_STATE, "no capture resident: rd_chan_upload first");
    if (n_out == 0) return RD_OK;
    if (n_out > h->wide_n / (size_t)h->cfg.decim || n_out > 0x7FFFFFFFull)
        return rd_fail_msg(RD_ERR_ARG, "n_out exceeds capture length / decim");
    if (dst_stream_stride < 2 * n_out || (dst_stream_stride & 1))
        return rd_fail_msg(RD_ERR_ARG, "destination stride too small for n_out samples");
    const size_t lds = rd_chan_lds_bytes(h->fmt, h->cfg.decim, h->t_pad);
    HIPCHK(hipFuncSetAttribute(chan_kernel(false, h->fmt), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned gx = (unsigned)((n_out + RD_CHAN_TT - 1) / RD_CHAN_TT);
    return chan_launch(h, false, h->d_wide, (long)h->wide_n, nullptr, h->n_early, 0L, (long)n_out, gx, dst_dev,
                       dst_stream_stride, (hipStream_t)hip_stream);
}

extern "C" int rd_chan_run_host(rd_chan *h, size_t n_out, uint8_t *out_host, size_t nbytes) {
    if (!h || !out_host) return rd_fail_msg(RD_ERR_ARG, "null argument");
    const size_t need = (size_t)h->cfg.n_channels * n_out * 2;
    if (nbytes != need) return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: got %zu bytes, expected %zu", nbytes, need);
    if (n_out == 0) return RD_OK;
    uint8_t *d = nullptr;
    HIPCHK(hipMalloc(&d, need));
    int rc = rd_chan_run(h, n_out, d, 2 * n_out, nullptr);
    if (rc == RD_OK) {
        hipError_t e = hipMemcpy(out_host, d, need, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = rd_fail_msg(RD_ERR_DEVICE, "hipMemcpy: %s", hipGetErrorString(e));
    }
    hipFree(d);
    return rc;
}

// SPECTRUM, one-shot form: the power spectrum of the uploaded capture (rd_spectrum.hip: the kernel and launch helper the
// streaming receiver uses per chunk, so a chunk uploaded alone gives that chunk's record bit for bit).  rd_chan_spectrum_dev
// queues it on a stream into device memory (as rd_chan_run does); rd_chan_spectrum is the synchronous host form.
extern "C" int rd_chan_spectrum_dev(rd_chan *h, int n_bins, void *dst_dev, void *hip_stream) {
    if (!h || !dst_dev) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (!h->dev_ready || !h->d_wide || !h->wide_n) return rd_fail_msg(RD_ERR_STATE, "no capture resident: rd_chan_upload first");
    int rc = rd_spec_check(n_bins, h->wide_n);
    if (rc) return rc;
    if (h->device >= 0) HIPCHK(hipSetDevice(h->device));
    if ((rc = rd_spec_prepare(&h->spec, n_bins, h->wide_n, (hipStream_t)hip_stream))) return rc;
    return rd_spec_launch(h->spec, h->d_wide, h->fmt, h->wide_n, 0, dst_dev, (hipStream_t)hip_stream);
}

extern "C" int rd_chan_spectrum(rd_chan *h, int n_bins, double *power_host, uint32_t *segments) {
    if (!h || !power_host) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (!h->dev_ready || !h->d_wide || !h->wide_n) return rd_fail_msg(RD_ERR_STATE, "no capture resident: rd_chan_upload first");
    int rc = rd_spec_check(n_bins, h->wide_n);
    if (rc) return rc;
    const size_t bytes = RD_SPEC_HDR_BYTES + (size_t)n_bins * sizeof(double);
    uint8_t *d = nullptr;
    HIPCHK(hipMalloc(&d, bytes));
    std::vector<uint8_t> rec(bytes);
    rc = rd_chan_spectrum_dev(h, n_bins, d, nullptr);
    if (rc == RD_OK) {
        hipError_t e = hipMemcpy(rec.data(), d, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = rd_fail_msg(RD_ERR_DEVICE, "hipMemcpy: %s", hipGetErrorString(e));
    }
    hipFree(d);
    if (rc) return rc;
    memcpy(power_host, rec.data() + RD_SPEC_HDR_BYTES, (size_t)n_bins * sizeof(double));
    if (segments) memcpy(segments, rec.data() + 8, sizeof(uint32_t));
    return RD_OK;
}

// ------------------------------------------------------------------------------------------
// Streaming form (rd_internal.h; used by rd_wideband.hip)
// ------------------------------------------------------------------------------------------
// the device tables, on the current device (no capture buffer: the caller owns its chunk buffers)
int rd_chan_stream_prepare(rd_chan *h) {
    if (!h) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = chan_alloc(h, 0);
    if (rc) return rc;
    const size_t lds = rd_chan_lds_bytes(h->fmt, h->cfg.decim, h->t_pad);
    HIPCHK(hipFuncSetAttribute(chan_kernel(true, h->fmt), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (!h->d_taps) {   // what a retune needs: the float64 taps, and the records' staging (two pinned slots, one on the device)
        const size_t rt_bytes = (size_t)h->cfg.n_channels * 4 * sizeof(int64_t);
        HIPCHK(hipMalloc(&h->d_taps, h->taps.size() * sizeof(double)));
        HIPCHK(hipMemcpy(h->d_taps, h->taps.data(), h->taps.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMalloc(&h->d_rt, rt_bytes));
        HIPCHK(hipHostMalloc((void **)&h->h_rt, 2 * rt_bytes, hipHostMallocDefault));
        HIPCHK(hipHostMalloc((void **)&h->h_gains, 2 * (size_t)h->cfg.n_channels * sizeof(float), hipHostMallocDefault));
        HIPCHK(hipFuncSetAttribute((const void *)k_chan_retune, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(h->t_pad * sizeof(float2))));
    }
    return RD_OK;
}

// Retune n channels (header: RETUNE): rec = n x (channel, shift in Hz as given, phase accumulator P in [0, out_rate)),
// the caller's arithmetic (rd_wideband.hip).  Before the device tables exist the channels are rebuilt on the host, which
// chan_alloc then uploads; afterwards the records go through pinned slot `slot` (0 / 1: the caller knows that slot's
// last copy has completed) and k_chan_retune, both queued on st - in front of the next rd_chan_stream_launch on it.
int rd_chan_retune(rd_chan *h, const int64_t *rec, int n, int slot, hipStream_t st) {
    if (!h || (n > 0 && !rec)) return rd_fail_msg(RD_ERR_ARG, "null argument");
    const int n_ch = h->cfg.n_channels;
    const int64_t fo = h->cfg.out_rate;
    if (n < 0 || n > n_ch || (slot & ~1)) return rd_fail_msg(RD_ERR_ARG, "retune: %d records for %d channels, slot %d", n, n_ch, slot);
    for (int i = 0; i < n; i++)
        if (rec[3 * i] < 0 || rec[3 * i] >= n_ch || rec[3 * i + 2] < 0 || rec[3 * i + 2] >= fo)
            return rd_fail_msg(RD_ERR_ARG, "retune: record %d out of range", i);
    if (n == 0) return RD_OK;
    if (!h->dev_ready) {
        for (int i = 0; i < n; i++) rd_chan_tables_build(h, (int)rec[3 * i], rec[3 * i + 1], rec[3 * i + 2]);
        return RD_OK;
    }
    if (!h->d_taps) return rd_fail_msg(RD_ERR_STATE, "rd_chan_stream_prepare first");
    int64_t *stage = h->h_rt + (size_t)slot * n_ch * 4;
    for (int i = 0; i < n; i++) {
        stage[4 * i] = rec[3 * i]; stage[4 * i + 1] = rec[3 * i + 1]; stage[4 * i + 2] = rd_chan_shift_mod(rec[3 * i + 1], fo);
        stage[4 * i + 3] = rec[3 * i + 2];
    }
    HIPCHK(hipMemcpyAsync(h->d_rt, stage, (size_t)n * 4 * sizeof(int64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_chan_retune, dim3((unsigned)n), dim3(256), h->t_pad * sizeof(float2), st, (const int64_t *)h->d_rt,
                       (const double *)h->d_taps, h->fmt, h->cfg.n_taps, h->t_pad, h->cfg.decim, (long)h->cfg.out_rate,
                       h->tap_scale, (uint4 *)h->d_amat, (float2 *)h->d_dc, h->d_shifts, h->d_phase);
    HIPCHK(hipGetLastError());
    // queued: only now does the host's record of what the tables hold follow (a failure above leaves it, and the
    // caller's pending retune, as they were - the next submit tries again)
    for (int i = 0; i < n; i++) {
        const int c = (int)stage[4 * i];
        h->shift_hz[c] = stage[4 * i + 1];
        h->shifts[c] = stage[4 * i + 2];
        h->phase[c] = stage[4 * i + 3];
    }
    return RD_OK;
}

// GAIN: the argument check of rd_chan_set_gain / rd_wb_set_gain (rd_chan_tables.cpp: rd_chan_tables_check_gains)
int rd_chan_check_gains(const rd_chan *h, const double *gain, int n) { return rd_chan_tables_check_gains(h, gain, n); }

// One-shot form: the gains of the runs that follow.  A quiet handle: the caller has waited for the streams its earlier
// rd_chan_run calls were queued on (the copy below is not ordered against them).
extern "C" int rd_chan_set_gain(rd_chan *h, const double *gain, int n) {
    int rc = rd_chan_check_gains(h, gain, n);
    if (rc) return rc;
    std::vector<float> g(n);
    for (int c = 0; c < n; c++) g[c] = (float)gain[c];
    if (h->dev_ready) {
        if (h->device >= 0) HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipMemcpy(h->d_gains, g.data(), g.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    h->gains = g;   // (before the device tables exist chan_alloc uploads them)
    return RD_OK;
}

const float *rd_chan_gains(const rd_chan *h) { return h->gains.data(); }

// Streaming form: make the table `gain` (n_channels float32, checked by the caller) for the kernels queued on st after
// this.  Nothing differs: nothing queued.  Before the device tables exist the host's copy changes; afterwards the table
// travels through pinned slot `slot` (free by the caller's ordering, as rd_chan_retune's) in one copy on st - the
// whole table, 4 bytes a channel, rather than a scatter of the entries that changed.
int rd_chan_stream_gains(rd_chan *h, const float *gain, int slot, hipStream_t st) {
    if (!h || !gain || (slot & ~1)) return rd_fail_msg(RD_ERR_ARG, "stream gains: null argument or slot %d", slot);
    const size_t n = h->gains.size();
    if (!memcmp(gain, h->gains.data(), n * sizeof(float))) return RD_OK;
    if (h->dev_ready) {
        if (!h->h_gains) return rd_fail_msg(RD_ERR_STATE, "rd_chan_stream_prepare first");
        float *stage = h->h_gains + (size_t)slot * n;
        memcpy(stage, gain, n * sizeof(float));
        HIPCHK(hipMemcpyAsync(h->d_gains, stage, n * sizeof(float), hipMemcpyHostToDevice, st));
    }
    h->gains.assign(gain, gain + n);
    return RD_OK;
}

void rd_chan_tuning(const rd_chan *h, const int64_t **shift_hz, const int64_t **phase) {
    *shift_hz = h->shift_hz.data();
    *phase = h->phase.data();
}

// Channelize one chunk of n_out * decim samples (of the handle's format) at `wide` (device) whose predecessor lies at `prev` (null: zero history)
// into dst (channel c at dst + c * dst_stride); t_base = the absolute output time of the chunk's first output.
int rd_chan_stream_launch(rd_chan *h, const uint8_t *wide, const uint8_t *prev, size_t n_out, uint64_t t_base, void *dst,
                          size_t dst_stride, hipStream_t st) {
    if (!h || !wide || !dst) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (!h->dev_ready) return rd_fail_msg(RD_ERR_STATE, "rd_chan_stream_prepare first");
    if (n_out == 0 || n_out % RD_CHAN_TT || n_out > 0x7FFFFFFFull / (size_t)h->cfg.decim || t_base % RD_CHAN_TT ||
        dst_stride < 2 * n_out || (dst_stride & 1))
        return rd_fail_msg(RD_ERR_ARG, "streamed chunk: n_out and t_base must be multiples of %d", RD_CHAN_TT);
    const int T = h->t_pad, D = h->cfg.decim;
    const long n_wide = (long)(n_out * (size_t)D);
    if (T > n_wide) return rd_fail_msg(RD_ERR_ARG, "the taps reach further back than one chunk");
    const long t_base_mod = (long)(t_base % (uint64_t)h->cfg.out_rate);
    const int n_early = t_base == 0 ? h->n_early : 0;   // the early DC table: absolute t < n_early only
    const unsigned gx = (unsigned)(n_out / RD_CHAN_TT);
    return chan_launch(h, true, wide, n_wide, prev, n_early, t_base_mod, (long)n_out, gx, dst, dst_stride, st);
}

int rd_chan_format(const rd_chan *h) { return h ? h->fmt : RD_IQ_U8; }
int rd_chan_n_channels(const rd_chan *h) { return h ? h->cfg.n_channels : 0; }
int rd_chan_decim(const rd_chan *h) { return h ? h->cfg.decim : 0; }
const float *rd_chan_device_gains(const rd_chan *h) { return h && h->dev_ready ? h->d_gains : nullptr; }
int64_t rd_chan_out_rate(const rd_chan *h) { return h ? h->cfg.out_rate : 0; }
int64_t rd_chan_wide_rate(const rd_chan *h) { return h ? (int64_t)h->cfg.out_rate * h->cfg.decim : 0; }
int rd_chan_bytes_per_sample(const rd_chan *h) { return h ? rd_fmt_in_bps(h->fmt) : 0; }
