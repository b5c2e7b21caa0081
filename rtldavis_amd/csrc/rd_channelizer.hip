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
// Levels: k = clip(rint(2^15 adm(v)), -32768, 32767) per component, i.e. int16 units (k_chan_levels).
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
// LEVELS (k_chan_levels, streaming form): what the gains leave of the byte range, per channel and chunk, and how hard the
// capture drives the ADC - exact integers for a gain control on the host (rtldavis_amd/agc.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/rtldavis_hip.h"
#include "rd_internal.h"

#define RD_CHAN_TB 4                        // 32-time blocks per wave
#define RD_CHAN_TT (32 * RD_CHAN_TB)        // output times per workgroup
#define RD_CHAN_RBG 4                       // row blocks (32 rows = 16 channels) per workgroup: one per wave
#define RD_CHAN_KC 8                        // window samples per K step of the 8-bit formats (taps are padded to a multiple)
#define RD_CHAN_TERMS 2                     // f16 digits per tap
#define RD_CHAN_Q_BYTES (RD_CHAN_TERMS * RD_CHAN_RBG * 64 * 16)  // A bytes per K step: terms x 4 row blocks x 64 lanes x 16 B
#ifndef RD_CHAN_NPF
#define RD_CHAN_NPF 2                       // A chunks in flight in registers
#endif
#ifndef RD_CHAN_MINWAVES
#define RD_CHAN_MINWAVES 4                  // waves per SIMD the register allocation aims at (26 KiB of LDS admit 6)
#endif
#define RD_CHAN_EARLY 64                    // outputs per channel with a partial-history DC term kept in a table
#define RD_CHAN_DCN (RD_CHAN_EARLY + 2)     // table entries per channel: the early DC terms, the steady one, and the
                                            // phasor of 32 output times e^{-j 2 pi frac(32 shift / Fo)} (cos, sin)

// per sample format (rtldavis_hip.h: RD_IQ_*): bytes of an IQ pair in memory and staged in LDS, window samples per K step
__host__ __device__ constexpr int rd_fmt_in_bps(int f) { return f == RD_IQ_CF32 ? 8 : f == RD_IQ_S16 ? 4 : 2; }
__host__ __device__ constexpr int rd_fmt_lds_bps(int f) { return f == RD_IQ_S16 || f == RD_IQ_CF32 ? 8 : 2; }
__host__ __device__ constexpr int rd_fmt_kc(int f) { return f == RD_IQ_S16 || f == RD_IQ_CF32 ? RD_CHAN_KC / 2 : RD_CHAN_KC; }
// two 16-bit digits per component (four lanes per staged sample): the formats whose B fragment is one ds_read_b128
__host__ __device__ constexpr bool rd_fmt_digits(int f) { return f == RD_IQ_S16 || f == RD_IQ_CF32; }
// RD_CF32_CLAMP (adm: |v| <= 8) and rd_chan_adm: rd_internal.h (k_chan_spectrum admits float32 components the same way)
#define RD_CF32_PRESCALE_LOG2 12            // staged s = 2^12 adm(v), |s| <= 2^15 < 65504

typedef float rd_f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 rd_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 rd_f16x2 __attribute__((ext_vector_type(2)));

struct rd_chan {
    rd_chan_config cfg;
    int fmt = RD_IQ_U8;            // sample format of the capture
    int n_groups = 0;              // groups of 64 channels
    int t_pad = 0;                 // taps rounded up to RD_CHAN_KC (zero taps appended)
    int n_early = 0;               // outputs whose window reaches before the capture: ceil((t_pad - 1) / D)
    float tap_unscale = 1.0f;      // 2^-s: the taps in h_amat are scaled by 2^s
    std::vector<uint16_t> h_amat;  // f16 A operand in fragment order [group][K step][term][row block][lane][8]
    std::vector<float> h_dc;       // [channel][RD_CHAN_DCN][2]: -127.4 (1+j) sum of the taps a given output sees; the 32-step phasor
    std::vector<int64_t> shifts;   // Hz, reduced mod out_rate
    // the tuning the tables hold (rd_chan_retune): the shifts as given, and the phase accumulators P_c in [0, out_rate)
    std::vector<int64_t> shift_hz, phase;
    std::vector<double> taps;      // the float64 prototype (a retune rebuilds a channel's tables from it)
    double tap_scale = 1.0;        // 2^s
    uint16_t *d_amat = nullptr;
    float *d_dc = nullptr;
    int64_t *d_shifts = nullptr;
    int64_t *d_phase = nullptr;
    // GAIN: the per-channel gains the table holds (float32, (float)cfg.gain each at create), the device table, and two
    // pinned slots of [n_channels] for the streaming form's updates (rd_chan_stream_gains)
    std::vector<float> gains;
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

// x mod m for integer-valued 0 <= x < 2^53, 1 <= m < 2^26 (exact: one fma, one correction step)
__device__ __forceinline__ double rd_chan_mod(double x, double m) {
    double r = fma(-floor(x / m), m, x);
    if (r < 0.0) r += m;
    if (r >= m) r -= m;
    return r;
}

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
// chan_build_channel writes for that channel, by the same expressions - the fp32 taps g through the exact 64-bit
// remainder (shift k) mod Fw and float64 sine / cosine, their two-term f16 split in the A operand's fragment order (every
// K step, both lane halves, both terms, the zero taps included: one 16-byte store per fragment), the DC entries summed in
// float64 in the host's order (one lane: t_pad dependent additions while the rest of its wave idles, beside the other
// waves' stores; not measured yet), the 32-output rotation, shift mod Fo and P.
// Equal to the host's tables UP TO LIBM: the device's float64 sin / cos need not equal glibc's in the last bit.  Every
// value is rounded to fp32 before anything else uses it, which absorbs a last-bit difference unless the product lies
// within a float64 ulp or two of an fp32 rounding boundary (about 2^-28 per tap), so the tests that compare a receiver
// reset after a retune with a fresh one byte for byte (tests/test_wideband_retune.py) rely on that, not on a guarantee.
// Should one fail on a new ROCm with a single differing table entry: the definition holds either way (both are the
// correctly-derived fp32 taps within half an ulp + libm's error, inside term 1 of tests/chan_bound.py) - change that test's
// seed or compare it through the model's bound, do not loosen the kernel.  The f16 values: a 2^s is an fp32 number and so is what the first digit leaves of it,
// so both digits are one rounding each, float -> half.  The stream orders it behind the previous chunk's k_channelize and
// in front of the next one's: no second copy of the tables.
__global__ __launch_bounds__(256) void k_chan_retune(const int64_t *__restrict__ rec, const double *__restrict__ taps,
                                                     int fmt, int T, int t_pad, int D, long out_rate, double tap_scale,
                                                     uint4 *amat, float2 *dc, int64_t *shifts, int64_t *phase) {
    extern __shared__ uint8_t lds[];
    float2 *g = (float2 *)lds;                    // the channel's fp32 taps (g_r, g_i), k < t_pad
    const int c = (int)rec[4 * blockIdx.x];
    const long shift = rec[4 * blockIdx.x + 1], smod = rec[4 * blockIdx.x + 2];
    const long fw = out_rate * D;
    const double wide_rate = (double)out_rate * D;
    for (int k = threadIdx.x; k < t_pad; k += blockDim.x) {
        float2 v = float2{0.0f, 0.0f};
        if (k < T) {
            long r = (shift * k) % fw;            // |shift| <= Fw / 2 < 2^37, k < 2^13: exact in 64 bits
            if (r < 0) r += fw;
            const double ph = 2.0 * M_PI * ((double)r / wide_rate);
            v = float2{(float)(taps[k] * cos(ph)), (float)(taps[k] * sin(ph))};
        }
        g[k] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        shifts[c] = smod;
        phase[c] = rec[4 * blockIdx.x + 3];
        const long inc = (smod * 32) % out_rate;
        const double ph = -2.0 * M_PI * ((double)inc / (double)out_rate);
        dc[(size_t)c * RD_CHAN_DCN + RD_CHAN_EARLY + 1] = float2{(float)cos(ph), (float)sin(ph)};
    }
    if (threadIdx.x == 64 && !rd_fmt_digits(fmt)) {   // (a lane of the second wave: the first one's has the rotation)
        const double dc_level = fmt == RD_IQ_U8 ? 127.4 : 128.0;
        double sr = 0.0, si = 0.0;
        int kdone = 0;
        for (int t = 0; t <= RD_CHAN_EARLY; t++) {
            const long kmax = t < RD_CHAN_EARLY && fmt == RD_IQ_U8 ? (long)D * t : (long)t_pad - 1;
            for (; kdone < t_pad && kdone <= kmax; kdone++) { sr += (double)g[kdone].x; si += (double)g[kdone].y; }
            dc[(size_t)c * RD_CHAN_DCN + t] = float2{(float)(-dc_level * (sr - si)), (float)(-dc_level * (sr + si))};
        }
    }
    const int kc = rd_fmt_kc(fmt), per_lane = kc / 2, n_q = t_pad / kc + 1;
    const bool two = rd_fmt_digits(fmt);          // two digits per component; int16's low one meets taps scaled 2^-8, cf32's does not
    const int grp = c / (16 * RD_CHAN_RBG), rb = (c / 16) % RD_CHAN_RBG, r0 = 2 * (c % 16);
    // one fragment (8 f16 = 16 bytes) per item: K step q, term, lane half hh, part
    for (int it = threadIdx.x; it < 8 * n_q; it += blockDim.x) {
        const int part = it & 1, hh = (it >> 1) & 1, tm = (it >> 2) & 1, q = it >> 3;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int el = 0; el < 8; el++) {
            // the inverse of chan_build_channel's element position: (I0 I1 Q0 Q1 | I2 I3 Q2 Q3), or (Ilo Ihi Qlo Qhi) x 2 (int16, cf32)
            const int comp = (el >> 1) & 1;
            const int sl = two ? el >> 2 : 2 * (el >> 2) + (el & 1), dig = two ? el & 1 : 1;
            const int k = t_pad - (q * kc + hh * per_lane + sl);
            if (k < 0 || k >= t_pad) continue;
            const float2 gk = g[k];
            const double a = part == 0 ? (comp == 0 ? (double)gk.x : -(double)gk.y) : (comp == 0 ? (double)gk.y : (double)gk.x);
            const double as = a * tap_scale * (fmt == RD_IQ_S16 && dig == 0 ? 1.0 / 256.0 : 1.0);
            const _Float16 hi = (_Float16)(float)as;
            const _Float16 lo = (_Float16)(float)(as - (double)hi);
            const uint32_t bits = (uint32_t)__builtin_bit_cast(uint16_t, tm == 0 ? hi : lo);
            w[el >> 1] |= bits << (16 * (el & 1));
        }
        const int lane = 32 * hh + r0 + part;
        amat[((((size_t)grp * n_q + q) * RD_CHAN_TERMS + tm) * RD_CHAN_RBG + rb) * 64 + lane] = uint4{w[0], w[1], w[2], w[3]};
    }
}

// LEVELS (rd_wideband.hip: rd_wb_set_levels / rd_wb_levels): the level records of one streamed chunk, every one an exact
// integer, so the order of summation does not matter.  One launch of n_channels + n_in workgroups behind the chunk's
// k_channelize.
//   workgroup c < n_channels: the 2 B bytes b of channel c's channelized chunk, a = 2 b - 255: peak = max |a|, clipped =
//     bytes 0 or 255, power = sum a^2 = 4 sum b^2 - 1020 sum b + 65025 (2 B), and the float32 gain in force.
//   the n_in workgroups behind them: the capture chunk's components in slices (a grid-stride loop over 16-byte vectors),
//     combined by integer atomics on five device words (max, max, add, 64-bit adds); the workgroup that draws the last
//     ticket takes the totals out (an exchange with 0, which leaves the words clear for the next launch) and writes the
//     record.  uint8: a = 2 k - 255 as above.  int8: bit 7 flipped, u = k + 128, is the same byte arithmetic with
//     a = u - 128, power = sum u^2 - 256 sum u + 16384 n, the ends -128 / 127 are u = 0 / 255.  int16: a = k per component.
//     float32: a = k = clip(rint(2^15 adm(v)), -32768, 32767) per component - int16 units, full scale 32768 -, clipped =
//     components with k at either end plus NaN components (a NaN is the value 0 for peak and power).
// Sum b and sum b^2 of a dword are one packed-byte dot product each (v_dot4_u32_u8 against 0x01010101 and against
// itself); the byte maxima are packed 16-bit maxima over the even and the odd bytes; a byte at an end of the range is a
// zero byte of w or of ~w, counted by the carry-free zero-byte test and a population count.  A lane adds a vector's two
// sums (<= 16 x 65025) to 64-bit totals; then a wave reduction by shuffles, LDS across the four waves, and lane 0 writes
// the record with plain stores - straight into the mapped host slot of the chunk's parity, which the host reads after
// the chunk's demodulator launch, later on the same stream, has reported.
// Overflow: a chunk has at most 2^32 - 2 components (rd_chan_stream_launch: n_out decim <= 2^31 - 1 IQ pairs), a^2 <=
// 65025 < 2^16 for the bytes and <= 2^30 for int16: power < 2^62, the 32-bit counts < 2^32 - no chunk
// rd_wb_create_fmt admits can overflow a field.  The device-side totals of the int8 / uint8 forms (sum u^2 < 2^48) likewise.
#define RD_LV_THREADS 256
#define RD_LV_MAX_SLICES 256                // workgroups over the capture chunk (8 vectors per lane and pass below that)
// RD_LV_ACC_WORDS (rd_internal.h) = 8: max b, max 255 - b (or max |k|), ends, ticket, sum u (64 bit), sum u^2 (64 bit)

typedef unsigned short rd_u16x2 __attribute__((ext_vector_type(2)));

struct rd_lv_sums {
    uint32_t hi, lo;       // packed 16-bit lanes while a lane runs, then scalars: max b and max (255 - b); int16, cf32: max |k|, 0
    uint32_t ends;
    uint64_t s1, s2;       // sum u, sum u^2 (int16: 0, sum k^2)
};

__device__ __forceinline__ uint32_t rd_lv_pkmax(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(rd_u16x2, a), __builtin_bit_cast(rd_u16x2, b)));
}
// bytes of n that are zero (no carry crosses a byte: 0x7F + 0x7F < 0x100)
__device__ __forceinline__ uint32_t rd_lv_zero_bytes(uint32_t n) {
    return (uint32_t)__builtin_popcount(~((((n & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | n) | 0x7F7F7F7Fu));
}
__device__ __forceinline__ void rd_lv_bytes(rd_lv_sums &a, uint4 v, uint32_t flip) {
    const uint32_t w[4] = {v.x ^ flip, v.y ^ flip, v.z ^ flip, v.w ^ flip};
    uint32_t s1 = 0u, s2 = 0u;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t e = w[i] & 0x00FF00FFu, o = (w[i] >> 8) & 0x00FF00FFu;
        a.hi = rd_lv_pkmax(rd_lv_pkmax(a.hi, e), o);
        a.lo = rd_lv_pkmax(rd_lv_pkmax(a.lo, e ^ 0x00FF00FFu), o ^ 0x00FF00FFu);
        a.ends += rd_lv_zero_bytes(w[i]) + rd_lv_zero_bytes(~w[i]);
        s1 = __builtin_amdgcn_udot4(w[i], 0x01010101u, s1, false);
        s2 = __builtin_amdgcn_udot4(w[i], w[i], s2, false);
    }
    a.s1 += s1;
    a.s2 += s2;
}
__device__ __forceinline__ void rd_lv_words(rd_lv_sums &a, uint4 v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int k0 = (int)(int16_t)(w[i] & 0xFFFFu), k1 = (int)w[i] >> 16;
        const uint32_t m0 = (uint32_t)(k0 < 0 ? -k0 : k0), m1 = (uint32_t)(k1 < 0 ? -k1 : k1);   // 0 .. 32768
        a.hi = max(a.hi, max(m0, m1));
        a.ends += (uint32_t)(k0 == -32768 || k0 == 32767) + (uint32_t)(k1 == -32768 || k1 == 32767);
        a.s2 += (uint64_t)(m0 * m0 + m1 * m1);   // <= 2^31
    }
}
// float32 components in int16 units (header: RD_IQ_CF32): k = clip(rint(2^15 adm(v)), -32768, 32767), the product exact
// in fp32, rint ties-to-even; a NaN is the value 0 and counts as clipped
__device__ __forceinline__ void rd_lv_floats(rd_lv_sums &a, uint4 v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float f = __builtin_bit_cast(float, w[i]);
        const int k = (int)fminf(fmaxf(rintf(rd_chan_adm(w[i]) * 32768.0f), -32768.0f), 32767.0f);
        const uint32_t m = (uint32_t)(k < 0 ? -k : k);   // 0 .. 32768
        a.hi = max(a.hi, m);
        a.ends += (uint32_t)(k == -32768 || k == 32767 || f != f);
        a.s2 += (uint64_t)(m * m);   // <= 2^30
    }
}
// the workgroup's totals in thread 0 (hi / lo as scalars)
__device__ __forceinline__ void rd_lv_reduce(rd_lv_sums &a, bool packed) {
    __shared__ uint32_t r32[3][RD_LV_THREADS / 64];
    __shared__ uint64_t r64[2][RD_LV_THREADS / 64];
    if (packed) {
        a.hi = max(a.hi & 0xFFFFu, a.hi >> 16);
        a.lo = max(a.lo & 0xFFFFu, a.lo >> 16);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a.hi = max(a.hi, (uint32_t)__shfl_xor((int)a.hi, off));
        a.lo = max(a.lo, (uint32_t)__shfl_xor((int)a.lo, off));
        a.ends += (uint32_t)__shfl_xor((int)a.ends, off);
        a.s1 += (uint64_t)__shfl_xor((unsigned long long)a.s1, off);
        a.s2 += (uint64_t)__shfl_xor((unsigned long long)a.s2, off);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { r32[0][wave] = a.hi; r32[1][wave] = a.lo; r32[2][wave] = a.ends; r64[0][wave] = a.s1; r64[1][wave] = a.s2; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < RD_LV_THREADS / 64; w++) {
            a.hi = max(a.hi, r32[0][w]); a.lo = max(a.lo, r32[1][w]); a.ends += r32[2][w]; a.s1 += r64[0][w]; a.s2 += r64[1][w];
        }
}

__global__ __launch_bounds__(RD_LV_THREADS) void k_chan_levels(const uint4 *__restrict__ chan, size_t ch_stride_vec, size_t ch_vec,
                                                               int n_ch, const float *__restrict__ gains,
                                                               const uint4 *__restrict__ wide, size_t in_vec, int fmt, unsigned n_in,
                                                               uint64_t seq, rd_chan_level *out, rd_input_level *in, uint32_t *acc) {
    rd_lv_sums a = {0u, 0u, 0u, 0ull, 0ull};
    if ((int)blockIdx.x < n_ch) {
        const int c = (int)blockIdx.x;
        const uint4 *src = chan + (size_t)c * ch_stride_vec;
#pragma unroll 4
        for (size_t q = threadIdx.x; q < ch_vec; q += RD_LV_THREADS) rd_lv_bytes(a, src[q], 0u);
        rd_lv_reduce(a, true);
        if (threadIdx.x == 0) {
            const uint64_t n = 16 * (uint64_t)ch_vec;
            out[c].power = 4 * a.s2 + 65025 * n - 1020 * a.s1;
            out[c].peak = max(2 * a.hi, 2 * a.lo) - 255u;     // (one of the two is >= 128)
            out[c].clipped = a.ends;
            out[c].gain = gains[c];
            out[c].chunk = (uint32_t)seq;
        }
        return;
    }
    const unsigned slice = blockIdx.x - (unsigned)n_ch;
    const size_t stride = (size_t)n_in * RD_LV_THREADS;
    if (fmt == RD_IQ_S16) {
#pragma unroll 4
        for (size_t q = (size_t)slice * RD_LV_THREADS + threadIdx.x; q < in_vec; q += stride) rd_lv_words(a, wide[q]);
    } else if (fmt == RD_IQ_CF32) {
#pragma unroll 4
        for (size_t q = (size_t)slice * RD_LV_THREADS + threadIdx.x; q < in_vec; q += stride) rd_lv_floats(a, wide[q]);
    } else {
        const uint32_t flip = fmt == RD_IQ_S8 ? 0x80808080u : 0u;
#pragma unroll 4
        for (size_t q = (size_t)slice * RD_LV_THREADS + threadIdx.x; q < in_vec; q += stride) rd_lv_bytes(a, wide[q], flip);
    }
    rd_lv_reduce(a, !rd_fmt_digits(fmt));
    if (threadIdx.x != 0) return;
    unsigned long long *acc64 = (unsigned long long *)(acc + 4);
    atomicMax(&acc[0], a.hi);
    atomicMax(&acc[1], a.lo);
    atomicAdd(&acc[2], a.ends);
    atomicAdd(&acc64[0], (unsigned long long)a.s1);
    atomicAdd(&acc64[1], (unsigned long long)a.s2);
    __threadfence();
    if (atomicAdd(&acc[3], 1u) != n_in - 1) return;
    __threadfence();
    // the last ticket: every slice's atomics have been performed; take the totals and leave zeros
    const uint32_t hi = atomicExch(&acc[0], 0u), lo = atomicExch(&acc[1], 0u), ends = atomicExch(&acc[2], 0u);
    const uint64_t s1 = atomicExch(&acc64[0], 0ull), s2 = atomicExch(&acc64[1], 0ull);
    atomicExch(&acc[3], 0u);
    const uint64_t n = 16 * (uint64_t)in_vec;                // bytes of the chunk
    if (fmt == RD_IQ_U8) {
        in->power = 4 * s2 + 65025 * n - 1020 * s1;
        in->peak = max(2 * hi, 2 * lo) - 255u;
    } else if (fmt == RD_IQ_S8) {
        in->power = s2 + 16384 * n - 256 * s1;
        in->peak = max(hi + 127u, lo + 128u) - 255u;         // max(max u - 128, 128 - min u)
    } else {
        in->power = s2;
        in->peak = hi;
    }
    in->clipped = ends;
    in->chunk = seq;
}

// ------------------------------------------------------------------------------------------
// C ABI (include/rtldavis_hip.h)
// ------------------------------------------------------------------------------------------

static uint16_t f16_rn(double v) {  // round to nearest even f16 (|v| < 65504)
    const _Float16 h = (_Float16)v;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}
static double f16_val(uint16_t b) {
    _Float16 h;
    memcpy(&h, &b, 2);
    return (double)h;
}

// LDS bytes of a workgroup's staged window (a multiple of 16, one spare vector)
static size_t chan_lds_bytes(int fmt, int decim, int t_pad) {
    const size_t span = (size_t)(RD_CHAN_TT - 1) * decim + t_pad + rd_fmt_kc(fmt);
    return (rd_fmt_lds_bps(fmt) * span + 15 + 16) & ~(size_t)15;
}

// The tables of channel c for the shift `shift_hz` (Hz, as given) and the phase accumulator `phase` (header: RETUNE; 0 at
// create): its two rows of the A operand, its DC entries and 32-output rotation, shifts[c].  On the host - rd_chan_create_fmt
// for every channel, rd_chan_retune for a channel retuned before the device tables exist; k_chan_retune is the same on
// the device.
static void chan_build_channel(rd_chan *h, int c, int64_t shift_hz, int64_t phase) {
    const rd_chan_config *cfg = &h->cfg;
    const int fmt = h->fmt, T = cfg->n_taps, t_pad = h->t_pad, kc = rd_fmt_kc(fmt), n_q = t_pad / kc + 1;
    const double *taps = h->taps.data();
    const double tap_scale = h->tap_scale;
    const double wide_rate = (double)cfg->out_rate * cfg->decim;
    const double dc_level = fmt == RD_IQ_U8 ? 127.4 : fmt == RD_IQ_S8 ? 128.0 : 0.0;
    h->shift_hz[c] = shift_hz;
    h->phase[c] = phase;
    h->shifts[c] = ((shift_hz % cfg->out_rate) + cfg->out_rate) % cfg->out_rate;  // shift mod Fo in [0, Fo): all the output phasor needs
    std::vector<double> gr(t_pad), gi(t_pad);
    for (int k = 0; k < t_pad; k++) {
        gr[k] = gi[k] = 0.0;
        if (k >= T) continue;
        // g_c[k] = h[k] e^{+j 2 pi shift k / Fw}; the phase through an exact integer remainder
        const __int128 prod = (__int128)shift_hz * k;
        const long fw = (long)cfg->out_rate * cfg->decim;
        long r = (long)(prod % fw);
        if (r < 0) r += fw;
        const double ph = 2.0 * M_PI * ((double)r / wide_rate);
        gr[k] = (double)(float)(taps[k] * cos(ph));  // the fp32 taps are the definition's taps on the device
        gi[k] = (double)(float)(taps[k] * sin(ph));
    }
    // DC term: output t sees taps k <= D t (zero history before)
    double sr = 0.0, si = 0.0;
    int kdone = 0;
    for (int t = 0; t <= RD_CHAN_EARLY; t++) {
        // (RD_IQ_S8 stages 0x80 = the value 0 before the capture: every output sees all the taps)
        const long kmax = t < RD_CHAN_EARLY && fmt == RD_IQ_U8 ? (long)cfg->decim * t : (long)t_pad - 1;
        for (; kdone < t_pad && kdone <= kmax; kdone++) { sr += gr[kdone]; si += gi[kdone]; }
        // lut(b) = (b - 127.4) / 127.6 and the kernel sums g b: the constant is -127.4 (1 + j)(sr + j si)
        // (128 for the offset-binary bytes of RD_IQ_S8, nothing for RD_IQ_S16)
        h->h_dc[((size_t)c * RD_CHAN_DCN + t) * 2] = (float)(-dc_level * (sr - si));
        h->h_dc[((size_t)c * RD_CHAN_DCN + t) * 2 + 1] = (float)(-dc_level * (sr + si));
    }
    {   // the rotation that takes the output phasor 32 output times on (exact remainder, float64 sin / cos)
        const long inc = (long)(((__int128)h->shifts[c] * 32) % cfg->out_rate);
        const double ph = -2.0 * M_PI * ((double)inc / (double)cfg->out_rate);
        h->h_dc[((size_t)c * RD_CHAN_DCN + RD_CHAN_EARLY + 1) * 2] = (float)cos(ph);
        h->h_dc[((size_t)c * RD_CHAN_DCN + RD_CHAN_EARLY + 1) * 2 + 1] = (float)sin(ph);
    }
    // rows 2c (re) and 2c+1 (im); kappa = 2 i + comp, window sample i = t_pad - 1 - k
    const int grp = c / (16 * RD_CHAN_RBG), rb = (c / 16) % RD_CHAN_RBG, r0 = 2 * (c % 16);
    // RD_IQ_S16: kappa = 4 i + 2 comp + digit, a lane holds two samples (Ilo Ihi Qlo Qhi each); the low digit's taps
    // are scaled by 2^-8 against the high digit's.  RD_IQ_CF32: the same layout, both digits against the same tap
    const int per_lane = kc / 2, n_dig = rd_fmt_digits(fmt) ? 2 : 1;
    for (int i = 0; i < kc * n_q; i++) {   // window sample i of a column <-> tap k = t_pad - i (the window starts at D t - t_pad)
        const int k = t_pad - i;
        if (k < 0 || k >= t_pad) continue;  // (zero taps: the entries stay 0)
        const int q = i / kc, hh = (i % kc) / per_lane, sl = i % per_lane;  // K step, lane half, sample within the lane's
        for (int part = 0; part < 2; part++)
            for (int comp = 0; comp < 2; comp++)
                for (int dig = 0; dig < n_dig; dig++) {
                    const double a = part == 0 ? (comp == 0 ? gr[k] : -gi[k]) : (comp == 0 ? gi[k] : gr[k]);
                    const double as = a * tap_scale * (fmt == RD_IQ_S16 && dig == 0 ? 1.0 / 256.0 : 1.0);
                    const uint16_t hi = f16_rn(as), lo = f16_rn(as - f16_val(hi));
                    const uint16_t term[RD_CHAN_TERMS] = {hi, lo};
                    const int lane = 32 * hh + r0 + part;
                    // element position inside the fragment, see the kernel's B fragments:
                    // (I0 I1 Q0 Q1 | I2 I3 Q2 Q3), or (Ilo Ihi Qlo Qhi | the same of the second sample)
                    const int el = rd_fmt_digits(fmt) ? 4 * sl + 2 * comp + dig : 4 * (sl / 2) + 2 * comp + (sl % 2);
                    for (int tm = 0; tm < RD_CHAN_TERMS; tm++) {
                        const size_t at = (((((size_t)grp * n_q + q) * RD_CHAN_TERMS + tm) * RD_CHAN_RBG + rb) * 64 + lane) * 8 + el;
                        h->h_amat[at] = term[tm];
                    }
                }
    }
}

extern "C" int rd_chan_create(const rd_chan_config *cfg, const double *taps, const int64_t *shift_hz, rd_chan **out) {
    return rd_chan_create_fmt(cfg, RD_IQ_U8, taps, shift_hz, out);
}

extern "C" int rd_chan_create_fmt(const rd_chan_config *cfg, int fmt, const double *taps, const int64_t *shift_hz,
                                  rd_chan **out) {
    if (!cfg || !taps || !shift_hz || !out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (fmt != RD_IQ_U8 && fmt != RD_IQ_S8 && fmt != RD_IQ_S16 && fmt != RD_IQ_CF32) return rd_fail_msg(RD_ERR_ARG, "unknown sample format %d", fmt);
    if (cfg->decim < 4 || cfg->decim > 4096 || cfg->decim % 4 || cfg->n_taps < 1 || cfg->n_taps > 8192 ||
        cfg->n_channels < 1 || cfg->n_channels > 4096 || cfg->out_rate < 1 || cfg->out_rate >= (1 << 26) ||
        !(cfg->gain > 0.0))
        return rd_fail_msg(RD_ERR_ARG, "channelizer config out of range (decim: a multiple of 4)");
    const int t_pad = (cfg->n_taps + RD_CHAN_KC - 1) / RD_CHAN_KC * RD_CHAN_KC;
    const int kc = rd_fmt_kc(fmt);
    const size_t span = (size_t)(RD_CHAN_TT - 1) * cfg->decim + t_pad + kc;
    if (rd_fmt_lds_bps(fmt) * span + 16 > 160 * 1024)
        return rd_fail_msg(RD_ERR_ARG, "decim x 127 + n_taps samples of %d bytes do not fit the 160 KiB LDS", rd_fmt_lds_bps(fmt));
    // (RD_IQ_S16 and RD_IQ_CF32 have no DC term, hence no table of early ones and no limit from it)
    const int n_early = rd_fmt_digits(fmt) ? 0 : (t_pad - 1 + cfg->decim - 1) / cfg->decim;
    if (n_early > RD_CHAN_EARLY) return rd_fail_msg(RD_ERR_ARG, "n_taps / decim too large");
    rd_chan *h = new rd_chan();
    h->cfg = *cfg;
    h->fmt = fmt;
    const int T = cfg->n_taps;
    h->t_pad = t_pad;
    h->n_early = n_early;
    h->n_groups = (cfg->n_channels + 16 * RD_CHAN_RBG - 1) / (16 * RD_CHAN_RBG);
    const int n_q = t_pad / kc + 1;  // the window starts one sample early (aligned): one more K step
    h->h_amat.assign((size_t)h->n_groups * n_q * (RD_CHAN_Q_BYTES / 2), 0);
    h->h_dc.assign((size_t)cfg->n_channels * RD_CHAN_DCN * 2, 0.0f);
    h->shifts.resize(cfg->n_channels);
    h->shift_hz.resize(cfg->n_channels);
    h->phase.resize(cfg->n_channels);
    h->gains.assign(cfg->n_channels, (float)cfg->gain);
    h->taps.assign(taps, taps + T);
    // every |g_c[k]| <= max |h[k]|: scale the taps by the power of two that brings that just below 2^15 (f16: 11
    // significant bits from 2^-14 up), the kernel multiplies the sums back
    double hmax = 0.0;
    for (int k = 0; k < T; k++) hmax = std::max(hmax, std::fabs(taps[k]));
    int sexp = 0;
    if (hmax > 0.0) sexp = 14 - (int)std::ceil(std::log2(hmax));
    if (sexp > 60) sexp = 60;
    if (sexp < -60) sexp = -60;
    h->tap_scale = std::ldexp(1.0, sexp);
    // (+24: the samples enter as k 2^-24; RD_IQ_S16: the low digit's taps carry 2^-8 more, so that the high digit's
    // factor 256 stays inside f16; RD_IQ_CF32: the samples enter as 2^12 x, real f16 values, not raw patterns)
    h->tap_unscale = fmt == RD_IQ_CF32 ? (float)std::ldexp(1.0, -sexp - RD_CF32_PRESCALE_LOG2)
                                       : (float)std::ldexp(1.0, -sexp + 24 + (fmt == RD_IQ_S16 ? 8 : 0));
    for (int c = 0; c < cfg->n_channels; c++) chan_build_channel(h, c, shift_hz[c], 0);
    *out = h;
    return RD_OK;
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
    const size_t lds = chan_lds_bytes(h->fmt, D, T);
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
    const size_t lds = chan_lds_bytes(h->fmt, h->cfg.decim, h->t_pad);
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
    const size_t lds = chan_lds_bytes(h->fmt, h->cfg.decim, h->t_pad);
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
        for (int i = 0; i < n; i++) chan_build_channel(h, (int)rec[3 * i], rec[3 * i + 1], rec[3 * i + 2]);
        return RD_OK;
    }
    if (!h->d_taps) return rd_fail_msg(RD_ERR_STATE, "rd_chan_stream_prepare first");
    int64_t *stage = h->h_rt + (size_t)slot * n_ch * 4;
    for (int i = 0; i < n; i++) {
        stage[4 * i] = rec[3 * i]; stage[4 * i + 1] = rec[3 * i + 1]; stage[4 * i + 2] = ((rec[3 * i + 1] % fo) + fo) % fo;
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

// GAIN: n = n_channels gains, every one finite and > 0 (the rule of cfg.gain), as the float32 values the table takes
static int chan_check_gains(const rd_chan *h, const double *gain, int n) {
    if (!h || !gain) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (n != h->cfg.n_channels) return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: %d gains for %d channels", n, h->cfg.n_channels);
    for (int c = 0; c < n; c++)
        if (!(gain[c] > 0.0) || !std::isfinite(gain[c]) || !((float)gain[c] > 0.0f) || !std::isfinite((float)gain[c]))
            return rd_fail_msg(RD_ERR_ARG, "channel %d: a gain must be finite and > 0 (in float32 too)", c);
    return RD_OK;
}
int rd_chan_check_gains(const rd_chan *h, const double *gain, int n) { return chan_check_gains(h, gain, n); }

// One-shot form: the gains of the runs that follow.  A quiet handle: the caller has waited for the streams its earlier
// rd_chan_run calls were queued on (the copy below is not ordered against them).
extern "C" int rd_chan_set_gain(rd_chan *h, const double *gain, int n) {
    int rc = chan_check_gains(h, gain, n);
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

// LEVELS: one launch behind a streamed chunk's k_channelize on st.  out / in: device addresses of mapped host memory
// (the caller's pinned slot of the chunk's parity); acc: RD_LV_ACC_WORDS words of device memory, zero between launches.
int rd_chan_stream_levels(rd_chan *h, const uint8_t *wide, size_t n_out, const uint8_t *chan_out, size_t out_stride,
                          uint64_t seq, rd_chan_level *out, rd_input_level *in, uint32_t *acc, hipStream_t st) {
    if (!h || !wide || !chan_out || !out || !in || !acc) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (!h->dev_ready) return rd_fail_msg(RD_ERR_STATE, "rd_chan_stream_prepare first");
    if (n_out == 0 || n_out % RD_CHAN_TT || out_stride < 2 * n_out || (out_stride & 15))
        return rd_fail_msg(RD_ERR_ARG, "levels: a chunk of %zu outputs, stride %zu", n_out, out_stride);
    const int n_ch = h->cfg.n_channels;
    // 16-byte vectors: 2 n_out bytes per channel (n_out % 128 == 0), n_out decim IQ pairs of the capture (decim % 4 == 0)
    const size_t ch_vec = 2 * n_out / 16, in_vec = (size_t)rd_fmt_in_bps(h->fmt) * n_out * (size_t)h->cfg.decim / 16;
    const unsigned n_in = (unsigned)std::min<size_t>(RD_LV_MAX_SLICES, (in_vec + RD_LV_THREADS * 8 - 1) / (RD_LV_THREADS * 8));
    hipLaunchKernelGGL(k_chan_levels, dim3((unsigned)n_ch + n_in), dim3(RD_LV_THREADS), 0, st, (const uint4 *)chan_out,
                       out_stride / 16, ch_vec, n_ch, (const float *)h->d_gains, (const uint4 *)wide, in_vec, h->fmt, n_in,
                       seq, out, in, acc);
    HIPCHK(hipGetLastError());
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
int64_t rd_chan_out_rate(const rd_chan *h) { return h ? h->cfg.out_rate : 0; }
int64_t rd_chan_wide_rate(const rd_chan *h) { return h ? (int64_t)h->cfg.out_rate * h->cfg.decim : 0; }
int rd_chan_bytes_per_sample(const rd_chan *h) { return h ? rd_fmt_in_bps(h->fmt) : 0; }
