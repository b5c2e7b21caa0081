// rd_chan_levels.hip - LEVELS (k_chan_levels, streaming form): what the gains leave of the byte range, per channel and
// chunk, and how hard the capture drives the ADC - exact integers for a gain control on the host (rtldavis_amd/agc.py).
// The sample formats and adm: rd_channelizer.hip's head.
//
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
#include <algorithm>

#include <hip/hip_runtime.h>

#include "rd_chan_tables.h"
#include "rd_internal.h"

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
// float32 components in int16 units (rd_channelizer.hip: RD_IQ_CF32): k = clip(rint(2^15 adm(v)), -32768, 32767), the product exact
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

// LEVELS: one launch behind a streamed chunk's k_channelize on st.  out / in: device addresses of mapped host memory
// (the caller's pinned slot of the chunk's parity); acc: RD_LV_ACC_WORDS words of device memory, zero between launches.
int rd_chan_stream_levels(rd_chan *h, const uint8_t *wide, size_t n_out, const uint8_t *chan_out, size_t out_stride,
                          uint64_t seq, rd_chan_level *out, rd_input_level *in, uint32_t *acc, hipStream_t st) {
    if (!h || !wide || !chan_out || !out || !in || !acc) return rd_fail_msg(RD_ERR_ARG, "null argument");
    const float *gains = rd_chan_device_gains(h);
    if (!gains) return rd_fail_msg(RD_ERR_STATE, "rd_chan_stream_prepare first");
    if (n_out == 0 || n_out % RD_CHAN_TT || out_stride < 2 * n_out || (out_stride & 15))
        return rd_fail_msg(RD_ERR_ARG, "levels: a chunk of %zu outputs, stride %zu", n_out, out_stride);
    const int n_ch = rd_chan_n_channels(h), fmt = rd_chan_format(h);
    // 16-byte vectors: 2 n_out bytes per channel (n_out % 128 == 0), n_out decim IQ pairs of the capture (decim % 4 == 0)
    const size_t ch_vec = 2 * n_out / 16, in_vec = (size_t)rd_fmt_in_bps(fmt) * n_out * (size_t)rd_chan_decim(h) / 16;
    const unsigned n_in = (unsigned)std::min<size_t>(RD_LV_MAX_SLICES, (in_vec + RD_LV_THREADS * 8 - 1) / (RD_LV_THREADS * 8));
    hipLaunchKernelGGL(k_chan_levels, dim3((unsigned)n_ch + n_in), dim3(RD_LV_THREADS), 0, st, (const uint4 *)chan_out,
                       out_stride / 16, ch_vec, n_ch, gains, (const uint4 *)wide, in_vec, fmt, n_in,
                       seq, out, in, acc);
    HIPCHK(hipGetLastError());
    return RD_OK;
}
