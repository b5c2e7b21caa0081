// rd_spectrum.hip - power spectrum of a wideband capture on the device (include/rtldavis_hip.h, SPECTRUM): Welch's method
// without overlap over the S = L / N whole segments of N samples a chunk (or an uploaded capture) of L IQ pairs holds,
// periodic Hann window, N a power of two in 64 .. 4096.  Used by rd_wideband.hip per streamed chunk (rd_wb_set_spectrum)
// and by rd_chan_spectrum on an uploaded capture: the same kernel and launch helper, so the two agree bit for bit.
//
//   x[n]    the capture's samples as complex float32, the channelizer's meaning of each format (below)
//   X_s[k]  = sum_n w[n] x[s N + n] e^{-2 pi i k n / N},  w[n] = 0.5 - 0.5 cos(2 pi n / N)
//   P[j]    = 1 / (S (N/2)^2) sum_s |X_s[(j + N/2) mod N]|^2          ascending frequency; (N/2)^2 = (sum w)^2
// Per-segment arithmetic is float32, the sum over segments and the scaling float64.
//
// Sample values.  uint8: (k - 127.4) / 127.6 = (10 k - 1274) / 1276 - the numerator an exact integer, one float32
// product with f32(1 / 1276): a RELATIVE error of 1.5 ulp (k - 127.4f would leave an absolute one that swamps a weak
// signal).  int8: k / 128, int16: k / 32768, both exact.  float32: adm(v) (rd_internal.h: rd_chan_adm).
//
// Kernel.  One workgroup of 256 threads handles one segment at a time, all of it in LDS:
//   load     16-byte vectors of the segment (8, 4 or 2 samples), convert, multiply with the window (a float32 table the
//            host rounds once from float64) and store at the BIT-REVERSED index
//   FFT      in-place radix-2 decimation in time, two stages fused per pass (a thread takes the four elements b + {0, h,
//            2h, 3h}, b = 4h (q / h) + q mod h, through stage h and stage 2h in registers: radix-2 arithmetic, half the
//            barriers); an odd log2 N starts with the lone stage h = 1.  Twiddles come from a float32 table laid out per
//            stage - entry h + j = e^{-2 pi i j / 2h}, j < h - so the lanes of a pass read consecutive entries; it is
//            copied into LDS once per workgroup.  No sine or cosine is evaluated on the device.
//   |X|^2    float32 per bin, added to the thread's float64 sums: thread t owns bins t, t + 256, ... (at most 16), read
//            from index j ^ N/2 - the shift to ascending frequency costs nothing
// LDS: element i lives at i + (i >> 5) (one complex of padding per 32, 33 KiB at N = 4096) beside the 32 KiB of twiddles:
// by the bank rule the passes h >= 64 and h = 1 are conflict-free (8-byte reads), h = 16 and h = 2 are 2-way, h = 4 and
// h = 8 remain 4-way on the unpadded stride of 16 or 32 elements - one pass in six at N = 4096 (not measured; derived).
// Determinism: G = min(S, RD_SP_MAX_GROUPS) workgroups, a function of the shape alone; workgroup g takes segments g, g +
// G, ... in ascending order and writes its N sums to part[g][N]; the workgroup that draws the last ticket adds the
// partials in ascending g, scales and writes the N doubles and the header with plain vector stores, and leaves the
// ticket word zero.  No floating-point atomics: the same input gives the same bits on every run.
// Cost: 5 N log2 N flop per segment, 45 MFLOP for the default chunk (819200 samples) at N = 2048, and one more read of
// the chunk the channelizer has just read.
#include <cmath>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "rd_internal.h"


#define RD_SP_THREADS 256
#define RD_SP_MAX_BINS 4096
#define RD_SP_MIN_BINS 64
#define RD_SP_PER (RD_SP_MAX_BINS / RD_SP_THREADS)   // bins a thread owns at most

__host__ __device__ constexpr int rd_sp_pad(int i) { return i + (i >> 5); }
// LDS bytes: the padded segment, the twiddles, one word for the ticket's verdict (every part a multiple of 16)
static size_t sp_lds_bytes(int n) { return (size_t)rd_sp_pad(n) * 8 + (size_t)n * 8 + 16; }

__device__ __forceinline__ float2 sp_mul(float2 w, float2 a) { return float2{w.x * a.x - w.y * a.y, w.x * a.y + w.y * a.x}; }
__device__ __forceinline__ float2 sp_add(float2 a, float2 b) { return float2{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ float2 sp_sub(float2 a, float2 b) { return float2{a.x - b.x, a.y - b.y}; }

// sample e of a 16-byte vector of the capture -> complex float32
template <int FMT>
__device__ __forceinline__ float2 sp_sample(const uint4 &v, int e) {
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
    if constexpr (FMT == RD_IQ_CF32) {
        return float2{rd_chan_adm(d[2 * e]), rd_chan_adm(d[2 * e + 1])};
    } else if constexpr (FMT == RD_IQ_S16) {
        const uint32_t w = d[e];
        return float2{(float)(int)(int16_t)(w & 0xFFFFu) * (1.0f / 32768.0f), (float)((int)w >> 16) * (1.0f / 32768.0f)};
    } else {
        const uint32_t w = d[e >> 1] >> (16 * (e & 1));
        if constexpr (FMT == RD_IQ_S8)
            return float2{(float)(int)(int8_t)(w & 0xFFu) * (1.0f / 128.0f), (float)(int)(int8_t)((w >> 8) & 0xFFu) * (1.0f / 128.0f)};
        const int ai = 10 * (int)(w & 0xFFu) - 1274, aq = 10 * (int)((w >> 8) & 0xFFu) - 1274;
        return float2{(float)ai * (1.0f / 1276.0f), (float)aq * (1.0f / 1276.0f)};
    }
}

template <int FMT>
__global__ __launch_bounds__(RD_SP_THREADS) void k_chan_spectrum(const uint8_t *__restrict__ wide, int n, int log2n,
                                                                 unsigned n_seg, const float *__restrict__ win,
                                                                 const float2 *__restrict__ tw, double *part, uint32_t *ticket,
                                                                 double scale, uint64_t seq, uint8_t *out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t sp_lds[];
    float2 *xs = (float2 *)sp_lds;                          // the segment, element i at rd_sp_pad(i)
    float2 *tws = xs + rd_sp_pad(n);                        // twiddles, entry h + j = e^{-2 pi i j / 2h}
    uint32_t *verdict = (uint32_t *)(tws + n);
    constexpr int IB = FMT == RD_IQ_CF32 ? 8 : FMT == RD_IQ_S16 ? 4 : 2, VS = 16 / IB;
    const int tid = (int)threadIdx.x;
    const unsigned n_grp = gridDim.x;
    for (int i = tid; i < n; i += RD_SP_THREADS) tws[i] = tw[i];
    double acc[RD_SP_PER];
#pragma unroll
    for (int i = 0; i < RD_SP_PER; i++) acc[i] = 0.0;
    const int n_vec = n / VS;
    for (unsigned seg = blockIdx.x; seg < n_seg; seg += n_grp) {
        const uint8_t *src = wide + (size_t)seg * (size_t)n * IB;
        for (int q = tid; q < n_vec; q += RD_SP_THREADS) {
            const uint4 v = *(const uint4 *)(src + 16 * (size_t)q);
#pragma unroll
            for (int e = 0; e < VS; e++) {
                const int nn = VS * q + e;
                const float2 x = sp_sample<FMT>(v, e);
                const float w = win[nn];
                xs[rd_sp_pad((int)(__brev((unsigned)nn) >> (32 - log2n)))] = float2{x.x * w, x.y * w};
            }
        }
        __syncthreads();
        int h = 1;
        if (log2n & 1) {                                    // the lone stage h = 1: its twiddle is 1
            for (int q = tid; q < n / 2; q += RD_SP_THREADS) {
                const int i0 = rd_sp_pad(2 * q), i1 = rd_sp_pad(2 * q + 1);
                const float2 a = xs[i0], b = xs[i1];
                xs[i0] = sp_add(a, b);
                xs[i1] = sp_sub(a, b);
            }
            __syncthreads();
            h = 2;
        }
        for (; h < n; h <<= 2) {                            // stages h and 2h
            for (int q = tid; q < n / 4; q += RD_SP_THREADS) {
                const int j = q & (h - 1), b = ((q - j) << 2) + j;
                const int i0 = rd_sp_pad(b), i1 = rd_sp_pad(b + h), i2 = rd_sp_pad(b + 2 * h), i3 = rd_sp_pad(b + 3 * h);
                const float2 w1 = tws[h + j], w2 = tws[2 * h + j], w3 = tws[3 * h + j];
                const float2 a0 = xs[i0], a1 = xs[i1], a2 = xs[i2], a3 = xs[i3];
                const float2 t1 = sp_mul(w1, a1), t3 = sp_mul(w1, a3);
                const float2 b0 = sp_add(a0, t1), b1 = sp_sub(a0, t1), b2 = sp_add(a2, t3), b3 = sp_sub(a2, t3);
                const float2 u2 = sp_mul(w2, b2), u3 = sp_mul(w3, b3);
                xs[i0] = sp_add(b0, u2);
                xs[i2] = sp_sub(b0, u2);
                xs[i1] = sp_add(b1, u3);
                xs[i3] = sp_sub(b1, u3);
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < RD_SP_PER; i++) {
            const int j = tid + RD_SP_THREADS * i;
            if (j < n) {
                const float2 v = xs[rd_sp_pad(j ^ (n >> 1))];
                acc[i] += (double)(v.x * v.x + v.y * v.y);
            }
        }
        __syncthreads();                                    // the next segment overwrites xs
    }
    double *mine = part + (size_t)blockIdx.x * (size_t)n;
#pragma unroll
    for (int i = 0; i < RD_SP_PER; i++) {
        const int j = tid + RD_SP_THREADS * i;
        if (j < n) mine[j] = acc[i];
    }
    // Hand the partial sums to the workgroup that draws the last ticket: every storing wave waits for its stores, one
    // lane releases at agent scope (the XCDs' L2s are not coherent with each other) and draws; the last workgroup
    // acquires - each wave for its own loads - and reads every partial with plain vector loads.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        *verdict = atomicAdd(ticket, 1u) == n_grp - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (*verdict == 0u) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double *p = (double *)(out + RD_SPEC_HDR_BYTES);
#pragma unroll
    for (int i = 0; i < RD_SP_PER; i++) {
        const int j = tid + RD_SP_THREADS * i;
        if (j < n) {
            double s = 0.0;
            for (unsigned g = 0; g < n_grp; g++) s += part[(size_t)g * (size_t)n + j];
            p[j] = s * scale;
        }
    }
    if (tid == 0) {
        atomicExch(ticket, 0u);                             // clear for the next launch
        *(uint64_t *)out = seq;
        *(uint32_t *)(out + 8) = n_seg;
        *(uint32_t *)(out + 12) = (uint32_t)n;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct rd_spec {
    int n = 0, log2n = 0;
    unsigned groups = 0;           // partial rows allocated
    float *d_win = nullptr;
    float2 *d_tw = nullptr;
    double *d_part = nullptr;
    uint32_t *d_ticket = nullptr;
};

static const void *sp_kernel(int fmt) {
    switch (fmt) {
    case RD_IQ_S8: return (const void *)k_chan_spectrum<RD_IQ_S8>;
    case RD_IQ_S16: return (const void *)k_chan_spectrum<RD_IQ_S16>;
    case RD_IQ_CF32: return (const void *)k_chan_spectrum<RD_IQ_CF32>;
    default: return (const void *)k_chan_spectrum<RD_IQ_U8>;
    }
}

int rd_spec_check(int n_bins, size_t n_samples) {
    if (n_bins < RD_SP_MIN_BINS || n_bins > RD_SP_MAX_BINS || (n_bins & (n_bins - 1)))
        return rd_fail_msg(RD_ERR_ARG, "n_bins %d is not a power of two in %d .. %d", n_bins, RD_SP_MIN_BINS, RD_SP_MAX_BINS);
    if ((size_t)n_bins > n_samples)
        return rd_fail_msg(RD_ERR_ARG, "n_bins %d exceeds the %zu samples there are", n_bins, n_samples);
    return RD_OK;
}

static unsigned sp_groups(int n_bins, size_t n_samples) {
    const size_t s = n_samples / (size_t)n_bins;
    return (unsigned)(s < RD_SP_MAX_GROUPS ? s : RD_SP_MAX_GROUPS);
}

void rd_spec_destroy(rd_spec *sp) {
    if (!sp) return;
    if (rd_owns_device_state()) {   // (device memory belongs to the process that allocated it)
        hipFree(sp->d_win); hipFree(sp->d_tw); hipFree(sp->d_part); hipFree(sp->d_ticket);
    }
    delete sp;
}

int rd_spec_prepare(rd_spec **spp, int n_bins, size_t n_samples, hipStream_t st) {
    if (!spp) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = rd_spec_check(n_bins, n_samples);
    if (rc) return rc;
    const unsigned groups = sp_groups(n_bins, n_samples);
    if (*spp && (*spp)->n == n_bins && (*spp)->groups >= groups) return RD_OK;
    rd_spec_destroy(*spp);
    *spp = nullptr;
    rd_spec *sp = new rd_spec();
    sp->n = n_bins;
    while ((1 << sp->log2n) < n_bins) sp->log2n++;
    sp->groups = groups;
    const int n = n_bins;
    // both tables in float64, rounded once; the argument is reduced exactly (integers) before it meets pi
    std::vector<float> win(n);
    std::vector<float> tw(2 * (size_t)n, 0.0f);
    for (int i = 0; i < n; i++) win[i] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)i / (double)n));
    tw[0] = 1.0f;                                           // (entry 0 is never read)
    for (int h = 1; h < n; h <<= 1)
        for (int j = 0; j < h; j++) {
            const double ph = -2.0 * M_PI * (double)j / (double)(2 * h);
            tw[2 * (size_t)(h + j)] = (float)cos(ph);
            tw[2 * (size_t)(h + j) + 1] = (float)sin(ph);
        }
    hipError_t e = hipMalloc(&sp->d_win, n * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&sp->d_tw, n * sizeof(float2));
    if (e == hipSuccess) e = hipMalloc(&sp->d_part, (size_t)groups * n * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&sp->d_ticket, 16);
    if (e == hipSuccess) e = hipMemcpyAsync(sp->d_win, win.data(), n * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(sp->d_tw, tw.data(), n * sizeof(float2), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(sp->d_ticket, 0, 16, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);      // (the tables above are this call's own vectors)
    for (int fmt : {RD_IQ_U8, RD_IQ_S8, RD_IQ_S16, RD_IQ_CF32})
        if (e == hipSuccess)
            e = hipFuncSetAttribute(sp_kernel(fmt), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp_lds_bytes(RD_SP_MAX_BINS));
    if (e != hipSuccess) {
        rd_spec_destroy(sp);
        return rd_fail_msg(RD_ERR_DEVICE, "spectrum tables: %s", hipGetErrorString(e));
    }
    *spp = sp;
    return RD_OK;
}

int rd_spec_launch(rd_spec *sp, const uint8_t *wide, int fmt, size_t n_samples, uint64_t seq, void *out, hipStream_t st) {
    if (!sp || !wide || !out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (fmt != RD_IQ_U8 && fmt != RD_IQ_S8 && fmt != RD_IQ_S16 && fmt != RD_IQ_CF32)
        return rd_fail_msg(RD_ERR_ARG, "unknown sample format %d", fmt);
    int rc = rd_spec_check(sp->n, n_samples);
    if (rc) return rc;
    const size_t n_seg = n_samples / (size_t)sp->n;
    const unsigned groups = sp_groups(sp->n, n_samples);
    if (groups > sp->groups || n_seg > 0xFFFFFFFFull || ((uintptr_t)wide & 15) || ((uintptr_t)out & 15))
        return rd_fail_msg(RD_ERR_ARG, "spectrum: %zu segments need %u workgroups of %u prepared, or a misaligned buffer", n_seg, groups, sp->groups);
    int n = sp->n, log2n = sp->log2n;
    unsigned segs = (unsigned)n_seg;
    const float *win = sp->d_win;
    const float2 *tw = sp->d_tw;
    double *part = sp->d_part;
    uint32_t *ticket = sp->d_ticket;
    double scale = 1.0 / ((double)n_seg * (double)(n / 2) * (double)(n / 2));
    uint8_t *o = (uint8_t *)out;
    void *args[] = {&wide, &n, &log2n, &segs, &win, &tw, &part, &ticket, &scale, &seq, &o};   // k_chan_spectrum's parameters, in order
    HIPCHK(hipLaunchKernel(sp_kernel(fmt), dim3(groups), dim3(RD_SP_THREADS), args, sp_lds_bytes(n), st));
    HIPCHK(hipGetLastError());
    return RD_OK;
}
