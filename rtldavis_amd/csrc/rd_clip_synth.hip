// rd_clip_synth.hip - synthesise noisy burst clips into the pool of CLIP DECODE (include/rtldavis_hip.h, CLIP SYNTH).
// The clip decoder runs ten to twenty million jobs per second; the clips it was given were made one by one in NumPy and
// pushed over the link.  k_clip_synth writes them where the decoder reads them, from one spec of 80 bytes per clip, in
// exact integers: tests/clip_synth_cases.py is its model, byte for byte.
//
// Kernel.  One workgroup of 256 threads per spec, grid = the number of specs.  The spec is read from device memory at a
// workgroup-uniform address and its bounds are checked again (the rules of rd_cs_check_specs that concern one spec):
// a spec that fails writes nothing.  LDS: the cosine table (8 KiB, copied from device memory; skipped for amp_q = 0) and
// cum[k] = the sum of the +-1 of symbols 0 .. k - 1, k <= 192, by popcounts of the spec's bits - so D(u) of an output in
// symbol k, r outputs into it, is SL cum[k] + (r + 1) (cum[k + 1] - cum[k]).  k = floor(v / SL) is one high multiply by
// inv = floor(2^32 / SL) + 1: exact while v (inv SL - 2^32) < 2^32, and v < 192 x 51, inv SL - 2^32 <= SL <= 51.
// A lane produces the 8 outputs of a vector - 16 Philox4x32-10 calls, each 32 x 32 -> 64 multiplies -, packs their 16
// bytes and stores them as one aligned uint4: a clip begins at a multiple of 8 outputs of a 16-byte aligned pool.  The
// outputs of the last vector past n are written as 0; the pool's device copy is padded to whole vectors.  Every byte is a
// function of the spec and t alone and every vector has one writer (the specs do not overlap: rd_cs_check_specs), so the
// order in which the workgroups arrive changes nothing.  The bytes that belong to no clip are zeroed by the
// hipMemsetAsync in front of the launch.  Plain vector stores, no atomics.
#include <vector>

#include <hip/hip_runtime.h>

#include "rd_burst_common.h"
#include "rd_clips.h"

static_assert(sizeof(rd_clip_spec) == 80, "the layout of CLIP SYNTH");
static_assert(RD_CS_MAX_SYM + 1 <= RD_BURST_THREADS && RD_CS_MAX_SYM == 8 * sizeof(((rd_clip_spec *)0)->bits), "one thread per prefix sum");
static_assert(RD_CS_TABLE * sizeof(int16_t) == 2 * 16 * RD_BURST_THREADS, "two vectors of the table per thread");

struct rd_cs_params {
    int sl;                    // SL
    uint32_t inv_sl;           // floor(2^32 / SL) + 1 (SL >= 2)
    uint64_t pool_outputs;     // outputs the pool holds
};

// Philox4x32-10 of the counter (c0, c1, 0, 0) under the key (k0, k1): the sum of the 16 bytes of its four words
__device__ __forceinline__ int rd_cs_noise(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1) {
    uint32_t c2 = 0u, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * (uint64_t)c0, p1 = (uint64_t)0xCD9E8D57u * (uint64_t)c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    // the four words' even and odd bytes in 16-bit halves (at most 4 x 255 each), then the halves
    const uint32_t ev = (c0 & 0x00FF00FFu) + (c1 & 0x00FF00FFu) + (c2 & 0x00FF00FFu) + (c3 & 0x00FF00FFu);
    const uint32_t od = ((c0 >> 8) & 0x00FF00FFu) + ((c1 >> 8) & 0x00FF00FFu) + ((c2 >> 8) & 0x00FF00FFu) + ((c3 >> 8) & 0x00FF00FFu);
    const uint32_t sum = ev + od;
    return (int)((sum & 0xFFFFu) + (sum >> 16));
}

__device__ __forceinline__ uint32_t rd_cs_byte(int64_t S) {
    const int64_t b = (S + (1ll << 21)) >> 22;
    return (uint32_t)(b < 0 ? 0 : (b > 255 ? 255 : b));
}

__global__ __launch_bounds__(RD_BURST_THREADS) void k_clip_synth(uint8_t *pool, rd_cs_params P, const rd_clip_spec *__restrict__ specs,
                                                                 const int16_t *__restrict__ tab) {
    __shared__ uint4 s_tab[RD_CS_TABLE * sizeof(int16_t) / 16];
    __shared__ int s_cum[RD_CS_MAX_SYM + 1];
    const unsigned tid = threadIdx.x;
    const rd_clip_spec J = specs[blockIdx.x];            // (a workgroup-uniform address: every thread gets the same spec)
    const bool ok = (J.offset & 7ull) == 0ull && J.n >= 1u && J.n <= (uint32_t)RD_CS_MAX_N && J.offset <= P.pool_outputs &&
                    (uint64_t)J.n <= P.pool_outputs - J.offset && J.n_sym <= (uint32_t)RD_CS_MAX_SYM && J.pre <= RD_CS_MAX_PRE &&
                    J.post <= RD_CS_MAX_PRE && J.amp_q <= RD_CS_MAX_AMP && J.noise_q <= RD_CS_MAX_NOISE && J.f_d < 0x80000000u &&
                    J.at >= -RD_CS_MAX_AT && J.at <= RD_CS_MAX_AT && J.pad == 0u;
    if (!ok) return;                                     // (uniform)
    const bool signal = J.amp_q != 0u;
    if (signal) {
        const uint4 *src = (const uint4 *)tab;
        s_tab[tid] = src[tid];
        s_tab[tid + RD_BURST_THREADS] = src[tid + RD_BURST_THREADS];
        if (tid <= (unsigned)RD_CS_MAX_SYM) {
            uint32_t ones = 0u;
#pragma unroll
            for (unsigned i = 0; i < sizeof J.bits / 4; i++) {
                uint32_t w;
                __builtin_memcpy(&w, J.bits + 4 * i, 4);
                w = __builtin_bswap32(w);                 // symbol 32 i + j in bit 31 - j
                if (i < (tid >> 5)) ones += (uint32_t)__popc(w);
                else if (i == (tid >> 5) && (tid & 31u)) ones += (uint32_t)__popc(w >> (32u - (tid & 31u)));
            }
            s_cum[tid] = 2 * (int)ones - (int)tid;
        }
    }
    __syncthreads();
    const int16_t *T = (const int16_t *)s_tab;
    const int SL = P.sl, n = (int)J.n, pre = (int)J.pre;
    const int body = SL * (int)J.n_sym, L = pre + body + (int)J.post;
    const int start = J.at - pre;                        // u = t - start; |start| <= 2^30 + 4096, t < 2^24
    const uint32_t k0 = (uint32_t)J.seed, k1 = (uint32_t)(J.seed >> 32);
    const int64_t mid = 256ll << 21;               // 128 bytes
    uint4 *dst = (uint4 *)(pool + 2ull * J.offset);
    const int n_vec = (n + 7) >> 3;
    for (int v8 = (int)tid; v8 < n_vec; v8 += RD_BURST_THREADS) {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            uint32_t word = 0u;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int t = 8 * v8 + 2 * i + h;
                if (t < n) {
                    int64_t si = mid, sq = mid;
                    const int u = t - start;
                    if (signal && u >= 0 && u < L) {
                        const int v = u - pre;
                        int D = 0;
                        if (v >= body) D = SL * s_cum[J.n_sym];
                        else if (v >= 0) {
                            const int k = SL == 1 ? v : (int)__umulhi((uint32_t)v, P.inv_sl);
                            const int r = v - k * SL, a = s_cum[k];
                            D = SL * a + (r + 1) * (s_cum[k + 1] - a);
                        }
                        const uint32_t phi = J.phase0 + (uint32_t)(u + 1) * (uint32_t)J.f_c + J.f_d * (uint32_t)D;
                        si += (int64_t)((int)J.amp_q * (int)T[phi >> 20]);
                        sq += (int64_t)((int)J.amp_q * (int)T[(phi - 0x40000000u) >> 20]);
                    }
                    if (J.noise_q != 0u) {
                        si += (int64_t)J.noise_q * (int64_t)(rd_cs_noise((uint32_t)t, 0u, k0, k1) - 2040);
                        sq += (int64_t)J.noise_q * (int64_t)(rd_cs_noise((uint32_t)t, 1u, k0, k1) - 2040);
                    }
                    word |= (rd_cs_byte(si) | (rd_cs_byte(sq) << 8)) << (16 * h);
                }
            }
            w[i] = word;
        }
        dst[v8] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ------------------------------------------------------------------------------------------
// host side: the C ABI
// ------------------------------------------------------------------------------------------
extern "C" int rd_clips_synth(rd_clips *h, const rd_clip_spec *specs, int n_specs, uint64_t pool_outputs) {
    if (!h) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (pool_outputs > RD_CS_MAX_POOL) return rd_fail_msg(RD_ERR_ARG, "clip synth: a pool of more than 2^40 outputs");
    int bad = -1;
    const char *why = "";
    if (rd_cs_check_specs(specs, n_specs, pool_outputs, &bad, &why)) return rd_fail_msg(RD_ERR_ARG, "clip synth: spec %d: %s", bad, why);
    int rc = rd_cd_prepare(h);
    if (rc) return rc;
    if (!h->sv0 && (hipEventCreate(&h->sv0) != hipSuccess || hipEventCreate(&h->sv1) != hipSuccess))
        return rd_fail_msg(RD_ERR_DEVICE, "clip synth: no events");
    if (!h->d_cs_tab) {
        std::vector<int16_t> tab(RD_CS_TABLE);
        rd_cs_table(tab.data());
        int16_t *d = nullptr;
        if (hipMalloc(&d, RD_CS_TABLE * sizeof(int16_t)) != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "clip synth: hipMalloc of the table failed");
        if (hipMemcpy(d, tab.data(), RD_CS_TABLE * sizeof(int16_t), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(d);
            return rd_fail_msg(RD_ERR_DEVICE, "clip synth: the copy of the table failed");
        }
        h->d_cs_tab = d;
    }
    const size_t ns = (size_t)n_specs;
    if (n_specs > h->cap_specs) {
        if (h->d_specs) (void)hipFree(h->d_specs);
        h->d_specs = nullptr;
        h->cap_specs = 0;
        if (hipMalloc(&h->d_specs, ns * sizeof(rd_clip_spec)) != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "clip synth: hipMalloc for %d specs failed", n_specs);
        h->cap_specs = n_specs;
    }
    size_t need = 0;
    if ((rc = rd_cd_size_pool(h, 2 * (size_t)pool_outputs, &need))) return rc;   // (no pool from here on until the kernel is through)
    rd_cs_params P;
    P.sl = h->cfg.symbol_length;
    P.inv_sl = P.sl >= 2 ? (uint32_t)(0x100000000ull / (uint64_t)P.sl) + 1u : 0u;
    P.pool_outputs = pool_outputs;
    h->synth_ms = -1.0f;
    if (hipMemcpyAsync(h->d_specs, specs, ns * sizeof(rd_clip_spec), hipMemcpyHostToDevice, h->st) != hipSuccess ||
        hipEventRecord(h->sv0, h->st) != hipSuccess || hipMemsetAsync(h->d_pool, 0, need, h->st) != hipSuccess)
        return rd_fail_msg(RD_ERR_DEVICE, "clip synth: the copy of the specs or the zeroing of the pool failed");
    hipLaunchKernelGGL(k_clip_synth, dim3((unsigned)n_specs), dim3(RD_BURST_THREADS), 0, h->st, h->d_pool, P, h->d_specs, h->d_cs_tab);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "k_clip_synth: %s", hipGetErrorString(e));
    if (hipEventRecord(h->sv1, h->st) != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "clip synth: hipEventRecord failed");
    if ((rc = rd_cd_wait(h, "k_clip_synth"))) return rc;
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, h->sv0, h->sv1) == hipSuccess) h->synth_ms = ms;
    h->pool_outputs = pool_outputs;
    return RD_OK;
}

extern "C" int rd_clips_download(rd_clips *h, uint8_t *out, size_t nbytes) {
    if (!h || !out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (!h->pool_outputs) return rd_fail_msg(RD_ERR_STATE, "clip decode: there is no pool to download");
    if ((uint64_t)nbytes != 2ull * h->pool_outputs)
        return rd_fail_msg(RD_ERR_ARG, "clip decode: %zu bytes asked for, the pool holds %llu", nbytes, 2ull * (unsigned long long)h->pool_outputs);
    int rc = rd_cd_prepare(h);
    if (rc) return rc;
    if (hipMemcpyAsync(out, h->d_pool, nbytes, hipMemcpyDeviceToHost, h->st) != hipSuccess)
        return rd_fail_msg(RD_ERR_DEVICE, "clip decode: the copy of the pool failed");
    return rd_cd_wait(h, "the copy of the pool");
}

extern "C" int rd_clips_synth_ms(rd_clips *h, float *ms) {
    if (!h || !ms) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (h->synth_ms < 0.0f) return rd_fail_msg(RD_ERR_STATE, "clip synth: no synthesis has completed");
    *ms = h->synth_ms;
    return RD_OK;
}
