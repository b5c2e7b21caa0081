// rd_burst_common.h - the small device helpers k_chan_burst_decode (rd_burst_decode.hip) and k_chan_burst_expect
// (rd_burst_expect.hip) share: the system-scope load, p and p' from LDS, the packed 16-bit dot product and the total
// orders of the candidates' reduction.  All forced inline: each kernel is compiled as if it held them itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

// (margin, tau) of lane a is the better candidate than that of lane b; tau = INT32_MAX: none
__device__ __forceinline__ bool rd_bd_better(uint64_t ma, int ta, uint64_t mb, int tb) {
    if (tb == INT32_MAX) return true;
    if (ta == INT32_MAX) return false;
    return ma > mb || (ma == mb && ta < tb);
}

// the same with the flips of step 6' in front: f = count | k1 << 8 | k2 << 16, 0 for an exact candidate
__device__ __forceinline__ bool rd_bd_better_r(uint32_t fa, uint64_t ma, int ta, uint32_t fb, uint64_t mb, int tb) {
    if (tb == INT32_MAX) return true;
    if (ta == INT32_MAX) return false;
    const uint32_t na = fa & 0xFFu, nb = fb & 0xFFu;
    if (na != nb) return na < nb;
    return ma > mb || (ma == mb && ta < tb);
}
