// rd_clip_decode.hip - decode recorded clips, many per launch (include/rtldavis_hip.h, CLIP DECODE).
// k_chan_burst_expect decodes where the host expects a packet in a channel of a live chunk; this kernel does the same
// for a clip that lies anywhere in an uploaded pool of channelized bytes, taken as a chunk of its own: no chunk before,
// any length, and - when the job gives no direction - sliced around the clip's own.  rd_clips_* below is its C ABI:
// the pool, the jobs, the records, the headers and the soft values all live in device memory, for a call takes up to
// 2^20 jobs, which is no load for a mapped slot.
//
// Kernel.  One workgroup of 256 threads per job, grid = the number of jobs.  The job is read from device memory at a
// workgroup-uniform address.  Candidates tau_a = max(tau_lo, SL) .. tau_b = min(tau_hi, n - 1 - SL (N - 1)); region
// t0 = tau_a - SL >= 0, t1 = tau_b + SL (N - 1) + 1 <= n, at most 4096 outputs.  The bytes are loaded from L0 = the filter's
// first output (t0 without the filter) rounded DOWN to 8 up to its last rounded UP to 8 by rd_bd_load_bytes in its form
// without a seam (L0 >= 0); a clip begins at a multiple of 8 outputs of a 16-byte aligned pool, so every
// vector is aligned, and the pool's device copy is padded to whole vectors, so the last one of a clip whose n is no
// multiple of 8 stays inside the allocation.  Everything behind the load indexes from t0 and stops at t1 (at zf0 .. zf1 for
// the filter, zf1 <= n): what the rounded loads bring along from the clip's neighbours is never read.
// Own direction (corr = (0, 0)): every thread sums p over its outputs of t0 < t < t1, a fixed tree of shuffles adds the
// lanes and the four waves' sums meet in LDS - integers, no atomics; then the shift of step 4n.
// Then the phases of rd_burst_common.h with one lane per tau over tau_a .. tau_b only, as in the expect kernel, and the
// winner's N symbol sums go out as the job's soft values, one thread per symbol.  The kernel spells out what
// rd_bd_best_in_region and rd_bd_packet_f<false> would do for it - the same phases, the same barriers: through them it
// gave the same results 1 % slower in three of its four forms (profiles/burst_region_refactor.txt), and this is the
// kernel whose time alone is a product figure (profiles/clip_replay.txt).  Keep the two in step.
// LDS: the expect kernel's budget - s (int64, 32 KiB), the bytes (8.25 KiB), y (16 KiB, narrow only), plus 32 bytes
// for the own direction: 41 KiB per workgroup without the filter (three workgroups on a CU's 160 KiB), 58 KiB with it
// (two).  Plain vector stores into device memory, no atomics.
#include <new>
#include <type_traits>

#include <hip/hip_runtime.h>

#include "rd_burst_common.h"
#include "rd_clips.h"

#define RD_CD_LEN (RD_CD_MAX_SPAN + RD_BD_MAX_LOOK_W * RD_BU_WINDOW)   // t1 - t0 at most: the span + N SL + 1
#define RD_CD_LOAD (RD_CD_LEN + 128)                                    // outputs loaded at most
static_assert(RD_CD_MAX_SPAN == RD_BX_MAX_SPAN, "a job's range is an expectation's");
static_assert(RD_CD_LEN + 2 * (RD_BD_NB_MAX_SL + 2) + 14 <= RD_CD_LOAD && RD_CD_LOAD % 8 == 0, "the filter's margins and the rounding to 8");
static_assert((RD_CD_LEN + RD_BD_NB_MAX_T - 1) * 4 <= RD_CD_LEN * 8, "the padded int16 region lies in s's place");
static_assert(sizeof(rd_clip_job) == 48 && sizeof(rd_cd_header) == 16 && sizeof(rd_burst_msg) == 64, "the layouts of CLIP DECODE");
static_assert(8 * RD_BD_DATA_BYTES <= RD_BURST_THREADS, "one thread per symbol of the soft values");

struct rd_cd_params {
    rd_bd_shape shape;
    uint64_t pool_outputs;     // outputs the pool holds
};

template <bool REPAIR, bool NARROW>
__global__ __launch_bounds__(RD_BURST_THREADS) void k_clip_decode(const uint8_t *__restrict__ pool, rd_cd_params P,
                                                                  const rd_clip_job *__restrict__ jobs, rd_burst_msg *recs,
                                                                  rd_cd_header *hdr, int64_t *soft,
                                                                  const uint32_t *__restrict__ nb_tab) {
    using f_t = std::conditional_t<NARROW, int64_t, int>;
    __shared__ int64_t s_s[RD_CD_LEN];                   // s[t0 + i] at i (i >= SL)
    __shared__ uint4 s_z[RD_CD_LOAD / 8];                // the loaded bytes: output L0 + i at bytes 2 i, 2 i + 1
    __shared__ uint64_t s_m[RD_BURST_THREADS / 64];
    __shared__ int s_t[RD_BURST_THREADS / 64];
    __shared__ f_t s_fr[RD_BURST_THREADS / 64], s_fi[RD_BURST_THREADS / 64];
    __shared__ int s_or[RD_BURST_THREADS / 64], s_oi[RD_BURST_THREADS / 64];   // (own direction) the waves' sums of p
    __shared__ uint16_t s_E[8 * RD_BD_DATA_BYTES];       // (REPAIR) E[k], 16 <= k < N
    __shared__ uint32_t s_f[RD_BURST_THREADS / 64];      // (REPAIR) the waves' flips
    __shared__ uint32_t s_y[RD_CD_LEN];                  // (NARROW) y[t0 + i] at i: re in the low half, im in the high one
    __shared__ uint32_t s_hA[RD_BD_NB_MAX_T], s_hB[RD_BD_NB_MAX_T];   // (NARROW) H[g][kk - M] as (re, -im) and (im, re)
    const unsigned x = blockIdx.x;
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const rd_clip_job J = jobs[x];                       // (a workgroup-uniform address: every thread gets the same job)
    if constexpr (REPAIR) rd_bd_syndrome_table(s_E, P.shape.n_sym, tid);   // (read behind the barrier that follows the load)
    const int SL = P.shape.sl, N = P.shape.n_sym, body = SL * (N - 1), M = SL + 2;
    // The job's geometry, in 64 bits until rd_cd_check_jobs' rules have been checked again: a job that fails is idle.
    const int64_t n = (int64_t)J.n;
    const int64_t a64 = J.tau_lo > SL ? (int64_t)J.tau_lo : (int64_t)SL;
    const int64_t b64 = (int64_t)J.tau_hi < n - 1 - body ? (int64_t)J.tau_hi : n - 1 - body;
    int32_t cr = J.corr_re, ci = J.corr_im;
    bool active = a64 <= b64 && b64 - a64 <= RD_CD_MAX_SPAN && J.tau_lo <= J.tau_hi && J.tau_lo >= -RD_CD_MAX_TAU &&
                  J.tau_hi <= RD_CD_MAX_TAU && (J.offset & 7ull) == 0ull && J.n >= 1u && J.offset <= P.pool_outputs &&
                  (uint64_t)J.n <= P.pool_outputs - J.offset && cr >= -32768 && cr <= 32767 && ci >= -32768 && ci <= 32767;
    const int tau_a = active ? (int)a64 : 0, tau_b = active ? (int)b64 : -1;
    const int t0 = tau_a - SL, t1 = tau_b + body + 1, len = t1 - t0;
    const int zf0 = NARROW ? max(t0 - M, 0) : t0, zf1 = NARROW ? ((int64_t)(t1 + M) < n ? t1 + M : (int)n) : t1;
    const int L0 = zf0 & ~7, L1 = (zf1 + 7) & ~7;         // (floor and ceiling; L1 may pass n by up to 7 outputs)
    active = active && t0 >= 0 && (int64_t)t1 <= n && len <= RD_CD_LEN && L1 - L0 <= RD_CD_LOAD;
    bool found = false;
    if (active) {
        const uint8_t *src = pool + 2ull * J.offset;
        const uint16_t *zl = (const uint16_t *)s_z;      // output L0 + i: I in the low byte, Q in the high one
        const uint16_t *zw = zl + (t0 - L0);             // output t0 + i
        rd_bd_load_bytes<false>(s_z, src, nullptr, L0, L1, 0l, tid);   // (L0 >= 0: there is no chunk before)
        __syncthreads();
        if (cr == 0 && ci == 0) {                         // own direction: F = the sum of p over t0 < t < t1
            int fr = 0, fi = 0;
            for (int j = 1 + (int)tid; j < len; j += RD_BURST_THREADS) {
                int re, im;
                rd_bd_p(zw, j, re, im);
                fr += re;
                fi += im;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                fr += __shfl_xor(fr, off);
                fi += __shfl_xor(fi, off);
            }
            if (lane == 0u) {
                s_or[wave] = fr;
                s_oi[wave] = fi;
            }
            __syncthreads();
            fr = 0;
            fi = 0;
            for (int wv = 0; wv < RD_BURST_THREADS / 64; wv++) {
                fr += s_or[wv];
                fi += s_oi[wv];
            }
            const int mr = fr < 0 ? -fr : fr, mi = fi < 0 ? -fi : fi;
            const uint32_t mag = (uint32_t)(mr > mi ? mr : mi);   // (< 2^30)
            const int bl = mag ? 32 - __clz((int)mag) : 0, sh = bl > 15 ? bl - 15 : 0;
            cr = fr >> sh;
            ci = fi >> sh;
        }
    }
    if (active && (cr != 0 || ci != 0)) {                // (uniform: every thread holds the same direction)
        const uint16_t *zl = (const uint16_t *)s_z;
        const uint16_t *zw = zl + (t0 - L0);
        int nb_g = 0;                                     // (NARROW) g of step 4n
        if constexpr (NARROW) {
            const int T = 2 * SL + 5;
            uint32_t *z16 = (uint32_t *)s_s;              // output t0 - M + i at word i
            nb_g = rd_bd_grid_choice(nb_tab, T, cr, ci, lane);
            rd_bd_load_taps(nb_tab, nb_g, T, s_hA, s_hB, tid);
            rd_bd_fill_z16(z16, zl, L0, t0 - M, len + 2 * M, zf0, zf1, tid);
            __syncthreads();
            rd_bd_filter(z16, len, T, s_hA, s_hB, s_y, tid);
            __syncthreads();                              // y is whole, and z16 has been read: s may be written
        }
        rd_bd_symbol_sums<NARROW>(zw, s_y, s_s, SL, len, cr, ci, tid);
        __syncthreads();
        // ---- one lane per tau = t0 + i, tau_a <= tau <= tau_b
        uint64_t best_m = 0ull;
        int best_t = INT32_MAX;
        uint32_t best_f = 0u;
        const int i_hi = len - body;                      // = SL + (tau_b - tau_a) + 1
        for (int i = SL + (int)tid; i < i_hi; i += RD_BURST_THREADS)
            rd_bd_consider<REPAIR>(s_s + i, SL, N, P.shape.sync, P.shape.max_flips, s_E, J.id, t0 + i, best_f, best_m, best_t);
        rd_bd_reduce_best<REPAIR>(best_f, best_m, best_t, s_f, s_m, s_t, lane, wave);
        found = best_t != INT32_MAX;                      // (uniform: every thread read the same four)
        if (found) {
            const int i0 = best_t - t0;                   // (>= SL: the first pair lies in the region)
            rd_bd_packet_f<NARROW>(zw, s_y, i0 - SL + 1, i0 + body, s_fr, s_fi, tid);
            if (tid == 0u)
                rd_bd_write_record<REPAIR, NARROW>(&recs[x], J.channel, (uint32_t)x, RD_BURST_MSG_REPLAYED, best_t, J.clock, best_m,
                                                   best_f, s_fr, s_fi, s_s + i0, SL, N, nb_g);
            if (soft && (int)tid < N) soft[(size_t)x * (size_t)N + tid] = s_s[i0 + SL * (int)tid];
        }
    }
    if (tid == 0u) {
        rd_cd_header h;
        h.n_msgs = found ? 1u : 0u;
        h.candidates = active ? (uint32_t)(tau_b - tau_a + 1) : 0u;
        h.ca = active ? cr : 0;
        h.cb = active ? ci : 0;
        hdr[x] = h;
    }
}

// ------------------------------------------------------------------------------------------
// host side: the C ABI
// ------------------------------------------------------------------------------------------
// the configuration rule of rd_wb_set_burst_decode without its block_size rule: block_size takes no part here
static int rd_cd_check_config(const rd_config *cfg) {
    if (!cfg) return rd_fail_msg(RD_ERR_ARG, "null argument");
    rd_config c = *cfg;
    c.block_size = RD_BD_MAX_LOOK_W * RD_BU_WINDOW;
    return rd_burst_decode_check(&c);
}

// the library's polling wait with its deadline (rd_hiphost.h); a wait that gave up leaves the handle busy
int rd_cd_wait(rd_clips *h, const char *what) {
    const int rc = rd_wait_stream(h->st, what);
    if (!rc) h->busy = false;
    else if (hipStreamQuery(h->st) == hipErrorNotReady) h->busy = true;
    return rc ? rd_fail_msg(rc, "clip decode: %s", rd_last_error()) : RD_OK;
}

int rd_cd_prepare(rd_clips *h) {
    int rc = rd_ensure_device();
    if (rc) return rc;
    if (!h->st) {
        if (hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&h->ev0) != hipSuccess ||
            hipEventCreate(&h->ev1) != hipSuccess)
            return rd_fail_msg(RD_ERR_DEVICE, "clip decode: no stream or events");
    }
    if (h->busy) return rd_cd_wait(h, "the work a timed-out call left behind");
    return RD_OK;
}

extern "C" int rd_clips_create(const rd_config *cfg, rd_clips **out) {
    if (!out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    *out = nullptr;
    int rc = rd_cd_check_config(cfg);
    if (rc) return rc;
    rd_clips *h = new (std::nothrow) rd_clips;
    if (!h) return rd_fail_msg(RD_ERR_DEVICE, "clip decode: out of host memory");
    h->cfg = *cfg;
    *out = h;
    return RD_OK;
}

extern "C" void rd_clips_destroy(rd_clips *h) {
    if (!h) return;
    if (h->st) {
        (void)hipStreamSynchronize(h->st);
        (void)hipStreamDestroy(h->st);
    }
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->sv0) (void)hipEventDestroy(h->sv0);
    if (h->sv1) (void)hipEventDestroy(h->sv1);
    void *bufs[] = {h->d_pool, h->d_jobs, h->d_recs, h->d_hdr, h->d_soft, h->d_nb, h->d_specs, h->d_cs_tab};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    delete h;
}

int rd_cd_size_pool(rd_clips *h, size_t nbytes, size_t *need_out) {
    const size_t need = (nbytes + 15) & ~(size_t)15;
    h->pool_outputs = 0;
    if (need > h->pool_cap) {
        if (h->d_pool) (void)hipFree(h->d_pool);
        h->d_pool = nullptr;
        h->pool_cap = 0;
        if (hipMalloc(&h->d_pool, need) != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "clip decode: hipMalloc of a pool of %zu bytes failed", need);
        h->pool_cap = need;
    }
    *need_out = need;
    return RD_OK;
}

extern "C" int rd_clips_upload(rd_clips *h, const uint8_t *pool, size_t nbytes) {
    if (!h || !pool) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (nbytes < 2 || (nbytes & 1)) return rd_fail_msg(RD_ERR_ARG, "clip decode: a pool of %zu bytes (an even number, at least 2)", nbytes);
    int rc = rd_cd_prepare(h);
    if (rc) return rc;
    size_t need = 0;
    if ((rc = rd_cd_size_pool(h, nbytes, &need))) return rc;
    if (hipMemcpyAsync(h->d_pool, pool, nbytes, hipMemcpyHostToDevice, h->st) != hipSuccess ||
        (need > nbytes && hipMemsetAsync(h->d_pool + nbytes, 0, need - nbytes, h->st) != hipSuccess))
        return rd_fail_msg(RD_ERR_DEVICE, "clip decode: the copy of the pool failed");
    if ((rc = rd_cd_wait(h, "the copy of the pool"))) return rc;
    h->pool_outputs = nbytes / 2;
    return RD_OK;
}

extern "C" int rd_clips_decode(rd_clips *h, const rd_clip_job *jobs, int n_jobs, int max_flips, int narrow, rd_burst_msg *msgs,
                               rd_cd_header *hdr, int64_t *soft) {
    if (!h) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = rd_burst_hook_modes(&h->cfg, max_flips, narrow);
    if (rc) return rc;
    if (!jobs || !msgs || !hdr) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (n_jobs < 1 || n_jobs > RD_CD_MAX_JOBS) return rd_fail_msg(RD_ERR_ARG, "clip decode: %d jobs, not 1 .. %d", n_jobs, RD_CD_MAX_JOBS);
    if (!h->pool_outputs) return rd_fail_msg(RD_ERR_STATE, "clip decode: no pool has been uploaded");
    int bad = -1;
    const char *why = "";
    if (rd_cd_check_jobs(&h->cfg, jobs, n_jobs, (size_t)h->pool_outputs, &bad, &why))
        return rd_fail_msg(RD_ERR_ARG, "clip decode: job %d: %s", bad, why);
    if ((rc = rd_cd_prepare(h))) return rc;
    const size_t N = (size_t)h->cfg.packet_symbols, nj = (size_t)n_jobs;
    if (n_jobs > h->cap_jobs) {
        void **bufs[] = {(void **)&h->d_jobs, (void **)&h->d_recs, (void **)&h->d_hdr};
        const size_t each[] = {sizeof(rd_clip_job), sizeof(rd_burst_msg), sizeof(rd_cd_header)};
        h->cap_jobs = 0;
        for (int i = 0; i < 3; i++) {
            if (*bufs[i]) (void)hipFree(*bufs[i]);
            *bufs[i] = nullptr;
            if (hipMalloc(bufs[i], nj * each[i]) != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "clip decode: hipMalloc for %d jobs failed", n_jobs);
        }
        h->cap_jobs = n_jobs;
    }
    if (soft && n_jobs > h->cap_soft) {
        if (h->d_soft) (void)hipFree(h->d_soft);
        h->d_soft = nullptr;
        h->cap_soft = 0;
        if (hipMalloc(&h->d_soft, nj * N * sizeof(int64_t)) != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "clip decode: hipMalloc of the soft values failed");
        h->cap_soft = n_jobs;
    }
    if (narrow && !h->d_nb && (rc = rd_bd_narrow_upload(h->cfg.symbol_length, &h->d_nb))) return rc;
    rd_cd_params P;
    P.shape = rd_bd_shape_of(&h->cfg, max_flips);
    P.pool_outputs = h->pool_outputs;
    int64_t *d_soft = soft ? h->d_soft : nullptr;
    // the record and header places of a job that writes none read 0
    if (hipMemcpyAsync(h->d_jobs, jobs, nj * sizeof(rd_clip_job), hipMemcpyHostToDevice, h->st) != hipSuccess ||
        hipMemsetAsync(h->d_recs, 0, nj * sizeof(rd_burst_msg), h->st) != hipSuccess ||
        hipMemsetAsync(h->d_hdr, 0, nj * sizeof(rd_cd_header), h->st) != hipSuccess ||
        (d_soft && hipMemsetAsync(d_soft, 0, nj * N * sizeof(int64_t), h->st) != hipSuccess) ||
        hipEventRecord(h->ev0, h->st) != hipSuccess)
        return rd_fail_msg(RD_ERR_DEVICE, "clip decode: the copy of the jobs failed");
    rd_bd_with_form(max_flips != 0, narrow != 0, [&](auto repair, auto narrow_form) {
        hipLaunchKernelGGL((k_clip_decode<decltype(repair)::value, decltype(narrow_form)::value>), dim3((unsigned)n_jobs),
                           dim3(RD_BURST_THREADS), 0, h->st, h->d_pool, P, h->d_jobs, h->d_recs, h->d_hdr, d_soft, h->d_nb);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "k_clip_decode: %s", hipGetErrorString(e));
    h->kernel_ms = -1.0f;
    if (hipEventRecord(h->ev1, h->st) != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "clip decode: hipEventRecord failed");
    // the kernel is waited for here, under the deadline: a copy into pageable memory would wait for it inside the runtime
    if ((rc = rd_cd_wait(h, "k_clip_decode"))) return rc;
    if (hipMemcpyAsync(msgs, h->d_recs, nj * sizeof(rd_burst_msg), hipMemcpyDeviceToHost, h->st) != hipSuccess ||
        hipMemcpyAsync(hdr, h->d_hdr, nj * sizeof(rd_cd_header), hipMemcpyDeviceToHost, h->st) != hipSuccess ||
        (soft && hipMemcpyAsync(soft, d_soft, nj * N * sizeof(int64_t), hipMemcpyDeviceToHost, h->st) != hipSuccess))
        return rd_fail_msg(RD_ERR_DEVICE, "clip decode: the copy of the results failed");
    if ((rc = rd_cd_wait(h, "the copy of the results"))) return rc;
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->kernel_ms = ms;
    return RD_OK;
}

extern "C" int rd_clips_kernel_ms(rd_clips *h, float *ms) {
    if (!h || !ms) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (h->kernel_ms < 0.0f) return rd_fail_msg(RD_ERR_STATE, "clip decode: no decode has completed");
    *ms = h->kernel_ms;
    return RD_OK;
}
