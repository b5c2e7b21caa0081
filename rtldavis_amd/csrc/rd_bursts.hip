// rd_bursts.hip - burst detection on the channelized chunk (include/rtldavis_hip.h, BURSTS): per channel, the energy and
// the lag-1 correlation of every window of 128 outputs, and one record per run of consecutive windows whose energy
// reaches the channel's threshold.  Used by rd_wideband.hip per streamed chunk (rd_wb_set_bursts): the carrier frequency
// of a burst the demodulator cannot decode yet is angle(sum r_w) out_rate / 2 pi (rtldavis_amd/acquire.py).
//
// Definition (exact integers throughout).  Channel c, its 2 B bytes b of the chunk, aI[t] = 2 b[2t] - 255,
// aQ[t] = 2 b[2t+1] - 255, z = aI + j aQ; nW = B / 128 windows; window w holds outputs [128 w, 128 w + 128):
//   p_w = sum |z[t]|^2 over its 128 outputs                     (<= 256 x 65025: uint32)
//   r_w = sum z[t] conj(z[t-1]) over its 127 inner pairs        (|re|, |im| <= 254 x 65025: int32)
// Nothing crosses a window, so the kernel is stateless.  Window w is ON when p_w >= thr[c]; a burst is a maximal run of
// ON windows inside the chunk, one rd_burst per run in ascending `first`; the OFF windows go to the channel's
// rd_burst_floor.
//
// Sums from the bytes.  With a_x a_y = 4 b_x b_y - 510 (b_x + b_y) + 65025 and k the byte index inside the window
// (I[t] = b[2t], Q[t] = b[2t+1]):
//   p    = 4 S2 - 1020 S1 + 256 x 65025                          S1 = sum b_k, S2 = sum b_k^2
//   re r = 4 X2 - 510 (2 S1 - b0 - b1 - b254 - b255) + 254 x 65025        X2 = sum_{k >= 2} b_k b_{k-2}
//   im r = 4 (X3 - X1) - 510 (b0 - b1 - b254 + b255)             X3 = sum_{odd k >= 3} b_k b_{k-3}   (Q[t] I[t-1])
//                                                                X1 = sum_{even k >= 2} b_k b_{k-1}  (I[t] Q[t-1])
// (the linear terms of im r telescope).  Every sum is a packed-byte dot product (v_dot4_u32_u8, as k_chan_levels) of a
// dword with itself, with ones, or with the byte stream shifted by 1, 2 or 3 bytes; for X3 and X1 the dword keeps its
// odd or its even bytes only.
//
// Kernel.  One workgroup of 256 threads per channel.  Pass 1: 16 lanes take one window - a lane loads one 16-byte vector
// (8 outputs); the dword in front of its own comes from the lane to its left (a shuffle within the 16), and the first
// lane of a window takes zeros there, which drops the pairs that would cross into the window before.  The lane's three
// linear combinations are reduced within the 16 lanes and p, re r, im r of the window go to LDS (48 KiB at nW = 4096,
// the most rd_bursts_check admits).  Pass 2, the first wave alone: 64 windows at a time, the ON mask by a ballot; a
// segmented inclusive scan by shuffles (lane l adds lane l - off only when its run began at or before l - off) gives
// every lane the sums of its run so far - 32 bits suffice inside 64 windows -; the lanes at a run's end write the
// record.  A run that reaches lane 63 is carried into the next 64 windows in wave-uniform 64-bit registers and joins the
// run that begins at lane 0 there, or is written by lane 0 when that window is OFF.
// Output layout: channel c owns cap = ceil(nW / 2) record places - the most runs nW windows can hold - and its floor
// record, so there is no overflow, no ticket between workgroups and no atomic: record i of channel c is its i-th run.
// The order and every bit are the same from run to run.  All stores are plain vector stores into the mapped host slot
// of the chunk's parity; the thresholds are read from that slot (the host wrote them before the launch; a system-scope
// load, so no cache of an earlier launch can answer) and echoed in the floor record.
// Cost: one more read of the chunk's channelized bytes (16 KiB per channel at B = 8192), five dot products per dword.
#include <cstring>

#include <hip/hip_runtime.h>

#include "rd_internal.h"

#define RD_BU_THREADS 256
#define RD_BU_LANES 16                           // lanes per window: 16 vectors of 16 bytes
#define RD_BU_PER_PASS (RD_BU_THREADS / RD_BU_LANES)

static_assert(sizeof(rd_burst) == 48 && sizeof(rd_burst_floor) == 40, "the slot layout of rd_bu_* (rd_internal.h)");

// bytes [4 i - s, 4 i - s + 4) of the stream whose dword i is cur and dword i - 1 is prev
__device__ __forceinline__ uint32_t rd_bu_back(uint32_t cur, uint32_t prev, int s) {
    return (uint32_t)((((uint64_t)cur << 32) | (uint64_t)prev) >> (32 - 8 * s));
}

__global__ __launch_bounds__(RD_BU_THREADS) void k_chan_bursts(const uint4 *__restrict__ chan, size_t ch_stride_vec, unsigned n_win,
                                                               unsigned cap, const uint32_t *thr_in, uint64_t seq,
                                                               rd_burst *recs, rd_burst_floor *floor) {
    __shared__ uint32_t s_p[RD_BU_MAX_WINDOWS];
    __shared__ int32_t s_re[RD_BU_MAX_WINDOWS], s_im[RD_BU_MAX_WINDOWS];
    const int c = (int)blockIdx.x;
    const uint4 *src = chan + (size_t)c * ch_stride_vec;
    const unsigned l16 = threadIdx.x & (RD_BU_LANES - 1);
    // ---- pass 1: p, re r, im r per window
    for (unsigned w = threadIdx.x / RD_BU_LANES; w < n_win; w += RD_BU_PER_PASS) {   // (the 16 lanes of a window agree on w)
        const uint4 v = src[(size_t)w * RD_BU_LANES + l16];
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
        uint32_t prev = (uint32_t)__shfl_up((int)v.w, 1, RD_BU_LANES);
        if (l16 == 0) prev = 0u;
        uint32_t s1 = 0u, s2 = 0u, x1 = 0u, x2 = 0u, x3 = 0u;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t cur = d[i];
            s1 = __builtin_amdgcn_udot4(cur, 0x01010101u, s1, false);
            s2 = __builtin_amdgcn_udot4(cur, cur, s2, false);
            x2 = __builtin_amdgcn_udot4(cur, rd_bu_back(cur, prev, 2), x2, false);
            x3 = __builtin_amdgcn_udot4(cur & 0xFF00FF00u, rd_bu_back(cur, prev, 3), x3, false);
            x1 = __builtin_amdgcn_udot4(cur & 0x00FF00FFu, rd_bu_back(cur, prev, 1), x1, false);
            prev = cur;
        }
        // the window's four edge bytes: b0, b1 in its first lane, b254, b255 in its last
        int e_re = 0, e_im = 0;
        if (l16 == 0) {
            const int b0 = (int)(v.x & 0xFFu), b1 = (int)((v.x >> 8) & 0xFFu);
            e_re = b0 + b1;
            e_im = b0 - b1;
        }
        if (l16 == RD_BU_LANES - 1) {
            const int b254 = (int)((v.w >> 16) & 0xFFu), b255 = (int)(v.w >> 24);
            e_re = b254 + b255;
            e_im = b255 - b254;
        }
        int p = 4 * (int)s2 - 1020 * (int)s1;                        // a lane's parts: |.| < 2^23
        int re = 4 * (int)x2 - 1020 * (int)s1 + 510 * e_re;
        int im = 4 * ((int)x3 - (int)x1) - 510 * e_im;
#pragma unroll
        for (int off = RD_BU_LANES / 2; off > 0; off >>= 1) {
            p += __shfl_xor(p, off, RD_BU_LANES);
            re += __shfl_xor(re, off, RD_BU_LANES);
            im += __shfl_xor(im, off, RD_BU_LANES);
        }
        if (l16 == 0) {
            s_p[w] = (uint32_t)(p + 256 * 65025);
            s_re[w] = re + 254 * 65025;
            s_im[w] = im;
        }
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    // ---- pass 2: runs of ON windows, 64 windows at a time
    const unsigned lane = threadIdx.x;
    const uint32_t thr = __hip_atomic_load(&thr_in[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    rd_burst *mine = recs + (size_t)c * cap;
    const uint64_t below_me = (1ull << lane) - 1ull;
    // the run that reached the end of the windows before this group (wave-uniform)
    bool open = false;
    uint32_t c_first = 0u, c_win = 0u, c_peak = 0u;
    uint64_t c_pow = 0ull;
    int64_t c_re = 0, c_im = 0;
    uint32_t n_done = 0u;
    // the OFF windows, a lane's own
    uint32_t off_n = 0u;
    uint64_t off_p = 0ull;
    int64_t off_re = 0, off_im = 0;
    for (unsigned g0 = 0; g0 < n_win; g0 += 64) {
        const unsigned w = g0 + lane;
        const bool valid = w < n_win;
        const uint32_t p = valid ? s_p[w] : 0u;
        const int32_t re = valid ? s_re[w] : 0, im = valid ? s_im[w] : 0;
        const bool on = valid && p >= thr;
        const uint64_t m = __ballot(on);
        if (valid && !on) {
            off_n++;
            off_p += p;
            off_re += re;
            off_im += im;
        }
        if (open && !(m & 1ull)) {                                    // the carried run ended with the group before
            if (lane == 0) {
                rd_burst r;
                r.channel = c; r.first = c_first; r.windows = c_win; r.flags = c_first == 0u ? 1u : 0u;
                r.power = c_pow; r.peak = c_peak; r.pad = 0u; r.corr_re = c_re; r.corr_im = c_im;
                mine[n_done] = r;
            }
            n_done++;
            open = false;
        }
        // s: the lane at which this lane's run begins inside the group (meaningful for ON lanes); dist: lanes since then
        const uint64_t off_below = ~m & below_me;
        const unsigned s = off_below ? 64u - (unsigned)__builtin_clzll(off_below) : 0u;
        const unsigned dist = lane - s;
        uint32_t sp = on ? p : 0u, pk = sp;
        int32_t sr = on ? re : 0, si = on ? im : 0;
#pragma unroll
        for (unsigned off = 1; off < 64; off <<= 1) {
            const uint32_t tp = (uint32_t)__shfl_up((int)sp, off), tk = (uint32_t)__shfl_up((int)pk, off);
            const int32_t tr = __shfl_up(sr, off), ti = __shfl_up(si, off);
            if (on && dist >= off) {
                sp += tp;
                pk = max(pk, tk);
                sr += tr;
                si += ti;
            }
        }
        const bool carry_out = g0 + 64 < n_win && (m >> 63) != 0ull;  // (window g0 + 64 exists: the run may go on)
        uint64_t ends = m & ~(m >> 1);
        if (carry_out) ends &= ~(1ull << 63);
        if ((ends >> lane) & 1ull) {
            const bool joins = open && s == 0u;
            rd_burst r;
            r.channel = c;
            r.first = joins ? c_first : g0 + s;
            r.windows = (joins ? c_win : 0u) + dist + 1u;
            r.flags = (r.first == 0u ? 1u : 0u) | (w == n_win - 1u ? 2u : 0u);
            r.power = (joins ? c_pow : 0ull) + sp;
            r.peak = joins ? max(c_peak, pk) : pk;
            r.pad = 0u;
            r.corr_re = (joins ? c_re : 0) + sr;
            r.corr_im = (joins ? c_im : 0) + si;
            mine[n_done + (uint32_t)__builtin_popcountll(ends & below_me)] = r;
        }
        n_done += (uint32_t)__builtin_popcountll(ends);
        if (carry_out) {
            const unsigned s63 = (unsigned)__shfl((int)s, 63);
            const uint32_t sp63 = (uint32_t)__shfl((int)sp, 63), pk63 = (uint32_t)__shfl((int)pk, 63);
            const int32_t sr63 = __shfl(sr, 63), si63 = __shfl(si, 63);
            const bool joins = open && s63 == 0u;
            c_first = joins ? c_first : g0 + s63;
            c_win = (joins ? c_win : 0u) + 64u - s63;
            c_pow = (joins ? c_pow : 0ull) + sp63;
            c_peak = joins ? max(c_peak, pk63) : pk63;
            c_re = (joins ? c_re : 0) + sr63;
            c_im = (joins ? c_im : 0) + si63;
        }
        open = carry_out;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        off_n += (uint32_t)__shfl_xor((int)off_n, off);
        off_p += (uint64_t)__shfl_xor((unsigned long long)off_p, off);
        off_re += (int64_t)__shfl_xor((long long)off_re, off);
        off_im += (int64_t)__shfl_xor((long long)off_im, off);
    }
    if (lane == 0) {
        rd_burst_floor f;
        f.threshold = thr; f.windows_off = off_n; f.n_bursts = n_done; f.chunk = (uint32_t)seq;
        f.power_off = off_p; f.corr_re_off = off_re; f.corr_im_off = off_im;
        floor[c] = f;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
int rd_bursts_check(size_t n_out) {
    if (n_out == 0 || n_out % RD_BU_WINDOW)
        return rd_fail_msg(RD_ERR_ARG, "bursts: a chunk of %zu outputs is no whole number of %d-output windows", n_out, RD_BU_WINDOW);
    if (n_out / RD_BU_WINDOW > RD_BU_MAX_WINDOWS)
        return rd_fail_msg(RD_ERR_ARG, "bursts: %zu windows per chunk, at most %d (block_size <= %d)", n_out / RD_BU_WINDOW,
                           RD_BU_MAX_WINDOWS, RD_BU_MAX_WINDOWS * RD_BU_WINDOW);
    return RD_OK;
}

int rd_bursts_launch(const uint8_t *chan_out, size_t out_stride, int n_ch, size_t n_out, uint64_t seq, void *slot, hipStream_t st) {
    if (!chan_out || !slot || n_ch < 1) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = rd_bursts_check(n_out);
    if (rc) return rc;
    if (out_stride < 2 * n_out || (out_stride & 15) || ((uintptr_t)chan_out & 15) || ((uintptr_t)slot & 15))
        return rd_fail_msg(RD_ERR_ARG, "bursts: stride %zu for %zu outputs, or a misaligned buffer", out_stride, n_out);
    const size_t n_win = n_out / RD_BU_WINDOW;
    uint8_t *base = (uint8_t *)slot;
    hipLaunchKernelGGL(k_chan_bursts, dim3((unsigned)n_ch), dim3(RD_BU_THREADS), 0, st, (const uint4 *)chan_out, out_stride / 16,
                       (unsigned)n_win, (unsigned)rd_bu_cap(n_win), (const uint32_t *)(base + rd_bu_thr_offset(n_ch, n_win)), seq,
                       (rd_burst *)base, (rd_burst_floor *)(base + rd_bu_floor_offset(n_ch, n_win)));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "k_chan_bursts: %s", hipGetErrorString(e));
    return RD_OK;
}

// Test hook (tests/test_burst_kernels_crafted.py): k_chan_bursts alone on host bytes, through rd_bursts_launch and a
// mapped host slot as the receiver allocates it.  The slot is filled with 0xA5 before the launch and copied out whole -
// all cap record places of every channel -, so the caller sees which places the kernel left alone.
extern "C" int rd_debug_bursts(const uint8_t *chan, size_t stride, int n_ch, size_t n_out, const uint32_t *thr, uint64_t seq,
                               rd_burst *recs_out, rd_burst_floor *floor_out) {
    if (!chan || !thr || !recs_out || !floor_out || n_ch < 1) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = rd_bursts_check(n_out);
    if (rc) return rc;                               // (nothing allocated, nothing launched)
    if (stride < 2 * n_out || (stride & 15)) return rd_fail_msg(RD_ERR_ARG, "bursts: stride %zu for %zu outputs", stride, n_out);
    rc = rd_ensure_device();
    if (rc) return rc;
    const size_t n_win = n_out / RD_BU_WINDOW, bytes = rd_bu_slot_bytes(n_ch, n_win);
    uint8_t *d_chan = nullptr, *slot = nullptr;
    void *d_slot = nullptr;
#define RD_DBG_CHK(x) do { if ((x) != hipSuccess) { rc = rd_fail_msg(RD_ERR_DEVICE, "%s failed", #x); goto out; } } while (0)
    RD_DBG_CHK(hipMalloc(&d_chan, (size_t)n_ch * stride));
    RD_DBG_CHK(hipMemcpy(d_chan, chan, (size_t)n_ch * stride, hipMemcpyHostToDevice));
    RD_DBG_CHK(hipHostMalloc((void **)&slot, bytes, hipHostMallocMapped));
    memset(slot, 0xA5, bytes);
    memcpy(slot + rd_bu_thr_offset(n_ch, n_win), thr, (size_t)n_ch * sizeof(uint32_t));
    RD_DBG_CHK(hipHostGetDevicePointer(&d_slot, slot, 0));
    rc = rd_bursts_launch(d_chan, stride, n_ch, n_out, seq, d_slot, nullptr);
    if (rc) goto out;
    RD_DBG_CHK(hipDeviceSynchronize());
    memcpy(recs_out, slot, rd_bu_floor_offset(n_ch, n_win));
    memcpy(floor_out, slot + rd_bu_floor_offset(n_ch, n_win), (size_t)n_ch * sizeof(rd_burst_floor));
out:
#undef RD_DBG_CHK
    if (slot) hipHostFree(slot);
    if (d_chan) hipFree(d_chan);
    return rc;
}
