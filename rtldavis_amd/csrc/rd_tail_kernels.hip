// rd_tail_kernels.hip - the tail of a run as separate kernels: every shape but the Davis one, RD_TAIL_IMPL=legacy, the
// overflow fallback of k_tail (rd_tail.hip) and the streaming handles' multi-launch form; and the uint8 streaming block
// that does the same steps in one launch.
// Reference stages (py = the reference's src/rtldavis/dsp.py, go = its dsp/dsp.go):
//   k_fixup        : exact integer re-evaluation of the listed groups
//   k_search       : Demodulator._search py:171-188 (go:115-131) on packed bits, bit-parallel
//   k_classify + k_rssi_u8 : Demodulator._slice py:190-246 without the final order (the host orders), batch path, Davis shape
//   k_slice_rssi   : the same in one kernel everywhere else (rd_device.h: the complex ring's instance is launched from
//                    rd_stream_kernels.hip)
//   k_stream_block : one Demodulator.demodulate() call py:139-246 in one launch (streaming handle, uint8).  It stands here
//                    and not in rd_stream_kernels.hip because of what the compiler does: alone in a file with the helpers
//                    it shares with k_fixup and k_rssi_u8 (rd_exact_group_dw, the rd_rssi_* family) it is compiled to other
//                    instructions than beside them.
#include "rd_device.h"

uint32_t rd_launch_demod(const rd_layout &lay, uint32_t *fix_list, uint32_t fix_cap, uint32_t *counters, hipStream_t st,
                         hipEvent_t ev_start, hipEvent_t ev_stop, uint32_t flags, uint32_t *chunk_out, uint32_t *bucket_cnt) {
    if (!bucket_cnt) flags &= ~RD_DEMOD_FIX_BUCKETS;
    const int bucketed = rd_launch_demod_mfma(lay, fix_list, fix_cap, counters, st, ev_start, ev_stop, nullptr, flags, chunk_out, bucket_cnt);
    if (bucketed < 0) return RD_DEMOD_REFUSED;
    return bucketed ? RD_DEMOD_FIX_BUCKETS : 0u;
}

// ------------------------------------------------------------------------------------------
// k_fixup: exact bits for the listed runs (one lane per run).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fixup(rd_layout lay, uint32_t runs_per_stream, const uint32_t *fix_list,
                                               uint32_t fix_cap, const uint32_t *counters, int all,
                                               uint32_t *zero_next, uint32_t zero_words) {
    // the counters of the handle's NEXT run (double-buffered) are cleared here, saving a memset launch
    if (zero_next && blockIdx.x == 0)
        for (uint32_t i = threadIdx.x; i < zero_words; i += blockDim.x) zero_next[i] = 0;
    uint64_t count;
    if (all) {
        count = (uint64_t)lay.n_streams * runs_per_stream;
    } else {
        count = counters[RD_CNT_FIX];
        if (count > fix_cap) count = fix_cap;  // overflow is detected and handled by the host
    }
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        if (all) {  // every run, one output word each
            const uint32_t s = (uint32_t)(i / runs_per_stream);
            const uint32_t run = (uint32_t)(i - (uint64_t)s * runs_per_stream);
            const long t0 = (long)run * RD_RUN;
            const long left = (long)lay.n_samples - t0;
            lay.bits[(size_t)s * lay.bits_stride + run] = rd_exact_run(rd_view_of(lay, s), t0, left < RD_RUN ? (int)left : RD_RUN);
        } else {  // listed runs: word index << 4 | mask of the 8-sample groups to re-evaluate
            const uint32_t e = fix_list[i];
            const uint32_t widx = e >> 4;
            const uint32_t s = widx / (uint32_t)lay.bits_stride;
            const uint32_t run = widx - s * (uint32_t)lay.bits_stride;
            const rd_stream_view v = rd_view_of(lay, s);
            // Where the 39 us go (ablations): launch + list read 9, byte stores 6.5, IQ reads 11,
            // float64 arithmetic 14.  Tried and measured no faster: a per-lane "lowest flagged group
            // first" loop (25 % slower), expanding the entries into one (word, group) item per lane
            // through LDS (-2 us), reading the run's window from a
            // scratch area the demod kernel fills from its registers (same time; demod kernel +6 %).
            for (int g = 0; g < RD_GROUPS; g++) {
                if (!((e >> g) & 1)) continue;
                const long t0 = (long)run * RD_RUN + g * RD_GROUP;
                const long left = (long)lay.n_samples - t0;
                if (left <= 0) break;
                const int count = left < RD_GROUP ? (int)left : RD_GROUP;
                // samples t0-10 .. t0+9 = 40 bytes at a 4-byte aligned address: ten independent loads.
                // Dwords wholly before the first readable sample are not touched (no history there).
                const uint8_t *p = v.base + 2 * (t0 - 10);
                uint32_t dw[10];
                // dword d holds samples t0-10+2d and +1.  Readable: its last sample is at or after
                // valid_from (d >= floor(x / 2), x = valid_from - (t0-10)) and its first sample lies
                // before the input's padded end (d < ceil(z / 2), z = n_samples + 8 - (t0-10)).
                // Two 64-bit subtractions, then 32-bit compares against constants.
                const long x = v.valid_from - (t0 - 10), z = (long)lay.n_samples + 8 - (t0 - 10);
                const int d_lo = x <= 0 ? 0 : x >= 20 ? 10 : (int)(x / 2);
                const int d_hi = z <= 0 ? 0 : z >= 20 ? 10 : (int)((z + 1) / 2);
#pragma unroll
                for (int d = 0; d < 10; d++) dw[d] = (d >= d_lo && d < d_hi) ? *(const uint32_t *)(p + 4 * d) : 0u;
                ((uint8_t *)lay.bits)[(size_t)widx * 4 + g] = (uint8_t)rd_exact_group_dw(dw, t0, count, v.valid_from);
            }
        }
    }
}

void rd_launch_fixup(const rd_layout &lay, const uint32_t *fix_list, uint32_t fix_cap, uint32_t *counters, int all,
                     uint32_t *zero_next, hipStream_t st, uint32_t zero_words, uint64_t expect) {
    const uint32_t rps = (lay.n_samples + RD_RUN - 1) / RD_RUN;
    if (rps == 0 || lay.n_streams == 0) return;
    uint64_t want = all ? (uint64_t)lay.n_streams * rps : fix_cap;
    // a list that is 4 % full does not need a grid for all of it: 4096 workgroups of which 3400 find nothing to do
    // take longer to dispatch than the listed groups take to re-evaluate
    if (!all && expect > 0) want = std::min<uint64_t>(want, std::max<uint64_t>(expect + expect / 4, 256 * 256));
    uint64_t wgs = (want + 255) / 256;
    if (wgs > 256ull * 16) wgs = 256ull * 16;
    if (wgs == 0) wgs = 1;
    hipLaunchKernelGGL(k_fixup, dim3((unsigned)wgs), dim3(256), 0, st, lay, rps, fix_list, fix_cap, counters, all,
                       zero_next, zero_words);
}

// ------------------------------------------------------------------------------------------
// k_search: bit-parallel preamble match (py:171-188, go:115-131).
// match[p] = AND_k (bit[p + k*S] == preamble[k]).  One lane = 128 consecutive positions
// (4 output words); the words that cover them are loaded once and every tap is a funnel
// shift (v_alignbit_b32).  Persistent waves; matches are staged in LDS per wave and appended
// to the global list ~100 at a time (a single counter word sustains only ~90 atomics/us).
// ------------------------------------------------------------------------------------------

#define RD_MATCH_PEND 128   // staged matches per wave
#define RD_SEARCH_WAVES 4    // waves per workgroup (16 was tried to cut the end-of-kernel atomics: no gain)
#ifndef RD_SEARCH_UNROLL
#define RD_SEARCH_UNROLL 2
#endif

__device__ __forceinline__ void rd_flush_matches(const rd_match *pend, uint32_t count, rd_match *matches,
                                                 uint32_t match_cap, uint32_t *counters, int lane) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&counters[RD_CNT_MATCH], count);
    base = __builtin_amdgcn_readfirstlane(base);
    for (uint32_t i = lane; i < count; i += 64)
        if (base + i < match_cap) matches[base + i] = pend[i];
}

// S_ > 0: compile-time symbol length / preamble length (register funnel with constant
// shifts); S_ == 0: run-time cfg.S / cfg.P (words fetched per tap).
template <int S_, int P_, uint64_t PRE_>
__global__ __launch_bounds__(64 * RD_SEARCH_WAVES) void k_search(const uint32_t *bits, size_t bits_stride, int n_streams, long nwords,
                                                long base, long groups_per_stream, long p_lo, long p_hi,
                                                rd_devcfg cfg, rd_match *matches, uint32_t match_cap,
                                                uint32_t *counters) {
    __shared__ rd_match pend_all[RD_SEARCH_WAVES][RD_MATCH_PEND];
    const int lane = threadIdx.x & 63;
    rd_match *pend = pend_all[threadIdx.x >> 6];
    uint32_t npend = 0;  // wave-uniform
    // a wave covers 64 consecutive lane-groups (128 positions each) of ONE stream, so the
    // stream / group split is scalar arithmetic
    const uint32_t wgps = (uint32_t)((groups_per_stream + 63) / 64);  // wave-groups per stream
    const uint32_t nwave_groups = (uint32_t)n_streams * wgps;
    const uint32_t nwaves = gridDim.x * RD_SEARCH_WAVES;
    const uint32_t wave0 = __builtin_amdgcn_readfirstlane(blockIdx.x * RD_SEARCH_WAVES + (threadIdx.x >> 6));
    // RD_SEARCH_UNROLL wave-groups per trip: all their loads are issued before the first is used.
    // Everything per lane is 32-bit (positions and word indices of one stream fit), the stream /
    // group split of a wave-group is carried in scalars (no division in the loop): half of this
    // kernel's instructions used to be 64-bit index arithmetic and bounds tests.
    constexpr int NW = S_ > 0 ? ((RD_SEARCH_OUT + ((P_ > 0 ? P_ - 1 : 0) * (S_ > 0 ? S_ : 1) + 31) / 32 + 1 + 3) / 4) * 4 : 4;
    const int nwords_i = (int)nwords, gps = (int)groups_per_stream, plo = (int)p_lo, phi = (int)p_hi;
    const int base_i = (int)base, base_w = (int)(base >> 5);
    // 16-byte loads need every stream's words and the first word index 16-byte aligned
    const bool aligned16 = (bits_stride % 4 == 0) && (base_w % 4 == 0) && ((size_t)bits % 16 == 0);
    // wave-group wg = s * wgps + rem; a trip advances by step = nwaves * UNROLL, a slot by nwaves
    const uint32_t dq_n = nwaves / wgps, dr_n = nwaves % wgps;
    uint32_t s0 = wave0 / wgps, rem0 = wave0 % wgps;
    for (uint32_t wg0 = wave0; wg0 < nwave_groups; wg0 += nwaves * RD_SEARCH_UNROLL) {
        uint32_t r[RD_SEARCH_UNROLL][NW];
        uint32_t su[RD_SEARCH_UNROLL], remu[RD_SEARCH_UNROLL];
        {
            uint32_t sx = s0, rx = rem0;
#pragma unroll
            for (int u = 0; u < RD_SEARCH_UNROLL; u++) {
                su[u] = sx; remu[u] = rx;
                sx += dq_n; rx += dr_n;
                if (rx >= wgps) { rx -= wgps; sx++; }
            }
            s0 = sx; rem0 = rx;  // the next trip's first slot
        }
        if constexpr (S_ > 0) {
#pragma unroll
            for (int u = 0; u < RD_SEARCH_UNROLL; u++) {
                const uint32_t wg = wg0 + u * nwaves;
                if (wg >= nwave_groups) break;  // wave-uniform
                const int gi = (int)remu[u] * 64 + lane;
                const uint32_t *w = bits + (size_t)su[u] * bits_stride;
                const int w0 = base_w + RD_SEARCH_OUT * gi;
                if (aligned16 && gi < gps && w0 >= 0 && w0 + NW <= nwords_i) {
                    // interior: NW/4 coalesced 16-byte loads (lane i reads bytes 16i.. of the wave's span)
#pragma unroll
                    for (int j = 0; j < NW / 4; j++) {
                        const uint4 v4 = *(const uint4 *)(w + w0 + 4 * j);
                        r[u][4 * j] = v4.x; r[u][4 * j + 1] = v4.y; r[u][4 * j + 2] = v4.z; r[u][4 * j + 3] = v4.w;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < NW; j++) r[u][j] = gi < gps ? rd_word_at(w, nwords, (long)w0 + j) : 0u;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < RD_SEARCH_UNROLL; u++) {
            const uint32_t wg = wg0 + u * nwaves;
            if (wg >= nwave_groups) break;  // wave-uniform
            const uint32_t s = su[u];
            const int gi = (int)remu[u] * 64 + lane;
            uint32_t m[RD_SEARCH_OUT] = {};
            int p0 = 0;
            if (gi < gps) {
                p0 = base_i + 32 * RD_SEARCH_OUT * gi;
                const uint32_t *w = bits + (size_t)s * bits_stride;
#pragma unroll
                for (int o = 0; o < RD_SEARCH_OUT; o++) m[o] = 0xFFFFFFFFu;
                if constexpr (S_ > 0) {
                    // compile-time preamble: all[o] = AND of the taps that must be 1, any[o] = OR of
                    // the taps that must be 0 (two at a time with v_or3_b32); match = all & ~any
                    uint32_t any[RD_SEARCH_OUT] = {};
                    uint32_t held[RD_SEARCH_OUT];
                    bool have_held = false;
#pragma unroll
                    for (int k = 0; k < P_; k++) {
                        const int wj = (k * S_) >> 5, sh = (k * S_) & 31;
                        const bool one = (PRE_ >> k) & 1;
#pragma unroll
                        for (int o = 0; o < RD_SEARCH_OUT; o++) {
                            const uint32_t v = sh ? __builtin_amdgcn_alignbit(r[u][o + wj + 1], r[u][o + wj], sh) : r[u][o + wj];
                            if (one) m[o] &= v;
                            else if (have_held) any[o] = any[o] | held[o] | v;
                            else held[o] = v;
                        }
                        if (!one) have_held = !have_held;
                    }
#pragma unroll
                    for (int o = 0; o < RD_SEARCH_OUT; o++) {
                        if (have_held) any[o] |= held[o];
                        m[o] &= ~any[o];
                    }
                } else {
                    for (int k = 0; k < cfg.P; k++) {
                        const uint32_t x = ((cfg.pre_mask >> k) & 1) ? 0u : 0xFFFFFFFFu;
#pragma unroll
                        for (int o = 0; o < RD_SEARCH_OUT; o++)
                            m[o] &= rd_bits32_at(w, nwords, (long)p0 + 32 * o + (long)k * cfg.S) ^ x;
                    }
                }
                // keep positions inside [p_lo, p_hi]: only the first and the last words of a stream
                if (p0 < plo || p0 + 32 * RD_SEARCH_OUT - 1 > phi) {
#pragma unroll
                    for (int o = 0; o < RD_SEARCH_OUT; o++) {
                        const int q0 = p0 + 32 * o;
                        if (q0 < plo) m[o] &= (plo - q0 >= 32) ? 0u : (0xFFFFFFFFu << (plo - q0));
                        if (q0 + 31 > phi) m[o] &= (phi < q0) ? 0u : (0xFFFFFFFFu >> (31 - (phi - q0)));
                    }
                }
            }
#pragma unroll
            for (int o = 0; o < RD_SEARCH_OUT; o++) {
                uint32_t mm = m[o];
                uint64_t any = __ballot(mm != 0);
                while (any) {  // each round, every lane with matches left contributes its lowest one
                    const uint32_t nf = (uint32_t)__popcll(any);
                    if (npend + nf > RD_MATCH_PEND) {
                        rd_flush_matches(pend, npend, matches, match_cap, counters, lane);
                        npend = 0;
                    }
                    if (mm) {
                        const int bpos = __builtin_ctz(mm);
                        mm &= mm - 1;
                        rd_match e;
                        e.stream = (int32_t)s;
                        e.pos = (int32_t)(p0 + 32 * o + bpos);
                        pend[npend + __builtin_amdgcn_mbcnt_hi((uint32_t)(any >> 32),
                                                               __builtin_amdgcn_mbcnt_lo((uint32_t)any, 0))] = e;
                    }
                    npend += nf;
                    any = __ballot(mm != 0);
                }
            }
        }
    }
    // End of kernel: the workgroup's leftovers leave through ONE atomic (every wave flushing
    // its own few entries made 8192 serialized atomics = 90 us of a 110 us kernel).  What is
    // left is issue-bound: 64 funnel shifts (v_alignbit_b32, 4-cycle class) per 128 positions.
    __shared__ uint32_t left[RD_SEARCH_WAVES + 1];
    if (lane == 0) left[threadIdx.x >> 6] = npend;
    __syncthreads();
    if ((threadIdx.x >> 6) == 0) {
        // exclusive prefix of the wave counts (lane v < RD_SEARCH_WAVES holds wave v's)
        const uint32_t mine = lane < RD_SEARCH_WAVES ? left[lane] : 0u;
        uint32_t incl = mine;
#pragma unroll
        for (int o = 1; o < RD_SEARCH_WAVES; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        const uint32_t tot = __shfl(incl, RD_SEARCH_WAVES - 1, 64);
        if (tot) {
            uint32_t base_slot = 0;
            if (lane == 0) base_slot = atomicAdd(&counters[RD_CNT_MATCH], tot);
            base_slot = __builtin_amdgcn_readfirstlane(base_slot);
#pragma unroll 1
            for (int wv = 0; wv < RD_SEARCH_WAVES; wv++) {
                const uint32_t n = __shfl(mine, wv, 64), off = __shfl(incl - mine, wv, 64);
                for (uint32_t i = lane; i < n; i += 64)
                    if (base_slot + off + i < match_cap) matches[base_slot + off + i] = pend_all[wv][i];
            }
        }
    }
}

// k_search's workgroups per CU: 8 waves per SIMD unless the tuning knob RD_K2_WGS_PER_CU (1 - 64) says otherwise.
// Read once per process (function-local static: thread-safe first use).
static int rd_search_wgs_per_cu() {
    static const int cap = [] {
        const char *e = getenv("RD_K2_WGS_PER_CU");
        const int v = e ? atoi(e) : 32 / 4;
        return (v < 1 || v > 64) ? 32 / 4 : v;
    }();
    return cap;
}

void rd_launch_search(const uint32_t *bits, size_t bits_stride, int n_streams, long n_bits, long p_lo, long p_hi,
                      const rd_devcfg &cfg, rd_match *matches, uint32_t match_cap, uint32_t *counters,
                      hipStream_t st) {
    if (p_hi < p_lo || n_streams == 0) return;
    const long base = (p_lo >> 5) << 5;  // floor to a word boundary (p_lo may be negative)
    const long nwords = (n_bits + 31) / 32;
    const long groups = (p_hi - base) / (32 * RD_SEARCH_OUT) + 1;
    const uint64_t total = (uint64_t)n_streams * groups;
    uint64_t wgs = (total + 64 * RD_SEARCH_WAVES - 1) / (64 * RD_SEARCH_WAVES);
    const int cap = rd_search_wgs_per_cu();
    if (wgs > 256ull * cap) wgs = 256ull * cap;
    if (rd_davis_search(cfg))
        hipLaunchKernelGGL((k_search<14, 16, 0x91D3ull>), dim3((unsigned)wgs), dim3(64 * RD_SEARCH_WAVES), 0, st, bits, bits_stride,
                           n_streams, nwords, base, groups, p_lo, p_hi, cfg, matches, match_cap, counters);
    else
        hipLaunchKernelGGL((k_search<0, 0, 0>), dim3((unsigned)wgs), dim3(64 * RD_SEARCH_WAVES), 0, st, bits, bits_stride, n_streams,
                           nwords, base, groups, p_lo, p_hi, cfg, matches, match_cap, counters);
}

// ------------------------------------------------------------------------------------------
// The same work in two kernels for a compile-time (S, K) and the batch path: k_classify takes one LANE per match -
// the wave-per-match kernel above spends ~80 instructions and a chain of three memory latencies on a match that
// two times out of three is voided - and k_rssi one wave per SURVIVING packet (its two RSSI windows are 448 filter
// outputs).  A lane reads the words that hold its packet's K symbols for positions pos-1, pos, pos+1, shifts them
// to a common origin, and then everything is static: symbol k sits at bit k S + 1.
// ------------------------------------------------------------------------------------------
struct rd_task {
    uint32_t rec;     // record index (primary slot, or match_cap + extra slot)
    int32_t stream;
    int32_t call;     // reported by this call ...
    int32_t q;        // ... at this window index
};

template <int S_, int K_>
__global__ __launch_bounds__(256) void k_classify(const uint32_t *bits, size_t bits_stride, int nwords, rd_devcfg cfg,
                                                  const rd_match *matches, uint32_t match_cap, int n_calls,
                                                  rd_packet *recs, rd_task *tasks, uint32_t *counters) {
    constexpr int NBITS = (K_ - 1) * S_ + 3;          // bits pos-1 .. of the three packets
    constexpr int NU = (NBITS + 31) / 32;              // words of the aligned stream
    constexpr int NW = NU + 1;                         // words fetched (funnel)
    constexpr int NBYTES = (K_ + 7) / 8;
    static_assert(K_ % 8 == 0 && NBYTES <= RD_MAX_PKT_BYTES, "whole bytes only");
    __shared__ uint32_t s_tot[4], s_base;
    const int lane = threadIdx.x & 63;
    uint32_t count = counters[RD_CNT_MATCH];
    if (count > match_cap) count = match_cap;
    const uint32_t nthreads = gridDim.x * blockDim.x;
    // trips are uniform over the WORKGROUP (barriers inside): the workgroup's first index decides
    for (uint32_t g0 = blockIdx.x * blockDim.x; g0 < count; g0 += nthreads) {
        const uint32_t i = g0 + threadIdx.x;
        const bool live = i < count;
        int stream = 0, pos = 0;
        if (live) { stream = matches[i].stream; pos = matches[i].pos; }
        // calls that report this position (py:194, q <= B), as in k_slice_rssi
        const uint32_t pl = (uint32_t)(pos + cfg.L), bq = pl / (uint32_t)cfg.B, br = pl - bq * (uint32_t)cfg.B;
        const int b0 = (int)bq - 1;
        const int q0 = pos - ((b0 + 1) * cfg.B - cfg.L);
        const bool ok0 = live && b0 >= 0 && b0 < n_calls;
        const int b1 = b0 - 1, q1 = q0 + cfg.B;
        const bool ok1 = live && br == 0 && b1 >= 0 && b1 < n_calls;
        // words holding bits pos-1 ..: zero outside the array (rd_bits32_at_i)
        const uint32_t *w = bits + (size_t)stream * bits_stride;
        const int o = pos - 1, wi0 = o >> 5;
        const uint32_t sh = (uint32_t)(o & 31);
        uint32_t W[NW];
#pragma unroll
        for (int j = 0; j < NW; j++) {
            const int wi = wi0 + j;
            W[j] = (live && wi >= 0 && wi < nwords) ? w[wi] : 0u;
        }
        uint32_t u[NU];
#pragma unroll
        for (int j = 0; j < NU; j++) u[j] = __builtin_amdgcn_alignbit(W[j + 1], W[j], sh);
        // symbol k of position pos-1 / pos / pos+1 = bit k S / k S + 1 / k S + 2 of u.
        // y = u ^ (u >> 1): bit kS set <=> prev differs from cur, bit kS + 1 set <=> cur differs from next
        uint32_t dprev = 0, dnext = 0;
#pragma unroll
        for (int j = 0; j < NU; j++) {
            const uint32_t nxt = j + 1 < NU ? u[j + 1] : 0u;
            const uint32_t y = u[j] ^ __builtin_amdgcn_alignbit(nxt, u[j], 1);
            uint32_t mp = 0, mn = 0;  // static masks of this word
#pragma unroll
            for (int k = 0; k < K_; k++) {
                if (((k * S_) >> 5) == j) mp |= 1u << ((k * S_) & 31);
                if (((k * S_ + 1) >> 5) == j) mn |= 1u << ((k * S_ + 1) & 31);
            }
            dprev |= y & mp;
            dnext |= y & mn;
        }
        const bool same_prev = dprev == 0, same_next = dnext == 0;
        // the packet's bytes: byte bi = symbols 8 bi .. 8 bi + 7, first symbol = MSB (py:197-200)
        uint32_t dw[(NBYTES + 3) / 4];
#pragma unroll
        for (int m = 0; m < (NBYTES + 3) / 4; m++) dw[m] = 0;
#pragma unroll
        for (int k = 0; k < K_; k++) {
            const int bit = k * S_ + 1, bi = k >> 3;
            const uint32_t b = (u[bit >> 5] >> (bit & 31)) & 1u;
            dw[bi >> 2] |= b << (8 * (bi & 3) + 7 - (k & 7));
        }
        auto superseded = [&](int q) { return RD_SUPERSEDED(S_, q, cfg.B, same_prev, same_next); };
        const bool use0 = ok0 && !superseded(q0), use1 = ok1 && !superseded(q1);
        const int ntask = (use0 ? 1 : 0) + (use1 ? 1 : 0);  // records of this match: task t owns record t (dense)
        // task slots: ONE atomic per workgroup and trip (a counter word sustains ~90 atomics per microsecond: one per
        // wave was 12 of this kernel's 20 us).  All waves of a workgroup make the same number of trips.
        const uint32_t incl = rd_wave_incl_scan_u32((uint32_t)ntask, lane);
        const uint32_t tot = __shfl(incl, 63, 64);
        const int wv = threadIdx.x >> 6;
        __syncthreads();  // the previous trip's s_tot / s_base have been read
        if (lane == 0) s_tot[wv] = tot;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t sum = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) sum += s_tot[k];
            s_base = sum ? atomicAdd(&counters[RD_CNT_TASKS], sum) : 0u;
        }
        __syncthreads();
        uint32_t base = s_base;
#pragma unroll
        for (int k = 0; k < 4; k++) base += k < wv ? s_tot[k] : 0u;
        base = __builtin_amdgcn_readfirstlane(base);
        if (ntask) {
            uint32_t t = base + incl - (uint32_t)ntask;
            const int pb = use0 ? b0 : b1, pq = use0 ? q0 : q1;
            auto put = [&](uint32_t ri, int call, int q) {
                uint32_t *r = (uint32_t *)&recs[ri];
                const uint4 hdr = {(uint32_t)stream, (uint32_t)call, (uint32_t)q, (uint32_t)NBYTES};
                *(uint4 *)r = hdr;
                uint32_t d8[RD_MAX_PKT_BYTES / 4];
#pragma unroll
                for (int m = 0; m < RD_MAX_PKT_BYTES / 4; m++) d8[m] = m < (NBYTES + 3) / 4 ? dw[m] : 0u;
#pragma unroll
                for (int m = 0; m < RD_MAX_PKT_BYTES / 16; m++)
                    *(uint4 *)(r + 4 + 4 * m) = uint4{d8[4 * m], d8[4 * m + 1], d8[4 * m + 2], d8[4 * m + 3]};
                const rd_task tk = {ri, stream, call, q};
                tasks[t++] = tk;
            };
            put(t, pb, pq);
            if (use0 && use1) put(t, b1, q1);  // a position on a block boundary: reported by both calls
        }
    }
}

// One wave per surviving packet.  The task entry two steps ahead and the window bytes of the next step are
// fetched while the current packet's block runs on the matrix pipe: the kernel is a chain of latencies otherwise.
__global__ __launch_bounds__(256) void k_rssi_u8(rd_layout lay, rd_devcfg cfg, const rd_task *tasks, uint32_t task_cap,
                                                 rd_packet *recs, const uint32_t *counters) {
    const int lane = threadIdx.x & 63;
    const uint32_t nw = gridDim.x * (blockDim.x >> 6);
    const uint32_t i0 = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    rd_k_h8 Ahi[3], Alo[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        Ahi[d] = *(const rd_k_h8 *)g_rssi_taps.v[0][d][lane];
        Alo[d] = *(const rd_k_h8 *)g_rssi_taps.v[1][d][lane];
    }
    rd_task t_cur = {0, 0, 0, 0}, t_nxt = {0, 0, 0, 0};
    if (i0 < task_cap) t_cur = tasks[i0];                 // (any index below task_cap is readable)
    if (i0 + nw < task_cap) t_nxt = tasks[i0 + nw];
    uint32_t count = counters[RD_CNT_TASKS];
    if (count > task_cap) count = task_cap;
    auto view = [&](int stream) { return rd_view_of(lay, stream); };
    auto job_of = [&](const rd_task &t) {
        const int stream = __builtin_amdgcn_readfirstlane(t.stream), call = __builtin_amdgcn_readfirstlane(t.call),
                  q = __builtin_amdgcn_readfirstlane(t.q);
        return rd_rssi_prepare(view(stream), call * cfg.B, cfg, q, lane);
    };
    rd_rssi_job j_cur = {};
    rd_rssi_data d_cur = {};
    if (i0 < count) {
        j_cur = job_of(t_cur);
        if (j_cur.ok) d_cur = rd_rssi_fetch(j_cur);
    }
    for (uint32_t i = i0; i < count; i += nw) {
        const rd_task t_now = t_cur;
        const rd_rssi_job j_now = j_cur;
        const rd_rssi_data d_now = d_cur;
        // next step's bytes, the entry after that
        if (i + nw < count) {
            j_cur = job_of(t_nxt);
            if (j_cur.ok) d_cur = rd_rssi_fetch(j_cur);
        }
        t_cur = t_nxt;
        if (i + 2 * nw < task_cap) t_nxt = tasks[i + 2 * nw];
        const uint32_t rec = __builtin_amdgcn_readfirstlane(t_now.rec);
        double rssi = 0.0, snr = 0.0;
        if (j_now.ok) {
            float noise, sig;
            rd_rssi_block(j_now, d_now, Ahi, Alo, lane, noise, sig);
            rd_rssi_finish(noise, sig, j_now.ns, j_now.pe, j_now.q, lane, rssi, snr);
        } else {  // a window that reaches outside the stream: the fp32 path with its per-sample checks
            const int stream = __builtin_amdgcn_readfirstlane(t_now.stream);
            rd_rssi_u8(view(stream), (long)__builtin_amdgcn_readfirstlane(t_now.call) * cfg.B, cfg,
                       (long)__builtin_amdgcn_readfirstlane(t_now.q), lane, rssi, snr);
        }
        if (lane == 0) { recs[rec].rssi = rssi; recs[rec].snr = snr; }
    }
}

int rd_launch_slice(const rd_layout &lay, const uint32_t *bits, size_t bits_stride, long n_bits, const rd_devcfg &cfg,
                    const rd_match *matches, uint32_t match_cap, int batch_mode, int n_calls, int call,
                    rd_packet *recs, rd_packet *recs_host, uint32_t *counters, hipStream_t st, hipEvent_t ev_stop,
                    void *tasks) {
    rd_u8_src src;
    src.lay = lay;
    // the Davis shape in the batch path: lane-per-match classification, then one wave per surviving packet
    if (tasks && batch_mode && recs && !recs_host && rd_davis_slice(cfg) && n_bits < (1l << 30)) {
        const uint32_t cg = std::min<uint32_t>((match_cap + 255) / 256, 1024);
        hipLaunchKernelGGL((k_classify<14, 80>), dim3(cg ? cg : 1), dim3(256), 0, st, bits, bits_stride,
                           (int)((n_bits + 31) / 32), cfg, matches, match_cap, n_calls, recs, (rd_task *)tasks, counters);
        // one resident generation of waves (4 per SIMD): each works through its ~6 packets with the next one's
        // bytes in flight; a larger grid means generations of waves that each pay the whole latency chain
        const uint32_t rg = std::min<uint32_t>(rd_slice_grid(match_cap), 1024);
        rd_launch_ev(k_rssi_u8, dim3(rg), dim3(256), 0, st, ev_stop, lay, cfg, (const rd_task *)tasks, 2 * match_cap, recs, counters);
        return 1;  // records: one per task, dense from index 0 (RD_CNT_TASKS of them)
    }
    rd_launch_ev(k_slice_rssi<rd_u8_src>, dim3(rd_slice_grid(match_cap)), dim3(256), 0, st, ev_stop, src, bits, bits_stride,
                 (n_bits + 31) / 32, cfg, matches, match_cap, batch_mode, n_calls, call, recs, recs_host, counters);
    return 0;  // records: one slot per match (RD_CNT_MATCH, void ones marked) + the block-boundary twins behind match_cap
}

// ------------------------------------------------------------------------------------------
// k_stream_block: ONE launch per demodulate() call of the streaming handle (py:139-246 for one block per stream).
// The multi-launch form (copy, three ring copies, memset, demod, fix-up, window update, search, slice, counter copy,
// event) spends 70 us on launch overheads and idle gaps for 16 KB of input; here one workgroup per stream does it all:
//   0  roll the raw ring (py:140,154) and take the new block straight from pinned host memory
//   1  the block's sign bits, EXACTLY (rd_exact_group_dw, one 8-sample group per thread: 8192 samples need no fast path)
//   2  quantized window = previous block's bits | new bits (py:157,163-166), kept in LDS and written out for the mirrors
//   3  preamble search over positions 0 .. B (py:171-188, q <= B: py:194)
//   4  slice + RSSI / SNR, one wave per match (py:190-246), records into mapped host memory
//   5  per stream: match count, then - behind a system-scope fence - the sequence number the host polls for
// Production shape class only (compile-time S, P, K; buffer_length = 2 block_size; block_size a multiple of 32, at most
// 16384): everything else keeps the multi-launch form.  Every position 0 .. B can be a match (a degenerate input makes
// it so): the match list in LDS and the stream's region of the mapped record array hold B + 1 entries.
// ------------------------------------------------------------------------------------------
template <int S_, int P_, uint64_t PRE_, int K_>
__global__ __launch_bounds__(RD_SB_THREADS) void k_stream_block(rd_sb_args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t sb_lds[];
    const int B = a.cfg.B, nwin = (2 * B) / 32, nbw = B / 32;
    uint8_t *s_iq = sb_lds;                                      // samples -16 .. B-1 as bytes: 32 + 2 B
    uint32_t *s_win = (uint32_t *)(sb_lds + 32 + 2 * (size_t)B);  // the 2 B-bit window
    int32_t *s_match = (int32_t *)(s_win + nwin);                // B + 1 positions
    __shared__ uint32_t s_nm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int stream = blockIdx.x;
    uint8_t *ring = a.ring + (size_t)stream * a.ring_stride;     // [hdr 32 B][previous block][newest block]
    const uint8_t *in = a.in + (size_t)stream * 2 * (size_t)B;
    const bool have_hist = a.seen_before > 0;
    RD_SB_STAMP(0);
    if (tid == 0) s_nm = 0;
    // ---- 0: the roll.  Every load first (two 16-byte pieces per thread cover 2 B <= 32 KiB), then a barrier, then the
    // stores: the old newest block is read whole before it is overwritten, the old previous block's tail before the old
    // newest block lands on it.
    const int pieces = (2 * B) / 16;
    uint4 nw[2], oc[2], ph = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int i = tid + RD_SB_THREADS * k;
        nw[k] = uint4{0, 0, 0, 0}; oc[k] = uint4{0, 0, 0, 0};
        if (i < pieces) {
            nw[k] = *(const uint4 *)(in + 16 * (size_t)i);  // pinned host memory
            if (have_hist) oc[k] = *(const uint4 *)(ring + 32 + 2 * (size_t)B + 16 * (size_t)i);
        }
    }
    if (have_hist && tid < 2) ph = *(const uint4 *)(ring + 2 * (size_t)B + 16 * (size_t)tid);  // last 32 bytes of the old previous block
    // the previous block's bits: the upper half of the old window becomes the lower half of the new one
    const uint32_t *win_in = a.win_in + (size_t)stream * nwin;
    uint32_t *win_out = a.win_out + (size_t)stream * nwin;
    uint32_t oldw = 0;
    if (tid < nbw) oldw = win_in[nbw + tid];
    __syncthreads();
    RD_SB_STAMP(1);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int i = tid + RD_SB_THREADS * k;
        if (i < pieces) {
            *(uint4 *)(ring + 32 + 2 * (size_t)B + 16 * (size_t)i) = nw[k];
            *(uint4 *)(s_iq + 32 + 16 * (size_t)i) = nw[k];
            if (have_hist) {
                *(uint4 *)(ring + 32 + 16 * (size_t)i) = oc[k];
                if (i >= pieces - 2) *(uint4 *)(s_iq + 16 * (i - (pieces - 2))) = oc[k];  // samples -16 .. -1
            }
        }
    }
    if (have_hist && tid < 2) *(uint4 *)(ring + 16 * (size_t)tid) = ph;
    if (!have_hist && tid < 2) *(uint4 *)(s_iq + 16 * tid) = uint4{0, 0, 0, 0};
    if (tid < nbw) s_win[tid] = oldw;
    rd_barrier_lds();   // (LDS only: the ring stores drain under the arithmetic - 2 us of waiting for their acknowledgement
                        // otherwise; the barriers in front of the slice, which reads the ring, wait for them)
    RD_SB_STAMP(2);
    // ---- 1: exact sign bits, one 8-sample group per thread (dsp.py:38-98 in exact integer arithmetic) ----
    const long vfrom = have_hist ? -16 : 0;  // (ten samples of history are all a group needs)
    for (int g = tid; g < B / 8; g += RD_SB_THREADS) {
        const int t0 = 8 * g;
        uint32_t dw[10];
#pragma unroll
        for (int d = 0; d < 10; d++) {
            const int smp = t0 - 10 + 2 * d;  // first sample of the dword
            dw[d] = (smp + 1 >= -16 && smp + 1 < B) ? *(const uint32_t *)(s_iq + 32 + 2 * smp) : 0u;
        }
        ((uint8_t *)(s_win + nbw))[g] = (uint8_t)rd_exact_group_dw(dw, (long)t0, 8, vfrom);
    }
    __syncthreads();
    RD_SB_STAMP(3);
    // ---- 2: the window goes out for the state mirrors (rd_copy_quantized) and the next call ----
    for (int i = tid; i < nwin; i += RD_SB_THREADS) win_out[i] = s_win[i];
    // ---- 3: search, one 32-position word per thread; positions 0 .. B ----
    rd_window_search<S_, P_, PRE_>(s_win, nwin, nbw, tid, RD_SB_THREADS, &s_nm, s_match);
    __syncthreads();
    RD_SB_STAMP(4);
    const uint32_t nm = s_nm;
    // ---- 4: slice + RSSI / SNR, one wave per match (k_slice_rssi's logic for batch_mode = 0) ----
    rd_packet *recs = a.recs_host + (size_t)stream * (size_t)(B + 1);
    int32_t *fe = a.fe_host + (size_t)stream * (size_t)(B + 1);   // (used with a.parse only)
    rd_stream_view v;
    v.base = ring + 32 + 2 * (size_t)B;
    v.valid_from = RD_SB_VALID_FROM(a.seen_before, B);
    v.n = B;
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // the ring stores above are read below (same CU)
        for (uint32_t i = (uint32_t)wave; i < nm; i += RD_SB_THREADS / 64) {
            const int pos = __builtin_amdgcn_readfirstlane(s_match[i]);
            uint32_t byte = 0;
            bool same_prev = true, same_next = true;
#define RD_BITS3(o) rd_lds_bits32(s_win, nwin, (o))
            RD_WAVE_BYTES(K_, S_, pos, lane, RD_BITS3, byte, same_prev, same_next);
#undef RD_BITS3
            const bool superseded = RD_SUPERSEDED(S_, pos, B, same_prev, same_next);
            if (superseded) {
                rd_store_void(nullptr, &recs[i], lane);
                if (a.parse && lane == 0) fe[i] = RD_FE_NONE;
                continue;
            }
            double rssi = 0.0, snr = 0.0;
            rd_rssi_u8(v, 0, a.cfg, (long)pos, lane, rssi, snr);
            rd_store_record(nullptr, &recs[i], lane, stream, (long)a.seen_before, (long)pos, a.cfg.nbytes, byte, rssi, snr);
            if (a.parse) {   // Parser.parse's front half for this packet (rd_wave_parse); step 5's release covers the store
                const int32_t e = rd_wave_parse(v, a.cfg, (long)pos, byte, lane);
                if (lane == 0) fe[i] = e;
            }
        }
    }
    // ---- 5: count, fence, flag ----
    __syncthreads();
    if (tid == 0) {
        a.cnt_host[stream] = nm;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope: records and count before the flag
        __hip_atomic_store(&a.flag_host[stream], a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    RD_SB_STAMP(5);
}

int rd_launch_stream_block(const rd_sb_args &a_in, int n_streams, hipStream_t st) {
    const rd_devcfg &c = a_in.cfg;
    if (!rd_davis_shape(c) || c.L != 2 * c.B || c.B % 32 || c.B < 2048 || c.B > 16384)
        return 0;
    rd_sb_args a = a_in;
    a.stamps = nullptr;
#ifdef RD_DIAG
    a.stamps = rd_sb_stamp_buffer();
#endif
    const size_t lds = 32 + 2 * (size_t)c.B + (size_t)(2 * c.B / 32) * 4 + ((size_t)c.B + 1) * 4;
    hipLaunchKernelGGL((k_stream_block<14, 16, 0x91D3ull, 80>), dim3((unsigned)n_streams), dim3(RD_SB_THREADS), lds, st, a);
    return 1;
}
