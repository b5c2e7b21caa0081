// rd_stream_kernels.hip - the streaming handle's kernels (host side: rd_stream.hip):
//   k_stream_block_cplx          : one Demodulator.demodulate() call py:139-246 in one launch, complex input (the uint8
//                                  form, k_stream_block: rd_tail_kernels.hip)
//   k_window_update, k_cplx_bits : the multi-launch form's own steps and its slice of the complex ring (its other kernels
//                                  are the batch path's: rd_tail_kernels.hip, rd_parse_kernels.hip)
// py = the reference's src/rtldavis/dsp.py
#include "rd_device.h"

// the multi-launch form's slice of the complex ring: k_slice_rssi (rd_device.h) reading its RSSI windows in float64
void rd_launch_cplx_slice(const rd_cplx_layout &lay, const uint32_t *bits, long n_bits, const rd_devcfg &cfg,
                          const rd_match *matches, uint32_t match_cap, int call, rd_packet *recs, rd_packet *recs_host,
                          uint32_t *counters, hipStream_t st) {
    rd_cplx_src src;
    src.v = rd_cplx_view_of(lay);
    hipLaunchKernelGGL(k_slice_rssi<rd_cplx_src>, dim3(rd_slice_grid(match_cap)), dim3(256), 0, st, src, bits,
                       (size_t)0, (n_bits + 31) / 32, cfg, matches, match_cap, 0, 0, call, recs, recs_host, counters);
}

// ------------------------------------------------------------------------------------------
// streaming search window: out = (in >> n_block_bits) | (block << (n_win_bits - n_block_bits))
// i.e. np.roll(quantized, -B) followed by writing the newest block at the end (py:157,163-166)
// ------------------------------------------------------------------------------------------
__global__ void k_window_update(uint32_t *out, const uint32_t *in, long n_win_bits, const uint32_t *block,
                                long n_block_bits, size_t win_stride, size_t block_stride) {
    const long nw = (n_win_bits + 31) / 32;
    const long nbw = (n_block_bits + 31) / 32;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nw) return;
    out += (size_t)blockIdx.y * win_stride;  // one stream per grid row
    in += (size_t)blockIdx.y * win_stride;
    block += (size_t)blockIdx.y * block_stride;
    const long keep = n_win_bits - n_block_bits;  // bits [0, keep) come from the old window
    const long o = 32 * i;
    const uint32_t oldv = rd_bits32_at(in, nw, o + n_block_bits);
    const uint32_t newv = rd_bits32_at(block, nbw, o - keep);
    uint32_t mask_old;
    if (o + 32 <= keep) mask_old = 0xFFFFFFFFu;
    else if (o >= keep) mask_old = 0u;
    else mask_old = (1u << (keep - o)) - 1u;
    uint32_t word = (oldv & mask_old) | (newv & ~mask_old);
    const long left = n_win_bits - o;
    if (left < 32) word &= (1u << left) - 1u;
    out[i] = word;
}

void rd_launch_window_update(uint32_t *win_out, const uint32_t *win_in, long n_win_bits, const uint32_t *block,
                             long n_block_bits, int n_streams, size_t win_stride, size_t block_stride,
                             hipStream_t st) {
    const long nw = (n_win_bits + 31) / 32;
    hipLaunchKernelGGL(k_window_update, dim3(rd_grid256(nw).x, (unsigned)n_streams), dim3(256), 0, st,
                       win_out, win_in, n_win_bits, block, n_block_bits, win_stride, block_stride);
}

#ifdef RD_DIAG
// diagnostic library: the stamps of the streaming blocks' phases (RD_SB_STAMP, rd_device.h)
static uint64_t *g_sb_stamps = nullptr;
uint64_t *rd_sb_stamp_buffer() {
    if (!getenv("RD_SB_STAMPS")) return nullptr;
    if (!g_sb_stamps && (hipMalloc(&g_sb_stamps, 64) != hipSuccess || hipMemset(g_sb_stamps, 0, 64) != hipSuccess)) g_sb_stamps = nullptr;
    return g_sb_stamps;
}
// stamps of the last streaming one-launch block (diagnostic library): 8 uint64 (s_memrealtime, 100 MHz)
extern "C" int rd_diag_read_sb_stamps(uint64_t *out) {
    if (!g_sb_stamps || !out) return RD_ERR_STATE;
    if (hipDeviceSynchronize() != hipSuccess) return RD_ERR_DEVICE;
    return hipMemcpy(out, g_sb_stamps, 64, hipMemcpyDeviceToHost) == hipSuccess ? RD_OK : RD_ERR_DEVICE;
}
#endif

// ------------------------------------------------------------------------------------------
// k_stream_block_cplx: the same ONE launch for the complex-input branch (py:144-150) - what pyrtlsdr's sdr.stream()
// feeds the live receiver (/root/reference/src/rtldavis/runners/rtlsdr.py:100-103).  Single stream; the raw ring holds
// complex128 [hdr 16][previous block][newest block]; the new block comes from the slot's mapped host buffer as
// complex128 (16 bytes per sample) or - a uint8 block on a handle that has seen complex input - as bytes through the
// LUT (py:26,38-39).  The block is 128 KB over the link: ONE workgroup asked for it at 10.7 GB/s (12 of its 19 us;
// a CU has only so many reads in flight), so block_size / (8 T) workgroups of T threads each take 8 T samples:
//   0  every load of the piece at once: the new samples from pinned host memory, the old newest block from the ring
//      (py:140,154: the roll); the 16 samples in front of the piece for the filter's history
//   1  ring stores (they drain under the arithmetic) and the ROTATED samples (py:46-49) into LDS, sample i in 16-byte
//      chunk i + i/8: a thread of step 2 reads the 17 consecutive samples of its 8-sample group, lanes 8 samples apart
//      = chunk stride 9, no bank asked twice (the same loads from global memory touched 64 cache lines per instruction)
//   2  signs from a float64 sum in tap order (rd_f_f64's), one 8-sample group per thread.  The sign of py:80-90's
//      quotient is the sign of its numerator - the denominator is a sum of squares + 1e-10 - so no float64 divide
//      (finite input; a NaN numerator has no sign to agree on)
//   3  the piece's sign words into the window; then the workgroup counts itself in.  The LAST one to arrive goes on
//      alone: window, search, slice, RSSI / SNR, records, flag (k_stream_block's steps 2 - 5)
// What one workgroup writes and another reads in the same launch: the window's words travel as relaxed agent-scope
// atomics (sc1: written through to, read from the level all XCDs share); the ring (the RSSI windows reach into other
// pieces and the previous block) is written with plain stores and ONE agent-scope release per wave in front of the
// workgroup's increment of the arrival counter (a write-back of this XCD's few dirty L2 lines: 0.6 us; the same ring as
// 32 write-through stores per thread took 6 us of issue) and read by the last workgroup with sc1 loads.  Nobody waits
// for anybody: a workgroup that is not the last simply ends.  The ring's last 16 samples (next block's filter
// history, and what the header copies) are read AND written by workgroup 0 only, whichever piece they belong to: no
// other workgroup's store can land on them before they are read.
// ------------------------------------------------------------------------------------------
RD_HD int rd_sbc_chunk(int slot) { return slot + (slot >> 3); }   // (slot = sample - piece start + 16)

__device__ __forceinline__ double rd_load_coh(const double *p) {
    return __builtin_bit_cast(double, __hip_atomic_load((const uint64_t *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// the complex ring as the last workgroup has to read it (rd_sample_f64 of rd_math.h with coherent loads)
struct rd_cplx_coh_view {
    const double *base;  // sample 0 of the newest block
    long valid_from;
    long n;
};
__device__ __forceinline__ rd_d2 rd_sample_f64(const rd_cplx_coh_view &v, long n) {
    rd_d2 y = {0.0, 0.0};
    if (n < v.valid_from) return y;
    return rd_rot_f64(rd_load_coh(v.base + 2 * n), rd_load_coh(v.base + 2 * n + 1), n);
}

template <int S_, int P_, uint64_t PRE_, int K_>
__global__ __launch_bounds__(RD_SBC_THREADS) void k_stream_block_cplx(rd_sbc_args a) {
    constexpr int T = RD_SBC_THREADS, C = 8 * T, PER = 8;
    extern __shared__ __attribute__((aligned(16))) uint8_t sb_lds[];
    const int B = a.cfg.B, nwin = (2 * B) / 32, nbw = B / 32;
    uint32_t *s_win = (uint32_t *)sb_lds;           // the 2 B-bit window (the last workgroup)
    uint4 *s_y = (uint4 *)(s_win + nwin);           // rotated samples -16 .. C-1 of the piece, padded (rd_sbc_chunk)
    int32_t *s_match = (int32_t *)s_y;              // B + 1 positions: over the samples, once the signs are made
    __shared__ uint32_t s_nm, s_last;
    __shared__ __attribute__((aligned(4))) uint8_t s_bytes[T];
    __shared__ double s_part[2][2][T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = blockIdx.x, NW = gridDim.x, s0 = w * C;
    double *ring = a.ring;                          // [hdr 32 doubles][previous block 2 B][newest block 2 B]
    uint4 *r_hdr = (uint4 *)ring, *r_prev = (uint4 *)(ring + 32), *r_cur = (uint4 *)(ring + 32 + 2 * (size_t)B);  // one uint4 = one sample
    const bool have_hist = a.seen_before > 0;
    if (w == 0) RD_SB_STAMP(0);
    struct smp { uint64_t re, im; };   // one complex128 sample as bit patterns
    const int in_is_u8 = a.in_is_u8;
    const void *in = a.in;
    auto fetch_in = [in, in_is_u8](int i) -> smp {
        if (in_is_u8) {  // py:26,38-39
            const uint8_t *q = (const uint8_t *)in + 2 * (size_t)i;
            const double re = ((double)q[0] - 127.4) / 127.6, im = ((double)q[1] - 127.4) / 127.6;
            return smp{__builtin_bit_cast(uint64_t, re), __builtin_bit_cast(uint64_t, im)};
        }
        const uint4 r = ((const uint4 *)in)[i];  // pinned host memory
        return smp{((uint64_t)r.y << 32) | r.x, ((uint64_t)r.w << 32) | r.z};
    };
    auto fetch_ring = [](const uint4 *p) -> smp {
        const uint4 r = *p;
        return smp{((uint64_t)r.y << 32) | r.x, ((uint64_t)r.w << 32) | r.z};
    };
    auto store_coh = [](uint4 *p, smp v) {   // (plain 16-byte store: the release fence in front of the count writes the L2 back)
        *p = uint4{(uint32_t)v.re, (uint32_t)(v.re >> 32), (uint32_t)v.im, (uint32_t)(v.im >> 32)};
    };
    auto rotated = [](smp x, int n) -> uint4 {  // py:46-49, x * j^(n mod 4) (rd_rot_f64), on the bit patterns: a negation flips bit 63
        const uint64_t neg = 1ull << 63;
        const int ph = n & 3;
        const uint64_t re = ph == 0 ? x.re : ph == 1 ? x.im ^ neg : ph == 2 ? x.re ^ neg : x.im;
        const uint64_t im = ph == 0 ? x.im : ph == 1 ? x.re : ph == 2 ? x.im ^ neg : x.re ^ neg;
        return uint4{(uint32_t)re, (uint32_t)(re >> 32), (uint32_t)im, (uint32_t)(im >> 32)};
    };
    // ---- 0: the piece's loads, all of them before the first store ----
    const uint4 zero4 = {0, 0, 0, 0};
    const smp zero = {0, 0};
    smp nw[PER], oc[PER], tl_new = zero, tl_old = zero, ph = zero, hist = zero;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int i = s0 + tid + T * k;
        nw[k] = zero; oc[k] = zero;
        if (i < B) {
            nw[k] = fetch_in(i);
            if (have_hist && i < B - 16) oc[k] = fetch_ring(&r_cur[i]);
        }
    }
    if (tid < 16) {
        if (w == 0) {
            tl_new = fetch_in(B - 16 + tid);
            if (have_hist) { tl_old = fetch_ring(&r_cur[B - 16 + tid]); ph = fetch_ring(&r_prev[B - 16 + tid]); }
            hist = tl_old;                      // (zeros without history: the zero state of py:133)
        } else {
            hist = fetch_in(s0 - 16 + tid);     // (the neighbour's samples, once more over the link)
        }
    }
    const int wj = s0 / 32 + tid;               // this thread's word of the piece (tid < C / 32)
    uint32_t oldw = 0;
    if (tid < C / 32 && wj < nbw) oldw = a.win_in[nbw + wj];
    // ---- 1: the old newest block moves down (it has been here a while), the new block follows as the link delivers it.
    // A thread overwrites only what it has read itself.
    if (have_hist) {
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int i = s0 + tid + T * k;
            if (i < B - 16) store_coh(&r_prev[i], oc[k]);
        }
    }
    if (tid < 16) s_y[rd_sbc_chunk(tid)] = (w > 0 || have_hist) ? rotated(hist, s0 - 16 + tid) : zero4;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int i = s0 + tid + T * k;
        if (i < B) {
            if (i < B - 16) store_coh(&r_cur[i], nw[k]);
            s_y[rd_sbc_chunk(i - s0 + 16)] = rotated(nw[k], i);
        }
    }
    if (w == 0 && tid < 16) {
        if (have_hist) { store_coh(&r_hdr[tid], ph); store_coh(&r_prev[B - 16 + tid], tl_old); }
        store_coh(&r_cur[B - 16 + tid], tl_new);
    }
    if (tid < C / 32 && wj < nbw) __hip_atomic_store(&a.win_out[wj], oldw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    rd_barrier_lds();   // (LDS only: the ring stores drain under the arithmetic)
    if (w == 0) RD_SB_STAMP(1);
    // ---- 2: sign bits in float64, one 8-sample group per thread (py:52-98; taps summed in order m = 0..8) ----
    {
        const int t0 = s0 + 8 * tid;
        uint32_t byte = 0;
        if (t0 < B) {
            const double c[9] = RD_TAPS9;
            rd_d2 y[17];
#pragma unroll
            for (int i = 0; i < 17; i++) {  // samples t0 - 10 + i
                const uint4 x = s_y[rd_sbc_chunk(8 * tid + 6 + i)];
                y[i].x = __builtin_bit_cast(double, uint2{x.x, x.y});
                y[i].y = __builtin_bit_cast(double, uint2{x.z, x.w});
            }
            rd_d2 prev = {0.0, 0.0};
#pragma unroll
            for (int j = 0; j < 9; j++) {  // f[t0 - 1 + j]
                rd_d2 f = {0.0, 0.0};
                if (have_hist || t0 - 1 + j >= 0) {
#pragma unroll
                    for (int m = 0; m < 9; m++) {
                        f.x += c[m] * y[j + m].x;
                        f.y += c[m] * y[j + m].y;
                    }
                }
                if (j > 0) byte |= rd_signbit_f64(prev.y * f.x - prev.x * f.y) << (j - 1);   // (py:80-90: the numerator's sign)
                prev = f;
            }
        }
        s_bytes[tid] = (uint8_t)byte;
    }
    rd_barrier_lds();
    if (w == 0) RD_SB_STAMP(2);
    // ---- 3: the piece's words, then the count ----
    if (tid < C / 32 && wj < nbw)
        __hip_atomic_store(&a.win_out[nbw + wj], ((const uint32_t *)s_bytes)[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the piece's ring stores are plain stores into this XCD's L2: one agent-scope release per wave (a write-back of the
    // L2's dirty lines - few here - and a wait for every store) puts them where the last workgroup's sc1 loads read.
    // (32 write-through stores per thread instead cost 6 us of issue: the vector memory queue backs up behind them.)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if (tid == 0) {
        const uint32_t before = __hip_atomic_fetch_add(a.sync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = before + 1u == (uint32_t)NW ? 1u : 0u;
        s_nm = 0;
    }
    __syncthreads();
    if (w == 0) RD_SB_STAMP(3);
    if (!s_last) return;
    // ---- the last workgroup: the window (every piece's words are in place), for the mirrors it is already out ----
    if (tid == 0) __hip_atomic_store(a.sync, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (the next launch counts from 0)
    for (int i = tid; i < nwin; i += T) s_win[i] = __hip_atomic_load(&a.win_out[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    RD_SBL_STAMP(4);
    // ---- search, one 32-position word per thread; positions 0 .. B ----
    rd_window_search<S_, P_, PRE_>(s_win, nwin, nbw, tid, T, &s_nm, s_match);
    __syncthreads();
    RD_SBL_STAMP(5);
    const uint32_t nm = s_nm;
    // ---- slice: a wave per match decides whether the match is superseded (a neighbour's identical bytes come first) ----
    rd_packet *recs = a.recs_host;
    auto bytes_of = [&](int pos, bool &superseded) -> uint32_t {   // lane bi < 10: byte bi of the packet at `pos`
        uint32_t byte = 0;
        bool same_prev = true, same_next = true;
#define RD_BITS3(o) rd_lds_bits32(s_win, nwin, (o))
        RD_WAVE_BYTES(K_, S_, pos, lane, RD_BITS3, byte, same_prev, same_next);
#undef RD_BITS3
        superseded = RD_SUPERSEDED(S_, pos, B, same_prev, same_next);
        return byte;
    };
    for (uint32_t i = (uint32_t)wave; i < nm; i += T / 64) {
        const int pos = __builtin_amdgcn_readfirstlane(s_match[i]);
        bool superseded;
        (void)bytes_of(pos, superseded);
        if (superseded) {
            rd_store_void(nullptr, &recs[i], lane);
            if (lane == 0) s_match[i] = pos | 0x40000000;
            if (a.parse && lane == 0) a.fe_host[i] = RD_FE_NONE;
        }
    }
    __syncthreads();
    // ---- RSSI / SNR of the others, one after the other, the whole workgroup on each (rd_rssi_f64's sums: |f|^2 over
    // [q - PL, q) and [q, q + PL), clipped to the newest block's filtered outputs, py:216-246).  A thread takes NINE
    // consecutive outputs: their 17 samples are asked for at once and slide through the taps - one round trip to where
    // the other workgroups' ring stores went, where an output per lane and trip (rd_rssi_f64) makes one per 64 outputs.
    const long vfrom = RD_SB_VALID_FROM(a.seen_before, B);
    const double *cur = ring + 32 + 2 * (size_t)B;   // sample 0 of the newest block
    uint32_t parity = 0;
    for (uint32_t i = 0; i < nm; i++) {
        const int pm = s_match[i];   // (uniform: every thread reads the same word)
        if (pm & 0x40000000) continue;
        const long q = pm;
        const long ns = q - a.cfg.PL < 0 ? 0 : q - a.cfg.PL;
        const long pe = q + a.cfg.PL > B + 1 ? B + 1 : q + a.cfg.PL;
        double noise = 0.0, sig = 0.0;
        constexpr int R = 9;
        for (long j0 = ns + (long)tid * R; j0 < pe; j0 += (long)T * R) {
            // outputs j0 .. j0 + 8 are f[j0 - 1 .. j0 + 7]: samples j0 - 10 .. j0 + 6
            const double c[9] = RD_TAPS9;
            rd_d2 y[R + 8];
#pragma unroll
            for (int k = 0; k < R + 8; k++) {
                const long n = j0 - 10 + k;
                y[k] = rd_d2{0.0, 0.0};
                if (n >= vfrom && n < B) y[k] = rd_rot_f64(rd_load_coh(cur + 2 * n), rd_load_coh(cur + 2 * n + 1), n);
            }
#pragma unroll
            for (int r = 0; r < R; r++) {
                const long j = j0 + r;
                rd_d2 f = {0.0, 0.0};
                if (j - 1 >= vfrom) {
#pragma unroll
                    for (int m = 0; m < 9; m++) {
                        f.x += c[m] * y[r + m].x;
                        f.y += c[m] * y[r + m].y;
                    }
                }
                const double p = f.x * f.x + f.y * f.y;
                if (j < pe) { if (j < q) noise += p; else sig += p; }
            }
        }
        noise = rd_wave_sum(noise);
        sig = rd_wave_sum(sig);
        if (lane == 0) { s_part[parity][0][wave] = noise; s_part[parity][1][wave] = sig; }
        __syncthreads();
        if (wave == 0) {
            bool superseded;
            const uint32_t byte = bytes_of((int)q, superseded);
            double rssi = 0.0, snr = 0.0;
            if (lane == 0) {
                double nsum = 0.0, ssum = 0.0;
#pragma unroll
                for (int k = 0; k < T / 64; k++) { nsum += s_part[parity][0][k]; ssum += s_part[parity][1][k]; }
                RD_RSSI_OF_SUMS_F64(nsum, ssum, ns, pe, q, rssi, snr);
            }
            rd_store_record(nullptr, &recs[i], lane, 0, (long)a.seen_before, q, a.cfg.nbytes, byte, rssi, snr);
            if (a.parse) {   // Parser.parse's front half (rd_wave_parse), the ring read where the other workgroups' stores went
                const rd_cplx_coh_view cv = {cur, vfrom, (long)B};
                const int32_t e = rd_wave_parse(cv, a.cfg, q, byte, lane);
                if (lane == 0) a.fe_host[i] = e;
            }
        }
        parity ^= 1u;   // (the next match's partial sums go to the other set: one barrier per match)
    }
    // ---- count, fence, flag ----
    __syncthreads();
    if (tid == 0) {
        a.cnt_host[0] = nm;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope: records and count before the flag
        __hip_atomic_store(&a.flag_host[0], a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    RD_SBL_STAMP(6);
}

int rd_launch_stream_block_cplx(const rd_sbc_args &a_in, hipStream_t st) {
    const rd_devcfg &c = a_in.cfg;
    if (!rd_davis_shape(c) || c.L != 2 * c.B || c.B % 32 || c.B < 2048 || c.B > 8192 || !a_in.sync)
        return 0;
    rd_sbc_args a = a_in;
    a.stamps = nullptr;
#ifdef RD_DIAG
    a.stamps = rd_sb_stamp_buffer();
#endif
    constexpr int C = 8 * RD_SBC_THREADS;
    const int chunks = rd_sbc_chunk(C + 16) + 1;
    const size_t lds = (size_t)(2 * c.B / 32) * 4 + std::max((size_t)chunks * 16, ((size_t)c.B + 1) * 4);
    static bool attr_set = false;
    rd_allow_lds((const void *)k_stream_block_cplx<14, 16, 0x91D3ull, 80>, 96 * 1024, attr_set);
    hipLaunchKernelGGL((k_stream_block_cplx<14, 16, 0x91D3ull, 80>), dim3((unsigned)((c.B + C - 1) / C)), dim3(RD_SBC_THREADS), lds, st, a);
    return 1;
}

// ------------------------------------------------------------------------------------------
// complex128 input branch (py:144-150), float64 throughout
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cplx_bits(rd_cplx_view v, uint32_t *bits) {
    const long run = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long t0 = run * 32;
    if (t0 >= v.n) return;
    rd_d2 prev = rd_f_f64(v, t0 - 1);
    uint32_t word = 0;
    for (int r = 0; r < 32 && t0 + r < v.n; r++) {
        const rd_d2 cur = rd_f_f64(v, t0 + r);
        word |= rd_signbit_f64(rd_disc_f64(prev, cur)) << r;
        prev = cur;
    }
    bits[run] = word;
}

void rd_launch_cplx_bits(const rd_cplx_layout &lay, uint32_t *bits, hipStream_t st) {
    const long runs = (lay.n + 31) / 32;
    if (runs <= 0) return;
    hipLaunchKernelGGL(k_cplx_bits, rd_grid256(runs), dim3(256), 0, st, rd_cplx_view_of(lay), bits);
}
