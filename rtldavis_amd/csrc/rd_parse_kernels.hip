// rd_parse_kernels.hip - Parser.parse front half, protocol.py:290-311 (opt-in): k_parse_select / k_freq_err over a batch
// run's records, k_stream_parse over the records of a streaming block's multi-launch form (the one-launch blocks call
// rd_wave_parse, rd_device.h, themselves).
#include "rd_device.h"

// ------------------------------------------------------------------------------------------
// Parser.parse front half (protocol.py:282-311), batch mode.
// k_parse_select: one lane per final record: bit-reverse every byte (:290, :79-83), CRC-16-CCITT
// (poly 0x1021, init 0; crc.py:19-26) over data[2:] must be 0 (:297); survivors are compacted.
// k_freq_err: one wave per survivor: mean of discriminated[index : index + preamble_length]
// (:304-311) in float64, where discriminated covers absolute samples [(call-1)B, (call+1)B).
// ------------------------------------------------------------------------------------------
// (rd_swap_bits8: rd_parse.h)
__global__ __launch_bounds__(256) void k_parse_select(const rd_packet *recs, uint32_t match_cap, rd_parsed *parsed,
                                                      uint32_t *counters, int dense) {
    // records: [0, matches) one per match (stream < 0: reported by no call) and
    // [match_cap, match_cap + RD_CNT_REC) the second records of block-boundary positions
    uint32_t nprim = counters[RD_CNT_MATCH], nextra = counters[RD_CNT_REC];
    if (nprim > match_cap) nprim = match_cap;
    if (nextra > match_cap) nextra = match_cap;
    if (dense) {  // the two-kernel slice writes one record per task, densely, from index 0
        nprim = counters[RD_CNT_TASKS];
        if (nprim > 2 * match_cap) nprim = 2 * match_cap;
        nextra = 0;
    }
    const uint32_t rec_cap = 2 * match_cap;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool ok = false;
    uint8_t sw[RD_MAX_PKT_BYTES];
    int nb = 0;
    if ((i < nprim || (!dense && i >= match_cap && i - match_cap < nextra)) && recs[i].stream >= 0) {
        const rd_packet *r = &recs[i];
        nb = r->nbytes;
        uint32_t crc = 0;
#pragma unroll
        for (int k = 0; k < RD_MAX_PKT_BYTES; k++) {
            const uint32_t b = k < nb ? rd_swap_bits8(r->data[k]) : 0u;
            sw[k] = (uint8_t)b;
            if (k >= 2 && k < nb) {  // crc.py:24-25, bitwise form
                crc ^= b << 8;
#pragma unroll
                for (int j = 0; j < 8; j++) crc = (crc & 0x8000) ? ((crc << 1) ^ 0x1021) & 0xFFFF : (crc << 1) & 0xFFFF;
            }
        }
        ok = nb > 2 && crc == 0;
    }
    const uint64_t km = __ballot(ok);
    if (!km) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&counters[RD_CNT_PARSED], (uint32_t)__popcll(km));
    base = __builtin_amdgcn_readfirstlane(base);
    if (!ok) return;
    const uint32_t dst = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(km >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)km, 0));
    if (dst >= rec_cap) return;
    const rd_packet *r = &recs[i];
    rd_parsed *o = &parsed[dst];
    o->stream = r->stream; o->call = r->call; o->index = r->index; o->freq_err = 0;
    o->id = sw[2] & 7; o->nbytes = nb - 2;
#pragma unroll
    for (int k = 0; k < RD_MAX_PKT_BYTES; k++) o->data[k] = (k + 2 < RD_MAX_PKT_BYTES && k + 2 < nb) ? sw[k + 2] : 0;
    o->rssi = r->rssi; o->snr = r->snr;
}

__global__ __launch_bounds__(256) void k_freq_err(rd_layout lay, rd_devcfg cfg, rd_parsed *parsed, uint32_t rec_cap,
                                                  const uint32_t *counters) {
    const int lane = threadIdx.x & 63;
    uint32_t count = counters[RD_CNT_PARSED];
    if (count > rec_cap) count = rec_cap;
    const uint32_t nw = gridDim.x * (blockDim.x >> 6);
    for (uint32_t i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < count; i += nw) {
        rd_parsed *o = &parsed[i];
        const rd_stream_view v = rd_view_of(lay, o->stream);
        // discriminated[j] of call b is d[(b-1)B + j], j in [0, 2B) (py:134,156,162)
        const long j0 = o->index;
        long j1 = j0 + cfg.PL;
        if (j1 > 2L * cfg.B) j1 = 2L * cfg.B;
        const long t_base = ((long)o->call - 1) * cfg.B;
        double sum = 0.0;
        for (long j = j0 + lane; j < j1; j += 64) {
            const long t = t_base + j;
            sum += rd_disc_f64(rd_f_f64(v, t - 1), rd_f_f64(v, t));
        }
        sum = rd_wave_sum(sum);
        if (lane == 0) o->freq_err = rd_freq_err_hz(sum, j1 - j0, cfg.fs);
    }
}

void rd_launch_parse(const rd_layout &lay, const rd_devcfg &cfg, const rd_packet *recs, uint32_t match_cap,
                     rd_parsed *parsed, uint32_t *counters, hipStream_t st, int dense) {
    const uint32_t rec_cap = 2 * match_cap;
    hipLaunchKernelGGL(k_parse_select, rd_grid256(rec_cap), dim3(256), 0, st, recs, match_cap, parsed,
                       counters, dense);
    uint32_t wgs = (rec_cap + 3) / 4;
    if (wgs > 2048) wgs = 2048;
    hipLaunchKernelGGL(k_freq_err, dim3(wgs), dim3(256), 0, st, lay, cfg, parsed, rec_cap, counters);
}

// ------------------------------------------------------------------------------------------
// k_stream_parse: the same front half for the streaming handle's MULTI-LAUNCH form (shapes the one-launch blocks decline):
// one wave per record of the slice kernel that ran in front of it on the stream, read where that kernel wrote them
// (mapped host memory: the kernel boundary orders the two), results into the slot's fe array - entry i belongs to
// record i, RD_FE_NONE for a void record or a failed CRC.  rd_wave_parse is what the one-launch blocks call: the forms
// give identical results.
// ------------------------------------------------------------------------------------------
struct rd_u8_views {
    rd_layout lay;
    __device__ __forceinline__ rd_stream_view of(int stream) const { return rd_view_of(lay, stream); }
};
struct rd_cplx_views {
    rd_cplx_view v;
    __device__ __forceinline__ rd_cplx_view of(int) const { return v; }
};

template <class Views>
__global__ __launch_bounds__(256) void k_stream_parse(Views src, rd_devcfg cfg, const rd_packet *recs, uint32_t match_cap,
                                                      int32_t *fe, const uint32_t *counters) {
    const int lane = threadIdx.x & 63;
    uint32_t count = counters[RD_CNT_MATCH];
    if (count > match_cap) count = match_cap;
    const uint32_t nw = gridDim.x * (blockDim.x >> 6);
    for (uint32_t i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < count; i += nw) {
        const rd_packet *r = &recs[i];
        const int stream = __builtin_amdgcn_readfirstlane(r->stream);
        if (stream < 0) {
            if (lane == 0) fe[i] = RD_FE_NONE;
            continue;
        }
        const long pos = __builtin_amdgcn_readfirstlane(r->index);
        const uint32_t byte = lane < RD_MAX_PKT_BYTES ? (uint32_t)r->data[lane] : 0u;
        const int32_t e = rd_wave_parse(src.of(stream), cfg, pos, byte, lane);
        if (lane == 0) fe[i] = e;
    }
}

void rd_launch_stream_parse(const rd_layout &lay, const rd_devcfg &cfg, const rd_packet *recs, uint32_t match_cap,
                            int32_t *fe, const uint32_t *counters, hipStream_t st) {
    rd_u8_views src;
    src.lay = lay;
    hipLaunchKernelGGL(k_stream_parse<rd_u8_views>, dim3(rd_slice_grid(match_cap)), dim3(256), 0, st, src, cfg, recs,
                       match_cap, fe, counters);
}

void rd_launch_cplx_stream_parse(const rd_cplx_layout &lay, const rd_devcfg &cfg, const rd_packet *recs, uint32_t match_cap,
                                 int32_t *fe, const uint32_t *counters, hipStream_t st) {
    rd_cplx_views src;
    src.v = rd_cplx_view_of(lay);
    hipLaunchKernelGGL(k_stream_parse<rd_cplx_views>, dim3(rd_slice_grid(match_cap)), dim3(256), 0, st, src, cfg, recs,
                       match_cap, fe, counters);
}
