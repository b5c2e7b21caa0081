// rd_slots.h - the layouts of the receiver's mapped pinned slots: what a burst kernel writes and the fetch reads
// (rd_host.cpp: rd_collect_*).  Nothing in here touches HIP; the launches that fill the slots: rd_internal.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/rtldavis_hip.h"

// Spectrum (rd_spectrum.hip):  {uint64 seq; uint32 segments; uint32 n_bins} | [n_bins] double
#define RD_SPEC_HDR_BYTES 16
// Bursts (rd_bursts.hip):  [n_ch][cap] rd_burst | [n_ch] rd_burst_floor | [n_ch] uint32 thresholds      cap = rd_bu_cap(n_win)
#define RD_BU_WINDOW 128
#define RD_BU_MAX_WINDOWS 4096
static inline size_t rd_bu_cap(size_t n_win) { return (n_win + 1) / 2; }
static inline size_t rd_bu_floor_offset(int n_ch, size_t n_win) { return (size_t)n_ch * rd_bu_cap(n_win) * sizeof(rd_burst); }
static inline size_t rd_bu_thr_offset(int n_ch, size_t n_win) { return rd_bu_floor_offset(n_ch, n_win) + (size_t)n_ch * sizeof(rd_burst_floor); }
static inline size_t rd_bu_slot_bytes(int n_ch, size_t n_win) { return rd_bu_thr_offset(n_ch, n_win) + (size_t)n_ch * sizeof(uint32_t); }
// Burst decode (rd_burst_decode.hip):  [n_ch][cap] rd_burst_msg | [n_ch] rd_bd_header
struct rd_bd_header {
    uint32_t n_msgs, long_runs;
    uint32_t chunk;              // the chunk's sequence number since create / reset, its low 32 bits
    uint32_t pad;
};
static inline size_t rd_bd_header_offset(int n_ch, size_t n_win) { return (size_t)n_ch * rd_bu_cap(n_win) * sizeof(rd_burst_msg); }
static inline size_t rd_bd_slot_bytes(int n_ch, size_t n_win) { return rd_bd_header_offset(n_ch, n_win) + (size_t)n_ch * sizeof(rd_bd_header); }
// Burst expect (rd_burst_expect.hip):  [RD_BX_MAX] rd_burst_msg | [RD_BX_MAX] rd_bx_header | [RD_BX_MAX] rd_bx_entry
struct rd_bx_header {
    uint32_t n_msgs, candidates;
    uint32_t chunk;              // the chunk's sequence number since create / reset, its low 32 bits
    uint32_t pad;
};
struct rd_bx_entry {
    int32_t channel;
    uint32_t id;
    int32_t tau_a, tau_b;        // tau_a > tau_b: idle in this chunk
    int32_t corr_re, corr_im;
    uint32_t pad[2];
};
#define RD_BX_HEADER_OFFSET ((size_t)RD_BX_MAX * sizeof(rd_burst_msg))
#define RD_BX_ENTRY_OFFSET (RD_BX_HEADER_OFFSET + (size_t)RD_BX_MAX * sizeof(rd_bx_header))
#define RD_BX_SLOT_BYTES (RD_BX_ENTRY_OFFSET + (size_t)RD_BX_MAX * sizeof(rd_bx_entry))
// Burst search (rd_burst_search.hip):  [RD_BS_MAX_CENTRES][n_ch][RD_BS_PER] rd_burst_msg | [RD_BS_MAX_CENTRES][n_ch] rd_bs_header
#define RD_BS_MAX_CHANNELS 4096
static inline size_t rd_bs_header_offset(int n_ch) { return (size_t)RD_BS_MAX_CENTRES * (size_t)n_ch * RD_BS_PER * sizeof(rd_burst_msg); }
static inline size_t rd_bs_slot_bytes(int n_ch) { return rd_bs_header_offset(n_ch) + (size_t)RD_BS_MAX_CENTRES * (size_t)n_ch * sizeof(rd_bs_header); }
// Burst quality (rd_burst_quality.hip):  [n_ch][cap] rd_burst_quality | [RD_BX_MAX] rd_burst_quality; rd_bq_header is
// how its kernel sees an rd_bd_header or an rd_bx_header
struct rd_bq_header {
    uint32_t n_msgs, other;
    uint32_t chunk;
    uint32_t pad;
};
static inline size_t rd_bq_expect_offset(int n_ch, size_t n_win) { return (size_t)n_ch * rd_bu_cap(n_win) * sizeof(rd_burst_quality); }
static inline size_t rd_bq_slot_bytes(int n_ch, size_t n_win) { return rd_bq_expect_offset(n_ch, n_win) + (size_t)RD_BX_MAX * sizeof(rd_burst_quality); }
// Burst clips (rd_burst_clips.hip):  [n_ch][RD_BC_PER] rd_burst_clip | [n_ch] rd_bc_header | padding to 16 | [n_ch][2 quota] bytes
struct rd_bc_header {
    uint32_t n_clips, dropped;
    uint32_t owed, used;         // outputs
    uint32_t chunk;              // the chunk's sequence number since create / reset, its low 32 bits
    uint32_t pad;
};
static inline size_t rd_bc_header_offset(int n_ch) { return (size_t)n_ch * RD_BC_PER * sizeof(rd_burst_clip); }
static inline size_t rd_bc_pool_offset(int n_ch) { return (rd_bc_header_offset(n_ch) + (size_t)n_ch * sizeof(rd_bc_header) + 15) & ~(size_t)15; }
static inline size_t rd_bc_slot_bytes(int n_ch, int quota) { return rd_bc_pool_offset(n_ch) + (size_t)n_ch * 2 * (size_t)quota; }
