// rd_internal.h - launch interface between the host logic of the C ABI (rd_batch.hip, rd_stream.hip, rd_stages.hip,
// rd_wideband.hip) and the kernels' translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rtldavis_hip.h"
#include "rd_hiphost.h"
#include "rd_host.h"
#include "rd_batch_plan.h"

// the counter slots (RD_CNT_*), the counter set's layout and RD_FT_STREAMS: rd_batch_plan.h (pure host code decides by them)
// rd_launch_demod flags
#define RD_DEMOD_FIX_BUCKETS 4u    /* the fix-up entries go to per-group buckets (the one-launch tail, k_tail): fix_list =
                                      [groups][fix_cap] entries, bucket_cnt = [groups] counters, group = stream >> RD_FT_GSH */
struct rd_ft_bufs {
    uint32_t *fixb = nullptr;    // [groups][fix_bcap] fix-up entries, filled by the demod kernel's waves
    uint32_t *fixcnt = nullptr;  // [groups] entries written (lives behind the counter set of the run: cleared with it)
    uint32_t fix_bcap = 0;
    uint32_t bcap = 0;           // matches a stream's list in LDS holds (a multiple of 32, rd_host.h: rd_ord_bucket_cap)
    uint32_t *gstate = nullptr;  // [3][groups]: (seq << 20 | records), matches, fix-up entries per group
};
// Geometry of the fused demod kernel
// (RD_TILE_SAMPLES, 64 lanes x 32 samples, one wave iteration: rd_batch_plan.h)
#define RD_TILE_BYTES 4096
#define RD_INPUT_PAD 8192     // bytes readable past the last stream (ragged last tile)

// One set of streams laid out with a fixed byte stride.
struct rd_layout {
    const uint8_t *iq;        // sample 0 of stream 0 (16-byte aligned)
    size_t stream_stride;     // bytes between streams (multiple of 16)
    int n_streams;
    uint32_t n_samples;       // samples per stream handled by this launch
    int hist_mode;            // 0: zero history before sample 0 (after reset);
                              // 1: >= 16 samples of raw history precede each stream's sample 0
    long valid_from;          // first readable sample (0 for hist_mode 0, negative otherwise)
    uint32_t *bits;           // packed sign bits, word w of stream s at bits[s*bits_stride + w]
    size_t bits_stride;       // words
};

// rd_devcfg: rd_host.h (the pure-host translation unit shares it); the slots' layouts and headers: rd_slots.h, through it

struct rd_match {
    int32_t stream;
    int32_t pos;  // bit-array coordinate of the first preamble sample
};

// rd_make_devcfg (rd_host.h) with its reason as the error text
static inline int rd_devcfg_checked(const rd_config *c, rd_devcfg *d) {
    const char *why = "";
    const int rc = rd_make_devcfg(c, d, &why);
    return rc ? rd_fail_msg(rc, "%s", why) : RD_OK;
}

// --- launches (all asynchronous on `st`) ---
// ev_start / ev_stop (optional): events that receive the kernel's own begin / end timestamps.
// flags: RD_DEMOD_FIX_BUCKETS with bucket_cnt (the groups' entry counters; fix_list = [groups][fix_cap] then).  Returns the
// flags the launched kernel honoured (the ablated kernels of the diagnostic library keep the one list: none).
// chunk_out: receives the tiles per chunk the launch used and the number of waves
// RD_DEMOD_REFUSED in the result: nothing was launched (rd_launch_demod_mfma's -1); the caller reports an error.
#define RD_DEMOD_REFUSED 0x80000000u
uint32_t rd_launch_demod(const rd_layout &lay, uint32_t *fix_list, uint32_t fix_cap, uint32_t *counters, hipStream_t st,
                         hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr, uint32_t flags = 0,
                         uint32_t *chunk_out = nullptr, uint32_t *bucket_cnt = nullptr);
// The kernel itself (rd_demod_mfma.hip).  dbg_g (test hook): when given, the kernel also dumps g[tile][2048][2].
// Returns 1 when the fix-up entries went to the buckets, 0 when they went to the one list, -1 when nothing was launched
// (the grid could not serve every work queue: rd_demod_mfma.hip, rd_mf_launch_variant).
int rd_launch_demod_mfma(const rd_layout &lay, uint32_t *fix_list, uint32_t fix_cap, uint32_t *counters, hipStream_t st,
                          hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr, float *dbg_g = nullptr,
                          uint32_t flags = 0, uint32_t *chunk_out = nullptr, uint32_t *bucket_cnt = nullptr);
// the test hook's last launch (rd_debug_demod_mfma): tiles per chunk, waves
void rd_debug_last_launch(uint32_t out[2]);
// all != 0: re-evaluate every run exactly (used when the guard list overflowed or the
// layout does not meet the fast kernel's alignment requirements).
// zero_next (may be null): RD_CNT_TOTAL words (counters and work queues) to clear for the handle's next run.
// zero_words: how many words at zero_next (the counter set, plus k_tail's per-group bucket counters when the handle
// has them behind it)
// expect (0: unknown): the list length of the handle's previous run - the grid is sized for it (+25 %) instead of
// for the list's capacity (every lane loops with the grid's stride, so a short grid is only slower, never wrong)
void rd_launch_fixup(const rd_layout &lay, const uint32_t *fix_list, uint32_t fix_cap, uint32_t *counters, int all,
                     uint32_t *zero_next, hipStream_t st, uint32_t zero_words = RD_CNT_TOTAL, uint64_t expect = 0);
// Search positions p in [p_lo, p_hi] of every stream's bit array (bits outside [0, n_bits) are 0).
void rd_launch_search(const uint32_t *bits, size_t bits_stride, int n_streams, long n_bits, long p_lo, long p_hi,
                      const rd_devcfg &cfg, rd_match *matches, uint32_t match_cap, uint32_t *counters,
                      hipStream_t st);
// The whole tail in one launch (k_tail): exact bits for the listed groups, search, slice with order and dedupe, RSSI /
// SNR, final records.  seq: 1..4095, different from the previous launch on fb.gstate.  skip_fix: the bits are final.
// Returns 1 when launched, 0 when the shape is not the one the kernel is built for.
int rd_launch_tail_fused(const rd_layout &lay, const rd_devcfg &cfg, int n_calls, long p_lo, long p_hi, const rd_ft_bufs &fb,
                         uint32_t bucket_limit, uint32_t seq, int skip_fix, rd_packet *recs, uint32_t rec_cap, uint32_t *counters,
                         hipStream_t st, hipEvent_t ev_stop = nullptr, uint32_t *zero_next = nullptr, uint32_t zero_words = 0);
// Slice + RSSI/SNR, one wave per match.  batch_mode = 1: position = absolute sample, calls derived
// from it (n_calls blocks from reset).  batch_mode = 0: position = window index q of call `call`,
// lay.iq points at the newest block's first sample.
// recs holds 2 * match_cap entries: recs[i] is match i's record (stream = -1 when no call reports
// it); the second record of a position on a block boundary (q = B in call b and q = 0 in call
// b+1, py:194) goes to recs[match_cap + k], k < RD_CNT_REC.  Per-call duplicates (py:203-205) are
// left to the host, which orders the records anyway.  recs (device memory) and recs_host (the
// device address of pinned, mapped host memory) are both optional: the kernel stores to each that
// is given; with recs_host the records need no device-to-host copy.
// returns 1 when the records were written densely (one per task, RD_CNT_TASKS of them from index 0), else 0
int rd_launch_slice(const rd_layout &lay, const uint32_t *bits, size_t bits_stride, long n_bits, const rd_devcfg &cfg,
                     const rd_match *matches, uint32_t match_cap, int batch_mode, int n_calls, int call,
                     rd_packet *recs, rd_packet *recs_host, uint32_t *counters, hipStream_t st,
                     hipEvent_t ev_stop = nullptr, void *tasks = nullptr);
// tasks: 2 * match_cap entries of RD_TASK_BYTES (the two-kernel form of the batch path; null: one kernel)
#define RD_TASK_BYTES 16
// Parser.parse front half (protocol.py:290-311) over the records of a batch run (layout as
// above): CRC-valid ones are written to `parsed` (RD_CNT_PARSED) with their frequency error.
void rd_launch_parse(const rd_layout &lay, const rd_devcfg &cfg, const rd_packet *recs, uint32_t match_cap,
                     rd_parsed *parsed, uint32_t *counters, hipStream_t st, int dense = 0);
// The same front half for the records the streaming handle's multi-launch form has just sliced (rd_launch_slice /
// rd_launch_cplx_slice with recs_host, batch_mode 0, queued on `st` in front of this): fe[i] = RD_FE_NONE or the
// frequency error of record i (rd_parse.h), i < RD_CNT_MATCH.  recs and fe: device addresses of mapped host memory.
void rd_launch_stream_parse(const rd_layout &lay, const rd_devcfg &cfg, const rd_packet *recs, uint32_t match_cap,
                            int32_t *fe, const uint32_t *counters, hipStream_t st);
struct rd_cplx_layout;
void rd_launch_cplx_stream_parse(const rd_cplx_layout &lay, const rd_devcfg &cfg, const rd_packet *recs, uint32_t match_cap,
                                 int32_t *fe, const uint32_t *counters, hipStream_t st);
// d[t0 .. t0+n) of stream `stream` in float64
void rd_launch_disc(const rd_layout &lay, int stream, long t0, long n, double *out, hipStream_t st);
// f[t0 .. t0+n) (interleaved re,im) of stream `stream` in float64
void rd_launch_filtered(const rd_layout &lay, int stream, long t0, long n, double *out, hipStream_t st);
// window <- (window >> shift_bits) with `block` (n_block_bits) appended at the top; window has n_win_bits
void rd_launch_window_update(uint32_t *win_out, const uint32_t *win_in, long n_win_bits, const uint32_t *block,
                             long n_block_bits, int n_streams, size_t win_stride, size_t block_stride,
                             hipStream_t st);

// The streaming handle's one-launch block (k_stream_block, rd_tail_kernels.hip): everything of one demodulate() call - ring
// roll, exact bits, window, search, slice + RSSI, results into mapped host memory - for NS streams in lock step.
#define RD_SB_THREADS 1024
#ifndef RD_SBC_THREADS
#define RD_SBC_THREADS 256   // k_stream_block_cplx: a workgroup takes 8 x this many samples of the block
#endif
struct rd_sb_args {
    rd_devcfg cfg;
    uint8_t *ring;            // the streams' raw rings: [hdr 32 B][previous block][newest block], ring_stride apart
    size_t ring_stride;
    const uint8_t *in;        // device address of the pinned input: NS x 2B bytes
    const uint32_t *win_in;   // quantized window before this block (2B bits per stream)
    uint32_t *win_out;        // ... and after it
    rd_packet *recs_host;     // mapped host memory: B + 1 records per stream (record i of a stream = its match i)
    uint32_t *cnt_host;       // mapped: matches per stream
    uint32_t *flag_host;      // mapped: seq per stream, stored last
    uint32_t seq;
    long seen_before;         // blocks since reset
    uint64_t *stamps;         // diagnostic library: phase stamps (else null)
    int parse;                // also run Parser.parse's front half for every record (rd_device.h: rd_wave_parse) ...
    int32_t *fe_host;         // ... into mapped host memory laid out like recs_host: RD_FE_NONE or the frequency error
};
// 1 when the kernel was launched, 0 when the configuration is not one it is built for
int rd_launch_stream_block(const rd_sb_args &a, int n_streams, hipStream_t st);

// The same for the complex-input branch (k_stream_block_cplx): one stream, complex128 ring, input from mapped host memory
// as complex128 or (in_is_u8) as bytes through the LUT
struct rd_sbc_args {
    rd_devcfg cfg;
    double *ring;             // [hdr 32 doubles][previous block][newest block]
    const void *in;           // device address of the pinned input: B complex128 or 2B bytes
    int in_is_u8;
    const uint32_t *win_in;
    uint32_t *win_out;
    rd_packet *recs_host;     // mapped host memory: B + 1 records
    uint32_t *cnt_host, *flag_host;
    uint32_t seq;
    long seen_before;
    uint32_t *sync;           // device word, zero between launches: the workgroups count themselves in
    uint64_t *stamps;         // diagnostic library: phase stamps (else null)
    int parse;                // as rd_sb_args
    int32_t *fe_host;
};
int rd_launch_stream_block_cplx(const rd_sbc_args &a, hipStream_t st);

// complex128 input path (py:144-150): raw ring of interleaved doubles
struct rd_cplx_layout {
    const double *x;   // sample 0 (interleaved re,im)
    long valid_from;   // first readable sample
    long n;            // samples
};
void rd_launch_cplx_bits(const rd_cplx_layout &lay, uint32_t *bits, hipStream_t st);
void rd_launch_cplx_disc(const rd_cplx_layout &lay, long t0, long n, double *out, hipStream_t st);
void rd_launch_cplx_filtered(const rd_cplx_layout &lay, long t0, long n, double *out, hipStream_t st);
void rd_launch_cplx_slice(const rd_cplx_layout &lay, const uint32_t *bits, long n_bits, const rd_devcfg &cfg,
                          const rd_match *matches, uint32_t match_cap, int call, rd_packet *recs, rd_packet *recs_host,
                          uint32_t *counters, hipStream_t st);
void rd_launch_lut(const uint8_t *in, double *out, size_t n_cplx, hipStream_t st);

// stage kernels on device arrays (float64)
void rd_launch_rotate(const double *in, double *out, size_t n, hipStream_t st);
void rd_launch_fir9(const double *in, double *out, size_t n_out, hipStream_t st);
void rd_launch_discriminate(const double *in, double *out, size_t n_out, hipStream_t st);
void rd_launch_quantize(const double *in, uint8_t *out, size_t n, hipStream_t st);
void rd_launch_pack_bytes(const uint8_t *in01, uint32_t *words, size_t n, hipStream_t st);

// --- wideband receiver (rd_wideband.hip): the streaming channelizer and a multi-stream demodulator fed from device memory ---
// rd_channelizer.hip: device tables of the handle on the current device; one streamed chunk (n_out a multiple of 128 output
// times, t_base its first output's absolute time, a multiple of 128; prev = the chunk before, null = zero history)
int rd_chan_stream_prepare(rd_chan *h);
int rd_chan_stream_launch(rd_chan *h, const uint8_t *wide, const uint8_t *prev, size_t n_out, uint64_t t_base, void *dst,
                          size_t dst_stride, hipStream_t st);
// Retune n channels of the handle (rd_channelizer.hip: RETUNE): rec = n x (channel, shift in Hz, phase accumulator P).
// On the host before the device tables exist; afterwards through pinned slot `slot` (0 / 1, free by the caller's
// ordering) and k_chan_retune, queued on st.  rd_chan_tuning: the shifts (as given) and phases the tables hold.
int rd_chan_retune(rd_chan *h, const int64_t *rec, int n, int slot, hipStream_t st);
void rd_chan_tuning(const rd_chan *h, const int64_t **shift_hz, const int64_t **phase);
// Gains (rd_channelizer.hip: GAIN): the argument check of rd_chan_set_gain / rd_wb_set_gain (rd_chan_tables.cpp); the float32 table the
// handle's kernels use (what the last rd_chan_stream_gains queued, or the host's before the device tables exist); and the
// update itself - the whole table through pinned slot `slot` in one copy on st, nothing when no entry differs.
int rd_chan_check_gains(const rd_chan *h, const double *gain, int n);
const float *rd_chan_gains(const rd_chan *h);
int rd_chan_stream_gains(rd_chan *h, const float *gain, int slot, hipStream_t st);
// Levels of one streamed chunk (rd_chan_levels.hip: k_chan_levels) behind its rd_chan_stream_launch on st: wide / chan_out as given to that
// launch; out ([n_channels]) and in: device addresses of mapped host memory; acc: RD_LV_ACC_WORDS zeroed device words
// (the kernel leaves them zero).
#define RD_LV_ACC_WORDS 8
int rd_chan_stream_levels(rd_chan *h, const uint8_t *wide, size_t n_out, const uint8_t *chan_out, size_t out_stride,
                          uint64_t seq, rd_chan_level *out, rd_input_level *in, uint32_t *acc, hipStream_t st);
// adm (include/rtldavis_hip.h: RD_IQ_CF32) of a float32 component given as its bits: NaN -> 0, else clamped to [-8, 8]
#define RD_CF32_CLAMP 8.0f
__device__ __forceinline__ float rd_chan_adm(uint32_t bits) {
    const float v = __builtin_bit_cast(float, bits);
    return v != v ? 0.0f : fminf(fmaxf(v, -RD_CF32_CLAMP), RD_CF32_CLAMP);
}
// Power spectrum of a capture (rd_spectrum.hip: k_chan_spectrum; the definition: include/rtldavis_hip.h, SPECTRUM).
// rd_spec: the tables of one n_bins (periodic Hann window, per-stage twiddles), the workgroups' partial sums and the
// ticket word, on the current device.  rd_spec_check: the argument rule (RD_ERR_ARG with a message, no device work).
// rd_spec_prepare: (re)builds *sp when it is null or holds another n_bins or fewer workgroups than n_samples needs - the
// caller knows that no launch on the old one is still running.  rd_spec_launch: one launch on st over IQ pairs
// [0, n_samples) of `wide` (device, 16-byte aligned, sample format fmt); out: RD_SPEC_HDR_BYTES of header {uint64 seq;
// uint32 segments; uint32 n_bins} + n_bins doubles, a device address (mapped host memory included).
#define RD_SP_MAX_GROUPS 64
struct rd_spec;
int rd_spec_check(int n_bins, size_t n_samples);
int rd_spec_prepare(rd_spec **sp, int n_bins, size_t n_samples, hipStream_t st);
int rd_spec_launch(rd_spec *sp, const uint8_t *wide, int fmt, size_t n_samples, uint64_t seq, void *out, hipStream_t st);
void rd_spec_destroy(rd_spec *sp);
// Bursts of a channelized chunk (rd_bursts.hip: k_chan_bursts; the definition: include/rtldavis_hip.h, BURSTS).
// rd_bursts_check: the argument rule for a chunk of n_out outputs per channel (RD_ERR_ARG with a message, no device work).
// rd_bursts_launch: one launch on st over chan_out (channel c at chan_out + c * out_stride, 2 n_out bytes each, 16-byte
// aligned); slot: a device address (mapped host memory) of rd_bu_slot_bytes laid out as
//   [n_ch][cap] rd_burst | [n_ch] rd_burst_floor | [n_ch] uint32 thresholds           cap = rd_bu_cap(n_win)
// The caller writes the thresholds before the launch; the kernel writes the floor records and, per channel, the first
// floor.n_bursts of its cap record places.
int rd_bursts_check(size_t n_out);
int rd_bursts_launch(const uint8_t *chan_out, size_t out_stride, int n_ch, size_t n_out, uint64_t seq, void *slot, hipStream_t st);
// Burst decode of a channelized chunk (rd_burst_decode.hip: k_chan_burst_decode; the definition: include/rtldavis_hip.h,
// BURST DECODE), queued behind rd_bursts_launch on the same stream.  rd_burst_decode_check: the argument rule for a
// configuration (RD_ERR_ARG with a message, no device work).  rd_burst_decode_launch: chan_out as given to rd_bursts_launch,
// chan_prev the chunk before laid out alike (null: none, no look-back), clock the absolute time of the chunk's first
// output; burst_slot: the slot that rd_bursts_launch filled; slot: a device address (mapped host memory) of
// rd_bd_slot_bytes laid out as
//   [n_ch][cap] rd_burst_msg | [n_ch] rd_bd_header                                    cap = rd_bu_cap(n_win)
// The kernel writes every header and, per channel, the first header.n_msgs of its cap record places.
// max_flips: R of the header's steps 5a / 5b / 6' (0 .. RD_BD_MAX_FLIPS, else RD_ERR_ARG and nothing launched); 0 launches
// the kernel without repair.  narrow_tab: null, or the device table of rd_bd_narrow_upload for cfg's symbol_length - then
// step 4n runs (RD_ERR_ARG with symbol_length < RD_BD_NB_MIN_SL).  rd_bd_narrow_upload: *d_tab = a device buffer of
// 64 x (2 sl + 5) taps and 64 centres, an int16 pair (re low, im high) per uint32, filled from rd_bd_narrow_table by a
// blocking copy; the caller frees it with hipFree.
#define RD_BD_MAX_W 32          /* a run of more windows is counted, not decoded */
#define RD_BD_MAX_LOOK_W 16     /* packet_symbols * symbol_length + 1 <= 2048 */
#define RD_BD_DATA_BYTES RD_BURST_MSG_BYTES
#define RD_BD_MAX_FLIPS 2       /* symbols a repair flips at most */
int rd_bd_look_windows(const rd_config *cfg);
int rd_burst_decode_check(const rd_config *cfg);
int rd_burst_decode_launch(const rd_config *cfg, const uint8_t *chan_out, const uint8_t *chan_prev, size_t out_stride, int n_ch,
                           size_t n_out, uint64_t clock, uint64_t seq, int max_flips, const uint32_t *narrow_tab,
                           const void *burst_slot, void *slot, hipStream_t st);
int rd_bd_narrow_upload(int sl, uint32_t **d_tab);
// Burst expect of a channelized chunk (rd_burst_expect.hip: k_chan_burst_expect; the definition: include/rtldavis_hip.h,
// BURST EXPECT), queued behind rd_burst_decode_launch on the same stream.  slot: mapped host memory of RD_BX_SLOT_BYTES,
//   [RD_BX_MAX] rd_burst_msg | [RD_BX_MAX] rd_bx_header | [RD_BX_MAX] rd_bx_entry
// rd_burst_expect_stage (host only): the candidate range of every expectation for `clock` into the slot's entries, as the
// kernel reads them; returns how many are active - 0: the caller launches nothing.  cand (may be null): n counts.
// rd_burst_expect_launch: one workgroup per entry; it writes every header below n and, for an expectation that found a
// packet, its record place.  slot_host / slot_dev: the host and device address of the same slot.
int rd_burst_expect_stage(const rd_config *cfg, int have_prev, uint64_t clock, const rd_expect *e, int n, void *slot_host,
                          uint32_t *cand);
int rd_burst_expect_launch(const rd_config *cfg, const uint8_t *chan_out, const uint8_t *chan_prev, size_t out_stride, int n_ch,
                           size_t n_out, uint64_t clock, uint64_t seq, int n, int max_flips, const uint32_t *narrow_tab,
                           void *slot_dev, hipStream_t st);
// Burst search of a channelized chunk (rd_burst_search.hip: k_chan_burst_search; the definition: include/rtldavis_hip.h,
// BURST SEARCH), queued behind rd_burst_expect_launch (or rd_burst_decode_launch) on the same stream.  slot: a device
// address (mapped host memory) of rd_bs_slot_bytes(n_ch) laid out as
//   [RD_BS_MAX_CENTRES][n_ch][RD_BS_PER] rd_burst_msg | [RD_BS_MAX_CENTRES][n_ch] rd_bs_header
// One workgroup per (channel, centre i < n): it writes its header and the first header.n_msgs of its RD_BS_PER record
// places; nothing of a centre index >= n is touched.  centres: host memory, n of them, checked by rd_bs_check_centres
// (rd_host.h); they travel in the kernel's arguments.  narrow_tab: the device table of rd_bd_narrow_upload for cfg's
// symbol_length (never null: the search is always a narrow-band one).
int rd_burst_search_launch(const rd_config *cfg, const uint8_t *chan_out, const uint8_t *chan_prev, size_t out_stride, int n_ch,
                           size_t n_out, uint64_t clock, uint64_t seq, const uint8_t *centres, int n, const uint32_t *narrow_tab,
                           void *slot_dev, hipStream_t st);
// Burst quality (rd_burst_quality.hip: k_chan_burst_quality; the definition: include/rtldavis_hip.h, BURST QUALITY),
// queued behind rd_burst_decode_launch / rd_burst_expect_launch on the same stream.  One launch walks a slot of n_groups
// groups of `cap` record places whose 16-byte headers begin with n_msgs and hold the chunk number in their third word -
// rd_bd_header and rd_bx_header both do: the decode slot with n_ch groups of rd_bu_cap(n_win) places, the expect slot with
// the table's size in groups of one.  recs, hdr: device addresses inside the slot the kernel in front filled; qual: a
// device address (mapped host memory) with room for n_groups x cap records, record [group][place] beside its message.
// The receiver's quality slot:  [n_ch][cap] rd_burst_quality | [RD_BX_MAX] rd_burst_quality.
// narrow_tab: the device table of rd_bd_narrow_upload for cfg's symbol_length; may be null with symbol_length < 4 only.
int rd_burst_quality_launch(const rd_config *cfg, const uint8_t *chan_out, const uint8_t *chan_prev, size_t out_stride, int n_ch,
                            size_t n_out, int noise_gap, const uint32_t *narrow_tab, const rd_burst_msg *recs, size_t cap,
                            const rd_bq_header *hdr, int n_groups, rd_burst_quality *qual, hipStream_t st);
// Burst clips (rd_burst_clips.hip: k_chan_burst_clips; the definition: include/rtldavis_hip.h, BURST CLIPS), queued behind
// the chunk's last burst kernel on the same stream.  One workgroup per channel.  It reads, where given, the slots the
// kernels in front filled - burst_slot (rd_bursts_launch), decode_slot (rd_burst_decode_launch; null: not launched),
// expect_slot with n_expect entries (null / 0: not launched), search_slot with n_search centres (null / 0) - and prev_hdr,
// the [n_ch] headers of the clip slot the chunk before wrote (null: that chunk had no clips, or there is none).  All are
// device addresses of mapped host memory, as is slot, of rd_bc_slot_bytes(n_ch, quota) laid out as
//   [n_ch][RD_BC_PER] rd_burst_clip | [n_ch] rd_bc_header | padding to a multiple of 16 | [n_ch][2 quota] bytes
// The kernel writes every header and, per channel, the first header.n_clips record places and the first 2 header.used
// bytes of its pool.  cfg is read for symbol_length and packet_symbols, and checked, with RD_BC_MESSAGES only.
int rd_burst_clips_check(int n_ch, int sources, int pre, int post, int quota);   // the rule of rd_wb_set_burst_clips: RD_ERR_ARG with a message
int rd_burst_clips_launch(const rd_config *cfg, const uint8_t *chan_out, const uint8_t *chan_prev, size_t out_stride, int n_ch,
                          size_t n_out, uint64_t clock, uint64_t seq, int sources, int pre, int post, int quota,
                          const void *burst_slot, const void *decode_slot, const void *expect_slot, int n_expect,
                          const void *search_slot, int n_search, const rd_bc_header *prev_hdr, void *slot, hipStream_t st);
int rd_chan_format(const rd_chan *h);             // RD_IQ_* of the handle
int rd_chan_n_channels(const rd_chan *h);
int rd_chan_decim(const rd_chan *h);
const float *rd_chan_device_gains(const rd_chan *h);   // the device's gain table; null before the device tables exist
int64_t rd_chan_out_rate(const rd_chan *h);
int64_t rd_chan_wide_rate(const rd_chan *h);
int rd_chan_bytes_per_sample(const rd_chan *h);   // of an IQ pair in the handle's sample format
// rd_stream.hip: the handle's device state and its two non-blocking streams (compute, copy)
int rd_demod_prepare(rd_demod *h, hipStream_t *st, hipStream_t *st_copy);
// drop the blocks a timed-out fetch gave up on, then RD_ERR_STATE if two blocks are in flight
int rd_demod_check_room(rd_demod *h);
// rd_demod_submit for a multi-stream uint8 handle whose block ([n_streams][2 * block_size]) already lies in device
// memory, written by work queued on the handle's compute stream
int rd_demod_submit_device(rd_demod *h, const uint8_t *dev_block);
// blocks in flight whose packets can still be fetched (rd_demod_inflight less those a timed-out fetch gave up on)
int rd_demod_pending(const rd_demod *h);
