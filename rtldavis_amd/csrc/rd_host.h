// rd_host.h - the pure-host parts of the C ABI: nothing in here touches HIP, so the same translation unit
// (rd_host.cpp) is compiled into librtldavis_hip.so by hipcc AND into tests/host_asan by g++ with
// -fsanitize=address,undefined (SURVEY section 5's sanitizer stance; the GPU pool allows no sanitizer runs).
//   rd_make_devcfg        PacketConfig's derived constants (py:101-125) and the limits the kernels rely on
//   rd_order_and_dedupe   the per-call order and first-occurrence dedupe of Demodulator._slice (py:171-205)
//   rd_ord_bucket_cap     matches a stream's list in k_tail's LDS holds, from the stream's length
//   rd_check_block_count  "Incompatible array sizes" (py:32-36, py:145-149)
//   rd_waiter             the polling policy of every host wait: spin, then yield, then sleep, with a deadline
//   rd_bq_windows_of      BURST QUALITY: a record's packet, sync and noise windows (inline: the kernel evaluates it too)
//   rd_bs_range           BURST SEARCH: a chunk's candidate positions (inline: the kernel evaluates it too)
//   rd_bc_window_of       BURST CLIPS: a request's clamp to the two chunks and to whole vectors (inline: the kernel evaluates it too)
//   rd_msg_repeats        steps 7, 7' and 7s: a record that reports again what the fetch of the chunk before delivered
//   rd_delivered          ... and what that fetch delivered
//   rd_collect_*          the receiver's fetch: one slot's records into the handle's vectors, every count checked first
//   rd_collect_block      the streaming demodulator's fetch: one slot's records, ordered, and their parsed messages
//   rd_order_parsed       a batch run's parsed messages in the order parse() sees them, a call's repeats dropped
// py = /root/reference/src/rtldavis/dsp.py
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/rtldavis_hip.h"
#include "rd_slots.h"

struct rd_devcfg {
    int32_t S, P, K, B, L, PL, nbytes;  // symbol_length, preamble/packet symbols, block, buffer, preamble_length
    uint64_t pre_mask;                  // bit m = preamble symbol m
    double fs;                          // sample rate = bit_rate * symbol_length (protocol.py:309)
};

// The Davis shape (protocol.py:68-76), the one the compile-time kernels are built for: 14 samples per symbol, the preamble
// 1100101110001001 (bit m of the mask = symbol m -> 0x91D3), 80 packet symbols.  The search has no use for the packet's
// length, the slice none for the preamble.
static inline bool rd_davis_search(const rd_devcfg &c) { return c.S == 14 && c.P == 16 && c.pre_mask == 0x91D3ull; }
static inline bool rd_davis_slice(const rd_devcfg &c) { return c.S == 14 && c.K == 80; }
static inline bool rd_davis_shape(const rd_devcfg &c) { return rd_davis_search(c) && c.K == 80; }

// RD_OK or RD_ERR_ARG; *why (never null on failure) names the offending field
int rd_make_devcfg(const rd_config *c, rd_devcfg *d, const char **why);

// Reference order inside one call: search is phase-major then ascending (py:175-186), slice keeps the first
// occurrence of each byte string (py:203-205).  Records are ordered by (stream, call, index % S, index); records with
// stream < 0 (a match reported by no call) are skipped.  Fills sc.kept with the indices of the records to return.
struct rd_order_scratch {  // kept per handle: no allocation per call once warm
    std::vector<uint32_t> idx, itmp, kept;
    std::vector<uint64_t> key, ktmp;
};
void rd_order_and_dedupe(const rd_packet *recs, size_t n, int S, rd_order_scratch &sc);

// k_tail: matches one stream's list must hold.  Noise gives one raw preamble match per 2^16 positions
// (~4 per second of a Davis stream), a burst a handful around its true position; the
// capacity is 4x the noise expectation plus 12 for bursts, rounded up to a multiple of 32, at least 32 and at
// most RD_BUCKET_MAX.
#define RD_BUCKET_MIN 32
#define RD_BUCKET_MAX 512
uint32_t rd_ord_bucket_cap(long n_samples);

// py:32-36 / py:145-149: RD_OK when `count` elements are what one call takes (complex: B samples of one stream;
// uint8: NS * 2B bytes), else RD_ERR_ARG with *expected set
int rd_check_block_count(int is_complex, size_t count, size_t B, size_t NS, size_t *expected);

// Steps 7, 7' and 7s (include/rtldavis_hip.h: BURST DECODE, BURST EXPECT, BURST SEARCH): record m reports again a packet
// that the fetch of the chunk before delivered - one of `delivered` has its channel and data and a time less than sl
// outputs from m's on the 64-bit clock.  The fetch drops such a record (rd_collect_*).  look_back: only a record that
// looked back (flags & 1) can repeat; same_centre: the two also share pad[3], for each centre gives its own record.
bool rd_msg_repeats(const rd_burst_msg &m, const rd_burst_msg *delivered, size_t n_delivered, int sl, bool look_back, bool same_centre);
static inline bool rd_bd_repeats(const rd_burst_msg &m, const rd_burst_msg *d, size_t n, int sl) { return rd_msg_repeats(m, d, n, sl, true, false); }
static inline bool rd_bx_repeats(const rd_burst_msg &m, const rd_burst_msg *d, size_t n, int sl) { return rd_msg_repeats(m, d, n, sl, false, false); }
static inline bool rd_bs_repeats(const rd_burst_msg &m, const rd_burst_msg *d, size_t n, int sl) { return rd_msg_repeats(m, d, n, sl, false, true); }
// What the fetch of chunk `chunk` delivered (last) and, while the next fetch collects, what the one before it delivered
// (prev), against which a record is a repeat.  A chunk that was never fetched delivered nothing: chunk = -1 while a
// collection is unfinished (it may fail) and -2 after reset(), when the fetch of chunk 0 looks for chunk -1 and must not
// take the run before for it.
struct rd_delivered {
    std::vector<rd_burst_msg> last, prev;
    long chunk = -1;
    void begin(long k) {
        if (chunk == k - 1) prev.swap(last);
        else prev.clear();
        chunk = -1;
        last.clear();
    }
    void commit(long k) { chunk = k; }
    void forget() { chunk = -2; prev.clear(); }
    bool repeats(const rd_burst_msg &m, int sl, bool look_back, bool same_centre) const {
        return rd_msg_repeats(m, prev.data(), prev.size(), sl, look_back, same_centre);
    }
};

// The receiver's fetch (rd_wideband.hip: wb_fetched), one function per slot kind.  `slot` is what the kernels of chunk
// `chunk` wrote (rd_slots.h) and is only read; every header is checked - it carries the chunk's number, its counts fit
// the slot - before a record place it bounds is read.  RD_OK, or RD_ERR_DEVICE with the message in err: a record of
// another chunk here would be an ordering bug, not something to hand on.  The outputs are undefined after a failure.
struct rd_errtext { char text[320]; };
int rd_collect_levels(const void *slot, int n_ch, long chunk, std::vector<rd_chan_level> &lv, rd_input_level *in, rd_errtext *err);
int rd_collect_spectrum(const void *slot, int n_bins, long chunk, rd_spectrum_info *info, std::vector<double> &power, rd_errtext *err);
// a channel's runs are the first n_bursts of its cap = rd_bu_cap(n_win) record places
int rd_collect_bursts(const void *slot, int n_ch, size_t n_win, long chunk, std::vector<rd_burst> &runs, std::vector<rd_burst_floor> &floor,
                      rd_errtext *err);
// a channel's messages are the first n_msgs of its cap record places; step 7 against hist, the kept ones into hist.last.
// qslot (null: quality off): record i of the quality slot belongs to record i of the message slot and goes where it goes.
int rd_collect_decode(const void *slot, const void *qslot, int n_ch, size_t n_win, long chunk, int sl, rd_delivered &hist,
                      std::vector<uint32_t> &long_runs, std::vector<rd_burst_quality> &qual, rd_errtext *err);
// n: the size of the table the chunk was submitted with, cand: the host's candidate counts; slot null: the submit launched
// nothing, zero records.  counts: RD_BX_MAX of them, RD_BX_NO_ENTRY from n on.  Step 7' against hist.
int rd_collect_expect(const void *slot, const void *qslot, int n_ch, size_t n_win, long chunk, int sl, int n, const uint32_t *cand,
                      rd_delivered &hist, uint32_t *counts, std::vector<rd_burst_quality> &qual, rd_errtext *err);
// n: the size of the list the chunk was submitted with (0: nothing is read).  Step 7s against hist.
int rd_collect_search(const void *slot, int n_ch, long chunk, int sl, int n, rd_delivered &hist, std::vector<rd_bs_header> &hdr,
                      rd_errtext *err);
// a channel's clips are the first n_clips of its record places, its bytes the first 2 * used of its pool of 2 * quota - only
// those are copied, packed channel after channel, and `offset` is rewritten to match
int rd_collect_clips(const void *slot, int n_ch, int quota, long chunk, std::vector<rd_burst_clip> &clips, std::vector<uint8_t> &bytes,
                     std::vector<uint32_t> &dropped, rd_errtext *err);

// The streaming demodulator's fetch (rd_stream.hip: demod_fetch) of one slot, which the block's kernels wrote into mapped
// memory and which is only read.  counts: n_lists counts; list i's records are the first counts[i] of the `per` places
// from recs + i * per - the one-launch form has a list per stream with per = B + 1, the multi-launch form one list of
// match_cap places.  A count beyond `per` is clamped to it, so no place outside the slot is read.  fe: null (the block
// was submitted with parse off) or the entries beside the record places: RD_FE_NONE or the record's frequency error.
// last: the records in the reference's order, per-call duplicates gone (rd_order_and_dedupe).  parsed: of those, the ones
// the device found CRC-valid, as messages with the bytes swapped here (rd_parse.h) - the parser's own dedupe on the
// swapped bytes (protocol.py:293-295) has nothing left to drop: the swap is a bijection and the per-call dedupe has run.
struct rd_block_scratch {  // kept per handle: no allocation per call once warm
    std::vector<rd_packet> recs;
    std::vector<int32_t> fe;
    rd_order_scratch order;
};
void rd_collect_block(const uint32_t *counts, size_t n_lists, size_t per, const rd_packet *recs, const int32_t *fe, int S,
                      rd_block_scratch &sc, std::vector<rd_packet> &last, std::vector<rd_parsed> &parsed);
// The parsed messages of a batch run, in place, into the order parse() sees them - packets of a call in _slice's order:
// (stream, call, index % S, index) - with a call's repeated byte strings dropped (py:203-205, the first occurrence wins:
// messages with equal bytes come from packets with equal bytes, the sync word being the matched preamble).  Returns how
// many are kept, at the front.
size_t rd_order_parsed(rd_parsed *recs, size_t n, int S);

// BURST EXPECT (include/rtldavis_hip.h), the host's parts.
// rd_bx_check_table: RD_OK, or RD_ERR_ARG with *bad = the first offending entry (-1: n itself) and *why naming the rule.
// rd_bx_range: the candidates of one expectation in the chunk whose first output has clock `clock`: false when it is
// idle there, else *tau_a <= *tau_b, the least and greatest tau with t_lo <= clock + tau <= t_hi on the 64-bit clock
// (every difference is taken modulo 2^64, so a clock near the wrap is like any other), 0 <= tau + sl (n_sym - 1) <
// block_size, and tau - sl >= 0 unless have_prev.  Needs t_hi - t_lo <= RD_BX_MAX_SPAN (rd_bx_check_table).
int rd_bx_check_table(const rd_expect *e, int n, int n_channels, int *bad, const char **why);
bool rd_bx_range(int sl, int n_sym, int block_size, int have_prev, uint64_t clock, uint64_t t_lo, uint64_t t_hi, int32_t *tau_a,
                 int32_t *tau_b);

// CLIP DECODE (include/rtldavis_hip.h): the rule of a job list, rd_cd_check_jobs, is part of the C ABI and declared there
// (rd_host.cpp, beside rd_bx_check_table).

// BURST SEARCH (include/rtldavis_hip.h), the parts that need no device.
// rd_bs_check_centres: RD_OK, or RD_ERR_ARG with *why naming the rule and *bad the offending centre's index (-1: the
// count n outside 0 .. RD_BS_MAX_CENTRES or a null list) - a centre >= RD_BD_NB_GRID, or one that repeats an earlier one.
// rd_bs_range: step 2s - false when the chunk has no candidate, else *tau_a .. *tau_b = max(lo + sl, -sl (n_sym - 1)) ..
// block_size - 1 - sl (n_sym - 1), lo = have_prev ? -look : 0 (defined below, inline).
int rd_bs_check_centres(const uint8_t *centres, int n, int *bad, const char **why);

// BURST QUALITY (include/rtldavis_hip.h): the three windows of a record whose first symbol ends at tau, as half-open
// ranges of outputs relative to the chunk's first - packet [p0, p1), sync [p0, s1), noise [n0, n1) with n1 - n0 = n_noise
// (n0 = n1 = p0 when the intersection with t >= lo_lim is empty).  rd_bq_windows_of: false, and *w zeroed, for a record
// that is not measurable - sl < 1, n_sym < 16, block_size < 1, gap < 0, p0 < lo_lim or p1 > block_size; tau is taken as a
// 64-bit value so that no record overflows the test.  The one definition serves the host (rd_bq_window, the C form the
// tests call) and k_chan_burst_quality, which checks every record again before it indexes anything.
#if defined(__HIPCC__)
#define RD_HOST_DEVICE __host__ __device__
#else
#define RD_HOST_DEVICE
#endif
// (rd_bs_range: the one definition serves the host's tests and k_chan_burst_search, which walks exactly this range)
RD_HOST_DEVICE static inline bool rd_bs_range(int sl, int n_sym, int block_size, int look, int have_prev, int32_t *tau_a, int32_t *tau_b) {
    if (sl < 1 || n_sym < 1 || block_size < 1 || look < 0 || !tau_a || !tau_b) return false;
    const int64_t body = (int64_t)sl * (int64_t)(n_sym - 1);
    const int64_t lo = have_prev ? -(int64_t)look : 0;
    const int64_t a = lo + sl > -body ? lo + sl : -body, b = (int64_t)block_size - 1 - body;
    if (b < a || a < INT32_MIN || b > INT32_MAX) return false;
    *tau_a = (int32_t)a;
    *tau_b = (int32_t)b;
    return true;
}
struct rd_bq_windows {
    int32_t p0, p1, s1, n0, n1;
};
RD_HOST_DEVICE static inline bool rd_bq_windows_of(int sl, int n_sym, int block_size, int have_prev, int64_t tau, int gap,
                                                   rd_bq_windows *w) {
    w->p0 = w->p1 = w->s1 = w->n0 = w->n1 = 0;
    if (sl < 1 || n_sym < 16 || block_size < 1 || gap < 0) return false;
    if (tau < -((int64_t)1 << 40) || tau > ((int64_t)1 << 40)) return false;   // (far outside any chunk; no sum below overflows)
    const int64_t lo_lim = have_prev ? -(int64_t)block_size : 0;
    const int64_t p0 = tau - (int64_t)sl + 1, p1 = p0 + (int64_t)n_sym * (int64_t)sl;
    if (p0 < lo_lim || p1 > (int64_t)block_size) return false;
    int64_t n1 = p0 - (int64_t)gap, n0 = n1 - 16 * (int64_t)sl;
    if (n0 < lo_lim) n0 = lo_lim;
    if (n1 <= n0) n0 = n1 = p0;                                  // nothing left of it
    w->p0 = (int32_t)p0;
    w->p1 = (int32_t)p1;
    w->s1 = (int32_t)(p0 + 16 * (int64_t)sl);
    w->n0 = (int32_t)n0;
    w->n1 = (int32_t)n1;
    return true;
}
// (rd_bq_window, include/rtldavis_hip.h, is the same through the C ABI)

// BURST CLIPS (include/rtldavis_hip.h): the clamp-and-round rule of one request [a, e) - t0 = max(a, lo_lim) rounded down to
// a multiple of 8, t1 = min(e, block_size) rounded up, n = t1 - t0, flags bits 0 .. 2.  false, and *c zeroed, for a request
// that gives no clip: e <= a, nothing of it inside lo_lim .. block_size, or a block_size that is no positive multiple of 8.
// a and e are 64-bit values and no request overflows the test.  The one definition serves the host (rd_bc_window, the C
// form the tests call) and k_chan_burst_clips, which bounds every copy by it.
struct rd_bc_clamped {
    int32_t t0, n, flags;
};
RD_HOST_DEVICE static inline bool rd_bc_window_of(int block_size, int have_prev, int64_t a, int64_t e, rd_bc_clamped *c) {
    c->t0 = c->n = c->flags = 0;
    if (block_size < 8 || (block_size & 7)) return false;
    const int64_t B = block_size, lo_lim = have_prev ? -B : 0;
    if (e <= a || a >= B || e <= lo_lim) return false;          // (from here on lo_lim - 7 <= every value below <= B)
    const int64_t t0 = (a > lo_lim ? a : lo_lim) & ~(int64_t)7;  // (two's complement: rounds towards minus infinity)
    const int64_t t1 = ((e < B ? e : B) + 7) & ~(int64_t)7;
    c->t0 = (int32_t)t0;
    c->n = (int32_t)(t1 - t0);
    c->flags = (a < lo_lim ? RD_BC_CUT_START : 0) | (e > B ? RD_BC_CUT_END : 0) | (t0 < 0 ? RD_BC_FROM_PREV : 0);
    return true;
}
// (rd_bc_window, include/rtldavis_hip.h, is the same through the C ABI)

// Host waits poll (the runtime's blocking waits add 10-20 ms of wake-up latency on this platform).  A wait spins on
// `pause` for the first ~50 us, then yields the core, then sleeps 50 us at a time; it gives up at its deadline.
struct rd_waiter {
    double t_start_ms, timeout_ms;
    uint32_t polls;
    explicit rd_waiter(double timeout_ms_);
    // call after an unsuccessful poll: false when the deadline has passed (the caller reports a timeout)
    bool relax();
    double waited_ms() const;
};
// RD_WAIT_TIMEOUT_MS (read once; default 10000) unless rd_set_wait_timeout_ms has set another value
double rd_wait_timeout_ms(void);
// returns the previous value; ms < 0 restores the environment's / default value.  0 = every wait that is not
// already satisfied at its first poll times out (the test hook of tests/test_gpu_parity.py::test_host_wait_deadline)
double rd_wait_timeout_set(double ms);
