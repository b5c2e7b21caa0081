// rd_batch_plan.h - the decisions of the batch demodulator (rd_batch.hip), as pure host code: nothing in here touches HIP,
// so rd_batch_plan.cpp is compiled into the library by hipcc AND into tests/_build/batch_plan_asan by a host compiler with
// -fsanitize=address,undefined (tests/test_batch_plan_sanitizers.py).  rd_batch.hip carries the decisions out.
//   rd_batch_check_size     the size rule of rd_batch_create
//   rd_batch_sizes_of       every size batch_alloc allocates by, from the shape and the test hooks
//   rd_batch_plan_run       which events ride on a run's demod dispatch, who carries an adoption, what ends the run
//   rd_batch_ladder_step    one rung of the overflow ladder: the counters read back -> what to launch, what to remember
//   rd_batch_ladder_run     the ladder's loop: read, step, carry out, at most RD_BATCH_ATTEMPTS times
//   rd_batch_result_counts  what rd_batch_results copies
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rd_host.h"

// counters[] slots (device uint32)
// FIX: flagged runs; MATCH: preamble matches (= primary records); REC: second records of
// block-boundary positions; PARSED: CRC-valid messages
// OVF: the one-launch tail could not hold this input (1: a stream with more matches than its list, 2: more records
// than the output array has room for, 8: a group's fix-up bucket overflowed, 16: a workgroup gave up waiting for the
// totals of the groups in front of it)
enum { RD_CNT_FIX = 0, RD_CNT_MATCH = 1, RD_CNT_REC = 2, RD_CNT_TASKS = 3, RD_CNT_PARSED = 4, RD_CNT_OVF = 5, RD_CNT_SLOTS = 8 };
// RD_CNT_FIX: entries in the global fix-up list (k_fixup's input; written by k_tail as the sum over its groups' buckets)
// The one-launch tail (rd_tail.hip: k_tail): a workgroup owns RD_FT_STREAMS consecutive streams
#define RD_FT_GSH 2
#define RD_FT_STREAMS (1 << RD_FT_GSH)
// Behind the RD_CNT_SLOTS counters the host reads back: the demod kernel's work queues (chunks handed out beyond
// the first one of every wave).  One counter word sustains ~90 atomics per microsecond, so there are RD_NQUEUE of
// them, 256 bytes apart; wave w draws from queue w % RD_NQUEUE, which owns the chunks nwaves + q + RD_NQUEUE k.
#define RD_NQUEUE 32
#define RD_QUEUE_STRIDE 64                                     /* words */
#define RD_CNT_QUEUE0 RD_QUEUE_STRIDE                          /* first queue's word index */
#define RD_CNT_TOTAL (RD_CNT_QUEUE0 + RD_NQUEUE * RD_QUEUE_STRIDE)  /* words per counter set */
#define RD_TILE_SAMPLES 2048  // 64 lanes x 32 samples: one wave iteration of the fused demod kernel
#define RD_BATCH_RUN 32       // samples per packed output word (rd_math.h: RD_RUN)
#define RD_BATCH_ATTEMPTS 8   // passes of the overflow ladder before "result lists kept overflowing"

// --- sizes ---
// RD_OK, or RD_ERR_ARG with *why the message of rd_batch_create: both counts >= 1, at most 0x7FFFFFF0 samples per stream
// and 2^28 32-sample runs per batch
int rd_batch_check_size(int n_streams, int n_blocks, int block_size, const char **why);

// The hooks of a handle, as the environment held them at its first device call (rd_batch_hooks_env).  A count of 0: absent.
struct rd_batch_hooks {
    bool legacy_tail = false;  // RD_TAIL_IMPL=legacy: the separate kernels + host ordering (A/B)
    long match_cap = 0;        // RD_TEST_MATCH_CAP: a short first match list, so that the lists grow on ordinary inputs
    long bucket_cap = 0;       // RD_TEST_BUCKET_CAP: short per-stream match lists in k_tail's LDS
    long fix_bcap = 0;         // RD_TEST_FIX_BCAP: small fix-up buckets
};
rd_batch_hooks rd_batch_hooks_env(void);

struct rd_batch_sizes {
    long n_samples = 0;       // per stream
    size_t bits_stride = 0;   // words per stream
    bool fast_ok = false;     // 16-byte aligned streams for the demod kernel's LDS-DMA loads
    size_t iq_bytes = 0;
    uint32_t fix_cap = 0;     // guard-band list: one entry per flagged 32-sample run (~1.5 % of the runs on noise)
    uint32_t match_cap = 0;   // the first lists: ~16 raw matches per 33-block stream on noise + one burst; they grow on overflow
    // the one-launch tail's buffers exist: Davis shape, RD_TAIL_IMPL unset, every index of k_tail in range
    bool ft_ok = false;
    size_t groups = 0;                    // workgroups of k_tail (0 without it)
    size_t cnt_stride = RD_CNT_TOTAL;     // words per counter set: the groups' fix-up counters live behind the counters ...
    size_t ft_cnt_off = 0;                // ... from this word on, cleared with the set
    uint32_t fix_bcap = 0;                // entries of a group's fix-up bucket
    uint32_t bcap = 0;                    // matches a stream's list in LDS holds at first (rd_ord_bucket_cap)
    uint32_t ft_limit = 0;                // RD_TEST_BUCKET_CAP where it applies (0: none)
};
rd_batch_sizes rd_batch_sizes_of(int n_streams, int n_blocks, const rd_devcfg &dc, const rd_batch_hooks &hooks);

// --- the launch plan of a run ---
// Events by role: the timed run's five (ev[0] .. ev[4]), kfirst (the stop event of an untimed demod launch that adopts
// another run) and kdone (behind an untimed run's last kernel).
enum rd_run_event : uint8_t { RD_RUN_EV_NONE = 0, RD_RUN_EV0, RD_RUN_EV1, RD_RUN_EV4, RD_RUN_KFIRST, RD_RUN_KDONE };
struct rd_run_plan {
    bool demod = false;        // the demod kernel runs (else k_fixup evaluates every run exactly)
    bool buckets = false;      // its fix-up entries go to the groups' buckets: the one-launch tail
    rd_run_event ride_start = RD_RUN_EV_NONE, ride_stop = RD_RUN_EV_NONE;  // events on the demod dispatch itself
    bool record_around = false;   // ev[0] and ev[1] are recorded around the (absent) demod launch instead
    rd_run_event carrier = RD_RUN_EV_NONE;  // the event a run parked on the launch stream is adopted by (none: nothing parked)
    bool record_carrier = false;  // ... which nothing has put on the stream yet
    bool defer = false;           // the tail carries no event: the run parks and waits for an adopter
    rd_run_event end = RD_RUN_EV_NONE;      // the event that ends the run's first pass (none: deferred) ...
    rd_run_event end_again = RD_RUN_EV_NONE;  // ... and a second pass, which never defers
};
struct rd_run_mode {
    bool fast_ok, ft_ok, tail_off, timing, timing_detail, pipelined, parse;
    bool parked;  // a pipelined run waits on the launch stream
};
rd_run_plan rd_batch_plan_run(const rd_run_mode &m);

// --- the overflow ladder ---
// What inputs have taught the handle.
struct rd_batch_learned {
    bool tail_off = false;    // an input overflowed k_tail's lists: the separate kernels + host ordering until the next upload
    bool ft_sticky = false;   // ... and they were the longest lists there are: uploads no longer re-enable k_tail
    uint32_t bcap = 0;        // matches a stream's list in k_tail's LDS holds (doubles when an input overflows it)
    uint32_t spec_recs = 1024;  // records copied back speculatively with the counters: the last run's count + 25 %
    uint64_t last_fix = 0, last_match = 0;  // rd_batch_get_counters
};
struct rd_ladder_in {
    uint32_t fix, match, ovf;          // the counters read back: RD_CNT_FIX, RD_CNT_MATCH, RD_CNT_OVF
    bool ft_run, second_pass, dev_order, fast_ok;
    int attempt;                       // 0 .. RD_BATCH_ATTEMPTS - 1
    uint32_t fix_cap, match_cap, ft_limit;
    uint64_t all_runs;                 // n_streams * bits_stride: what last_fix reports after an exact re-evaluation
};
// In the order they are carried out.
struct rd_ladder_action {
    bool exact_fixup = false;    // k_fixup re-evaluates every run exactly
    bool stamp_fix = false;      // fix_cap goes into the device's FIX counter: the guard rung must not see the count again
    uint32_t grow_to = 0;        // new lists for this many matches (0: keep them)
    bool second_pass = false;    // search and slice again with the separate kernels, over cleared lists
    bool done = false;           // the run is complete: nothing above is set
    bool dev_order = false;      // the run's records are (still) the device-ordered ones of k_tail
    bool tail_overflow = false;  // (diagnostic print) k_tail's match lists or the record array overflowed
};
rd_ladder_action rd_batch_ladder_step(const rd_ladder_in &in, rd_batch_learned &lr);
// The ladder as a whole, over whatever carries it out - the handle (rd_batch.hip: batch_ladder) or a test's scripted device:
//   int read(rd_ladder_in &in)                  wait for the pass in flight, fill in its counters and the run's state
//   int carry_out(const rd_ladder_action &a)    launch what the step decided, take over dev_order, note `done`
//   int gave_up()                               the error after RD_BATCH_ATTEMPTS passes that all overflowed
// Each returns RD_OK or the error that ends the ladder.
template <class Dev>
int rd_batch_ladder_run(Dev &dev, rd_batch_learned &lr) {
    for (int attempt = 0; attempt < RD_BATCH_ATTEMPTS; attempt++) {
        rd_ladder_in in = {};
        int rc = dev.read(in);
        if (rc) return rc;
        in.attempt = attempt;
        const rd_ladder_action a = rd_batch_ladder_step(in, lr);
        if ((rc = dev.carry_out(a))) return rc;
        if (a.done) return RD_OK;
    }
    return dev.gave_up();
}

// --- what rd_batch_results copies ---
// records copied back with the counters, before their number is known
uint32_t rd_batch_spec_count(bool dev_order, uint32_t match_cap, uint32_t rec_cap, uint32_t spec_recs);
// sparse layout: one slot per match + the block-boundary twins behind match_cap; dense: one record per task.  nprim
// records from index 0 - those beyond the speculative count are still to be copied - and nextra from index match_cap,
// placed behind the nprim on the host: nprim + nextra <= rec_cap = 2 * match_cap.
struct rd_result_counts { uint32_t nprim, nextra; };
rd_result_counts rd_batch_result_counts(const uint32_t *h_cnt, bool dense, uint32_t match_cap, uint32_t rec_cap);
