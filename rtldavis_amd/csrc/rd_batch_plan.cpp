// rd_batch_plan.cpp - see rd_batch_plan.h.  Pure host code: compiled by hipcc into the library and by a host compiler with
// -fsanitize into tests/_build/batch_plan_asan (tests/test_batch_plan_sanitizers.py).
#include "rd_batch_plan.h"

#include <stdlib.h>

#include <algorithm>

int rd_batch_check_size(int n_streams, int n_blocks, int block_size, const char **why) {
    if (n_streams < 1 || n_blocks < 1) { *why = "n_streams and n_blocks must be >= 1"; return RD_ERR_ARG; }
    const long n = (long)n_blocks * block_size;
    const uint64_t runs = (uint64_t)n_streams * ((n + RD_BATCH_RUN - 1) / RD_BATCH_RUN);
    if (n > 0x7FFFFFF0L || runs > 0x0FFFFFFFull) {
        *why = "batch too large: at most 2^28 32-sample runs (8.6e9 samples) per batch";
        return RD_ERR_ARG;
    }
    *why = "";
    return RD_OK;
}

rd_batch_hooks rd_batch_hooks_env(void) {
    rd_batch_hooks h;
    const char *ti = getenv("RD_TAIL_IMPL");
    h.legacy_tail = ti && ti[0] == 'l';
    if (const char *e = getenv("RD_TEST_MATCH_CAP")) h.match_cap = atol(e);
    if (const char *e = getenv("RD_TEST_BUCKET_CAP")) h.bucket_cap = atol(e);
    if (const char *e = getenv("RD_TEST_FIX_BCAP")) h.fix_bcap = atol(e);
    return h;
}

rd_batch_sizes rd_batch_sizes_of(int n_streams, int n_blocks, const rd_devcfg &dc, const rd_batch_hooks &hooks) {
    rd_batch_sizes z;
    const long n = (long)n_blocks * dc.B;
    z.n_samples = n;
    z.bits_stride = (size_t)((n + 31) / 32);
    z.fast_ok = ((size_t)n * 2) % 16 == 0;
    const uint64_t runs = (uint64_t)n_streams * z.bits_stride;
    z.iq_bytes = (size_t)n_streams * n * 2;
    z.fix_cap = (uint32_t)std::min<uint64_t>(runs, std::max<uint64_t>(4096, runs / 8));
    z.match_cap = (uint32_t)std::min<uint64_t>((uint64_t)n_streams * (8 + 1ull * n_blocks) + 1024, 1u << 26);
    // every hook applies below its threshold only: it makes a list shorter, never longer
    if (hooks.match_cap >= 1 && hooks.match_cap < (long)z.match_cap) z.match_cap = (uint32_t)hooks.match_cap;
    z.ft_ok = !hooks.legacy_tail && z.fast_ok && rd_davis_shape(dc) &&
              n < (1l << 30) && dc.B < (1 << 24) && z.bits_stride % 4 == 0 && dc.L >= dc.B &&
              (long)(n_blocks + 1) * dc.B - dc.L >= 0 &&   // (a batch shorter than a packet has no position to report)
              ((long)(n_blocks + 1) * dc.B - dc.L) / 32 + 16 <= (long)z.bits_stride;
    if (hooks.bucket_cap >= 1 && hooks.bucket_cap < RD_BUCKET_MIN) z.ft_limit = (uint32_t)hooks.bucket_cap;
    if (!z.ft_ok) return z;
    z.groups = ((size_t)n_streams + RD_FT_STREAMS - 1) / RD_FT_STREAMS;
    z.ft_cnt_off = z.cnt_stride;
    z.cnt_stride += (z.groups + 3) & ~(size_t)3;
    // a group's bucket: the first group of every chunk of tiles (chunks of four tiles at the least) and the first
    // run of each of its streams are always listed; twice that, plus room for the groups inside the guard band
    const uint64_t tps = ((uint64_t)n + RD_TILE_SAMPLES - 1) / RD_TILE_SAMPLES;
    z.fix_bcap = (uint32_t)std::min<uint64_t>((2 * RD_FT_STREAMS * (tps / 4 + 8) + 63) & ~63ull, 1u << 20);
    if (hooks.fix_bcap >= 1 && hooks.fix_bcap < (long)z.fix_bcap) z.fix_bcap = (uint32_t)hooks.fix_bcap;
    z.bcap = rd_ord_bucket_cap(n);
    return z;
}

// An event on a run's last kernel idles the GPU before the next kernel starts; one on the demod dispatch costs nothing
// (rd_batch.hip: pipelined completion).  So whatever can ride on the demod dispatch does: a timed run's ev[0] / ev[1], or
// kfirst when an untimed run adopts.  Without a demod kernel (streams not 16-byte aligned) the same events are recorded
// on the stream where the kernel would have been.
rd_run_plan rd_batch_plan_run(const rd_run_mode &m) {
    rd_run_plan p;
    p.demod = m.fast_ok;
    p.buckets = m.ft_ok && m.fast_ok && !m.tail_off && !(m.timing && m.timing_detail);
    if (m.timing && m.fast_ok) {
        p.ride_start = RD_RUN_EV0;
        p.ride_stop = RD_RUN_EV1;
    } else if (m.fast_ok && m.parked) {
        p.ride_stop = RD_RUN_KFIRST;
    }
    p.record_around = m.timing && !m.fast_ok;
    if (m.parked) {
        p.carrier = m.timing ? RD_RUN_EV1 : RD_RUN_KFIRST;
        p.record_carrier = !m.timing && !m.fast_ok;   // (a timed run's ev[1] is on the stream either way)
    }
    // the run's last kernel is the slice (the parse kernel follows it otherwise); a detailed timing wants every event
    p.defer = m.pipelined && !m.parse && !(m.timing && m.timing_detail);
    p.end_again = m.timing ? RD_RUN_EV4 : RD_RUN_KDONE;
    p.end = p.defer ? RD_RUN_EV_NONE : p.end_again;
    return p;
}

// The rungs, in the order they are tested (DESIGN.md has the table):
//   1  k_tail ran and a group's fix-up bucket overflowed (OVF & 8) or a workgroup gave up waiting (OVF & 16)
//   1' k_tail ran and a stream's match list in LDS overflowed (OVF & 1): only remembered here, rung 3 acts on it
//   2  the separate kernels ran and the global guard list overflowed (FIX > fix_cap)
//   3  k_tail's records are in use and any overflow flag is up (OVF & 1: a list in LDS, OVF & 2: the record array)
//   4  the separate kernels' match list overflowed (MATCH > match_cap)
// A run that took rung 1 or 2 goes on to rung 4 in the same step; rung 3 ends the step.
rd_ladder_action rd_batch_ladder_step(const rd_ladder_in &in, rd_batch_learned &lr) {
    rd_ladder_action a;
    a.dev_order = in.dev_order;
    const bool first_ft = in.ft_run && !in.second_pass;
    bool redo = false;
    if (first_ft && (in.ovf & (8u | 16u))) {
        a.exact_fixup = redo = true;
        lr.last_fix = in.all_runs;
        lr.tail_off = true;
        a.dev_order = false;
    } else {
        if (first_ft && (in.ovf & 1u)) {   // this input takes the separate kernels, the next upload gets lists twice as long
            if (!in.ft_limit && lr.bcap < RD_BUCKET_MAX) lr.bcap = std::min<uint32_t>(2 * lr.bcap, RD_BUCKET_MAX);
            else if (!in.ft_limit) lr.ft_sticky = true;   // (the longest lists there are: inputs like this one keep the separate kernels)
        }
        if (in.fast_ok && !in.ft_run && in.fix > in.fix_cap) {   // degenerate input
            a.exact_fixup = a.stamp_fix = redo = true;
            lr.last_fix = in.all_runs;
            if (lr.tail_off) a.dev_order = false;
        } else if (in.attempt == 0) {
            lr.last_fix = in.fix;
        }
        if (a.dev_order && in.ovf) {   // now and until the next upload
            lr.tail_off = true;
            a.tail_overflow = a.second_pass = true;
            return a;
        }
    }
    if (!a.dev_order && in.match > in.match_cap) {
        a.grow_to = in.match + in.match / 4 + 1024;
        redo = true;
    }
    a.second_pass = redo;
    a.done = !redo;
    if (a.done) lr.last_match = in.match;
    return a;
}

uint32_t rd_batch_spec_count(bool dev_order, uint32_t match_cap, uint32_t rec_cap, uint32_t spec_recs) {
    return std::min(dev_order ? rec_cap : match_cap, spec_recs);
}

rd_result_counts rd_batch_result_counts(const uint32_t *h_cnt, bool dense, uint32_t match_cap, uint32_t rec_cap) {
    rd_result_counts c;
    c.nprim = dense ? std::min(h_cnt[RD_CNT_TASKS], rec_cap) : std::min(h_cnt[RD_CNT_MATCH], match_cap);
    c.nextra = dense ? 0u : std::min(h_cnt[RD_CNT_REC], match_cap);
    return c;
}
