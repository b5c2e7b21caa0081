// batch_plan_asan.cpp - the decisions of the batch demodulator (rtldavis_amd/csrc/rd_batch_plan.cpp) under
// -fsanitize=address,undefined, driven by tests/test_batch_plan_sanitizers.py.  A stand-alone program:
//   batch_plan_asan ladder    one step of the overflow ladder against the flat loop body it replaced, over the cross product
//   batch_plan_asan runs      whole ladders over scripted counters with a fake device: named scenarios
//   batch_plan_asan sizes     the sizes of a handle against the flat expressions, the create limit, the hooks
//   batch_plan_asan plan      the launch plan of a run, all 256 inputs, against the three launch branches it replaced
//   batch_plan_asan counts    what results() copies, around every min(), and that no copy leaves the record array
// "old_*": a literal restatement of rd_batch.hip as it was before the decisions moved into rd_batch_plan.cpp - one flat
// handle, every HIP call replaced by a token appended to a list.  The new code runs against the same tokens.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../rtldavis_amd/csrc/rd_batch_plan.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

// tokens: what the runtime would have been asked to do
enum : uint32_t { T_FIXUP_ALL = 1, T_STAMP, T_ZERO, T_SEARCH_SLICE, T_WAIT, T_GROW = 0x80000000u /* | new match_cap */,
                  T_EV0 = 16, T_EV1, T_KFIRST, T_DEMOD_NONE, T_DEMOD_TIMED, T_DEMOD_KFIRST, T_ADOPT_EV1, T_ADOPT_KFIRST };
typedef std::vector<uint32_t> tokens;

// ---------------------------------------------------------------------------------------------------------------------
// The flat handle of before, as far as the ladder reads and writes it, and its "device": the counters every pass will
// read back (the last entry repeats).
// ---------------------------------------------------------------------------------------------------------------------
struct old_batch {
    bool fast_ok = true, ran = true, fetched = false;
    bool dev_order = false, tail_off = false, ft_run = false, ft_sticky = false, second_pass = false;
    uint32_t fix_cap = 4096, match_cap = 1000, ft_limit = 0, ft_bcap = 32;
    uint64_t last_fix = 0, last_match = 0, all_runs = 1234567;
    uint32_t h_cnt[RD_CNT_SLOTS] = {};
    tokens tok;
    std::vector<std::vector<uint32_t>> script;   // {FIX, MATCH, OVF} per pass
    size_t pass = 0;
};
static void script_read(old_batch *b, uint32_t *cnt) {
    const std::vector<uint32_t> &c = b->script[std::min(b->pass, b->script.size() - 1)];
    b->pass++;
    memset(cnt, 0, RD_CNT_SLOTS * sizeof(uint32_t));
    cnt[RD_CNT_FIX] = c[0]; cnt[RD_CNT_MATCH] = c[1]; cnt[RD_CNT_OVF] = c[2];
}
static int old_alloc_lists(old_batch *b, uint32_t match_cap) {
    b->tok.push_back(T_GROW | match_cap);
    b->match_cap = match_cap;
    return 0;
}
static int old_search_slice(old_batch *b) {   // (may_defer = false: the separate kernels, an event of its own)
    b->dev_order = false;
    b->tok.push_back(T_SEARCH_SLICE);
    return 0;
}
static int old_second_pass(old_batch *b) {
    b->tok.push_back(T_ZERO);
    b->second_pass = true;
    return old_search_slice(b);
}
// the body of batch_finish's loop: 1 = return RD_OK, 0 = next attempt
static int old_attempt(old_batch *b, int attempt) {
    b->tok.push_back(T_WAIT);
    script_read(b, b->h_cnt);
    bool redo_search = false;
    if (b->ft_run && !b->second_pass && (b->h_cnt[RD_CNT_OVF] & (8u | 16u))) {
        b->tok.push_back(T_FIXUP_ALL);
        b->last_fix = b->all_runs;
        b->tail_off = true;
        b->h_cnt[RD_CNT_OVF] = 0;
        b->h_cnt[RD_CNT_FIX] = 0;
        redo_search = true;
    } else if (b->ft_run && !b->second_pass && (b->h_cnt[RD_CNT_OVF] & 1u)) {
        if (!b->ft_limit && b->ft_bcap < RD_BUCKET_MAX) b->ft_bcap = std::min<uint32_t>(2 * b->ft_bcap, RD_BUCKET_MAX);
        else if (!b->ft_limit) b->ft_sticky = true;
    }
    if (redo_search) {
    } else if (b->fast_ok && !b->ft_run && b->h_cnt[RD_CNT_FIX] > b->fix_cap) {
        b->tok.push_back(T_FIXUP_ALL);
        b->tok.push_back(T_STAMP);
        b->last_fix = b->all_runs;
        redo_search = true;
    } else if (attempt == 0) {
        b->last_fix = (uint64_t)b->h_cnt[RD_CNT_FIX];
    }
    if (redo_search && b->tail_off) b->dev_order = false;
    if (b->dev_order && b->h_cnt[RD_CNT_OVF]) {
        b->tail_off = true;
        int rc2 = old_second_pass(b);
        CHECK(!rc2);
        return 0;
    }
    if (!b->dev_order && b->h_cnt[RD_CNT_MATCH] > b->match_cap) {
        int rc2 = old_alloc_lists(b, b->h_cnt[RD_CNT_MATCH] + b->h_cnt[RD_CNT_MATCH] / 4 + 1024);
        CHECK(!rc2);
        redo_search = true;
    }
    if (!redo_search) {
        b->last_match = b->h_cnt[RD_CNT_MATCH];
        b->fetched = true;
        return 1;
    }
    int rc2 = old_second_pass(b);
    CHECK(!rc2);
    return 0;
}
static int old_finish(old_batch *b) {   // RD_OK, or RD_ERR_DEVICE: "result lists kept overflowing"
    for (int attempt = 0; attempt < 8; attempt++)
        if (old_attempt(b, attempt)) return RD_OK;
    return RD_ERR_DEVICE;
}

// ---------------------------------------------------------------------------------------------------------------------
// The new ladder over the same scripted device: the run's state and the lists' capacity live in the fake, what inputs
// teach the handle in rd_batch_learned.
// ---------------------------------------------------------------------------------------------------------------------
struct fake_dev {
    old_batch s;            // the same fields, driven by the new code (tail_off, ft_sticky, ft_bcap, last_* unused: they are in lr)
    int read(rd_ladder_in &in) {
        s.tok.push_back(T_WAIT);
        script_read(&s, s.h_cnt);
        in = {s.h_cnt[RD_CNT_FIX], s.h_cnt[RD_CNT_MATCH], s.h_cnt[RD_CNT_OVF], s.ft_run, s.second_pass, s.dev_order, s.fast_ok, 0,
              s.fix_cap, s.match_cap, s.ft_limit, s.all_runs};
        return RD_OK;
    }
    int carry_out(const rd_ladder_action &a) {
        s.dev_order = a.dev_order;
        if (a.exact_fixup) s.tok.push_back(T_FIXUP_ALL);
        if (a.stamp_fix) s.tok.push_back(T_STAMP);
        if (a.grow_to) { s.tok.push_back(T_GROW | a.grow_to); s.match_cap = a.grow_to; }
        if (a.second_pass) { s.tok.push_back(T_ZERO); s.second_pass = true; s.dev_order = false; s.tok.push_back(T_SEARCH_SLICE); }
        if (a.done) s.fetched = true;
        CHECK(!a.done || !(a.exact_fixup || a.stamp_fix || a.grow_to || a.second_pass));
        return RD_OK;
    }
    int gave_up() { return RD_ERR_DEVICE; }
};
static rd_batch_learned learned_of(const old_batch &b) {
    rd_batch_learned lr;
    lr.tail_off = b.tail_off; lr.ft_sticky = b.ft_sticky; lr.bcap = b.ft_bcap; lr.last_fix = b.last_fix; lr.last_match = b.last_match;
    return lr;
}
static void check_same(const old_batch &o, const fake_dev &d, const rd_batch_learned &lr) {
    CHECK(o.tok == d.s.tok);
    CHECK(o.dev_order == d.s.dev_order && o.second_pass == d.s.second_pass && o.fetched == d.s.fetched && o.match_cap == d.s.match_cap);
    CHECK(o.ft_run == d.s.ft_run && o.fast_ok == d.s.fast_ok && o.fix_cap == d.s.fix_cap && o.ft_limit == d.s.ft_limit);
    CHECK(o.tail_off == lr.tail_off && o.ft_sticky == lr.ft_sticky && o.ft_bcap == lr.bcap);
    CHECK(o.last_fix == lr.last_fix && o.last_match == lr.last_match);
}

static int test_ladder(void) {
    const uint32_t ovfs[9] = {0, 1, 2, 3, 8, 9, 16, 24, 27};
    const uint32_t bcaps[3] = {RD_BUCKET_MIN, 128, RD_BUCKET_MAX};
    long cases = 0, done = 0, passes = 0;
    for (int flags = 0; flags < 64; flags++)
        for (uint32_t ovf : ovfs)
            for (int df = -1; df <= 1; df++)
                for (int dm = -1; dm <= 1; dm++)
                    for (int attempt = 0; attempt < 8; attempt++)
                        for (uint32_t bcap : bcaps)
                            for (uint32_t ft_limit : {0u, 2u}) {
                                old_batch o;
                                o.ft_run = flags & 1; o.second_pass = flags & 2; o.dev_order = flags & 4; o.fast_ok = flags & 8;
                                o.tail_off = flags & 16; o.ft_sticky = flags & 32;
                                o.ft_bcap = bcap; o.ft_limit = ft_limit;
                                o.last_fix = 77; o.last_match = 88;
                                o.script = {{o.fix_cap + df, o.match_cap + dm, ovf}};
                                fake_dev d;
                                d.s = o;
                                rd_batch_learned lr = learned_of(o);
                                const int fin = old_attempt(&o, attempt);
                                rd_ladder_in in;
                                CHECK(d.read(in) == RD_OK);
                                in.attempt = attempt;
                                const rd_ladder_action a = rd_batch_ladder_step(in, lr);
                                CHECK(d.carry_out(a) == RD_OK);
                                CHECK(a.done == (fin == 1));
                                check_same(o, d, lr);
                                cases++;
                                done += a.done;
                                passes += a.second_pass;
                            }
    printf("ladder ok %ld steps %ld done %ld passes\n", cases, done, passes);
    return 0;
}

// A named scenario: the run's flags after rd_batch_run, the counters pass by pass; both ladders must agree and end as stated.
struct scenario {
    const char *name;
    bool k_tail;                                  // the run's first pass was the one-launch tail (ft_run, dev_order)
    uint32_t ft_bcap, ft_limit;
    std::vector<std::vector<uint32_t>> script;    // {FIX, MATCH, OVF}
    int rc, waits;                                // the ladder's result and how many passes it waited for
    bool tail_off, ft_sticky;
    uint32_t bcap_after;
    uint64_t last_fix;
    uint32_t forms;                               // rd_batch_last_run_forms
    uint32_t match_cap_after;
};
static int test_runs(void) {
    const uint32_t KT = RD_FORM_ORDERED_TAIL | RD_FORM_ONE_LAUNCH_TAIL, SP = RD_FORM_SECOND_PASS;
    const uint64_t ALL = 1234567;   // (old_batch::all_runs)
    // fix_cap 4096, match_cap 1000 at the start
    const std::vector<scenario> all = {
        {"clean, k_tail", true, 32, 0, {{300, 40, 0}}, RD_OK, 1, false, false, 32, 300, KT, 1000},
        {"clean, separate kernels", false, 32, 0, {{300, 40, 0}}, RD_OK, 1, false, false, 32, 300, 0, 1000},
        {"guard list overflowed", false, 32, 0, {{5000, 40, 0}, {4096, 41, 0}}, RD_OK, 2, false, false, 32, ALL, SP, 1000},
        {"match list grown once", false, 32, 0, {{300, 1500, 0}, {300, 1500, 0}}, RD_OK, 2, false, false, 32, 300, SP, 1500 + 375 + 1024},
        {"match list grown twice", false, 32, 0, {{300, 1500, 0}, {300, 9000, 0}, {300, 9000, 0}}, RD_OK, 3, false, false, 32, 300, SP,
         9000 + 2250 + 1024},
        {"LDS list overflow -> separate kernels", true, 32, 0, {{300, 40, 1}, {300, 90, 0}}, RD_OK, 2, true, false, 64, 300, SP, 1000},
        {"LDS list overflow under RD_TEST_BUCKET_CAP", true, 32, 2, {{300, 40, 1}, {300, 90, 0}}, RD_OK, 2, true, false, 32, 300, SP, 1000},
        {"LDS list overflow of the longest lists", true, RD_BUCKET_MAX, 0, {{300, 40, 1}, {300, 90, 0}}, RD_OK, 2, true, true, RD_BUCKET_MAX, 300,
         SP, 1000},
        {"bucket overflow -> exact re-evaluation -> separate kernels", true, 32, 0, {{9999, 40, 8}, {0, 90, 0}}, RD_OK, 2, true, false, 32, ALL,
         SP, 1000},
        {"a workgroup gave up waiting", true, 32, 0, {{300, 40, 16}, {0, 90, 0}}, RD_OK, 2, true, false, 32, ALL, SP, 1000},
        {"bucket overflow, then the match list grows", true, 32, 0, {{300, 40, 8}, {0, 1200, 0}, {0, 1200, 0}}, RD_OK, 3, true, false, 32, ALL, SP,
         1200 + 300 + 1024},
        {"record array overflow", true, 32, 0, {{300, 40, 2}, {300, 90, 0}}, RD_OK, 2, true, false, 32, 300, SP, 1000},
        {"never settles", false, 32, 0, {{300, 0xF0000000u, 0}}, RD_ERR_DEVICE, 8, false, false, 32, 300, SP, 0xF0000000u + 0x3C000000u + 1024},
    };
    for (const scenario &sc : all) {
        old_batch o;
        o.ft_run = o.dev_order = sc.k_tail;
        o.ft_bcap = sc.ft_bcap; o.ft_limit = sc.ft_limit;
        o.script = sc.script;
        fake_dev d;
        d.s = o;
        rd_batch_learned lr = learned_of(o);
        const int rc_old = old_finish(&o);
        const int rc_new = rd_batch_ladder_run(d, lr);
        if (rc_old != rc_new || rc_new != sc.rc) { fprintf(stderr, "%s: rc %d / %d\n", sc.name, rc_old, rc_new); return 1; }
        check_same(o, d, lr);
        const long waits = std::count(d.s.tok.begin(), d.s.tok.end(), (uint32_t)T_WAIT);
        const uint32_t forms = (d.s.dev_order ? KT : 0u) | (d.s.second_pass ? SP : 0u);
        if (waits != sc.waits || lr.tail_off != sc.tail_off || lr.ft_sticky != sc.ft_sticky || lr.bcap != sc.bcap_after ||
            lr.last_fix != sc.last_fix || forms != sc.forms || d.s.match_cap != sc.match_cap_after || d.s.fetched != (sc.rc == RD_OK)) {
            fprintf(stderr, "%s: waits %ld tail_off %d sticky %d bcap %u last_fix %llu forms %u match_cap %u\n", sc.name, waits, lr.tail_off,
                    lr.ft_sticky, lr.bcap, (unsigned long long)lr.last_fix, forms, d.s.match_cap);
            return 1;
        }
        // a second call for the same run (results() after last_run_forms()): one wait, nothing launched, nothing learned anew
        if (sc.rc == RD_OK) {
            const size_t n_tok = d.s.tok.size();
            const rd_batch_learned before = lr;
            d.s.pass--;   // (the pinned counters still hold the last pass)
            o.pass--;
            CHECK(rd_batch_ladder_run(d, lr) == RD_OK && old_finish(&o) == RD_OK);
            CHECK(d.s.tok.size() == n_tok + 1 && d.s.tok.back() == T_WAIT);
            CHECK(lr.tail_off == before.tail_off && lr.ft_sticky == before.ft_sticky && lr.bcap == before.bcap);
            check_same(o, d, lr);
        }
    }
    printf("runs ok %zu scenarios\n", all.size());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// sizes: batch_alloc's expressions between its hipMalloc calls, as they stood (the environment as four strings)
// ---------------------------------------------------------------------------------------------------------------------
struct old_sizes {
    long n_samples; size_t bits_stride; bool fast_ok;
    size_t iq_bytes; uint32_t fix_cap, match_cap; bool ft_ok; size_t groups, cnt_stride, ft_cnt_off; uint32_t fix_bcap, bcap, ft_limit;
};
static old_sizes old_sizes_of(int n_streams, int n_blocks, const rd_config *cfg, const rd_devcfg &dc, const char *tail_impl,
                              const char *env_match, const char *env_bucket, const char *env_fixb) {
    old_sizes b = {};
    const long n = (long)n_blocks * cfg->block_size;
    b.n_samples = n;
    b.bits_stride = (size_t)((n + 31) / 32);
    b.fast_ok = ((size_t)n * 2) % 16 == 0;
    const uint64_t runs = (uint64_t)n_streams * b.bits_stride;
    b.iq_bytes = (size_t)n_streams * b.n_samples * 2;
    b.fix_cap = (uint32_t)std::min<uint64_t>(runs, std::max<uint64_t>(4096, runs / 8));
    uint32_t match_cap = (uint32_t)std::min<uint64_t>((uint64_t)n_streams * (8 + 1ull * n_blocks) + 1024, 1u << 26);
    if (const char *e = env_match) {
        const long v = atol(e);
        if (v >= 1 && v < (long)match_cap) match_cap = (uint32_t)v;
    }
    b.match_cap = match_cap;
    {
        const char *ti = tail_impl;
        const bool legacy = ti && ti[0] == 'l';
        b.ft_ok = !legacy && b.fast_ok && rd_davis_shape(dc) &&
                  b.n_samples < (1l << 30) && dc.B < (1 << 24) && b.bits_stride % 4 == 0 && dc.L >= dc.B &&
                  (long)(n_blocks + 1) * dc.B - dc.L >= 0 &&
                  ((long)(n_blocks + 1) * dc.B - dc.L) / 32 + 16 <= (long)b.bits_stride;
        if (const char *e = env_bucket) {
            const long v = atol(e);
            if (v >= 1 && v < RD_BUCKET_MIN) b.ft_limit = (uint32_t)v;
        }
    }
    b.cnt_stride = RD_CNT_TOTAL;
    if (b.ft_ok) {
        const size_t groups = ((size_t)n_streams + RD_FT_STREAMS - 1) / RD_FT_STREAMS;
        b.groups = groups;
        b.ft_cnt_off = b.cnt_stride;
        b.cnt_stride += (groups + 3) & ~(size_t)3;
        const uint64_t tps = ((uint64_t)b.n_samples + RD_TILE_SAMPLES - 1) / RD_TILE_SAMPLES;
        b.fix_bcap = (uint32_t)std::min<uint64_t>((2 * RD_FT_STREAMS * (tps / 4 + 8) + 63) & ~63ull, 1u << 20);
        if (const char *e = env_fixb) {
            const long v = atol(e);
            if (v >= 1 && v < (long)b.fix_bcap) b.fix_bcap = (uint32_t)v;
        }
        b.bcap = rd_ord_bucket_cap(b.n_samples);
    }
    return b;
}
static int old_check_size(const rd_config *cfg, int n_streams, int n_blocks, const char **msg) {   // rd_batch_create's rule
    if (n_streams < 1 || n_blocks < 1) { *msg = "n_streams and n_blocks must be >= 1"; return RD_ERR_ARG; }
    const long n = (long)n_blocks * cfg->block_size;
    const uint64_t runs = (uint64_t)n_streams * ((n + 32 - 1) / 32);
    if (n > 0x7FFFFFF0L || runs > 0x0FFFFFFFull) {
        *msg = "batch too large: at most 2^28 32-sample runs (8.6e9 samples) per batch";
        return RD_ERR_ARG;
    }
    *msg = "";
    return RD_OK;
}

static rd_config config(int S, int K, int B) {
    rd_config c;
    memset(&c, 0, sizeof c);
    c.bit_rate = 19200; c.symbol_length = S; c.preamble_symbols = 16; c.packet_symbols = K; c.block_size = B;
    const char *pre = "1100101110001001";
    for (int i = 0; i < 16; i++) c.preamble[i] = (uint8_t)(pre[i] - '0');
    return c;
}
// absent / below / at / above a threshold, as the environment's string
static const char *hook_str(int which, long threshold, char *buf) {
    if (which == 0) return nullptr;
    snprintf(buf, 32, "%ld", threshold + which - 2);
    return buf;
}

static int test_sizes(void) {
    // the Davis shape; Davis symbols in blocks of 96 (bits_stride % 4 and the packet's room vary with n_blocks); 10 samples per
    // symbol in blocks of 4100 (streams not always 16-byte aligned); 64 packet symbols
    const rd_config cfgs[4] = {config(14, 80, 8192), config(14, 80, 96), config(10, 80, 4100), config(14, 64, 8192)};
    long cases = 0, with_ft = 0;
    for (const rd_config &cfg : cfgs) {
        rd_devcfg dc;
        const char *why = nullptr;
        CHECK(rd_make_devcfg(&cfg, &dc, &why) == RD_OK);
        for (int n_streams : {1, 3, 4, 5, 13, 4096})
            for (int n_blocks : {1, 2, 5, 33, 330, 792}) {
                const old_sizes plain = old_sizes_of(n_streams, n_blocks, &cfg, dc, nullptr, nullptr, nullptr, nullptr);
                for (int legacy = 0; legacy < 2; legacy++)
                    for (int hm = 0; hm < 4; hm++)
                        for (int hb = 0; hb < 4; hb++)
                            for (int hf = 0; hf < 4; hf++) {
                                char sm[32], sb[32], sf[32];
                                const char *em = hook_str(hm, plain.match_cap, sm), *eb = hook_str(hb, RD_BUCKET_MIN, sb);
                                const char *ef = hook_str(hf, plain.ft_ok ? plain.fix_bcap : 64, sf), *ti = legacy ? "legacy" : nullptr;
                                const old_sizes o = old_sizes_of(n_streams, n_blocks, &cfg, dc, ti, em, eb, ef);
                                rd_batch_hooks h;
                                h.legacy_tail = legacy;
                                if (em) h.match_cap = atol(em);
                                if (eb) h.bucket_cap = atol(eb);
                                if (ef) h.fix_bcap = atol(ef);
                                const rd_batch_sizes z = rd_batch_sizes_of(n_streams, n_blocks, dc, h);
                                CHECK(z.n_samples == o.n_samples && z.bits_stride == o.bits_stride && z.fast_ok == o.fast_ok);
                                CHECK(z.iq_bytes == o.iq_bytes && z.fix_cap == o.fix_cap && z.match_cap == o.match_cap && z.ft_ok == o.ft_ok);
                                CHECK(z.groups == o.groups && z.cnt_stride == o.cnt_stride && z.ft_cnt_off == o.ft_cnt_off);
                                CHECK(z.fix_bcap == o.fix_bcap && z.bcap == o.bcap && z.ft_limit == o.ft_limit);
                                // a hook shortens a list below its threshold and does nothing at or above it
                                CHECK(z.match_cap == (hm == 1 && plain.match_cap > 1 ? plain.match_cap - 1 : plain.match_cap));
                                CHECK(z.ft_limit == (hb == 1 ? RD_BUCKET_MIN - 1 : 0u));
                                if (z.ft_ok) CHECK(z.fix_bcap == (hf == 1 ? plain.fix_bcap - 1 : plain.fix_bcap));
                                cases++;
                                with_ft += z.ft_ok;
                            }
                // what create derives before any hook is read is what the first device call derives again
                const rd_batch_sizes at_create = rd_batch_sizes_of(n_streams, n_blocks, dc, rd_batch_hooks());
                CHECK(at_create.n_samples == plain.n_samples && at_create.bits_stride == plain.bits_stride && at_create.fast_ok == plain.fast_ok);
            }
    }
    // the hooks from the environment: unset, set, not a number, RD_TAIL_IMPL by its first letter
    for (const char *name : {"RD_TAIL_IMPL", "RD_TEST_MATCH_CAP", "RD_TEST_BUCKET_CAP", "RD_TEST_FIX_BCAP"}) unsetenv(name);
    rd_batch_hooks h = rd_batch_hooks_env();
    CHECK(!h.legacy_tail && h.match_cap == 0 && h.bucket_cap == 0 && h.fix_bcap == 0);
    setenv("RD_TAIL_IMPL", "legacy", 1); setenv("RD_TEST_MATCH_CAP", "8", 1); setenv("RD_TEST_BUCKET_CAP", "2", 1); setenv("RD_TEST_FIX_BCAP", "x", 1);
    h = rd_batch_hooks_env();
    CHECK(h.legacy_tail && h.match_cap == 8 && h.bucket_cap == 2 && h.fix_bcap == 0);
    setenv("RD_TAIL_IMPL", "fused", 1); setenv("RD_TEST_FIX_BCAP", "-3", 1);
    h = rd_batch_hooks_env();
    CHECK(!h.legacy_tail && h.fix_bcap == -3);
    for (const char *name : {"RD_TAIL_IMPL", "RD_TEST_MATCH_CAP", "RD_TEST_BUCKET_CAP", "RD_TEST_FIX_BCAP"}) unsetenv(name);

    // the create limit, on both sides: counts below 1; 0x7FFFFFF0 samples per stream; 2^28 - 1 runs per batch
    long limits = 0;
    const rd_config big = config(14, 80, 0x7FFFFFF);   // (x 16 blocks = 0x7FFFFFF0 samples, 2^26 runs)
    struct { const rd_config *cfg; int ns, nb; } cases_lim[] = {
        {&cfgs[0], 0, 1}, {&cfgs[0], 1, 0}, {&cfgs[0], -1, 5}, {&cfgs[0], 1, 1},
        {&big, 1, 16}, {&big, 1, 17}, {&big, 3, 16}, {&big, 4, 16},        // 0x7FFFFFF0 samples | more; 3 x 2^26 runs | 2^28
        {&cfgs[0], 4096, 255}, {&cfgs[0], 4096, 256},                     // 4096 x 255 x 256 runs = 2^28 - 2^20 | 2^28
        {&cfgs[0], 1048575, 1}, {&cfgs[0], 1048576, 1},                   // 256 runs a stream: 2^28 - 256 | 2^28
        {&cfgs[1], 0x0FFFFFFF / 3, 1}, {&cfgs[1], 0x0FFFFFFF / 3 + 1, 1},  // 3 runs a stream: 2^28 - 1 | 2^28 + 2
    };
    for (auto &c : cases_lim) {
        const char *mo = nullptr, *mn = nullptr;
        const int ro = old_check_size(c.cfg, c.ns, c.nb, &mo), rn = rd_batch_check_size(c.ns, c.nb, c.cfg->block_size, &mn);
        CHECK(ro == rn && !strcmp(mo, mn));
        limits++;
    }
    const char *m = nullptr;
    CHECK(rd_batch_check_size(1, 16, big.block_size, &m) == RD_OK);
    CHECK(rd_batch_check_size(1, 17, big.block_size, &m) == RD_ERR_ARG && !strcmp(m, "batch too large: at most 2^28 32-sample runs (8.6e9 samples) per batch"));
    CHECK(rd_batch_check_size(0x0FFFFFFF / 3, 1, 96, &m) == RD_OK && rd_batch_check_size(0x0FFFFFFF / 3 + 1, 1, 96, &m) == RD_ERR_ARG);
    CHECK(rd_batch_check_size(0, 1, 8192, &m) == RD_ERR_ARG && !strcmp(m, "n_streams and n_blocks must be >= 1"));
    printf("sizes ok %ld cases %ld with the one-launch tail %ld limits\n", cases, with_ft, limits);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// the launch plan: rd_batch_run's three branches around the demod launch, and batch_search_slice's choice of the last event
// ---------------------------------------------------------------------------------------------------------------------
struct old_run { tokens tok; bool want_ft, defer; uint32_t last, last_again; };
static old_run old_run_of(const rd_run_mode &m) {
    old_run o;
    const bool adopt = m.parked;
    o.want_ft = m.ft_ok && m.fast_ok && !m.tail_off && !(m.timing && m.timing_detail);
    if (m.timing && m.fast_ok) {
        o.tok.push_back(T_DEMOD_TIMED);
        if (adopt) o.tok.push_back(T_ADOPT_EV1);
    } else if (m.fast_ok && adopt) {
        o.tok.push_back(T_DEMOD_KFIRST);
        o.tok.push_back(T_ADOPT_KFIRST);
    } else {
        if (m.timing) o.tok.push_back(T_EV0);
        if (m.fast_ok) o.tok.push_back(T_DEMOD_NONE);
        if (m.timing) o.tok.push_back(T_EV1);
        if (adopt) {
            if (!m.timing) o.tok.push_back(T_KFIRST);
            o.tok.push_back(m.timing ? T_ADOPT_EV1 : T_ADOPT_KFIRST);
        }
    }
    // batch_search_slice, may_defer = true and then false
    const bool last_on_slice = !m.parse;
    o.defer = true && m.pipelined && last_on_slice && !(m.timing && m.timing_detail);
    o.last = o.defer ? RD_RUN_EV_NONE : m.timing ? RD_RUN_EV4 : RD_RUN_KDONE;
    o.last_again = m.timing ? RD_RUN_EV4 : RD_RUN_KDONE;
    return o;
}
// rd_batch_run's launch sequence by the plan
static tokens run_tokens(const rd_run_plan &p) {
    tokens t;
    if (p.record_around) t.push_back(T_EV0);
    if (p.demod) {
        CHECK((p.ride_start == RD_RUN_EV_NONE && (p.ride_stop == RD_RUN_EV_NONE || p.ride_stop == RD_RUN_KFIRST)) ||
              (p.ride_start == RD_RUN_EV0 && p.ride_stop == RD_RUN_EV1));
        t.push_back(p.ride_start == RD_RUN_EV0 ? T_DEMOD_TIMED : p.ride_stop == RD_RUN_KFIRST ? T_DEMOD_KFIRST : T_DEMOD_NONE);
    }
    if (p.record_around) t.push_back(T_EV1);
    if (p.record_carrier) { CHECK(p.carrier == RD_RUN_KFIRST); t.push_back(T_KFIRST); }
    if (p.carrier) { CHECK(p.carrier == RD_RUN_EV1 || p.carrier == RD_RUN_KFIRST); t.push_back(p.carrier == RD_RUN_EV1 ? T_ADOPT_EV1 : T_ADOPT_KFIRST); }
    return t;
}
static int test_plan(void) {
    long n = 0, buckets = 0, defers = 0;
    for (int bits = 0; bits < 256; bits++) {
        const rd_run_mode m = {(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0, (bits & 16) != 0, (bits & 32) != 0,
                               (bits & 64) != 0, (bits & 128) != 0};
        const old_run o = old_run_of(m);
        const rd_run_plan p = rd_batch_plan_run(m);
        CHECK(run_tokens(p) == o.tok);
        CHECK(p.demod == m.fast_ok && p.buckets == o.want_ft && p.defer == o.defer && p.end == o.last && p.end_again == o.last_again);
        // an event of the timed run's five is named by a timed run only: an untimed handle has none
        for (rd_run_event e : {p.ride_start, p.ride_stop, p.carrier, p.end, p.end_again})
            CHECK(m.timing || (e != RD_RUN_EV0 && e != RD_RUN_EV1 && e != RD_RUN_EV4));
        CHECK((p.carrier != RD_RUN_EV_NONE) == m.parked);
        n++;
        buckets += p.buckets;
        defers += p.defer;
    }
    printf("plan ok %ld inputs %ld with buckets %ld deferred\n", n, buckets, defers);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// what rd_batch_results copies: batch_readback's `spec`, rd_batch_results' `have`, nprim and nextra
// ---------------------------------------------------------------------------------------------------------------------
static int test_counts(void) {
    long n = 0;
    for (uint32_t match_cap : {1u, 7u, 1000u, 1u << 26}) {
        const uint32_t rec_cap = 2 * match_cap;
        std::vector<uint32_t> around = {0, 1, 1023, 1024, 1025, 0xFFFFFFFFu};
        for (uint32_t c : {match_cap, rec_cap})
            for (int d = -1; d <= 1; d++)
                if ((int64_t)c + d >= 0) around.push_back(c + d);
        for (uint32_t spec_recs : around)
            for (int dense = 0; dense < 2; dense++)
                for (int dev_order = 0; dev_order < 2; dev_order++)
                    for (uint32_t matches : around)
                        for (uint32_t tasks : around)
                            for (uint32_t recs : around) {
                                uint32_t h_cnt[RD_CNT_SLOTS] = {};
                                h_cnt[RD_CNT_MATCH] = matches; h_cnt[RD_CNT_TASKS] = tasks; h_cnt[RD_CNT_REC] = recs;
                                // as they stood
                                const uint32_t spec = std::min(dev_order ? rec_cap : match_cap, spec_recs);
                                const uint32_t nprim = dense ? std::min(h_cnt[RD_CNT_TASKS], rec_cap) : std::min(h_cnt[RD_CNT_MATCH], match_cap);
                                const uint32_t nextra = dense ? 0u : std::min(h_cnt[RD_CNT_REC], match_cap);
                                const uint32_t have = std::min(dev_order ? rec_cap : match_cap, spec_recs);
                                const uint32_t got_have = rd_batch_spec_count(dev_order, match_cap, rec_cap, spec_recs);
                                const rd_result_counts c = rd_batch_result_counts(h_cnt, dense, match_cap, rec_cap);
                                CHECK(got_have == spec && got_have == have && c.nprim == nprim && c.nextra == nextra);
                                // the speculative copy [0, have), the late one [have, nprim) and the twins [nprim, nprim + nextra)
                                // on the host, [match_cap, match_cap + nextra) on the device: all inside rec_cap records
                                CHECK(have <= rec_cap);
                                if (c.nprim > have) CHECK((uint64_t)have + (c.nprim - have) <= rec_cap);
                                CHECK((uint64_t)c.nprim + c.nextra <= rec_cap && (uint64_t)match_cap + c.nextra <= rec_cap);
                                n++;
                            }
    }
    printf("counts ok %ld cases\n", n);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "ladder")) return test_ladder();
    if (argc == 2 && !strcmp(argv[1], "runs")) return test_runs();
    if (argc == 2 && !strcmp(argv[1], "sizes")) return test_sizes();
    if (argc == 2 && !strcmp(argv[1], "plan")) return test_plan();
    if (argc == 2 && !strcmp(argv[1], "counts")) return test_counts();
    fprintf(stderr, "usage: batch_plan_asan ladder|runs|sizes|plan|counts\n");
    return 2;
}
