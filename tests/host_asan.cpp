// Sanitizer harness for the pure-host translation unit of the C ABI (rtldavis_amd/csrc/rd_host.cpp).
// TEST INFRASTRUCTURE ONLY: built by tests/test_host_sanitizers.py with
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all host_asan.cpp ../rtldavis_amd/csrc/rd_host.cpp
// and run on the CPU (the GPU pool allows no sanitizer runs).  Exit code 0 = every check held and
// no sanitizer report.
//   host_asan soak <rounds> <seed>     random record sets through rd_order_and_dedupe against a naive model
//   host_asan file <in> <out> <S>      rd_packet records from <in>, kept indices (uint32) to <out>
//   host_asan config <rounds> <seed>   rd_make_devcfg / rd_check_block_count / rd_ord_bucket_cap on random and extreme input
//   host_asan waiter                   rd_waiter: deadline 0, a short deadline, the override hook
//   host_asan shape                    rd_davis_shape / _search / _slice: the condition of each of their seven sites
//   host_asan repeats <msgs> <delivered> <out> <SL>   rd_burst_msg records through rd_bd_repeats, kept indices (uint32) to <out>
//   host_asan block <n_lists> <per> <S> <counts> <recs> <fe|-> <last> <parsed>   one streaming slot through rd_collect_block
//   host_asan parsed <in> <out> <S>    rd_parsed records from <in> through rd_order_parsed, the kept ones to <out>
//   host_asan parsed-soak <rounds> <seed>   random rd_parsed sets through rd_order_parsed against a naive model
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>
#include <algorithm>

#include "../rtldavis_amd/csrc/rd_host.h"

static int fail(const char *what) { fprintf(stderr, "host_asan: %s\n", what); return 1; }

// the reference's rule, spelled out naively: stable order by (stream, call, index % S, index), then first occurrence
// of a byte string inside (stream, call) wins (py:171-205)
static std::vector<uint32_t> naive(const std::vector<rd_packet> &r, int S) {
    std::vector<uint32_t> idx;
    for (size_t i = 0; i < r.size(); i++) if (r[i].stream >= 0) idx.push_back((uint32_t)i);
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
        const rd_packet &x = r[a], &y = r[b];
        if (x.stream != y.stream) return x.stream < y.stream;
        if (x.call != y.call) return x.call < y.call;
        if (x.index % S != y.index % S) return x.index % S < y.index % S;
        return x.index < y.index;
    });
    std::vector<uint32_t> kept;
    for (uint32_t i : idx) {
        bool dup = false;
        for (uint32_t k : kept)
            if (r[k].stream == r[i].stream && r[k].call == r[i].call && memcmp(r[k].data, r[i].data, (size_t)r[i].nbytes) == 0) { dup = true; break; }
        if (!dup) kept.push_back(i);
    }
    return kept;
}

static int soak(int rounds, unsigned seed) {
    std::mt19937 g(seed);
    rd_order_scratch sc;  // reused across rounds, like a handle's
    for (int round = 0; round < rounds; round++) {
        const int S = 1 + (int)(g() % 20);
        const size_t n = (round % 3 == 0) ? g() % 40 : (round % 3 == 1) ? 400 + g() % 400 : 2000 + g() % 3000;
        const int n_streams = 1 + (int)(g() % (round % 5 == 0 ? 100000 : 50)), n_calls = 1 + (int)(g() % 40);
        const int n_index = 1 + (int)(g() % (round % 7 == 0 ? (1 << 24) : 9000)), n_bytes = 1 + (int)(g() % RD_MAX_PKT_BYTES);
        const int n_payloads = 1 + (int)(g() % 6);
        std::vector<rd_packet> r(n);
        for (auto &p : r) {
            memset(&p, 0, sizeof p);
            p.stream = (g() % 16 == 0) ? -1 : (int)(g() % n_streams);
            p.call = (int)(g() % n_calls);
            p.index = (int)(g() % n_index);
            p.nbytes = n_bytes;
            // few distinct payloads (duplicates inside a call are common), a function of the position like a real
            // packet's bytes: records with equal (stream, call, index) are then equal everywhere the order could show
            const unsigned pay = (unsigned)(p.index % n_payloads) + 7u * (unsigned)(p.stream & 1);
            for (int k = 0; k < n_bytes; k++) p.data[k] = (uint8_t)(pay * 37 + k);
        }
        rd_order_and_dedupe(r.data(), r.size(), S, sc);
        const std::vector<uint32_t> want = naive(r, S);
        if (want.size() != sc.kept.size()) return fail("kept count differs from the naive model");
        for (size_t i = 0; i < want.size(); i++) {
            const rd_packet &a = r[want[i]], &b = r[sc.kept[i]];
            if (a.stream != b.stream || a.call != b.call || a.index != b.index || memcmp(a.data, b.data, (size_t)a.nbytes))
                return fail("kept record differs from the naive model");
        }
    }
    rd_order_and_dedupe(nullptr, 0, 14, sc);
    if (!sc.kept.empty()) return fail("empty input kept something");
    printf("soak ok: %d rounds\n", rounds);
    return 0;
}

static int file_mode(const char *in, const char *out, int S) {
    FILE *f = fopen(in, "rb");
    if (!f) return fail("cannot open input");
    std::vector<rd_packet> r;
    rd_packet p;
    while (fread(&p, sizeof p, 1, f) == 1) r.push_back(p);
    fclose(f);
    rd_order_scratch sc;
    rd_order_and_dedupe(r.data(), r.size(), S, sc);
    f = fopen(out, "wb");
    if (!f) return fail("cannot open output");
    if (!sc.kept.empty() && fwrite(sc.kept.data(), 4, sc.kept.size(), f) != sc.kept.size()) return fail("short write");
    fclose(f);
    return 0;
}

static int config(int rounds, unsigned seed) {
    std::mt19937 g(seed);
    const int32_t extremes[] = {0, 1, -1, 4, 31, 32, 36, 512, 8192, 1 << 20, 0x3FFFFFFF, 0x7FFFFFFF, (int32_t)0x80000000};
    auto pick = [&]() -> int32_t { return (g() % 3) ? extremes[g() % (sizeof extremes / sizeof extremes[0])] : (int32_t)(g() % 100000) - 10; };
    int ok = 0;
    for (int i = 0; i < rounds; i++) {
        rd_config c;
        memset(&c, 0, sizeof c);
        c.bit_rate = pick(); c.symbol_length = pick(); c.preamble_symbols = (g() % 2) ? pick() : 1 + (int)(g() % 64);
        c.packet_symbols = (g() % 2) ? pick() : 1 + (int)(g() % 256); c.block_size = (g() % 2) ? pick() : 4 * (8 + (int)(g() % 4096));
        for (int k = 0; k < RD_MAX_PREAMBLE; k++) c.preamble[k] = (uint8_t)((g() % 50 == 0) ? 2 : g() & 1);
        rd_devcfg d;
        memset(&d, 0, sizeof d);
        const char *why = nullptr;
        const int rc = rd_make_devcfg(&c, &d, &why);
        if (rc != RD_OK && rc != RD_ERR_ARG) return fail("unexpected status");
        if (!why) return fail("why left null");
        if (rc == RD_OK) {
            ok++;
            if (d.L < 2 * d.B || d.L % d.B || d.PL != d.P * d.S || d.nbytes != (d.K + 7) / 8 || d.nbytes > RD_MAX_PKT_BYTES)
                return fail("derived constants inconsistent");
        } else if (!*why) return fail("failure without a reason");
    }
    {   // the production shape (protocol.py:68-76)
        rd_config c = {19200, 14, 16, 80, 8192, {1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 0, 1, 0, 0, 1}};
        rd_devcfg d;
        const char *why;
        if (rd_make_devcfg(&c, &d, &why) != RD_OK || d.L != 16384 || d.PL != 224 || d.nbytes != 10 || d.pre_mask != 0x91D3ull || d.fs != 268800.0)
            return fail("production shape");
        if (rd_make_devcfg(nullptr, &d, &why) != RD_ERR_ARG || rd_make_devcfg(&c, &d, nullptr) != RD_OK) return fail("null handling");
    }
    if (rd_ord_bucket_cap(33 * 8192) != 32 || rd_ord_bucket_cap(330 * 8192) != 192 || rd_ord_bucket_cap(0) != RD_BUCKET_MIN ||
        rd_ord_bucket_cap(-5) != RD_BUCKET_MIN || rd_ord_bucket_cap(0x7FFFFFF0L) != RD_BUCKET_MAX)
        return fail("bucket capacity");
    for (long n = 0; n < (1l << 31); n += 999983) {
        const uint32_t c = rd_ord_bucket_cap(n);
        if (c % 32 || c < RD_BUCKET_MIN || c > RD_BUCKET_MAX) return fail("bucket capacity range");
    }
    size_t want = 0;
    if (rd_check_block_count(0, 16384, 8192, 1, &want) != RD_OK || want != 16384 || rd_check_block_count(1, 8192, 8192, 1, &want) != RD_OK ||
        rd_check_block_count(1, 16384, 8192, 1, &want) != RD_ERR_ARG || want != 8192 || rd_check_block_count(0, 3 * 16384, 8192, 3, nullptr) != RD_OK)
        return fail("block count");
    printf("config ok: %d of %d random configurations accepted\n", ok, rounds);
    return 0;
}

// The Davis-shape predicates against the conditions their seven sites spelled out before they shared them: the one-launch
// tail (rd_launch_tail_fused, the batch handle's ft_ok), the one-launch streaming blocks (both launches, the streaming
// handle's one_ok) test S, P, K and the preamble; rd_launch_search does not test K; rd_launch_slice tests S and K only.
static int shape() {
    const rd_config prod = {19200, 14, 16, 80, 8192, {1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 0, 1, 0, 0, 1}};
    int n = 0, davis = 0;
    for (int sl : {14, 8, 1, 15})
        for (int ps : {16, 8, 15})
            for (int pk : {80, 64, 88})
                for (int flip : {-1, 0, 7, 15}) {
                    rd_config c = prod;
                    c.symbol_length = sl; c.preamble_symbols = ps; c.packet_symbols = pk;
                    if (flip >= 0) c.preamble[flip] ^= 1;
                    rd_devcfg d;
                    const char *why;
                    if (rd_make_devcfg(&c, &d, &why) != RD_OK) return fail("a shape the library takes was refused");
                    const bool whole = d.S == 14 && d.P == 16 && d.K == 80 && d.pre_mask == 0x91D3ull;
                    const bool search = d.S == 14 && d.P == 16 && d.pre_mask == 0x91D3ull;
                    const bool slice = d.S == 14 && d.K == 80;
                    if (rd_davis_shape(d) != whole || rd_davis_search(d) != search || rd_davis_slice(d) != slice)
                        return fail("a Davis-shape predicate differs from its site's condition");
                    n++;
                    davis += whole;
                }
    if (davis != 1) return fail("exactly one of the shapes is the Davis one");
    printf("shape ok: %d shapes\n", n);
    return 0;
}

static int waiter() {
    const double dflt = rd_wait_timeout_ms();
    if (dflt <= 0) return fail("default deadline");
    if (rd_wait_timeout_set(0) != dflt || rd_wait_timeout_ms() != 0) return fail("override");
    { rd_waiter w(rd_wait_timeout_ms()); if (w.relax()) return fail("deadline 0 must expire at the first poll"); }
    rd_wait_timeout_set(-1);
    if (rd_wait_timeout_ms() != dflt) return fail("restore");
    rd_waiter w(3.0);  // 3 ms: spins, yields, sleeps, then expires
    unsigned polls = 0;
    while (w.relax()) if (++polls > 100000000u) return fail("a 3 ms deadline never expired");
    if (w.waited_ms() < 3.0 || w.waited_ms() > 500.0) return fail("expired at the wrong time");
    printf("waiter ok: %u polls in %.2f ms\n", polls, w.waited_ms());
    return 0;
}

// BURST DECODE step 7: rd_burst_msg records from <msgs> against those of <delivered>; the indices (uint32) of the records
// rd_bd_repeats keeps go to <out>
static int repeats_mode(const char *msgs, const char *delivered, const char *out, int sl) {
    std::vector<rd_burst_msg> m, d;
    for (int k = 0; k < 2; k++) {
        FILE *f = fopen(k ? delivered : msgs, "rb");
        if (!f) return fail("cannot open the records");
        rd_burst_msg r;
        while (fread(&r, sizeof r, 1, f) == 1) (k ? d : m).push_back(r);
        fclose(f);
    }
    FILE *f = fopen(out, "wb");
    if (!f) return fail("cannot open the output");
    for (uint32_t i = 0; i < (uint32_t)m.size(); i++)
        if (!rd_bd_repeats(m[i], d.data(), d.size(), sl)) fwrite(&i, sizeof i, 1, f);
    fclose(f);
    printf("repeats ok\n");
    return 0;
}

// A file's bytes in a heap block of exactly its size (what a slot is to the fetch: one byte past it is a sanitizer report);
// false unless it holds `want` bytes
static bool exact_block(const char *path, size_t want, std::unique_ptr<uint8_t[]> *blk) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    blk->reset(new uint8_t[want]);
    uint8_t more;
    const bool ok = fread(blk->get(), 1, want, f) == want && fread(&more, 1, 1, f) == 0;
    fclose(f);
    return ok;
}

static bool write_all(const char *path, const void *p, size_t n) {
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = n == 0 || fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

// The streaming demodulator's fetch of one slot: n_lists counts, n_lists x per record places and (fe != "-") as many fe
// entries, each from its file into a heap block of exactly that size; the kept records and the messages go to the outputs.
// Run twice on one scratch, like a handle's second fetch: the outputs must not change.
static int block_mode(size_t n_lists, size_t per, int S, const char *counts, const char *recs, const char *fe, const char *last_out,
                      const char *parsed_out) {
    std::unique_ptr<uint8_t[]> c, r, e;
    const bool parse = strcmp(fe, "-") != 0;
    if (!exact_block(counts, n_lists * sizeof(uint32_t), &c) || !exact_block(recs, n_lists * per * sizeof(rd_packet), &r) ||
        (parse && !exact_block(fe, n_lists * per * sizeof(int32_t), &e)))
        return fail("a slot file of the wrong size");
    rd_block_scratch sc;
    std::vector<rd_packet> last, last2;
    std::vector<rd_parsed> parsed, parsed2;
    rd_collect_block((const uint32_t *)c.get(), n_lists, per, (const rd_packet *)r.get(), parse ? (const int32_t *)e.get() : nullptr, S, sc,
                     last2, parsed2);
    rd_collect_block((const uint32_t *)c.get(), n_lists, per, (const rd_packet *)r.get(), parse ? (const int32_t *)e.get() : nullptr, S, sc,
                     last, parsed);
    if (last.size() != last2.size() || parsed.size() != parsed2.size() ||
        (!last.empty() && memcmp(last.data(), last2.data(), last.size() * sizeof(rd_packet))) ||
        (!parsed.empty() && memcmp(parsed.data(), parsed2.data(), parsed.size() * sizeof(rd_parsed))))
        return fail("a second fetch of the same slot gave something else");
    if (!parse && !parsed.empty()) return fail("messages from a block submitted with parse off");
    if (!write_all(last_out, last.data(), last.size() * sizeof(rd_packet)) || !write_all(parsed_out, parsed.data(), parsed.size() * sizeof(rd_parsed)))
        return fail("cannot write the outputs");
    printf("block ok: %zu records, %zu messages\n", last.size(), parsed.size());
    return 0;
}

// rd_order_parsed's rule, spelled out naively: stable order by (stream, call, index % S, index), then the first occurrence
// of (nbytes, all of data) inside (stream, call) wins
static std::vector<rd_parsed> naive_parsed(std::vector<rd_parsed> r, int S) {
    std::stable_sort(r.begin(), r.end(), [S](const rd_parsed &x, const rd_parsed &y) {
        if (x.stream != y.stream) return x.stream < y.stream;
        if (x.call != y.call) return x.call < y.call;
        if (x.index % S != y.index % S) return x.index % S < y.index % S;
        return x.index < y.index;
    });
    std::vector<rd_parsed> kept;
    for (const rd_parsed &m : r) {
        bool dup = false;
        for (const rd_parsed &k : kept)
            if (k.stream == m.stream && k.call == m.call && k.nbytes == m.nbytes && !memcmp(k.data, m.data, sizeof m.data)) { dup = true; break; }
        if (!dup) kept.push_back(m);
    }
    return kept;
}

static int parsed_file_mode(const char *in, const char *out, int S) {
    FILE *f = fopen(in, "rb");
    if (!f) return fail("cannot open input");
    std::vector<rd_parsed> r;
    rd_parsed p;
    while (fread(&p, sizeof p, 1, f) == 1) r.push_back(p);
    fclose(f);
    std::vector<rd_parsed> exact(r);   // (capacity = size: the call may not touch a place past the last record)
    exact.shrink_to_fit();
    const size_t kept = rd_order_parsed(exact.data(), exact.size(), S);
    if (kept > exact.size()) return fail("kept more than there were");
    if (!write_all(out, exact.data(), kept * sizeof(rd_parsed))) return fail("cannot write the output");
    printf("parsed ok: %zu of %zu\n", kept, r.size());
    return 0;
}

// a few and a few thousand records; few distinct payloads, a function of the position like a real message's bytes, so
// that equal-bytes groups occur inside a (stream, call) and across them, and records with equal keys are equal
static int parsed_soak(int rounds, unsigned seed) {
    std::mt19937 g(seed);
    for (int round = 0; round < rounds; round++) {
        const int S = 1 + (int)(g() % 20);
        const size_t n = (round % 3 == 0) ? g() % 12 : (round % 3 == 1) ? 100 + g() % 300 : 2000 + g() % 3000;
        const int n_streams = 1 + (int)(g() % 6), n_calls = 1 + (int)(g() % 8), n_index = 1 + (int)(g() % 9000), n_payloads = 1 + (int)(g() % 5);
        std::vector<rd_parsed> r(n);
        for (auto &m : r) {
            memset(&m, 0, sizeof m);
            m.stream = (int)(g() % n_streams);
            m.call = (int)(g() % n_calls);
            m.index = (int)(g() % n_index);
            const unsigned pay = (unsigned)(m.index % n_payloads);
            m.nbytes = 8 - (int)(pay & 1u);             // (equal leading bytes with another length are another message)
            for (int k = 0; k < m.nbytes; k++) m.data[k] = (uint8_t)((pay >> 1) * 37 + k);
            m.id = m.data[0] & 7;
            m.freq_err = m.index - 4000;
        }
        const std::vector<rd_parsed> want = naive_parsed(r, S);
        r.shrink_to_fit();
        const size_t kept = rd_order_parsed(r.data(), r.size(), S);
        if (kept != want.size()) return fail("kept count differs from the naive model");
        if (kept && memcmp(r.data(), want.data(), kept * sizeof(rd_parsed))) return fail("kept messages differ from the naive model");
    }
    if (rd_order_parsed(nullptr, 0, 14) != 0) return fail("empty input kept something");
    printf("parsed soak ok: %d rounds\n", rounds);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 10 && !strcmp(argv[1], "block"))
        return block_mode((size_t)atol(argv[2]), (size_t)atol(argv[3]), atoi(argv[4]), argv[5], argv[6], argv[7], argv[8], argv[9]);
    if (argc >= 5 && !strcmp(argv[1], "parsed")) return parsed_file_mode(argv[2], argv[3], atoi(argv[4]));
    if (argc >= 4 && !strcmp(argv[1], "parsed-soak")) return parsed_soak(atoi(argv[2]), (unsigned)atoi(argv[3]));
    if (argc >= 6 && !strcmp(argv[1], "repeats")) return repeats_mode(argv[2], argv[3], argv[4], atoi(argv[5]));
    if (argc >= 4 && !strcmp(argv[1], "soak")) return soak(atoi(argv[2]), (unsigned)atoi(argv[3]));
    if (argc >= 5 && !strcmp(argv[1], "file")) return file_mode(argv[2], argv[3], atoi(argv[4]));
    if (argc >= 4 && !strcmp(argv[1], "config")) return config(atoi(argv[2]), (unsigned)atoi(argv[3]));
    if (argc >= 2 && !strcmp(argv[1], "waiter")) return waiter();
    if (argc >= 2 && !strcmp(argv[1], "shape")) return shape();
    return fail("usage: soak <rounds> <seed> | file <in> <out> <S> | config <rounds> <seed> | waiter | shape | repeats .. | block .. | parsed .. | parsed-soak ..");
}
