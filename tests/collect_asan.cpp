// collect_asan.cpp - the receiver's fetch (rtldavis_amd/csrc/rd_host.cpp: rd_collect_*, rd_delivered, rd_msg_repeats) under
// -fsanitize=address,undefined, driven by tests/test_collect_sanitizers.py.  A stand-alone program:
//   collect_asan run IN OUT          the operations of file IN in order, on one set of delivered histories; results to OUT
//   collect_asan rule                the one repeat rule against the three loops it replaced, over random records
// An operation is 10 int64 - kind, n_ch, a (windows | bins | quota), chunk, sl, n, slot bytes, quality slot bytes, candidate
// counts, 0; -1 bytes: no slot - and then the slot, the quality slot and the counts.  Every slot goes into a heap block of
// exactly its size: a read past its end is the sanitizer's to find.  A result is rc, the history's chunk, the message's
// length, the number of arrays; the message; per array its bytes and then the array.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../rtldavis_amd/csrc/rd_host.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

enum { K_LEVELS, K_SPECTRUM, K_BURSTS, K_DECODE, K_EXPECT, K_SEARCH, K_CLIPS, K_FORGET };

static uint8_t *exact_block(FILE *f, int64_t len) {
    if (len < 0) return nullptr;
    uint8_t *p = (uint8_t *)malloc((size_t)len ? (size_t)len : 1);
    CHECK(p && fread(p, 1, (size_t)len, f) == (size_t)len);
    return p;
}

struct result {
    std::vector<std::pair<const void *, size_t>> arrays;
    template <class T> void add(const std::vector<T> &v) { arrays.push_back({v.data(), v.size() * sizeof(T)}); }
    void add(const void *p, size_t n) { arrays.push_back({p, n}); }
};

static int run(const char *in_path, const char *out_path) {
    FILE *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
    CHECK(in && out);
    rd_delivered bm, xm, sm;
    int64_t op[10];
    long n_ops = 0;
    while (fread(op, sizeof op, 1, in) == 1) {
        const int kind = (int)op[0], n_ch = (int)op[1], sl = (int)op[4], n = (int)op[5];
        const size_t a = (size_t)op[2];
        const long chunk = (long)op[3];
        uint8_t *slot = exact_block(in, op[6]), *qslot = exact_block(in, op[7]);
        uint32_t *cand = (uint32_t *)exact_block(in, op[8] < 0 ? -1 : op[8] * 4);
        rd_errtext err;
        err.text[0] = 0;
        result r;
        int rc = RD_OK;
        int64_t hist = 0;
        std::vector<rd_chan_level> lv;
        rd_input_level lin;
        rd_spectrum_info info;
        std::vector<double> power;
        std::vector<rd_burst> runs;
        std::vector<rd_burst_floor> floor;
        std::vector<uint32_t> counts, dropped;
        std::vector<rd_burst_quality> qual;
        std::vector<rd_bs_header> hdr;
        std::vector<rd_burst_clip> clips;
        std::vector<uint8_t> bytes;
        switch (kind) {
        case K_LEVELS:
            rc = rd_collect_levels(slot, n_ch, chunk, lv, &lin, &err);
            r.add(lv), r.add(&lin, sizeof lin);
            break;
        case K_SPECTRUM:
            rc = rd_collect_spectrum(slot, (int)a, chunk, &info, power, &err);
            r.add(&info, sizeof info), r.add(power);
            break;
        case K_BURSTS:
            rc = rd_collect_bursts(slot, n_ch, a, chunk, runs, floor, &err);
            r.add(runs), r.add(floor);
            break;
        case K_DECODE:
            rc = rd_collect_decode(slot, qslot, n_ch, a, chunk, sl, bm, counts, qual, &err);
            r.add(bm.last), r.add(counts), r.add(qual);
            hist = bm.chunk;
            break;
        case K_EXPECT:
            counts.assign(RD_BX_MAX, 0u);
            rc = rd_collect_expect(slot, qslot, n_ch, a, chunk, sl, n, cand, xm, counts.data(), qual, &err);
            r.add(xm.last), r.add(counts), r.add(qual);
            hist = xm.chunk;
            break;
        case K_SEARCH:
            rc = rd_collect_search(slot, n_ch, chunk, sl, n, sm, hdr, &err);
            r.add(sm.last), r.add(hdr);
            hist = sm.chunk;
            break;
        case K_CLIPS:
            rc = rd_collect_clips(slot, n_ch, (int)a, chunk, clips, bytes, dropped, &err);
            r.add(clips), r.add(bytes), r.add(dropped);
            break;
        case K_FORGET:
            bm.forget(), xm.forget(), sm.forget();
            CHECK(bm.chunk == -2 && xm.chunk == -2 && sm.chunk == -2 && bm.prev.empty() && xm.prev.empty() && sm.prev.empty());
            hist = -2;
            break;
        default:
            CHECK(!"kind");
        }
        CHECK(rc == RD_OK || rc == RD_ERR_DEVICE);
        CHECK((rc == RD_OK) == (err.text[0] == 0));
        if (rc != RD_OK) r.arrays.clear();               // (undefined after a failure)
        const int64_t head[4] = {rc, hist, (int64_t)strlen(err.text), (int64_t)r.arrays.size()};
        CHECK(fwrite(head, sizeof head, 1, out) == 1);
        CHECK(fwrite(err.text, 1, (size_t)head[2], out) == (size_t)head[2]);
        for (const auto &arr : r.arrays) {
            const int64_t nb = (int64_t)arr.second;
            CHECK(fwrite(&nb, sizeof nb, 1, out) == 1);
            CHECK(!nb || fwrite(arr.first, 1, (size_t)nb, out) == (size_t)nb);
        }
        free(slot), free(qslot), free(cand);
        n_ops++;
    }
    CHECK(!fclose(out) && !fclose(in));
    printf("run ok: %ld operations\n", n_ops);
    return 0;
}

// the three loops as they stood before rd_msg_repeats replaced them
static bool old_bd_repeats(const rd_burst_msg &m, const rd_burst_msg *delivered, size_t n_delivered, int sl) {
    if (!(m.flags & 1u) || sl <= 0) return false;
    for (size_t i = 0; i < n_delivered; i++) {
        const rd_burst_msg &q = delivered[i];
        const uint64_t d = m.time - q.time, ad = d < 0ull - d ? d : 0ull - d;   // (the clock wraps at 2^64)
        if (q.channel == m.channel && !memcmp(q.data, m.data, sizeof m.data) && ad < (uint64_t)sl) return true;
    }
    return false;
}
static bool old_bx_repeats(const rd_burst_msg &m, const rd_burst_msg *delivered, size_t n_delivered, int sl) {
    if (sl <= 0) return false;
    for (size_t i = 0; i < n_delivered; i++) {
        const rd_burst_msg &q = delivered[i];
        const uint64_t d = m.time - q.time, ad = d < 0ull - d ? d : 0ull - d;   // (the clock wraps at 2^64)
        if (q.channel == m.channel && !memcmp(q.data, m.data, sizeof m.data) && ad < (uint64_t)sl) return true;
    }
    return false;
}
static bool old_bs_repeats(const rd_burst_msg &m, const rd_burst_msg *delivered, size_t n_delivered, int sl) {
    if (sl <= 0) return false;
    for (size_t i = 0; i < n_delivered; i++) {
        const rd_burst_msg &q = delivered[i];
        const uint64_t d = m.time - q.time, ad = d < 0ull - d ? d : 0ull - d;   // (the clock wraps at 2^64)
        if (q.channel == m.channel && q.pad[3] == m.pad[3] && !memcmp(q.data, m.data, sizeof m.data) && ad < (uint64_t)sl) return true;
    }
    return false;
}

// Few channels, payloads, centres and times near 0 / 2^64 and near each other, so that every clause of the rule decides
// about as often as it does not.
static int rule(void) {
    std::mt19937_64 g(20240607);
    const uint64_t bases[] = {0, 40, UINT64_MAX - 30, (uint64_t)1 << 40};
    auto draw = [&]() {
        rd_burst_msg m;
        memset(&m, 0, sizeof m);
        m.channel = (int32_t)(g() % 3);
        m.flags = (uint32_t)(g() % 64);
        m.time = bases[g() % 4] + g() % 60 - 30;
        memset(m.data, (int)(g() % 2), sizeof m.data);
        m.data[g() % sizeof m.data] ^= (uint8_t)(g() % 8 == 0);
        m.pad[3] = (uint8_t)(g() % 2);
        return m;
    };
    long yes[3] = {0, 0, 0}, cases = 0;
    for (int it = 0; it < 6000; it++) {
        std::vector<rd_burst_msg> d(g() % 5);            // (a heap block of exactly its size; empty lists included)
        for (auto &q : d) q = draw();
        const rd_burst_msg m = draw();
        const int sl = (int)(g() % 8 == 0 ? g() % 3 - 1 : 1 + g() % 51);
        const bool a = old_bd_repeats(m, d.data(), d.size(), sl), b = old_bx_repeats(m, d.data(), d.size(), sl),
                   c = old_bs_repeats(m, d.data(), d.size(), sl);
        CHECK(rd_msg_repeats(m, d.data(), d.size(), sl, true, false) == a && rd_bd_repeats(m, d.data(), d.size(), sl) == a);
        CHECK(rd_msg_repeats(m, d.data(), d.size(), sl, false, false) == b && rd_bx_repeats(m, d.data(), d.size(), sl) == b);
        CHECK(rd_msg_repeats(m, d.data(), d.size(), sl, false, true) == c && rd_bs_repeats(m, d.data(), d.size(), sl) == c);
        yes[0] += a, yes[1] += b, yes[2] += c, cases++;
    }
    printf("rule ok: %ld cases, repeats %ld %ld %ld\n", cases, yes[0], yes[1], yes[2]);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "rule")) return rule();
    fprintf(stderr, "usage: collect_asan run IN OUT | rule\n");
    return 2;
}
