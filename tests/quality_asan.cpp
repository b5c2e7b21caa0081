// quality_asan.cpp - the pure-host part of BURST QUALITY (rtldavis_amd/csrc/rd_host.h / rd_host.cpp: rd_bq_windows_of,
// rd_bq_window) under -fsanitize=address,undefined, driven by tests/test_quality_sanitizers.py.  A stand-alone program:
//   quality_asan naive <seed> <n>    the windows against a naive enumeration of every output, over random
//                                    (SL, N, block_size, have_prev, tau, gap), tau far out of range included
//   quality_asan file <in> <out>     cases from a file (6 x int64 each: sl, n_sym, block_size, have_prev, tau, gap)
//                                    -> 6 x int32 each (measurable, p0, p1, s1, n0, n1)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../rtldavis_amd/csrc/rd_host.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static uint64_t rng_state = 1;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static int test_naive(uint64_t seed, int n_cases) {
    rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
    int measurable = 0, cut = 0, empty = 0, far = 0;
    for (int it = 0; it < n_cases; it++) {
        const int n_sym = 40 + 8 * (int)(rnd() % 6);
        int sl = 1 + (int)(rnd() % 51);
        while (n_sym * sl + 1 > 2048) sl--;
        const int look = 128 * ((n_sym * sl + 1 + 127) / 128);
        const int bs = look * (1 + (int)(rnd() % 3));
        const int have_prev = (int)(rnd() & 1), gap = (int)(rnd() % (RD_BQ_MAX_GAP + 1));
        int64_t tau = (int64_t)(rnd() % (uint64_t)(2 * bs + 200)) - bs - 100;
        const unsigned kind = (unsigned)(rnd() % 16);
        if (kind == 0) tau = INT32_MIN;
        if (kind == 1) tau = INT32_MAX;
        if (kind == 2) tau = (int64_t)rnd();                     // anywhere on 64 bits
        if (kind <= 2) far++;
        rd_bq_windows w;
        const bool ok = rd_bq_windows_of(sl, n_sym, bs, have_prev, tau, gap, &w);
        int32_t c[5];
        CHECK(rd_bq_window(sl, n_sym, bs, have_prev, tau, gap, c) == (ok ? 1 : 0));
        CHECK(c[0] == w.p0 && c[1] == w.p1 && c[2] == w.s1 && c[3] == w.n0 && c[4] == w.n1);
        // the definition, output by output (only where the packet can lie in the two chunks at all)
        const int64_t lo_lim = have_prev ? -(int64_t)bs : 0;
        bool want = tau > -(int64_t)4 * bs && tau < (int64_t)4 * bs;
        const int64_t p0 = tau - sl + 1;
        if (want)
            for (int64_t t = p0; t < p0 + (int64_t)n_sym * sl; t++)
                if (t < lo_lim || t >= bs) { want = false; break; }
        CHECK(ok == want);
        if (!ok) {
            CHECK(!w.p0 && !w.p1 && !w.s1 && !w.n0 && !w.n1);
            continue;
        }
        measurable++;
        CHECK(w.p0 == p0 && w.p1 - w.p0 == n_sym * sl && w.s1 - w.p0 == 16 * sl);
        int64_t first = 0, count = 0;
        for (int64_t t = p0 - gap - 16 * (int64_t)sl; t < p0 - gap; t++)
            if (t >= lo_lim) {
                if (!count) first = t;
                count++;
            }
        CHECK(w.n1 - w.n0 == count);
        if (count) CHECK(w.n0 == first && w.n1 == p0 - gap);
        else CHECK(w.n0 == p0 && w.n1 == p0);
        if (count == 0) empty++;
        else if (count < 16 * sl) cut++;
    }
    printf("naive ok: %d measurable, %d cut, %d empty, %d far of %d\n", measurable, cut, empty, far, n_cases);
    return 0;
}

static int run_file(const char *in, const char *out) {
    FILE *f = fopen(in, "rb");
    CHECK(f);
    std::vector<int64_t> cases;
    int64_t rec[6];
    while (fread(rec, sizeof rec, 1, f) == 1) cases.insert(cases.end(), rec, rec + 6);
    fclose(f);
    std::vector<int32_t> res;
    for (size_t i = 0; i < cases.size(); i += 6) {
        int32_t c[5];
        const int ok = rd_bq_window((int)cases[i], (int)cases[i + 1], (int)cases[i + 2], (int)cases[i + 3], cases[i + 4], (int)cases[i + 5], c);
        res.push_back(ok);
        res.insert(res.end(), c, c + 5);
    }
    f = fopen(out, "wb");
    CHECK(f);
    CHECK(res.empty() || fwrite(res.data(), sizeof(int32_t), res.size(), f) == res.size());
    fclose(f);
    printf("file ok: %zu cases\n", cases.size() / 6);
    return 0;
}

int main(int argc, char **argv) {
    CHECK(rd_bq_window(14, 80, 1152, 1, 13, 0, nullptr) == 0);   // no room for the answer: refused, nothing written
    if (argc == 4 && !strcmp(argv[1], "naive")) return test_naive(strtoull(argv[2], nullptr, 10), atoi(argv[3]));
    if (argc == 4 && !strcmp(argv[1], "file")) return run_file(argv[2], argv[3]);
    fprintf(stderr, "usage: quality_asan naive <seed> <n> | file <in> <out>\n");
    return 2;
}
