// clip_asan.cpp - the pure-host part of BURST CLIPS (rtldavis_amd/csrc/rd_host.h / rd_host.cpp: rd_bc_window_of,
// rd_bc_window) under -fsanitize=address,undefined, driven by tests/test_clip_sanitizers.py.  A stand-alone program:
//   clip_asan naive <seed> <n>    the clamp against a naive enumeration of every output, over random (block_size,
//                                 have_prev, a, e), a and e anywhere on 64 bits included
//   clip_asan file <in> <out>     cases from a file (4 x int64 each: block_size, have_prev, a, e)
//                                 -> 4 x int32 each (clip, t0, n, flags)
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

static int64_t floor8(int64_t t) { return t >= 0 ? t / 8 * 8 : -((-t + 7) / 8 * 8); }

static int test_naive(uint64_t seed, int n_cases) {
    rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
    int clips = 0, cut_start = 0, cut_end = 0, from_prev = 0, none = 0, far = 0;
    for (int it = 0; it < n_cases; it++) {
        const int bs = 8 * (1 + (int)(rnd() % 64)) * (rnd() & 1 ? 16 : 1);        // 8 .. 8192, multiples of 8 and of 128
        const int have_prev = (int)(rnd() & 1);
        int64_t a = (int64_t)(rnd() % (uint64_t)(4 * bs + 400)) - 2 * bs - 200;
        int64_t e = a + (int64_t)(rnd() % (uint64_t)(3 * bs + 8)) - 4;
        const unsigned kind = (unsigned)(rnd() % 16);
        if (kind == 0) a = INT64_MIN;
        if (kind == 1) e = INT64_MAX;
        if (kind == 2) { a = (int64_t)rnd(); e = (int64_t)rnd(); }               // anywhere on 64 bits
        if (kind == 3) { a = INT64_MIN; e = INT64_MAX; }
        if (kind == 4) { a = INT64_MAX; e = INT64_MIN; }
        if (kind <= 4) far++;
        rd_bc_clamped w;
        const bool ok = rd_bc_window_of(bs, have_prev, a, e, &w);
        int32_t c[3];
        CHECK(rd_bc_window(bs, have_prev, a, e, c) == (ok ? 1 : 0));
        CHECK(c[0] == w.t0 && c[1] == w.n && c[2] == w.flags);
        // the definition, output by output: the outputs of [a, e) that the two chunks hold, then the groups of 8 they touch
        const int64_t lo_lim = have_prev ? -(int64_t)bs : 0;
        int64_t first = 0, last = 0, count = 0;
        for (int64_t t = lo_lim; t < bs; t++)
            if (t >= a && t < e) {
                if (!count) first = t;
                last = t;
                count++;
            }
        CHECK(ok == (count > 0));
        if (!ok) {
            CHECK(!w.t0 && !w.n && !w.flags);
            none++;
            continue;
        }
        clips++;
        CHECK(count == last - first + 1);
        CHECK(w.t0 == floor8(first) && w.t0 + w.n == floor8(last) + 8);
        CHECK(w.t0 % 8 == 0 && w.n % 8 == 0 && w.n >= 8 && w.t0 >= lo_lim && w.t0 + w.n <= bs);
        CHECK(((w.flags & RD_BC_CUT_START) != 0) == (a < lo_lim));
        CHECK(((w.flags & RD_BC_CUT_END) != 0) == (e > bs));
        CHECK(((w.flags & RD_BC_FROM_PREV) != 0) == (w.t0 < 0) && !(w.flags & ~7));
        cut_start += (w.flags & RD_BC_CUT_START) ? 1 : 0;
        cut_end += (w.flags & RD_BC_CUT_END) ? 1 : 0;
        from_prev += (w.flags & RD_BC_FROM_PREV) ? 1 : 0;
    }
    printf("naive ok: %d clips, %d cut_start, %d cut_end, %d from_prev, %d none, %d far of %d\n", clips, cut_start, cut_end, from_prev,
           none, far, n_cases);
    return 0;
}

static int run_file(const char *in, const char *out) {
    FILE *f = fopen(in, "rb");
    CHECK(f);
    std::vector<int64_t> cases;
    int64_t rec[4];
    while (fread(rec, sizeof rec, 1, f) == 1) cases.insert(cases.end(), rec, rec + 4);
    fclose(f);
    std::vector<int32_t> res;
    for (size_t i = 0; i < cases.size(); i += 4) {
        int32_t c[3];
        const int ok = rd_bc_window((int)cases[i], (int)cases[i + 1], cases[i + 2], cases[i + 3], c);
        res.push_back(ok);
        res.insert(res.end(), c, c + 3);
    }
    f = fopen(out, "wb");
    CHECK(f);
    CHECK(res.empty() || fwrite(res.data(), sizeof(int32_t), res.size(), f) == res.size());
    fclose(f);
    printf("file ok: %zu cases\n", cases.size() / 4);
    return 0;
}

int main(int argc, char **argv) {
    CHECK(rd_bc_window(1152, 1, 0, 100, nullptr) == 0);          // no room for the answer: refused, nothing written
    int32_t c[3] = {1, 1, 1};
    CHECK(rd_bc_window(0, 1, 0, 100, c) == 0 && rd_bc_window(-8, 1, 0, 100, c) == 0 && rd_bc_window(12, 1, 0, 100, c) == 0 && !c[0] && !c[1] && !c[2]);
    if (argc == 4 && !strcmp(argv[1], "naive")) return test_naive(strtoull(argv[2], nullptr, 10), atoi(argv[3]));
    if (argc == 4 && !strcmp(argv[1], "file")) return run_file(argv[2], argv[3]);
    fprintf(stderr, "usage: clip_asan naive <seed> <n> | file <in> <out>\n");
    return 2;
}
