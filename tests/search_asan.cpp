// search_asan.cpp - the pure-host parts of BURST SEARCH (rtldavis_amd/csrc/rd_host.cpp: rd_bs_check_centres, rd_bs_range,
// rd_bs_repeats) under -fsanitize=address,undefined, driven by tests/test_search_sanitizers.py.  A stand-alone program:
//   search_asan centres              every rule of the list, the limits on either side
//   search_asan range                rd_bs_range against a naive enumeration of every tau, over a grid of shapes
//   search_asan repeats              step 7s, the 64-bit clock near its wrap included
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../rtldavis_amd/csrc/rd_host.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static int test_centres(void) {
    int bad = 7;
    const char *why = nullptr;
    // (each list in a heap block of exactly its size: a read past its end is the sanitizer's to find)
    auto list = [](std::initializer_list<int> v) { return std::vector<uint8_t>(v.begin(), v.end()); };
    std::vector<uint8_t> l = list({0, 63, 7, 8, 9, 10, 11, 12});
    CHECK(rd_bs_check_centres(nullptr, 0, &bad, &why) == RD_OK && bad == -1);
    CHECK(rd_bs_check_centres(nullptr, 0, nullptr, nullptr) == RD_OK);
    CHECK(rd_bs_check_centres(l.data(), RD_BS_MAX_CENTRES, &bad, &why) == RD_OK && bad == -1);
    for (int n = 1; n <= RD_BS_MAX_CENTRES; n++) {
        std::vector<uint8_t> part(l.begin(), l.begin() + n);
        CHECK(rd_bs_check_centres(part.data(), n, &bad, &why) == RD_OK && bad == -1);
    }
    std::vector<uint8_t> nine = list({0, 1, 2, 3, 4, 5, 6, 7, 8});
    CHECK(rd_bs_check_centres(nine.data(), RD_BS_MAX_CENTRES + 1, &bad, &why) == RD_ERR_ARG && bad == -1 && why && *why);
    CHECK(rd_bs_check_centres(l.data(), -1, &bad, &why) == RD_ERR_ARG && bad == -1);
    CHECK(rd_bs_check_centres(nullptr, 1, &bad, &why) == RD_ERR_ARG && bad == -1);
    for (int at = 0; at < RD_BS_MAX_CENTRES; at++) {
        std::vector<uint8_t> u = l;
        u[(size_t)at] = 64;
        CHECK(rd_bs_check_centres(u.data(), RD_BS_MAX_CENTRES, &bad, &why) == RD_ERR_ARG && bad == at && why && *why);
        u[(size_t)at] = 255;
        CHECK(rd_bs_check_centres(u.data(), RD_BS_MAX_CENTRES, &bad, nullptr) == RD_ERR_ARG && bad == at);
        if (at) {
            u = l;
            u[(size_t)at] = u[0];                        // a duplicate is reported at its second occurrence
            CHECK(rd_bs_check_centres(u.data(), RD_BS_MAX_CENTRES, &bad, &why) == RD_ERR_ARG && bad == at);
            CHECK(rd_bs_check_centres(u.data(), at, &bad, &why) == RD_OK && bad == -1);
        }
    }
    printf("centres ok\n");
    return 0;
}

static int test_range(void) {
    long with = 0, without = 0;
    const int sls[] = {1, 4, 8, 14, 25, 51}, ns[] = {40, 64, 80};
    for (int sl : sls)
        for (int n : ns) {
            const int need = n * sl + 1, look = 128 * ((need + 127) / 128);
            for (int bs : {128, 256, 1024, 1152, 2048, 4096, 8192})
                for (int have_prev = 0; have_prev < 2; have_prev++) {
                    const int lo = have_prev ? -look : 0, body = sl * (n - 1);
                    long first = 1, last = 0;            // naive: every tau whose sums lie in lo .. bs - 1 and whose packet ends in 0 .. bs - 1
                    for (long tau = -3 * 8192; tau <= 3 * 8192; tau++) {
                        if (tau - sl < lo || tau + body > bs - 1 || tau + body < 0) continue;
                        if (first > last) first = tau;
                        last = tau;
                    }
                    int32_t a = 77, b = 77;
                    const bool got = rd_bs_range(sl, n, bs, look, have_prev, &a, &b);
                    CHECK(got == (first <= last));
                    if (got) {
                        CHECK(a == first && b == last);
                        with++;
                    } else {
                        CHECK(a == 77 && b == 77);
                        without++;
                    }
                }
        }
    int32_t a, b;
    CHECK(!rd_bs_range(0, 80, 2048, 1152, 1, &a, &b) && !rd_bs_range(14, 0, 2048, 1152, 1, &a, &b));
    CHECK(!rd_bs_range(14, 80, 0, 1152, 1, &a, &b) && !rd_bs_range(14, 80, 2048, -1, 1, &a, &b));
    CHECK(!rd_bs_range(14, 80, 2048, 1152, 1, nullptr, &b) && !rd_bs_range(14, 80, 2048, 1152, 1, &a, nullptr));
    CHECK(rd_bs_range(51, 80, INT32_MAX, INT32_MAX, 1, &a, &b) && a == -51 * 79 && b == INT32_MAX - 1 - 51 * 79);
    printf("range ok: %ld with candidates, %ld without\n", with, without);
    return 0;
}

static rd_burst_msg msg(int channel, uint64_t time, uint8_t g, uint8_t byte) {
    rd_burst_msg m;
    memset(&m, 0, sizeof m);
    m.channel = channel;
    m.time = time;
    m.flags = RD_BURST_MSG_SEARCHED | RD_BURST_MSG_NARROW;
    m.pad[3] = g;
    memset(m.data, byte, sizeof m.data);
    return m;
}

static int test_repeats(void) {
    const int sl = 14;
    std::vector<rd_burst_msg> d = {msg(3, 5000, 7, 0xAB), msg(4, 0, 9, 0xCD), msg(5, UINT64_MAX - 2, 9, 0xEF)};
    CHECK(!rd_bs_repeats(msg(3, 5000, 7, 0xAB), nullptr, 0, sl));
    CHECK(!rd_bs_repeats(msg(3, 5000, 7, 0xAB), d.data(), d.size(), 0));
    for (int off = -sl - 1; off <= sl + 1; off++) {
        const bool near = off > -sl && off < sl;
        CHECK(rd_bs_repeats(msg(3, 5000 + (uint64_t)(int64_t)off, 7, 0xAB), d.data(), d.size(), sl) == near);
        CHECK(rd_bs_repeats(msg(4, 0 + (uint64_t)(int64_t)off, 9, 0xCD), d.data(), d.size(), sl) == near);             // across 0
        CHECK(rd_bs_repeats(msg(5, UINT64_MAX - 2 + (uint64_t)(int64_t)off, 9, 0xEF), d.data(), d.size(), sl) == near);   // across 2^64
    }
    CHECK(!rd_bs_repeats(msg(2, 5000, 7, 0xAB), d.data(), d.size(), sl));   // another channel
    CHECK(!rd_bs_repeats(msg(3, 5000, 8, 0xAB), d.data(), d.size(), sl));   // another centre: each centre gives its record
    CHECK(!rd_bs_repeats(msg(3, 5000, 7, 0xAC), d.data(), d.size(), sl));   // another payload
    rd_burst_msg front = msg(3, 5000, 7, 0xAB);
    front.flags &= ~1u;                                  // (no flag is asked for, unlike step 7)
    CHECK(rd_bs_repeats(front, d.data(), d.size(), sl));
    printf("repeats ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "centres")) return test_centres();
    if (argc == 2 && !strcmp(argv[1], "range")) return test_range();
    if (argc == 2 && !strcmp(argv[1], "repeats")) return test_repeats();
    fprintf(stderr, "usage: search_asan centres | range | repeats\n");
    return 2;
}
