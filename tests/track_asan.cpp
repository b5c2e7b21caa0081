// track_asan.cpp - the pure-host parts of BURST EXPECT (rtldavis_amd/csrc/rd_host.cpp: rd_bx_check_table, rd_bx_range,
// rd_bx_repeats) under -fsanitize=address,undefined, driven by tests/test_track_sanitizers.py.  A stand-alone program:
//   track_asan table                 every rule of the table, the limits on either side; step 7'; the decoders' candidate test
//   track_asan range <seed> <n>      rd_bx_range against a naive enumeration of every tau, clocks near 0 and near 2^64
//   track_asan file <in> <out>       cases from a file (7 x int64 each: sl, n_sym, block_size, have_prev, clock, t_lo, t_hi
//                                    as bit patterns) -> 3 x int32 each (found, tau_a, tau_b)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../rtldavis_amd/csrc/rd_burst_candidate.h"
#include "../rtldavis_amd/csrc/rd_host.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static uint64_t rng_state = 1;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static rd_expect good(void) {
    rd_expect e;
    memset(&e, 0, sizeof e);
    e.channel = 1;
    e.id = 3;
    e.t_lo = 1000;
    e.t_hi = 1200;
    e.corr_re = 16384;
    e.corr_im = -1;
    return e;
}

static int test_table(void) {
    int bad = 7;
    const char *why = nullptr;
    std::vector<rd_expect> t((size_t)RD_BX_MAX + 1, good());
    CHECK(rd_bx_check_table(t.data(), 0, 3, &bad, &why) == RD_OK && bad == -1);
    CHECK(rd_bx_check_table(nullptr, 0, 3, nullptr, nullptr) == RD_OK);
    CHECK(rd_bx_check_table(t.data(), RD_BX_MAX, 3, &bad, &why) == RD_OK && bad == -1);
    CHECK(rd_bx_check_table(t.data(), RD_BX_MAX + 1, 3, &bad, &why) == RD_ERR_ARG && bad == -1 && why && *why);
    CHECK(rd_bx_check_table(t.data(), -1, 3, &bad, &why) == RD_ERR_ARG && bad == -1);
    CHECK(rd_bx_check_table(nullptr, 1, 3, &bad, &why) == RD_ERR_ARG && bad == -1);
    struct edit { int field; int64_t value; bool ok; };
    const edit edits[] = {{0, 0, true}, {0, 2, true}, {0, 3, false}, {0, -1, false}, {1, 0, true}, {1, 7, true}, {1, 8, false},
                          {1, 0xFF, true}, {1, 0xFE, false}, {1, 0x1FF, false}, {2, 999, false}, {2, 1000, true},
                          {2, 1000 + RD_BX_MAX_SPAN, true}, {2, 1001 + RD_BX_MAX_SPAN, false}, {3, 32767, true}, {3, 32768, false},
                          {3, -32768, true}, {3, -32769, false}, {4, 32767, true}, {4, 32768, false}, {4, -32768, true},
                          {4, -32769, false}};
    for (const edit &ed : edits)
        for (int at : {0, 5, RD_BX_MAX - 1}) {
            std::vector<rd_expect> u(t.begin(), t.begin() + RD_BX_MAX);
            rd_expect &e = u[(size_t)at];
            if (ed.field == 0) e.channel = (int32_t)ed.value;
            if (ed.field == 1) e.id = (uint32_t)ed.value;
            if (ed.field == 2) e.t_hi = (uint64_t)ed.value;
            if (ed.field == 3) e.corr_re = (int32_t)ed.value;
            if (ed.field == 4) e.corr_im = (int32_t)ed.value;
            const int rc = rd_bx_check_table(u.data(), RD_BX_MAX, 3, &bad, &why);
            CHECK(ed.ok ? (rc == RD_OK && bad == -1) : (rc == RD_ERR_ARG && bad == at && why && *why));
        }
    rd_expect z = good();
    z.corr_re = z.corr_im = 0;
    CHECK(rd_bx_check_table(&z, 1, 3, &bad, &why) == RD_ERR_ARG && bad == 0);
    z.corr_im = 1;
    CHECK(rd_bx_check_table(&z, 1, 3, &bad, &why) == RD_OK);
    z.t_lo = UINT64_MAX - 10;                                  // a window at the very end of the clock
    z.t_hi = UINT64_MAX;
    CHECK(rd_bx_check_table(&z, 1, 3, &bad, &why) == RD_OK);
    z.t_lo = UINT64_MAX;                                       // t_hi has wrapped: t_lo > t_hi
    z.t_hi = 5;
    CHECK(rd_bx_check_table(&z, 1, 3, &bad, &why) == RD_ERR_ARG && bad == 0);
    printf("table ok\n");
    return 0;
}

// every tau of the definition, one by one, with the clock's arithmetic modulo 2^64
static bool naive(int sl, int n_sym, int bs, int have_prev, uint64_t clock, uint64_t t_lo, uint64_t t_hi, int32_t *a, int32_t *b) {
    const int body = sl * (n_sym - 1);
    bool any = false;
    for (int tau = -body; tau + body < bs; tau++) {
        if (!have_prev && tau - sl < 0) continue;
        const uint64_t t = clock + (uint64_t)(int64_t)tau;
        if (t - t_lo > t_hi - t_lo) continue;                  // t_lo <= t <= t_hi on the circle; the span is at most 2048
        if (!any) *a = tau;
        *b = tau;
        any = true;
    }
    return any;
}

static int test_range(uint64_t seed, int n) {
    rng_state = seed * 2654435761ull + 1;
    const int shapes[][3] = {{14, 80, 2048}, {8, 40, 1152}, {51, 40, 2176}, {1, 40, 128}, {25, 80, 4096}};
    const uint64_t clocks[] = {0, 128, 2048, 1ull << 32, (1ull << 63) - 128, 1ull << 63, 0ull - 4096, 0ull - 2048, 0ull - 128};
    long found = 0, wrapped = 0;
    for (int i = 0; i < n; i++) {
        const int *sh = shapes[rnd() % 5];
        const uint64_t clock = clocks[rnd() % 9];
        const int have_prev = (int)(rnd() & 1);
        const uint64_t span = rnd() % 3 == 0 ? RD_BX_MAX_SPAN : rnd() % (RD_BX_MAX_SPAN + 1);
        uint64_t t_lo = clock + (uint64_t)((int64_t)(rnd() % 12000) - 5000);   // around the chunk, either side, across the wrap
        if (rnd() % 50 == 0) t_lo = rnd();                         // anywhere on the clock
        if (t_lo > UINT64_MAX - span) t_lo = UINT64_MAX - span;    // (the table's rule: t_lo <= t_hi)
        const uint64_t t_hi = t_lo + span;
        int32_t a = 0, b = 0, na = 0, nb = 0;
        const bool got = rd_bx_range(sh[0], sh[1], sh[2], have_prev, clock, t_lo, t_hi, &a, &b);
        const bool want = naive(sh[0], sh[1], sh[2], have_prev, clock, t_lo, t_hi, &na, &nb);
        CHECK(got == want);
        if (got) {
            CHECK(a == na && b == nb && a <= b && b - a <= RD_BX_MAX_SPAN);
            found++;
            if ((a >= 0) != (clock + (uint64_t)(int64_t)a >= clock)) wrapped++;   // the window lies beyond 2^64 from the chunk's clock
        }
    }
    int32_t a, b;
    CHECK(!rd_bx_range(14, 80, 2048, 1, 0, 10, 5, &a, &b));      // t_lo > t_hi
    CHECK(!rd_bx_range(0, 80, 2048, 1, 0, 0, 5, &a, &b) && !rd_bx_range(14, 80, 2048, 1, 0, 0, 5, nullptr, &b));
    CHECK(!rd_bx_range(14, 80, 1000, 1, 0, 0, 5000, &a, &b) || a <= b);   // a block shorter than the packet
    printf("range ok: %ld of %d active, %ld across the wrap\n", found, n, wrapped);
    return 0;
}

static int test_repeats(void) {
    rd_burst_msg q;
    memset(&q, 0, sizeof q);
    q.channel = 2;
    q.time = UINT64_MAX - 3;
    q.data[0] = 0xCB;
    rd_burst_msg m = q;
    m.time = 9;                                                // 13 outputs on, across the wrap
    CHECK(rd_bx_repeats(m, &q, 1, 14) && !rd_bx_repeats(m, &q, 1, 13) && !rd_bx_repeats(m, &q, 0, 14) && !rd_bx_repeats(m, nullptr, 0, 14));
    m.time = UINT64_MAX - 16;                                  // 13 before
    CHECK(rd_bx_repeats(m, &q, 1, 14) && !rd_bx_repeats(m, &q, 1, 0));
    m.channel = 1;
    CHECK(!rd_bx_repeats(m, &q, 1, 14));
    m.channel = 2;
    m.data[9] = 1;
    CHECK(!rd_bx_repeats(m, &q, 1, 14));
    printf("repeats ok\n");
    return 0;
}

// The candidate test both decoders compile (rd_burst_candidate.h) on arrays of exactly the size it may read: a packet
// with its CRC, then the same with one and with two weak wrong symbols, every |s| else equal - the list's ties -, at
// strides 1, 3 and 14.
static int test_candidate(void) {
    const uint32_t sync = 0xCB89u;
    for (int n : {40, 64, 80})
        for (int sl : {1, 3, 14}) {
            std::vector<uint16_t> e((size_t)n, 0);
            for (int k = 16; k < n; k++) e[(size_t)k] = (uint16_t)rd_bd_syndrome(k, n);
            std::vector<uint32_t> air((size_t)(n / 8), 0u);          // the on-air bytes: sync, payload, CRC of the bit-swapped payload
            air[0] = sync >> 8;
            air[1] = sync & 0xFFu;
            uint32_t crc = 0u;
            for (int b = 2; b < n / 8 - 2; b++) {
                air[(size_t)b] = (uint32_t)(rnd() & 0xFFu);
                crc = rd_crc16_step(crc, rd_swap_bits8(air[(size_t)b]));
            }
            air[(size_t)(n / 8 - 2)] = rd_swap_bits8(crc >> 8);
            air[(size_t)(n / 8 - 1)] = rd_swap_bits8(crc & 0xFFu);
            std::vector<int> bit((size_t)n, 0);
            uint32_t syn = 0u;                                         // and the table is linear: the syndrome of a packet is 0
            for (int k = 0; k < n; k++) {
                bit[(size_t)k] = (int)((air[(size_t)(k >> 3)] >> (7 - (k & 7))) & 1u);
                if (bit[(size_t)k]) syn ^= e[(size_t)k];
            }
            CHECK(syn == 0u);
            std::vector<int64_t> s((size_t)(sl * (n - 1) + 1), INT64_MIN);   // (what lies between the symbols is never read)
            for (int k = 0; k < n; k++) s[(size_t)(sl * k)] = bit[(size_t)k] ? 1000 : -1000;
            rd_bd_cand c;
            CHECK(rd_bd_candidate<false>(s.data(), sl, n, sync, 0, nullptr, c) && c.flips == 0u && c.margin == 1000u);
            CHECK(rd_bd_candidate<true>(s.data(), sl, n, sync, 2, e.data(), c) && c.flips == 0u);
            CHECK(c.id == (uint32_t)(bit[16] | bit[17] << 1 | bit[18] << 2));
            const int k1 = 16 + (int)(rnd() % 3), k2 = n - 1;
            s[(size_t)(sl * k1)] = bit[(size_t)k1] ? -7 : 7;
            CHECK(!rd_bd_candidate<false>(s.data(), sl, n, sync, 0, nullptr, c));
            CHECK(rd_bd_candidate<true>(s.data(), sl, n, sync, 1, e.data(), c) && c.flips == (1u | (uint32_t)k1 << 8) && c.margin == 1000u);
            CHECK(c.id == (uint32_t)(bit[16] | bit[17] << 1 | bit[18] << 2));
            s[(size_t)(sl * k2)] = bit[(size_t)k2] ? -9 : 9;
            CHECK(!rd_bd_candidate<true>(s.data(), sl, n, sync, 1, e.data(), c));
            CHECK(rd_bd_candidate<true>(s.data(), sl, n, sync, 2, e.data(), c) && c.flips == (2u | (uint32_t)k1 << 8 | (uint32_t)k2 << 16));
            s[0] = -s[0];                                          // a wrong sync symbol: never
            CHECK(!rd_bd_candidate<true>(s.data(), sl, n, sync, 2, e.data(), c));
        }
    printf("candidate ok\n");
    return 0;
}

static int run_file(const char *in, const char *out) {
    FILE *f = fopen(in, "rb");
    CHECK(f);
    std::vector<int64_t> v;
    int64_t rec[7];
    while (fread(rec, sizeof rec, 1, f) == 1) v.insert(v.end(), rec, rec + 7);
    fclose(f);
    std::vector<int32_t> res;
    for (size_t i = 0; i + 7 <= v.size(); i += 7) {
        int32_t a = 0, b = -1;
        const bool got = rd_bx_range((int)v[i], (int)v[i + 1], (int)v[i + 2], (int)v[i + 3], (uint64_t)v[i + 4], (uint64_t)v[i + 5],
                                     (uint64_t)v[i + 6], &a, &b);
        res.insert(res.end(), {got ? 1 : 0, got ? a : 0, got ? b : -1});
    }
    f = fopen(out, "wb");
    CHECK(f);
    if (!res.empty()) CHECK(fwrite(res.data(), sizeof(int32_t), res.size(), f) == res.size());
    fclose(f);
    printf("file ok: %zu cases\n", res.size() / 3);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "table")) return test_table() || test_repeats() || test_candidate();
    if (argc >= 4 && !strcmp(argv[1], "range")) return test_range(strtoull(argv[2], nullptr, 10), atoi(argv[3]));
    if (argc >= 4 && !strcmp(argv[1], "file")) return run_file(argv[2], argv[3]);
    fprintf(stderr, "usage: track_asan table | range <seed> <n> | file <in> <out>\n");
    return 2;
}
