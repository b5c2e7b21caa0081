// synth_asan.cpp - the pure-host part of CLIP SYNTH (rtldavis_amd/csrc/rd_host.cpp: rd_cs_check_specs, rd_cs_table) under
// -fsanitize=address,undefined, driven by tests/test_synth_sanitizers.py.  A stand-alone program:
//   synth_asan limits            every rule at its limit, on either side of it
//   synth_asan table <out>       rd_cs_table into a heap buffer of exactly 4096 entries -> the entries, int16
//   synth_asan file <in> <out>   spec lists from a file (per list: int64 count, uint64 pool_outputs, count x rd_clip_spec)
//                                -> 2 x int32 each (rc, bad)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../rtldavis_amd/csrc/rd_host.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static rd_clip_spec good(uint64_t offset, uint32_t n) {
    rd_clip_spec s;
    memset(&s, 0, sizeof s);
    s.offset = offset;
    s.n = n;
    s.seed = 7;
    s.n_sym = 24;
    s.bits[0] = 0xA5;
    s.bits[2] = 0x01;                                     // symbol 23: the last one
    s.amp_q = 9800;
    s.noise_q = 362105;
    s.f_c = -(1 << 30);
    s.f_d = 76695845u;
    return s;
}

// one spec behind a good one (outputs 0 .. 7): the answer and, when refused, the offender's index
static void expect(const rd_clip_spec &s, uint64_t pool, bool ok, int *n_ok, int *n_bad) {
    std::vector<rd_clip_spec> specs;                      // (exactly two: the sanitizer sees a read past the list)
    specs.push_back(good(0, 8));
    specs.push_back(s);
    int bad = 99;
    const char *why = nullptr;
    const int rc = rd_cs_check_specs(specs.data(), 2, pool, &bad, &why);
    CHECK(why != nullptr);
    if (ok) {
        CHECK(rc == RD_OK && bad == -1 && !*why);
        ++*n_ok;
    } else {
        CHECK(rc == RD_ERR_ARG && bad == 1 && *why);
        ++*n_bad;
    }
    CHECK(rd_cs_check_specs(specs.data(), 2, pool, nullptr, nullptr) == rc);   // the answers are optional
}

static int test_limits() {
    int n_ok = 0, n_bad = 0;
    const uint64_t pool = 4096;
    rd_clip_spec s = good(8, 100);
    expect(s, pool, true, &n_ok, &n_bad);
    for (uint64_t off : {8ull, 16ull, 4088ull}) { s = good(off, 8); expect(s, pool, true, &n_ok, &n_bad); }
    for (uint64_t off : {9ull, 12ull, 15ull, 4095ull}) { s = good(off, 1); expect(s, pool, false, &n_ok, &n_bad); }
    s = good(0, 8); expect(s, pool, false, &n_ok, &n_bad);                         // on top of the first clip
    s = good(4096, 1); expect(s, pool, false, &n_ok, &n_bad);                      // begins at the pool's end
    s = good(4088, 9); expect(s, pool, false, &n_ok, &n_bad);                      // one output past it
    s = good(8, 4088); expect(s, pool, true, &n_ok, &n_bad);
    s = good(8, 4089); expect(s, pool, false, &n_ok, &n_bad);
    s = good(8, 0); expect(s, pool, false, &n_ok, &n_bad);
    s = good(8, RD_CS_MAX_N); expect(s, 8ull + RD_CS_MAX_N, true, &n_ok, &n_bad);
    s = good(8, RD_CS_MAX_N + 1); expect(s, UINT64_MAX, false, &n_ok, &n_bad);
    s = good(8, UINT32_MAX); expect(s, UINT64_MAX, false, &n_ok, &n_bad);
    s = good(UINT64_MAX - 7, 8); expect(s, pool, false, &n_ok, &n_bad);            // offset + n wraps
    s = good(UINT64_MAX - 7, 7); expect(s, UINT64_MAX, true, &n_ok, &n_bad);       // the last clip there can be
    s = good(UINT64_MAX - 15, 8); expect(s, UINT64_MAX, true, &n_ok, &n_bad);
    for (uint32_t k : {0u, 1u, 24u}) { s = good(8, 8); s.n_sym = k; if (k < 24) memset(s.bits, 0, sizeof s.bits); expect(s, pool, true, &n_ok, &n_bad); }
    s = good(8, 8); s.n_sym = 23; expect(s, pool, false, &n_ok, &n_bad);           // symbol 23 is set
    s = good(8, 8); s.n_sym = RD_CS_MAX_SYM; memset(s.bits, 0xFF, sizeof s.bits); expect(s, pool, true, &n_ok, &n_bad);
    s.n_sym = RD_CS_MAX_SYM - 1; expect(s, pool, false, &n_ok, &n_bad);
    s.n_sym = RD_CS_MAX_SYM + 1; expect(s, pool, false, &n_ok, &n_bad);            // (no bit of bits[] lies past it: never read)
    s.n_sym = UINT32_MAX; expect(s, pool, false, &n_ok, &n_bad);
    s = good(8, 8); s.bits[23] = 1; expect(s, pool, false, &n_ok, &n_bad);         // the last bit there is
    for (uint16_t p : {(uint16_t)0, (uint16_t)1, (uint16_t)RD_CS_MAX_PRE}) {
        s = good(8, 8); s.pre = p; expect(s, pool, true, &n_ok, &n_bad);
        s = good(8, 8); s.post = p; expect(s, pool, true, &n_ok, &n_bad);
    }
    for (uint16_t p : {(uint16_t)(RD_CS_MAX_PRE + 1), (uint16_t)UINT16_MAX}) {
        s = good(8, 8); s.pre = p; expect(s, pool, false, &n_ok, &n_bad);
        s = good(8, 8); s.post = p; expect(s, pool, false, &n_ok, &n_bad);
    }
    s = good(8, 8); s.amp_q = 0; s.noise_q = 0; expect(s, pool, true, &n_ok, &n_bad);
    s = good(8, 8); s.amp_q = RD_CS_MAX_AMP; s.noise_q = RD_CS_MAX_NOISE; expect(s, pool, true, &n_ok, &n_bad);
    s = good(8, 8); s.amp_q = RD_CS_MAX_AMP + 1u; expect(s, pool, false, &n_ok, &n_bad);
    s = good(8, 8); s.noise_q = RD_CS_MAX_NOISE + 1u; expect(s, pool, false, &n_ok, &n_bad);
    s = good(8, 8); s.amp_q = UINT32_MAX; expect(s, pool, false, &n_ok, &n_bad);
    s = good(8, 8); s.noise_q = UINT32_MAX; expect(s, pool, false, &n_ok, &n_bad);
    for (uint32_t f : {0u, 0x7FFFFFFFu}) { s = good(8, 8); s.f_d = f; expect(s, pool, true, &n_ok, &n_bad); }
    for (uint32_t f : {0x80000000u, UINT32_MAX}) { s = good(8, 8); s.f_d = f; expect(s, pool, false, &n_ok, &n_bad); }
    for (int32_t c : {INT32_MIN, INT32_MAX, 0}) { s = good(8, 8); s.f_c = c; s.phase0 = UINT32_MAX; expect(s, pool, true, &n_ok, &n_bad); }
    for (int32_t a : {-RD_CS_MAX_AT, RD_CS_MAX_AT, 0}) { s = good(8, 8); s.at = a; expect(s, pool, true, &n_ok, &n_bad); }
    for (int32_t a : {-RD_CS_MAX_AT - 1, RD_CS_MAX_AT + 1, INT32_MIN, INT32_MAX}) { s = good(8, 8); s.at = a; expect(s, pool, false, &n_ok, &n_bad); }
    s = good(8, 8); s.pad = 1; expect(s, pool, false, &n_ok, &n_bad);
    s = good(8, 8); s.pad = UINT32_MAX; expect(s, pool, false, &n_ok, &n_bad);
    s = good(8, 8); s.seed = UINT64_MAX; expect(s, pool, true, &n_ok, &n_bad);
    // the distance to the clip before: a first clip of 9 outputs owns 0 .. 15
    {
        std::vector<rd_clip_spec> two{good(0, 9), good(8, 8)};
        int bad = 99;
        const char *why = nullptr;
        CHECK(rd_cs_check_specs(two.data(), 2, pool, &bad, &why) == RD_ERR_ARG && bad == 1 && *why);
        two[1].offset = 16;
        CHECK(rd_cs_check_specs(two.data(), 2, pool, &bad, &why) == RD_OK && bad == -1);
        two[0] = good(UINT64_MAX - 7, 7);                 // its round-up passes 2^64: nothing may follow
        two[1] = good(0, 8);
        CHECK(rd_cs_check_specs(two.data(), 2, UINT64_MAX, &bad, &why) == RD_ERR_ARG && bad == 1);
    }
    // the count itself, and the null pointer: refused before a spec is read
    rd_clip_spec one = good(0, 8);
    int bad = 99;
    const char *why = nullptr;
    for (int n : {0, -1, INT32_MIN, RD_CS_MAX_SPECS + 1, INT32_MAX}) {
        CHECK(rd_cs_check_specs(&one, n, pool, &bad, &why) == RD_ERR_ARG && bad == -1 && *why);
    }
    CHECK(rd_cs_check_specs(nullptr, 1, pool, &bad, &why) == RD_ERR_ARG && bad == -1);
    CHECK(rd_cs_check_specs(&one, 1, pool, &bad, &why) == RD_OK && bad == -1);
    CHECK(rd_cs_check_specs(&one, 1, 7, &bad, &why) == RD_ERR_ARG && bad == 0);
    CHECK(rd_cs_check_specs(&one, 1, 0, &bad, &why) == RD_ERR_ARG && bad == 0);
    std::vector<rd_clip_spec> most((size_t)RD_CS_MAX_SPECS);                       // the largest list, its last spec the offender
    for (size_t k = 0; k < most.size(); k++) most[k] = good(8 * k, 8);
    CHECK(rd_cs_check_specs(most.data(), RD_CS_MAX_SPECS, 8ull * RD_CS_MAX_SPECS, &bad, &why) == RD_OK);
    most.back().pad = 1;
    CHECK(rd_cs_check_specs(most.data(), RD_CS_MAX_SPECS, 8ull * RD_CS_MAX_SPECS, &bad, &why) == RD_ERR_ARG && bad == RD_CS_MAX_SPECS - 1);
    printf("limits ok: %d accepted, %d refused\n", n_ok, n_bad);
    return 0;
}

static int write_table(const char *out) {
    int16_t *t = (int16_t *)malloc(RD_CS_TABLE * sizeof(int16_t));                 // exactly the table: a write past it is seen
    CHECK(t);
    rd_cs_table(t);
    rd_cs_table(nullptr);                                                          // (a null pointer is ignored)
    FILE *f = fopen(out, "wb");
    CHECK(f);
    CHECK(fwrite(t, sizeof(int16_t), RD_CS_TABLE, f) == RD_CS_TABLE);
    fclose(f);
    free(t);
    printf("table ok\n");
    return 0;
}

static int run_file(const char *in, const char *out) {
    FILE *f = fopen(in, "rb");
    CHECK(f);
    std::vector<int32_t> res;
    int64_t count;
    uint64_t pool;
    size_t lists = 0;
    while (fread(&count, sizeof count, 1, f) == 1) {
        CHECK(fread(&pool, sizeof pool, 1, f) == 1);
        CHECK(count >= 1 && count <= 64);
        std::vector<rd_clip_spec> specs((size_t)count);
        CHECK(fread(specs.data(), sizeof(rd_clip_spec), specs.size(), f) == specs.size());
        int bad = 99;
        const char *why = nullptr;
        res.push_back(rd_cs_check_specs(specs.data(), (int)specs.size(), pool, &bad, &why));
        res.push_back(bad);
        lists++;
    }
    fclose(f);
    f = fopen(out, "wb");
    CHECK(f);
    CHECK(res.empty() || fwrite(res.data(), sizeof(int32_t), res.size(), f) == res.size());
    fclose(f);
    printf("file ok: %zu lists\n", lists);
    return 0;
}

int main(int argc, char **argv) {
    static_assert(sizeof(rd_clip_spec) == 80, "the layout of CLIP SYNTH");
    if (argc == 2 && !strcmp(argv[1], "limits")) return test_limits();
    if (argc == 3 && !strcmp(argv[1], "table")) return write_table(argv[2]);
    if (argc == 4 && !strcmp(argv[1], "file")) return run_file(argv[2], argv[3]);
    fprintf(stderr, "usage: synth_asan limits | table <out> | file <in> <out>\n");
    return 2;
}
