// replay_asan.cpp - the pure-host part of CLIP DECODE (rtldavis_amd/csrc/rd_host.cpp: rd_cd_check_jobs) under
// -fsanitize=address,undefined, driven by tests/test_replay_sanitizers.py.  A stand-alone program:
//   replay_asan limits            every rule at its limit, on either side of it
//   replay_asan file <in> <out>   job lists from a file (per list: int64 count, int64 pool_outputs, count x rd_clip_job)
//                                 -> 2 x int32 each (rc, bad)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../rtldavis_amd/csrc/rd_host.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static rd_config config() {
    rd_config c;
    memset(&c, 0, sizeof c);
    c.bit_rate = 19200;
    c.symbol_length = 14;
    c.preamble_symbols = 16;
    c.packet_symbols = 80;
    c.block_size = 2048;
    return c;
}

static rd_clip_job good(uint64_t offset, uint32_t n) {
    rd_clip_job j;
    memset(&j, 0, sizeof j);
    j.offset = offset;
    j.n = n;
    j.id = RD_BX_ANY_ID;
    j.tau_lo = 0;
    j.tau_hi = RD_CD_MAX_SPAN;
    return j;
}

// one job behind a good one: the answer and, when refused, the offender's index
static void expect(const rd_clip_job &j, size_t pool, bool ok, int *n_ok, int *n_bad) {
    const rd_config cfg = config();
    std::vector<rd_clip_job> jobs;                        // (exactly two: the sanitizer sees a read past the list)
    jobs.push_back(good(0, 8));
    jobs.push_back(j);
    int bad = 99;
    const char *why = nullptr;
    const int rc = rd_cd_check_jobs(&cfg, jobs.data(), 2, pool, &bad, &why);
    CHECK(why != nullptr);
    if (ok) {
        CHECK(rc == RD_OK && bad == -1 && !*why);
        ++*n_ok;
    } else {
        CHECK(rc == RD_ERR_ARG && bad == 1 && *why);
        ++*n_bad;
    }
    CHECK(rd_cd_check_jobs(&cfg, jobs.data(), 2, pool, nullptr, nullptr) == rc);   // the answers are optional
}

static int test_limits() {
    int n_ok = 0, n_bad = 0;
    const size_t pool = 4096;
    rd_clip_job j = good(8, 100);
    expect(j, pool, true, &n_ok, &n_bad);
    for (uint64_t off : {0ull, 8ull, 4088ull}) { j = good(off, 8); expect(j, pool, true, &n_ok, &n_bad); }
    for (uint64_t off : {1ull, 4ull, 7ull, 4095ull}) { j = good(off, 1); expect(j, pool, false, &n_ok, &n_bad); }
    j = good(4096, 1); expect(j, pool, false, &n_ok, &n_bad);                      // begins at the pool's end
    j = good(4088, 9); expect(j, pool, false, &n_ok, &n_bad);                      // one output past it
    j = good(0, 4096); expect(j, pool, true, &n_ok, &n_bad);
    j = good(0, 4097); expect(j, pool, false, &n_ok, &n_bad);
    j = good(0, 0); expect(j, pool, false, &n_ok, &n_bad);
    j = good(0, UINT32_MAX); expect(j, pool, false, &n_ok, &n_bad);
    j = good(UINT64_MAX - 7, 8); expect(j, pool, false, &n_ok, &n_bad);            // offset + n wraps
    j = good(UINT64_MAX - 7, UINT32_MAX); expect(j, pool, false, &n_ok, &n_bad);
    j = good(0, UINT32_MAX); expect(j, SIZE_MAX, true, &n_ok, &n_bad);             // the largest pool there is
    j = good(8, 8); j.tau_lo = 5; j.tau_hi = 5; expect(j, pool, true, &n_ok, &n_bad);
    j.tau_hi = 4; expect(j, pool, false, &n_ok, &n_bad);
    j.tau_lo = -100; j.tau_hi = -100 + RD_CD_MAX_SPAN; expect(j, pool, true, &n_ok, &n_bad);
    j.tau_hi++; expect(j, pool, false, &n_ok, &n_bad);
    j.tau_lo = INT32_MIN; j.tau_hi = INT32_MAX; expect(j, pool, false, &n_ok, &n_bad);   // the difference needs 64 bits
    j.tau_lo = -RD_CD_MAX_TAU; j.tau_hi = j.tau_lo + 10; expect(j, pool, true, &n_ok, &n_bad);
    j.tau_lo--; expect(j, pool, false, &n_ok, &n_bad);
    j.tau_hi = RD_CD_MAX_TAU; j.tau_lo = j.tau_hi - 10; expect(j, pool, true, &n_ok, &n_bad);
    j.tau_hi++; expect(j, pool, false, &n_ok, &n_bad);
    j.tau_lo = INT32_MIN; j.tau_hi = INT32_MIN; expect(j, pool, false, &n_ok, &n_bad);
    j.tau_lo = INT32_MAX; j.tau_hi = INT32_MAX; expect(j, pool, false, &n_ok, &n_bad);
    for (uint32_t id : {0u, 7u, (uint32_t)RD_BX_ANY_ID}) { j = good(8, 8); j.id = id; expect(j, pool, true, &n_ok, &n_bad); }
    for (uint32_t id : {8u, 0xFEu, 0x100u, UINT32_MAX}) { j = good(8, 8); j.id = id; expect(j, pool, false, &n_ok, &n_bad); }
    for (int32_t c : {-32768, 32767, 0}) {
        j = good(8, 8); j.corr_re = c; expect(j, pool, true, &n_ok, &n_bad);
        j = good(8, 8); j.corr_im = c; expect(j, pool, true, &n_ok, &n_bad);
    }
    for (int32_t c : {-32769, 32768, INT32_MIN, INT32_MAX}) {
        j = good(8, 8); j.corr_re = c; expect(j, pool, false, &n_ok, &n_bad);
        j = good(8, 8); j.corr_im = c; expect(j, pool, false, &n_ok, &n_bad);
    }
    j = good(8, 8); j.pad = 1; expect(j, pool, false, &n_ok, &n_bad);
    j = good(8, 8); j.pad = UINT32_MAX; expect(j, pool, false, &n_ok, &n_bad);
    // the count itself, and the null pointers: refused before a job is read
    const rd_config cfg = config();
    rd_clip_job one = good(0, 8);
    int bad = 99;
    const char *why = nullptr;
    for (int n : {0, -1, INT32_MIN, RD_CD_MAX_JOBS + 1, INT32_MAX}) {
        CHECK(rd_cd_check_jobs(&cfg, &one, n, pool, &bad, &why) == RD_ERR_ARG && bad == -1 && *why);
    }
    CHECK(rd_cd_check_jobs(&cfg, nullptr, 1, pool, &bad, &why) == RD_ERR_ARG && bad == -1);
    CHECK(rd_cd_check_jobs(nullptr, &one, 1, pool, &bad, &why) == RD_ERR_ARG && bad == -1);
    CHECK(rd_cd_check_jobs(&cfg, &one, 1, pool, &bad, &why) == RD_OK && bad == -1);
    CHECK(rd_cd_check_jobs(&cfg, &one, 1, 7, &bad, &why) == RD_ERR_ARG && bad == 0);
    std::vector<rd_clip_job> most((size_t)RD_CD_MAX_JOBS, good(0, 8));             // the largest list, its last job the offender
    CHECK(rd_cd_check_jobs(&cfg, most.data(), RD_CD_MAX_JOBS, pool, &bad, &why) == RD_OK);
    most.back().pad = 1;
    CHECK(rd_cd_check_jobs(&cfg, most.data(), RD_CD_MAX_JOBS, pool, &bad, &why) == RD_ERR_ARG && bad == RD_CD_MAX_JOBS - 1);
    printf("limits ok: %d accepted, %d refused\n", n_ok, n_bad);
    return 0;
}

static int run_file(const char *in, const char *out) {
    FILE *f = fopen(in, "rb");
    CHECK(f);
    const rd_config cfg = config();
    std::vector<int32_t> res;
    int64_t head[2];
    size_t lists = 0;
    while (fread(head, sizeof head, 1, f) == 1) {
        CHECK(head[0] >= 1 && head[0] <= 64);
        std::vector<rd_clip_job> jobs((size_t)head[0]);
        CHECK(fread(jobs.data(), sizeof(rd_clip_job), jobs.size(), f) == jobs.size());
        int bad = 99;
        const char *why = nullptr;
        res.push_back(rd_cd_check_jobs(&cfg, jobs.data(), (int)jobs.size(), (size_t)head[1], &bad, &why));
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
    static_assert(sizeof(rd_clip_job) == 48 && sizeof(rd_cd_header) == 16, "the layouts of CLIP DECODE");
    if (argc == 2 && !strcmp(argv[1], "limits")) return test_limits();
    if (argc == 4 && !strcmp(argv[1], "file")) return run_file(argv[2], argv[3]);
    fprintf(stderr, "usage: replay_asan limits | file <in> <out>\n");
    return 2;
}
