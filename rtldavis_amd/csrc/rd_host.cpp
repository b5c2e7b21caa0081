// rd_host.cpp - see rd_host.h.  Pure host code: compiled by hipcc into the library and by g++ -fsanitize into
// tests/_build/host_asan (tests/test_host_sanitizers.py).
#include "rd_host.h"
#include "rd_parse.h"

#include <math.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>

// ------------------------------------------------------------------------------------------
// configuration (py:101-125)
// ------------------------------------------------------------------------------------------
int rd_make_devcfg(const rd_config *c, rd_devcfg *d, const char **why) {
    static const char *none = "";
    const char *dummy;
    if (!why) why = &dummy;
    *why = none;
    if (!c || !d) { *why = "null config"; return RD_ERR_ARG; }
    if (c->symbol_length < 1 || c->preamble_symbols < 1 || c->preamble_symbols > RD_MAX_PREAMBLE ||
        c->packet_symbols < 1 || c->packet_symbols > 8 * RD_MAX_PKT_BYTES) {
        *why = "unsupported packet configuration";
        return RD_ERR_ARG;
    }
    if (c->packet_symbols < c->preamble_symbols) { *why = "packet_symbols < preamble_symbols is not supported"; return RD_ERR_ARG; }
    if (c->block_size < 32 || c->block_size % 4) {
        *why = "block_size must be a multiple of 4 and >= 32 (rotate_fs4, py:46-49)";
        return RD_ERR_ARG;
    }
    if (c->bit_rate < 1) { *why = "bit_rate must be positive"; return RD_ERR_ARG; }
    // (symbol_length is bounded by the products below; both fit 64 bits for any int32 inputs)
    const long packet_length = (long)c->packet_symbols * c->symbol_length;
    const long preamble_length = (long)c->preamble_symbols * c->symbol_length;
    const long L = (packet_length / c->block_size + 2) * (long)c->block_size;
    if (L > 0x3FFFFFFF || preamble_length > 0x3FFFFFFF) { *why = "buffer_length too large"; return RD_ERR_ARG; }
    d->S = c->symbol_length;
    d->P = c->preamble_symbols;
    d->K = c->packet_symbols;
    d->B = c->block_size;
    d->PL = (int32_t)preamble_length;
    d->L = (int32_t)L;
    d->nbytes = (c->packet_symbols + 7) / 8;
    d->fs = (double)c->bit_rate * (double)c->symbol_length;
    d->pre_mask = 0;
    for (int i = 0; i < c->preamble_symbols; i++) {
        if (c->preamble[i] > 1) { *why = "preamble symbols must be 0 or 1"; return RD_ERR_ARG; }
        d->pre_mask |= (uint64_t)c->preamble[i] << i;
    }
    return RD_OK;
}

int rd_check_block_count(int is_complex, size_t count, size_t B, size_t NS, size_t *expected) {
    const size_t want = is_complex ? B : NS * 2 * B;
    if (expected) *expected = want;
    return count == want ? RD_OK : RD_ERR_ARG;
}

// ------------------------------------------------------------------------------------------
// Parser.parse's front half for one packet (protocol.py:290-318), host only: the arithmetic of rd_parse.h
// ------------------------------------------------------------------------------------------
extern "C" int rd_parse_packet(const uint8_t *data, int nbytes, uint8_t *msg, int *id) {
    if (nbytes < 0 || nbytes > RD_MAX_PKT_BYTES || (nbytes > 0 && !data)) return RD_ERR_ARG;
    if (nbytes <= 2) return 0;
    uint32_t crc = 0;
    for (int k = 2; k < nbytes; k++) crc = rd_crc16_step(crc, rd_swap_bits8(data[k]));
    if (crc != 0) return 0;
    if (!msg || !id) return RD_ERR_ARG;
    for (int k = 2; k < nbytes; k++) msg[k - 2] = (uint8_t)rd_swap_bits8(data[k]);
    *id = msg[0] & 7;
    return 1;
}

uint32_t rd_ord_bucket_cap(long n_samples) {
    if (n_samples < 0) n_samples = 0;
    // 4 x (n / 2^16) + 12, rounded up to a multiple of 32: 33 blocks of 8192 -> 32 (what the bench shape has always
    // used), 330 blocks -> 192
    const long want = (4 * n_samples + 65535) / 65536 + 12;
    long cap = ((want + 31) / 32) * 32;
    if (cap < RD_BUCKET_MIN) cap = RD_BUCKET_MIN;
    if (cap > RD_BUCKET_MAX) cap = RD_BUCKET_MAX;
    return (uint32_t)cap;
}

// ------------------------------------------------------------------------------------------
// order + dedupe.  Small lists: std::sort.  Large lists: the key is packed into 64 bits (when the field widths
// allow) and sorted with LSD counting passes over (key, index) pairs - a comparison sort that moves 64-byte records
// costs tens of milliseconds at 7e4 records.  `recs` may be pinned memory.
// ------------------------------------------------------------------------------------------
void rd_order_and_dedupe(const rd_packet *recs, size_t n, int S, rd_order_scratch &sc) {
    std::vector<uint32_t> &idx = sc.idx, &kept = sc.kept;
    kept.clear();
    idx.clear();
    if (n == 0 || S < 1) return;
    idx.reserve(n);
    for (size_t i = 0; i < n; i++)
        if (recs[i].stream >= 0) idx.push_back((uint32_t)i);  // stream < 0: match reported by no call
    n = idx.size();
    if (n == 0) return;
    auto less = [&](uint32_t ia, uint32_t ib) {
        const rd_packet &a = recs[ia], &b = recs[ib];
        if (a.stream != b.stream) return a.stream < b.stream;
        if (a.call != b.call) return a.call < b.call;
        const int pa = a.index % S, pb = b.index % S;
        if (pa != pb) return pa < pb;
        return a.index < b.index;
    };
    bool radix = n >= 512;
    if (radix) {
        // field widths (negative calls / indices never come from the kernels; they take the comparison sort)
        uint32_t max_stream = 0, max_call = 0, max_index = 0;
        for (size_t i = 0; i < n && radix; i++) {
            const rd_packet &r = recs[idx[i]];
            if (r.call < 0 || r.index < 0) radix = false;
            max_stream = std::max(max_stream, (uint32_t)r.stream);
            max_call = std::max(max_call, (uint32_t)r.call);
            max_index = std::max(max_index, (uint32_t)r.index);
        }
        auto bits_for = [](uint32_t v) { int b = 1; while (b < 32 && (v >> b)) b++; return b; };
        const int bi = bits_for(max_index), bp = bits_for((uint32_t)(S - 1)), bc = bits_for(max_call),
                  bs = bits_for(max_stream);
        if (radix && bi + bp + bc + bs <= 64) {
            std::vector<uint64_t> &key = sc.key, &ktmp = sc.ktmp;
            std::vector<uint32_t> &itmp = sc.itmp;
            key.resize(n); ktmp.resize(n); itmp.resize(n);
            for (size_t i = 0; i < n; i++) {
                const rd_packet &r = recs[idx[i]];
                key[i] = ((((uint64_t)(uint32_t)r.stream << bc | (uint32_t)r.call) << bp | (uint32_t)(r.index % S)) << bi) |
                         (uint32_t)r.index;
            }
            // LSD passes of 12 bits (the bench shape's 36-bit key: three)
            const int total_bits = bi + bp + bc + bs;
            constexpr int DB = 12;
            static thread_local uint32_t count[(1 << DB) + 1];
            for (int shift = 0; shift < total_bits; shift += DB) {
                memset(count, 0, sizeof count);
                for (size_t i = 0; i < n; i++) count[((key[i] >> shift) & ((1u << DB) - 1)) + 1]++;
                for (int d = 0; d < (1 << DB); d++) count[d + 1] += count[d];
                for (size_t i = 0; i < n; i++) {
                    const uint32_t pos = count[(key[i] >> shift) & ((1u << DB) - 1)]++;
                    ktmp[pos] = key[i];
                    itmp[pos] = idx[i];
                }
                key.swap(ktmp);
                idx.swap(itmp);
            }
        } else {
            radix = false;
        }
    }
    if (!radix) std::sort(idx.begin(), idx.end(), less);
    // per-call dedupe (py:203-205): the first occurrence of a byte string inside (stream, call) wins
    kept.reserve(n);
    size_t group = 0;
    for (size_t i = 0; i < n; i++) {
        const rd_packet &r = recs[idx[i]];
        if (kept.empty() || r.stream != recs[kept.back()].stream || r.call != recs[kept.back()].call) group = kept.size();
        const size_t nb = r.nbytes < 0 ? 0 : r.nbytes > RD_MAX_PKT_BYTES ? (size_t)RD_MAX_PKT_BYTES : (size_t)r.nbytes;
        bool dup = false;
        for (size_t k = group; k < kept.size() && !dup; k++) dup = memcmp(recs[kept[k]].data, r.data, nb) == 0;
        if (!dup) kept.push_back(idx[i]);
    }
}

// ------------------------------------------------------------------------------------------
// host waits
// ------------------------------------------------------------------------------------------
static double mono_ms() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}

static double g_timeout_override = -1.0;  // < 0: none

static double env_timeout_ms() {
    static const double v = [] {
        const char *e = getenv("RD_WAIT_TIMEOUT_MS");
        if (e && *e) {
            char *end = nullptr;
            const double x = strtod(e, &end);
            if (end != e && x >= 0.0) return x;
        }
        return 10000.0;
    }();
    return v;
}

double rd_wait_timeout_ms(void) { return g_timeout_override >= 0.0 ? g_timeout_override : env_timeout_ms(); }

double rd_wait_timeout_set(double ms) {
    const double prev = rd_wait_timeout_ms();
    g_timeout_override = ms < 0.0 ? -1.0 : ms;
    return prev;
}

rd_waiter::rd_waiter(double timeout_ms_) : t_start_ms(mono_ms()), timeout_ms(timeout_ms_), polls(0) {}

double rd_waiter::waited_ms() const { return mono_ms() - t_start_ms; }

bool rd_waiter::relax() {
    polls++;
    if (timeout_ms <= 0.0) return false;  // (the test hook: whatever is not ready at its first poll times out)
    // the clock is read at the first poll and every 32 polls while spinning (a poll of a flag in pinned memory takes
    // tens of nanoseconds; a hipEventQuery about a microsecond), on every poll afterwards
    if (polls < 1024 && (polls & 31) != 1) {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
        return true;
    }
    const double waited = mono_ms() - t_start_ms;
    if (waited >= timeout_ms) return false;
    if (waited < 0.05) {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
        if (polls >= 1024) polls = 992;  // stay in the spinning regime until 50 us have passed
    } else if (waited < 1.0) {
        sched_yield();
    } else {
        struct timespec ts = {0, 50000};  // 50 us: an overdue wait does not pin a core
        nanosleep(&ts, nullptr);
    }
    return true;
}

bool rd_msg_repeats(const rd_burst_msg &m, const rd_burst_msg *delivered, size_t n_delivered, int sl, bool look_back, bool same_centre) {
    if ((look_back && !(m.flags & 1u)) || sl <= 0) return false;
    for (size_t i = 0; i < n_delivered; i++) {
        const rd_burst_msg &q = delivered[i];
        const uint64_t d = m.time - q.time, ad = d < 0ull - d ? d : 0ull - d;   // (the clock wraps at 2^64)
        if (q.channel == m.channel && (!same_centre || q.pad[3] == m.pad[3]) && !memcmp(q.data, m.data, sizeof m.data) && ad < (uint64_t)sl)
            return true;
    }
    return false;
}

// BURST EXPECT (include/rtldavis_hip.h): the table's rules, one expectation's candidates in a chunk
int rd_bx_check_table(const rd_expect *e, int n, int n_channels, int *bad, const char **why) {
    static const char *none = "";
    const char *dummy_why;
    int dummy_bad;
    if (!why) why = &dummy_why;
    if (!bad) bad = &dummy_bad;
    *why = none;
    *bad = -1;
    if (n < 0 || n > RD_BX_MAX) { *why = "the number of expectations (0 .. 64)"; return RD_ERR_ARG; }
    if (n > 0 && !e) { *why = "null table"; return RD_ERR_ARG; }
    for (int i = 0; i < n; i++) {
        const rd_expect &x = e[i];
        *bad = i;
        if (x.channel < 0 || x.channel >= n_channels) { *why = "channel"; return RD_ERR_ARG; }
        if (x.id >= 8u && x.id != RD_BX_ANY_ID) { *why = "id (0 .. 7 or 0xFF)"; return RD_ERR_ARG; }
        if (x.t_lo > x.t_hi) { *why = "t_lo > t_hi"; return RD_ERR_ARG; }
        if (x.t_hi - x.t_lo > (uint64_t)RD_BX_MAX_SPAN) { *why = "t_hi - t_lo (at most 2048)"; return RD_ERR_ARG; }
        if (x.corr_re < -32768 || x.corr_re > 32767 || x.corr_im < -32768 || x.corr_im > 32767) { *why = "corr (-32768 .. 32767)"; return RD_ERR_ARG; }
        if (x.corr_re == 0 && x.corr_im == 0) { *why = "corr = (0, 0)"; return RD_ERR_ARG; }
    }
    *bad = -1;
    return RD_OK;
}

bool rd_bx_range(int sl, int n_sym, int block_size, int have_prev, uint64_t clock, uint64_t t_lo, uint64_t t_hi, int32_t *tau_a,
                 int32_t *tau_b) {
    if (sl < 1 || n_sym < 1 || block_size < 1 || t_lo > t_hi || !tau_a || !tau_b) return false;
    const int64_t body = (int64_t)sl * (int64_t)(n_sym - 1);
    const int64_t lo_b = have_prev ? -body : (int64_t)sl;      // 0 <= tau + SL (N - 1); tau - SL >= 0 with no chunk before
    const int64_t hi_b = (int64_t)block_size - 1 - body;        // tau + SL (N - 1) < B
    if (hi_b < lo_b) return false;
    const uint64_t span = t_hi - t_lo;
    const uint64_t start = clock + (uint64_t)lo_b;              // the clock of tau = lo_b, modulo 2^64
    const uint64_t u = start - t_lo;                            // how far lo_b lies inside the window ...
    int64_t a;
    uint64_t room;                                              // ... and how much of the window is left from tau_a on
    if (u <= span) {
        a = lo_b;
        room = span - u;
    } else {
        const uint64_t v = t_lo - start;                        // outputs from lo_b to the window's first
        if (v > (uint64_t)(hi_b - lo_b)) return false;
        a = lo_b + (int64_t)v;
        room = span;
    }
    const int64_t b = room > (uint64_t)(hi_b - a) ? hi_b : a + (int64_t)room;
    *tau_a = (int32_t)a;
    *tau_b = (int32_t)b;
    return true;
}

// CLIP DECODE (include/rtldavis_hip.h): the rules of a job list.  cfg takes no part in them today - a job that has no
// candidate for its SL and N is legal and idle - and is there so that a rule that needs it changes no signature.
extern "C" int rd_cd_check_jobs(const rd_config *cfg, const rd_clip_job *jobs, int n_jobs, size_t pool_outputs, int *bad,
                                const char **why) {
    static const char *none = "";
    const char *dummy_why;
    int dummy_bad;
    if (!why) why = &dummy_why;
    if (!bad) bad = &dummy_bad;
    *why = none;
    *bad = -1;
    if (!cfg) { *why = "null configuration"; return RD_ERR_ARG; }
    if (n_jobs < 1 || n_jobs > RD_CD_MAX_JOBS) { *why = "the number of jobs (1 .. 2^20)"; return RD_ERR_ARG; }
    if (!jobs) { *why = "null job list"; return RD_ERR_ARG; }
    for (int i = 0; i < n_jobs; i++) {
        const rd_clip_job &j = jobs[i];
        *bad = i;
        if (j.offset % 8u) { *why = "offset (a multiple of 8)"; return RD_ERR_ARG; }
        if (j.n < 1u) { *why = "n < 1"; return RD_ERR_ARG; }
        if (j.offset > (uint64_t)pool_outputs || (uint64_t)j.n > (uint64_t)pool_outputs - j.offset) { *why = "offset + n past the pool"; return RD_ERR_ARG; }
        if (j.tau_lo > j.tau_hi) { *why = "tau_lo > tau_hi"; return RD_ERR_ARG; }
        if ((int64_t)j.tau_hi - (int64_t)j.tau_lo > (int64_t)RD_CD_MAX_SPAN) { *why = "tau_hi - tau_lo (at most 2048)"; return RD_ERR_ARG; }
        if (j.tau_lo < -RD_CD_MAX_TAU || j.tau_lo > RD_CD_MAX_TAU || j.tau_hi < -RD_CD_MAX_TAU || j.tau_hi > RD_CD_MAX_TAU) { *why = "tau (-2^30 .. 2^30)"; return RD_ERR_ARG; }
        if (j.id >= 8u && j.id != RD_BX_ANY_ID) { *why = "id (0 .. 7 or 0xFF)"; return RD_ERR_ARG; }
        if (j.corr_re < -32768 || j.corr_re > 32767 || j.corr_im < -32768 || j.corr_im > 32767) { *why = "corr (-32768 .. 32767)"; return RD_ERR_ARG; }
        if (j.pad != 0u) { *why = "pad != 0"; return RD_ERR_ARG; }
    }
    *bad = -1;
    return RD_OK;
}

// CLIP SYNTH (include/rtldavis_hip.h): the rules of a spec list.  k_clip_synth applies the per-spec bounds again; the
// order of the specs and their distance are checked here alone.
extern "C" int rd_cs_check_specs(const rd_clip_spec *specs, int n_specs, uint64_t pool_outputs, int *bad, const char **why) {
    static const char *none = "";
    const char *dummy_why;
    int dummy_bad;
    if (!why) why = &dummy_why;
    if (!bad) bad = &dummy_bad;
    *why = none;
    *bad = -1;
    if (n_specs < 1 || n_specs > RD_CS_MAX_SPECS) { *why = "the number of specs (1 .. 2^20)"; return RD_ERR_ARG; }
    if (!specs) { *why = "null spec list"; return RD_ERR_ARG; }
    uint64_t next = 0;                                          // roundup8 of the end of the clip before (below 2^64: see the pool rule)
    for (int i = 0; i < n_specs; i++) {
        const rd_clip_spec &s = specs[i];
        *bad = i;
        if (s.offset % 8u) { *why = "offset (a multiple of 8)"; return RD_ERR_ARG; }
        if (s.n < 1u || s.n > (uint32_t)RD_CS_MAX_N) { *why = "n (1 .. 2^24)"; return RD_ERR_ARG; }
        if (s.offset < next) { *why = "the specs ascend and do not overlap"; return RD_ERR_ARG; }
        if (s.offset > pool_outputs || (uint64_t)s.n > pool_outputs - s.offset) { *why = "offset + n past the pool"; return RD_ERR_ARG; }
        if (s.n_sym > (uint32_t)RD_CS_MAX_SYM) { *why = "n_sym (0 .. 192)"; return RD_ERR_ARG; }
        if (s.pre > RD_CS_MAX_PRE || s.post > RD_CS_MAX_PRE) { *why = "pre, post (0 .. 4096)"; return RD_ERR_ARG; }
        if (s.amp_q > RD_CS_MAX_AMP) { *why = "amp_q (at most 2^16)"; return RD_ERR_ARG; }
        if (s.noise_q > RD_CS_MAX_NOISE) { *why = "noise_q (at most 2^20)"; return RD_ERR_ARG; }
        if (s.f_d >= 0x80000000u) { *why = "f_d (below 2^31)"; return RD_ERR_ARG; }
        if (s.at < -RD_CS_MAX_AT || s.at > RD_CS_MAX_AT) { *why = "at (-2^30 .. 2^30)"; return RD_ERR_ARG; }
        if (s.pad != 0u) { *why = "pad != 0"; return RD_ERR_ARG; }
        for (uint32_t j = s.n_sym; j < 8u * sizeof s.bits; j++)
            if (s.bits[j >> 3] & (0x80u >> (j & 7u))) { *why = "a bit of bits[] past n_sym"; return RD_ERR_ARG; }
        // (offset + n <= pool_outputs < 2^64; the round-up wraps only for an end within 7 of 2^64, to 0: then nothing may follow)
        next = (s.offset + (uint64_t)s.n + 7u) & ~(uint64_t)7u;
        if (next < s.offset) next = UINT64_MAX;
    }
    *bad = -1;
    return RD_OK;
}

// CLIP SYNTH: T[j] = lrint(16384 cos(2 pi j / 4096)) in float64, the argument formed as written
extern "C" void rd_cs_table(int16_t out[RD_CS_TABLE]) {
    if (!out) return;
    for (int j = 0; j < RD_CS_TABLE; j++) out[j] = (int16_t)lrint(16384.0 * cos(2.0 * M_PI * (double)j / 4096.0));
}

// BURST SEARCH (include/rtldavis_hip.h): the list's rules (a chunk's candidates, step 2s: rd_host.h, inline)
int rd_bs_check_centres(const uint8_t *centres, int n, int *bad, const char **why) {
    static const char *none = "";
    const char *dummy_why;
    int dummy_bad;
    if (!why) why = &dummy_why;
    if (!bad) bad = &dummy_bad;
    *why = none;
    *bad = -1;
    if (n < 0 || n > RD_BS_MAX_CENTRES) { *why = "the number of centres (0 .. 8)"; return RD_ERR_ARG; }
    if (n > 0 && !centres) { *why = "null list"; return RD_ERR_ARG; }
    for (int i = 0; i < n; i++) {
        *bad = i;
        if (centres[i] >= RD_BD_NB_GRID) { *why = "centre (0 .. 63)"; return RD_ERR_ARG; }
        for (int j = 0; j < i; j++)
            if (centres[j] == centres[i]) { *why = "duplicate"; return RD_ERR_ARG; }
    }
    *bad = -1;
    return RD_OK;
}

// BURST DECODE step 4n (include/rtldavis_hip.h): designed in float64, every product and quotient in the order written
// there - tests/burst_narrow_cases.py evaluates the same expressions in NumPy and must get the same integers.
extern "C" int rd_bd_narrow_table(int sl, int16_t *taps, int16_t *centres) {
    if (sl < RD_BD_NB_MIN_SL || sl > RD_BD_NB_MAX_SL || !taps || !centres) return RD_ERR_ARG;
    const int T = 2 * sl + 5, M = sl + 2;
    const double pi = 3.141592653589793;
    std::vector<double> h((size_t)T);
    double sum = 0.0;
    for (int k = -M; k <= M; k++) {
        const double w = 0.54 + 0.46 * cos(2.0 * pi * (double)k / (double)(T - 1));
        const double x = 1.8 * (double)k / (double)sl;
        const double sinc = k == 0 ? 1.0 : sin(pi * x) / (pi * x);
        h[(size_t)(k + M)] = sinc * w;
        sum += h[(size_t)(k + M)];
    }
    for (int k = 0; k < T; k++) h[(size_t)k] /= sum;
    for (int g = 0; g < RD_BD_NB_GRID; g++) {
        for (int k = -M; k <= M; k++) {
            const int m = (((g * k) % RD_BD_NB_GRID) + RD_BD_NB_GRID) % RD_BD_NB_GRID;   // reduced in integers
            const double a = 2.0 * pi * (double)m / (double)RD_BD_NB_GRID, hk = 16384.0 * h[(size_t)(k + M)];
            taps[2 * ((size_t)g * (size_t)T + (size_t)(k + M))] = (int16_t)rint(hk * cos(a));
            taps[2 * ((size_t)g * (size_t)T + (size_t)(k + M)) + 1] = (int16_t)rint(hk * sin(a));
        }
        const double a = 2.0 * pi * (double)g / (double)RD_BD_NB_GRID;
        centres[2 * g] = (int16_t)rint(16384.0 * cos(a));
        centres[2 * g + 1] = (int16_t)rint(16384.0 * sin(a));
    }
    return RD_OK;
}

// BURST QUALITY (include/rtldavis_hip.h): the windows of one record, through the C ABI (rd_host.h: rd_bq_windows_of)
extern "C" int rd_bq_window(int sl, int n_sym, int block_size, int have_prev, int64_t tau, int gap, int32_t *out) {
    if (!out) return 0;
    rd_bq_windows w;
    const bool ok = rd_bq_windows_of(sl, n_sym, block_size, have_prev, tau, gap, &w);
    out[0] = w.p0;
    out[1] = w.p1;
    out[2] = w.s1;
    out[3] = w.n0;
    out[4] = w.n1;
    return ok ? 1 : 0;
}

// BURST CLIPS (include/rtldavis_hip.h): the clamp of one request, through the C ABI (rd_host.h: rd_bc_window_of)
extern "C" int rd_bc_window(int block_size, int have_prev, int64_t a, int64_t e, int32_t *out) {
    if (!out) return 0;
    rd_bc_clamped c;
    const bool ok = rd_bc_window_of(block_size, have_prev, a, e, &c);
    out[0] = c.t0;
    out[1] = c.n;
    out[2] = c.flags;
    return ok ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// the receiver's fetch (rd_host.h: rd_collect_*)
// ------------------------------------------------------------------------------------------
#define COLLECT_FAIL(...) return (snprintf(err->text, sizeof err->text, __VA_ARGS__), RD_ERR_DEVICE)

int rd_collect_levels(const void *slot, int n_ch, long chunk, std::vector<rd_chan_level> &lv, rd_input_level *in, rd_errtext *err) {
    const rd_chan_level *rec = (const rd_chan_level *)slot;
    lv.assign(rec, rec + n_ch);
    memcpy(in, rec + n_ch, sizeof *in);
    for (int c = 0; c < n_ch; c++)
        if (lv[c].chunk != (uint32_t)chunk) COLLECT_FAIL("level record of channel %d belongs to chunk %u, not %ld", c, lv[c].chunk, chunk);
    if (in->chunk != (uint64_t)chunk) COLLECT_FAIL("the input level record belongs to chunk %llu, not %ld", (unsigned long long)in->chunk, chunk);
    return RD_OK;
}

int rd_collect_spectrum(const void *slot, int n_bins, long chunk, rd_spectrum_info *info, std::vector<double> &power, rd_errtext *err) {
    memcpy(info, slot, sizeof *info);
    if (info->chunk != (uint64_t)chunk || (int)info->n_bins != n_bins)
        COLLECT_FAIL("the spectrum record belongs to chunk %llu (%u bins), not %ld (%d bins)", (unsigned long long)info->chunk, info->n_bins,
                     chunk, n_bins);
    const double *p = (const double *)((const uint8_t *)slot + RD_SPEC_HDR_BYTES);
    power.assign(p, p + n_bins);
    return RD_OK;
}

int rd_collect_bursts(const void *slot, int n_ch, size_t n_win, long chunk, std::vector<rd_burst> &runs, std::vector<rd_burst_floor> &floor,
                      rd_errtext *err) {
    const size_t cap = rd_bu_cap(n_win);
    const rd_burst *recs = (const rd_burst *)slot;
    const rd_burst_floor *fl = (const rd_burst_floor *)((const uint8_t *)slot + rd_bu_floor_offset(n_ch, n_win));
    floor.assign(fl, fl + n_ch);
    runs.clear();
    for (int c = 0; c < n_ch; c++) {
        if (floor[c].chunk != (uint32_t)chunk || floor[c].n_bursts > cap)
            COLLECT_FAIL("burst floor record of channel %d belongs to chunk %u (%u runs), not %ld", c, floor[c].chunk, floor[c].n_bursts, chunk);
        runs.insert(runs.end(), recs + (size_t)c * cap, recs + (size_t)c * cap + floor[c].n_bursts);
    }
    return RD_OK;
}

int rd_collect_decode(const void *slot, const void *qslot, int n_ch, size_t n_win, long chunk, int sl, rd_delivered &hist,
                      std::vector<uint32_t> &long_runs, std::vector<rd_burst_quality> &qual, rd_errtext *err) {
    const size_t cap = rd_bu_cap(n_win);
    const rd_burst_msg *recs = (const rd_burst_msg *)slot;
    const rd_bd_header *hd = (const rd_bd_header *)((const uint8_t *)slot + rd_bd_header_offset(n_ch, n_win));
    const rd_burst_quality *qrecs = (const rd_burst_quality *)qslot;
    hist.begin(chunk);
    qual.clear();
    long_runs.assign(n_ch, 0u);
    for (int c = 0; c < n_ch; c++) {
        const rd_bd_header h = hd[c];
        if (h.chunk != (uint32_t)chunk || h.n_msgs > cap)
            COLLECT_FAIL("burst message header of channel %d belongs to chunk %u (%u messages), not %ld", c, h.chunk, h.n_msgs, chunk);
        long_runs[c] = h.long_runs;
        for (uint32_t i = 0; i < h.n_msgs; i++) {
            const rd_burst_msg m = recs[(size_t)c * cap + i];
            if (hist.repeats(m, sl, true, false)) continue;   // step 7
            hist.last.push_back(m);
            if (!qrecs) continue;
            const rd_burst_quality q = qrecs[(size_t)c * cap + i];
            if (q.chunk != (uint32_t)chunk) COLLECT_FAIL("quality record %u of channel %d belongs to chunk %u, not %ld", i, c, q.chunk, chunk);
            qual.push_back(q);
        }
    }
    hist.commit(chunk);
    return RD_OK;
}

int rd_collect_expect(const void *slot, const void *qslot, int n_ch, size_t n_win, long chunk, int sl, int n, const uint32_t *cand,
                      rd_delivered &hist, uint32_t *counts, std::vector<rd_burst_quality> &qual, rd_errtext *err) {
    const rd_burst_msg *recs = (const rd_burst_msg *)slot;
    const rd_bx_header *hd = (const rd_bx_header *)((const uint8_t *)slot + RD_BX_HEADER_OFFSET);
    const rd_burst_quality *qrecs = qslot ? (const rd_burst_quality *)((const uint8_t *)qslot + rd_bq_expect_offset(n_ch, n_win)) : nullptr;
    hist.begin(chunk);
    qual.clear();
    for (int i = 0; i < RD_BX_MAX; i++) counts[i] = i < n ? 0u : RD_BX_NO_ENTRY;
    for (int i = 0; slot && i < n; i++) {
        const rd_bx_header h = hd[i];
        if (h.chunk != (uint32_t)chunk || h.n_msgs > 1u || h.candidates != cand[i])
            COLLECT_FAIL("expectation %d: header of chunk %u (%u messages, %u candidates), not of chunk %ld with %u candidates", i, h.chunk,
                         h.n_msgs, h.candidates, chunk, cand[i]);
        counts[i] = h.candidates;
        if (!h.n_msgs || hist.repeats(recs[i], sl, false, false)) continue;   // step 7'
        hist.last.push_back(recs[i]);
        if (!qrecs) continue;
        const rd_burst_quality q = qrecs[i];
        if (q.chunk != (uint32_t)chunk) COLLECT_FAIL("quality record of expectation %d belongs to chunk %u, not %ld", i, q.chunk, chunk);
        qual.push_back(q);
    }
    hist.commit(chunk);
    return RD_OK;
}

int rd_collect_search(const void *slot, int n_ch, long chunk, int sl, int n, rd_delivered &hist, std::vector<rd_bs_header> &hdr,
                      rd_errtext *err) {
    hist.begin(chunk);
    hdr.clear();
    if (n) {
        const rd_burst_msg *recs = (const rd_burst_msg *)slot;
        const rd_bs_header *hd = (const rd_bs_header *)((const uint8_t *)slot + rd_bs_header_offset(n_ch));
        hdr.assign(hd, hd + (size_t)n * (size_t)n_ch);
        for (size_t g = 0; g < hdr.size(); g++) {   // g = centre * n_ch + channel
            const rd_bs_header h = hdr[g];
            if (h.chunk != (uint32_t)chunk || h.n_msgs > (uint32_t)RD_BS_PER)
                COLLECT_FAIL("search header of centre %d, channel %d belongs to chunk %u (%u messages), not %ld", (int)(g / (size_t)n_ch),
                             (int)(g % (size_t)n_ch), h.chunk, h.n_msgs, chunk);
            for (uint32_t r = 0; r < h.n_msgs; r++) {
                const rd_burst_msg m = recs[g * RD_BS_PER + r];
                if (!hist.repeats(m, sl, false, true)) hist.last.push_back(m);   // step 7s
            }
        }
    }
    hist.commit(chunk);
    return RD_OK;
}

int rd_collect_clips(const void *slot, int n_ch, int quota, long chunk, std::vector<rd_burst_clip> &clips, std::vector<uint8_t> &bytes,
                     std::vector<uint32_t> &dropped, rd_errtext *err) {
    const size_t q = (size_t)quota;
    const rd_burst_clip *recs = (const rd_burst_clip *)slot;
    const rd_bc_header *hd = (const rd_bc_header *)((const uint8_t *)slot + rd_bc_header_offset(n_ch));
    const uint8_t *pool = (const uint8_t *)slot + rd_bc_pool_offset(n_ch);
    clips.clear();
    bytes.clear();
    dropped.assign(n_ch, 0u);
    for (int c = 0; c < n_ch; c++) {
        const rd_bc_header h = hd[c];
        if (h.chunk != (uint32_t)chunk || h.n_clips > (uint32_t)RD_BC_PER || h.used > q)
            COLLECT_FAIL("clip header of channel %d belongs to chunk %u (%u clips, %u outputs), not %ld", c, h.chunk, h.n_clips, h.used, chunk);
        dropped[c] = h.dropped;
        const size_t base = bytes.size() / 2;   // outputs packed so far
        for (uint32_t i = 0; i < h.n_clips; i++) {
            rd_burst_clip k = recs[(size_t)c * RD_BC_PER + i];
            if ((size_t)k.offset + k.n > h.used) COLLECT_FAIL("clip %u of channel %d lies at %u + %u of %u outputs", i, c, k.offset, k.n, h.used);
            k.offset = (uint32_t)(base + k.offset);
            clips.push_back(k);
        }
        bytes.insert(bytes.end(), pool + (size_t)c * 2 * q, pool + (size_t)c * 2 * q + 2 * (size_t)h.used);
    }
    return RD_OK;
}

// ------------------------------------------------------------------------------------------
// the streaming demodulator's fetch (rd_host.h: rd_collect_block), a batch run's parsed messages (rd_order_parsed)
// ------------------------------------------------------------------------------------------
void rd_collect_block(const uint32_t *counts, size_t n_lists, size_t per, const rd_packet *recs, const int32_t *fe, int S,
                      rd_block_scratch &sc, std::vector<rd_packet> &last, std::vector<rd_parsed> &parsed) {
    sc.recs.clear();
    sc.fe.clear();
    for (size_t l = 0; l < n_lists; l++) {
        const size_t c = std::min<size_t>(counts[l], per);
        sc.recs.insert(sc.recs.end(), recs + l * per, recs + l * per + c);
        if (fe) sc.fe.insert(sc.fe.end(), fe + l * per, fe + l * per + c);
    }
    rd_order_and_dedupe(sc.recs.data(), sc.recs.size(), S, sc.order);
    last.clear();
    parsed.clear();
    for (uint32_t k : sc.order.kept) {
        const rd_packet &r = sc.recs[k];
        last.push_back(r);
        if (!fe || sc.fe[k] == RD_FE_NONE) continue;
        rd_parsed m;
        memset(&m, 0, sizeof m);
        m.stream = r.stream; m.call = r.call; m.index = r.index; m.freq_err = sc.fe[k];
        m.nbytes = r.nbytes - 2;
        for (int b = 2; b < r.nbytes && b < RD_MAX_PKT_BYTES; b++) m.data[b - 2] = (uint8_t)rd_swap_bits8(r.data[b]);
        m.id = m.data[0] & 7;
        m.rssi = r.rssi; m.snr = r.snr;
        parsed.push_back(m);
    }
}

size_t rd_order_parsed(rd_parsed *recs, size_t n, int S) {
    std::sort(recs, recs + n, [S](const rd_parsed &x, const rd_parsed &y) {
        if (x.stream != y.stream) return x.stream < y.stream;
        if (x.call != y.call) return x.call < y.call;
        const int px = x.index % S, py = y.index % S;
        if (px != py) return px < py;
        return x.index < y.index;
    });
    size_t kept = 0, group = 0;
    for (size_t i = 0; i < n; i++) {
        const rd_parsed &r = recs[i];
        if (kept == 0 || r.stream != recs[kept - 1].stream || r.call != recs[kept - 1].call) group = kept;
        bool dup = false;
        for (size_t k = group; k < kept && !dup; k++)
            dup = recs[k].nbytes == r.nbytes && memcmp(recs[k].data, r.data, sizeof r.data) == 0;
        if (!dup) recs[kept++] = r;
    }
    return kept;
}
