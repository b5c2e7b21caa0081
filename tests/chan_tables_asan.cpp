// chan_tables_asan.cpp - the host half of the channelizer's tables (rtldavis_amd/csrc/rd_chan_tables.cpp and the functions
// of rd_chan_tables.h it shares with k_chan_retune) under -fsanitize=address,undefined, driven by
// tests/test_chan_tables_sanitizers.py.  A stand-alone program:
//   chan_tables_asan tables    the builder against a forward model (window sample -> element) over a grid of shapes
//   chan_tables_asan retune    the host path of a retune: rebuilt channels equal a fresh build, the others are untouched
//   chan_tables_asan args      every rule of create and of the gain check on either side of its limit
//   chan_tables_asan split     the two-term f16 split in its float form against the direct double -> half form
// Model and product run in one process against one libm, so the comparisons are exact on any machine.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <vector>

#include "../rtldavis_amd/csrc/rd_chan_tables.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

// the library's rd_fail_msg lives in a HIP translation unit: this one keeps the text for the checks below
static char g_err[512];
int rd_fail_msg(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
static bool said(const char *part) { return strstr(g_err, part) != nullptr; }

static uint64_t g_rng;
static uint32_t rnd(void) {   // (a 64-bit LCG's upper half)
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 32);
}

// ---------------------------------------------------------------------------------------------------------------------
// The model: the tables as the definition states them, walked FORWARD - window sample -> tap -> fragment element - with a
// 128-bit product for the tap's phase and the direct double -> half conversions.
// ---------------------------------------------------------------------------------------------------------------------
static uint16_t f16_rn(double v) {  // round to nearest even f16 (|v| < 65504)
    const _Float16 h = (_Float16)v;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}
static double f16_val(uint16_t b) {
    _Float16 h;
    memcpy(&h, &b, 2);
    return (double)h;
}

struct model {
    int fmt, n_ch, T, t_pad, decim, n_q;
    int64_t out_rate;
    double tap_scale;
    float tap_unscale;
    std::vector<double> taps;
    std::vector<uint16_t> amat;
    std::vector<float> dc;
    std::vector<int64_t> shifts;
};

static void model_channel(model &m, int c, int64_t shift_hz) {
    const int fmt = m.fmt, T = m.T, t_pad = m.t_pad;
    const bool digits = fmt == RD_IQ_S16 || fmt == RD_IQ_CF32;
    const int kc = digits ? 4 : 8, n_q = m.n_q;
    const double wide_rate = (double)m.out_rate * m.decim;
    const double dc_level = fmt == RD_IQ_U8 ? 127.4 : fmt == RD_IQ_S8 ? 128.0 : 0.0;
    m.shifts[c] = ((shift_hz % m.out_rate) + m.out_rate) % m.out_rate;
    std::vector<double> gr(t_pad), gi(t_pad);
    for (int k = 0; k < t_pad; k++) {
        gr[k] = gi[k] = 0.0;
        if (k >= T) continue;
        const __int128 prod = (__int128)shift_hz * k;
        const long fw = (long)m.out_rate * m.decim;
        long r = (long)(prod % fw);
        if (r < 0) r += fw;
        const double ph = 2.0 * M_PI * ((double)r / wide_rate);
        gr[k] = (double)(float)(m.taps[k] * cos(ph));
        gi[k] = (double)(float)(m.taps[k] * sin(ph));
    }
    double sr = 0.0, si = 0.0;
    int kdone = 0;
    for (int t = 0; t <= 64; t++) {   // DC term: output t sees taps k <= D t (zero history before)
        const long kmax = t < 64 && fmt == RD_IQ_U8 ? (long)m.decim * t : (long)t_pad - 1;
        for (; kdone < t_pad && kdone <= kmax; kdone++) { sr += gr[kdone]; si += gi[kdone]; }
        m.dc[((size_t)c * 66 + t) * 2] = (float)(-dc_level * (sr - si));
        m.dc[((size_t)c * 66 + t) * 2 + 1] = (float)(-dc_level * (sr + si));
    }
    {
        const long inc = (long)(((__int128)m.shifts[c] * 32) % m.out_rate);
        const double ph = -2.0 * M_PI * ((double)inc / (double)m.out_rate);
        m.dc[((size_t)c * 66 + 65) * 2] = (float)cos(ph);
        m.dc[((size_t)c * 66 + 65) * 2 + 1] = (float)sin(ph);
    }
    const int grp = c / 64, rb = (c / 16) % 4, r0 = 2 * (c % 16);
    const int per_lane = kc / 2, n_dig = digits ? 2 : 1;
    for (int i = 0; i < kc * n_q; i++) {   // window sample i of a column <-> tap k = t_pad - i
        const int k = t_pad - i;
        if (k < 0 || k >= t_pad) continue;
        const int q = i / kc, hh = (i % kc) / per_lane, sl = i % per_lane;
        for (int part = 0; part < 2; part++)
            for (int comp = 0; comp < 2; comp++)
                for (int dig = 0; dig < n_dig; dig++) {
                    const double a = part == 0 ? (comp == 0 ? gr[k] : -gi[k]) : (comp == 0 ? gi[k] : gr[k]);
                    const double as = a * m.tap_scale * (fmt == RD_IQ_S16 && dig == 0 ? 1.0 / 256.0 : 1.0);
                    const uint16_t hi = f16_rn(as), lo = f16_rn(as - f16_val(hi));
                    const uint16_t term[2] = {hi, lo};
                    const int lane = 32 * hh + r0 + part;
                    const int el = digits ? 4 * sl + 2 * comp + dig : 4 * (sl / 2) + 2 * comp + (sl % 2);
                    for (int tm = 0; tm < 2; tm++)
                        m.amat[(((((size_t)grp * n_q + q) * 2 + tm) * 4 + rb) * 64 + lane) * 8 + el] = term[tm];
                }
    }
}

static model model_build(const rd_chan_config &cfg, int fmt, const std::vector<double> &taps, const std::vector<int64_t> &shift) {
    model m;
    const bool digits = fmt == RD_IQ_S16 || fmt == RD_IQ_CF32;
    m.fmt = fmt; m.n_ch = cfg.n_channels; m.T = cfg.n_taps; m.decim = cfg.decim; m.out_rate = cfg.out_rate;
    m.t_pad = (m.T + 7) / 8 * 8;
    m.n_q = m.t_pad / (digits ? 4 : 8) + 1;
    m.taps = taps;
    m.amat.assign((size_t)((m.n_ch + 63) / 64) * m.n_q * 4096, 0);   // (per K step: 2 terms x 4 row blocks x 64 lanes x 8)
    m.dc.assign((size_t)m.n_ch * 66 * 2, 0.0f);
    m.shifts.assign(m.n_ch, 0);
    double hmax = 0.0;
    for (double v : taps) hmax = fmax(hmax, fabs(v));
    int sexp = 0;
    if (hmax > 0.0) sexp = 14 - (int)ceil(log2(hmax));
    if (sexp > 60) sexp = 60;
    if (sexp < -60) sexp = -60;
    m.tap_scale = ldexp(1.0, sexp);
    m.tap_unscale = fmt == RD_IQ_CF32 ? (float)ldexp(1.0, -sexp - 12) : (float)ldexp(1.0, -sexp + 24 + (fmt == RD_IQ_S16 ? 8 : 0));
    for (int c = 0; c < m.n_ch; c++) model_channel(m, c, shift[c]);
    return m;
}

template <class V>
static bool same_bytes(const V &a, const V &b) {
    return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), a.size() * sizeof a[0]));
}

static const int FORMATS[4] = {RD_IQ_U8, RD_IQ_S8, RD_IQ_S16, RD_IQ_CF32};

static std::vector<double> some_taps(int n, int scale_log2) {
    std::vector<double> t(n);
    for (int k = 0; k < n; k++) t[k] = ldexp((double)(int32_t)rnd() / 2147483648.0, scale_log2) * (0.5 + 0.5 * cos(0.37 * k));
    return t;
}
// 0, +-1 Hz, +-Fw/2, a negative multiple of Fo, one beyond Fw, one far below -Fw; then anything inside +-Fw/2
static std::vector<int64_t> some_shifts(int n, int64_t fo, int64_t fw, int first) {
    const int64_t special[8] = {0, 1, -1, fw / 2, -(fw / 2), -3 * fo, fw + 12345, -2 * fw - 1};
    std::vector<int64_t> s(n);
    for (int c = 0; c < n; c++)
        s[c] = c < 8 ? special[(c + first) % 8] : (int64_t)(((uint64_t)rnd() << 16 | (rnd() & 0xFFFF)) % (uint64_t)fw) - fw / 2;
    return s;
}

static int test_tables(void) {
    long configs = 0, entries = 0;
    g_rng = 20240607;
    for (int fmt : FORMATS)
        for (int n_taps : {1, 8, 13, 64, 255})
            for (int decim : {4, 100})
                for (int n_ch : {1, 17, 65}) {
                    rd_chan_config cfg;
                    memset(&cfg, 0, sizeof cfg);
                    cfg.decim = decim; cfg.n_taps = n_taps; cfg.n_channels = n_ch;
                    cfg.out_rate = decim == 4 ? (1 << 26) - 1 : 268800;   // (Fw = 2^28 - 4: the largest products)
                    cfg.gain = 1.5;
                    const int64_t fw = (int64_t)cfg.out_rate * decim;
                    const std::vector<double> taps = some_taps(n_taps, (int)(configs % 9) * 16 - 72);   // |h| from 2^-72 to 2^56
                    const std::vector<int64_t> shift = some_shifts(n_ch, cfg.out_rate, fw, (int)configs);
                    rd_chan_tables t;
                    CHECK(rd_chan_tables_create(&t, &cfg, fmt, taps.data(), shift.data()) == RD_OK);
                    const model m = model_build(cfg, fmt, taps, shift);
                    CHECK(t.t_pad == m.t_pad && t.n_groups == (n_ch + 63) / 64);
                    CHECK(same_bytes(t.h_amat, m.amat));
                    CHECK(same_bytes(t.h_dc, m.dc));
                    CHECK(same_bytes(t.shifts, m.shifts));
                    CHECK(same_bytes(t.shift_hz, shift) && same_bytes(t.phase, std::vector<int64_t>(n_ch, 0)));
                    CHECK(t.tap_scale == m.tap_scale && t.tap_unscale == m.tap_unscale);
                    CHECK(same_bytes(t.gains, std::vector<float>(n_ch, 1.5f)) && same_bytes(t.taps, taps));
                    configs++;
                    entries += (long)t.h_amat.size();
                }
    printf("tables ok %ld configurations %ld entries\n", configs, entries);
    return 0;
}

static int test_retune(void) {
    g_rng = 77;
    long rebuilt = 0;
    for (int fmt : FORMATS)
        for (int n_ch : {17, 65}) {
            rd_chan_config cfg;
            memset(&cfg, 0, sizeof cfg);
            cfg.decim = 100; cfg.n_taps = 13; cfg.n_channels = n_ch; cfg.out_rate = 268800; cfg.gain = 2.0;
            const int64_t fo = cfg.out_rate, fw = fo * cfg.decim;
            const std::vector<double> taps = some_taps(cfg.n_taps, -3);
            std::vector<int64_t> shift = some_shifts(n_ch, fo, fw, 3);
            rd_chan_tables t;
            CHECK(rd_chan_tables_create(&t, &cfg, fmt, taps.data(), shift.data()) == RD_OK);
            const rd_chan_tables before = t;
            std::vector<int64_t> phase(n_ch, 0);
            std::vector<char> hit(n_ch, 0);
            for (int c : {0, 5, 16, n_ch - 1}) {
                shift[c] = c == 5 ? fw + 99 : (int64_t)(rnd() % (uint32_t)fo) - fo / 2;
                phase[c] = (int64_t)(rnd() % (uint32_t)fo);
                hit[c] = 1;
                rd_chan_tables_build(&t, c, shift[c], phase[c]);
                rebuilt++;
            }
            rd_chan_tables fresh;
            CHECK(rd_chan_tables_create(&fresh, &cfg, fmt, taps.data(), shift.data()) == RD_OK);
            CHECK(same_bytes(t.h_amat, fresh.h_amat) && same_bytes(t.h_dc, fresh.h_dc) && same_bytes(t.shifts, fresh.shifts));
            CHECK(same_bytes(t.shift_hz, shift) && same_bytes(t.phase, phase));
            // the channels that were not named: byte for byte what they were.  Entry `at` of the A operand belongs to channel
            // 64 group + 16 row block + (lane mod 32) / 2
            const size_t n_q = (size_t)t.t_pad / (fmt == RD_IQ_S16 || fmt == RD_IQ_CF32 ? 4 : 8) + 1;
            long changed = 0;
            for (size_t at = 0; at < t.h_amat.size(); at++) {
                const size_t lane = (at / 8) % 64, rb = (at / 8 / 64) % 4, grp = at / 8 / 64 / 4 / 2 / n_q;
                const size_t c = 64 * grp + 16 * rb + (lane % 32) / 2;
                if (c >= (size_t)n_ch || !hit[c]) CHECK(t.h_amat[at] == before.h_amat[at]);
                else changed += t.h_amat[at] != before.h_amat[at];
            }
            CHECK(changed > 0);
            for (int c = 0; c < n_ch; c++) {
                if (hit[c]) continue;
                CHECK(!memcmp(&t.h_dc[(size_t)c * RD_CHAN_DCN * 2], &before.h_dc[(size_t)c * RD_CHAN_DCN * 2], RD_CHAN_DCN * 2 * sizeof(float)));
                CHECK(t.shifts[c] == before.shifts[c] && t.shift_hz[c] == before.shift_hz[c] && t.phase[c] == 0);
            }
            CHECK(same_bytes(t.taps, before.taps) && same_bytes(t.gains, before.gains) && t.tap_scale == before.tap_scale);
        }
    printf("retune ok %ld channels rebuilt\n", rebuilt);
    return 0;
}

static int create(int fmt, int decim, int n_taps, int n_ch, int64_t out_rate, double gain) {
    rd_chan_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.decim = decim; cfg.n_taps = n_taps; cfg.n_channels = n_ch; cfg.out_rate = out_rate; cfg.gain = gain;
    // (taps and shifts in heap blocks of exactly their size)
    const std::vector<double> taps(n_taps > 0 && n_taps <= 8193 ? n_taps : 1, 0.001);
    const std::vector<int64_t> shift(n_ch > 0 && n_ch <= 4097 ? n_ch : 1, 1000);
    rd_chan_tables t;
    g_err[0] = 0;
    return rd_chan_tables_create(&t, &cfg, fmt, taps.data(), shift.data());
}

static int test_args(void) {
    const char *range = "channelizer config out of range (decim: a multiple of 4)";
    const int64_t fo = 268800;
    CHECK(create(RD_IQ_U8, 100, 8, 2, fo, 1.0) == RD_OK);
    {   // null arguments
        rd_chan_config cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.decim = 100; cfg.n_taps = 1; cfg.n_channels = 1; cfg.out_rate = fo; cfg.gain = 1.0;
        const double tap = 1.0;
        const int64_t sh = 0;
        rd_chan_tables t;
        CHECK(rd_chan_tables_create(nullptr, &cfg, RD_IQ_U8, &tap, &sh) == RD_ERR_ARG && said("null argument"));
        CHECK(rd_chan_tables_create(&t, nullptr, RD_IQ_U8, &tap, &sh) == RD_ERR_ARG && said("null argument"));
        CHECK(rd_chan_tables_create(&t, &cfg, RD_IQ_U8, nullptr, &sh) == RD_ERR_ARG && said("null argument"));
        CHECK(rd_chan_tables_create(&t, &cfg, RD_IQ_U8, &tap, nullptr) == RD_ERR_ARG && said("null argument"));
        CHECK(rd_chan_tables_create(&t, &cfg, RD_IQ_U8, &tap, &sh) == RD_OK);
    }
    // decim: 0 / 4 / 98 / 4096 / 4100 (4096 passes the range rule and then meets the LDS rule)
    CHECK(create(RD_IQ_U8, 0, 8, 2, fo, 1.0) == RD_ERR_ARG && said(range));
    CHECK(create(RD_IQ_U8, 4, 8, 2, fo, 1.0) == RD_OK);
    CHECK(create(RD_IQ_U8, 98, 8, 2, fo, 1.0) == RD_ERR_ARG && said(range));
    CHECK(create(RD_IQ_U8, 4096, 8, 2, fo, 1.0) == RD_ERR_ARG && said("do not fit the 160 KiB LDS"));
    CHECK(create(RD_IQ_U8, 4100, 8, 2, fo, 1.0) == RD_ERR_ARG && said(range));
    CHECK(create(RD_IQ_U8, -4, 8, 2, fo, 1.0) == RD_ERR_ARG && said(range));
    // taps: 0 / 1 / 8192 / 8193
    CHECK(create(RD_IQ_U8, 128, 0, 2, fo, 1.0) == RD_ERR_ARG && said(range));
    CHECK(create(RD_IQ_U8, 128, 1, 2, fo, 1.0) == RD_OK);
    CHECK(create(RD_IQ_U8, 128, 8192, 2, fo, 1.0) == RD_OK);
    CHECK(create(RD_IQ_U8, 128, 8193, 2, fo, 1.0) == RD_ERR_ARG && said(range));
    // channels: 0 / 4096 / 4097
    CHECK(create(RD_IQ_U8, 100, 8, 0, fo, 1.0) == RD_ERR_ARG && said(range));
    CHECK(create(RD_IQ_U8, 100, 8, 4096, fo, 1.0) == RD_OK);
    CHECK(create(RD_IQ_U8, 100, 8, 4097, fo, 1.0) == RD_ERR_ARG && said(range));
    // out_rate: 0, 1, 2^26 - 1, 2^26
    CHECK(create(RD_IQ_U8, 100, 8, 2, 0, 1.0) == RD_ERR_ARG && said(range));
    CHECK(create(RD_IQ_U8, 100, 8, 2, 1, 1.0) == RD_OK);
    CHECK(create(RD_IQ_U8, 100, 8, 2, (1 << 26) - 1, 1.0) == RD_OK);
    CHECK(create(RD_IQ_U8, 100, 8, 2, 1 << 26, 1.0) == RD_ERR_ARG && said(range));
    // gain: 0, negative, NaN
    CHECK(create(RD_IQ_U8, 100, 8, 2, fo, 0.0) == RD_ERR_ARG && said(range));
    CHECK(create(RD_IQ_U8, 100, 8, 2, fo, -1.0) == RD_ERR_ARG && said(range));
    CHECK(create(RD_IQ_U8, 100, 8, 2, fo, std::numeric_limits<double>::quiet_NaN()) == RD_ERR_ARG && said(range));
    // the LDS limit per format: bytes per staged sample x (127 decim + 8 taps + one K step) + 16 <= 160 KiB
    for (int fmt : FORMATS) {
        const bool digits = fmt == RD_IQ_S16 || fmt == RD_IQ_CF32;
        const int bps = digits ? 8 : 2, kc = digits ? 4 : 8;
        int fits = 0;
        for (int d = 4; d <= 4096; d += 4)
            if ((long)bps * (127L * d + 8 + kc) + 16 <= 160L * 1024) fits = d;
        CHECK(fits == (digits ? 160 : 644));
        CHECK(create(fmt, fits, 8, 2, fo, 1.0) == RD_OK);
        CHECK(create(fmt, fits + 4, 8, 2, fo, 1.0) == RD_ERR_ARG && said("do not fit the 160 KiB LDS") && said(digits ? "of 8 bytes" : "of 2 bytes"));
    }
    // n_taps / decim: the 8-bit formats keep 64 early DC terms, the digit formats none
    for (int fmt : FORMATS) {
        const bool digits = fmt == RD_IQ_S16 || fmt == RD_IQ_CF32;
        CHECK(create(fmt, 4, 256, 2, fo, 1.0) == RD_OK);
        if (digits) CHECK(create(fmt, 4, 257, 2, fo, 1.0) == RD_OK);
        else CHECK(create(fmt, 4, 257, 2, fo, 1.0) == RD_ERR_ARG && said("n_taps / decim too large"));
    }
    // an unknown format
    CHECK(create(3, 100, 8, 2, fo, 1.0) == RD_ERR_ARG && said("unknown sample format 3"));
    CHECK(create(-1, 100, 8, 2, fo, 1.0) == RD_ERR_ARG && said("unknown sample format -1"));
    CHECK(create(5, 100, 8, 2, fo, 1.0) == RD_ERR_ARG && said("unknown sample format 5"));

    // the gain check
    rd_chan_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.decim = 100; cfg.n_taps = 8; cfg.n_channels = 3; cfg.out_rate = fo; cfg.gain = 1.0;
    const std::vector<double> taps(8, 0.01);
    const std::vector<int64_t> shift(3, 0);
    rd_chan_tables t;
    CHECK(rd_chan_tables_create(&t, &cfg, RD_IQ_S8, taps.data(), shift.data()) == RD_OK);
    auto gains = [&](std::vector<double> g) { g_err[0] = 0; return rd_chan_tables_check_gains(&t, g.data(), (int)g.size()); };
    const double inf = std::numeric_limits<double>::infinity();
    CHECK(gains({1.0, 2.0, 1e-30}) == RD_OK);
    CHECK(gains({1.0, 2.0}) == RD_ERR_ARG && said("Incompatible array sizes: 2 gains for 3 channels"));
    CHECK(gains({1.0, 2.0, 3.0, 4.0}) == RD_ERR_ARG && said("Incompatible array sizes: 4 gains for 3 channels"));
    CHECK(gains({1.0, 0.0, 1.0}) == RD_ERR_ARG && said("channel 1: a gain must be finite and > 0"));
    CHECK(gains({-1.0, 1.0, 1.0}) == RD_ERR_ARG && said("channel 0: a gain must be finite and > 0"));
    CHECK(gains({1.0, 1.0, inf}) == RD_ERR_ARG && said("channel 2: a gain must be finite and > 0"));
    CHECK(gains({1.0, 1.0, std::numeric_limits<double>::quiet_NaN()}) == RD_ERR_ARG && said("channel 2"));
    CHECK(gains({1.0, 1e-50, 1.0}) == RD_ERR_ARG && said("channel 1: a gain must be finite and > 0 (in float32 too)"));   // 0 as float32
    CHECK(gains({1e39, 1.0, 1.0}) == RD_ERR_ARG && said("channel 0: a gain must be finite and > 0 (in float32 too)"));    // Inf as float32
    CHECK(gains({3.0e38, 1.5e-45, 1.0}) == RD_OK);                                                                        // the ends of float32
    const double one = 1.0;
    CHECK(rd_chan_tables_check_gains(nullptr, &one, 1) == RD_ERR_ARG && said("null argument"));
    CHECK(rd_chan_tables_check_gains(&t, nullptr, 3) == RD_ERR_ARG && said("null argument"));
    printf("args ok\n");
    return 0;
}

// hi = f16((float)as), lo = f16((float)(as - hi)) (rd_chan_fragment) against hi = f16(as), lo = f16(as - hi) in float64: as = an
// fp32 value times the tap scale 2^s, every s the builder can choose, |as| < 2^15 as the scale guarantees
static int test_split(void) {
    g_rng = 4711;
    long n = 0, diff = 0;
    for (int s = -60; s <= 60; s++)
        for (int i = 0; i < 8000; i++) {
            const uint32_t r = rnd();
            const int e = (int)(rnd() % 60) - 45;                                  // |as| in [2^-45, 2^15)
            const float mant = 1.0f + (float)(r & 0x7FFFFF) / 8388608.0f;           // 24 significant bits
            const float a = ldexpf((r >> 31) ? -mant : mant, e - s);                // (normal in fp32: e - s in -105 .. 74)
            for (double digit : {1.0, 1.0 / 256.0}) {
                const double as = (double)a * ldexp(1.0, s) * digit;
                const _Float16 hi = (_Float16)(float)as;
                const _Float16 lo = (_Float16)(float)(as - (double)hi);
                const uint16_t hi_d = f16_rn(as), lo_d = f16_rn(as - f16_val(hi_d));
                uint16_t hi_f, lo_f;
                memcpy(&hi_f, &hi, 2);
                memcpy(&lo_f, &lo, 2);
                diff += hi_f != hi_d || lo_f != lo_d;
                n++;
            }
        }
    printf("split ok %ld values %ld differences\n", n, diff);
    return diff ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !strcmp(argv[1], "tables")) return test_tables();
    if (argc == 2 && !strcmp(argv[1], "retune")) return test_retune();
    if (argc == 2 && !strcmp(argv[1], "args")) return test_args();
    if (argc == 2 && !strcmp(argv[1], "split")) return test_split();
    fprintf(stderr, "usage: chan_tables_asan tables|retune|args|split\n");
    return 2;
}
