// rd_chan_tables.h - the tables k_channelize reads (rd_channelizer.hip: the definition and the GEMM mapping), defined once:
// the host builds them at create (rd_chan_tables.cpp: pure host, also compiled into tests/chan_tables_asan under
// -fsanitize=address,undefined), the device rebuilds a retuned channel's in place (k_chan_retune), both through the inline
// functions below, each side with its own libm.  No HIP include.  Per channel c, from the float64 prototype h[k], k < T
// (zero taps appended up to t_pad, a multiple of RD_CHAN_KC), the shift in Hz, Fo = out_rate and Fw = Fo decim:
//   taps      g_c[k] = h[k] e^{+j 2 pi shift k / Fw} rounded to fp32: the definition's taps on the device (rd_chan_tap)
//   A operand rows 2c (re) and 2c+1 (im); kappa = 2 i + comp, window sample i <-> tap k = t_pad - i (the window starts one
//             sample early, at D t - t_pad, aligned: one more K step, n_q = t_pad / kc + 1).  The taps times tap_scale = 2^s
//             as two f16 terms hi + lo, in fragment order [group][K step][term][row block][lane][8] (rd_chan_fragment,
//             rd_chan_amat_index).  RD_IQ_S16: kappa = 4 i + 2 comp + digit, a lane holds two samples (Ilo Ihi Qlo Qhi
//             each); the low digit's taps are scaled by 2^-8 against the high digit's.  RD_IQ_CF32: the same layout, both
//             digits against the same tap.
//   DC        entry t < RD_CHAN_EARLY: output t sees taps k <= D t (zero history before); entry RD_CHAN_EARLY: all of them.
//             lut(b) = (b - 127.4) / 127.6 and the kernel sums g b: the constant is -127.4 (1 + j)(sr + j si) - 128 for the
//             offset-binary bytes of RD_IQ_S8, which stages 0x80 = the value 0 before the capture, so every output sees all
//             the taps; nothing for the digit formats (rd_chan_dc_entries).  Entry RD_CHAN_EARLY + 1: rd_chan_rotation.
//   shifts    shift mod Fo in [0, Fo): all the output phasor needs (rd_chan_shift_mod)
// The f16 split is hi = f16((float)as), lo = f16((float)(as - hi)) on both sides: as = a 2^s, an fp32 tap times a power of
// two, is an fp32 number and so is what the first digit leaves of it (at most 13 significant bits), so both digits are one
// rounding each, float -> half, and equal the direct double -> half conversions the host used to make (13.5 M random
// values over every tap scale: no difference; tests/chan_tables_asan.cpp `split` keeps checking it).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/rtldavis_hip.h"
#include "rd_host.h"   // RD_HOST_DEVICE

#define RD_CHAN_TB 4                        // 32-time blocks per wave
#define RD_CHAN_TT (32 * RD_CHAN_TB)        // output times per workgroup
#define RD_CHAN_RBG 4                       // row blocks (32 rows = 16 channels) per workgroup: one per wave
#define RD_CHAN_KC 8                        // window samples per K step of the 8-bit formats (taps are padded to a multiple)
#define RD_CHAN_TERMS 2                     // f16 digits per tap
#define RD_CHAN_Q_BYTES (RD_CHAN_TERMS * RD_CHAN_RBG * 64 * 16)  // A bytes per K step: terms x 4 row blocks x 64 lanes x 16 B
#define RD_CHAN_EARLY 64                    // outputs per channel with a partial-history DC term kept in a table
#define RD_CHAN_DCN (RD_CHAN_EARLY + 2)     // table entries per channel: the early DC terms, the steady one, and the
                                            // phasor of 32 output times e^{-j 2 pi frac(32 shift / Fo)} (cos, sin)

// per sample format (rtldavis_hip.h: RD_IQ_*): bytes of an IQ pair in memory and staged in LDS, window samples per K step
RD_HOST_DEVICE constexpr int rd_fmt_in_bps(int f) { return f == RD_IQ_CF32 ? 8 : f == RD_IQ_S16 ? 4 : 2; }
RD_HOST_DEVICE constexpr int rd_fmt_lds_bps(int f) { return f == RD_IQ_S16 || f == RD_IQ_CF32 ? 8 : 2; }
RD_HOST_DEVICE constexpr int rd_fmt_kc(int f) { return f == RD_IQ_S16 || f == RD_IQ_CF32 ? RD_CHAN_KC / 2 : RD_CHAN_KC; }
// two 16-bit digits per component (four lanes per staged sample): the formats whose B fragment is one ds_read_b128
RD_HOST_DEVICE constexpr bool rd_fmt_digits(int f) { return f == RD_IQ_S16 || f == RD_IQ_CF32; }
// the level the DC term removes: the LUT's 127.4, 128 for the offset-binary bytes of RD_IQ_S8, none for signed digits
RD_HOST_DEVICE constexpr double rd_fmt_dc_level(int f) { return rd_fmt_digits(f) ? 0.0 : f == RD_IQ_U8 ? 127.4 : 128.0; }
// RD_CF32_CLAMP (adm: |v| <= 8) and rd_chan_adm: rd_internal.h (k_chan_spectrum admits float32 components the same way)
#define RD_CF32_PRESCALE_LOG2 12            // staged s = 2^12 adm(v), |s| <= 2^15 < 65504

// The window a workgroup stages: samples, and LDS bytes (a multiple of 16, one spare vector)
RD_HOST_DEVICE constexpr size_t rd_chan_span(int fmt, int decim, int t_pad) { return (size_t)(RD_CHAN_TT - 1) * decim + t_pad + rd_fmt_kc(fmt); }
RD_HOST_DEVICE constexpr size_t rd_chan_lds_bytes(int fmt, int decim, int t_pad) {
    return (rd_fmt_lds_bps(fmt) * rd_chan_span(fmt, decim, t_pad) + 15 + 16) & ~(size_t)15;
}

struct alignas(8) rd_chan_g { float r, i; };   // an fp32 tap (g_r, g_i); the device keeps a channel's in LDS as float2
RD_HOST_DEVICE static inline int64_t rd_chan_shift_mod(int64_t shift, int64_t fo) { return ((shift % fo) + fo) % fo; }

// g_c[k] = h[k] e^{+j 2 pi shift k / Fw}; the phase through an exact integer remainder: the shift reduced into [0, Fw)
// first, then (shift_mod k) mod Fw - Fw < 2^38 and k < 2^13, the product stays below 2^51 whatever the shift.
RD_HOST_DEVICE static inline rd_chan_g rd_chan_tap(double h, int64_t shift, int k, int64_t fw) {
    const int64_t r = (rd_chan_shift_mod(shift, fw) * k) % fw;
    const double ph = 2.0 * M_PI * ((double)r / (double)fw);
    return rd_chan_g{(float)(h * cos(ph)), (float)(h * sin(ph))};
}

// The channel's RD_CHAN_EARLY + 1 DC entries (re, im) from its taps g[k < t_pad]: float64 sums, in ascending k
RD_HOST_DEVICE static inline void rd_chan_dc_entries(int fmt, const rd_chan_g *g, int t_pad, int D, float *dc) {
    const double dc_level = rd_fmt_dc_level(fmt);
    double sr = 0.0, si = 0.0;
    int kdone = 0;
    for (int t = 0; t <= RD_CHAN_EARLY; t++) {
        const long kmax = t < RD_CHAN_EARLY && fmt == RD_IQ_U8 ? (long)D * t : (long)t_pad - 1;
        for (; kdone < t_pad && kdone <= kmax; kdone++) { sr += (double)g[kdone].r; si += (double)g[kdone].i; }
        dc[2 * t] = (float)(-dc_level * (sr - si));
        dc[2 * t + 1] = (float)(-dc_level * (sr + si));
    }
}

// The rotation by 32 output times (cos, sin) from shift mod Fo < Fo < 2^26 (exact remainder, float64 sin / cos)
RD_HOST_DEVICE static inline void rd_chan_rotation(int64_t smod, int64_t fo, float *cs) {
    const int64_t inc = (smod * 32) % fo;
    const double ph = -2.0 * M_PI * ((double)inc / (double)fo);
    cs[0] = (float)cos(ph), cs[1] = (float)sin(ph);
}

// One A fragment, 8 f16 = four dwords w: K step q, term tm (0 = hi, 1 = lo), lane half hh, part (0 = re, 1 = im).  Its
// elements are, in the kernel's B fragment order, (I0 I1 Q0 Q1 | I2 I3 Q2 Q3) of the lane's four window samples, or
// (Ilo Ihi Qlo Qhi) x 2 of its two (int16, cf32: two digits per component; int16's low one meets taps scaled 2^-8).
RD_HOST_DEVICE static inline void rd_chan_fragment(int fmt, const rd_chan_g *g, int t_pad, double tap_scale, int q, int tm, int hh,
                                                   int part, uint32_t w[4]) {
    const int kc = rd_fmt_kc(fmt), per_lane = kc / 2;
    const bool two = rd_fmt_digits(fmt);
    w[0] = w[1] = w[2] = w[3] = 0u;
#pragma unroll
    for (int el = 0; el < 8; el++) {
        const int comp = (el >> 1) & 1;
        const int sl = two ? el >> 2 : 2 * (el >> 2) + (el & 1), dig = two ? el & 1 : 1;
        const int k = t_pad - (q * kc + hh * per_lane + sl);
        if (k < 0 || k >= t_pad) continue;
        const rd_chan_g gk = g[k];
        const double a = part == 0 ? (comp == 0 ? (double)gk.r : -(double)gk.i) : (comp == 0 ? (double)gk.i : (double)gk.r);
        const double as = a * tap_scale * (fmt == RD_IQ_S16 && dig == 0 ? 1.0 / 256.0 : 1.0);
        const _Float16 hi = (_Float16)(float)as;
        const _Float16 lo = (_Float16)(float)(as - (double)hi);
        const uint32_t bits = (uint32_t)__builtin_bit_cast(uint16_t, tm == 0 ? hi : lo);
        w[el >> 1] |= bits << (16 * (el & 1));
    }
}

// Where that fragment lies in amat, in fragments of 16 bytes: [group][K step][term][row block][lane], the lane holding
// rows 2c, 2c+1 of its row block in its two halves' registers
RD_HOST_DEVICE static inline size_t rd_chan_amat_index(int c, int n_q, int q, int tm, int hh, int part) {
    const int grp = c / (16 * RD_CHAN_RBG), rb = (c / 16) % RD_CHAN_RBG, lane = 32 * hh + 2 * (c % 16) + part;
    return ((((size_t)grp * n_q + q) * RD_CHAN_TERMS + tm) * RD_CHAN_RBG + rb) * 64 + lane;
}

// The host's state of a channelizer handle (rd_channelizer.hip: rd_chan adds the device pointers)
struct rd_chan_tables {
    rd_chan_config cfg;
    int fmt = RD_IQ_U8;            // sample format of the capture
    int n_groups = 0;              // groups of 64 channels
    int t_pad = 0;                 // taps rounded up to RD_CHAN_KC (zero taps appended)
    int n_early = 0;               // outputs whose window reaches before the capture: ceil((t_pad - 1) / D)
    float tap_unscale = 1.0f;      // 2^-s: the taps in h_amat are scaled by 2^s
    double tap_scale = 1.0;        // 2^s
    std::vector<uint16_t> h_amat;  // f16 A operand in fragment order [group][K step][term][row block][lane][8]
    std::vector<float> h_dc;       // [channel][RD_CHAN_DCN][2]: -127.4 (1+j) sum of the taps a given output sees; the 32-step phasor
    std::vector<int64_t> shifts;   // Hz, reduced mod out_rate
    // the tuning the tables hold (rd_chan_retune): the shifts as given, and the phase accumulators P_c in [0, out_rate)
    std::vector<int64_t> shift_hz, phase;
    std::vector<double> taps;      // the float64 prototype (a retune rebuilds a channel's tables from it)
    std::vector<float> gains;      // GAIN: the per-channel gains the table holds (float32, (float)cfg.gain each at create)
};

int rd_fail_msg(int code, const char *fmt, ...);   // (rd_hiphost.h; host code)
// The argument rules of rd_chan_create_fmt and every table of every channel at phase 0; touches no device.
int rd_chan_tables_create(rd_chan_tables *t, const rd_chan_config *cfg, int fmt, const double *taps, const int64_t *shift_hz);
// The tables of channel c for the shift `shift_hz` (Hz, as given) and the phase accumulator `phase` (rd_channelizer.hip:
// RETUNE; 0 at create).  On the host - create for every channel, rd_chan_retune for a channel retuned before the device
// tables exist; k_chan_retune is the same on the device.
void rd_chan_tables_build(rd_chan_tables *t, int c, int64_t shift_hz, int64_t phase);
// GAIN: n = n_channels gains, every one finite and > 0 (the rule of cfg.gain), as the float32 values the table takes
int rd_chan_tables_check_gains(const rd_chan_tables *t, const double *gain, int n);
