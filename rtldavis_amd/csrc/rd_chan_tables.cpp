// rd_chan_tables.cpp - the host half of the channelizer's tables (rd_chan_tables.h): the argument rules of create, one
// channel's tables, the gain check.  Pure host code, no HIP: compiled into librtldavis_hip.so by the Makefile as rd_host.cpp
// is, and into tests/chan_tables_asan under -fsanitize=address,undefined (tests/test_chan_tables_sanitizers.py).
#include "rd_chan_tables.h"

#include <string.h>

#include <algorithm>
#include <cmath>

void rd_chan_tables_build(rd_chan_tables *t, int c, int64_t shift_hz, int64_t phase) {
    const rd_chan_config *cfg = &t->cfg;
    const int fmt = t->fmt, T = cfg->n_taps, t_pad = t->t_pad, n_q = t_pad / rd_fmt_kc(fmt) + 1;
    const int64_t fo = cfg->out_rate, fw = fo * cfg->decim;
    t->shift_hz[c] = shift_hz;
    t->phase[c] = phase;
    t->shifts[c] = rd_chan_shift_mod(shift_hz, fo);
    std::vector<rd_chan_g> g(t_pad, rd_chan_g{0.0f, 0.0f});
    for (int k = 0; k < T; k++) g[k] = rd_chan_tap(t->taps[k], shift_hz, k, fw);
    float *dc = &t->h_dc[(size_t)c * RD_CHAN_DCN * 2];
    rd_chan_dc_entries(fmt, g.data(), t_pad, cfg->decim, dc);
    rd_chan_rotation(t->shifts[c], fo, dc + 2 * (RD_CHAN_EARLY + 1));
    for (int it = 0; it < 8 * n_q; it++) {   // one fragment per item, as k_chan_retune's threads take them
        const int part = it & 1, hh = (it >> 1) & 1, tm = (it >> 2) & 1, q = it >> 3;
        uint32_t w[4];
        rd_chan_fragment(fmt, g.data(), t_pad, t->tap_scale, q, tm, hh, part, w);
        memcpy(&t->h_amat[8 * rd_chan_amat_index(c, n_q, q, tm, hh, part)], w, sizeof w);
    }
}

int rd_chan_tables_create(rd_chan_tables *t, const rd_chan_config *cfg, int fmt, const double *taps, const int64_t *shift_hz) {
    if (!t || !cfg || !taps || !shift_hz) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (fmt != RD_IQ_U8 && fmt != RD_IQ_S8 && fmt != RD_IQ_S16 && fmt != RD_IQ_CF32) return rd_fail_msg(RD_ERR_ARG, "unknown sample format %d", fmt);
    if (cfg->decim < 4 || cfg->decim > 4096 || cfg->decim % 4 || cfg->n_taps < 1 || cfg->n_taps > 8192 ||
        cfg->n_channels < 1 || cfg->n_channels > 4096 || cfg->out_rate < 1 || cfg->out_rate >= (1 << 26) ||
        !(cfg->gain > 0.0))
        return rd_fail_msg(RD_ERR_ARG, "channelizer config out of range (decim: a multiple of 4)");
    const int t_pad = (cfg->n_taps + RD_CHAN_KC - 1) / RD_CHAN_KC * RD_CHAN_KC;
    if (rd_fmt_lds_bps(fmt) * rd_chan_span(fmt, cfg->decim, t_pad) + 16 > 160 * 1024)
        return rd_fail_msg(RD_ERR_ARG, "decim x 127 + n_taps samples of %d bytes do not fit the 160 KiB LDS", rd_fmt_lds_bps(fmt));
    // (RD_IQ_S16 and RD_IQ_CF32 have no DC term, hence no table of early ones and no limit from it)
    const int n_early = rd_fmt_digits(fmt) ? 0 : (t_pad - 1 + cfg->decim - 1) / cfg->decim;
    if (n_early > RD_CHAN_EARLY) return rd_fail_msg(RD_ERR_ARG, "n_taps / decim too large");
    t->cfg = *cfg;
    t->fmt = fmt;
    const int T = cfg->n_taps;
    t->t_pad = t_pad;
    t->n_early = n_early;
    t->n_groups = (cfg->n_channels + 16 * RD_CHAN_RBG - 1) / (16 * RD_CHAN_RBG);
    const int n_q = t_pad / rd_fmt_kc(fmt) + 1;  // the window starts one sample early (aligned): one more K step
    t->h_amat.assign((size_t)t->n_groups * n_q * (RD_CHAN_Q_BYTES / 2), 0);
    t->h_dc.assign((size_t)cfg->n_channels * RD_CHAN_DCN * 2, 0.0f);
    t->shifts.resize(cfg->n_channels);
    t->shift_hz.resize(cfg->n_channels);
    t->phase.resize(cfg->n_channels);
    t->gains.assign(cfg->n_channels, (float)cfg->gain);
    t->taps.assign(taps, taps + T);
    // every |g_c[k]| <= max |h[k]|: scale the taps by the power of two that brings that just below 2^15 (f16: 11
    // significant bits from 2^-14 up), the kernel multiplies the sums back
    double hmax = 0.0;
    for (int k = 0; k < T; k++) hmax = std::max(hmax, std::fabs(taps[k]));
    int sexp = 0;
    if (hmax > 0.0) sexp = 14 - (int)std::ceil(std::log2(hmax));
    if (sexp > 60) sexp = 60;
    if (sexp < -60) sexp = -60;
    t->tap_scale = std::ldexp(1.0, sexp);
    // (+24: the samples enter as k 2^-24; RD_IQ_S16: the low digit's taps carry 2^-8 more, so that the high digit's
    // factor 256 stays inside f16; RD_IQ_CF32: the samples enter as 2^12 x, real f16 values, not raw patterns)
    t->tap_unscale = fmt == RD_IQ_CF32 ? (float)std::ldexp(1.0, -sexp - RD_CF32_PRESCALE_LOG2)
                                       : (float)std::ldexp(1.0, -sexp + 24 + (fmt == RD_IQ_S16 ? 8 : 0));
    for (int c = 0; c < cfg->n_channels; c++) rd_chan_tables_build(t, c, shift_hz[c], 0);
    return RD_OK;
}

int rd_chan_tables_check_gains(const rd_chan_tables *t, const double *gain, int n) {
    if (!t || !gain) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (n != t->cfg.n_channels) return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: %d gains for %d channels", n, t->cfg.n_channels);
    for (int c = 0; c < n; c++)
        if (!(gain[c] > 0.0) || !std::isfinite(gain[c]) || !((float)gain[c] > 0.0f) || !std::isfinite((float)gain[c]))
            return rd_fail_msg(RD_ERR_ARG, "channel %d: a gain must be finite and > 0 (in float32 too)", c);
    return RD_OK;
}
