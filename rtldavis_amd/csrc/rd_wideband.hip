// rd_wideband.hip - live wideband receiver (include/rtldavis_hip.h: rd_wideband_*): a capture that never ends, fed in
// chunks of decim x block_size samples (uint8, int8, int16 or float32 IQ: rd_wb_create_fmt), channelized into every hop channel and demodulated, all on the GPU.
//
// One handle owns one rd_chan configuration and one multi-stream rd_demod (n_streams = n_channels).  Per chunk, queued by
// rd_wideband_submit and returning at once:
//   copy stream:    pinned slot -> device chunk buffer (overlaps the previous chunk's kernels)
//   compute stream: k_channelize<true> (streaming form: the previous chunk's buffer is the history, the output clock is
//                   absolute) into a channelized buffer [n_channels][2 block_size], then the demodulator's one launch
//                   reading that buffer where it lies (rd_demod_submit_device)
// Two chunk buffers and two channelized buffers, indexed by the chunk's parity: chunk k reads chunk k-1's buffer as its
// history, so the copy of chunk k+1 into that buffer waits for chunk k's channelizer (an event); chunk k's channelized
// bytes stay valid until chunk k+2 is submitted.  At most two chunks are in flight (the demodulator's two slots).
// The output clock is a 64-bit count kept here; the kernel gets it mod out_rate, so the mixer phase stays exact however
// long the receiver runs.  A fetch that times out loses the chunk's packets, not the clock or the history: both advance
// at submit.
// Every per-chunk feature (levels, spectrum, bursts, decode, quality, expect, search, clips) is one stage, wb_queue_*: a
// kernel behind the chunk's channelizer and in front of its demodulator launch on the compute stream, writing a mapped
// pinned slot of the chunk's parity (wb_slots) that the fetch reads once that launch has reported (wb_fetched).  The
// argument that its slot is free and its inputs are ordered stands with each stage.
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "rd_internal.h"

// A pair of mapped pinned slots, one per chunk parity: a stage's kernel writes slot s through d[s], the fetch reads h[s].
// [fill, fill + fill_len) is the part that must never pass for a chunk's: 0xFF at allocation and after reset(), a
// sequence number or count no chunk can have.
struct wb_slots {
    uint8_t *h[2] = {nullptr, nullptr};
    uint8_t *d[2] = {nullptr, nullptr};   // the device's address of h[i], taken once
    size_t bytes = 0, fill = 0, fill_len = 0;
};
enum { WB_LV, WB_SP, WB_BU, WB_BD, WB_BX, WB_BQ, WB_BS, WB_BC, WB_SLOT_KINDS };

// Slots of at least `bytes`: allocated when first wanted, remade when a setting has grown them (the spectrum's n_bins, the
// clips' quota: the receiver was quiet when it changed, so nothing reads or writes the old ones).  The fill region of a
// remade slot is the old one's - the clip headers are what the last chunk owes the next.
static int wb_slots_ensure(wb_slots &p, size_t bytes, size_t fill, size_t fill_len) {
    if (p.h[0] && bytes <= p.bytes) return RD_OK;
    uint8_t *h[2] = {nullptr, nullptr}, *d[2] = {nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; i++) {
        e = hipHostMalloc((void **)&h[i], bytes, hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&d[i], h[i], 0);
    }
    if (e != hipSuccess) {               // (both or neither: the pair keeps one size)
        hipHostFree(h[0]);
        hipHostFree(h[1]);
        return rd_fail_msg(RD_ERR_DEVICE, "mapped pinned slot of %zu bytes: %s", bytes, hipGetErrorString(e));
    }
    for (int i = 0; i < 2; i++) {
        if (p.h[i]) memcpy(h[i] + fill, p.h[i] + p.fill, fill_len);
        else memset(h[i] + fill, 0xFF, fill_len);
        hipHostFree(p.h[i]);
        p.h[i] = h[i];
        p.d[i] = d[i];
    }
    p.bytes = bytes;
    p.fill = fill;
    p.fill_len = fill_len;
    return RD_OK;
}

// what chunk k's submit noted for the fetch of chunk k and the clip stage of chunk k + 1, by parity
struct wb_note {
    int bx_n = 0;                       // expect: the table's size, whether a launch was made, the host's candidate counts
    bool bx_launched = false;
    uint32_t bx_cand[RD_BX_MAX] = {};
    int bs_n = 0;                       // search: the list's size
    int bc_sources = 0, bc_quota = 0;   // clips: 0 - none, the slot holds no header of this chunk
};

struct rd_wideband {
    rd_chan *chan = nullptr;
    rd_demod *dem = nullptr;
    int n_ch = 0;
    size_t B = 0;                 // output samples per channel and chunk (the demodulator's block size)
    size_t chunk_bytes = 0;       // bytes of an IQ pair in the handle's format * decim * B
    uint64_t clock = 0;           // absolute output time of the next chunk's first output
    long n_sub = 0;               // chunks submitted since create / reset (chunk k uses buffers k & 1)
    long last = -1;               // chunk the last fetch returned
    bool dev_ready = false;
    hipStream_t st = nullptr, st_copy = nullptr;   // the demodulator's streams
    uint8_t *h_in[2] = {nullptr, nullptr};         // pinned staging of the host's chunk
    uint8_t *d_wide[2] = {nullptr, nullptr};       // device chunk buffers
    uint8_t *d_out[2] = {nullptr, nullptr};        // channelized chunks [n_channels][2 B]
    hipEvent_t e_in[2] = {nullptr, nullptr};       // chunk buffer k & 1 copied
    hipEvent_t e_chan[2] = {nullptr, nullptr};     // chunk k's channelizer done
    wb_slots slots[WB_SLOT_KINDS];                 // every stage's record slots (layouts: rd_slots.h)
    wb_note note[2];
    // tuning: the constructed shifts (reset() returns to them), the tuning in force (that of the last chunk submitted, or
    // (plan, 0) after create / reset - the channelizer's tables may still hold another, rd_chan_tuning) and the shifts
    // the last rd_wb_retune asked for
    std::vector<int64_t> plan, shift, phase, want;
    bool pending = false;                          // a retune waits for the next submit
    bool restored = false;                         // reset() since the last submit: the tables may hold an earlier retune
    std::vector<int64_t> rec, next_shift, next_phase;   // scratch: a submit's retune records and its tuning
    // gain: the constructed one (reset() returns to it) and what the next submitted chunk will use, as float32
    float gain0 = 0.0f;
    std::vector<float> gain;
    // Settings, each switched on a quiet receiver, so every chunk in flight has the same - bursts <- decode <- repair,
    // narrow, quality, expect, search, and bursts <- clips: switching one off switches off what needs it - and, as
    // last_* / *_last, what the last fetch kept of the features its chunk was submitted with.
    bool levels = false, last_levels = false;
    uint32_t *d_lvacc = nullptr;                   // k_chan_levels' device words
    std::vector<rd_chan_level> lv_last;
    rd_input_level lv_in_last = {};
    int spec_n = 0;                                // bins per record (0: off)
    bool last_spec = false;
    rd_spec *spec = nullptr;                       // the kernel's tables and scratch
    rd_spectrum_info sp_info_last = {};
    std::vector<double> sp_last;
    bool bursts = false, last_bursts = false;
    std::vector<uint32_t> thr;                     // the thresholds the next submitted chunk will use
    std::vector<rd_burst> bu_last;
    std::vector<rd_burst_floor> bf_last;
    rd_config cfg = {};                            // the demodulator's: symbol length, packet length and sync word
    bool decode = false, last_decode = false;
    int repair = 0;                                // max_flips of the chunks submitted from now on
    bool narrow = false;                           // step 4n for the chunks submitted from now on
    uint32_t *d_nb = nullptr;                      // its tables on the device, once a submit has needed them
    rd_delivered bm, xm, sm;                       // steps 7, 7', 7s: the messages the last fetch kept, and the one before
    std::vector<uint32_t> bl_last;
    std::vector<rd_expect> expect;                 // the table the next submitted chunk will use
    uint32_t xc_last[RD_BX_MAX] = {};
    std::vector<uint8_t> search;                   // the centres the next submitted chunk will use
    std::vector<rd_bs_header> sh_last;
    bool quality = false, last_quality = false;
    int q_gap = 0;
    std::vector<rd_burst_quality> bq_last, xq_last;   // rows beside bm.last and xm.last
    int bc_sources = 0, bc_pre = 256, bc_post = 128, bc_quota = 4096;   // sources 0: off
    bool last_clips = false;
    std::vector<rd_burst_clip> bc_last;
    std::vector<uint8_t> bc_bytes_last;
    std::vector<uint32_t> bc_dropped_last;
};
#define RD_BU_THR_DEFAULT 0xFFFFFFFFu   // no window's energy reaches it

static_assert(sizeof(rd_spectrum_info) == RD_SPEC_HDR_BYTES, "the slot's header is rd_spectrum_info");

// the tuning the next submitted chunk will use, channel c: the pending shift takes over at t_b = clock
static void wb_next_tuning(const rd_wideband *w, int c, int64_t *shift, int64_t *phase) {
    *shift = w->pending ? w->want[c] : w->shift[c];
    const __int128 fo = rd_chan_out_rate(w->chan);
    __int128 p = (__int128)w->phase[c] + (__int128)(w->shift[c] - *shift) * (__int128)(w->clock % (uint64_t)fo);
    p %= fo;
    *phase = (int64_t)(p < 0 ? p + fo : p);
}

// Retune (rd_wb_retune; the definition: rd_channelizer.hip, RETUNE): new mixer frequencies for any channels from the next
// chunk boundary on, phase-continuous, with chunks in flight.  The call only records the wanted shifts; the next submit
// turns them into (shift, P) at its boundary t_b = clock - P' = (P + (s - s') t_b) mod Fo, exact integers - and queues
// the records of the channels that change and k_chan_retune on the compute stream in front of that chunk's k_channelize
// (the previous chunk's is earlier on the same stream, so one set of tables serves).  Gain (rd_wb_set_gain;
// rd_channelizer.hip, GAIN) follows the same pattern: the call records what is wanted, the next submit stages the table
// and queues one copy in front of its k_channelize, only when an entry differs from what the table holds.
// wb_apply_tuning makes the channelizer's tables those of the next chunk's tuning: the channels that differ, on the host
// before the device tables exist, else as records in pinned slot `slot` and k_chan_retune.  Nothing differs: nothing queued.
static int wb_apply_tuning(rd_wideband *w, int slot) {
    if (!w->pending && !w->restored) return RD_OK;
    const int64_t *ts, *tp;
    rd_chan_tuning(w->chan, &ts, &tp);
    w->rec.clear();
    std::vector<int64_t> &ns = w->next_shift, &np = w->next_phase;
    ns.resize(w->n_ch);
    np.resize(w->n_ch);
    for (int c = 0; c < w->n_ch; c++) {
        wb_next_tuning(w, c, &ns[c], &np[c]);
        if (ns[c] != ts[c] || np[c] != tp[c]) w->rec.insert(w->rec.end(), {(int64_t)c, ns[c], np[c]});
    }
    const int rc = rd_chan_retune(w->chan, w->rec.data(), (int)(w->rec.size() / 3), slot, w->st);
    if (rc) return rc;           // (nothing queued, nothing recorded: the next submit tries again)
    for (int c = 0; c < w->n_ch; c++) { w->shift[c] = ns[c]; w->phase[c] = np[c]; }
    w->pending = w->restored = false;
    return RD_OK;
}

extern "C" int rd_wideband_create(const rd_config *cfg, const rd_chan_config *ccfg, const double *taps,
                                  const int64_t *shift_hz, rd_wideband **out) {
    return rd_wb_create_fmt(cfg, ccfg, RD_IQ_U8, taps, shift_hz, out);
}

extern "C" int rd_wb_create_fmt(const rd_config *cfg, const rd_chan_config *ccfg, int sample_format, const double *taps,
                                const int64_t *shift_hz, rd_wideband **out) {
    if (!cfg || !ccfg || !taps || !shift_hz || !out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (cfg->block_size < 128 || cfg->block_size % 128)
        return rd_fail_msg(RD_ERR_ARG, "block_size %d is not a positive multiple of 128", cfg->block_size);
    rd_chan *ch = nullptr;
    int rc = rd_chan_create_fmt(ccfg, sample_format, taps, shift_hz, &ch);
    if (rc) return rc;
    rd_demod *dem = nullptr;
    rc = rd_create_multi(cfg, ccfg->n_channels, &dem);
    if (rc) {
        rd_chan_destroy(ch);
        return rc;
    }
    rd_wideband *w = new rd_wideband();
    w->chan = ch;
    w->dem = dem;
    w->n_ch = ccfg->n_channels;
    w->B = (size_t)cfg->block_size;
    w->cfg = *cfg;
    w->chunk_bytes = (size_t)rd_chan_bytes_per_sample(ch) * (size_t)ccfg->decim * w->B;
    w->plan.assign(shift_hz, shift_hz + w->n_ch);
    w->shift = w->want = w->plan;
    w->phase.assign(w->n_ch, 0);
    w->gain0 = (float)ccfg->gain;
    w->gain.assign(w->n_ch, w->gain0);
    w->thr.assign(w->n_ch, RD_BU_THR_DEFAULT);
    *out = w;
    return RD_OK;
}

extern "C" void rd_wideband_destroy(rd_wideband *w) {
    if (!w) return;
    rd_destroy(w->dem);   // (waits for its streams, which carry all of this handle's work)
    if (w->dev_ready && rd_owns_device_state()) {
        for (int i = 0; i < 2; i++) {
            hipHostFree(w->h_in[i]); hipFree(w->d_wide[i]); hipFree(w->d_out[i]);
            if (w->e_in[i]) hipEventDestroy(w->e_in[i]);
            if (w->e_chan[i]) hipEventDestroy(w->e_chan[i]);
            for (wb_slots &p : w->slots) hipHostFree(p.h[i]);
        }
        hipFree(w->d_lvacc);
        hipFree(w->d_nb);
    }
    rd_spec_destroy(w->spec);   // (checks the owning process itself)
    rd_chan_destroy(w->chan);
    delete w;
}

// device state on the first submit (create does no device work: safe before fork)
static int wb_alloc(rd_wideband *w) {
    int rc = rd_demod_prepare(w->dem, &w->st, &w->st_copy);   // (makes the demodulator's device current)
    if (rc || w->dev_ready) return rc;
    rc = rd_chan_stream_prepare(w->chan);
    if (rc) return rc;
    const size_t out_bytes = (size_t)w->n_ch * 2 * w->B + RD_INPUT_PAD;
    for (int i = 0; i < 2; i++) {
        HIPCHK(hipHostMalloc((void **)&w->h_in[i], w->chunk_bytes, hipHostMallocDefault));
        HIPCHK(hipMalloc(&w->d_wide[i], w->chunk_bytes + 16));
        HIPCHK(hipMalloc(&w->d_out[i], out_bytes));
        HIPCHK(hipEventCreateWithFlags(&w->e_in[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&w->e_chan[i], hipEventDisableTiming));
    }
    w->dev_ready = true;
    return RD_OK;
}

static size_t wb_bu_windows(const rd_wideband *w) { return w->B / RD_BU_WINDOW; }
static size_t wb_wide_samples(const rd_wideband *w) { return w->chunk_bytes / (size_t)rd_chan_bytes_per_sample(w->chan); }

// What the settings in force need beside the slots: k_chan_levels' words, the spectrum's tables for its n_bins, and the
// narrow-band tables - for the narrow decoder, the search, and the quality kernel whenever symbol_length >= 4 - once.
static int wb_prepare_tables(rd_wideband *w) {
    if (w->levels && !w->d_lvacc) {
        uint32_t *acc = nullptr;
        HIPCHK(hipMalloc(&acc, RD_LV_ACC_WORDS * sizeof(uint32_t)));
        hipError_t e = hipMemsetAsync(acc, 0, RD_LV_ACC_WORDS * sizeof(uint32_t), w->st);   // (ordered before the first launch)
        if (e != hipSuccess) { hipFree(acc); return rd_fail_msg(RD_ERR_DEVICE, "hipMemsetAsync: %s", hipGetErrorString(e)); }
        w->d_lvacc = acc;
    }
    int rc = w->spec_n ? rd_spec_prepare(&w->spec, w->spec_n, wb_wide_samples(w), w->st) : RD_OK;
    if (rc) return rc;
    if ((w->narrow || !w->search.empty() || (w->quality && w->cfg.symbol_length >= RD_BD_NB_MIN_SL)) && !w->d_nb)
        return rd_bd_narrow_upload(w->cfg.symbol_length, &w->d_nb);
    return RD_OK;
}

// the slots of every feature in force, and which part of each no chunk may mistake for its own (wb_slots)
static int wb_ensure_slots(rd_wideband *w) {
    const int n = w->n_ch;
    const size_t nw = wb_bu_windows(w);
    const struct { int kind; bool on; size_t bytes, fill, fill_len; } want[] = {
        {WB_LV, w->levels, (size_t)n * sizeof(rd_chan_level) + sizeof(rd_input_level), 0, (size_t)n * sizeof(rd_chan_level) + sizeof(rd_input_level)},
        {WB_SP, w->spec_n != 0, RD_SPEC_HDR_BYTES + (size_t)w->spec_n * sizeof(double), 0, RD_SPEC_HDR_BYTES},
        {WB_BU, w->bursts, rd_bu_slot_bytes(n, nw), rd_bu_floor_offset(n, nw), (size_t)n * sizeof(rd_burst_floor)},
        {WB_BD, w->decode, rd_bd_slot_bytes(n, nw), rd_bd_header_offset(n, nw), (size_t)n * sizeof(rd_bd_header)},
        {WB_BX, w->decode, RD_BX_SLOT_BYTES, 0, RD_BX_SLOT_BYTES},
        {WB_BQ, w->quality, rd_bq_slot_bytes(n, nw), 0, rd_bq_slot_bytes(n, nw)},
        {WB_BS, !w->search.empty(), rd_bs_slot_bytes(n), 0, rd_bs_slot_bytes(n)},
        {WB_BC, w->bc_sources != 0, rd_bc_slot_bytes(n, w->bc_quota), rd_bc_header_offset(n), (size_t)n * sizeof(rd_bc_header)},
    };
    for (const auto &s : want) {
        const int rc = s.on ? wb_slots_ensure(w->slots[s.kind], s.bytes, s.fill, s.fill_len) : RD_OK;
        if (rc) return rc;
    }
    return RD_OK;
}

extern "C" int rd_wideband_reset(rd_wideband *w) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    int rc = rd_reset(w->dem);   // waits for the chunks in flight: their channelizers ran before their demod launches
    if (rc) return rc;
    w->clock = 0;
    w->n_sub = 0;                // (no previous chunk: zero history, no look-back)
    w->last = -1;
    w->shift = w->plan;          // a pending retune is dropped; the next submit rebuilds what the tables hold otherwise
    w->phase.assign(w->n_ch, 0);
    w->pending = false;
    w->restored = true;
    w->gain.assign(w->n_ch, w->gain0);   // a pending gain change is dropped; the next submit rewrites the table if it differs
    w->thr.assign(w->n_ch, RD_BU_THR_DEFAULT);   // a pending threshold change is dropped
    w->expect.clear();           // (the windows refer to the clock that has just restarted; every other setting stays)
    // chunk numbers restart: no record of the run before may pass for one of this run, in a slot or in what a fetch kept
    w->last_levels = w->last_spec = w->last_bursts = w->last_decode = w->last_quality = w->last_clips = false;
    for (wb_slots &p : w->slots)
        for (int i = 0; i < 2; i++)
            if (p.h[i]) memset(p.h[i] + p.fill, 0xFF, p.fill_len);
    w->note[0] = w->note[1] = wb_note();   // (what the run before owed goes: its clip headers, its expect and search lists)
    w->bm.forget();
    w->xm.forget();
    w->sm.forget();
    return RD_OK;
}

extern "C" int rd_wb_set_gain(rd_wideband *w, const double *gain, int n) {
    if (!w || !gain) return rd_fail_msg(RD_ERR_ARG, "null argument");
    int rc = rd_chan_check_gains(w->chan, gain, n);
    if (rc) return rc;
    for (int c = 0; c < n; c++) w->gain[c] = (float)gain[c];
    return RD_OK;
}

extern "C" int rd_wb_gains(rd_wideband *w, double *gain, int n) {
    if (!w || !gain) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (n != w->n_ch) return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: room for %d channels of %d", n, w->n_ch);
    for (int c = 0; c < n; c++) gain[c] = (double)w->gain[c];
    return RD_OK;
}

// A feature is switched on a quiet receiver only.  `what`: the feature with its verb, "levels are".
static int wb_quiet(rd_wideband *w, const char *what) {
    const int n = rd_demod_inflight(w->dem);
    return n ? rd_fail_msg(RD_ERR_STATE, "%d chunk(s) in flight: fetch them before %s switched", n, what) : RD_OK;
}
// The two halves of a result call: the last fetched chunk has the feature's records at all; and how many there are,
// with all of them or RD_ERR_CAPACITY.
static int wb_have(const rd_wideband *w, bool on, const char *feature, const char *setter) {
    if (w->last < 0) return rd_fail_msg(RD_ERR_STATE, "no chunk fetched since create / reset");
    if (!on) return rd_fail_msg(RD_ERR_STATE, "the last fetched chunk was submitted with %s off (%s)", feature, setter);
    return RD_OK;
}
template <class T>
static int wb_copy_out(const std::vector<T> &v, T *out, int cap, int *n, const char *what) {
    *n = (int)v.size();
    if (cap < *n) return rd_fail_msg(RD_ERR_CAPACITY, "%d %s, room for %d", *n, what, cap);
    if (*n) memcpy(out, v.data(), (size_t)*n * sizeof(T));
    return RD_OK;
}
#define WB_BAD_OUT(w, out, cap, n) (!(w) || !(n) || (cap) < 0 || (!(out) && (cap) > 0))

extern "C" int rd_wb_set_levels(rd_wideband *w, int enabled) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    if (int rc = wb_quiet(w, "levels are")) return rc;
    w->levels = enabled != 0;
    return RD_OK;
}

extern "C" int rd_wb_levels(rd_wideband *w, rd_chan_level *out, int n, rd_input_level *in) {
    if (!w || !out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (n != w->n_ch) return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: room for %d channels of %d", n, w->n_ch);
    if (int rc = wb_have(w, w->last_levels, "levels", "rd_wb_set_levels")) return rc;
    memcpy(out, w->lv_last.data(), (size_t)n * sizeof(rd_chan_level));
    if (in) *in = w->lv_in_last;
    return RD_OK;
}

extern "C" int rd_wb_set_spectrum(rd_wideband *w, int n_bins) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    if (int rc = wb_quiet(w, "the spectrum is")) return rc;
    if (n_bins != 0) {
        int rc = rd_spec_check(n_bins, wb_wide_samples(w));
        if (rc) return rc;
    }
    w->spec_n = n_bins;
    return RD_OK;
}

extern "C" int rd_wb_spectrum(rd_wideband *w, double *power, int n_bins, rd_spectrum_info *info) {
    if (!w || !power) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (int rc = wb_have(w, w->last_spec, "the spectrum", "rd_wb_set_spectrum")) return rc;
    if (n_bins != (int)w->sp_info_last.n_bins)
        return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: room for %d bins of %u", n_bins, w->sp_info_last.n_bins);
    memcpy(power, w->sp_last.data(), (size_t)n_bins * sizeof(double));
    if (info) *info = w->sp_info_last;
    return RD_OK;
}

// what needs burst decode goes off with it (clips of runs go on; nothing left: off)
static void wb_decode_off(rd_wideband *w) {
    w->decode = false;
    w->repair = 0;
    w->narrow = false;
    w->quality = false;
    w->expect.clear();
    w->search.clear();
    w->bc_sources &= ~(int)RD_BC_MESSAGES;
}

extern "C" int rd_wb_set_bursts(rd_wideband *w, int enabled) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    if (int rc = wb_quiet(w, "bursts are")) return rc;
    if (enabled) {
        int rc = rd_bursts_check(w->B);
        if (rc) return rc;
    }
    w->bursts = enabled != 0;
    if (!w->bursts) {                    // (the decoder and the clips read the burst records)
        wb_decode_off(w);
        w->bc_sources = 0;
    }
    return RD_OK;
}

extern "C" int rd_wb_set_burst_decode(rd_wideband *w, int enabled) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    if (int rc = wb_quiet(w, "burst decode is")) return rc;
    if (enabled) {
        if (!w->bursts) return rd_fail_msg(RD_ERR_STATE, "burst decode needs bursts on (rd_wb_set_bursts)");
        int rc = rd_burst_decode_check(&w->cfg);
        if (rc) return rc;
    }
    if (enabled) w->decode = true;
    else wb_decode_off(w);
    return RD_OK;
}

extern "C" int rd_wb_set_burst_repair(rd_wideband *w, int max_flips) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    if (max_flips < 0 || max_flips > RD_BD_MAX_FLIPS)
        return rd_fail_msg(RD_ERR_ARG, "burst repair: max_flips %d, not 0 .. %d", max_flips, RD_BD_MAX_FLIPS);
    if (int rc = wb_quiet(w, "burst repair is")) return rc;
    if (!w->decode) return rd_fail_msg(RD_ERR_STATE, "burst repair needs burst decode on (rd_wb_set_burst_decode)");
    w->repair = max_flips;
    return RD_OK;
}

extern "C" int rd_wb_burst_repair(rd_wideband *w, int *max_flips) {
    if (!w || !max_flips) return rd_fail_msg(RD_ERR_ARG, "null argument");
    *max_flips = w->repair;
    return RD_OK;
}

extern "C" int rd_wb_set_burst_narrow(rd_wideband *w, int on) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    if (int rc = wb_quiet(w, "the narrow-band filter is")) return rc;
    if (!w->decode) return rd_fail_msg(RD_ERR_STATE, "the narrow-band filter needs burst decode on (rd_wb_set_burst_decode)");
    if (on && w->cfg.symbol_length < RD_BD_NB_MIN_SL)
        return rd_fail_msg(RD_ERR_ARG, "narrow-band filter: symbol_length %d, at least %d", w->cfg.symbol_length, RD_BD_NB_MIN_SL);
    w->narrow = on != 0;
    return RD_OK;
}

extern "C" int rd_wb_burst_narrow(rd_wideband *w, int *on) {
    if (!w || !on) return rd_fail_msg(RD_ERR_ARG, "null argument");
    *on = w->narrow ? 1 : 0;
    return RD_OK;
}

extern "C" int rd_wb_set_burst_quality(rd_wideband *w, int on, int noise_gap) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    if (noise_gap < 0 || noise_gap > RD_BQ_MAX_GAP)
        return rd_fail_msg(RD_ERR_ARG, "burst quality: noise_gap %d, not 0 .. %d", noise_gap, RD_BQ_MAX_GAP);
    if (int rc = wb_quiet(w, "burst quality is")) return rc;
    if (!w->decode) return rd_fail_msg(RD_ERR_STATE, "burst quality needs burst decode on (rd_wb_set_burst_decode)");
    w->quality = on != 0;
    w->q_gap = noise_gap;
    return RD_OK;
}

extern "C" int rd_wb_burst_quality(rd_wideband *w, int *on, int *noise_gap) {
    if (!w || !on || !noise_gap) return rd_fail_msg(RD_ERR_ARG, "null argument");
    *on = w->quality ? 1 : 0;
    *noise_gap = w->q_gap;
    return RD_OK;
}

static int wb_quality_rows(rd_wideband *w, const std::vector<rd_burst_quality> &rows, rd_burst_quality *out, int cap, int *n) {
    if (WB_BAD_OUT(w, out, cap, n)) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (int rc = wb_have(w, w->last_quality, "burst quality", "rd_wb_set_burst_quality")) return rc;
    return wb_copy_out(rows, out, cap, n, "quality records");
}

extern "C" int rd_wb_burst_message_quality(rd_wideband *w, rd_burst_quality *out, int cap, int *n) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null argument");
    return wb_quality_rows(w, w->bq_last, out, cap, n);
}

extern "C" int rd_wb_expected_message_quality(rd_wideband *w, rd_burst_quality *out, int cap, int *n) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null argument");
    return wb_quality_rows(w, w->xq_last, out, cap, n);
}

extern "C" int rd_wb_burst_messages(rd_wideband *w, rd_burst_msg *out, int cap, int *n, uint32_t *long_runs, int n_channels) {
    if (WB_BAD_OUT(w, out, cap, n)) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (long_runs && n_channels != w->n_ch)
        return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: room for %d long-run counts of %d", n_channels, w->n_ch);
    if (int rc = wb_have(w, w->last_decode, "burst decode", "rd_wb_set_burst_decode")) return rc;
    if (long_runs) memcpy(long_runs, w->bl_last.data(), (size_t)w->n_ch * sizeof(uint32_t));
    return wb_copy_out(w->bm.last, out, cap, n, "burst messages");
}

extern "C" int rd_wb_set_burst_expect(rd_wideband *w, const rd_expect *e, int n) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    int bad = -1;
    const char *why = "";
    if (rd_bx_check_table(e, n, w->n_ch, &bad, &why)) {
        if (bad < 0) return rd_fail_msg(RD_ERR_ARG, "burst expect: %s, got %d", why, n);
        return rd_fail_msg(RD_ERR_ARG, "burst expect: entry %d: %s", bad, why);
    }
    if (!w->decode) return rd_fail_msg(RD_ERR_STATE, "burst expect needs burst decode on (rd_wb_set_burst_decode)");
    w->expect.assign(e, e + n);
    return RD_OK;
}

extern "C" int rd_wb_burst_expect(rd_wideband *w, rd_expect *out, int cap, int *n) {
    if (WB_BAD_OUT(w, out, cap, n)) return rd_fail_msg(RD_ERR_ARG, "null argument");
    return wb_copy_out(w->expect, out, cap, n, "expectations");
}

extern "C" int rd_wb_expected_messages(rd_wideband *w, rd_burst_msg *out, int cap, int *n, uint32_t *candidates, int n_cand) {
    if (WB_BAD_OUT(w, out, cap, n)) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (candidates && n_cand != RD_BX_MAX)
        return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: room for %d candidate counts of %d", n_cand, RD_BX_MAX);
    if (int rc = wb_have(w, w->last_decode, "burst decode", "rd_wb_set_burst_decode")) return rc;
    if (candidates) memcpy(candidates, w->xc_last, sizeof w->xc_last);
    return wb_copy_out(w->xm.last, out, cap, n, "expected messages");
}

extern "C" int rd_wb_set_burst_search(rd_wideband *w, const uint8_t *centres, int n) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    int bad = -1;
    const char *why = "";
    if (rd_bs_check_centres(centres, n, &bad, &why)) {
        if (bad < 0) return rd_fail_msg(RD_ERR_ARG, "burst search: %s, got %d", why, n);
        return rd_fail_msg(RD_ERR_ARG, "burst search: centre %d: %s", bad, why);
    }
    if (!w->decode) return rd_fail_msg(RD_ERR_STATE, "burst search needs burst decode on (rd_wb_set_burst_decode)");
    if (n > 0) {
        int rc = rd_burst_decode_check(&w->cfg);
        if (rc) return rc;
        if (w->cfg.symbol_length < RD_BD_NB_MIN_SL)
            return rd_fail_msg(RD_ERR_ARG, "burst search: symbol_length %d, at least %d", w->cfg.symbol_length, RD_BD_NB_MIN_SL);
        if (w->n_ch > RD_BS_MAX_CHANNELS) return rd_fail_msg(RD_ERR_ARG, "burst search: %d channels, at most %d", w->n_ch, RD_BS_MAX_CHANNELS);
    }
    w->search.assign(centres, centres + n);
    return RD_OK;
}

extern "C" int rd_wb_burst_search(rd_wideband *w, uint8_t *out, int cap, int *n) {
    if (WB_BAD_OUT(w, out, cap, n)) return rd_fail_msg(RD_ERR_ARG, "null argument");
    return wb_copy_out(w->search, out, cap, n, "centres");
}

extern "C" int rd_wb_searched_messages(rd_wideband *w, rd_burst_msg *out, int cap, int *n, rd_bs_header *hdr, int n_hdr) {
    if (WB_BAD_OUT(w, out, cap, n)) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (hdr && n_hdr != RD_BS_MAX_CENTRES * w->n_ch)
        return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: room for %d headers of %d", n_hdr, RD_BS_MAX_CENTRES * w->n_ch);
    if (int rc = wb_have(w, w->last_decode, "burst decode", "rd_wb_set_burst_decode")) return rc;
    if (hdr) {
        memset(hdr, 0xFF, (size_t)n_hdr * sizeof(rd_bs_header));
        if (!w->sh_last.empty()) memcpy(hdr, w->sh_last.data(), w->sh_last.size() * sizeof(rd_bs_header));
    }
    return wb_copy_out(w->sm.last, out, cap, n, "searched messages");
}

extern "C" int rd_wb_set_burst_clips(rd_wideband *w, int sources, int pre, int post, int quota) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    int rc = rd_burst_clips_check(w->n_ch, sources, pre, post, quota);
    if (rc) return rc;
    if ((rc = wb_quiet(w, "burst clips are"))) return rc;
    if (!w->bursts) return rd_fail_msg(RD_ERR_STATE, "burst clips need bursts on (rd_wb_set_bursts)");
    if ((sources & (int)RD_BC_MESSAGES) && !w->decode)
        return rd_fail_msg(RD_ERR_STATE, "burst clips of messages need burst decode on (rd_wb_set_burst_decode)");
    w->bc_sources = sources;
    w->bc_pre = pre;
    w->bc_post = post;
    w->bc_quota = quota;
    return RD_OK;
}

extern "C" int rd_wb_burst_clips_config(rd_wideband *w, int *sources, int *pre, int *post, int *quota) {
    if (!w || !sources || !pre || !post || !quota) return rd_fail_msg(RD_ERR_ARG, "null argument");
    *sources = w->bc_sources;
    *pre = w->bc_pre;
    *post = w->bc_post;
    *quota = w->bc_quota;
    return RD_OK;
}

// (two arrays with two capacities: its own tail)
extern "C" int rd_wb_burst_clips(rd_wideband *w, rd_burst_clip *out, int cap, int *n, uint8_t *bytes, size_t bytes_cap, size_t *n_bytes,
                                 uint32_t *dropped, int n_channels) {
    if (WB_BAD_OUT(w, out, cap, n) || !n_bytes || (!bytes && bytes_cap > 0)) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (dropped && n_channels != w->n_ch)
        return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: room for %d drop counts of %d", n_channels, w->n_ch);
    if (int rc = wb_have(w, w->last_clips, "burst clips", "rd_wb_set_burst_clips")) return rc;
    *n = (int)w->bc_last.size();
    *n_bytes = w->bc_bytes_last.size();
    if (dropped) memcpy(dropped, w->bc_dropped_last.data(), (size_t)w->n_ch * sizeof(uint32_t));
    if (cap < *n || bytes_cap < *n_bytes)
        return rd_fail_msg(RD_ERR_CAPACITY, "%d burst clips of %zu bytes, room for %d of %zu", *n, *n_bytes, cap, bytes_cap);
    if (*n) memcpy(out, w->bc_last.data(), (size_t)*n * sizeof(rd_burst_clip));
    if (*n_bytes) memcpy(bytes, w->bc_bytes_last.data(), *n_bytes);
    return RD_OK;
}

extern "C" int rd_wb_set_burst_threshold(rd_wideband *w, const uint32_t *thr, int n) {
    if (!w || !thr) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (n != w->n_ch) return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: %d thresholds for %d channels", n, w->n_ch);
    w->thr.assign(thr, thr + n);
    return RD_OK;
}

extern "C" int rd_wb_burst_thresholds(rd_wideband *w, uint32_t *thr, int n) {
    if (!w || !thr) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (n != w->n_ch) return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: room for %d channels of %d", n, w->n_ch);
    memcpy(thr, w->thr.data(), (size_t)n * sizeof(uint32_t));
    return RD_OK;
}

extern "C" int rd_wb_bursts(rd_wideband *w, rd_burst *out, int cap, int *n, rd_burst_floor *floor, int n_floor) {
    if (WB_BAD_OUT(w, out, cap, n)) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (floor && n_floor != w->n_ch)
        return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: room for %d floor records of %d", n_floor, w->n_ch);
    if (int rc = wb_have(w, w->last_bursts, "bursts", "rd_wb_set_bursts")) return rc;
    if (floor) memcpy(floor, w->bf_last.data(), (size_t)w->n_ch * sizeof(rd_burst_floor));
    return wb_copy_out(w->bu_last, out, cap, n, "burst records");
}

extern "C" int rd_wb_fetched_chunk(rd_wideband *w, uint64_t *chunk) {
    if (!w || !chunk) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (w->last < 0) return rd_fail_msg(RD_ERR_STATE, "no chunk fetched since create / reset");
    *chunk = (uint64_t)w->last;
    return RD_OK;
}

extern "C" int rd_wb_retune(rd_wideband *w, const int64_t *shift_hz, int n) {
    if (!w || !shift_hz) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (n != w->n_ch) return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: %d shifts for %d channels", n, w->n_ch);
    const int64_t half = rd_chan_wide_rate(w->chan) / 2;
    for (int c = 0; c < n; c++)
        if (shift_hz[c] > half || shift_hz[c] < -half)
            return rd_fail_msg(RD_ERR_ARG, "channel %d: a shift of %lld Hz lies outside the captured band", c, (long long)shift_hz[c]);
    w->want.assign(shift_hz, shift_hz + n);
    w->pending = true;
    return RD_OK;
}

extern "C" int rd_wb_tuning(rd_wideband *w, int64_t *shift_hz, int64_t *phase, int n) {
    if (!w || !shift_hz || !phase) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (n != w->n_ch) return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: room for %d channels of %d", n, w->n_ch);
    for (int c = 0; c < n; c++) wb_next_tuning(w, c, &shift_hz[c], &phase[c]);
    return RD_OK;
}

// The chunk a submit is queueing.  Every stage below writes the slot of parity s, last written for chunk k-2 and read by
// its fetch: free, because rd_demod_check_room refuses a third chunk - chunk k-2 has been fetched, or waited for as stale,
// so all its work on the compute stream is done.  Whoever relaxes that limit must give the slots an event of their own.
// Host writes into a slot made before a launch are visible to it.  The burst kernels read d_out[s], next written by the
// channelizer of chunk k+2, and below t = 0 the end of prev_out = d_out[s ^ 1], chunk k-1's channelized bytes, next
// written by the channelizer of chunk k+1: both later on the same stream.
struct wb_chunk {
    int s;                     // parity: which buffers and slots
    uint64_t k;                // sequence number since create / reset
    int have_prev;
    const uint8_t *prev_out;   // the chunk before's d_out, null for the first
};
static uint8_t *wb_dev(rd_wideband *w, int kind, const wb_chunk &c) { return w->slots[kind].d[c.s]; }

// Levels (rd_wb_set_levels / rd_wb_levels; rd_chan_levels.hip, LEVELS): k_chan_levels behind the chunk's k_channelize
// (behind e_chan: the copy stream never waits for it).  It and k_chan_spectrum READ d_wide[s]: that buffer is next
// overwritten by the copy of chunk k+2, which waits for e_chan of chunk k+1 - recorded later on the compute stream than
// either kernel of chunk k, so the copy cannot overtake them although they come behind chunk k's own e_chan.
static int wb_queue_levels(rd_wideband *w, const wb_chunk &c) {
    rd_chan_level *lv = (rd_chan_level *)wb_dev(w, WB_LV, c);
    return rd_chan_stream_levels(w->chan, w->d_wide[c.s], w->B, w->d_out[c.s], 2 * w->B, c.k, lv, (rd_input_level *)(lv + w->n_ch),
                                 w->d_lvacc, w->st);
}

// Spectrum (rd_wb_set_spectrum / rd_wb_spectrum; rd_spectrum.hip): k_chan_spectrum in the same place, beside
// k_chan_levels when both are on; the record is a header and n_bins doubles.  It reads d_wide[s] only (above).
static int wb_queue_spectrum(rd_wideband *w, const wb_chunk &c) {
    return rd_spec_launch(w->spec, w->d_wide[c.s], rd_chan_format(w->chan), wb_wide_samples(w), c.k, wb_dev(w, WB_SP, c), w->st);
}

// Bursts (rd_wb_set_bursts / rd_wb_bursts; rd_bursts.hip): k_chan_bursts over d_out[s].  The thresholds
// (rd_wb_set_burst_threshold: recorded by the call, in force from the next submit, like the gains) need no copy and no
// device table: they travel in the slot, and the kernel echoes what it used in the floor records.
static int wb_queue_bursts(rd_wideband *w, const wb_chunk &c) {
    memcpy(w->slots[WB_BU].h[c.s] + rd_bu_thr_offset(w->n_ch, wb_bu_windows(w)), w->thr.data(), (size_t)w->n_ch * sizeof(uint32_t));
    return rd_bursts_launch(w->d_out[c.s], 2 * w->B, w->n_ch, w->B, c.k, wb_dev(w, WB_BU, c), w->st);
}

// Burst decode (rd_wb_set_burst_decode / rd_wb_burst_messages; rd_burst_decode.hip): k_chan_burst_decode behind
// k_chan_bursts, whose slot it reads on the device, with d_out[s] and, for a run that begins with the chunk, prev_out.
// Repair (rd_wb_set_burst_repair) is one integer every submit hands to the launch, which picks the kernel instantiation by
// it: no table, no copy.  The narrow-band filter (rd_wb_set_burst_narrow) is one flag kept the same way and one device
// table (wb_prepare_tables); the launch gets the table when the flag is set and a null pointer otherwise.
static const uint32_t *wb_narrow(const rd_wideband *w) { return w->narrow ? w->d_nb : nullptr; }
static int wb_queue_decode(rd_wideband *w, const wb_chunk &c) {
    return rd_burst_decode_launch(&w->cfg, w->d_out[c.s], c.prev_out, 2 * w->B, w->n_ch, w->B, w->clock, c.k, w->repair, wb_narrow(w),
                                  wb_dev(w, WB_BU, c), wb_dev(w, WB_BD, c), w->st);
}

// Burst quality (rd_wb_set_burst_quality / rd_wb_burst_message_quality / rd_wb_expected_message_quality;
// rd_burst_quality.hip): a flag and the noise gap, kept like repair.  k_chan_burst_quality behind k_chan_burst_decode over
// the decode slot and, when k_chan_burst_expect was launched, behind it over the expect slot (over_expect); it reads on the
// device what the kernel in front wrote, d_out[s] and prev_out, and writes its own slot ([n_ch][cap] | [RD_BX_MAX] rows).
static int wb_queue_quality(rd_wideband *w, const wb_chunk &c, bool over_expect) {
    const size_t nw = wb_bu_windows(w), cap = over_expect ? 1 : rd_bu_cap(nw);
    const uint8_t *src = wb_dev(w, over_expect ? WB_BX : WB_BD, c);
    const uint8_t *hdr = src + (over_expect ? RD_BX_HEADER_OFFSET : rd_bd_header_offset(w->n_ch, nw));
    uint8_t *rows = wb_dev(w, WB_BQ, c) + (over_expect ? rd_bq_expect_offset(w->n_ch, nw) : 0);
    return rd_burst_quality_launch(&w->cfg, w->d_out[c.s], c.prev_out, 2 * w->B, w->n_ch, w->B, w->q_gap, w->d_nb, (const rd_burst_msg *)src,
                                   cap, (const rd_bq_header *)hdr, over_expect ? w->note[c.s].bx_n : w->n_ch, (rd_burst_quality *)rows, w->st);
}

// Burst expect (rd_wb_set_burst_expect / rd_wb_expected_messages; rd_burst_expect.hip): the table is host bookkeeping like
// the thresholds.  The submit works out from the clock alone which expectations have candidates in the chunk
// (rd_burst_expect_stage) and writes them, as candidate ranges, into the slot.  None active: nothing is launched, and the
// fetch reports zero records from the host's own note.  Otherwise k_chan_burst_expect behind k_chan_burst_decode.
static int wb_queue_expect(rd_wideband *w, const wb_chunk &c) {
    wb_note &nt = w->note[c.s];
    nt.bx_n = (int)w->expect.size();
    if (rd_burst_expect_stage(&w->cfg, c.have_prev, w->clock, w->expect.data(), nt.bx_n, w->slots[WB_BX].h[c.s], nt.bx_cand) <= 0) return RD_OK;
    const int rc = rd_burst_expect_launch(&w->cfg, w->d_out[c.s], c.prev_out, 2 * w->B, w->n_ch, w->B, w->clock, c.k, nt.bx_n, w->repair,
                                          wb_narrow(w), wb_dev(w, WB_BX, c), w->st);
    nt.bx_launched = rc == RD_OK;
    return rc;
}

// Burst search (rd_wb_set_burst_search / rd_wb_searched_messages; rd_burst_search.hip): the list of centres is host
// bookkeeping like the expect table; the submit notes its size and hands the centres to the launch in the kernel's
// arguments.  k_chan_burst_search behind k_chan_burst_expect (behind k_chan_burst_decode when that was not launched); it
// always needs the narrow-band tables.
static int wb_queue_search(rd_wideband *w, const wb_chunk &c) {
    const int n = (int)w->search.size();
    const int rc = rd_burst_search_launch(&w->cfg, w->d_out[c.s], c.prev_out, 2 * w->B, w->n_ch, w->B, w->clock, c.k, w->search.data(), n,
                                          w->d_nb, wb_dev(w, WB_BS, c), w->st);
    if (rc == RD_OK) w->note[c.s].bs_n = n;
    return rc;
}

// Burst clips (rd_wb_set_burst_clips / rd_wb_burst_clips; rd_burst_clips.hip): a source mask, two rolls and a quota, kept
// like repair.  k_chan_burst_clips behind the chunk's last burst kernel.  It reads, on the device, the burst and decode
// slots, the expect and search slots only when their kernels were launched for this chunk (the notes), and the headers of
// the OTHER parity's clip slot when chunk k-1 was submitted with clips on - written by that chunk's launch, earlier on the
// same stream; reset() forgets them.
static int wb_queue_clips(rd_wideband *w, const wb_chunk &c) {
    wb_note &nt = w->note[c.s];
    const uint8_t *prev_hdr = nullptr;
    if (c.have_prev && w->note[c.s ^ 1].bc_sources) prev_hdr = w->slots[WB_BC].d[c.s ^ 1] + rd_bc_header_offset(w->n_ch);
    const int rc = rd_burst_clips_launch(&w->cfg, w->d_out[c.s], c.prev_out, 2 * w->B, w->n_ch, w->B, w->clock, c.k, w->bc_sources, w->bc_pre,
                                         w->bc_post, w->bc_quota, wb_dev(w, WB_BU, c), w->decode ? wb_dev(w, WB_BD, c) : nullptr,
                                         nt.bx_launched ? wb_dev(w, WB_BX, c) : nullptr, nt.bx_launched ? nt.bx_n : 0,
                                         nt.bs_n ? wb_dev(w, WB_BS, c) : nullptr, nt.bs_n, (const rd_bc_header *)prev_hdr,
                                         wb_dev(w, WB_BC, c), w->st);
    if (rc) return rc;
    nt.bc_sources = w->bc_sources;
    nt.bc_quota = w->bc_quota;
    return RD_OK;
}

extern "C" int rd_wideband_submit(rd_wideband *w, const void *wide_iq, size_t nbytes) {
    if (!w || !wide_iq) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (nbytes != w->chunk_bytes)
        return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: got %zu bytes, expected %zu", nbytes, w->chunk_bytes);
    int rc = RD_OK;
    if (!w->dev_ready && (rc = wb_apply_tuning(w, 0))) return rc;   // (the tables are still the host's)
    if ((rc = wb_alloc(w)) || (rc = wb_ensure_slots(w)) || (rc = wb_prepare_tables(w))) return rc;
    rc = rd_demod_check_room(w->dem);   // a third chunk is refused before anything is queued
    if (rc) return rc;
    const int s = (int)(w->n_sub & 1);
    const bool prev = w->n_sub >= 1;
    const wb_chunk c = {s, (uint64_t)w->n_sub, prev ? 1 : 0, prev ? w->d_out[s ^ 1] : nullptr};
    // the pinned slot's previous copy (chunk k-2) has completed: its demod block has been fetched or dropped
    if (w->n_sub >= 2) HIPCHK(hipEventSynchronize(w->e_in[s]));
    memcpy(w->h_in[s], wide_iq, nbytes);
    // buffer s holds chunk k-2, the history chunk k-1's channelizer reads: overwrite it once that has run
    if (prev) HIPCHK(hipStreamWaitEvent(w->st_copy, w->e_chan[s ^ 1], 0));
    HIPCHK(hipMemcpyAsync(w->d_wide[s], w->h_in[s], nbytes, hipMemcpyHostToDevice, w->st_copy));
    HIPCHK(hipEventRecord(w->e_in[s], w->st_copy));
    // The retune records and the gain table travel through pinned slots of parity s as well, copied on the COMPUTE stream:
    // e_in[s] above (the copy stream's event) does not order that copy; they are free by wb_chunk's argument.
    if ((rc = wb_apply_tuning(w, s))) return rc;
    if ((rc = rd_chan_stream_gains(w->chan, w->gain.data(), s, w->st))) return rc;
    HIPCHK(hipStreamWaitEvent(w->st, w->e_in[s], 0));
    rc = rd_chan_stream_launch(w->chan, w->d_wide[s], prev ? w->d_wide[s ^ 1] : nullptr, w->B, w->clock, w->d_out[s], 2 * w->B, w->st);
    if (rc) return rc;
    HIPCHK(hipEventRecord(w->e_chan[s], w->st));
    if (w->levels && (rc = wb_queue_levels(w, c))) return rc;
    if (w->spec_n && (rc = wb_queue_spectrum(w, c))) return rc;
    w->note[s] = wb_note();   // (whatever chunk k-2 was submitted with: this chunk has a feature only once its launch is queued)
    if (w->bursts && (rc = wb_queue_bursts(w, c))) return rc;
    if (w->decode && (rc = wb_queue_decode(w, c))) return rc;
    if (w->quality && (rc = wb_queue_quality(w, c, false))) return rc;
    if (!w->expect.empty() && (rc = wb_queue_expect(w, c))) return rc;
    if (w->quality && w->note[s].bx_launched && (rc = wb_queue_quality(w, c, true))) return rc;
    if (!w->search.empty() && (rc = wb_queue_search(w, c))) return rc;
    if (w->bc_sources && (rc = wb_queue_clips(w, c))) return rc;
    w->clock += w->B;
    w->n_sub++;
    return rd_demod_submit_device(w->dem, w->d_out[s]);
}

// The chunk's demodulator launch has reported, and every stage's kernel ran before it on the same stream: keep their
// records (a slot is chunk last + 2's from its submit on).  The first refusal decides the error; a last_* flag is set
// only behind its collection.
static int wb_fetched(rd_wideband *w, int rc) {
    if (rc != RD_OK && rc != RD_ERR_CAPACITY) return rc;
    const long k = w->last = w->n_sub - 1 - rd_demod_pending(w->dem);  // (the oldest in flight)
    const int s = (int)(k & 1), n = w->n_ch, sl = w->cfg.symbol_length;
    const size_t nw = wb_bu_windows(w);
    const wb_note &nt = w->note[s];
    auto slot = [&](int kind) -> const uint8_t * { return w->slots[kind].h[s]; };
    const uint8_t *bq = w->quality ? slot(WB_BQ) : nullptr;
    w->last_levels = w->last_spec = w->last_bursts = w->last_decode = w->last_quality = w->last_clips = false;
    rd_errtext err;
    auto failed = [&](int bad) { return bad ? rd_fail_msg(bad, "%s", err.text) : RD_OK; };
    if (nt.bc_sources && failed(rd_collect_clips(slot(WB_BC), n, nt.bc_quota, k, w->bc_last, w->bc_bytes_last, w->bc_dropped_last, &err)))
        return RD_ERR_DEVICE;
    w->last_clips = nt.bc_sources != 0;
    if (w->decode && failed(rd_collect_decode(slot(WB_BD), bq, n, nw, k, sl, w->bm, w->bl_last, w->bq_last, &err))) return RD_ERR_DEVICE;
    if (w->decode && failed(rd_collect_expect(nt.bx_launched ? slot(WB_BX) : nullptr, bq, n, nw, k, sl, nt.bx_n, nt.bx_cand, w->xm, w->xc_last,
                                              w->xq_last, &err)))
        return RD_ERR_DEVICE;
    if (w->decode && failed(rd_collect_search(slot(WB_BS), n, k, sl, nt.bs_n, w->sm, w->sh_last, &err))) return RD_ERR_DEVICE;
    w->last_decode = w->decode;
    w->last_quality = w->decode && w->quality;
    if (w->bursts && failed(rd_collect_bursts(slot(WB_BU), n, nw, k, w->bu_last, w->bf_last, &err))) return RD_ERR_DEVICE;
    w->last_bursts = w->bursts;
    if (w->spec_n && failed(rd_collect_spectrum(slot(WB_SP), w->spec_n, k, &w->sp_info_last, w->sp_last, &err))) return RD_ERR_DEVICE;
    w->last_spec = w->spec_n != 0;
    if (w->levels && failed(rd_collect_levels(slot(WB_LV), n, k, w->lv_last, &w->lv_in_last, &err))) return RD_ERR_DEVICE;
    w->last_levels = w->levels;
    return rc;
}

extern "C" int rd_wideband_fetch(rd_wideband *w, rd_packet *out, int cap, int *n) {
    if (!w || !n) return rd_fail_msg(RD_ERR_ARG, "null argument");
    return wb_fetched(w, rd_demod_fetch(w->dem, out, cap, n));
}

extern "C" int rd_wideband_refetch(rd_wideband *w, rd_packet *out, int cap, int *n) {
    if (!w || !n) return rd_fail_msg(RD_ERR_ARG, "null argument");
    return rd_demod_refetch(w->dem, out, cap, n);
}

// Parser.parse's front half for every channel's packets, inside the demodulator's kernels (rd_demod_set_parse / rd_demod_parsed)
extern "C" int rd_wb_set_parse(rd_wideband *w, int enabled) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    return rd_demod_set_parse(w->dem, enabled);
}

extern "C" int rd_wb_parsed(rd_wideband *w, rd_parsed *out, int cap, int *n) {
    if (!w || !n) return rd_fail_msg(RD_ERR_ARG, "null argument");
    return rd_demod_parsed(w->dem, out, cap, n);
}

extern "C" int rd_wideband_inflight(rd_wideband *w) { return w ? rd_demod_pending(w->dem) : 0; }

extern "C" int rd_wideband_copy_channelized(rd_wideband *w, uint8_t *out, size_t nbytes) {
    if (!w || !out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    const size_t need = (size_t)w->n_ch * 2 * w->B;
    if (nbytes != need) return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: got %zu bytes, expected %zu", nbytes, need);
    if (w->last < 0) return rd_fail_msg(RD_ERR_STATE, "no chunk fetched since create / reset");
    if (w->n_sub - w->last > 2) return rd_fail_msg(RD_ERR_STATE, "the last fetched chunk's buffer has been reused by a later submit");
    const int s = (int)(w->last & 1);
    HIPCHK(hipStreamWaitEvent(w->st_copy, w->e_chan[s], 0));
    HIPCHK(hipMemcpyAsync(out, w->d_out[s], need, hipMemcpyDeviceToHost, w->st_copy));
    HIPCHK(hipStreamSynchronize(w->st_copy));
    return RD_OK;
}

extern "C" int rd_wideband_copy_discriminated(rd_wideband *w, int channel, double *out, size_t n) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    return rd_copy_discriminated_stream(w->dem, channel, out, n);
}

extern "C" int rd_wideband_debug_advance_clock(rd_wideband *w, uint64_t n_out) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    if (n_out % 128) return rd_fail_msg(RD_ERR_ARG, "the clock moves in multiples of 128 output times");
    if (rd_demod_inflight(w->dem)) return rd_fail_msg(RD_ERR_STATE, "chunks in flight: fetch them first");
    w->clock += n_out;
    return RD_OK;
}
