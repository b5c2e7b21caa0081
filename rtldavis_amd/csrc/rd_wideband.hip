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
//
// Retune (rd_wb_retune; the definition: rd_channelizer.hip, RETUNE): new mixer frequencies for any channels from the next
// chunk boundary on, phase-continuous, with chunks in flight.  The call only records the wanted shifts; the next submit
// turns them into (shift, P) at its boundary t_b = clock - P' = (P + (s - s') t_b) mod Fo, exact integers - and queues
// the records of the channels that change and k_chan_retune on the compute stream in front of that chunk's k_channelize
// (the previous chunk's is earlier on the same stream, so one set of tables serves).  The records travel through a
// pinned slot of the chunk's parity: chunk k-2, the slot's last user, has been fetched or dropped - all its work is done.
// Before the first submit the tables are still the host's, and are rebuilt there.
//
// Gain (rd_wb_set_gain; rd_channelizer.hip, GAIN): the same pattern for the per-channel gains - the call records what is
// wanted, the next submit stages the table in the pinned slot of its parity and queues one copy in front of its
// k_channelize, only when an entry differs from what the table holds.
// Levels (rd_wb_set_levels / rd_wb_levels; rd_channelizer.hip, LEVELS): with levels on, k_chan_levels is queued behind the
// chunk's k_channelize (behind e_chan: the copy stream never waits for it) and writes its records into the mapped pinned
// slot of the chunk's parity.  The chunk's demodulator launch comes after it on the compute stream, so when a fetch has
// seen that launch report, the records are complete; the fetch copies them out of the slot, which chunk k+2 reuses.
// Spectrum (rd_wb_set_spectrum / rd_wb_spectrum; rd_spectrum.hip): with n_bins set, k_chan_spectrum is queued in the same
// place - behind e_chan, in front of the chunk's demodulator launch, beside k_chan_levels when both are on - and writes
// the record (header + n_bins doubles) into a mapped pinned slot of the chunk's parity, which the fetch copies out like
// the level records.  Both kernels READ d_wide[s] after the chunk's channelizer: that buffer is next overwritten by the
// copy of chunk k+2, which waits for e_chan of chunk k+1 - recorded later on the compute stream than either kernel of
// chunk k, so the copy cannot overtake them although they come behind chunk k's own e_chan.
// Bursts (rd_wb_set_bursts / rd_wb_bursts; rd_bursts.hip): with bursts on, k_chan_bursts is queued in the same place and
// writes its records into a mapped pinned slot of the chunk's parity, which the fetch copies out.  It reads d_out[s], the
// chunk's channelized bytes, like the chunk's demodulator launch behind it: d_out[s] is next written by the channelizer of
// chunk k+2, later on the same stream.  Its thresholds (rd_wb_set_burst_threshold: recorded by the call, in force from the
// next submit, like the gains) need no copy and no device table: the submit writes the table into the slot itself, which
// is free by the argument for the level slot, and the kernel reads it there - host writes made before the launch are
// visible to it - and echoes what it used in the floor records.
// Burst decode (rd_wb_set_burst_decode / rd_wb_burst_messages; rd_burst_decode.hip): with decode on, k_chan_burst_decode is
// queued behind k_chan_bursts, in front of the chunk's demodulator launch.  It reads the burst slot of the chunk's parity
// (written by the kernel in front of it), d_out[s] and, for a run that begins with the chunk, the end of d_out[s ^ 1]:
// chunk k-1's channelized bytes, next written by the channelizer of chunk k+1, later on the same stream.  Its records go
// into a mapped pinned slot of the chunk's parity, which the fetch copies out like the burst records.  Repair
// (rd_wb_set_burst_repair) is one integer the handle keeps and every submit hands to the launch, which picks the kernel
// instantiation by it: no table, no copy, and with 0 the launch of a receiver that never heard of it.  The narrow-band
// filter (rd_wb_set_burst_narrow) is one flag kept the same way and one device table (rd_bd_narrow_upload: 64 x (2 SL + 5)
// taps and the 64 centres, designed on the host) that the first submit with the flag set uploads, as the spectrum's tables
// are; the launch gets the table when the flag is set and a null pointer otherwise, and picks the instantiation by it.
// Burst expect (rd_wb_set_burst_expect / rd_wb_expected_messages; rd_burst_expect.hip): the table is host bookkeeping like
// the thresholds - recorded by the call, in force from the next submit.  The submit works out from the clock alone which
// expectations have candidates in the chunk (rd_burst_expect_stage) and writes them, as candidate ranges, into a mapped
// pinned slot of the chunk's parity - free by the argument for the level slot; host writes made before the launch are
// visible to it.  None active: nothing is launched, and the fetch reports zero records from the host's own note.
// Otherwise k_chan_burst_expect is queued behind k_chan_burst_decode and in front of the chunk's demodulator launch.  It
// reads d_out[s] and, below t = 0, the end of d_out[s ^ 1] under the same ordering as burst decode: chunk k-1's bytes are
// next written by the channelizer of chunk k+1, later on the same stream, and d_out[s] by that of chunk k+2.  Its records
// and headers go into the same slot, which the fetch copies out; step 7' runs there, against what the fetch of the chunk
// before delivered.
// Burst quality (rd_wb_set_burst_quality / rd_wb_burst_message_quality / rd_wb_expected_message_quality;
// rd_burst_quality.hip): a flag and the noise gap, kept like repair.  With it on, k_chan_burst_quality is queued behind
// k_chan_burst_decode over the decode slot and, when k_chan_burst_expect was launched, behind it over the expect slot; it
// reads what the kernel in front wrote into the mapped slot, d_out[s] and d_out[s ^ 1] under the ordering above, and
// writes into a mapped pinned slot of its own per parity ([n_ch][cap] | [RD_BX_MAX] records).  The fetch copies a quality
// record out with its message and drops it with it (steps 7 / 7').  It needs the narrow-band tables whenever
// symbol_length >= 4, whether or not the narrow decoder is on: the submit uploads them once.  Off: nothing is allocated,
// nothing launched, nothing copied.
// Burst search (rd_wb_set_burst_search / rd_wb_searched_messages; rd_burst_search.hip): the list of centres is host
// bookkeeping like the expect table - recorded by the call, in force from the next submit, which notes the list's size
// with the chunk's parity and hands the centres to the launch in the kernel's arguments.  k_chan_burst_search is queued
// behind k_chan_burst_expect (behind k_chan_burst_decode when that was not launched) and in front of the chunk's
// demodulator launch; it reads d_out[s] and the end of d_out[s ^ 1] under the ordering above and needs the narrow-band
// tables.  Its slot per parity ([8][n_ch][4] records | [8][n_ch] headers) is allocated by the first submit with a list in
// force; the fetch checks every header's chunk and runs step 7s.  An empty list: nothing allocated, launched or copied.
// Burst clips (rd_wb_set_burst_clips / rd_wb_burst_clips; rd_burst_clips.hip): a source mask, two rolls and a quota, kept
// like repair.  With a source set, k_chan_burst_clips is queued behind the chunk's last burst kernel and in front of its
// demodulator launch.  It reads, on the device, the burst, decode, expect and search slots of the chunk's parity that the
// kernels in front wrote (the expect and search slots only when their kernels were launched for this chunk), the headers
// of the OTHER parity's clip slot when chunk k-1 was submitted with clips on - written by that chunk's launch, earlier on
// the same stream; reset() forgets them -, d_out[s] and d_out[s ^ 1] under the ordering above, and writes records, headers
// and bytes into a mapped pinned slot of its own per parity, allocated by the first submit with clips in force (again
// when the quota grows: the receiver was quiet when it changed).  The fetch checks every header's chunk and copies out
// the records and only the used part of each channel's pool.  Off: nothing allocated, launched or copied.
#include <cstring>
#include <vector>
#include <unistd.h>

#include <hip/hip_runtime.h>

#include "rd_internal.h"

extern int rd_fail_msg(int code, const char *fmt, ...);  // rd_api.hip: sets rd_last_error

#define WCHK(x)                                                                                             \
    do {                                                                                                    \
        hipError_t e_ = (x);                                                                                \
        if (e_ != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "%s: %s", #x, hipGetErrorString(e_));      \
    } while (0)

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
    pid_t pid = 0;
    hipStream_t st = nullptr, st_copy = nullptr;   // the demodulator's streams
    uint8_t *h_in[2] = {nullptr, nullptr};         // pinned staging of the host's chunk
    uint8_t *d_wide[2] = {nullptr, nullptr};       // device chunk buffers
    uint8_t *d_out[2] = {nullptr, nullptr};        // channelized chunks [n_channels][2 B]
    hipEvent_t e_in[2] = {nullptr, nullptr};       // chunk buffer k & 1 copied
    hipEvent_t e_chan[2] = {nullptr, nullptr};     // chunk k's channelizer done
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
    // levels: on / off (switched on a quiet receiver: every chunk in flight has the same), the mapped pinned slots
    // [n_channels] rd_chan_level + one rd_input_level per parity, the kernel's device words, and the records the last
    // fetch kept
    bool levels = false, last_levels = false;
    rd_chan_level *h_lv[2] = {nullptr, nullptr};
    uint32_t *d_lvacc = nullptr;
    std::vector<rd_chan_level> lv_last;
    rd_input_level lv_in_last = {};
    // spectrum: bins per record (0: off; switched on a quiet receiver like levels), the kernel's tables and scratch, the
    // mapped pinned slots (header + sp_slot_n doubles) per parity, and the record the last fetch kept
    int spec_n = 0, sp_slot_n = 0;
    bool last_spec = false;
    rd_spec *spec = nullptr;
    uint8_t *h_sp[2] = {nullptr, nullptr};
    rd_spectrum_info sp_info_last = {};
    std::vector<double> sp_last;
    // bursts: on / off (switched on a quiet receiver like levels), the thresholds the next submitted chunk will use, the
    // mapped pinned slots per parity (rd_internal.h: rd_bu_slot_bytes) and the records the last fetch kept
    bool bursts = false, last_bursts = false;
    std::vector<uint32_t> thr;
    uint8_t *h_bu[2] = {nullptr, nullptr};
    std::vector<rd_burst> bu_last;
    std::vector<rd_burst_floor> bf_last;
    // burst decode: the demodulator's configuration (the kernel's symbol length, packet length and sync word), on / off
    // (switched on a quiet receiver; never on without bursts), the mapped pinned slots per parity (rd_internal.h:
    // rd_bd_slot_bytes) and the records the last fetch kept
    rd_config cfg = {};
    bool decode = false, last_decode = false;
    int repair = 0;                                // max_flips of the chunks submitted from now on (0 whenever decode is off)
    bool narrow = false;                           // step 4n for the chunks submitted from now on (false whenever decode is off)
    uint32_t *d_nb = nullptr;                      // its tables on the device, once a submit has needed them
    uint8_t *h_bd[2] = {nullptr, nullptr};
    std::vector<rd_burst_msg> bm_last;
    std::vector<uint32_t> bl_last;
    // step 7 of the definition: what the fetch of chunk bm_chunk delivered (bm_last), and during the next fetch what the
    // fetch before it delivered (bm_prev), against which a look-back record is a second report of the same packet
    std::vector<rd_burst_msg> bm_prev;
    long bm_chunk = -1;
    // burst expect: the table the next submitted chunk will use (empty whenever decode is off), the mapped pinned slots per
    // parity (rd_internal.h: RD_BX_SLOT_BYTES), what each parity's chunk was submitted with (its table's size, whether a
    // launch was made, the host's candidate counts), and the records the last fetch kept - step 7' as step 7 above
    std::vector<rd_expect> expect;
    uint8_t *h_bx[2] = {nullptr, nullptr};
    int bx_n[2] = {0, 0};
    bool bx_launched[2] = {false, false};
    uint32_t bx_cand[2][RD_BX_MAX] = {};
    std::vector<rd_burst_msg> xm_last, xm_prev;
    uint32_t xc_last[RD_BX_MAX] = {};
    long xm_chunk = -1;
    // burst search: the centres the next submitted chunk will use (empty whenever decode is off), the mapped pinned slots
    // per parity (rd_internal.h: rd_bs_slot_bytes; allocated when a list is first in force), the list each parity's chunk
    // was submitted with, and the records and headers the last fetch kept - step 7s as step 7 above
    std::vector<uint8_t> search;
    uint8_t *h_bs[2] = {nullptr, nullptr};
    int bs_n[2] = {0, 0};
    std::vector<rd_burst_msg> sm_last, sm_prev;
    std::vector<rd_bs_header> sh_last;
    long sm_chunk = -1;
    // burst quality: on / off and the noise gap of the chunks submitted from now on (off whenever decode is off), the
    // mapped pinned slots per parity (rd_internal.h: rd_bq_slot_bytes), and the rows the last fetch kept beside bm_last
    // and xm_last
    bool quality = false, last_quality = false;
    int q_gap = 0;
    uint8_t *h_bq[2] = {nullptr, nullptr};
    std::vector<rd_burst_quality> bq_last, xq_last;
    // burst clips: the settings of the chunks submitted from now on (sources 0: off; never on without bursts, RD_BC_MESSAGES
    // never without decode), the mapped pinned slots per parity (rd_internal.h: rd_bc_slot_bytes of bc_slot_quota), what
    // each parity's chunk was submitted with (its sources - 0: none, the slot holds no header of it - and quota), and the
    // records, packed bytes and drop counts the last fetch kept
    int bc_sources = 0, bc_pre = 256, bc_post = 128, bc_quota = 4096;
    int bc_slot_quota = 0;
    uint8_t *h_bc[2] = {nullptr, nullptr};
    int bc_sub[2] = {0, 0}, bc_sub_quota[2] = {0, 0};
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

// Make the channelizer's tables those of the next chunk's tuning: the channels that differ, on the host before the device
// tables exist, else as records in pinned slot `slot` and k_chan_retune on the compute stream.  Nothing differs: nothing queued.
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
    if (w->dev_ready && w->pid == getpid()) {
        for (int i = 0; i < 2; i++) {
            hipHostFree(w->h_in[i]); hipFree(w->d_wide[i]); hipFree(w->d_out[i]);
            if (w->e_in[i]) hipEventDestroy(w->e_in[i]);
            if (w->e_chan[i]) hipEventDestroy(w->e_chan[i]);
            hipHostFree(w->h_lv[i]);
            hipHostFree(w->h_sp[i]);
            hipHostFree(w->h_bu[i]);
            hipHostFree(w->h_bd[i]);
            hipHostFree(w->h_bx[i]);
            hipHostFree(w->h_bs[i]);
            hipHostFree(w->h_bq[i]);
            hipHostFree(w->h_bc[i]);
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
    w->pid = getpid();
    const size_t out_bytes = (size_t)w->n_ch * 2 * w->B + RD_INPUT_PAD;
    for (int i = 0; i < 2; i++) {
        WCHK(hipHostMalloc((void **)&w->h_in[i], w->chunk_bytes, hipHostMallocDefault));
        WCHK(hipMalloc(&w->d_wide[i], w->chunk_bytes + 16));
        WCHK(hipMalloc(&w->d_out[i], out_bytes));
        WCHK(hipEventCreateWithFlags(&w->e_in[i], hipEventDisableTiming));
        WCHK(hipEventCreateWithFlags(&w->e_chan[i], hipEventDisableTiming));
    }
    w->dev_ready = true;
    return RD_OK;
}

// the level records' slots and the kernel's words, when levels are first wanted
static size_t wb_lv_bytes(const rd_wideband *w) { return (size_t)w->n_ch * sizeof(rd_chan_level) + sizeof(rd_input_level); }
static int wb_alloc_levels(rd_wideband *w) {
    if (w->d_lvacc) return RD_OK;
    for (int i = 0; i < 2; i++)
        if (!w->h_lv[i]) {
            WCHK(hipHostMalloc((void **)&w->h_lv[i], wb_lv_bytes(w), hipHostMallocMapped));
            memset(w->h_lv[i], 0xFF, wb_lv_bytes(w));   // (no chunk has the sequence number 2^64 - 1)
        }
    uint32_t *acc = nullptr;
    WCHK(hipMalloc(&acc, RD_LV_ACC_WORDS * sizeof(uint32_t)));
    hipError_t e = hipMemsetAsync(acc, 0, RD_LV_ACC_WORDS * sizeof(uint32_t), w->st);   // (ordered before the first launch)
    if (e != hipSuccess) { hipFree(acc); return rd_fail_msg(RD_ERR_DEVICE, "hipMemsetAsync: %s", hipGetErrorString(e)); }
    w->d_lvacc = acc;
    return RD_OK;
}

// the spectrum's tables and scratch for the setting in force, and the two record slots (remade when n_bins changes:
// the receiver was quiet when it did, so nothing reads or writes the old ones)
static size_t wb_sp_bytes(int n) { return RD_SPEC_HDR_BYTES + (size_t)n * sizeof(double); }
static int wb_alloc_spectrum(rd_wideband *w) {
    const size_t samples = w->chunk_bytes / (size_t)rd_chan_bytes_per_sample(w->chan);
    int rc = rd_spec_prepare(&w->spec, w->spec_n, samples, w->st);
    if (rc || w->sp_slot_n == w->spec_n) return rc;
    for (int i = 0; i < 2; i++) {
        if (w->h_sp[i]) WCHK(hipHostFree(w->h_sp[i]));
        w->h_sp[i] = nullptr;
    }
    w->sp_slot_n = 0;
    for (int i = 0; i < 2; i++) {
        WCHK(hipHostMalloc((void **)&w->h_sp[i], wb_sp_bytes(w->spec_n), hipHostMallocMapped));
        memset(w->h_sp[i], 0xFF, RD_SPEC_HDR_BYTES);   // (no chunk has the sequence number 2^64 - 1)
    }
    w->sp_slot_n = w->spec_n;
    return RD_OK;
}

// the burst records' slots, when bursts are first wanted
static size_t wb_bu_windows(const rd_wideband *w) { return w->B / RD_BU_WINDOW; }
static rd_burst_floor *wb_bu_floor(const rd_wideband *w, int i) {
    return (rd_burst_floor *)(w->h_bu[i] + rd_bu_floor_offset(w->n_ch, wb_bu_windows(w)));
}
static int wb_alloc_bursts(rd_wideband *w) {
    for (int i = 0; i < 2; i++)
        if (!w->h_bu[i]) {
            WCHK(hipHostMalloc((void **)&w->h_bu[i], rd_bu_slot_bytes(w->n_ch, wb_bu_windows(w)), hipHostMallocMapped));
            memset(wb_bu_floor(w, i), 0xFF, (size_t)w->n_ch * sizeof(rd_burst_floor));   // (a run count no chunk can have)
        }
    return RD_OK;
}

// the decoded messages' slots, when decode is first wanted
static rd_bd_header *wb_bd_header(const rd_wideband *w, int i) {
    return (rd_bd_header *)(w->h_bd[i] + rd_bd_header_offset(w->n_ch, wb_bu_windows(w)));
}
static int wb_alloc_decode(rd_wideband *w) {
    for (int i = 0; i < 2; i++)
        if (!w->h_bd[i]) {
            WCHK(hipHostMalloc((void **)&w->h_bd[i], rd_bd_slot_bytes(w->n_ch, wb_bu_windows(w)), hipHostMallocMapped));
            memset(wb_bd_header(w, i), 0xFF, (size_t)w->n_ch * sizeof(rd_bd_header));   // (a message count no chunk can have)
        }
    for (int i = 0; i < 2; i++)
        if (!w->h_bx[i]) {
            WCHK(hipHostMalloc((void **)&w->h_bx[i], RD_BX_SLOT_BYTES, hipHostMallocMapped));
            memset(w->h_bx[i], 0xFF, RD_BX_SLOT_BYTES);
        }
    if (w->quality)
        for (int i = 0; i < 2; i++)
            if (!w->h_bq[i]) {
                WCHK(hipHostMalloc((void **)&w->h_bq[i], rd_bq_slot_bytes(w->n_ch, wb_bu_windows(w)), hipHostMallocMapped));
                memset(w->h_bq[i], 0xFF, rd_bq_slot_bytes(w->n_ch, wb_bu_windows(w)));
            }
    if (!w->search.empty())
        for (int i = 0; i < 2; i++)
            if (!w->h_bs[i]) {
                WCHK(hipHostMalloc((void **)&w->h_bs[i], rd_bs_slot_bytes(w->n_ch), hipHostMallocMapped));
                memset(w->h_bs[i], 0xFF, rd_bs_slot_bytes(w->n_ch));
            }
    if ((w->narrow || !w->search.empty() || (w->quality && w->cfg.symbol_length >= RD_BD_NB_MIN_SL)) && !w->d_nb)
        return rd_bd_narrow_upload(w->cfg.symbol_length, &w->d_nb);
    return RD_OK;
}

// the clip slots for the quota in force, when clips are first wanted.  Remade when the quota has grown: the receiver was
// quiet when it changed, so nothing reads or writes the old ones, and their headers - what the last chunk owes the next -
// are final and move into the new ones.
static int wb_alloc_clips(rd_wideband *w) {
    if (w->bc_slot_quota >= w->bc_quota) return RD_OK;
    const size_t ho = rd_bc_header_offset(w->n_ch), hb = (size_t)w->n_ch * sizeof(rd_bc_header);
    for (int i = 0; i < 2; i++) {
        uint8_t *slot = nullptr;
        WCHK(hipHostMalloc((void **)&slot, rd_bc_slot_bytes(w->n_ch, w->bc_quota), hipHostMallocMapped));
        if (w->h_bc[i]) {
            memcpy(slot + ho, w->h_bc[i] + ho, hb);
            hipHostFree(w->h_bc[i]);
        } else {
            memset(slot + ho, 0xFF, hb);                  // (a clip count no chunk can have)
        }
        w->h_bc[i] = slot;
    }
    w->bc_slot_quota = w->bc_quota;
    return RD_OK;
}

extern "C" int rd_wideband_reset(rd_wideband *w) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    int rc = rd_reset(w->dem);   // waits for the chunks in flight: their channelizers ran before their demod launches
    if (rc) return rc;
    w->clock = 0;
    w->n_sub = 0;                // (no previous chunk: zero history)
    w->last = -1;
    w->shift = w->plan;          // a pending retune is dropped; the next submit rebuilds what the tables hold otherwise
    w->phase.assign(w->n_ch, 0);
    w->pending = false;
    w->restored = true;
    w->gain.assign(w->n_ch, w->gain0);   // a pending gain change is dropped; the next submit rewrites the table if it differs
    w->last_levels = false;
    for (int i = 0; i < 2; i++)   // (chunk numbers restart: no record of the run before may pass for one of this run)
        if (w->h_lv[i]) memset(w->h_lv[i], 0xFF, wb_lv_bytes(w));
    w->last_spec = false;         // (the setting stays; the record of the run before goes)
    for (int i = 0; i < 2; i++)
        if (w->h_sp[i]) memset(w->h_sp[i], 0xFF, RD_SPEC_HDR_BYTES);
    w->thr.assign(w->n_ch, RD_BU_THR_DEFAULT);   // a pending threshold change is dropped
    w->last_bursts = false;
    for (int i = 0; i < 2; i++)
        if (w->h_bu[i]) memset(wb_bu_floor(w, i), 0xFF, (size_t)w->n_ch * sizeof(rd_burst_floor));
    w->last_quality = false;      // (the setting stays)
    w->last_decode = false;       // (the setting stays; n_sub = 0: the first chunk has no look-back)
    w->bm_chunk = -2;             // (... and no chunk before it whose records its own could repeat: -2, for the fetch of
    w->bm_prev.clear();           //  chunk 0 looks for chunk -1 and must not take the run before for it)
    for (int i = 0; i < 2; i++)
        if (w->h_bd[i]) memset(wb_bd_header(w, i), 0xFF, (size_t)w->n_ch * sizeof(rd_bd_header));
    w->expect.clear();            // (the windows refer to the clock that has just restarted)
    w->xm_chunk = -2;             // (as bm_chunk: an expected record of chunk 0 repeats nothing of the run before)
    w->xm_prev.clear();
    for (int i = 0; i < 2; i++) {
        w->bx_n[i] = 0;
        w->bx_launched[i] = false;
        if (w->h_bx[i]) memset(w->h_bx[i], 0xFF, RD_BX_SLOT_BYTES);
        if (w->h_bq[i]) memset(w->h_bq[i], 0xFF, rd_bq_slot_bytes(w->n_ch, wb_bu_windows(w)));
        w->bs_n[i] = 0;               // (the search list stays; what step 7s remembers goes)
        if (w->h_bs[i]) memset(w->h_bs[i], 0xFF, rd_bs_slot_bytes(w->n_ch));
    }
    w->sm_chunk = -2;
    w->sm_prev.clear();
    w->last_clips = false;        // (the settings stay; what the run before owed goes)
    for (int i = 0; i < 2; i++) {
        w->bc_sub[i] = 0;
        if (w->h_bc[i]) memset(w->h_bc[i] + rd_bc_header_offset(w->n_ch), 0xFF, (size_t)w->n_ch * sizeof(rd_bc_header));
    }
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

extern "C" int rd_wb_set_levels(rd_wideband *w, int enabled) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    if (rd_demod_inflight(w->dem))
        return rd_fail_msg(RD_ERR_STATE, "%d chunk(s) in flight: fetch them before levels are switched", rd_demod_inflight(w->dem));
    w->levels = enabled != 0;
    return RD_OK;
}

extern "C" int rd_wb_levels(rd_wideband *w, rd_chan_level *out, int n, rd_input_level *in) {
    if (!w || !out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (n != w->n_ch) return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: room for %d channels of %d", n, w->n_ch);
    if (w->last < 0) return rd_fail_msg(RD_ERR_STATE, "no chunk fetched since create / reset");
    if (!w->last_levels) return rd_fail_msg(RD_ERR_STATE, "the last fetched chunk was submitted with levels off (rd_wb_set_levels)");
    memcpy(out, w->lv_last.data(), (size_t)n * sizeof(rd_chan_level));
    if (in) *in = w->lv_in_last;
    return RD_OK;
}

extern "C" int rd_wb_set_spectrum(rd_wideband *w, int n_bins) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    if (rd_demod_inflight(w->dem))
        return rd_fail_msg(RD_ERR_STATE, "%d chunk(s) in flight: fetch them before the spectrum is switched", rd_demod_inflight(w->dem));
    if (n_bins != 0) {
        int rc = rd_spec_check(n_bins, w->chunk_bytes / (size_t)rd_chan_bytes_per_sample(w->chan));
        if (rc) return rc;
    }
    w->spec_n = n_bins;
    return RD_OK;
}

extern "C" int rd_wb_spectrum(rd_wideband *w, double *power, int n_bins, rd_spectrum_info *info) {
    if (!w || !power) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (w->last < 0) return rd_fail_msg(RD_ERR_STATE, "no chunk fetched since create / reset");
    if (!w->last_spec) return rd_fail_msg(RD_ERR_STATE, "the last fetched chunk was submitted with the spectrum off (rd_wb_set_spectrum)");
    if (n_bins != (int)w->sp_info_last.n_bins)
        return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: room for %d bins of %u", n_bins, w->sp_info_last.n_bins);
    memcpy(power, w->sp_last.data(), (size_t)n_bins * sizeof(double));
    if (info) *info = w->sp_info_last;
    return RD_OK;
}

extern "C" int rd_wb_set_bursts(rd_wideband *w, int enabled) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    if (rd_demod_inflight(w->dem))
        return rd_fail_msg(RD_ERR_STATE, "%d chunk(s) in flight: fetch them before bursts are switched", rd_demod_inflight(w->dem));
    if (enabled) {
        int rc = rd_bursts_check(w->B);
        if (rc) return rc;
    }
    w->bursts = enabled != 0;
    if (!w->bursts) {                    // (the decoder reads the burst records)
        w->decode = false;
        w->repair = 0;
        w->narrow = false;
        w->quality = false;
        w->expect.clear();
        w->search.clear();
        w->bc_sources = 0;
    }
    return RD_OK;
}

extern "C" int rd_wb_set_burst_decode(rd_wideband *w, int enabled) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    if (rd_demod_inflight(w->dem))
        return rd_fail_msg(RD_ERR_STATE, "%d chunk(s) in flight: fetch them before burst decode is switched", rd_demod_inflight(w->dem));
    if (enabled) {
        if (!w->bursts) return rd_fail_msg(RD_ERR_STATE, "burst decode needs bursts on (rd_wb_set_bursts)");
        int rc = rd_burst_decode_check(&w->cfg);
        if (rc) return rc;
    }
    w->decode = enabled != 0;
    if (!w->decode) {
        w->repair = 0;
        w->narrow = false;
        w->quality = false;
        w->expect.clear();
        w->search.clear();
        w->bc_sources &= ~(int)RD_BC_MESSAGES;   // (clips of runs go on; nothing left: off)
    }
    return RD_OK;
}

extern "C" int rd_wb_set_burst_repair(rd_wideband *w, int max_flips) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    if (max_flips < 0 || max_flips > RD_BD_MAX_FLIPS)
        return rd_fail_msg(RD_ERR_ARG, "burst repair: max_flips %d, not 0 .. %d", max_flips, RD_BD_MAX_FLIPS);
    if (rd_demod_inflight(w->dem))
        return rd_fail_msg(RD_ERR_STATE, "%d chunk(s) in flight: fetch them before burst repair is switched", rd_demod_inflight(w->dem));
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
    if (rd_demod_inflight(w->dem))
        return rd_fail_msg(RD_ERR_STATE, "%d chunk(s) in flight: fetch them before the narrow-band filter is switched", rd_demod_inflight(w->dem));
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
    if (rd_demod_inflight(w->dem))
        return rd_fail_msg(RD_ERR_STATE, "%d chunk(s) in flight: fetch them before burst quality is switched", rd_demod_inflight(w->dem));
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
    if (!w || !n || cap < 0 || (!out && cap > 0)) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (w->last < 0) return rd_fail_msg(RD_ERR_STATE, "no chunk fetched since create / reset");
    if (!w->last_quality) return rd_fail_msg(RD_ERR_STATE, "the last fetched chunk was submitted with burst quality off (rd_wb_set_burst_quality)");
    *n = (int)rows.size();
    if (cap < *n) return rd_fail_msg(RD_ERR_CAPACITY, "%d quality records, room for %d", *n, cap);
    if (*n) memcpy(out, rows.data(), (size_t)*n * sizeof(rd_burst_quality));
    return RD_OK;
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
    if (!w || !n || cap < 0 || (!out && cap > 0)) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (long_runs && n_channels != w->n_ch)
        return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: room for %d long-run counts of %d", n_channels, w->n_ch);
    if (w->last < 0) return rd_fail_msg(RD_ERR_STATE, "no chunk fetched since create / reset");
    if (!w->last_decode) return rd_fail_msg(RD_ERR_STATE, "the last fetched chunk was submitted with burst decode off (rd_wb_set_burst_decode)");
    *n = (int)w->bm_last.size();
    if (long_runs) memcpy(long_runs, w->bl_last.data(), (size_t)w->n_ch * sizeof(uint32_t));
    if (cap < *n) return rd_fail_msg(RD_ERR_CAPACITY, "%d burst messages, room for %d", *n, cap);
    if (*n) memcpy(out, w->bm_last.data(), (size_t)*n * sizeof(rd_burst_msg));
    return RD_OK;
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
    if (!w || !n || cap < 0 || (!out && cap > 0)) return rd_fail_msg(RD_ERR_ARG, "null argument");
    *n = (int)w->expect.size();
    if (cap < *n) return rd_fail_msg(RD_ERR_CAPACITY, "%d expectations, room for %d", *n, cap);
    if (*n) memcpy(out, w->expect.data(), (size_t)*n * sizeof(rd_expect));
    return RD_OK;
}

extern "C" int rd_wb_expected_messages(rd_wideband *w, rd_burst_msg *out, int cap, int *n, uint32_t *candidates, int n_cand) {
    if (!w || !n || cap < 0 || (!out && cap > 0)) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (candidates && n_cand != RD_BX_MAX)
        return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: room for %d candidate counts of %d", n_cand, RD_BX_MAX);
    if (w->last < 0) return rd_fail_msg(RD_ERR_STATE, "no chunk fetched since create / reset");
    if (!w->last_decode) return rd_fail_msg(RD_ERR_STATE, "the last fetched chunk was submitted with burst decode off (rd_wb_set_burst_decode)");
    *n = (int)w->xm_last.size();
    if (candidates) memcpy(candidates, w->xc_last, sizeof w->xc_last);
    if (cap < *n) return rd_fail_msg(RD_ERR_CAPACITY, "%d expected messages, room for %d", *n, cap);
    if (*n) memcpy(out, w->xm_last.data(), (size_t)*n * sizeof(rd_burst_msg));
    return RD_OK;
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
    if (!w || !n || cap < 0 || (!out && cap > 0)) return rd_fail_msg(RD_ERR_ARG, "null argument");
    *n = (int)w->search.size();
    if (cap < *n) return rd_fail_msg(RD_ERR_CAPACITY, "%d centres, room for %d", *n, cap);
    if (*n) memcpy(out, w->search.data(), (size_t)*n);
    return RD_OK;
}

extern "C" int rd_wb_searched_messages(rd_wideband *w, rd_burst_msg *out, int cap, int *n, rd_bs_header *hdr, int n_hdr) {
    if (!w || !n || cap < 0 || (!out && cap > 0)) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (hdr && n_hdr != RD_BS_MAX_CENTRES * w->n_ch)
        return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: room for %d headers of %d", n_hdr, RD_BS_MAX_CENTRES * w->n_ch);
    if (w->last < 0) return rd_fail_msg(RD_ERR_STATE, "no chunk fetched since create / reset");
    if (!w->last_decode) return rd_fail_msg(RD_ERR_STATE, "the last fetched chunk was submitted with burst decode off (rd_wb_set_burst_decode)");
    *n = (int)w->sm_last.size();
    if (hdr) {
        memset(hdr, 0xFF, (size_t)n_hdr * sizeof(rd_bs_header));
        if (!w->sh_last.empty()) memcpy(hdr, w->sh_last.data(), w->sh_last.size() * sizeof(rd_bs_header));
    }
    if (cap < *n) return rd_fail_msg(RD_ERR_CAPACITY, "%d searched messages, room for %d", *n, cap);
    if (*n) memcpy(out, w->sm_last.data(), (size_t)*n * sizeof(rd_burst_msg));
    return RD_OK;
}

extern "C" int rd_wb_set_burst_clips(rd_wideband *w, int sources, int pre, int post, int quota) {
    if (!w) return rd_fail_msg(RD_ERR_ARG, "null handle");
    int rc = rd_burst_clips_check(w->n_ch, sources, pre, post, quota);
    if (rc) return rc;
    if (rd_demod_inflight(w->dem))
        return rd_fail_msg(RD_ERR_STATE, "%d chunk(s) in flight: fetch them before burst clips are switched", rd_demod_inflight(w->dem));
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

extern "C" int rd_wb_burst_clips(rd_wideband *w, rd_burst_clip *out, int cap, int *n, uint8_t *bytes, size_t bytes_cap, size_t *n_bytes,
                                 uint32_t *dropped, int n_channels) {
    if (!w || !n || !n_bytes || cap < 0 || (!out && cap > 0) || (!bytes && bytes_cap > 0)) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (dropped && n_channels != w->n_ch)
        return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: room for %d drop counts of %d", n_channels, w->n_ch);
    if (w->last < 0) return rd_fail_msg(RD_ERR_STATE, "no chunk fetched since create / reset");
    if (!w->last_clips) return rd_fail_msg(RD_ERR_STATE, "the last fetched chunk was submitted with burst clips off (rd_wb_set_burst_clips)");
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
    if (!w || !n || cap < 0 || (!out && cap > 0)) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (floor && n_floor != w->n_ch)
        return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: room for %d floor records of %d", n_floor, w->n_ch);
    if (w->last < 0) return rd_fail_msg(RD_ERR_STATE, "no chunk fetched since create / reset");
    if (!w->last_bursts) return rd_fail_msg(RD_ERR_STATE, "the last fetched chunk was submitted with bursts off (rd_wb_set_bursts)");
    *n = (int)w->bu_last.size();
    if (floor) memcpy(floor, w->bf_last.data(), (size_t)w->n_ch * sizeof(rd_burst_floor));
    if (cap < *n) return rd_fail_msg(RD_ERR_CAPACITY, "%d burst records, room for %d", *n, cap);
    if (*n) memcpy(out, w->bu_last.data(), (size_t)*n * sizeof(rd_burst));
    return RD_OK;
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

extern "C" int rd_wideband_submit(rd_wideband *w, const void *wide_iq, size_t nbytes) {
    if (!w || !wide_iq) return rd_fail_msg(RD_ERR_ARG, "null argument");
    if (nbytes != w->chunk_bytes)
        return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: got %zu bytes, expected %zu", nbytes, w->chunk_bytes);
    int rc = RD_OK;
    if (!w->dev_ready && (rc = wb_apply_tuning(w, 0))) return rc;   // (the tables are still the host's)
    rc = wb_alloc(w);
    if (rc) return rc;
    if (w->levels && (rc = wb_alloc_levels(w))) return rc;
    if (w->spec_n && (rc = wb_alloc_spectrum(w))) return rc;
    if (w->bursts && (rc = wb_alloc_bursts(w))) return rc;
    if (w->decode && (rc = wb_alloc_decode(w))) return rc;
    if (w->bursts && w->bc_sources && (rc = wb_alloc_clips(w))) return rc;
    rc = rd_demod_check_room(w->dem);   // a third chunk is refused before anything is queued
    if (rc) return rc;
    const int s = (int)(w->n_sub & 1);
    // the pinned slot's previous copy (chunk k-2) has completed: its demod block has been fetched or dropped
    if (w->n_sub >= 2) WCHK(hipEventSynchronize(w->e_in[s]));
    memcpy(w->h_in[s], wide_iq, nbytes);
    // buffer s holds chunk k-2, the history chunk k-1's channelizer reads: overwrite it once that has run
    if (w->n_sub >= 1) WCHK(hipStreamWaitEvent(w->st_copy, w->e_chan[s ^ 1], 0));
    WCHK(hipMemcpyAsync(w->d_wide[s], w->h_in[s], nbytes, hipMemcpyHostToDevice, w->st_copy));
    WCHK(hipEventRecord(w->e_in[s], w->st_copy));
    // Pinned record slot s was last used by chunk k-2, whose records were copied on the COMPUTE stream: e_in[s] above (the
    // copy stream's event) does not order that copy.  The slot is free because rd_demod_check_room refuses a third chunk:
    // chunk k-2 has been fetched, or waited for as stale, so all its work on the compute stream is done.  Whoever relaxes
    // that limit must give the slot an event of its own.
    if ((rc = wb_apply_tuning(w, s))) return rc;
    if ((rc = rd_chan_stream_gains(w->chan, w->gain.data(), s, w->st))) return rc;   // (its own slot s, free by the same argument)
    WCHK(hipStreamWaitEvent(w->st, w->e_in[s], 0));
    rc = rd_chan_stream_launch(w->chan, w->d_wide[s], w->n_sub >= 1 ? w->d_wide[s ^ 1] : nullptr, w->B, w->clock,
                               w->d_out[s], 2 * w->B, w->st);
    if (rc) return rc;
    WCHK(hipEventRecord(w->e_chan[s], w->st));
    if (w->levels) {
        // level slot s was last written for chunk k-2 and read by its fetch (or the chunk was dropped): free, as above
        rd_chan_level *lv = nullptr;
        WCHK(hipHostGetDevicePointer((void **)&lv, w->h_lv[s], 0));
        rc = rd_chan_stream_levels(w->chan, w->d_wide[s], w->B, w->d_out[s], 2 * w->B, (uint64_t)w->n_sub, lv,
                                   (rd_input_level *)(lv + w->n_ch), w->d_lvacc, w->st);
        if (rc) return rc;
    }
    if (w->spec_n) {
        // spectrum slot s: free by the argument for the level slot; the kernel reads d_wide[s] only (header comment)
        void *sp = nullptr;
        WCHK(hipHostGetDevicePointer(&sp, w->h_sp[s], 0));
        rc = rd_spec_launch(w->spec, w->d_wide[s], rd_chan_format(w->chan), w->chunk_bytes / (size_t)rd_chan_bytes_per_sample(w->chan),
                            (uint64_t)w->n_sub, sp, w->st);
        if (rc) return rc;
    }
    w->bc_sub[s] = 0;   // (whatever chunk k-2 was submitted with: this chunk has clips only once its launch is queued below)
    if (w->bursts) {
        // burst slot s: free by the argument for the level slot; the thresholds travel in it (header comment)
        memcpy(w->h_bu[s] + rd_bu_thr_offset(w->n_ch, wb_bu_windows(w)), w->thr.data(), (size_t)w->n_ch * sizeof(uint32_t));
        void *bu = nullptr;
        WCHK(hipHostGetDevicePointer(&bu, w->h_bu[s], 0));
        rc = rd_bursts_launch(w->d_out[s], 2 * w->B, w->n_ch, w->B, (uint64_t)w->n_sub, bu, w->st);
        if (rc) return rc;
        void *bd = nullptr, *bx_used = nullptr, *bs_used = nullptr;   // what the clip kernel may read: the slots written for this chunk
        if (w->decode) {
            // decode slot s: free by the argument for the level slot; d_out[s ^ 1] holds chunk k-1 (header comment)
            WCHK(hipHostGetDevicePointer(&bd, w->h_bd[s], 0));
            rc = rd_burst_decode_launch(&w->cfg, w->d_out[s], w->n_sub >= 1 ? w->d_out[s ^ 1] : nullptr, 2 * w->B, w->n_ch, w->B,
                                        w->clock, (uint64_t)w->n_sub, w->repair, w->narrow ? w->d_nb : nullptr, bu, bd, w->st);
            if (rc) return rc;
            // quality slot s: free by the argument for the level slot; the decode slot is read on the device (header comment)
            rd_burst_quality *bq = nullptr;
            const size_t q_cap = rd_bu_cap(wb_bu_windows(w));
            const uint8_t *q_prev = w->n_sub >= 1 ? w->d_out[s ^ 1] : nullptr;
            if (w->quality) {
                WCHK(hipHostGetDevicePointer((void **)&bq, w->h_bq[s], 0));
                rc = rd_burst_quality_launch(&w->cfg, w->d_out[s], q_prev, 2 * w->B, w->n_ch, w->B, w->q_gap, w->d_nb, (const rd_burst_msg *)bd,
                                             q_cap, (const rd_bq_header *)((uint8_t *)bd + rd_bd_header_offset(w->n_ch, wb_bu_windows(w))),
                                             w->n_ch, bq, w->st);
                if (rc) return rc;
            }
            // expect slot s: free by the argument for the level slot; the candidate ranges travel in it (header comment)
            const int nx = (int)w->expect.size();
            w->bx_n[s] = nx;
            w->bx_launched[s] = false;
            if (nx && rd_burst_expect_stage(&w->cfg, w->n_sub >= 1 ? 1 : 0, w->clock, w->expect.data(), nx, w->h_bx[s], w->bx_cand[s]) > 0) {
                void *bx = nullptr;
                WCHK(hipHostGetDevicePointer(&bx, w->h_bx[s], 0));
                rc = rd_burst_expect_launch(&w->cfg, w->d_out[s], w->n_sub >= 1 ? w->d_out[s ^ 1] : nullptr, 2 * w->B, w->n_ch, w->B,
                                            w->clock, (uint64_t)w->n_sub, nx, w->repair, w->narrow ? w->d_nb : nullptr, bx, w->st);
                if (rc) return rc;
                w->bx_launched[s] = true;
                bx_used = bx;
                if (w->quality) {
                    rc = rd_burst_quality_launch(&w->cfg, w->d_out[s], q_prev, 2 * w->B, w->n_ch, w->B, w->q_gap, w->d_nb, (const rd_burst_msg *)bx,
                                                 1, (const rd_bq_header *)((uint8_t *)bx + RD_BX_HEADER_OFFSET), nx,
                                                 bq + (size_t)w->n_ch * q_cap, w->st);
                    if (rc) return rc;
                }
            }
            // search slot s: free by the argument for the level slot; the centres travel in the kernel's arguments
            const int ns = (int)w->search.size();
            w->bs_n[s] = ns;
            if (ns) {
                void *bs = nullptr;
                WCHK(hipHostGetDevicePointer(&bs, w->h_bs[s], 0));
                rc = rd_burst_search_launch(&w->cfg, w->d_out[s], w->n_sub >= 1 ? w->d_out[s ^ 1] : nullptr, 2 * w->B, w->n_ch, w->B,
                                            w->clock, (uint64_t)w->n_sub, w->search.data(), ns, w->d_nb, bs, w->st);
                if (rc) return rc;
                bs_used = bs;
            }
        }
        if (w->bc_sources) {
            // clip slot s: free by the argument for the level slot; slot s ^ 1 holds chunk k-1's headers when that chunk
            // had clips on, written by its launch earlier on this stream (header comment)
            void *bc = nullptr, *bc_prev = nullptr;
            WCHK(hipHostGetDevicePointer(&bc, w->h_bc[s], 0));
            if (w->n_sub >= 1 && w->bc_sub[s ^ 1]) {
                WCHK(hipHostGetDevicePointer(&bc_prev, w->h_bc[s ^ 1], 0));
                bc_prev = (uint8_t *)bc_prev + rd_bc_header_offset(w->n_ch);
            }
            rc = rd_burst_clips_launch(&w->cfg, w->d_out[s], w->n_sub >= 1 ? w->d_out[s ^ 1] : nullptr, 2 * w->B, w->n_ch, w->B, w->clock,
                                       (uint64_t)w->n_sub, w->bc_sources, w->bc_pre, w->bc_post, w->bc_quota, bu, bd, bx_used,
                                       bx_used ? w->bx_n[s] : 0, bs_used, bs_used ? w->bs_n[s] : 0, (const rd_bc_header *)bc_prev, bc,
                                       w->st);
            if (rc) return rc;
            w->bc_sub[s] = w->bc_sources;
            w->bc_sub_quota[s] = w->bc_quota;
        }
    }
    w->clock += w->B;
    w->n_sub++;
    return rd_demod_submit_device(w->dem, w->d_out[s]);
}

static int wb_fetched(rd_wideband *w, int rc) {
    if (rc != RD_OK && rc != RD_ERR_CAPACITY) return rc;
    w->last = w->n_sub - 1 - rd_demod_pending(w->dem);  // (the oldest in flight)
    w->last_levels = false;
    w->last_spec = false;
    w->last_bursts = false;
    w->last_decode = false;
    w->last_quality = false;
    w->last_clips = false;
    if (w->bc_sub[w->last & 1]) {
        // as the burst records below: k_chan_burst_clips ran before the demodulator launch that has reported.  Every header
        // carries the chunk's number; a channel's clips are the first n_clips of its record places, its bytes the first
        // 2 * used of its pool - only those are copied, packed channel after channel, and `offset` is rewritten to match.
        const int sc = (int)(w->last & 1);
        const size_t q = (size_t)w->bc_sub_quota[sc];
        const rd_burst_clip *recs = (const rd_burst_clip *)w->h_bc[sc];
        const rd_bc_header *hd = (const rd_bc_header *)(w->h_bc[sc] + rd_bc_header_offset(w->n_ch));
        const uint8_t *pool = w->h_bc[sc] + rd_bc_pool_offset(w->n_ch);
        w->bc_last.clear();
        w->bc_bytes_last.clear();
        w->bc_dropped_last.assign(w->n_ch, 0u);
        for (int c = 0; c < w->n_ch; c++) {
            const rd_bc_header h = hd[c];
            if (h.chunk != (uint32_t)w->last || h.n_clips > (uint32_t)RD_BC_PER || h.used > q)
                return rd_fail_msg(RD_ERR_DEVICE, "clip header of channel %d belongs to chunk %u (%u clips, %u outputs), not %ld", c, h.chunk,
                                   h.n_clips, h.used, w->last);
            w->bc_dropped_last[c] = h.dropped;
            const size_t base = w->bc_bytes_last.size() / 2;   // outputs packed so far
            for (uint32_t i = 0; i < h.n_clips; i++) {
                rd_burst_clip k = recs[(size_t)c * RD_BC_PER + i];
                if ((size_t)k.offset + k.n > h.used)
                    return rd_fail_msg(RD_ERR_DEVICE, "clip %u of channel %d lies at %u + %u of %u outputs", i, c, k.offset, k.n, h.used);
                k.offset = (uint32_t)(base + k.offset);
                w->bc_last.push_back(k);
            }
            w->bc_bytes_last.insert(w->bc_bytes_last.end(), pool + (size_t)c * 2 * q, pool + (size_t)c * 2 * q + 2 * (size_t)h.used);
        }
        w->last_clips = true;
    }
    if (w->decode) {
        // as the burst records below: k_chan_burst_decode ran before the demodulator launch that has reported.  Every
        // header carries the chunk's number; a channel's messages are the first n_msgs of its record places.
        const size_t cap_c = rd_bu_cap(wb_bu_windows(w));
        const rd_burst_msg *recs = (const rd_burst_msg *)w->h_bd[w->last & 1];
        const rd_bd_header *hd = wb_bd_header(w, (int)(w->last & 1));
        // quality on: record i of the quality slot belongs to record i of the message slot, and goes where it goes
        const rd_burst_quality *qrecs = w->quality ? (const rd_burst_quality *)w->h_bq[w->last & 1] : nullptr;
        w->bq_last.clear();
        w->xq_last.clear();
        // Step 7 (include/rtldavis_hip.h, BURST DECODE): a look-back record that repeats - same channel, same data, less
        // than SL outputs apart - a record the fetch of the chunk before DELIVERED is the second report of a packet that
        // ends at the boundary, and is dropped.  A chunk that was never fetched delivered nothing.
        if (w->bm_chunk == w->last - 1) w->bm_prev.swap(w->bm_last);
        else w->bm_prev.clear();
        w->bm_chunk = -1;
        w->bm_last.clear();
        w->bl_last.assign(w->n_ch, 0u);
        for (int c = 0; c < w->n_ch; c++) {
            const rd_bd_header h = hd[c];
            if (h.chunk != (uint32_t)w->last || h.n_msgs > cap_c)
                return rd_fail_msg(RD_ERR_DEVICE, "burst message header of channel %d belongs to chunk %u (%u messages), not %ld", c,
                                   h.chunk, h.n_msgs, w->last);
            w->bl_last[c] = h.long_runs;
            for (uint32_t i = 0; i < h.n_msgs; i++) {
                const rd_burst_msg m = recs[(size_t)c * cap_c + i];
                if (rd_bd_repeats(m, w->bm_prev.data(), w->bm_prev.size(), w->cfg.symbol_length)) continue;
                w->bm_last.push_back(m);
                if (qrecs) {
                    const rd_burst_quality q = qrecs[(size_t)c * cap_c + i];
                    if (q.chunk != (uint32_t)w->last)
                        return rd_fail_msg(RD_ERR_DEVICE, "quality record %u of channel %d belongs to chunk %u, not %ld", i, c, q.chunk, w->last);
                    w->bq_last.push_back(q);
                }
            }
        }
        w->bm_chunk = w->last;
        // Burst expect: the slot's headers and records when the chunk's submit launched the kernel, else nothing.  Step 7'
        // (include/rtldavis_hip.h, BURST EXPECT) against what the fetch of the chunk before delivered.
        const int sx = (int)(w->last & 1), nx = w->bx_n[sx];
        if (w->xm_chunk == w->last - 1) w->xm_prev.swap(w->xm_last);
        else w->xm_prev.clear();
        w->xm_chunk = -1;
        w->xm_last.clear();
        for (int i = 0; i < RD_BX_MAX; i++) w->xc_last[i] = i < nx ? 0u : RD_BX_NO_ENTRY;
        if (nx && w->bx_launched[sx]) {
            const rd_burst_msg *xr = (const rd_burst_msg *)w->h_bx[sx];
            const rd_bx_header *xh = (const rd_bx_header *)(w->h_bx[sx] + RD_BX_HEADER_OFFSET);
            for (int i = 0; i < nx; i++) {
                const rd_bx_header h = xh[i];
                if (h.chunk != (uint32_t)w->last || h.n_msgs > 1u || h.candidates != w->bx_cand[sx][i])
                    return rd_fail_msg(RD_ERR_DEVICE, "expectation %d: header of chunk %u (%u messages, %u candidates), not of chunk %ld with %u candidates",
                                       i, h.chunk, h.n_msgs, h.candidates, w->last, w->bx_cand[sx][i]);
                w->xc_last[i] = h.candidates;
                if (!h.n_msgs || rd_bx_repeats(xr[i], w->xm_prev.data(), w->xm_prev.size(), w->cfg.symbol_length)) continue;
                w->xm_last.push_back(xr[i]);
                if (qrecs) {
                    const rd_burst_quality q = qrecs[(size_t)w->n_ch * cap_c + (size_t)i];
                    if (q.chunk != (uint32_t)w->last)
                        return rd_fail_msg(RD_ERR_DEVICE, "quality record of expectation %d belongs to chunk %u, not %ld", i, q.chunk, w->last);
                    w->xq_last.push_back(q);
                }
            }
        }
        w->xm_chunk = w->last;
        // Burst search: the headers and records of the list the chunk was submitted with.  Step 7s (include/rtldavis_hip.h,
        // BURST SEARCH) against what the fetch of the chunk before delivered.
        const int nsr = w->bs_n[sx];
        if (w->sm_chunk == w->last - 1) w->sm_prev.swap(w->sm_last);
        else w->sm_prev.clear();
        w->sm_chunk = -1;
        w->sm_last.clear();
        w->sh_last.clear();
        if (nsr) {
            const rd_burst_msg *sr = (const rd_burst_msg *)w->h_bs[sx];
            const rd_bs_header *sh = (const rd_bs_header *)(w->h_bs[sx] + rd_bs_header_offset(w->n_ch));
            w->sh_last.assign(sh, sh + (size_t)nsr * (size_t)w->n_ch);
            for (int i = 0; i < nsr; i++)
                for (int c = 0; c < w->n_ch; c++) {
                    const rd_bs_header h = w->sh_last[(size_t)i * (size_t)w->n_ch + (size_t)c];
                    if (h.chunk != (uint32_t)w->last || h.n_msgs > (uint32_t)RD_BS_PER)
                        return rd_fail_msg(RD_ERR_DEVICE, "search header of centre %d, channel %d belongs to chunk %u (%u messages), not %ld",
                                           i, c, h.chunk, h.n_msgs, w->last);
                    for (uint32_t r = 0; r < h.n_msgs; r++) {
                        const rd_burst_msg m = sr[((size_t)i * (size_t)w->n_ch + (size_t)c) * RD_BS_PER + r];
                        if (!rd_bs_repeats(m, w->sm_prev.data(), w->sm_prev.size(), w->cfg.symbol_length)) w->sm_last.push_back(m);
                    }
                }
        }
        w->sm_chunk = w->last;
        w->last_decode = true;
        w->last_quality = w->quality;
    }
    if (w->bursts) {
        // as the level records below: k_chan_bursts ran before the demodulator launch that has reported.  Every floor
        // record carries the chunk's number; a channel's runs are the first n_bursts of its record places.
        const size_t cap_c = rd_bu_cap(wb_bu_windows(w));
        const rd_burst *recs = (const rd_burst *)w->h_bu[w->last & 1];
        const rd_burst_floor *fl = wb_bu_floor(w, (int)(w->last & 1));
        w->bf_last.assign(fl, fl + w->n_ch);
        w->bu_last.clear();
        for (int c = 0; c < w->n_ch; c++) {
            if (w->bf_last[c].chunk != (uint32_t)w->last || w->bf_last[c].n_bursts > cap_c)
                return rd_fail_msg(RD_ERR_DEVICE, "burst floor record of channel %d belongs to chunk %u (%u runs), not %ld", c,
                                   w->bf_last[c].chunk, w->bf_last[c].n_bursts, w->last);
            w->bu_last.insert(w->bu_last.end(), recs + (size_t)c * cap_c, recs + (size_t)c * cap_c + w->bf_last[c].n_bursts);
        }
        w->last_bursts = true;
    }
    if (w->spec_n) {
        // as the level records below: k_chan_spectrum ran before the demodulator launch that has reported
        const uint8_t *slot = w->h_sp[w->last & 1];
        memcpy(&w->sp_info_last, slot, sizeof(rd_spectrum_info));
        if (w->sp_info_last.chunk != (uint64_t)w->last || (int)w->sp_info_last.n_bins != w->spec_n)
            return rd_fail_msg(RD_ERR_DEVICE, "the spectrum record belongs to chunk %llu (%u bins), not %ld (%d bins)",
                               (unsigned long long)w->sp_info_last.chunk, w->sp_info_last.n_bins, w->last, w->spec_n);
        const double *p = (const double *)(slot + RD_SPEC_HDR_BYTES);
        w->sp_last.assign(p, p + w->spec_n);
        w->last_spec = true;
    }
    if (!w->levels) return rc;
    // The chunk's demodulator launch has reported, and k_chan_levels ran before it on the same stream: keep its records
    // (the slot is chunk last + 2's from its submit on).  Every record carries the chunk's number - a record of another
    // chunk here would be an ordering bug, not something to hand on.
    const rd_chan_level *lv = w->h_lv[w->last & 1];
    w->lv_last.assign(lv, lv + w->n_ch);
    memcpy(&w->lv_in_last, lv + w->n_ch, sizeof(rd_input_level));
    for (int c = 0; c < w->n_ch; c++)
        if (w->lv_last[c].chunk != (uint32_t)w->last)
            return rd_fail_msg(RD_ERR_DEVICE, "level record of channel %d belongs to chunk %u, not %ld", c, w->lv_last[c].chunk, w->last);
    if (w->lv_in_last.chunk != (uint64_t)w->last)
        return rd_fail_msg(RD_ERR_DEVICE, "the input level record belongs to chunk %llu, not %ld", (unsigned long long)w->lv_in_last.chunk, w->last);
    w->last_levels = true;
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
    WCHK(hipStreamWaitEvent(w->st_copy, w->e_chan[s], 0));
    WCHK(hipMemcpyAsync(out, w->d_out[s], need, hipMemcpyDeviceToHost, w->st_copy));
    WCHK(hipStreamSynchronize(w->st_copy));
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
