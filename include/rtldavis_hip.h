/*
 * rtldavis_hip.h - C ABI of librtldavis_hip.so: the MI355X (gfx950) implementation of
 * rtldavis's IQ -> bits -> packets path.
 *
 * The reference has no FFI for this path (it is pure Python/NumPy, and the legacy Go
 * twin is pure Go), so each entry point below names the reference function whose work
 * it takes over.  "py" = /root/reference/src/rtldavis/dsp.py, "go" = /root/reference/dsp/dsp.go.
 * The ctypes stub a maintainer of the reference would add is in INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes only; every function returns RD_OK (0) or a
 * negative rd_status; outputs are caller-allocated; no callbacks; no global state other
 * than the per-process HIP context, which is created lazily by the first call that
 * needs the device (never by rd_create / rd_create_multi / rd_batch_create), so a handle
 * may be created before fork() (py worker model: __main__.py:277, worker.py:29); a process
 * forked AFTER the device was used gets RD_ERR_DEVICE instead of undefined behaviour.
 * A handle is used by one thread at a time (like a reference Demodulator); different handles
 * are independent.  There is no CPU fallback: without a usable HIP device every entry point
 * that computes returns RD_ERR_DEVICE.
 * rd_last_error() returns a thread-local, human-readable message for the last failure.
 */
#ifndef RTLDAVIS_HIP_H
#define RTLDAVIS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RD_MAX_PREAMBLE 64   /* symbols */
#define RD_MAX_PKT_BYTES 32  /* (packet_symbols + 7) / 8 */

typedef enum rd_status {
    RD_OK = 0,
    RD_ERR_ARG = -1,      /* bad argument / "Incompatible array sizes" (py:32-36,145-149) */
    RD_ERR_DEVICE = -2,   /* HIP failure: no device, launch or copy error */
    RD_ERR_CAPACITY = -3, /* caller's output array too small; *n holds the needed count */
    RD_ERR_STATE = -4     /* call order violated (e.g. results before run) */
} rd_status;

/* py:101-125 PacketConfig / go:172-218 NewPacketConfig.  Derived constants are computed inside. */
typedef struct rd_config {
    int32_t bit_rate;
    int32_t symbol_length;    /* samples per symbol */
    int32_t preamble_symbols; /* <= RD_MAX_PREAMBLE */
    int32_t packet_symbols;   /* <= 8 * RD_MAX_PKT_BYTES */
    int32_t block_size;       /* samples per demodulate() call; multiple of 4 */
    uint8_t preamble[RD_MAX_PREAMBLE]; /* 0/1 per symbol */
} rd_config;

/* py:12-17 Packet, plus where it came from.  index is the window-relative q_idx of py:190-246. */
typedef struct rd_packet {
    int32_t stream; /* stream number in a batch (0 for rd_handle) */
    int32_t call;   /* block number b of the demodulate() call that returns it */
    int32_t index;
    int32_t nbytes;
    uint8_t data[RD_MAX_PKT_BYTES];
    double rssi;
    double snr;
} rd_packet;

/* One CRC-valid message of protocol.Parser.parse's front half (/root/reference/src/rtldavis/
 * protocol.py:282-318): bytes bit-reversed (:290), CRC-16-CCITT over data[2:] == 0 (:297),
 * frequency error from the mean discriminator output over the preamble window (:304-311). */
typedef struct rd_parsed {
    int32_t stream;
    int32_t call;
    int32_t index;     /* Packet.index of the packet it came from */
    int32_t freq_err;  /* Hz, -int(mean * sample_rate / 2pi) */
    int32_t id;        /* transmitter id: data[2] & 7 after the bit swap (:318) */
    int32_t nbytes;    /* length of data[] = packet bytes - 2 */
    uint8_t data[RD_MAX_PKT_BYTES]; /* bit-swapped message bytes, sync word removed (msg_data, :317) */
    double rssi;
    double snr;
} rd_parsed;

/* Mean per-launch duration of the kernels of the rd_batch_run calls made since timing was
 * enabled or last read (HIP events recorded on each run's stream). */
typedef struct rd_timing {
    float demod_ms;  /* fused LUT+rotate+FIR+discriminator-sign+pack kernel */
    float fixup_ms;  /* exact re-evaluation of guard-band samples */
    float search_ms; /* preamble search */
    float slice_ms;  /* slice + RSSI/SNR */
    float total_ms;
    int32_t runs;    /* runs averaged */
} rd_timing;

const char *rd_last_error(void);
/* Number of visible HIP devices (<0 on error).  Does not create a context. */
int rd_device_count(void);
/* Bind this process/thread's later calls to a device (hipSetDevice). */
int rd_set_device(int device);
/* Deadline of every host-side wait of this library (the polling waits for a run's results, a block's kernels, a
 * device-to-host copy), in milliseconds; returns the previous value.  Default: RD_WAIT_TIMEOUT_MS from the
 * environment, else 10000; ms < 0 restores that default.  A wait that passes its deadline returns RD_ERR_DEVICE
 * ("timed out after ... waiting for ...") instead of spinning for ever, so that the caller's per-block try/except
 * (/root/reference/src/rtldavis/worker.py:56-58: log, drop the block, continue) fires when a kernel never completes.
 * The handle stays usable: a streaming handle drops the blocks in flight (waits for them again, discards their
 * packets) at its next rd_demod_submit / rd_demod_block / rd_reset; a batch handle's next rd_batch_results waits again.
 * ms = 0 makes every wait that is not satisfied at its first poll time out (test hook). */
int rd_set_wait_timeout_ms(int ms);

/* ---------------------------------------------------------------------------------------------
 * Streaming demodulator: one stream, one block per call, state carried across calls.
 * Replaces py:128-253 Demodulator / go:220-310.
 * ------------------------------------------------------------------------------------------- */
typedef struct rd_demod rd_demod;

/* py:129-137 __init__ (no device work; safe before fork). */
int rd_create(const rd_config *cfg, rd_demod **out);
void rd_destroy(rd_demod *h);
/* py:248-253 reset. */
int rd_reset(rd_demod *h);
/*
 * py:139-169 demodulate.  `samples` is either uint8 interleaved I,Q (is_complex = 0,
 * count = 2 * block_size bytes; py:151-152) or complex128 (is_complex = 1, count =
 * block_size elements, interleaved re,im doubles; py:144-150).  Any other count returns
 * RD_ERR_ARG ("Incompatible array sizes").  Packets are written in the reference's order
 * (phase-major search order, per-call dedupe, py:171-205).
 */
int rd_demod_block(rd_demod *h, const void *samples, size_t count, int is_complex, rd_packet *out, int cap, int *n);
/*
 * Several receivers in lock step: n_streams independent Demodulators (one per SDR / hop channel)
 * fed one block each per call, all streams in one set of launches.  State is carried per stream
 * exactly as for rd_create.  iq: uint8 [n_streams][2 * block_size], stream-major; packets carry
 * their stream number and come sorted by (stream, reference order).  This is the shape
 * worker.py:34-54 would take with more than one dongle.
 */
int rd_create_multi(const rd_config *cfg, int n_streams, rd_demod **out);
int rd_demod_blocks(rd_demod *h, const uint8_t *iq, size_t nbytes, rd_packet *out, int cap, int *n);
/*
 * The same call split in two, for a receiver loop that must not wait (replaces the hop
 * runners/rtlsdr.py:100-103 `data_queue.put(samples)` -> worker.py:34-50 `demodulate(samples)`):
 * rd_demod_submit copies the block(s) to where the device takes them from (see rd_set_input_push below; the multi-launch
 * form: a pinned slot and a host-to-device copy on a copy stream) and queues the kernels, then returns; rd_demod_fetch
 * waits (polling) for the OLDEST submitted block and returns its packets exactly as rd_demod_block / rd_demod_blocks would.
 * Two blocks may be in flight (RD_ERR_STATE on a third submit): block i+1's copy overlaps block i's
 * kernels.  count: 2 * block_size * n_streams bytes, or block_size complex128 samples (single stream).
 * The state mirrors below need a quiet handle (everything fetched); rd_demod_parsed does not.
 */
int rd_demod_submit(rd_demod *h, const void *samples, size_t count, int is_complex);
/*
 * How rd_demod_submit hands a block to the device.  Where the whole of device memory is host-visible (PCIe large BAR:
 * hipDeviceAttributeIsLargeBar) and the runtime publishes the device's HDP flush register, the one-launch forms take the
 * block from an uncached DEVICE buffer the host has written it into (memcpy, sfence, HDP flush, launch: 128 KB in ~3 us
 * at ~45 GB/s) instead of reading a pinned host slot across the bus from inside the kernel (~13 GB/s).  Same packets
 * either way.  rd_set_input_push: -1 = use the push where available (default; RD_PUSH_INPUT=0 in the environment turns
 * it off), 0 = never, 1 = as -1; applies to handles whose device state is created afterwards; returns 1 when the push
 * is available on the current device (0 otherwise, < 0 on a device error).  rd_demod_input_mode: 1 when this handle's
 * copied blocks are pushed, 0 when they go through the pinned slot.
 */
int rd_set_input_push(int mode);
int rd_demod_input_mode(rd_demod *h);
/*
 * The same without ANY copy on the way in - SURVEY section 8f-4's "pinned-memory ring replacing the pickled-ndarray
 * queue hop" (/root/reference/src/rtldavis/runners/rtlsdr.py:100-103 `data_queue.put(samples)` ->
 * /root/reference/src/rtldavis/worker.py:37 `data_queue.get()`): rd_demod_register_input pins a buffer the PRODUCER owns
 * (a multiprocessing.shared_memory ring an SDR process fills, rtldavis_amd/ring.py) and maps it into the device;
 * rd_demod_submit_from launches on the block that lies at `offset` bytes into it (16-byte aligned; count as for
 * rd_demod_submit) - the one-launch block reads it across the bus where it is.  The block must stay untouched until its
 * rd_demod_fetch has returned.  One buffer per handle; registering again replaces it, host = NULL unregisters
 * (rd_destroy does too); needs a quiet handle.
 */
int rd_demod_register_input(rd_demod *h, void *host, size_t nbytes);
int rd_demod_submit_from(rd_demod *h, size_t offset, size_t count, int is_complex);
int rd_demod_fetch(rd_demod *h, rd_packet *out, int cap, int *n);
int rd_demod_inflight(rd_demod *h);
/*
 * The packets of the block returned last, again: a call that ended in RD_ERR_CAPACITY has consumed its
 * block (the reference's list is unbounded, py:190-246: up to block_size + 1 positions per call are legal),
 * *n told how many there are - grow the array and fetch them here.  Nothing is lost.
 */
int rd_demod_refetch(rd_demod *h, rd_packet *out, int cap, int *n);
/*
 * Parser.parse's front half (/root/reference/src/rtldavis/protocol.py:282-318, the rd_parsed struct above) for the
 * streaming forms, computed inside the block's own kernels: the wave that slices a packet also bit-swaps it, checks the
 * CRC and - for the survivors only - averages the float64 discriminator over the preamble window of the stream's state
 * as it is right after that block (what rd_copy_discriminated_stream would return on a quiet handle at that moment).
 * So the receiver loop of /root/reference/src/rtldavis/worker.py:49-50 needs no quiet handle and no state mirror: two
 * blocks stay in flight and each fetched block brings its messages with their frequency errors.
 * rd_demod_set_parse: opt-in (default 0), quiet handle only (else RD_ERR_STATE), no device work (safe before fork);
 * applies to the blocks submitted afterwards.  rd_demod_parsed: the CRC-valid messages of the block the last
 * rd_demod_fetch / rd_demod_block(s) returned, sorted like its packets, stream and call as in the packet each came from;
 * may be called any number of times, with later blocks in flight.  RD_ERR_CAPACITY sets *n and loses nothing;
 * RD_ERR_STATE when nothing has been fetched since create / reset or that block was submitted with parse off.
 */
int rd_demod_set_parse(rd_demod *h, int enabled);
int rd_demod_parsed(rd_demod *h, rd_parsed *out, int cap, int *n);
/* The same decision for one packet on the host, no device involved: data = the nbytes (<= RD_MAX_PKT_BYTES) on-air bytes
 * of an rd_packet.  Returns 1 when nbytes > 2 and the CRC-16-CCITT over the bit-swapped bytes [2:] is 0 - then msg
 * (nbytes - 2 bytes: the swapped message, sync word removed) and *id (msg[0] & 7) are filled -, 0 when not (msg, id
 * untouched), RD_ERR_ARG for a null pointer or nbytes out of range. */
int rd_parse_packet(const uint8_t *data, int nbytes, uint8_t *msg, int *id);
/* discriminated (py:134) of one stream of a multi-stream handle */
int rd_copy_discriminated_stream(rd_demod *h, int stream, double *out, size_t n);
/* Lazily materialised mirrors of the reference's state arrays after the last call:
 * discriminated f64[2*block_size] (py:134), filtered complex128[block_size+1] as
 * interleaved doubles (py:133), quantized uint8[buffer_length] 0/1 (py:135). */
int rd_copy_discriminated(rd_demod *h, double *out, size_t n);
int rd_copy_filtered(rd_demod *h, double *out_interleaved, size_t n_complex);
int rd_copy_quantized(rd_demod *h, uint8_t *out, size_t n);

/* ---------------------------------------------------------------------------------------------
 * Batch demodulator: n_streams independent streams of n_blocks blocks each, all demodulated
 * from reset in one pass.  Output is, per stream and per call, exactly what n_blocks
 * successive Demodulator.demodulate() calls return (py:139-169).
 * ------------------------------------------------------------------------------------------- */
typedef struct rd_batch rd_batch;

int rd_batch_create(const rd_config *cfg, int n_streams, int n_blocks, rd_batch **out);
void rd_batch_destroy(rd_batch *b);
/* Device address of the resident input buffer, uint8 [n_streams][n_blocks*block_size][2]
 * (dense, stream-major), so a producer on the GPU can fill it in place. */
int rd_batch_input_ptr(rd_batch *b, void **dev_ptr, size_t *nbytes);
/* Host -> device copy of the whole input (PCIe; not part of the timed region of bench.py). */
int rd_batch_upload(rd_batch *b, const uint8_t *iq_host, size_t nbytes);
/* The same copy issued on `hip_stream` (hipStream_t, a copy stream of the caller's) without waiting: the handle's next
 * rd_batch_run waits for it on the device, so the upload of one resident batch overlaps the kernels of another
 * (host-fed pipelines: SURVEY section 7 "PCIe vs HBM").  iq_host: pinned memory, untouched until that run's results
 * have been fetched.  The copy queues behind the handle's previous run (which still reads the input). */
int rd_batch_upload_async(rd_batch *b, const uint8_t *iq_host, size_t nbytes, void *hip_stream);
/* Run the whole path on the resident input.  hip_stream: a hipStream_t (NULL = default
 * stream).  Asynchronous; rd_batch_results synchronises. */
int rd_batch_run(rd_batch *b, void *hip_stream);
/* Packets of the last run, sorted by (stream, call, reference order).  *n = count. */
int rd_batch_results(rd_batch *b, rd_packet *out, int cap, int *n);
/* Packed bitstream of one stream: sample t -> byte t/8, bit t%8 (LSB first);
 * nbytes >= (n_blocks*block_size + 7) / 8.  (go:105-113 Pack is the nearest reference stage;
 * the Python reference keeps one byte per bit, py:135.) */
int rd_batch_copy_bits(rd_batch *b, int stream, uint8_t *out, size_t nbytes);
/* Full-precision discriminator output d[t0 .. t0+n) of one stream (py:76-90), float64. */
int rd_batch_copy_discriminated(rd_batch *b, int stream, size_t t0, double *out, size_t n);
/* Parser.parse front half on the device for the whole batch (opt-in, before rd_batch_run):
 * after a run, rd_batch_parsed returns the CRC-valid messages sorted like rd_batch_results. */
int rd_batch_set_parse(rd_batch *b, int enabled);
int rd_batch_parsed(rd_batch *b, rd_parsed *out, int cap, int *n);
/* HIP-event timing on the run's stream.  enabled = 1: the demod kernel and the whole run (its
 * start/stop events and the end-of-run event are attached to the kernel dispatches themselves, so
 * they cost no idle time); 2: every stage (two more events recorded between kernels, ~6 us of GPU
 * idle time each); 0: off.  get_timing synchronises, returns the mean over the runs recorded so
 * far and starts a new window (stages not timed read 0). */
int rd_batch_set_timing(rd_batch *b, int enabled);
int rd_batch_get_timing(rd_batch *b, rd_timing *out);
/* Pipelined completion (opt-in; no counterpart in the reference, whose demodulate() py:128-253 returns its packets
 * synchronously).  enabled = 1: rd_batch_run ends without an event of its own; the run's readback is hung on the
 * stop event of the NEXT demod kernel launched on the same HIP stream, by this handle or any other - an event on a
 * run's last kernel idles the stream for 6-11 us, one on the demod kernel does not.  For callers that keep several
 * runs queued on one stream (bench.py: resident batches demodulated round-robin): a run's results are ready one
 * demod kernel later, the stream never idles.  If nothing is launched behind a run, the first call that needs its
 * results (rd_batch_results, rd_batch_get_timing, ...) records the event then.  A timed pipelined run has no
 * end-of-run event: rd_timing.total_ms covers the runs that have one (0 if none).  0 (default): off. */
int rd_batch_set_pipelined(rd_batch *b, int enabled);
/* Which forms of the kernels the last run took (it is waited for first; no counterpart in the reference - for tests and
 * tools that must know that an opt-in form really ran and did not fall back): a mask of RD_FORM_*. */
#define RD_FORM_ORDERED_TAIL 1u   /* records ordered and deduped on the device */
#define RD_FORM_SECOND_PASS 8u    /* a list or bucket overflowed: search and slice ran a second time, in full */
#define RD_FORM_ONE_LAUNCH_TAIL 16u /* everything behind the demod kernel ran as ONE launch (k_tail; implies ORDERED_TAIL) */
int rd_batch_last_run_forms(rd_batch *b, uint32_t *forms);
/* Counters of the last run: 32-sample runs with at least one 8-sample group re-evaluated
 * exactly (guard band), raw preamble matches. */
int rd_batch_get_counters(rd_batch *b, uint64_t *fixup_runs, uint64_t *matches);
/* The schedule of the handle's last demod launch: tiles per chunk and waves of the persistent grid (a wave takes chunk
 * number wave first and draws further ones from the work queues when there are more chunks than waves).  b == NULL: of the
 * last rd_debug_demod_mfma launch of this process.  For tests: results do not depend on the schedule. */
int rd_k1_schedule(rd_batch *b, uint32_t *tiles_per_chunk, uint32_t *waves);

/* ---------------------------------------------------------------------------------------------
 * Stage functions on host arrays (caller-allocated out-params, like the reference's).
 * Each runs its own float64 kernel on the device.
 * ------------------------------------------------------------------------------------------- */
/* py:20-39 ByteToCmplxLUT.execute / go:26-44: n_bytes must equal 2 * n_cplx else RD_ERR_ARG. */
int rd_lut_execute(const uint8_t *in_bytes, size_t n_bytes, double *out_cplx, size_t n_cplx);
/* py:42-49 rotate_fs4 / go:46-63 RotateFs4 (in == out allowed). */
int rd_rotate_fs4(const double *in_cplx, double *out_cplx, size_t n_cplx);
/* py:52-73 fir9 / go:65-83 FIR9: out[i] = sum_m c[m] * in[i+m], n_out <= n_in - 8. */
int rd_fir9(const double *in_cplx, size_t n_in, double *out_cplx, size_t n_out);
/* py:76-90 discriminate / go:85-95 Discriminate: n_out = n_in - 1. */
int rd_discriminate(const double *in_cplx, size_t n_in, double *out, size_t n_out);
/* py:93-98 quantize / go:97-103 Quantize: sign bit. */
int rd_quantize(const double *in, uint8_t *out, size_t n);
/* go:105-113 Pack + go:115-131 Search / py:171-188 _search on a 0/1-per-byte buffer:
 * indices in the reference's order; *n = count (RD_ERR_CAPACITY if > cap). */
int rd_search(const rd_config *cfg, const uint8_t *quantized, size_t n, int32_t *indices, int cap, int *count);

/* ---------------------------------------------------------------------------------------------
 * Wideband front end: one IQ capture (uint8, int8, int16 or float32) at decim * out_rate samples/s ->
 * one out_rate uint8 IQ stream per channel, e.g. the 51 US hop channels (protocol.py:119-171) out
 * of one 26.88 MS/s capture, written straight into a batch demodulator's input buffer.
 * The reference has no channelizer (it retunes one dongle per hop, runners/rtlsdr.py:51,72):
 * parity is unpinned; the definition is in rtldavis_amd/csrc/rd_channelizer.hip and restated in
 * float64 by oracle/channelizer_oracle.py.  It runs on the matrix cores (f16 MFMA with the taps split
 * into two f16 digits, 2^-22 relative; the samples are exact in f16 - a 16-bit one as two 8-bit sign-magnitude
 * digits -, accumulation is fp32).
 * Contract: with Z the float64 model's value in front of the quantiser (channelize_z), every output byte
 * is within one step of clip(rint(Z), 0, 255), and equals it wherever Z lies more than delta from every
 * rounding boundary k + 1/2; delta, a few hundredths of a step at 512 taps, is derived from the kernel's
 * arithmetic in tests/chan_bound.py:error_bound (its one unmeasured input: the hardware sine's accuracy,
 * assumed 2^-16).  Measured: the bytes that differ lie within 1/50 of delta of a boundary.
 * ------------------------------------------------------------------------------------------- */
typedef struct rd_chan_config {
    int32_t out_rate;   /* Hz per channel (19200 * symbol_length = 268800, protocol.py:309) */
    int32_t decim;      /* wideband rate = decim * out_rate; a multiple of 4 */
    int32_t n_taps;     /* length of the real low-pass prototype */
    int32_t n_channels;
    double gain;        /* applied before the 8-bit quantiser clip(rint(z * 127.6 + 127.4), 0, 255) */
} rd_chan_config;
typedef struct rd_chan rd_chan;

/* Sample format of the wideband capture (the output is uint8 whatever the input):
 *   RD_IQ_U8   uint8 I, Q                    x = (I - 127.4) / 127.6 + j (Q - 127.4) / 127.6   (RTL-SDR; dsp.py:20-39)
 *   RD_IQ_S8   int8 I, Q                     x = I / 128 + j Q / 128                           (sc8 / CS8)
 *   RD_IQ_S16  int16 I, Q, host byte order   x = I / 32768 + j Q / 32768                       (sc16 / CS16)
 *   RD_IQ_CF32 float32 I, Q, host byte order x = adm(I) + j adm(Q)                             (CF32 / fc32 / numpy complex64)
 *              8 bytes per IQ pair, nominal full scale +-1.0; adm(v) = 0 if v is NaN, else v clamped to [-8, +8] (+-Inf
 *              is +-8: 18 dB of headroom, and one NaN does not poison every window it falls into).  No DC term; samples
 *              outside the capture are exactly 0.  The kernel splits 2^12 adm(v) into two f16 digits hi = f16(s),
 *              lo = f16(s - hi), exact to max(2^-22 |x|, 2^-37).
 * Everything behind x - filter, mixer, phase accumulator, per-channel gain, output quantiser, the contract above - is
 * the same; the bound of a format is tests/chan_bound_fmt.py:error_bound_fmt, of RD_IQ_CF32
 * tests/chan_bound_cf32.py:error_bound_cf32.  Code 3 stays unassigned and the name "f32" unknown: both are errors. */
#define RD_IQ_U8 0
#define RD_IQ_S8 1
#define RD_IQ_S16 2
#define RD_IQ_CF32 4

/* taps: n_taps doubles; shift_hz[c]: the wideband frequency (Hz, relative to the capture's centre)
 * that channel c moves to 0 Hz of its output - for rtldavis the channel centre plus out_rate / 4,
 * because the demodulator's Fs/4 rotation (dsp.py:42-49) expects the carrier at -Fs/4.  No device
 * work (safe before fork).  rd_chan_create is rd_chan_create_fmt with RD_IQ_U8. */
int rd_chan_create(const rd_chan_config *cfg, const double *taps, const int64_t *shift_hz, rd_chan **out);
/* The same for a capture in sample_format (another value: RD_ERR_ARG).  Limits, all formats: decim a multiple of 4
 * in 4 .. 4096, 1 .. 8192 taps, 1 .. 4096 channels, out_rate < 2^26; with t_pad = n_taps rounded up to 8:
 *   RD_IQ_U8, RD_IQ_S8  2 (127 decim + t_pad + 8) + 16 <= 160 KiB of LDS, and ceil((t_pad - 1) / decim) <= 64
 *   RD_IQ_S16           8 (127 decim + t_pad + 4) + 16 <= 160 KiB of LDS (a sample is staged as four 16-bit lanes)
 *                       and no limit on n_taps / decim (there is no DC term to tabulate).
 *   RD_IQ_CF32          as RD_IQ_S16 (the same four lanes per staged sample): decim <= 160 at 8 taps. */
int rd_chan_create_fmt(const rd_chan_config *cfg, int sample_format, const double *taps, const int64_t *shift_hz,
                       rd_chan **out);
void rd_chan_destroy(rd_chan *h);
/* Host -> device copy of a capture (I,Q interleaved, in the handle's format; nbytes a whole number of its IQ
 * pairs, else RD_ERR_ARG "Incompatible array sizes"), or the device address of the resident capture buffer (at
 * least n_wide_samples IQ pairs of that format) for a producer on the GPU. */
int rd_chan_upload(rd_chan *h, const void *wide_iq, size_t nbytes);
int rd_chan_input_ptr(rd_chan *h, size_t n_wide_samples, void **dev_ptr);
/* Channelize output samples 0 .. n_out-1 (n_out <= capture length / decim; zero history before
 * the capture) of every channel into device memory: channel c at dst_dev + c * dst_stream_stride,
 * 2 bytes per sample - rd_batch_input_ptr's layout with stride 2 * n_blocks * block_size.
 * Asynchronous on hip_stream (NULL = default stream). */
int rd_chan_run(rd_chan *h, size_t n_out, void *dst_dev, size_t dst_stream_stride, void *hip_stream);
/* Same, into a host array uint8 [n_channels][n_out][2] (synchronous). */
int rd_chan_run_host(rd_chan *h, size_t n_out, uint8_t *out_host, size_t nbytes);
/* Power spectrum of the uploaded capture (SPECTRUM below: the definition, with L = the capture's IQ pairs; the same kernel
 * as the streaming receiver's, so a chunk uploaded alone gives that chunk's record bit for bit).  power_host: n_bins
 * doubles in ascending frequency; *segments (may be NULL) = L / n_bins.  Synchronous, like rd_chan_run_host.
 * RD_ERR_STATE without a resident capture, RD_ERR_ARG for an n_bins that is no power of two in 64 .. 4096 or exceeds L. */
int rd_chan_spectrum(rd_chan *h, int n_bins, double *power_host, uint32_t *segments);
/* The same, asynchronous on hip_stream (NULL = default stream) into device memory, as rd_chan_run is to rd_chan_run_host:
 * dst_dev (16-byte aligned) receives the record {uint64 chunk = 0; uint32 segments; uint32 n_bins} + n_bins doubles.
 * The first call with a new n_bins builds the tables and waits for that stream once. */
int rd_chan_spectrum_dev(rd_chan *h, int n_bins, void *dst_dev, void *hip_stream);
/* Per-channel gain: gain[c] replaces cfg.gain for channel c (n = n_channels, every gain finite and > 0 - in float32
 * too, which is what the kernel multiplies with - else RD_ERR_ARG and nothing changes) in the runs that follow.  With every
 * entry equal to cfg.gain the output is the scalar form's, byte for byte.  Needs a quiet handle: the caller has waited
 * for the streams its earlier rd_chan_run calls were queued on. */
int rd_chan_set_gain(rd_chan *h, const double *gain, int n);

/* ---------------------------------------------------------------------------------------------
 * Wideband receiver (rtldavis_amd/csrc/rd_wideband.hip): one capture that never ends, fed in
 * chunks of decim * block_size wideband samples, channelized into every channel and demodulated
 * with the state of both carried across chunks.  Owns one rd_chan configuration and one
 * multi-stream rd_demod with n_streams = n_channels.  For any capture split into chunks, the
 * channelized bytes equal rd_chan_run on the whole capture, byte for byte.  Parity: unpinned, as
 * for the channelizer.
 * ------------------------------------------------------------------------------------------- */
typedef struct rd_wideband rd_wideband;
/* no device work (safe before fork), like rd_create / rd_chan_create; block_size % 128 == 0.  rd_wideband_create is
 * rd_wb_create_fmt with RD_IQ_U8; rd_wb_create_fmt takes chunks in sample_format (limits: rd_chan_create_fmt) and
 * returns the same handle type, which every rd_wideband_* call below takes. */
int rd_wideband_create(const rd_config *cfg, const rd_chan_config *ccfg, const double *taps,
                       const int64_t *shift_hz, rd_wideband **out);
int rd_wb_create_fmt(const rd_config *cfg, const rd_chan_config *ccfg, int sample_format, const double *taps,
                     const int64_t *shift_hz, rd_wideband **out);
void rd_wideband_destroy(rd_wideband *w);
/* clock to 0, history to zero, demod state as rd_reset (waits for the chunks in flight) */
int rd_wideband_reset(rd_wideband *w);
/* one chunk: I,Q of decim * block_size wideband samples in the handle's format, i.e. (2 or, for RD_IQ_S16, 4, for
 * RD_IQ_CF32, 8) * decim * block_size bytes (else RD_ERR_ARG "Incompatible array sizes"); host->device copy, channelize (streaming form), one demod launch - all queued on the
 * handle's own non-blocking streams, returns at once.  At most two chunks in flight (a third:
 * RD_ERR_STATE); the copy of chunk k+1 overlaps chunk k's kernels.  The clock and the history
 * advance here, so a fetch that times out loses only that chunk's packets. */
int rd_wideband_submit(rd_wideband *w, const void *wide_iq, size_t nbytes);
/* as rd_demod_fetch / rd_demod_refetch: packets of the oldest chunk in flight, stream = channel, call = chunk */
int rd_wideband_fetch(rd_wideband *w, rd_packet *out, int cap, int *n);
int rd_wideband_refetch(rd_wideband *w, rd_packet *out, int cap, int *n);
/* chunks in flight whose packets can still be fetched */
int rd_wideband_inflight(rd_wideband *w);
/* the channelized bytes uint8 [n_channels][2 * block_size] of the chunk the last fetch returned (valid until
 * the next submit), and one channel's discriminator output as rd_copy_discriminated_stream */
int rd_wideband_copy_channelized(rd_wideband *w, uint8_t *out, size_t nbytes);
int rd_wideband_copy_discriminated(rd_wideband *w, int channel, double *out, size_t n);
/* as rd_demod_set_parse / rd_demod_parsed: the CRC-valid messages of the chunk the last fetch returned, stream = channel,
 * call = chunk, with their frequency errors - chunk k's while chunk k+1 is in flight (rd_wideband_copy_discriminated
 * shows the state after the NEWEST chunk and needs a quiet receiver) */
int rd_wb_set_parse(rd_wideband *w, int enabled);
int rd_wb_parsed(rd_wideband *w, rd_parsed *out, int cap, int *n);
/* Retune: channel c mixes with shift_hz[c] (as rd_wb_create_fmt's; n = n_channels, |shift| <= wide rate / 2, else
 * RD_ERR_ARG and nothing changes) from the next submitted chunk on, phase-continuous at that boundary: with t the
 * absolute output time, the output phase is frac((s_c t + P_c) / out_rate), P_c an integer in [0, out_rate) that is 0
 * after create and reset, and a retune s -> s' at the boundary t_b sets P' = (P + (s - s') t_b) mod out_rate.  Every
 * output from t_b on is filtered with the new band-pass, the few whose window reaches into the previous chunk included.
 * Host bookkeeping only: no device work, no wait, legal with chunks in flight; the next rd_wideband_submit queues the
 * rebuild of the changed channels' tables (a kernel) in front of its channelizer.  Calls before that submit collapse
 * into the last; shifts equal to those in force change nothing.  Filter history, clock and demodulator state are kept.
 * rd_wideband_reset drops a pending retune and returns to the constructed shifts with P = 0.
 * rd_wb_tuning: the tuning the next submitted chunk will use, shifts as given and P_c (host only, no device needed). */
int rd_wb_retune(rd_wideband *w, const int64_t *shift_hz, int n);
int rd_wb_tuning(rd_wideband *w, int64_t *shift_hz, int64_t *phase, int n);
/* Gain (the mechanism of an AGC; the policy is the caller's, e.g. rtldavis_amd/agc.py): channel c is re-quantised with
 * gain[c] - absolute values that replace cfg.gain, stored as float32 - from the next submitted chunk on, exactly at
 * that chunk boundary.  n = n_channels and every gain finite and > 0 (in float32 too), else RD_ERR_ARG and nothing
 * changes.  Host bookkeeping only, like rd_wb_retune: no device work, no wait, legal with two chunks in flight; the next
 * rd_wideband_submit queues the table (one copy through the pinned slot of the chunk's parity, only if an entry differs)
 * in front of its channelizer.  Nothing else is touched: filter history, clock, phase accumulators, demodulator state.
 * With every gain equal to cfg.gain the bytes are those of a receiver that never called it.
 * rd_wb_gains: the gains the next submitted chunk will use (the float32 values; host only, no device needed).
 * rd_wideband_reset drops a pending change and returns to cfg.gain. */
int rd_wb_set_gain(rd_wideband *w, const double *gain, int n);
int rd_wb_gains(rd_wideband *w, double *gain, int n);
/* Level metering (k_chan_levels, rd_chan_levels.hip): with levels on, every chunk carries one more launch behind its
 * channelizer.  All quantities are exact integers.
 *   per channel, over the 2 * block_size bytes b of its channelized chunk, a = 2 b - 255:
 *     peak = max |a|, clipped = bytes equal to 0 or 255, power = sum a^2, gain = the float32 gain in force for the chunk
 *     (RMS as a fraction of full scale: sqrt(power / (2 * block_size)) / 255)
 *   for the input chunk, over its 2 * decim * block_size components k, a = 2 k - 255 (RD_IQ_U8) or a = k (RD_IQ_S8, _S16):
 *     peak = max |a|, clipped = components at either end of the format's range, power = sum a^2
 *     RD_IQ_CF32, in int16 units (full scale 32768): a = k = clip(rint(adm(v) * 32768), -32768, 32767), rint ties-to-even;
 *     clipped = components with k at either end plus NaN components (a NaN is the value 0 for peak and power)
 *     (no admissible chunk overflows a field: < 2^32 components, a^2 <= 2^30)
 *   chunk = the chunk's sequence number since create / reset (rd_packet.call of its packets); rd_chan_level carries its low 32 bits.
 * rd_wb_set_levels needs a quiet receiver (RD_ERR_STATE otherwise), like rd_wb_set_parse; off (the default): nothing is
 * launched.  rd_wb_levels: the records of the chunk the last fetch returned (n = n_channels; `in` may be NULL), kept by
 * that fetch - valid with later chunks in flight, until the next fetch.  RD_ERR_STATE before any fetch and when that chunk
 * was submitted with levels off. */
typedef struct rd_chan_level {
    uint64_t power;
    uint32_t peak;
    uint32_t clipped;
    float gain;
    uint32_t chunk;
} rd_chan_level;
typedef struct rd_input_level {
    uint64_t power;
    uint64_t chunk;
    uint32_t peak;
    uint32_t clipped;
} rd_input_level;
int rd_wb_set_levels(rd_wideband *w, int enabled);
int rd_wb_levels(rd_wideband *w, rd_chan_level *out, int n, rd_input_level *in);
/* SPECTRUM (k_chan_spectrum, rd_spectrum.hip): the power spectrum of every chunk, on the device.  With N = n_bins a power
 * of two in 64 .. 4096, L = decim * block_size the chunk's IQ pairs (N <= L) and S = L / N whole segments (segment s =
 * samples [s N, (s + 1) N) of this chunk; the L - S N samples at its end are not used; no state crosses chunks):
 *   x[n]   the sample as complex float32, the channelizer's meaning of each format: RD_IQ_U8 (10 k - 1274) * f32(1 / 1276)
 *          per component (= (k - 127.4) / 127.6 to 1.5 ulp relative), RD_IQ_S8 k / 128, RD_IQ_S16 k / 32768, RD_IQ_CF32 adm(v)
 *   w[n]   = 0.5 - 0.5 cos(2 pi n / N), periodic Hann, a float32 table rounded once from float64 (the twiddles likewise)
 *   X_s[k] = sum_n w[n] x[s N + n] e^{-2 pi i k n / N}                                  (float32 arithmetic per segment)
 *   P[j]   = 1 / (S (N/2)^2) sum_s |X_s[(j + N/2) mod N]|^2                             (float64 sum and scaling)
 * in ascending frequency: bin j lies at centre + (j - N/2) wide_rate / N, and (N/2)^2 = (sum w)^2, so a full-scale
 * complex tone on a bin centre reads 1.0.  Against the same in float64 every bin is within 2.01 ((6.7 log2 N + 4) 2^-24)
 * sum_k P[k] (tests/spectrum_model.py).  The same chunk and N give the same bits on every run: a fixed number of
 * workgroups min(S, 64), each summing its segments in ascending order, their partial sums added in ascending order.
 * rd_wb_set_spectrum: n_bins, or 0 = off (the default: nothing is launched).  Needs a quiet receiver (RD_ERR_STATE
 * otherwise), like rd_wb_set_levels; RD_ERR_ARG for another value or n_bins > L.  No device work (safe before fork): the
 * tables and record slots are made by the next submit.
 * rd_wb_spectrum: the record of the chunk the last fetch returned (power: n_bins doubles; info may be NULL), kept by that
 * fetch - valid with later chunks in flight, until the next fetch.  RD_ERR_STATE before any fetch and when that chunk was
 * submitted with the spectrum off; RD_ERR_ARG when n_bins is not that record's.  rd_wideband_reset keeps the setting and
 * drops the record. */
typedef struct rd_spectrum_info {
    uint64_t chunk;      /* the chunk's sequence number since create / reset */
    uint32_t segments;   /* S */
    uint32_t n_bins;     /* N */
} rd_spectrum_info;
int rd_wb_set_spectrum(rd_wideband *w, int n_bins);
int rd_wb_spectrum(rd_wideband *w, double *power, int n_bins, rd_spectrum_info *info);
/* BURSTS (k_chan_bursts, rd_bursts.hip): where on each channel there is energy, and at which frequency - from bursts the
 * demodulator cannot decode, e.g. because the receiver's reference is further off than the +-4.8 kHz deviation
 * (rtldavis_amd/acquire.py turns the records into one retune).  With bursts on, every chunk carries one more launch behind
 * its channelizer.  All quantities are exact integers.  Channel c, the 2 * block_size bytes b of its channelized chunk,
 * aI[t] = 2 b[2t] - 255, aQ[t] = 2 b[2t+1] - 255, z = aI + j aQ; windows of 128 outputs, nW = block_size / 128; window w:
 *   p_w = sum |z[t]|^2 over its 128 outputs
 *   r_w = sum z[t] conj(z[t-1]) over the 127 pairs inside it (nothing crosses a window or a chunk: no state)
 *   ON when p_w >= thr[c]; the default thr[c] = 0xFFFFFFFF leaves every window OFF (p_w <= 16646400)
 * A burst is a maximal run of consecutive ON windows inside the chunk: one rd_burst per run, a channel's in ascending
 * `first`, the channels in ascending order; the OFF windows are summed in the channel's rd_burst_floor (the noise floor,
 * and the correlation the channel filter gives noise - what an estimator subtracts).  The same chunk and thresholds give
 * the same bits on every run.
 * rd_wb_set_bursts: on / off (the default: nothing is launched).  Needs a quiet receiver (RD_ERR_STATE otherwise), like
 * rd_wb_set_levels; RD_ERR_ARG when switched on with nW > 4096.  No device work (safe before fork).
 * rd_wb_set_burst_threshold: thr[c] for channel c (n = n_channels, else RD_ERR_ARG and nothing changes) from the next
 * submitted chunk on, exactly at that boundary.  Host bookkeeping only, like rd_wb_set_gain: legal with two chunks in
 * flight; calls before that submit collapse into the last.  The table in force for a chunk is echoed in its floor
 * records.  rd_wideband_reset returns to the default table.  rd_wb_burst_thresholds: what the next submitted chunk will use.
 * rd_wb_bursts: the records of the chunk the last fetch returned, kept by that fetch - valid with later chunks in flight,
 * until the next fetch.  *n = the number of records; with cap < *n: RD_ERR_CAPACITY, nothing is lost, call again (out may
 * be NULL with cap = 0).  floor: NULL, or room for n_floor = n_channels records.  RD_ERR_STATE before any fetch and when
 * that chunk was submitted with bursts off. */
typedef struct rd_burst {
    int32_t  channel;
    uint32_t first;          /* first window of the run */
    uint32_t windows;        /* length of the run in windows */
    uint32_t flags;          /* bit 0: first == 0; bit 1: the run ends at window nW-1 */
    uint64_t power;          /* sum of p_w over the run */
    uint32_t peak;           /* max p_w over the run */
    uint32_t pad;
    int64_t  corr_re, corr_im;   /* sum of r_w over the run */
} rd_burst;
typedef struct rd_burst_floor {      /* one per channel */
    uint32_t threshold;      /* thr[c] in force for this chunk */
    uint32_t windows_off;
    uint32_t n_bursts;
    uint32_t chunk;          /* the chunk's sequence number since create / reset, its low 32 bits */
    uint64_t power_off;      /* sum of p_w over the off-windows */
    int64_t  corr_re_off, corr_im_off;
} rd_burst_floor;
int rd_wb_set_bursts(rd_wideband *w, int enabled);
int rd_wb_set_burst_threshold(rd_wideband *w, const uint32_t *thr, int n);
int rd_wb_burst_thresholds(rd_wideband *w, uint32_t *thr, int n);
int rd_wb_bursts(rd_wideband *w, rd_burst *out, int cap, int *n, rd_burst_floor *floor, int n_floor);
/* BURST DECODE (k_chan_burst_decode, rd_burst_decode.hip): the messages of the bursts above, wherever in the channel
 * filter's pass band their carrier lies.  The demodulator slices the discriminator around 0 Hz and gets no message from a
 * burst further off than the deviation; here every run is sliced around its OWN mean frequency - its record's correlation
 * sum - and sync word plus CRC-16 prove a message, so one burst gives a message and a carrier estimate, and a burst of any
 * other device gives nothing.  With decode on, every chunk carries one more launch behind k_chan_bursts.  All quantities
 * are exact integers.  SL = symbol_length, N = packet_symbols, sync = the preamble's bits; LOOK_W = ceil((N SL + 1) / 128),
 * LOOK = 128 LOOK_W (9 windows for SL 14, N 80), MAX_W = 32.  Channel c of chunk k: b = its channelized bytes, continued to
 * t < 0 by chunk k-1's bytes (t + block_size); have_prev: a chunk has been submitted since create / reset; a = 2 b - 255,
 * z[t] = aI[t] + j aQ[t], p[t] = z[t] conj(z[t-1]).  For every rd_burst of that channel and chunk:
 *   1. windows > MAX_W: not decoded, counted in long_runs[c].    2. (corr_re, corr_im) = (0, 0): skipped.
 *   3. region t0 = 128 first - (LOOK if (flags & 1) and have_prev else 0), t1 = 128 (first + windows); skipped when
 *      t1 - t0 < N SL + 1.
 *   4. d[t] = im p[t] corr_re - re p[t] corr_im for t0 < t < t1 (Im of p times the conjugate of the run's own correlation
 *      sum); s[t] = sum_{i < SL} d[t - i] for t0 + SL <= t < t1 (|s| < 2^54); bit[t] = s[t] > 0.
 *   5. candidate tau, the end of the first symbol: t0 + SL <= tau and tau + SL (N - 1) < t1; symbols bit[tau + SL i],
 *      i < N; the first 16 equal sync; the N symbols, packed MSB first into N / 8 on-air bytes, pass the CRC gate of
 *      rd_parse_packet (CRC-16-CCITT over the bit-swapped bytes [2:] is 0); and the packet ends in this chunk,
 *      tau + SL (N - 1) >= 0 - a message is reported with the chunk in which its packet ends, as the demodulator does.
 *      This rule alone does not keep the look-back from reporting a packet twice: a packet has about SL - 2 adjacent
 *      valid taus, so when its last symbol ends within SL outputs of the chunk boundary, chunk k can report a tau that
 *      ends before the boundary and chunk k+1 one that ends after it.  Step 7 drops the second report.
 *   6. at most one record per run: the candidate with the largest margin = min_i |s[tau + SL i]|, ties to the smallest tau.
 *   Repair (rd_wb_set_burst_repair; off by default, and then nothing below applies).  R = max_flips is 0, 1 or 2,
 *   L = RD_BD_REPAIR_L = 8.  The CRC of rd_parse.h has init 0, so it is linear over GF(2): for 16 <= k < N, E[k] is the
 *   CRC-16 of the bit-swapped bytes [2:] of the packet whose only set symbol is k, and flipping the symbols of a set F
 *   turns a packet of syndrome S (the CRC of step 5, S != 0) into a valid one exactly when the E[k], k in F, XOR to S.
 *   5a. a candidate tau that meets every condition of step 5 except the CRC gate is repairable when R > 0 and a flip set
 *       exists by 5b.  The first 16 symbols must still equal sync exactly: sync symbols are never flipped.
 *   5b. the flip set: rank the payload symbols k = 16 .. N-1 by |s[tau + SL k]| ascending, ties to the smaller k;
 *       r_0 .. r_7 are the first L.  Subsets are tried in this order: the singles {r_a}, a ascending; then, if R = 2, the
 *       pairs {r_a, r_b}, a < b, ordered by (a, b).  The flip set is the first subset whose E values XOR to S.  The order
 *       is fixed because the answer is not unique: the generator x^16 + x^12 + x^5 + 1 is itself a codeword of weight
 *       4, so two different pairs can share a syndrome.
 *   6'. replaces step 6: at most one record per run; the candidates are ordered by (flips ascending, margin descending,
 *       tau ascending), flips = 0 for a candidate that passes the CRC as it is; the margin of a repaired candidate is
 *       the minimum of |s| over the symbols that were NOT flipped.  An exact candidate always beats a repaired one: a run
 *       that yields a record at R = 0 yields the same record, bit for bit, at any R.
 *   The record of a repaired candidate: flags bit 1 (RD_BURST_MSG_REPAIRED) is set; pad[0] = the number of flips, pad[1]
 *   and pad[2] the flipped symbol indices ascending (pad[2] = 0 for one flip), pad[3] = 0; data, ones and id come from the
 *   corrected symbols; tau, time, f_re, f_im and first are as for any record.  An unrepaired record has pad = 0 and bit 1
 *   clear.  Step 7 is unchanged: it compares the corrected data and tests flags & 1 only.
 *   What a repaired record proves: less than a CRC-proven one.  Against a random syndrome a candidate is accepted with
 *   probability at most 8 / 65535 at R = 1 (8 singles) and at most 36 / 65535 at R = 2 (8 singles + 28 pairs), where an
 *   exact candidate has 1 / 65536; and a real packet has about SL - 2 adjacent candidates, each with its own list.  Bit 1
 *   is there so that the caller can treat the two classes differently (rtldavis_amd/acquire.py ignores repaired rows
 *   unless asked).  Not repaired: flips inside the sync word, more than two flips, symbols outside the list.
 *   Narrow-band filter (rd_wb_set_burst_narrow; off by default, and then nothing below applies).  The channel filter
 *   passes +-110 kHz because the carrier may be anywhere in it; a burst occupies about +-15 kHz, and the discriminator of
 *   step 4 multiplies all of that noise with itself.  With the filter on, step 4 is replaced by 4n; steps 1 - 3, 5, 5a,
 *   5b, 6, 6' and 7 run unchanged on the new s[t].  It needs SL >= 4.  G = RD_BD_NB_GRID = 64, T = 2 SL + 5 taps,
 *   M = SL + 2.  Tables, designed on the host in float64 (rd_bd_narrow_table, rd_host.cpp), k = -M .. M:
 *     w[k] = 0.54 + 0.46 cos(2 pi k / (T - 1));  h[k] = sinc(1.8 k / SL) w[k] / sum, sinc(x) = sin(pi x) / (pi x), the sum
 *     (over k ascending) making sum_k h[k] = 1: a low-pass with its cutoff at 0.9 symbol rates;
 *     H[g][k] = (rint(2^14 h[k] cos(a)), rint(2^14 h[k] sin(a))), a = 2 pi ((g k) mod 64) / 64 - the product reduced in
 *     integers to 0 .. 63 before the call -, an int16 pair;  C[g] = (rint(2^14 cos(2 pi g / 64)), rint(2^14 sin(2 pi g / 64))).
 *   4n. per run, after steps 1 - 3: sh = max(0, bitlength(max(|corr_re|, |corr_im|)) - 15), ca = corr_re >> sh,
 *       cb = corr_im >> sh (arithmetic shifts: floor; not both 0, each in -2^15 .. 2^15 - 1); g = the smallest g that
 *       maximises ca C[g].re + cb C[g].im (|score| < 2^30).  z[t] as above for t0 <= t < t1 and 0 outside the region - no
 *       state, no load beyond the region.  acc[t] = sum_{k = -M .. M} H[g][k] z[t - k] (complex);
 *       y[t] = (acc[t] + 2^10) >> 11 per component (RD_BD_NB_SHIFT, arithmetic shift).  The largest
 *       sum_k (|H.re| + |H.im|) over g is 25633 at SL 4, 24727 at 8, 23986 at 14, 23471 at 25 and 23181 at 51, so
 *       |acc| <= 255 x 25633 < 2^23 and |y| <= 3192 per component.  p'[t] = y[t] conj(y[t-1]) for t0 < t < t1 (components
 *       < 2^25);  d[t] = im p'[t] ca - re p'[t] cb;  s[t] = sum_{i < SL} d[t - i] for t0 + SL <= t < t1: the SL-sums of p'
 *       stay below 2^31 and |s| < 2^47;  bit[t] = s[t] > 0.
 *   The record of a run decoded this way: flags bit 2 (RD_BURST_MSG_NARROW) is set; pad[3] = g; f_re, f_im = the sum of
 *   p' over the packet's N SL outputs (< 2^36); margin is in the units of the new s - not comparable with a record
 *   without bit 2; everything else as for any record.  Repair composes with it: pad = (flips, k1, k2, g),
 *   flags = 4 | 2 | back.
 *   7. on the host, when the fetch of chunk k+1 copies the records out: a record with flags & 1 is dropped when its
 *      channel and data equal those of a record that the fetch of chunk k delivered (after its own drop) and its time
 *      differs from that record's by less than SL.  The device cannot do this: chunk k slices with another run's
 *      correlation sum and may not have decoded the packet at all.  n_msgs and the records rd_wb_burst_messages hands out
 *      are those after the drop; rd_wideband_reset forgets the previous chunk's records; a chunk that was never fetched
 *      (dropped after a timeout) delivered none.
 * A rd_burst that k_chan_bursts never writes - windows = 0, first >= nW, first + windows > nW, or a place past the
 * channel's ceil(nW / 2) - is skipped (after step 1).
 * Records: channels ascending, a channel's runs ascending.  The same chunks and thresholds give the same bits on every run.
 * Not solved here, for a station never yet heard: a packet of which only the last few outputs reach into a chunk whose
 * window 0 stays OFF, a run of more than 32 windows, and a packet that ends a few outputs into a chunk whose run holds
 * nothing but the transmission's trailing symbols are missed.  For a station heard once, BURST EXPECT below decodes at
 * the predicted place without a run and has none of the three gaps; BURST SEARCH, further below, tests every position
 * of every channel and needs neither a run nor a station heard before.  A burst the demodulator decodes too is reported by
 * both paths (rd_wb_parsed and here): the caller dedupes by channel, chunk and data.
 * rd_wb_set_burst_decode: on / off (the default: nothing is launched).  Needs a quiet receiver (RD_ERR_STATE otherwise),
 * like rd_wb_set_bursts, and bursts on (RD_ERR_STATE otherwise; rd_wb_set_bursts(w, 0) switches decode off too).
 * RD_ERR_ARG for a configuration other than preamble_symbols = 16, N a multiple of 8 in 40 .. 8 RD_BURST_MSG_BYTES,
 * N SL + 1 <= 2048, or with block_size < LOOK.  No device work (safe before fork).
 * rd_wb_burst_messages: the records of the chunk the last fetch returned, kept by that fetch - valid with later chunks in
 * flight, until the next fetch.  *n = the number of records; with cap < *n: RD_ERR_CAPACITY, nothing is lost, call again
 * (out may be NULL with cap = 0).  long_runs: NULL, or room for n_channels counts.  RD_ERR_STATE before any fetch and when
 * that chunk was submitted with decode off.
 * rd_wb_set_burst_repair: max_flips = R for the chunks submitted from now on; 0 (the default) is the behaviour without
 * repair, byte for byte.  RD_ERR_ARG outside 0 .. 2; RD_ERR_STATE unless the receiver is quiet and burst decode is on;
 * rd_wb_set_burst_decode(w, 0) and rd_wb_set_bursts(w, 0) put it back to 0, rd_wideband_reset keeps it.  A chunk's records
 * come from the value in force when it was submitted.  No device work (safe before fork).  rd_wb_burst_repair: the value
 * the next submitted chunk will use.
 * rd_wb_set_burst_narrow: step 4n on / off for the chunks submitted from now on; off (the default) is the behaviour
 * without it, byte for byte.  RD_ERR_STATE unless the receiver is quiet and burst decode is on; RD_ERR_ARG when switched
 * on with symbol_length < 4; rd_wb_set_burst_decode(w, 0) and rd_wb_set_bursts(w, 0) switch it off, rd_wideband_reset
 * keeps it.  A chunk's records come from the value in force when it was submitted.  No device work (safe before fork):
 * the next submit uploads the tables.  rd_wb_burst_narrow: the value the next submitted chunk will use. */
#define RD_BURST_MSG_BYTES 10    /* packet_symbols / 8 at most */
#define RD_BURST_MSG_REPAIRED 2u /* rd_burst_msg.flags: the symbols pad[1] (and pad[2]) were flipped to satisfy the CRC */
#define RD_BD_REPAIR_L 8         /* the least reliable payload symbols a repair may flip */
#define RD_BURST_MSG_NARROW 4u   /* rd_burst_msg.flags: decoded behind the narrow-band filter of step 4n, pad[3] = g */
#define RD_BD_NB_GRID 64         /* G: the centre frequencies of step 4n, g / 64 cycles per output */
#define RD_BD_NB_SHIFT 11        /* y = (acc + 2^10) >> 11 */
#define RD_BD_NB_MIN_SL 4        /* step 4n needs symbol_length >= 4 ... */
#define RD_BD_NB_MAX_SL 51       /* ... and N SL + 1 <= 2048 with N >= 40 leaves no more: 2 SL + 5 <= 107 taps */
typedef struct rd_burst_msg {
    int32_t  channel;
    uint32_t first;          /* the run's first window (its rd_burst); with bit 3: the expectation's index in its table */
    int32_t  tau;            /* the end of the first symbol, relative to the chunk's first output; may be negative */
    uint32_t flags;          /* bit 0: the region reached into the previous chunk; bit 1 (RD_BURST_MSG_REPAIRED): repaired;
                                bit 2 (RD_BURST_MSG_NARROW): step 4n; bit 3 (RD_BURST_MSG_EXPECTED): a record of BURST EXPECT,
                                whose bit 0 says that the region began before the chunk; bit 4 (RD_BURST_MSG_SEARCHED): a
                                record of BURST SEARCH, whose bit 0 says that the packet began before the chunk, `first` is
                                the centre's index in the list and pad = (hits, 0, 0, g); bit 5 (RD_BURST_MSG_REPLAYED): a
                                record of CLIP DECODE, `first` is the job's index */
    uint64_t time;           /* the chunk's absolute output clock + tau */
    uint64_t margin;         /* min_i |s[tau + SL i]|, for a repaired record over the symbols that were not flipped; in
                                the units of step 4n when bit 2 is set: not comparable across the two kinds */
    int64_t  f_re, f_im;     /* sum of p[t] (bit 2: of p'[t]) over the packet's N SL outputs tau - SL + 1 .. tau + SL (N - 1) */
    uint8_t  data[RD_BURST_MSG_BYTES];   /* on-air bytes, as rd_packet.data */
    uint8_t  ones;           /* symbols that are 1 */
    uint8_t  id;             /* transmitter id: bit-swapped data[2] & 7 */
    uint8_t  pad[4];         /* pad[0 .. 2]: all 0, or for a repaired record pad[0] = flips (1, 2), pad[1] < pad[2] the flipped
                                symbols (pad[2] = 0 for one flip); pad[3]: 0, or g of step 4n when flags bit 2 is set */
} rd_burst_msg;
int rd_wb_set_burst_decode(rd_wideband *w, int enabled);
int rd_wb_set_burst_repair(rd_wideband *w, int max_flips);
int rd_wb_burst_repair(rd_wideband *w, int *max_flips);
int rd_wb_set_burst_narrow(rd_wideband *w, int on);
int rd_wb_burst_narrow(rd_wideband *w, int *on);
/* The tables of step 4n for symbol_length sl, designed on the host (no device is touched): taps = int16 [64][2 sl + 5][2],
 * H[g][k] at [g][k + sl + 2] as (re, im); centres = int16 [64][2], C[g].  RD_ERR_ARG for sl outside 4 .. 51 or a null pointer. */
int rd_bd_narrow_table(int sl, int16_t *taps, int16_t *centres);
int rd_wb_burst_messages(rd_wideband *w, rd_burst_msg *out, int cap, int *n, uint32_t *long_runs, int n_channels);
/* BURST EXPECT (k_chan_burst_expect, rd_burst_expect.hip): decode where the HOST expects a packet, with no energy gate.
 * BURST DECODE needs a clean run of ON windows first, and its slicing direction is the run's own noisy correlation sum.
 * A station heard once is predictable: its next channel follows from its hop pattern, its next time is one dwell period
 * later to within tens of outputs, and its carrier offset does not change from hop to hop.  An expectation says so
 * (rtldavis_amd/track.py makes the tables), and the kernel decodes exactly there.  With a non-empty table in force, a
 * chunk in which an expectation has candidates carries one more launch behind k_chan_burst_decode.  All quantities are
 * exact integers; SL, N, sync, LOOK, z, p, have_prev are those of BURST DECODE.  Chunk k has clock K (the absolute output
 * clock of its first output) and B = block_size outputs.  For expectation e the candidates of chunk k are the relative
 * tau that meet all of
 *     t_lo <= K + tau <= t_hi  (on the 64-bit clock: differences modulo 2^64);
 *     0 <= tau + SL (N - 1) < B  - the packet ends in this chunk, as everywhere else;
 *     tau - SL >= 0 when !have_prev.
 * No tau qualifies: e is idle in this chunk - header candidates = 0, no record, the record place untouched.  Otherwise
 * tau_a, tau_b = the least and greatest candidate, t0 = tau_a - SL, t1 = tau_b + SL (N - 1) + 1: t0 >= -N SL >= -LOOK, so
 * only chunk k-1 is ever needed, t1 <= B, and t1 - t0 = (tau_b - tau_a) + N SL + 1 <= 4096.
 *   4.  as step 4 of BURST DECODE with (corr_re, corr_im) of e in place of the run's: d[t] = im p[t] corr_re - re p[t]
 *       corr_im for t0 < t < t1, s[t] = sum_{i < SL} d[t - i] for t0 + SL <= t < t1; |s| < 2^41.
 *   4n. (narrow) ca = corr_re, cb = corr_im as they are (sh = 0); g chosen as in BURST DECODE.  z[t] is the chunk's (or,
 *       for t < 0, chunk k-1's) for zf0 <= t < zf1, zf0 = max(t0 - M, have_prev ? -LOOK : 0), zf1 = min(t1 + M, B), and 0
 *       outside: the filter sees the real samples beside the candidates' first and last symbols wherever the two chunks
 *       hold them - a run's edge sits on the zero extension, an expectation's does not.  acc, y for t0 <= t < t1, p', d, s
 *       as in BURST DECODE.
 *   5, 5a, 5b, 6, 6' run unchanged over the candidates tau_a .. tau_b ONLY (a narrower range than the region's).  One
 *       condition more: with e.id < 8, a candidate whose id (bit-swapped data[2] & 7 of the corrected symbols, after 5b)
 *       differs is no candidate.
 *   At most one record per expectation and chunk, a rd_burst_msg: flags = RD_BURST_MSG_EXPECTED | repaired | narrow |
 *   (bit 0: t0 < 0, the region reached below t = 0); first = the expectation's index in the table; channel = e.channel;
 *   every other field as for any record (pad[3] = g with narrow).
 *   Header per expectation: { n_msgs (0 / 1), candidates = tau_b - tau_a + 1 (0: idle), chunk, pad = 0 }.
 *   7'. on the host, at the fetch: an expectation whose window straddles the chunk in which the packet ends can be served
 *       by chunks k and k+1, and a packet has about SL - 2 adjacent valid taus, so both may report it.  An expected record
 *       is dropped when its channel and data equal those of an expected record that the previous fetch delivered (after
 *       its own drop) and the times differ by less than SL.  Two expectations of one table that cover the same packet
 *       each give their own record.
 * A packet may now be reported by up to three paths: rd_wb_parsed, rd_wb_burst_messages and here.  The caller dedupes
 * by channel, time and data.  The same chunks and table give the same bits on every run.
 * rd_wb_set_burst_expect: the table (n entries, at most RD_BX_MAX; n = 0 clears it) in force from the next submitted
 * chunk on, exactly at that boundary.  Host bookkeeping only, like rd_wb_set_burst_threshold: legal with two chunks in
 * flight, calls before a submit collapse into the last, no device work (safe before fork).  RD_ERR_ARG, and nothing
 * changes, for n outside 0 .. 64, a channel outside 0 .. n_channels-1, an id that is neither below 8 nor 0xFF,
 * t_lo > t_hi, t_hi - t_lo > RD_BX_MAX_SPAN, a corr component outside -2^15 .. 2^15-1 or corr = (0, 0).  RD_ERR_STATE
 * unless burst decode is on.  rd_wb_set_burst_decode(w, 0), rd_wb_set_bursts(w, 0) and rd_wideband_reset clear the table
 * (reset restarts the clock the windows refer to).  Repair and narrow in force for a chunk apply to its expectations.
 * rd_wb_burst_expect: the table the next submit will use (*n entries; RD_ERR_CAPACITY with cap < *n).
 * rd_wb_expected_messages: the records of the chunk the last fetch returned, after step 7', kept by that fetch; capacity
 * and state rules are those of rd_wb_burst_messages.  candidates: NULL, or room for n_cand = RD_BX_MAX counts - entry i
 * is the header's count of expectation i of the table that chunk was submitted with, RD_BX_NO_ENTRY past its end.  A
 * chunk submitted with an empty table gives *n = 0, not an error. */
#define RD_BURST_MSG_EXPECTED 8u /* rd_burst_msg.flags: decoded at an expectation; `first` is its index in the table */
#define RD_BX_MAX 64             /* expectations per table */
#define RD_BX_MAX_SPAN 2048      /* t_hi - t_lo at most */
#define RD_BX_ANY_ID 0xFFu       /* rd_expect.id: a message of any transmitter */
#define RD_BX_NO_ENTRY 0xFFFFFFFFu
typedef struct rd_expect {
    int32_t  channel;            /* 0 .. n_channels-1 */
    uint32_t id;                 /* 0 .. 7: only a message of this transmitter; RD_BX_ANY_ID: any */
    uint64_t t_lo, t_hi;         /* absolute output clock of the end of the first symbol (rd_burst_msg.time), inclusive */
    int32_t  corr_re, corr_im;   /* the direction to slice around: each in -2^15 .. 2^15-1, not both 0 */
} rd_expect;
int rd_wb_set_burst_expect(rd_wideband *w, const rd_expect *e, int n);
int rd_wb_burst_expect(rd_wideband *w, rd_expect *out, int cap, int *n);
int rd_wb_expected_messages(rd_wideband *w, rd_burst_msg *out, int cap, int *n, uint32_t *candidates, int n_cand);
/* BURST SEARCH (k_chan_burst_search, rd_burst_search.hip): find a station NEVER yet heard, with no energy gate and no
 * prior knowledge of time.  BURST DECODE needs a clean run of ON windows and BURST EXPECT a station heard before; between
 * the level at which a run is found and the level at which an expectation still decodes lie about 7 dB.  The sync word
 * 0xCB89 has eight ones and eight zeros, so behind the narrow-band filter the sum of the 16 sync symbols' phase-difference
 * sums points along the carrier, and each symbol can be sliced around that sum: sync equality plus CRC-16 then prove a
 * message at every output position of every channel.  The host passes a short list of filter centres (one centre covers
 * about +-2 grid steps at moderate noise, +-1 near the limit; rtldavis_amd/acquire.py: search_centres).  With a non-empty
 * list in force a chunk carries one more launch, behind k_chan_burst_expect (or k_chan_burst_decode) and in front of the
 * demodulator: a price, one filter pass over every channel per centre.  All quantities are exact integers.  SL, N, sync,
 * LOOK, have_prev, z, the tables H[g] and C[g], M = SL + 2 and the shift RD_BD_NB_SHIFT are those of BURST DECODE step 4n.
 * Chunk k has clock K and B = block_size outputs; lo = have_prev ? -LOOK : 0.  For every channel c and every centre g_i
 * of the list (i ascending):
 *   1s. z[t] is the chunk's own for lo <= t < B, chunk k-1's for t < 0, and 0 outside lo .. B-1 at both ends.
 *       y[t] = (sum_k H[g][k] z[t-k] + 2^10) >> 11 for lo <= t < B.  p'[t] = y[t] conj(y[t-1]) for lo < t < B.
 *       S[t] = sum_{i < SL} p'[t-i], complex with components below 2^31, for lo + SL <= t < B.
 *   2s. candidates: tau with max(lo + SL, -SL (N-1)) <= tau <= B - 1 - SL (N-1).  The packet ends in this chunk, as
 *       everywhere else; the candidates of consecutive chunks do not overlap.
 *   3s. per tau: D = sum_{k < 16} S[tau + SL k], components below 2^35.  D = (0, 0): no candidate.
 *       sh = max(0, bitlength(max(|D.re|, |D.im|)) - 15), ca = D.re >> sh, cb = D.im >> sh (arithmetic: floor, as in 4n);
 *       ca = cb = 0: no candidate.  s_k = S[tau + SL k].im ca - S[tau + SL k].re cb for k < N, |s| < 2^47; bit_k = s_k > 0.
 *       The first 16 bits equal sync - such a position counts in sync_hits -, and the N symbols pass the CRC gate of
 *       BURST DECODE step 5.  margin = min_{k < N} |s_k|.  No repair, whatever max_flips is: a repaired candidate passes
 *       a random syndrome up to 36 times as often, and the search tests every position.  A sync word with other than
 *       eight ones is accepted as configured, and then D is biased towards the more frequent symbol's frequency by
 *       (ones - 8) / 16 of the deviation's phase step: the slicing direction is off by that much.
 *   4s. a passing tau is reported unless another passing tau' of the same (c, g_i) with |tau' - tau| < SL has a larger
 *       margin, or the same margin and tau' < tau.  hits = the passing tau' with |tau' - tau| < SL, tau itself included
 *       (at most 2 SL - 1 <= 101).
 *   5s. per (i, c) at most RD_BS_PER = 4 records, the first four reported by tau, in fixed places of the slot.  Header per
 *       (i, c): { n_msgs, sync_hits, chunk, dropped }, dropped = the reported taus beyond the fourth.  The record is a
 *       rd_burst_msg: flags = RD_BURST_MSG_SEARCHED | RD_BURST_MSG_NARROW | (bit 0: tau - SL < 0); first = i;
 *       pad = (hits, 0, 0, g); f_re, f_im = the sum of p' over the packet's N SL outputs (= sum_{k < N} S[tau + SL k]), so
 *       a carrier estimate follows as for any narrow record; tau, time, margin, data, ones, id as for any record.
 *   7s. on the host, at the fetch: a searched record is dropped when its channel, pad[3] and data equal those of a
 *       searched record that the previous fetch delivered (after its own drop) and the times differ by less than SL.  Two
 *       centres that both decode a packet each give their record; the caller dedupes by channel, time and data.
 * Records: centres in list order, channels ascending, a (centre, channel)'s records by tau.  The same chunks and centres
 * give the same bits on every run, and the result does not depend on how the kernel tiles a channel (RD_BS_TILE
 * candidates per tile; every tile computes its halos again from the bytes).
 * What a searched record proves: less per hour than any other record.  A random position passes the sync test with
 * probability about 2^-16 and the CRC with 2^-16; a receiver of 51 channels and 8192 outputs per chunk tests 4 x 10^5
 * positions per chunk and centre, which gives a false record every few minutes per centre (derived).  Bit 4 is there so
 * that the caller can treat such a record as provisional (rtldavis_amd/track.py does).  hits and margin are reported and
 * not gated on: a real packet has about SL - 2 adjacent passing positions, a false one has one.
 * rd_wb_set_burst_search: the list (n centres, 0 .. RD_BS_MAX_CENTRES; n = 0, the default, clears it, and then nothing is
 * launched and every other call returns what it returns without this section, byte for byte) in force from the next
 * submitted chunk on.  Host bookkeeping like rd_wb_set_burst_expect: legal with two chunks in flight, no device work.
 * RD_ERR_ARG, and nothing changes, for n outside 0 .. 8, a centre >= 64, a duplicate, symbol_length < 4, or a
 * configuration that rd_wb_set_burst_decode refuses; RD_ERR_STATE unless burst decode is on.  rd_wb_set_burst_decode(w, 0)
 * and rd_wb_set_bursts(w, 0) clear the list; rd_wideband_reset keeps it and forgets step 7s's memory.
 * rd_wb_burst_search: the list the next submit will use (*n centres; RD_ERR_CAPACITY with cap < *n).
 * rd_wb_searched_messages: the records of the chunk the last fetch returned, after step 7s, kept by that fetch; capacity
 * and state rules are those of rd_wb_expected_messages.  hdr: NULL, or room for n_hdr = RD_BS_MAX_CENTRES x n_channels
 * headers - [i][c] is the header of centre i of the list that chunk was submitted with and channel c, its n_msgs the
 * device's count BEFORE step 7s; every field is RD_BX_NO_ENTRY past the list's end.  A chunk submitted with an empty list
 * gives *n = 0, not an error. */
#define RD_BURST_MSG_SEARCHED 16u /* rd_burst_msg.flags: found by BURST SEARCH; `first` is the centre's index in the list */
#define RD_BS_MAX_CENTRES 8       /* centres per list */
#define RD_BS_PER 4               /* records per (centre, channel) and chunk */
#define RD_BS_TILE 1024           /* candidates per tile of k_chan_burst_search (tests place packets across its boundaries) */
typedef struct rd_bs_header {
    uint32_t n_msgs, sync_hits;
    uint32_t chunk;               /* the chunk's sequence number since create / reset, its low 32 bits */
    uint32_t dropped;
} rd_bs_header;
int rd_wb_set_burst_search(rd_wideband *w, const uint8_t *centres, int n);
int rd_wb_burst_search(rd_wideband *w, uint8_t *out, int cap, int *n);
int rd_wb_searched_messages(rd_wideband *w, rd_burst_msg *out, int cap, int *n, rd_bs_header *hdr, int n_hdr);
/* BURST QUALITY (k_chan_burst_quality, rd_burst_quality.hip): the power, the noise in front and the clipping of every
 * record of BURST DECODE and BURST EXPECT - what the demodulator path reports as rd_packet.rssi / .snr, in integers, and
 * the same behind the narrow-band filter of step 4n (an in-band figure: the one that corresponds to what the narrow
 * decoder can do).  With quality on, a chunk carries one more launch behind k_chan_burst_decode and one behind
 * k_chan_burst_expect when that was launched; the kernels in front are not changed.  All quantities are exact integers in
 * the notation of BURST DECODE (b, a = 2 b - 255, z, SL, N, M = SL + 2, T = 2 SL + 5, H[g], C[g], have_prev); B = block_size.
 * A record of channel c with first symbol end tau: the first output of its packet is P0 = tau - SL + 1.  Windows:
 *     packet   P0 .. P0 + N SL - 1
 *     sync     P0 .. P0 + 16 SL - 1                          (the reference's preamble_iq)
 *     noise    P0 - gap - 16 SL .. P0 - gap - 1, intersected with t >= lo_lim;  lo_lim = -B with have_prev, else 0
 * n_noise = the outputs the intersection leaves, 0 .. 16 SL.  With gap = 0 this is the reference's noise window.  gap
 * (noise_gap, 0 .. RD_BQ_MAX_GAP outputs) is a parameter because what a real transmitter sends in front of its sync word
 * has NOT been measured in this project: the synthetic bursts of the tests have a lead-in of alternating symbols there,
 * and then the window holds signal, not noise (rtldavis_amd/acquire.py: snr_floor_db takes the noise from the channel's
 * OFF windows instead).  A default, not a measurement - as Tracker's period and guard.
 * Raw sums of |z[t]|^2 = aI^2 + aQ^2 (<= 130050): pkt, sig, noise over the three windows; each at most 2047 x 130050
 * < 2^28.  peak = the maximum over the packet of max(|aI|, |aQ|) (1 .. 255); clipped = the bytes equal to 0 or 255 among
 * the packet's 2 N SL bytes.
 * In-band sums, valid only when flags bit 0 is set: g by the rule of step 4n applied to the record's own (f_re, f_im) -
 * sh = max(0, bitlength(max(|f_re|, |f_im|)) - 15) on the 64-bit values, ca = f_re >> sh, cb = f_im >> sh (arithmetic),
 * the smallest g that maximises ca C[g].re + cb C[g].im.  The same rule for records with and without flags bit 2: it is
 * NOT pad[3], which followed from the run's correlation sum.  y[t] = (sum_{k = -M .. M} H[g][k] z[t - k] + 2^10) >> 11
 * per component with z = 0 outside lo_lim <= t < B, exactly as in 4n.  pkt_nb, sig_nb, noise_nb = the sums of
 * |y[t]|^2 over the same three windows: |y| <= 3192 per component, so |y|^2 <= 2 x 3192^2 = 20377728 < 2^25 and a sum
 * over at most 2047 outputs is below 2^25 x 2^11 = 2^36.  Bit 0 is clear and the four in-band fields (and g) are 0 when
 * SL < 4 or (f_re, f_im) = (0, 0).
 * Before it indexes anything the kernel checks again that 0 <= c < n_channels, P0 >= lo_lim and P0 + N SL <= B (tau taken
 * as a 64-bit value: no tau overflows the test); a record that fails gets flags = RD_BQ_UNMEASURABLE and zeros elsewhere
 * (chunk excepted).  Quality record i of a slot belongs to message record i of the slot it was launched over.  The same
 * bytes, records and gap give the same bits on every run.
 * rd_wb_set_burst_quality: on / off and noise_gap for the chunks submitted from now on.  Off is the default: then nothing
 * is launched and every other call returns what it returns without this section, byte for byte.  RD_ERR_ARG for noise_gap
 * outside 0 .. 1024 (checked first); RD_ERR_STATE unless the receiver is quiet and burst decode is on;
 * rd_wb_set_burst_decode(w, 0) and rd_wb_set_bursts(w, 0) switch it off, rd_wideband_reset keeps it.  A chunk's records
 * come from the values in force when it was submitted.  No device work (safe before fork).  rd_wb_burst_quality: the
 * values the next submitted chunk will use.
 * rd_wb_burst_message_quality / rd_wb_expected_message_quality: row i belongs to row i of rd_wb_burst_messages /
 * rd_wb_expected_messages of the same fetch, after steps 7 / 7' - the fetch drops a dropped record's quality with it.
 * *n = the number of rows; with cap < *n: RD_ERR_CAPACITY, nothing is lost, call again (out may be NULL with cap = 0).
 * RD_ERR_STATE before any fetch, and when the last fetched chunk was submitted with quality off. */
#define RD_BQ_MAX_GAP 1024       /* noise_gap at most */
#define RD_BQ_INBAND 1u          /* rd_burst_quality.flags: g, pkt_nb, sig_nb, noise_nb are valid */
#define RD_BQ_UNMEASURABLE 128u  /* rd_burst_quality.flags: the record's channel or tau is out of range; every sum is 0 */
typedef struct rd_burst_quality {
    uint64_t pkt, sig, noise;              /* sums of |z|^2 over the packet, the sync word, the noise window */
    uint64_t pkt_nb, sig_nb, noise_nb;     /* the same of |y|^2 (flags bit 0) */
    uint32_t n_noise, clipped;
    uint16_t peak; uint8_t g; uint8_t flags;   /* bit 0: in-band fields valid; bit 7: the record was not measurable */
    uint32_t chunk;                        /* the chunk's sequence number since create / reset, its low 32 bits */
} rd_burst_quality;
int rd_wb_set_burst_quality(rd_wideband *w, int on, int noise_gap);
int rd_wb_burst_quality(rd_wideband *w, int *on, int *noise_gap);
int rd_wb_burst_message_quality(rd_wideband *w, rd_burst_quality *out, int cap, int *n);
int rd_wb_expected_message_quality(rd_wideband *w, rd_burst_quality *out, int cap, int *n);
/* The windows of one record, on the host (no device is touched): out = { p0, p1, s1, n0, n1 } - packet p0 .. p1 - 1, sync
 * p0 .. s1 - 1, noise n0 .. n1 - 1 (n0 = n1 = p0 when nothing of it is left).  Returns 1, or 0 with out zeroed for a record
 * that is not measurable (or a null out). */
int rd_bq_window(int sl, int n_sym, int block_size, int have_prev, int64_t tau, int gap, int32_t *out);
/* BURST CLIPS (k_chan_burst_clips, rd_burst_clips.hip): the channelized IQ bytes of every burst, cut out on the device -
 * the bursts that were decoded, those that were not, those of other devices on the band, with what lies in front of and
 * behind each.  The host cannot fetch them afterwards: with two chunks in flight chunk k's channelized buffer is being
 * overwritten by the time the host has read chunk k's records.  With clips on, a chunk carries one more launch behind its
 * last burst kernel and in front of the demodulator; the kernels in front are not changed.  A clip is a copy of bytes,
 * nothing else.  Notation of BURST DECODE: B = block_size, K = the chunk's absolute output clock, have_prev,
 * lo_lim = -B with have_prev else 0; channel c's bytes are continued to t < 0 by chunk k-1's bytes.
 * Settings: sources = a bit mask, RD_BC_RUNS (every rd_burst of k_chan_bursts) | RD_BC_MESSAGES (every row the decode,
 * expect and search kernels wrote for this chunk), 0 = off; pre, post = the outputs in front of and behind a request, each
 * a multiple of 8 in 0 .. RD_BC_MAX_ROLL; quota Q = the outputs per channel and chunk, a multiple of 8 in 8 .. 65536 with
 * n_channels Q 2 <= 2^26 bytes; RD_BC_PER = 16 clip records per channel and chunk.
 * A request is a half-open interval [a, e) of outputs of one channel, relative to the chunk's first output:
 *     source                                          a                 e                              ref
 *     1 run: an rd_burst k_chan_bursts really wrote   128 first - pre   128 (first + windows) + post   first
 *     2, 3, 4 message row, first symbol end tau,      P0 - pre          P0 + N SL + post               the row's time
 *       P0 = tau - SL + 1
 *     0 tail                                          0                 owed                           0
 * Runs: the "never writes" rule of BURST DECODE applies - windows = 0, first >= nW, first + windows > nW or a place past
 * ceil(nW / 2) is skipped; windows > MAX_W is no obstacle here.  Message rows are those of the decode slot of channel c
 * (source 2), the rows of the expect slot whose channel is c (3) and the rows of the search slot of channel c (4), as the
 * kernels wrote them - before the host's steps 7 / 7' / 7s.  A slot whose kernel was not launched for this chunk
 * contributes nothing.  A row whose channel field is not c - out of range included - or that fails the test of BURST
 * QUALITY (tau as a 64-bit value; lo_lim <= P0 and P0 + N SL <= B) is skipped.
 * Tail: the post-roll the previous chunk could not deliver.  When the previous chunk of this receiver was submitted with
 * clips on and its header of channel c says 0 < owed <= RD_BC_MAX_ROLL, the first request of channel c is the tail.
 * Clamping (rd_bc_window): t0 = max(a, lo_lim) rounded down to a multiple of 8, t1 = min(e, B) rounded up to one,
 * n = t1 - t0; a request with n <= 0 (or e <= a) is skipped.  lo_lim and B are multiples of 8, so every clip is whole
 * 16-byte vectors that lie in one chunk each.  flags: bit 0 RD_BC_CUT_START: a < lo_lim; bit 1 RD_BC_CUT_END: e > B; bit 2
 * RD_BC_FROM_PREV: t0 < 0, bytes of the previous chunk are included.
 * Order of a channel's requests: the tail; runs in record order; decode rows in record order; expect rows by table index;
 * search rows by (centre index, place).  Allocation is in that order: a request gets offset = the outputs used so far; it
 * is dropped whole, and counted in `dropped`, when offset + n > Q or RD_BC_PER records are already written; later
 * requests are still tried.  Overlapping requests are not merged: each gets its own copy (rtldavis_amd/clips.py merges).
 * owed for the next chunk = the maximum of e - B over the clips WRITTEN with RD_BC_CUT_END, at most RD_BC_MAX_ROLL; a tail
 * that is cut again carries its remainder on (B < owed).
 * A clip's bytes are outputs t0 .. t1 - 1 of the channel as they lie, 2 bytes each.  Header per channel: { n_clips,
 * dropped, owed, used (outputs), chunk, pad = 0 }.  The same chunks, records and settings give the same bits on every run:
 * one workgroup per channel, no atomics, the list built in one fixed order.
 * rd_wb_set_burst_clips: the values for the chunks submitted from now on; sources = 0, the default, is off - then nothing
 * is launched and every other call returns what it returns without this section, byte for byte.  RD_ERR_ARG (checked
 * first) for unknown source bits, a roll or quota outside its range or no multiple of 8, or a pool over 2^26 bytes;
 * RD_ERR_STATE unless the receiver is quiet and bursts are on, and for RD_BC_MESSAGES unless burst decode is on.
 * rd_wb_set_bursts(w, 0) switches clips off; rd_wb_set_burst_decode(w, 0) clears RD_BC_MESSAGES, and switches clips off
 * when nothing is left.  rd_wideband_reset keeps the settings and forgets owed.  No device work (safe before fork): the
 * first submit with clips in force allocates the slots.  rd_wb_burst_clips_config: the values the next submit will use.
 * rd_wb_burst_clips: the clips of the chunk the last fetch returned, kept by that fetch - which copies only the used part
 * of each channel's pool - and valid with later chunks in flight, until the next fetch.  Channels ascending, a channel's
 * clips in their order; `offset` is rewritten to the clip's place in the packed `bytes`, in outputs (2 bytes each).
 * *n = the records, *n_bytes = the bytes; with cap < *n or bytes_cap < *n_bytes: RD_ERR_CAPACITY, nothing is lost, call
 * again (out / bytes may be NULL with a capacity of 0).  dropped: NULL, or room for n_channels counts.  RD_ERR_STATE before
 * any fetch and when that chunk was submitted with clips off. */
#define RD_BC_RUNS 1u
#define RD_BC_MESSAGES 2u
#define RD_BC_MAX_ROLL 1024      /* pre, post and owed at most */
#define RD_BC_MAX_QUOTA 65536
#define RD_BC_MAX_POOL (1u << 26) /* n_channels x quota x 2 bytes at most */
#define RD_BC_PER 16             /* clip records per channel and chunk */
#define RD_BC_CUT_START 1        /* rd_burst_clip.flags */
#define RD_BC_CUT_END 2
#define RD_BC_FROM_PREV 4
typedef struct rd_burst_clip {
    int32_t  channel;
    uint32_t source;   /* 0 tail, 1 run, 2 decode row, 3 expected row, 4 searched row */
    uint32_t flags;
    int32_t  t0;       /* first output, relative to the chunk; may be negative */
    uint32_t n;        /* outputs */
    uint32_t offset;   /* outputs: where the clip lies (see rd_wb_burst_clips) */
    uint64_t time;     /* K + t0 */
    uint64_t ref;
    uint32_t chunk;    /* low 32 bits of the chunk's sequence number */
    uint32_t pad;
} rd_burst_clip;
int rd_wb_set_burst_clips(rd_wideband *w, int sources, int pre, int post, int quota);
int rd_wb_burst_clips_config(rd_wideband *w, int *sources, int *pre, int *post, int *quota);
int rd_wb_burst_clips(rd_wideband *w, rd_burst_clip *out, int cap, int *n, uint8_t *bytes, size_t bytes_cap, size_t *n_bytes,
                      uint32_t *dropped, int n_channels);
/* The clamp of one request, on the host (no device is touched): out = { t0, n, flags }.  Returns 1, or 0 with out zeroed for
 * a request that gives no clip (or a null out, or a block_size that is no positive multiple of 8). */
int rd_bc_window(int block_size, int have_prev, int64_t a, int64_t e, int32_t *out);
/* CLIP DECODE (k_clip_decode, rd_clip_decode.hip): decode RECORDED clips, many per launch.  BURST CLIPS brings the
 * channelized IQ of every burst home; this section asks of such bytes what a live chunk can be asked only once: would
 * this burst have decoded with the filter on, with two flips, around another direction?  No receiver, no channelizer and
 * no chunk are involved.  A POOL is a byte array of channelized IQ (cu8: I, Q per output) that rd_clips_upload copies to
 * the device; a JOB (rd_clip_job) names a clip in it - `n` outputs from output `offset` - and the places to test.  One
 * launch takes up to 2^20 jobs, one workgroup each.  All quantities are exact integers.
 * Semantics: those of BURST EXPECT with the clip taken as a chunk of its own - B = n, clock K = job.clock,
 * have_prev = 0, the expectation (channel, id, t_lo = K + tau_lo, t_hi = K + tau_hi, corr).  B need not be a multiple of 8
 * or of 128, nor reach LOOK.  Written out: the candidates are tau_a = max(tau_lo, SL) .. tau_b = min(tau_hi, n - 1 -
 * SL (N - 1)).  None: the job is idle - no record, and its header reads { 0, 0, 0, 0 }.  Otherwise t0 = tau_a - SL,
 * t1 = tau_b + SL (N - 1) + 1 (0 <= t0, t1 <= n, t1 - t0 <= 4096); with the filter on zf0 = max(t0 - M, 0), zf1 =
 * min(t1 + M, n): the filter sees the clip's real samples where the clip holds them and zeros outside the clip.
 * Steps 4 / 4n, 5, 5a, 5b, 6 / 6' and the id rule of BURST EXPECT run as written, over tau_a .. tau_b only.
 *   Own direction, corr = (0, 0): F = the sum of p[t] over t0 < t < t1 - unfiltered, from the bytes of the job's region,
 *   exact, components below 4096 x 2 x 255^2 < 2^30; sh = max(0, bitlength(max(|F.re|, |F.im|)) - 15), ca = F.re >> sh,
 *   cb = F.im >> sh (arithmetic shifts, as in step 4n).  ca = cb = 0 (F = (0, 0)): candidates is still counted, and there
 *   is no record.  Otherwise (ca, cb) takes the place of corr everywhere, the choice of g included.
 *   At most one record per job, a rd_burst_msg: flags = RD_BURST_MSG_REPLAYED | repaired | narrow - bit 0 and bit 3 are
 *   never set -, first = the job's index, channel = job.channel, tau relative to the clip's output 0, time = clock + tau;
 *   every other field as for an expected record.
 *   Header per job: { n_msgs (0 / 1), candidates = tau_b - tau_a + 1, ca, cb = the direction that was used, given or own }.
 *   Soft values: for a job with a record soft[j][k] = s[tau + SL k], k < N, of the winning tau, before any flip (in the
 *   units of step 4n behind the filter); zeros for a job without a record.
 * Isolation: no byte outside outputs 0 .. n - 1 of a job's clip influences that job's record, header or soft values -
 * the 16-byte loads may touch the 7 outputs past a clip whose n is no multiple of 8, and nothing reads what they bring.
 * The same pool and jobs give the same bits on every run; the order of the jobs and a clip's neighbours change nothing.
 * Out of scope: a replay of BURST SEARCH (its per-position direction is another algorithm, and noise chunks stream
 * through the live search at thousands of chunks per second), the figures of BURST QUALITY, and more than one record per
 * job (rtldavis_amd/replay.py tiles a long recording with jobs instead).
 * rd_clips_create: RD_ERR_ARG for a configuration that rd_wb_set_burst_decode refuses, except the block_size rule -
 * block_size is ignored here.  No device work (safe before fork).
 * rd_clips_upload: the pool (nbytes even, at least 2), copied to the device and kept until the next upload or synthesis
 * (CLIP SYNTH below).
 * rd_clips_decode: synchronous, its wait under the deadline of every host wait (RD_WAIT_TIMEOUT_MS).  Any number of
 * calls on one uploaded pool.  msgs[n_jobs] and hdr[n_jobs]: row j is job j, zeros where there is no record / the job is
 * idle; soft: NULL, or [n_jobs][N].  RD_ERR_ARG, with nothing launched, for max_flips outside 0 .. 2, narrow other than
 * 0 / 1 or with symbol_length < 4, n_jobs outside 1 .. RD_CD_MAX_JOBS, a null pointer, and any job rd_cd_check_jobs
 * refuses; RD_ERR_STATE before any upload.  rd_clips_kernel_ms: the kernel time of the last decode, by device events.
 * rd_cd_check_jobs (no device is touched): RD_OK, or RD_ERR_ARG with *bad = the first offending job (-1: n_jobs itself or
 * a null pointer) and *why naming the rule - offset % 8 != 0, n < 1, offset + n past the pool's pool_outputs, tau_lo >
 * tau_hi, tau_hi - tau_lo > RD_CD_MAX_SPAN, |tau_lo| or |tau_hi| above 2^30, an id that is neither below 8 nor
 * RD_BX_ANY_ID, a corr component outside -2^15 .. 2^15-1, pad != 0.  A job that merely has no candidate is legal and idle. */
#define RD_BURST_MSG_REPLAYED 32u   /* rd_burst_msg.flags bit 5: a record of CLIP DECODE; `first` is the job's index */
#define RD_CD_MAX_SPAN 2048         /* tau_hi - tau_lo at most (= RD_BX_MAX_SPAN) */
#define RD_CD_MAX_JOBS (1 << 20)    /* jobs per call */
#define RD_CD_MAX_TAU (1 << 30)     /* |tau_lo|, |tau_hi| at most */
typedef struct rd_clip_job {
    uint64_t offset;             /* the clip's first output in the pool, in outputs; a multiple of 8 */
    uint64_t clock;              /* absolute output clock of the clip's output 0 (Recording.time); time = clock + tau */
    uint32_t n;                  /* outputs in the clip, any number >= 1 */
    uint32_t id;                 /* 0 .. 7, or RD_BX_ANY_ID */
    int32_t  tau_lo, tau_hi;     /* candidate range, inclusive, relative to the clip's output 0 */
    int32_t  corr_re, corr_im;   /* direction to slice around, each in -2^15 .. 2^15-1; (0, 0): the clip's own */
    int32_t  channel;            /* copied into the record */
    uint32_t pad;                /* 0 */
} rd_clip_job;
typedef struct rd_cd_header { uint32_t n_msgs, candidates; int32_t ca, cb; } rd_cd_header;
typedef struct rd_clips rd_clips;
int rd_clips_create(const rd_config *cfg, rd_clips **out);
void rd_clips_destroy(rd_clips *h);
int rd_clips_upload(rd_clips *h, const uint8_t *pool, size_t nbytes);
int rd_clips_decode(rd_clips *h, const rd_clip_job *jobs, int n_jobs, int max_flips, int narrow, rd_burst_msg *msgs,
                    rd_cd_header *hdr, int64_t *soft);
int rd_clips_kernel_ms(rd_clips *h, float *ms);
int rd_cd_check_jobs(const rd_config *cfg, const rd_clip_job *jobs, int n_jobs, size_t pool_outputs, int *bad, const char **why);
/* CLIP SYNTH (k_clip_synth, rd_clip_synth.hip): fill the pool of CLIP DECODE on the device with synthetic noisy burst
 * clips, one small SPEC (rd_clip_spec) per clip and no host bytes - the replay decoder as a Monte-Carlo instrument.  All
 * quantities are exact integers: tests/clip_synth_cases.py evaluates the same expressions in NumPy and must get the same
 * bytes, and the same specs give the same pool on every machine and every run.
 * Spec k describes a clip of `n` outputs at output `offset` of the pool; its output t (0 <= t < n) is two bytes I, Q.
 *   Burst.  n_sym symbols (0 .. RD_CS_MAX_SYM) whose bits are packed MSB first in bits[] (symbol j is bit 7 - j % 8 of
 *   bits[j / 8]); `pre` outputs of unmodulated carrier in front of them, `post` behind (each 0 .. RD_CS_MAX_PRE).  The
 *   first symbol begins at output `at`, which may be negative or past the clip: the clip cuts the burst.  With SL the
 *   handle's symbol_length, u = t - (at - pre) and L = pre + SL n_sym + post the burst is ON at t iff 0 <= u < L.
 *   Phase.  phi(u) = phase0 + (u + 1) f_c + f_d D(u) mod 2^32, in units of 2^-32 cycle; D(u) = the sum over the burst's
 *   outputs 0 .. u of +1 inside a symbol that is 1, -1 inside a symbol that is 0, 0 in pre / post.  f_c (int32) and f_d
 *   (uint32 < 2^31) are in 2^-32 cycle per output: a Davis burst at the channelizer's IF has f_c = round((-1/4 + cfo /
 *   out_rate) 2^32) and f_d = round(2^32 / (4 SL)).
 *   Table.  T[j] = lrint(16384 cos(2 pi j / 4096)), j < 4096 (rd_cs_table; computed once on the host and uploaded);
 *   c = T[phi >> 20], s = T[((phi - 2^30) mod 2^32) >> 20].
 *   Noise.  Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85), key = (seed's low
 *   word, seed's high word), counter = (t, comp, 0, 0) with comp = 0 for I and 1 for Q; g = the sum of the 16 bytes of
 *   the four output words - 2040.  The noise depends on the seed and on t alone: not on offset, not on the spec's place
 *   in the list, not on a neighbour.
 *   Byte.  S = (256 << 21) + (ON ? amp_q * (c for I, s for Q) : 0) + noise_q * g in int64; byte = clamp((S + 2^21) >> 22,
 *   0, 255), the shift arithmetic: the bytes are centred on 128 - mid-scale of the offset-binary byte, half a byte above
 *   the 127.5 the decoders subtract (z = 2 b - 255) - and rounded half up, so the byte mean of a noise-only clip is 128.  amp_q <= 2^16: the amplitude in bytes is amp_q / 256.  noise_q <= 2^20: sigma in bytes
 *   is noise_q sqrt(16 x 65535 / 12) / 2^22 = noise_q x 295.601 / 2^22.  With both 0 every byte is 128.
 *   Pool.  rd_clips_synth zeroes the whole device pool (hipMemsetAsync on the handle's stream, in front of the launch)
 *   and the kernel then writes each clip in whole vectors of 8 outputs: the slack between a clip's end and the next
 *   multiple of 8 is written as 0, and every byte that belongs to no clip is 0 after the call, whatever the pool held.
 * Rules (rd_cs_check_specs; no device is touched; *bad and *why as rd_cd_check_jobs): 1 <= n_specs <= RD_CS_MAX_SPECS;
 * offset % 8 == 0; 1 <= n <= RD_CS_MAX_N; the specs ascend and do not overlap, offset[k] >= roundup8(offset[k-1] +
 * n[k-1]); offset + n <= pool_outputs; n_sym <= RD_CS_MAX_SYM; pre, post <= RD_CS_MAX_PRE; amp_q <= RD_CS_MAX_AMP;
 * noise_q <= RD_CS_MAX_NOISE; f_d < 2^31; |at| <= 2^30; pad == 0; the bits of bits[] from n_sym on are 0.  The kernel
 * applies the per-spec bounds again: a spec that breaks one writes nothing, so no list makes it store outside the pool.
 * rd_clips_synth: sizes the device pool to pool_outputs (grown as rd_clips_upload grows it, padded to whole vectors),
 * runs the kernel and waits under the deadline of every host wait.  Afterwards the handle is in the state an upload of
 * the same bytes leaves it in: rd_clips_decode works on it, and a later rd_clips_upload replaces it.  RD_ERR_ARG with
 * nothing launched - the pool, and a decode that follows, untouched - for anything rd_cs_check_specs refuses and for a
 * pool_outputs above RD_CS_MAX_POOL.  rd_clips_synth_ms: the device time of the last synthesis, the zeroing included, by
 * device events; rd_clips_kernel_ms keeps its meaning.  rd_clips_download: the pool as the device holds it, uploaded or
 * synthesised; RD_ERR_STATE without a pool, RD_ERR_ARG unless nbytes = 2 pool_outputs. */
#define RD_CS_MAX_SYM 192
#define RD_CS_MAX_PRE 4096
#define RD_CS_MAX_N (1 << 24)
#define RD_CS_MAX_SPECS (1 << 20)
#define RD_CS_MAX_AMP (1u << 16)
#define RD_CS_MAX_NOISE (1u << 20)
#define RD_CS_MAX_AT (1 << 30)
#define RD_CS_MAX_POOL (1ull << 40) /* outputs in a synthesised pool at most (2 TiB: above any device's memory) */
#define RD_CS_TABLE 4096
typedef struct rd_clip_spec {
    uint64_t offset;             /* the clip's first output in the pool, in outputs; a multiple of 8 */
    uint64_t seed;               /* the noise's Philox key */
    uint32_t n;                  /* outputs in the clip, 1 .. RD_CS_MAX_N */
    int32_t  at;                 /* the output at which the first symbol begins, relative to the clip's output 0 */
    uint32_t phase0;             /* 2^-32 cycle */
    int32_t  f_c;                /* carrier, 2^-32 cycle per output */
    uint32_t f_d;                /* deviation, 2^-32 cycle per output, < 2^31 */
    uint32_t amp_q;              /* amplitude in 1/256 byte, at most 2^16 */
    uint32_t noise_q;            /* noise scale, at most 2^20 */
    uint32_t n_sym;              /* symbols, 0 .. RD_CS_MAX_SYM */
    uint16_t pre, post;          /* outputs of plain carrier before and behind the symbols, each 0 .. RD_CS_MAX_PRE */
    uint32_t pad;                /* 0 */
    uint8_t  bits[24];           /* the symbols, MSB first; 0 from bit n_sym on */
} rd_clip_spec;
int rd_clips_synth(rd_clips *h, const rd_clip_spec *specs, int n_specs, uint64_t pool_outputs);
int rd_clips_download(rd_clips *h, uint8_t *out, size_t nbytes);
int rd_clips_synth_ms(rd_clips *h, float *ms);
int rd_cs_check_specs(const rd_clip_spec *specs, int n_specs, uint64_t pool_outputs, int *bad, const char **why);
void rd_cs_table(int16_t out[RD_CS_TABLE]);
/* The number (since create / reset; rd_packet.call of its packets) of the chunk the last fetch returned - the chunk whose
 * records rd_wb_levels, rd_wb_spectrum, rd_wb_bursts and rd_wb_burst_messages hand out, and against which the fetch
 * checked them.  RD_ERR_STATE before any fetch.  Host bookkeeping only. */
int rd_wb_fetched_chunk(rd_wideband *w, uint64_t *chunk);
/* test hook (quiet handle): move the output clock forward by n_out (a multiple of 128), history kept */
int rd_wideband_debug_advance_clock(rd_wideband *w, uint64_t n_out);

/* ---------------------------------------------------------------------------------------------
 * Test hooks of the fused demod kernel (rtldavis_amd/csrc/rd_demod_mfma.hip).  Not part of the
 * drop-in surface: tests/test_mfma_model.py and tests/test_gpu_mfma.py use them to check the tap
 * matrix and the raw matrix-pipe outputs against an integer model.
 * ------------------------------------------------------------------------------------------- */
/* The constant A operand: uint16 [2 digits][3 k-steps][64 lanes][8 elements] f16 bit patterns. */
void rd_debug_mfma_taps(uint16_t *out);
/* The A operand of the 8-output formulation (rd_mfma.h, RD_OPT_B8): uint16 [2 k-steps][64 lanes][8 elements]; a row of
 * the 32-row tile is one digit of one component of one of 8 outputs. */
void rd_debug_mfma_taps8(uint16_t *out);
/* the same matrix compressed for the 2:4-sparse matrix instruction: vals[64][8] f16 bit patterns, idx[64] (rd_mfma.h) */
void rd_debug_mfma_taps8s(uint16_t *vals, uint32_t *idx);
/* Run k_demod_mfma alone on host data: g_out float [n_streams * tiles][2048][2] (kernel units),
 * bits_out the packed signs BEFORE the exact fix-up (words per stream = ceil(n_samples / 32)),
 * fix_out / n_fix the fix-up list it produced ((word index << 4) | group mask).  hist_mode: every
 * stream is preceded by hist_bytes of history (stride = hist_bytes + 2 n_samples, multiples of 16).
 * With g_out the kernel instantiation that also dumps g runs; g_out == NULL launches the instantiation the
 * product uses (no dump, the one global fix-up list) and returns bits_out, fix_out and n_fix alone. */
int rd_debug_demod_mfma(const uint8_t *iq_host, int n_streams, uint32_t n_samples, int hist_mode,
                        uint32_t hist_bytes, float *g_out, uint32_t *bits_out, uint32_t *fix_out,
                        uint32_t fix_cap, uint32_t *n_fix);
/* Test hooks of the burst kernels (rd_bursts.hip, rd_burst_decode.hip), not part of the drop-in surface either:
 * tests/test_burst_kernels_crafted.py puts exact bytes, ties and offsets in front of each kernel alone.  Host arrays in, host
 * arrays out; the bytes are uploaded, the slot is mapped host memory as the receiver allocates it, filled with 0xA5, written
 * by one launch through the product's launch function and copied out WHOLE - cap = ceil(nW / 2) places per channel, those
 * past n_bursts / n_msgs still 0xA5.  No receiver is involved.
 * rd_debug_bursts: chan = n_ch x stride bytes (channel c's 2 n_out bytes at c * stride, stride a multiple of 16);
 * RD_ERR_ARG with nothing launched for an n_out that rd_wb_set_bursts refuses.
 * rd_debug_burst_decode: n_out = cfg->block_size; cur / prev laid out alike (prev NULL: no chunk before); runs[n_ch][cap]
 * and n_runs[n_ch] are written into a burst slot as they are - records k_chan_bursts never writes included; per channel
 * the header comes back in n_msgs, long_runs and chunk.
 * rd_debug_burst_decode_repair: the same with max_flips (0 .. 2, else RD_ERR_ARG before any device work);
 * rd_debug_burst_decode is it with max_flips = 0.
 * rd_debug_burst_decode_narrow: the same with `narrow` (0 or 1, else RD_ERR_ARG; 1 with symbol_length < 4: RD_ERR_ARG), all
 * before any device work; with narrow = 0 it hands back rd_debug_burst_decode_repair's bytes. */
int rd_debug_bursts(const uint8_t *chan, size_t stride, int n_ch, size_t n_out, const uint32_t *thr, uint64_t seq,
                    rd_burst *recs_out, rd_burst_floor *floor_out);
int rd_debug_burst_decode(const rd_config *cfg, const uint8_t *cur, const uint8_t *prev, size_t stride, int n_ch,
                          uint64_t clock, uint64_t seq, const rd_burst *runs, const uint32_t *n_runs,
                          rd_burst_msg *msgs_out, uint32_t *n_msgs, uint32_t *long_runs, uint32_t *chunk);
int rd_debug_burst_decode_repair(const rd_config *cfg, const uint8_t *cur, const uint8_t *prev, size_t stride, int n_ch,
                                 uint64_t clock, uint64_t seq, const rd_burst *runs, const uint32_t *n_runs, int max_flips,
                                 rd_burst_msg *msgs_out, uint32_t *n_msgs, uint32_t *long_runs, uint32_t *chunk);
int rd_debug_burst_decode_narrow(const rd_config *cfg, const uint8_t *cur, const uint8_t *prev, size_t stride, int n_ch,
                                 uint64_t clock, uint64_t seq, const rd_burst *runs, const uint32_t *n_runs, int max_flips,
                                 int narrow, rd_burst_msg *msgs_out, uint32_t *n_msgs, uint32_t *long_runs, uint32_t *chunk);
/* rd_debug_burst_expect (tests/test_burst_track.py): k_chan_burst_expect alone, the same pattern - cur / prev as above, the
 * table e[n_e] checked by the rule of rd_wb_set_burst_expect (RD_ERR_ARG before any device work; n_e >= 1), max_flips and
 * narrow as above.  msgs_out: RD_BX_MAX record places, hdr_out: RD_BX_MAX headers of four uint32 { n_msgs, candidates,
 * chunk, pad }; both slots are filled with 0xA5 and copied out whole, so places of idle expectations and everything past
 * n_e come back as 0xA5 - and so does every header when no expectation has a candidate, for then nothing is launched. */
int rd_debug_burst_expect(const rd_config *cfg, const uint8_t *cur, const uint8_t *prev, size_t stride, int n_ch,
                          uint64_t clock, uint64_t seq, const rd_expect *e, int n_e, int max_flips, int narrow,
                          rd_burst_msg *msgs_out, uint32_t *hdr_out);
/* rd_debug_burst_search (tests/test_burst_search.py): k_chan_burst_search alone, the same pattern - cur / prev as above,
 * the centres checked by the rule of rd_wb_set_burst_search (RD_ERR_ARG before any device work; n >= 1; symbol_length >= 4;
 * n_ch at most 4096).  msgs_out: RD_BS_MAX_CENTRES x n_ch x RD_BS_PER record places, hdr_out: RD_BS_MAX_CENTRES x n_ch
 * headers, the receiver's slot: filled with 0xA5 and copied out whole, so the places past a header's n_msgs and
 * everything of a centre index >= n come back as 0xA5. */
int rd_debug_burst_search(const rd_config *cfg, const uint8_t *cur, const uint8_t *prev, size_t stride, int n_ch,
                          uint64_t clock, uint64_t seq, const uint8_t *centres, int n, rd_burst_msg *msgs_out,
                          rd_bs_header *hdr_out);
/* rd_debug_burst_quality (tests/test_burst_quality.py): k_chan_burst_quality alone, the same pattern - cur / prev as
 * above; msgs[n_ch][cap] (cap = ceil(nW / 2)) and n_msgs_per_channel[n_ch] are written into a decode slot as they are,
 * records no decoder would write included, with chunk = RD_BQ_DEBUG_CHUNK in every header.  out: n_ch x cap + RD_BX_MAX
 * quality records, the receiver's slot [n_ch][cap] | [RD_BX_MAX]: filled with 0xA5, written by ONE launch over the decode
 * part and copied out whole - the places past a channel's n_msgs and the whole expect part come back as 0xA5.
 * RD_ERR_ARG before any device work for noise_gap outside 0 .. 1024, an n_msgs above cap, or a configuration
 * rd_wb_set_burst_decode refuses. */
#define RD_BQ_DEBUG_CHUNK 0x51A7u
int rd_debug_burst_quality(const rd_config *cfg, const uint8_t *cur, const uint8_t *prev, size_t stride, int n_ch,
                           int noise_gap, const rd_burst_msg *msgs, const uint32_t *n_msgs_per_channel, rd_burst_quality *out);
/* rd_debug_burst_clips (tests/test_burst_clips.py): k_chan_burst_clips alone, the same pattern - cur / prev as above;
 * runs[n_ch][cap] and n_runs[n_ch] go into a burst slot as they are, msgs[n_ch][cap] and n_msgs[n_ch] into a decode slot
 * (msgs and n_msgs may be NULL without RD_BC_MESSAGES); x_msgs[RD_BX_MAX] with x_hdr[RD_BX_MAX][4] and n_expect (1 .. RD_BX_MAX), or
 * NULLs and 0: the expect kernel was not launched; s_msgs[RD_BS_MAX_CENTRES][n_ch][RD_BS_PER] with
 * s_hdr[RD_BS_MAX_CENTRES][n_ch] and n_search (1 .. RD_BS_MAX_CENTRES), or NULLs and 0; owed_prev[n_ch]: `owed` of the
 * previous chunk's headers, or NULL when no chunk before had clips on.  out: the receiver's slot of rd_bc_slot_size(n_ch,
 * quota) bytes - [n_ch][RD_BC_PER] rd_burst_clip | [n_ch] six uint32 { n_clips, dropped, owed, used, chunk, pad } | padding
 * to a multiple of 16 | [n_ch][2 quota] bytes - filled with 0xA5, written by one launch and copied out whole.  RD_ERR_ARG
 * before any device work for settings rd_wb_set_burst_clips refuses, sources = 0, a block_size that is no multiple of 128,
 * and with RD_BC_MESSAGES a configuration rd_wb_set_burst_decode refuses. */
size_t rd_bc_slot_size(int n_ch, int quota);
int rd_debug_burst_clips(const rd_config *cfg, const uint8_t *cur, const uint8_t *prev, size_t stride, int n_ch, uint64_t clock,
                         uint64_t seq, const rd_burst *runs, const uint32_t *n_runs, const rd_burst_msg *msgs,
                         const uint32_t *n_msgs, const rd_burst_msg *x_msgs, const uint32_t *x_hdr, int n_expect,
                         const rd_burst_msg *s_msgs, const rd_bs_header *s_hdr, int n_search, const uint32_t *owed_prev,
                         int sources, int pre, int post, int quota, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif /* RTLDAVIS_HIP_H */
