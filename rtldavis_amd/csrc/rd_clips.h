// rd_clips.h - the handle of CLIP DECODE and CLIP SYNTH (include/rtldavis_hip.h), shared by rd_clip_decode.hip, which
// creates and destroys it, uploads a pool and decodes jobs on it, and rd_clip_synth.hip, which fills the pool on the
// device and copies it back.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rd_hiphost.h"

struct rd_clips {
    rd_config cfg;
    uint8_t *d_pool = nullptr;           // the pool, padded to whole 16-byte vectors
    size_t pool_cap = 0;                 // bytes allocated
    uint64_t pool_outputs = 0;           // 0: nothing uploaded or synthesised yet
    rd_clip_job *d_jobs = nullptr;
    rd_burst_msg *d_recs = nullptr;
    rd_cd_header *d_hdr = nullptr;
    int64_t *d_soft = nullptr;
    int cap_jobs = 0, cap_soft = 0;      // jobs the buffers hold
    uint32_t *d_nb = nullptr;            // the narrow-band table, from the first narrow decode on
    rd_clip_spec *d_specs = nullptr;     // (synth) the specs of the last synthesis
    int cap_specs = 0;
    int16_t *d_cs_tab = nullptr;         // (synth) the cosine table, from the first synthesis on
    hipStream_t st = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t sv0 = nullptr, sv1 = nullptr;   // (synth) around the zeroing and the kernel, from the first synthesis on
    bool busy = false;                   // a wait gave up: the stream may still hold work on the buffers
    float kernel_ms = -1.0f;
    float synth_ms = -1.0f;
};

// the device, the handle's stream and events; waits first for what a timed-out call left behind (rd_clip_decode.hip)
int rd_cd_prepare(rd_clips *h);
// the library's polling wait on the handle's stream, under the deadline; a wait that gave up leaves the handle busy
int rd_cd_wait(rd_clips *h, const char *what);
// make the device pool hold `nbytes` bytes, padded to whole vectors (grown, never shrunk); pool_outputs is 0 afterwards
// until the caller has filled it.  *need: the padded size.
int rd_cd_size_pool(rd_clips *h, size_t nbytes, size_t *need);
