// rd_hiphost.h - what the host side of every HIP translation unit of the library shares (definitions: rd_api.hip): the
// error slot behind rd_last_error, the one check of a HIP call, the lazy fork-aware device context and the polling waits.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rtldavis_hip.h"

// sets the calling thread's rd_last_error text (printf-style) and returns `code`
int rd_fail_msg(int code, const char *fmt, ...);

#define HIPCHK(expr)                                                                                                          \
    do {                                                                                                                      \
        hipError_t e_ = (expr);                                                                                               \
        if (e_ != hipSuccess)                                                                                                 \
            return rd_fail_msg(RD_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);    \
    } while (0)

// Lazy HIP initialisation; RD_OK or RD_ERR_DEVICE.  HIP state does not survive fork(): a child of a process that already
// used the device must not reuse it.  Handles created before fork hold no device state.
int rd_ensure_device(void);
// A handle is tied to the device that was current when its buffers were allocated; every entry point makes that device
// current for the calling thread first (handles may be used from several threads).  device < 0: nothing to do.
int rd_use_device(int device);
// this process is the one whose device state the library's handles hold: only then does a destroy function free any
bool rd_owns_device_state(void);

// Wait for an event / a stream by polling, with the deadline of every host wait (rd_host.h: rd_waiter): RD_ERR_DEVICE
// "timed out after ... waiting for <what>" when it passes.
int rd_wait_event(hipEvent_t ev, const char *what);
int rd_wait_stream(hipStream_t st, const char *what);
// device -> host copy of n bytes on `st`, completed on return (polling wait)
int rd_copy_d2h(void *dst, const void *src, size_t n, hipStream_t st);

// Host push (rd_api.hip): the register whose write flushes the host data path of device `dev` behind the host's stores
// into its memory, or null when the host may not write blocks there (no large BAR, no register, RD_PUSH_INPUT=0)
volatile uint32_t *rd_push_flush_reg(int dev);
