// rd_api.hip - what every handle of librtldavis_hip.so stands on (rd_hiphost.h; the C ABI: include/rtldavis_hip.h):
// the error slot, the device context, the host waits and the host-push probe.  The handles themselves: rd_batch.hip
// (batch demodulator), rd_stream.hip (streaming demodulator), rd_stages.hip (stage functions on host arrays).
//
// Host-side orchestration only.  All arithmetic of the path runs in the kernel files (rd_device.h names them); there is no CPU
// fallback - without a usable HIP device every compute entry point returns RD_ERR_DEVICE.
#include <unistd.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>

#include "rd_hiphost.h"
#include "rd_host.h"

// ------------------------------------------------------------------------------------------
// errors / device context
// ------------------------------------------------------------------------------------------
static thread_local std::string g_err;

int rd_fail_msg(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" const char *rd_last_error(void) { return g_err.c_str(); }

static pid_t g_hip_pid = 0;  // pid that first touched the device through this library

int rd_ensure_device(void) {
    const pid_t me = getpid();
    if (g_hip_pid != 0 && g_hip_pid != me)
        return rd_fail_msg(RD_ERR_DEVICE, "HIP was initialised in parent process %d before fork(); "
                                          "create the device state in the child instead", (int)g_hip_pid);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return rd_fail_msg(RD_ERR_DEVICE, "no HIP device available (%s); librtldavis_hip has no CPU fallback",
                           e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    g_hip_pid = me;
    return RD_OK;
}

bool rd_owns_device_state(void) { return g_hip_pid == getpid(); }

int rd_use_device(int device) {
    if (device >= 0) HIPCHK(hipSetDevice(device));
    return RD_OK;
}

extern "C" int rd_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

extern "C" int rd_set_device(int device) {
    int rc = rd_ensure_device();
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    return RD_OK;
}

// Wait for an event / a stream by polling.  The runtime's blocking waits (hipStreamSynchronize, synchronous
// hipMemcpy) were measured to add 10-20 ms of wake-up latency per call on this platform, an order of magnitude more
// than a whole batch takes on the GPU.  Every wait has a deadline (rd_host.h: rd_waiter; RD_WAIT_TIMEOUT_MS, default
// 10 s): a kernel that never completes must surface as RD_ERR_DEVICE so that the caller's "log, drop the block, go on"
// (/root/reference/src/rtldavis/worker.py:56-58) can fire, not pin a core for ever.
int rd_wait_event(hipEvent_t ev, const char *what) {
    rd_waiter w(rd_wait_timeout_ms());
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return RD_OK;
        if (e != hipErrorNotReady) return rd_fail_msg(RD_ERR_DEVICE, "hipEventQuery: %s", hipGetErrorString(e));
        if (!w.relax()) return rd_fail_msg(RD_ERR_DEVICE, "timed out after %.0f ms waiting for %s", w.waited_ms(), what);
    }
}

int rd_wait_stream(hipStream_t st, const char *what) {
    rd_waiter w(rd_wait_timeout_ms());
    for (;;) {
        const hipError_t e = hipStreamQuery(st);
        if (e == hipSuccess) return RD_OK;
        if (e != hipErrorNotReady) return rd_fail_msg(RD_ERR_DEVICE, "hipStreamQuery: %s", hipGetErrorString(e));
        if (!w.relax()) return rd_fail_msg(RD_ERR_DEVICE, "timed out after %.0f ms waiting for %s", w.waited_ms(), what);
    }
}

extern "C" int rd_set_wait_timeout_ms(int ms) { return (int)rd_wait_timeout_set((double)ms); }

int rd_copy_d2h(void *dst, const void *src, size_t n, hipStream_t st) {
    if (n == 0) return RD_OK;
    HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, st));
    return rd_wait_stream(st, "a device-to-host copy");
}

// ------------------------------------------------------------------------------------------
// Host push (streaming handle).  A kernel's own reads of pinned host memory run at ~13 GB/s however many CUs ask
// (profiles/r04_stream_stamps.txt: a complex128 block's 128 KB = 10 of the kernel's 15 us), the host's stores into device
// memory through the PCIe BAR at ~45 GB/s (tools/ubench/bar_write.hip: 128 KB in 2.9 us).  Where the whole of device memory
// is host-visible (hipDeviceAttributeIsLargeBar) rd_demod_submit therefore copies the block straight into an UNCACHED
// device buffer (no stale line in an XCD's L2 when the slot is written again), makes the stores leave the CPU's
// write-combining buffers (sfence), flushes the GPU's host data path (HDP: the register ROCr publishes for exactly this,
// HSA_AMD_AGENT_INFO_HDP_FLUSH) and launches; PCIe keeps posted writes in order, so the block is in HBM before the launch's
// doorbell arrives.  Without a large BAR, without the register, or with RD_PUSH_INPUT=0: the pinned slot, as before.
// ------------------------------------------------------------------------------------------
#define RD_MAX_DEVICES 64
struct rd_push_info {
    int state = 0;                        // 0 not probed, 1 available, -1 not available
    volatile uint32_t *hdp_flush = nullptr;
};
static rd_push_info g_push[RD_MAX_DEVICES];

struct rd_hdp_find { uint32_t bdf, domain; volatile uint32_t *reg; bool found; };
static hsa_status_t rd_hdp_cb(hsa_agent_t agent, void *data) {
    rd_hdp_find *f = (rd_hdp_find *)data;
    hsa_device_type_t t;
    if (hsa_agent_get_info(agent, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS || t != HSA_DEVICE_TYPE_GPU) return HSA_STATUS_SUCCESS;
    uint32_t bdf = 0, dom = 0;
    if (hsa_agent_get_info(agent, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
    if (hsa_agent_get_info(agent, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &dom) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
    if (bdf != f->bdf || dom != f->domain) return HSA_STATUS_SUCCESS;
    hsa_amd_hdp_flush_t h = {nullptr, nullptr};
    if (hsa_agent_get_info(agent, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_HDP_FLUSH, &h) == HSA_STATUS_SUCCESS) f->reg = h.HDP_MEM_FLUSH_CNTL;
    f->found = true;
    return HSA_STATUS_INFO_BREAK;
}

// true when the host may write blocks straight into device memory of `dev` (and knows how to flush the HDP behind them)
static int g_push_mode = -1;   // rd_set_input_push: 0 = never
static bool push_available(int dev) {
    if (dev < 0 || dev >= RD_MAX_DEVICES || g_push_mode == 0) return false;
    static std::mutex mu;   // (handles may be created from several threads)
    std::lock_guard<std::mutex> lock(mu);
    rd_push_info &p = g_push[dev];
    if (p.state) return p.state > 0;
    p.state = -1;
    const char *e = getenv("RD_PUSH_INPUT");
    if (e && atoi(e) == 0) return false;
    int large = 0;
    if (hipDeviceGetAttribute(&large, hipDeviceAttributeIsLargeBar, dev) != hipSuccess || !large) return false;
    char id[64] = {0};
    unsigned dom = 0, bus = 0, d = 0, fn = 0;
    if (hipDeviceGetPCIBusId(id, sizeof id, dev) != hipSuccess || sscanf(id, "%x:%x:%x.%x", &dom, &bus, &d, &fn) != 4) return false;
    if (hsa_init() != HSA_STATUS_SUCCESS) return false;   // (a reference on the runtime HIP already runs on; kept)
    rd_hdp_find f = {(bus << 8) | (d << 3) | fn, dom, nullptr, false};
    hsa_iterate_agents(rd_hdp_cb, &f);
    if (!f.found || !f.reg) return false;
    p.hdp_flush = f.reg;
    p.state = 1;
    return true;
}

volatile uint32_t *rd_push_flush_reg(int dev) { return push_available(dev) ? g_push[dev].hdp_flush : nullptr; }

extern "C" int rd_set_input_push(int mode) {
    int rc = rd_ensure_device();
    if (rc) return rc;
    g_push_mode = mode == 0 ? 0 : -1;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return rd_fail_msg(RD_ERR_DEVICE, "hipGetDevice failed");
    return push_available(dev) ? 1 : 0;
}
