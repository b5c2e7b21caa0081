// rd_stages.hip - the stage functions of the C ABI on host arrays (include/rtldavis_hip.h: rd_lut_execute .. rd_search):
// one stage of the path at a time, for tests and for callers that want a single step.  Each uploads its input, launches
// the stage's float64 kernel (rd_stage_kernels.hip) on the null stream and downloads the result.
#include <algorithm>
#include <vector>

#include "rd_internal.h"

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
};

// upload `in`, launch(device input, device output), download `out`
template <class Launch> static int stage_run(const void *in, size_t in_bytes, void *out, size_t out_bytes, Launch launch) {
    int rc = rd_ensure_device();
    if (rc) return rc;
    DevBuf a, b;
    HIPCHK(hipMalloc(&a.p, in_bytes));
    HIPCHK(hipMalloc(&b.p, out_bytes));
    HIPCHK(hipMemcpy(a.p, in, in_bytes, hipMemcpyHostToDevice));
    launch(a.p, b.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, b.p, out_bytes, hipMemcpyDeviceToHost));
    return RD_OK;
}

extern "C" int rd_lut_execute(const uint8_t *in_bytes, size_t n_bytes, double *out_cplx, size_t n_cplx) {
    if (n_bytes != 2 * n_cplx) return rd_fail_msg(RD_ERR_ARG, "Incompatible array sizes: in_bytes.size=%zu, out_cplx.size=%zu", n_bytes, n_cplx);
    if (n_cplx == 0) return RD_OK;
    if (!in_bytes || !out_cplx) return rd_fail_msg(RD_ERR_ARG, "null argument");
    return stage_run(in_bytes, n_bytes, out_cplx, n_cplx * 16,
                     [=](const void *a, void *b) { rd_launch_lut((const uint8_t *)a, (double *)b, n_cplx, nullptr); });
}

extern "C" int rd_rotate_fs4(const double *in_cplx, double *out_cplx, size_t n_cplx) {
    if (n_cplx == 0) return RD_OK;
    if (!in_cplx || !out_cplx) return rd_fail_msg(RD_ERR_ARG, "null argument");
    return stage_run(in_cplx, n_cplx * 16, out_cplx, n_cplx * 16,
                     [=](const void *a, void *b) { rd_launch_rotate((const double *)a, (double *)b, n_cplx, nullptr); });
}

extern "C" int rd_fir9(const double *in_cplx, size_t n_in, double *out_cplx, size_t n_out) {
    if (n_in < 9 || n_out > n_in - 8) return rd_fail_msg(RD_ERR_ARG, "fir9: n_out must be <= n_in - 8");
    if (n_out == 0) return RD_OK;
    if (!in_cplx || !out_cplx) return rd_fail_msg(RD_ERR_ARG, "null argument");
    return stage_run(in_cplx, n_in * 16, out_cplx, n_out * 16,
                     [=](const void *a, void *b) { rd_launch_fir9((const double *)a, (double *)b, n_out, nullptr); });
}

extern "C" int rd_discriminate(const double *in_cplx, size_t n_in, double *out, size_t n_out) {
    if (n_in < 1 || n_out != n_in - 1) return rd_fail_msg(RD_ERR_ARG, "discriminate: n_out must be n_in - 1");
    if (n_out == 0) return RD_OK;
    if (!in_cplx || !out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    return stage_run(in_cplx, n_in * 16, out, n_out * 8,
                     [=](const void *a, void *b) { rd_launch_discriminate((const double *)a, (double *)b, n_out, nullptr); });
}

extern "C" int rd_quantize(const double *in, uint8_t *out, size_t n) {
    if (n == 0) return RD_OK;
    if (!in || !out) return rd_fail_msg(RD_ERR_ARG, "null argument");
    return stage_run(in, n * 8, out, n, [=](const void *a, void *b) { rd_launch_quantize((const double *)a, (uint8_t *)b, n, nullptr); });
}

extern "C" int rd_search(const rd_config *cfg, const uint8_t *quantized, size_t n, int32_t *indices, int cap,
                         int *count) {
    if (!count) return rd_fail_msg(RD_ERR_ARG, "null count");
    if (!cfg) return rd_fail_msg(RD_ERR_ARG, "null config");
    rd_devcfg dc;
    rd_config c2 = *cfg;
    if (c2.block_size < 32) c2.block_size = 32;  // block size is irrelevant to a bare search
    c2.block_size -= c2.block_size % 4;
    int rc = rd_devcfg_checked(&c2, &dc);
    if (rc) return rc;
    *count = 0;
    const long span = (long)(dc.P - 1) * dc.S;
    if ((long)n <= span) return RD_OK;
    if (!quantized) return rd_fail_msg(RD_ERR_ARG, "null argument");
    rc = rd_ensure_device();
    if (rc) return rc;
    DevBuf a, w, m, cnt;
    const uint32_t mcap = (uint32_t)n;
    HIPCHK(hipMalloc(&a.p, n));
    HIPCHK(hipMalloc(&w.p, ((n + 31) / 32) * 4));
    HIPCHK(hipMalloc(&m.p, (size_t)mcap * sizeof(rd_match)));
    HIPCHK(hipMalloc(&cnt.p, RD_CNT_TOTAL * 4));
    HIPCHK(hipMemset(cnt.p, 0, RD_CNT_TOTAL * 4));
    HIPCHK(hipMemcpy(a.p, quantized, n, hipMemcpyHostToDevice));
    rd_launch_pack_bytes((const uint8_t *)a.p, (uint32_t *)w.p, n, nullptr);
    rd_launch_search((const uint32_t *)w.p, 0, 1, (long)n, 0, (long)n - 1 - span, dc, (rd_match *)m.p, mcap,
                     (uint32_t *)cnt.p, nullptr);
    HIPCHK(hipGetLastError());
    uint32_t h_cnt[RD_CNT_SLOTS];
    HIPCHK(hipMemcpy(h_cnt, cnt.p, sizeof h_cnt, hipMemcpyDeviceToHost));
    const uint32_t nm = std::min(h_cnt[RD_CNT_MATCH], mcap);
    std::vector<rd_match> ms(nm);
    if (nm) HIPCHK(hipMemcpy(ms.data(), m.p, (size_t)nm * sizeof(rd_match), hipMemcpyDeviceToHost));
    const int S = dc.S;
    std::sort(ms.begin(), ms.end(), [S](const rd_match &x, const rd_match &y) {
        const int px = x.pos % S, py = y.pos % S;
        return px != py ? px < py : x.pos < y.pos;
    });
    *count = (int)nm;
    if ((int)nm > cap) return rd_fail_msg(RD_ERR_CAPACITY, "need room for %u indices", nm);
    for (uint32_t i = 0; i < nm; i++) indices[i] = ms[i].pos;
    return RD_OK;
}
