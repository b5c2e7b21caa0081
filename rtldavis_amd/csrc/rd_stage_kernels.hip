// rd_stage_kernels.hip - float64 kernels behind rd_stages.hip and the state mirrors:
//   k_disc / k_filt : float64 discriminate / fir9 values of a stream or of the complex ring (py:133-134)
//   stage kernels   : one float64 kernel per reference stage function
// py = the reference's src/rtldavis/dsp.py
#include "rd_device.h"

// ------------------------------------------------------------------------------------------
// float64 values of d and f (state mirrors / parse()'s frequency error, protocol.py:307-311)
// ------------------------------------------------------------------------------------------
template <class View>
__global__ __launch_bounds__(256) void k_disc(View v, long t0, long n, double *out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long t = t0 + i;
    out[i] = rd_disc_f64(rd_f_f64(v, t - 1), rd_f_f64(v, t));
}

template <class View>
__global__ __launch_bounds__(256) void k_filt(View v, long t0, long n, double *out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const rd_d2 f = rd_f_f64(v, t0 + i);
    out[2 * i] = f.x;
    out[2 * i + 1] = f.y;
}

void rd_launch_disc(const rd_layout &lay, int stream, long t0, long n, double *out, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_disc<rd_stream_view>, rd_grid256(n), dim3(256), 0, st,
                       rd_view_of(lay, stream), t0, n, out);
}

void rd_launch_filtered(const rd_layout &lay, int stream, long t0, long n, double *out, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_filt<rd_stream_view>, rd_grid256(n), dim3(256), 0, st,
                       rd_view_of(lay, stream), t0, n, out);
}

void rd_launch_cplx_disc(const rd_cplx_layout &lay, long t0, long n, double *out, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_disc<rd_cplx_view>, rd_grid256(n), dim3(256), 0, st, rd_cplx_view_of(lay), t0, n, out);
}

void rd_launch_cplx_filtered(const rd_cplx_layout &lay, long t0, long n, double *out, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_filt<rd_cplx_view>, rd_grid256(n), dim3(256), 0, st, rd_cplx_view_of(lay), t0, n, out);
}

// ------------------------------------------------------------------------------------------
// stage kernels: one per reference stage function, float64, on device arrays
// ------------------------------------------------------------------------------------------
__global__ void k_lut(const uint8_t *in, double *out, size_t n) {  // py:38-39
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[2 * i] = ((double)in[2 * i] - 127.4) / 127.6;
    out[2 * i + 1] = ((double)in[2 * i + 1] - 127.4) / 127.6;
}
void rd_launch_lut(const uint8_t *in, double *out, size_t n, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_lut, rd_grid256(n), dim3(256), 0, st, in, out, n);
}

__global__ void k_rotate(const double *in, double *out, size_t n) {  // py:46-49
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const rd_d2 y = rd_rot_f64(in[2 * i], in[2 * i + 1], (long)i);
    out[2 * i] = y.x;
    out[2 * i + 1] = y.y;
}
void rd_launch_rotate(const double *in, double *out, size_t n, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_rotate, rd_grid256(n), dim3(256), 0, st, in, out, n);
}

__global__ void k_fir9(const double *in, double *out, size_t n_out) {  // py:71-73
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out) return;
    const double c[9] = RD_TAPS9;
    double ar = 0.0, ai = 0.0;
#pragma unroll
    for (int m = 0; m < 9; m++) {
        ar += c[m] * in[2 * (i + m)];
        ai += c[m] * in[2 * (i + m) + 1];
    }
    out[2 * i] = ar;
    out[2 * i + 1] = ai;
}
void rd_launch_fir9(const double *in, double *out, size_t n_out, hipStream_t st) {
    if (n_out) hipLaunchKernelGGL(k_fir9, rd_grid256(n_out), dim3(256), 0, st, in, out, n_out);
}

__global__ void k_discriminate(const double *in, double *out, size_t n_out) {  // py:80-90
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out) return;
    const rd_d2 n = {in[2 * i], in[2 * i + 1]}, np = {in[2 * i + 2], in[2 * i + 3]};
    out[i] = rd_disc_f64(n, np);
}
void rd_launch_discriminate(const double *in, double *out, size_t n_out, hipStream_t st) {
    if (n_out)
        hipLaunchKernelGGL(k_discriminate, rd_grid256(n_out), dim3(256), 0, st, in, out, n_out);
}

__global__ void k_quantize(const double *in, uint8_t *out, size_t n) {  // py:98
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (uint8_t)rd_signbit_f64(in[i]);
}
void rd_launch_quantize(const double *in, uint8_t *out, size_t n, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_quantize, rd_grid256(n), dim3(256), 0, st, in, out, n);
}

__global__ void k_pack_bytes(const uint8_t *in01, uint32_t *words, size_t n) {  // go:105-113 Pack
    const size_t wi = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (wi * 32 >= n) return;
    uint32_t w = 0;
    for (int b = 0; b < 32 && wi * 32 + b < n; b++) w |= (uint32_t)(in01[wi * 32 + b] & 1u) << b;
    words[wi] = w;
}
void rd_launch_pack_bytes(const uint8_t *in01, uint32_t *words, size_t n, hipStream_t st) {
    const size_t nw = (n + 31) / 32;
    if (nw) hipLaunchKernelGGL(k_pack_bytes, rd_grid256(nw), dim3(256), 0, st, in01, words, n);
}
