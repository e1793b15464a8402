// The main14b_2 variant's backward kernels that are no GEMM: ELU backward, the bias gradient of the transposed convolutions (channel
// sum), row sums and the dense embedding gradient.  One launch each (the channel sum: two); they share nothing with gconv_fwd.hip
// or gconv_wgrad.hip.
#include "wm_common.hpp"
using namespace wm;

namespace {

// dz = g * elu'(y) with y = ELU(z):  elu'(z) = 1 for y > 0 else y + 1   (alpha = 1)
__global__ void elu_bwd_kernel(const float* __restrict__ g, const float* __restrict__ y, float* __restrict__ dz, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float yy = y[i];
    dz[i] = g[i] * (yy > 0.f ? 1.f : yy + 1.f);
}

// partial[c][y] = sum over clips nb == y (mod gridDim.y) and all t of x[nb][c][t]; channel_sum_final adds the partials of a
// channel in fixed order (bias gradient of the transposed convolutions; no atomics: bit-reproducible)
__global__ __launch_bounds__(256) void channel_sum_kernel(const float* __restrict__ x, float* __restrict__ partial, int NB, int C, int L) {
    __shared__ float scratch[4];
    const int c = blockIdx.x;
    float s = 0.f;
    for (int nb = blockIdx.y; nb < NB; nb += gridDim.y) {
        const float* r = x + ((size_t)nb * C + c) * L;
        for (int t = threadIdx.x; t < L; t += 256) s += r[t];
    }
    s = block_sum<4>(s, scratch);
    if (threadIdx.x == 0) partial[(size_t)c * gridDim.y + blockIdx.y] = s;
}
__global__ void channel_sum_final_kernel(const float* __restrict__ partial, float* __restrict__ out, int C, int ny, int accumulate) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int y = 0; y < ny; ++y) s += (double)partial[(size_t)c * ny + y];
    out[c] = (float)((accumulate ? (double)out[c] : 0.0) + s);
}

// out[row] = sum_t x[row][t] for any row length
__global__ __launch_bounds__(256) void rowsum_any_kernel(const float* __restrict__ x, float* __restrict__ out, int L) {
    __shared__ float scratch[4];
    const float* r = x + (size_t)blockIdx.x * L;
    float s = 0.f;
    for (int t = threadIdx.x; t < L; t += 256) s += r[t];
    s = block_sum<4>(s, scratch);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// dtable[idx[b]][:] += dvec[b][:]   (dense embedding gradient for any embedding width).  One thread per column walks the
// batch in order, so duplicate ids add in a fixed order (bit-reproducible; B is ~128, the cost is nil)
__global__ void rows_scatter_add_kernel(float* __restrict__ dtable, const long long* __restrict__ idx,
                                        const float* __restrict__ dvec, int Bn, int dim, int nrows) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= dim) return;
    for (int b = 0; b < Bn; ++b) {
        const long long m = idx[b];
        if (m < 0 || m >= nrows) continue;
        dtable[(size_t)m * dim + d] += dvec[(size_t)b * dim + d];
    }
}

}  // namespace

extern "C" {

int wm_elu_bwd(const float* g, const float* y, float* dz, long long n, hipStream_t stream) {
    hipLaunchKernelGGL(elu_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, g, y, dz, (size_t)n);
    WM_CHECK_LAUNCH();
    return 0;
}

// out[c] (+)= sum_{nb,t} x[nb][c][t]; partial: >= 64*C floats of scratch.  Fixed summation order (no atomics).
int wm_channel_sum(const float* x, float* out, float* partial, int NB, int C, int L, int accumulate, hipStream_t stream) {
    if (NB <= 0 || C <= 0 || L <= 0 || !partial) return (int)hipErrorInvalidValue;
    const int ny = NB < 64 ? NB : 64;
    hipLaunchKernelGGL(channel_sum_kernel, dim3(C, ny), dim3(256), 0, stream, x, partial, NB, C, L);
    WM_CHECK_LAUNCH();
    hipLaunchKernelGGL(channel_sum_final_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, partial, out, C, ny, accumulate);
    WM_CHECK_LAUNCH();
    return 0;
}

int wm_rowsum_any(const float* x, float* out, int rows, int L, hipStream_t stream) {
    hipLaunchKernelGGL(rowsum_any_kernel, dim3(rows), dim3(256), 0, stream, x, out, L);
    WM_CHECK_LAUNCH();
    return 0;
}

int wm_rows_scatter_add(float* dtable, const long long* idx, const float* dvec, int Bn, int dim, int nrows, hipStream_t stream) {
    hipLaunchKernelGGL(rows_scatter_add_kernel, dim3((dim + 255) / 256), dim3(256), 0, stream, dtable, idx, dvec, Bn, dim, nrows);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
