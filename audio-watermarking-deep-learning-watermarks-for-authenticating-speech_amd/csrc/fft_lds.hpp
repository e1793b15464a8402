// The complex FFT in LDS that the spectral kernels share (stft_loss.hip, clip_features.hip, masking.hip): radix-2, decimation in
// frequency, by 256 threads, the result left in bit-reversed order.  The fp64 overload is masking.hip's forward: a transform's rounding
// is absolute, about 2^-22 of the LARGEST bin, and a geometric mean over the bins (the tonality measure) sees the small ones.
#pragma once
#include "wm_common.hpp"

namespace wm {

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// z [2^LOGN] in LDS, tw[k] = e^(-2 pi i k / 2^LOGN) for k < 2^(LOGN-1), tid in [0, 256).  Every thread of the workgroup calls it (one
// barrier per stage); z must be published before the call and is published on return.
template <int LOGN>
__device__ __forceinline__ void fft_dif(float2* z, const float2* tw, int tid) {
    constexpr int N = 1 << LOGN;
#pragma unroll 1
    for (int st = 0; st < LOGN; ++st) {
        const int lm = LOGN - 1 - st, m = 1 << lm;           // half size of this stage's butterflies
        for (int j = tid; j < N / 2; j += 256) {
            const int pos = j & (m - 1), i0 = ((j >> lm) << (lm + 1)) + pos, i1 = i0 + m;
            const float2 a = z[i0], b = z[i1], w = tw[pos << st];
            z[i0] = make_float2(a.x + b.x, a.y + b.y);
            z[i1] = cmul(make_float2(a.x - b.x, a.y - b.y), w);
        }
        __syncthreads();
    }
}
__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
template <int LOGN>
__device__ __forceinline__ void fft_dif(double2* z, const double2* tw, int tid) {
    constexpr int N = 1 << LOGN;
#pragma unroll 1
    for (int st = 0; st < LOGN; ++st) {
        const int lm = LOGN - 1 - st, m = 1 << lm;
        for (int j = tid; j < N / 2; j += 256) {
            const int pos = j & (m - 1), i0 = ((j >> lm) << (lm + 1)) + pos, i1 = i0 + m;
            const double2 a = z[i0], b = z[i1], w = tw[pos << st];
            z[i0] = make_double2(a.x + b.x, a.y + b.y);
            z[i1] = cmul(make_double2(a.x - b.x, a.y - b.y), w);
        }
        __syncthreads();
    }
}
template <int LOGN>
__device__ __forceinline__ int brev(int k) { return (int)(__brev((unsigned)k) >> (32 - LOGN)); }

}  // namespace wm
