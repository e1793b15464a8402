// Time warp along the last axis of rows x n fp32 data through a windowed-sinc interpolator, and its adjoint: a speed change, sinusoidal
// wow / flutter and a cut at the front as a step of the graph.  The definition is the comment of wm_time_warp in include/wm_hip.h; this
// file is how it is computed.
//
// Launch.  One lane owns one sample of the result -- an output y[t] of the forward map, an input position k of the adjoint -- and runs its
// whole fmaf chain, so there is one writer per sample, no atomics, no scratch, and the bits know nothing of the grid.  A workgroup of 256
// lanes takes tiles of 256 consecutive samples of one row, grid-stride, and keeps the table (Z R + 2 words, 32 KiB at 16 x 512) in LDS
// for all of them: as many workgroups a CU as the table leaves room for, each loading it once.  Neighbouring lanes read neighbouring
// stretches of the row (lane l + 1 starts a samples after lane l), so a wave's load of one tap touches a few consecutive cache lines; the
// row is read through the caches, not staged, because nothing bounds the stretch a tile of garbage parameters would ask for.
// Table reads: tab[i] and tab[i + 1] per tap, i = floor(c |p - k| R).  At c = 1 a lane's taps sit R words apart, all on one bank, and the
// lanes of a wave differ in the fractional part of p alone: one address at speed 1 (a broadcast), 64 scattered ones at any other speed.
// No layout of the table removes that scatter -- the fraction is data -- so none is tried.
//
// Safety.  Every index into the row is clamped to [0, n) in fp64 before it becomes an integer and every loop has a fixed cap (260 taps
// forward, 4096 terms and 35 bisection steps in the adjoint), whatever the parameters hold; the predicate v < Z keeps the table index
// below Z R, and it is clamped all the same.
#include "wm_common.hpp"
using namespace wm;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxTerms = 4096;                 // terms of one adjoint sample
constexpr int kMaxTaps = 2 * 129 + 2;           // candidate taps of one forward sample: c >= 1/4, Z <= 32, one sample of margin each side
constexpr size_t kMaxTableBytes = 128 * 1024;
constexpr size_t kLdsPerCU = 160 * 1024;

struct Args {
    const float* x; const float* params; const float* tab; float* y;
    long long rows, n, tpr, tiles;              // tpr tiles per row
    int Z, R, adjoint;
};

struct Row {
    double a, off, d, w, phi, c, h;             // h = Z / c + 1: the half support and one sample of margin
    float c32;
    bool ok;                                    // a > 0 and everything finite: the rows the adjoint is defined for
};

__device__ __forceinline__ Row load_row(const float* __restrict__ q, int Z) {
    Row r;
    r.a = q[0]; r.off = q[1]; r.d = q[2]; r.w = q[3]; r.phi = q[4];
    const float c = q[5];
    r.c32 = c != c ? 1.f : fminf(fmaxf(c, 0.25f), 1.f);
    r.c = r.c32;
    r.h = (double)Z / r.c + 1.0;
    const double big = 1.7e308;
    r.ok = r.a > 0.0 && r.a < big && fabs(r.off) < big && fabs(r.d) < big && fabs(r.w) < big && fabs(r.phi) < big;
    return r;
}

// t arrives as a double (exact below 2^53): the tap loops step it by 1.0 instead of converting a 64-bit integer per term
__device__ __forceinline__ double position(const Row& r, double td) {
#pragma clang fp contract(off)
    double p = fma(r.a, td, r.off);
    if (r.d != 0.0) {
        const double q = fma(r.w, td, r.phi);
        const double s = sinpi(2.0 * (q - floor(q)));
        const double ds = r.d * s;
        p = p + ds;
    }
    return p;
}

// the weight of u = p - k; outside the support: false and W = 0, without a branch, so that the loops around it can run their loads ahead
__device__ __forceinline__ bool weight(const Row& r, double u, int Z, int R, const float* tab, float& W) {
#pragma clang fp contract(off)
    const double v = r.c * fabs(u);
    const bool in = v < (double)Z;              // NaN fails
    const double s = in ? v * (double)R : 0.0;
    int i = (int)s;                             // 0 <= s < Z R: the floor
    i = i < 0 ? 0 : (i > Z * R - 1 ? Z * R - 1 : i);
    const float f = (float)(s - (double)i);
    const float t0 = tab[i];
    const float dt = tab[i + 1] - t0;
    W = in ? r.c32 * fmaf(f, dt, t0) : 0.f;
    return in;
}

__global__ __launch_bounds__(kThreads) void time_warp_kernel(Args a) {
    extern __shared__ __align__(16) float tab[];
    const int tid = threadIdx.x, Z = a.Z, R = a.R;
    for (int i = tid; i < Z * R + 2; i += kThreads) tab[i] = a.tab[i];
    __syncthreads();
    const long long n = a.n;
    for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long r = tile / a.tpr;
        const long long idx = (tile - r * a.tpr) * kThreads + tid;
        if (idx >= n) continue;
        const Row row = load_row(a.params + 6 * r, Z);
        const float* __restrict__ xr = a.x + r * n;
        float acc = 0.f;
        if (!a.adjoint) {
            const double p = position(row, (double)idx);
            if (fabs(p) < 1e18) {                                                 // NaN and infinities: no tap
                const double lo = fmax(ceil(p - row.h), 0.0), hi = fmin(floor(p + row.h), (double)(n - 1));
                if (lo <= hi) {
                    const double span = hi - lo;                                  // an integer, at most 2 h + 1
                    const int cnt = span < (double)kMaxTaps ? (int)span + 1 : kMaxTaps;
                    const float* __restrict__ xp = xr + (long long)lo;            // xp[0 .. cnt) lies inside the row
                    double kd = lo;
                    // a tap outside the support enters as fmaf(0, 0, acc) = acc (acc is never -0): the chain's bits are those of
                    // the taps inside alone, and x there is neither used nor able to spoil the sum
                    for (int j = 0; j < cnt; ++j, kd += 1.0) {
                        float W;
                        const bool in = weight(row, p - kd, Z, R, tab, W);
                        const float xv = xp[j];
                        acc = fmaf(W, in ? xv : 0.f, acc);
                    }
                }
            }
        } else if (row.ok) {
            const double kd = (double)idx, m = row.h + fabs(row.d);
            // p(t) lies within |d| of a t + off: outside this bracket no t can reach the support
            const double tA = fmax(floor((kd - m - row.off) / row.a) - 1.0, 0.0);
            const double tB = fmin(ceil((kd + m - row.off) / row.a) + 1.0, (double)(n - 1));
            if (tA <= tB) {
                long long lo = (long long)tA, hi = (long long)tB + 1;
                const long long last = hi - 1;
                while (lo < hi) {                                                 // the first t with p(t) - k >= -h, p increasing
                    const long long mid = lo + ((hi - lo) >> 1);
                    if (position(row, (double)mid) - kd < -row.h) lo = mid + 1; else hi = mid;
                }
                const long long left = last - lo + 1;                             // <= 0: nothing
                const int cnt = left < kMaxTerms ? (int)left : kMaxTerms;
                const float* __restrict__ xp = xr + lo;                           // xp[0 .. cnt) lies inside the row
                double td = (double)lo;
                for (int j = 0; j < cnt; ++j, td += 1.0) {
                    const double u = position(row, td) - kd;
                    if (u > row.h) break;
                    float W;
                    const bool in = weight(row, u, Z, R, tab, W);
                    const float xv = xp[j];
                    acc = fmaf(W, in ? xv : 0.f, acc);
                }
            }
        }
        a.y[r * n + idx] = acc;
    }
}

}  // namespace

extern "C" {

int wm_time_warp(const float* x, const float* params, const float* tab, float* y, long long rows, long long n, int zeros, int res,
                 int adjoint, hipStream_t stream) {
    if (rows < 1 || n < 1 || n > (1ll << 34) || rows > (1ll << 46) / n) return (int)hipErrorInvalidValue;
    if (zeros < 4 || zeros > 32 || res < 64 || res > 1024 || (res & (res - 1))) return (int)hipErrorInvalidValue;
    const size_t lds = ((size_t)zeros * res + 2) * sizeof(float);
    if (lds > kMaxTableBytes) return (int)hipErrorInvalidValue;
    if (!x || !params || !tab || !y || (uintptr_t)x % 4 || (uintptr_t)params % 4 || (uintptr_t)tab % 4 || (uintptr_t)y % 4)
        return (int)hipErrorInvalidValue;
    const unsigned long long bytes = (unsigned long long)rows * (unsigned long long)n * 4;
    if (overlap(x, bytes, y, bytes) || overlap(params, (unsigned long long)rows * 24, y, bytes) || overlap(tab, lds, y, bytes))
        return (int)hipErrorInvalidValue;                                         // in place is refused
    static DevOnce done;
    if (lds > 64 * 1024 && !dev_done(done)) {
        WM_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(time_warp_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)kMaxTableBytes));
        dev_mark(done);
    }
    Args a;
    a.x = x; a.params = params; a.tab = tab; a.y = y; a.rows = rows; a.n = n;
    a.tpr = (n + kThreads - 1) / kThreads;
    a.tiles = rows * a.tpr;
    a.Z = zeros; a.R = res; a.adjoint = adjoint != 0;
    long long per_cu = (long long)(kLdsPerCU / lds);                              // workgroups a CU holds: each loads the table once
    if (per_cu > 8) per_cu = 8;
    const long long cap = kNumCU * per_cu;
    hipLaunchKernelGGL(time_warp_kernel, dim3((unsigned)(a.tiles < cap ? a.tiles : cap)), dim3(kThreads), lds, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
