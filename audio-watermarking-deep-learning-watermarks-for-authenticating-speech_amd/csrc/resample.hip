// Polyphase sinc resampler of the file ingest: channel mean -> band-limited interpolation P -> Q -> zero-padded 1-s segments,
// one launch (the reference mixes down, runs torchaudio.transforms.Resample(sr, 16000) and pads the tail before it calls a model).
//
//   y[m*Q + i] = sum_{k < W} taps[i][k] * xmono[m*P + first[i] + k - width]        (xmono = 0 outside [0, N))
//
// taps / first are the COMPACT table ops.py builds in float64: the Hann-windowed sinc is exactly zero outside +-6 zero crossings, so of the
// K = 2*width + P taps of a phase only a run of W <= 2*width + 2 can be non-zero; first[i] is where that run starts.  The sum runs k = 0..W-1 with
// one fmaf per tap into one accumulator in BOTH kernels below, so a sample's value depends on its phase and its inputs only, never on the
// tile, the workgroup or the path that produced it.
//
// Tile kernel (table and tile fit LDS): a workgroup owns M whole output periods at a time.  It stages the M*P + 2*width input samples they read
// once (channel mean applied on the way in, 16-byte loads where the rows allow), keeps the table in LDS for all its tiles, and a thread
// computes kR periods of ONE phase together: a tap is read once for kR FMAs, and the kR periods lie M/kR apart so that neighbouring lanes
// read LDS P floats apart (odd P: no bank conflict; ops.py makes W odd for the same reason).  Results go through LDS to be written as
// 16-byte rows, the zeros of the padded tail included.
// Cache kernel (16001 -> 16000 has 16000 phases): one thread per output sample, table and input read through the cache.  Same sums.
#include "wm_common.hpp"
using namespace wm;

namespace {

constexpr int kThreads = 256;
constexpr int kR = 4;                       // periods a thread computes per tap read
constexpr int kTileFloats = 8192;           // input + output floats of one tile (32 KB); half of it beside a table of more than 8 KB
constexpr int kMaxTableBytes = 40 * 1024;   // 44.1 k -> 16 k: 160 phases x (35 taps + first) = 23 KB; 11.025 k -> 16 k: 640 x 14 = 35 KB
constexpr int kMaxLdsBytes = 64 * 1024;     // stays below the opt-in limit: no function attribute, no state

struct Plan { int M; int lds; };            // M == 0: cache kernel

Plan make_plan(int P, int Q, int width, int W) {
    const long long table = (long long)Q * (W + 1) * 4;
    if (table > kMaxTableBytes) return {0, 0};
    // a large table already takes the LDS of a workgroup or two: smaller tiles keep four workgroups on a CU to overlap each other's
    // load, filter and store phases (44.1 k -> 16 k, one hour of stereo: 0.75 ms with 12-period tiles, 0.54 ms with 4-period tiles)
    long long M = (table > 8 * 1024 ? kTileFloats / 2 : kTileFloats) / ((long long)P + Q);
    M -= M % kR;
    if (M < kR) M = kR;
    const long long lds = (M * Q + M * P + 2ll * width) * 4 + table;
    if (lds > kMaxLdsBytes) return {0, 0};
    return {(int)M, (int)lds};
}

// channel mean with ONE float32 rounding: the channels are added in float64 (exact to 2^-53, also where they cancel), so the error of the
// mean is one float32 ulp of the mean itself and not of the largest partial sum -- what the error bound of the filter assumes
__device__ __forceinline__ float mono_at(const float* __restrict__ x, int C, long long N, long long n, double inv_c) {
    if (C == 1) return x[n];
    double v = (double)x[n];
    for (int c = 1; c < C; ++c) v += (double)x[(long long)c * N + n];
    return (float)(v * inv_c);
}

__global__ __launch_bounds__(kThreads) void resample_tile_kernel(const float* __restrict__ x, const float* __restrict__ taps,
                                                                 const int* __restrict__ first, float* __restrict__ y, int C, long long N,
                                                                 int P, int Q, int width, int W, long long L, long long total, int M,
                                                                 long long tiles, int xvec, int yvec, double inv_c) {
    extern __shared__ __align__(16) float smem[];
    const int win = M * P + 2 * width;
    float* ys = smem;                       // [M*Q]   (M % 4 == 0: 16-byte rows)
    float* xs = ys + M * Q;                 // [win]   xs[j] = xmono[m0*P - width + j]
    float* hs = xs + win;                   // [Q*W]
    int* fs = (int*)(hs + Q * W);           // [Q]
    const int tid = threadIdx.x;
    for (int i = tid; i < Q * W; i += kThreads) hs[i] = taps[i];
    for (int i = tid; i < Q; i += kThreads) fs[i] = min(max(first[i], 0), 2 * width + P - W);   // keeps every LDS read inside xs
    const int G = M / kR, items = G * Q, step = G * P;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long m0 = tile * M, n0 = m0 * P - width;
        __syncthreads();                    // the previous tile's ys / xs are no longer read (first pass: nothing pending)
        // ---- input window, channel mean on the way in; quads on absolute multiples of 4 so that every row is 16-byte aligned
        const long long a0 = n0 & ~3ll;
        const int quads = (int)((n0 + win - a0 + 3) >> 2);
        for (int q = tid; q < quads; q += kThreads) {
            const long long n = a0 + 4ll * q;
            float v[4];
            if (xvec && n >= 0 && n + 4 <= N) {
                const f32x4 s0 = *reinterpret_cast<const f32x4*>(x + n);
                if (C == 1) {
                    v[0] = s0[0]; v[1] = s0[1]; v[2] = s0[2]; v[3] = s0[3];
                } else {
                    double d[4] = {(double)s0[0], (double)s0[1], (double)s0[2], (double)s0[3]};
                    for (int c = 1; c < C; ++c) {
                        const f32x4 sc = *reinterpret_cast<const f32x4*>(x + (long long)c * N + n);
#pragma unroll
                        for (int e = 0; e < 4; ++e) d[e] += (double)sc[e];
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (float)(d[e] * inv_c);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (n + e >= 0 && n + e < N) ? mono_at(x, C, N, n + e, inv_c) : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long long j = n + e - n0;
                if (j >= 0 && j < win) xs[j] = v[e];
            }
        }
        __syncthreads();
        // ---- kR periods of one phase per work item
        for (int w = tid; w < items; w += kThreads) {
            const int g = w / Q, u = w - g * Q;
            const float* hp = hs + u * W;
            const float* xp = xs + g * P + fs[u];
            float acc[kR];
#pragma unroll
            for (int r = 0; r < kR; ++r) acc[r] = 0.f;
            for (int k = 0; k < W; ++k) {
                const float h = hp[k];
#pragma unroll
                for (int r = 0; r < kR; ++r) acc[r] = fmaf(h, xp[r * step + k], acc[r]);
            }
#pragma unroll
            for (int r = 0; r < kR; ++r) ys[(g + r * G) * Q + u] = acc[r];
        }
        __syncthreads();
        // ---- coalesced rows out; samples behind L are the zero padding of the last segment
        const long long o0 = m0 * Q;        // a multiple of 4
        for (int q = tid; q < (M * Q) / 4; q += kThreads) {
            const long long o = o0 + 4ll * q;
            if (o >= total) break;
            f32x4 s = *reinterpret_cast<const f32x4*>(ys + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) if (o + e >= L) s[e] = 0.f;
            if (yvec && o + 4 <= total) {
                *reinterpret_cast<f32x4*>(y + o) = s;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (o + e < total) y[o + e] = s[e];
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void resample_cache_kernel(const float* __restrict__ x, const float* __restrict__ taps,
                                                                  const int* __restrict__ first, float* __restrict__ y, int C, long long N,
                                                                  int P, int Q, int width, int W, long long L, long long total, double inv_c) {
    for (long long o = (long long)blockIdx.x * kThreads + threadIdx.x; o < total; o += (long long)gridDim.x * kThreads) {
        float acc = 0.f;
        if (o < L) {
            const long long m = o / Q;
            const int i = (int)(o - m * Q);
            const long long nb = m * P + min(max(first[i], 0), 2 * width + P - W) - width;
            const float* hp = taps + (long long)i * W;
            for (int k = 0; k < W; ++k) {
                const long long n = nb + k;
                const float xv = (n >= 0 && n < N) ? mono_at(x, C, N, n, inv_c) : 0.f;
                acc = fmaf(hp[k], xv, acc);
            }
        }
        y[o] = acc;
    }
}

}  // namespace

extern "C" {

// host-only query: output periods per tile of the LDS kernel for this rate pair, 0 when the cache kernel runs
int wm_resample_plan(int P, int Q, int width, int W, long long* tile_periods, hipStream_t) {
    if (P <= 0 || Q <= 0 || width < 0 || W <= 0 || W > 2 * width + P || !tile_periods) return (int)hipErrorInvalidValue;
    *tile_periods = make_plan(P, Q, width, W).M;
    return 0;
}

// x (C, N) channel-major -> y[0 .. total): the L resampled samples of the channel mean, then zeros.  taps [Q][W], first [Q] (int32).
int wm_resample(const float* x, const float* taps, const int* first, float* y, int C, long long N, int P, int Q, int width, int W,
                long long L, long long total, hipStream_t stream) {
    if (C <= 0 || N < 0 || P <= 0 || Q <= 0 || width < 0 || W <= 0 || W > 2 * width + P || L < 0 || total < L)
        return (int)hipErrorInvalidValue;
    if ((long long)P + Q > (1ll << 30) || (long long)Q * W > (1ll << 30)) return (int)hipErrorInvalidValue;
    if (total == 0) return 0;
    if (!x || !taps || !first || !y) return (int)hipErrorInvalidValue;
    const Plan p = make_plan(P, Q, width, W);
    if (p.M == 0) {
        const long long blocks = (total + kThreads - 1) / kThreads;
        const int grid = (int)(blocks < (1ll << 20) ? blocks : (1ll << 20));
        hipLaunchKernelGGL(resample_cache_kernel, dim3(grid), dim3(kThreads), 0, stream, x, taps, first, y, C, N, P, Q, width, W, L, total,
                           1.0 / (double)C);
        WM_CHECK_LAUNCH();
        return 0;
    }
    const long long periods = (total + Q - 1) / Q;
    const long long tiles = (periods + p.M - 1) / p.M;
    const long long cap = 8ll * kNumCU;
    const int grid = (int)(tiles < cap ? tiles : cap);
    const int xvec = ((uintptr_t)x % 16 == 0) && (C == 1 || N % 4 == 0);
    const int yvec = ((uintptr_t)y % 16 == 0);
    hipLaunchKernelGGL(resample_tile_kernel, dim3(grid), dim3(kThreads), (size_t)p.lds, stream, x, taps, first, y, C, N, P, Q, width, W, L,
                       total, p.M, tiles, xvec, yvec, 1.0 / (double)C);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
