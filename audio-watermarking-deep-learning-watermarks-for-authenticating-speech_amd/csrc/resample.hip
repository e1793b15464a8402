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
//
// wm_resample_add is the way back of the embed path: delta (model rate) -> the recording's rate, added to every channel of the recording,
//   up[m*Q + i] = the sum above with xmono = delta (0 outside [0, Nd));   out[c][o] = x[c][o] + up[o],
// with the same two kernels around the same tap loops (filter_tile / filter_sample below), so `up` is wm_resample's result bit for bit.
// Its tile kernel leaves the results in LDS and walks the rows of x / out (and up) through them: each is read / written once, coalesced.
//
// wm_resample_rows is the filter alone on a batch: x (rows, N) -> y (rows, L), every row by itself (no mixdown, no padding, any L), again the
// same two kernels around the same tap loops, tiles numbered per row from period 0 of that row.  With the transposed table of
// ops.resample_adjoint_table the same launch on (dy, rows, L -> N) is the resampler's adjoint: one tap loop, two tables.
#include <type_traits>
#include "wm_common.hpp"
using namespace wm;

namespace {

constexpr int kThreads = 256;
constexpr int kR = 4;                       // periods a thread computes per tap read
constexpr int kTileFloats = 8192;           // input + output floats of one tile (32 KB); half of it beside a table of more than 8 KB
constexpr int kMaxTableBytes = 40 * 1024;   // 44.1 k -> 16 k: 160 phases x (35 taps + first) = 23 KB; 11.025 k -> 16 k: 640 x 14 = 35 KB
constexpr int kMaxLdsBytes = 64 * 1024;     // stays below the opt-in limit: no function attribute, no state
constexpr int kMaxChannels = 1 << 16;       // wm_resample_add: channels x floats of a tile stays a 32-bit count

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

// ---- the pieces both launches are made of (wm_resample, wm_resample_add): table -> LDS, input window -> LDS, the tap loop

// LDS image of a tile, in this order (M % 4 == 0, so ys is made of 16-byte rows)
struct Tile {
    float* ys;                              // [M*Q]   results of the tile
    float* xs;                              // [win]   xs[j] = input[m0*P - width + j], win = M*P + 2*width
    float* hs;                              // [Q*W]
    int* fs;                                // [Q]
};

__device__ __forceinline__ Tile tile_of(float* smem, int M, int P, int Q, int width, int W) {
    Tile t;
    t.ys = smem;
    t.xs = t.ys + M * Q;
    t.hs = t.xs + M * P + 2 * width;
    t.fs = (int*)(t.hs + Q * W);
    return t;
}

__device__ __forceinline__ void load_table(const Tile& t, const float* __restrict__ taps, const int* __restrict__ first, int P, int Q,
                                           int width, int W, int tid) {
    for (int i = tid; i < Q * W; i += kThreads) t.hs[i] = taps[i];
    for (int i = tid; i < Q; i += kThreads) t.fs[i] = min(max(first[i], 0), 2 * width + P - W);   // keeps every LDS read inside xs
}

// input window of the tile that starts at sample n0, channel mean on the way in, zero outside [0, N) BY PREDICATE (what lies there is
// never read); quads on absolute multiples of 4 so that every row is 16-byte aligned
__device__ __forceinline__ void stage_window(float* xs, const float* __restrict__ x, int C, long long N, long long n0, int win, int xvec,
                                             double inv_c, int tid) {
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
}

// THE tap loop of the tile kernels: kR periods of one phase per work item, ys[m*Q + i] = sum_k hs[i][k] * xs[m*P + fs[i] + k]
__device__ __forceinline__ void filter_tile(const Tile& t, int M, int P, int Q, int W, int tid) {
    const int G = M / kR, items = G * Q, step = G * P;
    for (int w = tid; w < items; w += kThreads) {
        const int g = w / Q, u = w - g * Q;
        const float* hp = t.hs + u * W;
        const float* xp = t.xs + g * P + t.fs[u];
        float acc[kR];
#pragma unroll
        for (int r = 0; r < kR; ++r) acc[r] = 0.f;
        for (int k = 0; k < W; ++k) {
            const float h = hp[k];
#pragma unroll
            for (int r = 0; r < kR; ++r) acc[r] = fmaf(h, xp[r * step + k], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < kR; ++r) t.ys[(g + r * G) * Q + u] = acc[r];
    }
}

// THE tap loop of the one-thread-per-sample kernels: output sample o, the input read through `in(n)` (which answers 0 outside the signal)
template <class In>
__device__ __forceinline__ float filter_sample(const float* __restrict__ taps, const int* __restrict__ first, long long o, int P, int Q,
                                               int width, int W, In in) {
    const long long m = o / Q;
    const int i = (int)(o - m * Q);
    const long long nb = m * P + min(max(first[i], 0), 2 * width + P - W) - width;
    const float* hp = taps + (long long)i * W;
    float acc = 0.f;
    for (int k = 0; k < W; ++k) acc = fmaf(hp[k], in(nb + k), acc);
    return acc;
}

// ---- wm_resample

__global__ __launch_bounds__(kThreads) void resample_tile_kernel(const float* __restrict__ x, const float* __restrict__ taps,
                                                                 const int* __restrict__ first, float* __restrict__ y, int C, long long N,
                                                                 int P, int Q, int width, int W, long long L, long long total, int M,
                                                                 long long tiles, int xvec, int yvec, double inv_c) {
    extern __shared__ __align__(16) float smem[];
    const Tile t = tile_of(smem, M, P, Q, width, W);
    const float* ys = t.ys;
    const int win = M * P + 2 * width;
    const int tid = threadIdx.x;
    load_table(t, taps, first, P, Q, width, W, tid);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long m0 = tile * M;
        __syncthreads();                    // the previous tile's ys / xs are no longer read (first pass: nothing pending)
        stage_window(t.xs, x, C, N, m0 * P - width, win, xvec, inv_c, tid);
        __syncthreads();
        filter_tile(t, M, P, Q, W, tid);
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
        if (o < L)
            acc = filter_sample(taps, first, o, P, Q, width, W,
                                [&](long long n) { return (n >= 0 && n < N) ? mono_at(x, C, N, n, inv_c) : 0.f; });
        y[o] = acc;
    }
}

// ---- wm_resample_rows: x (rows, N) -> y (rows, L), every row alone.  A tile is (row, tile in that row) and starts at period m0 = tile-in-row * M
// of ITS row, so a sample sits where wm_resample of that row alone would put it; the last tile of a row stages and filters only the periods
// the row still has (rounded up to kR).  Outside [0, N) of its own row a window reads zero by predicate: a neighbour's samples are never read.

__global__ __launch_bounds__(kThreads) void resample_rows_tile_kernel(const float* __restrict__ x, const float* __restrict__ taps,
                                                                      const int* __restrict__ first, float* __restrict__ y, long long N,
                                                                      int P, int Q, int width, int W, long long L, int M,
                                                                      long long row_tiles, long long tiles, int xvec, int yvec) {
    extern __shared__ __align__(16) float smem[];
    const Tile t = tile_of(smem, M, P, Q, width, W);
    const float* ys = t.ys;
    const int tid = threadIdx.x;
    const long long periods = (L + Q - 1) / Q;
    load_table(t, taps, first, P, Q, width, W, tid);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long row = tile / row_tiles;
        const long long m0 = (tile - row * row_tiles) * M;
        const long long left = periods - m0;                            // > 0: row_tiles = ceil(periods / M)
        const int Mt = left < M ? (int)((left + kR - 1) / kR) * kR : M;  // periods of this tile, a multiple of kR, <= M
        const float* xr = x + row * N;
        float* yr = y + row * L;
        __syncthreads();                    // the previous tile's ys / xs are no longer read (first pass: nothing pending)
        stage_window(t.xs, xr, 1, N, m0 * P - width, Mt * P + 2 * width, xvec, 1.0, tid);
        __syncthreads();
        filter_tile(t, Mt, P, Q, W, tid);
        __syncthreads();
        const long long o0 = m0 * Q;        // a multiple of 4
        for (int q = tid; q < (Mt * Q) / 4; q += kThreads) {
            const long long o = o0 + 4ll * q;
            if (o >= L) break;
            const f32x4 s = *reinterpret_cast<const f32x4*>(ys + 4 * q);
            if (yvec && o + 4 <= L) {
                *reinterpret_cast<f32x4*>(yr + o) = s;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (o + e < L) yr[o + e] = s[e];
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void resample_rows_cache_kernel(const float* __restrict__ x, const float* __restrict__ taps,
                                                                       const int* __restrict__ first, float* __restrict__ y, long long N,
                                                                       int P, int Q, int width, int W, long long L, long long total) {
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kThreads) {
        const long long row = e / L;
        const float* xr = x + row * N;
        y[e] = filter_sample(taps, first, e - row * L, P, Q, width, W, [&](long long n) { return (n >= 0 && n < N) ? xr[n] : 0.f; });
    }
}

// ---- wm_resample_add: the way back.  up = delta resampled to the recording's rate, out[c] = x[c] + up for every channel.
// x and out carry no __restrict__: out may be x itself.  Every thread reads the elements of x it is going to write before it writes them and
// no other thread touches them, which is all that in-place operation needs.

constexpr int kRowsInFlight = 4;            // loads of x a thread issues before it adds and stores: the store phase is pure HBM latency

// rows of one tile: out[c][o0 + e] = x[c][o0 + e] + ys[e], e < count, all channels, V floats (V = 4: 16-byte rows) per access.  The C * count / V
// accesses of the tile are dealt round-robin to the threads whatever C is, so a small tile of many channels keeps as many loads in flight
// as a large one of one channel.
template <int V>
__device__ __forceinline__ void add_rows(const float* x, float* out, float* up, const float* ys, int C, long long N, long long o0, int count,
                                         int tid) {
    using vec = typename std::conditional<V == 4, f32x4, float>::type;
    const unsigned per = (unsigned)(count / V);
    unsigned q = (unsigned)tid, c = 0;
    if (q >= per) { c = q / per; q -= c * per; }
    while (c < (unsigned)C) {
        vec v[kRowsInFlight];
        long long at[kRowsInFlight];
        unsigned qs[kRowsInFlight];
#pragma unroll
        for (int j = 0; j < kRowsInFlight; ++j) {
            at[j] = -1;
            if (c < (unsigned)C) {
                at[j] = (long long)c * N + o0 + (long long)V * q;
                qs[j] = q;
                v[j] = *reinterpret_cast<const vec*>(x + at[j]);
                q += kThreads;
                if (q >= per) { const unsigned dc = q / per; c += dc; q -= dc * per; }
            }
        }
#pragma unroll
        for (int j = 0; j < kRowsInFlight; ++j)
            if (at[j] >= 0) *reinterpret_cast<vec*>(out + at[j]) = v[j] + *reinterpret_cast<const vec*>(ys + V * qs[j]);
    }
    if (up)
        for (unsigned e = (unsigned)tid; e < per; e += kThreads)
            *reinterpret_cast<vec*>(up + o0 + (long long)V * e) = *reinterpret_cast<const vec*>(ys + V * e);
}

__global__ __launch_bounds__(kThreads) void resample_add_tile_kernel(const float* __restrict__ d, const float* __restrict__ taps,
                                                                     const int* __restrict__ first, const float* x, float* out, float* up,
                                                                     int C, long long N, long long Nd, int P, int Q, int width, int W, int M,
                                                                     long long tiles, int dvec, int rowvec) {
    extern __shared__ __align__(16) float smem[];
    const Tile t = tile_of(smem, M, P, Q, width, W);
    const int win = M * P + 2 * width;
    const int tid = threadIdx.x;
    load_table(t, taps, first, P, Q, width, W, tid);
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long m0 = tile * M;
        __syncthreads();                    // the previous tile's ys / xs are no longer read (first pass: nothing pending)
        stage_window(t.xs, d, 1, Nd, m0 * P - width, win, dvec, 1.0, tid);
        __syncthreads();
        filter_tile(t, M, P, Q, W, tid);
        __syncthreads();
        const long long o0 = m0 * Q;        // a multiple of 4; o0 < N because tiles = ceil(ceil(N / Q) / M)
        const long long left = N - o0;
        const int count = (int)(left < (long long)M * Q ? left : (long long)M * Q);
        if (rowvec) add_rows<4>(x, out, up, t.ys, C, N, o0, count, tid);     // N % 4 == 0: count is a multiple of 4 too
        else add_rows<1>(x, out, up, t.ys, C, N, o0, count, tid);
    }
}

__global__ __launch_bounds__(kThreads) void resample_add_cache_kernel(const float* __restrict__ d, const float* __restrict__ taps,
                                                                      const int* __restrict__ first, const float* x, float* out, float* up,
                                                                      int C, long long N, long long Nd, int P, int Q, int width, int W) {
    for (long long o = (long long)blockIdx.x * kThreads + threadIdx.x; o < N; o += (long long)gridDim.x * kThreads) {
        const float u = filter_sample(taps, first, o, P, Q, width, W, [&](long long n) { return (n >= 0 && n < Nd) ? d[n] : 0.f; });
        for (int c = 0; c < C; ++c) out[(long long)c * N + o] = x[(long long)c * N + o] + u;
        if (up) up[o] = u;
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

// x (rows, N) -> y (rows, L), both contiguous: y[r][m*Q + i] = sum_k taps[i][k] * x[r][m*P + first[i] + k - width], x[r][.] = 0 outside [0, N).
// L is any number of outputs per row.  taps [Q][W], first [Q] (int32).
int wm_resample_rows(const float* x, const float* taps, const int* first, float* y, long long rows, long long N, long long L, int P, int Q,
                     int width, int W, hipStream_t stream) {
    if (rows < 0 || N < 0 || L < 0 || P <= 0 || Q <= 0 || width < 0 || W <= 0 || W > 2 * width + P) return (int)hipErrorInvalidValue;
    if ((long long)P + Q > (1ll << 30) || (long long)Q * W > (1ll << 30)) return (int)hipErrorInvalidValue;
    if (rows > (1ll << 40) || N > (1ll << 40) || L > (1ll << 40) || (N > 0 && rows > (1ll << 60) / N) || (L > 0 && rows > (1ll << 60) / L))
        return (int)hipErrorInvalidValue;    // rows * N and rows * L (and the tile count) stay 64-bit counts
    if (rows == 0 || L == 0) return 0;
    if ((!x && N > 0) || !taps || !first || !y) return (int)hipErrorInvalidValue;
    const Plan p = make_plan(P, Q, width, W);
    if (p.M == 0) {
        const long long total = rows * L;
        const long long blocks = (total + kThreads - 1) / kThreads;
        const int grid = (int)(blocks < (1ll << 20) ? blocks : (1ll << 20));
        hipLaunchKernelGGL(resample_rows_cache_kernel, dim3(grid), dim3(kThreads), 0, stream, x, taps, first, y, N, P, Q, width, W, L, total);
        WM_CHECK_LAUNCH();
        return 0;
    }
    const long long periods = (L + Q - 1) / Q;
    const long long row_tiles = (periods + p.M - 1) / p.M;
    const long long tiles = rows * row_tiles;
    const long long cap = 8ll * kNumCU;
    const int grid = (int)(tiles < cap ? tiles : cap);
    // row r starts at x + r*N / y + r*L: on the 16-byte grid for every row only when the base is and the row length is a multiple of 4
    const int xvec = ((uintptr_t)x % 16 == 0) && (rows == 1 || N % 4 == 0);
    const int yvec = ((uintptr_t)y % 16 == 0) && (rows == 1 || L % 4 == 0);
    hipLaunchKernelGGL(resample_rows_tile_kernel, dim3(grid), dim3(kThreads), (size_t)p.lds, stream, x, taps, first, y, N, P, Q, width, W, L,
                       p.M, row_tiles, tiles, xvec, yvec);
    WM_CHECK_LAUNCH();
    return 0;
}

// d: delta at the rate P (flat, the first Nd samples count; what lies behind them is never read) -> up (N,) at the rate Q, may be NULL;
// out (C, N) = x (C, N) + up on every channel, out may be x.  taps [Q][W], first [Q]: the table of the pair (delta rate, recording rate).
int wm_resample_add(const float* d, const float* taps, const int* first, const float* x, float* out, float* up, int C, long long N,
                    long long Nd, int P, int Q, int width, int W, hipStream_t stream) {
    if (C <= 0 || C > kMaxChannels || N < 0 || Nd < 0 || P <= 0 || Q <= 0 || width < 0 || W <= 0 || W > 2 * width + P)
        return (int)hipErrorInvalidValue;
    if ((long long)P + Q > (1ll << 30) || (long long)Q * W > (1ll << 30)) return (int)hipErrorInvalidValue;
    if (N == 0) return 0;
    if ((!d && Nd > 0) || !taps || !first || !x || !out) return (int)hipErrorInvalidValue;
    const Plan p = make_plan(P, Q, width, W);
    if (p.M == 0) {
        const long long blocks = (N + kThreads - 1) / kThreads;
        const int grid = (int)(blocks < (1ll << 20) ? blocks : (1ll << 20));
        hipLaunchKernelGGL(resample_add_cache_kernel, dim3(grid), dim3(kThreads), 0, stream, d, taps, first, x, out, up, C, N, Nd, P, Q,
                           width, W);
        WM_CHECK_LAUNCH();
        return 0;
    }
    const long long periods = (N + Q - 1) / Q;
    const long long tiles = (periods + p.M - 1) / p.M;
    const long long cap = 8ll * kNumCU;
    const int grid = (int)(tiles < cap ? tiles : cap);
    const int dvec = ((uintptr_t)d % 16 == 0);
    const int rowvec = N % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)up % 16 == 0;
    hipLaunchKernelGGL(resample_add_tile_kernel, dim3(grid), dim3(kThreads), (size_t)p.lds, stream, d, taps, first, x, out, up, C, N, Nd, P,
                       Q, width, W, p.M, tiles, dvec, rowvec);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
