// Second-order IIR section along the last axis of rows x n fp32 data, with the 16-bit PCM codec of the save path as its epilogue:
// the 7 kHz biquad low-pass -> clamp -> x32767 -> int16 of py/main15.py:850-867, and main15c's perceptual_postprocess
// (round(lowpass_biquad(x) * 32767) / 32767).  Every row starts from a zero state:
//
//   y[u] = b0 x[u] + b1 x[u-1] + b2 x[u-2] - a1 y[u-1] - a2 y[u-2]        u = t, or u = n-1-t with `reverse` (index mirroring, no flipped copy)
//
// ONE chain of roundings per sample, in both kernels (biquad_step below): a product and four fmaf, the y[u-1] term last so that the
// recursion's critical path is one fmaf.
//
// Chunk kernel (warm >= 0).  A recursion cannot be split exactly, but a stable section forgets: its state decays like r^k (r the pole
// radius), so a recursion started `warm` samples early from a zero state agrees with the true one to r^warm (the host picks warm with
// r^warm <= 2^-40, far below an fp32 ulp of anything the row holds).  The row is cut, in u, into chunks of kChunk = 32 samples at multiples
// of 32; a lane owns one chunk, runs warm + 32 steps and keeps the last 32.  Samples before the row are zeros, so a chunk that starts within
// `warm` of the row start is exact.  Which chunk a sample belongs to, and therefore its bits, depends on (u, warm) only -- never on the
// tile, the grid or the workgroup.
// A workgroup takes a tile of 256 chunks of one row: it stages the 8192 + warm samples they read into LDS with coalesced 16-byte loads
// (quads on absolute 16-byte boundaries, so any 4-byte aligned pointer and any n use them; ends and mirrored rows element-wise),
// lane i walks logical positions i*32 - warm .. i*32 + 31 with LDS index j + j/32 (lanes 33 words apart: no bank conflict), keeps its 32
// results in registers until every lane has read its warm-up, writes them back over the inputs, and the tile leaves through the epilogue
// as 16-byte (fp32) or 8-byte (int16) rows.  No atomics: every output element and every mask word has one writer.
// Row kernel (warm = -1): where the warm-up would be longer than kMaxWarm the exact recursion runs instead, one lane per row, through the
// same staging and epilogue (2048-sample tiles, the state carried in registers from tile to tile).
#include <type_traits>
#include "wm_common.hpp"
using namespace wm;

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 32;                      // samples a lane owns = the samples of one mask word
constexpr int kTile = kThreads * kChunk;        // 8192 samples of one row
constexpr int kMaxWarm = 1024;                  // beyond it a lane would run > 33 steps per sample it keeps: the row kernel takes over
constexpr int kRowThreads = 64;
constexpr int kRowTile = 2048;

struct Coef { float b0, b1, b2, a1, a2; };

__device__ __forceinline__ int pad(int j) { return j + (j >> 5); }
constexpr int padded(int j) { return j + (j >> 5) + 1; }

__device__ __forceinline__ float biquad_step(const Coef& c, float x0, float x1, float x2, float y1, float y2) {
    float acc = c.b0 * x0;
    acc = fmaf(c.b1, x1, acc);
    acc = fmaf(c.b2, x2, acc);
    acc = fmaf(-c.a2, y2, acc);
    return fmaf(-c.a1, y1, acc);
}

// xs[pad(u - ub)] = x[row][t(u)] (times its bit of mask_in) for u in [us, ue), then zeros up to the end of the chunk that holds ue - 1.
// t(u) = u, or n-1-u when mirrored.  xo: (address of x / 4) % 4, so that `a` below counts floats from a 16-byte boundary.
__device__ __forceinline__ void stage(float* xs, const float* __restrict__ x, const unsigned* __restrict__ mask_in, long long row,
                                      long long n, long long nw, long long ub, long long us, long long ue, int reverse, int xo, int tid,
                                      int nthreads) {
    const long long tl = reverse ? n - ue : us, th = reverse ? n - us : ue;
    const long long base = row * n;
    const long long a0 = (base + tl + xo) & ~3ll;
    const int quads = (int)((base + th + xo - a0 + 3) >> 2);
    for (int q = tid; q < quads; q += nthreads) {
        const long long a = a0 + 4ll * q;
        const long long t0 = a - xo - base;
        float v[4];
        if (t0 >= tl && t0 + 4 <= th) {
            const f32x4 s = *reinterpret_cast<const f32x4*>(x + (a - xo));
            v[0] = s[0]; v[1] = s[1]; v[2] = s[2]; v[3] = s[3];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (t0 + e >= tl && t0 + e < th) ? x[base + t0 + e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long t = t0 + e;
            if (t >= tl && t < th) {
                if (mask_in) v[e] *= (float)((mask_in[row * nw + (t >> 5)] >> (t & 31)) & 1u);
                const long long u = reverse ? n - 1 - t : t;
                xs[pad((int)(u - ub))] = v[e];
            }
        }
    }
    const int j0 = (int)(ue - ub), j1 = (int)(((ue + kChunk - 1) & ~(long long)(kChunk - 1)) - ub);
    for (int j = j0 + tid; j < j1; j += nthreads) xs[pad(j)] = 0.f;
}

__device__ __forceinline__ float clamp1(float y) { return y < -1.f ? -1.f : (y > 1.f ? 1.f : y); }   // NaN stays NaN, as torch.clamp

// mode 0: fp32 | 1: fp32 on the 16-bit grid (round half to even, IEEE division) | 2: int16 codes, truncated toward zero
template <int MODE>
__device__ __forceinline__ typename std::conditional<MODE == 2, short, float>::type epilogue(float y, int clamp) {
    const float c = clamp ? clamp1(y) : y;
    if constexpr (MODE == 0) return c;
    else if constexpr (MODE == 1) return __fdiv_rn(rintf(c * 32767.0f), 32767.0f);
    else return (short)(int)(c * 32767.0f);
}

// the tile's results ys[pad(u - ub)], u in [u0, ue), leave for out[row][t(u)]; quads of 4 elements on absolute boundaries of 4 elements
// (oo: (address of out / element size) % 4).  mask_out (never with `reverse`; u0 % 32 == 0): bit u % 32 of word u / 32 = |y[u]| <= 1.
template <int MODE>
__device__ __forceinline__ void store_tile(const float* ys, void* out_, unsigned* __restrict__ mask_out, long long row, long long n,
                                           long long nw, long long ub, long long u0, long long ue, int reverse, int clamp, int oo, int tid,
                                           int nthreads) {
    using T = typename std::conditional<MODE == 2, short, float>::type;
    typedef T Tx4 __attribute__((ext_vector_type(4)));
    T* out = reinterpret_cast<T*>(out_);
    const long long tl = reverse ? n - ue : u0, th = reverse ? n - u0 : ue;
    const long long base = row * n;
    const long long a0 = (base + tl + oo) & ~3ll;
    const int quads = (int)((base + th + oo - a0 + 3) >> 2);
    for (int q = tid; q < quads; q += nthreads) {
        const long long a = a0 + 4ll * q;
        const long long t0 = a - oo - base;
        Tx4 v = {0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long t = t0 + e;
            if (t >= tl && t < th) {
                const long long u = reverse ? n - 1 - t : t;
                v[e] = epilogue<MODE>(ys[pad((int)(u - ub))], clamp);
            }
        }
        if (t0 >= tl && t0 + 4 <= th) {
            *reinterpret_cast<Tx4*>(out + (a - oo)) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (t0 + e >= tl && t0 + e < th) out[base + t0 + e] = v[e];
        }
    }
    if (mask_out) {
        const int words = (int)((ue - u0 + kChunk - 1) / kChunk);
        for (int w = tid; w < words; w += nthreads) {
            const long long uw = u0 + (long long)w * kChunk;
            const int jb = (int)(uw - ub);
            unsigned bits = 0;
#pragma unroll
            for (int k = 0; k < kChunk; ++k) bits |= (uw + k < ue && fabsf(ys[pad(jb + k)]) <= 1.f) ? (1u << k) : 0u;
            mask_out[row * nw + uw / kChunk] = bits;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void biquad_chunk_kernel(const float* __restrict__ x, void* out, unsigned* __restrict__ mask_out,
                                                                const unsigned* __restrict__ mask_in, Coef c, long long n, long long nw,
                                                                int warm, int clamp, int reverse, int identity, long long tiles_per_row,
                                                                long long tiles, int xo, int oo) {
    extern __shared__ __align__(16) float xs[];
    const int tid = threadIdx.x;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long row = tile / tiles_per_row;
        const long long u0 = (tile - row * tiles_per_row) * kTile;
        const long long ub = u0 - warm;                                       // logical position of xs[0]
        const long long us = ub < 0 ? 0 : ub;
        const long long ue = u0 + kTile < n ? u0 + kTile : n;
        __syncthreads();                                                      // the previous tile has left xs
        stage(xs, x, mask_in, row, n, nw, ub, us, ue, reverse, xo, tid, kThreads);
        __syncthreads();
        const long long c0 = u0 + (long long)tid * kChunk;                    // this lane's chunk
        const int jb = warm + tid * kChunk;
        const bool mine = !identity && c0 < ue;
        float y[kChunk];
        if (mine) {
            int k = c0 - warm < 0 ? (int)-c0 : -warm;                         // before the row: zeros in, zero state -- nothing to run
            float x1 = 0.f, x2 = 0.f, y1 = 0.f, y2 = 0.f;
#pragma unroll 4
            for (; k < 0; ++k) {
                const float x0 = xs[pad(jb + k)];
                const float yy = biquad_step(c, x0, x1, x2, y1, y2);
                x2 = x1; x1 = x0; y2 = y1; y1 = yy;
            }
#pragma unroll
            for (k = 0; k < kChunk; ++k) {
                const float x0 = xs[pad(jb + k)];
                const float yy = biquad_step(c, x0, x1, x2, y1, y2);
                x2 = x1; x1 = x0; y2 = y1; y1 = yy;
                y[k] = yy;
            }
        }
        __syncthreads();                                                      // every lane has read the inputs it shares with its neighbours
        if (mine) {
#pragma unroll
            for (int k = 0; k < kChunk; ++k) xs[pad(jb + k)] = y[k];
        }
        __syncthreads();
        store_tile<MODE>(xs, out, mask_out, row, n, nw, ub, u0, ue, reverse, clamp, oo, tid, kThreads);
    }
}

template <int MODE>
__global__ __launch_bounds__(kRowThreads) void biquad_row_kernel(const float* __restrict__ x, void* out, unsigned* __restrict__ mask_out,
                                                                 const unsigned* __restrict__ mask_in, Coef c, long long rows, long long n,
                                                                 long long nw, int clamp, int reverse, int identity, int xo, int oo) {
    __shared__ __align__(16) float xs[padded(kRowTile)];
    const int tid = threadIdx.x;
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        float x1 = 0.f, x2 = 0.f, y1 = 0.f, y2 = 0.f;                         // lane 0 carries the row's state from tile to tile
        for (long long u0 = 0; u0 < n; u0 += kRowTile) {
            const long long ue = u0 + kRowTile < n ? u0 + kRowTile : n;
            __syncthreads();
            stage(xs, x, mask_in, row, n, nw, u0, u0, ue, reverse, xo, tid, kRowThreads);
            __syncthreads();
            if (tid == 0 && !identity) {
                const int len = (int)(ue - u0);
                for (int j = 0; j < len; ++j) {
                    const float x0 = xs[pad(j)];
                    const float yy = biquad_step(c, x0, x1, x2, y1, y2);
                    x2 = x1; x1 = x0; y2 = y1; y1 = yy;
                    xs[pad(j)] = yy;
                }
            }
            __syncthreads();
            store_tile<MODE>(xs, out, mask_out, row, n, nw, u0, u0, ue, reverse, clamp, oo, tid, kRowThreads);
        }
    }
}

}  // namespace

extern "C" {

// host-only query: samples per chunk of the time-parallel kernel for this warm-up, 0 when the one-lane-per-row kernel runs
int wm_biquad_plan(int warm, int* chunk_len, hipStream_t) {
    if (warm < -1 || !chunk_len) return (int)hipErrorInvalidValue;
    *chunk_len = (warm >= 0 && warm <= kMaxWarm) ? kChunk : 0;
    return 0;
}

int wm_biquad(const float* x, void* out, void* mask_out, const void* mask_in, float b0, float b1, float b2, float a1, float a2,
              long long rows, long long n, int warm, int mode, int clamp, int reverse, hipStream_t stream) {
    if (rows < 1 || n < 1 || rows > (1ll << 46) / n || !x || !out) return (int)hipErrorInvalidValue;
    if (warm < -1 || warm > kMaxWarm || mode < 0 || mode > 2 || (mode == 2 && !clamp) || (mask_out && reverse))
        return (int)hipErrorInvalidValue;
    const unsigned long long count = (unsigned long long)rows * (unsigned long long)n;
    const unsigned long long xbytes = count * 4, obytes = count * (mode == 2 ? 2 : 4);
    const long long nw = (n + 31) / 32;
    const unsigned long long mbytes = (unsigned long long)rows * (unsigned long long)nw * 4;
    if ((uintptr_t)x % 4 || (uintptr_t)out % (mode == 2 ? 2 : 4) || (uintptr_t)mask_out % 4 || (uintptr_t)mask_in % 4)
        return (int)hipErrorInvalidValue;
    if (overlap(x, xbytes, out, obytes)) return (int)hipErrorInvalidValue;      // a chunk reads x behind itself: never in place
    if (mask_out && (overlap(mask_out, mbytes, x, xbytes) || overlap(mask_out, mbytes, out, obytes) ||
                     (mask_in && overlap(mask_out, mbytes, mask_in, mbytes))))
        return (int)hipErrorInvalidValue;
    if (mask_in && overlap(mask_in, mbytes, out, obytes)) return (int)hipErrorInvalidValue;
    const Coef c{b0, b1, b2, a1, a2};
    const int identity = b0 == 1.f && b1 == 0.f && b2 == 0.f && a1 == 0.f && a2 == 0.f;   // quantiser only: x itself, no 0 * inf
    const int xo = (int)(((uintptr_t)x >> 2) & 3);
    const int oo = (int)(((uintptr_t)out >> (mode == 2 ? 1 : 2)) & 3);
    unsigned* mo = reinterpret_cast<unsigned*>(mask_out);
    const unsigned* mi = reinterpret_cast<const unsigned*>(mask_in);
    if (warm < 0) {
        const int grid = (int)(rows < (1ll << 20) ? rows : (1ll << 20));
#define WM_ROW(M) hipLaunchKernelGGL(biquad_row_kernel<M>, dim3(grid), dim3(kRowThreads), 0, stream, x, out, mo, mi, c, rows, n, nw, \
                                     clamp, reverse, identity, xo, oo)
        if (mode == 0) WM_ROW(0); else if (mode == 1) WM_ROW(1); else WM_ROW(2);
#undef WM_ROW
        WM_CHECK_LAUNCH();
        return 0;
    }
    const long long tiles_per_row = (n + kTile - 1) / kTile;
    const long long tiles = rows * tiles_per_row;
    const long long cap = 8ll * kNumCU;
    const int grid = (int)(tiles < cap ? tiles : cap);
    const size_t lds = (size_t)padded(warm + kTile) * 4;                        // <= 38 KB at kMaxWarm
#define WM_CHUNK(M) hipLaunchKernelGGL(biquad_chunk_kernel<M>, dim3(grid), dim3(kThreads), lds, stream, x, out, mo, mi, c, n, nw, warm, \
                                       clamp, reverse, identity, tiles_per_row, tiles, xo, oo)
    if (mode == 0) WM_CHUNK(0); else if (mode == 1) WM_CHUNK(1); else WM_CHUNK(2);
#undef WM_CHUNK
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
