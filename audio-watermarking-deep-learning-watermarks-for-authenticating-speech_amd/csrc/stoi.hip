// STOI (short-time objective intelligibility, Taal et al. 2011) of rows x n fp32 pairs at 10 kHz.  The definition is the comment of
// wm_stoi in include/wm_hip.h; this file is how it is computed.
//
// Five launches on one stream, every one sized for F = the frames a row of n samples can have; K (the frames a row keeps) is data and
// stays on the device: workgroups whose frames or segments lie beyond it leave early.
//   1 norms     one wave per frame of x: ||w x_f|| (64 lanes x 4 samples, a butterfly sum), NaN where x or y holds a non-finite sample in
//               the frame (the last frame also looks at the samples behind it, which no frame covers).
//   2 compact   one workgroup of 1024 per row: the largest norm, then the kept-frame list in increasing order, 1024 frames a step through
//               wave ballots and a running base; K goes to `kept`, the row's non-finite flag to scratch.
//   3 bands     one workgroup of 256 per 4 spectral frames: frame j of the overlap-added signal is formed on load from the kept frames
//               j - 1, j, j + 1 of x (xs itself never exists), windowed again, and x + i y goes through ONE complex 512-point transform in
//               LDS -- radix-2, decimation in frequency, its first stage folded into the load because the upper 256 inputs are zero, the
//               result left in bit-reversed order.  The two spectra are separated from Z[k] and Z[512 - k] for the 212 bins in use, and
//               2 x 15 lanes per frame add the band's |.|^2 in increasing k.  15 magnitudes per frame and signal go to scratch.
//               The shared transform leaves about 2^-23 of the louder signal in the other one's spectrum; a frame that is all zeros
//               gets bands of exactly zero.
//   4 segments  one lane per segment (256 a workgroup): its 30 frames of a band in registers, the clipped and normalised correlation, the 15
//               bands added in increasing order, one block sum per 256 segments to scratch.
//   5 mean      one workgroup per row adds those partial sums in a fixed order and writes d (or the sentinel, or NaN).
// No atomics: every sum has one owner and an order that depends on the frame or segment index alone, so a row's bits know nothing of
// the batch or of the grid (all grids are strided loops over tiles that carry their row).
//
// Scratch per launch, rows x (32 F + C + 1) words, F' = max(F, 1), C = chunks of 256 segments:  norms [rows][F'] | list [rows][F'] int |
// bands [rows][2][15][F'] | partial [rows][C'] | flag [rows] int.
//
// Safety.  The list holds frame numbers this launch wrote itself; they are clamped to [0, F) all the same before they become an
// address, every loop over frames or segments is bounded by F, and a frame f < F ends at 128 f + 255 < n.
#include "wm_common.hpp"
using namespace wm;

namespace {

constexpr int kFrame = 256, kHop = 128, kFFT = 512, kBands = 15, kSeg = 30, kBin0 = 7, kBins = 212;
constexpr int kNormFrames = 16;                 // frames a workgroup of launch 1 takes: 4 waves x 4
constexpr int kSpecFrames = 4;                  // frame pairs a workgroup of launch 3 transforms at once
constexpr int kSegChunk = 256;                  // segments a workgroup of launch 4 takes
constexpr int kCompact = 1024;
constexpr long long kGridCap = kNumCU * 8;
constexpr float kEps = 2.220446049250313e-16f;  // 2^-52
constexpr float kClip = 6.623413251903491f;     // 1 + 10^(15/20)
constexpr float kSentinel = 1e-5f;

__constant__ int kEdge[kBands + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

struct Args {
    const float* x; const float* y; float* d; int* kept;
    float* norms; int* list; float* bands; float* partial; int* flag;
    long long rows, n;
    int F, Fs, C, Cs;                           // Fs = max(F, 1), Cs = max(C, 1): the strides
};

__device__ __forceinline__ float hann(int t) { return (float)(0.5 * (1.0 - cospi(2.0 * (double)(t + 1) / 257.0))); }
__device__ __forceinline__ bool finite32(float v) { return fabsf(v) < __builtin_huge_valf(); }

// ---- 1: ||w x_f|| per frame, NaN where the frame of x or of y holds a non-finite sample
__global__ __launch_bounds__(256) void stoi_norms_kernel(Args a) {
    __shared__ float w[kFrame];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    w[tid] = hann(tid);
    __syncthreads();
    const long long tpr = (a.F + kNormFrames - 1) / kNormFrames, tiles = a.rows * tpr;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r = tile / tpr;
        const int f0 = (int)(tile - r * tpr) * kNormFrames + wave * 4;
        const float* __restrict__ xr = a.x + r * a.n;
        const float* __restrict__ yr = a.y + r * a.n;
        for (int i = 0; i < 4; ++i) {
            const int f = f0 + i;
            if (f >= a.F) break;
            const long long s = (long long)f * kHop;
            float e = 0.f;
            bool bad = false;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int t = lane + 64 * q;
                const float xv = xr[s + t], yv = yr[s + t];
                bad |= !finite32(xv) || !finite32(yv);
                const float v = w[t] * xv;
                e = fmaf(v, v, e);
            }
            if (f == a.F - 1)                                                     // the samples behind the last frame: at most 128
                for (long long t = s + kFrame + lane; t < a.n; t += 64) bad |= !finite32(xr[t]) || !finite32(yr[t]);
            e = wave_sum(e);
            if (__any(bad)) e = __builtin_nanf("");
            if (lane == 0) a.norms[r * a.Fs + f] = sqrtf(e);
        }
    }
}

// ---- 2: the kept-frame list of a row, in increasing order
__global__ __launch_bounds__(kCompact) void stoi_compact_kernel(Args a) {
    __shared__ float smax[kCompact / 64];
    __shared__ int sbad[kCompact / 64], scount[kCompact / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = a.F;
    for (long long r = blockIdx.x; r < a.rows; r += gridDim.x) {
        const float* __restrict__ nr = a.norms + r * a.Fs;
        int* __restrict__ lr = a.list + r * a.Fs;
        float m = 0.f;
        bool bad = false;
        if (F == 0) {                                                             // no frame has looked at the samples: n <= 256 of them
            for (long long t = tid; t < a.n; t += kCompact) bad |= !finite32(a.x[r * a.n + t]) || !finite32(a.y[r * a.n + t]);
        }
        for (int f = tid; f < F; f += kCompact) {
            const float v = nr[f];
            bad |= !finite32(v);                                                  // NaN from launch 1, or an energy beyond fp32
            m = fmaxf(m, v);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        const bool wbad = __any(bad);
        __syncthreads();                                                          // the arrays' readers of the row before are done
        if (lane == 0) { smax[wave] = m; sbad[wave] = wbad; }
        __syncthreads();
        bool rbad = false;
#pragma unroll
        for (int i = 0; i < kCompact / 64; ++i) { m = fmaxf(m, smax[i]); rbad |= sbad[i] != 0; }
        const float thr = 0.01f * (m + kEps);
        int base = 0;
        if (!rbad) {
            for (int f0 = 0; f0 < F; f0 += kCompact) {
                const int f = f0 + tid;
                const bool keep = f < F && nr[f < F ? f : 0] + kEps > thr;
                const unsigned long long b = __ballot(keep);
                __syncthreads();
                if (lane == 0) scount[wave] = __popcll(b);
                __syncthreads();
                int before = 0, total = 0;
#pragma unroll
                for (int i = 0; i < kCompact / 64; ++i) { const int c = scount[i]; before += i < wave ? c : 0; total += c; }
                if (keep) lr[base + before + __popcll(b & ((1ull << lane) - 1ull))] = f;
                base += total;
            }
        }
        if (tid == 0) { a.kept[r] = base; a.flag[r] = rbad; }
    }
}

// ---- 3: band magnitudes of the spectral frames
__device__ __forceinline__ int bitrev9(int k) { return (int)(__brev((unsigned)k) >> 23); }

__global__ __launch_bounds__(256) void stoi_bands_kernel(Args a) {
    __shared__ float w[kFrame];
    __shared__ float2 tw[kFFT / 2];                                               // e^(-2 pi i k / 512)
    __shared__ float2 z[kSpecFrames][kFFT];
    __shared__ float pw[kSpecFrames][2][kBins];
    __shared__ int nz[kSpecFrames][2][4];                                         // per wave: does the frame of x / of y hold a non-zero sample
    const int tid = threadIdx.x;
    w[tid] = hann(tid);
    {
        double sn, cs;
        sincospi((double)tid / 256.0, &sn, &cs);
        tw[tid] = make_float2((float)cs, (float)-sn);
    }
    __syncthreads();
    const int F = a.F;
    const long long tpr = (F - 1 + kSpecFrames - 1) / kSpecFrames, tiles = F > 1 ? a.rows * tpr : 0;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r = tile / tpr;
        const int j0 = (int)(tile - r * tpr) * kSpecFrames;
        int K = a.kept[r];
        K = K < F ? K : F;
        const int S = K - 1;
        if (j0 >= S) continue;                                                    // the same for the whole workgroup
        const float* __restrict__ xr = a.x + r * a.n;
        const float* __restrict__ yr = a.y + r * a.n;
        const int* __restrict__ lr = a.list + r * a.Fs;
        const int u = tid;
#pragma unroll
        for (int q = 0; q < kSpecFrames; ++q) {
            const int j = j0 + q;
            float2 v = make_float2(0.f, 0.f);
            if (j < S) {                                                          // j + 1 <= K - 1: the list has it
                const int jn = u < kHop ? j - 1 : j + 1;                          // the neighbour that overlaps this half
                const int un = u < kHop ? u + kHop : u - kHop;
                int fc = lr[j], fn = lr[jn < 0 ? 0 : jn];
                fc = min(max(fc, 0), F - 1);
                fn = min(max(fn, 0), F - 1);
                const long long sc = (long long)fc * kHop + u, sn = (long long)fn * kHop + un;
                const float wn = jn < 0 ? 0.f : w[un];
                const float xs = fmaf(wn, xr[sn], w[u] * xr[sc]);
                const float ys = fmaf(wn, yr[sn], w[u] * yr[sc]);
                v = make_float2(w[u] * xs, w[u] * ys);
            }
            const bool anyx = __any(v.x != 0.f), anyy = __any(v.y != 0.f);
            if ((tid & 63) == 0) { nz[q][0][tid >> 6] = anyx; nz[q][1][tid >> 6] = anyy; }
            const float2 t = tw[u];
            z[q][u] = v;                                                          // the first stage: the partner z[u + 256] is zero
            z[q][u + 256] = make_float2(v.x * t.x - v.y * t.y, v.x * t.y + v.y * t.x);
        }
        __syncthreads();
#pragma unroll
        for (int half = 128; half >= 1; half >>= 1) {
            const int pos = tid & (half - 1), i = ((tid - pos) << 1) + pos, jj = i + half;
            const float2 t = tw[pos * (256 / half)];
#pragma unroll
            for (int q = 0; q < kSpecFrames; ++q) {
                const float2 p = z[q][i], c = z[q][jj];
                const float dx = p.x - c.x, dy = p.y - c.y;
                z[q][i] = make_float2(p.x + c.x, p.y + c.y);
                z[q][jj] = make_float2(dx * t.x - dy * t.y, dx * t.y + dy * t.x);
            }
            __syncthreads();
        }
        if (tid < kBins) {
            const int k = kBin0 + tid, i1 = bitrev9(k), i2 = bitrev9(kFFT - k);
#pragma unroll
            for (int q = 0; q < kSpecFrames; ++q) {
                const float2 p = z[q][i1], c = z[q][i2];                          // X = (Z[k] + conj Z[-k]) / 2, Y = (Z[k] - conj Z[-k]) / 2i
                const float xr2 = p.x + c.x, xi2 = p.y - c.y, yr2 = p.y + c.y, yi2 = c.x - p.x;
                pw[q][0][tid] = 0.25f * fmaf(xr2, xr2, xi2 * xi2);
                pw[q][1][tid] = 0.25f * fmaf(yr2, yr2, yi2 * yi2);
            }
        }
        __syncthreads();
        if (tid < kSpecFrames * 2 * kBands) {
            const int q = tid / (2 * kBands), sig = (tid / kBands) & 1, b = tid % kBands, j = j0 + q;
            if (j < S) {
                // x and y share the transform, and rounding leaves about 2^-23 of the one in the spectrum of the other: a frame of
                // zeros has a spectrum of zeros all the same (an all-zero row scores exactly 0)
                const bool live = (nz[q][sig][0] | nz[q][sig][1] | nz[q][sig][2] | nz[q][sig][3]) != 0;
                float s = 0.f;
                for (int k = kEdge[b]; k < kEdge[b + 1]; ++k) s += pw[q][sig][k - kBin0];
                s = live ? s : 0.f;
                a.bands[((r * 2 + sig) * kBands + b) * a.Fs + j] = sqrtf(s);
            }
        }
        __syncthreads();                                                          // z and pw are free for the next tile
    }
}

// ---- 4: the correlations of 256 segments, all bands
__global__ __launch_bounds__(256) void stoi_segments_kernel(Args a) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const long long tiles = a.rows * a.C;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r = tile / a.C;
        const int c = (int)(tile - r * a.C);
        int K = a.kept[r];
        K = K < a.F ? K : a.F;
        const int M = K - kSeg;                                                   // S - 29 segments
        if (c * kSegChunk >= M) continue;                                         // the same for the whole workgroup
        const int m = c * kSegChunk + tid;
        float acc = 0.f;
        if (m < M) {
            for (int b = 0; b < kBands; ++b) {
                const float* __restrict__ xb = a.bands + ((r * 2 + 0) * kBands + b) * a.Fs + m;
                const float* __restrict__ yb = a.bands + ((r * 2 + 1) * kBands + b) * a.Fs + m;
                float xi[kSeg], eta[kSeg];
                float nx = 0.f, ny = 0.f;
#pragma unroll
                for (int i = 0; i < kSeg; ++i) {
                    xi[i] = xb[i]; eta[i] = yb[i];
                    nx = fmaf(xi[i], xi[i], nx); ny = fmaf(eta[i], eta[i], ny);
                }
                const float alpha = sqrtf(nx) / (sqrtf(ny) + kEps);
                float mx = 0.f, my = 0.f;
#pragma unroll
                for (int i = 0; i < kSeg; ++i) {
                    eta[i] = fminf(alpha * eta[i], kClip * xi[i]);
                    mx += xi[i]; my += eta[i];
                }
                mx /= (float)kSeg; my /= (float)kSeg;
                float sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
                for (int i = 0; i < kSeg; ++i) {
                    const float p = xi[i] - mx, q = eta[i] - my;
                    sxx = fmaf(p, p, sxx); syy = fmaf(q, q, syy); sxy = fmaf(p, q, sxy);
                }
                acc += sxy / ((sqrtf(sxx) + kEps) * (sqrtf(syy) + kEps));
            }
        }
        const float total = block_sum<4>(acc, red);
        if (tid == 0) a.partial[r * a.Cs + c] = total;
    }
}

// ---- 5: d per row
__global__ __launch_bounds__(256) void stoi_mean_kernel(Args a) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    for (long long r = blockIdx.x; r < a.rows; r += gridDim.x) {
        int K = a.kept[r];
        K = K < a.F ? K : a.F;
        const int M = K - kSeg;
        const int chunks = M > 0 ? (M + kSegChunk - 1) / kSegChunk : 0;           // <= C
        float s = 0.f;
        for (int c = tid; c < chunks && c < a.C; c += 256) s += a.partial[r * a.Cs + c];
        const float total = block_sum<4>(s, red);
        if (tid == 0) {
            float d = kSentinel;
            if (M > 0) d = total / ((float)kBands * (float)M);
            if (a.flag[r]) d = __builtin_nanf("");
            a.d[r] = d;
        }
    }
}

bool plan(long long rows, long long n, Args& a, long long& words) {
    if (rows < 1 || n < 1 || n > (1ll << 34) || rows > (1ll << 46) / n) return false;
    const long long F = n > kFrame ? (n - kFrame + kHop - 1) / kHop : 0;
    const long long C = F > kSeg ? (F - kSeg + kSegChunk - 1) / kSegChunk : 0;
    a.rows = rows; a.n = n;
    a.F = (int)F; a.Fs = (int)(F > 0 ? F : 1);
    a.C = (int)C; a.Cs = (int)(C > 0 ? C : 1);
    words = rows * ((2 + 2 * kBands) * (long long)a.Fs + a.Cs + 1);
    return true;
}

unsigned grid_for(long long tiles) { return (unsigned)(tiles < 1 ? 1 : (tiles < kGridCap ? tiles : kGridCap)); }

}  // namespace

extern "C" {

int wm_stoi_plan(long long rows, long long n, long long* scratch_bytes, hipStream_t) {
    Args a;
    long long words = 0;
    if (!scratch_bytes || !plan(rows, n, a, words)) return (int)hipErrorInvalidValue;
    *scratch_bytes = words * 4;
    return 0;
}

int wm_stoi(const float* x, const float* y, float* d, int* kept, void* scratch, long long rows, long long n, hipStream_t stream) {
    Args a;
    long long words = 0;
    if (!plan(rows, n, a, words)) return (int)hipErrorInvalidValue;
    if (!x || !y || !d || !kept || !scratch) return (int)hipErrorInvalidValue;
    if ((uintptr_t)x % 4 || (uintptr_t)y % 4 || (uintptr_t)d % 4 || (uintptr_t)kept % 4 || (uintptr_t)scratch % 4) return (int)hipErrorInvalidValue;
    const unsigned long long in_bytes = (unsigned long long)rows * (unsigned long long)n * 4, out_bytes = (unsigned long long)rows * 4;
    const unsigned long long sc_bytes = (unsigned long long)words * 4;
    const void* outs[3] = {d, kept, scratch};
    const unsigned long long outs_bytes[3] = {out_bytes, out_bytes, sc_bytes};
    for (int i = 0; i < 3; ++i) {                                                 // what is written overlaps neither an input nor another output
        if (overlap(x, in_bytes, outs[i], outs_bytes[i]) || overlap(y, in_bytes, outs[i], outs_bytes[i])) return (int)hipErrorInvalidValue;
        for (int k = i + 1; k < 3; ++k)
            if (overlap(outs[i], outs_bytes[i], outs[k], outs_bytes[k])) return (int)hipErrorInvalidValue;
    }
    a.x = x; a.y = y; a.d = d; a.kept = kept;
    float* p = static_cast<float*>(scratch);
    a.norms = p;                               p += rows * a.Fs;
    a.list = reinterpret_cast<int*>(p);        p += rows * a.Fs;
    a.bands = p;                               p += rows * 2 * kBands * (long long)a.Fs;
    a.partial = p;                             p += rows * a.Cs;
    a.flag = reinterpret_cast<int*>(p);
    const long long F = a.F;
    if (F > 0) {
        hipLaunchKernelGGL(stoi_norms_kernel, dim3(grid_for(rows * ((F + kNormFrames - 1) / kNormFrames))), dim3(256), 0, stream, a);
        WM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(stoi_compact_kernel, dim3(grid_for(rows)), dim3(kCompact), 0, stream, a);
    WM_CHECK_LAUNCH();
    if (F > kSeg) {                                                               // fewer frames: no row has a segment
        hipLaunchKernelGGL(stoi_bands_kernel, dim3(grid_for(rows * ((F - 1 + kSpecFrames - 1) / kSpecFrames))), dim3(256), 0, stream, a);
        WM_CHECK_LAUNCH();
        hipLaunchKernelGGL(stoi_segments_kernel, dim3(grid_for(rows * a.C)), dim3(256), 0, stream, a);
        WM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(stoi_mean_kernel, dim3(grid_for(rows)), dim3(256), 0, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
