// Spectral masking (Bark bands, Schroeder spreading, Johnston's tonality offset, Terhardt's threshold in quiet) of rows x n fp32 pairs at
// 16 kHz: the noise-to-mask ratio of d = y - x against the mask of x, and the gradient of its hinge with respect to y.  The definition is
// the comment of wm_masking_fwd in include/wm_hip.h; this file is how it is computed.
//
// Forward, two launches on one stream:
//   1 cells     one workgroup of 256 per (row, chunk of kChunk = 16 frames).  The frames go through in pairs: frames f and f + 1 OF THE
//               SAME SIGNAL are the real and the imaginary part of one complex 512-point transform in LDS (wm::fft_dif<9>, result in
//               bit-reversed order), one transform for w x and one for w d, and the two spectra of a pair are separated through conjugate
//               symmetry.  x and d do NOT share a transform: rounding leaves a fixed fraction of the louder part in the spectrum of the
//               other, and d is 40 to 80 dB below x.  Per pair: 257 bin powers per frame and signal to LDS, the two tonality sums
//               (wave butterflies, then four wave totals in a fixed order), 2 x 2 x 22 lanes add the band's bins in increasing k,
//               2 x 22 lanes form the spread mask, the ratio r and (optionally) the backward's coefficient.  Lane (q, b) carries its
//               cells' sums over the chunk; one wave butterfly ends the chunk: 6 words to scratch.
//               THE FORWARD IS FP64 from the window on (the fp64 overload of fft_dif; the window is formed here, not read from a table):
//               the tonality measure is a geometric mean over the bins, so the bins between the harmonics, 70 dB down, decide the offset
//               of the whole frame, and both a transform's rounding (absolute: a fraction of its LARGEST bin) and the rounding of an fp32
//               window (noise 150 dB below the signal in every bin) are relative errors of 1e-5 to 1e-3 there.  Measured on a one-frame
//               row whose float32 yardstick is off by 1e-7 dB in over_db: fp32 throughout 1.8e-6 dB, fp64 transforms behind an fp32 window
//               8e-7, of which the window alone is 5e-7 (the yardstick with only its window rounded).  The price: the transforms' LDS traffic
//               doubles and their arithmetic runs at the fp64 rate (DESIGN.md section 4u has the times).  The tables c_k, S, G, A stay fp32 (2e-7 dB).
//   2 finish    one workgroup per row adds the chunks' sums in fp64 in a fixed order, looks at the samples no frame covers for
//               non-finite values and writes the row's two floats and two counts.
// Backward, one launch: one workgroup per (row, 256 output samples).  Output block h is covered by the second half of frame h - 1 and the
// first half of frame h: w d of the two frames is ONE complex transform, the two spectra are separated, scaled per band and put together
// again as U_a + i U_b with both Hermitian, and the inverse transform (fft_dif on the conjugate) gives u_a in the real and u_b in the
// imaginary part.  Every output sample has one owner and one order of its two terms: no atomics, no carry between workgroups.  A block
// whose 44 coefficients are all zero (and every block no frame covers) is written as zeros without a transform.
// The backward forms w, c_k and band(k) itself: they are closed forms of the definition (the bin counts per band are the header's pin).
//
// No atomics anywhere; all grids are strided loops over tiles that carry their row, so a row's bits know nothing of the batch or the grid.
//
// Safety.  Frame f < F ends at 256 f + 511 < n; the loops over frames, chunks and blocks are bounded by F, C and H from the plan; band
// numbers from the caller's table are clamped to [0, 22) before they become an LDS index.
#include "fft_lds.hpp"
using namespace wm;

namespace {

constexpr int kN = 512, kHop = 256, kBins = 257, kZ = 22, kChunk = 16;
constexpr int kTabC = 0, kTabBand = kTabC + kBins, kTabS = kTabBand + kBins, kTabG = kTabS + kZ * kZ, kTabA = kTabG + kZ;
constexpr int kTabWords = kTabA + kZ;                                             // 1042
constexpr int kPartWords = 6;                                                     // sum r (fp64, lo hi) | sum hinge (fp64) | audible | bad
constexpr long long kGridCap = kNumCU * 8;
constexpr double kD10OverLn10 = 4.342944819032518276511289189166;
constexpr double kTiny = 1e-30;
constexpr float kUnit = (float)((8.0 / 3.0) / (512.0 * 512.0));                   // c_k at k = 0 and 256

// first bin of every band, from the header's bin counts 4 3 3 4 3 4 4 5 5 6 6 8 8 11 13 16 20 23 28 32 38 13
__constant__ int kEdge[kZ + 1] = {0, 4, 7, 10, 14, 17, 21, 25, 30, 35, 41, 47, 55, 63, 74, 87, 103, 123, 146, 174, 206, 244, 257};

struct Fwd {
    const float* x; const float* y; const float* tab;
    float* nmr; float* over; int* counts; float* coef; int* part;
    long long rows, n;
    int F, C, Cs;                                                                 // Cs = max(C, 1): the stride of part
};
struct Bwd {
    const float* x; const float* y; const float* coef; const float* gout; float* gy;
    long long rows, n, H;                                                         // H = ceil(n / 256) output blocks a row
    int F;
};

__device__ __forceinline__ bool finite32(float v) { return fabsf(v) < __builtin_huge_valf(); }
__device__ __forceinline__ double sq(double v) { return v * v; }
__device__ __forceinline__ void twiddles(float2* tw, int tid) {
    double sn, cs;
    sincospi((double)tid / 256.0, &sn, &cs);
    tw[tid] = make_float2((float)cs, (float)-sn);
}

// ---- forward 1: the cells of 16 frames
__global__ __launch_bounds__(256) void masking_cells_kernel(Fwd a) {
    __shared__ double2 tw[kN / 2], zx[kN], zd[kN];
    __shared__ double w[kN], px[2][kBins], pd[2][kBins], ex[2][kZ], ed[2][kZ], red[4][4];
    __shared__ float ck[kBins], S[kZ * kZ], G[kZ], A[kZ];
    __shared__ int band[kBins], edge[kZ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < kN; i += 256) w[i] = 0.5 * (1.0 - cospi((double)i / 256.0));
    for (int i = tid; i < kBins; i += 256) {
        ck[i] = a.tab[kTabC + i];
        band[i] = min(max(__float_as_int(a.tab[kTabBand + i]), 0), kZ - 1);
    }
    for (int i = tid; i < kZ * kZ; i += 256) S[i] = a.tab[kTabS + i];
    if (tid < kZ) { G[tid] = a.tab[kTabG + tid]; A[tid] = a.tab[kTabA + tid]; edge[tid] = kBins; }
    {
        double sn, cs;
        sincospi((double)tid / 256.0, &sn, &cs);
        tw[tid] = make_double2(cs, -sn);
    }
    __syncthreads();
    for (int k = tid; k < kBins; k += 256)
        if (k == 0 || band[k] != band[k - 1]) edge[band[k]] = k;                  // the band table rises: one writer per band
    __syncthreads();
    const int F = a.F;
    const long long tiles = a.rows * a.C;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r = tile / a.C;
        const int c = (int)(tile - r * a.C);
        const int f0 = c * kChunk, fend = min(f0 + kChunk, F);
        const float* __restrict__ xr = a.x + r * a.n;
        const float* __restrict__ yr = a.y + r * a.n;
        double acc_r = 0.0, acc_o = 0.0;                                          // lanes 0..43 of wave 0: (frame parity q, band b)
        int acc_n = 0;
        bool bad = false;
        for (int f = f0; f < fend; f += 2) {
            const bool two = f + 1 < fend;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int t = tid + 256 * h;
                const long long s = (long long)f * kHop + t;
                const float xa = xr[s], ya = yr[s];
                const float xb = two ? xr[s + kHop] : 0.f, yb = two ? yr[s + kHop] : 0.f;
                bad |= !finite32(xa) || !finite32(ya) || !finite32(xb) || !finite32(yb);
                const double wt = w[t];
                zx[t] = make_double2(wt * (double)xa, wt * (double)xb);
                zd[t] = make_double2(wt * (double)(ya - xa), wt * (double)(yb - xb));
            }
            __syncthreads();
            fft_dif<9>(zx, tw, tid);
            fft_dif<9>(zd, tw, tid);
            double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;                           // the logs are near -20 each: their sum in fp32 costs the offset 1e-5 dB
            for (int k = tid; k < kBins; k += 256) {                              // thread 0 takes bin 256 as well
                const int i1 = brev<9>(k), i2 = brev<9>((kN - k) & (kN - 1));
                const double q4 = 0.25 * (double)ck[k];
                double2 p = zx[i1], m = zx[i2];                                   // A = (Z[k] + conj Z[-k]) / 2, B = (Z[k] - conj Z[-k]) / 2i
                const double pa = q4 * (sq(p.x + m.x) + sq(p.y - m.y)), pb = q4 * (sq(p.y + m.y) + sq(m.x - p.x));
                px[0][k] = pa; px[1][k] = pb;
                p = zd[i1]; m = zd[i2];
                pd[0][k] = q4 * (sq(p.x + m.x) + sq(p.y - m.y));
                pd[1][k] = q4 * (sq(p.y + m.y) + sq(m.x - p.x));
                if (k >= 1 && k <= 255) { v0 += log(pa + kTiny); v1 += pa; v2 += log(pb + kTiny); v3 += pb; }
            }
            v0 = wave_sum_d(v0); v1 = wave_sum_d(v1); v2 = wave_sum_d(v2); v3 = wave_sum_d(v3);
            if (lane == 0) { red[wave][0] = v0; red[wave][1] = v1; red[wave][2] = v2; red[wave][3] = v3; }
            __syncthreads();
            if (tid < 4 * kZ) {
                const int q = tid / (2 * kZ), sig = (tid / kZ) & 1, b = tid % kZ;
                const double* __restrict__ src = sig ? pd[q] : px[q];
                double s = 0.0;
                for (int k = edge[b]; k < kBins && band[k] == b; ++k) s += src[k];
                (sig ? ed[q] : ex[q])[b] = s;
            }
            __syncthreads();
            if (tid < 2 * kZ) {
                const int q = tid / kZ, b = tid % kZ;
                if (q == 0 || two) {
                    double C = 0.0;
#pragma unroll
                    for (int j = 0; j < kZ; ++j) C = fma((double)S[b * kZ + j], ex[q][j], C);
                    // the offset, the mask and the ratio's logarithm in fp64: 44 lanes a pair, and fp32 here would cost more than the transforms do
                    const double sl = (red[0][2 * q] + red[1][2 * q]) + (red[2][2 * q] + red[3][2 * q]);
                    const double sp = (red[0][2 * q + 1] + red[1][2 * q + 1]) + (red[2][2 * q + 1] + red[3][2 * q + 1]);
                    const double sfm = kD10OverLn10 * (sl / 255.0 - log(sp / 255.0 + 1e-30));
                    const double alpha = fmin(fmax(sfm / -60.0, 0.0), 1.0);
                    const double O = alpha * (14.5 + (double)b) + (1.0 - alpha) * 5.5;
                    const double T = fmax(C * exp(-O / kD10OverLn10) / (double)G[b], (double)A[b]);
                    const double E = ed[q][b], rr = E / T;
                    const bool hot = rr > 1.0;
                    acc_r += rr;
                    if (hot) { acc_o += kD10OverLn10 * log(rr); ++acc_n; }
                    if (a.coef) a.coef[((r * F) + f + q) * kZ + b] = hot ? (float)(kD10OverLn10 / E) : 0.f;
                }
            }
            // the next pair writes zx / zd (last read before two barriers), px / pd / red behind the transforms' barriers
        }
        const int anybad = __syncthreads_or(bad ? 1 : 0);
        if (wave == 0) {
            acc_r = wave_sum_d(acc_r); acc_o = wave_sum_d(acc_o);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc_n += __shfl_xor(acc_n, o);
            if (lane == 0) {
                int* __restrict__ p = a.part + (r * a.Cs + c) * kPartWords;
                p[0] = __double2loint(acc_r); p[1] = __double2hiint(acc_r);
                p[2] = __double2loint(acc_o); p[3] = __double2hiint(acc_o);
                p[4] = acc_n; p[5] = anybad;
            }
        }
    }
}

// ---- forward 2: the row's numbers
__global__ __launch_bounds__(256) void masking_finish_kernel(Fwd a) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    for (long long r = blockIdx.x; r < a.rows; r += gridDim.x) {
        double sr = 0.0, so = 0.0, cnt = 0.0;
        int bad = 0;
        for (int c = tid; c < a.C; c += 256) {
            const int* __restrict__ p = a.part + (r * a.Cs + c) * kPartWords;
            sr += __hiloint2double(p[1], p[0]);
            so += __hiloint2double(p[3], p[2]);
            cnt += (double)p[4];
            bad |= p[5];
        }
        const long long t0 = a.F > 0 ? (long long)kHop * (a.F + 1) : 0;           // the samples no frame covers: fewer than 512
        for (long long t = t0 + tid; t < a.n; t += 256) bad |= (!finite32(a.x[r * a.n + t]) || !finite32(a.y[r * a.n + t])) ? 1 : 0;
        sr = block_sum_d<4>(sr, red);
        so = block_sum_d<4>(so, red);
        cnt = block_sum_d<4>(cnt, red);                                           // whole numbers below 2^53: exact
        const int anybad = __syncthreads_or(bad);
        if (tid == 0) {
            const double cells = (double)kZ * (double)a.F;
            float nmr = __builtin_nanf(""), over = 0.f;
            int audible = 0, ncells = 0;
            if (anybad) over = __builtin_nanf("");
            else if (a.F > 0) {
                nmr = (float)(10.0 * log10(sr / cells));
                over = (float)(so / cells);
                audible = (int)cnt; ncells = kZ * a.F;
            }
            a.nmr[r] = nmr; a.over[r] = over;
            a.counts[2 * r] = audible; a.counts[2 * r + 1] = ncells;
        }
    }
}

// ---- backward: 256 samples of gy
__global__ __launch_bounds__(256) void masking_bwd_kernel(Bwd a) {
    __shared__ float2 tw[kN / 2], z[kN], v[kN];
    __shared__ float w[kN], g[2][kZ];
    __shared__ int band[kBins];
    const int tid = threadIdx.x;
    for (int i = tid; i < kN; i += 256) w[i] = (float)(0.5 * (1.0 - cospi((double)i / 256.0)));
    for (int k = tid; k < kBins; k += 256) {
        int b = 0;
#pragma unroll
        for (int j = 1; j < kZ; ++j) b += k >= kEdge[j] ? 1 : 0;
        band[k] = b;
    }
    twiddles(tw, tid);
    __syncthreads();
    const int F = a.F;
    const float hc = 2.f * kUnit;                                                 // 2 c_k over the one-sided sum = this over all 512 bins
    const long long tiles = a.rows * a.H;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r = tile / a.H, h = tile - r * a.H;
        const bool hasa = h >= 1 && h - 1 < F, hasb = h < F;                      // frame h - 1 (its second half) and frame h (its first)
        const float* __restrict__ xr = a.x + r * a.n;
        const float* __restrict__ yr = a.y + r * a.n;
        float mine = 0.f;
        if (tid < 2 * kZ) {
            const int q = tid / kZ, b = tid % kZ;
            if (q ? hasb : hasa) mine = a.coef[((r * F) + (h - 1 + q)) * kZ + b];
            g[q][b] = mine;
        }
        const int any = __syncthreads_or(mine != 0.f ? 1 : 0);                    // also: g is published, the tile before is done with v
        const long long tout = h * kHop + tid;
        if (!any) {                                                               // the same for the whole workgroup
            if (tout < a.n) a.gy[r * a.n + tout] = 0.f;
            continue;
        }
        const float scale = a.gout[r] / ((float)kZ * (float)F);                   // any != 0: F > 0
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t = tid + 256 * u;
            const long long sa = (h - 1) * kHop + t, sb = h * kHop + t;
            const float da = hasa ? yr[sa] - xr[sa] : 0.f, db = hasb ? yr[sb] - xr[sb] : 0.f;
            z[t] = make_float2(w[t] * da, w[t] * db);
        }
        __syncthreads();
        fft_dif<9>(z, tw, tid);
        {
            const int k = tid, k2 = tid == 0 ? kN / 2 : kN - tid;                 // thread 0: bins 0 and 256, each its own mirror
            for (int e = 0; e < 2; ++e) {
                const int kk = e == 0 ? k : k2, km = (kN - kk) & (kN - 1);
                if (e == 1 && tid != 0) break;
                const float2 p = z[brev<9>(kk)], m = z[brev<9>(km)];
                const float ax = 0.5f * (p.x + m.x), ay = 0.5f * (p.y - m.y), bx = 0.5f * (p.y + m.y), by = 0.5f * (m.x - p.x);
                const int bk = band[kk <= kN / 2 ? kk : kN - kk];
                const float ga = hc * g[0][bk], gb = hc * g[1][bk];
                // V = ga A + i gb B at kk, ga conj A + i gb conj B at its mirror; the CONJUGATES go into v
                v[kk] = make_float2(ga * ax - gb * by, -(ga * ay + gb * bx));
                if (km != kk) v[km] = make_float2(ga * ax + gb * by, ga * ay - gb * bx);
            }
        }
        __syncthreads();
        fft_dif<9>(v, tw, tid);
        const float2 ra = v[brev<9>(tid + kHop)], rb = v[brev<9>(tid)];          // conj of the transform: u_a = Re, u_b = -Im
        const float val = fmaf(w[tid + kHop], ra.x, w[tid] * -rb.y);
        if (tout < a.n) a.gy[r * a.n + tout] = scale * val;
    }
}

bool plan(long long rows, long long n, long long& F, long long& C) {
    if (rows < 1 || n < 1 || n > (1ll << 34) || rows > (1ll << 46) / n) return false;
    F = n >= kN ? 1 + (n - kN) / kHop : 0;
    C = (F + kChunk - 1) / kChunk;
    return true;
}

unsigned grid_for(long long tiles) { return (unsigned)(tiles < 1 ? 1 : (tiles < kGridCap ? tiles : kGridCap)); }

}  // namespace

extern "C" {

int wm_masking_plan(long long rows, long long n, long long* frames, long long* chunk, long long* scratch_bytes, hipStream_t) {
    long long F = 0, C = 0;
    if (!frames || !chunk || !scratch_bytes || !plan(rows, n, F, C)) return (int)hipErrorInvalidValue;
    *frames = F;
    *chunk = kChunk;
    *scratch_bytes = rows * (C > 0 ? C : 1) * kPartWords * 4;
    return 0;
}

int wm_masking_fwd(const float* x, const float* y, const float* tables, float* nmr_db, float* over_db, int* counts, float* coef,
                   void* scratch, long long rows, long long n, hipStream_t stream) {
    long long F = 0, C = 0;
    if (!plan(rows, n, F, C)) return (int)hipErrorInvalidValue;
    if (!x || !y || !tables || !nmr_db || !over_db || !counts || !scratch) return (int)hipErrorInvalidValue;
    const void* all[8] = {x, y, tables, nmr_db, over_db, counts, coef, scratch};
    for (const void* p : all)
        if ((uintptr_t)p % 4) return (int)hipErrorInvalidValue;
    const unsigned long long in_bytes = (unsigned long long)rows * (unsigned long long)n * 4, row_bytes = (unsigned long long)rows * 4;
    const unsigned long long Cs = (unsigned long long)(C > 0 ? C : 1);
    const void* ins[3] = {x, y, tables};
    const unsigned long long ins_bytes[3] = {in_bytes, in_bytes, (unsigned long long)kTabWords * 4};
    const void* outs[5] = {nmr_db, over_db, counts, scratch, coef};
    const unsigned long long outs_bytes[5] = {row_bytes, row_bytes, 2 * row_bytes, (unsigned long long)rows * Cs * kPartWords * 4,
                                              (unsigned long long)rows * (unsigned long long)F * kZ * 4};
    for (int i = 0; i < 5; ++i) {                                                 // what is written overlaps neither an input nor another output
        if (!outs[i] || !outs_bytes[i]) continue;
        for (int k = 0; k < 3; ++k)
            if (overlap(ins[k], ins_bytes[k], outs[i], outs_bytes[i])) return (int)hipErrorInvalidValue;
        for (int k = i + 1; k < 5; ++k)
            if (outs[k] && outs_bytes[k] && overlap(outs[i], outs_bytes[i], outs[k], outs_bytes[k])) return (int)hipErrorInvalidValue;
    }
    Fwd a;
    a.x = x; a.y = y; a.tab = tables; a.nmr = nmr_db; a.over = over_db; a.counts = counts; a.coef = coef;
    a.part = static_cast<int*>(scratch);
    a.rows = rows; a.n = n; a.F = (int)F; a.C = (int)C; a.Cs = (int)Cs;
    if (F > 0) {
        hipLaunchKernelGGL(masking_cells_kernel, dim3(grid_for(rows * C)), dim3(256), 0, stream, a);
        WM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(masking_finish_kernel, dim3(grid_for(rows)), dim3(256), 0, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}

int wm_masking_bwd(const float* x, const float* y, const float* coef, const float* gout, float* gy, long long rows, long long n,
                   hipStream_t stream) {
    long long F = 0, C = 0;
    if (!plan(rows, n, F, C)) return (int)hipErrorInvalidValue;
    if (!x || !y || !gout || !gy || (F > 0 && !coef)) return (int)hipErrorInvalidValue;
    if ((uintptr_t)x % 4 || (uintptr_t)y % 4 || (uintptr_t)coef % 4 || (uintptr_t)gout % 4 || (uintptr_t)gy % 4) return (int)hipErrorInvalidValue;
    const unsigned long long in_bytes = (unsigned long long)rows * (unsigned long long)n * 4;
    const unsigned long long coef_bytes = (unsigned long long)rows * (unsigned long long)F * kZ * 4;
    if (overlap(x, in_bytes, gy, in_bytes) || overlap(y, in_bytes, gy, in_bytes) || overlap(gout, (unsigned long long)rows * 4, gy, in_bytes) ||
        (coef && coef_bytes && overlap(coef, coef_bytes, gy, in_bytes)))
        return (int)hipErrorInvalidValue;
    Bwd a;
    a.x = x; a.y = y; a.coef = coef; a.gout = gout; a.gy = gy;
    a.rows = rows; a.n = n; a.H = (n + kHop - 1) / kHop; a.F = (int)F;
    hipLaunchKernelGGL(masking_bwd_kernel, dim3(grid_for(rows * a.H)), dim3(256), 0, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
