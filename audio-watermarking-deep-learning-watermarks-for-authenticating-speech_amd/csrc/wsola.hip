// Pitch-preserving time stretch along the last axis of rows x n fp32 data by waveform-similarity overlap-add (WSOLA), and its adjoint
// with the chosen segment positions held constant.  The definition is the comment of wm_wsola in include/wm_hip.h; this file is how it
// is computed.
//
// Search (mode 0).  One workgroup of 256 lanes per row, the rows grid-stride; the frames of a row in sequence, because frame k's template
// starts where frame k - 1 was placed.  Per frame the template T (L floats) and the candidate region C (L + 2 S floats, rounded up to
// whole groups of four candidates: 12 KiB together at L = 1024, S = 512) are staged in LDS, zero-extended outside the row, so the inner
// loop knows no bounds.  A work item is one of P parts of the sum over j for four neighbouring candidates, item = part NG + group, dealt
// to the lanes 256 at a time: a lane keeps the eight words C[4 g + j .. 4 g + j + 7] in registers and slides them, so four steps of j for
// four candidates -- 16 terms -- cost one 16-byte read of C per lane (consecutive lanes, consecutive 16-byte slots: no bank conflict) and
// one of T (one address: a broadcast), and the loop is bound by its 32 vector instructions, not by LDS.  With one candidate a lane and
// 4-byte reads the same search took 763 us at (512, 16000); see DESIGN.md section 4n.  P exists because the groups never fill the
// workgroup evenly: at (512, 128) 65 groups as whole sums would leave three quarters of the lanes idle; 32 parts of 16 terms make 2080
// items, 9 rounds where 8.1 is the ideal.  The part sums go through LDS (4 NG P floats, at most 34 KiB) and are added in rising part by
// the lane that owns the candidate; the argmin under the tie order is a comparison of (score, rank) pairs -- in the lane, through the
// wave by the xor butterfly, through the four waves by LDS.  Three barriers a frame.  The hop that frame k completes (outputs
// [(k - 1) Hs, k Hs)) is written right after the decision, from the row itself through the caches: 2 Hs loads against (2 S + 1) L terms
// of search.
//
// Synthesis from given positions (mode 1) and the adjoint (mode 2) are sequential in nothing: one lane owns one sample of the result,
// tiles of 256 consecutive samples of one row, grid-stride; one writer per sample, no atomics, no scratch.
//
// Safety.  Every index into a row passes 0 <= i < n before the load, a delta is clamped to [-S, S] on load, the adjoint's bracket of
// frames is cut to [0, K) and to 20 members, and a row whose rate is not in [1/4, 4] is never searched: it gets zeros.
#include "wm_common.hpp"
using namespace wm;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxBracket = 20;                 // frames of one adjoint sample: 4 (L + 2 S) / Hs + 3 <= 19
constexpr int kNoRank = 0x7fffffff;

struct Args {
    const float* x; const float* rate; const float* win; float* y; int* delta;
    long long rows, n_in, n_out, K, tpr, tiles; // K frames a row; tpr tiles per row of the result (modes 1, 2)
    int L, S, Hs, P, NG;                        // P parts of a score's sum, NG groups of four candidates
};

__device__ __forceinline__ bool rate_ok(float r) { return r >= 0.25f && r <= 4.f; }     // NaN fails

// a_k = floor(r o_k + 0.5), o_k = (k - 1) Hs: one fp64 product, one fp64 sum, |a_k| < 2^33
__device__ __forceinline__ long long nominal(double r, long long k, int Hs) {
#pragma clang fp contract(off)
    const double o = (double)((k - 1) * Hs);
    const double v = r * o;
    return (long long)floor(v + 0.5);
}

__device__ __forceinline__ float ext(const float* __restrict__ xr, long long i, long long n) { return (i >= 0 && i < n) ? xr[i] : 0.f; }

__device__ __forceinline__ int clamp_delta(int d, int S) { return d < -S ? -S : (d > S ? S : d); }

// p_k from the caller's delta; entry 0 is not read
__device__ __forceinline__ long long placed(const int* __restrict__ dr, double r, long long k, int Hs, int S) {
    return nominal(r, k, Hs) + (k == 0 ? 0 : clamp_delta(dr[k], S));
}

// output j of the hop between the frames placed at pm and pm1
__device__ __forceinline__ float synth(const float* __restrict__ xr, long long n_in, const float* __restrict__ win, long long pm,
                                       long long pm1, int j, int Hs) {
#pragma clang fp contract(off)
    const float u = ext(xr, pm1 + j, n_in), v = ext(xr, pm + Hs + j, n_in);
    const float d = u - v;
    return fmaf(win[j], d, v);
}

__device__ __forceinline__ bool better(float s, int rank, float best, int brank) { return s < best || (s == best && rank < brank); }

__global__ __launch_bounds__(kThreads) void wsola_search_kernel(Args a) {
    extern __shared__ __align__(16) float lds[];
    __shared__ float wbest[kWaves];
    __shared__ int wrank[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = a.L, S = a.S, Hs = a.Hs, P = a.P, NC = 2 * S + 1, NG = a.NG, PL = L / P, items = NG * P;
    float* __restrict__ T = lds;
    float* __restrict__ C = lds + L;
    float* __restrict__ part = lds + L + L + 4 * NG + 4;
    for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) {
        const float r32 = a.rate[row];
        const float* __restrict__ xr = a.x + row * a.n_in;
        float* __restrict__ yr = a.y + row * a.n_out;
        int* __restrict__ dr = a.delta + row * a.K;
        if (!rate_ok(r32)) {                                                      // the same in every lane of the workgroup
            for (long long t = tid; t < a.n_out; t += kThreads) yr[t] = 0.f;
            for (long long k = tid; k < a.K; k += kThreads) dr[k] = 0;
            continue;
        }
        const double r = r32;
        long long pprev = nominal(r, 0, Hs);
        if (tid == 0) dr[0] = 0;
        for (long long k = 1; k < a.K; ++k) {
            const long long ak = nominal(r, k, Hs), q = pprev + Hs, c0 = ak - S;
            for (int j = tid; j < L; j += kThreads) T[j] = ext(xr, q + j, a.n_in);
            for (int i = tid; i < L + 4 * NG + 4; i += kThreads) C[i] = ext(xr, c0 + i, a.n_in);
            __syncthreads();
            for (int it = tid; it < items; it += kThreads) {
                const int p = it / NG, g = it - p * NG;
                const f32x4* __restrict__ tp = reinterpret_cast<const f32x4*>(T + p * PL);
                const f32x4* __restrict__ cp = reinterpret_cast<const f32x4*>(C + 4 * g + p * PL);
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};                                 // candidates 4 g .. 4 g + 3
                f32x4 lo = cp[0];
#pragma unroll 2
                for (int j = 0; j < PL / 4; ++j) {
                    const f32x4 t = tp[j], hi = cp[j + 1];
                    const float w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
#pragma unroll
                        for (int m = 0; m < 4; ++m) {
                            const float d = t[jj] - w[jj + m];
                            acc[m] = fmaf(d, d, acc[m]);
                        }
                    }
                    lo = hi;
                }
                reinterpret_cast<f32x4*>(part)[it] = acc;
            }
            __syncthreads();
            float best = INFINITY;
            int brank = kNoRank;
            for (int c = tid; c < NC; c += kThreads) {
                float s = part[c];
                for (int p = 1; p < P; ++p) s += part[p * 4 * NG + c];
                const int d = c - S;
                const int rank = d == 0 ? 0 : (d < 0 ? -2 * d - 1 : 2 * d);           // 0, -1, +1, -2, +2, ...
                if (better(s, rank, best, brank)) { best = s; brank = rank; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ob = __shfl_xor(best, o);
                const int orank = __shfl_xor(brank, o);
                if (better(ob, orank, best, brank)) { best = ob; brank = orank; }
            }
            if (lane == 0) { wbest[wave] = best; wrank[wave] = brank; }
            __syncthreads();
            best = wbest[0]; brank = wrank[0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w)
                if (better(wbest[w], wrank[w], best, brank)) { best = wbest[w]; brank = wrank[w]; }
            // a frame whose every score is NaN has no rank: it continues at the nominal position
            const int d = brank == kNoRank ? 0 : ((brank & 1) ? -((brank + 1) >> 1) : (brank >> 1));
            const long long pk = ak + d;
            if (tid == 0) dr[k] = d;
            const long long t0 = (k - 1) * Hs;
            for (int j = tid; j < Hs; j += kThreads)
                if (t0 + j < a.n_out) yr[t0 + j] = synth(xr, a.n_in, a.win, pprev, pk, j, Hs);
            pprev = pk;
        }
    }
}

// mode 1: y[t], t = m Hs + j, from p_m and p_(m+1)
__global__ __launch_bounds__(kThreads) void wsola_synth_kernel(Args a) {
    const int tid = threadIdx.x, Hs = a.Hs;
    for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long row = tile / a.tpr;
        const long long t = (tile - row * a.tpr) * kThreads + tid;
        if (t >= a.n_out) continue;
        const float r32 = a.rate[row];
        float v = 0.f;
        if (rate_ok(r32)) {
            const double r = r32;
            const int* __restrict__ dr = a.delta + row * a.K;
            const long long m = t / Hs;                                           // m + 1 <= K - 1
            v = synth(a.x + row * a.n_in, a.n_in, a.win, placed(dr, r, m, Hs, a.S), placed(dr, r, m + 1, Hs, a.S), (int)(t - m * Hs), Hs);
        }
        a.y[row * a.n_out + t] = v;
    }
}

// mode 2: dx[s] = sum_k W[s - p_k] g[o_k + s - p_k], a gather over the bracket of frames that can reach s.  x is g (rows, n_out), y is dx
// (rows, n_in)
__global__ __launch_bounds__(kThreads) void wsola_adjoint_kernel(Args a) {
    const int tid = threadIdx.x, Hs = a.Hs, L = a.L, S = a.S;
    for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long row = tile / a.tpr;
        const long long s = (tile - row * a.tpr) * kThreads + tid;
        if (s >= a.n_in) continue;
        const float r32 = a.rate[row];
        float acc = 0.f;
        if (rate_ok(r32)) {
            const double r = r32, rh = r * (double)Hs, sd = (double)s;
            const int* __restrict__ dr = a.delta + row * a.K;
            const float* __restrict__ gr = a.x + row * a.n_out;
            // p_k lies within S + 1/2 of r o_k: frame k reaches s only if s - L - S + 1/2 <= r o_k <= s + S + 1/2; one frame of margin each side
            const double lo = fmax(ceil((sd - (double)(L + S) + 0.5) / rh), 0.0), hi = fmin(floor((sd + (double)S + 0.5) / rh) + 2.0, (double)(a.K - 1));
            if (lo <= hi) {
                const long long k0 = (long long)lo;
                const long long span = (long long)hi - k0 + 1;
                const int cnt = span < kMaxBracket ? (int)span : kMaxBracket;
                for (int f = 0; f < cnt; ++f) {
                    const long long k = k0 + f;
                    const long long i = s - placed(dr, r, k, Hs, S);
                    const long long t = (k - 1) * Hs + i;
                    if (i >= 0 && i < L && t >= 0 && t < a.n_out) {
                        const float W = i < Hs ? a.win[i] : 1.f - a.win[i - Hs];
                        acc = fmaf(W, gr[t], acc);
                    }
                }
            }
        }
        a.y[row * a.n_in + s] = acc;
    }
}

}  // namespace

extern "C" {

int wm_wsola(const float* x, const float* rate, const float* win, float* y, int* delta, long long rows, long long n_in, long long n_out,
             int L, int S, int mode, hipStream_t stream) {
    const long long nmax = 1ll << 30;
    if (rows < 1 || n_in < 1 || n_in > nmax || n_out < 1 || n_out > nmax || rows > (1ll << 46) / (n_in > n_out ? n_in : n_out))
        return (int)hipErrorInvalidValue;
    if (L < 64 || L > 1024 || (L & (L - 1)) || S < 1 || S > L / 2 || mode < 0 || mode > 2) return (int)hipErrorInvalidValue;
    if (!x || !rate || !win || !y || !delta || (uintptr_t)x % 4 || (uintptr_t)rate % 4 || (uintptr_t)win % 4 || (uintptr_t)y % 4 ||
        (uintptr_t)delta % 4)
        return (int)hipErrorInvalidValue;
    const int Hs = L / 2;
    const long long K = (n_out + Hs - 1) / Hs + 1;
    const long long n_x = mode == 2 ? n_out : n_in, n_y = mode == 2 ? n_in : n_out;
    const unsigned long long bx = (unsigned long long)rows * n_x * 4, by = (unsigned long long)rows * n_y * 4;
    const unsigned long long br = (unsigned long long)rows * 4, bw = (unsigned long long)Hs * 4, bd = (unsigned long long)rows * K * 4;
    if (overlap(x, bx, y, by) || overlap(rate, br, y, by) || overlap(win, bw, y, by) || overlap(delta, bd, y, by))
        return (int)hipErrorInvalidValue;                                         // in place is refused
    if (mode == 0 && (overlap(x, bx, delta, bd) || overlap(rate, br, delta, bd) || overlap(win, bw, delta, bd)))
        return (int)hipErrorInvalidValue;
    Args a;
    a.x = x; a.rate = rate; a.win = win; a.y = y; a.delta = delta;
    a.rows = rows; a.n_in = n_in; a.n_out = n_out; a.K = K;
    a.L = L; a.S = S; a.Hs = Hs;
    int P = 1;                                                                    // the largest power of two <= min(4096 / S, L / 8)
    while (2 * P <= 4096 / S && 2 * P <= L / 8) P *= 2;
    a.P = P;
    a.NG = (2 * S + 1 + 3) / 4;
    a.tpr = (n_y + kThreads - 1) / kThreads;
    a.tiles = rows * a.tpr;
    const long long cap = (long long)kNumCU * 8;
    if (mode == 0) {
        const size_t lds = ((size_t)2 * L + 4 * a.NG + 4 + (size_t)4 * a.NG * P) * sizeof(float);
        hipLaunchKernelGGL(wsola_search_kernel, dim3((unsigned)(rows < cap ? rows : cap)), dim3(kThreads), lds, stream, a);
    } else if (mode == 1) {
        hipLaunchKernelGGL(wsola_synth_kernel, dim3((unsigned)(a.tiles < cap ? a.tiles : cap)), dim3(kThreads), 0, stream, a);
    } else {
        hipLaunchKernelGGL(wsola_adjoint_kernel, dim3((unsigned)(a.tiles < cap ? a.tiles : cap)), dim3(kThreads), 0, stream, a);
    }
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
