// Short-time spectral Wiener gate with a decision-directed a-priori SNR on rows x n fp32 rows at 16 kHz: the gains come from x, they are
// applied to src (x itself in the forward, dy in the backward: with the gains held the map src -> y is self-adjoint).  The definition is
// the comment of wm_noise_suppress in include/wm_hip.h; this file is how it is computed.
//
// Three launches on one stream, every phase parallel:
//   A analysis   one workgroup of 256 per (row, chunk of kChunk = 16 frames).  Frames m and m + 1 of x are the real and the imaginary part
//                of one complex 512-point transform in LDS (wm::fft_dif<9>, result in bit-reversed order) and are separated through
//                conjugate symmetry.  P[m,k] goes to scratch as fp32; thread k carries the chunk's sum of ln(P + eps) of its bin in a
//                register, frame after frame, and writes it as one fp64 word pair; the chunk's "a sample was not finite" flag follows.
//                THE ANALYSIS IS FP64 from the window on (the fp64 overload of fft_dif): the noise estimate is a geometric mean over
//                the frames, so the weak bins between the harmonics count as much as the strong ones, and a transform's rounding is
//                absolute, about 2^-22 of its LARGEST bin in fp32.
//   B gains      one thread per (row, bin), coalesced over the bins, in workgroups of one wave (an hour in one row is five waves: they
//                should not share a CU).  It adds the chunks' sums in increasing chunk order (an order that depends on n alone), forms
//                N[k], runs the recursion over m in fp64 and overwrites P[m,k] with G[m,k] in place (and writes gain_out / noise_out
//                when given).  The recursion is a dependent chain per bin, so what it waits for is kept off it: P arrives in batches of
//                32 frames, the next batch in flight while this one is walked, P / (over N + eps) is a multiplication by a reciprocal
//                formed once, and xi / (1 + xi) uses the hardware's reciprocal with two Newton steps.  A row with a flag set gets NaN
//                gains and a NaN profile, which the synthesis turns into a NaN row.
//   C synthesis  one workgroup per (row, output hop of 256 samples), fp32.  Output hop h is covered by the second half of frame h and the
//                first half of frame h + 1: w src of the two frames is ONE complex transform, the two spectra are separated, scaled by
//                G[h] and G[h + 1] and put together again as V_a + i V_b with both Hermitian, and the inverse transform (fft_dif on the
//                conjugate) gives frame h's output in the real and frame h + 1's in the imaginary part.  Every output sample has one
//                owner and one order of its two terms; every frame is transformed twice (once as either half), which is what lets a
//                tile know nothing of its neighbours.
//
// No atomics anywhere; all grids are strided loops over tiles that carry their row, so a row's bits know nothing of the batch or the grid.
//
// Safety.  Frame m covers the row's samples (m - 1) 256 + t, t < 512: every read of x and src is guarded by 0 <= s < n.  Frames are bounded
// by M, chunks by C, hops by Hn from the plan; scratch holds rows M 257 floats | rows C 257 word pairs | rows C flags, and every index is
// formed in 64 bits.
#include "fft_lds.hpp"
using namespace wm;

namespace {

constexpr int kN = 512, kHop = 256, kBins = 257, kChunk = 16, kAhead = 8, kBatch = 32, kGainLanes = 64;
constexpr long long kGridCap = kNumCU * 8;
constexpr double kEps = 1e-10;
constexpr double kExpGammaE = 1.7810724179901979852365041031071795491696452143034;    // e^0.5772156649015329

struct Args {
    const float* x; const float* src; const float* noise_in; const float* reduce_db;
    float* y; float* gain_out; float* noise_out;
    float* pg;                                                                    // scratch: P, then G, (rows, M, 257)
    int* part;                                                                    // scratch: the chunks' sums of ln(P + eps), (rows, C, 257) fp64 as word pairs
    int* flag;                                                                    // scratch: (rows, C), 1 where the chunk met a non-finite sample
    long long rows, n, M, C, Hn;                                                  // Hn = ceil(n / 256) output hops a row
    double alpha, over;
};

__device__ __forceinline__ bool finite32(float v) { return fabsf(v) < __builtin_huge_valf(); }
__device__ __forceinline__ double sq(double v) { return v * v; }

// ---- A: the bin powers of 16 frames and their log sums
__global__ __launch_bounds__(256) void ns_analysis_kernel(Args a) {
    __shared__ double2 tw[kN / 2], z[kN];
    __shared__ double w[kN];
    const int tid = threadIdx.x;
    for (int i = tid; i < kN; i += 256) w[i] = sinpi(((double)i + 0.5) / 512.0);
    {
        double sn, cs;
        sincospi((double)tid / 256.0, &sn, &cs);
        tw[tid] = make_double2(cs, -sn);
    }
    __syncthreads();
    const long long tiles = a.rows * a.C;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r = tile / a.C, c = tile - r * a.C;
        const long long f0 = c * kChunk, fend = min(f0 + (long long)kChunk, a.M);
        const float* __restrict__ xr = a.x + r * a.n;
        double acc[2] = {0.0, 0.0};                                               // bin tid, and bin 256 in thread 0
        const bool sums = !a.noise_in;                                            // a given profile: the sums are never read
        bool bad = false;
        for (long long f = f0; f < fend; f += 2) {
            const bool two = f + 1 < fend;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int t = tid + 256 * h;
                const long long sa = (f - 1) * kHop + t, sb = sa + kHop;
                const float xa = (sa >= 0 && sa < a.n) ? xr[sa] : 0.f;
                const float xb = (two && sb < a.n) ? xr[sb] : 0.f;                // sb >= 0 always
                bad |= !finite32(xa) || !finite32(xb);
                const double wt = w[t];
                z[t] = make_double2(wt * (double)xa, wt * (double)xb);
            }
            __syncthreads();
            fft_dif<9>(z, tw, tid);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int k = tid + 256 * j;
                if (k < kBins) {                                                  // j = 1: thread 0 alone, bin 256
                    const double2 p = z[brev<9>(k)], m = z[brev<9>((kN - k) & (kN - 1))];
                    // A = (Z[k] + conj Z[-k]) / 2, B = (Z[k] - conj Z[-k]) / 2i
                    const double pa = 0.25 * (sq(p.x + m.x) + sq(p.y - m.y)), pb = 0.25 * (sq(p.y + m.y) + sq(m.x - p.x));
                    float* __restrict__ dst = a.pg + (r * a.M + f) * kBins + k;
                    dst[0] = (float)pa;
                    if (sums) acc[j] += log(pa + kEps);
                    if (two) {
                        dst[kBins] = (float)pb;
                        if (sums) acc[j] += log(pb + kEps);
                    }
                }
            }
            __syncthreads();                                                      // the next pair writes z
        }
        const int anybad = __syncthreads_or(bad ? 1 : 0);
        int* __restrict__ p = a.part + ((r * a.C + c) * kBins) * 2;
        p[2 * tid] = __double2loint(acc[0]); p[2 * tid + 1] = __double2hiint(acc[0]);
        if (tid == 0) {
            p[2 * 256] = __double2loint(acc[1]); p[2 * 256 + 1] = __double2hiint(acc[1]);
            a.flag[r * a.C + c] = anybad;
        }
    }
}

// ---- B: the noise profile and the gains of one bin
// 1 / d for 1 <= d < inf: the hardware's estimate and two Newton steps (the recursion is a dependent chain: a full division doubles it)
__device__ __forceinline__ double rcp1(double d) {
    double r = __builtin_amdgcn_rcp(d);
    r = fma(r, fma(-d, r, 1.0), r);
    return fma(r, fma(-d, r, 1.0), r);
}

__global__ __launch_bounds__(kGainLanes) void ns_gains_kernel(Args a) {
    const long long total = a.rows * kBins;
    for (long long idx = (long long)blockIdx.x * kGainLanes + threadIdx.x; idx < total; idx += (long long)gridDim.x * kGainLanes) {
        const long long r = idx / kBins;
        const int k = (int)(idx - r * kBins);
        int bad = 0;
        double s = 0.0;
        const int* __restrict__ fl = a.flag + r * a.C;
        const int* __restrict__ pp = a.part + (r * a.C * kBins + k) * 2;
        for (long long c0 = 0; c0 < a.C; c0 += kAhead) {                          // the loads of eight chunks together, their sums in chunk order
            int f[kAhead], lo[kAhead], hi[kAhead];
#pragma unroll
            for (int j = 0; j < kAhead; ++j) {                                    // beyond C: the last chunk again, unused (a load, not a branch)
                const long long c = min(c0 + j, a.C - 1);
                f[j] = fl[c];
                lo[j] = pp[c * kBins * 2];
                hi[j] = pp[c * kBins * 2 + 1];
            }
#pragma unroll
            for (int j = 0; j < kAhead; ++j) {
                const bool in = c0 + j < a.C;
                bad |= in ? f[j] : 0;
                s += in ? __hiloint2double(hi[j], lo[j]) : 0.0;
            }
        }
        const double N = a.noise_in ? (double)a.noise_in[idx] : kExpGammaE * exp(s / (double)a.M);
        float rd = a.reduce_db[r];
        rd = rd != rd ? 0.f : fminf(fmaxf(rd, 0.f), 60.f);
        const double gmin = exp10(-(double)rd / 20.0);
        const double iden = 1.0 / (a.over * N + kEps), alpha = a.alpha, beta = 1.0 - a.alpha;
        const float nanf32 = __builtin_nanf("");
        float* __restrict__ col = a.pg + r * a.M * kBins + k;
        float* __restrict__ gout = a.gain_out ? a.gain_out + r * a.M * kBins + k : nullptr;
        double q = 1.0;
        // two batches of kBatch frames in registers: the loads of the next batch are in flight while the recursion walks this one
        float cur[kBatch], nxt[kBatch];
        const long long last = a.M - 1;
#pragma unroll
        for (int j = 0; j < kBatch; ++j) cur[j] = col[min((long long)j, last) * kBins];
        for (long long m0 = 0; m0 < a.M; m0 += kBatch) {
#pragma unroll
            for (int j = 0; j < kBatch; ++j) nxt[j] = col[min(m0 + kBatch + j, last) * kBins];     // beyond M: frame M - 1 again, unused
            const bool whole = m0 + kBatch <= a.M;                                // one branch a batch, none a frame
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
                if (whole || m0 + j < a.M) {
                    const double g = (double)cur[j] * iden;
                    const double xi = fma(alpha, q, beta * fmax(g - 1.0, 0.0));
                    const double G = fmax(xi * rcp1(1.0 + xi), gmin);
                    q = G * G * g;
                    const float Gf = bad ? nanf32 : (float)G;
                    col[(m0 + j) * kBins] = Gf;
                    if (gout) gout[(m0 + j) * kBins] = Gf;
                }
            }
#pragma unroll
            for (int j = 0; j < kBatch; ++j) cur[j] = nxt[j];
        }
        if (a.noise_out) a.noise_out[idx] = bad ? nanf32 : (float)N;
    }
}

// ---- C: 256 samples of y
__global__ __launch_bounds__(256) void ns_synthesis_kernel(Args a) {
    __shared__ float2 tw[kN / 2], z[kN], v[kN];
    __shared__ float w[kN];
    const int tid = threadIdx.x;
    for (int i = tid; i < kN; i += 256) w[i] = (float)sinpi(((double)i + 0.5) / 512.0);
    {
        double sn, cs;
        sincospi((double)tid / 256.0, &sn, &cs);
        tw[tid] = make_float2((float)cs, (float)-sn);
    }
    __syncthreads();
    const float* __restrict__ src = a.src ? a.src : a.x;
    const long long tiles = a.rows * a.Hn;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r = tile / a.Hn, h = tile - r * a.Hn;                     // frames h (its second half) and h + 1 (its first): h + 1 <= M - 1
        const float* __restrict__ sr = src + r * a.n;
        const float* __restrict__ ga_row = a.pg + (r * a.M + h) * kBins;
        const float* __restrict__ gb_row = ga_row + kBins;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t = tid + 256 * u;
            const long long sa = (h - 1) * kHop + t, sb = h * kHop + t;
            const float da = (sa >= 0 && sa < a.n) ? sr[sa] : 0.f, db = sb < a.n ? sr[sb] : 0.f;
            z[t] = make_float2(w[t] * da, w[t] * db);
        }
        __syncthreads();                                                          // also: the tile before is done with v
        fft_dif<9>(z, tw, tid);
        for (int e = 0; e < 2; ++e) {
            if (e == 1 && tid != 0) break;                                        // thread 0: bins 0 and 256, each its own mirror
            const int kk = e == 0 ? tid : kN / 2, km = (kN - kk) & (kN - 1);
            const float2 p = z[brev<9>(kk)], m = z[brev<9>(km)];
            const float ax = 0.5f * (p.x + m.x), ay = 0.5f * (p.y - m.y), bx = 0.5f * (p.y + m.y), by = 0.5f * (m.x - p.x);
            const float ga = ga_row[kk], gb = gb_row[kk];                         // kk <= 256: the bin itself
            // V = ga A + i gb B at kk, ga conj A + i gb conj B at its mirror; the CONJUGATES go into v
            v[kk] = make_float2(ga * ax - gb * by, -(ga * ay + gb * bx));
            if (km != kk) v[km] = make_float2(ga * ax + gb * by, ga * ay - gb * bx);
        }
        __syncthreads();
        fft_dif<9>(v, tw, tid);
        const float2 ra = v[brev<9>(tid + kHop)], rb = v[brev<9>(tid)];          // conj of the transform: frame h in Re, frame h + 1 in -Im
        const float val = fmaf(w[tid + kHop], ra.x, w[tid] * -rb.y) * (1.f / 512.f);
        const long long tout = h * kHop + tid;
        if (tout < a.n) a.y[r * a.n + tout] = val;
    }
}

bool plan(long long rows, long long n, long long& M, long long& C) {
    if (rows < 1 || n < 1 || n > (1ll << 34) || rows > (1ll << 46) / n) return false;
    M = (n + kHop - 1) / kHop + 1;
    C = (M + kChunk - 1) / kChunk;
    return true;
}
unsigned long long pg_bytes(long long rows, long long M) { return (unsigned long long)rows * M * kBins * 4; }
unsigned long long part_bytes(long long rows, long long C) { return (unsigned long long)rows * C * kBins * 8; }
unsigned long long flag_bytes(long long rows, long long C) { return (unsigned long long)rows * C * 4; }

unsigned grid_for(long long tiles) { return (unsigned)(tiles < 1 ? 1 : (tiles < kGridCap ? tiles : kGridCap)); }

}  // namespace

extern "C" {

int wm_noise_suppress_plan(long long rows, long long n, long long* frames, long long* scratch_bytes, hipStream_t) {
    long long M = 0, C = 0;
    if (!frames || !scratch_bytes || !plan(rows, n, M, C)) return (int)hipErrorInvalidValue;
    *frames = M;
    *scratch_bytes = (long long)(pg_bytes(rows, M) + part_bytes(rows, C) + flag_bytes(rows, C));
    return 0;
}

int wm_noise_suppress(const float* x, const float* src, const float* noise_in, const float* reduce_db, float* y, float* gain_out,
                      float* noise_out, void* scratch, long long rows, long long n, float alpha, float over, hipStream_t stream) {
    long long M = 0, C = 0;
    if (!plan(rows, n, M, C)) return (int)hipErrorInvalidValue;
    if (!x || !reduce_db || !y || !scratch) return (int)hipErrorInvalidValue;
    if (!(alpha >= 0.f && alpha < 1.f) || !(over > 0.f && over < __builtin_huge_valf())) return (int)hipErrorInvalidValue;
    const void* all[8] = {x, src, noise_in, reduce_db, y, gain_out, noise_out, scratch};
    for (const void* p : all)
        if ((uintptr_t)p % 4) return (int)hipErrorInvalidValue;
    const unsigned long long in_bytes = (unsigned long long)rows * (unsigned long long)n * 4, row_bytes = (unsigned long long)rows * 4;
    const unsigned long long prof_bytes = (unsigned long long)rows * kBins * 4;
    const unsigned long long sc_bytes = pg_bytes(rows, M) + part_bytes(rows, C) + flag_bytes(rows, C);
    const void* ins[4] = {x, src, noise_in, reduce_db};
    const unsigned long long ins_bytes[4] = {in_bytes, in_bytes, prof_bytes, row_bytes};
    const void* outs[4] = {y, gain_out, noise_out, scratch};
    const unsigned long long outs_bytes[4] = {in_bytes, pg_bytes(rows, M), prof_bytes, sc_bytes};
    for (int i = 0; i < 4; ++i) {                                                 // what is written overlaps neither an input nor another output
        if (!outs[i]) continue;
        for (int k = 0; k < 4; ++k)
            if (ins[k] && overlap(ins[k], ins_bytes[k], outs[i], outs_bytes[i])) return (int)hipErrorInvalidValue;
        for (int k = i + 1; k < 4; ++k)
            if (outs[k] && overlap(outs[i], outs_bytes[i], outs[k], outs_bytes[k])) return (int)hipErrorInvalidValue;
    }
    Args a;
    a.x = x; a.src = src; a.noise_in = noise_in; a.reduce_db = reduce_db; a.y = y; a.gain_out = gain_out; a.noise_out = noise_out;
    a.pg = static_cast<float*>(scratch);
    a.part = reinterpret_cast<int*>(static_cast<char*>(scratch) + pg_bytes(rows, M));
    a.flag = reinterpret_cast<int*>(static_cast<char*>(scratch) + pg_bytes(rows, M) + part_bytes(rows, C));
    a.rows = rows; a.n = n; a.M = M; a.C = C; a.Hn = (n + kHop - 1) / kHop;
    a.alpha = (double)alpha; a.over = (double)over;
    hipLaunchKernelGGL(ns_analysis_kernel, dim3(grid_for(rows * C)), dim3(256), 0, stream, a);
    WM_CHECK_LAUNCH();
    hipLaunchKernelGGL(ns_gains_kernel, dim3(grid_for((rows * kBins + kGainLanes - 1) / kGainLanes)), dim3(kGainLanes), 0, stream, a);
    WM_CHECK_LAUNCH();
    hipLaunchKernelGGL(ns_synthesis_kernel, dim3(grid_for(rows * a.Hn)), dim3(256), 0, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
