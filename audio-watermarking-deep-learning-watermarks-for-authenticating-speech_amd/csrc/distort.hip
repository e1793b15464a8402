// Channel distortions along the last axis of rows x n fp32 data: a per-row gain and white Gaussian noise at a per-row SNR, the "volume
// changes" and "additive noise" of the reference README's "Robustness Testing" section, as a step of the graph (forward and backward).
//
//   ms_r = (1/n) sum_t x[r][t]^2      g_r = 10^(gain_db_r / 20)      s_r = |g_r| sqrt(ms_r) 10^(-snr_db_r / 20)   (0: the row gets no noise)
//   y[r][t] = g_r x[r][t] + s_r z(seed, draw, row0 + r, t)
//
// Noise.  z is counter-based (Philox4x32-10, key = the seed's two halves, counter = (t >> 2, 0, row0 + r, draw); its four words give the
// samples 4q .. 4q+3 through two Box-Muller pairs), so nothing is stored for the backward pass, which regenerates it, and no value depends
// on the grid.  A row's gain, SNR and noise coin come from the counter (~0, ~0, row0 + r, draw), which no sample has (n <= 2^34).
//
// Sums.  ms_r and the backward's sum_u dy[u] z(u) are added in ONE order, a function of n alone.  The row is cut into segments of
// kSeg = 16384 samples at multiples of kSeg; one workgroup of 256 lanes sums a segment: lane i takes the quads (4 samples at a multiple of
// 4 IN THE ROW) i, i + 256, ... of the segment in rising order into four chains, one per position in the quad, fmaf(a, b, chain);
// lane total = (c0 + c1) + (c2 + c3); wave total = the xor butterfly 32, 16, .. 1; segment total = wave 0 + 1 + 2 + 3.  A row of one
// segment is finished by that workgroup; a longer one leaves its segment totals in the caller's scratch and a one-wave kernel adds them:
// lane j takes segments j, j + 64, ... in rising order, then the same butterfly.  So a (1, 10^7) row is summed by 611 workgroups.
// Because quads are counted from the row start, a row whose first sample is not on a 16-byte boundary is read by 4-byte loads there.
//
// The apply kernels have no order to keep: a lane owns a group of 4 samples on an absolute 16-byte boundary of the OUTPUT and stores it as
// one 16-byte access wherever the whole group lies inside the row (4-byte accesses at the row's two ends); the inputs are read the same
// way when they share the output's alignment.  Where the group straddles two quads of the row (row start off a 16-byte boundary) the
// lane draws both.  Rows without noise skip the generator: they run at the speed of the copy.  No atomics: one writer per element.
#include <cmath>
#include "wm_draw.hpp"
using namespace wm;

namespace {

constexpr int kThreads = 256;
constexpr int kSeg = 16384;                     // samples of one partial sum
constexpr int kSegQuads = kSeg / 4;
constexpr int kTile = kThreads * 4;             // samples a workgroup applies per step

struct Draw { float gain_lo, gain_hi, snr_lo, snr_hi, p_noise; };

// z of samples 4q .. 4q+3 of row `row`: accurate logf / sincospif (2 u_b is exact, so the angle carries no rounding of its own)
__device__ __forceinline__ void normal_quad(const Rng& g, long long q, unsigned row, float (&z)[4]) {
    unsigned o[4];
    philox4x32_10((unsigned)q, (unsigned)(q >> 32), row, g.draw, g.k0, g.k1, o);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float rad = sqrtf(-2.f * logf(unit(o[2 * p])));
        float sn, cs;
        sincospif(2.f * unit(o[2 * p + 1]), &sn, &cs);
        z[2 * p] = rad * cs;
        z[2 * p + 1] = rad * sn;
    }
}

__device__ __forceinline__ float exp10_db(float db) { return db == 0.f ? 1.f : exp10f(__fdiv_rn(db, 20.f)); }   // 0 dB is exactly 1

// the row's parameters from its mean square: stat[r] = {g, s, ms, snr_db or +inf}
__device__ __forceinline__ void finish_stat(float sum, long long r, long long n, const Rng& g, const Draw& d, float* __restrict__ stat) {
    const float ms = (float)((double)sum / (double)n);
    unsigned o[4];
    philox4x32_10(0xFFFFFFFFu, 0xFFFFFFFFu, (unsigned)(g.row0 + r), g.draw, g.k0, g.k1, o);
    const float gain_db = fmaf(d.gain_hi - d.gain_lo, unit(o[0]), d.gain_lo);
    const float snr_db = fmaf(d.snr_hi - d.snr_lo, unit(o[1]), d.snr_lo);
    const bool noisy = unit(o[2]) < d.p_noise;
    const float gain = exp10_db(gain_db);
    stat[4 * r + 0] = gain;
    stat[4 * r + 1] = noisy ? fabsf(gain) * sqrtf(ms) * exp10_db(-snr_db) : 0.f;
    stat[4 * r + 2] = ms;
    stat[4 * r + 3] = noisy ? snr_db : __builtin_inff();
}

// the factor of x in dx: through * s / (n ms) * sum_u dy[u] z(u); 0 where the level does not depend on x
__device__ __forceinline__ void finish_coef(float sum, long long r, long long n, const float* __restrict__ stat, float* __restrict__ coef) {
    const float s = stat[4 * r + 1], ms = stat[4 * r + 2];
    coef[r] = (s != 0.f && ms != 0.f) ? (float)((double)s * (double)sum / ((double)n * (double)ms)) : 0.f;
}

// BWD 0: the segment's sum of x^2 | 1: of dy z (a is dy); rows without noise have none
template <int BWD>
__global__ __launch_bounds__(kThreads) void distort_sum_kernel(const float* __restrict__ a, float* __restrict__ stat,
                                                               float* __restrict__ partial, float* __restrict__ coef, long long n,
                                                               long long nseg, long long segs, Rng g, Draw d) {
    __shared__ float red[kThreads / kWave];
    const int tid = threadIdx.x;
    for (long long sg = blockIdx.x; sg < segs; sg += gridDim.x) {
        const long long r = sg / nseg, j = sg - r * nseg;
        const long long base = r * n;
        float tot = 0.f;
        if (!BWD || stat[4 * r + 1] != 0.f) {                        // the same for the whole workgroup
            const bool al = aligned16(a, base);
            float c[4] = {0.f, 0.f, 0.f, 0.f};
            for (int k = tid; k < kSegQuads; k += kThreads) {
                const long long q = j * kSegQuads + k;
                if (4 * q >= n) break;
                float v[4], w[4];
                load4(a, base, 4 * q, n, al, v);                     // past the row: zeros, which add nothing
                if (BWD) normal_quad(g, q, (unsigned)(g.row0 + r), w);
#pragma unroll
                for (int e = 0; e < 4; ++e) c[e] = fmaf(v[e], BWD ? w[e] : v[e], c[e]);
            }
            tot = (c[0] + c[1]) + (c[2] + c[3]);
        }
        tot = block_sum<kThreads / kWave>(tot, red);
        if (tid == 0) {
            if (nseg > 1) partial[sg] = tot;
            else if (BWD) finish_coef(tot, r, n, stat, coef);
            else finish_stat(tot, r, n, g, d, stat);
        }
    }
}

// rows of more than one segment: one wave adds a row's segment totals
template <int BWD>
__global__ __launch_bounds__(kWave) void distort_finish_kernel(const float* __restrict__ partial, float* __restrict__ stat,
                                                               float* __restrict__ coef, long long rows, long long n, long long nseg,
                                                               Rng g, Draw d) {
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        float tot = 0.f;
        for (long long j = threadIdx.x; j < nseg; j += kWave) tot += partial[r * nseg + j];
        tot = wave_sum(tot);
        if (threadIdx.x == 0) {
            if (BWD) finish_coef(tot, r, n, stat, coef);
            else finish_stat(tot, r, n, g, d, stat);
        }
    }
}

// BWD 0: out = g a + s z (a is x) | 1: out = g a + coef b (a is dy, b is x)
template <int BWD>
__global__ __launch_bounds__(kThreads) void distort_apply_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                 const float* __restrict__ stat, const float* __restrict__ coef,
                                                                 float* __restrict__ out, long long n, long long tiles_per_row,
                                                                 long long tiles, Rng g) {
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r = tile / tiles_per_row;
        const long long base = r * n;
        const int ob = (int)((((uintptr_t)out >> 2) + (unsigned long long)base) & 3);   // floats from the 16-byte boundary to the row start
        const long long grp = (tile - r * tiles_per_row) * kThreads + threadIdx.x;      // this lane's group of the row
        const long long t0 = 4 * grp - ob;
        if (t0 >= n) continue;
        const float gain = stat[4 * r + 0];
        const float k = BWD ? (coef ? coef[r] : 0.f) : stat[4 * r + 1];                 // the same for the whole workgroup
        float va[4], y[4];
        load4(a, base, t0, n, aligned16(a, base + t0), va);
        if (k == 0.f) {
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = gain * va[e];
        } else if (BWD) {
            float vb[4];
            load4(b, base, t0, n, aligned16(b, base + t0), vb);
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = fmaf(k, vb[e], gain * va[e]);
        } else {
            float z[4];
            normal_quad(g, grp, (unsigned)(g.row0 + r), z);          // samples 4 grp .. 4 grp + 3: the group's elements e >= ob
            if (ob) {                                                // its elements e < ob are the tail of the quad before
                float zb[4] = {0.f, 0.f, 0.f, 0.f};
                if (grp > 0) normal_quad(g, grp - 1, (unsigned)(g.row0 + r), zb);
                float zz[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    zz[e] = 0.f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) if (((e - ob) & 3) == i) zz[e] = e < ob ? zb[i] : z[i];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) z[e] = zz[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = fmaf(k, z[e], gain * va[e]);
        }
        store4(out, base, t0, n, y);
    }
}

// Synthetic room responses (wm_rir_synth): one workgroup per row.  Tap k takes the normal of "sample" k from the counter
// (k >> 2, 0xFFFFFFFE, row0 + r, draw) -- normal_quad with q = 0xFFFFFFFE00000000 | (k >> 2), a high word no sample has -- times
// exp(-k c), the exponent and its argument in fp64, the product in fp32.  E = sum e^2 in the order of the sums above: lane i takes the
// quads i, i + 256, ... in rising order into four fmaf chains, (c0 + c1) + (c2 + c3), the wave butterfly, waves 0 + 1 + 2 + 3.  The
// unscaled taps wait in h itself (a lane reads back only what it wrote); the scalars are formed in fp64 and rounded once.
__global__ __launch_bounds__(kThreads) void rir_synth_kernel(const float* __restrict__ params, float* __restrict__ h, long long rows, int K,
                                                             float sample_rate, Rng g) {
    __shared__ float red[kThreads / kWave];
    const int tid = threadIdx.x;
    const long long qhi = (long long)0xFFFFFFFE00000000ull;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        const float rt60 = params[2 * r], drr = params[2 * r + 1];
        float* __restrict__ hr = h + r * K;
        const bool ok = rt60 > 0.f && __builtin_isfinite(drr);       // the same for the whole workgroup
        const double c = ok ? 6.907755278982137 / ((double)rt60 * (double)sample_rate) : 0.0;      // 3 ln 10
        float ch[4] = {0.f, 0.f, 0.f, 0.f};
        if (ok) {
            for (int q = tid; 4 * q < K; q += kThreads) {
                float z[4];
                normal_quad(g, qhi | (long long)q, (unsigned)(g.row0 + r), z);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = 4 * q + e;
                    if (k >= K) continue;
                    const float ev = k ? z[e] * (float)exp(-(double)k * c) : 0.f;
                    hr[k] = ev;
                    ch[e] = fmaf(ev, ev, ch[e]);
                }
            }
        }
        const float E = block_sum<kThreads / kWave>((ch[0] + ch[1]) + (ch[2] + ch[3]), red);
        const double w = ok ? exp10(-(double)fminf(fmaxf(drr, -100.f), 100.f) / 10.0) : 0.0;
        const double s = 1.0 / sqrt(1.0 + w);
        const float scale = (float)(sqrt(w / (double)E) * s);
        const bool flat = !ok || !(E > 0.f) || !__builtin_isfinite(scale);        // K = 1, E = 0: the response is {1, 0, ...}
        const float h0 = flat ? 1.f : (float)s;
        for (int q = tid; 4 * q < K; q += kThreads) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = 4 * q + e;
                if (k < K) hr[k] = k == 0 ? h0 : (flat ? 0.f : scale * hr[k]);
            }
        }
    }
}

bool shape_ok(long long rows, long long n, long long row0, long long draw) {
    return rows >= 1 && n >= 1 && n <= (1ll << 34) && rows <= (1ll << 46) / n && row0 >= 0 && row0 <= (1ll << 32) - rows && draw >= 0 &&
           draw < (1ll << 32);
}

}  // namespace

extern "C" {

// host-only query: the fp32 elements of scratch both calls need for this shape
int wm_distort_plan(long long rows, long long n, long long* scratch_floats, hipStream_t) {
    if (!scratch_floats || !shape_ok(rows, n, 0, 0)) return (int)hipErrorInvalidValue;
    *scratch_floats = rows * ((n + kSeg - 1) / kSeg + 1);
    return 0;
}

int wm_distort(const float* x, float* y, float* stat, float* scratch, long long rows, long long n, long long row0, long long seed,
               long long draw, float gain_lo, float gain_hi, float snr_lo, float snr_hi, float p_noise, hipStream_t stream) {
    if (!shape_ok(rows, n, row0, draw) || !x || !y || !stat || !scratch) return (int)hipErrorInvalidValue;
    if (!(p_noise >= 0.f && p_noise <= 1.f) || !std::isfinite(gain_lo) || !std::isfinite(gain_hi) || !std::isfinite(snr_lo) ||
        !std::isfinite(snr_hi) ||
        gain_lo > gain_hi || snr_lo > snr_hi)
        return (int)hipErrorInvalidValue;
    if ((uintptr_t)x % 4 || (uintptr_t)y % 4 || (uintptr_t)stat % 4 || (uintptr_t)scratch % 4) return (int)hipErrorInvalidValue;
    const unsigned long long bytes = (unsigned long long)rows * (unsigned long long)n * 4;
    if (overlap(x, bytes, y, bytes)) return (int)hipErrorInvalidValue;            // in place is refused
    const Rng g = make_rng(seed, draw, row0);
    const Draw d{gain_lo, gain_hi, snr_lo, snr_hi, p_noise};
    const long long nseg = (n + kSeg - 1) / kSeg, segs = rows * nseg;
    hipLaunchKernelGGL(distort_sum_kernel<0>, dim3(grid_for(segs)), dim3(kThreads), 0, stream, x, stat, scratch, nullptr, n, nseg, segs, g, d);
    WM_CHECK_LAUNCH();
    if (nseg > 1) {
        hipLaunchKernelGGL(distort_finish_kernel<0>, dim3(grid_for(rows)), dim3(kWave), 0, stream, scratch, stat, nullptr, rows, n, nseg, g, d);
        WM_CHECK_LAUNCH();
    }
    const long long tiles_per_row = (n + 3 + kTile - 1) / kTile, tiles = rows * tiles_per_row;
    hipLaunchKernelGGL(distort_apply_kernel<0>, dim3(grid_for(tiles)), dim3(kThreads), 0, stream, x, nullptr, stat, nullptr, y, n,
                       tiles_per_row, tiles, g);
    WM_CHECK_LAUNCH();
    return 0;
}

int wm_distort_bwd(const float* dy, const float* x, const float* stat, float* dx, float* scratch, long long rows, long long n,
                   long long row0, long long seed, long long draw, int through, hipStream_t stream) {
    if (!shape_ok(rows, n, row0, draw) || !dy || !x || !stat || !dx || !scratch) return (int)hipErrorInvalidValue;
    if ((uintptr_t)dy % 4 || (uintptr_t)x % 4 || (uintptr_t)stat % 4 || (uintptr_t)dx % 4 || (uintptr_t)scratch % 4)
        return (int)hipErrorInvalidValue;
    const unsigned long long bytes = (unsigned long long)rows * (unsigned long long)n * 4;
    if (overlap(dx, bytes, dy, bytes) || overlap(dx, bytes, x, bytes)) return (int)hipErrorInvalidValue;
    const Rng g = make_rng(seed, draw, row0);
    const Draw d{};
    const long long nseg = (n + kSeg - 1) / kSeg, segs = rows * nseg;
    float* coef = through ? scratch + segs : nullptr;                             // behind the segment totals
    float* st = const_cast<float*>(stat);                                         // read only on this path
    if (through) {
        hipLaunchKernelGGL(distort_sum_kernel<1>, dim3(grid_for(segs)), dim3(kThreads), 0, stream, dy, st, scratch, coef, n, nseg, segs, g, d);
        WM_CHECK_LAUNCH();
        if (nseg > 1) {
            hipLaunchKernelGGL(distort_finish_kernel<1>, dim3(grid_for(rows)), dim3(kWave), 0, stream, scratch, st, coef, rows, n, nseg, g, d);
            WM_CHECK_LAUNCH();
        }
    }
    const long long tiles_per_row = (n + 3 + kTile - 1) / kTile, tiles = rows * tiles_per_row;
    hipLaunchKernelGGL(distort_apply_kernel<1>, dim3(grid_for(tiles)), dim3(kThreads), 0, stream, dy, x, stat, coef, dx, n, tiles_per_row,
                       tiles, g);
    WM_CHECK_LAUNCH();
    return 0;
}

int wm_rir_synth(const float* params, float* h, long long rows, int K, float sample_rate, long long row0, long long seed, long long draw,
                 hipStream_t stream) {
    if (K < 1 || K > 16384 || !shape_ok(rows, K, row0, draw) || !params || !h) return (int)hipErrorInvalidValue;
    if (!std::isfinite(sample_rate) || !(sample_rate > 0.f)) return (int)hipErrorInvalidValue;
    if ((uintptr_t)params % 4 || (uintptr_t)h % 4) return (int)hipErrorInvalidValue;
    if (overlap(params, (unsigned long long)rows * 8, h, (unsigned long long)rows * (unsigned long long)K * 4)) return (int)hipErrorInvalidValue;
    const Rng g = make_rng(seed, draw, row0);
    hipLaunchKernelGGL(rir_synth_kernel, dim3(grid_for(rows)), dim3(kThreads), 0, stream, params, h, rows, K, sample_rate, g);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
