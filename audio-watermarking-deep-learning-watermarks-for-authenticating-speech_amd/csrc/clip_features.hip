// Speech / noise / silence features of rows x n fp32 clips: the feature table of dataset_creation/noise.py and the rms of silent.py in ONE
// launch.  The definition is the comment of wm_clip_features in include/wm_hip.h; this file is how it is computed.
//
// One workgroup of 512 threads per row (a strided loop over rows), no scratch, no atomics: every sum has one owner and an order that
// depends on n and the sample rate alone, so a row's bits know nothing of the batch or of the grid.
//   stage     the row goes to LDS while its sum, its sum of squares and its non-finite flag are taken (n <= 16384: one read from HBM; a
//             longer row stays where it is and the later passes re-read it through L2)
//   moments   the mean first, then the central second and fourth moments
//   energy    one wave per 25-ms frame: its mean square to LDS, then mean and population deviation over the frames, two passes
//   band-pass 256 of the threads, one chunk of ceil(n / 256) | 1 samples each (odd: the lanes' LDS reads fall on different banks), five
//             cascaded second-order sections in transposed direct form II from zero state, started `warm` samples before the chunk
//             (or at sample 0, where the zero state is the true one); the chunk's own outputs are squared and added
//   spectra   two groups of 256 threads, one PAIR of neighbouring frames each: frame 2p real, frame 2p + 1 imaginary, one complex
//             2048-point transform in LDS (fft_lds.hpp), the two spectra separated from Z[k] and Z[2048 - k].  Neighbours overlap by
//             three quarters, so the 2^-23 of the louder frame that rounding leaves in the other one's spectrum stays 2^-23 of its own; a
//             frame whose windowed samples are all zero gets a spectrum of exactly zero.  The magnitudes go back to LDS in natural
//             order, index k + (k >> 5) (the writers of a wave differ in bits 5..9 of k: the skew spreads them over the banks).
//             Each thread then owns four neighbouring bins: one inclusive wave scan per frame gives sum S and the prefix sums the
//             roll-off bin is searched in, a second pass the bandwidth around the centroid.  2 x 128 threads form the mel energies
//             of the pair and their dB into the F x 128 table; the weights are the dense table's non-zero runs (band limits klo / khi),
//             copied to LDS once per workgroup, one run after the other.
//             The zero-crossing count of a frame is taken while the frame is loaded.
//   cepstrum  dB clamped at the clip's maximum - 80, 13 x F dot products with the DCT rows, mean and variance over the frames per
//             coefficient, the means of those
//   finish    thread 0 adds the per-frame values in frame order, forms the ratios and the score, and writes the row.
//
// Safety.  No index depends on a sample's value.  Every sample index is clamped to [0, n) or tested against it, frames and 25-ms frames
// are counted from n on the host (plan), the mel band limits are clamped to [0, 1024], and all LDS regions are carved from plan's sizes.
#include "fft_lds.hpp"
using namespace wm;

namespace {

constexpr int kN = 2048, kLog = 11, kHop = 512, kMels = 128, kMfcc = 13, kSections = 5;
constexpr int kThreads = 512, kWaves = kThreads / 64, kGroups = kThreads / 256;
constexpr int kBpThreads = 256;
constexpr int kMinN = 400, kMaxN = 32768, kStageMax = 16384;
constexpr int kMaxF = 1 + kMaxN / kHop;          // 65
constexpr int kFs = 68;                          // stride of the per-frame arrays (>= kMaxF, a multiple of 4)
constexpr int kDbStride = kMels + 1;             // rows of the dB table are read down a column by the cepstrum
constexpr int kFeat = 16, kCounts = 4;
constexpr int kTail = 4 * kFs + kWaves * 4 + 2 * kGroups * 4 * 6 + 48;      // per-frame arrays, the three reduction areas, cepstrum and row stats
constexpr int kWcap = 2304;                      // mel weights kept in LDS: the triangles' non-zero runs, one after the other (2050 + 128 at most
                                                 // for triangles that overlap by half; a mel whose run no longer fits reads the dense table)
constexpr int kMelTab = kWcap + 3 * kMels;
constexpr float kTiny = 1.17549435e-38f;

struct Args {
    const float* x; const float* sos; const float* fb; const int* klo; const int* khi; const float* dct;
    float* feat; int* counts; float* frames;
    long long rows;
    int n, sr, F, L, H, NF, warm, stage;         // stage: floats of LDS that hold the row; 0: the row is read where it is
};

constexpr int db_floats(int F) { return (F * kDbStride + 3) & ~3; }
constexpr size_t lds_bytes(int stage, int F) { return (size_t)(stage + db_floats(F) + kGroups * 2 * kN + kN + kTail + kMelTab) * sizeof(float); }
constexpr size_t kLdsMax = lds_bytes(kStageMax, 1 + kStageMax / kHop) > lds_bytes(0, kMaxF) ? lds_bytes(kStageMax, 1 + kStageMax / kHop)
                                                                                             : lds_bytes(0, kMaxF);
static_assert(kLdsMax <= 160 * 1024, "one workgroup's LDS");

__device__ __forceinline__ bool finite32(float v) { return fabsf(v) < __builtin_huge_valf(); }
__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
__device__ __forceinline__ int pad(int k) { return k + (k >> 5); }
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_incl_scan(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}
// sums over the workgroup of K values per thread, the waves added in rising order; valid in every thread.  red: kWaves * 4 floats
template <int K>
__device__ __forceinline__ void block_sums(float (&v)[K], float* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[w * 4 + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < kWaves; ++i) s += red[i * 4 + k];
        v[k] = s;
    }
}
// does position i of a frame count as a zero crossing: v is the sample there, u the one before it
__device__ __forceinline__ int crossing(float v, float u) {
    v = fabsf(v) <= 1e-10f ? 0.f : v;
    u = fabsf(u) <= 1e-10f ? 0.f : u;
    return (int)((__float_as_uint(v) ^ __float_as_uint(u)) >> 31);
}

// -DWM_CLIP_FEATURES_STAMPS (a diagnostic build, never the product): thread 0 reads the 100 MHz clock between the stages and the
// reserved columns 13..15 carry the ticks of the time-domain passes, the band-pass and the spectra
#ifdef WM_CLIP_FEATURES_STAMPS
#define WM_CF_STAMP(i) stamp[i] = wall_clock64()
#else
#define WM_CF_STAMP(i)
#endif

__global__ __launch_bounds__(kThreads) void clip_features_kernel(Args a) {
    extern __shared__ __align__(16) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = tid >> 8, t = tid & 255, gw = wave & 3;
    const int n = a.n, F = a.F;
    float* row = smem;
    float* db = smem + a.stage;
    float2* z = reinterpret_cast<float2*>(db + db_floats(F));
    float2* tw = z + kGroups * kN;
    float* fcen = reinterpret_cast<float*>(tw + kN / 2);
    float* fbw = fcen + kFs;
    float* fro = fbw + kFs;
    int* fzc = reinterpret_cast<int*>(fro + kFs);
    float* bred = reinterpret_cast<float*>(fzc + kFs);                            // [kWaves][4]
    float* gredf = bred + kWaves * 4;                                             // [kGroups][4 waves][6]
    int* gredi = reinterpret_cast<int*>(gredf + kGroups * 4 * 6);                 // [kGroups][4 waves][6]
    float* mstat = reinterpret_cast<float*>(gredi + kGroups * 4 * 6);             // [2][16]
    float* rstat = mstat + 32;                                                    // the row's time-domain sums, kept by thread 0's readers
    float* wc = rstat + 16;                                                       // [kWcap]
    int* mk0 = reinterpret_cast<int*>(wc + kWcap);                                // [kMels] first bin, length and place in wc (-1: not held)
    int* mlen = mk0 + kMels;
    int* moff = mlen + kMels;
    float2* zg = z + g * kN;
    float* gf = gredf + g * 4 * 6;
    int* gi = gredi + g * 4 * 6;

    for (int k = tid; k < kN / 2; k += kThreads) {
        float s, c;
        sincospif(-2.0f * (float)k / (float)kN, &s, &c);
        tw[k] = make_float2(c, s);
    }
    if (tid < kMels) {
        const int k0 = max(a.klo[tid], 0), k1 = min(a.khi[tid], kN / 2);
        mk0[tid] = k0;
        mlen[tid] = max(k1 - k0 + 1, 0);
    }
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int m = 0; m < kMels; ++m) {
            const bool fits = o + mlen[m] <= kWcap;
            moff[m] = fits ? o : -1;
            o += fits ? mlen[m] : 0;
        }
    }
    __syncthreads();
    for (int m = wave; m < kMels; m += kWaves)
        if (moff[m] >= 0)
            for (int i = lane; i < mlen[m]; i += 64) wc[moff[m] + i] = a.fb[(mk0[m] + i) * kMels + m];
    const float hz = (float)a.sr / (float)kN;
    const int npairs = (F + 1) >> 1;

    for (long long r = blockIdx.x; r < a.rows; r += gridDim.x) {
        const float* __restrict__ xr = a.x + r * n;
        const float* src = a.stage ? row : xr;
        __syncthreads();                                                          // the row before is finished with LDS; tw is published
#ifdef WM_CLIP_FEATURES_STAMPS
        unsigned long long stamp[4];
#endif
        WM_CF_STAMP(0);
        // ---- stage, sum, sum of squares, the non-finite flag
        float m[2] = {0.f, 0.f};
        int bad = 0;
#pragma unroll 4
        for (int i = tid; i < n; i += kThreads) {
            const float v = xr[i];
            if (a.stage) row[i] = v;
            m[0] += v;
            m[1] = fmaf(v, v, m[1]);
            bad |= !finite32(v);
        }
        bad = __syncthreads_or(bad);                                              // publishes the staged row as well
        block_sums<2>(m, bred);
        const float mean = m[0] / (float)n;
        if (tid == 0) rstat[0] = m[1] / (float)n;
        // ---- central moments
        float c[2] = {0.f, 0.f};
#pragma unroll 4
        for (int i = tid; i < n; i += kThreads) {
            const float d = src[i] - mean, d2 = d * d;
            c[0] += d2;
            c[1] = fmaf(d2, d2, c[1]);
        }
        block_sums<2>(c, bred);
        if (tid == 0) { rstat[1] = c[0] / (float)n; rstat[2] = c[1] / (float)n; }
        // ---- spread of the 25-ms frame energies
        float* ef = reinterpret_cast<float*>(z);
        for (int f = wave; f < a.NF; f += kWaves) {
            const int s0 = f * a.H;
            float e = 0.f;
#pragma unroll 2
            for (int i = lane; i < a.L; i += 64) {
                const float v = src[s0 + i];
                e = fmaf(v, v, e);
            }
            e = wave_sum(e);
            if (lane == 0) ef[f] = e / (float)a.L;
        }
        __syncthreads();
        float es[1] = {0.f};
        for (int f = tid; f < a.NF; f += kThreads) es[0] += ef[f];
        block_sums<1>(es, bred);
        const float emean = es[0] / (float)a.NF;
        float ev[1] = {0.f};
        for (int f = tid; f < a.NF; f += kThreads) {
            const float d = ef[f] - emean;
            ev[0] = fmaf(d, d, ev[0]);
        }
        block_sums<1>(ev, bred);                                                  // its barriers also free ef (= z) for the frames
        if (tid == 0) rstat[3] = sqrtf(ev[0] / (float)a.NF);
        // ---- band-pass energy
        WM_CF_STAMP(1);
        float bp[1] = {0.f};
        if (tid < kBpThreads) {
            const int C = ((n + kBpThreads - 1) / kBpThreads) | 1, start = tid * C;
            if (start < n) {
                const int end = min(start + C, n), i0 = max(start - a.warm, 0);
                float coef[kSections][5];                                         // b0 b1 b2 a1 a2 of a section (a0 = 1)
#pragma unroll
                for (int s = 0; s < kSections; ++s) {
                    coef[s][0] = a.sos[6 * s]; coef[s][1] = a.sos[6 * s + 1]; coef[s][2] = a.sos[6 * s + 2];
                    coef[s][3] = a.sos[6 * s + 4]; coef[s][4] = a.sos[6 * s + 5];
                }
                float s1[kSections], s2[kSections];
#pragma unroll
                for (int s = 0; s < kSections; ++s) s1[s] = s2[s] = 0.f;
#pragma unroll 2
                for (int i = i0; i < end; ++i) {
                    float v = src[i];
#pragma unroll
                    for (int s = 0; s < kSections; ++s) {
                        const float y = fmaf(coef[s][0], v, s1[s]);
                        s1[s] = fmaf(coef[s][1], v, s2[s]) - coef[s][3] * y;
                        s2[s] = coef[s][2] * v - coef[s][4] * y;
                        v = y;
                    }
                    if (i >= start) bp[0] = fmaf(v, v, bp[0]);
                }
            }
        }
        block_sums<1>(bp, bred);
        if (tid == 0) rstat[4] = bp[0] / (float)n;

        // ---- spectra, one pair of frames per group of 256 threads
        WM_CF_STAMP(2);
        float dmax = -__builtin_huge_valf();
        for (int p0 = 0; p0 < npairs; p0 += kGroups) {
            const int p = p0 + g, fa = 2 * p;
            const bool pv = p < npairs, bv = pv && fa + 1 < F;
            int zca = 0, zcb = 0;
            bool nza = false, nzb = false;
#pragma unroll 2
            for (int j = 0; j < kN / 256; ++j) {
                const int idx = t + 256 * j;
                float va = 0.f, vb = 0.f;
                if (pv) {
                    const float cs = tw[idx & (kN / 2 - 1)].x;                    // cos(2 pi idx / 2048) = -cos(2 pi (idx - 1024) / 2048)
                    const float w = idx < kN / 2 ? 0.5f - 0.5f * cs : 0.5f + 0.5f * cs;     // the periodic Hann window
                    const int pa = fa * kHop + idx - kN / 2, pb = pa + kHop;
                    const float ca = src[clampi(pa, n)], ua = src[clampi(pa - 1, n)];
                    if (idx >= 1) zca += crossing(ca, ua);
                    va = (pa >= 0 && pa < n) ? ca * w : 0.f;
                    if (bv) {
                        const float cb = src[clampi(pb, n)], ub = src[clampi(pb - 1, n)];
                        if (idx >= 1) zcb += crossing(cb, ub);
                        vb = (pb >= 0 && pb < n) ? cb * w : 0.f;
                    }
                }
                nza |= va != 0.f;
                nzb |= vb != 0.f;
                zg[idx] = make_float2(va, vb);
            }
            zca = wave_sum_i(zca);
            zcb = wave_sum_i(zcb);
            const int anya = __any(nza) ? 1 : 0, anyb = __any(nzb) ? 1 : 0;
            if (lane == 0) { gi[gw * 6 + 0] = zca; gi[gw * 6 + 1] = zcb; gi[gw * 6 + 2] = anya; gi[gw * 6 + 3] = anyb; }
            __syncthreads();
            fft_dif<kLog>(zg, tw, t);
            // the two spectra, from the slots in the order they lie in: even slots hold the bins below 1024, slot 1 holds bin 1024
            const bool la = (gi[2] | gi[8] | gi[14] | gi[20]) != 0, lb = (gi[3] | gi[9] | gi[15] | gi[21]) != 0;
            float2 S[5];
            int kk[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int s = j < 4 ? 2 * (t + 256 * j) : 1;
                const int k = brev<kLog>(s);
                const float2 zk = zg[s], zn = zg[brev<kLog>((kN - k) & (kN - 1))];
                const float ax = 0.5f * (zk.x + zn.x), ay = 0.5f * (zk.y - zn.y), bx = 0.5f * (zk.y + zn.y), by = 0.5f * (zn.x - zk.x);
                S[j] = make_float2(la ? sqrtf(fmaf(ax, ax, ay * ay)) : 0.f, lb ? sqrtf(fmaf(bx, bx, by * by)) : 0.f);
                kk[j] = k;
            }
            __syncthreads();                                                      // every slot has been read
#pragma unroll
            for (int j = 0; j < 5; ++j)
                if (j < 4 || t == 0) zg[pad(kk[j])] = S[j];
            __syncthreads();
            // four neighbouring bins per thread (thread 255: bin 1024 as well)
            float2 v[5];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = zg[pad(4 * t + j)];
            v[4] = t == 255 ? zg[pad(kN / 2)] : make_float2(0.f, 0.f);
            float suma = 0.f, sumb = 0.f, ksa = 0.f, ksb = 0.f;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const float kf = (float)(4 * t + j);
                suma += v[j].x; sumb += v[j].y;
                ksa = fmaf(kf, v[j].x, ksa); ksb = fmaf(kf, v[j].y, ksb);
            }
            const float ia = wave_incl_scan(suma, lane), ib = wave_incl_scan(sumb, lane);
            ksa = wave_sum(ksa);
            ksb = wave_sum(ksb);
            if (lane == 63) { gf[gw * 6 + 0] = ia; gf[gw * 6 + 1] = ib; gf[gw * 6 + 2] = ksa; gf[gw * 6 + 3] = ksb; }
            __syncthreads();
            float offa = 0.f, offb = 0.f, tota = 0.f, totb = 0.f, kta = 0.f, ktb = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                if (w == gw) { offa = tota; offb = totb; }
                tota += gf[w * 6 + 0]; totb += gf[w * 6 + 1]; kta += gf[w * 6 + 2]; ktb += gf[w * 6 + 3];
            }
            const bool oka = tota >= kTiny, okb = totb >= kTiny;                  // false for a NaN as well
            const float cena = oka ? kta / tota : 0.f, cenb = okb ? ktb / totb : 0.f;     // in bins
            const float thra = 0.85f * tota, thrb = 0.85f * totb;
            float cuma = offa + (ia - suma), cumb = offb + (ib - sumb), bwa = 0.f, bwb = 0.f;
            int roa = kN, rob = kN;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int k = 4 * t + j;
                if (j < 4 || t == 255) {
                    cuma += v[j].x; cumb += v[j].y;
                    if (cuma >= thra && roa == kN) roa = k;
                    if (cumb >= thrb && rob == kN) rob = k;
                    const float da = (float)k - cena, dbn = (float)k - cenb;
                    bwa = fmaf(v[j].x, da * da, bwa); bwb = fmaf(v[j].y, dbn * dbn, bwb);
                }
            }
            bwa = wave_sum(bwa);
            bwb = wave_sum(bwb);
            roa = wave_min_i(roa);
            rob = wave_min_i(rob);
            if (lane == 0) { gf[gw * 6 + 4] = bwa; gf[gw * 6 + 5] = bwb; gi[gw * 6 + 4] = roa; gi[gw * 6 + 5] = rob; }
            __syncthreads();
            if (t == 0 && pv) {
                float ba = 0.f, bb = 0.f;
                int ra = kN / 2, rb = kN / 2, za = 0, zb = 0;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    ba += gf[w * 6 + 4]; bb += gf[w * 6 + 5];
                    ra = min(ra, gi[w * 6 + 4]); rb = min(rb, gi[w * 6 + 5]);
                    za += gi[w * 6 + 0]; zb += gi[w * 6 + 1];
                }
                fcen[fa] = cena * hz;
                fbw[fa] = oka ? sqrtf(ba / tota) * hz : 0.f;
                fro[fa] = oka ? (float)ra : 0.f;
                fzc[fa] = za;
                if (bv) {
                    fcen[fa + 1] = cenb * hz;
                    fbw[fa + 1] = okb ? sqrtf(bb / totb) * hz : 0.f;
                    fro[fa + 1] = okb ? (float)rb : 0.f;
                    fzc[fa + 1] = zb;
                }
            }
            {   // mel energies and their dB: threads 0..127 frame 2p, 128..255 frame 2p + 1
                const int sig = t >> 7, mel = t & (kMels - 1), f = fa + sig;
                if (pv && f < F) {
                    const int k0 = mk0[mel], len = mlen[mel], off = moff[mel];
                    const float* __restrict__ wsrc = off >= 0 ? wc + off : a.fb + (size_t)k0 * kMels + mel;
                    const int wstep = off >= 0 ? 1 : kMels;
                    float acc = 0.f;
#pragma unroll 4
                    for (int i = 0; i < len; ++i) {
                        const float2 sv = zg[pad(k0 + i)];
                        const float s = sig ? sv.y : sv.x;
                        acc = fmaf(wsrc[i * wstep], s * s, acc);
                    }
                    const float d = 10.0f * log10f(fmaxf(1e-10f, acc));
                    db[f * kDbStride + mel] = d;
                    dmax = fmaxf(dmax, d);
                }
            }
            __syncthreads();                                                      // z and the group areas are free for the next pairs
        }

        // ---- cepstrum
        WM_CF_STAMP(3);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dmax = fmaxf(dmax, __shfl_xor(dmax, o));
        if (lane == 0) bred[wave * 4] = dmax;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kWaves; ++i) dmax = fmaxf(dmax, bred[i * 4]);
        const float floor_db = dmax - 80.0f;
        float* mf = reinterpret_cast<float*>(z);                                  // [kMfcc][kFs]
        for (int o = tid; o < kMfcc * F; o += kThreads) {
            const int cc = o % kMfcc, f = o / kMfcc;
            float acc = 0.f;
            for (int k = 0; k < kMels; ++k) acc = fmaf(a.dct[cc * kMels + k], fmaxf(db[f * kDbStride + k], floor_db), acc);
            mf[cc * kFs + f] = acc;
        }
        __syncthreads();
        if (tid < kMfcc) {
            const float first = mf[tid * kFs];                                     // moments of the distance from the first frame: a clip
            float s = 0.f;                                                        // whose frames are all alike has a variance of exactly 0
            for (int f = 0; f < F; ++f) s += mf[tid * kFs + f] - first;
            const float mu = s / (float)F;
            float q = 0.f;
            for (int f = 0; f < F; ++f) {
                const float d = (mf[tid * kFs + f] - first) - mu;
                q = fmaf(d, d, q);
            }
            mstat[tid] = first + mu;
            mstat[16 + tid] = q / (float)F;
        }
        __syncthreads();

        // ---- the row
        const float nanv = __builtin_nanf("");
        if (a.frames && tid < F) {
            float* fo = a.frames + (r * F + tid) * 4;
            fo[0] = bad ? nanv : fcen[tid];
            fo[1] = bad ? nanv : fbw[tid];
            fo[2] = bad ? nanv : fro[tid];
            fo[3] = bad ? nanv : (float)fzc[tid];
        }
        if (tid == 0) {
            const float energy = rstat[0], m2 = rstat[1], m4 = rstat[2], estd = rstat[3], sbe = rstat[4];
            float sc = 0.f, sb = 0.f, sr = 0.f, mm = 0.f, mv = 0.f;
            int zc = 0;
            for (int f = 0; f < F; ++f) { sc += fcen[f]; sb += fbw[f]; sr += fro[f]; zc += fzc[f]; }
            for (int i = 0; i < kMfcc; ++i) { mm += mstat[i]; mv += mstat[16 + i]; }
            const float zcr = (float)zc / ((float)F * (float)kN);
            const float cen = sc / (float)F, bw = sb / (float)F, ro = sr / (float)F * hz;
            const float kurt = m4 / (m2 * m2) - 3.0f;
            const float ratio = sbe / (energy + 1e-10f);
            int score = (sbe > 0.001f) + (zcr < 0.1f) + (cen < 3000.0f) + (kurt > 5.0f) + (estd > 0.01f) + 2 * (ratio > 0.6f);
            float o[kFeat] = {(float)n / (float)a.sr, energy, sbe, zcr, cen, bw, ro, mm / (float)kMfcc, mv / (float)kMfcc, kurt, estd, ratio,
                              sqrtf(energy), 0.f, 0.f, 0.f};
            if (bad) {
#pragma unroll
                for (int i = 0; i < 13; ++i) o[i] = nanv;
                zc = 0;
                score = 0;
            }
#ifdef WM_CLIP_FEATURES_STAMPS
            for (int i = 0; i < 3; ++i) o[13 + i] = (float)(stamp[i + 1] - stamp[i]);
#endif
            float* fr = a.feat + r * kFeat;
#pragma unroll
            for (int i = 0; i < kFeat; ++i) fr[i] = o[i];
            int* cr = a.counts + r * kCounts;
            cr[0] = zc; cr[1] = score; cr[2] = bad ? 1 : 0; cr[3] = bad ? -1 : (score >= 4 ? 1 : 0);
        }
    }
}

// the launch's shape from (rows, n, sample_rate); false where they are out of range
bool plan(long long rows, long long n, int sr, Args& a, size_t& lds) {
    if (rows < 1 || rows > (1ll << 40) || n < kMinN || n > kMaxN || sr <= 6000 || sr > (1 << 20)) return false;
    const int L = (int)((double)sr * 0.025), H = (int)((double)sr * 0.010);
    if (L < 1 || H < 1 || L > n) return false;
    a.rows = rows; a.n = (int)n; a.sr = sr;
    a.F = 1 + (int)n / kHop;
    a.L = L; a.H = H; a.NF = 1 + ((int)n - L) / H;
    a.stage = n <= kStageMax ? (((int)n + 3) & ~3) : 0;
    if (a.NF > kGroups * 2 * kN) return false;                                    // the frame energies borrow the transform's workspace
    lds = lds_bytes(a.stage, a.F);
    return true;
}

wm::DevOnce g_once;

}  // namespace

extern "C" {

int wm_clip_features_plan(long long rows, long long n, int sample_rate, int* frames, int* energy_frames, int* lds_bytes, hipStream_t) {
    Args a;
    size_t lds = 0;
    if (!frames || !energy_frames || !lds_bytes || !plan(rows, n, sample_rate, a, lds)) return (int)hipErrorInvalidValue;
    *frames = a.F; *energy_frames = a.NF; *lds_bytes = (int)lds;
    return 0;
}

int wm_clip_features(const float* x, const float* sos, const float* fb, const int* klo, const int* khi, const float* dct, float* feat,
                     int* counts, float* frames_out, long long rows, long long n, int sample_rate, int warm, hipStream_t stream) {
    Args a;
    size_t lds = 0;
    if (!plan(rows, n, sample_rate, a, lds)) return (int)hipErrorInvalidValue;
    if (!x || !sos || !fb || !klo || !khi || !dct || !feat || !counts || warm < 0 || warm > kMaxN) return (int)hipErrorInvalidValue;
    const void* ptrs[9] = {x, sos, fb, klo, khi, dct, feat, counts, frames_out};
    for (const void* p : ptrs)
        if ((uintptr_t)p % 4) return (int)hipErrorInvalidValue;
    const unsigned long long urows = (unsigned long long)rows;
    const void* ins[6] = {x, sos, fb, klo, khi, dct};
    const unsigned long long ins_bytes[6] = {urows * (unsigned long long)n * 4, kSections * 6 * 4, (unsigned long long)(kN / 2 + 1) * kMels * 4,
                                             kMels * 4, kMels * 4, kMfcc * kMels * 4};
    const void* outs[3] = {feat, counts, frames_out};
    const unsigned long long outs_bytes[3] = {urows * kFeat * 4, urows * kCounts * 4, urows * (unsigned long long)a.F * 16};
    for (int i = 0; i < 3; ++i) {                                                 // what is written overlaps neither an input nor another output
        if (!outs[i]) continue;
        for (int k = 0; k < 6; ++k)
            if (overlap(ins[k], ins_bytes[k], outs[i], outs_bytes[i])) return (int)hipErrorInvalidValue;
        for (int k = i + 1; k < 3; ++k)
            if (outs[k] && overlap(outs[i], outs_bytes[i], outs[k], outs_bytes[k])) return (int)hipErrorInvalidValue;
    }
    a.x = x; a.sos = sos; a.fb = fb; a.klo = klo; a.khi = khi; a.dct = dct; a.feat = feat; a.counts = counts; a.frames = frames_out;
    a.warm = warm;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(clip_features_kernel), kLdsMax, g_once)) return rc;
    const unsigned grid = (unsigned)(rows < kNumCU * 4 ? rows : kNumCU * 4);
    hipLaunchKernelGGL(clip_features_kernel, dim3(grid), dim3(kThreads), lds, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
