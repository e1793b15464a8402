// Transform-codec stand-in along the last axis of rows x n fp32 data: lapped MDCT analysis, a per-band uniform quantiser whose step follows
// the band's own energy, an optional bandwidth cut, MDCT synthesis with overlap-add -- the signal path lossy codecs share, as a step of the
// graph.  It is NOT an MP3 or AAC encoder and parity with one is unmeasured.  The definition is the comment of wm_mdct_codec in
// include/wm_hip.h; this file is how it is computed.
//
// Fold.  With z = w . x_f cut into quarters (a, b, c, d) the MDCT of a frame is the DCT-IV of the M folded samples
//     u[i] = -z[3M/2 - 1 - i] - z[3M/2 + i]   (i < M/2)        u[i] = z[i - M/2] - z[3M/2 - 1 - i]   (i >= M/2)
//     X[k] = sum_i u[i] cos(pi/M (i + 1/2)(k + 1/2))
// and synthesis is the transpose: v = DCT-IV(Xq) (the matrix is symmetric), t[j] = v[j + M/2] (j < M/2), -v[3M/2 - 1 - j] (M/2 <= j < 3M/2),
// -v[j - 3M/2] (j >= 3M/2), y_f[j] = (2/M) w[j] t[j].  Both transforms are therefore ONE M x M product per frame.
//
// Launch.  A workgroup of 256 lanes (4 waves) takes W = 32 or 64 consecutive frames f0 .. f0 + W - 1 of one row and owns the W - 1 hops of
// output between them (hop b = second half of frame b + first half of frame b + 1), so neighbouring workgroups share one frame and each
// computes it: no atomics, no scratch, one writer per sample.  The frames are folded from global memory straight into LDS as U[i][frame]
// (a hop is read by the two frames that hold it: the second read is a cache hit), the DCT-IV runs on the fp32 matrix cores,
// v_mfma_f32_32x32x2_f32 with A = 32 rows k of the cosine matrix, B = 32 frames of U: wave w accumulates the k-tiles w M/128 ..
// (w + 1) M/128 - 1 over i in ascending pairs -- one fixed order per coefficient, whatever the frame's column and whatever W, so the shared
// frame has the same bits on both sides and the host is free to pick W per shape (wm_mdct_codec_plan: the fewest padded frames).  The
// cosines come from an LDS table of the 2M values cos(pi (2i + 1) / (4M)) (cospif of an exact argument, built by each workgroup):
// (2i + 1)(2k + 1) is odd, so the entry is table[((2i + 1)(2k + 1) mod 4M) >> 1], negated in the second half period; 32 lanes with
// consecutive k read it at an odd stride: no bank conflict.  The window is the same table (w[j] = table[M - 1 - j], w[M + j] = table[j]).
// The spectrum goes back to the same LDS buffer, one lane quantises one (frame, band) in place, the second product follows, and the hops
// leave as 4-byte stores, consecutive lanes on consecutive samples.  The spectrum never reaches HBM; the int16 codes do where asked for.
#include <cmath>
#include "wm_common.hpp"
using namespace wm;

namespace {

constexpr int kThreads = 256;
// A workgroup transforms 32 NT consecutive frames (NT column tiles of the 32x32x2 MFMA, NT = 1 or 2) and owns the 32 NT - 1 hops between
// them; an LDS row holds 32 NT + 1 floats, so that lanes on consecutive rows fall on consecutive banks.  NT is the host's choice per shape
// (fewest padded frames); a coefficient's sum does not know its column, so the choice does not reach the bits.

struct Args {
    const float* x; float* y; short* codes; const short* mask; const float* snr_db;
    long long rows, n, F, wpr, tiles;           // F frames per row, wpr workgroups per row
    int band, kcut, quantise;
    float floor_step;
};

constexpr size_t lds_bytes(int M, int NT) { return (size_t)(M * (32 * NT + 1) + 2 * M) * sizeof(float); }

// cos(pi j / (4M)) for an odd j >= 0 from the table of the first half period
template <int M>
__device__ __forceinline__ float cos_odd(const float* __restrict__ tab, int j) {
    const float t = tab[(j & (4 * M - 1)) >> 1];
    return (j & (4 * M)) ? -t : t;
}

// acc[i][c] (rows k0_i + mfma_row(r, lane >> 5), column 32 c + (lane & 31)) = sum_{n < nend} cos(pi/M (n + 1/2)(k + 1/2)) buf[n][column], n
// ascending.  One table read feeds NT MFMAs, one read of buf M / 128 of them.
template <int M, int NT>
__device__ __forceinline__ void dct4(const float* __restrict__ tab, const float* __restrict__ buf, int nend, f32x16 (&acc)[M / 128][NT]) {
    constexpr int KT = M / 128, kPad = 32 * NT + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, half = lane >> 5;
    int idx[KT], inc[KT];
#pragma unroll
    for (int i = 0; i < KT; ++i) {
        const int k = 32 * (wave * KT + i) + col;
        idx[i] = (2 * k + 1) * (2 * half + 1);
        inc[i] = 4 * (2 * k + 1);
#pragma unroll
        for (int c = 0; c < NT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][c][r] = 0.f;
    }
    const float* b = buf + half * kPad + col;
    for (int n0 = 0; n0 < nend; n0 += 4) {                           // nend is a multiple of 4 (M, or kcut: a multiple of band)
#pragma unroll
        for (int h = 0; h < 4; h += 2) {
            float bv[NT];
#pragma unroll
            for (int c = 0; c < NT; ++c) bv[c] = b[(n0 + h) * kPad + 32 * c];
#pragma unroll
            for (int i = 0; i < KT; ++i) {
                const float av = cos_odd<M>(tab, idx[i]);
#pragma unroll
                for (int c = 0; c < NT; ++c) acc[i][c] = mfma32(av, bv[c], acc[i][c]);
                idx[i] += inc[i];
            }
        }
    }
}

template <int M, int NT>
__device__ __forceinline__ void store_tiles(float* __restrict__ buf, const f32x16 (&acc)[M / 128][NT]) {
    constexpr int KT = M / 128, kPad = 32 * NT + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, half = lane >> 5;
#pragma unroll
    for (int i = 0; i < KT; ++i)
#pragma unroll
        for (int c = 0; c < NT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) buf[(32 * (wave * KT + i) + mfma_row(r, half)) * kPad + 32 * c + col] = acc[i][c][r];
}

template <int M, int NT>
__global__ __launch_bounds__(kThreads) void mdct_codec_kernel(Args a) {
    constexpr int kFrames = 32 * NT, kOwn = kFrames - 1, kPad = kFrames + 1;
    extern __shared__ __align__(16) float smem[];
    float* buf = smem;                          // [M][kPad]: U, then X / Xq, then v
    float* tab = smem + M * kPad;               // [2M]: cos(pi (2i + 1) / (4M))
    const int tid = threadIdx.x;
    for (int i = tid; i < 2 * M; i += kThreads) tab[i] = cospif((float)(2 * i + 1) * (1.f / (4 * M)));   // the argument is exact
    for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long r = tile / a.wpr;
        const long long f0 = (tile - r * a.wpr) * kOwn;              // the first frame, and the first hop owned
        const float* __restrict__ xr = a.x + r * a.n;
        __syncthreads();                                             // the table is there; the tile before has left buf
        for (int e = tid; e < kFrames * M; e += kThreads) {
            const int f = e / M, i = e % M;
            float u = 0.f;
            if (f0 + f < a.F) {
                const long long s0 = (f0 + f - 1) * M;               // frame f holds samples s0 .. s0 + 2M - 1
                const int j1 = i < M / 2 ? 3 * M / 2 - 1 - i : i - M / 2, j2 = i < M / 2 ? 3 * M / 2 + i : 3 * M / 2 - 1 - i;
                const long long t1 = s0 + j1, t2 = s0 + j2;
                const int w1 = 2 * M - 2 * j1 - 1, w2 = 2 * M - 2 * j2 - 1;          // w[j] = cos(pi (2M - 2j - 1) / (4M)), cos is even
                const float z1 = (t1 >= 0 && t1 < a.n) ? tab[(w1 < 0 ? -w1 : w1) >> 1] * xr[t1] : 0.f;
                const float z2 = (t2 >= 0 && t2 < a.n) ? tab[(w2 < 0 ? -w2 : w2) >> 1] * xr[t2] : 0.f;
                u = i < M / 2 ? -z1 - z2 : z1 - z2;
            }
            buf[i * kPad + f] = u;
        }
        __syncthreads();
        f32x16 acc[M / 128][NT];
        dct4<M, NT>(tab, buf, M, acc);
        __syncthreads();                                             // every wave has read all of U
        store_tiles<M, NT>(buf, acc);
        __syncthreads();
        // cut, mask and quantise in place: one lane per (frame, band); a frame past the row's last is all zeros already
        float scale = 0.f;
        if (a.quantise) scale = exp10f(__fdiv_rn(-fminf(fmaxf(a.snr_db[r], 0.f), 60.f), 20.f));
        const int bands = M / a.band;
        for (int t = tid; t < kFrames * bands; t += kThreads) {
            const int f = t % kFrames, k0 = (t / kFrames) * a.band;
            const long long gf = f0 + f;
            if (gf >= a.F) continue;
            float* p = buf + k0 * kPad + f;
            const long long cbase = (r * a.F + gf) * M + k0;
            const bool writes = a.codes && (f < kOwn || gf == a.F - 1);             // the shared frame is written by the tile it starts
            if (k0 >= a.kcut) {
                for (int i = 0; i < a.band; ++i) {
                    p[i * kPad] = 0.f;
                    if (writes) a.codes[cbase + i] = 0;
                }
                continue;
            }
            float ss = 0.f;
            for (int i = 0; i < a.band; ++i) {
                float v = p[i * kPad];
                if (a.mask && a.mask[cbase + i] == 0) p[i * kPad] = v = 0.f;
                ss = fmaf(v, v, ss);
            }
            if (!a.quantise) continue;
            const float step = fmaxf(__fsqrt_rn(12.f * __fdiv_rn(ss, (float)a.band)) * scale, a.floor_step);
            for (int i = 0; i < a.band; ++i) {
                const float q = rintf(__fdiv_rn(p[i * kPad], step));
                p[i * kPad] = q * step;
                if (writes) a.codes[cbase + i] = (short)q;
            }
        }
        __syncthreads();
        dct4<M, NT>(tab, buf, a.kcut, acc);                          // the rows from kcut on are zero
        __syncthreads();
        store_tiles<M, NT>(buf, acc);
        __syncthreads();
        float* __restrict__ yr = a.y + r * a.n;
        for (int e = tid; e < kOwn * M; e += kThreads) {
            const int g = e / M, j = e % M;
            const long long t = (f0 + g) * M + j;
            if (t >= a.n) continue;
            // hop g: t[M + j] of frame g and t[j] of frame g + 1
            const float ta = j < M / 2 ? -buf[(M / 2 - 1 - j) * kPad + g] : -buf[(j - M / 2) * kPad + g];
            const float tb = j < M / 2 ? buf[(j + M / 2) * kPad + g + 1] : -buf[(3 * M / 2 - 1 - j) * kPad + g + 1];
            yr[t] = (2.f / M) * fmaf(tab[j], ta, tab[M - 1 - j] * tb);
        }
    }
}

long long tiles_per_row(long long nb, int NT) { return (nb + 32 * NT - 2) / (32 * NT - 1); }

// 64 frames per workgroup where that leaves no more padded frames than 32 do (M = 512 stays at 32: two of its 64-frame buffers do not
// fit the LDS of a CU side by side)
int column_tiles(long long nb, int M) { return M <= 256 && 64 * tiles_per_row(nb, 2) <= 32 * tiles_per_row(nb, 1) ? 2 : 1; }

template <int M, int NT>
int launch(Args& a, long long nb, hipStream_t stream) {
    static DevOnce done;
    if (lds_bytes(M, NT) > 64 * 1024 && !dev_done(done)) {
        WM_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(mdct_codec_kernel<M, NT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds_bytes(M, NT)));
        dev_mark(done);
    }
    a.wpr = tiles_per_row(nb, NT);
    a.tiles = a.rows * a.wpr;
    const long long cap = 1ll << 20;
    hipLaunchKernelGGL((mdct_codec_kernel<M, NT>), dim3((unsigned)(a.tiles < cap ? a.tiles : cap)), dim3(kThreads), lds_bytes(M, NT), stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" {

// host-only query: the frames a workgroup transforms (32 or 64) and the workgroups per row for this shape
int wm_mdct_codec_plan(long long n, int M, int* frames_per_workgroup, long long* workgroups_per_row, hipStream_t) {
    if (n < 1 || n > (1ll << 34) || (M != 128 && M != 256 && M != 512) || !frames_per_workgroup || !workgroups_per_row)
        return (int)hipErrorInvalidValue;
    const long long nb = (n + M - 1) / M;
    const int NT = column_tiles(nb, M);
    *frames_per_workgroup = 32 * NT;
    *workgroups_per_row = tiles_per_row(nb, NT);
    return 0;
}

int wm_mdct_codec(const float* x, float* y, void* codes_out, const void* mask_in, const float* snr_db, long long rows,
                             long long n, int M, int band, int kcut, float floor_step, int quantise, hipStream_t stream) {
    if (rows < 1 || n < 1 || n > (1ll << 34) || rows > (1ll << 46) / n) return (int)hipErrorInvalidValue;
    if (M != 128 && M != 256 && M != 512) return (int)hipErrorInvalidValue;
    if (band != 4 && band != 8 && band != 16 && band != 32) return (int)hipErrorInvalidValue;
    if (kcut < band || kcut > M || kcut % band) return (int)hipErrorInvalidValue;
    if (!std::isfinite(floor_step) || !(floor_step > 0.f)) return (int)hipErrorInvalidValue;
    if (!x || !y || !snr_db || (uintptr_t)x % 4 || (uintptr_t)y % 4 || (uintptr_t)snr_db % 4) return (int)hipErrorInvalidValue;
    if ((uintptr_t)codes_out % 2 || (uintptr_t)mask_in % 2) return (int)hipErrorInvalidValue;
    if (codes_out && !quantise) return (int)hipErrorInvalidValue;                 // there are no codes without the quantiser
    const long long nb = (n + M - 1) / M, F = nb + 1;
    const unsigned long long bytes = (unsigned long long)rows * (unsigned long long)n * 4;
    const unsigned long long cbytes = (unsigned long long)rows * (unsigned long long)F * (unsigned long long)M * 2;
    if (overlap(x, bytes, y, bytes)) return (int)hipErrorInvalidValue;            // in place is refused
    if (codes_out && (overlap(codes_out, cbytes, x, bytes) || overlap(codes_out, cbytes, y, bytes) ||
                      overlap(codes_out, cbytes, snr_db, (unsigned long long)rows * 4)))
        return (int)hipErrorInvalidValue;
    if (mask_in && (overlap(mask_in, cbytes, y, bytes) || (codes_out && overlap(mask_in, cbytes, codes_out, cbytes))))
        return (int)hipErrorInvalidValue;
    if (overlap(snr_db, (unsigned long long)rows * 4, y, bytes)) return (int)hipErrorInvalidValue;
    Args a;
    a.x = x; a.y = y; a.codes = static_cast<short*>(codes_out); a.mask = static_cast<const short*>(mask_in); a.snr_db = snr_db;
    a.rows = rows; a.n = n; a.F = F; a.wpr = a.tiles = 0;
    a.band = band; a.kcut = kcut; a.quantise = quantise != 0; a.floor_step = floor_step;
    const bool wide = column_tiles(nb, M) == 2;
    switch (M) {
        case 128: return wide ? launch<128, 2>(a, nb, stream) : launch<128, 1>(a, nb, stream);
        case 256: return wide ? launch<256, 2>(a, nb, stream) : launch<256, 1>(a, nb, stream);
        default: return launch<512, 1>(a, nb, stream);
    }
}

}  // extern "C"
