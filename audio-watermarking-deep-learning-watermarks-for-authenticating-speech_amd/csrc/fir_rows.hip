// Per-row causal FIR convolution along the last axis of rows x n fp32 data, and its adjoint: the long convolutive channel (a room, a
// loudspeaker-microphone path, an echo) as a step of the graph.  The definition is the comment of wm_fir_rows in include/wm_hip.h; this
// file is how it is computed.
//
// Blocks.  Cut the row into blocks of 32 samples, t = 32 T + j.  H is lower-triangular Toeplitz, and so is every 32 x 32 block of it:
//     y[32 T + j] = sum_{d >= 0} sum_{m < 32} h[32 d + j - m] x[32 (T - d) + m]          (h[k] = 0 outside [0, K), x = 0 outside [0, n))
// d = 0 is the triangle on the diagonal, d = D - 1 = floor((K + 30) / 32) the last block that holds a tap: D blocks, all dense but the two
// ends.  For 32 output blocks T at once this is a (32 blocks x 32 m) panel of x times a (32 m x 32 j) Toeplitz block of taps, on
// v_mfma_f32_32x32x2_f32: exact fp32 products, bitwise a fmaf chain over d ascending, m ascending inside -- one fixed order per sample, a
// function of j = t mod 32 alone.  Padding terms are exact zeros (0 * finite adds nothing), so neither the column a block sits in nor the
// workgroup that owns it reaches the bits.
//
// Launch.  A workgroup of 256 lanes (4 waves) owns 128 NT consecutive blocks of one row (NT = 1 or 2: wave w the NT groups of 32 blocks
// from 32 NT w on) and all D lag blocks for them: no atomics, no scratch, one writer per sample.  It keeps in LDS
//     hs[q] = h[q - 31], q < 32 D + 31        read at 32 d + 31 + j - m: 32 lanes on consecutive words, no bank conflict
//     xs[b][m], b < 128 NT + D - 1            the owned blocks and the D - 1 before them, 33 words per block: the 32 lanes of a panel read
//                                             32 blocks at one m, stride 33, no bank conflict
// both filled by predicate (outside the row, or outside the taps: zero; a neighbouring row is never read).  One read of hs feeds NT
// MFMAs.  Lag blocks whose whole panel lies before the row start (d > the wave's last block) are skipped.  The accumulators leave
// straight from registers: a register holds one block's sample j per lane, 32 lanes on 128 consecutive bytes.
// reverse: the loader and the store mirror the index (t -> n - 1 - t), so the adjoint is flip(H flip(x)) with the forward's bits.
// NT = 2 where its LDS stays within 64 KB (three workgroups a CU at K = 2048), else NT = 1: K = 16384 needs 147 KB, one workgroup a CU.
#include "wm_common.hpp"
using namespace wm;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kPad = 33;                        // words per block of 32 samples in LDS
constexpr int kMaxTaps = 16384;

struct Args {
    const float* x; const float* h; float* y;
    long long rows, n, h_stride, wpr, tiles;    // wpr workgroups per row
    int K, D, reverse;
};

constexpr int hs_floats(int D) { return 32 * D + 32; }                           // 32 D + 31 used
constexpr size_t lds_bytes(int D, int NT) { return (size_t)(hs_floats(D) + (32 * NT * kWaves + D - 1) * kPad) * sizeof(float); }
int lag_blocks(int K) { return (K + 30) / 32 + 1; }

template <int NT>
__global__ __launch_bounds__(kThreads) void fir_rows_kernel(Args a) {
    constexpr int kCols = 32 * NT * kWaves;     // blocks a workgroup owns
    extern __shared__ __align__(16) float smem[];
    const int D = a.D, NB = kCols + D - 1;
    float* hs = smem;
    float* xs = smem + hs_floats(D);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, half = lane >> 5;
    const long long nblk = (a.n + 31) / 32;
    for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long long r = tile / a.wpr;
        const long long T0 = (tile - r * a.wpr) * kCols;             // the first block owned
        const float* __restrict__ xr = a.x + r * a.n;
        const float* __restrict__ hr = a.h + r * a.h_stride;
        __syncthreads();                                             // the tile before has left LDS
        for (int q = tid; q < 32 * D + 31; q += kThreads) {
            const int k = q - 31;
            hs[q] = (k >= 0 && k < a.K) ? hr[k] : 0.f;
        }
        const long long p0 = 32 * (T0 - (D - 1));                    // the sample xs[0][0] stands for
        for (int e = tid; e < NB * 32; e += kThreads) {
            const long long p = p0 + e;
            xs[(e >> 5) * kPad + (e & 31)] = (p >= 0 && p < a.n) ? xr[a.reverse ? a.n - 1 - p : p] : 0.f;
        }
        __syncthreads();
        const long long Tw = T0 + 32 * NT * wave;                    // this wave's first block
        if (Tw >= nblk) continue;                                    // wave-uniform; the barriers above are passed by every wave
        f32x16 acc[NT];
#pragma unroll
        for (int c = 0; c < NT; ++c)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[c][i] = 0.f;
        // lag blocks with d > T hold only samples before the row start for block T: stop at the wave's last block
        const long long last = Tw + 32 * NT - 1;
        const int dend = last < D - 1 ? (int)last : D - 1;
        const float* pa = hs + 31 + j - half;                                     // + 32 d - m0
        const float* pb = xs + (32 * NT * wave + j + D - 1) * kPad + half;        // block Tw + j at lag 0; - 33 d, + m0
        for (int d = 0; d <= dend; ++d) {
            const float* qa = pa + 32 * d;
            const float* qb = pb - kPad * d;
#pragma unroll
            for (int m0 = 0; m0 < 32; m0 += 2) {
                const float hv = qa[-m0];
#pragma unroll
                for (int c = 0; c < NT; ++c) acc[c] = mfma32(qb[c * 32 * kPad + m0], hv, acc[c]);
            }
        }
        float* __restrict__ yr = a.y + r * a.n;
#pragma unroll
        for (int c = 0; c < NT; ++c)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const long long t = 32 * (Tw + 32 * c + mfma_row(i, half)) + j;
                if (t < a.n) yr[a.reverse ? a.n - 1 - t : t] = acc[c][i];
            }
    }
}

template <int NT>
int launch(Args& a, hipStream_t stream) {
    static DevOnce done;
    const size_t lds = lds_bytes(a.D, NT);
    if (lds > 64 * 1024 && !dev_done(done)) {
        WM_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(fir_rows_kernel<NT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds_bytes(lag_blocks(kMaxTaps), NT)));
        dev_mark(done);
    }
    const long long nblk = (a.n + 31) / 32, cols = 32 * NT * kWaves;
    a.wpr = (nblk + cols - 1) / cols;
    a.tiles = a.rows * a.wpr;
    const long long cap = 1ll << 20;
    hipLaunchKernelGGL(fir_rows_kernel<NT>, dim3((unsigned)(a.tiles < cap ? a.tiles : cap)), dim3(kThreads), lds, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" {

int wm_fir_rows(const float* x, const float* h, float* y, long long rows, long long n, int K, long long h_stride, int reverse,
                hipStream_t stream) {
    if (rows < 1 || n < 1 || n > (1ll << 34) || rows > (1ll << 46) / n || K < 1 || K > kMaxTaps) return (int)hipErrorInvalidValue;
    if (h_stride != 0 && (h_stride < K || h_stride > (1ll << 46) / rows)) return (int)hipErrorInvalidValue;
    if (!x || !h || !y || (uintptr_t)x % 4 || (uintptr_t)h % 4 || (uintptr_t)y % 4) return (int)hipErrorInvalidValue;
    const unsigned long long bytes = (unsigned long long)rows * (unsigned long long)n * 4;
    const unsigned long long hbytes = ((unsigned long long)(rows - 1) * (unsigned long long)h_stride + (unsigned long long)K) * 4;
    if (overlap(x, bytes, y, bytes) || overlap(h, hbytes, y, bytes)) return (int)hipErrorInvalidValue;   // in place is refused
    Args a;
    a.x = x; a.h = h; a.y = y; a.rows = rows; a.n = n; a.h_stride = h_stride; a.wpr = a.tiles = 0;
    a.K = K; a.D = lag_blocks(K); a.reverse = reverse != 0;
    return lds_bytes(a.D, 2) <= 64 * 1024 ? launch<2>(a, stream) : launch<1>(a, stream);
}

}  // extern "C"
