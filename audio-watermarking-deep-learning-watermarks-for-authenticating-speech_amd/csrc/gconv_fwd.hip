// Generic-shape convolution family for the main14b_2 deep-residual variant (py/main14b_2.py:83-224, BASELINE config 5):
// strided Conv1d(k3, stride 2/4/5/8), 1x1 strided skip convs, nn.Linear, Conv1d(k7), and ConvTranspose1d(k=2*st,
// stride st, padding st/2) for channel counts 1..512 -- one implicit-GEMM kernel on the fp32 matrix cores:
//     acc[m][n] = sum_{ci,k} wp[ci*K + k][m] * x[nb][ci][n*S + k - P]
// with M = output rows (channels, or channel*phase for the transposed convolutions), N = output positions, and a
// K-dimension of (input channel, tap) pairs streamed through LDS 8 channels at a time.
//   * A transposed convolution with stride st and kernel 2*st is a 2-tap stride-1 convolution onto Cout*st "phase
//     channels" followed by a pixel shuffle (t' = n*st + phase - padding); the shuffle is applied in the store.
//   * Data gradients reuse the kernel with re-packed weights (dgrad of a strided conv = transposed conv and vice
//     versa); the packing itself is pure data movement done by the host mirror.
// Epilogue: + bias[channel] + vec[nb][channel] (message embedding) + residual, then optional ELU (alpha = 1).
// The family's other units: gconv_wgrad.hip (weight gradients), gconv_small.hip (ELU backward, bias and
// embedding gradients), lstm_seq.hip (the variant's LSTM).
#include "wm_common.hpp"
#include <type_traits>
using namespace wm;

namespace {

struct GConvArgs {
    const float* x;      // [NB][Cin][Lin]
    const float* wp;     // [Cin*K][Mtot]
    const float* bias;   // [Cout] or null
    const float* vec;    // [NB][Cout] or null
    const float* res;    // same layout as y, or null
    float* y;            // [NB][Cout][Lout]
    int NB, Cin, Lin, K, S, P, Mtot, Nout;
    int st;              // 1: plain (Cout == Mtot, t' = n); >1: pixel shuffle, row m = co*st + phase
    int shp;             // padding of the transposed convolution (t' = n*st + phase - shp)
    int Cout, Lout;
    int act;             // 0 none | 1 ELU | 2 multiply by ELU'(aux): aux = `res` holds y = ELU(z) of the tensor the result is a gradient of
    int CI;              // input channels per LDS chunk (even; CI*K <= KR_MAX; CI*XW <= 256*xr_of(BN))
    int XW;              // input span of one N tile: (BN-1)*S + K
    const float* x2;     // optional second source: input channels >= Cin1 are rows of x2 [NB][Cin - Cin1][Lin] (two gradients
    int Cin1;            //   contracted by one launch: a strided conv and its 1x1 skip conv); Cin1 % CI == 0
    int nph;             // phases per output channel when st > 1: row m = co*nph + phase, phase < nph <= st
};

// (channel, tap) rows of the weight image per chunk: sized so that three workgroups' double buffers fit the 160 KB of LDS
constexpr int kr_max_of(int bm) { return bm >= 128 ? 36 : 48; }
constexpr int xr_of(int bn) { return bn >= 256 ? 16 : 10; }   // input-tile elements a thread stages per chunk, by tile width

// Implicit-GEMM tile kernel.  Workgroup = 4 waves as MW x (4/MW); a wave owns WM x WN blocks of 32 x 32 (fp32 MFMA
// 32x32x2, the two k of an instruction = the two channels of a pair at one tap).  Per chunk of CI input channels the
// workgroup stages the input rows [CI][XW] (dword loads, coalesced along time, any alignment) and the weight rows
// [(pair, tap, parity)][BM] (float4 loads when Mtot % 4 == 0) through REGISTERS into the other LDS buffer while the
// matrix cores work on the current one: one barrier per chunk.  Staging costs no address arithmetic inside the loop: every
// element's 32-bit offset is formed once, the chunk advances two wave-uniform base pointers, LDS stores are unconditional
// (the regions are padded to whole 256-thread passes) and zero padding is applied only by the tiles that touch a clip edge.
template <int MW, int WM, int WN, bool VECW>
__global__ __launch_bounds__(256, 3) void gconv2_kernel(GConvArgs a) {
    constexpr int NWN = 4 / MW, BM = MW * WM * 32, BN = NWN * WN * 32, XR = xr_of(BN), KR_MAX = kr_max_of(BM);
    constexpr int WPT = VECW ? (KR_MAX * BM / 4 + 255) / 256 : (KR_MAX * BM + 255) / 256;   // weight pieces per thread
    constexpr int WV = VECW ? 4 : 1;
    extern __shared__ __align__(16) float smem[];
    const int K = a.K, S = a.S, CI = a.CI, XW = a.XW, KR = CI * K;
    const int xsz = CI * XW;
    const int nx = (xsz + 255) >> 8, xreg = nx * 256;                       // padded regions: whole passes of 256 threads
    const int nwp = (KR * BM / WV + 255) >> 8, wreg = nwp * 256 * WV;
    const int bufsz = xreg + wreg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int wm_ = wave % MW, wn = wave / MW;
    const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM, nb = blockIdx.z;
    const int u0 = n0 * S - a.P;
    const bool edge_tile = (u0 < 0) || (u0 + XW > a.Lin);                   // wave-uniform

    // ---- chunk-invariant staging maps
    unsigned xo[XR];            // ci * Lin + clamped column
    unsigned xz = 0;            // bit i: element i is zero padding (outside the clip)
#pragma unroll
    for (int i = 0; i < XR; ++i) {
        const int idx = tid + 256 * i;
        const int ci = min(idx / XW, CI - 1), j = idx - (idx / XW) * XW, u = u0 + j;
        xz |= ((u < 0 || u >= a.Lin) ? 1u : 0u) << i;
        xo[i] = (unsigned)(ci * a.Lin + min(max(u, 0), a.Lin - 1));
    }
    unsigned wo[WPT];           // row * Mtot + m0 + column of the chunk's weight slab (0 for pieces outside it)
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
        const int idx = tid + 256 * i;
        int r, c;
        if (VECW) { r = idx / (BM / 4); c = (idx - r * (BM / 4)) * 4; } else { r = idx / BM; c = idx - r * BM; }
        const int pr = r >> 1, q = pr / K, tap = pr - q * K, ci = 2 * q + (r & 1);
        const bool ok = (r < KR) && (m0 + c < a.Mtot);
        wo[i] = ok ? (unsigned)((ci * K + tap) * a.Mtot + m0 + c) : 0u;
    }

    f32x16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float xr[XR];
    f32x4 wr4[VECW ? WPT : 1];
    float wr1[VECW ? 1 : WPT];
    // buffer loads: per-lane 32-bit byte offsets (xo / wo, formed once) + a wave-uniform chunk offset; no 64-bit address
    // registers, no vector-ALU address arithmetic
    const int cin1 = a.x2 ? a.Cin1 : a.Cin;
    const wm_srd_t sx = make_srd(a.x + (size_t)nb * cin1 * a.Lin, (size_t)cin1 * a.Lin * sizeof(float));
    const wm_srd_t sx2 = make_srd(a.x2 ? a.x2 + (size_t)nb * (a.Cin - cin1) * a.Lin : a.x, (size_t)(a.Cin - cin1) * a.Lin * sizeof(float));
    const wm_srd_t sw = make_srd(a.wp, (size_t)a.Cin * K * a.Mtot * sizeof(float));
#pragma unroll
    for (int i = 0; i < XR; ++i) xo[i] *= 4u;
#pragma unroll
    for (int i = 0; i < WPT; ++i) wo[i] *= 4u;

    auto load_chunk = [&](int c0) {
        const int crem = a.Cin - c0;
        const bool second = c0 >= cin1;                      // wave-uniform: the chunk lies in the second source
        const wm_srd_t sxc = second ? sx2 : sx;
        const unsigned xs0 = (unsigned)((c0 - (second ? cin1 : 0)) * a.Lin) * 4u, ws0 = (unsigned)(c0 * K * a.Mtot) * 4u;
        if (crem >= CI) {                                    // full chunk: offsets only
#pragma unroll
            for (int i = 0; i < XR; ++i)
                if (i < nx) xr[i] = buf_load(sxc, xo[i], xs0);
#pragma unroll
            for (int i = 0; i < WPT; ++i) {
                if (i < nwp) {
                    if (VECW) wr4[i] = buf_load4(sw, wo[i], ws0);
                    else wr1[i] = buf_load(sw, wo[i], ws0);
                }
            }
        } else {                                             // last chunk of a channel count that CI does not divide
#pragma unroll
            for (int i = 0; i < XR; ++i) {
                if (i < nx) {
                    const int idx = tid + 256 * i;
                    const int ci = min(idx / XW, CI - 1);
                    const float v = buf_load(sxc, xo[i] - (unsigned)((ci - min(ci, crem - 1)) * a.Lin) * 4u, xs0);
                    xr[i] = ci < crem ? v : 0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < WPT; ++i) {
                if (i < nwp) {
                    const int idx = tid + 256 * i;
                    const int r = VECW ? idx / (BM / 4) : idx / BM;
                    const int ci = 2 * ((r >> 1) / K) + (r & 1);
                    const bool ok = ci < crem;
                    if (VECW) {
                        const f32x4 v = buf_load4(sw, ok ? wo[i] : 0u, ws0);
                        wr4[i] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
                    } else {
                        const float v = buf_load(sw, ok ? wo[i] : 0u, ws0);
                        wr1[i] = ok ? v : 0.f;
                    }
                }
            }
        }
        if (edge_tile) {
#pragma unroll
            for (int i = 0; i < XR; ++i)
                if (i < nx) xr[i] = ((xz >> i) & 1u) ? 0.f : xr[i];
        }
    };
    auto store_chunk = [&](float* buf) {
#pragma unroll
        for (int i = 0; i < XR; ++i)
            if (i < nx) buf[tid + 256 * i] = xr[i];
        float* Ws = buf + xreg;
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
            if (i < nwp) {
                if (VECW) *reinterpret_cast<f32x4*>(Ws + (tid + 256 * i) * 4) = wr4[i];
                else Ws[tid + 256 * i] = wr1[i];
            }
        }
    };

    const int nchunks = (a.Cin + CI - 1) / CI;
    load_chunk(0);
    store_chunk(smem);
    __syncthreads();
    const int npair = KR >> 1;
    for (int ch = 0; ch < nchunks; ++ch) {
        const float* cur = smem + (ch & 1) * bufsz;
        if (ch + 1 < nchunks) load_chunk((ch + 1) * CI);
        const float* wa = cur + xreg + half * BM + wm_ * (WM * 32) + l31;
        const float* xp = cur + half * XW + (wn * (WN * 32) + l31) * S;
        // software-pipelined pair loop, two pairs per trip with two operand sets: each set is read one MFMA group (4 x 64
        // cycles) before it is used, so no LDS latency is exposed
        float av[WM], bv[WN], an[WM], bn[WN];
        int tap = 0, xoff = 0;
        auto advance = [&]() {
            ++tap; ++xoff;
            if (tap == K) { tap = 0; xoff += 2 * XW - K; }
            wa += 2 * BM;
        };
        auto rd = [&](float (&A_)[WM], float (&B_)[WN]) {
#pragma unroll
            for (int i = 0; i < WM; ++i) A_[i] = wa[i * 32];
#pragma unroll
            for (int j = 0; j < WN; ++j) B_[j] = xp[xoff + j * 32 * S];
        };
        auto mm = [&](const float (&A_)[WM], const float (&B_)[WN]) {
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = mfma32(A_[i], B_[j], acc[i][j]);
        };
        rd(av, bv);
        // (reads past the last pair stay inside the workgroup's LDS allocation: see the slack in launch_gconv2)
        for (int p = 0; p < npair; p += 2) {
            advance();
            rd(an, bn);
            __builtin_amdgcn_sched_barrier(0);
            mm(av, bv);
            __builtin_amdgcn_sched_barrier(0);
            advance();
            rd(av, bv);
            __builtin_amdgcn_sched_barrier(0);
            if (p + 1 < npair) mm(an, bn);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (ch + 1 < nchunks) store_chunk(smem + ((ch + 1) & 1) * bufsz);
        __syncthreads();
    }

    // ---- epilogue: + bias + per-clip vector + residual, ELU, (pixel-shuffled) store.  Addresses are 32-bit offsets into
    // this clip's output rows (buffer stores: per-lane offset + a wave-uniform row offset), so a stored element costs its
    // arithmetic only; tiles that lie inside the output skip every bound check.
    const size_t clip = (size_t)nb * a.Cout * a.Lout;
    const wm_srd_t sy = make_srd(a.y + clip, (size_t)a.Cout * a.Lout * sizeof(float));
    const wm_srd_t sr = make_srd(a.res ? a.res + clip : a.y + clip, (size_t)a.Cout * a.Lout * sizeof(float));
    const bool has_res = a.res != nullptr && a.act != 2, act = a.act == 1, mul_dact = a.act == 2 && a.res != nullptr;
    const float* vecb = a.vec ? a.vec + (size_t)nb * a.Cout : nullptr;
    // per 32-row block: (1) + bias (+ per-clip vector), (2) all residual loads issued together, one wait, (3) ELU, (4) stores --
    // the optional stages are wave-uniform branches around straight-line code, never a branch per element
    const unsigned inv = (65536u + (unsigned)a.nph - 1u) / (unsigned)a.nph;     // exact m / nph for m < 8192, nph <= 8
    const bool shuffle = a.st > 1;
    int ncol[WN];                                                               // output position index n of this lane
#pragma unroll
    for (int j = 0; j < WN; ++j) ncol[j] = n0 + (wn * WN + j) * 32 + l31;
    const int tlo = n0 * a.st - a.shp, thi = (n0 + BN - 1) * a.st + a.st - 1 - a.shp;
    const bool inner = (m0 + BM <= a.Mtot) && (n0 + BN <= a.Nout) && (!shuffle || (tlo >= 0 && thi < a.Lout));
#pragma unroll
    for (int i = 0; i < WM; ++i) {
#pragma unroll
        for (int rh = 0; rh < 16; rh += 8) {                                    // 8 rows at a time: bounds the live offsets / loads
            unsigned off[8][WN];                                                // byte offset inside the clip, 0xffffffff = no store
#pragma unroll
            for (int r8 = 0; r8 < 8; ++r8) {
                const int r = rh + r8;
                const int m = m0 + (wm_ * WM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const int mc = min(m, a.Mtot - 1);
                int co = mc, ph = 0;
                if (shuffle) { co = (int)(((unsigned)mc * inv) >> 16); ph = mc - co * a.nph; }
                float add = a.bias ? a.bias[co] : 0.f;
                if (vecb) add += vecb[co];
                const int rowv = co * a.Lout + ph - (shuffle ? a.shp : 0);
#pragma unroll
                for (int j = 0; j < WN; ++j) {
                    const int t = shuffle ? ncol[j] * a.st + ph - a.shp : ncol[j];
                    const bool ok = inner || (m < a.Mtot && ncol[j] < a.Nout && t >= 0 && t < a.Lout);
                    off[r8][j] = ok ? (unsigned)(rowv + (shuffle ? ncol[j] * a.st : ncol[j])) * 4u : 0xffffffffu;
                    acc[i][j][r] += add;
                }
            }
            if (has_res) {
                float rv[8][WN];
#pragma unroll
                for (int r8 = 0; r8 < 8; ++r8)
#pragma unroll
                    for (int j = 0; j < WN; ++j) rv[r8][j] = buf_load(sr, off[r8][j], 0u);    // 0xffffffff is out of range: reads 0
#pragma unroll
                for (int r8 = 0; r8 < 8; ++r8)
#pragma unroll
                    for (int j = 0; j < WN; ++j) acc[i][j][rh + r8] += rv[r8][j];
            }
            if (act) {
#pragma unroll
                for (int r8 = 0; r8 < 8; ++r8)
#pragma unroll
                    for (int j = 0; j < WN; ++j) acc[i][j][rh + r8] = elu1(acc[i][j][rh + r8]);
            }
            if (mul_dact) {                                                     // dz = g * ELU'(z), ELU'(z) = 1 (y > 0) | y + 1
                float yv[8][WN];
#pragma unroll
                for (int r8 = 0; r8 < 8; ++r8)
#pragma unroll
                    for (int j = 0; j < WN; ++j) yv[r8][j] = buf_load(sr, off[r8][j], 0u);
#pragma unroll
                for (int r8 = 0; r8 < 8; ++r8)
#pragma unroll
                    for (int j = 0; j < WN; ++j) acc[i][j][rh + r8] *= (yv[r8][j] > 0.f ? 1.f : yv[r8][j] + 1.f);
            }
#pragma unroll
            for (int r8 = 0; r8 < 8; ++r8)
#pragma unroll
                for (int j = 0; j < WN; ++j) buf_store(sy, acc[i][j][rh + r8], off[r8][j], 0u);   // out-of-range offsets are dropped by the hardware
        }
    }
}

// largest even ci <= lim that divides Cin (so no partial tail chunk exists), unless that costs more than half the chunk
static int pick_ci(int Cin, int lim) {
    lim &= ~1;
    if (lim >= Cin + (Cin & 1)) return Cin + (Cin & 1);
    for (int c = lim; c >= 2 && 2 * c > lim; c -= 2)
        if (Cin % c == 0) return c;
    return lim;
}

template <int MW, int WM, int WN, bool VECW>
int launch_gconv2(GConvArgs a, hipStream_t stream) {
    constexpr int BM = MW * WM * 32, BN = (4 / MW) * WN * 32, WV = VECW ? 4 : 1, XR = xr_of(BN), KR_MAX = kr_max_of(BM);
    a.XW = (BN - 1) * a.S + a.K;
    int lim = KR_MAX / a.K;                                 // weight rows per chunk <= KR_MAX
    const int cx = (256 * XR) / a.XW;                       // staged input elements per thread <= XR
    if (cx < lim) lim = cx;
    if (lim < 2) return (int)hipErrorInvalidValue;
    a.CI = pick_ci(a.Cin, lim);
    if (a.x2) {                                             // chunks must not straddle the two sources
        int c = lim & ~1;
        while (c >= 2 && (a.Cin1 % c != 0 || a.Cin % c != 0)) c -= 2;
        if (c < 2) return (int)hipErrorInvalidValue;
        a.CI = c;
    }
    const int KR = a.CI * a.K;
    const size_t xreg = (((size_t)a.CI * a.XW + 255) >> 8) * 256, wreg = (((size_t)KR * BM / WV + 255) >> 8) * 256 * WV;
    // + slack: the pipelined pair loop reads up to two pairs past the chunk (four weight rows, two input rows further)
    const size_t lds = (2 * (xreg + wreg) + 4 * BM + 4 * (size_t)a.XW + 64) * sizeof(float);
    if (lds > 160 * 1024) return (int)hipErrorInvalidValue;
    auto kern = gconv2_kernel<MW, WM, WN, VECW>;
    static wm::DevOnce once;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(kern), 160 * 1024, once)) return rc;
    dim3 grid((a.Nout + BN - 1) / BN, (a.Mtot + BM - 1) / BM, a.NB);
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// The same implicit GEMM on the f16 matrix cores with the f16 two-piece split (hi = f16(v s), lo = f16(v s - hi); three products
// lo hi, hi lo, hi hi per product, fp32 accumulate: fp32-grade) for layers whose input channel count is a multiple
// of 16 -- v_mfma_f32_32x32x16_f16 contracts 16 (channel, tap) pairs per instruction where v_mfma_f32_32x32x2_f32 contracts 2 at half
// the rate, so the wide layers gain most.  The K dimension is walked as (16-channel chunk, tap):
//   * weights: a pre-packed f16 image [chunk][tap][Mtot][16 channels] x {hi, lo} (wm_gconv_pack_h: w * ws, ws a power of two from
//     max |w|, {ws, 1 / ws} behind the image).  An A fragment (one output row, 8 consecutive channels) is ONE 16-byte global load,
//     coalesced over the wave's 32 rows: the weights never pass through LDS (L2 / L1 serve the re-use between tiles and waves).
//   * input: a chunk's [16][XW] window is staged global -> registers -> LDS as a channel-minor image [position][16 channels] x {hi, lo}
//     (pitch 24 halves), one chunk ahead of the matrix phase; a B fragment (one output position, 8 consecutive channels at one tap) is
//     one aligned ds_read_b128 at row position * S + tap.  gscale: the input is multiplied by gs before the split and clamped to the
//     f16 range; the accumulators leave times 1 / (ws gs).  One gs for the launch (gradients) or one per clip (per_clip: activations).
// Epilogue as gconv2_kernel's.
// ---------------------------------------------------------------------------------------------------------------
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct GConvHArgs {
    GConvArgs g;
    const unsigned short* wph;      // [2 pieces][Cin / 16][K][Mtot][16] f16, then {ws, 1 / ws}
    const float* gscale;            // {gs, 1 / gs} or null
    float* ymax;                    // optional: max |y| over everything the launch stores (atomic max of non-negative floats as ints; zeroed by the caller)
    int per_clip;                   // 1: gscale holds max |x| per clip ([NB]; gs derived here) and ymax receives one maximum per clip ([NB])
};

template <int MW, int WM, int WN, int XRH>   // XRH: staged window elements (channel pairs) per thread, 8 XW <= 256 XRH
__global__ __launch_bounds__(256) void gconvh_kernel(GConvHArgs ha) {
    const GConvArgs& a = ha.g;
    constexpr int NWN = 4 / MW, BM = MW * WM * 32, BN = NWN * WN * 32, PX = 24;
    extern __shared__ __align__(16) unsigned char smem_h[];
    unsigned short* Xs = reinterpret_cast<unsigned short*>(smem_h);      // [2 buffers][2 pieces][XWP][PX]
    const int K = a.K, S = a.S, XW = a.XW;
    const int XWP = XW + 8;                                                 // slack rows: discarded columns read past the window
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), half = lane >> 5, l31 = lane & 31;
    const int wm_ = wave % MW, wn = wave / MW;
    const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM, nb = blockIdx.z;
    const int u0 = n0 * S - a.P;
    const int nchunks = a.Cin >> 4;
    const size_t piece = (size_t)nchunks * K * a.Mtot * 16;                 // halves per weight piece
    const float* tail = reinterpret_cast<const float*>(ha.wph + 2 * piece);
    float gs = 1.f, gsinv = 1.f;
    if (ha.gscale && ha.per_clip) {                                        // the power of two that puts this clip's max |x| into (2^11, 2^12]
        const float m = ha.gscale[nb];
        if (m > 0.f && m < 3.0e38f) gs = fminf(fmaxf(exp2f(floorf(12.f - log2f(m))), 1.0e-30f), 1.0e30f);
        gsinv = 1.f / gs;
    } else if (ha.gscale) {
        gs = ha.gscale[0];
        gsinv = ha.gscale[1];
    }
    const float dinv = tail[1] * gsinv;

    // ---- staging map: element i of a thread = (channel pair cp, window position j): idx = tid + 256 i = cp * XW + j
    const int nx = (8 * XW + 255) >> 8;
    unsigned xo[XRH];            // byte offset of channel 2 cp at the clamped position
    unsigned xl[XRH];            // LDS dword index (position * PX / 2 + cp), 0xffffffff: nothing to write
    unsigned xz = 0;             // bit i: zero padding
#pragma unroll
    for (int i = 0; i < XRH; ++i) {
        const int idx = tid + 256 * i, cp = idx / XW, j = idx - cp * XW, u = u0 + j;
        const bool live = (i < nx) && (cp < 8);
        xz |= ((u < 0 || u >= a.Lin) ? 1u : 0u) << i;
        xo[i] = (unsigned)((2 * min(cp, 7)) * a.Lin + min(max(u, 0), a.Lin - 1)) * 4u;
        xl[i] = live ? (unsigned)(j * (PX / 2) + cp) : 0xffffffffu;
    }
    const int cin1 = a.x2 ? a.Cin1 : a.Cin;
    const wm_srd_t sx = make_srd(a.x + (size_t)nb * cin1 * a.Lin, (size_t)cin1 * a.Lin * sizeof(float));
    const wm_srd_t sx2 = make_srd(a.x2 ? a.x2 + (size_t)nb * (a.Cin - cin1) * a.Lin : a.x, (size_t)(a.Cin - cin1) * a.Lin * sizeof(float));
    const wm_srd_t sw = make_srd(reinterpret_cast<const float*>(ha.wph), 2 * piece * sizeof(unsigned short));
    float xa[XRH], xb[XRH];
    auto load_chunk = [&](int c) {
        const int c0 = 16 * c;
        const bool second = c0 >= cin1;
        const wm_srd_t sxc = second ? sx2 : sx;
        const unsigned s0 = (unsigned)((c0 - (second ? cin1 : 0)) * a.Lin) * 4u;
#pragma unroll
        for (int i = 0; i < XRH; ++i)
            if (i < nx) { xa[i] = buf_load(sxc, xo[i], s0); xb[i] = buf_load(sxc, xo[i] + (unsigned)a.Lin * 4u, s0); }
    };
    auto store_chunk = [&](unsigned short* buf) {
        unsigned* hi32 = reinterpret_cast<unsigned*>(buf);
        unsigned* lo32 = reinterpret_cast<unsigned*>(buf + XWP * PX);
#pragma unroll
        for (int i = 0; i < XRH; ++i) {
            if (i < nx) {
                const bool z = (xz >> i) & 1u;
                const float va = z ? 0.f : __builtin_amdgcn_fmed3f(xa[i] * gs, -6.0e4f, 6.0e4f);
                const float vb = z ? 0.f : __builtin_amdgcn_fmed3f(xb[i] * gs, -6.0e4f, 6.0e4f);
                const h16x2 h_ = __builtin_convertvector(f32x2{va, vb}, h16x2);
                const h16x2 l_ = __builtin_convertvector(f32x2{va - (float)h_.x, vb - (float)h_.y}, h16x2);
                if (xl[i] != 0xffffffffu) { hi32[xl[i]] = __builtin_bit_cast(unsigned, h_); lo32[xl[i]] = __builtin_bit_cast(unsigned, l_); }
            }
        }
    };
    const int bufh = 2 * XWP * PX;                                          // halves per buffer (two pieces)
    // the slack rows are read by discarded columns only: keep them finite
    for (int i = tid; i < 2 * 2 * 8 * PX / 2; i += 256) {
        const int bq = i / (8 * PX / 2), r = i - bq * (8 * PX / 2);          // bq = buffer * 2 + piece
        reinterpret_cast<unsigned*>(Xs + (bq >> 1) * bufh + (bq & 1) * XWP * PX + XW * PX)[r] = 0u;
    }
    f32x16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // weight fragment of (chunk c, tap, row tile i, piece p): 16 bytes at ((c K + tap) Mtot + row) * 16 + 8 half halves; rows past Mtot read 0
    unsigned wrow[WM], wrow_lo[WM];
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        const int m = m0 + (wm_ * WM + i) * 32 + l31;
        wrow[i] = (m < a.Mtot) ? (unsigned)(m * 16 + 8 * half) * 2u : 0xfffffff0u;
        wrow_lo[i] = (m < a.Mtot) ? wrow[i] + (unsigned)(piece * 2) : 0xfffffff0u;
    }
    auto load_w = [&](int c, int tap, u32x4 (&A)[WM][2]) {
        const unsigned s0 = (unsigned)(((size_t)(c * K + tap) * a.Mtot) * 16) * 2u;
#pragma unroll
        for (int i = 0; i < WM; ++i) {
            A[i][0] = __builtin_bit_cast(u32x4, buf_load4(sw, wrow[i], s0));
            A[i][1] = __builtin_bit_cast(u32x4, buf_load4(sw, wrow_lo[i], s0));
        }
    };
    auto mma = [&](const u32x4& A_, const u32x4& B_, f32x16 c) -> f32x16 {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, A_), __builtin_bit_cast(h16x8, B_), c, 0, 0, 0);
    };
    load_chunk(0);
    store_chunk(Xs);
    __syncthreads();
    // weight fragments of this k-step and of the next two (in flight): an L2 hit takes longer than the 6-12 MFMAs of one k-step
    u32x4 Ac[WM][2], An[WM][2], An2[WM][2];
    const int nq = nchunks * K;                                             // k-steps q = c K + tap
    auto load_q = [&](int q, u32x4 (&A)[WM][2]) {
        if (q < nq) { const int c_ = q / K; load_w(c_, q - c_ * K, A); }
    };
    load_q(0, Ac); load_q(1, An);
    for (int c = 0; c < nchunks; ++c) {
        const unsigned short* cur = Xs + (c & 1) * bufh;
        if (c + 1 < nchunks) load_chunk(c + 1);
        const unsigned short* xrow = cur + ((wn * (WN * 32) + l31) * S) * PX + 8 * half;
        u32x4 Bh[WN], Bl[WN], Bhn[WN], Bln[WN];          // this tap's input fragments, the next tap's (LDS reads in flight)
        auto load_b = [&](int tap, u32x4 (&H_)[WN], u32x4 (&L_)[WN]) {
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                const unsigned short* pB = xrow + (j * 32 * S + tap) * PX;
                H_[j] = *reinterpret_cast<const u32x4*>(pB);
                L_[j] = *reinterpret_cast<const u32x4*>(pB + XWP * PX);
            }
        };
        load_b(0, Bh, Bl);
        for (int tap = 0; tap < K; ++tap) {
            load_q(c * K + tap + 2, An2);
            if (tap + 1 < K) load_b(tap + 1, Bhn, Bln);
            // piece products outermost: the WM x WN accumulators form independent chains between two dependent MFMAs
#pragma unroll
            for (int pp = 0; pp < 3; ++pp)
#pragma unroll
                for (int i = 0; i < WM; ++i)
#pragma unroll
                    for (int j = 0; j < WN; ++j)
                        acc[i][j] = mma(Ac[i][pp == 0 ? 1 : 0], pp == 1 ? Bl[j] : Bh[j], acc[i][j]);     // lo hi, hi lo, hi hi
#pragma unroll
            for (int i = 0; i < WM; ++i) { Ac[i][0] = An[i][0]; Ac[i][1] = An[i][1]; An[i][0] = An2[i][0]; An[i][1] = An2[i][1]; }
#pragma unroll
            for (int j = 0; j < WN; ++j) { Bh[j] = Bhn[j]; Bl[j] = Bln[j]; }
        }
        if (c + 1 < nchunks) store_chunk(Xs + ((c + 1) & 1) * bufh);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] *= dinv;

    // ---- epilogue (gconv2_kernel's): + bias + per-clip vector + residual, ELU / ELU', (pixel-shuffled) store
    float vmax = 0.f;
    const size_t clip = (size_t)nb * a.Cout * a.Lout;
    const wm_srd_t sy = make_srd(a.y + clip, (size_t)a.Cout * a.Lout * sizeof(float));
    const wm_srd_t sr = make_srd(a.res ? a.res + clip : a.y + clip, (size_t)a.Cout * a.Lout * sizeof(float));
    const bool has_res = a.res != nullptr && a.act != 2, act = a.act == 1, mul_dact = a.act == 2 && a.res != nullptr;
    const float* vecb = a.vec ? a.vec + (size_t)nb * a.Cout : nullptr;
    const unsigned inv = (65536u + (unsigned)a.nph - 1u) / (unsigned)a.nph;
    const bool shuffle = a.st > 1;
    int ncol[WN];
#pragma unroll
    for (int j = 0; j < WN; ++j) ncol[j] = n0 + (wn * WN + j) * 32 + l31;
    const int tlo = n0 * a.st - a.shp, thi = (n0 + BN - 1) * a.st + a.st - 1 - a.shp;
    const bool inner = (m0 + BM <= a.Mtot) && (n0 + BN <= a.Nout) && (!shuffle || (tlo >= 0 && thi < a.Lout));
#pragma unroll
    for (int i = 0; i < WM; ++i) {
#pragma unroll
        for (int rh = 0; rh < 16; rh += 8) {
            unsigned off[8][WN];
#pragma unroll
            for (int r8 = 0; r8 < 8; ++r8) {
                const int r = rh + r8;
                const int m = m0 + (wm_ * WM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const int mc = min(m, a.Mtot - 1);
                int co = mc, ph = 0;
                if (shuffle) { co = (int)(((unsigned)mc * inv) >> 16); ph = mc - co * a.nph; }
                float add = a.bias ? a.bias[co] : 0.f;
                if (vecb) add += vecb[co];
                const int rowv = co * a.Lout + ph - (shuffle ? a.shp : 0);
#pragma unroll
                for (int j = 0; j < WN; ++j) {
                    const int t = shuffle ? ncol[j] * a.st + ph - a.shp : ncol[j];
                    const bool ok = inner || (m < a.Mtot && ncol[j] < a.Nout && t >= 0 && t < a.Lout);
                    off[r8][j] = ok ? (unsigned)(rowv + (shuffle ? ncol[j] * a.st : ncol[j])) * 4u : 0xffffffffu;
                    acc[i][j][r] += add;
                }
            }
            if (has_res) {
                float rv[8][WN];
#pragma unroll
                for (int r8 = 0; r8 < 8; ++r8)
#pragma unroll
                    for (int j = 0; j < WN; ++j) rv[r8][j] = buf_load(sr, off[r8][j], 0u);
#pragma unroll
                for (int r8 = 0; r8 < 8; ++r8)
#pragma unroll
                    for (int j = 0; j < WN; ++j) acc[i][j][rh + r8] += rv[r8][j];
            }
            if (act) {
#pragma unroll
                for (int r8 = 0; r8 < 8; ++r8)
#pragma unroll
                    for (int j = 0; j < WN; ++j) acc[i][j][rh + r8] = elu1(acc[i][j][rh + r8]);
            }
            if (mul_dact) {
                float yv[8][WN];
#pragma unroll
                for (int r8 = 0; r8 < 8; ++r8)
#pragma unroll
                    for (int j = 0; j < WN; ++j) yv[r8][j] = buf_load(sr, off[r8][j], 0u);
#pragma unroll
                for (int r8 = 0; r8 < 8; ++r8)
#pragma unroll
                    for (int j = 0; j < WN; ++j) acc[i][j][rh + r8] *= (yv[r8][j] > 0.f ? 1.f : yv[r8][j] + 1.f);
            }
#pragma unroll
            for (int r8 = 0; r8 < 8; ++r8)
#pragma unroll
                for (int j = 0; j < WN; ++j) {
                    buf_store(sy, acc[i][j][rh + r8], off[r8][j], 0u);
                    vmax = fmaxf(vmax, off[r8][j] != 0xffffffffu ? fabsf(acc[i][j][rh + r8]) : 0.f);
                }
        }
    }
    if (ha.ymax) {                                   // the next consumer's gradient scale without a pass over y
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o));
        if (lane == 0 && vmax == vmax && vmax < 3.0e38f) atomicMax(reinterpret_cast<int*>(ha.ymax) + (ha.per_clip ? nb : 0), __float_as_int(vmax));
    }
}

template <int MW, int WM, int WN, int XRH>
int launch_gconvh_x(GConvHArgs ha, hipStream_t stream) {
    GConvArgs& a = ha.g;
    constexpr int BM = MW * WM * 32, BN = (4 / MW) * WN * 32;
    a.XW = (BN - 1) * a.S + a.K;
    if (8 * a.XW > 256 * XRH) return (int)hipErrorInvalidValue;         // staged window elements per thread <= XRH
    const size_t lds = (size_t)2 * 2 * (a.XW + 8) * 24 * sizeof(unsigned short);
    if (lds > 160 * 1024) return (int)hipErrorInvalidValue;
    auto kern = gconvh_kernel<MW, WM, WN, XRH>;
    static wm::DevOnce once;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(kern), 160 * 1024, once)) return rc;
    dim3 grid((a.Nout + BN - 1) / BN, (a.Mtot + BM - 1) / BM, a.NB);
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, stream, ha);
    WM_CHECK_LAUNCH();
    return 0;
}
template <int MW, int WM, int WN>
int launch_gconvh(GConvHArgs ha, hipStream_t stream) {
    constexpr int BN = (4 / MW) * WN * 32;
    const int XW = (BN - 1) * ha.g.S + ha.g.K;
    if (8 * XW <= 256 * 6) return launch_gconvh_x<MW, WM, WN, 6>(ha, stream);     // stride-1 layers: a short window, 56 registers less
    return launch_gconvh_x<MW, WM, WN, 20>(ha, stream);
}

// f16 two-piece image of a wm_gconv weight matrix wp [Cin * K][Mtot] (row ci * K + tap): out[piece][ci / 16][tap][m][ci % 16];
// the scale {ws, 1 / ws} sits behind the image (written by gscale_from_max beforehand)
// (ws_fixed > 0: that scale is used and written behind the image by workgroup 0 -- no pass for max |w|)
// mode -1: wp is the wm_gconv matrix [Cin * K][Mtot].  mode 0 / 1: wp is a Conv1d weight w [Cout][Cin_w][K] itself and the re-indexing of
// the host mirror happens here -- 0 forward (GEMM channel = ci, row = co), 1 stride-1 data gradient (GEMM channel = co, row = ci, taps
// flipped): the permute / flip / contiguous launches of the mirror disappear
__global__ __launch_bounds__(256) void gconv_pack_h_kernel(const float* __restrict__ wp, unsigned short* __restrict__ out, int Cin, int K, int Mtot,
                                                           float ws_fixed, int mode) {
    const size_t n = (size_t)Cin * K * Mtot, piece = n;
    float* tail = reinterpret_cast<float*>(out + 2 * piece);
    const float ws = ws_fixed > 0.f ? ws_fixed : tail[0];
    if (ws_fixed > 0.f && blockIdx.x == 0 && threadIdx.x == 0) { tail[0] = ws_fixed; tail[1] = 1.f / ws_fixed; }
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        // i walks the OUTPUT image: ((c K + tap) Mtot + m) * 16 + e
        const int e = (int)(i & 15);
        const size_t q = i >> 4;
        const int m = (int)(q % Mtot);
        const size_t ct = q / Mtot;
        const int tap = (int)(ct % K), c = (int)(ct / K);
        const int qch = 16 * c + e;                  // GEMM input channel
        const size_t src = mode < 0 ? ((size_t)qch * K + tap) * Mtot + m
                         : mode == 0 ? ((size_t)m * Cin + qch) * K + tap                    // w[co = m][ci = q][tap]
                                     : ((size_t)qch * Mtot + m) * K + (K - 1 - tap);        // w[co = q][ci = m][K - 1 - tap]
        const float v = __builtin_amdgcn_fmed3f(wp[src] * ws, -6.0e4f, 6.0e4f);
        const _Float16 hi = (_Float16)v;
        const _Float16 lo = (_Float16)(v - (float)hi);
        out[i] = __builtin_bit_cast(unsigned short, hi);
        out[piece + i] = __builtin_bit_cast(unsigned short, lo);
    }
}

}  // namespace

extern "C" {

// y[nb][co][t'] = act( bias[co] + vec[nb][co] + res + sum_{ci,k} wp[ci*K+k][m] * x[nb][ci][n*S + k - P] )
//   st == 1: m = co, t' = n (Cout == Mtot, Lout == Nout);  st > 1: m = co*st + phase, t' = n*st + phase - shp.
int wm_gconv(const float* x, const float* wp, const float* bias, const float* vec, const float* res, float* y, int NB,
             int Cin, int Lin, int K, int S, int P, int Mtot, int Nout, int st, int shp, int Cout, int Lout, int act,
             const float* x2, int Cin1, int nph, hipStream_t stream) {
    if (NB <= 0 || Cin <= 0 || K <= 0 || K > 16 || S <= 0 || S > 8 || Mtot <= 0 || Nout <= 0 || st < 1 || st > 8 || Lin <= 0 ||
        Lin >= (1 << 24) || NB > 65535 || Mtot >= 8192)
        return (int)hipErrorInvalidValue;
    if (nph <= 0) nph = st;
    if (nph > st || (x2 && (Cin1 <= 0 || Cin1 >= Cin))) return (int)hipErrorInvalidValue;
    GConvArgs a{x, wp, bias, vec, res, y, NB, Cin, Lin, K, S, P, Mtot, Nout, st, shp, Cout, Lout, act, 0, 0, x2, x2 ? Cin1 : Cin, nph};
    const bool vec4 = (Mtot % 4 == 0) && ((reinterpret_cast<uintptr_t>(wp) & 15) == 0);
    // tile shape by problem shape: (rows, columns) = (128,128) | (64,128) | (32,256); short sequences (<= 64): (128,64) | (64,64)
    if (!vec4) {
        if (Mtot > 32) return (int)hipErrorInvalidValue;     // unaligned weight rows: only the narrow heads (1 / 17 channels)
        return launch_gconv2<1, 1, 2, false>(a, stream);
    }
    int rc;
    if (Nout <= 64) rc = Mtot > 64 ? launch_gconv2<2, 2, 1, true>(a, stream) : launch_gconv2<2, 1, 1, true>(a, stream);
    else if (Mtot > 64) rc = launch_gconv2<2, 2, 2, true>(a, stream);
    else if (Mtot > 32) rc = launch_gconv2<2, 1, 2, true>(a, stream);
    else rc = launch_gconv2<1, 1, 2, true>(a, stream);
    if (rc == (int)hipErrorInvalidValue) rc = launch_gconv2<2, 1, 1, true>(a, stream);   // widest-stride shapes: the narrowest input tile
    return rc;
}

// wm_gconv on the f16 two-piece split: wph = wm_gconv_pack_h's image of the SAME wp; Cin % 16 == 0 (and Cin1 % 16 == 0 with two sources);
// gscale = {gs, 1 / gs} for the input (wm_gscale_absmax), or max |x| per clip with per_clip (a producer's ymax, wm_absmax_rows), NULL:
// split unscaled.
// hipErrorInvalidValue when the shape is outside the kernel's window limits (the caller then uses wm_gconv).
int wm_gconv_h(const float* x, const void* wph, const float* bias, const float* vec, const float* res, float* y, int NB,
               int Cin, int Lin, int K, int S, int P, int Mtot, int Nout, int st, int shp, int Cout, int Lout, int act,
               const float* x2, int Cin1, int nph, const float* gscale, float* ymax, int per_clip, hipStream_t stream) {
    if (NB <= 0 || Cin <= 0 || (Cin & 15) || K <= 0 || K > 16 || S <= 0 || S > 8 || Mtot <= 0 || Nout <= 0 || st < 1 || st > 8 || Lin <= 0 ||
        Lin >= (1 << 24) || NB > 65535 || Mtot >= 8192 || !wph)
        return (int)hipErrorInvalidValue;
    if (nph <= 0) nph = st;
    if (nph > st || (x2 && (Cin1 <= 0 || Cin1 >= Cin || (Cin1 & 15)))) return (int)hipErrorInvalidValue;
    GConvHArgs ha{GConvArgs{x, nullptr, bias, vec, res, y, NB, Cin, Lin, K, S, P, Mtot, Nout, st, shp, Cout, Lout, act, 0, 0, x2,
                            x2 ? Cin1 : Cin, nph},
                  reinterpret_cast<const unsigned short*>(wph), gscale, ymax, per_clip ? 1 : 0};
    int rc;
    if (Nout <= 64) rc = Mtot > 64 ? launch_gconvh<2, 2, 1>(ha, stream) : launch_gconvh<2, 1, 1>(ha, stream);
    else if (Mtot > 64) rc = launch_gconvh<2, 2, 2>(ha, stream);
    else if (Mtot > 32) rc = launch_gconvh<2, 1, 2>(ha, stream);
    else rc = launch_gconvh<1, 1, 2>(ha, stream);
    if (rc == (int)hipErrorInvalidValue && Nout > 64) rc = Mtot > 64 ? launch_gconvh<2, 2, 1>(ha, stream) : launch_gconvh<2, 1, 1>(ha, stream);
    return rc;
}

// f16 image of wp [Cin * K][Mtot] for wm_gconv_h: wph holds 2 * Cin * K * Mtot f16 + 2 floats; scratch >= 1024 floats
int wm_gconv_pack_h(const float* wp, void* wph, float* scratch, int Cin, int K, int Mtot, hipStream_t stream) {
    if (!wp || !wph || Cin <= 0 || (Cin & 15) || K <= 0 || Mtot <= 0) return (int)hipErrorInvalidValue;
    const long long n = (long long)Cin * K * Mtot;
    unsigned short* out = reinterpret_cast<unsigned short*>(wph);
    float* tail = reinterpret_cast<float*>(out + 2 * n);
    // scratch == NULL: the fixed scale 2^8 (one launch).  Weights of magnitude 4e-6 ... 250 keep a normal hi piece and lose nothing that an
    // fp32 product would keep: the scale only has to hold the pieces inside f16's 30 binades; larger weights saturate at +-6e4 / 2^8
    if (scratch) {
        int rc = wm_gscale_absmax(wp, n, scratch, 10.0f, tail, stream);   // max |w| ws in (2^9, 2^10]
        if (rc) return rc;
    }
    const int grid = (int)((n + 255) / 256 < 512 ? (n + 255) / 256 : 512);
    hipLaunchKernelGGL(gconv_pack_h_kernel, dim3(grid), dim3(256), 0, stream, wp, out, Cin, K, Mtot, scratch ? 0.f : 256.f, -1);
    WM_CHECK_LAUNCH();
    return 0;
}

// the same image straight from a Conv1d weight w [Cout][Cin][K] (fixed scale 2^8): mode 0 = the forward matrix (GEMM channels Cin, rows
// Cout), mode 1 = the stride-1 data-gradient matrix (GEMM channels Cout, rows Cin, taps flipped).  wph: 2 * Cout * Cin * K f16 + 2 floats
int wm_gconv_pack_h_conv(const float* w, void* wph, int Cout, int Cin, int K, int mode, hipStream_t stream) {
    const int gch = mode == 0 ? Cin : Cout, rows = mode == 0 ? Cout : Cin;
    if (!w || !wph || (mode != 0 && mode != 1) || Cout <= 0 || Cin <= 0 || K <= 0 || (gch & 15)) return (int)hipErrorInvalidValue;
    const long long n = (long long)Cout * Cin * K;
    const int grid = (int)((n + 255) / 256 < 512 ? (n + 255) / 256 : 512);
    hipLaunchKernelGGL(gconv_pack_h_kernel, dim3(grid), dim3(256), 0, stream, w, reinterpret_cast<unsigned short*>(wph), gch, K, rows, 256.f, mode);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
