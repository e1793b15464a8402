// The thin ends of the two networks (py/main16.py):
//   stem   Conv1d(1,64,7,padding=3)   Generator.encoder[0] :134 / Detector.model[0] :177
//   head1  Conv1d(64,1,1)             Generator.decoder[2] :146
//   headN  Conv1d(64,1+bits,1)        Detector.model[3]    :180, bits 0..63, written directly in the
//                                     (B,T,1+bits) layout Detector.forward returns (:186)
// These are HBM-bound (one 64-channel frame in or out per sample, a handful of FLOPs per
// byte) so they are plain VALU kernels with 16-B coalesced frame accesses; only the tiny
// one-channel side goes through LDS.
#include "wm_common.hpp"
using namespace wm;

namespace {

// ------------------------------------------------------------------------------- stem forward
// block = (clip, 1024-sample tile); thread = 4 consecutive samples; loop over the 64 filters.
__global__ __launch_bounds__(256) void stem_fwd_kernel(const float* __restrict__ s, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ y, int T) {
    __shared__ float ss[1024 + 8];
    __shared__ float ws[64 * 8];
    const int tilesPerClip = (T + 1023) / 1024;
    const int b = blockIdx.x / tilesPerClip, t0 = (blockIdx.x % tilesPerClip) * 1024;
    const float* sb = s + (size_t)b * T;
    for (int i = threadIdx.x; i < 1024 + 6; i += 256) {
        const int t = t0 - 3 + i;
        ss[i] = (t >= 0 && t < T) ? sb[t] : 0.f;
    }
    for (int i = threadIdx.x; i < 512; i += 256) {
        const int co = i >> 3, j = i & 7;
        ws[i] = (j < 7) ? w[co * 7 + j] : bias[co];
    }
    __syncthreads();
    const int t = t0 + 4 * threadIdx.x;
    if (t >= T) return;
    float v[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) v[i] = ss[4 * threadIdx.x + i];
    float* yb = y + (size_t)b * 64 * T + t;
#pragma unroll 4
    for (int co = 0; co < 64; ++co) {
        const float* wc = ws + co * 8;
        float4 o = make_float4(wc[7], wc[7], wc[7], wc[7]);
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const float wj = wc[j];
            o.x = fmaf(wj, v[j], o.x);
            o.y = fmaf(wj, v[j + 1], o.y);
            o.z = fmaf(wj, v[j + 2], o.z);
            o.w = fmaf(wj, v[j + 3], o.w);
        }
        *reinterpret_cast<float4*>(yb + (size_t)co * T) = o;
    }
}

// ------------------------------------------------------------------------------ stem backward
// g [B,64,T]; persistent blocks over (clip, 256-sample) tiles, next tile prefetched into registers.
//   dw[co][j] = sum_{b,t} g[co,t] s[t+j-3] ; db[co] = sum g[co,t]  -> on the fp32 matrix cores: M = co, K = time,
//               N = 8 columns (7 taps + a column of ones for the bias) padded to 32     -> partial[block][64*8]
//   ds[b,t]   = sum_{co,j} g[co,t-j+3] w[co][j]   (only if ds != nullptr; clips >= nds are skipped): VALU, register
//               blocked 4 samples x 16 channels per thread, the four channel groups are summed through LDS.
__global__ __launch_bounds__(256) void stem_bwd_kernel(const float* __restrict__ g, const float* __restrict__ s,
                                                       const float* __restrict__ w, float* __restrict__ ds,
                                                       float* __restrict__ partial, int B, int T, int nds) {
    constexpr int NT = 256, GS = NT + 8;             // g tile row: 3 halo | 256 | 3 halo starting at column 1; main part at 4
    extern __shared__ __align__(16) float smem[];
    float* gs = smem;                                // [64][GS]
    float* ss = gs + 64 * GS;                        // [NT + 40]: s[t0 - 3 + i]; zero padded so that B-operand reads stay in range
    float* dsp = ss + NT + 40;                       // [4][NT] partial ds of the four channel groups (16-byte aligned: 17192 floats in)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int tilesPerClip = (T + NT - 1) / NT, ntiles = B * tilesPerClip;
    f32x16 acc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
    float4 sg[16];
    float hg[2], sv[2];
    // piece p < 16: one row group of the g tile; piece 16: halo columns + the clip samples.  Branch-free (clamped addresses).
    // The main loop issues one piece per two k-steps of the dw product instead of the whole 64-KB tile at once.
    auto load_piece = [&](int tile, int p) {
        const int b = tile / tilesPerClip, t0 = (tile % tilesPerClip) * NT;
        const float* gb = g + (size_t)b * 64 * T;
        if (p < 16) {
            const int i = tid + p * 256, c = i >> 6, q = i & 63;
            sg[p] = *reinterpret_cast<const float4*>(gb + (size_t)c * T + min(t0 + 4 * q, T - 4));
            return;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = min(tid + k * 256, 64 * 6 - 1), c = i / 6, h = i % 6;
            const int t = (h < 3) ? t0 - 3 + h : t0 + NT + (h - 3);
            hg[k] = gb[(size_t)c * T + min(max(t, 0), T - 1)];
            const int ts_ = t0 - 3 + tid + k * 256;
            sv[k] = s[(size_t)b * T + min(max(ts_, 0), T - 1)];
        }
    };
    auto load_tile = [&](int tile) {
#pragma unroll
        for (int p = 0; p <= 16; ++p) load_piece(tile, p);
    };
    auto write_tile = [&](int tile) {
        const int t0 = (tile % tilesPerClip) * NT;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int i = tid + k * 256, c = i >> 6, q = i & 63;
            float4 v = sg[k];
            if (t0 + 4 * q >= T) v = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(gs + c * GS + 4 + 4 * q) = v;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = tid + k * 256;
            if (i < 64 * 6) {
                const int c = i / 6, h = i % 6;
                const int t = (h < 3) ? t0 - 3 + h : t0 + NT + (h - 3);
                gs[c * GS + ((h < 3) ? 1 + h : 4 + NT + (h - 3))] = (t >= 0 && t < T) ? hg[k] : 0.f;
            }
            if (i < NT + 40) {
                const int ts_ = t0 - 3 + i;
                ss[i] = (i < NT + 6 && ts_ >= 0 && ts_ < T) ? sv[k] : 0.f;
            }
        }
    };
    int tile = blockIdx.x;
    if (tile < ntiles) load_tile(tile);
    __syncthreads();
    if (tile < ntiles) write_tile(tile);
    __syncthreads();
    while (tile < ntiles) {
        const int next = tile + gridDim.x, nextc = min(next, ntiles - 1);     // clamped: loaded (valid memory), never written
        const int b = tile / tilesPerClip, t0 = (tile % tilesPerClip) * NT;
        // ---- dw / db: this wave's 64 time steps.  A[i = co][k = t] = gs[co][t];  B[k = t][j] = s[t + j - 3] (j < 7), 1 (j == 7), 0
        {
            const float* ap = gs + l31 * GS + 4 + wave * 64 + half;
            const float* bp = ss + wave * 64 + half + l31;        // ss[t - t0 + j] = s[t + j - 3]
            const bool tapcol = l31 < 7, onecol = l31 == 7;
#pragma unroll
            for (int k2 = 0; k2 < 32; ++k2) {
                if ((k2 & 1) == 0 || k2 == 31) load_piece(nextc, k2 == 31 ? 16 : k2 >> 1);
                const float sval = bp[2 * k2];
                const float bv = tapcol ? sval : (onecol ? 1.f : 0.f);
                acc[0] = mfma32(ap[2 * k2], bv, acc[0]);
                acc[1] = mfma32(ap[32 * GS + 2 * k2], bv, acc[1]);
            }
        }
        // ---- ds (Detector stem: gradient w.r.t. the watermarked half of the batch)
        if (ds && b < nds) {
            // 16 channels x 4 samples per thread.  The channel is the same in every lane of a wave, so the seven taps come
            // from w through the scalar cache into scalar registers: three LDS reads per channel (the g row) instead of five
            const int cg = __builtin_amdgcn_readfirstlane(wave), tq = lane;
            float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;
#pragma unroll 4
            for (int cc = 0; cc < 16; ++cc) {
                const int co = cg * 16 + cc;
                const f32x4 ga = lds_read4(gs + co * GS + 4 * tq);          // t0+4tq-4 .. -1
                const f32x4 gb4 = lds_read4(gs + co * GS + 4 * tq + 4);     // t0+4tq   .. +3
                const f32x4 gc = lds_read4(gs + co * GS + 4 * tq + 8);      // t0+4tq+4 .. +7
                const float* wc = w + co * 7;
                // gv[i] = g[co][t0 + 4tq - 3 + i], i = 0..9 ;  ds[t] = sum_j g[t + 3 - j] w[j]
                const float gv[10] = {ga.y, ga.z, ga.w, gb4.x, gb4.y, gb4.z, gb4.w, gc.x, gc.y, gc.z};
                const float wj[7] = {wc[0], wc[1], wc[2], wc[3], wc[4], wc[5], wc[6]};
#pragma unroll
                for (int j = 0; j < 7; ++j) {
                    o0 = fmaf(gv[6 - j], wj[j], o0); o1 = fmaf(gv[7 - j], wj[j], o1);
                    o2 = fmaf(gv[8 - j], wj[j], o2); o3 = fmaf(gv[9 - j], wj[j], o3);
                }
            }
            *reinterpret_cast<float4*>(dsp + cg * NT + 4 * tq) = make_float4(o0, o1, o2, o3);
        }
        __syncthreads();
        if (ds && b < nds) {
            const int t = t0 + tid;
            if (t < T) ds[(size_t)b * T + t] = (dsp[tid] + dsp[NT + tid]) + (dsp[2 * NT + tid] + dsp[3 * NT + tid]);
        }
        if (next < ntiles) write_tile(next);
        __syncthreads();
        tile = next;
    }
    // fixed-order reduction of the four waves' [64 x 8] tiles
    float* red = gs;
    for (int wv = 0; wv < 4; ++wv) {
        if (wave == wv && l31 < 8) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int o = (mt * 32 + mfma_row(r, half)) * 8 + l31;
                    red[o] = (wv == 0) ? acc[mt][r] : red[o] + acc[mt][r];
                }
        }
        __syncthreads();
    }
    float* out = partial + (size_t)blockIdx.x * 512;
    for (int i = tid; i < 512; i += 256) out[i] = red[i];
}

// out[i] (+)= sum_p partial[p*stride + i],  i < count.  Block = 64 outputs x 4 part-groups of the slab list (column_sum_d:
// fp64, fixed order, bit-reproducible); launch with 256 threads and ceil(count / 64) blocks.
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ partial, int nparts, int stride, int count,
                                                              float* __restrict__ out, int accumulate) {
    __shared__ double sq[4][64];
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const float s = (float)column_sum_d<4>(partial, nparts, (size_t)stride, i, i < count, sq);
    if (threadIdx.x < 64 && i < count) out[i] = accumulate ? out[i] + s : s;
}
// stem partial [nparts][64][8] -> dw[64][7], db[64].  nparts reaches 2 x NCU = 512 slabs: 8 blocks of 64 columns x 16
// part-groups (<= 32 slabs per thread, four at a time), where one thread per column used to walk all of them.
__global__ __launch_bounds__(1024) void stem_reduce_kernel(const float* __restrict__ partial, int nparts, float* dw, float* db,
                                                           int accumulate) {
    __shared__ double sq[16][64];
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);            // grid = 8: i < 512
    const float s = (float)column_sum_d<16>(partial, nparts, (size_t)512, i, true, sq);
    if (threadIdx.x >= 64) return;
    const int co = i >> 3, j = i & 7;
    float* dst = (j < 7) ? dw + co * 7 + j : db + co;
    *dst = accumulate ? *dst + s : s;
}

// ------------------------------------------------------------------------------------ head1
__global__ __launch_bounds__(256) void head1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ y, int T4,
                                                        int total4) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int b = i / T4, q = i % T4;
    const float4* xb = reinterpret_cast<const float4*>(x) + (size_t)b * 64 * T4 + q;
    const float b0 = bias[0];
    float4 o = make_float4(b0, b0, b0, b0);
#pragma unroll 8
    for (int c = 0; c < 64; ++c) {
        const float4 v = xb[(size_t)c * T4];
        const float wc = w[c];
        o.x = fmaf(wc, v.x, o.x); o.y = fmaf(wc, v.y, o.y); o.z = fmaf(wc, v.z, o.z); o.w = fmaf(wc, v.w, o.w);
    }
    reinterpret_cast<float4*>(y)[i] = o;
}

// head1 with the ResBlock tail in front of it: v = relu(x + y2*scale[c] + shift[c]) (bn_add_relu_kernel's expression, csrc/bn.hip)
// is formed here, stored to `out` (head1_bwd's saved input) and never read back; MASK: its sign bits in wm_bn_add_relu_mask's
// layout.  block = (clip, 1024-step tile), so that lane & 7 == q & 7 and eight lanes cover one mask word (merged by three lane
// exchanges, which need all 64 lanes: no early return, lanes past the clip work on a clamped address and store nothing).
// Channels go in groups of 8 with the group's loads issued first; the channel order into the one accumulator is head1_fwd_kernel's.
template <bool MASK>
__global__ __launch_bounds__(256) void head1_tail_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y2,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             float* __restrict__ out, unsigned* __restrict__ mask,
                                                             const float* __restrict__ w, const float* __restrict__ bias,
                                                             float* __restrict__ y, int T4) {
    const int tilesPerClip = (T4 + 255) / 256;
    const int b = blockIdx.x / tilesPerClip, q = (blockIdx.x % tilesPerClip) * 256 + (int)threadIdx.x;
    const bool ok = q < T4;
    const int lane = threadIdx.x & 63, nw = (T4 + 7) >> 3;
    const size_t base = (size_t)b * 64 * T4 + min(q, T4 - 1);
    const float4* x4 = reinterpret_cast<const float4*>(x) + base;
    const float4* y4 = reinterpret_cast<const float4*>(y2) + base;
    float4* o4 = reinterpret_cast<float4*>(out) + base;
    const float b0 = bias[0];
    float4 o = make_float4(b0, b0, b0, b0);
#pragma unroll 1
    for (int c0 = 0; c0 < 64; c0 += 8) {
        float4 a[8], r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { a[k] = stream_load(x4 + (size_t)(c0 + k) * T4); r[k] = stream_load(y4 + (size_t)(c0 + k) * T4); }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = c0 + k;
            const float sc = scale[c], sh = shift[c], wc = w[c];
            float4 v;
            v.x = fmaxf(a[k].x + fmaf(r[k].x, sc, sh), 0.f);
            v.y = fmaxf(a[k].y + fmaf(r[k].y, sc, sh), 0.f);
            v.z = fmaxf(a[k].z + fmaf(r[k].z, sc, sh), 0.f);
            v.w = fmaxf(a[k].w + fmaf(r[k].w, sc, sh), 0.f);
            if (ok) stream_store(o4 + (size_t)c * T4, v);
            if (MASK) {
                unsigned m = ((v.x > 0.f) ? 1u : 0u) | ((v.y > 0.f) ? 2u : 0u) | ((v.z > 0.f) ? 4u : 0u) | ((v.w > 0.f) ? 8u : 0u);
                m = ok ? m << (4 * (lane & 7)) : 0u;
                m |= __shfl_xor(m, 1); m |= __shfl_xor(m, 2); m |= __shfl_xor(m, 4);
                if ((lane & 7) == 0 && ok) mask[((size_t)b * 64 + c) * nw + (q >> 3)] = m;
            }
            o.x = fmaf(wc, v.x, o.x); o.y = fmaf(wc, v.y, o.y); o.z = fmaf(wc, v.z, o.z); o.w = fmaf(wc, v.w, o.w);
        }
    }
    if (ok) reinterpret_cast<float4*>(y)[(size_t)b * T4 + q] = o;
}

// dx[c,t] = w[c] g[t];  dw[c] = sum g[t] x[c,t];  db = sum g   -> partial[block][65]
// DX = false: dx is not written (its readers rebuild w[c] g[t] on load: wm_relu_bwd_reduce_mask_r1, wm_dwgrad64_bf_r1); the loop, the
// grid and the order of acc[] are the same, so dw and db keep their bits.
template <bool DX>
__global__ __launch_bounds__(256) void head1_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                        const float* __restrict__ w, float* __restrict__ dx,
                                                        float* __restrict__ partial, int T4, int total4) {
    __shared__ float red[4][65];
    float acc[65];
#pragma unroll
    for (int c = 0; c < 65; ++c) acc[c] = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total4; i += gridDim.x * 256) {
        const int b = i / T4, q = i % T4;
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        const size_t base = (size_t)b * 64 * T4 + q;
        acc[64] += (gv.x + gv.y) + (gv.z + gv.w);
#pragma unroll
        for (int c = 0; c < 64; ++c) {
            const float4 v = reinterpret_cast<const float4*>(x)[base + (size_t)c * T4];
            acc[c] += fmaf(gv.x, v.x, gv.y * v.y) + fmaf(gv.z, v.z, gv.w * v.w);
            if (DX) {
                const float wc = w[c];
                reinterpret_cast<float4*>(dx)[base + (size_t)c * T4] = make_float4(wc * gv.x, wc * gv.y, wc * gv.z, wc * gv.w);
            }
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 65; ++c) {
        const float v = wave_sum(acc[c]);
        if (lane == 0) red[wv][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < 65)
        partial[(size_t)blockIdx.x * 65 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// ------------------------------------------------------------------------------------ headN
// i / d for 0 <= i <= 2^14 and 2 <= d <= 64, with magic = ceil(2^32 / d): the error i * (magic - 2^32/d) / 2^32 < 2^-18 stays
// below the 1/d gap between i/d and the next integer
__device__ __forceinline__ int div_small(int i, unsigned magic) { return (int)__umulhi((unsigned)i, magic); }

// logits[r,t,o] = bias[o] + sum_c w[o][c] v[r,c,t]     NO = 1 + message_bits
// One thread = one time step: its 64 channel values sit in registers and every weight is a wave-uniform scalar
// operand (s_load through the scalar cache) -- the first version broadcast the weights through LDS reads, whose
// return path (64 lanes x 16 B per read) bounded the kernel at half the HBM rate.
// NOC > 0: the width is a compile-time constant (1 and 17: the 0- and 16-bit models).  NOC == 0: a run-time width 2 <= no <= 64 with
// magic = ceil(2^32 / no); the loop over outputs is then not unrolled or software-pipelined (either keeps more weights live than
// there are scalar registers and spills) and the staging rows get the odd stride no | 1 (a row stride of 32 or 64 floats would put
// every lane's store on one bank).
// TAIL: v = relu(x + y2*scale[c] + shift[c]), the ResBlock tail in bn_add_relu_kernel's own expression (csrc/bn.hip), formed here in
//   groups of 16 channels (the group's loads first, then its tail and stores) and stored to `out` -- headN_bwd's saved input, never
//   read back in forward.  mask (optional): the sign bits in wm_bn_add_relu_mask's layout; a wave's ballot of v > 0 IS words
//   t / 32, t / 32 + 1 of one row; lane c keeps channel c's pair and writes it at the end.  Lanes past T (clamped address) add zero
//   bits and store nothing.  Else v = x.
// LOSS: both BCE sums of bce_fwd_kernel (csrc/losses.hip) from the logits the thread holds: partial[block] = sum of the detection
//   terms (output 0, label 1 for rows < BL), partial[gridDim.x + block] = sum of the bit terms (outputs >= 1 of rows < BL).
template <int NOC, bool TAIL, bool LOSS>
__global__ __launch_bounds__(256) void headN_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y2,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        float* __restrict__ out, unsigned* __restrict__ mask,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ y, const long long* __restrict__ message, int BL,
                                                        float* __restrict__ partial, int T, int no, unsigned magic) {
    extern __shared__ float os[];                                // [256][OS]
    __shared__ float scratch[8];
    const int NO = NOC > 0 ? NOC : no, OS = NOC > 0 ? NOC : (no | 1);
    const int tilesPerClip = (T + 255) / 256;
    const int b = blockIdx.x / tilesPerClip, t0 = (blockIdx.x % tilesPerClip) * 256;
    const bool valid = t0 + (int)threadIdx.x < T;
    const int t = min(t0 + (int)threadIdx.x, T - 1);           // clamped: lanes past T compute a copy that is never stored
    const size_t base = (size_t)b * 64 * T + t;
    float v[64];
    if constexpr (TAIL) {
        const int lane = threadIdx.x & 63;
        unsigned mlo = 0u, mhi = 0u;
#pragma unroll
        for (int c0 = 0; c0 < 64; c0 += 16) {
            float xa[16], ya[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) { xa[k] = stream_load(x + base + (size_t)(c0 + k) * T); ya[k] = stream_load(y2 + base + (size_t)(c0 + k) * T); }
#pragma unroll
            for (int k = 0; k < 16; ++k) v[c0 + k] = fmaxf(xa[k] + fmaf(ya[k], scale[c0 + k], shift[c0 + k]), 0.f);
            if (valid) {
#pragma unroll
                for (int k = 0; k < 16; ++k) stream_store(out + base + (size_t)(c0 + k) * T, v[c0 + k]);
            }
            if (mask) {
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const unsigned long long bal = __ballot(valid && v[c0 + k] > 0.f);
                    if (lane == c0 + k) { mlo = (unsigned)bal; mhi = (unsigned)(bal >> 32); }
                }
            }
        }
        if (mask) {
            const int nw = (T + 31) >> 5, w0 = (t0 >> 5) + 2 * (int)(threadIdx.x >> 6);
            unsigned* mrow = mask + ((size_t)b * 64 + lane) * nw;
            if (w0 < nw) mrow[w0] = mlo;
            if (w0 + 1 < nw) mrow[w0 + 1] = mhi;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 64; ++c) v[c] = x[base + (size_t)c * T];
    }
    float sl = 0.f, sb = 0.f, yl = 0.f;
    long long msg = 0;
    if constexpr (LOSS) {
        if (b < BL) { msg = message[b]; yl = 1.f; }
    }
    auto one_output = [&](int o) {
        const float* wo = w + o * 64;                            // uniform address: scalar loads
        float a0 = bias[o], a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int c = 0; c < 64; c += 4) {
            a0 = fmaf(wo[c], v[c], a0); a1 = fmaf(wo[c + 1], v[c + 1], a1);
            a2 = fmaf(wo[c + 2], v[c + 2], a2); a3 = fmaf(wo[c + 3], v[c + 3], a3);
        }
        const float lg = (a0 + a1) + (a2 + a3);
        os[threadIdx.x * OS + o] = lg;
        if constexpr (LOSS) {
            const float term = valid ? bce_logits(lg, o == 0 ? yl : (float)((msg >> ((o - 1) & 63)) & 1)) : 0.f;
            if (o == 0) sl += term;
            else if (b < BL) sb += term;
        }
    };
    if constexpr (NOC > 0) {
#pragma unroll
        for (int o = 0; o < NOC; ++o) one_output(o);
    } else {
#pragma unroll 1
        for (int o = 0; o < no; ++o) {
            __builtin_amdgcn_sched_barrier(0);                  // keep the next output's 64 weights from being hoisted
            one_output(o);
        }
    }
    __syncthreads();
    const int nvalid = min(256, T - t0) * NO;
    float* yb = y + ((size_t)b * T + t0) * NO;
    for (int i = threadIdx.x; i < nvalid; i += 256) {
        if constexpr (NOC > 0) yb[i] = os[i];
        else { const int r = div_small(i, magic); yb[i] = os[r * OS + (i - r * NO)]; }
    }
    if constexpr (LOSS) {
        sl = block_sum<4>(sl, scratch);
        sb = block_sum<4>(sb, scratch + 4);
        if (threadIdx.x == 0) { partial[blockIdx.x] = sl; partial[gridDim.x + blockIdx.x] = sb; }
    }
}

// g [B,T,NO] -> dx[b,c,t] = sum_o w[o][c] g[b,t,o];  dw[o][c] = sum g[b,t,o] x[b,c,t];  db[o] = sum g
// Both products run on the fp32 matrix cores (the VALU/LDS version spent 11.5 ms per step at B=256):
//   dx: M = channel (2 tiles), N = time (the wave's 64 steps), K = output index padded to even
//   dw: M = output index padded to 32*NT (NT tiles), N = channel (2 tiles), K = time; accumulators persist over tiles
// NOC > 0: the width is a compile-time constant (1 and 17: the 0- and 16-bit models, NT = 1).  NOC == 0: any width
// 2 <= no <= 32*NT, given at run time with magic = ceil(2^32 / no) for the tile scatter.
// partial[block][NO*64 + NO]
// DL: g holds the LOGITS, and the gradient of g_loc * loc + g_bce * bce is formed from them while the tile is staged -- element for
// element what bce_bwd_kernel (csrc/losses.hip) would have written (rows < BL carry a message and the label 1), so neither that
// launch nor its [B,T,NO] tensor exists.  Everything behind the staging is the same code on the same values.
template <int NOC, int NT, bool DL>
__global__ __launch_bounds__(256) void headN_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                        const float* __restrict__ w, float* __restrict__ dx,
                                                        float* __restrict__ partial, int B, int T, int no, unsigned magic,
                                                        const long long* __restrict__ message, const float* __restrict__ g_loc,
                                                        const float* __restrict__ g_bce, int BL) {
    constexpr int XS = 257, OB = 32 * NT, GS = OB + 1;
    constexpr int NOMAX = NOC > 0 ? NOC : OB;
    const int NO = NOC > 0 ? NOC : no;
    const int KS = (NO + 1) / 2;                 // k-steps of the dx product
    float kl = 0.f, kb = 0.f;                    // DL: the scales of bce_bwd_kernel
    if constexpr (DL) {
        kl = g_loc[0] / (float)((double)B * T);
        kb = (NO > 1) ? g_bce[0] / (float)((double)BL * T * (NO - 1)) : 0.f;
    }
    extern __shared__ __align__(16) float smem[];
    float* xs = smem;                  // [64][XS]
    float* gsm = xs + 64 * XS;         // [256][GS], columns >= NO are zero
    float* ws = gsm + 256 * GS;        // [OB][64],  rows >= NO are zero
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    for (int i = tid; i < OB * 64; i += 256) ws[i] = (i < NO * 64) ? w[i] : 0.f;
    for (int i = tid; i < 256 * GS; i += 256) gsm[i] = 0.f;
    const int tilesPerClip = (T + 255) / 256, ntiles = B * tilesPerClip;
    f32x16 accw[NT][2];
#pragma unroll
    for (int mt = 0; mt < NT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { accw[mt][0][r] = 0.f; accw[mt][1][r] = 0.f; }
    float accb = 0.f;
    // next tile is fetched into registers (16-B loads, clamped addresses, no branches) while this one is processed
    constexpr int NG4 = (256 * NOMAX + 3) / 4, NGV = (NG4 + 255) / 256;
    float4 sx[16], sgv[NGV];
    // piece p of the staging: 0..15 x rows, 16.. the g tile.  The main loop issues one piece per k-step of the dw product
    // (an 81-KB burst would block the wave at issue, see conv64bf3_kernel)
    auto load_piece = [&](int tile, int p) {
        const int b = tile / tilesPerClip, t0 = (tile % tilesPerClip) * 256;
        if (p < 16) {
            const int i = tid + p * 256, c = i >> 6, q = i & 63;
            sx[p] = *reinterpret_cast<const float4*>(x + ((size_t)b * 64 + c) * T + min(t0 + 4 * q, T - 4));
        } else {
            // the g tile is 256*NO contiguous floats starting at a 16-B aligned address (t0 % 256 == 0, T % 4 == 0)
            const float4* gb4 = reinterpret_cast<const float4*>(g + ((size_t)b * T + t0) * NO);
            const int lim4 = ((T - t0 < 256 ? T - t0 : 256) * NO) / 4;        // whole float4s available in this clip
            sgv[p - 16] = gb4[min(tid + (p - 16) * 256, lim4 - 1)];
        }
    };
    auto load_tile = [&](int tile) {
#pragma unroll
        for (int p = 0; p < 16 + NGV; ++p) load_piece(tile, p);
    };
    auto write_tile = [&](int tile) {
        const int t0 = (tile % tilesPerClip) * 256;
        const int nt = min(256, T - t0);
        const int row = tile / tilesPerClip;
        long long msg = 0;
        if constexpr (DL) msg = (row < BL) ? message[row] : 0;
        const float yl = row < BL ? 1.f : 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int i = tid + k * 256, c = i >> 6, q = i & 63;
            float4 v = sx[k];
            if (4 * q >= nt) v = make_float4(0.f, 0.f, 0.f, 0.f);
            float* d = xs + c * XS + 4 * q;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
#pragma unroll
        for (int k = 0; k < NGV; ++k) {
            const int f = tid + k * 256;
            if (f < NG4) {
                const float e[4] = {sgv[k].x, sgv[k].y, sgv[k].z, sgv[k].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = 4 * f + j;
                    if (i < 256 * NO) {
                        const int r = NOC > 0 ? i / NO : div_small(i, magic), o = i - r * NO;
                        float val = e[j];
                        if constexpr (DL) {
                            if (o == 0) val = bce_logits_grad(val, yl, kl);
                            else val = (row < BL) ? bce_logits_grad(val, (float)((msg >> (o - 1)) & 1), kb) : 0.f;
                        }
                        gsm[r * GS + o] = (i < nt * NO) ? val : 0.f;
                    }
                }
            }
        }
    };
    int tile = blockIdx.x;
    if (tile < ntiles) load_tile(tile);
    __syncthreads();                       // ws / gsm zero fill visible
    if (tile < ntiles) write_tile(tile);
    __syncthreads();
    while (tile < ntiles) {
        const int next = tile + gridDim.x, nextc = min(next, ntiles - 1);     // clamped: loaded (valid memory), never written
        const int b = tile / tilesPerClip, t0 = (tile % tilesPerClip) * 256;
        const int nt = min(256, T - t0);
        // ---- dx tile: D[c][t]
        {
            f32x16 acc[2][2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[mt][n2][r] = 0.f;
#pragma unroll
            for (int s = 0; s < (NOMAX + 1) / 2; ++s) {
                if (s < KS) {                      // always true at a compile-time width
                    const float a0 = ws[(2 * s + half) * 64 + l31], a1 = ws[(2 * s + half) * 64 + 32 + l31];
                    const float b0 = gsm[(wave * 64 + l31) * GS + 2 * s + half], b1 = gsm[(wave * 64 + 32 + l31) * GS + 2 * s + half];
                    acc[0][0] = mfma32(a0, b0, acc[0][0]); acc[0][1] = mfma32(a0, b1, acc[0][1]);
                    acc[1][0] = mfma32(a1, b0, acc[1][0]); acc[1][1] = mfma32(a1, b1, acc[1][1]);
                }
            }
            float* dxb = dx + (size_t)b * 64 * T + t0;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int c = mt * 32 + mfma_row(r, half), tt = wave * 64 + n2 * 32 + l31;
                        if (tt < nt) dxb[(size_t)c * T + tt] = acc[mt][n2][r];
                    }
        }
        // ---- dw: D[o][c] += sum over this wave's 64 steps
        {
            const float* ap = gsm + (wave * 64 + half) * GS + l31;
            const float* bp = xs + l31 * XS + wave * 64 + half;
#pragma unroll
            for (int s = 0; s < 32; ++s) {
                if (s < 16 + NGV) load_piece(nextc, s);
#pragma unroll
                for (int mt = 0; mt < NT; ++mt) {
                    const float a = ap[2 * s * GS + mt * 32];
                    accw[mt][0] = mfma32(a, bp[2 * s], accw[mt][0]);
                    accw[mt][1] = mfma32(a, bp[32 * XS + 2 * s], accw[mt][1]);
                }
            }
        }
        if ((tid & (OB - 1)) < NO) {       // bias sums: output tid % OB, OB-step segment tid / OB (short loops, not one long one)
            const float* gp = gsm + (tid / OB) * OB * GS + (tid & (OB - 1));
#pragma unroll 8
            for (int tt = 0; tt < OB; ++tt) accb += gp[tt * GS];
        }
        __syncthreads();
        if (next < ntiles) write_tile(next);
        __syncthreads();
        tile = next;
    }
    // fixed-order reduction of the four waves' dw tiles through LDS
    __syncthreads();
    float* red = xs;     // [OB][64]
    for (int wv = 0; wv < 4; ++wv) {
        if (wave == wv) {
#pragma unroll
            for (int mt = 0; mt < NT; ++mt)
#pragma unroll
                for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int o = mt * 32 + mfma_row(r, half), c = n2 * 32 + l31;
                        red[o * 64 + c] = (wv == 0) ? accw[mt][n2][r] : red[o * 64 + c] + accw[mt][n2][r];
                    }
        }
        __syncthreads();
    }
    float* out = partial + (size_t)blockIdx.x * (NO * 64 + NO);
    for (int i = tid; i < NO * 64; i += 256) out[i] = red[i];
    __syncthreads();
    red[tid] = ((tid & (OB - 1)) < NO) ? accb : 0.f;          // [256 / OB segments][OB]
    __syncthreads();
    if (tid < NO) {
        if constexpr (NT == 1)
            out[NO * 64 + tid] = ((red[tid] + red[32 + tid]) + (red[64 + tid] + red[96 + tid])) +
                                 ((red[128 + tid] + red[160 + tid]) + (red[192 + tid] + red[224 + tid]));
        else
            out[NO * 64 + tid] = (red[tid] + red[64 + tid]) + (red[128 + tid] + red[192 + tid]);
    }
}

}  // namespace

extern "C" {

int wm_stem_fwd(const float* s, const float* w, const float* bias, float* y, int B, int T, hipStream_t stream) {
    if (T & 3) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(stem_fwd_kernel, dim3(B * ((T + 1023) / 1024)), dim3(256), 0, stream, s, w, bias, y, T);
    WM_CHECK_LAUNCH();
    return 0;
}

#ifndef WM_STEM_WGS_PER_CU
#define WM_STEM_WGS_PER_CU 2      // 71 KB of LDS per workgroup: two fit a CU, one's matrix phase runs under the other's loads / ds phase
#endif
// partial: >= 512*512 floats of scratch.  ds may be NULL (Generator stem: the clip is data); only clips [0, nds) get a ds row
// (Detector stem: the clean half of [watermarked; clean] needs no input gradient).
int wm_stem_bwd(const float* g, const float* s, const float* w, float* ds, float* partial, float* dw, float* db, int B,
                int T, int nds, int accumulate, hipStream_t stream) {
    if (T & 3) return (int)hipErrorInvalidValue;
    constexpr size_t lds = (size_t)(64 * 264 + 296 + 4 * 256) * sizeof(float);
    static wm::DevOnce attr_done;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(stem_bwd_kernel), lds, attr_done)) return rc;
    const int ntiles = B * ((T + 255) / 256);
    const int grid = ntiles < WM_STEM_WGS_PER_CU * kNumCU ? ntiles : WM_STEM_WGS_PER_CU * kNumCU;
    hipLaunchKernelGGL(stem_bwd_kernel, dim3(grid), dim3(256), lds, stream, g, s, w, ds, partial, B, T, nds);
    WM_CHECK_LAUNCH();
    hipLaunchKernelGGL(stem_reduce_kernel, dim3(8), dim3(1024), 0, stream, (const float*)partial, grid, dw, db, accumulate);
    WM_CHECK_LAUNCH();
    return 0;
}

int wm_head1_fwd(const float* x, const float* w, const float* bias, float* y, int B, int T, hipStream_t stream) {
    if (T & 3) return (int)hipErrorInvalidValue;
    const int total4 = B * (T / 4);
    hipLaunchKernelGGL(head1_fwd_kernel, dim3((total4 + 255) / 256), dim3(256), 0, stream, x, w, bias, y, T / 4, total4);
    WM_CHECK_LAUNCH();
    return 0;
}

// wm_bn_add_relu(_mask) + wm_head1_fwd in one launch: out = relu(x + y2*scale + shift) is written once and not read back
int wm_head1_tail_fwd(const float* x, const float* y2, const float* scale, const float* shift, const float* w, const float* bias,
                      float* out, void* mask, float* y, int B, int T, hipStream_t stream) {
    if ((T & 3) || B <= 0 || !y2 || !out) return (int)hipErrorInvalidValue;
    const int T4 = T / 4, grid = B * ((T4 + 255) / 256);
    if (mask) hipLaunchKernelGGL(head1_tail_fwd_kernel<true>, dim3(grid), dim3(256), 0, stream, x, y2, scale, shift, out, (unsigned*)mask, w, bias, y, T4);
    else hipLaunchKernelGGL(head1_tail_fwd_kernel<false>, dim3(grid), dim3(256), 0, stream, x, y2, scale, shift, out, (unsigned*)nullptr, w, bias, y, T4);
    WM_CHECK_LAUNCH();
    return 0;
}

// partial: >= 1024*65 floats.  dwb: [65] = dw[64] followed by db[1] (two separate tensors on the host side).  dx == NULL: dw and db only.
int wm_head1_bwd(const float* g, const float* x, const float* w, float* dx, float* partial, float* dw, float* db, int B,
                 int T, int accumulate, hipStream_t stream) {
    if (T & 3) return (int)hipErrorInvalidValue;
    const int total4 = B * (T / 4);
    int grid = (total4 + 255) / 256;
    if (grid > 1024) grid = 1024;
    if (dx) hipLaunchKernelGGL(head1_bwd_kernel<true>, dim3(grid), dim3(256), 0, stream, g, x, w, dx, partial, T / 4, total4);
    else hipLaunchKernelGGL(head1_bwd_kernel<false>, dim3(grid), dim3(256), 0, stream, g, x, w, dx, partial, T / 4, total4);
    WM_CHECK_LAUNCH();
    // partial [grid][65]: first 64 -> dw, last -> db
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, stream, (const float*)partial, grid, 65, 64, dw, accumulate);
    WM_CHECK_LAUNCH();
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, stream, (const float*)partial + 64, grid, 65, 1, db, accumulate);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"

namespace {
struct HeadNFwd {
    const float *x, *y2, *scale, *shift, *w, *bias;
    float *out, *y, *partial;
    unsigned* mask;
    const long long* message;
    int BL, R, T, NO;
};
template <int NOC, bool TAIL, bool LOSS>
int launch_headN_fwd(const HeadNFwd& a, hipStream_t stream) {
    const size_t lds = (size_t)256 * (NOC > 0 ? NOC : (a.NO | 1)) * sizeof(float);
    if constexpr (NOC == 0) {                                   // up to 65 KB of staging rows
        static wm::DevOnce done;
        if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(headN_fwd_kernel<NOC, TAIL, LOSS>), 256 * 65 * sizeof(float), done)) return rc;
    }
    const unsigned magic = (unsigned)((0x100000000ull + a.NO - 1) / a.NO);
    hipLaunchKernelGGL((headN_fwd_kernel<NOC, TAIL, LOSS>), dim3(a.R * ((a.T + 255) / 256)), dim3(256), lds, stream, a.x, a.y2, a.scale,
                       a.shift, a.out, a.mask, a.w, a.bias, a.y, a.message, a.BL, a.partial, a.T, a.NO, magic);
    WM_CHECK_LAUNCH();
    return 0;
}
// 1 and 17 run exact-width instantiations
template <bool TAIL, bool LOSS>
int launch_headN_fwd_width(const HeadNFwd& a, hipStream_t stream) {
    if (a.NO == 17) return launch_headN_fwd<17, TAIL, LOSS>(a, stream);
    if (a.NO == 1) return launch_headN_fwd<1, TAIL, LOSS>(a, stream);
    return launch_headN_fwd<0, TAIL, LOSS>(a, stream);
}
}  // namespace

extern "C" {

// NO = 1 + message_bits, 1 <= NO <= 64 (message ids are int64: at most 63 bits)
int wm_headN_fwd(const float* x, const float* w, const float* bias, float* y, int B, int T, int NO, hipStream_t stream) {
    if (NO < 1 || NO > 64 || B <= 0 || T <= 0) return (int)hipErrorInvalidValue;
    const HeadNFwd a{x, nullptr, nullptr, nullptr, w, bias, nullptr, y, nullptr, nullptr, nullptr, 0, B, T, NO};
    return launch_headN_fwd_width<false, false>(a, stream);
}

// The Detector head with what surrounds it (see headN_fwd_kernel): y2 != NULL -- the ResBlock tail in front (out, optional mask);
// message != NULL -- both BCE terms behind (partial: >= 2 * R * ceil(T / 256) floats; finished in fp64 and a fixed order with
// wm_bce_fwd's scales; NO == 1 leaves bce_out untouched, as wm_bce_fwd does)
int wm_headN_tail_fwd(const float* x, const float* y2, const float* scale, const float* shift, const float* w, const float* bias,
                      const long long* message, int B, float* partial, float* loc_out, float* bce_out, float* out, void* mask,
                      float* logits, int R, int T, int NO, hipStream_t stream) {
    if (NO < 1 || NO > 64 || R <= 0 || T <= 0) return (int)hipErrorInvalidValue;
    if (y2 && (!scale || !shift || !out)) return (int)hipErrorInvalidValue;
    if (message && (B < 0 || B > R || !partial || !loc_out || (NO > 1 && !bce_out))) return (int)hipErrorInvalidValue;
    const HeadNFwd a{x, y2, scale, shift, w, bias, out, logits, partial, y2 ? (unsigned*)mask : nullptr, message, B, R, T, NO};
    const int rc = y2 ? (message ? launch_headN_fwd_width<true, true>(a, stream) : launch_headN_fwd_width<true, false>(a, stream))
                      : (message ? launch_headN_fwd_width<false, true>(a, stream) : launch_headN_fwd_width<false, false>(a, stream));
    if (rc || !message) return rc;
    const int grid = R * ((T + 255) / 256);
    WM_TRY((hipError_t)wm::launch_sum_scale2(partial, grid, 1.0 / ((double)R * T), loc_out, stream));
    if (NO > 1) WM_TRY((hipError_t)wm::launch_sum_scale2(partial + grid, grid, 1.0 / ((double)B * T * (NO - 1)), bce_out, stream));
    return 0;
}

}  // extern "C"

namespace {
// NOC, NT, DL: see headN_bwd_kernel.  LDS: x tile [64][257], g tile [256][32*NT+1], weights [32*NT][64] -- 145.25 KB at NT = 2
struct HeadNBwd {
    const float *g, *x, *w;
    float *dx, *partial;
    const long long* message;           // DL: g = logits, with the three below
    const float *g_loc, *g_bce;
    int BL, R, T, NO;
};
template <int NOC, int NT, bool DL>
int launch_headN_bwd(const HeadNBwd& a, int grid, hipStream_t stream) {
    constexpr size_t lds = (size_t)(64 * 257 + 256 * (32 * NT + 1) + 32 * NT * 64) * sizeof(float);
    static wm::DevOnce done;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(headN_bwd_kernel<NOC, NT, DL>), lds, done)) return rc;
    const unsigned magic = a.NO > 1 ? (unsigned)((0x100000000ull + a.NO - 1) / a.NO) : 0u;
    hipLaunchKernelGGL((headN_bwd_kernel<NOC, NT, DL>), dim3(grid), dim3(256), lds, stream, a.g, a.x, a.w, a.dx, a.partial, a.R, a.T, a.NO,
                       magic, a.message, a.g_loc, a.g_bce, a.BL);
    WM_CHECK_LAUNCH();
    return 0;
}
template <bool DL>
int headN_bwd(const HeadNBwd& a, float* dw, float* db, int accumulate, hipStream_t stream) {
    const int NO = a.NO;
    if (NO < 1 || NO > 64) return (int)hipErrorInvalidValue;
    const int ntiles = a.R * ((a.T + 255) / 256);
    const int grid = ntiles < kNumCU ? ntiles : kNumCU;
    int rc;
    if (NO == 17) rc = launch_headN_bwd<17, 1, DL>(a, grid, stream);
    else if (NO == 1) rc = launch_headN_bwd<1, 1, DL>(a, grid, stream);
    else if (NO <= 32) rc = launch_headN_bwd<0, 1, DL>(a, grid, stream);
    else rc = launch_headN_bwd<0, 2, DL>(a, grid, stream);
    if (rc) return rc;
    const int n = NO * 64 + NO;
    // partial rows are [NO*64 weights | NO biases]; reduce the two pieces with matching row stride
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((NO * 64 + 63) / 64), dim3(256), 0, stream, (const float*)a.partial, grid, n, NO * 64, dw, accumulate);
    WM_CHECK_LAUNCH();
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, stream, (const float*)a.partial + NO * 64, grid, n, NO, db, accumulate);
    WM_CHECK_LAUNCH();
    return 0;
}
}  // namespace

extern "C" {

// partial: >= 256*(NO*64+NO) floats (one row per workgroup, at most one workgroup per CU)
int wm_headN_bwd(const float* g, const float* x, const float* w, float* dx, float* partial, float* dw, float* db, int B,
                 int T, int NO, int accumulate, hipStream_t stream) {
    const HeadNBwd a{g, x, w, dx, partial, nullptr, nullptr, nullptr, 0, B, T, NO};
    return headN_bwd<false>(a, dw, db, accumulate, stream);
}

// wm_bce_bwd + wm_headN_bwd in one launch: the gradient of g_loc * loc + g_bce * bce w.r.t. the logits [R,T,NO] is formed while
// the logits are staged (rows < B carry message[row] and the label 1); no dlogits tensor
int wm_headN_bwd_bce(const float* logits, const long long* message, const float* g_loc, const float* g_bce, const float* x,
                     const float* w, float* dx, float* partial, float* dw, float* db, int B, int R, int T, int NO, int accumulate,
                     hipStream_t stream) {
    if (!message || !g_loc || !g_bce || B < 0 || B > R) return (int)hipErrorInvalidValue;
    const HeadNBwd a{logits, x, w, dx, partial, message, g_loc, g_bce, B, R, T, NO};
    return headN_bwd<true>(a, dw, db, accumulate, stream);
}

}  // extern "C"
