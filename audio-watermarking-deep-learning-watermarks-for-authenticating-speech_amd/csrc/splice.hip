// The editing attack and what localisation needs: a splice of unmarked audio into the watermarked signal that also emits per-sample
// labels (wm_splice / wm_splice_bwd), both detection losses against those labels (wm_bce_masked_fwd / _bwd) and the confusion counts of
// the per-sample prediction (wm_loc_score).  include/wm_hip.h has the definitions.
//
// Labels travel as bit masks: lab (rows, W = ceil(n / 32)) uint32, bit j of word w of row r is sample 32 w + j of row r, 1 = "still
// watermarked", bits at t >= n are zero.  Whoever produces a mask forms it with a wave ballot: lane l of a wave looks at sample t0 + l,
// the 64 predicates are two words, lane 0 stores the low one and lane 32 the high one.  One writer per word and per sample, so no
// read-modify-write anywhere and every result is a function of the arguments alone.
//
// wm_splice.  The spans of a row are drawn by the first lanes of the workgroup (two Philox4x32-10 calls per span, integer geometry, the
// three probability thresholds compared in fp64) into LDS once per chunk of kChunk samples; the chunk's labels are then balloted 64
// samples per wave, and its samples copied as in wm_distort's apply kernel: a lane owns a group of 4 samples on a 16-byte boundary of
// the OUTPUT, stored as one 16-byte access wherever the whole group lies inside the row; a and b are read the same way when they share
// the output's alignment, and only where the group needs them; "moved" samples are gathered one by one.  Samples are selected, never
// computed with: every value leaves with the bits it came with.
//
// wm_bce_masked_*.  wm_bce_fwd's and wm_bce_bwd's kernels (csrc/losses.hip) with the target of channel 0 read from the mask and the
// bit terms gated by it: the same chunks of 4096 elements, the same fp32 partial per workgroup, the same fp64 finish in a fixed order.
// N1, the number of set label bits, is counted in integers (per workgroup at channel 0, added by the finish) and stays on the device
// for the finish and the backward.  A workgroup's label words (at most 128) are staged in LDS once.
#include <cmath>
#include "wm_draw.hpp"
using namespace wm;

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 4096;                    // samples of a row one workgroup handles between two draws of the spans (a multiple of 64)
constexpr int kTile = kThreads * 4;
constexpr int kMaxSpans = 8;

struct Cut { int max_spans, len_lo, len_hi; double p_span, t_original, t_silence; };
struct Span { int start, end, kind, shift; };   // [start, end) is empty for a span that is not active; kind 0 original | 1 silence | 2 moved

// span j of row `row` (= row0 + r): counters (0xFFFFFFFB - 2j, ~0, row, draw) and (0xFFFFFFFA - 2j, ~0, row, draw)
__device__ __forceinline__ Span draw_span(const Rng& g, const Cut& c, unsigned row, int j, int n) {
    unsigned o[4], p[4];
    philox4x32_10(0xFFFFFFFBu - 2u * (unsigned)j, 0xFFFFFFFFu, row, g.draw, g.k0, g.k1, o);
    philox4x32_10(0xFFFFFFFAu - 2u * (unsigned)j, 0xFFFFFFFFu, row, g.draw, g.k0, g.k1, p);
    Span s{0, 0, 0, 0};
    if (!(unit_d(o[0]) < c.p_span)) return s;
    const int L = c.len_lo + (int)(((unsigned long long)(o[1] >> 9) * (unsigned long long)(c.len_hi - c.len_lo + 1)) >> 23);
    s.start = (int)(((unsigned long long)(o[2] >> 9) * (unsigned long long)(n - L + 1)) >> 23);
    s.end = s.start + L;
    const double u = unit_d(o[3]);
    s.kind = u < c.t_original ? 0 : (u < c.t_silence ? 1 : 2);
    s.shift = 1 + (int)(((unsigned long long)(p[0] >> 9) * (unsigned long long)(n - 1)) >> 23);
    if (n == 1) s.kind = s.kind == 2 ? 0 : s.kind;                     // nowhere to move from
    return s;
}

// the largest j whose span holds t, or -1
__device__ __forceinline__ int span_of(const Span* __restrict__ sp, int nsp, int t) {
    int hit = -1;
    for (int j = 0; j < nsp; ++j) hit = (t >= sp[j].start && t < sp[j].end) ? j : hit;
    return hit;
}

// the two words of a wave's 64 predicates (sample t0 + lane, t0 a multiple of 64) into row `lrow` of a mask of W words
__device__ __forceinline__ void store_ballot(unsigned* __restrict__ lrow, int W, int t0, bool pred) {
    const unsigned long long m = __ballot(pred);
    const int lane = threadIdx.x & 63, w = (t0 >> 5) + (lane >> 5);
    if ((lane & 31) == 0 && w < W) lrow[w] = lane ? (unsigned)(m >> 32) : (unsigned)m;
}

__global__ __launch_bounds__(kThreads) void splice_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y,
                                                          unsigned* __restrict__ lab, int n, int W, long long chunks_per_row,
                                                          long long chunks, Rng g, Cut c) {
    __shared__ Span sp[kMaxSpans];
    const int tid = threadIdx.x;
    for (long long ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const long long r = ch / chunks_per_row;
        const int c0 = (int)(ch - r * chunks_per_row) * kChunk;        // a multiple of 64; < n
        const long long base = r * (long long)n;
        __syncthreads();                                               // the spans of the chunk before are no longer read
        if (tid < c.max_spans) sp[tid] = draw_span(g, c, (unsigned)(g.row0 + r), tid, n);
        __syncthreads();
        const int nsp = c.max_spans;
        // labels: whole waves walk the chunk, 64 samples each, up to the last word that has a sample
        const int lab_end = min(c0 + kChunk, (n + 63) & ~63);
        for (int t = c0 + tid; t < lab_end; t += kThreads)
            store_ballot(lab + r * W, W, t - (tid & 63), t < n && span_of(sp, nsp, t) < 0);
        // samples: groups of 4 on 16-byte boundaries of y; this chunk takes the groups that START in [c0, c0 + kChunk) (the first chunk
        // also the one that starts before the row), so every sample has one writer
        const int ob = (int)((((uintptr_t)y >> 2) + (unsigned long long)base) & 3);
        for (int k = tid; k < kChunk / 4 + 1; k += kThreads) {
            const int t0 = c0 + 4 * k - ob;                            // k = kChunk / 4 belongs to the next chunk unless ob != 0 ...
            if (t0 >= n || t0 >= c0 + kChunk || (t0 < c0 && c0 != 0)) continue;   // ... in which case group 0 of that chunk started before it
            int hit[4];
            bool any_a = false, any_b = false;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int t = t0 + e;
                hit[e] = (t >= 0 && t < n) ? span_of(sp, nsp, t) : -1;
                any_a |= hit[e] < 0;
                any_b |= hit[e] >= 0 && sp[hit[e]].kind == 0;
            }
            float va[4] = {0.f, 0.f, 0.f, 0.f}, vb[4] = {0.f, 0.f, 0.f, 0.f}, out[4];
            if (any_a) load4(a, base, t0, n, aligned16(a, base + t0), va);
            if (any_b) load4(b, base, t0, n, aligned16(b, base + t0), vb);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = va[e];
                if (hit[e] >= 0) {
                    const Span s = sp[hit[e]];
                    if (s.kind == 0) v = vb[e];
                    else if (s.kind == 1) v = 0.f;
                    else {
                        int src = t0 + e + s.shift;                    // shift <= n - 1: one subtraction wraps
                        src -= src >= n ? n : 0;
                        v = b[base + src];
                    }
                }
                out[e] = v;
            }
            store4(y, base, t0, n, out);
        }
    }
}

// da = dy where the label bit is set, else +0
__global__ __launch_bounds__(kThreads) void splice_bwd_kernel(const float* __restrict__ dy, const unsigned* __restrict__ lab,
                                                              float* __restrict__ da, int n, int W, long long tiles_per_row, long long tiles) {
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r = tile / tiles_per_row;
        const long long base = r * (long long)n;
        const int ob = (int)((((uintptr_t)da >> 2) + (unsigned long long)base) & 3);
        const int t0 = (int)(tile - r * tiles_per_row) * kTile + 4 * (int)threadIdx.x - ob;
        if (t0 >= n) continue;
        const unsigned* __restrict__ lrow = lab + r * W;
        const int w0 = max(t0, 0) >> 5, w1 = min(t0 + 3, n - 1) >> 5;
        const unsigned m0 = lrow[w0], m1 = w1 != w0 ? lrow[w1] : m0;
        float v[4], out[4];
        load4(dy, base, t0, n, aligned16(dy, base + t0), v);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int t = t0 + e;
            const unsigned m = (t >> 5) == w0 ? m0 : m1;
            out[e] = (t >= 0 && t < n && ((m >> (t & 31)) & 1u)) ? v[e] : 0.f;
        }
        store4(da, base, t0, n, out);
    }
}

// ---------------------------------------------------------------------------------------------- masked detection losses
// idx = q * n + rem for 0 <= idx < 2^23 from a float reciprocal with a fix-up (csrc/losses.hip's mod_small, with the quotient)
__device__ __forceinline__ void divmod_small(int idx, int n, float inv_n, int& q, int& rem) {
    q = (int)((float)idx * inv_n);
    rem = idx - q * n;
    if (rem < 0) { rem += n; --q; }
    if (rem >= n) { rem -= n; ++q; }
}

constexpr int kLabWords = 4096 / 32 + 4;       // the label words one workgroup of the BCE kernels can need (NO = 1: 128)

// the label words of the samples t that the elements [blockIdx.x * 4096, + 4096) of a clip belong to, into LDS; returns the first word's
// index.  Rows without labels (marked false, the same for the whole workgroup) stage nothing and meet no barrier.  The forward kernel
// issues its 16 loads of logits BEFORE this, so the words' latency hides behind those loads instead of standing in front of them.
__device__ __forceinline__ int stage_labels(const unsigned* __restrict__ lrow, bool marked, int T, int NO, unsigned (&lw)[kLabWords]) {
    const int first = blockIdx.x * 4096;
    const int w_first = (first / NO) >> 5, w_last = min(T - 1, (first + 4095) / NO) >> 5;     // once per workgroup: plain divisions
    if (marked) {
        for (int i = threadIdx.x; i <= w_last - w_first && i < kLabWords; i += 256) lw[i] = lrow[w_first + i];
        __syncthreads();
    }
    return w_first;
}

// bce_fwd_kernel with the target of channel 0 and the gate of the bit terms read from the mask; ipartial[blk] = the set label bits the
// workgroup met (counted at channel 0, so every (r, t) once)
__global__ __launch_bounds__(256) void bce_masked_fwd_kernel(const float* __restrict__ logits, const long long* __restrict__ message,
                                                             const unsigned* __restrict__ lab, int B, int T, int NO, int W,
                                                             float* __restrict__ partial, int* __restrict__ ipartial) {
    __shared__ float scratch[8];
    __shared__ int iscratch[4];
    __shared__ unsigned lw[kLabWords];
    const int r = blockIdx.y, per_clip = T * NO;
    const float inv = 1.0f / (float)NO;
    const bool marked = r < B;
    const long long msg = marked ? message[r] : 0;
    const float* lp = logits + (size_t)r * per_clip;
    float xs[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int idx = blockIdx.x * 4096 + k * 256 + threadIdx.x;
        xs[k] = idx < per_clip ? lp[idx] : 0.f;
    }
    const int w_first = stage_labels(lab + (size_t)(marked ? r : 0) * W, marked, T, NO, lw);
    float sl = 0.f, sb = 0.f;
    int n1 = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int idx = blockIdx.x * 4096 + k * 256 + threadIdx.x;
        if (idx < per_clip) {
            int t, o;
            divmod_small(idx, NO, inv, t, o);
            const float x = xs[k];
            const bool on = marked && ((lw[(t >> 5) - w_first] >> (t & 31)) & 1u);
            if (o == 0) { sl += bce_logits(x, on ? 1.f : 0.f); n1 += on; }
            else if (on) sb += bce_logits(x, (float)((msg >> (o - 1)) & 1));
        }
    }
    sl = block_sum<4>(sl, scratch);
    sb = block_sum<4>(sb, scratch + 4);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n1 += __shfl_xor(n1, o);
    if ((threadIdx.x & 63) == 0) iscratch[threadIdx.x >> 6] = n1;
    __syncthreads();
    const int blk = blockIdx.y * gridDim.x + blockIdx.x, nblk = gridDim.x * gridDim.y;
    if (threadIdx.x == 0) {
        partial[blk] = sl;
        partial[nblk + blk] = sb;
        ipartial[blk] = (iscratch[0] + iscratch[1]) + (iscratch[2] + iscratch[3]);
    }
}

// N1 = sum of the integer partials -> count[0]; then, where out != NULL, sum_scale2_kernel (csrc/losses.hip) in its order with the scale
// 1 / (N1 (NO - 1)); N1 = 0: out = 0
__global__ __launch_bounds__(1024) void sum_scale_count_kernel(const float* __restrict__ partial, const int* __restrict__ ipartial, int n,
                                                               long long* __restrict__ count, int NO, float* out) {
    __shared__ double scratch[16];
    __shared__ long long iscratch[16];
    long long c = 0;
    for (int i = threadIdx.x; i < n; i += 1024) c += ipartial[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) iscratch[threadIdx.x >> 6] = c;
    __syncthreads();
    long long n1 = 0;
    if (threadIdx.x == 0) {
        for (int i = 0; i < 16; ++i) n1 += iscratch[i];
        count[0] = n1;
    }
    if (out == nullptr) return;                                       // the same for the whole workgroup
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int i = threadIdx.x;
    for (; i + 3072 < n; i += 4096) {
        const float v0 = partial[i], v1 = partial[i + 1024], v2 = partial[i + 2048], v3 = partial[i + 3072];
        s0 += (double)v0; s1 += (double)v1; s2 += (double)v2; s3 += (double)v3;
    }
    if (i < n) s0 += (double)partial[i];
    if (i + 1024 < n) s1 += (double)partial[i + 1024];
    if (i + 2048 < n) s2 += (double)partial[i + 2048];
    const double s = block_sum_d<16>((s0 + s1) + (s2 + s3), scratch);
    if (threadIdx.x == 0) out[0] = n1 > 0 ? (float)(s * (1.0 / ((double)n1 * (NO - 1)))) : 0.f;
}

__global__ __launch_bounds__(256) void bce_masked_bwd_kernel(const float* __restrict__ logits, const long long* __restrict__ message,
                                                             const unsigned* __restrict__ lab, const long long* __restrict__ count,
                                                             const float* __restrict__ g_loc, const float* __restrict__ g_bce,
                                                             int B, int R, int T, int NO, int W, float* __restrict__ dlogits) {
    __shared__ unsigned lw[kLabWords];
    const int r = blockIdx.y, per_clip = T * NO;
    const float inv = 1.0f / (float)NO;
    const long long n1 = count[0];
    const float kl = g_loc[0] / (float)((double)R * T);
    const float kb = (NO > 1 && n1 > 0) ? g_bce[0] / (float)((double)n1 * (NO - 1)) : 0.f;
    const bool marked = r < B;
    const long long msg = marked ? message[r] : 0;
    const float* lp = logits + (size_t)r * per_clip;
    float* dp = dlogits + (size_t)r * per_clip;
    // the words are staged IN FRONT of the loop here: with all 16 loads first, as in the forward kernel, a thread's 16 stores leave in one
    // burst and the pass was 13 % slower than wm_bce_bwd at B = 256; loads and stores interleaved four by four it is 2 % slower
    const int w_first = stage_labels(lab + (size_t)(marked ? r : 0) * W, marked, T, NO, lw);
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int idx = blockIdx.x * 4096 + k * 256 + threadIdx.x;
        if (idx < per_clip) {
            int t, o;
            divmod_small(idx, NO, inv, t, o);
            const float x = lp[idx];
            const bool on = marked && ((lw[(t >> 5) - w_first] >> (t & 31)) & 1u);
            float d;
            if (o == 0) d = bce_logits_grad(x, on ? 1.f : 0.f, kl);
            else d = (on && n1 > 0) ? bce_logits_grad(x, (float)((msg >> (o - 1)) & 1), kb) : 0.f;
            dp[idx] = d;
        }
    }
}

// ---------------------------------------------------------------------------------------------- localisation score
// one workgroup per row: prediction logits[r][t][0] > thr against the label bit; {tp, fp, fn, tn} as integers, pred as a mask
__global__ __launch_bounds__(kThreads) void loc_score_kernel(const float* __restrict__ logits, const unsigned* __restrict__ lab, float thr,
                                                             int* __restrict__ counts, unsigned* __restrict__ pred, int R, int T, int NO,
                                                             int W, int lab_rows) {
    __shared__ int red[kThreads / kWave][4];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int r = blockIdx.x; r < R; r += gridDim.x) {
        const float* __restrict__ lp = logits + (size_t)r * T * NO;
        const bool has = lab == nullptr || r < lab_rows;               // else every label is 0
        const unsigned* __restrict__ lrow = (lab != nullptr && has) ? lab + (size_t)r * W : nullptr;
        int tp = 0, fp = 0, fn = 0, tn = 0;                            // the same in every lane of a wave
        const int t_end = (T + 63) & ~63;
        for (int t = tid; t < t_end; t += kThreads) {
            const bool in = t < T;
            const bool p = in && lp[(size_t)t * NO] > thr;             // NaN: false
            const bool y = in && has && (lrow == nullptr || ((lrow[t >> 5] >> (t & 31)) & 1u));
            if (pred != nullptr) store_ballot(pred + (size_t)r * W, W, t - lane, p);
            tp += __popcll(__ballot(p && y));
            fp += __popcll(__ballot(p && !y && in));
            fn += __popcll(__ballot(!p && y));
            tn += __popcll(__ballot(!p && !y && in));
        }
        __syncthreads();                                               // the row before has been read out of red
        if (lane == 0) { red[tid >> 6][0] = tp; red[tid >> 6][1] = fp; red[tid >> 6][2] = fn; red[tid >> 6][3] = tn; }
        __syncthreads();
        if (tid < 4) {
            int s = 0;
#pragma unroll
            for (int w = 0; w < kThreads / kWave; ++w) s += red[w][tid];
            counts[4 * r + tid] = s;
        }
    }
}

bool rows_ok(long long rows, long long n) { return rows >= 1 && n >= 1 && n <= (1ll << 24) && rows <= (1ll << 46) / n; }

bool prob(float p) { return p >= 0.f && p <= 1.f; }                    // NaN: false

bool bce_shape_ok(int B, int R, int T, int NO) {
    return R >= 1 && R <= 65535 && B >= 0 && B <= R && T >= 1 && NO >= 1 && NO <= 64 && (long long)T * NO < (1 << 23);
}

}  // namespace

extern "C" {

int wm_splice(const float* a, const float* b, float* y, int* lab_, long long rows, long long n, long long row0, long long seed,
              long long draw, int max_spans, float p_span, long long len_lo, long long len_hi, float p_original, float p_silence,
              hipStream_t stream) {
    unsigned* lab = reinterpret_cast<unsigned*>(lab_);
    if (!rows_ok(rows, n) || row0 < 0 || row0 > (1ll << 32) - rows || draw < 0 || draw >= (1ll << 32)) return (int)hipErrorInvalidValue;
    if (!a || !b || !y || !lab || (uintptr_t)a % 4 || (uintptr_t)b % 4 || (uintptr_t)y % 4 || (uintptr_t)lab % 4) return (int)hipErrorInvalidValue;
    if (max_spans < 1 || max_spans > kMaxSpans || len_lo < 1 || len_lo > len_hi || len_hi > n) return (int)hipErrorInvalidValue;
    if (!prob(p_span) || !prob(p_original) || !prob(p_silence) || (double)p_original + (double)p_silence > 1.0) return (int)hipErrorInvalidValue;
    const long long W = (n + 31) / 32;
    const unsigned long long bytes = (unsigned long long)rows * (unsigned long long)n * 4, lbytes = (unsigned long long)rows * (unsigned long long)W * 4;
    if (overlap(y, bytes, a, bytes) || overlap(y, bytes, b, bytes) || overlap(lab, lbytes, a, bytes) || overlap(lab, lbytes, b, bytes) ||
        overlap(lab, lbytes, y, bytes))
        return (int)hipErrorInvalidValue;                                         // in place is refused
    const Rng g = make_rng(seed, draw, row0);
    const Cut c{max_spans, (int)len_lo, (int)len_hi, (double)p_span, (double)p_original, (double)p_original + (double)p_silence};
    const long long chunks_per_row = (n + kChunk - 1) / kChunk, chunks = rows * chunks_per_row;
    hipLaunchKernelGGL(splice_kernel, dim3(grid_for(chunks)), dim3(kThreads), 0, stream, a, b, y, lab, (int)n, (int)W, chunks_per_row, chunks, g, c);
    WM_CHECK_LAUNCH();
    return 0;
}

int wm_splice_bwd(const float* dy, const int* lab_, float* da, long long rows, long long n, hipStream_t stream) {
    const unsigned* lab = reinterpret_cast<const unsigned*>(lab_);
    if (!rows_ok(rows, n) || !dy || !lab || !da || (uintptr_t)dy % 4 || (uintptr_t)lab % 4 || (uintptr_t)da % 4) return (int)hipErrorInvalidValue;
    const long long W = (n + 31) / 32;
    const unsigned long long bytes = (unsigned long long)rows * (unsigned long long)n * 4, lbytes = (unsigned long long)rows * (unsigned long long)W * 4;
    if (overlap(da, bytes, dy, bytes) || overlap(da, bytes, lab, lbytes)) return (int)hipErrorInvalidValue;
    const long long tiles_per_row = (n + 3 + kTile - 1) / kTile, tiles = rows * tiles_per_row;
    hipLaunchKernelGGL(splice_bwd_kernel, dim3(grid_for(tiles)), dim3(kThreads), 0, stream, dy, lab, da, (int)n, (int)W, tiles_per_row, tiles);
    WM_CHECK_LAUNCH();
    return 0;
}

int wm_bce_masked_fwd(const float* logits, const long long* message, const int* lab_, float* partial, long long* count_out,
                      float* loc_out, float* bce_out, int B, int R, int T, int NO, hipStream_t stream) {
    const unsigned* lab = reinterpret_cast<const unsigned*>(lab_);
    if (!bce_shape_ok(B, R, T, NO) || !logits || !partial || !count_out || !loc_out || (NO > 1 && !bce_out)) return (int)hipErrorInvalidValue;
    if (B > 0 && (!message || !lab)) return (int)hipErrorInvalidValue;
    const int W = (T + 31) / 32, chunks = (T * NO + 4095) / 4096, grid = chunks * R;
    int* ipartial = reinterpret_cast<int*>(partial + 2 * (size_t)grid);            // behind the two float slabs
    hipLaunchKernelGGL(bce_masked_fwd_kernel, dim3(chunks, R), dim3(256), 0, stream, logits, message, lab, B, T, NO, W, partial, ipartial);
    WM_CHECK_LAUNCH();
    const int rc = launch_sum_scale2(partial, grid, 1.0 / ((double)R * T), loc_out, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(sum_scale_count_kernel, dim3(1), dim3(1024), 0, stream, (const float*)partial + grid, (const int*)ipartial, grid,
                       count_out, NO, NO > 1 ? bce_out : (float*)nullptr);
    WM_CHECK_LAUNCH();
    return 0;
}

int wm_bce_masked_bwd(const float* logits, const long long* message, const int* lab_, const long long* count, const float* g_loc,
                      const float* g_bce, float* dlogits, int B, int R, int T, int NO, hipStream_t stream) {
    const unsigned* lab = reinterpret_cast<const unsigned*>(lab_);
    if (!bce_shape_ok(B, R, T, NO) || !logits || !count || !g_loc || !g_bce || !dlogits) return (int)hipErrorInvalidValue;
    if (B > 0 && (!message || !lab)) return (int)hipErrorInvalidValue;
    const unsigned long long bytes = (unsigned long long)R * T * NO * 4;
    if (overlap(dlogits, bytes, logits, bytes)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(bce_masked_bwd_kernel, dim3((T * NO + 4095) / 4096, R), dim3(256), 0, stream, logits, message, lab, count, g_loc,
                       g_bce, B, R, T, NO, (T + 31) / 32, dlogits);
    WM_CHECK_LAUNCH();
    return 0;
}

int wm_loc_score(const float* logits, const int* lab_, float thr_logit, int* counts, int* pred_, int R, int T, int NO,
                 int lab_rows, hipStream_t stream) {
    const unsigned* lab = reinterpret_cast<const unsigned*>(lab_);
    unsigned* pred = reinterpret_cast<unsigned*>(pred_);
    if (R < 1 || T < 1 || NO < 1 || !logits || !counts || lab_rows < 0 || lab_rows > R || std::isnan(thr_logit)) return (int)hipErrorInvalidValue;
    if ((long long)R * T > (1ll << 46) / NO) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(loc_score_kernel, dim3(grid_for(R)), dim3(kThreads), 0, stream, logits, lab, thr_logit, counts, pred, R, T, NO,
                       (T + 31) / 32, lab_rows);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
