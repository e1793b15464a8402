// Per-clip detection scores of the Detector's logits (wm_clip_scores): the mean sigmoid of channel 0, the mean logit of every channel,
// exact vote counts, the decoded message words (majority of hard decisions, and the sign of the summed logits) and their bit errors
// against the embedded message.  include/wm_hip.h has the definition.
//
// Two launches, no atomics.  A row of T * NO floats is cut into chunks of kChunk ELEMENTS (not samples: a chunk boundary may fall inside
// a sample); kChunk is a constant, so the cut depends on (T, NO) alone.
//   clip_partial_kernel   one workgroup per (row, chunk), grid-stride.  The chunk goes through LDS: 16-byte loads wherever a whole
//       aligned group lies inside the chunk, placed so that the global group and the LDS quad share their alignment (element e of the
//       chunk sits at buf[mis + e], mis = the chunk's first address mod 16 bytes in floats).  The channel is the fastest axis, so the
//       threads then walk the chunk at a stride S = NO * floor(256 / NO): a thread's channel never changes, consecutive threads read
//       consecutive LDS words, and one thread keeps one fp32 sum and one integer count.  The S / NO threads of a channel are added by
//       the thread that owns the channel, four chains in a fixed order.  The sigmoid runs in a pass of its own over the chunk's
//       channel-0 elements alone (256 per step), so that no wave evaluates an exponential with 1 lane in NO active.
//       Out: fsum / icnt [chunk][NO] and psig [chunk].
//   clip_finish_kernel    one workgroup per row adds the row's partials over its chunks in fp64 (integers in 64 bits) in an order that
//       depends on the number of chunks alone, and forms prob, llr, votes, both words and the bit errors; the words are wave ballots.
// Where an element lands in LDS depends on the pointer's alignment, which element a thread adds does not: the bits are a function of
// the row's samples, T, NO, thr_logit and the message.
#include <cmath>
#include "wm_common.hpp"
using namespace wm;

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 8192;                    // elements of a row per workgroup: 32 KB of LDS, 8 16-byte loads per thread
constexpr int kQuads = kChunk / 4;
constexpr int kPerThread = kQuads / kThreads;
constexpr long long kGridCap = 8ll * kNumCU;

struct Partials { float* fsum; int* icnt; float* psig; };

__global__ __launch_bounds__(kThreads) void clip_partial_kernel(const float* __restrict__ logits, float thr, Partials out, int per_row,
                                                                int NO, long long nch, long long chunks) {
    __shared__ __attribute__((aligned(16))) float buf[kChunk + 4];
    __shared__ float ps[kThreads];
    __shared__ int pc[kThreads];
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const int per = kThreads / NO, S = per * NO;
    for (long long ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const long long r = ch / nch;
        const int c0 = (int)(ch - r * nch) * kChunk;                   // < per_row <= 2^30
        const int n_el = min(kChunk, per_row - c0);
        const float* __restrict__ src = logits + r * (long long)per_row + c0;
        const int mis = (int)(((uintptr_t)src >> 2) & 3);
        __syncthreads();                                               // the chunk before is no longer read from buf, ps, pc
        // quad q = buf[4q .. 4q + 3] = elements 4q - mis .. 4q - mis + 3; a thread whose eight quads all lie inside takes the plain path
        if (4 * tid - mis >= 0 && 4 * (tid + (kPerThread - 1) * kThreads) - mis + 4 <= n_el) {
            f32x4 v[kPerThread];
#pragma unroll
            for (int i = 0; i < kPerThread; ++i)
                v[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + (4 * (tid + i * kThreads) - mis)));
#pragma unroll
            for (int i = 0; i < kPerThread; ++i) *reinterpret_cast<f32x4*>(buf + 4 * (tid + i * kThreads)) = v[i];
        } else {
#pragma unroll 2
            for (int i = 0; i < kPerThread; ++i) {
                const int q = tid + i * kThreads, e0 = 4 * q - mis;
                if (e0 >= n_el) break;
                f32x4 v;
                if (e0 >= 0 && e0 + 4 <= n_el) {
                    v = *reinterpret_cast<const f32x4*>(src + e0);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = (e0 + j >= 0 && e0 + j < n_el) ? src[e0 + j] : 0.f;
                }
                *reinterpret_cast<f32x4*>(buf + 4 * q) = v;
            }
        }
        if (tid < mis && kChunk - mis + tid < n_el) buf[kChunk + tid] = src[kChunk - mis + tid];       // the quad behind the last one
        __syncthreads();
        const float* __restrict__ el = buf + mis;
        const int ph = c0 % NO;                                        // the channel of element 0 of the chunk
        // sums and votes: thread tid < S owns the elements tid, tid + S, ... -- all of channel (ph + tid) mod NO
        float s = 0.f;
        int c = 0;
        if (tid < S) {
            const float th = (ph + tid) % NO == 0 ? thr : 0.f;
#pragma unroll 4
            for (int e = tid; e < n_el; e += S) {
                const float x = el[e];
                s += x;
                c += x > th ? 1 : 0;                                   // NaN: no vote
            }
        }
        ps[tid] = s;
        pc[tid] = c;
        // the sigmoid of the chunk's channel-0 elements: the first is at (NO - ph) mod NO, then every NO-th
        float sg = 0.f;
        for (int e = (ph ? NO - ph : 0) + tid * NO; e < n_el; e += kThreads * NO) sg += sigmoidf_acc(el[e]);
        sg = block_sum<4>(sg, red);                                    // (its barriers also publish ps and pc)
        if (tid < NO) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            int cc = 0, j = 0;
            for (; j + 3 < per; j += 4) {
                a0 += ps[j * NO + tid]; a1 += ps[(j + 1) * NO + tid]; a2 += ps[(j + 2) * NO + tid]; a3 += ps[(j + 3) * NO + tid];
                cc += (pc[j * NO + tid] + pc[(j + 1) * NO + tid]) + (pc[(j + 2) * NO + tid] + pc[(j + 3) * NO + tid]);
            }
            if (j < per) { a0 += ps[j * NO + tid]; cc += pc[j * NO + tid]; }
            if (j + 1 < per) { a1 += ps[(j + 1) * NO + tid]; cc += pc[(j + 1) * NO + tid]; }
            if (j + 2 < per) { a2 += ps[(j + 2) * NO + tid]; cc += pc[(j + 2) * NO + tid]; }
            const int o = (ph + tid) % NO;
            out.fsum[ch * NO + o] = (a0 + a1) + (a2 + a3);
            out.icnt[ch * NO + o] = cc;
        }
        if (tid == 0) out.psig[ch] = sg;
    }
}

__global__ __launch_bounds__(kThreads) void clip_finish_kernel(Partials in, const long long* __restrict__ message, float* __restrict__ prob,
                                                               float* __restrict__ llr, int* __restrict__ votes,
                                                               long long* __restrict__ words, int* __restrict__ biterr, long long R,
                                                               long long B, int T, int NO, int nch) {
    __shared__ double sq[4][64];
    __shared__ long long cq[4][64];
    __shared__ double red[4];
    const int tid = threadIdx.x, il = tid & 63, grp = tid >> 6;
    const int per = (nch + 3) / 4, p0 = grp * per, p1 = min(p0 + per, nch);
    for (long long r = blockIdx.x; r < R; r += gridDim.x) {
        const float* __restrict__ f = in.fsum + r * nch * NO;
        const int* __restrict__ ic = in.icnt + r * nch * NO;
        const float* __restrict__ pg = in.psig + r * nch;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        long long c = 0;
        if (il < NO) {
            int p = p0;
            for (; p + 3 < p1; p += 4) {
                const float v0 = f[(size_t)p * NO + il], v1 = f[(size_t)(p + 1) * NO + il];
                const float v2 = f[(size_t)(p + 2) * NO + il], v3 = f[(size_t)(p + 3) * NO + il];
                c += ((long long)ic[(size_t)p * NO + il] + ic[(size_t)(p + 1) * NO + il]) +
                     ((long long)ic[(size_t)(p + 2) * NO + il] + ic[(size_t)(p + 3) * NO + il]);
                s0 += (double)v0; s1 += (double)v1; s2 += (double)v2; s3 += (double)v3;
            }
            for (int k = 0; p < p1; ++p, ++k) {
                const double v = (double)f[(size_t)p * NO + il];
                if (k == 0) s0 += v; else if (k == 1) s1 += v; else s2 += v;
                c += ic[(size_t)p * NO + il];
            }
        }
        double sp = 0.0;
        for (int p = tid; p < nch; p += kThreads) sp += (double)pg[p];
        __syncthreads();                                               // the row before has been read out of sq and cq
        sq[grp][il] = (s0 + s1) + (s2 + s3);
        cq[grp][il] = c;
        sp = block_sum_d<4>(sp, red);                                  // (its barriers also publish sq and cq)
        if (grp == 0) {
            double s = 0.0;
            long long n = 0;
#pragma unroll
            for (int g = 0; g < 4; ++g) { s += sq[g][il]; n += cq[g][il]; }
            const bool valid = il < NO;
            if (valid) {
                if (llr != nullptr) llr[r * NO + il] = (float)(s / (double)T);
                votes[r * NO + il] = (int)n;
            }
            const unsigned long long hard = __ballot(valid && il >= 1 && 2 * n > (long long)T) >> 1;   // a tie is 0
            const unsigned long long soft = __ballot(valid && il >= 1 && s > 0.0) >> 1;                 // NaN: 0
            if (il == 0) {
                if (prob != nullptr) prob[r] = (float)(sp / (double)T);
                if (words != nullptr) { words[2 * r] = (long long)hard; words[2 * r + 1] = (long long)soft; }
                if (biterr != nullptr && message != nullptr && r < B) {
                    const unsigned long long mask = (1ull << (NO - 1)) - 1ull, m = (unsigned long long)message[r];
                    biterr[2 * r] = __popcll((hard ^ m) & mask);
                    biterr[2 * r + 1] = __popcll((soft ^ m) & mask);
                }
            }
        }
    }
}

// the chunks of one row; false where the shape is refused
bool plan(long long R, long long T, long long NO, long long& nch) {
    if (R < 1 || T < 1 || T > (1ll << 24) || NO < 1 || NO > 64 || R > (1ll << 46) / (T * NO)) return false;
    nch = (T * NO + kChunk - 1) / kChunk;
    return true;
}

}  // namespace

extern "C" {

int wm_clip_scores_plan(long long R, int T, int NO, long long* scratch_bytes, hipStream_t) {
    long long nch = 0;
    if (!scratch_bytes || !plan(R, T, NO, nch)) return (int)hipErrorInvalidValue;
    *scratch_bytes = R * nch * (2 * (long long)NO + 1) * 4;
    return 0;
}

int wm_clip_scores(const float* logits, const long long* message, float thr_logit, float* prob, float* llr, int* votes, long long* words,
                   int* biterr, void* scratch, long long B, long long R, int T, int NO, hipStream_t stream) {
    long long nch = 0;
    if (!plan(R, T, NO, nch) || B < 0 || B > R || std::isnan(thr_logit)) return (int)hipErrorInvalidValue;
    if (!logits || !votes || !scratch) return (int)hipErrorInvalidValue;
    if ((uintptr_t)logits % 4 || (uintptr_t)prob % 4 || (uintptr_t)llr % 4 || (uintptr_t)votes % 4 || (uintptr_t)biterr % 4 ||
        (uintptr_t)scratch % 4 || (uintptr_t)message % 8 || (uintptr_t)words % 8)
        return (int)hipErrorInvalidValue;
    const bool has_msg = message != nullptr && B > 0;
    const unsigned long long ur = (unsigned long long)R, uno = (unsigned long long)NO;
    const unsigned long long in_bytes = ur * (unsigned long long)T * uno * 4, msg_bytes = has_msg ? (unsigned long long)B * 8 : 0;
    const unsigned long long sc_bytes = ur * (unsigned long long)nch * (2 * uno + 1) * 4;
    const void* outs[6] = {prob, llr, votes, words, has_msg ? biterr : nullptr, scratch};
    const unsigned long long outs_bytes[6] = {ur * 4, ur * uno * 4, ur * uno * 4, ur * 16, (unsigned long long)B * 8, sc_bytes};
    for (int i = 0; i < 6; ++i) {                                      // what is written overlaps neither an input nor another output
        if (!outs[i]) continue;
        if (overlap(logits, in_bytes, outs[i], outs_bytes[i]) || (has_msg && overlap(message, msg_bytes, outs[i], outs_bytes[i])))
            return (int)hipErrorInvalidValue;
        for (int k = i + 1; k < 6; ++k)
            if (outs[k] && overlap(outs[i], outs_bytes[i], outs[k], outs_bytes[k])) return (int)hipErrorInvalidValue;
    }
    const long long chunks = R * nch;
    Partials p;
    p.fsum = static_cast<float*>(scratch);
    p.icnt = reinterpret_cast<int*>(p.fsum + chunks * NO);
    p.psig = reinterpret_cast<float*>(p.icnt + chunks * NO);
    hipLaunchKernelGGL(clip_partial_kernel, dim3((unsigned)(chunks < kGridCap ? chunks : kGridCap)), dim3(kThreads), 0, stream, logits,
                       thr_logit, p, T * NO, NO, nch, chunks);
    WM_CHECK_LAUNCH();
    hipLaunchKernelGGL(clip_finish_kernel, dim3((unsigned)(R < kGridCap ? R : kGridCap)), dim3(kThreads), 0, stream, p,
                       has_msg ? message : (const long long*)nullptr, prob, llr, votes, words, biterr, R, B, T, NO, (int)nch);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
