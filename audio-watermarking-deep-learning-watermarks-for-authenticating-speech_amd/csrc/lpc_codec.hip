// Predictive speech-codec stand-in along the last axis of rows x n fp32 data: per-frame linear prediction (windowed autocorrelation,
// Levinson-Durbin), open-loop quantisation of the prediction residual at a per-row SNR, all-pole synthesis -- and the adjoint of the
// linear map synthesis . mask . analysis at given coefficients.  The definition is the comment of wm_lpc_codec in include/wm_hip.h; this
// file is how it is computed.
//
// One workgroup per row (the rows grid-stride), one launch, three stages that overlap on a ring of three LDS buffers.  A chunk is NF
// consecutive frames (7, or 4 at L = 640, which keeps the kernel's LDS under 64 KiB).  In iteration i
//   PRE   the producer waves 1 .. NF fill chunk i.  Forward: wave w owns frame w - 1 of the chunk -- windowed segment into its own LDS
//         scratch, the p + 1 lags (lane l over j = l, l + 64, .., xor butterfly), Levinson-Durbin redundantly in every lane (16 x 16 serial
//         flops are not worth a broadcast), then residual, frame energy, step, codes, and eq into the ring.  Adjoint: g, the mask and
//         the NF + 1 coefficient sets the chunk can meet.
//   SERIAL  wave 0 runs the recursion over chunk i - 1 in place.  Sixteen samples at a time, fully unrolled: the last sixteen outputs
//         live in sixteen registers and are renamed, not moved, and the block is 256 v_fma_f32 -- the sum in FALLING k, so the term of
//         the newest output is the last of its chain and the fifteen before it do not wait for it.  Every lane computes the same
//         numbers (the operands are LDS broadcasts), lane 0 writes; the next block's inputs are read while the block runs (worth
//         11 % in the adjoint, nothing in the forward).  The adjoint is the same block run down the row; the block that ends a
//         frame takes the coefficients of the terms that cross the boundary from the next frame's set (compile-time select).
//   POST  the producer waves finish chunk i - 2: the forward copies it to y in whole coalesced rows, the adjoint forms
//         dx = A^T v from the masked u of the ring and a sixteen-sample halo of the chunk after it.
// One barrier an iteration.  The recursion is the critical path (DESIGN.md section 4o has the measured cycles per sample); PRE and POST
// of a chunk cost a small fraction of its SERIAL stage, so the producers mostly wait.
//
// Safety.  Every index into a row passes 0 <= t < n before the access, the ring is indexed by local offsets below NF L (+ 16 for the
// halo, which has its own array), the frame index of a coefficient set is checked against F, and codes are clamped to int16 before
// the conversion.
#include "wm_common.hpp"
using namespace wm;

namespace {

constexpr int kOrd = 16;                         // the recursion always runs 16 taps; a_k = 0 for k > p

struct Args {
    const float* x; float* y; const float* coeffs_in; float* coeffs_out; short* codes_out; const short* mask_in;
    const float* snr_db; const float* lag; const float* expand;
    long long rows, n, F;
    int p, quantise;
    float floor_step;
};

template <int L> struct Geo {
    static constexpr int NF = L == 640 ? 4 : 7;  // frames a chunk = producer waves
    static constexpr int kThreads = 64 * (NF + 1);
    static constexpr int kWavesPerSimd = L == 640 ? 3 : 4;     // two workgroups a CU: 512 rows are one round on 256 CUs
    static constexpr int CH = NF * L;            // samples a chunk
    static constexpr int PER = (L + 63) / 64;    // samples of a frame per lane
};

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Sixteen steps of out[i] = in[i] - sum_k c[k] prev_k, prev_k the k-th output before it, the sum one fmaf chain in falling k.  old: the
// sixteen outputs before this block in processing order (old[15] the newest).  nc / nn hold the NEGATED coefficients, entry k - 1 for
// tap k; CROSS: a term that reaches into the block before takes nn (the adjoint's first block of a frame), every other term nc.
template <bool CROSS>
__device__ __forceinline__ void rec16(float (&old)[16], const float (&in)[16], const float (&nc)[16], const float (&nn)[16]) {
    float out[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        float acc = in[i];
#pragma unroll
        for (int k = kOrd; k >= 1; --k) {
            const bool before = i - k < 0;
            const float prev = before ? old[16 + i - k] : out[i - k];
            const float c = (CROSS && before) ? nn[k - 1] : nc[k - 1];
            acc = fmaf(c, prev, acc);
        }
        out[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) old[i] = out[i];
}

__device__ __forceinline__ void load_neg16(const float* c, float (&d)[16]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 v = lds_read4(c + 4 * q);
        d[4 * q] = -v.x; d[4 * q + 1] = -v.y; d[4 * q + 2] = -v.z; d[4 * q + 3] = -v.w;
    }
}

// sixteen consecutive floats of LDS in time order, and in processing order of the adjoint (falling time: d[i] = p[15 - i])
__device__ __forceinline__ void load16(const float* p, float (&d)[16]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 v = lds_read4(p + 4 * q);
        d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
    }
}
__device__ __forceinline__ void load16r(const float* p, float (&d)[16]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 v = lds_read4(p + 4 * q);
        d[15 - 4 * q] = v.x; d[14 - 4 * q] = v.y; d[13 - 4 * q] = v.z; d[12 - 4 * q] = v.w;
    }
}

// Levinson-Durbin on Rc[0 .. p] and the bandwidth expansion; a[k - 1] is tap k, 0 for k > p.  The same in every lane.
__device__ __forceinline__ void levinson(const float (&Rc)[kOrd + 1], int p, const float* __restrict__ expand, float (&a)[kOrd]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < kOrd; ++k) a[k] = 0.f;
    float E = Rc[0];
    bool go = E > 0.f;
#pragma unroll
    for (int i = 1; i <= kOrd; ++i) {
        if (go && i <= p) {
            float acc = Rc[i];
#pragma unroll
            for (int j = 1; j < i; ++j) acc = fmaf(a[j - 1], Rc[i - j], acc);
            const float k = -acc / E;
            if (fabsf(k) < 1.f) {
                float t[kOrd];
#pragma unroll
                for (int j = 1; j < i; ++j) t[j - 1] = fmaf(k, a[i - j - 1], a[j - 1]);
#pragma unroll
                for (int j = 1; j < i; ++j) a[j - 1] = t[j - 1];
                a[i - 1] = k;
                E = E * fmaf(-k, k, 1.f);
            } else {
                go = false;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kOrd; ++k)
        if (k < p) a[k] = a[k] * expand[k];
}

template <int L, bool ADJ>
__global__ __launch_bounds__(Geo<L>::kThreads, Geo<L>::kWavesPerSimd) void lpc_kernel(Args A) {
    using G = Geo<L>;
    constexpr int NF = G::NF, CH = G::CH, PER = G::PER;
    __shared__ __align__(16) float D[3][CH];                  // the ring: eq -> y (forward), g -> mask * u (adjoint)
    __shared__ __align__(16) float C[3][(NF + 1) * kOrd];     // the chunk's coefficient sets, and the one after them (adjoint)
    __shared__ __align__(16) float S[2 * CH];                 // forward: a 2L scratch per producer wave; adjoint: the mask, two chunks
    __shared__ __align__(16) float W[ADJ ? 4 : 2 * L];        // forward: the analysis window
    __shared__ __align__(16) float H[2][kOrd];                // adjoint: the first sixteen v of the chunk after this one
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n = A.n, F = A.F;
    const int p = A.p;
    const long long NC = (F + NF - 1) / NF;
    const bool analyse = !ADJ && A.coeffs_in == nullptr;

    if (!ADJ && analyse) {
        for (int j = tid; j < 2 * L; j += G::kThreads) W[j] = (float)(0.5 - 0.5 * cospi((double)(2 * j + 1) / (double)(2 * L)));
    }

    for (long long row = blockIdx.x; row < A.rows; row += gridDim.x) {
        const float* __restrict__ xr = A.x + row * n;
        float* __restrict__ yr = A.y + row * n;
        const short* __restrict__ mr = A.mask_in ? A.mask_in + row * n : nullptr;
        float scale = 0.f;
        if (!ADJ && A.quantise) {
            float s = A.snr_db[row];
            s = s >= 0.f ? (s <= 60.f ? s : 60.f) : 0.f;                              // NaN -> 0
            scale = (float)pow(10.0, -(double)s / 20.0);
        }
        if (tid < 2 * kOrd) (&H[0][0])[tid] = 0.f;
        __syncthreads();                                                              // W, H; the last row's readers are done
        float old[16];                                                                // wave 0: the recursion's state
#pragma unroll
        for (int i = 0; i < 16; ++i) old[i] = 0.f;

        for (long long it = 0; it < NC + 2; ++it) {
            if (wave > 0) {
                // ---- POST of chunk it - 2
                if (it >= 2) {
                    const long long ci = it - 2, cid = ADJ ? NC - 1 - ci : ci, t0 = cid * CH;
                    const float* __restrict__ Dp = D[ci % 3];
                    if (!ADJ) {
                        for (int i = tid - 64; i < CH; i += NF * 64)
                            if (t0 + i < n) yr[t0 + i] = Dp[i];
                    } else {
                        const float* __restrict__ Cp = C[ci % 3];
                        const float* __restrict__ Hp = H[(ci + 1) & 1];               // left by the POST before this one
                        for (int i = tid - 64; i < CH; i += NF * 64) {
                            float acc = Dp[i];
#pragma unroll
                            for (int k = 1; k <= kOrd; ++k) {
                                const int j = i + k;
                                const float v = j < CH ? Dp[j] : Hp[j - CH];
                                acc = fmaf(Cp[(j / L) * kOrd + k - 1], v, acc);
                            }
                            if (t0 + i < n) yr[t0 + i] = acc;
                        }
                        if (tid - 64 < kOrd) H[ci & 1][tid - 64] = Dp[tid - 64];
                    }
                }
                // ---- PRE of chunk it
                if (it < NC) {
                    const long long cid = ADJ ? NC - 1 - it : it, f0 = cid * NF, t0 = cid * CH;
                    float* __restrict__ Dq = D[it % 3];
                    float* __restrict__ Cq = C[it % 3];
                    if (ADJ) {
                        float* __restrict__ Mq = S + (it & 1) * CH;
                        for (int i = tid - 64; i < CH; i += NF * 64) {
                            const long long t = t0 + i;
                            const bool in = t < n;
                            Dq[i] = in ? xr[t] : 0.f;
                            Mq[i] = (in && (!mr || mr[t] != 0)) ? 1.f : 0.f;
                        }
                        for (int i = tid - 64; i < (NF + 1) * kOrd; i += NF * 64) {
                            const long long f = f0 + i / kOrd;
                            const int k = i % kOrd;
                            Cq[i] = (f < F && k < p) ? A.coeffs_in[(row * F + f) * p + k] : 0.f;
                        }
                    } else {
                        const int fw = wave - 1;
                        const long long f = f0 + fw, tf = f * L;                      // this wave's frame and its first sample
                        float a[kOrd];
#pragma unroll
                        for (int k = 0; k < kOrd; ++k) a[k] = 0.f;
                        if (f < F) {
                            if (analyse) {
                                float* __restrict__ s = S + fw * 2 * L;
                                for (int j = lane; j < 2 * L; j += 64) {
                                    const long long t = tf - L / 2 + j;
                                    s[j] = W[j] * ((t >= 0 && t < n) ? xr[t] : 0.f);
                                }
                                wave_sync();
                                float Rc[kOrd + 1];
#pragma unroll
                                for (int k = 0; k <= kOrd; ++k) {
                                    float r = 0.f;
                                    if (k <= p) {
                                        for (int j = lane; j < 2 * L - k; j += 64) r = fmaf(s[j], s[j + k], r);
                                        r = wave_sum(r) * A.lag[k];
                                    }
                                    Rc[k] = r;
                                }
                                wave_sync();                                          // s is free for the next chunk's frame
                                levinson(Rc, p, A.expand, a);
                            } else {
#pragma unroll
                                for (int k = 0; k < kOrd; ++k)
                                    if (k < p) a[k] = A.coeffs_in[(row * F + f) * p + k];
                            }
                            if (lane == 0 && A.coeffs_out) {
#pragma unroll
                                for (int k = 0; k < kOrd; ++k)
                                    if (k < p) A.coeffs_out[(row * F + f) * p + k] = a[k];
                            }
                        }
                        if (lane == 0) {
#pragma unroll
                            for (int k = 0; k < kOrd; ++k) Cq[fw * kOrd + k] = a[k];
                        }
                        // residual, energy, step, codes; samples outside the row give eq = 0
                        float e[PER];
                        float en = 0.f;
#pragma unroll
                        for (int i = 0; i < PER; ++i) {
                            const int tl = lane + 64 * i;
                            const long long t = tf + tl;
                            float acc = 0.f;
                            if (tl < L && t < n) {
                                acc = xr[t];
#pragma unroll
                                for (int k = 1; k <= kOrd; ++k) acc = fmaf(a[k - 1], t - k >= 0 ? xr[t - k] : 0.f, acc);
                                en = fmaf(acc, acc, en);
                            }
                            e[i] = acc;
                        }
                        float step = 1.f;
                        if (A.quantise) {
#pragma clang fp contract(off)
                            const long long left = n - tf;
                            const float cnt = (float)(left < L ? (left > 0 ? left : 1) : L);
                            const float P = wave_sum(en) / cnt;
                            step = fmaxf(sqrtf(12.f * P) * scale, A.floor_step);
                        }
#pragma unroll
                        for (int i = 0; i < PER; ++i) {
                            const int tl = lane + 64 * i;
                            const long long t = tf + tl;
                            if (tl < L) {
                                float v = e[i];
                                const bool in = t < n;
                                if (A.quantise) {
                                    float q = rintf(v / step);
                                    q = q >= -32767.f ? (q <= 32767.f ? q : 32767.f) : -32767.f;      // NaN -> -32767, never met with finite data
                                    if (in && A.codes_out) A.codes_out[row * n + t] = (short)(int)q;
                                    v = q * step;
                                }
                                if (!in || (mr && mr[t] == 0)) v = 0.f;
                                Dq[fw * L + tl] = v;
                            }
                        }
                    }
                }
            } else if (it >= 1 && it <= NC) {
                // ---- SERIAL over chunk it - 1, in place
                const long long ci = it - 1, cid = ADJ ? NC - 1 - ci : ci;
                float* __restrict__ Ds = D[ci % 3];
                const float* __restrict__ Cs = C[ci % 3];
                const long long left = F - cid * NF;
                const int nfc = left < NF ? (int)left : NF;
                if (!ADJ) {
                    for (int fw = 0; fw < nfc; ++fw) {
                        float nc[16];
                        load_neg16(Cs + fw * kOrd, nc);
                        float in[16];
                        load16(Ds + fw * L, in);
#pragma unroll 2
                        for (int b = 0; b < L / 16; ++b) {
                            float* __restrict__ dp = Ds + fw * L + 16 * b;
                            float nx[16];                                             // the next block's eq, read while this one runs
                            load16(dp + (b + 1 < L / 16 ? 16 : 0), nx);
                            rec16<false>(old, in, nc, nc);
                            if (lane == 0) {
#pragma unroll
                                for (int q = 0; q < 4; ++q)
                                    *reinterpret_cast<f32x4*>(dp + 4 * q) = f32x4{old[4 * q], old[4 * q + 1], old[4 * q + 2], old[4 * q + 3]};
                            }
#pragma unroll
                            for (int i = 0; i < 16; ++i) in[i] = nx[i];
                        }
                    }
                } else {
                    const float* __restrict__ Ms = S + (ci & 1) * CH;
                    for (int fw = nfc - 1; fw >= 0; --fw) {
                        float nc[16], nn[16];
                        load_neg16(Cs + fw * kOrd, nc);
                        load_neg16(Cs + (fw + 1) * kOrd, nn);
                        float in[16], mk[16];
                        load16r(Ds + fw * L + L - 16, in);
                        load16r(Ms + fw * L + L - 16, mk);
#pragma unroll 2
                        for (int b = L / 16 - 1; b >= 0; --b) {
                            float* __restrict__ dp = Ds + fw * L + 16 * b;
                            float nx[16], nm[16];                                     // the block before in time, read while this one runs
                            load16r(dp - (b > 0 ? 16 : 0), nx);
                            load16r(Ms + fw * L + 16 * b - (b > 0 ? 16 : 0), nm);
                            if (b == L / 16 - 1) rec16<true>(old, in, nc, nn);
                            else rec16<false>(old, in, nc, nc);
                            if (lane == 0) {
#pragma unroll
                                for (int q = 0; q < 4; ++q)
                                    *reinterpret_cast<f32x4*>(dp + 4 * q) =
                                        f32x4{old[15 - 4 * q] * mk[15 - 4 * q], old[14 - 4 * q] * mk[14 - 4 * q],
                                              old[13 - 4 * q] * mk[13 - 4 * q], old[12 - 4 * q] * mk[12 - 4 * q]};
                            }
#pragma unroll
                            for (int i = 0; i < 16; ++i) { in[i] = nx[i]; mk[i] = nm[i]; }
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
}

template <int L>
int launch(const Args& a, bool adjoint, long long rows, hipStream_t stream) {
    const long long cap = (long long)kNumCU * 8;
    const dim3 grid((unsigned)(rows < cap ? rows : cap)), block(Geo<L>::kThreads);
    if (adjoint) hipLaunchKernelGGL((lpc_kernel<L, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((lpc_kernel<L, false>), grid, block, 0, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" {

int wm_lpc_codec(const float* x, float* y, const float* coeffs_in, float* coeffs_out, void* codes_out, const void* mask_in,
                 const float* snr_db, const float* lag, const float* expand, long long rows, long long n, int L, int p, float floor_step,
                 int quantise, int adjoint, hipStream_t stream) {
    if (rows < 1 || n < 1 || n > (1ll << 34) || rows > (1ll << 46) / n) return (int)hipErrorInvalidValue;
    if ((L != 160 && L != 320 && L != 640) || p < 2 || p > 16) return (int)hipErrorInvalidValue;
    if (!x || !y || (uintptr_t)x % 4 || (uintptr_t)y % 4 || (uintptr_t)coeffs_in % 4 || (uintptr_t)coeffs_out % 4 ||
        (uintptr_t)codes_out % 2 || (uintptr_t)mask_in % 2 || (uintptr_t)snr_db % 4 || (uintptr_t)lag % 4 || (uintptr_t)expand % 4)
        return (int)hipErrorInvalidValue;
    if (adjoint && (!coeffs_in || quantise || coeffs_out || codes_out)) return (int)hipErrorInvalidValue;
    if (!coeffs_in && (!lag || !expand)) return (int)hipErrorInvalidValue;
    if (quantise && (!snr_db || !(floor_step > 0.f) || !(floor_step < INFINITY))) return (int)hipErrorInvalidValue;
    if (!quantise && codes_out) return (int)hipErrorInvalidValue;
    const long long F = (n + L - 1) / L;
    const unsigned long long bx = (unsigned long long)rows * n * 4, bc = (unsigned long long)rows * F * p * 4,
                             bq = (unsigned long long)rows * n * 2, br = (unsigned long long)rows * 4;
    struct Span { const void* p; unsigned long long b; };
    const Span ins[] = {{x, bx}, {coeffs_in, bc}, {mask_in, bq}, {snr_db, br}, {lag, (unsigned long long)(p + 1) * 4},
                        {expand, (unsigned long long)p * 4}};
    const Span outs[] = {{y, bx}, {coeffs_out, bc}, {codes_out, bq}};
    for (const Span& o : outs) {
        if (!o.p) continue;
        for (const Span& i : ins)
            if (i.p && overlap(i.p, i.b, o.p, o.b)) return (int)hipErrorInvalidValue;   // in place is refused
        for (const Span& o2 : outs)
            if (o2.p && o2.p != o.p && overlap(o2.p, o2.b, o.p, o.b)) return (int)hipErrorInvalidValue;
    }
    Args a;
    a.x = x; a.y = y; a.coeffs_in = coeffs_in; a.coeffs_out = coeffs_out; a.codes_out = (short*)codes_out;
    a.mask_in = (const short*)mask_in; a.snr_db = snr_db; a.lag = lag; a.expand = expand;
    a.rows = rows; a.n = n; a.F = F; a.p = p; a.quantise = quantise ? 1 : 0; a.floor_step = floor_step;
    if (L == 160) return launch<160>(a, adjoint != 0, rows, stream);
    if (L == 320) return launch<320>(a, adjoint != 0, rows, stream);
    return launch<640>(a, adjoint != 0, rows, stream);
}

}  // extern "C"
