// Shared device helpers for the gfx950 (MI355X / CDNA4) watermark kernels.
// Wave = 64 lanes everywhere; no portability layer on purpose.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>

#define WM_CHECK_LAUNCH() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)
#define WM_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return (int)e_; } while (0)

// the one entry point called across units without a family header: bn.hip defines it against this declaration, wm_gconv_pack_h (gconv_fwd.hip) calls it
extern "C" int wm_gscale_absmax(const float* x, long long n, float* scratch, float log2_target, float* gscale, hipStream_t stream);

namespace wm {

// hipFuncSetAttribute (the > 64 KB dynamic-LDS opt-in) is a PER-DEVICE setting: remember it per device ordinal, so one
// process may drive several GPUs (and several host threads: the attribute call is idempotent, a race only repeats it).
// The only mutable state the launchers keep is this cache.
struct DevOnce {
    std::atomic<unsigned long long> mask{0};
};
inline bool dev_done(const DevOnce& d) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    return (d.mask.load(std::memory_order_acquire) >> (dev & 63)) & 1ull;
}
inline void dev_mark(DevOnce& d) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return;
    d.mask.fetch_or(1ull << (dev & 63), std::memory_order_release);
}
// the opt-in itself, once per device and kernel (one DevOnce per kernel); 0 or the hipError_t of the attribute call
inline int lds_opt_in(const void* kern, size_t lds, DevOnce& once) {
    if (dev_done(once)) return 0;
    WM_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    dev_mark(once);
    return 0;
}

// host only: do [a, a + na) and [b, b + nb) share a byte?  The launchers refuse in-place calls with it.
inline bool overlap(const void* a, unsigned long long na, const void* b, unsigned long long nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// One 16-byte-aligned ds_read_b128 that stays one.  hipcc narrows a plain float4 LDS load of which not every component is used
// and merges it with its neighbours: the stem backward's three quads per channel became ds_read_b64 at addresses = 4 (mod 8)
// plus ds_read2_b32.  With the reads kept whole and aligned (and the taps out of LDS) the Detector's stem_bwd launch went from
// 0.77 to 0.62 ms.  p points into LDS; the explicit address space keeps the volatile access a DS
// instruction (through a generic pointer it becomes a flat load).
typedef const volatile __attribute__((address_space(3))) f32x4 lds_f32x4_t;
__device__ __forceinline__ f32x4 lds_read4(const float* p) { return *(lds_f32x4_t*)p; }

constexpr int kWave = 64;
constexpr int kNumCU = 256;          // MI355X: 8 XCD x 32 CU

// D(32x32) += A(32x2) * B(2x32), exact fp32 (v_mfma_f32_32x32x2_f32).
// lane l supplies A[i = l&31][k = l>>5] and B[k = l>>5][j = l&31];
// D: col = l&31, row = (r&3) + 8*(r>>2) + 4*(l>>5) for register r in [0,16).
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int mfma_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// sum over the 32 lanes that share (lane>>5)
__device__ __forceinline__ float half_wave_sum(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// Transposing butterfly: every lane brings 32 values x[0..31]; on return lane l of each 32-lane half-wave holds
// the sum over that half-wave of x[l & 31].  31 shuffles instead of the 160 of 32 independent tree reductions,
// and the 5 stages are 16/8/4/2/1 independent shuffles wide, so they pipeline.
__device__ __forceinline__ float half_wave_transpose_sum32(float (&x)[32], int lane) {
#pragma unroll
    for (int s = 4; s >= 0; --s) {
        const int h = 1 << s;
        const bool up = (lane >> s) & 1;
#pragma unroll
        for (int i = 0; i < h; ++i) {
            const float keep = up ? x[i + h] : x[i];
            const float send = up ? x[i] : x[i + h];
            x[i] = keep + __shfl_xor(send, h);
        }
    }
    return x[0];
}
// 16-value variant: on return every lane l holds the half-wave total of x[l & 15]
__device__ __forceinline__ float half_wave_transpose_sum16(float (&x)[16], int lane) {
#pragma unroll
    for (int s = 3; s >= 0; --s) {
        const int h = 1 << s;
        const bool up = (lane >> s) & 1;
#pragma unroll
        for (int i = 0; i < h; ++i) {
            const float keep = up ? x[i + h] : x[i];
            const float send = up ? x[i] : x[i + h];
            x[i] = keep + __shfl_xor(send, h);
        }
    }
    return x[0] + __shfl_xor(x[0], 16);
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// block-wide sum for blocks of NW waves; result valid in every thread. scratch: >= NW floats of LDS.
template <int NW>
__device__ __forceinline__ float block_sum(float v, float* scratch) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) scratch[w] = v;
    __syncthreads();
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) r += scratch[i];
    return r;
}
template <int NW>
__device__ __forceinline__ double block_sum_d(double v, double* scratch) {
    v = wave_sum_d(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) scratch[w] = v;
    __syncthreads();
    double r = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) r += scratch[i];
    return r;
}

// Column sum of the partial-slab reductions (stem / head / LSTM weight gradients): sum_p partial[p*stride + i] in fp64.
// A block of NG*64 threads owns 64 consecutive columns i (coalesced over i); part-group g = threadIdx.x >> 6 adds the slabs
// [g*per, (g+1)*per), per = ceil(nparts / NG), slab p0 + k into accumulator k & 3 (four independent chains, four loads in
// flight), and thread (0, i) adds the NG group sums from LDS in increasing g.  The grouping depends on nparts alone:
// bit-reproducible.  Every thread of the block calls it (one barrier inside); the total is returned where g == 0.
template <int NG>
__device__ __forceinline__ double column_sum_d(const float* __restrict__ partial, int nparts, size_t stride, int i, bool valid,
                                               double (&sq)[NG][64]) {
    const int il = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int per = (nparts + NG - 1) / NG, p0 = grp * per, p1 = min(p0 + per, nparts);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (valid) {
        const float* col = partial + i;
        int p = p0;
        for (; p + 3 < p1; p += 4) {
            const float v0 = col[(size_t)p * stride], v1 = col[(size_t)(p + 1) * stride];
            const float v2 = col[(size_t)(p + 2) * stride], v3 = col[(size_t)(p + 3) * stride];
            s0 += (double)v0; s1 += (double)v1; s2 += (double)v2; s3 += (double)v3;
        }
        if (p < p1) s0 += (double)col[(size_t)p * stride];
        if (p + 1 < p1) s1 += (double)col[(size_t)(p + 1) * stride];
        if (p + 2 < p1) s2 += (double)col[(size_t)(p + 2) * stride];
    }
    sq[grp][il] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    double s = 0.0;
    if (grp == 0) {
#pragma unroll
        for (int g = 0; g < NG; ++g) s += sq[g][il];
    }
    return s;
}

__device__ __forceinline__ float sigmoidf_acc(float x) { return 1.0f / (1.0f + expf(-x)); }

// softplus(-|x|) = log1p(e^-|x|) on the hardware transcendentals: u = e^-|x| in (0, 1]; a cubic series below 0.01 (error
// < 3e-9 absolute), log(1 + u) above (the rounding of 1 + u costs <= 6e-6 relative there).  libm's log1pf/expf pair made
// the 139 M-element BCE pass VALU-bound (0.7 ms at B = 256).
__device__ __forceinline__ float softplus_neg_abs(float x) {
    const float u = __expf(-fabsf(x));
    return (u < 0.01f) ? u * fmaf(u, fmaf(u, 0.33333334f, -0.5f), 1.0f) : __logf(1.0f + u);
}
// BCEWithLogits of one element (csrc/losses.hip, and the Detector head's forward in csrc/small_convs.hip)
__device__ __forceinline__ float bce_logits(float x, float y) { return fmaxf(x, 0.f) - x * y + softplus_neg_abs(x); }
// its derivative times k: the element of d(loss)/d(logits) that wm_bce_bwd writes and headN_bwd_kernel forms on load
__device__ __forceinline__ float bce_logits_grad(float x, float y, float k) {
    const float sg = __builtin_amdgcn_rcpf(1.0f + __expf(-x));     // as in the LSTM gates: error <= 3e-8
    return k * (sg - y);
}

// out[0] = (float)(scale * sum_i partial[i]) in fp64 and a fixed order, one 1024-thread workgroup (csrc/losses.hip)
int launch_sum_scale2(const float* partial, int n, double scale, float* out, hipStream_t stream);

#ifndef WM_STREAM_NT
#define WM_STREAM_NT 1      // nontemporal loads / stores on the frame streams: 0.59 -> 0.57 ms (bn_add_relu), 0.34 -> 0.32 ms (sums pass) at B = 256
#endif
// frame-sized operands that are read / written once per launch (1 GB per frame at B = 256: far beyond L2 + Infinity Cache)
__device__ __forceinline__ float4 stream_load(const float4* p) {
#if WM_STREAM_NT
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
#else
    return *p;
#endif
}
__device__ __forceinline__ void stream_store(float4* p, const float4& v) {
#if WM_STREAM_NT
    __builtin_nontemporal_store(f32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<f32x4*>(p));
#else
    *p = v;
#endif
}
__device__ __forceinline__ float stream_load(const float* p) {
#if WM_STREAM_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
__device__ __forceinline__ void stream_store(float* p, float v) {
#if WM_STREAM_NT
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

// ELU (alpha = 1) with a cheap expm1: Taylor to the 6th order on (-0.35, 0] (error < 4e-7 of the value), exp(v) - 1 below
__device__ __forceinline__ float elu1(float v) {
    const float p = v * (1.f + v * (0.5f + v * (0.16666667f + v * (0.041666668f + v * (0.0083333338f + v * 0.0013888889f)))));
    const float e = __expf(v) - 1.f;
    const float n = v > -0.35f ? p : e;
    return v > 0.f ? v : n;
}



// ---- bf16x6 split arithmetic (see conv64_fwd.hip): x = hi + mid + lo as three bf16 pieces, exact to 24 bits
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// two values -> three dwords, each holding the (a: low half, b: high half) pair of one piece
__device__ __forceinline__ void split3_pair(float a, float b, unsigned& p0, unsigned& p1, unsigned& p2) {
    bf16x2 h = {(__bf16)a, (__bf16)b};
    p0 = __builtin_bit_cast(unsigned, h);
    a -= __uint_as_float(p0 << 16); b -= __uint_as_float(p0 & 0xffff0000u);
    bf16x2 m = {(__bf16)a, (__bf16)b};
    p1 = __builtin_bit_cast(unsigned, m);
    a -= __uint_as_float(p1 << 16); b -= __uint_as_float(p1 & 0xffff0000u);
    bf16x2 l = {(__bf16)a, (__bf16)b};
    p2 = __builtin_bit_cast(unsigned, l);
}

// acc += A*B to fp32 grade from the 3-piece fragments: the six piece products of weight >= 2^-16, small terms first
__device__ __forceinline__ f32x16 mfma_bf16x6(const bf16x8 (&A)[3], const bf16x8 (&B)[3], f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[1], B[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0], B[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[2], B[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0], B[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[1], B[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0], B[0], acc, 0, 0, 0);
    return acc;
}

// ---- buffer addressing (scalar descriptor + 32-bit per-lane byte offset + scalar offset; out-of-range lanes read 0 / are dropped)
typedef __amdgpu_buffer_rsrc_t wm_srd_t;   // 128-bit buffer resource descriptor (kept in scalar registers)

// buffer descriptor over [p, p + bytes): 32-bit per-lane byte offsets + a scalar offset, reads past the end return 0
__device__ __forceinline__ wm_srd_t make_srd(const float* p, size_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), (short)0, (int)(bytes > 0xfffff000ull ? 0xfffff000ull : bytes),
                                             0x00020000);
}
__device__ __forceinline__ float buf_load(wm_srd_t srd, unsigned voff_bytes, unsigned soff_bytes) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(srd, (int)voff_bytes, (int)soff_bytes, 0));
}
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 buf_load4(wm_srd_t srd, unsigned voff_bytes, unsigned soff_bytes) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd, (int)voff_bytes, (int)soff_bytes, 0));
}
typedef float f32x3 __attribute__((ext_vector_type(3)));
typedef unsigned u32x3 __attribute__((ext_vector_type(3)));
__device__ __forceinline__ f32x3 buf_load3(wm_srd_t srd, unsigned voff_bytes, unsigned soff_bytes) {
    return __builtin_bit_cast(f32x3, __builtin_amdgcn_raw_buffer_load_b96(srd, (int)voff_bytes, (int)soff_bytes, 0));
}
__device__ __forceinline__ void buf_store4(wm_srd_t srd, f32x4 v, unsigned voff_bytes, unsigned soff_bytes) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), srd, (int)voff_bytes, (int)soff_bytes, 0);
}
__device__ __forceinline__ void buf_store(wm_srd_t srd, float v, unsigned voff_bytes, unsigned soff_bytes) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), srd, (int)voff_bytes, (int)soff_bytes, 0);
}

// ---- sign bits of a staged frame tile (the ResBlock tail formed in its consumer: conv64bf3's PRO_TAIL, lstm_fwd_ws's TAIL)
// In the staging map shared by those kernels (channel pair = lane & 7, time quad = lane >> 3) the eight lanes with one lane & 7 hold
// the 32 steps of one word of wm_bn_add_relu_mask's layout.  nibble: bit e = (element e > 0); mask_merge8: OR over lane >> 3 without a
// trip through LDS (one DPP rotate inside the 16-lane row, then the two gfx950 row / half swaps), valid in every lane.
__device__ __forceinline__ unsigned sign_nibble(const float4& v) {
    return ((v.x > 0.f) ? 1u : 0u) | ((v.y > 0.f) ? 2u : 0u) | ((v.z > 0.f) ? 4u : 0u) | ((v.w > 0.f) ? 8u : 0u);
}
__device__ __forceinline__ unsigned mask_merge8(unsigned m) {
    m |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x128, 0xf, 0xf, true);          // row_ror:8 = lane ^ 8
    const auto r16 = __builtin_amdgcn_permlane16_swap(m, m, false, false);                  // lane ^ 16
    m = r16[0] | r16[1];
    const auto r32 = __builtin_amdgcn_permlane32_swap(m, m, false, false);                  // lane ^ 32
    return r32[0] | r32[1];
}

}  // namespace wm
