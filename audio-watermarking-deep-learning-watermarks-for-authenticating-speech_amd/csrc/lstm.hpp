// nn.LSTM(64, 64, batch_first=True), one layer, zero initial state, gate order i,f,g,o
// (py/main16.py:138,152-154) over T = 16000 dependent steps per clip.
//
// Split the MI355X way:
//   1. wm_lstm_xproj     xp[b,t,:] = W_ih x[b,:,t] + b_ih + b_hh for every t at once -- a GEMM with
//                        time as M, on the fp32 matrix cores, reading the channel-first encoder
//                        frame directly (no permute pass).
//   2. wm_lstm_fwd       the recurrence: ONE 256-thread workgroup per clip, persistent over all T
//                        steps.  W_hh (256x64 fp32) lives in registers (one gate row per lane), h is
//                        broadcast through a double-buffered 256-B LDS line, the four gates of a
//                        hidden unit sit in one wave (lane = gate*16 + unit) and are exchanged with
//                        bpermutes, so there is exactly one s_barrier per time step.  H = 64 makes
//                        the recurrent product a 256x64 GEMV per clip: an LDS-broadcast dot product,
//                        not an MFMA shape.  h is written channel-first [B,64,T] for the decoder.
//   3. wm_lstm_bwd       BPTT with the same geometry (dh = W_hh^T da as per-wave partial GEMVs, one
//                        barrier per step); it overwrites the saved gate activations with the
//                        pre-activation gradients da[b,t,256].
//   4. wm_lstm_dx / wm_lstm_wgrad   everything that is NOT sequential leaves the recurrence:
//                        dx = da W_ih, dW_ih = da^T x, dW_hh = da^T h_{t-1}, db = sum da are MFMA GEMMs.
//   5. wm_lstm_bwd_wgrad / wm_lstm_bwd_wgrad_dx   ... and comes back beside it: four helper waves per workgroup form the
//                        weight gradients, and two of them dx, on the matrix cores the recurrence leaves idle, from an
//                        LDS image of da (lstm_bwd_ws_kernel); with dx inside, da never reaches memory.
//
// One translation unit per kernel family; this header is what they share and is no unit of its own:
//   lstm_fwd.hip    steps 1 and 2: the input projection and the three forward recurrences (plain, projection inside, wave-specialised
//                   with or without the ResBlock tail)
//   lstm_bwd.hip    steps 3 and 5: the three BPTT recurrences (plain, dx inside, wave-specialised with the weight gradients and dx)
//   lstm_grad.hip   step 4: the dx and weight-gradient GEMMs, fp32 and bf16x6
// An entry point lives with every kernel it can launch; lstm_wgrad_reduce_kernel (below) is compiled once per including unit, so
// nothing needs relocatable device code.  The per-step-launch LSTM of the main14b_2 variant (lstm_seq_*, in lstm_seq.hip) shares nothing with these.
#pragma once
#include "wm_common.hpp"
#include <type_traits>
using namespace wm;

// host side: the wm_set_lstm_dx_bf16x6 switch, which lstm_grad.hip holds (one definition) and the fallback of wm_lstm_bwd_wgrad_dx in
// lstm_bwd.hip reads.  Not part of the library's ABI.
namespace wm {
__attribute__((visibility("hidden"))) int lstm_dx_bf16x6();
}
// the one entry point a unit calls across the C ABI (that fallback): lstm_grad.hip defines it against this declaration
extern "C" int wm_lstm_dx(const float* da, const float* w_ih, float* dx, int B, int T, hipStream_t stream);

namespace {

// -DWM_STAMP (diagnostic build, tests/diag_stamp_lstm.py): s_memtime stamps inside a recurrence step, summed over the steps of a
// clip per segment and written to a buffer of their own.  LSTAMP(var, val) stamps once `val` exists (and holds later uses of it back).
#ifdef WM_STAMP
__device__ unsigned long long* g_lstm_stamp = nullptr;
#define LSTAMP(var, val) unsigned long long var; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var), "+v"(val))
#define LSTAMP_ACC(i, a, b) tm[i] += (b) - (a)
#else
#define LSTAMP(var, val)
#define LSTAMP_ACC(i, a, b)
#endif

// Per-step tensors (xp / gates / da) are stored [B][T][256] with the column order  n' = unit*4 + gate  so that the
// four gates of a hidden unit sit in four adjacent lanes (one DPP quad) of the recurrence kernels and every per-step
// access of a wave is one contiguous 256-B segment.  gate row of the PyTorch parameters: n = gate*64 + unit.
__device__ __forceinline__ int gate_row(int np) { return (np & 3) * 64 + (np >> 2); }

typedef float v2f __attribute__((ext_vector_type(2)));
// broadcast lane k of every quad (DPP quad_perm: no LDS round trip, unlike ds_bpermute)
template <int K>
__device__ __forceinline__ float quad_bcast(float v) {
    constexpr int ctrl = K | (K << 2) | (K << 4) | (K << 6);
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xf, 0xf, false));
}

// sigmoid via v_exp_f32 + v_rcp_f32.  With U = 2^-24: the exponential carries |z| U from the rounded product z log2(e) and 2 U (1 ulp)
// from v_exp_f32, which move sigma by sigma (1 - sigma) times that (the derivative vanishes where |z| is large); the sum 1 + e (U) and
// v_rcp_f32 (1 ulp) move it by sigma times theirs:  |error| <= sigma (1 - sigma) (|z| + 2) U + 3 U sigma  <= 1.9e-7 for every z,
// fp32 round-off of a value near 1 (the first term alone is below 3e-8; correctly rounded fp32 arithmetic is no closer than the sum).
// tanh_s doubles it and rounds once more, <= 4.3e-7 absolute: near z = 0 that is a relative error of order U / |z| (2 s - 1 cancels).
// tests/lstm_yardstick.py derives both bounds, tests/test_gpu_lstm_edges.py holds the functions to them over +-1e4.
__device__ __forceinline__ float sigm(float z) { return __builtin_amdgcn_rcpf(1.0f + __expf(-z)); }
__device__ __forceinline__ float tanh_s(float z) { return fmaf(2.0f, sigm(2.0f * z), -1.0f); }
// one transcendental pair per lane whatever the gate: tanh(x) = 2*sigmoid(2x) - 1 for the g lanes
__device__ __forceinline__ float gate_act(float x, bool is_g) {
    const float s = sigm(is_g ? 2.0f * x : x);
    return is_g ? fmaf(2.0f, s, -1.0f) : s;
}

// acc += w * {v[lane k], v[lane k+1]}: the two broadcast values travel through an SGPR pair (v_readlane), which
// v_pk_fma_f32 takes directly as an operand -- no LDS return traffic, no VGPR copies
template <typename T2>
__device__ __forceinline__ T2 pk_fma_lanes(T2 w, float v, int k, T2 acc) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane(__float_as_int(v), k);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane(__float_as_int(v), k + 1);
    const unsigned long long pr = ((unsigned long long)hi << 32) | lo;
    asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "s"(pr));
    return acc;
}

// The same products with the lane reads issued AHEAD of the products that consume them: a v_readlane writes its SGPR late, and a
// product issued right behind the two reads of its own operand pair stalls on that write (the stamped step showed 610 cycles
// for 32 reads + 32 products).  N values (lanes k0 .. k0 + N - 1 of v) go into N scalar registers first, behind a scheduling
// fence; the products then find their operands complete.
template <int N>
__device__ __forceinline__ void lanes_to_sgprs(float v, int k0, unsigned long long (&pr)[N / 2]) {
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane(__float_as_int(v), k0 + 2 * i);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane(__float_as_int(v), k0 + 2 * i + 1);
        pr[i] = ((unsigned long long)hi << 32) | lo;
    }
    __builtin_amdgcn_sched_barrier(0);
}
template <typename T2>
__device__ __forceinline__ T2 pk_fma_s(T2 w, unsigned long long pr, T2 acc) {
    asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "s"(pr));
    return acc;
}

// ---- the recurrent 64-term dot product without lane reads: acc += v[lane i of my 16-lane row] * w  (DPP row_newbcast)
// Four registers hold the 64 broadcast values row-replicated (H[j][lane] = value[16 j + lane % 16]); product (j, i) is ONE
// v_fmac_f32_dpp.  Measured on one wave per SIMD (tests/diag/dpp_gemv.hip): 390 cycles per 64 products against 494 for
// 32 v_readlane + 32 v_pk_fma_f32 with scalar operand pairs (a lone wave issues a packed fp32 FMA every 8 cycles, not 4).
// sixteen products with the sixteen lanes of the row as ONE asm statement (hipcc pads every statement boundary with a wait state
// whose cost is an issue slot of the lone wave: 64 single-instruction statements carried 14 s_nop per step)
template <int J>
__device__ __forceinline__ void fmac_row16(float (&acc)[4], float H, const float (&w)[64]) {
    asm volatile(
        "v_fmac_f32_dpp %0, %4, %5 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %1, %4, %6 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %2, %4, %7 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %3, %4, %8 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %0, %4, %9 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %1, %4, %10 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %2, %4, %11 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %3, %4, %12 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %0, %4, %13 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %1, %4, %14 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %2, %4, %15 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %3, %4, %16 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %0, %4, %17 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %1, %4, %18 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %2, %4, %19 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %3, %4, %20 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
        : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3])
        : "v"(H), "v"(w[16 * J]), "v"(w[16 * J + 1]), "v"(w[16 * J + 2]), "v"(w[16 * J + 3]), "v"(w[16 * J + 4]), "v"(w[16 * J + 5]),
          "v"(w[16 * J + 6]), "v"(w[16 * J + 7]), "v"(w[16 * J + 8]), "v"(w[16 * J + 9]), "v"(w[16 * J + 10]), "v"(w[16 * J + 11]),
          "v"(w[16 * J + 12]), "v"(w[16 * J + 13]), "v"(w[16 * J + 14]), "v"(w[16 * J + 15]));
}
__device__ __forceinline__ float dot64_rowbcast(const float (&H)[4], const float (&w)[64], float init = 0.f) {
    float acc[4] = {init, 0.f, 0.f, 0.f};
    // a DPP read needs two wait states behind a VALU write of its source (the swaps of rows_replicate); the compiler pads only
    // what it can see, not the inside of an asm statement
    asm volatile("s_nop 1" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));
    fmac_row16<0>(acc, H[0], w); fmac_row16<1>(acc, H[1], w); fmac_row16<2>(acc, H[2], w); fmac_row16<3>(acc, H[3], w);
    return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}
// where value k of the broadcast vector sits in its 64-float LDS line: lane l reads ONE float4 at 4 (l % 16) and has H[0..3]
__device__ __forceinline__ int rowbcast_slot(int k) { return (k & 15) * 4 + (k >> 4); }
// the same four registers from a value held lane-wise (lane l has value[l]): three half / row swaps, no LDS
__device__ __forceinline__ void rows_replicate(float v, float (&H)[4]) {
    const unsigned x = __float_as_uint(v);
    const auto r32 = __builtin_amdgcn_permlane32_swap(x, x, false, false);    // [r0 r1 r0 r1], [r2 r3 r2 r3]
    const auto a = __builtin_amdgcn_permlane16_swap(r32[0], r32[0], false, false);   // [r0 x4], [r1 x4]
    const auto b = __builtin_amdgcn_permlane16_swap(r32[1], r32[1], false, false);   // [r2 x4], [r3 x4]
    H[0] = __uint_as_float(a[0]); H[1] = __uint_as_float(a[1]); H[2] = __uint_as_float(b[0]); H[3] = __uint_as_float(b[1]);
}

#ifndef WM_LSTM_HS_BWD
#define WM_LSTM_HS_BWD 64       // measured: 32 -> 7.84 ms, 48 -> 7.65 ms, 64 (no LDS round trip at all) -> 7.53 ms
#endif
#ifndef WM_LSTM_HS
#define WM_LSTM_HS 32
#endif

// per-clip (or per-workgroup) slabs [nparts][256*128 + 256] -> the four gradients.  Block = 64 columns x 8 part-groups
// (column_sum_d), 516 blocks: at B = 256 every thread adds 32 slabs, four loads in flight, coalesced over the column.
constexpr int kWgradSlab = 256 * 128 + 256;
__global__ __launch_bounds__(512) void lstm_wgrad_reduce_kernel(const float* __restrict__ partial, int nparts, float* dw_ih,
                                                                float* dw_hh, float* db_ih, float* db_hh, int accumulate) {
    __shared__ double sq[8][64];
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);            // kWgradSlab % 64 == 0: every column is valid
    const float s = (float)column_sum_d<8>(partial, nparts, (size_t)kWgradSlab, i, true, sq);
    if (threadIdx.x >= 64) return;
    if (i < 256 * 128) {
        const int n = gate_row(i >> 7), j = i & 127;
        float* dst = (j < 64) ? dw_ih + n * 64 + j : dw_hh + n * 64 + (j - 64);
        *dst = accumulate ? *dst + s : s;
    } else {
        const int n = gate_row(i - 256 * 128);
        db_ih[n] = accumulate ? db_ih[n] + s : s;
        db_hh[n] = accumulate ? db_hh[n] + s : s;
    }
}
static_assert(kWgradSlab % 64 == 0, "lstm_wgrad_reduce_kernel: whole 64-column blocks");

}  // namespace
