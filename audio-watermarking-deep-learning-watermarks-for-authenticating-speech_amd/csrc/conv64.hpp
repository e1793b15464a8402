// 64 -> 64 channel 1-D convolutions on [B,64,T] fp32 frames as implicit GEMMs on the gfx950
// fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32, frees the VALU for the fused
// prologue / epilogue work).
//
// Replaces, for the hot path of py/main16.py:
//   * ResBlock's two Conv1d(64,64,3,padding=1) (+ the BatchNorm1d / ReLU around them)   :115-121
//   * Generator.decoder[0] = ConvTranspose1d(64,64,7,padding=3) (+ the embedding add)      :144,156-159
//   * their data-gradients (same kernel, re-packed weights) and weight-gradients.
//
// One persistent 256-thread workgroup per CU streams (clip, time-tile) tiles:
//   global --(dwordx4, software-pipelined one tile ahead, through registers so the prologue
//   transform can be applied)--> LDS [64][NT+halo]  --ds_read_b32--> MFMA B operand
//   packed weights [tap][cin][cout] live in LDS for the whole kernel --> MFMA A operand
//   D tile (cout x time) leaves the accumulators as 128-B row segments (time is contiguous).
//
// This header: what the conv64*.hip units (one kernel family each) share, and nothing else.  Each unit
// compiles its own copy.  For those units only: it opens namespace wm and defines file-local typedefs and knob defaults.
#pragma once
#include "wm_common.hpp"
using namespace wm;
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#ifdef WM_STAMP
// diagnostic build only (-DWM_STAMP): per-wave cycle totals of the kernel's phases.  A device global cannot span translation units
// without relocatable device code: every unit has its own copy, and one that stamps defines its own setter with WM_STAMP_SETTER
static __device__ unsigned long long* g_wm_stamp = nullptr;
#define STAMP(var) unsigned long long var = __builtin_amdgcn_s_memtime()
#define WM_STAMP_SETTER(name) int name(unsigned long long* buf) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_wm_stamp), &buf, sizeof(buf)); }
#else
#define STAMP(var)
#define WM_STAMP_SETTER(name)
#endif

#ifndef WM_LOADPOS
#define WM_LOADPOS 1
#endif
#ifndef WM_LOAD_H
#define WM_LOAD_H 17
#endif
#ifndef WM_XCD_MAP
#define WM_XCD_MAP 1
#endif
#ifndef WM_TILE_CONTIG
#define WM_TILE_CONTIG 0
#endif
#ifndef WM_NT_STORE
#define WM_NT_STORE 0
#endif
#ifndef WM_BF3_MANUAL
#define WM_BF3_MANUAL 1
#endif
#ifndef WM_BF3_PIN_W
#define WM_BF3_PIN_W 1
#endif
#ifndef WM_BF7_PIPE
#define WM_BF7_PIPE 1        // 7-tap convolution: 1 = register-resident weights, pipelined (T % 128 == 0), 0 = LDS weights, phase-serial
#endif
#ifndef WM_WGRAD_PIPE
#define WM_WGRAD_PIPE 1      // k3 weight gradient: 1 = pipelined 64-step tiles (wgrad64bfp_kernel), 0 = phase-serial 128-step tiles
#endif

namespace {
enum { PRO_NONE = 0, PRO_BNRELU = 1, PRO_ADDVEC = 2, PRO_BNBWD = 3,
       PRO_TAIL = 4,      // conv64bf3 (f16 build) only: the previous ResBlock's tail relu(x + x2 * pa + pb), also stored to tout / tmask
       PRO_STEM = 5 };    // conv64bf3 (f16 build) only: the stem's output pb[c] + sum_j pa[c][j] x[b, t + j - 3] of the clips x [B,1,T], also stored to tout;
                          // dwgrad64bf (XPRO, f16 build): the same value as the weight-gradient operand, from DWArgs' ss / sw / sb
enum { EPI_BIAS = 0, EPI_RELUMASK = 1, EPI_ADD = 2, EPI_NONE = 3, EPI_BNADDRELU = 4,    // 4: relu(e1 + (acc + bias) * ea + eb), conv64bf3 only
       EPI_BIASELU = 5, EPI_BIASADDELU = 6, EPI_MULDELU = 7,    // main14b_2's 64-channel blocks (conv64bf_kernel only): elu(acc + bias),
                                                                 // elu(acc + bias + e1), acc * ELU'(e1) with e1 = the ELU output y
       EPI_ADDSTATS = 8 };    // dwgrad64bf only: EPI_ADD, then the ReLU mask of the PREVIOUS block and its two BatchNorm sums

struct Conv64Args {
    const float* x;     // [B,64,T] primary input
    const float* x2;    // [B,64,T] second input (PRO_BNBWD)
    const float* wp;    // packed weights [KW][64 in][64 out]
    const float* pa;    // prologue per-channel a  (BNRELU: scale, BNBWD: A, ADDVEC: vec[B,64])
    const float* pb;    // prologue per-channel b  (BNRELU: shift, BNBWD: B)
    const float* pc;    // prologue per-channel c  (BNBWD: C)
    const float* bias;  // [64] (EPI_BIAS)
    const float* e1;    // [B,64,T] epilogue tensor (RELUMASK: pre-BN activation, ADD: addend)
    const float* ea;    // [64] epilogue scale (RELUMASK)
    const float* eb;    // [64] epilogue shift (RELUMASK)
    float* y;           // [B,64,T]
    float* stats;       // [gridDim.x][2][64] partial sums or nullptr
    int B, T;
    float* tout = nullptr;       // [B,64,T] PRO_TAIL: the formed input, as wm_bn_add_relu_mask writes it; PRO_STEM: as wm_stem_fwd writes it
    unsigned* tmask = nullptr;   // [B*64][T/32] PRO_TAIL: its sign bits (wm_bn_add_relu_mask's layout) or nullptr
};

template <int PRO>
__device__ __forceinline__ float pro_apply(float v, float v2, float ca, float cb, float cc, float cl = 0.f) {
    if (PRO == PRO_BNRELU) return fmaxf(fmaf(v, ca, cb), 0.f);
    if (PRO == PRO_ADDVEC) return v + ca;
    if (PRO == PRO_BNBWD) return fmaf(ca, v, fmaf(cc, v2, cb)) + cl;      // cb + cl: offset as hi + lo words (pb[0..63], pb[64..127])
    if (PRO == PRO_TAIL) return fmaxf(v + fmaf(v2, ca, cb), 0.f);         // bn_add_relu_kernel's expression (bn.hip), to the letter
    return v;
}

struct Wgrad64Args {
    const float* g;  const float* g2;                   // gradient tensor(s) [B,64,T]
    const float* ga; const float* gb; const float* gc;  // BNBWD constants for g
    const float* x;                                     // layer input [B,64,T]
    const float* xa; const float* xb;                   // x prologue constants (BNRELU scale/shift, ADDVEC vec[B,64])
    float* partial;                                     // [grid][KW*4096 + 64]
    int B, T;
};

// XCD-aware workgroup -> tile-slot map.  Workgroups are dealt round-robin to the 8 XCDs (blockIdx % 8), each with its
// own L2.  Giving XCD x the 1/8 of the tile sequence [x*G/8, (x+1)*G/8) makes time-adjacent tiles share an L2, so the
// halo columns (a 128-B line per channel per side, +50 % fetched bytes otherwise) and the neighbours' lines hit in L2.
__device__ __forceinline__ int xcd_slot() {
    const int g = gridDim.x, b = blockIdx.x;
    return (g & 7) ? b : (b & 7) * (g >> 3) + (b >> 3);
}

__device__ __forceinline__ void lds_barrier() {          // s_barrier without draining vmcnt (global stores/prefetches stay in flight)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// dst layout: mode 0 conv  dW[out][in][KW]   <- G[tap][out][in]
//             mode 1 convT dW[in][out][KW]   <- G[KW-1-k][out][in]
__global__ __launch_bounds__(256) void wgrad64_reduce_kernel(const float* __restrict__ partial, int nparts, int KW, int mode,
                                                             float* __restrict__ dw, float* __restrict__ dbias, int accumulate) {
    // block = 64 outputs x 4 quarters of the slab list; fixed order, fp64: bitwise reproducible and cancellation-safe
    __shared__ double sq[4][64];
    const int il = threadIdx.x & 63, grp = threadIdx.x >> 6, i = blockIdx.x * 64 + il;
    const int stride = KW * 4096 + 64;
    const int per = (nparts + 3) / 4, p0 = grp * per, p1 = min(p0 + per, nparts);
    double s0 = 0.0, s1 = 0.0;
    if (i < stride) {
        int p = p0;
        for (; p + 1 < p1; p += 2) {
            s0 += (double)partial[(size_t)p * stride + i];
            s1 += (double)partial[(size_t)(p + 1) * stride + i];
        }
        if (p < p1) s0 += (double)partial[(size_t)p * stride + i];
    }
    sq[grp][il] = s0 + s1;
    __syncthreads();
    if (grp != 0 || i >= stride) return;
    const float s = (float)((sq[0][il] + sq[1][il]) + (sq[2][il] + sq[3][il]));
    if (i < KW * 4096) {
        const int tap = i / 4096, out = (i / 64) % 64, in = i % 64;
        const int dst = (mode == 0) ? (out * 64 + in) * KW + tap : (in * 64 + out) * KW + (KW - 1 - tap);
        dw[dst] = accumulate ? dw[dst] + s : s;
    } else if (dbias) {
        const int c = i - KW * 4096;
        dbias[c] = accumulate ? dbias[c] + s : s;
    }
}
}  // namespace
