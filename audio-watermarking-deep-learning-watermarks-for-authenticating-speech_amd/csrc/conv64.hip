// The bf16x6 / f16 split families of the 64 -> 64 convolutions (conv64.hpp): the k3 forward and data-gradient kernels
// (phase-serial conv64bf, pipelined conv64bf3), the two 7-tap kernels with their weight gradient, the k3 weight gradients.
// The fp32, inference and fused families are conv64_fp32.hip, conv64_eval.hip and conv64_dwgrad.hip.
#include "conv64.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// bf16x6 variant of the k3 convolution: fp32-grade results on the bf16 matrix cores.
// Every fp32 operand is split into three bf16 pieces (x = hi + mid + lo exactly to 24 bits) when it is staged
// into LDS; a product a*b is the sum of the six piece products of weight >= 2^-16 (hi*hi, hi*mid, mid*hi, hi*lo,
// lo*hi, mid*mid), accumulated in fp32 by v_mfma_f32_32x32x16_bf16.  The dropped terms are <= 2^-24 relative, i.e.
// the result carries the same error as a native fp32 FMA chain, at 6/16 of the matrix-pipe time of
// v_mfma_f32_32x32x2_f32 -- and, unlike the fp32 MFMA, the bf16 MFMA does not share the SIMD's VALU pipe.
// LDS images are channel-minor ([time][channel] and [tap][cout][cin], 144-B pitch) so that an MFMA fragment
// (8 consecutive k = 8 input channels) is one aligned ds_read_b128.
// ---------------------------------------------------------------------------------------------
template <int PRO, int EPI, bool STATS>
__global__ __launch_bounds__(256) void conv64bf_kernel(Conv64Args a) {
    constexpr int KW = 3, PAD = 1, NT = 128, ROWS = NT + 2, PITCH = 72, NP = 3;
    constexpr int NC = 4;                         // (channel pair, time quad) combos per thread
    constexpr bool TWO = (PRO == PRO_BNBWD);
    constexpr bool E1 = (EPI == EPI_RELUMASK || EPI == EPI_ADD || EPI == EPI_BIASADDELU || EPI == EPI_MULDELU);
    constexpr bool HASBIAS = (EPI == EPI_BIAS || EPI == EPI_BIASELU || EPI == EPI_BIASADDELU);
    extern __shared__ __align__(16) unsigned char smem_raw[];
    unsigned short* Wb = reinterpret_cast<unsigned short*>(smem_raw);              // [NP][KW][64 out][PITCH]
    unsigned short* Xb = Wb + NP * KW * 64 * PITCH;                                // [NP][ROWS][PITCH]
    float* Cs = reinterpret_cast<float*>(Xb + NP * ROWS * PITCH);                  // [6][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int T = a.T;
    const int tilesPerClip = (T + NT - 1) / NT, ntiles = a.B * tilesPerClip;

    float4 sa[NC], sb[NC], sa2[TWO ? NC : 1], sb2[TWO ? NC : 1];
    float hl, hl2 = 0.f;
    // staging map: a wave covers 8 channel pairs x 8 time quads (128-B global segments, 2-way LDS write conflicts)
    auto combo = [&](int i, int& cp, int& q) {
        const int idx = tid + i * 256, widx = idx >> 6, l = idx & 63;
        cp = (widx & 3) * 8 + (l & 7);
        q = (widx >> 2) * 8 + (l >> 3);
    };
    auto load_tile = [&](int tile) {              // branch-free: clamped addresses, masked when written to LDS
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        const float* xb = a.x + (size_t)b * 64 * T;
        const float* xb2 = TWO ? a.x2 + (size_t)b * 64 * T : nullptr;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            int cp, q;
            combo(i, cp, q);
            const size_t o = (size_t)(2 * cp) * T + min(t0 + 4 * q, T - 4);
            sa[i] = *reinterpret_cast<const float4*>(xb + o);
            sb[i] = *reinterpret_cast<const float4*>(xb + o + T);
            if (TWO) { sa2[i] = *reinterpret_cast<const float4*>(xb2 + o); sb2[i] = *reinterpret_cast<const float4*>(xb2 + o + T); }
        }
        const int hc = (tid & 127) >> 1, hh = tid & 1;
        const int ht = min(max(hh ? t0 + NT : t0 - 1, 0), T - 1);
        hl = xb[(size_t)hc * T + ht];
        if (TWO) hl2 = xb2[(size_t)hc * T + ht];
    };
    auto write_tile = [&](int tile) {
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        unsigned* X32 = reinterpret_cast<unsigned*>(Xb);
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            int cp, q;
            combo(i, cp, q);
            const int c = 2 * cp, t = t0 + 4 * q;
            float va[4] = {sa[i].x, sa[i].y, sa[i].z, sa[i].w}, vb[4] = {sb[i].x, sb[i].y, sb[i].z, sb[i].w};
            if (PRO != PRO_NONE) {
                const float ca0 = (PRO == PRO_ADDVEC) ? a.pa[b * 64 + c] : Cs[c], ca1 = (PRO == PRO_ADDVEC) ? a.pa[b * 64 + c + 1] : Cs[c + 1];
                const float cb0 = Cs[64 + c], cb1 = Cs[64 + c + 1], cc0 = Cs[128 + c], cc1 = Cs[128 + c + 1];
                const float cl0 = TWO ? Cs[192 + c] : 0.f, cl1 = TWO ? Cs[192 + c + 1] : 0.f;
                float wa[4] = {0.f, 0.f, 0.f, 0.f}, wb[4] = {0.f, 0.f, 0.f, 0.f};
                if (TWO) { wa[0] = sa2[i].x; wa[1] = sa2[i].y; wa[2] = sa2[i].z; wa[3] = sa2[i].w; wb[0] = sb2[i].x; wb[1] = sb2[i].y; wb[2] = sb2[i].z; wb[3] = sb2[i].w; }
#pragma unroll
                for (int e = 0; e < 4; ++e) { va[e] = pro_apply<PRO>(va[e], wa[e], ca0, cb0, cc0, cl0); vb[e] = pro_apply<PRO>(vb[e], wb[e], ca1, cb1, cc1, cl1); }
            }
            const bool ok = t < T;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned p0, p1, p2;
                split3_pair(ok ? va[e] : 0.f, ok ? vb[e] : 0.f, p0, p1, p2);
                const int o = ((1 + 4 * q + e) * PITCH + c) >> 1;
                X32[o] = p0; X32[(ROWS * PITCH >> 1) + o] = p1; X32[2 * (ROWS * PITCH >> 1) + o] = p2;
            }
        }
        if (tid < 128) {
            const int hc = tid >> 1, hh = tid & 1, t = hh ? t0 + NT : t0 - 1;
            float v = hl;
            if (PRO != PRO_NONE) {
                const float ca = (PRO == PRO_ADDVEC) ? a.pa[b * 64 + hc] : Cs[hc];
                v = pro_apply<PRO>(v, hl2, ca, Cs[64 + hc], Cs[128 + hc], TWO ? Cs[192 + hc] : 0.f);
            }
            if (t < 0 || t >= T) v = 0.f;
            unsigned p0, p1, p2;
            split3_pair(v, 0.f, p0, p1, p2);
            const int o = (hh ? NT + 1 : 0) * PITCH + hc;
            Xb[o] = (unsigned short)p0; Xb[ROWS * PITCH + o] = (unsigned short)p1; Xb[2 * ROWS * PITCH + o] = (unsigned short)p2;
        }
    };

    int tile = blockIdx.x;
    if (tile < ntiles) load_tile(tile);
    // resident weights: global image [NP][KW][64][64] bf16 -> LDS pitch 72, 16 B at a time
    for (int i = tid; i < NP * KW * 64 * 8; i += 256) {
        const int row = i >> 3, seg = i & 7;
        *reinterpret_cast<uint4*>(Wb + row * PITCH + seg * 8) = reinterpret_cast<const uint4*>(a.wp)[i];
    }
    if (tid < 64) {
        Cs[tid] = (PRO == PRO_BNRELU || PRO == PRO_BNBWD) ? a.pa[tid] : 0.f;
        Cs[64 + tid] = (PRO == PRO_BNRELU || PRO == PRO_BNBWD) ? a.pb[tid] : 0.f;
        Cs[128 + tid] = (PRO == PRO_BNBWD) ? a.pc[tid] : 0.f;
        Cs[192 + tid] = (PRO == PRO_BNBWD) ? a.pb[64 + tid] : ((HASBIAS && a.bias) ? a.bias[tid] : 0.f);
        Cs[256 + tid] = (EPI == EPI_RELUMASK) ? a.ea[tid] : 0.f;
        Cs[320 + tid] = (EPI == EPI_RELUMASK) ? a.eb[tid] : 0.f;
    }
    __syncthreads();
    if (tile < ntiles) write_tile(tile);
    __syncthreads();

    float s1[STATS ? 32 : 1], s2[STATS ? 32 : 1];
    if (STATS) {
#pragma unroll
        for (int j = 0; j < 32; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    }
#ifdef WM_STAMP
    unsigned long long tm[6] = {0, 0, 0, 0, 0, 0};
#endif
    while (tile < ntiles) {
        STAMP(ts0);
        const int next = tile + gridDim.x;
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        const int tcol = t0 + wave * 32 + l31;
        float e1r[E1 ? 32 : 1];
        // The global loads of the next tile (and of this tile's epilogue operand) are issued LOADPOS taps into the
        // matrix phase: issued at the top they queue behind the previous tile's output stores and the wave stalls
        // at issue until those drain, with the matrix cores idle.
        auto issue_loads = [&]() {
            if (next < ntiles) load_tile(next);
            if (E1) {
                const float* eb1 = a.e1 + (size_t)b * 64 * T + min(tcol, T - 1);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) e1r[mt * 16 + r] = eb1[(size_t)(mt * 32 + mfma_row(r, half)) * T];
            }
        };
        if (WM_LOADPOS == 0) issue_loads();
        STAMP(ts1);
        f32x16 acc[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
        const unsigned short* wbase = Wb + l31 * PITCH + 8 * half;
        const unsigned short* xbase = Xb + (wave * 32 + l31) * PITCH + 8 * half;
#pragma unroll 1
        for (int tap = 0; tap < KW; ++tap) {
            if (WM_LOADPOS > 0 && tap == WM_LOADPOS) issue_loads();
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                bf16x8 A[2][NP], Bf[NP];
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    Bf[p] = *reinterpret_cast<const bf16x8*>(xbase + (p * ROWS + tap) * PITCH + 16 * ch);
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
                        A[mt][p] = *reinterpret_cast<const bf16x8*>(wbase + ((p * KW + tap) * 64 + mt * 32) * PITCH + 16 * ch);
                }
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][1], Bf[1], acc[mt], 0, 0, 0);
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][0], Bf[2], acc[mt], 0, 0, 0);
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][2], Bf[0], acc[mt], 0, 0, 0);
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][0], Bf[1], acc[mt], 0, 0, 0);
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][1], Bf[0], acc[mt], 0, 0, 0);
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][0], Bf[0], acc[mt], 0, 0, 0);
                }
            }
        }
        STAMP(ts2);
        float* yb = a.y + (size_t)b * 64 * T + tcol;
        const bool ok = tcol < T;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = mt * 32 + mfma_row(r, half);
                float v = acc[mt][r];
                float q = 0.f;
                if (HASBIAS) v += Cs[192 + co];
                if (EPI == EPI_RELUMASK) { q = e1r[mt * 16 + r]; v = (fmaf(q, Cs[256 + co], Cs[320 + co]) > 0.f) ? v : 0.f; }
                if (EPI == EPI_ADD || EPI == EPI_BIASADDELU) v += e1r[mt * 16 + r];
                if (EPI == EPI_BIASELU || EPI == EPI_BIASADDELU) v = elu1(v);
                if (EPI == EPI_MULDELU) { const float yy = e1r[mt * 16 + r]; v *= (yy > 0.f ? 1.f : yy + 1.f); }
                if (ok) {
                    yb[(size_t)co * T] = v;
                    if (STATS) { s1[mt * 16 + r] += v; s2[mt * 16 + r] += (EPI == EPI_RELUMASK) ? v * q : v * v; }
                }
            }
        STAMP(ts3);
        __syncthreads();
        STAMP(ts4);
        if (next < ntiles) write_tile(next);
        STAMP(ts5);
        __syncthreads();
        STAMP(ts6);
#ifdef WM_STAMP
        tm[0] += ts1 - ts0; tm[1] += ts2 - ts1; tm[2] += ts3 - ts2; tm[3] += ts4 - ts3; tm[4] += ts5 - ts4; tm[5] += ts6 - ts5;
#endif
        tile = next;
    }
#ifdef WM_STAMP
    if (g_wm_stamp && lane == 0) {
        unsigned long long* d = g_wm_stamp + ((size_t)blockIdx.x * 4 + wave) * 6;
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = tm[i];
    }
#endif
    if (STATS) {
        float* red = reinterpret_cast<float*>(Xb);          // [4 waves][2][64]
#pragma unroll
        for (int j = 0; j < 32; ++j) { s1[j] = half_wave_sum(s1[j]); s2[j] = half_wave_sum(s2[j]); }
        if (l31 == 0) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = mt * 32 + mfma_row(r, half);
                    red[wave * 128 + co] = s1[mt * 16 + r];
                    red[wave * 128 + 64 + co] = s2[mt * 16 + r];
                }
        }
        __syncthreads();
        if (tid < 128)
            a.stats[(size_t)blockIdx.x * 128 + tid] = red[tid] + red[128 + tid] + red[256 + tid] + red[384 + tid];
    }
}

template <int PRO, int EPI, bool STATS>
int launch_conv64bf(const Conv64Args& a, hipStream_t stream) {
    constexpr size_t lds = (size_t)(3 * 3 * 64 * 72 + 3 * 130 * 72) * 2 + 6 * 64 * sizeof(float);
    static wm::DevOnce attr_done;
    auto kern = conv64bf_kernel<PRO, EPI, STATS>;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(kern), lds, attr_done)) return rc;
    const int ntiles = a.B * ((a.T + 127) / 128);
    const int grid = ntiles < kNumCU ? ntiles : kNumCU;
    if (STATS && grid < kNumCU) WM_TRY(hipMemsetAsync(a.stats, 0, sizeof(float) * 128 * kNumCU, stream));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}


// ---------------------------------------------------------------------------------------------
// bf16x6 convolution, register-resident weights and an interleaved pipeline ("bf3").
// conv64bf_kernel above runs its phases back to back on one wave per SIMD: matrix phase, epilogue, barrier, split +
// LDS write, barrier -- the matrix cores idle through every VALU phase (measured: 5.6 K of 14 K cycles per tile).
// Here wave (mt, nh) keeps the weight fragments of its 32 output rows in registers for the whole kernel
// (12 k-steps x 3 pieces x 4 VGPRs = 144 of the 512 a single resident wave may use), so LDS only carries the input
// image -- small enough (2 x 55 KB) to double-buffer.  While the matrix cores work on tile i out of image A, the
// same instruction stream, a few VALU/DS instructions after every MFMA, splits tile i+1 into image B and then
// issues the global loads of tile i+2: one LDS-only barrier per tile, output stores stay in flight across it.
// ---------------------------------------------------------------------------------------------
// H = true: the f16 two-piece build (pieces hi = f16(x), lo = f16(x - hi); three products lo hi, hi lo, hi hi on v_mfma_f32_32x32x16_f16;
// weight image from wm_pack_w64_h: w * ws with ws a power of two, the accumulators are multiplied by 1 / ws in the epilogue)
template <int PRO, int EPI, bool STATS, bool H = false>
__global__ __launch_bounds__(256) void conv64bf3_kernel(Conv64Args a) {
    constexpr int KW = 3, NT = 128, ROWS = NT + 2, PITCH = 72, NP = H ? 2 : 3, NC = 4;
    constexpr int XBUF = NP * ROWS * PITCH;               // bf16 elements per input image
    constexpr bool TWO = (PRO == PRO_BNBWD);
    constexpr bool E1 = (EPI == EPI_RELUMASK || EPI == EPI_ADD || EPI == EPI_BNADDRELU);
    extern __shared__ __align__(16) unsigned char smem_raw[];
    unsigned short* Xb0 = reinterpret_cast<unsigned short*>(smem_raw);             // 2 x [NP][ROWS][PITCH]
    float* Cs = reinterpret_cast<float*>(Xb0 + 2 * XBUF);                           // [6][64]
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform values stay in SGPRs (scalar address math)
    const int mt = wave & 1, nh = wave >> 1;
    const int T = a.T;                             // T % 128 == 0 (checked by the launcher): no partial tiles
    const int tilesPerClip = (T + NT - 1) / NT, ntiles = a.B * tilesPerClip;

    // ---- resident weight fragments: packed image [NP][KW][64 out][64 in] bf16
    u32x4 Wr[12][NP];
    {
        const uint4* wg = reinterpret_cast<const uint4*>(a.wp);
#pragma unroll
        for (int s = 0; s < 12; ++s)
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int e = ((p * KW + (s >> 2)) * 64 + 32 * mt + l31) * 64 + 16 * (s & 3) + 8 * half;
                u32x4 w_ = __builtin_bit_cast(u32x4, wg[e >> 3]);
#if WM_BF3_PIN_W
                // pinned to the AGPR half of the register file (the MFMA reads its A operand from there directly); left to the
                // allocator, the fragments beyond the VGPR budget are copied back (v_accvgpr_read) in front of their k-step
                asm volatile("" : "+a"(w_));
#endif
                Wr[s][p] = w_;
            }
    }
    const float winv = H ? reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(a.wp) + NP * KW * 4096)[1] : 1.f;
    const float wsc = H ? reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(a.wp) + NP * KW * 4096)[0] : 1.f;
    // ---- staging map (fixed per thread): channel pair cp = 8*wave + (lane & 7), time quads q = 8*i + (lane >> 3)
    const int cp = wave * 8 + (lane & 7), c0 = 2 * cp, q0 = lane >> 3;
    const int hc = (tid & 127) >> 1, hh = tid & 1;
    float4 sa[NC], sb[NC], sa2[TWO ? NC : 1], sb2[TWO ? NC : 1];
    float hl, hl2 = 0.f;
    // global -> register staging of one tile, in five pieces (4 combos + halo) so that the main loop can issue them
    // a few at a time: a 32-KB burst per CU backs up the memory pipeline and blocks the wave at issue for ~2.5 K cycles
    auto load_combo = [&](int tile, int i) {
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        const size_t o = ((size_t)b * 64 + c0) * T + t0 + 4 * (q0 + 8 * i);
        sa[i] = *reinterpret_cast<const float4*>(a.x + o);
        sb[i] = *reinterpret_cast<const float4*>(a.x + o + T);
        if (TWO) { sa2[i] = *reinterpret_cast<const float4*>(a.x2 + o); sb2[i] = *reinterpret_cast<const float4*>(a.x2 + o + T); }
    };
    auto load_halo = [&](int tile) {              // branch-free: clamped address, masked when written to LDS
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        const int ht = min(max(hh ? t0 + NT : t0 - 1, 0), T - 1);
        hl = a.x[((size_t)b * 64 + hc) * T + ht];
        if (TWO) hl2 = a.x2[((size_t)b * 64 + hc) * T + ht];
    };
    auto load_tile = [&](int tile) {
#pragma unroll
        for (int i = 0; i < NC; ++i) load_combo(tile, i);
        load_halo(tile);
    };

#if WM_TILE_CONTIG
    const int chunk = (ntiles + (int)gridDim.x - 1) / (int)gridDim.x, tstep = 1;
    int tile = blockIdx.x * chunk;
    const int tend = min(tile + chunk, ntiles);
#else
    const int tstep = gridDim.x, tend = ntiles;
    int tile = WM_XCD_MAP ? xcd_slot() : (int)blockIdx.x;        // grid <= ntiles
#endif
    load_tile(min(tile, ntiles - 1));
    if (tid < 64) {
        Cs[tid] = (PRO == PRO_BNRELU || PRO == PRO_BNBWD) ? a.pa[tid] : 0.f;
        Cs[64 + tid] = (PRO == PRO_BNRELU || PRO == PRO_BNBWD) ? a.pb[tid] : 0.f;
        Cs[128 + tid] = (PRO == PRO_BNBWD) ? a.pc[tid] : 0.f;
        Cs[192 + tid] = (PRO == PRO_BNBWD) ? a.pb[64 + tid] : (((EPI == EPI_BIAS || EPI == EPI_BNADDRELU) && a.bias) ? a.bias[tid] : 0.f);
        Cs[256 + tid] = (EPI == EPI_RELUMASK || EPI == EPI_BNADDRELU) ? a.ea[tid] : 0.f;
        Cs[320 + tid] = (EPI == EPI_RELUMASK || EPI == EPI_BNADDRELU) ? a.eb[tid] : 0.f;
    }
    __syncthreads();
    // per-thread prologue constants (the staging channels never change)
    const float ka0 = Cs[c0], ka1 = Cs[c0 + 1], kb0 = Cs[64 + c0], kb1 = Cs[64 + c0 + 1];
    const float kc0 = Cs[128 + c0], kc1 = Cs[128 + c0 + 1], kl0 = TWO ? Cs[192 + c0] : 0.f, kl1 = TWO ? Cs[192 + c0 + 1] : 0.f;
    const float ha = Cs[hc], hb = Cs[64 + hc], hcc = Cs[128 + hc], hlo = TWO ? Cs[192 + hc] : 0.f;

    // one (combo i, element e) unit of the split: two channels x one time step -> 3 dwords
    auto split_unit = [&](unsigned* X32, int t0, int i, int e) {
        const float4 fa = sa[i], fb = sb[i];
        float va = (e == 0) ? fa.x : (e == 1) ? fa.y : (e == 2) ? fa.z : fa.w;
        float vb = (e == 0) ? fb.x : (e == 1) ? fb.y : (e == 2) ? fb.z : fb.w;
        if (PRO != PRO_NONE) {
            float wa = 0.f, wb = 0.f;
            if (TWO) {
                const float4 ga = sa2[i], gb = sb2[i];
                wa = (e == 0) ? ga.x : (e == 1) ? ga.y : (e == 2) ? ga.z : ga.w;
                wb = (e == 0) ? gb.x : (e == 1) ? gb.y : (e == 2) ? gb.z : gb.w;
            }
            va = pro_apply<PRO>(va, wa, ka0, kb0, kc0, kl0);
            vb = pro_apply<PRO>(vb, wb, ka1, kb1, kc1, kl1);
        }
        const int o = (1 + 4 * (q0 + 8 * i) + e) * (PITCH / 2) + cp;
        if (H) {
            const h16x2 h_ = __builtin_convertvector(f32x2{va, vb}, h16x2);
            const h16x2 l_ = __builtin_convertvector(f32x2{va - (float)h_.x, vb - (float)h_.y}, h16x2);
            X32[o] = __builtin_bit_cast(unsigned, h_); X32[(ROWS * PITCH >> 1) + o] = __builtin_bit_cast(unsigned, l_);
        } else {
            unsigned p0, p1, p2;
            split3_pair(va, vb, p0, p1, p2);
            X32[o] = p0; X32[(ROWS * PITCH >> 1) + o] = p1; X32[2 * (ROWS * PITCH >> 1) + o] = p2;
        }
    };
    auto split_halo = [&](unsigned short* X, int t0) {
        {                                             // threads 128..255 repeat the writes of 0..127 (no branch)
            const int t = hh ? t0 + NT : t0 - 1;
            float v = hl;
            if (PRO != PRO_NONE) v = pro_apply<PRO>(v, hl2, ha, hb, hcc, hlo);
            if (t < 0 || t >= T) v = 0.f;
            const int o = (hh ? NT + 1 : 0) * PITCH + hc;
            if (H) {
                const _Float16 h_ = (_Float16)v;
                const _Float16 l_ = (_Float16)(v - (float)h_);
                X[o] = __builtin_bit_cast(unsigned short, h_); X[ROWS * PITCH + o] = __builtin_bit_cast(unsigned short, l_);
            } else {
                unsigned p0, p1, p2;
                split3_pair(v, 0.f, p0, p1, p2);
                X[o] = (unsigned short)p0; X[ROWS * PITCH + o] = (unsigned short)p1; X[2 * ROWS * PITCH + o] = (unsigned short)p2;
            }
        }
    };
    // the same split in stages, one per scheduling slice of the main loop (WM_BF3_MANUAL)
    float sva = 0.f, svb = 0.f;
    unsigned sp0 = 0, sp1 = 0;
    auto split_pick = [&](int i, int e) {
        const float4 fa = sa[i], fb = sb[i];
        float va = (e == 0) ? fa.x : (e == 1) ? fa.y : (e == 2) ? fa.z : fa.w;
        float vb = (e == 0) ? fb.x : (e == 1) ? fb.y : (e == 2) ? fb.z : fb.w;
        if (PRO != PRO_NONE) {
            float wa = 0.f, wb = 0.f;
            if (TWO) {
                const float4 ga = sa2[i], gb = sb2[i];
                wa = (e == 0) ? ga.x : (e == 1) ? ga.y : (e == 2) ? ga.z : ga.w;
                wb = (e == 0) ? gb.x : (e == 1) ? gb.y : (e == 2) ? gb.z : gb.w;
            }
            va = pro_apply<PRO>(va, wa, ka0, kb0, kc0, kl0);
            vb = pro_apply<PRO>(vb, wb, ka1, kb1, kc1, kl1);
        }
        sva = va; svb = vb;
        asm volatile("" : "+v"(sva), "+v"(svb));
    };
    auto split_st1 = [&]() {
        if (H) {
            const h16x2 hh_ = __builtin_convertvector(f32x2{sva, svb}, h16x2);
            sp0 = __builtin_bit_cast(unsigned, hh_);
            sva -= (float)hh_.x; svb -= (float)hh_.y;
        } else {
            const bf16x2 hh_ = {(__bf16)sva, (__bf16)svb};
            sp0 = __builtin_bit_cast(unsigned, hh_);
            sva -= __uint_as_float(sp0 << 16); svb -= __uint_as_float(sp0 & 0xffff0000u);
        }
        asm volatile("" : "+v"(sva), "+v"(svb), "+v"(sp0));
    };
    auto split_st2 = [&]() {
        if (H) return;                                   // two pieces: no middle one
        const bf16x2 mm_ = {(__bf16)sva, (__bf16)svb};
        sp1 = __builtin_bit_cast(unsigned, mm_);
        sva -= __uint_as_float(sp1 << 16); svb -= __uint_as_float(sp1 & 0xffff0000u);
        asm volatile("" : "+v"(sva), "+v"(svb), "+v"(sp1));
    };
    auto last_piece = [&]() -> unsigned {
        if (H) return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{sva, svb}, h16x2));
        const bf16x2 ll_ = {(__bf16)sva, (__bf16)svb};
        return __builtin_bit_cast(unsigned, ll_);
    };
    auto split_out = [&](unsigned* X32, int i, int e) {
        const unsigned sp2 = last_piece();
        const int o = (1 + 4 * (q0 + 8 * i) + e) * (PITCH / 2) + cp;
        X32[o] = sp0; if (!H) X32[(ROWS * PITCH >> 1) + o] = sp1; X32[(NP - 1) * (ROWS * PITCH >> 1) + o] = sp2;
    };
    auto halo_pick = [&](int t0) {
        const int t = hh ? t0 + NT : t0 - 1;
        float v = hl;
        if (PRO != PRO_NONE) v = pro_apply<PRO>(v, hl2, ha, hb, hcc, hlo);
        if (t < 0 || t >= T) v = 0.f;
        sva = v; svb = 0.f;
        asm volatile("" : "+v"(sva), "+v"(svb));
    };
    auto halo_out = [&](unsigned short* X) {
        const unsigned sp2 = last_piece();
        const int o = (hh ? NT + 1 : 0) * PITCH + hc;
        X[o] = (unsigned short)sp0; if (!H) X[ROWS * PITCH + o] = (unsigned short)sp1; X[(NP - 1) * ROWS * PITCH + o] = (unsigned short)sp2;
    };
    {
        const int t0 = (min(tile, ntiles - 1) % tilesPerClip) * NT;
#pragma unroll
        for (int u = 0; u < 16; ++u) split_unit(reinterpret_cast<unsigned*>(Xb0), t0, u >> 2, u & 3);
        split_halo(Xb0, t0);
    }
    load_tile(min(tile + tstep, ntiles - 1));
    __syncthreads();
    // nothing pending on entry: the loop's vmcnt waits are then derived from its own (steady-state) issue order only
    __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0)

    float s1[STATS ? 16 : 1], s2[STATS ? 16 : 1];
    if (STATS) {
#pragma unroll
        for (int j = 0; j < 16; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    }
    int buf = 0;
#ifdef WM_STAMP
    unsigned long long tm[6] = {0, 0, 0, 0, 0, 0};
#endif
    // The epilogue of a tile is deferred into the matrix phase of the NEXT tile (accp = its accumulators): the
    // output stores trickle out between MFMAs instead of arriving as one 8-MB burst from all 256 CUs at once.
    f32x16 accp[2];
    // "previous tile" of the first iteration = the first tile itself with accumulators that make its epilogue values ZERO (minus
    // the bias where one is added): they are stored (and overwritten one iteration later by the same lanes, in program order) and
    // add nothing to the sums -- no flag, no extra multiply per value
    int pb_ = min(tile, ntiles - 1) / tilesPerClip, pt0 = (min(tile, ntiles - 1) % tilesPerClip) * NT;
    bool any_tile = false;
    float e1r[E1 ? 32 : 1];
    // per-row epilogue constants of this lane's 16 accumulator rows, in registers: an LDS read inside an epilogue slice stalls
    // the wave for the whole LDS latency in front of the next MFMA
    constexpr bool KB = (EPI == EPI_BIAS || EPI == EPI_BNADDRELU), KE = (EPI == EPI_RELUMASK || EPI == EPI_BNADDRELU);
    float kbias[KB ? 16 : 1], kea[KE ? 16 : 1], keb[KE ? 16 : 1];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = 32 * mt + mfma_row(r, half);
        if (KB) kbias[r] = Cs[192 + co];
        if (KE) { kea[r] = Cs[256 + co]; keb[r] = Cs[320 + co]; }
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) accp[nt][r] = (EPI == EPI_BIAS) ? -kbias[r] * wsc : 0.f;       // wsc: a power of two (exact)
    // output / epilogue-operand addressing through buffer descriptors over the wave's 32 channel rows of a clip: per-lane offset
    // = column, scalar offset = row (sixteen loop-invariant scalars), the column block nt as the immediate -- one instruction per
    // value instead of a 64-bit scalar add, a 64-bit vector add and the access
    const unsigned lcol = (unsigned)(4 * half * T + l31) * 4u;
    unsigned rowT[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) rowT[r] = (unsigned)(((r & 3) + 8 * (r >> 2)) * T) * 4u;
    auto row_srd = [&](const float* base, int cb) { return make_srd(base + ((size_t)cb * 64 + 32 * mt) * T, (size_t)32 * T * sizeof(float)); };
    wm_srd_t syp = row_srd(a.y, pb_);                         // output rows of the PREVIOUS tile's clip
    unsigned vcolp = lcol + (unsigned)(pt0 + 64 * nh) * 4u;
    if (E1) {
#pragma unroll
        for (int j = 0; j < 32; ++j) e1r[j] = 0.f;
    }
    // epilogue of value idx = nt * 16 + r of the previous tile; se1c / vcolc = the tile being computed now, whose epilogue
    // operand replaces the consumed one in the same register (it is needed one full iteration from now)
    auto epi_value = [&](int idx, bool fetch, const wm_srd_t& se1c, unsigned vcolc) {
        const int nt = idx >> 4, r = idx & 15;
        float v = accp[nt][r];
        float q = 0.f;
        if (H) v *= winv;                               // exact (power of two); contracts with the bias add
        if (EPI == EPI_BIAS) v += kbias[r];
        if (EPI == EPI_RELUMASK) { q = e1r[idx]; v = (fmaf(q, kea[r], keb[r]) > 0.f) ? v : 0.f; }
        if (EPI == EPI_ADD) v += e1r[idx];
        if (EPI == EPI_BNADDRELU) v = fmaxf(e1r[idx] + fmaf(v + kbias[r], kea[r], keb[r]), 0.f);   // = wm_bn_add_relu of the biased conv
        buf_store(syp, v, vcolp + 128u * nt, rowT[r]);
        if (STATS) { s1[r] += v; s2[r] = fmaf(v, (EPI == EPI_RELUMASK) ? q : v, s2[r]); }
#if WM_BF3_MANUAL
        if (STATS) asm volatile("" : "+v"(s1[r]), "+v"(s2[r]));
#endif
        if (E1 && fetch) e1r[idx] = buf_load(se1c, vcolc + 128u * nt, rowT[r]);
    };
    auto mma = [&](const u32x4& A_, const u32x4& B_, f32x16 c) -> f32x16 {
        if (H) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, A_), __builtin_bit_cast(h16x8, B_), c, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A_), __builtin_bit_cast(bf16x8, B_), c, 0, 0, 0);
    };
    while (tile < tend) {
        STAMP(ts0);
        // tiles past the end are clamped: their (valid) data lands in the image nobody reads again
        const int next = min(tile + tstep, ntiles - 1), next2 = min(tile + 2 * tstep, ntiles - 1);
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        const int nt0 = (next % tilesPerClip) * NT;
        const wm_srd_t se1c = E1 ? row_srd(a.e1, b) : syp;
        const unsigned vcolc = lcol + (unsigned)(t0 + 64 * nh) * 4u;
        const unsigned short* xcur = Xb0 + buf * XBUF;
        unsigned short* xnxt = Xb0 + (buf ^ 1) * XBUF;
        f32x16 acc[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
        const unsigned short* xrow = xcur + (64 * nh + l31) * PITCH + 8 * half;
        u32x4 Bq[2][NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) Bq[0][p] = *reinterpret_cast<const u32x4*>(xrow + p * ROWS * PITCH);
#if WM_BF3_MANUAL
        // Hand-pinned schedule: every MFMA is followed by one slice of the side work (sched_barrier fences; the arithmetic of a
        // slice is tied to it by an empty asm on its results).  The six MFMAs of a half-step chain on one accumulator, each
        // waiting 8 passes for its predecessor, so a slice of <= 8 VALU instructions between two of them costs nothing.  The
        // group-barrier pattern of the other branch leaves lumps of 30-40 instructions in front of back-to-back MFMAs.
#define FENCE __builtin_amdgcn_sched_barrier(0)
#define BF3_SLICE(k)                                                                                                        \
    {                                                                                                                           \
        if (h < 16) {                                                                                                           \
            if ((k) == 0) split_pick(h >> 2, h & 3);                                                                            \
            if ((k) == 1) split_st1();                                                                                          \
            if ((k) == 2) split_st2();                                                                                          \
            if ((k) == 3) { split_out(reinterpret_cast<unsigned*>(xnxt), h >> 2, h & 3); if ((h & 3) == 3) load_combo(next2, h >> 2); } \
        } else if (h == 16) {                                                                                                   \
            if ((k) == 0) halo_pick(nt0);                                                                                       \
            if ((k) == 1) split_st1();                                                                                          \
            if ((k) == 2) split_st2();                                                                                          \
            if ((k) == 3) halo_out(xnxt);                                                                                       \
        } else if (h == 17) {                                                                                                   \
            if ((k) == 0) load_halo(next2);                                                                                     \
        }                                                                                                                       \
        if (h < 8) {                                                                                                            \
            if ((k) == 4) epi_value(2 * h, true, se1c, vcolc);                                                                              \
            if ((k) == 5) epi_value(2 * h + 1, true, se1c, vcolc);                                                                          \
        } else if ((k) == 4) epi_value(8 + h, true, se1c, vcolc);                                                                           \
    }
#pragma unroll
        for (int h = 0; h < 24; ++h) {
            const int s = h >> 1, nt = h & 1;
            if (h + 1 < 24) {
                const int s1_ = (h + 1) >> 1, n1 = (h + 1) & 1;
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    Bq[(h + 1) & 1][p] = *reinterpret_cast<const u32x4*>(xrow + (p * ROWS + 32 * n1 + (s1_ >> 2)) * PITCH + 16 * (s1_ & 3));
            }
            const u32x4* Bf = Bq[h & 1];
            FENCE;
            if (H) {                                     // lo hi, hi lo, hi hi: two slices behind every MFMA
                acc[nt] = mma(Wr[s][1], Bf[0], acc[nt]); FENCE; BF3_SLICE(0) FENCE; BF3_SLICE(1) FENCE;
                acc[nt] = mma(Wr[s][0], Bf[1], acc[nt]); FENCE; BF3_SLICE(3) FENCE; BF3_SLICE(4) FENCE;
                acc[nt] = mma(Wr[s][0], Bf[0], acc[nt]); FENCE; BF3_SLICE(5) FENCE;
            } else {
                acc[nt] = mma(Wr[s][1], Bf[1], acc[nt]); FENCE; BF3_SLICE(0) FENCE;
                acc[nt] = mma(Wr[s][0], Bf[2], acc[nt]); FENCE; BF3_SLICE(1) FENCE;
                acc[nt] = mma(Wr[s][2], Bf[0], acc[nt]); FENCE; BF3_SLICE(2) FENCE;
                acc[nt] = mma(Wr[s][0], Bf[1], acc[nt]); FENCE; BF3_SLICE(3) FENCE;
                acc[nt] = mma(Wr[s][1], Bf[0], acc[nt]); FENCE; BF3_SLICE(4) FENCE;
                acc[nt] = mma(Wr[s][0], Bf[0], acc[nt]); FENCE; BF3_SLICE(5) FENCE;
            }
#ifdef WM_STAMP
#ifdef WM_STAMP_FINE
            if (h == 16) { STAMP(tsa); tm[0] += tsa - ts0; }
            if (h == 17) { STAMP(tsb); tm[1] += tsb - ts0; }
            if (h == 18) { STAMP(tsb); tm[3] += tsb - ts0; }
            if (h == 20) { STAMP(tsb); tm[5] += tsb - ts0; }
#else
            if (h == 3) { STAMP(tsa); tm[0] += tsa - ts0; }
            if (h == 15) { STAMP(tsb); tm[1] += tsb - ts0; }
#endif
#endif
        }
#undef FENCE
#undef BF3_SLICE
#else
#pragma unroll
        for (int h = 0; h < 24; ++h) {
            const int s = h >> 1, nt = h & 1;
            if (h + 1 < 24) {
                const int s1_ = (h + 1) >> 1, n1 = (h + 1) & 1;
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    Bq[(h + 1) & 1][p] = *reinterpret_cast<const u32x4*>(xrow + (p * ROWS + 32 * n1 + (s1_ >> 2)) * PITCH + 16 * (s1_ & 3));
            }
            const u32x4* Bf = Bq[h & 1];
            static_assert(!H, "the f16 build exists in the hand-pinned schedule only");
            acc[nt] = mma(Wr[s][1], Bf[1], acc[nt]);
            acc[nt] = mma(Wr[s][0], Bf[2], acc[nt]);
            acc[nt] = mma(Wr[s][2], Bf[0], acc[nt]);
            acc[nt] = mma(Wr[s][0], Bf[1], acc[nt]);
            acc[nt] = mma(Wr[s][1], Bf[0], acc[nt]);
            acc[nt] = mma(Wr[s][0], Bf[0], acc[nt]);
            // side work of this half-step
            if (h < 16) {
                split_unit(reinterpret_cast<unsigned*>(xnxt), nt0, h >> 2, h & 3);
                if ((h & 3) == 3) load_combo(next2, h >> 2);          // this combo's registers are free again
            } else if (h == 16) split_halo(xnxt, nt0);
            else if (h == 17) load_halo(next2);
            if (h < 8) { epi_value(2 * h, true, se1c, vcolc); epi_value(2 * h + 1, true, se1c, vcolc); }
            else epi_value(8 + h, true, se1c, vcolc);
            // interleave: after the fragment reads, one MFMA then a handful of the side instructions, six times
            __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
#pragma unroll
            for (int kk = 0; kk < 6; ++kk) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);
                __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x040, 1, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
#ifdef WM_STAMP
#ifdef WM_STAMP_FINE
            if (h == 16) { STAMP(tsa); tm[0] += tsa - ts0; }
            if (h == 17) { STAMP(tsb); tm[1] += tsb - ts0; }
            if (h == 18) { STAMP(tsb); tm[3] += tsb - ts0; }
            if (h == 20) { STAMP(tsb); tm[5] += tsb - ts0; }
#else
            if (h == 3) { STAMP(tsa); tm[0] += tsa - ts0; }
            if (h == 15) { STAMP(tsb); tm[1] += tsb - ts0; }
#endif
#endif
        }
#endif
        STAMP(ts1);
        accp[0] = acc[0]; accp[1] = acc[1];
        pb_ = b; pt0 = t0; any_tile = true;
        syp = row_srd(a.y, b); vcolp = vcolc;
        STAMP(ts2);
        lds_barrier();
        STAMP(ts3);
#ifdef WM_STAMP
#ifdef WM_STAMP_FINE
        tm[2] += ts1 - ts0; tm[4] += ts3 - ts2;
#else
        tm[2] += ts1 - ts0; tm[3] += ts2 - ts1; tm[4] += ts3 - ts2;
#endif
#endif
        tile += tstep;
        buf ^= 1;
    }
#ifdef WM_STAMP
    if (g_wm_stamp && lane == 0) {
        unsigned long long* d = g_wm_stamp + ((size_t)blockIdx.x * 4 + wave) * 6;
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = tm[i];
    }
#endif
    if (any_tile) {                                  // flush: the last tile's epilogue (its operand is already in e1r)
#pragma unroll
        for (int idx = 0; idx < 32; ++idx) epi_value(idx, false, syp, 0u);
    }
    if (STATS) {
        float* red = reinterpret_cast<float*>(Xb0);          // [2 column halves][2][64]
#pragma unroll
        for (int j = 0; j < 16; ++j) { s1[j] = half_wave_sum(s1[j]); s2[j] = half_wave_sum(s2[j]); }
        __syncthreads();
        if (l31 == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = 32 * mt + mfma_row(r, half);
                red[nh * 128 + co] = s1[r];
                red[nh * 128 + 64 + co] = s2[r];
            }
        }
        __syncthreads();
        if (tid < 128) a.stats[(size_t)blockIdx.x * 128 + tid] = red[tid] + red[128 + tid];
    }
}

template <int PRO, int EPI, bool STATS, bool H = false>
int launch_conv64bf3(const Conv64Args& a, hipStream_t stream) {
    constexpr size_t lds = (size_t)(2 * (H ? 2 : 3) * 130 * 72) * 2 + 6 * 64 * sizeof(float);
    static wm::DevOnce attr_done;
    auto kern = conv64bf3_kernel<PRO, EPI, STATS, H>;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(kern), lds, attr_done)) return rc;
    const int ntiles = a.B * ((a.T + 127) / 128);
    const int grid = ntiles < kNumCU ? ntiles : kNumCU;
    if (STATS && grid < kNumCU) WM_TRY(hipMemsetAsync(a.stats, 0, sizeof(float) * 128 * kNumCU, stream));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}


// ---------------------------------------------------------------------------------------------
// bf16x6 build of the 7-tap convolution (Generator.decoder[0] = ConvTranspose1d(64,64,7,padding=3), py/main16.py:144,
// forward and data gradient).  The 3-piece image of all 7 taps is 194 KB -- more than LDS -- so a workgroup keeps the
// taps of HALF the output channels (97 KB) and the (tile, half) pairs are dealt over the grid: workgroup g owns half
// g & 1 for its whole life.  The input tile is read by two workgroups (8 MB/clip extra on a kernel that moves 8 MB per
// 918 MFLOP: still far from HBM-bound); each of the four waves owns 32 columns of the 32 x 128 output tile.
// ---------------------------------------------------------------------------------------------
template <int PRO, int EPI>
__global__ __launch_bounds__(256) void conv64bf7_kernel(Conv64Args a) {
    constexpr int KW = 7, PAD = 3, NT = 128, ROWS = NT + 2 * PAD, PITCH = 72, NP = 3, NC = 4, MR = 32;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    unsigned short* Wb = reinterpret_cast<unsigned short*>(smem_raw);              // [NP][KW][MR][PITCH]
    unsigned short* Xb = Wb + NP * KW * MR * PITCH;                                // [NP][ROWS][PITCH]
    float* Cs = reinterpret_cast<float*>(Xb + NP * ROWS * PITCH);                  // [32] bias of this half
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int mh = blockIdx.x & 1, nslots = gridDim.x >> 1;                        // gridDim.x is even
    const int T = a.T;
    const int tilesPerClip = (T + NT - 1) / NT, ntiles = a.B * tilesPerClip;

    float4 sa[NC], sb[NC];
    float hl[2];
    float pv0[NC], pv1[NC], hv[2];                // ADDVEC: the clip's embedding values, prefetched with the tile (a load
                                                  // inside write_tile would put a global round trip into the serial phase)
    auto combo = [&](int i, int& cp, int& q) {
        const int idx = tid + i * 256, widx = idx >> 6, l = idx & 63;
        cp = (widx & 3) * 8 + (l & 7);
        q = (widx >> 2) * 8 + (l >> 3);
    };
    auto halo_of = [&](int k, int t0, int& c, int& r, int& t) {                    // k-th halo element of this thread
        const int idx = min(tid + k * 256, 64 * 2 * PAD - 1);
        c = idx / (2 * PAD);
        const int h = idx % (2 * PAD);
        r = (h < PAD) ? h : NT + h;                                                 // image row: time = t0 - PAD + r
        t = t0 - PAD + r;
    };
    // piece i < NC: one staging combo; piece NC: the halo.  Branch-free (clamped addresses, masked at the LDS write); the
    // main loop issues one piece per tap so that the tile's loads never arrive at the memory pipeline as one burst
    auto load_piece = [&](int tile, int i) {
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        const float* xb = a.x + (size_t)b * 64 * T;
        if (i < NC) {
            int cp, q;
            combo(i, cp, q);
            const size_t o = (size_t)(2 * cp) * T + min(t0 + 4 * q, T - 4);
            sa[i] = *reinterpret_cast<const float4*>(xb + o);
            sb[i] = *reinterpret_cast<const float4*>(xb + o + T);
            if (PRO == PRO_ADDVEC) { pv0[i] = a.pa[b * 64 + 2 * cp]; pv1[i] = a.pa[b * 64 + 2 * cp + 1]; }
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                int c, r, t;
                halo_of(k, t0, c, r, t);
                hl[k] = xb[(size_t)c * T + min(max(t, 0), T - 1)];
                if (PRO == PRO_ADDVEC) hv[k] = a.pa[b * 64 + c];
            }
        }
    };
    auto load_tile = [&](int tile) {
#pragma unroll
        for (int i = 0; i <= NC; ++i) load_piece(tile, i);
    };
    auto write_tile = [&](int tile) {
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        unsigned* X32 = reinterpret_cast<unsigned*>(Xb);
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            int cp, q;
            combo(i, cp, q);
            const int c = 2 * cp, t = t0 + 4 * q;
            float va[4] = {sa[i].x, sa[i].y, sa[i].z, sa[i].w}, vb[4] = {sb[i].x, sb[i].y, sb[i].z, sb[i].w};
            if (PRO == PRO_ADDVEC) {
                const float v0 = pv0[i], v1 = pv1[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) { va[e] += v0; vb[e] += v1; }
            }
            const bool ok = t < T;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned p0, p1, p2;
                split3_pair(ok ? va[e] : 0.f, ok ? vb[e] : 0.f, p0, p1, p2);
                const int o = ((PAD + 4 * q + e) * PITCH + c) >> 1;
                X32[o] = p0; X32[(ROWS * PITCH >> 1) + o] = p1; X32[2 * (ROWS * PITCH >> 1) + o] = p2;
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (tid + k * 256 < 64 * 2 * PAD) {
                int c, r, t;
                halo_of(k, t0, c, r, t);
                float v = hl[k];
                if (PRO == PRO_ADDVEC) v += hv[k];
                if (t < 0 || t >= T) v = 0.f;
                unsigned p0, p1, p2;
                split3_pair(v, 0.f, p0, p1, p2);
                const int o = r * PITCH + c;
                Xb[o] = (unsigned short)p0; Xb[ROWS * PITCH + o] = (unsigned short)p1; Xb[2 * ROWS * PITCH + o] = (unsigned short)p2;
            }
        }
    };

    int tile = blockIdx.x >> 1;
    if (tile < ntiles) load_tile(tile);
    // resident weights of this half: global image [NP][KW][64 out][64 in] bf16 -> LDS [NP][KW][32][PITCH]
    for (int i = tid; i < NP * KW * MR * 8; i += 256) {
        const int row = i >> 3, seg = i & 7, pt = row / MR, o = row % MR;
        *reinterpret_cast<uint4*>(Wb + row * PITCH + seg * 8) = reinterpret_cast<const uint4*>(a.wp)[(pt * 64 + mh * MR + o) * 8 + seg];
    }
    if (tid < MR) Cs[tid] = (EPI == EPI_BIAS && a.bias) ? a.bias[mh * MR + tid] : 0.f;
    __syncthreads();
    if (tile < ntiles) write_tile(tile);
    __syncthreads();

    while (tile < ntiles) {
        const int next = tile + nslots, nextc = min(next, ntiles - 1);   // clamped: loaded (valid memory) but never written
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        const int tcol = t0 + wave * 32 + l31;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const unsigned short* wbase = Wb + l31 * PITCH + 8 * half;
        const unsigned short* xbase = Xb + (wave * 32 + l31) * PITCH + 8 * half;
#pragma unroll
        for (int tap = 0; tap < KW; ++tap) {
            if (tap >= 1 && tap <= NC + 1) load_piece(nextc, tap - 1);
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                bf16x8 A[NP], Bf[NP];
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    Bf[p] = *reinterpret_cast<const bf16x8*>(xbase + (p * ROWS + tap) * PITCH + 16 * ch);
                    A[p] = *reinterpret_cast<const bf16x8*>(wbase + ((p * KW + tap) * MR) * PITCH + 16 * ch);
                }
                acc = mfma_bf16x6(A, Bf, acc);
            }
        }
        float* yb = a.y + ((size_t)b * 64 + mh * MR) * T + tcol;
        if (tcol < T) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = mfma_row(r, half);
                yb[(size_t)row * T] = acc[r] + Cs[row];
            }
        }
        __syncthreads();
        if (next < ntiles) write_tile(next);
        __syncthreads();
        tile = next;
    }
}

template <int PRO, int EPI>
int launch_conv64bf7(const Conv64Args& a, hipStream_t stream) {
    constexpr size_t lds = (size_t)(3 * 7 * 32 * 72 + 3 * 134 * 72) * 2 + 32 * sizeof(float);
    static wm::DevOnce attr_done;
    auto kern = conv64bf7_kernel<PRO, EPI>;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(kern), lds, attr_done)) return rc;
    const int ntiles = a.B * ((a.T + 127) / 128);
    const int grid = 2 * (ntiles < kNumCU / 2 ? ntiles : kNumCU / 2);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}

// bf16 three-piece image [piece][tap][out][in] of a 7-tap ConvTranspose1d weight w[in][out][7]: mode 2 forward, 3 dgrad
// ---------------------------------------------------------------------------------------------
// Pipelined build of the 7-tap convolution (conv64bf3_kernel's scheme with KW = 7).  conv64bf7_kernel above keeps the
// weight image in LDS (97 KB per output half), so two workgroups split every input tile twice and the matrix cores idle
// through each split phase.  Here wave (mt, nh) keeps the weight fragments of its 32 output rows in REGISTERS for the whole
// kernel (28 k-steps x 3 pieces x 4 = 336 of the 512 a lone resident wave may use), one workgroup computes all 64 rows of
// a 128-column tile (336 MFMAs per wave), and LDS only carries the input image, double-buffered (2 x 58 KB): the split of
// tile i+1 and the fetch of tile i+2 ride, one hand-pinned slice per MFMA, in the matrix phase of tile i.  T % 128 == 0.
// ---------------------------------------------------------------------------------------------
// H = true: f16 two-piece build (three products per product; weight image from wm_pack_w64_h7: w * ws; a.pb, when given, = {gs, 1 / gs}:
// the input -- a gradient -- is multiplied by gs before the split and clamped to the f16 range; the accumulators leave times 1 / (ws gs))
template <int PRO, int EPI, bool H = false>
__global__ __launch_bounds__(256) void conv64bf7p_kernel(Conv64Args a) {
    static_assert(PRO == PRO_NONE || PRO == PRO_ADDVEC, "prologue: none or + vec[b][c]");
    constexpr int KW = 7, PAD = 3, NT = 128, ROWS = NT + 2 * PAD, PITCH = 72, NP = H ? 2 : 3, NC = 4, NS = KW * 4;
    constexpr int XBUF = NP * ROWS * PITCH;               // bf16 elements per input image
    extern __shared__ __align__(16) unsigned char smem_raw[];
    unsigned short* Xb0 = reinterpret_cast<unsigned short*>(smem_raw);             // 2 x [NP][ROWS][PITCH]
    float* Cs = reinterpret_cast<float*>(Xb0 + 2 * XBUF);                           // [64] bias
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mt = wave & 1, nh = wave >> 1;
    const int T = a.T;                             // T % 128 == 0 (checked by the launcher): no partial tiles
    const int tilesPerClip = T / NT, ntiles = a.B * tilesPerClip;

    // ---- resident weight fragments: packed image [NP][KW][64 out][64 in] bf16; k-step s = tap * 4 + 16-channel block
    u32x4 Wr[NS][NP];
    {
        const uint4* wg = reinterpret_cast<const uint4*>(a.wp);
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int e = ((p * KW + (s >> 2)) * 64 + 32 * mt + l31) * 64 + 16 * (s & 3) + 8 * half;
                u32x4 w_ = __builtin_bit_cast(u32x4, wg[e >> 3]);
                if (s >= 8) asm volatile("" : "+a"(w_));      // 336 fragment registers: all but the first 8 k-steps pinned into AGPRs,
                Wr[s][p] = w_;                                 // where the MFMA reads them in place (no spill / copy-back traffic)
            }
    }
    float gs = 1.f, dinv = 1.f;                    // H: input scale, output scale
    if (H) {
        const float* tail = reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(a.wp) + NP * KW * 4096);
        dinv = tail[1];
        if (a.pb) { gs = a.pb[0]; dinv *= a.pb[1]; }
    }
    // ---- staging map (fixed per thread): channel pair cp, time quads q0 + 8 i; halo element k: channel hcn[k], image row hr[k]
    const int cp = wave * 8 + (lane & 7), c0 = 2 * cp, q0 = lane >> 3;
    int hcn[2], hr[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int idx = min(tid + k * 256, 64 * 2 * PAD - 1), h = idx % (2 * PAD);
        hcn[k] = idx / (2 * PAD);
        hr[k] = (h < PAD) ? h : NT + h;                                             // time = t0 - PAD + row
    }
    float4 sa[NC], sb[NC];
    float hl[2];
    float pv0 = 0.f, pv1 = 0.f, hv[2] = {0.f, 0.f};      // ADDVEC: the embedding values of the clip whose tile sits in the registers
    float nv0 = 0.f, nv1 = 0.f, nhv[2] = {0.f, 0.f};     // ... and of the tile being fetched
    auto load_combo = [&](int tile, int i) {
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        const size_t o = ((size_t)b * 64 + c0) * T + t0 + 4 * (q0 + 8 * i);
        sa[i] = *reinterpret_cast<const float4*>(a.x + o);
        sb[i] = *reinterpret_cast<const float4*>(a.x + o + T);
    };
    auto load_halo = [&](int tile) {              // branch-free: clamped addresses, masked when written to LDS
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            hl[k] = a.x[((size_t)b * 64 + hcn[k]) * T + min(max(t0 - PAD + hr[k], 0), T - 1)];
            if (PRO == PRO_ADDVEC) nhv[k] = a.pa[b * 64 + hcn[k]];
        }
        if (PRO == PRO_ADDVEC) { nv0 = a.pa[b * 64 + c0]; nv1 = a.pa[b * 64 + c0 + 1]; }
    };

    const int tstep = gridDim.x;
    int tile = WM_XCD_MAP ? xcd_slot() : (int)blockIdx.x;        // grid <= ntiles
#pragma unroll
    for (int i = 0; i < NC; ++i) load_combo(tile, i);
    load_halo(tile);
    if (tid < 64) Cs[tid] = (EPI == EPI_BIAS && a.bias) ? a.bias[tid] : 0.f;

    // ---- the split of one (combo i, element e) unit = two channels x one time step, in four stages (one slice each)
    float sva = 0.f, svb = 0.f;
    unsigned sp0 = 0, sp1 = 0;
    auto split_pick = [&](int i, int e) {
        const float4 fa = sa[i], fb = sb[i];
        float va = (e == 0) ? fa.x : (e == 1) ? fa.y : (e == 2) ? fa.z : fa.w;
        float vb = (e == 0) ? fb.x : (e == 1) ? fb.y : (e == 2) ? fb.z : fb.w;
        if (PRO == PRO_ADDVEC) { va += pv0; vb += pv1; }
        if (H) { va = __builtin_amdgcn_fmed3f(va * gs, -6.0e4f, 6.0e4f); vb = __builtin_amdgcn_fmed3f(vb * gs, -6.0e4f, 6.0e4f); }
        sva = va; svb = vb;
        asm volatile("" : "+v"(sva), "+v"(svb));
    };
    auto split_st1 = [&]() {
        if (H) {
            const h16x2 h_ = __builtin_convertvector(f32x2{sva, svb}, h16x2);
            sp0 = __builtin_bit_cast(unsigned, h_);
            sva -= (float)h_.x; svb -= (float)h_.y;
        } else {
            const bf16x2 h_ = {(__bf16)sva, (__bf16)svb};
            sp0 = __builtin_bit_cast(unsigned, h_);
            sva -= __uint_as_float(sp0 << 16); svb -= __uint_as_float(sp0 & 0xffff0000u);
        }
        asm volatile("" : "+v"(sva), "+v"(svb), "+v"(sp0));
    };
    auto last_piece = [&]() -> unsigned {
        if (H) return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{sva, svb}, h16x2));
        const bf16x2 l_ = {(__bf16)sva, (__bf16)svb};
        return __builtin_bit_cast(unsigned, l_);
    };
    auto split_st2 = [&]() {
        if (H) return;                                   // two pieces: no middle one
        const bf16x2 m_ = {(__bf16)sva, (__bf16)svb};
        sp1 = __builtin_bit_cast(unsigned, m_);
        sva -= __uint_as_float(sp1 << 16); svb -= __uint_as_float(sp1 & 0xffff0000u);
        asm volatile("" : "+v"(sva), "+v"(svb), "+v"(sp1));
    };
    auto split_out = [&](unsigned short* X, int i, int e) {
        const unsigned sp2 = last_piece();
        unsigned* X32 = reinterpret_cast<unsigned*>(X);
        const int o = (PAD + 4 * (q0 + 8 * i) + e) * (PITCH / 2) + cp;
        X32[o] = sp0; if (!H) X32[(ROWS * PITCH >> 1) + o] = sp1; X32[(NP - 1) * (ROWS * PITCH >> 1) + o] = sp2;
    };
    auto halo_pick = [&](int t0, int k) {
        const int t = t0 - PAD + hr[k];
        float v = hl[k];
        if (PRO == PRO_ADDVEC) v += hv[k];
        if (H) v = __builtin_amdgcn_fmed3f(v * gs, -6.0e4f, 6.0e4f);
        sva = (t < 0 || t >= T) ? 0.f : v; svb = 0.f;
        asm volatile("" : "+v"(sva), "+v"(svb));
    };
    auto halo_out = [&](unsigned short* X, int k) {
        const unsigned sp2 = last_piece();
        if (tid + k * 256 < 64 * 2 * PAD) {
            const int o = hr[k] * PITCH + hcn[k];
            X[o] = (unsigned short)sp0; if (!H) X[ROWS * PITCH + o] = (unsigned short)sp1; X[(NP - 1) * ROWS * PITCH + o] = (unsigned short)sp2;
        }
    };
    {   // first tile: split serially, then fetch the second
        const int t0 = (tile % tilesPerClip) * NT;
        pv0 = nv0; pv1 = nv1; hv[0] = nhv[0]; hv[1] = nhv[1];
#pragma unroll
        for (int u = 0; u < 16; ++u) { split_pick(u >> 2, u & 3); split_st1(); split_st2(); split_out(Xb0, u >> 2, u & 3); }
#pragma unroll
        for (int k = 0; k < 2; ++k) { halo_pick(t0, k); split_st1(); split_st2(); halo_out(Xb0, k); }
        const int nx = min(tile + tstep, ntiles - 1);
#pragma unroll
        for (int i = 0; i < NC; ++i) load_combo(nx, i);
        load_halo(nx);
    }
    __syncthreads();

    int buf = 0;
    auto mma = [&](const u32x4& A_, const u32x4& B_, f32x16 c) -> f32x16 {
        if (H) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, A_), __builtin_bit_cast(h16x8, B_), c, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A_), __builtin_bit_cast(bf16x8, B_), c, 0, 0, 0);
    };
#define FENCE __builtin_amdgcn_sched_barrier(0)
    while (tile < ntiles) {
        // registers: the operands of tile + tstep (clamped: a tile past the end lands in the image nobody reads again)
        const int next = min(tile + tstep, ntiles - 1), next2 = min(tile + 2 * tstep, ntiles - 1);
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        const int nt0 = (next % tilesPerClip) * NT;
        const unsigned short* xcur = Xb0 + buf * XBUF;
        unsigned short* xnxt = Xb0 + (buf ^ 1) * XBUF;
        f32x16 acc[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
        const unsigned short* xrow = xcur + (64 * nh + l31) * PITCH + 8 * half;
        u32x4 Bq[2][NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) Bq[0][p] = *reinterpret_cast<const u32x4*>(xrow + p * ROWS * PITCH);
        // the embedding values of the tile in the registers become current; load_halo() below refills the "next" set
        pv0 = nv0; pv1 = nv1; hv[0] = nhv[0]; hv[1] = nhv[1];
#define BF7_SLICE(k)                                                                                                        \
    {                                                                                                                           \
        if (h < 16) {                                                                                                           \
            if ((k) == 0) split_pick(h >> 2, h & 3);                                                                            \
            if ((k) == 1) split_st1();                                                                                          \
            if ((k) == 2) split_st2();                                                                                          \
            if ((k) == 3) { split_out(xnxt, h >> 2, h & 3); if ((h & 3) == 3) load_combo(next2, h >> 2); }                      \
        } else if (h < 18) {                                                                                                    \
            if ((k) == 0) halo_pick(nt0, h - 16);                                                                               \
            if ((k) == 1) split_st1();                                                                                          \
            if ((k) == 2) split_st2();                                                                                          \
            if ((k) == 3) halo_out(xnxt, h - 16);                                                                               \
        } else if (h == 18) {                                                                                                   \
            if ((k) == 0) load_halo(next2);                                                                                     \
        }                                                                                                                       \
    }
#pragma unroll
        for (int h = 0; h < 2 * NS; ++h) {
            const int s = h >> 1, nt = h & 1;
            if (h + 1 < 2 * NS) {
                const int s1_ = (h + 1) >> 1, n1 = (h + 1) & 1;
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    Bq[(h + 1) & 1][p] = *reinterpret_cast<const u32x4*>(xrow + (p * ROWS + 32 * n1 + (s1_ >> 2)) * PITCH + 16 * (s1_ & 3));
            }
            const u32x4* Bf = Bq[h & 1];
            FENCE;
            if (H) {                                     // lo hi, hi lo, hi hi
                acc[nt] = mma(Wr[s][1], Bf[0], acc[nt]); FENCE; BF7_SLICE(0) FENCE; BF7_SLICE(1) FENCE;
                acc[nt] = mma(Wr[s][0], Bf[1], acc[nt]); FENCE; BF7_SLICE(3) FENCE;
                acc[nt] = mma(Wr[s][0], Bf[0], acc[nt]); FENCE;
            } else {
                acc[nt] = mma(Wr[s][1], Bf[1], acc[nt]); FENCE; BF7_SLICE(0) FENCE;
                acc[nt] = mma(Wr[s][0], Bf[2], acc[nt]); FENCE; BF7_SLICE(1) FENCE;
                acc[nt] = mma(Wr[s][2], Bf[0], acc[nt]); FENCE; BF7_SLICE(2) FENCE;
                acc[nt] = mma(Wr[s][0], Bf[1], acc[nt]); FENCE; BF7_SLICE(3) FENCE;
                acc[nt] = mma(Wr[s][1], Bf[0], acc[nt]); FENCE;
                acc[nt] = mma(Wr[s][0], Bf[0], acc[nt]); FENCE;
            }
        }
#undef BF7_SLICE
        // epilogue (serial: 32 values against 336 MFMAs)
        {
            float* yb = a.y + ((size_t)b * 64 + 32 * mt + 4 * half) * T + t0 + 64 * nh + l31;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2);
                    float v = acc[nt][r];
                    if (H) v *= dinv;
                    if (EPI == EPI_BIAS) v += Cs[32 * mt + 4 * half + row];
                    yb[(size_t)row * T + 32 * nt] = v;
                }
        }
        lds_barrier();
        tile += tstep;
        buf ^= 1;
    }
#undef FENCE
}

template <int PRO, int EPI, bool H = false>
int launch_conv64bf7p(const Conv64Args& a, hipStream_t stream) {
    constexpr size_t lds = (size_t)(2 * (H ? 2 : 3) * 134 * 72) * 2 + 64 * sizeof(float);
    static wm::DevOnce attr_done;
    auto kern = conv64bf7p_kernel<PRO, EPI, H>;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(kern), lds, attr_done)) return rc;
    const int ntiles = a.B * (a.T / 128);
    const int grid = ntiles < kNumCU ? ntiles : kNumCU;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}

__global__ void pack_w64_bf7_kernel(const float* __restrict__ w, unsigned short* __restrict__ wpb, int mode) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 7 * 4096) return;
    const int tap = i / 4096, out = (i / 64) % 64, in = i % 64;
    const float v = (mode == 2) ? w[(in * 64 + out) * 7 + (6 - tap)] : w[(out * 64 + in) * 7 + tap];
    unsigned p0, p1, p2;
    split3_pair(v, 0.f, p0, p1, p2);
    wpb[i] = (unsigned short)p0; wpb[7 * 4096 + i] = (unsigned short)p1; wpb[2 * 7 * 4096 + i] = (unsigned short)p2;
}

// bf16 three-piece weight image [piece][tap][out][in] (uint16) for the k3 convolutions; mode as wm_pack_w64 (0 / 1)
__global__ void pack_w64_bf_kernel(const float* __restrict__ w, const float* __restrict__ row_scale,
                                   unsigned short* __restrict__ wpb, int mode) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * 4096) return;
    const int tap = i / 4096, out = (i / 64) % 64, in = i % 64;
    float v = (mode == 0) ? w[(out * 64 + in) * 3 + tap] : w[(in * 64 + out) * 3 + (2 - tap)];
    if (row_scale) v *= row_scale[out];          // a per-output-channel factor (folded BatchNorm scale) rides in the weights
    unsigned p0, p1, p2;
    split3_pair(v, 0.f, p0, p1, p2);
    wpb[i] = (unsigned short)p0; wpb[3 * 4096 + i] = (unsigned short)p1; wpb[2 * 3 * 4096 + i] = (unsigned short)p2;
}

// ---------------------------------------------------------------------------------------------
// bf16x6 weight gradient of the k3 convolution.  The contraction runs over time, so both operands keep the natural
// [channel][time] layout in LDS (one aligned ds_read_b128 = 8 consecutive time steps of a channel = one MFMA fragment,
// no transposition).  The +-1 time shift of taps 0 and 2 is made in registers: the centre fragment plus the two
// neighbouring elements are funnel-shifted with v_alignbit (VALU work that runs beside the bf16 MFMA pipe).
// ---------------------------------------------------------------------------------------------
template <int GPRO, int XPRO>
__global__ __launch_bounds__(256) void wgrad64bf_kernel(Wgrad64Args a) {
    constexpr int KW = 3, NT = 128, NP = 3, PG = 136, PX = 152, XO = 8;   // X element index = (t - t0) + XO
    constexpr int QR = NT / 4, NV = 64 * QR / 256;
    constexpr bool GTWO = (GPRO == PRO_BNBWD);
    extern __shared__ __align__(16) unsigned char smem_raw[];
    unsigned short* Gb = reinterpret_cast<unsigned short*>(smem_raw);          // [NP][64][PG]
    unsigned short* Xb = Gb + NP * 64 * PG;                                    // [NP][64][PX]
    float* Cs = reinterpret_cast<float*>(Xb + NP * 64 * PX);                   // [5][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int T = a.T;
    const int tilesPerClip = (T + NT - 1) / NT, ntiles = a.B * tilesPerClip;

    float4 sg[NV], sg2[GTWO ? NV : 1], sx[NV];
    float hx;
    float bsum[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) bsum[i] = 0.f;

    // global -> register staging in NV + 1 pieces: the main loop issues one piece per MFMA block (a 64..96-KB burst per
    // CU backs up the memory pipeline and blocks the wave at issue for thousands of cycles; see conv64bf3_kernel)
    auto load_piece = [&](int tile, int i) {    // branch-free
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        const size_t base = (size_t)b * 64 * T;
        if (i < NV) {
            const int idx = tid + i * 256, c = idx / QR, q = idx % QR;
            const int t = min(t0 + 4 * q, T - 4);
            sg[i] = *reinterpret_cast<const float4*>(a.g + base + (size_t)c * T + t);
            if (GTWO) sg2[i] = *reinterpret_cast<const float4*>(a.g2 + base + (size_t)c * T + t);
            sx[i] = *reinterpret_cast<const float4*>(a.x + base + (size_t)c * T + t);
        } else {
            const int hc = (tid & 127) >> 1, hh = tid & 1;
            hx = a.x[base + (size_t)hc * T + min(max(hh ? t0 + NT : t0 - 1, 0), T - 1)];
        }
    };
    auto load_tile = [&](int tile) {
#pragma unroll
        for (int i = 0; i <= NV; ++i) load_piece(tile, i);
    };
    auto put4 = [&](unsigned short* dst, int stride_p, float v0, float v1, float v2, float v3) {
        unsigned a0, a1, a2, b0, b1, b2;
        split3_pair(v0, v1, a0, a1, a2);
        split3_pair(v2, v3, b0, b1, b2);
        *reinterpret_cast<uint2*>(dst) = make_uint2(a0, b0);
        *reinterpret_cast<uint2*>(dst + stride_p) = make_uint2(a1, b1);
        *reinterpret_cast<uint2*>(dst + 2 * stride_p) = make_uint2(a2, b2);
    };
    auto write_tile = [&](int tile) {
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + i * 256, c = idx / QR, q = idx % QR, t = t0 + 4 * q;
            float4 v = sg[i], u = sx[i];
            if (GPRO == PRO_BNBWD) {
                const float ca = Cs[c], cb = Cs[64 + c], cc = Cs[128 + c], cl = Cs[320 + c];
                const float4 w = sg2[i];
                v.x = pro_apply<PRO_BNBWD>(v.x, w.x, ca, cb, cc, cl); v.y = pro_apply<PRO_BNBWD>(v.y, w.y, ca, cb, cc, cl);
                v.z = pro_apply<PRO_BNBWD>(v.z, w.z, ca, cb, cc, cl); v.w = pro_apply<PRO_BNBWD>(v.w, w.w, ca, cb, cc, cl);
            }
            if (XPRO != PRO_NONE) {
                const float ca = (XPRO == PRO_ADDVEC) ? a.xa[b * 64 + c] : Cs[192 + c];
                const float cb = Cs[256 + c];
                u.x = pro_apply<XPRO>(u.x, 0.f, ca, cb, 0.f); u.y = pro_apply<XPRO>(u.y, 0.f, ca, cb, 0.f);
                u.z = pro_apply<XPRO>(u.z, 0.f, ca, cb, 0.f); u.w = pro_apply<XPRO>(u.w, 0.f, ca, cb, 0.f);
            }
            if (t >= T) { v = make_float4(0.f, 0.f, 0.f, 0.f); u = v; }
            bsum[i] += (v.x + v.y) + (v.z + v.w);
            put4(Gb + c * PG + 4 * q, 64 * PG, v.x, v.y, v.z, v.w);
            put4(Xb + c * PX + XO + 4 * q, 64 * PX, u.x, u.y, u.z, u.w);
        }
        if (tid < 128) {
            const int hc = tid >> 1, hh = tid & 1, t = hh ? t0 + NT : t0 - 1;
            float v = hx;
            if (XPRO != PRO_NONE) {
                const float ca = (XPRO == PRO_ADDVEC) ? a.xa[b * 64 + hc] : Cs[192 + hc];
                v = pro_apply<XPRO>(v, 0.f, ca, Cs[256 + hc], 0.f);
            }
            if (t < 0 || t >= T) v = 0.f;
            unsigned p0, p1, p2;
            split3_pair(v, 0.f, p0, p1, p2);
            const int o = hc * PX + (hh ? XO + NT : XO - 1);
            Xb[o] = (unsigned short)p0; Xb[64 * PX + o] = (unsigned short)p1; Xb[2 * 64 * PX + o] = (unsigned short)p2;
        }
    };

    int tile = WM_XCD_MAP ? xcd_slot() : (int)blockIdx.x;
    if (tile < ntiles) load_tile(tile);
    if (tid < 64) {
        Cs[tid] = GTWO ? a.ga[tid] : 0.f;
        Cs[64 + tid] = GTWO ? a.gb[tid] : 0.f;
        Cs[128 + tid] = GTWO ? a.gc[tid] : 0.f;
        Cs[192 + tid] = (XPRO == PRO_BNRELU) ? a.xa[tid] : 0.f;
        Cs[256 + tid] = (XPRO == PRO_BNRELU) ? a.xb[tid] : 0.f;
        Cs[320 + tid] = GTWO ? a.gb[64 + tid] : 0.f;        // low word of the BatchNorm-backward offset
    }
    // the element right of the right halo is read by the funnel shift of the last fragment: keep it defined
    for (int i = tid; i < NP * 64; i += 256) Xb[i * PX + XO + NT + 1] = 0;
    __syncthreads();
    if (tile < ntiles) write_tile(tile);
    __syncthreads();

    f32x16 acc[KW][2][2];
#pragma unroll
    for (int k = 0; k < KW; ++k)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[k][mt][nt][r] = 0.f;

    while (tile < ntiles) {
        const int next = tile + gridDim.x;
        const int nextc = min(next, ntiles - 1);         // clamped: a tile past the end is loaded (valid memory) but never written
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {                 // this wave's 32 time steps = 2 k-blocks of 16
            const int e0 = wave * 32 + ss * 16 + 8 * half;
            bf16x8 A[2][NP];
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    A[mt][p] = *reinterpret_cast<const bf16x8*>(Gb + (p * 64 + mt * 32 + l31) * PG + e0);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                bf16x8 Bc[NP], Bl[NP], Br[NP];
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const unsigned short* xr = Xb + (p * 64 + nt * 32 + l31) * PX + XO + e0;
                    const uint4 f = *reinterpret_cast<const uint4*>(xr);
                    const unsigned L = *reinterpret_cast<const unsigned*>(xr - 2), R = *reinterpret_cast<const unsigned*>(xr + 8);
                    const uint4 fl = make_uint4(__builtin_amdgcn_alignbit(f.x, L, 16), __builtin_amdgcn_alignbit(f.y, f.x, 16),
                                                __builtin_amdgcn_alignbit(f.z, f.y, 16), __builtin_amdgcn_alignbit(f.w, f.z, 16));
                    const uint4 fr = make_uint4(__builtin_amdgcn_alignbit(f.y, f.x, 16), __builtin_amdgcn_alignbit(f.z, f.y, 16),
                                                __builtin_amdgcn_alignbit(f.w, f.z, 16), __builtin_amdgcn_alignbit(R, f.w, 16));
                    Bc[p] = __builtin_bit_cast(bf16x8, f);
                    Bl[p] = __builtin_bit_cast(bf16x8, fl);
                    Br[p] = __builtin_bit_cast(bf16x8, fr);
                }
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
#define WM_MM6(ACC, BB)                                                                              \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][1], BB[1], ACC, 0, 0, 0);                     \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][0], BB[2], ACC, 0, 0, 0);                     \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][2], BB[0], ACC, 0, 0, 0);                     \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][0], BB[1], ACC, 0, 0, 0);                     \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][1], BB[0], ACC, 0, 0, 0);                     \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][0], BB[0], ACC, 0, 0, 0);
                    WM_MM6(acc[0][mt][nt], Bl)
                    WM_MM6(acc[1][mt][nt], Bc)
                    WM_MM6(acc[2][mt][nt], Br)
#undef WM_MM6
                    load_piece(nextc, (ss * 2 + nt) * 2 + mt);       // pieces 0..7 ride along the 8 MFMA blocks
                }
            }
        }
        load_piece(nextc, NV);
        __syncthreads();
        if (next < ntiles) write_tile(next);
        __syncthreads();
        tile = next;
    }

    float* out = a.partial + (size_t)blockIdx.x * (KW * 4096 + 64);
    float* red = reinterpret_cast<float*>(smem_raw);          // KW*4096 floats = 48 KB <= LDS images (104 KB)
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int k = 0; k < KW; ++k)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int o = (k * 64 + mt * 32 + mfma_row(r, half)) * 64 + nt * 32 + l31;
                            red[o] = (w == 0) ? acc[k][mt][nt][r] : red[o] + acc[k][mt][nt][r];
                        }
        }
        __syncthreads();
    }
    for (int i = tid; i < KW * 4096; i += 256) out[i] = red[i];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float v = half_wave_sum(bsum[i]);
        if (l31 == 0) out[KW * 4096 + (tid >> 5) + 8 * i] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// Pipelined build of wgrad64bf_kernel.  The kernel above runs its phases back to back on one wave per SIMD -- matrix phase,
// barrier, prologue + split + LDS write (640 VALU instructions per lane), barrier -- and the matrix cores sit idle through
// every VALU phase (38 % busy).  Here a tile is 64 time steps, so both 3-piece images fit twice (2 x 60 KB): while the
// 72 MFMAs of tile i run out of one image pair, the same instruction stream prologues / splits tile i+1 into the other
// and fetches tile i+2, ONE slice of side work (<= 8 VALU / LDS / global instructions) pinned behind each MFMA by
// sched_barrier fences (see conv64bf3_kernel: the six MFMAs of a piece-product group chain on one accumulator and wait
// 8 passes for each other, so a slice costs nothing).  The +-1 shifted B fragments of a column block are built while
// its unshifted products run.  One LDS-only barrier per tile.
// ---------------------------------------------------------------------------------------------
template <int GPRO, int XPRO>
__global__ __launch_bounds__(256) void wgrad64bfp_kernel(Wgrad64Args a) {
    static_assert(XPRO == PRO_NONE || XPRO == PRO_BNRELU, "x prologue: none or BN+ReLU");
    constexpr int KW = 3, NT = 64, NP = 3, PG = 72, PX = 88, XO = 8;   // X element index = (t - t0) + XO
    constexpr int QR = NT / 4, NV = 64 * QR / 256;                     // 16 quads per channel row, 4 units per thread and tensor
    constexpr bool GTWO = (GPRO == PRO_BNBWD);
    constexpr int GIMG = NP * 64 * PG, XIMG = NP * 64 * PX;            // bf16 elements per image
    extern __shared__ __align__(16) unsigned char smem_raw[];
    unsigned short* Gb0 = reinterpret_cast<unsigned short*>(smem_raw);         // [2][NP][64][PG]
    unsigned short* Xb0 = Gb0 + 2 * GIMG;                                      // [2][NP][64][PX]
    float* Cs = reinterpret_cast<float*>(Xb0 + 2 * XIMG);                      // [6][64]
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int T = a.T;
    const int tilesPerClip = (T + NT - 1) / NT, ntiles = a.B * tilesPerClip;

    // staging coordinates (fixed per thread): unit i = channel cq + 16 i, time quad q
    const int cq = tid >> 4, q = tid & 15;
    const int hc = (tid & 127) >> 1, hh = tid & 1;
    float4 sg[NV], sg2[GTWO ? NV : 1], sx[NV];
    float hx = 0.f;
    float bsum[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) bsum[i] = 0.f;

    // operand fetch of one tile: per-tile scalar descriptors of the clip + ONE per-lane byte offset; unit i sits 16 i rows further
    wm_srd_t dg = make_srd(a.g, 0), dg2 = dg, dx = dg;
    unsigned voff = 0, hoff = 0;
    bool okq = true, okh = true;                    // the unit's quad / the halo column lies inside the clip
    auto set_tile = [&](int tile) {
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        const size_t clip = (size_t)b * 64 * T, bytes = (size_t)64 * T * sizeof(float);
        dg = make_srd(a.g + clip, bytes);
        if (GTWO) dg2 = make_srd(a.g2 + clip, bytes);
        dx = make_srd(a.x + clip, bytes);
        voff = (unsigned)(cq * T + min(t0 + 4 * q, T - 4)) * 4u;
        const int th = hh ? t0 + NT : t0 - 1;
        hoff = (unsigned)(hc * T + min(max(th, 0), T - 1)) * 4u;
        okq = t0 + 4 * q < T;
        okh = th >= 0 && th < T;
    };
    const unsigned rowstep = (unsigned)(16 * T) * 4u;
    auto load_g = [&](int i) {                     // branch-free: clamped address, masked at the split
        sg[i] = __builtin_bit_cast(float4, buf_load4(dg, voff, rowstep * i));
        if (GTWO) sg2[i] = __builtin_bit_cast(float4, buf_load4(dg2, voff, rowstep * i));
    };
    auto load_x = [&](int i) { sx[i] = __builtin_bit_cast(float4, buf_load4(dx, voff, rowstep * i)); };
    auto load_halo = [&]() { hx = buf_load(dx, hoff, 0u); };

    const int tstep = gridDim.x;
    int tile = WM_XCD_MAP ? xcd_slot() : (int)blockIdx.x;            // grid <= ntiles
    set_tile(tile);
    bool okq_cur = okq, okh_cur = okh;              // masks of the tile whose operands are in the registers
#pragma unroll
    for (int i = 0; i < NV; ++i) { load_g(i); load_x(i); }
    load_halo();
    if (tid < 64) {
        Cs[tid] = GTWO ? a.ga[tid] : 0.f;
        Cs[64 + tid] = GTWO ? a.gb[tid] : 0.f;
        Cs[128 + tid] = GTWO ? a.gc[tid] : 0.f;
        Cs[192 + tid] = (XPRO == PRO_BNRELU) ? a.xa[tid] : 0.f;
        Cs[256 + tid] = (XPRO == PRO_BNRELU) ? a.xb[tid] : 0.f;
        Cs[320 + tid] = GTWO ? a.gb[64 + tid] : 0.f;        // low word of the BatchNorm-backward offset
    }
    // the element right of the right halo only feeds bits that the funnel shift drops: keep it defined in both images
    for (int i = tid; i < 2 * NP * 64; i += 256) Xb0[(i / (NP * 64)) * XIMG + (i % (NP * 64)) * PX + XO + NT + 1] = 0;
    __syncthreads();
    // per-thread prologue constants: the unit channels never change
    float gca[GTWO ? NV : 1], gcb[GTWO ? NV : 1], gcc[GTWO ? NV : 1], gcl[GTWO ? NV : 1], xca[NV], xcb[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = cq + 16 * i;
        if (GTWO) { gca[i] = Cs[c]; gcb[i] = Cs[64 + c]; gcc[i] = Cs[128 + c]; gcl[i] = Cs[320 + c]; }
        xca[i] = Cs[192 + c]; xcb[i] = Cs[256 + c];
    }
    const float hxa = Cs[192 + hc], hxb = Cs[256 + hc];

    // ---- the split of one staged unit (four consecutive time steps of one channel = two value pairs) in six stages
    float va = 0.f, vb = 0.f, vc = 0.f, vd = 0.f;
    unsigned pa0 = 0, pa1 = 0, pb0 = 0, pb1 = 0;
    float bflag = 1.f;                  // 0 while a clamped duplicate of the last tile is being split (it must not reach the bias sums)
    float wc = 0.f, wd = 0.f;           // second half of a two-tensor unit, parked while its registers are refilled
    auto g_pro_a = [&](int i) {         // first value pair of unit i: prologue + mask + bias sum; the second pair is parked raw
        const float4 v = sg[i];
        float x0 = v.x, x1 = v.y;
        vc = v.z; vd = v.w;
        if (GTWO) {
            const float4 w = sg2[i];
            x0 = pro_apply<PRO_BNBWD>(x0, w.x, gca[i], gcb[i], gcc[i], gcl[i]); x1 = pro_apply<PRO_BNBWD>(x1, w.y, gca[i], gcb[i], gcc[i], gcl[i]);
            wc = w.z; wd = w.w;
        }
        va = okq_cur ? x0 : 0.f; vb = okq_cur ? x1 : 0.f;
        bsum[i] = fmaf(bflag, va + vb, bsum[i]);
        asm volatile("" : "+v"(va), "+v"(vb), "+v"(vc), "+v"(vd), "+v"(wc), "+v"(wd), "+v"(bsum[i]));
    };
    auto g_pro_b = [&](int i) {         // second value pair
        float x2 = vc, x3 = vd;
        if (GTWO) { x2 = pro_apply<PRO_BNBWD>(x2, wc, gca[i], gcb[i], gcc[i], gcl[i]); x3 = pro_apply<PRO_BNBWD>(x3, wd, gca[i], gcb[i], gcc[i], gcl[i]); }
        vc = okq_cur ? x2 : 0.f; vd = okq_cur ? x3 : 0.f;
        bsum[i] = fmaf(bflag, vc + vd, bsum[i]);
        asm volatile("" : "+v"(vc), "+v"(vd), "+v"(bsum[i]));
    };
    auto x_pro = [&](int i) {
        float4 u = sx[i];
        if (XPRO != PRO_NONE) {
            u.x = pro_apply<XPRO>(u.x, 0.f, xca[i], xcb[i], 0.f); u.y = pro_apply<XPRO>(u.y, 0.f, xca[i], xcb[i], 0.f);
            u.z = pro_apply<XPRO>(u.z, 0.f, xca[i], xcb[i], 0.f); u.w = pro_apply<XPRO>(u.w, 0.f, xca[i], xcb[i], 0.f);
        }
        const bool ok = okq_cur;
        va = ok ? u.x : 0.f; vb = ok ? u.y : 0.f; vc = ok ? u.z : 0.f; vd = ok ? u.w : 0.f;
        asm volatile("" : "+v"(va), "+v"(vb), "+v"(vc), "+v"(vd));
    };
    auto h_pro = [&]() {
        float v = hx;
        if (XPRO != PRO_NONE) v = pro_apply<XPRO>(v, 0.f, hxa, hxb, 0.f);
        va = okh_cur ? v : 0.f; vb = 0.f;
        asm volatile("" : "+v"(va), "+v"(vb));
    };
    auto s1a = [&]() {
        const bf16x2 h_ = {(__bf16)va, (__bf16)vb};
        pa0 = __builtin_bit_cast(unsigned, h_);
        va -= __uint_as_float(pa0 << 16); vb -= __uint_as_float(pa0 & 0xffff0000u);
        asm volatile("" : "+v"(va), "+v"(vb), "+v"(pa0));
    };
    auto s2a = [&]() {
        const bf16x2 m_ = {(__bf16)va, (__bf16)vb};
        pa1 = __builtin_bit_cast(unsigned, m_);
        va -= __uint_as_float(pa1 << 16); vb -= __uint_as_float(pa1 & 0xffff0000u);
        asm volatile("" : "+v"(va), "+v"(vb), "+v"(pa1));
    };
    auto s1b = [&]() {
        const bf16x2 h_ = {(__bf16)vc, (__bf16)vd};
        pb0 = __builtin_bit_cast(unsigned, h_);
        vc -= __uint_as_float(pb0 << 16); vd -= __uint_as_float(pb0 & 0xffff0000u);
        asm volatile("" : "+v"(vc), "+v"(vd), "+v"(pb0));
    };
    auto s2b = [&]() {
        const bf16x2 m_ = {(__bf16)vc, (__bf16)vd};
        pb1 = __builtin_bit_cast(unsigned, m_);
        vc -= __uint_as_float(pb1 << 16); vd -= __uint_as_float(pb1 & 0xffff0000u);
        asm volatile("" : "+v"(vc), "+v"(vd), "+v"(pb1));
    };
    auto out4 = [&](unsigned short* dst, int stride_p) {         // last stage + the three 8-byte LDS writes
        const bf16x2 la = {(__bf16)va, (__bf16)vb}, lb = {(__bf16)vc, (__bf16)vd};
        *reinterpret_cast<uint2*>(dst) = make_uint2(pa0, pb0);
        *reinterpret_cast<uint2*>(dst + stride_p) = make_uint2(pa1, pb1);
        *reinterpret_cast<uint2*>(dst + 2 * stride_p) = make_uint2(__builtin_bit_cast(unsigned, la), __builtin_bit_cast(unsigned, lb));
    };
    auto h_out = [&](unsigned short* X) {
        const bf16x2 la = {(__bf16)va, (__bf16)vb};
        const int o = hc * PX + (hh ? XO + NT : XO - 1);
        X[o] = (unsigned short)pa0; X[64 * PX + o] = (unsigned short)pa1; X[2 * 64 * PX + o] = (unsigned short)__builtin_bit_cast(unsigned, la);
    };
    // Side work of one tile as a sequence of slices: the operands in the registers are split into images (G, X) and the
    // consumed registers are refilled from the tile set_tile() last pointed at.  Units (G0, X0, G1, X1, ...), then the halo.
    // A gradient unit takes SG slices (prologue a | hi a + refill | mid a | prologue b | hi b | mid b | lo + LDS writes),
    // an input unit 6 (prologue | hi a + refill | mid a | hi b | mid b | lo + LDS writes), the halo 4.
    constexpr int SG = 7, SX = 6, NSLICE = NV * (SG + SX) + 4;
    auto side = [&](int u, unsigned short* G, unsigned short* X) __attribute__((always_inline)) {
        if (u < NV * (SG + SX)) {
            const int i = u / (SG + SX), r = u % (SG + SX);
            if (r < SG) {
                if (r == 0) g_pro_a(i);
                if (r == 1) { s1a(); load_g(i); }
                if (r == 2) s2a();
                if (r == 3) g_pro_b(i);
                if (r == 4) s1b();
                if (r == 5) s2b();
                if (r == 6) out4(G + (cq + 16 * i) * PG + 4 * q, 64 * PG);
            } else {
                const int st = r - SG;
                if (st == 0) x_pro(i);
                if (st == 1) { s1a(); load_x(i); }
                if (st == 2) s2a();
                if (st == 3) s1b();
                if (st == 4) s2b();
                if (st == 5) out4(X + (cq + 16 * i) * PX + XO + 4 * q, 64 * PX);
            }
        } else {
            const int st = u - NV * (SG + SX);
            if (st == 0) { h_pro(); load_halo(); }
            if (st == 1) s1a();
            if (st == 2) s2a();
            if (st == 3) { if (tid < 128) h_out(X); }
        }
    };
    static_assert(NSLICE <= 60, "72 MFMAs per tile, 12 of their slices build the shifted fragments");

    {   // first tile: split serially while the second is fetched
        set_tile(min(tile + tstep, ntiles - 1));
        const bool okq_n = okq, okh_n = okh;
#pragma unroll
        for (int u = 0; u < NSLICE; ++u) side(u, Gb0, Xb0);
        okq_cur = okq_n; okh_cur = okh_n;
    }
    __syncthreads();

    f32x16 acc[KW][2][2];
#pragma unroll
    for (int k = 0; k < KW; ++k)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[k][mt][nt][r] = 0.f;

    const int e0 = wave * 16 + 8 * half;             // this lane's 8 time steps of the tile (k index of the MFMA)
    int buf = 0;
#define FENCE __builtin_amdgcn_sched_barrier(0)
    while (tile < ntiles) {
        // registers: tile + tstep (split below into the other image pair); fetched below: tile + 2 tstep
        bflag = (tile + tstep < ntiles) ? 1.f : 0.f;
        set_tile(min(tile + 2 * tstep, ntiles - 1));
        const bool okq_n = okq, okh_n = okh;
        const unsigned short* Gc = Gb0 + buf * GIMG;
        const unsigned short* Xc = Xb0 + buf * XIMG;
        unsigned short* Gn = Gb0 + (buf ^ 1) * GIMG;
        unsigned short* Xn = Xb0 + (buf ^ 1) * XIMG;
        bf16x8 A[2][NP];
        uint4 f[2][NP];
        unsigned Lw[2][NP], Rw[2][NP];
        bf16x8 Bl[NP], Br[NP];
        auto read_b = [&](int nt) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const unsigned short* xr = Xc + (p * 64 + nt * 32 + l31) * PX + XO + e0;
                f[nt][p] = *reinterpret_cast<const uint4*>(xr);
                Lw[nt][p] = *reinterpret_cast<const unsigned*>(xr - 2);
                Rw[nt][p] = *reinterpret_cast<const unsigned*>(xr + 8);
            }
        };
        auto shl = [&](int nt, int p) {      // fragment shifted to t - 1
            const uint4 g = f[nt][p];
            uint4 s_ = make_uint4(__builtin_amdgcn_alignbit(g.x, Lw[nt][p], 16), __builtin_amdgcn_alignbit(g.y, g.x, 16),
                                  __builtin_amdgcn_alignbit(g.z, g.y, 16), __builtin_amdgcn_alignbit(g.w, g.z, 16));
            asm volatile("" : "+v"(s_.x), "+v"(s_.y), "+v"(s_.z), "+v"(s_.w));      // built in this slice, not at its first use
            Bl[p] = __builtin_bit_cast(bf16x8, s_);
        };
        auto shr = [&](int nt, int p) {      // fragment shifted to t + 1
            const uint4 g = f[nt][p];
            uint4 s_ = make_uint4(__builtin_amdgcn_alignbit(g.y, g.x, 16), __builtin_amdgcn_alignbit(g.z, g.y, 16),
                                  __builtin_amdgcn_alignbit(g.w, g.z, 16), __builtin_amdgcn_alignbit(Rw[nt][p], g.w, 16));
            asm volatile("" : "+v"(s_.x), "+v"(s_.y), "+v"(s_.z), "+v"(s_.w));
            Br[p] = __builtin_bit_cast(bf16x8, s_);
        };
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                A[mt][p] = *reinterpret_cast<const bf16x8*>(Gc + (p * 64 + mt * 32 + l31) * PG + e0);
        read_b(0);
#pragma unroll
        for (int m = 0; m < 72; ++m) {
            const int nt = m / 36, tg = (m % 36) / 12, mt = (m % 12) / 6, j = m % 6;
            const int pa = (j == 0 || j == 4) ? 1 : (j == 2 ? 2 : 0), pb = (j == 0 || j == 3) ? 1 : (j == 1 ? 2 : 0);
            FENCE;
            if (tg == 0)
                acc[1][mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][pa], __builtin_bit_cast(bf16x8, f[nt][pb]), acc[1][mt][nt], 0, 0, 0);
            else if (tg == 1)
                acc[0][mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][pa], Bl[pb], acc[0][mt][nt], 0, 0, 0);
            else
                acc[2][mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[mt][pa], Br[pb], acc[2][mt][nt], 0, 0, 0);
            FENCE;
            // ---- the slice behind MFMA m
            const int mm = m % 36;
            if (mm < 3) shl(nt, mm);
            else if (mm < 6) shr(nt, mm - 3);
            else {
                const int u = (nt == 0) ? mm - 6 : 30 + (mm - 6);          // 0..59: side-work slice index
                if (u < NSLICE) side(u, Gn, Xn);
            }
            if (m == 30) read_b(1);
            FENCE;
        }
        okq_cur = okq_n; okh_cur = okh_n;
        lds_barrier();
        tile += tstep;
        buf ^= 1;
    }
#undef FENCE

    float* out = a.partial + (size_t)blockIdx.x * (KW * 4096 + 64);
    float* red = reinterpret_cast<float*>(smem_raw);          // KW*4096 floats = 48 KB <= the images (120 KB)
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int k = 0; k < KW; ++k)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int o = (k * 64 + mt * 32 + mfma_row(r, half)) * 64 + nt * 32 + l31;
                            red[o] = (w == 0) ? acc[k][mt][nt][r] : red[o] + acc[k][mt][nt][r];
                        }
        }
        __syncthreads();
    }
    for (int i = tid; i < KW * 4096; i += 256) out[i] = red[i];
#pragma unroll
    for (int i = 0; i < NV; ++i) {       // the 16 lanes of a channel row sit side by side
        float v = bsum[i];
        v += __shfl_xor(v, 8); v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
        if (q == 0) out[KW * 4096 + cq + 16 * i] = v;
    }
}

template <int GPRO, int XPRO>
int launch_wgrad64bfp(const Wgrad64Args& a, int* grid_out, hipStream_t stream) {
    constexpr size_t lds = (size_t)(2 * 3 * 64 * 72 + 2 * 3 * 64 * 88) * 2 + 6 * 64 * sizeof(float);
    static wm::DevOnce attr_done;
    auto kern = wgrad64bfp_kernel<GPRO, XPRO>;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(kern), lds, attr_done)) return rc;
    const int ntiles = a.B * ((a.T + 63) / 64);
    const int grid = ntiles < kNumCU ? ntiles : kNumCU;
    *grid_out = grid;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}

// Output-split build of the same kernel: a wave keeps one 32 x 32 block per tap instead of the whole 64 x 64 x 3 result, so the
// workgroup needs ~200 registers per lane and can be co-resident with the LSTM recurrence kernels (side-stream overlap).
template <int GPRO, int XPRO>
__global__ __launch_bounds__(256) void wgrad64bf_small_kernel(Wgrad64Args a) {
    constexpr int KW = 3, NT = 128, NP = 3, PG = 136, PX = 152, XO = 8;   // X element index = (t - t0) + XO
    constexpr int QR = NT / 4, NV = 64 * QR / 256;
    constexpr bool GTWO = (GPRO == PRO_BNBWD);
    extern __shared__ __align__(16) unsigned char smem_raw[];
    unsigned short* Gb = reinterpret_cast<unsigned short*>(smem_raw);          // [NP][64][PG]
    unsigned short* Xb = Gb + NP * 64 * PG;                                    // [NP][64][PX]
    float* Cs = reinterpret_cast<float*>(Xb + NP * 64 * PX);                   // [5][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int T = a.T;
    const int tilesPerClip = (T + NT - 1) / NT, ntiles = a.B * tilesPerClip;

    float4 sg[NV], sg2[GTWO ? NV : 1], sx[NV];
    float hx;
    float bsum[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) bsum[i] = 0.f;

    // global -> register staging in NV + 1 pieces: the main loop issues one piece per MFMA block (a 64..96-KB burst per
    // CU backs up the memory pipeline and blocks the wave at issue for thousands of cycles; see conv64bf3_kernel)
    auto load_piece = [&](int tile, int i) {    // branch-free
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        const size_t base = (size_t)b * 64 * T;
        if (i < NV) {
            const int idx = tid + i * 256, c = idx / QR, q = idx % QR;
            const int t = min(t0 + 4 * q, T - 4);
            sg[i] = *reinterpret_cast<const float4*>(a.g + base + (size_t)c * T + t);
            if (GTWO) sg2[i] = *reinterpret_cast<const float4*>(a.g2 + base + (size_t)c * T + t);
            sx[i] = *reinterpret_cast<const float4*>(a.x + base + (size_t)c * T + t);
        } else {
            const int hc = (tid & 127) >> 1, hh = tid & 1;
            hx = a.x[base + (size_t)hc * T + min(max(hh ? t0 + NT : t0 - 1, 0), T - 1)];
        }
    };
    auto load_tile = [&](int tile) {
#pragma unroll
        for (int i = 0; i <= NV; ++i) load_piece(tile, i);
    };
    auto put4 = [&](unsigned short* dst, int stride_p, float v0, float v1, float v2, float v3) {
        unsigned a0, a1, a2, b0, b1, b2;
        split3_pair(v0, v1, a0, a1, a2);
        split3_pair(v2, v3, b0, b1, b2);
        *reinterpret_cast<uint2*>(dst) = make_uint2(a0, b0);
        *reinterpret_cast<uint2*>(dst + stride_p) = make_uint2(a1, b1);
        *reinterpret_cast<uint2*>(dst + 2 * stride_p) = make_uint2(a2, b2);
    };
    auto write_tile = [&](int tile) {
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + i * 256, c = idx / QR, q = idx % QR, t = t0 + 4 * q;
            float4 v = sg[i], u = sx[i];
            if (GPRO == PRO_BNBWD) {
                const float ca = Cs[c], cb = Cs[64 + c], cc = Cs[128 + c], cl = Cs[320 + c];
                const float4 w = sg2[i];
                v.x = pro_apply<PRO_BNBWD>(v.x, w.x, ca, cb, cc, cl); v.y = pro_apply<PRO_BNBWD>(v.y, w.y, ca, cb, cc, cl);
                v.z = pro_apply<PRO_BNBWD>(v.z, w.z, ca, cb, cc, cl); v.w = pro_apply<PRO_BNBWD>(v.w, w.w, ca, cb, cc, cl);
            }
            if (XPRO != PRO_NONE) {
                const float ca = (XPRO == PRO_ADDVEC) ? a.xa[b * 64 + c] : Cs[192 + c];
                const float cb = Cs[256 + c];
                u.x = pro_apply<XPRO>(u.x, 0.f, ca, cb, 0.f); u.y = pro_apply<XPRO>(u.y, 0.f, ca, cb, 0.f);
                u.z = pro_apply<XPRO>(u.z, 0.f, ca, cb, 0.f); u.w = pro_apply<XPRO>(u.w, 0.f, ca, cb, 0.f);
            }
            if (t >= T) { v = make_float4(0.f, 0.f, 0.f, 0.f); u = v; }
            bsum[i] += (v.x + v.y) + (v.z + v.w);
            put4(Gb + c * PG + 4 * q, 64 * PG, v.x, v.y, v.z, v.w);
            put4(Xb + c * PX + XO + 4 * q, 64 * PX, u.x, u.y, u.z, u.w);
        }
        if (tid < 128) {
            const int hc = tid >> 1, hh = tid & 1, t = hh ? t0 + NT : t0 - 1;
            float v = hx;
            if (XPRO != PRO_NONE) {
                const float ca = (XPRO == PRO_ADDVEC) ? a.xa[b * 64 + hc] : Cs[192 + hc];
                v = pro_apply<XPRO>(v, 0.f, ca, Cs[256 + hc], 0.f);
            }
            if (t < 0 || t >= T) v = 0.f;
            unsigned p0, p1, p2;
            split3_pair(v, 0.f, p0, p1, p2);
            const int o = hc * PX + (hh ? XO + NT : XO - 1);
            Xb[o] = (unsigned short)p0; Xb[64 * PX + o] = (unsigned short)p1; Xb[2 * 64 * PX + o] = (unsigned short)p2;
        }
    };

    int tile = WM_XCD_MAP ? xcd_slot() : (int)blockIdx.x;
    if (tile < ntiles) load_tile(tile);
    if (tid < 64) {
        Cs[tid] = GTWO ? a.ga[tid] : 0.f;
        Cs[64 + tid] = GTWO ? a.gb[tid] : 0.f;
        Cs[128 + tid] = GTWO ? a.gc[tid] : 0.f;
        Cs[192 + tid] = (XPRO == PRO_BNRELU) ? a.xa[tid] : 0.f;
        Cs[256 + tid] = (XPRO == PRO_BNRELU) ? a.xb[tid] : 0.f;
        Cs[320 + tid] = GTWO ? a.gb[64 + tid] : 0.f;        // low word of the BatchNorm-backward offset
    }
    // the element right of the right halo is read by the funnel shift of the last fragment: keep it defined
    for (int i = tid; i < NP * 64; i += 256) Xb[i * PX + XO + NT + 1] = 0;
    __syncthreads();
    if (tile < ntiles) write_tile(tile);
    __syncthreads();

    // wave (mt, nt) owns ONE 32 x 32 block of every tap's matrix (48 accumulator registers instead of 192) and walks the whole
    // 128-step tile: ~200 registers per lane in all, so a workgroup fits beside the 152-register LSTM recurrence waves
    const int mt = wave & 1, nt = wave >> 1;
    f32x16 acc[KW];
#pragma unroll
    for (int k = 0; k < KW; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

    while (tile < ntiles) {
        const int next = tile + gridDim.x;
        const int nextc = min(next, ntiles - 1);         // clamped: a tile past the end is loaded (valid memory) but never written
#pragma unroll
        for (int kb = 0; kb < NT / 16; ++kb) {           // the tile's 8 k-blocks of 16 time steps
            const int e0 = kb * 16 + 8 * half;
            bf16x8 A[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) A[p] = *reinterpret_cast<const bf16x8*>(Gb + (p * 64 + mt * 32 + l31) * PG + e0);
            bf16x8 Bc[NP], Bl[NP], Br[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const unsigned short* xr = Xb + (p * 64 + nt * 32 + l31) * PX + XO + e0;
                const uint4 f = *reinterpret_cast<const uint4*>(xr);
                const unsigned L = *reinterpret_cast<const unsigned*>(xr - 2), R = *reinterpret_cast<const unsigned*>(xr + 8);
                const uint4 fl = make_uint4(__builtin_amdgcn_alignbit(f.x, L, 16), __builtin_amdgcn_alignbit(f.y, f.x, 16),
                                            __builtin_amdgcn_alignbit(f.z, f.y, 16), __builtin_amdgcn_alignbit(f.w, f.z, 16));
                const uint4 fr = make_uint4(__builtin_amdgcn_alignbit(f.y, f.x, 16), __builtin_amdgcn_alignbit(f.z, f.y, 16),
                                            __builtin_amdgcn_alignbit(f.w, f.z, 16), __builtin_amdgcn_alignbit(R, f.w, 16));
                Bc[p] = __builtin_bit_cast(bf16x8, f);
                Bl[p] = __builtin_bit_cast(bf16x8, fl);
                Br[p] = __builtin_bit_cast(bf16x8, fr);
            }
#define WM_MM6(ACC, BB)                                                                              \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[1], BB[1], ACC, 0, 0, 0);                         \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0], BB[2], ACC, 0, 0, 0);                         \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[2], BB[0], ACC, 0, 0, 0);                         \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0], BB[1], ACC, 0, 0, 0);                         \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[1], BB[0], ACC, 0, 0, 0);                         \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0], BB[0], ACC, 0, 0, 0);
            WM_MM6(acc[0], Bl)
            WM_MM6(acc[1], Bc)
            WM_MM6(acc[2], Br)
#undef WM_MM6
            load_piece(nextc, kb);                       // pieces 0..7 ride along the 8 k-blocks
        }
        load_piece(nextc, NV);
        __syncthreads();
        if (next < ntiles) write_tile(next);
        __syncthreads();
        tile = next;
    }

    float* out = a.partial + (size_t)blockIdx.x * (KW * 4096 + 64);
#pragma unroll
    for (int k = 0; k < KW; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(k * 64 + mt * 32 + mfma_row(r, half)) * 64 + nt * 32 + l31] = acc[k][r];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float v = half_wave_sum(bsum[i]);
        if (l31 == 0) out[KW * 4096 + (tid >> 5) + 8 * i] = v;
    }
}

template <int GPRO, int XPRO>
int launch_wgrad64bf_small(const Wgrad64Args& a, int* grid_out, hipStream_t stream) {
    constexpr size_t lds = (size_t)(3 * 64 * 136 + 3 * 64 * 152) * 2 + 6 * 64 * sizeof(float);
    static wm::DevOnce attr_done;
    auto kern = wgrad64bf_small_kernel<GPRO, XPRO>;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(kern), lds, attr_done)) return rc;
    const int ntiles = a.B * ((a.T + 127) / 128);
    const int grid = ntiles < kNumCU ? ntiles : kNumCU;
    *grid_out = grid;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}

template <int GPRO, int XPRO>
int launch_wgrad64bf(const Wgrad64Args& a, int* grid_out, hipStream_t stream) {
#if WM_WGRAD_PIPE
    return launch_wgrad64bfp<GPRO, XPRO>(a, grid_out, stream);
#endif
    constexpr size_t lds = (size_t)(3 * 64 * 136 + 3 * 64 * 152) * 2 + 6 * 64 * sizeof(float);
    static wm::DevOnce attr_done;
    auto kern = wgrad64bf_kernel<GPRO, XPRO>;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(kern), lds, attr_done)) return rc;
    const int ntiles = a.B * ((a.T + 127) / 128);
    const int grid = ntiles < kNumCU ? ntiles : kNumCU;
    *grid_out = grid;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------
// bf16x6 weight gradient of the 7-tap ConvTranspose1d: G[tap][out][in] = sum_t g[out][t] x[in][t + tap - 3].
// Same LDS scheme as wgrad64bf_kernel ([channel][time] 3-piece images, fragments = aligned ds_read_b128 along time).
// Wave (nt, kh) owns the 32 input-channel columns nt and half kh of the tile's time range for ALL seven taps and both
// output halves (224 accumulator registers): per 16-step k-block it reads one 24-element window per piece and builds
// the seven shifted B fragments from it in registers (dword selects for even shifts, v_alignbit for odd ones), so the
// matrix phase needs 15 LDS reads per 84 MFMAs.  The two time halves meet in the final slab reduction.
// ---------------------------------------------------------------------------------------------
// H = true: f16 two-piece build (three products per product): a.ga = {gs, 1 / gs}, the gradient is multiplied by gs before the split and
// clamped to the f16 range, x is split unscaled, the sums leave times 1 / gs (the bias sums are formed from the unscaled gradient)
template <int XPRO, bool H = false>
__global__ __launch_bounds__(256) void wgrad64bf7_kernel(Wgrad64Args a) {
    constexpr int KW = 7, PAD = 3, NT = 128, NP = H ? 2 : 3, PG = 136, PX = 152, XO = 8;
    constexpr int QR = NT / 4, NV = 64 * QR / 256;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    unsigned short* Gb = reinterpret_cast<unsigned short*>(smem_raw);          // [NP][64][PG]
    unsigned short* Xb = Gb + NP * 64 * PG;                                    // [NP][64][PX]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int nt = wave & 1, mt = wave >> 1;           // this wave's 32 x 32 block of every tap's [out][in] matrix
    const int T = a.T;
    const int tilesPerClip = (T + NT - 1) / NT, ntiles = a.B * tilesPerClip;
    const int c0 = tid >> 5, q = tid & 31;             // staging: rows c0 + 8 i, float4 column q

    float4 sg[NV], sx[NV];
    float xv[NV], hx[2], hv[2];
    float bsum[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) bsum[i] = 0.f;
    const float gs = (H && a.ga) ? a.ga[0] : 1.f, ginv = (H && a.ga) ? a.ga[1] : 1.f;

    auto halo_of = [&](int k, int t0, int& c, int& e, int& t) {   // k-th halo element of this thread: channel, image element, time
        const int idx = min(tid + k * 256, 64 * 2 * PAD - 1);
        c = idx / (2 * PAD);
        const int h = idx % (2 * PAD);
        e = (h < PAD) ? XO - PAD + h : XO + NT + (h - PAD);
        t = t0 + e - XO;
    };
    auto load_piece = [&](int tile, int i) {        // branch-free (clamped addresses); piece NV = halo
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        const size_t base = (size_t)b * 64 * T;
        if (i < NV) {
            const int c = c0 + 8 * i, t = min(t0 + 4 * q, T - 4);
            sg[i] = *reinterpret_cast<const float4*>(a.g + base + (size_t)c * T + t);
            sx[i] = *reinterpret_cast<const float4*>(a.x + base + (size_t)c * T + t);
            if (XPRO == PRO_ADDVEC) xv[i] = a.xa[b * 64 + c];
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                int c, e, t;
                halo_of(k, t0, c, e, t);
                hx[k] = a.x[base + (size_t)c * T + min(max(t, 0), T - 1)];
                if (XPRO == PRO_ADDVEC) hv[k] = a.xa[b * 64 + c];
            }
        }
    };
    auto put4 = [&](unsigned short* dst, int stride_p, float v0, float v1, float v2, float v3) {
        if (H) {
            const h16x2 ha = __builtin_convertvector(f32x2{v0, v1}, h16x2), hb = __builtin_convertvector(f32x2{v2, v3}, h16x2);
            const h16x2 la = __builtin_convertvector(f32x2{v0 - (float)ha.x, v1 - (float)ha.y}, h16x2);
            const h16x2 lb = __builtin_convertvector(f32x2{v2 - (float)hb.x, v3 - (float)hb.y}, h16x2);
            *reinterpret_cast<uint2*>(dst) = make_uint2(__builtin_bit_cast(unsigned, ha), __builtin_bit_cast(unsigned, hb));
            *reinterpret_cast<uint2*>(dst + stride_p) = make_uint2(__builtin_bit_cast(unsigned, la), __builtin_bit_cast(unsigned, lb));
            return;
        }
        unsigned a0, a1, a2, b0, b1, b2;
        split3_pair(v0, v1, a0, a1, a2);
        split3_pair(v2, v3, b0, b1, b2);
        *reinterpret_cast<uint2*>(dst) = make_uint2(a0, b0);
        *reinterpret_cast<uint2*>(dst + stride_p) = make_uint2(a1, b1);
        *reinterpret_cast<uint2*>(dst + 2 * stride_p) = make_uint2(a2, b2);
    };
    auto write_tile = [&](int tile) {
        const int t0 = (tile % tilesPerClip) * NT;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = c0 + 8 * i, t = t0 + 4 * q;
            float4 v = sg[i], u = sx[i];
            if (XPRO == PRO_ADDVEC) { u.x += xv[i]; u.y += xv[i]; u.z += xv[i]; u.w += xv[i]; }
            if (t >= T) { v = make_float4(0.f, 0.f, 0.f, 0.f); u = v; }
            bsum[i] += (v.x + v.y) + (v.z + v.w);
            if (H) {
                v.x = __builtin_amdgcn_fmed3f(v.x * gs, -6.0e4f, 6.0e4f); v.y = __builtin_amdgcn_fmed3f(v.y * gs, -6.0e4f, 6.0e4f);
                v.z = __builtin_amdgcn_fmed3f(v.z * gs, -6.0e4f, 6.0e4f); v.w = __builtin_amdgcn_fmed3f(v.w * gs, -6.0e4f, 6.0e4f);
            }
            put4(Gb + c * PG + 4 * q, 64 * PG, v.x, v.y, v.z, v.w);
            put4(Xb + c * PX + XO + 4 * q, 64 * PX, u.x, u.y, u.z, u.w);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (tid + k * 256 < 64 * 2 * PAD) {
                int c, e, t;
                halo_of(k, t0, c, e, t);
                float v = hx[k];
                if (XPRO == PRO_ADDVEC) v += hv[k];
                if (t < 0 || t >= T) v = 0.f;
                const int o = c * PX + e;
                if (H) {
                    const _Float16 h_ = (_Float16)v;
                    const _Float16 l_ = (_Float16)(v - (float)h_);
                    Xb[o] = __builtin_bit_cast(unsigned short, h_); Xb[64 * PX + o] = __builtin_bit_cast(unsigned short, l_);
                } else {
                    unsigned p0, p1, p2;
                    split3_pair(v, 0.f, p0, p1, p2);
                    Xb[o] = (unsigned short)p0; Xb[64 * PX + o] = (unsigned short)p1; Xb[2 * 64 * PX + o] = (unsigned short)p2;
                }
            }
        }
    };

    int tile = WM_XCD_MAP ? xcd_slot() : (int)blockIdx.x;          // grid <= ntiles
#pragma unroll
    for (int i = 0; i <= NV; ++i) load_piece(tile, i);
    // window elements outside [XO - 3, XO + NT + 3) are read but never reach an MFMA: give them a defined value once
    for (int i = tid; i < NP * 64 * PX; i += 256) Xb[i] = 0;
    __syncthreads();
    write_tile(tile);
    __syncthreads();

    f32x16 acc[KW];
#pragma unroll
    for (int k = 0; k < KW; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

    auto mma = [&](const u32x4& A_, const u32x4& B_, f32x16 c) -> f32x16 {
        if (H) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, A_), __builtin_bit_cast(h16x8, B_), c, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A_), __builtin_bit_cast(bf16x8, B_), c, 0, 0, 0);
    };
    while (tile < ntiles) {
        const int next = tile + gridDim.x;
        const int nextc = min(next, ntiles - 1);         // clamped: loaded (valid memory) but never written
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) {                 // the tile's 128 time steps = 8 k-blocks of 16
            const int e0 = kb * 16 + 8 * half;
            u32x4 A[NP];
            unsigned W[NP][12];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                A[p] = *reinterpret_cast<const u32x4*>(Gb + (p * 64 + mt * 32 + l31) * PG + e0);
                const unsigned short* xr = Xb + (p * 64 + nt * 32 + l31) * PX + XO + e0;
                const uint4 w0 = *reinterpret_cast<const uint4*>(xr - 8), w1 = *reinterpret_cast<const uint4*>(xr),
                            w2 = *reinterpret_cast<const uint4*>(xr + 8);
                W[p][0] = w0.x; W[p][1] = w0.y; W[p][2] = w0.z; W[p][3] = w0.w;
                W[p][4] = w1.x; W[p][5] = w1.y; W[p][6] = w1.z; W[p][7] = w1.w;
                W[p][8] = w2.x; W[p][9] = w2.y; W[p][10] = w2.z; W[p][11] = w2.w;
            }
#pragma unroll
            for (int tap = 0; tap < KW; ++tap) {
                // fragment = 8 elements from window element 8 + (tap - PAD): dword d0, odd start -> funnel shift
                constexpr int dummy = 0; (void)dummy;
                const int st = 8 + tap - PAD, d0 = st >> 1;
                u32x4 Bt[NP];
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    uint4 f;
                    if (st & 1)
                        f = make_uint4(__builtin_amdgcn_alignbit(W[p][d0 + 1], W[p][d0], 16), __builtin_amdgcn_alignbit(W[p][d0 + 2], W[p][d0 + 1], 16),
                                       __builtin_amdgcn_alignbit(W[p][d0 + 3], W[p][d0 + 2], 16), __builtin_amdgcn_alignbit(W[p][d0 + 4], W[p][d0 + 3], 16));
                    else
                        f = make_uint4(W[p][d0], W[p][d0 + 1], W[p][d0 + 2], W[p][d0 + 3]);
                    Bt[p] = u32x4{f.x, f.y, f.z, f.w};
                }
                if (H) {                                 // lo hi, hi lo, hi hi
                    acc[tap] = mma(A[1], Bt[0], acc[tap]); acc[tap] = mma(A[0], Bt[1], acc[tap]); acc[tap] = mma(A[0], Bt[0], acc[tap]);
                } else {
                    acc[tap] = mma(A[1], Bt[1], acc[tap]); acc[tap] = mma(A[0], Bt[NP - 1], acc[tap]); acc[tap] = mma(A[NP - 1], Bt[0], acc[tap]);
                    acc[tap] = mma(A[0], Bt[1], acc[tap]); acc[tap] = mma(A[1], Bt[0], acc[tap]); acc[tap] = mma(A[0], Bt[0], acc[tap]);
                }
                if (tap == 0) load_piece(nextc, kb);                 // pieces 0..7 ride along the matrix phase
            }
        }
        load_piece(nextc, NV);
        __syncthreads();
        if (next < ntiles) write_tile(next);
        __syncthreads();
        tile = next;
    }

    float* out = a.partial + (size_t)blockIdx.x * (KW * 4096 + 64);
    // every wave owns its block of the slab: straight to global (128-B row segments)
#pragma unroll
    for (int k = 0; k < KW; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(k * 64 + mt * 32 + mfma_row(r, half)) * 64 + nt * 32 + l31] = H ? acc[k][r] * ginv : acc[k][r];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float v = half_wave_sum(bsum[i]);
        if (l31 == 0) out[KW * 4096 + c0 + 8 * i] = v;
    }
}

template <int XPRO, bool H = false>
int launch_wgrad64bf7(const Wgrad64Args& a, int* grid_out, hipStream_t stream) {
    constexpr size_t lds = (size_t)((H ? 2 : 3) * 64 * 136 + (H ? 2 : 3) * 64 * 152) * 2;
    static wm::DevOnce attr_done;
    auto kern = wgrad64bf7_kernel<XPRO, H>;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(kern), lds, attr_done)) return rc;
    const int ntiles = a.B * ((a.T + 127) / 128);
    const int grid = ntiles < kNumCU ? ntiles : kNumCU;
    *grid_out = grid;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}

// f16 two-piece image of a k3 weight for dwgrad64bf_kernel<..., H = true>: [2 pieces][3 taps][64 out][64 in] f16 of w * ws, ws = the power
// of two that brings max |w| to [2^9, 2^10), followed by {ws, 1 / ws} as two floats.  One workgroup (12 288 values).
__global__ __launch_bounds__(1024) void pack_w64_h_kernel(const float* __restrict__ w, const float* __restrict__ row_scale,
                                                          unsigned short* __restrict__ wph, int mode) {
    __shared__ float red[16];
    float v[12];                                    // the thread's 12 of the 12 288 values: one trip to memory
    float mx = 0.f;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        const int i = threadIdx.x + 1024 * j, tap = i / 4096, out = (i / 64) % 64, in = i % 64;
        v[j] = (mode == 0) ? w[(out * 64 + in) * 3 + tap] : w[(in * 64 + out) * 3 + (2 - tap)];
        if (row_scale) v[j] *= row_scale[out];      // a per-output-channel factor (folded BatchNorm scale) rides in the weights
        mx = fmaxf(mx, fabsf(v[j]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) m = fmaxf(m, red[i]);
    float ws = 1.f;
    if (m > 0.f && m < 3.0e38f) ws = exp2f(floorf(log2f(1023.f / m)));
    ws = fminf(fmaxf(ws, 1.0e-30f), 1.0e30f);
    if (threadIdx.x == 0) {
        float* tail = reinterpret_cast<float*>(wph + 2 * 3 * 4096);
        tail[0] = ws; tail[1] = 1.f / ws;
    }
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        const int i = threadIdx.x + 1024 * j;
        const float x = v[j] * ws;
        const _Float16 hi = (_Float16)x;
        const _Float16 lo = (_Float16)(x - (float)hi);
        wph[i] = __builtin_bit_cast(unsigned short, hi);
        wph[3 * 4096 + i] = __builtin_bit_cast(unsigned short, lo);
    }
}

// the same for the 7-tap ConvTranspose1d weight w[in][out][7] (conv64bf7p_kernel<.., H = true>): [2 pieces][7 taps][64 out][64 in] f16 +
// {ws, 1 / ws}; mode 2 forward, 3 data gradient (as wm_pack_w64_bf7)
__global__ __launch_bounds__(1024) void pack_w64_h7_kernel(const float* __restrict__ w, unsigned short* __restrict__ wph, int mode) {
    __shared__ float red[16];
    float v[28];
    float mx = 0.f;
#pragma unroll
    for (int j = 0; j < 28; ++j) {
        const int i = threadIdx.x + 1024 * j, tap = i / 4096, out = (i / 64) % 64, in = i % 64;
        v[j] = (mode == 2) ? w[(in * 64 + out) * 7 + (6 - tap)] : w[(out * 64 + in) * 7 + tap];
        mx = fmaxf(mx, fabsf(v[j]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) m = fmaxf(m, red[i]);
    float ws = 1.f;
    if (m > 0.f && m < 3.0e38f) ws = exp2f(floorf(log2f(1023.f / m)));
    ws = fminf(fmaxf(ws, 1.0e-30f), 1.0e30f);
    if (threadIdx.x == 0) {
        float* tail = reinterpret_cast<float*>(wph + 2 * 7 * 4096);
        tail[0] = ws; tail[1] = 1.f / ws;
    }
#pragma unroll
    for (int j = 0; j < 28; ++j) {
        const int i = threadIdx.x + 1024 * j;
        const float x = v[j] * ws;
        const _Float16 hi = (_Float16)x;
        const _Float16 lo = (_Float16)(x - (float)hi);
        wph[i] = __builtin_bit_cast(unsigned short, hi);
        wph[7 * 4096 + i] = __builtin_bit_cast(unsigned short, lo);
    }
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

WM_STAMP_SETTER(wm_debug_set_stamp_buffer)

// bf16x6 build of the k3 convolution (fp32-grade results on the bf16 matrix cores); wpb from wm_pack_w64_bf.
// Same pro / epi / stats contract as wm_conv64 with KW = 3.
int wm_pack_w64_bf(const float* w, void* wpb, int mode, hipStream_t stream) {
    if (mode < 0 || mode > 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_w64_bf_kernel, dim3(48), dim3(256), 0, stream, w, (const float*)nullptr, reinterpret_cast<unsigned short*>(wpb), mode);
    WM_CHECK_LAUNCH();
    return 0;
}
// forward image (mode 0) of w[out][in][k] * row_scale[out]
int wm_pack_w64_bf_scaled(const float* w, const float* row_scale, void* wpb, hipStream_t stream) {
    if (!w || !row_scale || !wpb) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_w64_bf_kernel, dim3(48), dim3(256), 0, stream, w, row_scale, reinterpret_cast<unsigned short*>(wpb), 0);
    WM_CHECK_LAUNCH();
    return 0;
}

static int g_bf_schedule = 2;   // 0: phase-serial kernel | 2: register-resident weights + interleaved pipeline (fastest, needs T % 128 == 0)
int wm_set_conv_bf_schedule(int schedule, hipStream_t) { g_bf_schedule = (schedule == 2) ? 2 : 0; return 0; }

int wm_conv64_bf(const float* x, const float* x2, const void* wpb, const float* pa, const float* pb, const float* pc,
                 const float* bias, const float* e1, const float* ea, const float* eb, float* y, float* stats,
                 int B, int T, int pro, int epi, int arith, hipStream_t stream) {
    if (B <= 0 || T <= 0 || (T & 3)) return (int)hipErrorInvalidValue;
    Conv64Args a{x, x2, reinterpret_cast<const float*>(wpb), pa, pb, pc, bias, e1, ea, eb, y, stats, B, T};
    const bool st = stats != nullptr;
    if (arith == 1) {                    // f16 two-piece split (wpb from wm_pack_w64_h): the forward convolutions of the pipelined kernel only
        if (g_bf_schedule != 2 || (T & 127)) return (int)hipErrorInvalidValue;
        if (pro == PRO_BNRELU && epi == EPI_BNADDRELU && !st) return launch_conv64bf3<PRO_BNRELU, EPI_BNADDRELU, false, true>(a, stream);
        if (epi != EPI_BIAS) return (int)hipErrorInvalidValue;
        if (pro == PRO_NONE) return st ? launch_conv64bf3<PRO_NONE, EPI_BIAS, true, true>(a, stream) : launch_conv64bf3<PRO_NONE, EPI_BIAS, false, true>(a, stream);
        if (pro == PRO_BNRELU) return st ? launch_conv64bf3<PRO_BNRELU, EPI_BIAS, true, true>(a, stream) : launch_conv64bf3<PRO_BNRELU, EPI_BIAS, false, true>(a, stream);
        return (int)hipErrorInvalidValue;
    }
    if (arith != 0) return (int)hipErrorInvalidValue;
    if (pro == PRO_NONE && !st) {        // main14b_2's 64-channel blocks (no BatchNorm): the phase-serial kernel, any T % 4 == 0
        if (epi == EPI_BIASELU) return launch_conv64bf<PRO_NONE, EPI_BIASELU, false>(a, stream);
        if (epi == EPI_BIASADDELU) return launch_conv64bf<PRO_NONE, EPI_BIASADDELU, false>(a, stream);
        if (epi == EPI_MULDELU) return launch_conv64bf<PRO_NONE, EPI_MULDELU, false>(a, stream);
        if (epi == EPI_ADD) return launch_conv64bf<PRO_NONE, EPI_ADD, false>(a, stream);
        if (epi == EPI_NONE) return launch_conv64bf<PRO_NONE, EPI_NONE, false>(a, stream);
    }
    if (g_bf_schedule == 2 && (T & 127) == 0) {
        if (pro == PRO_BNRELU && epi == EPI_BNADDRELU && !st) return launch_conv64bf3<PRO_BNRELU, EPI_BNADDRELU, false>(a, stream);
        if (pro == PRO_NONE && epi == EPI_BIAS) return st ? launch_conv64bf3<PRO_NONE, EPI_BIAS, true>(a, stream) : launch_conv64bf3<PRO_NONE, EPI_BIAS, false>(a, stream);
        if (pro == PRO_BNRELU && epi == EPI_BIAS) return st ? launch_conv64bf3<PRO_BNRELU, EPI_BIAS, true>(a, stream) : launch_conv64bf3<PRO_BNRELU, EPI_BIAS, false>(a, stream);
        if (pro == PRO_BNBWD && epi == EPI_RELUMASK && st) return launch_conv64bf3<PRO_BNBWD, EPI_RELUMASK, true>(a, stream);
        if (pro == PRO_BNBWD && epi == EPI_ADD && !st) return launch_conv64bf3<PRO_BNBWD, EPI_ADD, false>(a, stream);
        if (pro == PRO_BNBWD && epi == EPI_NONE && !st) return launch_conv64bf3<PRO_BNBWD, EPI_NONE, false>(a, stream);
        return (int)hipErrorInvalidValue;
    }
    if (pro == PRO_NONE && epi == EPI_BIAS) return st ? launch_conv64bf<PRO_NONE, EPI_BIAS, true>(a, stream) : launch_conv64bf<PRO_NONE, EPI_BIAS, false>(a, stream);
    if (pro == PRO_BNRELU && epi == EPI_BIAS) return st ? launch_conv64bf<PRO_BNRELU, EPI_BIAS, true>(a, stream) : launch_conv64bf<PRO_BNRELU, EPI_BIAS, false>(a, stream);
    if (pro == PRO_BNBWD && epi == EPI_RELUMASK && st) return launch_conv64bf<PRO_BNBWD, EPI_RELUMASK, true>(a, stream);
    if (pro == PRO_BNBWD && epi == EPI_ADD && !st) return launch_conv64bf<PRO_BNBWD, EPI_ADD, false>(a, stream);
    if (pro == PRO_BNBWD && epi == EPI_NONE && !st) return launch_conv64bf<PRO_BNBWD, EPI_NONE, false>(a, stream);
    return (int)hipErrorInvalidValue;
}

// bf16x6 build of the 7-tap ConvTranspose1d (forward: mode 2 image, pro 0|2, epi 0; data gradient: mode 3 image, pro 0, epi 3)
int wm_pack_w64_bf7(const float* w, void* wpb, int mode, hipStream_t stream) {
    if (mode != 2 && mode != 3) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_w64_bf7_kernel, dim3((7 * 4096 + 255) / 256), dim3(256), 0, stream, w, reinterpret_cast<unsigned short*>(wpb), mode);
    WM_CHECK_LAUNCH();
    return 0;
}
int wm_conv64_bf7(const float* x, const void* wpb, const float* vec, const float* bias, float* y, int B, int T, int pro, int epi,
                  int arith, const float* gscale, hipStream_t stream) {
    if (B <= 0 || T <= 0 || (T & 3)) return (int)hipErrorInvalidValue;
    Conv64Args a{x, nullptr, reinterpret_cast<const float*>(wpb), vec, gscale, nullptr, bias, nullptr, nullptr, nullptr, y, nullptr, B, T};
    if (arith == 1) {                     // f16 two-piece split (wpb from wm_pack_w64_h7): the pipelined kernel only
        if (!WM_BF7_PIPE || (T & 127)) return (int)hipErrorInvalidValue;
        if (pro == PRO_NONE && epi == EPI_BIAS) return launch_conv64bf7p<PRO_NONE, EPI_BIAS, true>(a, stream);
        if (pro == PRO_ADDVEC && epi == EPI_BIAS) return launch_conv64bf7p<PRO_ADDVEC, EPI_BIAS, true>(a, stream);
        if (pro == PRO_NONE && epi == EPI_NONE) return launch_conv64bf7p<PRO_NONE, EPI_NONE, true>(a, stream);
        return (int)hipErrorInvalidValue;
    }
    if (arith != 0) return (int)hipErrorInvalidValue;
    a.pb = nullptr;
#if WM_BF7_PIPE
    if ((T & 127) == 0) {                 // register-resident weights + double-buffered input image (conv64bf7p_kernel)
        if (pro == PRO_NONE && epi == EPI_BIAS) return launch_conv64bf7p<PRO_NONE, EPI_BIAS>(a, stream);
        if (pro == PRO_ADDVEC && epi == EPI_BIAS) return launch_conv64bf7p<PRO_ADDVEC, EPI_BIAS>(a, stream);
        if (pro == PRO_NONE && epi == EPI_NONE) return launch_conv64bf7p<PRO_NONE, EPI_NONE>(a, stream);
    }
#endif
    if (pro == PRO_NONE && epi == EPI_BIAS) return launch_conv64bf7<PRO_NONE, EPI_BIAS>(a, stream);
    if (pro == PRO_ADDVEC && epi == EPI_BIAS) return launch_conv64bf7<PRO_ADDVEC, EPI_BIAS>(a, stream);
    if (pro == PRO_NONE && epi == EPI_NONE) return launch_conv64bf7<PRO_NONE, EPI_NONE>(a, stream);
    return (int)hipErrorInvalidValue;
}

int wm_pack_w64_h7(const float* w, void* wph, int mode, hipStream_t stream) {
    if (mode != 2 && mode != 3) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_w64_h7_kernel, dim3(1), dim3(1024), 0, stream, w, reinterpret_cast<unsigned short*>(wph), mode);
    WM_CHECK_LAUNCH();
    return 0;
}

// bf16x6 build of the 7-tap ConvTranspose1d weight gradient (= wm_wgrad64 with KW 7, gpro 0, layout 1): dw [in][out][7]
int wm_wgrad64_bf7(const float* g, const float* x, const float* vec, float* partial, float* dw, float* dbias, int B, int T,
                   int xpro, int accumulate, int arith, const float* gscale, hipStream_t stream) {
    if (B <= 0 || T <= 0 || (T & 3) || (arith != 0 && arith != 1) || (arith == 1 && !gscale)) return (int)hipErrorInvalidValue;
    Wgrad64Args a{g, nullptr, arith == 1 ? gscale : nullptr, nullptr, nullptr, x, vec, nullptr, partial, B, T};
    int grid = 0, rc = (int)hipErrorInvalidValue;
    if (arith == 1) {
        if (xpro == PRO_ADDVEC) rc = launch_wgrad64bf7<PRO_ADDVEC, true>(a, &grid, stream);
        else if (xpro == PRO_NONE) rc = launch_wgrad64bf7<PRO_NONE, true>(a, &grid, stream);
    } else if (xpro == PRO_ADDVEC) rc = launch_wgrad64bf7<PRO_ADDVEC>(a, &grid, stream);
    else if (xpro == PRO_NONE) rc = launch_wgrad64bf7<PRO_NONE>(a, &grid, stream);
    if (rc) return rc;
    const int n = 7 * 4096 + 64;
    hipLaunchKernelGGL(wgrad64_reduce_kernel, dim3((n + 63) / 64), dim3(256), 0, stream, (const float*)partial, grid, 7, 1, dw,
                       dbias, accumulate);
    WM_CHECK_LAUNCH();
    return 0;
}

// bf16x6 build of the k3 weight gradient (same contract as wm_wgrad64 with KW = 3, layout 0)
int wm_wgrad64_bf(const float* g, const float* g2, const float* ga, const float* gb, const float* gc,
                  const float* x, const float* xa, const float* xb, float* partial, float* dw, float* dbias,
                  int B, int T, int gpro, int xpro, int accumulate, hipStream_t stream) {
    if (B <= 0 || T <= 0 || (T & 3)) return (int)hipErrorInvalidValue;
    Wgrad64Args a{g, g2, ga, gb, gc, x, xa, xb, partial, B, T};
    int grid = 0, rc = (int)hipErrorInvalidValue;
    const bool small = (accumulate & 2) != 0;            // output-split build: ~200 registers, co-resident with the LSTM recurrences
    if (gpro == PRO_BNBWD && xpro == PRO_BNRELU)
        rc = small ? launch_wgrad64bf_small<PRO_BNBWD, PRO_BNRELU>(a, &grid, stream) : launch_wgrad64bf<PRO_BNBWD, PRO_BNRELU>(a, &grid, stream);
    else if (gpro == PRO_BNBWD && xpro == PRO_NONE)
        rc = small ? launch_wgrad64bf_small<PRO_BNBWD, PRO_NONE>(a, &grid, stream) : launch_wgrad64bf<PRO_BNBWD, PRO_NONE>(a, &grid, stream);
    else if (gpro == PRO_NONE && xpro == PRO_NONE)            // main14b_2's 64-channel blocks: both operands as they are
        rc = launch_wgrad64bf<PRO_NONE, PRO_NONE>(a, &grid, stream);
    if (rc) return rc;
    const int n = 3 * 4096 + 64;
    hipLaunchKernelGGL(wgrad64_reduce_kernel, dim3((n + 63) / 64), dim3(256), 0, stream, (const float*)partial, grid, 3, 0, dw,
                       dbias, accumulate & 1);
    WM_CHECK_LAUNCH();
    return 0;
}

// f16 two-piece weight image for wm_dwgrad64_bf arith 1: 2 * 3 * 4096 f16 + 2 floats (mode 0 forward | 1 data gradient, as wm_pack_w64_bf)
int wm_pack_w64_h(const float* w, void* wph, int mode, hipStream_t stream) {
    if (!w || !wph || mode < 0 || mode > 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_w64_h_kernel, dim3(1), dim3(1024), 0, stream, w, (const float*)nullptr, reinterpret_cast<unsigned short*>(wph), mode);
    WM_CHECK_LAUNCH();
    return 0;
}
// forward image (mode 0) of w[out][in][k] * row_scale[out] (wm_resblock_eval_bf arith 1)
int wm_pack_w64_h_scaled(const float* w, const float* row_scale, void* wph, hipStream_t stream) {
    if (!w || !row_scale || !wph) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_w64_h_kernel, dim3(1), dim3(1024), 0, stream, w, row_scale, reinterpret_cast<unsigned short*>(wph), 0);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
