// conv64.hpp's k3 forward / data-gradient family: the phase-serial conv64bf and the pipelined conv64bf3 kernels, and the k3 weight
// images (bf16 three-piece, f16 two-piece) that the conv64_eval and conv64_dwgrad units also consume
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
    constexpr bool TAIL = (PRO == PRO_TAIL);              // the input is the previous ResBlock's tail, formed here from x and x2 = y2
    constexpr bool STEM = (PRO == PRO_STEM);              // the input is the stem's output, formed here from the clips x = s [B,1,T]
    constexpr bool FORM = TAIL || STEM;                   // the formed input also leaves through tout
    constexpr bool TWO = (PRO == PRO_BNBWD || TAIL);
    static_assert(!FORM || H, "the tail and stem prologues exist in the f16 build only");
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
    // PRO_STEM stages the clip instead of a frame: per combo the ten samples s[tq - 3 .. tq + 6] around its time quad tq as three
    // loads out of the aligned quads at tq - 4, tq, tq + 4, per halo column the two quads that hold its seven taps.  Buffer loads over
    // the clip's T samples: a quad outside [0, T) reads zero, which is the stem's padding (T % 128 == 0, so a quad is inside or
    // outside as a whole; the one in front of the clip takes an offset past every clip instead of a negative one).  The signal is
    // 1/64 of a frame and stays in L2.  Only what the taps read is loaded (s[tq - 4] and s[tq + 7] are not): a register that is loaded
    // and never read is handed out again at once, and the write to it then waits for the load -- with the stores in front of it.
    f32x3 sgl[STEM ? NC : 1], sgr[STEM ? NC : 1];
    f32x4 sgm[STEM ? NC : 1], hg[2];
    auto clip_srd = [&](int b) { return make_srd(a.x + (size_t)b * T, (size_t)T * sizeof(float)); };
    // global -> register staging of one tile, in five pieces (4 combos + halo) so that the main loop can issue them
    // a few at a time: a 32-KB burst per CU backs up the memory pipeline and blocks the wave at issue for ~2.5 K cycles
    auto load_combo = [&](int tile, int i) {
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        if (STEM) {
            const wm_srd_t sc = clip_srd(b);
            const int tq = t0 + 4 * (q0 + 8 * i);
            sgl[STEM ? i : 0] = buf_load3(sc, tq >= 4 ? (unsigned)(tq - 3) * 4u : 0xFFFFFF00u, 0);
            sgm[STEM ? i : 0] = buf_load4(sc, (unsigned)tq * 4u, 0);
            sgr[STEM ? i : 0] = buf_load3(sc, (unsigned)(tq + 4) * 4u, 0);
            return;
        }
        const size_t o = ((size_t)b * 64 + c0) * T + t0 + 4 * (q0 + 8 * i);
        sa[i] = *reinterpret_cast<const float4*>(a.x + o);
        sb[i] = *reinterpret_cast<const float4*>(a.x + o + T);
        if (TWO) { sa2[i] = *reinterpret_cast<const float4*>(a.x2 + o); sb2[i] = *reinterpret_cast<const float4*>(a.x2 + o + T); }
    };
    auto load_halo = [&](int tile) {              // branch-free: clamped address, masked when written to LDS
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        if (STEM) {                               // column t0 - 1: s[t0 - 4 .. t0 + 2]; column t0 + NT: s[t0 + NT - 3 .. t0 + NT + 3]
            const wm_srd_t sc = clip_srd(b);
            const int hq = hh ? t0 + NT - 4 : t0 - 4;
            hg[0] = buf_load4(sc, hq >= 0 ? (unsigned)hq * 4u : 0xFFFFFF00u, 0);
            hg[1] = buf_load4(sc, (unsigned)(hq + 4) * 4u, 0);
            return;
        }
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
        Cs[tid] = (PRO == PRO_BNRELU || PRO == PRO_BNBWD || TAIL) ? a.pa[tid] : 0.f;
        Cs[64 + tid] = (PRO == PRO_BNRELU || PRO == PRO_BNBWD || TAIL) ? a.pb[tid] : 0.f;
        Cs[128 + tid] = (PRO == PRO_BNBWD) ? a.pc[tid] : 0.f;
        Cs[192 + tid] = (PRO == PRO_BNBWD) ? a.pb[64 + tid] : (((EPI == EPI_BIAS || EPI == EPI_BNADDRELU) && a.bias) ? a.bias[tid] : 0.f);
        Cs[256 + tid] = (EPI == EPI_RELUMASK || EPI == EPI_BNADDRELU) ? a.ea[tid] : 0.f;
        Cs[320 + tid] = (EPI == EPI_RELUMASK || EPI == EPI_BNADDRELU) ? a.eb[tid] : 0.f;
    }
    __syncthreads();
    // per-thread prologue constants (the staging channels never change)
    const float ka0 = Cs[c0], ka1 = Cs[c0 + 1], kb0 = Cs[64 + c0], kb1 = Cs[64 + c0 + 1];
    const float kc0 = Cs[128 + c0], kc1 = Cs[128 + c0 + 1];
    const float kl0 = (PRO == PRO_BNBWD) ? Cs[192 + c0] : 0.f, kl1 = (PRO == PRO_BNBWD) ? Cs[192 + c0 + 1] : 0.f;
    const float ha = Cs[hc], hb = Cs[64 + hc], hcc = Cs[128 + hc], hlo = (PRO == PRO_BNBWD) ? Cs[192 + hc] : 0.f;
    // PRO_STEM: the seven taps and the bias of the two staging channels and of the halo channel (pa = the stem's w [64][7], pb = its bias)
    float kw0[STEM ? 7 : 1], kw1[STEM ? 7 : 1], kwh[STEM ? 7 : 1], kbs0 = 0.f, kbs1 = 0.f, kbsh = 0.f;
    if (STEM) {
#pragma unroll
        for (int j = 0; j < 7; ++j) { kw0[STEM ? j : 0] = a.pa[c0 * 7 + j]; kw1[STEM ? j : 0] = a.pa[(c0 + 1) * 7 + j]; kwh[STEM ? j : 0] = a.pa[hc * 7 + j]; }
        kbs0 = a.pb[c0]; kbs1 = a.pb[c0 + 1]; kbsh = a.pb[hc];
    }
    // stem_fwd_kernel's chain (small_convs.hip), to the letter: o = bias, then o = fmaf(w[j], s[t + j - 3], o) for j = 0..6 -- a tap
    // outside the clip is a multiply by the zero that was loaded, never skipped
    auto stem_form = [&](int i, int e, const float* w, float bias) -> float {
        const f32x3 g0 = sgl[STEM ? i : 0], g2 = sgr[STEM ? i : 0];
        const f32x4 g1 = sgm[STEM ? i : 0];
        const float g[10] = {g0.x, g0.y, g0.z, g1.x, g1.y, g1.z, g1.w, g2.x, g2.y, g2.z};       // s[tq - 3 .. tq + 6]
        float o = bias;
        // the chain starts and ends at an opaque point of its own slice: left to the optimiser, the two channels' chains are paired into
        // v_pk_fma_f32 (dearer beside MFMAs than the two v_fma_f32) and later elements' chains are hoisted out of their slices
        asm volatile("" : "+v"(o));
#pragma unroll
        for (int j = 0; j < 7; ++j) o = fmaf(w[STEM ? j : 0], g[e + j], o);
        asm volatile("" : "+v"(o));
        return o;
    };
    auto stem_form_halo = [&]() -> float {
        const float g[8] = {hg[0].x, hg[0].y, hg[0].z, hg[0].w, hg[1].x, hg[1].y, hg[1].z, hg[1].w};
        float o = kbsh;
#pragma unroll
        for (int j = 0; j < 7; ++j) o = fmaf(kwh[STEM ? j : 0], hh ? g[j + 1] : g[j], o);
        return o;
    };

    // PRO_TAIL: the formed value goes back into its staging register, and tail_store() writes the combo's two rows x one time quad
    // to `tout` as the tail kernel would have (16-B stores), with their sign bits: the eight lanes that share lane & 7 hold the 32
    // steps of one mask word of each row; lane >> 3 == 0 stores the first row's word, == 1 the second's (a null tmask: a descriptor
    // of zero bytes, every store dropped).  A halo column is rebuilt from x and x2 and never stored.
    // PRO_STEM: the same two 16-B stores of the formed rows, no sign bits (nothing behind the stem clamps).
    auto keep_formed = [&](int i, int e, float va, float vb) {
        if (e == 0) { sa[i].x = va; sb[i].x = vb; } else if (e == 1) { sa[i].y = va; sb[i].y = vb; }
        else if (e == 2) { sa[i].z = va; sb[i].z = vb; } else { sa[i].w = va; sb[i].w = vb; }
    };
    const wm_srd_t smask = make_srd(reinterpret_cast<const float*>(a.tmask), (TAIL && a.tmask) ? (size_t)a.B * 64 * (T >> 5) * 4 : 0);
    auto tail_store = [&](int tb, int tt0, int i) {
        const size_t o = ((size_t)tb * 64 + c0) * T + tt0 + 4 * (q0 + 8 * i);
        *reinterpret_cast<float4*>(a.tout + o) = sa[i];
        *reinterpret_cast<float4*>(a.tout + o + T) = sb[i];
        if (STEM) return;
        const unsigned ma = mask_merge8(sign_nibble(sa[i]) << (4 * q0)), mb = mask_merge8(sign_nibble(sb[i]) << (4 * q0));
        const unsigned word = (unsigned)(tb * 64 + c0 + (q0 & 1)) * (unsigned)(T >> 5) + (unsigned)((tt0 >> 5) + i);
        __builtin_amdgcn_raw_buffer_store_b32((q0 & 1) ? mb : ma, smask, (int)(q0 < 2 ? word * 4u : 0xFFFFFF00u), 0, 0);
    };

    // one (combo i, element e) unit of the split: two channels x one time step -> 3 dwords
    auto split_unit = [&](unsigned* X32, int t0, int i, int e) {
        const float4 fa = sa[i], fb = sb[i];
        float va = (e == 0) ? fa.x : (e == 1) ? fa.y : (e == 2) ? fa.z : fa.w;
        float vb = (e == 0) ? fb.x : (e == 1) ? fb.y : (e == 2) ? fb.z : fb.w;
        if (STEM) {
            va = stem_form(i, e, kw0, kbs0); vb = stem_form(i, e, kw1, kbs1);
            keep_formed(i, e, va, vb);
        } else if (PRO != PRO_NONE) {
            float wa = 0.f, wb = 0.f;
            if (TWO) {
                const float4 ga = sa2[i], gb = sb2[i];
                wa = (e == 0) ? ga.x : (e == 1) ? ga.y : (e == 2) ? ga.z : ga.w;
                wb = (e == 0) ? gb.x : (e == 1) ? gb.y : (e == 2) ? gb.z : gb.w;
            }
            va = pro_apply<PRO>(va, wa, ka0, kb0, kc0, kl0);
            vb = pro_apply<PRO>(vb, wb, ka1, kb1, kc1, kl1);
            if (TAIL) keep_formed(i, e, va, vb);
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
            if (STEM) v = stem_form_halo();
            else if (PRO != PRO_NONE) v = pro_apply<PRO>(v, hl2, ha, hb, hcc, hlo);
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
            if (TAIL) keep_formed(i, e, va, vb);
        }
        sva = va; svb = vb;
        asm volatile("" : "+v"(sva), "+v"(svb));
    };
    // PRO_STEM's pick in two slices, one seven-FMA chain each: the first channel, then the second and the hand-over
    auto stem_pick_a = [&](int i, int e) {
        sva = stem_form(i, e, kw0, kbs0);
        asm volatile("" : "+v"(sva));
    };
    auto stem_pick_b = [&](int i, int e) {
        svb = stem_form(i, e, kw1, kbs1);
        keep_formed(i, e, sva, svb);
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
        if (STEM) v = stem_form_halo();
        else if (PRO != PRO_NONE) v = pro_apply<PRO>(v, hl2, ha, hb, hcc, hlo);
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
        if (FORM) {
#pragma unroll
            for (int i = 0; i < NC; ++i) tail_store(min(tile, ntiles - 1) / tilesPerClip, t0, i);
        }
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
        const int nb_ = next / tilesPerClip, nt0 = (next - nb_ * tilesPerClip) * NT;
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
        if (STEM && h < 16) {                                                                                                   \
            if ((k) == 0) stem_pick_a(h >> 2, h & 3);                                                                           \
            if ((k) == 1) stem_pick_b(h >> 2, h & 3);                                                                           \
            if ((k) == 2) { split_st1(); if ((h & 3) == 3) tail_store(nb_, nt0, h >> 2); }                                      \
            if ((k) == 3) { split_out(reinterpret_cast<unsigned*>(xnxt), h >> 2, h & 3); if ((h & 3) == 3) load_combo(next2, h >> 2); } \
        } else if (h < 16) {                                                                                                    \
            if ((k) == 0) split_pick(h >> 2, h & 3);                                                                            \
            if ((k) == 1) split_st1();                                                                                          \
            if ((k) == 2) { split_st2(); if (TAIL && (h & 3) == 3) tail_store(nb_, nt0, h >> 2); }                              \
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
                if (FORM) {                              // slice 2 (free in this build) stores a finished combo of the formed tile
                    acc[nt] = mma(Wr[s][0], Bf[1], acc[nt]); FENCE; BF3_SLICE(2) FENCE; BF3_SLICE(3) FENCE;
                    acc[nt] = mma(Wr[s][0], Bf[0], acc[nt]); FENCE; BF3_SLICE(4) FENCE; BF3_SLICE(5) FENCE;
                } else {
                    acc[nt] = mma(Wr[s][0], Bf[1], acc[nt]); FENCE; BF3_SLICE(3) FENCE; BF3_SLICE(4) FENCE;
                    acc[nt] = mma(Wr[s][0], Bf[0], acc[nt]); FENCE; BF3_SLICE(5) FENCE;
                }
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

// A training ResBlock's conv1 whose input is the PREVIOUS block's tail, formed on load: out = relu(x + y2 * sc2 + sh2) and its sign
// bits leave as side products exactly as wm_bn_add_relu_mask writes them (mask may be null), y = conv(out) + bias and stats exactly as
// wm_conv64_bf(pro 0, epi 0, arith 1) on that out.  wpb_h from wm_pack_w64_h (mode 0).  The pipelined f16 build only: anything else
// (T % 128 != 0, schedule 0, no stats) is hipErrorInvalidValue and nothing is written.
int wm_conv64_bf_tail(const float* x, const float* y2, const void* wpb_h, const float* sc2, const float* sh2, const float* bias,
                      float* out, void* mask, float* y, float* stats, int B, int T, hipStream_t stream) {
    if (B <= 0 || T <= 0 || (T & 127) || g_bf_schedule != 2) return (int)hipErrorInvalidValue;
    if (!x || !y2 || !wpb_h || !sc2 || !sh2 || !out || !y || !stats) return (int)hipErrorInvalidValue;
    if ((unsigned long long)B * 64ull * (unsigned long long)(T >> 5) * 4ull >= 0xfffff000ull) return (int)hipErrorInvalidValue;   // mask offsets are 32-bit
    Conv64Args a{x, y2, reinterpret_cast<const float*>(wpb_h), sc2, sh2, nullptr, bias, nullptr, nullptr, nullptr, y, stats, B, T,
                 out, reinterpret_cast<unsigned*>(mask)};
    return launch_conv64bf3<PRO_TAIL, EPI_BIAS, true, true>(a, stream);
}

// The first training ResBlock's conv1 with the stem in front formed on load: y0 = Conv1d(1, 64, 7, padding = 3)(s) leaves as a side
// product exactly as wm_stem_fwd writes it, y = conv(y0) + bias and stats exactly as wm_conv64_bf(pro 0, epi 0, arith 1) on that y0.
// s [B,1,T], stem_w [64,7], stem_b [64]; wpb_h from wm_pack_w64_h (mode 0).  wm_conv64_bf_tail's conditions: anything else
// (T % 128 != 0, schedule 0, a null pointer) is hipErrorInvalidValue and nothing is written.
int wm_conv64_bf_stem(const float* s, const float* stem_w, const float* stem_b, const void* wpb_h, const float* bias, float* y0,
                      float* y, float* stats, int B, int T, hipStream_t stream) {
    if (B <= 0 || T <= 0 || (T & 127) || T >= (1 << 29) || g_bf_schedule != 2) return (int)hipErrorInvalidValue;   // clip offsets are 32-bit bytes
    if (!s || !stem_w || !stem_b || !wpb_h || !y0 || !y || !stats) return (int)hipErrorInvalidValue;
    Conv64Args a{s, nullptr, reinterpret_cast<const float*>(wpb_h), stem_w, stem_b, nullptr, bias, nullptr, nullptr, nullptr, y, stats, B, T,
                 y0, nullptr};
    return launch_conv64bf3<PRO_STEM, EPI_BIAS, true, true>(a, stream);
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
