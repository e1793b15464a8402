// conv64.hpp's 7-tap ConvTranspose1d family: the two forward / data-gradient kernels, their weight images and the weight gradient
#include "conv64.hpp"

namespace {

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

extern "C" {

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

}  // extern "C"
