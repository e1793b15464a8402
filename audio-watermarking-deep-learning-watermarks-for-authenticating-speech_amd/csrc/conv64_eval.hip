// conv64.hpp's inference family: the one-launch ResBlock
#include "conv64.hpp"

namespace {
// ---------------------------------------------------------------------------------------------
// Inference ResBlock in ONE launch:  out = relu(x + BN2(conv2(relu(BN1(conv1(x))))))  with both BatchNorms in eval
// mode (running statistics folded into per-channel scale / shift), py/main16.py:112-125.  Frame passes over HBM: x in,
// out out -- the intermediate never leaves the CU.
// A workgroup walks 124-column output tiles.  Its x window is the 128 columns [w0, w0+128), w0 = 124 k - 4: exactly 32
// aligned float4 per channel, no halo loads.  conv1 runs over MFMA columns j = 0..127 (a1 at time w0 + 1 + j, valid for
// j < 126), its epilogue applies BN1 + ReLU (and the zero padding of conv2: a1 = 0 outside the clip), splits the result
// into its three bf16 pieces and writes them to a second LDS image; conv2 reads that image (output column i = time
// w0 + 2 + i, valid for i < 124) and its epilogue adds BN2 and the residual x (re-read from L2 in accumulator layout) and
// stores.  Both convolutions keep the weight fragments of the wave's 32 output rows in registers (2 x 144 VGPRs of the
// 512 a lone wave may use), so LDS holds only the two activation images (2 x 55 KB).  While conv2 runs, the same
// instruction stream splits the NEXT tile's x window into the (by then free) x image; while conv1 runs, it fetches the
// residual operand.
// ---------------------------------------------------------------------------------------------
struct RbeArgs {
    const float* x;       // [B,64,T]
    const void* w1;       // packed bf16 image [3 pieces][3 taps][64 out][64 in] of w * sc[out] (wm_pack_w64_bf_scaled)
    const void* w2;
    const float* b1; const float* sc1; const float* sh1;     // conv bias, folded BN scale / shift
    const float* b2; const float* sc2; const float* sh2;
    float* y;             // [B,64,T]
    int B, T;
};

// H = true: f16 two-piece build (three products per product): w1 / w2 = wm_pack_w64_h_scaled images (w * sc[out] * ws, {ws, 1 / ws} behind
// the image), x and the intermediate a1 split into hi / lo f16 pieces unscaled, accumulators times 1 / ws in both epilogues
template <bool H>
__global__ __launch_bounds__(256) void resblock_eval_kernel(RbeArgs a) {
    constexpr int KW = 3, NTO = 124, ROWS = 130, PITCH = 72, NP = H ? 2 : 3, NC = 4;
    constexpr int XBUF = NP * ROWS * PITCH;               // bf16 elements per image
    extern __shared__ __align__(16) unsigned char smem_raw[];
    unsigned short* Xb = reinterpret_cast<unsigned short*>(smem_raw);              // x window: row r = time w0 + r
    unsigned short* Ab = Xb + XBUF;                                                // a1: row j = time w0 + 1 + j
    float* Cs = reinterpret_cast<float*>(Ab + XBUF);                               // [2][64]: k1 k2 (offsets; the scales ride in the weights)
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mt = wave & 1, nh = wave >> 1;
    const int T = a.T;
    const int tilesPerClip = (T + 2 + NTO - 1) / NTO, ntiles = a.B * tilesPerClip;

    u32x4 W1[12][NP], W2[12][NP];
    {
        const uint4* wg1 = reinterpret_cast<const uint4*>(a.w1);
        const uint4* wg2 = reinterpret_cast<const uint4*>(a.w2);
#pragma unroll
        for (int s = 0; s < 12; ++s)
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int e = ((p * KW + (s >> 2)) * 64 + 32 * mt + l31) * 64 + 16 * (s & 3) + 8 * half;
                // the second convolution's fragments are pinned into AGPRs (the MFMA reads its A operand from there in place):
                // 288 fragment registers do not fit the 256 VGPRs, and fragments the allocator spills are copied back per use
                u32x4 w2_ = __builtin_bit_cast(u32x4, wg2[e >> 3]);
                asm volatile("" : "+a"(w2_));
                W1[s][p] = __builtin_bit_cast(u32x4, wg1[e >> 3]);
                W2[s][p] = w2_;
            }
    }
    const float winv1 = H ? reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(a.w1) + NP * KW * 4096)[1] : 1.f;
    const float winv2 = H ? reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(a.w2) + NP * KW * 4096)[1] : 1.f;
    // staging map (fixed per thread): channel pair cp, time quads q0 + 8 i
    const int cp = wave * 8 + (lane & 7), c0 = 2 * cp, q0 = lane >> 3;
    float4 sa[NC], sb[NC];
    auto load_combo = [&](int tile, int i) {      // branch-free: clamped address, masked when written to LDS
        const int b = tile / tilesPerClip, w0 = (tile - b * tilesPerClip) * NTO - 4;
        const int t = min(max(w0 + 4 * (q0 + 8 * i), 0), T - 4);
        const size_t o = ((size_t)b * 64 + c0) * T + t;
        sa[i] = *reinterpret_cast<const float4*>(a.x + o);
        sb[i] = *reinterpret_cast<const float4*>(a.x + o + T);
    };
    auto split_unit = [&](int w0, int i, int e) {  // two channels x one time step of the window starting at w0 -> 3 dwords
        const int t = w0 + 4 * (q0 + 8 * i);
        const bool ok = (t >= 0) && (t < T);        // T % 4 == 0 and w0 % 4 == 0: a quad is inside or outside as a whole
        const float4 fa = sa[i], fb = sb[i];
        float va = (e == 0) ? fa.x : (e == 1) ? fa.y : (e == 2) ? fa.z : fa.w;
        float vb = (e == 0) ? fb.x : (e == 1) ? fb.y : (e == 2) ? fb.z : fb.w;
        va = ok ? va : 0.f; vb = ok ? vb : 0.f;
        unsigned* X32 = reinterpret_cast<unsigned*>(Xb);
        const int o = (4 * (q0 + 8 * i) + e) * (PITCH / 2) + cp;
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

    const int tstep = gridDim.x;
    int tile = xcd_slot();                                         // grid <= ntiles
#pragma unroll
    for (int i = 0; i < NC; ++i) load_combo(tile, i);
    if (tid < 64) {
        Cs[tid] = fmaf(a.b1 ? a.b1[tid] : 0.f, a.sc1[tid], a.sh1[tid]);
        Cs[64 + tid] = fmaf(a.b2 ? a.b2[tid] : 0.f, a.sc2[tid], a.sh2[tid]);
    }
    // rows 128, 129 of both images are read by the discarded MFMA columns only: keep them finite (zero)
    for (int i = tid; i < NP * 2 * (PITCH / 2); i += 256) {
        const int p = i / (2 * (PITCH / 2)), rem = i - p * (2 * (PITCH / 2));
        const int o = (p * ROWS + 128) * (PITCH / 2) + rem;
        reinterpret_cast<unsigned*>(Xb)[o] = 0u;
        reinterpret_cast<unsigned*>(Ab)[o] = 0u;
    }
    {
        const int w0 = (tile % tilesPerClip) * NTO - 4;
#pragma unroll
        for (int u = 0; u < 16; ++u) split_unit(w0, u >> 2, u & 3);
    }
    __syncthreads();
    // per-lane epilogue offsets: the 16 channels of this lane's accumulator rows (the same for both column blocks)
    float k1[16], k2[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = 32 * mt + mfma_row(r, half);
        k1[r] = Cs[co]; k2[r] = Cs[64 + co];
    }

    float e1r[32];
#ifdef WM_STAMP
    unsigned long long tm[6] = {0, 0, 0, 0, 0, 0};
#endif
    unsigned* const X32 = reinterpret_cast<unsigned*>(Xb);
    unsigned* const A32 = reinterpret_cast<unsigned*>(Ab);

    // One k-step of a matrix phase: the fragment reads of the NEXT step, then the six piece products with one slice of side
    // work (f0..f5: a handful of VALU / LDS / global instructions) pinned behind each of them.  The six MFMAs of a step
    // chain on one accumulator, so each waits 8 passes for its predecessor: the slice between two of them is free.  The
    // order is fixed by hand (sched_barrier fences): the group-barrier pattern conv64bf3 uses is not honoured here (the
    // weight fragments of two convolutions overflow into AGPRs and their copies break the pattern; the side work then lands
    // in one lump in front of six back-to-back MFMAs).
#define FENCE __builtin_amdgcn_sched_barrier(0)
    auto nop = []() {};
    auto mma = [&](const u32x4& A_, const u32x4& B_, f32x16 c) -> f32x16 {
        if (H) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, A_), __builtin_bit_cast(h16x8, B_), c, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A_), __builtin_bit_cast(bf16x8, B_), c, 0, 0, 0);
    };
    auto kstep = [&](const u32x4 (&W)[12][NP], const unsigned short* img, f32x16& ac, u32x4 (&Bq)[2][NP], int nt, int s,
                     auto&& f0, auto&& f1, auto&& f2, auto&& f3, auto&& f4, auto&& f5) __attribute__((always_inline)) {
        if (s + 1 < 12) {
#pragma unroll
            for (int p = 0; p < NP; ++p)
                Bq[(s + 1) & 1][p] = *reinterpret_cast<const u32x4*>(img + (p * ROWS + 32 * nt + ((s + 1) >> 2)) * PITCH + 16 * ((s + 1) & 3));
        }
        const u32x4* Bf = Bq[s & 1];
        FENCE;
        if (H) {                                         // lo hi, hi lo, hi hi: two slices behind every MFMA
            ac = mma(W[s][1], Bf[0], ac); FENCE; f0(); FENCE; f1(); FENCE;
            ac = mma(W[s][0], Bf[1], ac); FENCE; f2(); FENCE; f3(); FENCE;
            ac = mma(W[s][0], Bf[0], ac); FENCE; f4(); FENCE; f5(); FENCE;
        } else {
            ac = mma(W[s][1], Bf[1], ac); FENCE; f0(); FENCE;
            ac = mma(W[s][0], Bf[NP - 1], ac); FENCE; f1(); FENCE;
            ac = mma(W[s][NP - 1], Bf[0], ac); FENCE; f2(); FENCE;
            ac = mma(W[s][0], Bf[1], ac); FENCE; f3(); FENCE;
            ac = mma(W[s][1], Bf[0], ac); FENCE; f4(); FENCE;
            ac = mma(W[s][0], Bf[0], ac); FENCE; f5(); FENCE;
        }
    };
    // the bf16x3 split of a value pair in three stages (one slice each)
    float sva = 0.f, svb = 0.f;
    unsigned sp0 = 0, sp1 = 0, sp2 = 0;
    auto st1 = [&]() {
        if (H) {
            const h16x2 h = __builtin_convertvector(f32x2{sva, svb}, h16x2);
            sp0 = __builtin_bit_cast(unsigned, h);
            sva -= (float)h.x; svb -= (float)h.y;
        } else {
            const bf16x2 h = {(__bf16)sva, (__bf16)svb};
            sp0 = __builtin_bit_cast(unsigned, h);
            sva -= __uint_as_float(sp0 << 16); svb -= __uint_as_float(sp0 & 0xffff0000u);
        }
        asm volatile("" : "+v"(sva), "+v"(svb), "+v"(sp0));      // pins the stage into its slice (pure arithmetic sinks to its use otherwise)
    };
    auto st2 = [&]() {
        if (H) return;                                   // two pieces: no middle one
        const bf16x2 m = {(__bf16)sva, (__bf16)svb};
        sp1 = __builtin_bit_cast(unsigned, m);
        sva -= __uint_as_float(sp1 << 16); svb -= __uint_as_float(sp1 & 0xffff0000u);
        asm volatile("" : "+v"(sva), "+v"(svb), "+v"(sp1));
    };
    auto st3 = [&](unsigned* img32, int o) {
        if (H) {
            sp2 = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{sva, svb}, h16x2));
            img32[o] = sp0; img32[(ROWS * PITCH >> 1) + o] = sp2;
            return;
        }
        const bf16x2 l = {(__bf16)sva, (__bf16)svb};
        sp2 = __builtin_bit_cast(unsigned, l);
        img32[o] = sp0; img32[(ROWS * PITCH >> 1) + o] = sp1; img32[2 * (ROWS * PITCH >> 1) + o] = sp2;
    };

    while (tile < ntiles) {
        const int next = min(tile + tstep, ntiles - 1);
        const int b = tile / tilesPerClip, w0 = (tile - b * tilesPerClip) * NTO - 4, o0 = w0 + 2;
        const int nw0 = (next % tilesPerClip) * NTO - 4;
        // output column of accumulator block nt of this lane: byte offset inside a channel row, 0xffffffff (dropped by the
        // buffer unit / read as 0) when the column is not an output of this tile; in1[nt]: the a1 column lies inside the clip
        unsigned tcl[2];
        bool in1[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int i = 64 * nh + 32 * nt + l31, t = o0 + i, u = w0 + 1 + i;
            const bool ok = (i < NTO) && (t >= 0) && (t < T);
            tcl[nt] = ok ? (unsigned)(t + 4 * half * T) * 4u : 0xffffffffu;
            in1[nt] = (u >= 0) && (u < T);
        }
        // this wave's 32 channel rows of clip b, as buffer descriptors (scalar); row r sits at the scalar offset roff(r)
        const size_t slab = ((size_t)b * 64 + 32 * mt) * T;
        const wm_srd_t sxr = make_srd(a.x + slab, (size_t)32 * T * sizeof(float));
        const wm_srd_t syr = make_srd(a.y + slab, (size_t)32 * T * sizeof(float));
        auto roff = [&](int r) { return (unsigned)(((r & 3) + 8 * (r >> 2)) * T) * 4u; };                  // wave-uniform
        auto e1_load = [&](int idx) { e1r[idx] = buf_load(sxr, tcl[idx >> 4], roff(idx & 15)); };
        // epilogue 1 of accumulator pair pi (rows 2 pi, 2 pi + 1 = two adjacent channels) of block nt, in slices:
        // BN1 offset + ReLU + zero padding -> split stages -> a1 image
        auto e1_act = [&](const f32x16& ac, int nt, int pi) {
            const float v0 = fmaxf(H ? fmaf(ac[2 * pi], winv1, k1[2 * pi]) : ac[2 * pi] + k1[2 * pi], 0.f),
                        v1 = fmaxf(H ? fmaf(ac[2 * pi + 1], winv1, k1[2 * pi + 1]) : ac[2 * pi + 1] + k1[2 * pi + 1], 0.f);
            sva = in1[nt] ? v0 : 0.f; svb = in1[nt] ? v1 : 0.f;
            asm volatile("" : "+v"(sva), "+v"(svb));
        };
        auto e1_out = [&](int nt, int pi) {
            const int j = 64 * nh + 32 * nt + l31, co = 32 * mt + mfma_row(2 * pi, half);
            st3(A32, (j * PITCH + co) >> 1);
        };
        // split of unit (combo i, element e) of the next tile's x window, in slices
        auto x_pick = [&](int i, int e) {
            const int t = nw0 + 4 * (q0 + 8 * i);
            const bool ok = (t >= 0) && (t < T);
            const float4 fa = sa[i], fb = sb[i];
            const float va = (e == 0) ? fa.x : (e == 1) ? fa.y : (e == 2) ? fa.z : fa.w;
            const float vb = (e == 0) ? fb.x : (e == 1) ? fb.y : (e == 2) ? fb.z : fb.w;
            sva = ok ? va : 0.f; svb = ok ? vb : 0.f;
            asm volatile("" : "+v"(sva), "+v"(svb));
        };
        auto x_out = [&](int i, int e) { st3(X32, (4 * (q0 + 8 * i) + e) * (PITCH / 2) + cp); };
        // epilogue 2 of accumulator row r of block nt: BN2 offset + residual + ReLU + store
        auto e2_value = [&](const f32x16& ac, int nt, int r) {
            const float v = fmaxf(e1r[nt * 16 + r] + (H ? fmaf(ac[r], winv2, k2[r]) : ac[r] + k2[r]), 0.f);
            buf_store(syr, v, tcl[nt], roff(r));
        };

        f32x16 acc[2];
        u32x4 Bq[2][NP];
        STAMP(ts0);
        // ---------------- conv1 from the x image
        const unsigned short* xrow = Xb + (64 * nh + l31) * PITCH + 8 * half;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
#pragma unroll
        for (int p = 0; p < NP; ++p) Bq[0][p] = *reinterpret_cast<const u32x4*>(xrow + p * ROWS * PITCH);
        // column block 0; side work: fetch the next tile's x window (split during conv2)
#pragma unroll
        for (int s = 0; s < 12; ++s) {
            if (s < 4) kstep(W1, xrow, acc[0], Bq, 0, s, [&]() { load_combo(next, s); }, nop, nop, nop, nop, nop);
            else kstep(W1, xrow, acc[0], Bq, 0, s, nop, nop, nop, nop, nop, nop);
        }
        STAMP(ts1);
#pragma unroll
        for (int p = 0; p < NP; ++p) Bq[0][p] = *reinterpret_cast<const u32x4*>(xrow + (p * ROWS + 32) * PITCH);
        // column block 1; side work: epilogue 1 of block 0
#pragma unroll
        for (int s = 0; s < 12; ++s) {
            if (s < 8)
                kstep(W1, xrow, acc[1], Bq, 1, s, [&]() { e1_act(acc[0], 0, s); }, st1, st2, [&]() { e1_out(0, s); }, nop, nop);
            else kstep(W1, xrow, acc[1], Bq, 1, s, nop, nop, nop, nop, nop, nop);
        }
        // epilogue 1 of block 1 (serial)
        STAMP(ts2);
#pragma unroll
        for (int pi = 0; pi < 8; ++pi) { e1_act(acc[1], 1, pi); st1(); st2(); e1_out(1, pi); }
        STAMP(ts3);
        lds_barrier();          // a1 image complete; every wave is done with the x image
        STAMP(ts4);
        // ---------------- conv2 from the a1 image
        const unsigned short* arow = Ab + (64 * nh + l31) * PITCH + 8 * half;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
#pragma unroll
        for (int p = 0; p < NP; ++p) Bq[0][p] = *reinterpret_cast<const u32x4*>(arow + p * ROWS * PITCH);
        // column block 0; side work: first half of the next tile's x window, residual operand of block 0
#pragma unroll
        for (int s = 0; s < 12; ++s) {
            if (s < 8)
                kstep(W2, arow, acc[0], Bq, 0, s, [&]() { x_pick(s >> 2, s & 3); }, st1, st2, [&]() { x_out(s >> 2, s & 3); },
                      [&]() { e1_load(2 * s); }, [&]() { e1_load(2 * s + 1); });
            else kstep(W2, arow, acc[0], Bq, 0, s, nop, nop, nop, nop, nop, nop);
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) Bq[0][p] = *reinterpret_cast<const u32x4*>(arow + (p * ROWS + 32) * PITCH);
        // column block 1; side work: second half of the window, residual operand of block 1, epilogue 2 of block 0
#pragma unroll
        for (int s = 0; s < 12; ++s) {
            if (s < 4)
                kstep(W2, arow, acc[1], Bq, 1, s, [&]() { x_pick(2 + (s >> 2), s & 3); }, st1, st2, [&]() { x_out(2 + (s >> 2), s & 3); },
                      [&]() { e1_load(16 + 4 * s); e1_load(17 + 4 * s); }, [&]() { e1_load(18 + 4 * s); e1_load(19 + 4 * s); });
            else if (s < 8)
                kstep(W2, arow, acc[1], Bq, 1, s, [&]() { x_pick(2 + (s >> 2), s & 3); }, st1, st2, [&]() { x_out(2 + (s >> 2), s & 3); },
                      [&]() { e2_value(acc[0], 0, 2 * (s - 4)); }, [&]() { e2_value(acc[0], 0, 2 * (s - 4) + 1); });
            else
                kstep(W2, arow, acc[1], Bq, 1, s, nop, nop, nop, nop,
                      [&]() { e2_value(acc[0], 0, 2 * (s - 4)); }, [&]() { e2_value(acc[0], 0, 2 * (s - 4) + 1); });
        }
        // epilogue 2 of block 1 (serial)
        STAMP(ts5);
#pragma unroll
        for (int r = 0; r < 16; ++r) e2_value(acc[1], 1, r);
        lds_barrier();          // next x image complete; a1 image free
        STAMP(ts6);
#ifdef WM_STAMP
        tm[0] += ts1 - ts0; tm[1] += ts2 - ts1; tm[2] += ts3 - ts2; tm[3] += ts4 - ts3; tm[4] += ts5 - ts4; tm[5] += ts6 - ts5;
#endif
        tile += tstep;
    }
#undef FENCE
#ifdef WM_STAMP
    if (g_wm_stamp && lane == 0) {
        unsigned long long* d = g_wm_stamp + ((size_t)blockIdx.x * 4 + wave) * 6;
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = tm[i];
    }
#endif
}

template <bool H>
static int launch_resblock_eval(const RbeArgs& a, hipStream_t stream) {
    constexpr size_t lds = (size_t)(2 * (H ? 2 : 3) * 130 * 72) * 2 + 2 * 64 * sizeof(float);
    static wm::DevOnce attr_done;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(resblock_eval_kernel<H>), lds, attr_done)) return rc;
    const int ntiles = a.B * ((a.T + 2 + 123) / 124);
    const int grid = ntiles < kNumCU ? ntiles : kNumCU;
    hipLaunchKernelGGL(resblock_eval_kernel<H>, dim3(grid), dim3(256), lds, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}
}  // namespace

extern "C" {
WM_STAMP_SETTER(wm_debug_set_stamp_buffer_eval)
// inference ResBlock in one launch (both BatchNorms folded): see resblock_eval_kernel
int wm_resblock_eval_bf(const float* x, const void* w1pb, const void* w2pb, const float* b1, const float* sc1, const float* sh1,
                        const float* b2, const float* sc2, const float* sh2, float* y, int B, int T, int arith, hipStream_t stream) {
    if (B <= 0 || T <= 0 || (T & 3) || (arith != 0 && arith != 1)) return (int)hipErrorInvalidValue;
    if (!x || !w1pb || !w2pb || !sc1 || !sh1 || !sc2 || !sh2 || !y) return (int)hipErrorInvalidValue;
    RbeArgs a{x, w1pb, w2pb, b1, sc1, sh1, b2, sc2, sh2, y, B, T};
    return arith == 1 ? launch_resblock_eval<true>(a, stream) : launch_resblock_eval<false>(a, stream);
}
}  // extern "C"
