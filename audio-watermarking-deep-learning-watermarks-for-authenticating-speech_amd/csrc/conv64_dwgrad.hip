// conv64.hpp's fused family: data gradient and weight gradient of a k3 convolution in one launch
#include "conv64.hpp"

namespace {
// ---------------------------------------------------------------------------------------------
// Data gradient AND weight gradient of a k3 convolution in ONE launch (ResBlock backward, py/main16.py:112-125 under
// autograd).  Both read the same gradient frames (dz, and y for the BatchNorm-backward rebuild g = A dz + B + C y): as two
// launches the pair moves 7 frames, fused 4 (conv2: dz2 y2 y1 in, dz1 out) or 5 (conv1: dz1 y1 x dz2 in, dx out).
// A workgroup walks 64-step tiles.  The staging thread holds two channels x four steps of the gradient, rebuilds g once and
// splits it once: time pairs of bf16 pieces go into the [channel][time] image of the weight gradient (phase A); the
// [time][channel] image of the data gradient takes channel pairs, which are the same pieces re-paired by v_perm (phase B).
// The data gradient is accumulated transposed (rows = time, columns = channel), so that a lane's accumulator quads are four
// consecutive steps of one channel: epilogue operand and result move as dwordx4.  Per tile and wave:
//   phase A: 72 MFMAs of the data gradient (weight fragments of its 32 output rows resident in registers, as conv64bf3)
//            out of image D(i); side work: tile i+1 -> images G'(i+1), X'(i+1) (double-buffered), the epilogue operand of tile i
//   barrier
//   phase B: 72 MFMAs of the weight gradient (one 32 x 32 block of each tap per wave, as wgrad64bf_small) out of G'(i), X'(i);
//            side work: tile i+1 -> image D (single-buffered), epilogue of the data gradient of tile i, refill for tile i+2
//   barrier
// One slice of side work pinned behind every MFMA.  LDS: 28 + 2 x 27 + 2 x 33 KB.  T % 64 == 0.
// ---------------------------------------------------------------------------------------------
struct DWArgs {
    const float* g;  const float* g2;                   // gradient dz and the BN input y [B,64,T]
    const float* ga; const float* gb; const float* gc;  // g = ga[c] dz + gb[c] (+ gb[64+c]) + gc[c] y
    const void* wp;                                     // data-gradient weight image (wm_pack_w64_bf mode 1)
    const float* x;  const float* xa; const float* xb;  // weight-gradient input operand (+ BN+ReLU constants when XPRO = BNRELU)
    const float* e1; const float* ea; const float* eb;  // data-gradient epilogue tensor (RELUMASK: pre-BN activation + its scale/shift; ADD: addend)
    float* y;                                           // data gradient out [B,64,T]
    float* stats;                                       // [grid][2][64] (RELUMASK) or null
    float* partial;                                     // weight-gradient slabs [grid][3*4096 + 64]
    int B, T;
    const unsigned* gmask;                              // GM: sign bits of the ReLU the incoming gradient passes (bit t % 32 of dword
                                                        // [row][t / 32]): applied to g (conv2 pair) / to e1 (conv1 pair) on load
    const unsigned* pmask; const float* py2;            // EPI_ADDSTATS: sign bits / pre-BatchNorm activation y2 of the block BEFORE this
                                                        // one: y = (data gradient + e1) masked, stats = (sum y, sum y py2)
    const float* gscale;                                // H (f16 two-piece split): {gs, 1 / gs}, the power-of-two scale of the rebuilt
                                                        // gradient (wm_bn_bwd_finalize); the weight image carries its own scale
    float* dzmax;                                       // H, epi 1 / 2 / 8: max |y| per workgroup [grid] (sizes the NEXT launch's scale)
    const float* g1; const float* hw;                   // R1: the rank-one frame w[c] g1[b][t] that stands in for g (conv2 pair) / e1 (conv1 pair)
    const float* ss; const float* sw; const float* sb;  // XS: the clips [B,1,T] and the stem's w [64][7], bias [64] whose output stands in for x
};

// H = false: bf16 three-piece split, six piece products per product (bf16x6).  H = true: f16 TWO-piece split (hi = RNE_f16(x s),
// lo = RNE_f16(x s - hi): 22 bits), three products hi hi + hi lo + lo hi on v_mfma_f32_32x32x16_f16 -- half the matrix work, two
// thirds of the split / LDS work.  The f16 range is met by power-of-two scales: the weights' (chosen by the pack kernel from
// max |w|, stored behind the image), the gradient's (gs from wm_bn_bwd_finalize: max |A| max |dz| -> 2^9, applied through the
// BatchNorm-backward constants, i.e. for free; the rebuilt value is clamped to +-6e4 so that a pathological element saturates
// instead of becoming an infinity); activations need none.  Results are unscaled in the epilogue / at the slab write.
// R1 (GM, H; the block in front of the Conv1d(64, 1, 1) head): the gradient that reaches the block output is the rank-one frame
// hw[c] g1[b][t] (head1_bwd_kernel's dx).  It is not read from memory but formed from the clip's row g1 [B][T] and the 64 weights with
// that kernel's one multiply, in front of the mask AND: as the gradient operand g (conv2 pair: one dwordx4 of g1 per unit instead of
// one per channel and unit) / as the epilogue addend e1 (conv1 pair: one dwordx4 of g1 per lane instead of four row fetches).
// XPRO = PRO_STEM (XS; the first block behind a stem: conv1 pair, no mask, H): the weight-gradient operand x is the stem's output Conv1d(1, 64, 7,
// padding = 3)(s).  It is not read from memory but formed from the clip's samples and the stem's parameters with stem_fwd_kernel's
// fmaf chain (small_convs.hip): per unit the ten samples around its time quad (three loads) instead of two frame quads, per halo
// column two.  Buffer loads over the clip: a quad outside [0, T) reads zero, the stem's padding.  One seven-FMA chain per slice.
template <int EPI, int XPRO, bool GM, bool H, bool R1 = false>
__global__ __launch_bounds__(256) void dwgrad64bf_kernel(DWArgs a) {
    constexpr bool XS = (XPRO == PRO_STEM);
    static_assert((EPI == EPI_RELUMASK && XPRO == PRO_BNRELU) || ((EPI == EPI_ADD || EPI == EPI_ADDSTATS) && XPRO == PRO_NONE) ||
                  (EPI == EPI_ADD && XS && !GM && H && !R1), "conv2 pair, conv1 pair, or the plain f16 conv1 pair behind a stem");
    static_assert(!R1 || (GM && H && (EPI == EPI_RELUMASK || EPI == EPI_ADD)), "rank-one gradient: masked on load, f16 build");
    constexpr bool R1G = R1 && EPI == EPI_RELUMASK, R1E = R1 && EPI == EPI_ADD;     // ... as g / as e1
    constexpr int NCS = R1 ? 9 : 8;                        // rows of Cs: R1 adds the head's weights
    constexpr int KW = 3, NT = 64, NP = H ? 2 : 3, ROWS = NT + 2, PITCH = 72, PG = 72, PX = 88, XO = 8;
    constexpr int NPR = H ? 3 : 6, SPM = 6 / NPR;          // piece products per product; side-work slices per MFMA
    constexpr bool STATS = (EPI == EPI_RELUMASK || EPI == EPI_ADDSTATS);
    constexpr bool FOLD = (EPI == EPI_ADDSTATS);          // conv1 pair that also does the previous block's ReLU backward + BN sums
    constexpr int DIMG = NP * ROWS * PITCH, GIMG = NP * 64 * PG, XIMG = NP * 64 * PX;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    unsigned short* Db = reinterpret_cast<unsigned short*>(smem_raw);          // [NP][ROWS][PITCH]   row r = time t0 - 1 + r
    unsigned short* Gb0 = Db + DIMG;                                           // [2][NP][64][PG]
    unsigned short* Xb0 = Gb0 + 2 * GIMG;                                      // [2][NP][64][PX]     element XO + (t - t0)
    float* Cs = reinterpret_cast<float*>(Xb0 + 2 * XIMG);                      // [NCS][64]
    // H: a wave-private [32 channels][32 steps (+4)] exchange tile.  In the accumulator layout a lane owns one channel, so a dwordx4
    // access touches 32 rows with 16 bytes each; such a store (load) holds the wave at issue for ~300 cycles (measured: the four
    // epilogue stores were 1 200 of a tile's 7 000 cycles).  Epilogue operands and results therefore cross HBM in ROW layout (a lane
    // = 4 steps, 8 lanes = one 128-byte row segment, 8 rows per instruction) and change layout through this tile.
    constexpr bool XL = H;
    constexpr int EXP = 36;
    float* Ex = Cs + NCS * 64 + (threadIdx.x >> 6) * (32 * EXP);
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mt = wave & 1, nh = wave >> 1;           // data gradient: 32 output rows x 32 columns; weight gradient: block (mt, nt = nh)
    const int T = a.T;
    const int tilesPerClip = T / NT, ntiles = a.B * tilesPerClip;

    // ---- resident data-gradient weight fragments
    u32x4 Wr[12][NP];
    // H: {ws, 1 / ws} behind the [NP][KW][64][64] image
    const float winv = H ? reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(a.wp) + NP * KW * 4096)[1] : 1.f;
    const float gs = H ? a.gscale[0] : 1.f, ginv = H ? a.gscale[1] : 1.f;
    const float dinv = ginv * winv;                        // data gradient: (g gs) (w ws) -> g w
    {
        const uint4* wg = reinterpret_cast<const uint4*>(a.wp);
#pragma unroll
        for (int s = 0; s < 12; ++s)
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int e = ((p * KW + (s >> 2)) * 64 + 32 * mt + l31) * 64 + 16 * (s & 3) + 8 * half;
                u32x4 w_ = __builtin_bit_cast(u32x4, wg[e >> 3]);
                // pinned to the AGPR half of the register file: the MFMA reads its A operand from there directly.  Left to the
                // allocator the fragments are SPILLED to AGPRs and copied back (v_accvgpr_read) in front of every k-step.
                asm volatile("" : "+a"(w_));
                Wr[s][p] = w_;
            }
    }
    // ---- staging map: channel pair cp (channels c0, c0 + 1), unit u = time quad q0 + 8 u; halo: channel hc, side hh
    const int cp = wave * 8 + (lane & 7), c0 = 2 * cp, q0 = lane >> 3;
    const int hc = (tid & 127) >> 1, hh = tid & 1;
    float4 ra_[2], rb_[2], ya_[2], yb_[2], xa_[2], xb_[2];     // raw, per unit: dz / y of channel c0 (a) and c0 + 1 (b); x of both
    float4 gz_;                                                // the rebuilt gradient of the (unit, channel) being split
    unsigned gp_[2][2][6];                                     // its bf16 pieces [unit][channel][piece * 2 + time pair] (phase A -> phase B)
    float hg = 0.f, hy = 0.f, hxv = 0.f;
    // XS: the samples s[tq - 3 .. tq + 6] of a unit (three loads; what no tap reads is not loaded: a register that is loaded and never
    // read is handed out again at once, and the write to it then waits for the load) / s[hq .. hq + 7] of the halo column
    f32x3 sxl_[XS ? 2 : 1], sxr_[XS ? 2 : 1];
    f32x4 sxm_[XS ? 2 : 1], hxq_[2];
    unsigned voffs = 0, voffs0 = 0, hoffs0 = 0, hoffs1 = 0;
    wm_srd_t dsg = make_srd(a.g, 0), dsy = dsg, dsx = dsg, dsm = dsg;
    unsigned voff = 0, hoff = 0;
    unsigned voffr = 0, hoffr = 0;                       // R1G: the same places in the clip's row of g1
    bool okh = true;
    constexpr bool GMG = GM && EPI == EPI_RELUMASK;      // the mask belongs to the gradient operand g (else, with GM, to e1)
    unsigned mk_[2][2] = {{0u, 0u}, {0u, 0u}}, hmk = 0u; // mask dwords of (unit, channel) / of the halo step, as loaded
    unsigned voffm = 0, hoffm = 0, hsh = 0, hsh_cur = 0;
    const unsigned nwm = (unsigned)T >> 5;               // mask dwords per row (T % 64 == 0)
    auto set_tile = [&](int tile) {
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        const size_t clip = (size_t)b * 64 * T, bytes = (size_t)64 * T * sizeof(float);
        dsg = R1G ? make_srd(a.g1 + (size_t)b * T, (size_t)T * sizeof(float)) : make_srd(a.g + clip, bytes);
        dsy = make_srd(a.g2 + clip, bytes);
        if (XS) dsx = make_srd(a.ss + (size_t)b * T, (size_t)T * sizeof(float));
        else dsx = make_srd(a.x + clip, bytes);
        voff = (unsigned)(c0 * T + t0 + 4 * q0) * 4u;
        const int th = hh ? t0 + NT : t0 - 1;
        if (XS) {               // (the quad in front of the clip takes an offset past every clip instead of a negative one)
            const int tq = t0 + 4 * q0, hq = hh ? t0 + NT - 4 : t0 - 4;      // column t0 - 1: s[t0 - 4 .. t0 + 2]; column t0 + NT: s[t0 + NT - 3 .. t0 + NT + 3]
            voffs = (unsigned)tq * 4u;
            voffs0 = tq >= 4 ? voffs - 12u : 0xFFFFFF00u;
            hoffs0 = hq >= 0 ? (unsigned)hq * 4u : 0xFFFFFF00u;
            hoffs1 = (unsigned)(hq + 4) * 4u;
        }
        hoff = (unsigned)(hc * T + min(max(th, 0), T - 1)) * 4u;
        okh = th >= 0 && th < T;
        if (R1G) {
            voffr = (unsigned)(t0 + 4 * q0) * 4u;
            hoffr = (unsigned)min(max(th, 0), T - 1) * 4u;
        }
        if (GMG) {
            dsm = make_srd(reinterpret_cast<const float*>(a.gmask) + (size_t)b * 64 * nwm, (size_t)64 * nwm * sizeof(unsigned));
            voffm = ((unsigned)c0 * nwm + ((unsigned)t0 >> 5)) * 4u;
            const int thc = min(max(th, 0), T - 1);
            hoffm = ((unsigned)hc * nwm + ((unsigned)thc >> 5)) * 4u;
            hsh = (unsigned)thc & 31u;
        }
    };
    const unsigned rowT = (unsigned)T * 4u;
    auto load_g = [&](int u) {
        if (R1G) ra_[u] = __builtin_bit_cast(float4, buf_load4(dsg, voffr + 128u * u, 0u));     // both channels' g1 quad; rb_ unused
        else {
            ra_[u] = __builtin_bit_cast(float4, buf_load4(dsg, voff + 128u * u, 0u));
            rb_[u] = __builtin_bit_cast(float4, buf_load4(dsg, voff + 128u * u, rowT));
        }
        ya_[u] = __builtin_bit_cast(float4, buf_load4(dsy, voff + 128u * u, 0u));
        yb_[u] = __builtin_bit_cast(float4, buf_load4(dsy, voff + 128u * u, rowT));
    };
    auto load_xs = [&](int u, int k) {              // XS: quad k of unit u (unit 1 sits 32 steps behind unit 0: its first quad is inside)
        if (k == 0) sxl_[XS ? u : 0] = buf_load3(dsx, u ? voffs + 116u : voffs0, 0u);
        if (k == 1) sxm_[XS ? u : 0] = buf_load4(dsx, voffs + 128u * u, 0u);
        if (k == 2) sxr_[XS ? u : 0] = buf_load3(dsx, voffs + 128u * u + 16u, 0u);
    };
    auto load_x = [&](int u) {
        if (XS) { load_xs(u, 0); load_xs(u, 1); load_xs(u, 2); return; }
        xa_[u] = __builtin_bit_cast(float4, buf_load4(dsx, voff + 128u * u, 0u));
        xb_[u] = __builtin_bit_cast(float4, buf_load4(dsx, voff + 128u * u, rowT));
    };
    // The refills of the raw staging registers are dealt ONE load at a time over both phases (a register set is free from the slice
    // that consumed it until the same slice of the next tile): a burst of four 1-KB loads from one wave stalls that wave at issue
    // whenever the CU's miss queue is full, a different wave every tile -- measured as 430 of 8 250 cycles per tile spent at the
    // phase-A barrier waiting for whichever wave was hit.
    auto refillA = [&](int m) {                     // phase-A slice m
        // (R1G: ra_[u] serves both channels of unit u -- last read by slice 12 / 30 -- and the rb_ slots stay empty)
        if (m == 14) ra_[0] = __builtin_bit_cast(float4, R1G ? buf_load4(dsg, voffr, 0u) : buf_load4(dsg, voff, 0u));
        if (m == 20 && !R1G) rb_[0] = __builtin_bit_cast(float4, buf_load4(dsg, voff, rowT));
        if (m == 26) ya_[0] = __builtin_bit_cast(float4, buf_load4(dsy, voff, 0u));
        if (m == 32) yb_[0] = __builtin_bit_cast(float4, buf_load4(dsy, voff, rowT));
        if (m == 38) ra_[1] = __builtin_bit_cast(float4, R1G ? buf_load4(dsg, voffr + 128u, 0u) : buf_load4(dsg, voff + 128u, 0u));
        if (m == 44 && !R1G) rb_[1] = __builtin_bit_cast(float4, buf_load4(dsg, voff + 128u, rowT));
        if (m == 50) ya_[1] = __builtin_bit_cast(float4, buf_load4(dsy, voff + 128u, 0u));
        if (m == 56) yb_[1] = __builtin_bit_cast(float4, buf_load4(dsy, voff + 128u, rowT));
        if (GMG) {
            if (m == 16) mk_[0][0] = __builtin_bit_cast(unsigned, buf_load(dsm, voffm, 0u));
            if (m == 22) mk_[0][1] = __builtin_bit_cast(unsigned, buf_load(dsm, voffm, nwm * 4u));
            if (m == 40) mk_[1][0] = __builtin_bit_cast(unsigned, buf_load(dsm, voffm + 4u, 0u));
            if (m == 46) mk_[1][1] = __builtin_bit_cast(unsigned, buf_load(dsm, voffm + 4u, nwm * 4u));
        }
    };
    auto refillB = [&](int v) {                     // phase-B free slice v
        if (XS) { if ((v & 3) == 1) load_xs(v / 12, (v % 12) >> 2); return; }      // v = 1, 5, 9 | 13, 17, 21
        if (v == 1) xa_[0] = __builtin_bit_cast(float4, buf_load4(dsx, voff, 0u));
        if (v == 7) xb_[0] = __builtin_bit_cast(float4, buf_load4(dsx, voff, rowT));
        if (v == 13) xa_[1] = __builtin_bit_cast(float4, buf_load4(dsx, voff + 128u, 0u));
        if (v == 19) xb_[1] = __builtin_bit_cast(float4, buf_load4(dsx, voff + 128u, rowT));
    };
    auto load_ghalo = [&]() {
        hg = buf_load(dsg, R1G ? hoffr : hoff, 0u); hy = buf_load(dsy, hoff, 0u);
        if (GMG) hmk = __builtin_bit_cast(unsigned, buf_load(dsm, hoffm, 0u));
    };
    auto load_gmask = [&](int u) {
        mk_[u][0] = __builtin_bit_cast(unsigned, buf_load(dsm, voffm + 4u * u, 0u));
        mk_[u][1] = __builtin_bit_cast(unsigned, buf_load(dsm, voffm + 4u * u, nwm * 4u));
    };
    auto load_xhalo = [&]() {
        if (XS) { hxq_[0] = buf_load4(dsx, hoffs0, 0u); hxq_[1] = buf_load4(dsx, hoffs1, 0u); return; }
        hxv = buf_load(dsx, hoff, 0u);
    };

    const int tstep = gridDim.x;
    int tile = WM_XCD_MAP ? xcd_slot() : (int)blockIdx.x;          // grid <= ntiles
    set_tile(tile);
    bool okh_cur = okh;
    load_g(0); load_g(1); load_x(0); load_x(1); load_ghalo(); load_xhalo();
    if (GMG) { load_gmask(0); load_gmask(1); }
    hsh_cur = hsh;
    if (tid < 64) {
        Cs[tid] = a.ga[tid];
        Cs[64 + tid] = a.gb[tid];
        Cs[128 + tid] = a.gc[tid];
        Cs[192 + tid] = a.gb[64 + tid];                  // low word of the BatchNorm-backward offset
        Cs[256 + tid] = (XPRO == PRO_BNRELU) ? a.xa[tid] : 0.f;
        Cs[320 + tid] = (XPRO == PRO_BNRELU) ? a.xb[tid] : 0.f;
        Cs[384 + tid] = (EPI == EPI_RELUMASK) ? a.ea[tid] : 0.f;
        Cs[448 + tid] = (EPI == EPI_RELUMASK) ? a.eb[tid] : 0.f;
        if (R1) Cs[512 + tid] = a.hw[tid];
    }
    // the element right of the right halo only feeds bits that the funnel shift drops: keep it defined in both images
    for (int i = tid; i < 2 * NP * 64; i += 256) Xb0[(i / (NP * 64)) * XIMG + (i % (NP * 64)) * PX + XO + NT + 1] = 0;
    __syncthreads();
    // per-thread constants (the staging channels never change)
    float kga[2], kgb[2], kgc[2], kgl[2], kxa[2], kxb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        kga[j] = Cs[c0 + j] * gs; kgb[j] = Cs[64 + c0 + j] * gs; kgc[j] = Cs[128 + c0 + j] * gs; kgl[j] = Cs[192 + c0 + j] * gs;   // gs = 1 | 2^k: exact
        kxa[j] = Cs[256 + c0 + j]; kxb[j] = Cs[320 + c0 + j];
    }
    // R1G: the head's weights of the staging channels / of the halo channel
    const float kw[2] = {R1G ? Cs[512 + c0] : 0.f, R1G ? Cs[512 + c0 + 1] : 0.f}, khw = R1G ? Cs[512 + hc] : 0.f;
    // XS: the seven taps and the bias of the two staging channels and of the halo channel
    float ksw[2][XS ? 7 : 1], ksh[XS ? 7 : 1], ksb[2] = {0.f, 0.f}, ksbh = 0.f;
    if (XS) {
#pragma unroll
        for (int j = 0; j < 7; ++j) { ksw[0][XS ? j : 0] = a.sw[c0 * 7 + j]; ksw[1][XS ? j : 0] = a.sw[(c0 + 1) * 7 + j]; ksh[XS ? j : 0] = a.sw[hc * 7 + j]; }
        ksb[0] = a.sb[c0]; ksb[1] = a.sb[c0 + 1]; ksbh = a.sb[hc];
    }
    const float hga = Cs[hc] * gs, hgb = Cs[64 + hc] * gs, hgc = Cs[128 + hc] * gs, hgl = Cs[192 + hc] * gs, hxa = Cs[256 + hc], hxb = Cs[320 + hc];

    // ---- split stages on a value pair (va, vb) -> pieces (p0, p1, [lo]) and a second pair (vc, vd) -> (q0_, q1_, [lo])
    float va = 0.f, vb = 0.f, vc = 0.f, vd = 0.f;
    unsigned p0 = 0, p1 = 0, r0 = 0, r1 = 0;
    float bsum[2] = {0.f, 0.f};
    float bflag = 1.f;
    auto s1a = [&]() {
        if (H) {
            const h16x2 h_ = __builtin_convertvector(f32x2{va, vb}, h16x2);
            p0 = __builtin_bit_cast(unsigned, h_);
            va -= (float)h_.x; vb -= (float)h_.y;
        } else {
            const bf16x2 h_ = {(__bf16)va, (__bf16)vb};
            p0 = __builtin_bit_cast(unsigned, h_);
            va -= __uint_as_float(p0 << 16); vb -= __uint_as_float(p0 & 0xffff0000u);
        }
        asm volatile("" : "+v"(va), "+v"(vb), "+v"(p0));
    };
    auto s2a = [&]() {
        if (H) return;                                   // two pieces: no middle one
        const bf16x2 m_ = {(__bf16)va, (__bf16)vb};
        p1 = __builtin_bit_cast(unsigned, m_);
        va -= __uint_as_float(p1 << 16); vb -= __uint_as_float(p1 & 0xffff0000u);
        asm volatile("" : "+v"(va), "+v"(vb), "+v"(p1));
    };
    auto s1b = [&]() {
        if (H) {
            const h16x2 h_ = __builtin_convertvector(f32x2{vc, vd}, h16x2);
            r0 = __builtin_bit_cast(unsigned, h_);
            vc -= (float)h_.x; vd -= (float)h_.y;
        } else {
            const bf16x2 h_ = {(__bf16)vc, (__bf16)vd};
            r0 = __builtin_bit_cast(unsigned, h_);
            vc -= __uint_as_float(r0 << 16); vd -= __uint_as_float(r0 & 0xffff0000u);
        }
        asm volatile("" : "+v"(vc), "+v"(vd), "+v"(r0));
    };
    auto s2b = [&]() {
        if (H) return;
        const bf16x2 m_ = {(__bf16)vc, (__bf16)vd};
        r1 = __builtin_bit_cast(unsigned, m_);
        vc -= __uint_as_float(r1 << 16); vd -= __uint_as_float(r1 & 0xffff0000u);
        asm volatile("" : "+v"(vc), "+v"(vd), "+v"(r1));
    };
    unsigned l0 = 0, l1 = 0;
    auto lo_pair = [&](float x0, float x1) -> unsigned {         // the last piece of a value pair
        if (H) return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x0, x1}, h16x2));
        const bf16x2 l_ = {(__bf16)x0, (__bf16)x1};
        return __builtin_bit_cast(unsigned, l_);
    };
    auto out4 = [&](unsigned short* dst, int stride_p) {         // two time pairs of one channel row: 8-byte writes
        l0 = lo_pair(va, vb); l1 = lo_pair(vc, vd);
        *reinterpret_cast<uint2*>(dst) = make_uint2(p0, r0);
        if (!H) *reinterpret_cast<uint2*>(dst + stride_p) = make_uint2(p1, r1);
        *reinterpret_cast<uint2*>(dst + (NP - 1) * stride_p) = make_uint2(l0, l1);
    };
    // gradient rebuild of channel j of unit u from the raw staging registers (free for the refill afterwards): one value per slice
    // (a slice must stay within the shadow of one MFMA, about seven instructions: a twelve-instruction slice costs its excess in full)
    auto g_build = [&](int u, int j, int e) {
        const float4 dz = (j && !R1G) ? rb_[u] : ra_[u], yy = j ? yb_[u] : ya_[u];
        float4& gz = gz_;
        float d = (e == 0) ? dz.x : (e == 1) ? dz.y : (e == 2) ? dz.z : dz.w;
        const float yv = (e == 0) ? yy.x : (e == 1) ? yy.y : (e == 2) ? yy.z : yy.w;
        if (R1G) d = __fmul_rn(kw[j], d);   // the frame element, rounded once as head1_bwd_kernel rounds it
        if (GMG) {                          // dz = g_out where the block output was positive: its bit, sign-extended, ANDed in
            if (e == 0) mk_[u][j] >>= 4 * q0;
            d = __uint_as_float(__float_as_uint(d) & (unsigned)__builtin_amdgcn_sbfe((int)mk_[u][j], e, 1));
        }
        float v = pro_apply<PRO_BNBWD>(d, yv, kga[j], kgb[j], kgc[j], kgl[j]);
        if (H) v = __builtin_amdgcn_fmed3f(v, -6.0e4f, 6.0e4f);      // a spike saturates; it never becomes an f16 infinity
        bsum[j] = fmaf(bflag, v, bsum[j]);
        asm volatile("" : "+v"(v), "+v"(bsum[j]));
        if (e == 0) gz.x = v; else if (e == 1) gz.y = v; else if (e == 2) gz.z = v; else gz.w = v;
    };
    auto g_pick_t = [&](int u, int j) {                         // time pairs of channel j of unit u
        const float4 gz = gz_;
        va = gz.x; vb = gz.y; vc = gz.z; vd = gz.w;
        asm volatile("" : "+v"(va), "+v"(vb), "+v"(vc), "+v"(vd));
    };
    auto x_pick_t = [&](int u, int j) {
        float4 xx = j ? xb_[u] : xa_[u];
        if (XPRO == PRO_BNRELU) {
            xx.x = pro_apply<PRO_BNRELU>(xx.x, 0.f, kxa[j], kxb[j], 0.f); xx.y = pro_apply<PRO_BNRELU>(xx.y, 0.f, kxa[j], kxb[j], 0.f);
            xx.z = pro_apply<PRO_BNRELU>(xx.z, 0.f, kxa[j], kxb[j], 0.f); xx.w = pro_apply<PRO_BNRELU>(xx.w, 0.f, kxa[j], kxb[j], 0.f);
        }
        va = xx.x; vb = xx.y; vc = xx.z; vd = xx.w;
        asm volatile("" : "+v"(va), "+v"(vb), "+v"(vc), "+v"(vd));
    };
    // XS: step e of channel j of unit u -- stem_fwd_kernel's chain to the letter: o = bias, then o = fmaf(w[k], s[t + k - 3], o), k = 0..6
    // (a tap outside the clip multiplies the zero that was loaded; nothing is skipped, nothing regrouped)
    auto xs_form = [&](int u, int j, int e) -> float {
        const f32x3 g0 = sxl_[XS ? u : 0], g2 = sxr_[XS ? u : 0];
        const f32x4 g1 = sxm_[XS ? u : 0];
        const float g[10] = {g0[0], g0[1], g0[2], g1[0], g1[1], g1[2], g1[3], g2[0], g2[1], g2[2]};       // s[tq - 3 .. tq + 6]
        float o = ksb[j];
#pragma unroll
        for (int k = 0; k < 7; ++k) o = fmaf(ksw[j][XS ? k : 0], g[e + k], o);
        asm volatile("" : "+v"(o));
        return o;
    };
    // image D wants channel pairs (c0, c0 + 1) at ONE time step; the pieces of a value do not depend on what it is paired with, so
    // they are taken from the time-pair dwords of the two channels with one v_perm each instead of splitting the gradient again
    auto d_out = [&](int u, int e) {
        const unsigned sel = (e & 1) ? 0x07060302u : 0x05040100u;   // high | low halves of (channel c0 + 1 : channel c0)
        const int pr = e >> 1;
        const unsigned d0 = __builtin_amdgcn_perm(gp_[u][1][pr], gp_[u][0][pr], sel);
        const unsigned d1 = __builtin_amdgcn_perm(gp_[u][1][2 + pr], gp_[u][0][2 + pr], sel);
        const unsigned d2 = __builtin_amdgcn_perm(gp_[u][1][4 + pr], gp_[u][0][4 + pr], sel);
        unsigned* D32 = reinterpret_cast<unsigned*>(Db);
        const int o = (1 + 4 * (q0 + 8 * u) + e) * (PITCH / 2) + cp;
        D32[o] = d0;
        if (!H) D32[(ROWS * PITCH >> 1) + o] = d1;
        D32[(NP - 1) * (ROWS * PITCH >> 1) + o] = d2;
    };
    // halos: the gradient's for image D (rows 0 and 65), the input operand's for image X' (elements XO - 1, XO + 64)
    auto hx_pick = [&]() {
        float v = hxv;
        if (XS) {
            const float g[8] = {hxq_[0][0], hxq_[0][1], hxq_[0][2], hxq_[0][3], hxq_[1][0], hxq_[1][1], hxq_[1][2], hxq_[1][3]};
            v = ksbh;
#pragma unroll
            for (int k = 0; k < 7; ++k) v = fmaf(ksh[XS ? k : 0], hh ? g[k + 1] : g[k], v);
        }
        if (XPRO == PRO_BNRELU) v = pro_apply<PRO_BNRELU>(v, 0.f, hxa, hxb, 0.f);
        va = okh_cur ? v : 0.f; vb = 0.f;
        asm volatile("" : "+v"(va), "+v"(vb));
    };
    auto hx_out = [&](unsigned short* X) {
        const unsigned la = lo_pair(va, vb);
        if (tid < 128) {
            const int o = hc * PX + (hh ? XO + NT : XO - 1);
            X[o] = (unsigned short)p0;
            if (!H) X[64 * PX + o] = (unsigned short)p1;
            X[(NP - 1) * 64 * PX + o] = (unsigned short)la;
        }
    };
    auto hg_pick = [&]() {
        float hgm = R1G ? __fmul_rn(khw, hg) : hg;
        if (GMG) hgm = __uint_as_float(__float_as_uint(hgm) & (unsigned)__builtin_amdgcn_sbfe((int)(hmk >> hsh_cur), 0, 1));
        float v = pro_apply<PRO_BNBWD>(hgm, hy, hga, hgb, hgc, hgl);
        if (H) v = __builtin_amdgcn_fmed3f(v, -6.0e4f, 6.0e4f);
        va = okh_cur ? v : 0.f; vb = 0.f;
        asm volatile("" : "+v"(va), "+v"(vb));
    };
    auto hg_out = [&]() {
        const unsigned la = lo_pair(va, vb);
        if (tid < 128) {
            const int o = (hh ? NT + 1 : 0) * PITCH + hc;
            Db[o] = (unsigned short)p0;
            if (!H) Db[ROWS * PITCH + o] = (unsigned short)p1;
            Db[(NP - 1) * ROWS * PITCH + o] = (unsigned short)la;
        }
    };
    // phase-A side work, slice v of 64 (the other 8 slices fetch the epilogue operand): the operands in the registers -> images G', X'
    //   v 0..35  gradient: per (unit, channel) 9 slices: rebuild x 4 | pick | hi a | mid a + hi b | mid b | lo + write
    //   v 36..59 input:    per (unit, channel) 6 slices: pick (+ BN + ReLU) | hi a | mid a | hi b | mid b | lo + write
    //   v 60..63 input halo
    // XS (all 72 slices of the phase; the f16 build fetches no epilogue operand here):
    //   v 36..67 input:    per (unit, channel) 8 slices: form a | form b | hi (a, b) | form c | form d | hi (c, d) | lo + write | -
    //   v 68..71 input halo
    constexpr int NSA = XS ? 72 : 64;
    auto sideA = [&](int v, unsigned short* G, unsigned short* X) __attribute__((always_inline)) {
        if (v < 36) {
            const int uj = v / 9, st = v % 9, u = uj >> 1, j = uj & 1;
            if (st < 4) g_build(u, j, st);
            if (st == 4) g_pick_t(u, j);
            if (st == 5) s1a();
            if (st == 6) { s2a(); s1b(); }
            if (st == 7) s2b();
            if (st == 8) {
                out4(G + (c0 + j) * PG + 4 * (q0 + 8 * u), 64 * PG);
                gp_[u][j][0] = p0; gp_[u][j][1] = r0; gp_[u][j][2] = p1; gp_[u][j][3] = r1; gp_[u][j][4] = l0; gp_[u][j][5] = l1;
            }
        } else if (XS && v < 68) {
            const int w = v - 36, uj = w / 8, st = w % 8, u = uj >> 1, j = uj & 1;
            if (st == 0) va = xs_form(u, j, 0);
            if (st == 1) vb = xs_form(u, j, 1);
            if (st == 2) s1a();
            if (st == 3) vc = xs_form(u, j, 2);
            if (st == 4) vd = xs_form(u, j, 3);
            if (st == 5) s1b();
            if (st == 6) out4(X + (c0 + j) * PX + XO + 4 * (q0 + 8 * u), 64 * PX);
        } else if (!XS && v < 60) {
            const int w = v - 36, uj = w / 6, st = w % 6, u = uj >> 1, j = uj & 1;
            if (st == 0) x_pick_t(u, j);
            if (st == 1) s1a();
            if (st == 2) s2a();
            if (st == 3) s1b();
            if (st == 4) s2b();
            if (st == 5) out4(X + (c0 + j) * PX + XO + 4 * (q0 + 8 * u), 64 * PX);
        } else {
            const int st = v - (XS ? 68 : 60);
            if (st == 0) { hx_pick(); load_xhalo(); }
            if (st == 1) s1a();
            if (st == 2) s2a();
            if (st == 3) hx_out(X);
        }
    };
    // phase-B side work, slice v of 12: the gradient's pieces -> image D (channel pairs by v_perm)
    //   v 0..7  one slice per (unit, time step): 3 perms + 3 writes;   v 8..11 gradient halo
    constexpr int NSB = 12;
    auto sideB = [&](int v) __attribute__((always_inline)) {
        if (v < 8) {
            d_out(v >> 2, v & 3);
        } else {
            const int st = v - 8;
            if (st == 0) { hg_pick(); load_ghalo(); }
            if (st == 1) s1a();
            if (st == 2) s2a();
            if (st == 3) hg_out();
        }
    };
    {   // first tile: all images serially; the refills inside the slices already fetch the second tile
        set_tile(min(tile + tstep, ntiles - 1));
        const bool okh_n = okh;
#pragma unroll
        for (int v = 0; v < NSA; ++v) { sideA(v, Gb0, Xb0); refillA(v); }
        const unsigned hsh_n = hsh;
#pragma unroll
        for (int v = 0; v < 2 * NSB; ++v) { if ((v & 1) == 0) sideB(v >> 1); else refillB(v); }
        okh_cur = okh_n; hsh_cur = hsh_n;
    }
    __syncthreads();

    f32x16 wacc[KW];
#pragma unroll
    for (int k = 0; k < KW; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) wacc[k][r] = 0.f;
    // The data gradient is accumulated TRANSPOSED (gradient image = A operand, weights = B operand): a lane then owns ONE output
    // channel (32 mt + l31) and, per accumulator quad, four consecutive time steps -- the epilogue operand comes in and the
    // result goes out as dwordx4 (8 memory instructions per tile instead of 32), the ReLU-mask constants and the two BatchNorm
    // sums are one register each instead of sixteen.
    float s1 = 0.f, s2 = 0.f;
    f32x4 e1q[4];
    // conv2 pair: the epilogue operand IS the input operand of the weight gradient (the pre-BatchNorm activation), read a second
    // time in the accumulator layout.  Fetched one tile AHEAD (e1n, for the next tile, while this one is in phase A) it follows
    // the staging loads of the same tile by less than one tile's worth of traffic and is served by the XCD's L2 instead of HBM
    // (fetched as late as the tile needs it, 32 % of the kernel's HBM traffic was this re-read).
    // (round 3, f16 build: with half the MFMAs per phase an operand fetched in phase A no longer has a phase's worth of time to arrive
    // before the epilogue in phase B needs it -- EVERY epilogue operand of every form is now fetched one tile ahead: e1, the mask words,
    // the previous block's y2)
    constexpr bool EAHEAD = true;
    f32x4 e1n[4];
    unsigned emk = 0u, pmk = 0u, emkn = 0u, pmkn = 0u;
    f32x4 pyq[FOLD ? 4 : 1], pyn[FOLD ? 4 : 1];
    f32x4 ec[(XL && !R1E) ? 4 : 1], pyc[(XL && FOLD) ? 4 : 1];     // row-layout staging of the next tile's epilogue operands (R1E: g1)
    const int xrow = lane >> 3, xcol = 4 * (lane & 7);       // row layout: lane -> (row xrow + 8 r, steps xcol .. xcol + 3)
    const unsigned xlane = (unsigned)(xrow * T + xcol) * 4u;
    unsigned row8T[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) row8T[r] = (unsigned)(8 * r * T) * 4u;
    const float kwa = R1E ? Cs[512 + 32 * mt + l31] : 0.f;     // the head's weight of the lane's accumulator channel
    const float kea = (EPI == EPI_RELUMASK) ? Cs[384 + 32 * mt + l31] : 0.f, keb = (EPI == EPI_RELUMASK) ? Cs[448 + 32 * mt + l31] : 0.f;
    int buf = 0;
#ifdef WM_STAMP
    unsigned long long tm[6] = {0, 0, 0, 0, 0, 0};
#endif
    {                                                    // the first tile's epilogue operands
        const int b0 = tile / tilesPerClip, t00 = (tile - b0 * tilesPerClip) * NT;
        const size_t slab0 = ((size_t)b0 * 64 + 32 * mt) * T;
        const unsigned eo0 = (unsigned)(l31 * T + t00 + 32 * nh + 4 * half) * 4u, mo0 = ((unsigned)l31 * nwm + ((unsigned)t00 >> 5) + (unsigned)nh) * 4u;
        const wm_srd_t s0 = R1E ? make_srd(a.g1 + (size_t)b0 * T, (size_t)T * sizeof(float)) : make_srd(a.e1 + slab0, (size_t)32 * T * sizeof(float));
        if (R1E) {                                       // the lane's channel times the clip's row, in the accumulator layout
            const unsigned go0 = (unsigned)(t00 + 32 * nh + 4 * half) * 4u;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const f32x4 gq = buf_load4(s0, go0 + 32u * q4, 0u);
                e1q[q4] = f32x4{__fmul_rn(kwa, gq[0]), __fmul_rn(kwa, gq[1]), __fmul_rn(kwa, gq[2]), __fmul_rn(kwa, gq[3])};
            }
        } else {
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) e1q[q4] = buf_load4(s0, eo0 + 32u * q4, 0u);
        }
        if (GM && (EPI == EPI_ADD || EPI == EPI_ADDSTATS))
            emk = __builtin_bit_cast(unsigned, buf_load(make_srd(reinterpret_cast<const float*>(a.gmask) + ((size_t)b0 * 64 + 32 * mt) * nwm,
                                                                 (size_t)32 * nwm * sizeof(unsigned)), mo0, 0u));
        if (FOLD) {
            pmk = __builtin_bit_cast(unsigned, buf_load(make_srd(reinterpret_cast<const float*>(a.pmask) + ((size_t)b0 * 64 + 32 * mt) * nwm,
                                                                 (size_t)32 * nwm * sizeof(unsigned)), mo0, 0u));
            const wm_srd_t sp0 = make_srd(a.py2 + slab0, (size_t)32 * T * sizeof(float));
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) pyq[q4] = buf_load4(sp0, eo0 + 32u * q4, 0u);
        }
    }
#define FENCE __builtin_amdgcn_sched_barrier(0)
    // one piece product on raw 128-bit fragments; the j-th product of a k-step pairs piece PA(j) of the first operand with piece PB(j)
    // of the second, small terms first (bf16x6: mid mid, hi lo, lo hi, hi mid, mid hi, hi hi; f16: lo hi, hi lo, hi hi)
    auto mma = [&](const u32x4& A_, const u32x4& B_, f32x16 c) -> f32x16 {
        if (H) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, A_), __builtin_bit_cast(h16x8, B_), c, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A_), __builtin_bit_cast(bf16x8, B_), c, 0, 0, 0);
    };
    auto PA = [](int j) { return H ? (j == 0 ? 1 : 0) : ((j == 0 || j == 4) ? 1 : (j == 2 ? 2 : 0)); };
    auto PB = [](int j) { return H ? (j == 1 ? 1 : 0) : ((j == 0 || j == 3) ? 1 : (j == 1 ? 2 : 0)); };
    float vmax = 0.f;                                    // H: running max |y| of the data-gradient values this lane stores
    while (tile < ntiles) {
        // registers: the raw operands of tile + tstep (clamped: the duplicate of the last tile is split but never used)
        const int b = tile / tilesPerClip, t0 = (tile - b * tilesPerClip) * NT;
        bflag = (tile + tstep < ntiles) ? 1.f : 0.f;
        set_tile(min(tile + 2 * tstep, ntiles - 1));       // what the refills inside the slices fetch
        const bool okh_n = okh;
        const unsigned hsh_n = hsh;
        const unsigned short* Gc = Gb0 + buf * GIMG;
        const unsigned short* Xc = Xb0 + buf * XIMG;
        unsigned short* Gn = Gb0 + (buf ^ 1) * GIMG;
        unsigned short* Xn = Xb0 + (buf ^ 1) * XIMG;
        // data-gradient output / epilogue operand of this lane: channel 32 mt + l31, steps t0 + 32 nh + 8 q + 4 half + (0..3) for quad q
        const size_t slab = ((size_t)b * 64 + 32 * mt) * T;
        const wm_srd_t sye = make_srd(a.y + slab, (size_t)32 * T * sizeof(float));
        const wm_srd_t se1 = R1E ? make_srd(a.g1 + (size_t)b * T, (size_t)T * sizeof(float)) : make_srd(a.e1 + slab, (size_t)32 * T * sizeof(float));
        const unsigned eoff = (unsigned)(l31 * T + t0 + 32 * nh + 4 * half) * 4u;
        const int tnx = min(tile + tstep, ntiles - 1), bnx = tnx / tilesPerClip, t0nx = (tnx - bnx * tilesPerClip) * NT;
        const wm_srd_t se1n = R1E ? make_srd(a.g1 + (size_t)bnx * T, (size_t)T * sizeof(float))
                                  : EAHEAD ? make_srd(a.e1 + ((size_t)bnx * 64 + 32 * mt) * T, (size_t)32 * T * sizeof(float)) : se1;
        const unsigned eoffn = (unsigned)(l31 * T + t0nx + 32 * nh + 4 * half) * 4u;
        // GM, conv1 pair: e1 is the gradient that reaches the block output; its ReLU bits: dword t0 / 32 + nh of the lane's row
        constexpr bool GME = GM && (EPI == EPI_ADD || EPI == EPI_ADDSTATS);
        const wm_srd_t spm = FOLD ? make_srd(reinterpret_cast<const float*>(a.pmask) + ((size_t)b * 64 + 32 * mt) * nwm,
                                             (size_t)32 * nwm * sizeof(unsigned)) : se1;
        const wm_srd_t spy = FOLD ? make_srd(a.py2 + slab, (size_t)32 * T * sizeof(float)) : se1;
        const wm_srd_t sme = GME ? make_srd(reinterpret_cast<const float*>(a.gmask) + ((size_t)b * 64 + 32 * mt) * nwm,
                                            (size_t)32 * nwm * sizeof(unsigned)) : se1;
        const size_t slabn = ((size_t)bnx * 64 + 32 * mt) * T;
        const wm_srd_t spmn = FOLD ? make_srd(reinterpret_cast<const float*>(a.pmask) + ((size_t)bnx * 64 + 32 * mt) * nwm,
                                              (size_t)32 * nwm * sizeof(unsigned)) : se1;
        const wm_srd_t spyn = FOLD ? make_srd(a.py2 + slabn, (size_t)32 * T * sizeof(float)) : se1;
        const wm_srd_t smen = GME ? make_srd(reinterpret_cast<const float*>(a.gmask) + ((size_t)bnx * 64 + 32 * mt) * nwm,
                                             (size_t)32 * nwm * sizeof(unsigned)) : se1;
        const unsigned emoffn = ((unsigned)l31 * nwm + ((unsigned)t0nx >> 5) + (unsigned)nh) * 4u;
        const unsigned goffn = (unsigned)(t0nx + 32 * nh + xcol) * 4u;        // R1E: the lane's four steps in the next tile's row of g1
        const unsigned xoffn = xlane + (unsigned)(t0nx + 32 * nh) * 4u, xoff = xlane + (unsigned)(t0 + 32 * nh) * 4u;

        STAMP(ts0);
        // ---------------- phase A: data gradient out of image D
        f32x16 dacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) dacc[r] = 0.f;
        {
            const unsigned short* drow = Db + (32 * nh + l31) * PITCH + 8 * half;
            u32x4 Bq[2][NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) Bq[0][p] = *reinterpret_cast<const u32x4*>(drow + p * ROWS * PITCH);
#pragma unroll
            for (int s = 0; s < 12; ++s) {
                if (s + 1 < 12) {
#pragma unroll
                    for (int p = 0; p < NP; ++p)
                        Bq[(s + 1) & 1][p] = *reinterpret_cast<const u32x4*>(drow + (p * ROWS + ((s + 1) >> 2)) * PITCH + 16 * ((s + 1) & 3));
                }
                const u32x4* Bf = Bq[s & 1];
                // the weight-gradient accumulators stay where they are across this phase: left alone, the allocator lends a[0:15] of
                // one of them to dacc and copies it out and back around every phase A (32 v_accvgpr moves per tile)
                if ((s & 3) == 1) asm volatile("" : "+a"(wacc[0]), "+a"(wacc[1]), "+a"(wacc[2]));
#pragma unroll
                for (int j = 0; j < NPR; ++j) {
                    FENCE;
                    dacc = mma(Bf[PB(j)], Wr[s][PA(j)], dacc);      // D^T: rows = time, columns = channel (gradient piece PB, weight piece PA)
                    FENCE;
                    // SPM slices of side work behind this MFMA (72 slices per phase whatever the arithmetic)
#pragma unroll
                    for (int i_ = 0; i_ < SPM; ++i_) {
                        const int m = (s * NPR + j) * SPM + i_;          // 0..71
                        if (R1E) { if (m == 1) ec[0] = buf_load4(se1n, goffn, 0u); }
                        else if (XL && m < 8 && (m & 1)) ec[m >> 1] = buf_load4(se1n, xoffn, row8T[m >> 1]);
                        if (XL && FOLD && m >= 8 && m < 16 && (m & 1)) pyc[(m - 8) >> 1] = buf_load4(spyn, xoffn, row8T[(m - 8) >> 1]);
                        if (m < NSA) {
                            sideA(m, Gn, Xn); refillA(m);
                            if (GME && m == 61) emkn = __builtin_bit_cast(unsigned, buf_load(smen, emoffn, 0u));
                            if (FOLD && m == 62) pmkn = __builtin_bit_cast(unsigned, buf_load(spmn, emoffn, 0u));
                        }
                        else if (XL) { }
                        else if (((m - NSA) & 1) == 0) e1n[(m - NSA) >> 1] = buf_load4(se1n, eoffn + 32u * ((m - NSA) >> 1), 0u);
                        else if (FOLD) pyn[(m - NSA) >> 1] = buf_load4(spyn, eoffn + 32u * ((m - NSA) >> 1), 0u);
                    }
                    FENCE;
                }
            }
        }
        STAMP(ts1);
#ifdef WM_STAMP
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        STAMP(ts1b);
        asm volatile("s_barrier" ::: "memory");
#else
        lds_barrier();          // every wave is done with image D; images G', X' of the next tile are complete
#endif
        STAMP(ts2);
        // ---------------- phase B: weight gradient out of images G', X'; image D of the next tile, epilogue of this one
        {
            const int e0 = 8 * half;
            u32x4 A[2][NP];
            uint4 f[2][NP];
            unsigned Lw[2][NP], Rw[2][NP];
            u32x4 Bl[NP], Br[NP];
            auto read_kb = [&](int kb, int set) {
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    A[set][p] = *reinterpret_cast<const u32x4*>(Gc + (p * 64 + mt * 32 + l31) * PG + kb * 16 + e0);
                    const unsigned short* xr = Xc + (p * 64 + nh * 32 + l31) * PX + XO + kb * 16 + e0;
                    f[set][p] = *reinterpret_cast<const uint4*>(xr);
                    Lw[set][p] = *reinterpret_cast<const unsigned*>(xr - 2);
                    Rw[set][p] = *reinterpret_cast<const unsigned*>(xr + 8);
                }
            };
            auto shl = [&](int set, int p) {
                const uint4 g = f[set][p];
                uint4 s_ = make_uint4(__builtin_amdgcn_alignbit(g.x, Lw[set][p], 16), __builtin_amdgcn_alignbit(g.y, g.x, 16),
                                      __builtin_amdgcn_alignbit(g.z, g.y, 16), __builtin_amdgcn_alignbit(g.w, g.z, 16));
                asm volatile("" : "+v"(s_.x), "+v"(s_.y), "+v"(s_.z), "+v"(s_.w));
                Bl[p] = __builtin_bit_cast(u32x4, s_);
            };
            auto shr = [&](int set, int p) {
                const uint4 g = f[set][p];
                uint4 s_ = make_uint4(__builtin_amdgcn_alignbit(g.y, g.x, 16), __builtin_amdgcn_alignbit(g.z, g.y, 16),
                                      __builtin_amdgcn_alignbit(g.w, g.z, 16), __builtin_amdgcn_alignbit(Rw[set][p], g.w, 16));
                asm volatile("" : "+v"(s_.x), "+v"(s_.y), "+v"(s_.z), "+v"(s_.w));
                Br[p] = __builtin_bit_cast(u32x4, s_);
            };
            // epilogue of accumulator registers 2 i, 2 i + 1 of the data gradient (two time steps of the lane's channel); every second
            // call completes a quad and stores it
            auto epi2 = [&](int i) {
                const int r0 = 2 * i, r1 = 2 * i + 1;
                float v0 = dacc[r0], v1 = dacc[r1];
                if (H) { v0 *= dinv; v1 *= dinv; }                // undo the gradient's and the weights' scales (a power of two: exact)
                const float q0_ = e1q[r0 >> 2][r0 & 3], q1_ = e1q[r1 >> 2][r1 & 3];
                if (EPI == EPI_RELUMASK) {
                    // both compares first, both selects after: a select right behind its compare costs two wait states
                    const bool k0 = fmaf(q0_, kea, keb) > 0.f, k1 = fmaf(q1_, kea, keb) > 0.f;
                    v0 = k0 ? v0 : 0.f; v1 = k1 ? v1 : 0.f;
                    s1 += v0; s2 = fmaf(v0, q0_, s2);
                    s1 += v1; s2 = fmaf(v1, q1_, s2);
                    asm volatile("" : "+v"(s1), "+v"(s2));
                } else if (GM) {
                    // bits 8 q + 4 half + e of the row's dword: shifted by 4 half once (first call), then constant field positions
                    if (i == 0) emk >>= 4 * half;
                    v0 += __uint_as_float(__float_as_uint(q0_) & (unsigned)__builtin_amdgcn_sbfe((int)emk, 8 * (r0 >> 2) + (r0 & 3), 1));
                    v1 += __uint_as_float(__float_as_uint(q1_) & (unsigned)__builtin_amdgcn_sbfe((int)emk, 8 * (r1 >> 2) + (r1 & 3), 1));
                } else {
                    v0 += q0_; v1 += q1_;
                }
                if (FOLD) {
                    // what leaves is dz2 of the PREVIOUS block: its output's ReLU mask on the gradient just formed, and the two sums its
                    // BatchNorm backward needs (sum dz2, sum dz2 y2) -- that block then has no reduction pass of its own
                    if (i == 0) pmk >>= 4 * half;
                    v0 = __uint_as_float(__float_as_uint(v0) & (unsigned)__builtin_amdgcn_sbfe((int)pmk, 8 * (r0 >> 2) + (r0 & 3), 1));
                    v1 = __uint_as_float(__float_as_uint(v1) & (unsigned)__builtin_amdgcn_sbfe((int)pmk, 8 * (r1 >> 2) + (r1 & 3), 1));
                    s1 += v0; s2 = fmaf(v0, pyq[r0 >> 2][r0 & 3], s2);
                    s1 += v1; s2 = fmaf(v1, pyq[r1 >> 2][r1 & 3], s2);
                    asm volatile("" : "+v"(s1), "+v"(s2));
                }
                dacc[r0] = v0; dacc[r1] = v1;
                if (H && (STATS || EPI == EPI_ADD)) vmax = fmaxf(vmax, fmaxf(fabsf(v0), fabsf(v1)));   // one v_max3 per pair
                if (i & 1) {
                    const int q4 = i >> 1;
                    const f32x4 quad = {dacc[4 * q4], dacc[4 * q4 + 1], dacc[4 * q4 + 2], dacc[4 * q4 + 3]};
                    if (XL) *reinterpret_cast<f32x4*>(Ex + l31 * EXP + 8 * q4 + 4 * half) = quad;
                    else buf_store4(sye, quad, eoff + 32u * q4, 0u);
                }
            };
            read_kb(0, 0);
            // the slice behind old-style MFMA index m (18 per k-block): shifts of the X fragments first, then 12 free slices per k-block
            // = 48: image D of the next tile in every second one of the first 24, the epilogue quads in the last 24
            auto sliceB = [&](int m) __attribute__((always_inline)) {
                const int kb = m / 18, mm = m % 18, set = kb & 1;
                if (mm < 3) { if (mm < NP) shl(set, mm); }
                else if (mm < 6) { if (mm - 3 < NP) shr(set, mm - 3); }
                else {
                    const int v = kb * 12 + (mm - 6);             // 0..47
                    if (v < 2 * NSB) {
                        if ((v & 1) == 0) sideB(v >> 1); else refillB(v);
                        if (XL) {       // the next tile's epilogue operands: row layout -> exchange tile -> accumulator layout
                            if (R1E) {
                                // every channel's row of the frame is the clip's row of g1 times that channel's weight: the 32 steps go
                                // through the exchange tile once (eight copies, rows 0..7: lanes 8 apart fetched the same quad), a lane reads
                                // its four quads from row l31 % 8 and multiplies by its own channel's weight, two quads per slice
                                if (v == 3) *reinterpret_cast<f32x4*>(Ex + xrow * EXP + xcol) = ec[0];
                                if (v == 5) {
#pragma unroll
                                    for (int q4 = 0; q4 < 4; ++q4) e1n[q4] = *reinterpret_cast<const f32x4*>(Ex + (l31 & 7) * EXP + 8 * q4 + 4 * half);
                                }
                                if (v == 9 || v == 11) {
#pragma unroll
                                    for (int q4 = v - 9; q4 < v - 7; ++q4)
                                        e1n[q4] = f32x4{__fmul_rn(kwa, e1n[q4][0]), __fmul_rn(kwa, e1n[q4][1]), __fmul_rn(kwa, e1n[q4][2]), __fmul_rn(kwa, e1n[q4][3])};
                                }
                            }
                            if (!R1E && v == 3) {
#pragma unroll
                                for (int r = 0; r < 4; ++r) *reinterpret_cast<f32x4*>(Ex + (xrow + 8 * r) * EXP + xcol) = ec[r];
                            }
                            if (!R1E && v == 5) {
#pragma unroll
                                for (int q4 = 0; q4 < 4; ++q4) e1n[q4] = *reinterpret_cast<const f32x4*>(Ex + l31 * EXP + 8 * q4 + 4 * half);
                            }
                            if (FOLD && v == 9) {
#pragma unroll
                                for (int r = 0; r < 4; ++r) *reinterpret_cast<f32x4*>(Ex + (xrow + 8 * r) * EXP + xcol) = pyc[r];
                            }
                            if (FOLD && v == 11) {
#pragma unroll
                                for (int q4 = 0; q4 < 4; ++q4) pyn[q4] = *reinterpret_cast<const f32x4*>(Ex + l31 * EXP + 8 * q4 + 4 * half);
                            }
                        }
                    }
                    else if (XL) {      // epilogue quads every second slice, then the result tile leaves in row layout
                        if (v < 40) { if ((v & 1) == 0) epi2((v - 24) >> 1); }
                        else if ((v & 1) == 0) {
                            const int r = (v - 40) >> 1;
                            buf_store4(sye, *reinterpret_cast<const f32x4*>(Ex + (xrow + 8 * r) * EXP + xcol), xoff, row8T[r]);
                        }
                    }
                    else if (v >= 24 && ((v - 24) % 3) == 0) epi2((v - 24) / 3);
                }
                // the next k-block's fragments (the other register set is free since this k-block began); with two slices per MFMA the
                // old place (slice 12 of 18) left them only three MFMAs to arrive
                if (mm == (H ? 4 : 12) && kb + 1 < 4) read_kb(kb + 1, set ^ 1);
            };
#pragma unroll
            for (int m = 0; m < 12 * NPR; ++m) {
                const int kb = m / (3 * NPR), tg = (m % (3 * NPR)) / NPR, j = m % NPR, set = kb & 1;
                FENCE;
                if (tg == 0)
                    wacc[1] = mma(A[set][PA(j)], __builtin_bit_cast(u32x4, f[set][PB(j)]), wacc[1]);
                else if (tg == 1)
                    wacc[0] = mma(A[set][PA(j)], Bl[PB(j)], wacc[0]);
                else
                    wacc[2] = mma(A[set][PA(j)], Br[PB(j)], wacc[2]);
                FENCE;
#pragma unroll
                for (int i_ = 0; i_ < SPM; ++i_) sliceB(m * SPM + i_);
                FENCE;
#ifdef WM_STAMP
                if (m == 6 * NPR - 1) { STAMP(tsh); tm[5] += tsh - ts2; }     // end of the second k-block: first half of phase B
#endif
            }
            okh_cur = okh_n; hsh_cur = hsh_n;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) { e1q[q4] = e1n[q4]; if (FOLD) pyq[q4] = pyn[q4]; }
            emk = emkn; pmk = pmkn;
        }
        STAMP(ts3);
        lds_barrier();          // image D of the next tile is complete; images G', X' of this tile are free
        STAMP(ts4);
#ifdef WM_STAMP
        tm[0] += ts1 - ts0; tm[1] += ts2 - ts1; tm[2] += ts3 - ts2; tm[3] += ts4 - ts3; tm[4] += ts1b - ts1;
#endif
        tile += tstep;
        buf ^= 1;
    }
#undef FENCE

#ifdef WM_STAMP
    if (g_wm_stamp && lane == 0) {
        unsigned long long* d = g_wm_stamp + ((size_t)blockIdx.x * 4 + wave) * 6;
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = tm[i];
    }
#endif
    // ---- outputs: weight-gradient slab (every wave owns its block), bias sums, BatchNorm sums of the data gradient
    float* out = a.partial + (size_t)blockIdx.x * (KW * 4096 + 64);
#pragma unroll
    for (int k = 0; k < KW; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(k * 64 + mt * 32 + mfma_row(r, half)) * 64 + nh * 32 + l31] = wacc[k][r] * ginv;   // x is unscaled
#pragma unroll
    for (int j = 0; j < 2; ++j) {       // the eight lanes of a channel pair sit 8 apart
        float v = bsum[j] * ginv;
        v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
        if (lane < 8) out[KW * 4096 + c0 + j] = v;
    }
    if (STATS) {
        float* red = reinterpret_cast<float*>(smem_raw);          // [2 column halves][2][64]
        s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);       // the two time halves of the lane's channel
        __syncthreads();
        if (half == 0) {
            red[nh * 128 + 32 * mt + l31] = s1;
            red[nh * 128 + 64 + 32 * mt + l31] = s2;
        }
        __syncthreads();
        if (tid < 128) a.stats[(size_t)blockIdx.x * 128 + tid] = red[tid] + red[128 + tid];
    }
    if (H && (STATS || EPI == EPI_ADD) && a.dzmax) {          // max |y| of this workgroup's output: the next consumer's gradient scale
        float* red = reinterpret_cast<float*>(smem_raw);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o));
        __syncthreads();
        if (lane == 0) red[wave] = vmax;
        __syncthreads();
        if (tid == 0) a.dzmax[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    }
}

template <int EPI, int XPRO, bool GM, bool H, bool R1 = false>
int launch_dwgrad64bf(const DWArgs& a, int* grid_out, hipStream_t stream) {
    constexpr int NP = H ? 2 : 3;
    constexpr size_t lds = (size_t)(NP * 66 * 72 + 2 * NP * 64 * 72 + 2 * NP * 64 * 88) * 2 + (R1 ? 9 : 8) * 64 * sizeof(float) +
                           (H ? (size_t)4 * 32 * 36 * sizeof(float) : 0);
    static wm::DevOnce attr_done;
    auto kern = dwgrad64bf_kernel<EPI, XPRO, GM, H, R1>;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(kern), lds, attr_done)) return rc;
    const int ntiles = a.B * (a.T / 64);
    const int grid = ntiles < kNumCU ? ntiles : kNumCU;
    *grid_out = grid;
    if (a.stats && grid < kNumCU) WM_TRY(hipMemsetAsync(a.stats, 0, sizeof(float) * 128 * kNumCU, stream));
    if (H && a.dzmax && grid < kNumCU) WM_TRY(hipMemsetAsync(a.dzmax, 0, sizeof(float) * kNumCU, stream));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, a);
    WM_CHECK_LAUNCH();
    return 0;
}

// the slabs of the launch above -> dw [64][64][3], dbias [64]
int reduce_dwgrad_slabs(const float* partial, int grid, float* dw, float* dbias, int accumulate, hipStream_t stream) {
    const int n = 3 * 4096 + 64;
    hipLaunchKernelGGL(wgrad64_reduce_kernel, dim3((n + 63) / 64), dim3(256), 0, stream, partial, grid, 3, 0, dw, dbias, accumulate & 1);
    WM_CHECK_LAUNCH();
    return 0;
}
}  // namespace

extern "C" {
WM_STAMP_SETTER(wm_debug_set_stamp_buffer_dwgrad)
// data gradient + weight gradient of a k3 convolution in one launch (dwgrad64bf_kernel); T % 64 == 0
int wm_dwgrad64_bf(const float* g, const float* g2, const float* ga, const float* gb, const float* gc, const void* wpb,
                   const float* x, const float* xa, const float* xb, const float* e1, const float* ea, const float* eb,
                   float* y, float* stats, float* partial, float* dw, float* dbias, int B, int T, int xpro, int epi, int accumulate,
                   const void* gmask, int arith, const float* gscale, float* dzmax, hipStream_t stream) {
    if (B <= 0 || T <= 0 || (T & 63)) return (int)hipErrorInvalidValue;
    if (!g || !g2 || !ga || !gb || !gc || !wpb || !x || !e1 || !y || !partial || !dw) return (int)hipErrorInvalidValue;
    if (arith != 0 && (arith != 1 || !gscale)) return (int)hipErrorInvalidValue;
    DWArgs a{g, g2, ga, gb, gc, wpb, x, xa, xb, e1, ea, eb, y, stats, partial, B, T, reinterpret_cast<const unsigned*>(gmask),
             epi == EPI_ADDSTATS ? reinterpret_cast<const unsigned*>(eb) : nullptr, epi == EPI_ADDSTATS ? ea : nullptr, gscale, dzmax,
             nullptr, nullptr};
    int grid = 0, rc = (int)hipErrorInvalidValue;
#define WM_DW(E, X, G) (arith ? launch_dwgrad64bf<E, X, G, true>(a, &grid, stream) : launch_dwgrad64bf<E, X, G, false>(a, &grid, stream))
    if (epi == EPI_RELUMASK && xpro == PRO_BNRELU && stats && xa && xb && ea && eb)
        rc = gmask ? WM_DW(EPI_RELUMASK, PRO_BNRELU, true) : WM_DW(EPI_RELUMASK, PRO_BNRELU, false);
    else if (epi == EPI_ADD && xpro == PRO_NONE && !stats)
        rc = gmask ? WM_DW(EPI_ADD, PRO_NONE, true) : WM_DW(EPI_ADD, PRO_NONE, false);
    else if (epi == EPI_ADDSTATS && xpro == PRO_NONE && stats && ea && eb && gmask)
        rc = WM_DW(EPI_ADDSTATS, PRO_NONE, true);
#undef WM_DW
    if (rc) return rc;
    return reduce_dwgrad_slabs(partial, grid, dw, dbias, accumulate, stream);
}

// wm_dwgrad64_bf for the block in front of the Conv1d(64, 1, 1) head, whose output gradient is the rank-one frame hw[c] g1[b][t]
// (wm_head1_bwd's dx): the frame is formed on load from g1 [B][T] and hw [64] instead of being read.  Two forms, both with gmask and
// arith 1: (xpro 1, epi 1) with g == NULL, the frame is the gradient operand; (xpro 0, epi 2) with e1 == NULL, it is the addend.
// Everything else, and every result bit for bit, as wm_dwgrad64_bf on the materialised frame.
int wm_dwgrad64_bf_r1(const float* g, const float* g2, const float* ga, const float* gb, const float* gc, const void* wpb,
                      const float* x, const float* xa, const float* xb, const float* e1, const float* ea, const float* eb,
                      float* y, float* stats, float* partial, float* dw, float* dbias, int B, int T, int xpro, int epi, int accumulate,
                      const void* gmask, int arith, const float* gscale, float* dzmax, const float* g1, const float* hw,
                      hipStream_t stream) {
    if (B <= 0 || T <= 0 || (T & 63)) return (int)hipErrorInvalidValue;
    if (!g1 || !hw || !gmask || !g2 || !ga || !gb || !gc || !wpb || !x || !y || !partial || !dw) return (int)hipErrorInvalidValue;
    if (arith != 1 || !gscale) return (int)hipErrorInvalidValue;
    DWArgs a{g, g2, ga, gb, gc, wpb, x, xa, xb, e1, ea, eb, y, stats, partial, B, T, reinterpret_cast<const unsigned*>(gmask),
             nullptr, nullptr, gscale, dzmax, g1, hw};
    int grid = 0, rc = (int)hipErrorInvalidValue;
    if (epi == EPI_RELUMASK && xpro == PRO_BNRELU && !g && e1 && stats && xa && xb && ea && eb)
        rc = launch_dwgrad64bf<EPI_RELUMASK, PRO_BNRELU, true, true, true>(a, &grid, stream);
    else if (epi == EPI_ADD && xpro == PRO_NONE && g && !e1 && !stats)
        rc = launch_dwgrad64bf<EPI_ADD, PRO_NONE, true, true, true>(a, &grid, stream);
    if (rc) return rc;
    return reduce_dwgrad_slabs(partial, grid, dw, dbias, accumulate, stream);
}

// wm_dwgrad64_bf's plain conv1 pair (xpro 0, epi 2, no gmask, arith 1) for the first block behind a stem: the weight-gradient operand
// x = Conv1d(1, 64, 7, padding = 3)(s) is formed on load from the clips s [B,1,T] and the stem's stem_w [64,7], stem_b [64] instead
// of being read.  e1 = the addend of the data gradient.  Everything else, and every result bit for bit, as wm_dwgrad64_bf on the
// materialised x.  A null pointer (dzmax may be null) or T % 64 != 0 is hipErrorInvalidValue, and nothing is written.
int wm_dwgrad64_bf_stem(const float* g, const float* g2, const float* ga, const float* gb, const float* gc, const void* wpb,
                        const float* e1, float* y, float* partial, float* dw, float* dbias, int B, int T, int accumulate,
                        const float* gscale, float* dzmax, const float* s, const float* stem_w, const float* stem_b,
                        hipStream_t stream) {
    if (B <= 0 || T <= 0 || (T & 63) || T >= (1 << 29)) return (int)hipErrorInvalidValue;            // clip offsets are 32-bit bytes
    if (!g || !g2 || !ga || !gb || !gc || !wpb || !e1 || !y || !partial || !dw || !gscale || !s || !stem_w || !stem_b) return (int)hipErrorInvalidValue;
    DWArgs a{g, g2, ga, gb, gc, wpb, nullptr, nullptr, nullptr, e1, nullptr, nullptr, y, nullptr, partial, B, T, nullptr,
             nullptr, nullptr, gscale, dzmax, nullptr, nullptr, s, stem_w, stem_b};
    int grid = 0;
    if (int rc = launch_dwgrad64bf<EPI_ADD, PRO_STEM, false, true>(a, &grid, stream)) return rc;
    return reduce_dwgrad_slabs(partial, grid, dw, dbias, accumulate, stream);
}
}  // extern "C"
