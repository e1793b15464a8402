// lstm.hpp's forward family: the input projection and the three forward recurrences (plain, projection inside, wave-specialised)
#include "lstm.hpp"

namespace {

// ------------------------------------------------------------------------------------ xproj
// block = (clip, 128-step tile); wave w owns gate columns [64w, 64w+64); D rows = time, cols = gate.
__global__ __launch_bounds__(256) void lstm_xproj_kernel(const float* __restrict__ x, const float* __restrict__ w_ih,
                                                         const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                         float* __restrict__ xp, int T) {
    constexpr int NT = 128, XS = NT + 4;
    __shared__ __align__(16) float xs[64 * XS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int tilesPerClip = (T + NT - 1) / NT;
    const int b = blockIdx.x / tilesPerClip, t0 = (blockIdx.x % tilesPerClip) * NT;
    const float* xb = x + (size_t)b * 64 * T;
    for (int i = tid; i < 64 * (NT / 4); i += 256) {
        const int c = i / (NT / 4), q = i % (NT / 4), t = t0 + 4 * q;
        // unconditional load from a clamped address (rows past T are never stored): no branch, no vmcnt drain
        *reinterpret_cast<float4*>(xs + c * XS + 4 * q) = *reinterpret_cast<const float4*>(xb + (size_t)c * T + min(t, T - 4));
    }
    // B operand (W_ih^T) for this wave's two 32-column tiles: B[k = c][j = n] = w_ih[n][c]
    float breg[2][32];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int s = 0; s < 32; ++s) breg[nt][s] = w_ih[gate_row(wave * 64 + nt * 32 + l31) * 64 + 2 * s + half];
    float bias[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int n = gate_row(wave * 64 + nt * 32 + l31);
        bias[nt] = b_ih[n] + b_hh[n];
    }
    __syncthreads();
#pragma unroll 1
    for (int mt = 0; mt < 4; ++mt) {
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
        const float* ap = xs + half * XS + mt * 32 + l31;     // A[i = t][k = c] = xs[c][t]
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            const float a = ap[2 * s * XS];
            acc0 = mfma32(a, breg[0][s], acc0);
            acc1 = mfma32(a, breg[1][s], acc1);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int t = t0 + mt * 32 + mfma_row(r, half);
            if (t < T) {
                float* o = xp + ((size_t)b * T + t) * 256 + wave * 64 + l31;
                o[0] = acc0[r] + bias[0];
                o[32] = acc1[r] + bias[1];
            }
        }
    }
}

// ------------------------------------------------------------------------------- recurrence fwd
template <bool SAVE>
__global__ __launch_bounds__(256) void lstm_fwd_kernel(const float* xp, const float* __restrict__ w_hh,
                                                       float* __restrict__ hout, float* gates,   // gates may alias xp
                                                       float* __restrict__ cst, int T) {
    constexpr int HS = WM_LSTM_HS;                  // h values taken through SGPRs (multiple of 8, power of two), rest via LDS broadcast
    __shared__ __align__(16) float hs[2][64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane & 3, ul = lane >> 2, u = wave * 16 + ul, n = q * 64 + u, np = wave * 64 + lane;
    // one W_hh row per lane, as 32 register pairs: the recurrent dot product issues v_pk_fma_f32, which keeps the
    // SIMD's fp32 pipe full from a single wave (a lone wave issues one VALU op per 4 cycles; a plain v_fma only
    // occupies the pipe for 2 of them)
    v2f wr[32];
#pragma unroll
    for (int k = 0; k < 64; k += 4) {
        const float4 v = *reinterpret_cast<const float4*>(w_hh + n * 64 + k);
        wr[k / 2] = v2f{v.x, v.y};
        wr[k / 2 + 1] = v2f{v.z, v.w};
    }
    if (tid < 128) (&hs[0][0])[tid] = 0.f;
    float c = 0.f;
    const float* xpb = xp + (size_t)b * T * 256 + np;
    float* gb = SAVE ? gates + (size_t)b * T * 256 + np : nullptr;
    float* cb = SAVE ? cst + (size_t)b * T * 64 + u : nullptr;
    float* hb = hout + ((size_t)b * 64 + u) * T;
    const bool is_g = (q == 2);

    float xa[16], xb_[16];
    auto prefetch = [&](float (&buf)[16], int t0) {
#pragma unroll
        for (int s = 0; s < 16; ++s) buf[s] = xpb[(size_t)min(t0 + s, T - 1) * 256];      // unconditional (clamped)
    };
    auto run_chunk = [&](const float (&xin)[16], int t0) {
        float hk[4];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int t = t0 + s;
            if (t < T) {                                   // uniform across the workgroup
                // h reaches the lanes two ways at once.  Broadcasting all 64 values to all 256 lanes through LDS reads
                // is 64 KB per step = 512 cycles of the CU's LDS return path -- the step's bottleneck.  So the first
                // HS values come as ONE ds_read_b32 per wave + v_readlane into SGPRs (VALU work, scalar FMA operands)
                // and only the rest as broadcast ds_read_b128: LDS and VALU each carry about half.
                const float hv = hs[s & 1][lane & (HS - 1)];
                const float4* hp = reinterpret_cast<const float4*>(hs[s & 1]);
                float4 hq[(64 - HS) / 4];
#pragma unroll
                for (int k = 0; k < (64 - HS) / 4; ++k) hq[k] = hp[HS / 4 + k];
                v2f a01 = v2f{xin[s], 0.f}, a23 = v2f{0.f, 0.f}, b01 = a23, b23 = a23;
                {
                    unsigned long long hp[HS / 2];
                    lanes_to_sgprs<HS>(hv, 0, hp);
#pragma unroll
                    for (int k = 0; k < HS; k += 8) {
                        a01 = pk_fma_s(wr[k / 2], hp[k / 2], a01);
                        a23 = pk_fma_s(wr[k / 2 + 1], hp[k / 2 + 1], a23);
                        b01 = pk_fma_s(wr[k / 2 + 2], hp[k / 2 + 2], b01);
                        b23 = pk_fma_s(wr[k / 2 + 3], hp[k / 2 + 3], b23);
                    }
                }
#pragma unroll
                for (int k = 0; k < (64 - HS) / 4; k += 2) {
                    const float4 h0 = hq[k], h1 = hq[k + 1];
                    a01 = __builtin_elementwise_fma(wr[HS / 2 + 2 * k], v2f{h0.x, h0.y}, a01);
                    a23 = __builtin_elementwise_fma(wr[HS / 2 + 2 * k + 1], v2f{h0.z, h0.w}, a23);
                    b01 = __builtin_elementwise_fma(wr[HS / 2 + 2 * k + 2], v2f{h1.x, h1.y}, b01);
                    b23 = __builtin_elementwise_fma(wr[HS / 2 + 2 * k + 3], v2f{h1.z, h1.w}, b23);
                }
                const v2f sm = (a01 + a23) + (b01 + b23);
                const float act = gate_act(sm.x + sm.y, is_g);
                const float gi = quad_bcast<0>(act), gf = quad_bcast<1>(act), gg = quad_bcast<2>(act), go = quad_bcast<3>(act);
                c = fmaf(gf, c, gi * gg);
                const float h = go * tanh_s(c);
                if (q == 0) hs[(s + 1) & 1][u] = h;
                if (SAVE) {
                    gb[(size_t)t * 256] = act;             // one contiguous 256-B segment per wave
                    if (q == 1) cb[(size_t)t * 64] = c;
                }
                if (((s >> 2) & 3) == q) hk[s & 3] = h;
                if (s == 15) {
                    // every lane now holds h for steps t0+4q .. t0+4q+3 of its unit
                    *reinterpret_cast<float4*>(hb + t0 + 4 * q) = make_float4(hk[0], hk[1], hk[2], hk[3]);
                }
                __syncthreads();
            }
        }
        // ragged tail (T not a multiple of 16): flush what the last partial chunk produced
        if (t0 + 16 > T) {
            const int tq = t0 + 4 * q;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (tq + j < T) hb[tq + j] = hk[j];
        }
    };

    prefetch(xa, 0);
    __syncthreads();
    for (int t0 = 0; t0 < T; t0 += 32) {
        prefetch(xb_, t0 + 16);
        run_chunk(xa, t0);
        prefetch(xa, t0 + 32);
        if (t0 + 16 < T) run_chunk(xb_, t0 + 16);
    }
}

// ------------------------------------------------------ recurrence fwd with the input projection inside
// Same recurrence as lstm_fwd_kernel, but xp = W_ih x + b is never materialised in HBM (4.2 GB written by
// lstm_xproj and read back here at B = 256).  While the workgroup steps through 32-step chunk c it also computes chunk
// c+1's projection [32 steps x 256 gate rows] on the bf16 matrix cores (bf16x6 split, fp32-grade; a separate pipe from
// the VALU the recurrence runs on): 48 MFMAs per wave dealt two per step between the recurrence's own instructions.
// W_ih lives in registers as 3-piece A fragments (96 VGPRs: this wave's 64 gate rows), the x tile goes global ->
// registers (two chunks ahead) -> split -> LDS [step][channel] pieces (B fragments), results land in a double-buffered
// LDS table xps[2][32][256(+1)] from which every lane picks its own gate row, one ds_read_b32 per step.
// dynamic LDS of this kernel and of lstm_fwd_ws_kernel, which carves the same layout: the double-buffered table xps [2][32][257] fp32,
// the x image Xb [3 pieces][32 steps][pitch 72] bf16, the h line hsm [2][64] fp32
constexpr size_t kLstmFwdLds = (size_t)2 * 32 * 257 * sizeof(float) + (size_t)3 * 32 * 72 * 2 + 128 * sizeof(float);
template <bool SAVE>
__global__ __launch_bounds__(256) void lstm_fwd_fused_kernel(const float* __restrict__ x, const float* __restrict__ w_ih,
                                                             const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                             const float* __restrict__ w_hh, float* __restrict__ hout,
                                                             float* __restrict__ gates, float* __restrict__ cst, int T) {
    constexpr int HS = WM_LSTM_HS, CH = 32, XPP = 257, PITCH = 72, NP = 3;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    float* xps = reinterpret_cast<float*>(smem_raw);                                  // [2][CH][XPP]
    unsigned short* Xb = reinterpret_cast<unsigned short*>(xps + 2 * CH * XPP);       // [NP][CH][PITCH]
    float* hsm = reinterpret_cast<float*>(Xb + NP * CH * PITCH);                      // [2][64]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int q = lane & 3, ul = lane >> 2, u = wave * 16 + ul, n = q * 64 + u, np = wave * 64 + lane;
    float wr[64];                                  // W_hh row n of this lane
#pragma unroll
    for (int k = 0; k < 64; k += 4) {
        const float4 v = *reinterpret_cast<const float4*>(w_hh + n * 64 + k);
        wr[k] = v.x; wr[k + 1] = v.y; wr[k + 2] = v.z; wr[k + 3] = v.w;
    }
    // W_ih A fragments: row i = l31 of m-tile mt <-> gate column n' = wave*64 + mt*32 + l31, k = 16 ks + 8 half + j
    bf16x8 Wi[2][4][NP];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const float* wp = w_ih + gate_row(wave * 64 + mt * 32 + l31) * 64 + 16 * ks + 8 * half;
            const float4 v0 = *reinterpret_cast<const float4*>(wp), v1 = *reinterpret_cast<const float4*>(wp + 4);
            unsigned a[4], m[4], l[4];
            split3_pair(v0.x, v0.y, a[0], m[0], l[0]); split3_pair(v0.z, v0.w, a[1], m[1], l[1]);
            split3_pair(v1.x, v1.y, a[2], m[2], l[2]); split3_pair(v1.z, v1.w, a[3], m[3], l[3]);
            Wi[mt][ks][0] = __builtin_bit_cast(bf16x8, make_uint4(a[0], a[1], a[2], a[3]));
            Wi[mt][ks][1] = __builtin_bit_cast(bf16x8, make_uint4(m[0], m[1], m[2], m[3]));
            Wi[mt][ks][2] = __builtin_bit_cast(bf16x8, make_uint4(l[0], l[1], l[2], l[3]));
        }
    const float bias = b_ih[n] + b_hh[n];
    if (tid < 128) hsm[tid] = 0.f;
    float c = 0.f;
    // per-step outputs through buffer descriptors: the step index travels as a scalar offset, the lane's part is fixed, lanes that
    // have nothing to store point past the end of the descriptor (the hardware drops the access): no 64-bit address arithmetic and
    // no lane mask on the recurrence's critical path
    const wm_srd_t sgb = make_srd(SAVE ? gates + (size_t)b * T * 256 : hout, SAVE ? (size_t)T * 256 * sizeof(float) : 0);
    const wm_srd_t scb = make_srd(SAVE ? cst + (size_t)b * T * 64 : hout, SAVE ? (size_t)T * 64 * sizeof(float) : 0);
    const wm_srd_t shb = make_srd(hout + (size_t)b * 64 * T, (size_t)64 * T * sizeof(float));
    const unsigned vgb = (unsigned)np * 4u, vcb = (q == 1) ? (unsigned)u * 4u : 0xFFFFFF00u;
    const unsigned vhb = (unsigned)(u * T + 4 * q) * 4u;
    float* hb = hout + ((size_t)b * 64 + u) * T;
    const bool is_g = (q == 2);

    // x tile staging (one combo per thread): channel pair cp, time quad tq of the chunk
    const int cp = wave * 8 + (lane & 7), tq = lane >> 3;
    const float* xc = x + ((size_t)b * 64 + 2 * cp) * T + 4 * tq;
    float4 sa, sb;
    auto load_x = [&](int t0) {                    // clamped: chunks past the end re-read the last valid quad
        const int t = min(t0, T - 4 - 4 * tq);
        sa = *reinterpret_cast<const float4*>(xc + max(t, -4 * tq));
        sb = *reinterpret_cast<const float4*>(xc + T + max(t, -4 * tq));
    };
    auto split_x = [&]() {
        unsigned* X32 = reinterpret_cast<unsigned*>(Xb);
        const float va[4] = {sa.x, sa.y, sa.z, sa.w}, vb[4] = {sb.x, sb.y, sb.z, sb.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            unsigned p0, p1, p2;
            split3_pair(va[e], vb[e], p0, p1, p2);
            const int o = (4 * tq + e) * (PITCH / 2) + cp;
            X32[o] = p0; X32[CH * PITCH / 2 + o] = p1; X32[2 * (CH * PITCH / 2) + o] = p2;
        }
    };
    f32x16 acc[2];
    bf16x8 Bf[NP];
    // idx-th of the 48 MFMAs of a chunk's projection: block m = idx / 6 = ks * 2 + mt, piece product idx % 6.  They are
    // issued ONE at a time, far apart in the instruction stream: back-to-back dependent MFMAs would stall the wave's
    // in-order issue (and with it the latency-bound recurrence) for the 32 cycles each one occupies the pipe.
    auto mfma_one = [&](int idx) {
        const int m = idx / 6, pr = idx % 6, ks = m >> 1, mt = m & 1;
        const int pa = (pr == 0 || pr == 4) ? 1 : (pr == 2 ? 2 : 0), pb = (pr == 0 || pr == 3) ? 1 : (pr == 1 ? 2 : 0);
        if (mt == 0 && pr == 0) {
#pragma unroll
            for (int p = 0; p < NP; ++p) Bf[p] = *reinterpret_cast<const bf16x8*>(Xb + (p * CH + l31) * PITCH + 16 * ks + 8 * half);
        }
        if (ks == 0 && pr == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
        }
        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Wi[mt][ks][pa], Bf[pb], acc[mt], 0, 0, 0);
    };
    auto store_xp = [&](int buf) {                 // D row = gate column (this wave's 64), D column = step
        float* dst = xps + (buf * CH + l31) * XPP + wave * 64 + 4 * half;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[mt * 32 + (r & 3) + 8 * (r >> 2)] = acc[mt][r];
    };

    // ---- prologue: projection of chunk 0, x tile of chunk 1 in flight
    load_x(0);
    __syncthreads();
    split_x();
    load_x(CH);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 48; ++i) mfma_one(i);
    store_xp(0);
    __syncthreads();

    float hk[4];
    int t0 = 0, cbuf = 0;
#ifdef WM_STAMP
    unsigned long long tm[6] = {0, 0, 0, 0, 0, 0};
#endif
    // eight steps of the chunk with compile-time positions s = 8*SUB + j (register-array indices must be constants)
    auto run8 = [&](auto sub_c) {
        constexpr int SUB = decltype(sub_c)::value;
#pragma unroll
        for (int j8 = 0; j8 < 8; ++j8) {
            const int s = SUB * 8 + j8;
            const int t = t0 + s;
            // ---- side work: projection of the next chunk (independent of the recurrence; no effect past the end)
            if (s == 0) { split_x(); load_x(t0 + 2 * CH); }
            if (s >= 2 && s < 26) mfma_one(2 * (s - 2));
            if (s == 28) store_xp(cbuf ^ 1);
            if (t < T) {                                   // uniform across the workgroup
                LSTAMP(ls0, c);
                const float xin = xps[(cbuf * CH + s) * XPP + np] + bias;
                const float* hcur = hsm + (s & 1) * 64;
                const float4 hq4 = *reinterpret_cast<const float4*>(hcur + 4 * (lane & 15));   // h(t-1), row-replicated: one read per lane
                float Hh[4] = {hq4.x, hq4.y, hq4.z, hq4.w};
                float hv = Hh[0];
                LSTAMP(ls1, hv);                           // h of the previous step is in registers (LDS read latency)
                Hh[0] = hv;
                if (s >= 2 && s < 26) mfma_one(2 * (s - 2) + 1);
                float pre = dot64_rowbcast(Hh, wr, xin);     // the projection term rides in as the first accumulator's start value
                LSTAMP(ls2, pre);                          // 64-term dot product of the lane's gate row done
                float act = gate_act(pre, is_g);
                LSTAMP(ls3, act);                          // gate activation (exp + rcp)
                const float gi = quad_bcast<0>(act), gf = quad_bcast<1>(act), gg = quad_bcast<2>(act), go = quad_bcast<3>(act);
                c = fmaf(gf, c, gi * gg);
                float h = go * tanh_s(c);
                LSTAMP(ls4, h);                            // quad exchange, cell update, tanh(c)
                hsm[((s + 1) & 1) * 64 + rowbcast_slot(u)] = h;            // the four lanes of a quad hold the same h: no lane mask
                if (SAVE) {
                    buf_store(sgb, act, vgb, (unsigned)t * 1024u);      // one contiguous 256-B segment per wave
                    buf_store(scb, c, vcb, (unsigned)t * 256u);         // the q == 1 lane of every quad
                }
                if (((s >> 2) & 3) == q) hk[s & 3] = h;
                if ((s & 15) == 15)                        // every lane holds h for steps 4q .. 4q+3 of this 16-step group
                    buf_store4(shb, f32x4{hk[0], hk[1], hk[2], hk[3]}, vhb, (unsigned)(t0 + (s - 15)) * 4u);
                LSTAMP(ls5, h);                            // h to LDS, saved activations / outputs issued
                __syncthreads();
                LSTAMP(ls6, c);                            // barrier
                LSTAMP_ACC(0, ls0, ls1); LSTAMP_ACC(1, ls1, ls2); LSTAMP_ACC(2, ls2, ls3); LSTAMP_ACC(3, ls3, ls4);
                LSTAMP_ACC(4, ls4, ls5); LSTAMP_ACC(5, ls5, ls6);
            }
        }
    };
    for (; t0 < T; t0 += CH, cbuf ^= 1) {
        run8(std::integral_constant<int, 0>{});
        run8(std::integral_constant<int, 1>{});
        run8(std::integral_constant<int, 2>{});
        run8(std::integral_constant<int, 3>{});
        // ragged tail (T % 16 != 0): flush what the last partial 16-step group produced
        if (t0 + CH > T && (T & 15)) {
            const int g0 = (T >> 4) << 4, tq0 = g0 + 4 * q;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (tq0 + j < T) hb[tq0 + j] = hk[j];
        }
    }
#ifdef WM_STAMP
    if (g_lstm_stamp && lane == 0) {
        unsigned long long* d = g_lstm_stamp + ((size_t)blockIdx.x * 4 + wave) * 6;
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = tm[i];
    }
#endif
}

// ------------------------------------------ recurrence fwd, wave-specialised: the input projection beside it
// lstm_fwd_fused_kernel with the roles split over eight waves (as lstm_bwd_ws_kernel): waves 0..3 run the recurrence and nothing else;
// waves 4..7 -- the second wave of each SIMD -- compute chunk c+1's projection [32 steps x 256 gate rows] on the matrix cores (bf16x6,
// W_ih fragments in THEIR registers: the recurrence waves lose 96 registers, 48 MFMAs, the x split and the table stores per chunk)
// into the other half of the double-buffered LDS table.  The helpers execute the recurrence's one barrier per step and use those
// barriers as their own phase separators: slot 0 of a chunk splits the x tile into the LDS image, slots 1..24 issue two MFMAs each,
// slot 26 stores the table.  Same arithmetic and summation order as the fused kernel: bit-identical results.
// TAIL (T % 32 == 0): x is the input of the ResBlock in front of the LSTM and the helpers form that block's tail while they stage it,
// v = relu(x + y2 * sc2 + sh2) in bn_add_relu_kernel's expression (bn.hip), split v as before, and in the idle slot 27 store the
// chunk's v to `out` and its sign bits to `mask` (wm_bn_add_relu_mask's layout; the staging map is conv64bf3's, see sign_nibble)
template <bool TAIL>
struct LstmTailArgs {};
template <>
struct LstmTailArgs<true> {
    const float* y2; const float* sc2; const float* sh2;   // [B,64,T], [64], [64]
    float* out; unsigned* mask;                            // [B,64,T], [B*64][T/32] or nullptr
};
template <bool SAVE, bool TAIL = false>
__global__ __launch_bounds__(512) void lstm_fwd_ws_kernel(const float* __restrict__ x, const float* __restrict__ w_ih,
                                                          const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                          const float* __restrict__ w_hh, float* __restrict__ hout,
                                                          float* __restrict__ gates, float* __restrict__ cst, int T,
                                                          LstmTailArgs<TAIL> tl) {
    constexpr int CH = 32, XPP = 257, PITCH = 72, NP = 3;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    float* xps = reinterpret_cast<float*>(smem_raw);                                  // [2][CH][XPP]
    unsigned short* Xb = reinterpret_cast<unsigned short*>(xps + 2 * CH * XPP);       // [NP][CH][PITCH]
    float* hsm = reinterpret_cast<float*>(Xb + NP * CH * PITCH);                      // [2][64]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (wave < 4) {
        // ------------------------------------------------------------------ the recurrence
        __builtin_amdgcn_s_setprio(3);
        const int q = lane & 3, ul = lane >> 2, u = wave * 16 + ul, n = q * 64 + u, np = wave * 64 + lane;
        float wr[64];                                  // W_hh row n of this lane
#pragma unroll
        for (int k = 0; k < 64; k += 4) {
            const float4 v = *reinterpret_cast<const float4*>(w_hh + n * 64 + k);
            wr[k] = v.x; wr[k + 1] = v.y; wr[k + 2] = v.z; wr[k + 3] = v.w;
        }
        const float bias = b_ih[n] + b_hh[n];
        if (tid < 128) hsm[tid] = 0.f;
        float c = 0.f;
        const wm_srd_t sgb = make_srd(SAVE ? gates + (size_t)b * T * 256 : hout, SAVE ? (size_t)T * 256 * sizeof(float) : 0);
        const wm_srd_t scb = make_srd(SAVE ? cst + (size_t)b * T * 64 : hout, SAVE ? (size_t)T * 64 * sizeof(float) : 0);
        const wm_srd_t shb = make_srd(hout + (size_t)b * 64 * T, (size_t)64 * T * sizeof(float));
        const unsigned vgb = (unsigned)np * 4u, vcb = (q == 1) ? (unsigned)u * 4u : 0xFFFFFF00u;
        const unsigned vhb = (unsigned)(u * T + 4 * q) * 4u;
        float* hb = hout + ((size_t)b * 64 + u) * T;
        const bool is_g = (q == 2);
        __syncthreads(); __syncthreads(); __syncthreads();          // the helpers' prologue: projection of chunk 0
        float hk[4];
        int t0 = 0, cbuf = 0;
        auto run8 = [&](auto sub_c) {
            constexpr int SUB = decltype(sub_c)::value;
#pragma unroll
            for (int j8 = 0; j8 < 8; ++j8) {
                const int s = SUB * 8 + j8;
                const int t = t0 + s;
                if (t < T) {                                   // uniform across the workgroup
                    const float xin = xps[(cbuf * CH + s) * XPP + np] + bias;
                    const float* hcur = hsm + (s & 1) * 64;
                    const float4 hq4 = *reinterpret_cast<const float4*>(hcur + 4 * (lane & 15));   // h(t-1), row-replicated
                    const float Hh[4] = {hq4.x, hq4.y, hq4.z, hq4.w};
                    const float pre = dot64_rowbcast(Hh, wr, xin);
                    const float act = gate_act(pre, is_g);
                    const float gi = quad_bcast<0>(act), gf = quad_bcast<1>(act), gg = quad_bcast<2>(act), go = quad_bcast<3>(act);
                    c = fmaf(gf, c, gi * gg);
                    const float h = go * tanh_s(c);
                    hsm[((s + 1) & 1) * 64 + rowbcast_slot(u)] = h;
                    if (SAVE) {
                        buf_store(sgb, act, vgb, (unsigned)t * 1024u);
                        buf_store(scb, c, vcb, (unsigned)t * 256u);
                    }
                    if (((s >> 2) & 3) == q) hk[s & 3] = h;
                    if ((s & 15) == 15)
                        buf_store4(shb, f32x4{hk[0], hk[1], hk[2], hk[3]}, vhb, (unsigned)(t0 + (s - 15)) * 4u);
                    __syncthreads();
                }
            }
        };
        for (; t0 < T; t0 += CH, cbuf ^= 1) {
            run8(std::integral_constant<int, 0>{});
            run8(std::integral_constant<int, 1>{});
            run8(std::integral_constant<int, 2>{});
            run8(std::integral_constant<int, 3>{});
            if (t0 + CH > T && (T & 15)) {                   // ragged tail: flush what the last partial 16-step group produced
                const int g0 = (T >> 4) << 4, tq0 = g0 + 4 * q;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (tq0 + j < T) hb[tq0 + j] = hk[j];
            }
        }
        return;
    }
    // ---------------------------------------------------------------------- the helpers: projection of the next chunk
    const int hw = wave - 4;
    bf16x8 Wi[2][4][NP];                                   // W_ih A fragments: row l31 of m-tile mt <-> gate column hw*64 + mt*32 + l31
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const float* wp = w_ih + gate_row(hw * 64 + mt * 32 + l31) * 64 + 16 * ks + 8 * half;
            const float4 v0 = *reinterpret_cast<const float4*>(wp), v1 = *reinterpret_cast<const float4*>(wp + 4);
            unsigned a[4], m[4], l[4];
            split3_pair(v0.x, v0.y, a[0], m[0], l[0]); split3_pair(v0.z, v0.w, a[1], m[1], l[1]);
            split3_pair(v1.x, v1.y, a[2], m[2], l[2]); split3_pair(v1.z, v1.w, a[3], m[3], l[3]);
            Wi[mt][ks][0] = __builtin_bit_cast(bf16x8, make_uint4(a[0], a[1], a[2], a[3]));
            Wi[mt][ks][1] = __builtin_bit_cast(bf16x8, make_uint4(m[0], m[1], m[2], m[3]));
            Wi[mt][ks][2] = __builtin_bit_cast(bf16x8, make_uint4(l[0], l[1], l[2], l[3]));
        }
    const int cp = hw * 8 + (lane & 7), tq = lane >> 3;    // x tile staging: channel pair cp, time quad tq of the chunk
    const float* xc = x + ((size_t)b * 64 + 2 * cp) * T + 4 * tq;
    float4 sa, sb;
    [[maybe_unused]] float4 sa2, sb2, oa, ob;      // TAIL: the y2 quads in flight, the formed quads until their store
    [[maybe_unused]] const float* yc = nullptr;
    [[maybe_unused]] float* oc = nullptr;
    [[maybe_unused]] float tsc0 = 0.f, tsc1 = 0.f, tsh0 = 0.f, tsh1 = 0.f;
    if constexpr (TAIL) {
        yc = tl.y2 + ((size_t)b * 64 + 2 * cp) * T + 4 * tq;
        oc = tl.out + ((size_t)b * 64 + 2 * cp) * T + 4 * tq;
        tsc0 = tl.sc2[2 * cp]; tsc1 = tl.sc2[2 * cp + 1]; tsh0 = tl.sh2[2 * cp]; tsh1 = tl.sh2[2 * cp + 1];
    }
    auto load_x = [&](int t0) {                    // clamped: chunks past the end re-read the last valid quad
        const int t = min(t0, T - 4 - 4 * tq);
        sa = *reinterpret_cast<const float4*>(xc + max(t, -4 * tq));
        sb = *reinterpret_cast<const float4*>(xc + T + max(t, -4 * tq));
        if constexpr (TAIL) {
            sa2 = *reinterpret_cast<const float4*>(yc + max(t, -4 * tq));
            sb2 = *reinterpret_cast<const float4*>(yc + T + max(t, -4 * tq));
        }
    };
    auto split_x = [&]() {
        unsigned* X32 = reinterpret_cast<unsigned*>(Xb);
        float va[4] = {sa.x, sa.y, sa.z, sa.w}, vb[4] = {sb.x, sb.y, sb.z, sb.w};
        if constexpr (TAIL) {
            const float wa[4] = {sa2.x, sa2.y, sa2.z, sa2.w}, wb[4] = {sb2.x, sb2.y, sb2.z, sb2.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                va[e] = fmaxf(va[e] + fmaf(wa[e], tsc0, tsh0), 0.f);
                vb[e] = fmaxf(vb[e] + fmaf(wb[e], tsc1, tsh1), 0.f);
            }
            oa = make_float4(va[0], va[1], va[2], va[3]); ob = make_float4(vb[0], vb[1], vb[2], vb[3]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            unsigned p0, p1, p2;
            split3_pair(va[e], vb[e], p0, p1, p2);
            const int o = (4 * tq + e) * (PITCH / 2) + cp;
            X32[o] = p0; X32[CH * PITCH / 2 + o] = p1; X32[2 * (CH * PITCH / 2) + o] = p2;
        }
    };
    f32x16 acc[2];
    bf16x8 Bf[NP];
    auto mfma_one = [&](int idx) {                 // idx-th of the 48 MFMAs of a chunk: block m = idx / 6 = ks * 2 + mt, piece product idx % 6
        const int m = idx / 6, pr = idx % 6, ks = m >> 1, mt = m & 1;
        const int pa = (pr == 0 || pr == 4) ? 1 : (pr == 2 ? 2 : 0), pb = (pr == 0 || pr == 3) ? 1 : (pr == 1 ? 2 : 0);
        if (mt == 0 && pr == 0) {
#pragma unroll
            for (int p = 0; p < NP; ++p) Bf[p] = *reinterpret_cast<const bf16x8*>(Xb + (p * CH + l31) * PITCH + 16 * ks + 8 * half);
        }
        if (ks == 0 && pr == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
        }
        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Wi[mt][ks][pa], Bf[pb], acc[mt], 0, 0, 0);
    };
    auto store_xp = [&](int buf) {                 // D row = gate column (this wave's 64), D column = step
        float* dst = xps + (buf * CH + l31) * XPP + hw * 64 + 4 * half;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[mt * 32 + (r & 3) + 8 * (r >> 2)] = acc[mt][r];
    };
    // TAIL: the formed chunk at steps [tc, tc + 32) (tc < T, so nothing was clamped): two 16-B stores, and the two rows' mask words
    // from the lanes with tq == 0 / 1 (a null mask: a descriptor of zero bytes, the stores are dropped)
    [[maybe_unused]] auto store_tail = [&](int tc) {
        if constexpr (TAIL) {
            *reinterpret_cast<float4*>(oc + tc) = oa;
            *reinterpret_cast<float4*>(oc + T + tc) = ob;
            const wm_srd_t smask = make_srd(reinterpret_cast<const float*>(tl.mask) + (size_t)b * 64 * (T >> 5),
                                            tl.mask ? (size_t)64 * (T >> 5) * 4 : 0);
            const unsigned ma = mask_merge8(sign_nibble(oa) << (4 * tq)), mb = mask_merge8(sign_nibble(ob) << (4 * tq));
            const unsigned word = (unsigned)(2 * cp + (tq & 1)) * (unsigned)(T >> 5) + (unsigned)(tc >> 5);
            __builtin_amdgcn_raw_buffer_store_b32((tq & 1) ? mb : ma, smask, (int)(tq < 2 ? word * 4u : 0xFFFFFF00u), 0, 0);
        }
    };
    // ---- prologue: projection of chunk 0, x tile of chunk 1 in flight (three barriers, matched by the recurrence waves)
    load_x(0);
    __syncthreads();
    split_x();
    store_tail(0);
    load_x(CH);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 48; ++i) mfma_one(i);
    store_xp(0);
    __syncthreads();
    int cbuf = 0;
    for (int t0 = 0; t0 < T; t0 += CH, cbuf ^= 1) {
#pragma unroll
        for (int s = 0; s < CH; ++s) {
            if (s == 0) { split_x(); load_x(t0 + 2 * CH); }
            if (s >= 1 && s <= 24) { mfma_one(2 * (s - 1)); mfma_one(2 * (s - 1) + 1); }
            if (s == 26) store_xp(cbuf ^ 1);
            if (TAIL && s == 27 && t0 + CH < T) store_tail(t0 + CH);
            if (t0 + s < T) __syncthreads();           // = the barrier of one recurrence step
        }
    }
}

}  // namespace

extern "C" {

#ifdef WM_STAMP
int wm_debug_set_lstm_stamp_buffer(unsigned long long* buf) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_lstm_stamp), &buf, sizeof(buf));
}
#endif

// xp [B,T,256] = x[B,64,T]^T W_ih^T + b_ih + b_hh
int wm_lstm_xproj(const float* x, const float* w_ih, const float* b_ih, const float* b_hh, float* xp, int B, int T,
                  hipStream_t stream) {
    if (T & 3) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(lstm_xproj_kernel, dim3(B * ((T + 127) / 128)), dim3(256), 0, stream, x, w_ih, b_ih, b_hh, xp, T);
    WM_CHECK_LAUNCH();
    return 0;
}

// hout [B,64,T]; gates [B,T,256] and cst [B,T,64] are written only when both are non-NULL (training).
int wm_lstm_fwd(const float* xp, const float* w_hh, float* hout, float* gates, float* cst, int B, int T, hipStream_t stream) {
    if (T & 3) return (int)hipErrorInvalidValue;
    if (gates && cst) hipLaunchKernelGGL(lstm_fwd_kernel<true>, dim3(B), dim3(256), 0, stream, xp, w_hh, hout, gates, cst, T);
    else hipLaunchKernelGGL(lstm_fwd_kernel<false>, dim3(B), dim3(256), 0, stream, xp, w_hh, hout, gates, cst, T);
    WM_CHECK_LAUNCH();
    return 0;
}

static int g_lstm_fwd_ws = 1;       // 1: lstm_fwd_ws_kernel (projection on helper waves) | 0: lstm_fwd_fused_kernel (inside the recurrence's waves)
int wm_set_lstm_fwd_wave_specialised(int on, hipStream_t) { g_lstm_fwd_ws = on ? 1 : 0; return 0; }

// Recurrence with the input projection inside (no xp tensor): x [B,64,T] -> hout; gates / cst as wm_lstm_fwd.
int wm_lstm_fwd_fused(const float* x, const float* w_ih, const float* b_ih, const float* b_hh, const float* w_hh, float* hout,
                      float* gates, float* cst, int B, int T, hipStream_t stream) {
    if ((T & 3) || T < 8) return (int)hipErrorInvalidValue;
    constexpr size_t lds = kLstmFwdLds;
    static wm::DevOnce done[2];
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(lstm_fwd_fused_kernel<true>), lds, done[0])) return rc;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(lstm_fwd_fused_kernel<false>), lds, done[1])) return rc;
    if (g_lstm_fwd_ws) {                            // wave-specialised build: the projection on four helper waves (default)
        static wm::DevOnce donew[2];
        if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(lstm_fwd_ws_kernel<true>), lds, donew[0])) return rc;
        if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(lstm_fwd_ws_kernel<false>), lds, donew[1])) return rc;
        if (gates && cst) hipLaunchKernelGGL(lstm_fwd_ws_kernel<true>, dim3(B), dim3(512), lds, stream, x, w_ih, b_ih, b_hh, w_hh, hout, gates, cst, T, LstmTailArgs<false>{});
        else hipLaunchKernelGGL(lstm_fwd_ws_kernel<false>, dim3(B), dim3(512), lds, stream, x, w_ih, b_ih, b_hh, w_hh, hout, gates, cst, T, LstmTailArgs<false>{});
        WM_CHECK_LAUNCH();
        return 0;
    }
    if (gates && cst) hipLaunchKernelGGL(lstm_fwd_fused_kernel<true>, dim3(B), dim3(256), lds, stream, x, w_ih, b_ih, b_hh, w_hh, hout, gates, cst, T);
    else hipLaunchKernelGGL(lstm_fwd_fused_kernel<false>, dim3(B), dim3(256), lds, stream, x, w_ih, b_ih, b_hh, w_hh, hout, gates, cst, T);
    WM_CHECK_LAUNCH();
    return 0;
}

// wm_lstm_fwd_fused on out = relu(xres + y2 * sc2 + sh2), the tail of the ResBlock in front of the LSTM, which the wave-specialised
// kernel's helper waves form while they stage it: `out` and its sign bits (`mask`, may be null) are written exactly as
// wm_bn_add_relu_mask writes them, hout / gates / cst exactly as wm_lstm_fwd_fused on that out.  Always the wave-specialised build;
// T % 32 != 0 is hipErrorInvalidValue and nothing is written (no fallback inside: the caller keeps the two launches).
int wm_lstm_fwd_tail(const float* xres, const float* y2, const float* sc2, const float* sh2, float* out, void* mask, const float* w_ih,
                     const float* b_ih, const float* b_hh, const float* w_hh, float* hout, float* gates, float* cst, int B, int T,
                     hipStream_t stream) {
    if (B <= 0 || T < 32 || (T & 31) || !xres || !y2 || !sc2 || !sh2 || !out) return (int)hipErrorInvalidValue;
    constexpr size_t lds = kLstmFwdLds;
    static wm::DevOnce done[2];
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(lstm_fwd_ws_kernel<true, true>), lds, done[0])) return rc;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(lstm_fwd_ws_kernel<false, true>), lds, done[1])) return rc;
    const LstmTailArgs<true> tl{y2, sc2, sh2, out, reinterpret_cast<unsigned*>(mask)};
    if (gates && cst) hipLaunchKernelGGL((lstm_fwd_ws_kernel<true, true>), dim3(B), dim3(512), lds, stream, xres, w_ih, b_ih, b_hh, w_hh, hout, gates, cst, T, tl);
    else hipLaunchKernelGGL((lstm_fwd_ws_kernel<false, true>), dim3(B), dim3(512), lds, stream, xres, w_ih, b_ih, b_hh, w_hh, hout, gates, cst, T, tl);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
