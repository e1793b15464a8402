// lstm.hpp's BPTT family: the three backward recurrences (plain, dx inside, wave-specialised with the weight gradients and dx beside it)
#include "lstm.hpp"

namespace {

// ------------------------------------------------------------------------------- recurrence bwd
// gates: in = saved activations, out = pre-activation gradients da  [B,T,256] (column order n' = unit*4 + gate)
__global__ __launch_bounds__(256) void lstm_bwd_kernel(float* __restrict__ gates, const float* __restrict__ cst,
                                                       const float* __restrict__ dh_out, const float* __restrict__ w_hh,
                                                       int T) {
    __builtin_amdgcn_s_setprio(3);   // latency-bound recurrence: win issue arbitration against co-resident weight-gradient waves
    __shared__ __align__(16) float part[2][64][4];  // [buffer][k][wave] partial dh
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane & 3, ul = lane >> 2, u = wave * 16 + ul, np = wave * 64 + lane;
    // transposed-product operand: lane = output k, register j = the gate row held by lane j of this wave
    float wt[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) wt[j] = w_hh[((j & 3) * 64 + wave * 16 + (j >> 2)) * 64 + lane];
    if (tid < 512 / 4) reinterpret_cast<float4*>(&part[0][0][0])[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
    float dc = 0.f;
    // per-step operands through buffer descriptors (scalar step offset + a fixed lane part): no 64-bit address arithmetic
    const wm_srd_t sgb = make_srd(gates + (size_t)b * T * 256, (size_t)T * 256 * sizeof(float));
    const wm_srd_t scb = make_srd(cst + (size_t)b * T * 64, (size_t)T * 64 * sizeof(float));
    const wm_srd_t sdh = make_srd(dh_out + (size_t)b * 64 * T, (size_t)64 * T * sizeof(float));
    const unsigned vgb = (unsigned)np * 4u, vcb = (unsigned)u * 4u, vdh = (unsigned)(u * T) * 4u;

    constexpr int CH = 8;
    struct Buf { float ga[CH], cc[CH + 1], dh[CH]; };
    Buf A, Bf;
    // chunk covers steps t1-CH+1 .. t1 (descending); cc[j] = c_{t1-CH+j} so cc[CH] = c_{t1}.  Loads are unconditional
    // (clamped indices); steps with t < 0 are never executed and c_{-1} is selected to 0 at use.
    auto prefetch = [&](Buf& f, int t1) {
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int t = max(t1 - CH + 1 + j, 0);
            f.ga[j] = buf_load(sgb, vgb, (unsigned)t * 1024u);
            f.dh[j] = buf_load(sdh, vdh, (unsigned)t * 4u);
        }
#pragma unroll
        for (int j = 0; j <= CH; ++j) f.cc[j] = buf_load(scb, vcb, (unsigned)max(t1 - CH + j, 0) * 256u);
    };
    const bool is0 = q == 0, is1 = q == 1, is2 = q == 2, is3 = q == 3;
    int pb = 0;   // partial buffer parity
#ifdef WM_STAMP
    unsigned long long tm[6] = {0, 0, 0, 0, 0, 0};
#endif
    auto run_chunk = [&](const Buf& f, int t1) {
#pragma unroll
        for (int jj = 0; jj < CH; ++jj) {
            const int j = CH - 1 - jj, t = t1 - jj;
            if (t >= 0) {
                LSTAMP(ls0, dc);
                const float4 p = *reinterpret_cast<const float4*>(&part[pb][u][0]);
                // everything that does not need dh of this step first (it overlaps the LDS read above), branch-free: a lane's role
                // (its gate q) only selects operands.  da = base * S * D with  base = dc_t (gates i, f, g) | dh_t (gate o),
                // S = g | c_{t-1} | i | tanh(c_t),  D = a (1 - a) for the sigmoid gates, 1 - a^2 for g  (a = the lane's own activation)
                const float act = f.ga[j];
                const float gi = quad_bcast<0>(act), gf = quad_bcast<1>(act), gg = quad_bcast<2>(act), go = quad_bcast<3>(act);
                const float tc = tanh_s(f.cc[j + 1]);
                const float cprev = (t >= 1) ? f.cc[j] : 0.f;
                const float S = is0 ? gg : (is1 ? cprev : (is2 ? gi : tc));
                const float D = is2 ? fmaf(-act, act, 1.f) : act * (1.f - act);
                const float M = S * D;
                const float K = go * fmaf(-tc, tc, 1.f);
                float dht = f.dh[j] + ((p.x + p.y) + (p.z + p.w));
                LSTAMP(ls1, dht);                          // the four waves' partial dh read back and summed
                const float dct = fmaf(dht, K, dc);
                float da = (is3 ? dht : dct) * M;
                dc = dct * gf;
                LSTAMP(ls2, da);                           // quad exchange, tanh(c), gate derivatives
                buf_store(sgb, da, vgb, (unsigned)t * 1024u);
                // lane k's partial dh[k] over the wave's own 64 gate rows: da row-replicated by three half / row swaps, then 64 products
                // with the DPP row broadcast (no lane reads, no LDS round trip)
                float Dd[4];
                rows_replicate(da, Dd);
                float psum = dot64_rowbcast(Dd, wt);
                LSTAMP(ls3, psum);                         // W_hh^T da over the wave's 64 gate rows (readlane + pk_fma)
                part[pb ^ 1][lane][wave] = psum;
                pb ^= 1;
                LSTAMP(ls4, psum);
                __syncthreads();
                LSTAMP(ls5, dc);
                LSTAMP_ACC(0, ls0, ls1); LSTAMP_ACC(1, ls1, ls2); LSTAMP_ACC(2, ls2, ls3); LSTAMP_ACC(3, ls3, ls4); LSTAMP_ACC(4, ls4, ls5);
            }
        }
    };
    prefetch(A, T - 1);
    __syncthreads();
    for (int t1 = T - 1; t1 >= 0; t1 -= 2 * CH) {
        prefetch(Bf, t1 - CH);
        run_chunk(A, t1);
        prefetch(A, t1 - 2 * CH);
        run_chunk(Bf, t1 - CH);
    }
#ifdef WM_STAMP
    if (g_lstm_stamp && lane == 0) {
        unsigned long long* d = g_lstm_stamp + ((size_t)blockIdx.x * 4 + wave) * 6;
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = tm[i];
    }
#endif
}

// ------------------------------------------------ recurrence bwd with the weight gradients beside it
// Wave-specialised BPTT.  Waves 0..3 run lstm_bwd_kernel's recurrence unchanged (one clip per workgroup, one barrier per step); waves
// 4..7 -- a second wave on each SIMD, whose matrix cores the recurrence never touches -- form the clip's weight gradients
//   dW_ih[n'][c] = sum_t da[t][n'] x[t][c],   dW_hh[n'][k] = sum_t da[t][n'] h[t-1][k]
// out of the 32-step chunk of da the recurrence finished LAST, while it walks the next one: da never has to be read back from HBM
// for them (lstm_wgrad_bf_kernel: 4.2 GB at B = 256, and its A fragments -- 8 consecutive steps of one gate column -- were gathered
// with ds_read_u16 from a [step][n'] image).  Here the recurrence lane that owns gate column n' drops its eight da values of an
// 8-step block as two ds_write_b128 into a [n'][step] fp32 image (double-buffered by chunk); a helper lane reads 8 consecutive steps
// of one column = one A fragment, splits it in registers (bf16x6) and multiplies it with B fragments that come straight from global
// memory (x and h are [B,64,T]: 8 consecutive steps of one channel are contiguous).  Helper wave w owns gate columns [64 w, 64 w + 64)
// for all 128 z rows (128 accumulator registers), 96 MFMAs per chunk = 3 per step.  Helpers execute the recurrence's barrier once
// per step (s_barrier counts every wave of the workgroup) with a 1/32 slice of a chunk's work in between, so they can never run
// behind; the recurrence keeps issue priority (s_setprio 3).  Per-clip slab: [256 n'][128 z] + [256] bias sums (the recurrence lanes
// add their own da), reduced by lstm_wgrad_reduce_kernel.  T % 32 == 0.
//
// DX = true: the input gradient dx[c][t] = sum_n' W_ih[gate_row(n')][c] da[t][n'] is formed here as well, and da is NOT written to
// `gates` (it keeps the saved activations): the [n'][step] image is the only copy of da there ever is.  Helper hw < 2 owns the
// channel half mt = hw of a chunk = one 32 x 32 tile, lstm_dx_bf_kernel's product bit for bit -- the same A fragment (row = channel
// mt*32 + l31, k = 16 ks + 8 half + j) and B fragment (column = step, the same k), the same split3_pair pieces, mfma_bf16x6's product
// order, one accumulator chain from zero over ks = 0..15 ascending (an MFMA output column depends on its own B column only, so a 32-step
// chunk in place of a 64-step tile changes nothing).  The B fragment is gathered from the image with eight ds_read_b32, one per n', and
// split once per k-step; its six products issue one slot later (dx_slot).
// W_ih's pieces (192 registers per tile if resident) live in memory, built by the helper's own lanes in the prologue and only ever read
// back by the lane that wrote them: pieces 0 and 1 in LDS (64 KiB beside the 74 KiB the kernel has already), piece 2 -- one product in
// six -- in the first 16 KiB of the helper's own quarter of the clip's `partial` slab, which is not written until the helper's
// accumulators go out at the very end; it stays in L2 and is fetched three and four slots ahead.
// LDS banks (64 x 4 B): a B-fragment read has lane l31 at float (n' * 36 + l31): 32 consecutive banks per half-wave, and the other half
// is 8 columns = 288 floats = 32 banks further on -- conflict-free.  The W_ih image is [ks][piece][lane] x 16 B, read and written as
// lane-consecutive b128: the canonical conflict-free pattern.
// dynamic LDS: the da image daT [2 chunks][256 n'][pitch 36] fp32 and the partial dh part [2][64][4] fp32; with DX behind them W_ih's
// pieces 0 and 1, [2 helpers][16 ks][2 pieces][64 lanes] x 16 B
constexpr size_t kLstmBwdWsLds = (size_t)(2 * 256 * 36 + 2 * 64 * 4) * sizeof(float);
constexpr size_t kLstmBwdWsDxLds = kLstmBwdWsLds + (size_t)2 * 16 * 2 * 64 * 16;
template <bool DX>
__global__ __launch_bounds__(512) void lstm_bwd_ws_kernel(float* __restrict__ gates, const float* __restrict__ cst,
                                                          const float* __restrict__ dh_out, const float* __restrict__ w_hh,
                                                          const float* __restrict__ x, const float* __restrict__ hseq,
                                                          float* __restrict__ partial, const float* __restrict__ w_ih,
                                                          float* __restrict__ dx, int T) {
    constexpr int CT = 32, PT = 36;                 // chunk length, fp32 pitch of one gate column's chunk (16-byte multiple)
    extern __shared__ __align__(16) unsigned char smem_raw[];
    float* daT = reinterpret_cast<float*>(smem_raw);                      // [2][256][PT]
    float (*part)[64][4] = reinterpret_cast<float (*)[64][4]>(daT + 2 * 256 * PT);     // [2][64][4] partial dh
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* out = partial + (size_t)b * (256 * 128 + 256);
    if (wave < 4) {
        // ------------------------------------------------------------------ the recurrence (lstm_bwd_kernel)
        __builtin_amdgcn_s_setprio(3);
        const int q = lane & 3, ul = lane >> 2, u = wave * 16 + ul, np = wave * 64 + lane;
        float wt[64];
#pragma unroll
        for (int j = 0; j < 64; ++j) wt[j] = w_hh[((j & 3) * 64 + wave * 16 + (j >> 2)) * 64 + lane];
        if (tid < 512 / 4) reinterpret_cast<float4*>(&part[0][0][0])[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
        float dc = 0.f, dbs = 0.f;
        const wm_srd_t sgb = make_srd(gates + (size_t)b * T * 256, (size_t)T * 256 * sizeof(float));
        const wm_srd_t scb = make_srd(cst + (size_t)b * T * 64, (size_t)T * 64 * sizeof(float));
        const wm_srd_t sdh = make_srd(dh_out + (size_t)b * 64 * T, (size_t)64 * T * sizeof(float));
        const unsigned vgb = (unsigned)np * 4u, vcb = (unsigned)u * 4u, vdh = (unsigned)(u * T) * 4u;
        constexpr int CH = 8;
        struct Buf { float ga[CH], cc[CH + 1], dh[CH]; };
        Buf A, Bf;
        auto prefetch = [&](Buf& f, int t1) {
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                const int t = max(t1 - CH + 1 + j, 0);
                f.ga[j] = buf_load(sgb, vgb, (unsigned)t * 1024u);
                f.dh[j] = buf_load(sdh, vdh, (unsigned)t * 4u);
            }
#pragma unroll
            for (int j = 0; j <= CH; ++j) f.cc[j] = buf_load(scb, vcb, (unsigned)max(t1 - CH + j, 0) * 256u);
        };
        const bool is0 = q == 0, is1 = q == 1, is2 = q == 2, is3 = q == 3;
        int pb = 0;
        auto run_chunk = [&](const Buf& f, int t1) {            // t1 % 8 == 7, t1 >= 7 (T % 16 == 0)
            float dav[CH];
#pragma unroll
            for (int jj = 0; jj < CH; ++jj) {
                const int j = CH - 1 - jj, t = t1 - jj;
                const float4 p = *reinterpret_cast<const float4*>(&part[pb][u][0]);
                const float act = f.ga[j];
                const float gi = quad_bcast<0>(act), gf = quad_bcast<1>(act), gg = quad_bcast<2>(act), go = quad_bcast<3>(act);
                const float tc = tanh_s(f.cc[j + 1]);
                const float cprev = (t >= 1) ? f.cc[j] : 0.f;
                const float S = is0 ? gg : (is1 ? cprev : (is2 ? gi : tc));
                const float D = is2 ? fmaf(-act, act, 1.f) : act * (1.f - act);
                const float M = S * D;
                const float K = go * fmaf(-tc, tc, 1.f);
                const float dht = f.dh[j] + ((p.x + p.y) + (p.z + p.w));
                const float dct = fmaf(dht, K, dc);
                const float da = (is3 ? dht : dct) * M;
                dc = dct * gf;
                dav[j] = da;
                if constexpr (!DX) buf_store(sgb, da, vgb, (unsigned)t * 1024u);
                float Dd[4];
                rows_replicate(da, Dd);
                const float psum = dot64_rowbcast(Dd, wt);
                part[pb ^ 1][lane][wave] = psum;
                pb ^= 1;
                if (jj == CH - 1) {                              // the block's eight values, oldest step first: [n'][t % 32 ...]
                    const int t0 = t1 - (CH - 1);
                    float* d = daT + (((t0 >> 5) & 1) * 256 + np) * PT + (t0 & (CT - 1));
                    *reinterpret_cast<float4*>(d) = make_float4(dav[0], dav[1], dav[2], dav[3]);
                    *reinterpret_cast<float4*>(d + 4) = make_float4(dav[4], dav[5], dav[6], dav[7]);
                }
                dbs += da;
                __syncthreads();
            }
        };
        prefetch(A, T - 1);
        __syncthreads();
        for (int t1 = T - 1; t1 >= 0; t1 -= 2 * CH) {
            prefetch(Bf, t1 - CH);
            run_chunk(A, t1);
            prefetch(A, t1 - 2 * CH);
            run_chunk(Bf, t1 - CH);
        }
        out[256 * 128 + np] = dbs;
        return;
    }
    // ---------------------------------------------------------------------- the helpers: weight gradients of the finished chunk
    const int hw = wave - 4, half = lane >> 5, l31 = lane & 31;
    f32x16 acc[2][2][2];                           // [z: x | h][row tile of the wave's 64 gate columns][column tile of 64 channels]
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i >> 2][(i >> 1) & 1][i & 1][r] = 0.f;
    const wm_srd_t sx = make_srd(x + (size_t)b * 64 * T, (size_t)64 * T * sizeof(float));
    const wm_srd_t sh = make_srd(hseq + (size_t)b * 64 * T, (size_t)64 * T * sizeof(float));
    // unit u of a chunk = (ks = u >> 2, z = (u >> 1) & 1, ct = u & 1): the B fragment (z, ct, ks) against both row tiles' A fragments
    // of k-step ks.  Raw operands of unit u + 1 are fetched while unit u multiplies.
    float raw[8];
    auto load_raw = [&](int chunk, int u_) {       // chunk, u_ wave-uniform: the step rides in the scalar offset
        const int ks = u_ >> 2, z = (u_ >> 1) & 1, ct = u_ & 1;
        const unsigned v = (unsigned)((32 * ct + l31) * T + 8 * half) * 4u;
        const int ts = chunk * CT + 16 * ks;
        if (z == 0) {
            const f32x4 a0 = buf_load4(sx, v, (unsigned)ts * 4u), a1 = buf_load4(sx, v, (unsigned)(ts + 4) * 4u);
            raw[0] = a0[0]; raw[1] = a0[1]; raw[2] = a0[2]; raw[3] = a0[3]; raw[4] = a1[0]; raw[5] = a1[1]; raw[6] = a1[2]; raw[7] = a1[3];
        } else {                                    // h[t - 1]: one step earlier (not 16-byte aligned), zero initial state
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int te = ts + e - 1;
                // te = -1 (first step of the clip, wave-uniform): the upper half's lanes want step 7 = voffset - 4, the lower half's h[-1] = 0
                const float r_ = buf_load(sh, te < 0 ? v - 4u : v, (unsigned)max(te, 0) * 4u);
                raw[e] = (te < 0 && half == 0) ? 0.f : r_;
            }
        }
    };
    auto split8 = [&](const float (&v)[8], bf16x8 (&P)[3]) {
        unsigned w_[3][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) split3_pair(v[2 * i], v[2 * i + 1], w_[0][i], w_[1][i], w_[2][i]);
#pragma unroll
        for (int p = 0; p < 3; ++p) P[p] = __builtin_bit_cast(bf16x8, make_uint4(w_[p][0], w_[p][1], w_[p][2], w_[p][3]));
    };
    bf16x8 Af[2][3], Bp[3];
    auto slot = [&](int chunk, int sl) {            // slot sl = 0..31 of the chunk's work; four slots per unit
        const int u_ = sl >> 2, k = sl & 3, ks = u_ >> 2, z = (u_ >> 1) & 1, ct = u_ & 1;
        if (k == 0) {
            if ((u_ & 3) == 0) {                    // new k-step: the two row tiles' A fragments from the [n'][t] image
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    const float* src = daT + ((chunk & 1) * 256 + 64 * hw + 32 * rt + l31) * PT + 16 * ks + 8 * half;
                    const float4 a0 = *reinterpret_cast<const float4*>(src), a1 = *reinterpret_cast<const float4*>(src + 4);
                    const float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                    split8(v, Af[rt]);
                }
            }
            split8(raw, Bp);
            if (u_ < 7) load_raw(chunk, u_ + 1); else load_raw(max(chunk - 1, 0), 0);
            return;
        }
        // k = 1..3: four of the unit's twelve piece products each (bf16x6 order: small terms first)
        constexpr int PA[6] = {1, 0, 2, 0, 1, 0}, PB[6] = {1, 2, 0, 1, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = 4 * (k - 1) + i, rt = m / 6, j = m % 6;
            acc[z][rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Af[rt][PA[j]], Bp[PB[j]], acc[z][rt][ct], 0, 0, 0);
        }
    };
    // ---- DX: the chunk's dx tile on helpers 0 and 1 (hw is wave-uniform; no barrier inside, so the barrier count stays T + 1)
    bf16x8* const wl = reinterpret_cast<bf16x8*>(smem_raw + (2 * 256 * PT + 2 * 64 * 4) * sizeof(float)) + hw * (16 * 2 * 64) + lane;
    // piece 2: [ks][lane] x 16 B at the head of the helper's own quarter of the slab; dx rows of the tile: scalar row and chunk offsets
    const wm_srd_t swg = make_srd(out + hw * (64 * 128), (size_t)16 * 64 * 16);
    const wm_srd_t sdx = make_srd(DX ? dx + ((size_t)b * 64 + hw * 32) * T : nullptr, (size_t)32 * T * sizeof(float));
    const unsigned vdx = (unsigned)(4 * half * T + l31) * 4u;
    bf16x8 Bd[3], A2[2];
    f32x16 dacc;
    if constexpr (DX) {
        if (hw < 2) {
#pragma unroll 2
            for (int ks = 0; ks < 16; ++ks) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = w_ih[gate_row(16 * ks + 8 * half + j) * 64 + hw * 32 + l31];
                bf16x8 P[3];
                split8(v, P);
                wl[(2 * ks) * 64] = P[0];
                wl[(2 * ks + 1) * 64] = P[1];
                buf_store4(swg, __builtin_bit_cast(f32x4, P[2]), (unsigned)lane * 16u, (unsigned)ks * 1024u);
            }
        }
    }
    auto load_a2 = [&](int ks) { return __builtin_bit_cast(bf16x8, buf_load4(swg, (unsigned)lane * 16u, (unsigned)ks * 1024u)); };
    auto dx_gather = [&](int chunk, int ks) {      // the B fragment of k-step ks: this lane's step, eight consecutive n', split once
        const float* src = daT + ((chunk & 1) * 256 + 16 * ks + 8 * half) * PT + l31;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = src[j * PT];
        split8(v, Bd);
    };
    auto dx_mul = [&](int ks, const bf16x8& a2) {   // pieces 0 and 1 read right before their products
        const bf16x8 Ap[3] = {wl[(2 * ks) * 64], wl[(2 * ks + 1) * 64], a2};
        dacc = mfma_bf16x6(Ap, Bd, dacc);
    };
    // Four slots = two k-steps (2g, 2g + 1), dealt around the weight gradients' own pattern (slot k = 0: their splits, no MFMA; k = 1..3:
    // four MFMAs each, no VALU): k = 1 gather + split, k = 2 six products + gather + split, k = 3 six products.  The piece-2 fragments of
    // the NEXT four slots are fetched at k = 3, i.e. before the weight gradients' raw loads of the following k = 0 slot: the memory counter
    // retires in order, and a fetch issued behind those loads (x and h come from HBM) would make its consumer wait for them.
    auto dx_slot = [&](int chunk, int sl) {
        if (hw >= 2) return;
        const int g = sl >> 2, k = sl & 3;
        if (sl == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) dacc[r] = 0.f;
        }
        if (k == 1) dx_gather(chunk, 2 * g);
        if (k == 2) {
            dx_mul(2 * g, A2[0]);
            dx_gather(chunk, 2 * g + 1);
        }
        if (k == 3) {
            dx_mul(2 * g + 1, A2[1]);
            A2[0] = load_a2((2 * g + 2) & 15);     // (the last slot of a chunk fetches k-steps 0 and 1 for the next one)
            A2[1] = load_a2((2 * g + 3) & 15);
            if (sl == CT - 1) {
#pragma unroll
                for (int r = 0; r < 16; ++r) buf_store(sdx, dacc[r], vdx, (unsigned)(mfma_row(r, 0) * T + chunk * CT) * 4u);
            }
        }
    };
    if constexpr (DX) {
        if (hw < 2) {
            A2[0] = load_a2(0);
            A2[1] = load_a2(1);
        }
    }
    const int nch = T / CT;
    load_raw(nch - 1, 0);
    __syncthreads();                                 // the recurrence's start-up barrier
    if constexpr (DX) {
        // the same T barriers as below with the idle first chunk peeled off: a per-slot `if (work)` leaves paths that skip one slot's
        // loads and run the next slot's, and the wait counts the compiler derives for them are needlessly strict
#pragma unroll 1
        for (int sl = 0; sl < CT; ++sl) __syncthreads();
        for (int c = nch - 2; c >= 0; --c) {
#pragma unroll
            for (int sl = 0; sl < CT; ++sl) {
                slot(c + 1, sl);
                dx_slot(c + 1, sl);
                __syncthreads();
            }
        }
    } else
    for (int c = nch - 1; c >= 0; --c) {             // the recurrence walks chunk c; chunk c + 1 is complete
        const bool work = c + 1 < nch;
#pragma unroll
        for (int sl = 0; sl < CT; ++sl) {
            if (work) slot(c + 1, sl);
            __syncthreads();                         // = the barrier of one recurrence step
        }
    }
#pragma unroll
    for (int sl = 0; sl < CT; ++sl) {                // chunk 0, after the recurrence's last step
        slot(0, sl);
        if constexpr (DX) dx_slot(0, sl);
    }
    // the accumulators below overwrite the piece-2 image: every read of it has returned first
    if constexpr (DX) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int z = 0; z < 2; ++z)
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    out[(64 * hw + 32 * rt + mfma_row(r, half)) * 128 + 64 * z + 32 * ct + l31] = acc[z][rt][ct][r];
}

// --------------------------------------------------- recurrence bwd with the input gradient inside
// Same BPTT as lstm_bwd_kernel; in addition dx[b,c,t] = sum_n' w_ih[gate_row(n')][c] da[t][n'] is formed here instead of
// in a separate GEMM over the 4.2-GB da tensor.  Every lane drops the three bf16 pieces of its da into a wave-private
// LDS image [piece][step][gate column] as it produces it; one 32-step chunk later the wave multiplies that image with its
// 64 rows of W_ih^T (A fragments resident in registers) on the bf16 matrix cores -- 48 MFMAs dealt two per step beside
// the VALU recurrence -- and the four waves' partial [64 x 32] tiles are summed through LDS and stored as coalesced rows.
// dynamic LDS: the da images Dab [2][4 waves][3 pieces][32 steps][pitch 72] bf16, then fp32: the partial tiles Pd [4 waves][64][pitch 33],
// the da vectors das [4][64], the partial dh part [2][64][4]
constexpr size_t kLstmBwdFusedLds = (size_t)2 * 4 * 3 * 32 * 72 * 2 + (size_t)(4 * 64 * 33 + 4 * 64 + 2 * 64 * 4) * sizeof(float);
__global__ __launch_bounds__(256) void lstm_bwd_fused_kernel(float* __restrict__ gates, const float* __restrict__ cst,
                                                             const float* __restrict__ dh_out, const float* __restrict__ w_hh,
                                                             const float* __restrict__ w_ih, float* __restrict__ dx, int T) {
    constexpr int HS = WM_LSTM_HS, CHK = 32, PITCH = 72, NP = 3, PDP = 33;
    constexpr int DIMG = NP * CHK * PITCH;                       // bf16 elements of one wave's image
    extern __shared__ __align__(16) unsigned char smem_raw[];
    unsigned short* Dab = reinterpret_cast<unsigned short*>(smem_raw);             // [2][4 waves][NP][CHK][PITCH]
    float* Pd = reinterpret_cast<float*>(Dab + 2 * 4 * DIMG);                       // [4 waves][64][PDP]
    float* das = Pd + 4 * 64 * PDP;                                                 // [4][64] wave-private da vectors
    float* part = das + 4 * 64;                                                     // [2][64][4] partial dh
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int q = lane & 3, ul = lane >> 2, u = wave * 16 + ul, np = wave * 64 + lane;
    v2f wt[32];                                    // transposed W_hh operand: lane = output k, register j = gate row of lane j
#pragma unroll
    for (int j = 0; j < 64; j += 2)
        wt[j / 2] = v2f{w_hh[((j & 3) * 64 + wave * 16 + (j >> 2)) * 64 + lane],
                        w_hh[(((j + 1) & 3) * 64 + wave * 16 + ((j + 1) >> 2)) * 64 + lane]};
    // W_ih^T A fragments: A[i = channel mt*32 + l31][k = this wave's gate column 16 ks + 8 half + j]
    bf16x8 Wt[2][4][NP];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = w_ih[gate_row(wave * 64 + 16 * ks + 8 * half + j) * 64 + mt * 32 + l31];
            unsigned a[4], m[4], l[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) split3_pair(v[2 * j], v[2 * j + 1], a[j], m[j], l[j]);
            Wt[mt][ks][0] = __builtin_bit_cast(bf16x8, make_uint4(a[0], a[1], a[2], a[3]));
            Wt[mt][ks][1] = __builtin_bit_cast(bf16x8, make_uint4(m[0], m[1], m[2], m[3]));
            Wt[mt][ks][2] = __builtin_bit_cast(bf16x8, make_uint4(l[0], l[1], l[2], l[3]));
        }
    if (tid < 128) reinterpret_cast<float4*>(part)[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
    float dc = 0.f;
    float* gb = gates + (size_t)b * T * 256 + np;
    const float* cb = cst + (size_t)b * T * 64 + u;
    const float* dhb = dh_out + ((size_t)b * 64 + u) * T;

    constexpr int CH = 8;
    struct Buf { float ga[CH], cc[CH + 1], dh[CH]; };
    Buf A, Bf;
    auto prefetch = [&](Buf& f, int t1) {          // steps t1-CH+1 .. t1; unconditional loads from clamped indices
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int t = max(t1 - CH + 1 + j, 0);
            f.ga[j] = gb[(size_t)t * 256];
            f.dh[j] = dhb[t];
        }
#pragma unroll
        for (int j = 0; j <= CH; ++j) f.cc[j] = cb[(size_t)max(t1 - CH + j, 0) * 64];
    };
    f32x16 acc[2];
    bf16x8 Bq[NP];
    int ibuf = 0;                                  // image being filled by the current 32-step chunk
    // idx-th of the 48 MFMAs of the previous chunk's product (block idx / 6 = ks*2 + mt, piece product idx % 6), issued one
    // at a time and far apart: see lstm_fwd_fused_kernel
    auto mfma_one = [&](int idx, int img) {
        const int m = idx / 6, pr = idx % 6, ks = m >> 1, mt = m & 1;
        const int pa = (pr == 0 || pr == 4) ? 1 : (pr == 2 ? 2 : 0), pbi = (pr == 0 || pr == 3) ? 1 : (pr == 1 ? 2 : 0);
        const unsigned short* im = Dab + (img * 4 + wave) * DIMG;
        if (mt == 0 && pr == 0) {
#pragma unroll
            for (int p = 0; p < NP; ++p) Bq[p] = *reinterpret_cast<const bf16x8*>(im + (p * CHK + l31) * PITCH + 16 * ks + 8 * half);
        }
        if (ks == 0 && pr == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
        }
        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Wt[mt][ks][pa], Bq[pbi], acc[mt], 0, 0, 0);
    };
    auto store_partial = [&]() {                   // D row = channel, D column = step of the chunk
        float* dst = Pd + (wave * 64 + 4 * half) * PDP + l31;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[(mt * 32 + (r & 3) + 8 * (r >> 2)) * PDP] = acc[mt][r];
    };
    auto reduce_store = [&](int tlo) {             // thread -> channel tid>>2, 8 steps from 8*(tid&3)
        const int ch = tid >> 2, j0 = 8 * (tid & 3);
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = ch * PDP + j0 + j;
            o[j] = (Pd[i] + Pd[64 * PDP + i]) + (Pd[2 * 64 * PDP + i] + Pd[3 * 64 * PDP + i]);
        }
        float* dst = dx + ((size_t)b * 64 + ch) * T + tlo + j0;
        if (tlo + j0 >= 0) *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        if (tlo + j0 + 4 >= 0) *reinterpret_cast<float4*>(dst + 4) = make_float4(o[4], o[5], o[6], o[7]);
    };
    int pb = 0;   // partial buffer parity
    int prev_tlo = 0;
    bool have_prev = false;
    // SUB = 8-step quarter of the 32-step chunk whose top step is t1 + 8*SUB
    auto run_chunk = [&](const Buf& f, int t1, auto sub_c) {
        constexpr int SUB = decltype(sub_c)::value;
        unsigned short* myimg = Dab + (ibuf * 4 + wave) * DIMG;
#pragma unroll
        for (int jj = 0; jj < CH; ++jj) {
            const int j = CH - 1 - jj, t = t1 - jj;
            constexpr int dummy = 0; (void)dummy;
            const int s32 = SUB * 8 + jj, tt = 31 - s32;   // position in the chunk: time = tlo + tt
            // ---- side work for the previous chunk (its image is complete)
            if (have_prev) {
                if (s32 >= 2 && s32 < 26) mfma_one(2 * (s32 - 2), ibuf ^ 1);
                if (s32 == 26) store_partial();
                if (s32 == 27) { __syncthreads(); reduce_store(prev_tlo); }
            }
            if (t >= 0) {
                const float4 p = *reinterpret_cast<const float4*>(part + (pb * 64 + u) * 4);
                const float dht = f.dh[j] + ((p.x + p.y) + (p.z + p.w));
                const float act = f.ga[j];
                const float gi = quad_bcast<0>(act), gf = quad_bcast<1>(act), gg = quad_bcast<2>(act), go = quad_bcast<3>(act);
                const float tc = tanh_s(f.cc[j + 1]);
                const float cprev = (t >= 1) ? f.cc[j] : 0.f;
                const float dct = fmaf(dht * go, 1.f - tc * tc, dc);
                float da;
                if (q == 0) da = dct * gg * gi * (1.f - gi);
                else if (q == 1) da = dct * cprev * gf * (1.f - gf);
                else if (q == 2) da = dct * gi * (1.f - gg * gg);
                else da = dht * tc * go * (1.f - go);
                dc = dct * gf;
                gb[(size_t)t * 256] = da;
                das[wave * 64 + lane] = da;                 // same wave reads it back: no barrier needed
                __builtin_amdgcn_wave_barrier();
                const float4* dp = reinterpret_cast<const float4*>(das + wave * 64);
                float4 dq[(64 - HS) / 4];
#pragma unroll
                for (int k = 0; k < (64 - HS) / 4; ++k) dq[k] = dp[HS / 4 + k];
                {   // under the latency of those reads: bf16 pieces of da for the dx product, [piece][step tt][gate column]
                    unsigned p0, p1, p2;
                    split3_pair(da, 0.f, p0, p1, p2);
                    unsigned short* d = myimg + tt * PITCH + lane;
                    d[0] = (unsigned short)p0; d[CHK * PITCH] = (unsigned short)p1; d[2 * CHK * PITCH] = (unsigned short)p2;
                }
                v2f a01 = v2f{0.f, 0.f}, a23 = a01;
                // two batches of 32 lane reads, each ahead of its 16 products (64 scalar registers at once would not fit beside the rest)
#pragma unroll
                for (int k0 = 0; k0 < HS; k0 += 32) {
                    constexpr int NB = HS < 32 ? HS : 32;
                    unsigned long long dp[NB / 2];
                    lanes_to_sgprs<NB>(da, k0, dp);
#pragma unroll
                    for (int k = 0; k < NB; k += 4) {
                        a01 = pk_fma_s(wt[(k0 + k) / 2], dp[k / 2], a01);
                        a23 = pk_fma_s(wt[(k0 + k) / 2 + 1], dp[k / 2 + 1], a23);
                    }
                }
#pragma unroll
                for (int k = 0; k < (64 - HS) / 4; ++k) {
                    const float4 d = dq[k];
                    a01 = __builtin_elementwise_fma(wt[HS / 2 + 2 * k], v2f{d.x, d.y}, a01);
                    a23 = __builtin_elementwise_fma(wt[HS / 2 + 2 * k + 1], v2f{d.z, d.w}, a23);
                }
                const v2f sm = a01 + a23;
                part[((pb ^ 1) * 64 + lane) * 4 + wave] = sm.x + sm.y;
                pb ^= 1;
                if (have_prev && s32 >= 2 && s32 < 26) mfma_one(2 * (s32 - 2) + 1, ibuf ^ 1);
                __syncthreads();
            } else {
                // steps before the clip: zero pieces so that the partial last chunk multiplies zeros
                unsigned short* d = myimg + tt * PITCH + lane;
                d[0] = 0; d[CHK * PITCH] = 0; d[2 * CHK * PITCH] = 0;
                if (have_prev && s32 >= 2 && s32 < 26) mfma_one(2 * (s32 - 2) + 1, ibuf ^ 1);
            }
        }
    };
    prefetch(A, T - 1);
    __syncthreads();
    for (int t1 = T - 1; t1 >= 0; t1 -= CHK) {
        prefetch(Bf, t1 - CH);
        run_chunk(A, t1, std::integral_constant<int, 0>{});
        prefetch(A, t1 - 2 * CH);
        run_chunk(Bf, t1 - CH, std::integral_constant<int, 1>{});
        prefetch(Bf, t1 - 3 * CH);
        run_chunk(A, t1 - 2 * CH, std::integral_constant<int, 2>{});
        prefetch(A, t1 - 4 * CH);
        run_chunk(Bf, t1 - 3 * CH, std::integral_constant<int, 3>{});
        prev_tlo = t1 - (CHK - 1);
        have_prev = true;
        ibuf ^= 1;
    }
    // flush: the last chunk's product
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 48; ++i) mfma_one(i, ibuf ^ 1);
    store_partial();
    __syncthreads();
    reduce_store(prev_tlo);
}

}  // namespace

extern "C" {

#ifdef WM_STAMP
// this unit's copy of g_lstm_stamp (lstm_bwd_kernel's stamps); wm_debug_set_lstm_stamp_buffer is lstm_fwd.hip's
int wm_debug_set_lstm_stamp_buffer_bwd(unsigned long long* buf) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_lstm_stamp), &buf, sizeof(buf));
}
#endif

// gates: saved activations in, da out.  dh_out [B,64,T] = gradient w.r.t. hout.
int wm_lstm_bwd(float* gates, const float* cst, const float* dh_out, const float* w_hh, int B, int T, hipStream_t stream) {
    hipLaunchKernelGGL(lstm_bwd_kernel, dim3(B), dim3(256), 0, stream, gates, cst, dh_out, w_hh, T);
    WM_CHECK_LAUNCH();
    return 0;
}

// BPTT + input gradient in one launch (no separate pass over da for dx): gates in = saved activations, out = da.
int wm_lstm_bwd_fused(float* gates, const float* cst, const float* dh_out, const float* w_hh, const float* w_ih, float* dx,
                      int B, int T, hipStream_t stream) {
    if ((T & 3) || T < 4) return (int)hipErrorInvalidValue;
    constexpr size_t lds = kLstmBwdFusedLds;
    static wm::DevOnce done;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(lstm_bwd_fused_kernel), lds, done)) return rc;
    hipLaunchKernelGGL(lstm_bwd_fused_kernel, dim3(B), dim3(256), lds, stream, gates, cst, dh_out, w_hh, w_ih, dx, T);
    WM_CHECK_LAUNCH();
    return 0;
}

// BPTT + the clip's weight gradients in one launch (wave-specialised: see lstm_bwd_ws_kernel), then the fixed-order reduction
// over clips.  gates: saved activations in, da out (for wm_lstm_dx).  partial: >= B * (256*128 + 256) floats.  T % 32 == 0, T >= 64.
int wm_lstm_bwd_wgrad(float* gates, const float* cst, const float* dh_out, const float* w_hh, const float* x, const float* h,
                      float* partial, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, int B, int T, int accumulate,
                      hipStream_t stream) {
    if (B <= 0 || (T & 31) || T < 64) return (int)hipErrorInvalidValue;
    constexpr size_t lds = kLstmBwdWsLds;
    static wm::DevOnce done;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(lstm_bwd_ws_kernel<false>), lds, done)) return rc;
    hipLaunchKernelGGL(lstm_bwd_ws_kernel<false>, dim3(B), dim3(512), lds, stream, gates, cst, dh_out, w_hh, x, h, partial,
                       (const float*)nullptr, (float*)nullptr, T);
    WM_CHECK_LAUNCH();
    hipLaunchKernelGGL(lstm_wgrad_reduce_kernel, dim3(kWgradSlab / 64), dim3(512), 0, stream, (const float*)partial, B,
                       dw_ih, dw_hh, db_ih, db_hh, accumulate);
    WM_CHECK_LAUNCH();
    return 0;
}

// wm_lstm_bwd_wgrad + wm_lstm_dx in one launch: helpers 0 and 1 also form dx from the LDS image of da (lstm_bwd_ws_kernel<true>), bit
// for bit wm_lstm_dx's bf16x6 result; da is never written, gates keeps the saved activations.  partial must be 16-byte aligned (each
// clip's slab holds W_ih's third piece, 2 x 16 KiB, until the slab's own values replace it).  Under wm_set_lstm_dx_bf16x6(0) there
// is no such kernel: a const-cast of gates and the two launches (gates then holds da, as after wm_lstm_bwd_wgrad).
int wm_lstm_bwd_wgrad_dx(const float* gates, const float* cst, const float* dh_out, const float* w_hh, const float* w_ih,
                         const float* x, const float* h, float* partial, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh,
                         float* dx, int B, int T, int accumulate, hipStream_t stream) {
    if (B <= 0 || (T & 31) || T < 64 || !dx || !w_ih || (reinterpret_cast<uintptr_t>(partial) & 15)) return (int)hipErrorInvalidValue;
    if (!wm::lstm_dx_bf16x6()) {
        if (int rc = wm_lstm_bwd_wgrad(const_cast<float*>(gates), cst, dh_out, w_hh, x, h, partial, dw_ih, dw_hh, db_ih, db_hh, B, T,
                                       accumulate, stream))
            return rc;
        return wm_lstm_dx(gates, w_ih, dx, B, T, stream);
    }
    constexpr size_t lds = kLstmBwdWsDxLds;
    static wm::DevOnce done;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(lstm_bwd_ws_kernel<true>), lds, done)) return rc;
    hipLaunchKernelGGL(lstm_bwd_ws_kernel<true>, dim3(B), dim3(512), lds, stream, const_cast<float*>(gates), cst, dh_out, w_hh, x, h,
                       partial, w_ih, dx, T);
    WM_CHECK_LAUNCH();
    hipLaunchKernelGGL(lstm_wgrad_reduce_kernel, dim3(kWgradSlab / 64), dim3(512), 0, stream, (const float*)partial, B,
                       dw_ih, dw_hh, db_ih, db_hh, accumulate);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
