// nn.LSTM(hd, hd, num_layers=2) over the T = 50 latent steps (py/main14b_2.py:137, :165): the recurrence of ONE layer as
// a chain of per-step launches issued back to back by the C launcher (no host work between them; the kernel boundary is
// the step barrier, so no grid-wide spin and nothing that can hang).  Layouts: time-major, batch contiguous.
// The batch-major <-> time-major permute around it lives here too, this LSTM being its only use.  (The other models' LSTM, lstm.hpp
// and its three units, shares nothing with this one: DESIGN.md sections 4p, 4q.)
#include "wm_common.hpp"
using namespace wm;

namespace {

// forward step:  gates[q*H + u][b] = xp[q*H + u][b] + sum_k W_hh[q*H + u][k] * h_prev[k][b];  cell update.
//   workgroup = 8 units x 4 gates (32 gate rows) x 32 batch columns; its 4 waves split the contraction (K = H): lane
//   (i, half) of wave w owns k = w*H/4 + half*H/8 + s, s < H/8 -- a contiguous run of ITS weight row, so the A operand is
//   H/32 float4 loads straight from the PyTorch weight (no transpose, no LDS); the B operand rows are 128-byte coalesced.
//   All loads are issued up front, then H/8 MFMAs per wave; partial tiles are summed through LDS in wave order.
__global__ __launch_bounds__(256) void lstm_seq_fwd_kernel(const float* xp, const float* __restrict__ whh,
                                                           const float* __restrict__ hprev, const float* __restrict__ cprev,
                                                           float* __restrict__ hout, float* __restrict__ cout, float* gates_out,
                                                           int H, int Bn) {
    constexpr int MAXS = 32;                     // H/8 <= 32  (H <= 256)
    __shared__ float red[4][16][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int u0 = blockIdx.x * 8, b0 = blockIdx.y * 32;
    const int SL = H >> 3;                       // contraction values per lane
    const int grow = (l31 >> 3) * H + u0 + (l31 & 7);                  // this lane's gate row (A operand row)
    const int kbase = wave * (H >> 2) + half * SL;
    const int bcol = min(b0 + l31, Bn - 1);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (hprev) {
        f32x4 a4[MAXS / 4];
        float bv[MAXS];
        const float* wr = whh + (size_t)grow * H + kbase;
#pragma unroll
        for (int i = 0; i < MAXS / 4; ++i)
            if (4 * i < SL) a4[i] = *reinterpret_cast<const f32x4*>(wr + 4 * i);
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s < SL) bv[s] = hprev[(size_t)(kbase + s) * Bn + bcol];
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s < SL) acc = mfma32(a4[s >> 2][s & 3], bv[s], acc);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[r];
    __syncthreads();
    // cell update: thread = (unit, batch column); gate q of unit u is tile row q*8 + u = register (row&3) + 4*((row>>3)&3)... of lane half
    const int u = tid >> 5, bl = tid & 31, b = b0 + bl;
    if (b >= Bn) return;
    float pre[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = q * 8 + u;               // D row = (r&3) + 8*(r>>2) + 4*half
        const int hf = (row >> 2) & 1, r = (row & 3) + 4 * (row >> 3);
        const int ln = hf * 32 + bl;
        pre[q] = ((red[0][r][ln] + red[1][r][ln]) + red[2][r][ln]) + red[3][r][ln] + xp[(size_t)(q * H + u0 + u) * Bn + b];
    }
    const float gi = 1.f / (1.f + expf(-pre[0])), gf = 1.f / (1.f + expf(-pre[1])), gg = tanhf(pre[2]), go = 1.f / (1.f + expf(-pre[3]));
    const size_t o = (size_t)(u0 + u) * Bn + b;
    const float cp = cprev ? cprev[o] : 0.f;
    const float c = gf * cp + gi * gg;
    hout[o] = go * tanhf(c);
    cout[o] = c;
    if (gates_out) {
        gates_out[(size_t)(0 * H + u0 + u) * Bn + b] = gi; gates_out[(size_t)(1 * H + u0 + u) * Bn + b] = gf;
        gates_out[(size_t)(2 * H + u0 + u) * Bn + b] = gg; gates_out[(size_t)(3 * H + u0 + u) * Bn + b] = go;
    }
}

// backward step:  dh[u][b] = dout[u][b] + sum_g W_hh[g][u] * da_next[g][b]  (K = 4H), then the pointwise gate backward:
//   gates (activations) -> da (in place), dc (in/out).  Workgroup = 16 units x 16 batch columns (fp32 MFMA 16x16x4), its 4
//   waves split K; lane (i, kq) of wave w owns g = w*H + kq*H/4 + s, s < H/4 -- contiguous in the TRANSPOSED weight whhT
//   [H][4H] (float4 loads); the B operand rows are 64-byte segments of da_next.
__global__ __launch_bounds__(256) void lstm_seq_bwd_kernel(float* gates, const float* __restrict__ danext, const float* __restrict__ whhT,
                                                           const float* __restrict__ c, const float* __restrict__ cprev,
                                                           const float* __restrict__ dout, float* __restrict__ dc, int H, int Bn) {
    constexpr int MAXS = 64;                     // H/4 <= 64
    __shared__ float red[4][4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4, l15 = lane & 15;
    const int u0 = blockIdx.x * 16, b0 = blockIdx.y * 16;
    const int SL = H >> 2;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (danext) {
        const int gbase = wave * H + kq * SL;
        const int bcol = min(b0 + l15, Bn - 1);
        const float* wr = whhT + (size_t)(u0 + l15) * 4 * H + gbase;
        f32x4 a4[MAXS / 4];
        float bv[MAXS];
#pragma unroll
        for (int i = 0; i < MAXS / 4; ++i)
            if (4 * i < SL) a4[i] = *reinterpret_cast<const f32x4*>(wr + 4 * i);
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s < SL) bv[s] = danext[(size_t)(gbase + s) * Bn + bcol];
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s < SL) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[s >> 2][s & 3], bv[s], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][r][lane] = acc[r];
    __syncthreads();
    const int ul = tid >> 4, bl = tid & 15, b = b0 + bl;       // D: col = lane&15, row = (lane>>4)*4 + reg
    if (b >= Bn) return;
    const int r = ul & 3, ln = (ul >> 2) * 16 + bl;
    const size_t o = (size_t)(u0 + ul) * Bn + b, hb = (size_t)H * Bn;
    const float dht = ((red[0][r][ln] + red[1][r][ln]) + red[2][r][ln]) + red[3][r][ln] + dout[o];
    const float gi = gates[o], gf = gates[hb + o], gg = gates[2 * hb + o], go = gates[3 * hb + o];
    const float tc = tanhf(c[o]);
    const float dct = dc[o] + dht * go * (1.f - tc * tc);
    const float cp = cprev ? cprev[o] : 0.f;
    gates[o] = dct * gg * gi * (1.f - gi);
    gates[hb + o] = dct * cp * gf * (1.f - gf);
    gates[2 * hb + o] = dct * gi * (1.f - gg * gg);
    gates[3 * hb + o] = dht * tc * go * (1.f - go);
    dc[o] = dct * gf;
}

// [A][C][L] -> [L][C][A]   (batch-major <-> time-major sequence layouts around the LSTM)
__global__ void permute_acl_kernel(const float* __restrict__ x, float* __restrict__ y, int A, int C, int L) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)A * C * L) return;
    const int l = (int)(i % L), c = (int)((i / L) % C), aa = (int)(i / ((size_t)L * C));
    y[((size_t)l * C + c) * A + aa] = x[i];
}

}  // namespace

extern "C" {

// One layer of nn.LSTM(H, H) over T steps, zero initial state (py/main14b_2.py:165).  xp [T][4H][B] = W_ih x_t + b_ih + b_hh
// (overwritten in place by the gate activations when save != 0 -- what wm_lstm_seq_bwd consumes); whh = weight_hh [4H][H];
// hs, cs [T+1][H][B] with hs[0] / cs[0] = 0 provided by the caller: h_t = hs[t+1].  T launches, issued back to back.
int wm_lstm_seq_fwd(float* xp, const float* whh, float* hs, float* cs, int T, int H, int B, int save, hipStream_t stream) {
    if (T <= 0 || H <= 0 || (H & 31) || H > 256 || B <= 0) return (int)hipErrorInvalidValue;
    const size_t hb = (size_t)H * B;
    dim3 grid(H / 8, (B + 31) / 32);
    for (int t = 0; t < T; ++t) {
        float* g = xp + (size_t)t * 4 * hb;
        hipLaunchKernelGGL(lstm_seq_fwd_kernel, grid, dim3(256), 0, stream, g, whh, t ? hs + (size_t)t * hb : nullptr,
                           t ? cs + (size_t)t * hb : nullptr, hs + (size_t)(t + 1) * hb, cs + (size_t)(t + 1) * hb, save ? g : nullptr, H, B);
    }
    WM_CHECK_LAUNCH();
    return 0;
}

// BPTT of that layer: gates [T][4H][B] (activations in, pre-activation gradients da out, in place), cs as written by the
// forward, dout [T][H][B] = dL/dh_t from above, whhT = weight_hh^T [H][4H], dc [H][B] scratch (zeroed here).  T launches.
int wm_lstm_seq_bwd(float* gates, const float* cs, const float* dout, const float* whhT, float* dc, int T, int H, int B,
                    hipStream_t stream) {
    if (T <= 0 || H <= 0 || (H & 31) || H > 256 || B <= 0) return (int)hipErrorInvalidValue;
    const size_t hb = (size_t)H * B;
    WM_TRY(hipMemsetAsync(dc, 0, hb * sizeof(float), stream));
    dim3 grid(H / 16, (B + 15) / 16);
    for (int t = T - 1; t >= 0; --t) {
        hipLaunchKernelGGL(lstm_seq_bwd_kernel, grid, dim3(256), 0, stream, gates + (size_t)t * 4 * hb,
                           t + 1 < T ? gates + (size_t)(t + 1) * 4 * hb : nullptr, whhT, cs + (size_t)(t + 1) * hb,
                           t ? cs + (size_t)t * hb : nullptr, dout + (size_t)t * hb, dc, H, B);
    }
    WM_CHECK_LAUNCH();
    return 0;
}

int wm_permute_acl(const float* x, float* y, int A, int C, int L, hipStream_t stream) {
    const size_t n = (size_t)A * C * L;
    hipLaunchKernelGGL(permute_acl_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, y, A, C, L);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
