// lstm.hpp's non-sequential gradient GEMMs: dx and the weight gradients over a finished da, fp32 and bf16x6
#include "lstm.hpp"

namespace {

// ------------------------------------------------------------------------------------ dx GEMM
// dx[b,c,t] = sum_n da[b,t,n'] w_ih[gate_row(n')][c] ;  persistent blocks over (clip, 64-step) tiles, the next da
// tile is fetched into registers while the matrix cores work on the current one; wave = (c half, t half)
// dynamic LDS: the W_ih image ws [256 n'][64] and the da tile ds [64 steps][pitch 257], fp32
constexpr size_t kLstmDxLds = (size_t)(256 * 64 + 64 * 257) * sizeof(float);
__global__ __launch_bounds__(256) void lstm_dx_kernel(const float* __restrict__ da, const float* __restrict__ w_ih,
                                                      float* __restrict__ dx, int B, int T) {
    constexpr int NT = 64, DS = 257;
    extern __shared__ __align__(16) float smem[];
    float* ws = smem;               // [256][64]  A[i = c][k = n'] = w_ih[gate_row(n')][c]
    float* ds = smem + 256 * 64;    // [NT][DS]   B[k = n'][j = t] = da[t][n']
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int tilesPerClip = (T + NT - 1) / NT, ntiles = B * tilesPerClip;
    for (int i = tid; i < 256 * 16; i += 256)      // row n' of the LDS image = parameter row gate_row(n')
        reinterpret_cast<float4*>(ws)[i] = reinterpret_cast<const float4*>(w_ih)[gate_row(i >> 4) * 16 + (i & 15)];
    float4 st[16];
    auto load_piece = [&](int tile, int k) {       // branch-free: rows past T read a clamped row, never stored
        const int b = tile / tilesPerClip, t0 = (tile % tilesPerClip) * NT;
        const int i = tid + k * 256;
        st[k] = reinterpret_cast<const float4*>(da + (size_t)b * T * 256)[(size_t)min(t0 + (i >> 6), T - 1) * 64 + (i & 63)];
    };
    auto load_tile = [&](int tile) {
#pragma unroll
        for (int k = 0; k < 16; ++k) load_piece(tile, k);
    };
    auto write_tile = [&]() {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int i = tid + k * 256;
            float* d = ds + (i >> 6) * DS + 4 * (i & 63);
            d[0] = st[k].x; d[1] = st[k].y; d[2] = st[k].z; d[3] = st[k].w;
        }
    };
    int tile = blockIdx.x;
    if (tile < ntiles) load_tile(tile);
    __syncthreads();
    if (tile < ntiles) write_tile();
    __syncthreads();
    const int mt = wave & 1, nt = wave >> 1;
    const float* ap = ws + half * 64 + mt * 32 + l31;
    const float* bp = ds + (nt * 32 + l31) * DS + half;
    while (tile < ntiles) {
        const int next = tile + gridDim.x, nextc = min(next, ntiles - 1);     // clamped: loaded (valid memory), never written
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int g8 = 0; g8 < 16; ++g8) {              // the next tile's 64 KB arrive one piece per 8 MFMAs, not as one burst
            load_piece(nextc, g8);
#pragma unroll
            for (int s = 8 * g8; s < 8 * g8 + 8; ++s) acc = mfma32(ap[2 * s * 64], bp[2 * s], acc);
        }
        const int b = tile / tilesPerClip, t0 = (tile % tilesPerClip) * NT;
        const int t = t0 + nt * 32 + l31;
        if (t < T) {
#pragma unroll
            for (int r = 0; r < 16; ++r) dx[((size_t)b * 64 + mt * 32 + mfma_row(r, half)) * T + t] = acc[r];
        }
        __syncthreads();
        if (next < ntiles) write_tile();
        __syncthreads();
        tile = next;
    }
}

// ------------------------------------------------------------------------------------ dx GEMM, bf16x6
// Same product as lstm_dx_kernel on the bf16 matrix cores (bf16x6 split, fp32-grade).  The contraction runs over the gate
// column n', which is the contiguous axis of da [t][n']: a B fragment (one time step, 8 consecutive n') is one aligned
// ds_read_b128 of the 3-piece LDS image of the tile, no transposition.  W_ih^T lives in registers as A fragments
// (16 k-steps x 3 pieces = 192 VGPRs for this wave's 32 channels).  Wave = (channel half mt, time half nt) of a 64-step tile.
// dynamic LDS: the da image Db [3 pieces][64 steps][pitch 264] bf16
constexpr size_t kLstmDxBfLds = (size_t)3 * 64 * 264 * 2;
__global__ __launch_bounds__(256) void lstm_dx_bf_kernel(const float* __restrict__ da, const float* __restrict__ w_ih,
                                                         float* __restrict__ dx, int B, int T) {
    constexpr int NT = 64, NP = 3, PD = 264;         // image row pitch in bf16 (528 B = 33 x 16 B)
    extern __shared__ __align__(16) unsigned char smem_raw[];
    unsigned short* Db = reinterpret_cast<unsigned short*>(smem_raw);          // [NP][NT][PD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int mt = wave & 1, nt = wave >> 1;
    const int tilesPerClip = (T + NT - 1) / NT, ntiles = B * tilesPerClip;
    // A[i = channel mt*32 + l31][k = n' = 16 ks + 8 half + j] = w_ih[gate_row(n')][channel]
    bf16x8 Wt[16][NP];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = w_ih[gate_row(16 * ks + 8 * half + j) * 64 + mt * 32 + l31];
        unsigned a[4], m[4], l[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) split3_pair(v[2 * j], v[2 * j + 1], a[j], m[j], l[j]);
        Wt[ks][0] = __builtin_bit_cast(bf16x8, make_uint4(a[0], a[1], a[2], a[3]));
        Wt[ks][1] = __builtin_bit_cast(bf16x8, make_uint4(m[0], m[1], m[2], m[3]));
        Wt[ks][2] = __builtin_bit_cast(bf16x8, make_uint4(l[0], l[1], l[2], l[3]));
    }
    float4 st[16];
    auto load_piece = [&](int tile, int k) {       // branch-free: rows past T read a clamped row, never stored
        const int b = tile / tilesPerClip, t0 = (tile % tilesPerClip) * NT;
        const int i = tid + k * 256;
        st[k] = reinterpret_cast<const float4*>(da + (size_t)b * T * 256)[(size_t)min(t0 + (i >> 6), T - 1) * 64 + (i & 63)];
    };
    auto write_tile = [&]() {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int i = tid + k * 256;
            unsigned a0, a1, a2, b0, b1, b2;
            split3_pair(st[k].x, st[k].y, a0, a1, a2);
            split3_pair(st[k].z, st[k].w, b0, b1, b2);
            unsigned short* d = Db + (i >> 6) * PD + 4 * (i & 63);
            *reinterpret_cast<uint2*>(d) = make_uint2(a0, b0);
            *reinterpret_cast<uint2*>(d + NT * PD) = make_uint2(a1, b1);
            *reinterpret_cast<uint2*>(d + 2 * NT * PD) = make_uint2(a2, b2);
        }
    };
    int tile = blockIdx.x;
#pragma unroll
    for (int k = 0; k < 16; ++k) load_piece(min(tile, ntiles - 1), k);
    __syncthreads();
    write_tile();
    __syncthreads();
    const unsigned short* brow = Db + (nt * 32 + l31) * PD + 8 * half;
    while (tile < ntiles) {
        const int next = tile + gridDim.x, nextc = min(next, ntiles - 1);     // clamped: loaded (valid memory), never written
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            bf16x8 Bf[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) Bf[p] = *reinterpret_cast<const bf16x8*>(brow + p * NT * PD + 16 * ks);
            acc = mfma_bf16x6(Wt[ks], Bf, acc);
            load_piece(nextc, ks);                 // the next tile's 64 KB arrive one piece per k-step
        }
        const int b = tile / tilesPerClip, t0 = (tile % tilesPerClip) * NT;
        const int t = t0 + nt * 32 + l31;
        if (t < T) {
#pragma unroll
            for (int r = 0; r < 16; ++r) dx[((size_t)b * 64 + mt * 32 + mfma_row(r, half)) * T + t] = acc[r];
        }
        __syncthreads();
        if (next < ntiles) write_tile();
        __syncthreads();
        tile = next;
    }
}

// ---------------------------------------------------------------------------------- wgrad GEMM
// G[n'][j] = sum_{b,t} da[b,t,n'] * z[b,j,t],  z = [x (64 rows) ; h shifted by one step (64 rows)]
// persistent blocks over (clip, 64-step) tiles, next tile prefetched into registers during the MFMA phase;
// partial[block][256*128 + 256 (bias)]
// dynamic LDS: the da tile ds [64 steps][256] and the z tile zs [128 rows][pitch 67], fp32
constexpr size_t kLstmWgradLds = (size_t)(64 * 256 + 128 * 67) * sizeof(float);
__global__ __launch_bounds__(256) void lstm_wgrad_kernel(const float* __restrict__ da, const float* __restrict__ x,
                                                         const float* __restrict__ h, float* __restrict__ partial,
                                                         int B, int T) {
    constexpr int NT = 64, ZS = 67;  // odd stride: the B operand is read down a column (32 lanes = 32 rows)
    extern __shared__ __align__(16) float smem[];
    float* ds = smem;                // [NT][256]
    float* zs = smem + NT * 256;     // [128][ZS]; h rows are stored shifted: column tt holds h[t0 + tt - 1]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int tilesPerClip = (T + NT - 1) / NT, ntiles = B * tilesPerClip;
    f32x16 acc[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
    float bsum = 0.f;
    float4 sd[16], sx[4], sh[4];
    float hh;
    // piece p of a tile's staging: 0..15 da rows, 16..19 x, 20..23 h, 24 the halo column h[t0 - 1].  Branch-free (clamped
    // addresses), masked when written to LDS.  The main loop issues one piece per k-step: the 96-KB tile would otherwise
    // hit the memory pipeline as one burst and block the wave at issue (see conv64bf3_kernel).
    auto load_piece = [&](int tile, int p) {
        const int b = tile / tilesPerClip, t0 = (tile % tilesPerClip) * NT;
        if (p < 16) {
            const int i = tid + p * 256;
            sd[p] = reinterpret_cast<const float4*>(da + (size_t)b * T * 256)[(size_t)min(t0 + (i >> 6), T - 1) * 64 + (i & 63)];
        } else if (p < 24) {
            const int k = p & 3, i = tid + k * 256, j = i >> 4, q = i & 15;
            const size_t off = ((size_t)b * 64 + j) * T + min(t0 + 4 * q, T - 4);
            if (p < 20) sx[k] = *reinterpret_cast<const float4*>(x + off);
            else sh[k] = *reinterpret_cast<const float4*>(h + off);
        } else {
            hh = h[((size_t)b * 64 + (tid & 63)) * T + max(t0 - 1, 0)];
        }
    };
    auto load_tile = [&](int tile) {
#pragma unroll
        for (int p = 0; p < 25; ++p) load_piece(tile, p);
    };
    auto write_tile = [&](int tile) {
        const int t0 = (tile % tilesPerClip) * NT;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int i = tid + k * 256;
            float4 v = sd[k];
            if (t0 + (i >> 6) >= T) v = make_float4(0.f, 0.f, 0.f, 0.f);      // zero rows kill every product past T
            reinterpret_cast<float4*>(ds)[i] = v;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = tid + k * 256, j = i >> 4, q = i & 15;
            float* zx = zs + j * ZS + 4 * q;
            zx[0] = sx[k].x; zx[1] = sx[k].y; zx[2] = sx[k].z; zx[3] = sx[k].w;
            float* zh = zs + (64 + j) * ZS + 4 * q + 1;
            zh[0] = sh[k].x; zh[1] = sh[k].y; zh[2] = sh[k].z; zh[3] = sh[k].w;
        }
        if (tid < 64) zs[(64 + tid) * ZS] = (t0 >= 1) ? hh : 0.f;              // zero initial state
    };
    int tile = blockIdx.x;
    if (tile < ntiles) load_tile(tile);
    __syncthreads();
    if (tile < ntiles) write_tile(tile);
    __syncthreads();
    // A[i = n'][k = t] = ds[t][n'] ; B[k = t][j] = zs[j][t]
    const float* ap = ds + half * 256 + wave * 64 + l31;
    const float* bp = zs + l31 * ZS + half;
    while (tile < ntiles) {
        const int next = tile + gridDim.x, nextc = min(next, ntiles - 1);     // clamped: loaded (valid memory), never written
#pragma unroll
        for (int s = 0; s < NT / 2; ++s) {
            if (s < 25) load_piece(nextc, s);
            const float a0 = ap[2 * s * 256], a1 = ap[2 * s * 256 + 32];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const float bv = bp[nt * 32 * ZS + 2 * s];
                acc[0][nt] = mfma32(a0, bv, acc[0][nt]);
                acc[1][nt] = mfma32(a1, bv, acc[1][nt]);
            }
        }
#pragma unroll 8
        for (int tt = 0; tt < NT; ++tt) bsum += ds[tt * 256 + tid];
        __syncthreads();
        if (next < ntiles) write_tile(next);
        __syncthreads();
        tile = next;
    }
    float* out = partial + (size_t)blockIdx.x * (256 * 128 + 256);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                out[(wave * 64 + mt * 32 + mfma_row(r, half)) * 128 + nt * 32 + l31] = acc[mt][nt][r];
    out[256 * 128 + tid] = bsum;
}

// ---------------------------------------------------------------------------------- wgrad GEMM, bf16x6
// Same sums as lstm_wgrad_kernel on the bf16 matrix cores (bf16x6 split).  The contraction axis is time, the STRIDED
// axis of da [t][n']: its A fragments (one gate column, 8 consecutive steps) are gathered from the [piece][step][n']
// LDS image with eight ds_read_u16 per piece (lanes run along n': conflict-free) and packed with v_perm; z = [x ; h
// shifted by one step] is time-contiguous, so its B fragments are aligned ds_read_b128.  32-step tiles; wave w owns the
// gate columns [64 w, 64 w + 64) for all 128 z rows (128 accumulator registers).
// dynamic LDS: the da image Dd [3 pieces][32 steps][pitch 264] and the z image Zb [3 pieces][128 rows][pitch 40], bf16
constexpr size_t kLstmWgradBfLds = (size_t)(3 * 32 * 264 + 3 * 128 * 40) * 2;
__global__ __launch_bounds__(256) void lstm_wgrad_bf_kernel(const float* __restrict__ da, const float* __restrict__ x,
                                                            const float* __restrict__ h, float* __restrict__ partial,
                                                            int B, int T) {
    constexpr int NT = 32, NP = 3, PDD = 264, PZ = 40;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    unsigned short* Dd = reinterpret_cast<unsigned short*>(smem_raw);          // [NP][NT][PDD]   da pieces, [step][n']
    unsigned short* Zb = Dd + NP * NT * PDD;                                   // [NP][128][PZ]   z pieces, [row][step]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int tilesPerClip = (T + NT - 1) / NT, ntiles = B * tilesPerClip;
    f32x16 acc[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
    float bs[4] = {0.f, 0.f, 0.f, 0.f};            // bias sums of gate columns 4 (tid & 63) .. + 3 over this thread's steps
    float4 sd[8], sx[2];
    float sh[2][4];
    // piece p: 0..7 da rows (step (tid >> 6) + 4 p, columns 4 (tid & 63)..), 8..9 x, 10..11 h (shifted: column tt = h[t0 + tt - 1])
    auto load_piece = [&](int tile, int p) {
        const int b = tile / tilesPerClip, t0 = (tile % tilesPerClip) * NT;
        if (p < 8) {
            const int t = min(t0 + (tid >> 6) + 4 * p, T - 1);
            sd[p] = reinterpret_cast<const float4*>(da + ((size_t)b * T + t) * 256)[tid & 63];
        } else {
            const int k = p & 1, i = tid + k * 256, j = i >> 3, q = i & 7;
            const size_t row = ((size_t)b * 64 + j) * T;
            if (p < 10) sx[k] = *reinterpret_cast<const float4*>(x + row + min(t0 + 4 * q, T - 4));
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) sh[k][e] = h[row + min(max(t0 + 4 * q + e - 1, 0), T - 1)];
            }
        }
    };
    auto put4 = [&](unsigned short* d, int stride_p, float v0, float v1, float v2, float v3) {
        unsigned a0, a1, a2, b0, b1, b2;
        split3_pair(v0, v1, a0, a1, a2);
        split3_pair(v2, v3, b0, b1, b2);
        *reinterpret_cast<uint2*>(d) = make_uint2(a0, b0);
        *reinterpret_cast<uint2*>(d + stride_p) = make_uint2(a1, b1);
        *reinterpret_cast<uint2*>(d + 2 * stride_p) = make_uint2(a2, b2);
    };
    auto write_tile = [&](int tile) {
        const int t0 = (tile % tilesPerClip) * NT;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int tt = (tid >> 6) + 4 * p;
            float4 v = sd[p];
            if (t0 + tt >= T) v = make_float4(0.f, 0.f, 0.f, 0.f);            // zero rows kill every product past T
            bs[0] += v.x; bs[1] += v.y; bs[2] += v.z; bs[3] += v.w;
            put4(Dd + tt * PDD + 4 * (tid & 63), NT * PDD, v.x, v.y, v.z, v.w);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = tid + k * 256, j = i >> 3, q = i & 7;
            put4(Zb + j * PZ + 4 * q, 128 * PZ, sx[k].x, sx[k].y, sx[k].z, sx[k].w);
            float hv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) hv[e] = (t0 + 4 * q + e - 1 >= 0) ? sh[k][e] : 0.f;      // zero initial state
            put4(Zb + (64 + j) * PZ + 4 * q, 128 * PZ, hv[0], hv[1], hv[2], hv[3]);
        }
    };
    int tile = blockIdx.x;
#pragma unroll
    for (int p = 0; p < 12; ++p) load_piece(min(tile, ntiles - 1), p);
    __syncthreads();
    write_tile(min(tile, ntiles - 1));
    __syncthreads();
    while (tile < ntiles) {
        const int next = tile + gridDim.x, nextc = min(next, ntiles - 1);     // clamped: loaded (valid memory), never written
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int e0 = kb * 16 + 8 * half;
            bf16x8 Bf[4][NP];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    Bf[nt][p] = *reinterpret_cast<const bf16x8*>(Zb + (p * 128 + nt * 32 + l31) * PZ + e0);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                bf16x8 A[NP];
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const unsigned short* col = Dd + (p * NT + e0) * PDD + wave * 64 + mt * 32 + l31;
                    unsigned w[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) w[j] = (unsigned)col[(2 * j) * PDD] | ((unsigned)col[(2 * j + 1) * PDD] << 16);
                    A[p] = __builtin_bit_cast(bf16x8, make_uint4(w[0], w[1], w[2], w[3]));
                }
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    acc[mt][nt] = mfma_bf16x6(A, Bf[nt], acc[mt][nt]);
                    if ((kb * 2 + mt) * 4 + nt < 12) load_piece(nextc, (kb * 2 + mt) * 4 + nt);     // 12 pieces ride along the first 12 of 16 blocks
                }
            }
        }
        __syncthreads();
        if (next < ntiles) write_tile(next);
        __syncthreads();
        tile = next;
    }
    float* out = partial + (size_t)blockIdx.x * (256 * 128 + 256);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                out[(wave * 64 + mt * 32 + mfma_row(r, half)) * 128 + nt * 32 + l31] = acc[mt][nt][r];
    // bias: the four threads tid, tid + 64, .. share the gate columns 4 (tid & 63) .. + 3
    float* red = reinterpret_cast<float*>(smem_raw);          // [4][256]
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) red[(tid >> 6) * 256 + 4 * (tid & 63) + e] = bs[e];
    __syncthreads();
    out[256 * 128 + tid] = (red[tid] + red[256 + tid]) + (red[512 + tid] + red[768 + tid]);
}

}  // namespace

extern "C" {

static int g_lstm_dx_bf = 1;        // 1: bf16x6 split on the bf16 matrix cores (default) | 0: native fp32 MFMA
int wm_set_lstm_dx_bf16x6(int on, hipStream_t) { g_lstm_dx_bf = on ? 1 : 0; return 0; }

int wm_lstm_dx(const float* da, const float* w_ih, float* dx, int B, int T, hipStream_t stream) {
    const int ntiles = B * ((T + 63) / 64);
    if (g_lstm_dx_bf) {
        constexpr size_t ldsb = kLstmDxBfLds;
        static wm::DevOnce doneb;
        if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(lstm_dx_bf_kernel), ldsb, doneb)) return rc;
        hipLaunchKernelGGL(lstm_dx_bf_kernel, dim3(ntiles < kNumCU ? ntiles : kNumCU), dim3(256), ldsb, stream, da, w_ih, dx, B, T);
        WM_CHECK_LAUNCH();
        return 0;
    }
    constexpr size_t lds = kLstmDxLds;
    static wm::DevOnce done;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(lstm_dx_kernel), lds, done)) return rc;
    hipLaunchKernelGGL(lstm_dx_kernel, dim3(ntiles < kNumCU ? ntiles : kNumCU), dim3(256), lds, stream, da, w_ih, dx, B, T);
    WM_CHECK_LAUNCH();
    return 0;
}

// partial: >= 256 * (256*128 + 256) floats
int wm_lstm_wgrad(const float* da, const float* x, const float* h, float* partial, float* dw_ih, float* dw_hh,
                  float* db_ih, float* db_hh, int B, int T, int accumulate, hipStream_t stream) {
    int grid;
    if (g_lstm_dx_bf) {                           // same switch as wm_lstm_dx: bf16x6 (default) | native fp32 MFMA
        constexpr size_t ldsb = kLstmWgradBfLds;
        static wm::DevOnce doneb;
        if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(lstm_wgrad_bf_kernel), ldsb, doneb)) return rc;
        const int ntiles = B * ((T + 31) / 32);
        grid = ntiles < kNumCU ? ntiles : kNumCU;
        hipLaunchKernelGGL(lstm_wgrad_bf_kernel, dim3(grid), dim3(256), ldsb, stream, da, x, h, partial, B, T);
    } else {
        constexpr size_t lds = kLstmWgradLds;
        static wm::DevOnce done;
        if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(lstm_wgrad_kernel), lds, done)) return rc;
        const int ntiles = B * ((T + 63) / 64);
        grid = ntiles < kNumCU ? ntiles : kNumCU;
        hipLaunchKernelGGL(lstm_wgrad_kernel, dim3(grid), dim3(256), lds, stream, da, x, h, partial, B, T);
    }
    WM_CHECK_LAUNCH();
    hipLaunchKernelGGL(lstm_wgrad_reduce_kernel, dim3(kWgradSlab / 64), dim3(512), 0, stream, (const float*)partial, grid,
                       dw_ih, dw_hh, db_ih, db_hh, accumulate);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"

int wm::lstm_dx_bf16x6() { return g_lstm_dx_bf; }     // for lstm_bwd.hip (lstm.hpp)
