// Generic weight gradient as ONE plain GEMM with the taps folded into the column index:
//     G[a][j] = sum_{nb,t} A[nb][a][t] * Bx[nb][b][t + k - P],      j = b*K + k   (= the memory order of dW[a][b][k])
//   Conv1d (stride 1): A = dL/dy (rows = out channels),  Bx = layer input  -> dW[out][in][k]
//   Linear / LSTM:     K = 1 (the "time" axis is whatever axis is contiguous: positions or batch columns)
//   strided Conv1d and ConvTranspose1d: the strided operand is first re-laid by wm_gather_taps (tap planes / stride
//   phases become channels), which turns them into stride-1 problems with K = 1 / K = 2; `remap` puts the columns back
//   into the weight's own order in the reduce.
// M = Ca rows, N = Cb*K columns, contraction over (clip, position).  A wave owns a 32 x (32*NS) block (NS <= 4
// accumulators, whatever K is: a 8 x 8 x 3 layer is ONE MFMA per position pair, not three); the workgroup's four waves
// split rows (WA), columns (WJW) and -- when the matrix is smaller than that -- the positions of each chunk (WT, summed in
// fixed order at the end).  Per chunk of TC positions the A rows and the Bx rows the tile's columns touch are staged
// through registers (buffer loads: wave-uniform row offset + one per-lane constant, no vector-ALU address arithmetic)
// into LDS while the matrix cores work on the previous chunk; lanes run along the position axis (coalesced), LDS pitches
// are chosen so both operand reads are conflict-free (A: odd pitch, read down a column; Bx: pitch == K mod 32, so
// column j of the tile reads bank j).
// Split-K over gridDim.y: every workgroup writes its partial tile to slab[z] and a fixed-order reduce kernel forms the
// result -- no float atomics, bit-reproducible.  dbias[a] = sum A[a][t] rides along (column tile 0, VALU sums of the
// staged rows).
#include "wm_common.hpp"
using namespace wm;

namespace {

struct GWArgs {
    const float* A;
    const float* Bx;
    float* slab;     // [gz][Ca][NJ]
    float* slabb;    // [gz][Ca] or null
    int NB, Ca, Cb, La, Lb, K, P;
    long long bcs;   // floats between consecutive clips of Bx (>= Cb*Lb: Bx may be a channel slice of a wider tensor)
    int NJ;          // Cb*K
    int TC;          // positions per chunk: multiple of 8
    int nchunks;     // chunks per clip
    int nsub;        // 32-column blocks per wave (1..4)
    int WJW, WT;     // waves along the columns / along the positions of a chunk (WA*WJW*WT == 4)
    int ntj;         // column tiles
    int NBCH;        // Bx rows (channels) staged per workgroup
    int ncb;         // 64-position blocks per staged row (A and Bx alike)
    int AP, BP;      // LDS pitches
    int nwork;       // NB * nchunks
};

constexpr int GW_RA = 16;   // A staging units per wave and chunk (unit = one wave-wide dword load)
constexpr int GW_RB = 24;   // Bx staging units per wave and chunk

template <int WA, int NS, bool GEO1>   // GEO1: one 64-position block per staged row (ncb == 1, rows wider than 32): no unit decode
__global__ __launch_bounds__(256, 3) void gwgrad2_kernel(GWArgs g) {
    constexpr int TA = 32 * WA;
    extern __shared__ __align__(16) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wa = wave % WA, rest = wave / WA, wj = rest % g.WJW, wt = rest / g.WJW;
    const int ta = blockIdx.x / g.ntj, tj = blockIdx.x - ta * g.ntj;
    const int TJ = g.WJW * 32 * g.nsub;
    const int a0 = ta * TA, j0 = tj * TJ, b0 = j0 / g.K;
    const int TC = g.TC, BW = TC + g.K - 1, ncb = GEO1 ? 1 : g.ncb;
    // staging geometry (wave-uniform).  A unit is one wave-wide dword load: 64 positions of one row, or (rows <= 32 wide)
    // 32 positions of two rows.  Only rows that exist are staged; LDS rows are padded to whole units (no store predicate).
    const int rpu = GEO1 ? 1 : (BW <= 32 ? 2 : 1);          // rows per unit, A and Bx alike (BW >= TC)
    const int a_rows = min(TA, g.Ca - a0), b_rows = min(g.NBCH, g.Cb - b0);
    const int a_units = ((a_rows + rpu - 1) / rpu) * ncb, b_units = ((b_rows + rpu - 1) / rpu) * ncb;
    const int row_l = rpu == 2 ? half : 0, col_l = rpu == 2 ? l31 : lane;
    const int asz = TA * g.AP, zrow = asz + g.NBCH * g.BP;         // + one all-zero row: what columns past NJ read
    const unsigned inv_ncb = (65536u + (unsigned)ncb - 1u) / (unsigned)ncb;
    const unsigned vA = (unsigned)(row_l * g.La + col_l), vB = (unsigned)(row_l * g.Lb + col_l);
    const unsigned lA = (unsigned)(row_l * g.AP + col_l), lB = (unsigned)(asz + row_l * g.BP + col_l);
    const bool even_rows = ((a_rows % rpu) == 0) && ((b_rows % rpu) == 0);

    // per-lane column maps of the MFMA B operand (LDS float index of position 0 of the column)
    int boff[NS];
#pragma unroll
    for (int jt = 0; jt < NS; ++jt) {
        const int j = j0 + (wj * g.nsub + jt) * 32 + l31;
        const int b = j / g.K, k = j - b * g.K;
        const bool ok = (jt < g.nsub) && (j < g.NJ);
        boff[jt] = (ok ? asz + (b - b0) * g.BP + k : zrow) + half;
    }
    f32x16 acc[NS];
#pragma unroll
    for (int jt = 0; jt < NS; ++jt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[jt][r] = 0.f;
    float bsum = 0.f;
    const bool do_bias = (g.slabb != nullptr) && (tj == 0);
    const int bparts = 256 / TA, brow = tid % TA, bpart = tid / TA, bcpp = TC / bparts;

    float ra[GW_RA], rb[GW_RB];
    auto load_work = [&](int w) {
        int wv = wave;
        asm volatile("" : "+s"(wv));                         // opaque: the per-unit scalars are not hoisted out of the chunk loop
        const int nb = w / g.nchunks, t0 = (w - nb * g.nchunks) * TC, u0 = t0 - g.P;
        const float* Ab = g.A + (size_t)nb * g.Ca * g.La;
        const float* Bb = g.Bx + (size_t)nb * g.bcs;
        // fast path: every lane of every unit reads inside its own row of the clip -- buffer loads with a wave-uniform
        // offset (row, chunk start) plus one per-lane constant, no address arithmetic on the vector ALU (which the fp32
        // matrix instructions share)
        const bool fast = even_rows && (t0 + ncb * (rpu == 2 ? 32 : 64) <= g.La) && (u0 >= 0) && (u0 + ncb * (rpu == 2 ? 32 : 64) <= g.Lb);
        if (fast) {
            const wm_srd_t sa = make_srd(Ab, ((size_t)(g.NB - nb) * g.Ca * g.La) * sizeof(float));
            const wm_srd_t sb = make_srd(Bb, ((size_t)(g.NB - 1 - nb) * g.bcs + (size_t)g.Cb * g.Lb) * sizeof(float));
#pragma unroll
            for (int i = 0; i < GW_RA; ++i) {
                const int u = wv + 4 * i;
                if (u < a_units) {
                    const int rg = GEO1 ? u : (int)(((unsigned)u * inv_ncb) >> 16), cb = GEO1 ? 0 : u - rg * ncb;
                    ra[i] = buf_load(sa, vA * 4u, (unsigned)((a0 + rg * rpu) * g.La + t0 + cb * 64) * 4u);
                }
            }
#pragma unroll
            for (int i = 0; i < GW_RB; ++i) {
                const int u = wv + 4 * i;
                if (u < b_units) {
                    const int rg = GEO1 ? u : (int)(((unsigned)u * inv_ncb) >> 16), cb = GEO1 ? 0 : u - rg * ncb;
                    rb[i] = buf_load(sb, vB * 4u, (unsigned)((b0 + rg * rpu) * g.Lb + u0 + cb * 64) * 4u);
                }
            }
        } else {                                             // clip edges / odd row counts: clamp every address, zero the padding
#pragma unroll
            for (int i = 0; i < GW_RA; ++i) {
                const int u = wv + 4 * i;
                if (u < a_units) {
                    const int rg = GEO1 ? u : (int)(((unsigned)u * inv_ncb) >> 16), cb = GEO1 ? 0 : u - rg * ncb;
                    const int a = a0 + rg * rpu + row_l, col = cb * 64 + col_l, t = t0 + col;
                    const bool ok = (a < g.Ca) && (col < TC) && (t < g.La);
                    const float v = Ab[(unsigned)(min(a, g.Ca - 1) * g.La + min(t, g.La - 1))];
                    ra[i] = ok ? v : 0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < GW_RB; ++i) {
                const int u = wv + 4 * i;
                if (u < b_units) {
                    const int rg = GEO1 ? u : (int)(((unsigned)u * inv_ncb) >> 16), cb = GEO1 ? 0 : u - rg * ncb;
                    const int b = b0 + rg * rpu + row_l, col = cb * 64 + col_l, uu = u0 + col;
                    const bool ok = (b < g.Cb) && (col < BW) && (uu >= 0) && (uu < g.Lb);
                    const float v = Bb[(unsigned)(min(b, g.Cb - 1) * g.Lb + min(max(uu, 0), g.Lb - 1))];
                    rb[i] = ok ? v : 0.f;
                }
            }
        }
    };
    auto store_work = [&]() {
        int wv = wave;
        asm volatile("" : "+s"(wv));
#pragma unroll
        for (int i = 0; i < GW_RA; ++i) {
            const int u = wv + 4 * i;
            if (u < a_units) {
                const int rg = GEO1 ? u : (int)(((unsigned)u * inv_ncb) >> 16), cb = GEO1 ? 0 : u - rg * ncb;
                (smem + rg * rpu * g.AP + cb * 64)[lA] = ra[i];
            }
        }
#pragma unroll
        for (int i = 0; i < GW_RB; ++i) {
            const int u = wv + 4 * i;
            if (u < b_units) {
                const int rg = GEO1 ? u : (int)(((unsigned)u * inv_ncb) >> 16), cb = GEO1 ? 0 : u - rg * ncb;
                (smem + rg * rpu * g.BP + cb * 64)[lB] = rb[i];
            }
        }
    };

    for (int i = tid; i < g.BP; i += 256) smem[zrow + i] = 0.f;
    const int z = blockIdx.y, nz = gridDim.y;
    const int tbeg = wt * (TC / g.WT), npair = TC / g.WT / 2;
    load_work(z);
    for (int w = z; w < g.nwork; w += nz) {
        __syncthreads();                                     // the previous chunk's operand reads are done
        store_work();
        __syncthreads();
        if (w + nz < g.nwork) load_work(w + nz);             // in flight while the matrix cores run this chunk
        // software-pipelined position-pair loop, two pairs per trip with two operand sets (each read one MFMA group before
        // its use); the read-ahead index is clamped (scalar) so it stays inside the row: AP, BP carry 2 positions of slack
        const float* ap = smem + (wa * 32 + l31) * g.AP + half + tbeg;
        const float* bp[NS];
        float av = ap[0], bv[NS], an, bn[NS];
#pragma unroll
        for (int jt = 0; jt < NS; ++jt) { bp[jt] = smem + boff[jt] + tbeg; bv[jt] = bp[jt][0]; }
        for (int p = 0; p < npair; p += 2) {
            an = ap[2 * p + 2];
#pragma unroll
            for (int jt = 0; jt < NS; ++jt) bn[jt] = bp[jt][2 * p + 2];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int jt = 0; jt < NS; ++jt) acc[jt] = mfma32(av, bv[jt], acc[jt]);
            __builtin_amdgcn_sched_barrier(0);
            const int t2 = min(2 * p + 4, 2 * npair);
            av = ap[t2];
#pragma unroll
            for (int jt = 0; jt < NS; ++jt) bv[jt] = bp[jt][t2];
            __builtin_amdgcn_sched_barrier(0);
            if (p + 1 < npair) {
#pragma unroll
                for (int jt = 0; jt < NS; ++jt) acc[jt] = mfma32(an, bn[jt], acc[jt]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (do_bias) {
            const float* rp = smem + brow * g.AP + bpart * bcpp;
            for (int c = 0; c < bcpp; ++c) bsum += rp[c];
        }
    }
    __syncthreads();

    // ---- waves that split the positions: sum in wave order (fixed), then the wt == 0 wave holds the tile
    if (g.WT > 1) {
        float* red = smem;                                   // [(WT-1)][waves with wt==0][NS][16][64]
        const int owner = wa + WA * wj;                      // index among the wt == 0 waves
        const int nown = WA * g.WJW;
        if (wt > 0) {
#pragma unroll
            for (int jt = 0; jt < NS; ++jt)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[((((wt - 1) * nown + owner) * NS + jt) * 16 + r) * 64 + lane] = acc[jt][r];
        }
        __syncthreads();
        if (wt == 0) {
            for (int o = 0; o < g.WT - 1; ++o)
#pragma unroll
                for (int jt = 0; jt < NS; ++jt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[jt][r] += red[(((o * nown + owner) * NS + jt) * 16 + r) * 64 + lane];
        }
        __syncthreads();
    }
    if (wt == 0) {
#pragma unroll
        for (int jt = 0; jt < NS; ++jt) {
            if (jt >= g.nsub) continue;
            const int j = j0 + (wj * g.nsub + jt) * 32 + l31;
            if (j >= g.NJ) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int a = a0 + wa * 32 + mfma_row(r, half);
                if (a < g.Ca) g.slab[((size_t)z * g.Ca + a) * g.NJ + j] = acc[jt][r];
            }
        }
    }
    if (do_bias) {
        float* bred = smem;                                  // [bparts][TA]
        bred[bpart * TA + brow] = bsum;
        __syncthreads();
        if (bpart == 0 && a0 + brow < g.Ca) {
            float sacc = 0.f;
            for (int p = 0; p < bparts; ++p) sacc += bred[p * TA + brow];
            g.slabb[(size_t)z * g.Ca + a0 + brow] = sacc;
        }
    }
}

// out[perm(i)] (+)= sum_z slab[z][i]: 8 z-lanes per output, each a fixed-order chain, combined in fixed order (fp64).  Outputs
// i >= n are the bias gradient: bout[i - n] (+)= sum_z bslab[z][i - n] (nb of them; bslab / bout may be null with nb = 0).
//   remap 0: identity | 1: column j' = k*r1 + b -> b*r2 + k (tap planes -> dW[a][b][k]; r1 = Cb, r2 = K)
//        | 2: column j' = (co*r1 + ph)*2 + q -> co*2*r1 + q*r1 + ph (stride phases -> ConvTranspose taps; r1 = stride)
__global__ __launch_bounds__(256) void gwgrad2_reduce_kernel(const float* __restrict__ slab, float* __restrict__ out, size_t n, int nz,
                                                             int NJ, int accumulate, int remap, int r1, int r2,
                                                             const float* __restrict__ bslab, float* __restrict__ bout, int nb) {
    __shared__ double part[8][32];
    const int o = threadIdx.x & 31, zl = threadIdx.x >> 5;
    const size_t i = (size_t)blockIdx.x * 32 + o;
    const bool is_w = i < n, is_b = !is_w && i < n + (size_t)nb;
    double s = 0.0;
    if (is_w)
        for (int z = zl; z < nz; z += 8) s += (double)slab[(size_t)z * n + i];
    else if (is_b)
        for (int z = zl; z < nz; z += 8) s += (double)bslab[(size_t)z * nb + (i - n)];
    part[zl][o] = s;
    __syncthreads();
    if (zl == 0 && (is_w || is_b)) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += part[q][o];
        if (is_b) {
            float* d = bout + (i - n);
            *d = (float)((accumulate ? (double)*d : 0.0) + t);
            return;
        }
        size_t d = i;
        if (remap) {
            const size_t a = i / (size_t)NJ;
            const int jp = (int)(i - a * (size_t)NJ);
            int j;
            if (remap == 1) { const int k = jp / r1, b = jp - k * r1; j = b * r2 + k; }
            else { const int q2 = jp & 1, cp = jp >> 1, co = cp / r1, ph = cp - co * r1; j = co * 2 * r1 + q2 * r1 + ph; }
            d = a * (size_t)NJ + j;
        }
        out[d] = (float)((accumulate ? (double)out[d] : 0.0) + t);
    }
}

// y[nb][row][t] = x[nb][c][t*S + k - P] (0 outside the clip), t in [0, Lout), for c < C, k < K:
//   order 0: row = k*C + c (tap planes: a strided Conv1d's weight gradient becomes a K = 1 GEMM, and its 1x1 strided
//            skip convolution reads plane P);  order 1: row = c*K + k (stride phases of a ConvTranspose1d's output gradient)
__global__ __launch_bounds__(256) void gather_taps_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int Lin, int K,
                                                          int S, int P, int Lout, int order) {
    // one workgroup = 256 output positions of one input row: the span of x they touch is read ONCE, coalesced, into LDS;
    // every tap plane is then a strided LDS read and a coalesced store
    __shared__ float xs[255 * 8 + 16 + 8];
    const int t0 = blockIdx.x * 256, c = blockIdx.y, nb = blockIdx.z, tid = threadIdx.x;
    const float* xr = x + ((size_t)nb * C + c) * Lin;
    const int u0 = t0 * S - P, span = 255 * S + K;
    for (int i = tid; i < span; i += 256) {
        const int u = u0 + i;
        xs[i] = (u >= 0 && u < Lin) ? xr[u] : 0.f;
    }
    __syncthreads();
    const int t = t0 + tid;
    if (t >= Lout) return;
    float* yb = y + (size_t)nb * C * K * Lout;
    for (int k = 0; k < K; ++k) {
        const int row = order ? c * K + k : k * C + c;
        yb[(size_t)row * Lout + t] = xs[tid * S + k];
    }
}

template <int WA, int NS, bool GEO1>
int launch_gwgrad2(const GWArgs& g, dim3 grid, size_t lds, hipStream_t stream) {
    auto kern = gwgrad2_kernel<WA, NS, GEO1>;
    static wm::DevOnce once;
    if (int rc = wm::lds_opt_in(reinterpret_cast<const void*>(kern), 150 * 1024, once)) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, stream, g);
    WM_CHECK_LAUNCH();
    return 0;
}

struct GWPlan {
    bool ok;
    int WA, TC, nchunks, nsub, WJW, WT, ntj, nta, NBCH, ncb, AP, BP, gz;
    size_t lds, slab_floats;
};

GWPlan gw_plan(int NB, int Ca, int Cb, int La, int K) {
    GWPlan p{};
    p.WA = Ca > 32 ? 2 : 1;
    const int TA = 32 * p.WA, R = 4 / p.WA, NJ = Cb * K;
    p.nta = (Ca + TA - 1) / TA;
    const int nsub_total = (NJ + 31) / 32;
    // wave split of the columns (WJW of the R waves that do not split rows) x 32-column blocks per wave (ns <= 4): the tile must
    // not touch more Bx rows than the staging registers hold (K = 1: every column is its own row); among those, waste the fewest
    // matrix-core columns over all column tiles, then take the widest tile (fewest re-reads of A), then the most column waves
    int bw = 1, bn = 1, best_waste = 1 << 30, best_tj = 0;
    for (int wjw = R; wjw >= 1; wjw >>= 1) {
        for (int ns = 4; ns >= 1; --ns) {
            const int tjb = wjw * ns;                                    // blocks per column tile
            if (tjb > nsub_total && !(wjw == 1 && ns == 1) && (tjb - nsub_total) >= ns) continue;   // a whole wave would idle
            int rows = (tjb * 32 - 1) / K + 2;
            if (rows > Cb) rows = Cb;
            if (rows > 4 * GW_RB && !(wjw == 1 && ns == 1)) continue;
            const int waste = ((nsub_total + tjb - 1) / tjb) * tjb - nsub_total;
            if (waste < best_waste || (waste == best_waste && tjb > best_tj)) { best_waste = waste; best_tj = tjb; bw = wjw; bn = ns; }
        }
    }
    p.WJW = bw;
    p.nsub = bn;
    p.WT = R / p.WJW;
    {
        const int TJ0 = p.WJW * 32 * p.nsub;
        p.NBCH = (TJ0 - 1) / K + 2;
        if (p.NBCH > Cb) p.NBCH = Cb;
    }
    const int TJ = p.WJW * 32 * p.nsub;
    p.ntj = (NJ + TJ - 1) / TJ;
    const int ra = Ca < TA ? Ca : TA, rbx = p.NBCH;          // rows staged per chunk
    // positions per chunk: ncb blocks of 64 (one block of 32 for short sequences); few rows -> long chunks (up to 256)
    for (int ncb = 4; ncb >= 1 && !p.ok; --ncb) {
        for (int narrow = 0; narrow < 2 && !p.ok; ++narrow) {
            if (narrow && ncb > 1) continue;
            const int width = narrow ? 32 : 64 * ncb;            // staged span of a row
            int tcmax = (width - (K - 1)) & ~7;                  // so that BW = TC + K - 1 <= width
            if (tcmax < 8) continue;
            if (!narrow && ncb > 1 && La < 64 * (ncb - 1)) continue;
            if (!narrow && ncb == 1 && La <= 24) continue;       // short sequences: the 32-wide form wastes fewer lanes
            p.nchunks = (La + tcmax - 1) / tcmax;
            p.TC = (((La + p.nchunks - 1) / p.nchunks) + 7) & ~7;
            if (p.TC > tcmax) p.TC = tcmax;
            p.nchunks = (La + p.TC - 1) / p.TC;
            const int BW = p.TC + K - 1, rpu = BW <= 32 ? 2 : 1;
            if ((rpu == 2) != (narrow == 1)) continue;
            const int a_units = ((ra + rpu - 1) / rpu) * ncb, b_units = ((rbx + rpu - 1) / rpu) * ncb;
            // pitches: whole staging units wide (unconditional stores) + slack for the pipelined loop's read-ahead (2 positions);
            // A: odd (operand read down a column); Bx: == K (mod 32), so tile column j reads bank j
            p.AP = (width + 2) | 1;
            const int bpw = width + 2;
            p.BP = bpw + (((K - bpw) % 32) + 32) % 32;
            size_t lds = ((size_t)TA * p.AP + (size_t)(p.NBCH + 1) * p.BP) * sizeof(float);
            const size_t red = (size_t)(p.WT - 1) * p.WA * p.WJW * 4 * 16 * 64 * sizeof(float);
            if (red > lds) lds = red;
            if (lds < 1024 * sizeof(float)) lds = 1024 * sizeof(float);
            if (a_units <= 4 * GW_RA && b_units <= 4 * GW_RB && lds <= 52 * 1024) { p.lds = lds; p.ncb = ncb; p.ok = true; }   // three workgroups per CU
        }
    }
    if (!p.ok) return p;
    const long long nwork = (long long)NB * p.nchunks;
    const int tiles = p.nta * p.ntj;
    long long gz = tiles >= 768 ? 1 : 768 / tiles;         // <= 768 workgroups = three per CU (registers and LDS admit three): one round
    if (gz > nwork) gz = nwork;
    if (gz < 1) gz = 1;
    p.gz = (int)gz;
    p.slab_floats = (size_t)p.gz * Ca * (NJ + 1);           // [gz][Ca][NJ] then [gz][Ca] bias partials
    return p;
}

}  // namespace

extern "C" {

// workspace of wm_gwgrad for a problem shape: *slab_floats = number of fp32 elements the caller must provide
int wm_gwgrad_plan(int NB, int Ca, int Cb, int La, int K, long long* slab_floats, hipStream_t) {
    if (NB <= 0 || Ca <= 0 || Cb <= 0 || La <= 0 || K <= 0 || K > 16 || !slab_floats) return (int)hipErrorInvalidValue;
    const GWPlan p = gw_plan(NB, Ca, Cb, La, K);
    if (!p.ok) return (int)hipErrorInvalidValue;
    *slab_floats = (long long)p.slab_floats;
    return 0;
}

// G[a][b][k] (+)= sum_{nb,t} A[nb][a][t] * Bx[nb][b][t + k - P]; dbias[a] (+)= sum A (dbias may be NULL).  Deterministic
// (split-K partial tiles in `slab`, >= wm_gwgrad_plan floats, then a fixed-order reduce).  accumulate: 0 overwrite | 1 add.
// b_clip_stride: floats between clips of Bx (0 = dense, Cb*Lb); remap / r1 / r2: column order of the result (see the reduce).
int wm_gwgrad(const float* A, const float* Bx, float* G, float* dbias, float* slab, int NB, int Ca, int Cb, int La, int Lb,
              int K, int P, long long b_clip_stride, int remap, int r1, int r2, int accumulate, hipStream_t stream) {
    if (NB <= 0 || Ca <= 0 || Cb <= 0 || La <= 0 || Lb <= 0 || K <= 0 || K > 16 || !slab || remap < 0 || remap > 2 ||
        (size_t)Ca * La >= (1u << 30) || (size_t)Cb * Lb >= (1u << 30))
        return (int)hipErrorInvalidValue;
    if (b_clip_stride == 0) b_clip_stride = (long long)Cb * Lb;
    if (b_clip_stride < (long long)Cb * Lb) return (int)hipErrorInvalidValue;
    const int NJ = Cb * K;
    if ((remap == 1 && (r1 <= 0 || r2 <= 0 || r1 * r2 != NJ)) || (remap == 2 && (r1 <= 0 || K != 2 || Cb % r1 != 0)))
        return (int)hipErrorInvalidValue;
    const GWPlan p = gw_plan(NB, Ca, Cb, La, K);
    if (!p.ok) return (int)hipErrorInvalidValue;
    float* slabb = dbias ? slab + (size_t)p.gz * Ca * NJ : nullptr;
    GWArgs g{A, Bx, slab, slabb, NB, Ca, Cb, La, Lb, K, P, b_clip_stride, NJ, p.TC, p.nchunks, p.nsub, p.WJW, p.WT, p.ntj, p.NBCH,
             p.ncb, p.AP, p.BP, NB * p.nchunks};
    dim3 grid(p.nta * p.ntj, p.gz);
    const int ns = p.nsub == 1 ? 1 : (p.nsub == 2 ? 2 : 4);
    int rc = 0;
    const bool geo1 = (p.ncb == 1) && (p.TC + K - 1 > 32);
#define WM_GW(WA_, NS_) (geo1 ? launch_gwgrad2<WA_, NS_, true>(g, grid, p.lds, stream) : launch_gwgrad2<WA_, NS_, false>(g, grid, p.lds, stream))
    if (p.WA == 1) rc = ns == 1 ? WM_GW(1, 1) : ns == 2 ? WM_GW(1, 2) : WM_GW(1, 4);
    else rc = ns == 1 ? WM_GW(2, 1) : ns == 2 ? WM_GW(2, 2) : WM_GW(2, 4);
#undef WM_GW
    if (rc) return rc;
    const size_t n = (size_t)Ca * NJ;
    const int nbias = dbias ? Ca : 0;
    hipLaunchKernelGGL(gwgrad2_reduce_kernel, dim3((unsigned)((n + nbias + 31) / 32)), dim3(256), 0, stream, slab, G, n, p.gz, NJ, accumulate,
                       remap, r1, r2, slabb, dbias, nbias);
    WM_CHECK_LAUNCH();
    return 0;
}

// y[nb][row][t] = x[nb][c][t*S + k - P] (0 outside), t < Lout; order 0: row = k*C + c | 1: row = c*K + k   (see gather_taps_kernel)
int wm_gather_taps(const float* x, float* y, int NB, int C, int Lin, int K, int S, int P, int Lout, int order, hipStream_t stream) {
    if (NB <= 0 || NB > 65535 || C <= 0 || C > 65535 || Lin <= 0 || K <= 0 || K > 16 || S <= 0 || S > 8 || Lout <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_taps_kernel, dim3((Lout + 255) / 256, C, NB), dim3(256), 0, stream, x, y, C, Lin, K, S, P, Lout, order);
    WM_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
