// The attacks' counter-based draws on the device (distort.hip, splice.hip): Philox4x32-10 (Salmon et al., SC'11), the 24-bit unit map, and
// the groups of 4 samples the apply kernels read and write, all in namespace wm.  The counter families are listed once, in
// draws.py's FAMILIES, and the output words in use in its WORDS; draws.py restates the generator on the host and tests/draw_yardstick.py
// checks both.
#pragma once
#include "wm_common.hpp"

namespace wm {

struct Rng { unsigned k0, k1, draw; long long row0; };          // the key is the seed's two halves
inline Rng make_rng(long long seed, long long draw, long long row0) {
    return Rng{(unsigned)((unsigned long long)seed & 0xffffffffu), (unsigned)((unsigned long long)seed >> 32), (unsigned)draw, row0};
}

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&o)[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// u = ((o >> 9) + 0.5) 2^-23 has 24 bits: exact in either type, never 0 or 1; as a double the comparison with a threshold is the host's
__device__ __forceinline__ float unit(unsigned o) { return ((float)(o >> 9) + 0.5f) * 0x1p-23f; }
__device__ __forceinline__ double unit_d(unsigned o) { return ((double)(o >> 9) + 0.5) * 0x1p-23; }

__device__ __forceinline__ bool aligned16(const void* p, long long i) { return (((uintptr_t)p >> 2) + (unsigned long long)i) % 4 == 0; }

// v[e] = p[base + t0 + e] where 0 <= t0 + e < n, else 0; one 16-byte load when `aligned` (the address of p[base + t0] is a multiple of 16)
// and the four lie inside the row
template <typename I>
__device__ __forceinline__ void load4(const float* __restrict__ p, long long base, I t0, I n, bool aligned, float (&v)[4]) {
    if (aligned && t0 >= 0 && t0 + 4 <= n) {
        const f32x4 s = *reinterpret_cast<const f32x4*>(p + base + t0);
        v[0] = s[0]; v[1] = s[1]; v[2] = s[2]; v[3] = s[3];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (t0 + e >= 0 && t0 + e < n) ? p[base + t0 + e] : 0.f;
    }
}
template <typename I>
__device__ __forceinline__ void store4(float* __restrict__ p, long long base, I t0, I n, const float (&v)[4]) {
    if (t0 >= 0 && t0 + 4 <= n) {                                    // the caller's groups are on 16-byte boundaries of p
        const f32x4 s = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(p + base + t0) = s;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (t0 + e >= 0 && t0 + e < n) p[base + t0 + e] = v[e];
    }
}

inline int grid_for(long long work) { const long long cap = 8ll * kNumCU; return (int)(work < cap ? work : cap); }

}  // namespace wm
