"""The float64 generator every attack yardstick draws from, written from the published definition (Salmon et al., "Parallel random
numbers: as easy as 1, 2, 3", SC'11) and the comments of include/wm_hip.h with numpy alone -- nothing from the package.  Shared by
fir_yardstick, time_warp_yardstick, splice_yardstick and test_gpu_attacks; tests/test_attacks_cpu.py pins it to the Random123 vectors.

  philox4x32_10(counter, key)   four counter words (values or arrays that broadcast), two key words -> uint32 array (4, ...)
  unit(o)                       u = ((o >> 9) + 0.5) 2^-23, exact in float32 and float64, never 0 or 1
  key_of(seed)                  the seed's two halves
  normals(seed, draw, row, n, high)   Box-Muller on the counters (t >> 2, high, row, draw)
  affine32(pair, u)             fmaf(high - low, u, low) in float32
  FAMILIES                      (word 0, word 1) of every counter family that is not a sample's or a tap's"""
import math

import numpy as np

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    c = list(np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for v in counter]))
    k0, k1 = (int(k) & 0xFFFFFFFF for k in key)
    lo = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c).astype(np.uint32)


def unit(o):
    return ((o >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def key_of(seed):
    seed = int(seed) & (2 ** 64 - 1)
    return seed & 0xFFFFFFFF, seed >> 32


# the first two counter words of the families: samples have (q, SAMPLE_HIGH), a synthetic response's taps (k >> 2, RIR_HIGH), the
# parameter counters (~0 - i, ~0); Splice's span j draws its geometry from splice_span(j) and its shift from splice_shift(j)
SAMPLE_HIGH, RIR_HIGH = 0, 0xFFFFFFFE
PARAM, PARAM2, WARP, WARP_PHASE = ((0xFFFFFFFF - i, 0xFFFFFFFF) for i in range(4))
SPLICE_MAX_SPANS = 8


def splice_span(j):
    return 0xFFFFFFFB - 2 * j, 0xFFFFFFFF


def splice_shift(j):
    return 0xFFFFFFFA - 2 * j, 0xFFFFFFFF


FAMILIES = dict(param=PARAM, param2=PARAM2, warp=WARP, warp_phase=WARP_PHASE,
                **{f"splice_span{j}": splice_span(j) for j in range(SPLICE_MAX_SPANS)},
                **{f"splice_shift{j}": splice_shift(j) for j in range(SPLICE_MAX_SPANS)})


def normals(seed, draw, row, n, high):
    """the Box-Muller normals of "samples" t < n from the counters (t >> 2, high, row, draw); high None: q's own high word"""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    o = philox4x32_10((q, q >> np.uint64(32) if high is None else high, int(row), int(draw)), key_of(seed))
    z = np.empty((len(q), 4))
    for p in (0, 1):
        rad, th = np.sqrt(-2.0 * np.log(unit(o[2 * p]))), 2.0 * math.pi * unit(o[2 * p + 1])
        z[:, 2 * p], z[:, 2 * p + 1] = rad * np.cos(th), rad * np.sin(th)
    return z.reshape(-1)[:n]


def affine32(pair, u):
    lo, hi = np.float32(pair[0]), np.float32(pair[1])
    return (np.float64(hi - lo) * u + np.float64(lo)).astype(np.float32)          # fmaf(hi - lo, u, lo): the product is exact in float64
