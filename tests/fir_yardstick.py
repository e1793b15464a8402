"""The float64 yardstick of the reverb / echo attack (wm_fir_rows, wm_rir_synth, attacks.Convolved / Reverb), written from the
definitions in include/wm_hip.h with numpy alone -- nothing from the package -- and shared by tests/test_reverb_cpu.py and
tests/test_gpu_fir_rows.py.

  fir(x, h)          np.convolve(x_r, h_r)[:n] per row, float64 (int64 for integer inputs)
  fir_adjoint(x, h)  y[t] = sum_k h[k] x[t + k], written as flip(fir(flip(x), h))
  bound(x, h)        gamma(K + 2) * sum_k |h_k x_{t-k}|: for ANY summation order of K rounded fp32 products
                     |y - y64| <= gamma(K + 2) sum |h x|, gamma(m) = m u / (1 - m u), u = 2^-24 (Higham, Accuracy and Stability, ch. 3-4)
  philox4x32_10, unit, normals      the generator of tests/draw_yardstick.py, handed on under the names the tests use
  reverb_params, bank_index, rir    the draws and the response of the comment of wm_rir_synth"""
import functools
import math

import numpy as np

from draw_yardstick import PARAM, PARAM2, RIR_HIGH, SAMPLE_HIGH, affine32, key_of, normals, philox4x32_10, unit  # noqa: F401
from yardstick_common import gamma

# the device normal against float64 Box-Muller: 4 * the largest error tests/test_gpu_attacks.py has measured on an MI355X (NOISE_MEASURED
# = 6.679e-7 there, NOISE_TOL = 4 * that); restated, not imported
NOISE_TOL = 4 * 6.679e-7
RIR_REL = 2e-5                                    # fp32 scalars, exp and the sum's order in a response: relative, next to gamma(K + 2)

# (rows, n, K): one sample, rows shorter than a block, a whole block, one past it, K > n, more than one group of 32 blocks, a K that is no
# multiple of 32, more than one workgroup per row, the default shape, the shape where a workgroup owns 128 blocks instead of 256; and the
# longest response there is, whose taps and history need more than 64 KB of LDS
CASES = [(3, n, K) for n, K in ((1, 1), (5, 1), (31, 2), (32, 32), (33, 33), (40, 100), (1000, 257), (1025, 64), (4099, 1000),
                                (16000, 2048))] + [(2, 16000, 4096), (1, 4200, 16384)]


# ------------------------------------------------------------------------------------------ the convolution
def _taps(h, rows):
    h = np.asarray(h)
    return np.broadcast_to(h, (rows, h.shape[-1])) if h.ndim == 1 else h


def fir(x, h):
    """y[r][t] = sum_{k <= t} h_r[k] x[r][t - k]; x (rows, n), h (K,) or (rows, K); the dtype follows numpy's promotion of the inputs"""
    x = np.asarray(x)
    n = x.shape[1]
    return np.stack([np.convolve(xr, hr)[:n] for xr, hr in zip(x, _taps(h, x.shape[0]))])


def fir_adjoint(x, h):
    """y[r][t] = sum_{t + k < n} h_r[k] x[r][t + k] = flip(H flip(x))"""
    return fir(np.asarray(x)[:, ::-1], h)[:, ::-1]


def bound(x, h):
    K = np.asarray(h).shape[-1]
    return gamma(K + 2) * fir(np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(h, dtype=np.float64)))


def bound_adjoint(x, h):
    K = np.asarray(h).shape[-1]
    return gamma(K + 2) * fir_adjoint(np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(h, dtype=np.float64)))


@functools.lru_cache(maxsize=None)
def int_case(rows, n, K):
    """x integers in [-8, 8], h integers in [-4, 4] (flat: every tap counts), per-row taps; int64"""
    rng = np.random.default_rng(1000 * n + K)
    x, h = rng.integers(-8, 9, (rows, n)), rng.integers(-4, 5, (rows, K))
    for a in (x, h):
        a.setflags(write=False)
    return x, h


@functools.lru_cache(maxsize=None)
def float_case(rows, n, K):
    """unit-variance x and decaying taps (the yardstick's own responses at rt60 = 0.3 s, 6 dB), both rounded to float32 and held in float64"""
    rng = np.random.default_rng(2000 * n + K)
    x = rng.standard_normal((rows, n)).astype(np.float32).astype(np.float64)
    h = np.stack([rir(5, 0, r, 0.3, 6.0, K, 16000.0)[0] for r in range(rows)]).astype(np.float32).astype(np.float64)
    for a in (x, h):
        a.setflags(write=False)
    return x, h


@functools.lru_cache(maxsize=None)
def float_ref(rows, n, K, shared, reverse):
    x, h = float_case(rows, n, K)
    hh = h[0] if shared else h
    ref = (fir_adjoint if reverse else fir)(x, hh), (bound_adjoint if reverse else bound)(x, hh)
    for a in ref:
        a.setflags(write=False)
    return ref


# ------------------------------------------------------------------------------------------ the draws (the generator is tests/draw_yardstick.py's)
def reverb_params(seed, draw, rows, rt60, drr_db):
    o = philox4x32_10((PARAM2[0], PARAM2[1], np.asarray(rows, dtype=np.uint64), int(draw)), key_of(seed))
    return affine32(rt60, unit(o[0])), affine32(drr_db, unit(o[1]))


def bank_index(seed, draw, rows, entries):
    o = philox4x32_10((PARAM2[0], PARAM2[1], np.asarray(rows, dtype=np.uint64), int(draw)), key_of(seed))
    return np.floor(unit(o[2]) * entries).astype(np.int64)


def rir(seed, draw, row, rt60, drr_db, K, sample_rate):
    """(h, envelope): the response of the comment of wm_rir_synth in float64, and a exp(-k c) -- an error of the normal z_k reaches h[k]
    multiplied by no more than that (zeros where the response is {1, 0, ...})"""
    rt60, drr_db, sample_rate = float(np.float32(rt60)), float(np.float32(drr_db)), float(np.float32(sample_rate))
    h, env = np.zeros(K), np.zeros(K)
    h[0] = 1.0
    if K == 1:
        return h, env
    c = 3.0 * math.log(10.0) / (rt60 * sample_rate)
    decay = np.exp(-np.arange(K) * c)
    e = normals(seed, draw, row, K, RIR_HIGH) * decay
    e[0] = 0.0
    E = float((e * e).sum())
    if not E > 0.0:
        return h, env
    w = 10.0 ** (-drr_db / 10.0)
    a = math.sqrt(w / E)
    h = a * e / math.sqrt(1.0 + w)
    h[0] = 1.0 / math.sqrt(1.0 + w)
    env = a * decay
    env[0] = 0.0
    return h, env


def rir_bound(h64, env):
    """|h - h64| <= a exp(-k c) NOISE_TOL + (gamma(K + 2) + 2e-5) |h64| + 1e-37"""
    return env * NOISE_TOL + (gamma(len(h64) + 2) + RIR_REL) * np.abs(h64) + 1e-37


# ------------------------------------------------------------------------------------------ arguments the launchers refuse
_X, _H, _Y, _P = 1 << 20, 1 << 24, 1 << 26, 1 << 28                               # made-up, never dereferenced addresses
# wm_fir_rows(x, h, y, rows, n, K, h_stride, reverse, stream)
BAD_FIR_ARGS = ((_X, _H, _Y, 0, 1000, 64, 64, 0, None),                          # rows < 1
                (_X, _H, _Y, 2, 0, 64, 64, 0, None),                             # n < 1
                (_X, _H, _Y, 1, (1 << 34) + 1, 64, 64, 0, None),                 # n above 2^34
                (_X, _H, _Y, 2, 1000, 0, 0, 0, None),                            # K < 1
                (_X, _H, _Y, 2, 1000, 16385, 16385, 0, None),                    # K above 16384
                (_X, _H, _Y, 2, 1000, 64, 63, 0, None),                          # h_stride between 0 and K
                (_X, _H, _Y, 2, 1000, 64, -64, 0, None),
                (None, _H, _Y, 2, 1000, 64, 64, 0, None),                        # null pointers
                (_X, None, _Y, 2, 1000, 64, 64, 0, None),
                (_X, _H, None, 2, 1000, 64, 64, 0, None),
                (_X + 2, _H, _Y, 2, 1000, 64, 64, 0, None),                      # misaligned
                (_X, _H + 1, _Y, 2, 1000, 64, 64, 0, None),
                (_X, _H, _Y + 3, 2, 1000, 64, 64, 0, None),
                (_X, _H, _X, 2, 1000, 64, 64, 0, None),                          # in place
                (_X, _H, _X, 2, 1000, 64, 64, 1, None),
                (_X, _H, _X + 7996, 2, 1000, 64, 64, 0, None),                   # y overlaps the last float of x
                (_X, _Y + 4000, _Y, 2, 1000, 64, 0, 0, None),                    # shared taps inside y
                (_X, _Y - 508, _Y, 2, 1000, 64, 64, 0, None))                    # y overlaps the last tap of the last row
# wm_rir_synth(params, h, rows, K, sample_rate, row0, seed, draw, stream)
BAD_RIR_ARGS = ((_P, _H, 0, 64, 16000.0, 0, 0, 0, None),                         # rows < 1
                (_P, _H, 2, 0, 16000.0, 0, 0, 0, None),                          # K out of range
                (_P, _H, 2, 16385, 16000.0, 0, 0, 0, None),
                (_P, _H, 2, 64, 0.0, 0, 0, 0, None),                             # sample_rate
                (_P, _H, 2, 64, -16000.0, 0, 0, 0, None),
                (_P, _H, 2, 64, float("nan"), 0, 0, 0, None),
                (_P, _H, 2, 64, float("inf"), 0, 0, 0, None),
                (_P, _H, 2, 64, 16000.0, -1, 0, 0, None),                        # row0, draw
                (_P, _H, 2, 64, 16000.0, (1 << 32) - 1, 0, 0, None),
                (_P, _H, 2, 64, 16000.0, 0, 0, -1, None),
                (_P, _H, 2, 64, 16000.0, 0, 0, 1 << 32, None),
                (None, _H, 2, 64, 16000.0, 0, 0, 0, None),                       # null, misaligned
                (_P, None, 2, 64, 16000.0, 0, 0, 0, None),
                (_P + 2, _H, 2, 64, 16000.0, 0, 0, 0, None),
                (_P, _H + 1, 2, 64, 16000.0, 0, 0, 0, None),
                (_H + 8, _H, 2, 64, 16000.0, 0, 0, 0, None))                     # params inside h
