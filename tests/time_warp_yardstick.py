"""The float64 yardstick of the speed-change / wow-and-flutter attack (wm_time_warp, attacks.TimeWarp), written from the definition in
include/wm_hip.h with numpy alone -- nothing from the package -- and shared by tests/test_time_warp_cpu.py and
tests/test_gpu_time_warp.py.

  table(zeros, res)            the Hann-windowed sinc half response in float64, rounded to float32, with its pinned entries
  position(prm, n)             p(t), t < n, of one parameter row {a, off, d, w, phi, c}
  taps(prm, n, tab, Z, R)      for every t the candidate taps k, their float64 weights W(p(t) - k) (0 outside the support or the row) and the
                               support predicate: the dense (n, J) form every map below is read from
  forward / adjoint            y[t] = sum_k W x[k] and dx[k] = sum_t W dy[t] per row, with their per-sample bounds
  matrix(prm, n, tab, Z, R)    the dense (n, n) float64 matrix M[t, k] = W(p(t) - k), for small n
  philox4x32_10, unit, warp_params   the generator of tests/draw_yardstick.py, handed on, and TimeWarp's draws

The bound.  With u = 2^-24, T the number of taps in a sample's support and gamma(m) = m u / (1 - m u) (Higham, Accuracy and Stability,
ch. 3-4):
    |y - y64| <= gamma(T + 4) sum_k |W x_k|  +  Lip eps_p sum_{k in support} |x_k|
  gamma(T + 4): T rounded products added in any order, and the four fp32 roundings of a weight (f, the table difference, the fmaf, the
                product with c32); the float64 W below carries none of them
  Lip = c^2 R max_i |tab[i + 1] - tab[i]|   the slope of the interpolated table in u = p - k
  eps_p = 2^-50 (|p| + |d|)                 fp64 rounding of p (fma or not) and of a sinpi good to a few ulp
For the adjoint the same two terms are summed over t for every k."""
import functools
import math

import numpy as np

from draw_yardstick import PARAM, PARAM2, RIR_HIGH, WARP, WARP_PHASE, affine32, key_of, philox4x32_10, unit  # noqa: F401
from yardstick_common import gamma

TILE = 256                                        # the samples a workgroup of csrc/time_warp.hip takes at a time
NS = (1, 2, 33, TILE - 1, TILE, TILE + 1, 1025, 4099, 16000)
SPEEDS = (0.5, 0.8, 1.0, 1.25, 2.0)
# (Hz, relative depth, phase in cycles): the deep slow one is +-1273 a samples wide, so it starts at phase 1/2, where the excursion is 0
# and the slope of p the smallest there is, a (1 - depth) -- at any other phase a short row would be read outside itself, all silence
FLUTTERS = (None, (4.0, 0.01, 0.3), (0.5, 0.25, 0.5))
SAMPLE_RATE = 16000.0
ZEROS, RES = 16, 512


# ------------------------------------------------------------------------------------------ the table
@functools.lru_cache(maxsize=None)
def table(zeros=ZEROS, res=RES):
    """sinc(v) * 0.5 (1 + cos(pi v / zeros)) at v = i / res, i < zeros * res + 2; entry 0 exactly 1, the other multiples of res and the
    last two entries exactly 0; float32"""
    v = np.arange(zeros * res + 2) / float(res)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.sin(np.pi * v) / (np.pi * v) * 0.5 * (1.0 + np.cos(np.pi * v / zeros))
    t[0] = 1.0
    t[np.arange(res, zeros * res + 2, res)] = 0.0
    t[-2:] = 0.0
    t = t.astype(np.float32)
    t.setflags(write=False)
    return t


# ------------------------------------------------------------------------------------------ the map
def clamp_c(c):
    c = np.float32(c)
    return np.float32(1.0) if np.isnan(c) else min(max(c, np.float32(0.25)), np.float32(1.0))


def sinpi(v):
    k = np.rint(v)
    return np.sin(np.pi * (v - k)) * (1.0 - 2.0 * np.mod(k, 2.0))


def position(prm, n):
    a, off, d, w, phi = (float(np.float32(v)) for v in prm[:5])
    t = np.arange(n, dtype=np.float64)
    p = a * t + off
    if d != 0.0:
        q = w * t + phi
        p = p + d * sinpi(2.0 * (q - np.floor(q)))
    return p


def taps(prm, n, tab, Z=ZEROS, R=RES):
    """(k, W, inside, p): k (n, J) int64 clamped into the row, W (n, J) float64 weights with zeros outside the support and outside the
    row, inside (n, J) the predicate c |p - k| < Z and 0 <= k < n, p (n,)"""
    c = float(clamp_c(prm[5]))
    p = position(prm, n)
    H = int(math.ceil(Z / c))
    k = (np.floor(p) - H)[:, None] + np.arange(2 * H + 2, dtype=np.float64)[None, :]
    v = c * np.abs(p[:, None] - k)
    inside = (v < Z) & (k >= 0) & (k < n)
    s = np.where(v < Z, v, 0.0) * R
    i = np.floor(s).astype(np.int64)
    t64 = tab.astype(np.float64)
    W = np.where(inside, c * (t64[i] + (s - i) * (t64[i + 1] - t64[i])), 0.0)
    return np.clip(k, 0, n - 1).astype(np.int64), W, inside, p


def _lip_eps(prm, p, tab, R):
    c = float(clamp_c(prm[5]))
    lip = c * c * R * float(np.abs(np.diff(tab.astype(np.float64))).max())
    return lip * 2.0 ** -50 * (np.abs(p) + abs(float(np.float32(prm[2]))))


def forward(x, params, tab, Z=ZEROS, R=RES):
    """(y64, bound), both (rows, n) float64"""
    x = np.asarray(x, dtype=np.float64)
    y, b = np.zeros_like(x), np.zeros_like(x)
    n = x.shape[1]
    for r, prm in enumerate(np.asarray(params)):
        k, W, inside, p = taps(prm, n, tab, Z, R)
        xk = x[r][k]
        y[r] = (W * xk).sum(axis=1)
        b[r] = gamma(inside.sum(axis=1) + 4) * np.abs(W * xk).sum(axis=1) + _lip_eps(prm, p, tab, R) * (inside * np.abs(xk)).sum(axis=1)
    return y, b


def adjoint(dy, params, tab, Z=ZEROS, R=RES):
    """(dx64, bound): dx[k] = sum_t W(p(t) - k) dy[t], the transposed map"""
    dy = np.asarray(dy, dtype=np.float64)
    dx, b = np.zeros_like(dy), np.zeros_like(dy)
    n = dy.shape[1]
    for r, prm in enumerate(np.asarray(params)):
        k, W, inside, p = taps(prm, n, tab, Z, R)
        kk = k[inside]
        terms = (W * dy[r][:, None])[inside]
        dx[r] = np.bincount(kk, weights=terms, minlength=n)
        count = np.bincount(kk, minlength=n)
        slope = (_lip_eps(prm, p, tab, R) * np.abs(dy[r]))[:, None] * inside
        b[r] = gamma(count + 4) * np.bincount(kk, weights=np.abs(terms), minlength=n) + np.bincount(kk, weights=slope[inside], minlength=n)
    return dx, b


def matrix(prm, n, tab, Z=ZEROS, R=RES):
    k, W, inside, _ = taps(prm, n, tab, Z, R)
    M = np.zeros((n, n))
    t = np.broadcast_to(np.arange(n)[:, None], k.shape)
    M[t[inside], k[inside]] = W[inside]
    return M


# ------------------------------------------------------------------------------------------ the cases
def derived(a, off, flutter, sample_rate=SAMPLE_RATE):
    """one parameter row as the Python layer derives it: w = hz / sample_rate, d = depth a / (2 pi w), c = min(1, 1 / (a (1 + depth)))"""
    hz, depth, phi = flutter if flutter is not None else (0.0, 0.0, 0.0)
    w = np.float32(hz / sample_rate)
    d = depth * a / (2.0 * math.pi * float(w)) if hz and depth else 0.0
    return np.array([a, off, d, w, phi if d else 0.0, min(1.0, 1.0 / (a * (1.0 + depth)))], dtype=np.float32)


def offsets(n):
    return (0.0, -7.3, 100.5, n + 50.0, -n - 50.0)


@functools.lru_cache(maxsize=None)
def case(n, fi):
    """(x, params): every speed times every offset at flutter FLUTTERS[fi], 25 rows of unit-variance data rounded to float32"""
    params = np.stack([derived(a, off, FLUTTERS[fi]) for a in SPEEDS for off in offsets(n)])
    x = np.random.default_rng(7000 * n + fi).standard_normal((len(params), n)).astype(np.float32)
    for v in (x, params):
        v.setflags(write=False)
    return x, params


@functools.lru_cache(maxsize=None)
def case_ref(n, fi, adj):
    x, params = case(n, fi)
    ref = (adjoint if adj else forward)(x, params, table())
    for v in ref:
        v.setflags(write=False)
    return ref


# ------------------------------------------------------------------------------------------ the draws (the generator is tests/draw_yardstick.py's)
def warp_params(seed, draw, rows, speed, shift_s, flutter_hz, flutter_depth, sample_rate=SAMPLE_RATE):
    """(len(rows), 6) float32: words o0..o3 of (0xFFFFFFFD, 0xFFFFFFFF, row, draw) onto speed, shift, flutter rate and depth, word o0 of
    (0xFFFFFFFC, 0xFFFFFFFF, row, draw) the phase; derived in float64 from the float32 draws and rounded once each"""
    rows = np.asarray(rows, dtype=np.uint64)
    o = philox4x32_10((WARP[0], WARP[1], rows, int(draw)), key_of(seed))
    ph = unit(philox4x32_10((WARP_PHASE[0], WARP_PHASE[1], rows, int(draw)), key_of(seed))[0])
    out = np.zeros((len(rows), 6), dtype=np.float32)
    for r in range(len(rows)):
        a = float(affine32(speed, unit(o[0][r])))
        shift = float(affine32(shift_s, unit(o[1][r])))
        hz = float(affine32(flutter_hz, unit(o[2][r]))) if flutter_hz is not None else 0.0
        depth = float(affine32(flutter_depth, unit(o[3][r]))) if flutter_depth is not None else 0.0
        w = np.float32(hz / sample_rate)
        on = w != 0 and depth != 0
        out[r] = [a, shift * sample_rate, depth * a / (2.0 * math.pi * float(w)) if on else 0.0, w, ph[r] if on else 0.0,
                  min(1.0, 1.0 / (a * (1.0 + depth)))]
    return out


# ------------------------------------------------------------------------------------------ arguments the launcher refuses
_X, _P, _T, _Y = 1 << 20, 1 << 24, 1 << 26, 1 << 28                               # made-up, never dereferenced addresses
# wm_time_warp(x, params, tab, y, rows, n, zeros, res, adjoint, stream)
BAD_ARGS = ((_X, _P, _T, _Y, 0, 1000, 16, 512, 0, None),                         # rows < 1
            (_X, _P, _T, _Y, 2, 0, 16, 512, 0, None),                            # n < 1
            (_X, _P, _T, _Y, 1, (1 << 34) + 1, 16, 512, 0, None),                # n above 2^34
            (_X, _P, _T, _Y, 2, 1000, 3, 512, 0, None),                          # zeros outside 4..32
            (_X, _P, _T, _Y, 2, 1000, 33, 512, 0, None),
            (_X, _P, _T, _Y, 2, 1000, 16, 32, 0, None),                          # res outside 64..1024, or no power of two
            (_X, _P, _T, _Y, 2, 1000, 16, 2048, 0, None),
            (_X, _P, _T, _Y, 2, 1000, 16, 500, 0, None),
            (_X, _P, _T, _Y, 2, 1000, 32, 1024, 0, None),                        # a table above 128 KiB
            (None, _P, _T, _Y, 2, 1000, 16, 512, 0, None),                       # null pointers
            (_X, None, _T, _Y, 2, 1000, 16, 512, 0, None),
            (_X, _P, None, _Y, 2, 1000, 16, 512, 0, None),
            (_X, _P, _T, None, 2, 1000, 16, 512, 1, None),
            (_X + 2, _P, _T, _Y, 2, 1000, 16, 512, 0, None),                     # misaligned
            (_X, _P + 1, _T, _Y, 2, 1000, 16, 512, 0, None),
            (_X, _P, _T + 2, _Y, 2, 1000, 16, 512, 0, None),
            (_X, _P, _T, _Y + 3, 2, 1000, 16, 512, 0, None),
            (_X, _P, _T, _X, 2, 1000, 16, 512, 0, None),                         # in place
            (_X, _P, _T, _X, 2, 1000, 16, 512, 1, None),
            (_X, _P, _T, _X + 7996, 2, 1000, 16, 512, 0, None),                  # y overlaps the last float of x
            (_X, _Y + 4000, _T, _Y, 2, 1000, 16, 512, 0, None),                  # params inside y
            (_X, _Y - 44, _T, _Y, 2, 1000, 16, 512, 0, None),                    # y overlaps the last parameter
            (_X, _P, _Y + 400, _Y, 2, 1000, 16, 512, 0, None),                   # the table inside y
            (_X, _P, _Y - 4, _Y, 2, 1000, 16, 512, 0, None))                     # y overlaps the table's second word
