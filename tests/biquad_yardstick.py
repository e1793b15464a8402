"""The float64 yardstick of the biquad section in float mode, for tests/test_gpu_biquad.py, tests/test_gpu_attacks.py (Lowpass) and the
coefficient check of tests/test_biquad_cpu.py (`import biquad_yardstick as Y`).  It uses nothing from the package:
y64 = scipy.signal.lfilter in float64 with the float32-rounded coefficients of the published RBJ low-pass section, on the float64 image
of the input.  Tolerance (derived, nothing tuned, no rtol):

    |y - y64| <= (|g| * e)[t] + tail + spacing(float32(|y64|))

g: float64 impulse response of 1 / A(z);  e[t] = gamma6 (|b0 x[t]| + |b1 x[t-1]| + |b2 x[t-2]| + |a1 y64[t-1]| + |a2 y64[t-2]|), gamma6 =
6u / (1 - 6u), u = 2^-24: the local rounding error of one step of the direct-form-I recursion (five roundings, six allowed), carried to
the output by the recursion itself;  tail = max|x| sum_{k >= W} |h[k]|, h the impulse response of the whole section and W =
ops.biquad_warm(coeffs): what a chunk that starts W samples early from a zero state can have missed;  the spacing term is the
representation of y64 in float32.  (|g| is cut where it has decayed below 1e-40 of its start, which only makes the bound smaller.)"""
import functools
import math

import numpy as np
from scipy.signal import lfilter

from yardstick_common import gamma, ulp32

GAMMA6 = gamma(6)


@functools.lru_cache(maxsize=None)
def section(rate, cutoff, Q=0.707):
    """(b (3,), a (3,)) float64 images of the float32-rounded RBJ low-pass coefficients, a[0] = 1"""
    w0 = 2.0 * math.pi * cutoff / rate
    alpha = math.sin(w0) / (2.0 * Q)
    cw = math.cos(w0)
    b = np.array([(1.0 - cw) / 2.0, 1.0 - cw, (1.0 - cw) / 2.0], dtype=np.float64)
    a = np.array([1.0 + alpha, -2.0 * cw, 1.0 - alpha], dtype=np.float64)
    return (b / a[0]).astype(np.float32).astype(np.float64), (a / a[0]).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def responses(rate, cutoff, W):
    """(|g| cut where it has decayed below 1e-40 of its start, sum_{k >= W} |h[k]|)"""
    b, a = section(rate, cutoff)
    imp = np.zeros(W + 60000)
    imp[0] = 1.0
    g = np.abs(lfilter([1.0], a, imp))
    h = np.abs(lfilter(b, a, imp))
    live = np.nonzero(g > 1e-40 * g[0])[0]
    return g[:int(live[-1]) + 1], float(h[W:].sum())


def shifted(v, k):
    out = np.zeros_like(v)
    if k < v.shape[-1]:
        out[..., k:] = v[..., :v.shape[-1] - k]
    return out


def yardstick(x, rate, cutoff, W):
    """x (rows, n) float -> (y64 (rows, n), bound (rows, n)), both float64"""
    b, a = section(rate, cutoff)
    x = np.asarray(x, dtype=np.float64)
    y = lfilter(b, a, x, axis=-1)
    e = GAMMA6 * (np.abs(b[0] * x) + np.abs(b[1] * shifted(x, 1)) + np.abs(b[2] * shifted(x, 2)) +
                  np.abs(a[1] * shifted(y, 1)) + np.abs(a[2] * shifted(y, 2)))
    g, tail = responses(rate, cutoff, W)
    n = x.shape[-1]
    carried = np.stack([np.convolve(row, g[:n])[:n] for row in e])
    return y, carried + np.abs(x).max() * tail + ulp32(y)
