"""The two formulations of the resampler in tests/resample_yardstick.py held against each other, in float64 alone: yardstick() (frames of
the whole recording times the table) and apply64 / adjoint64 (A @ x and A.T @ dy over the periods).  Nothing from the package.

Bounds (derived): both sides sum the same float64 products in an order a BLAS may choose, so each is within gamma_n * sum |terms| of the
exact value, gamma_n = n v / (1 - n v), v = 2**-53, n the number of roundings a product can pass through (Higham, Accuracy and Stability,
ch. 3): K for one output sample.  No golden file: the table goes through np.sin / np.cos, whose last bit may differ between machines."""
import numpy as np
import pytest

from resample_yardstick import adjoint64, apply64, design, yardstick
from yardstick_common import assert_within

PAIRS = [(16000, 8000), (8000, 16000), (16000, 12000), (44100, 16000), (16000, 12345)]
V = 2.0 ** -53


def gamma64(n):
    return n * V / (1 - n * V)


def lengths(P):
    """one sample, just below one period (the empty recording where P = 1), one period, several periods and a rest"""
    return sorted({1, P - 1, P, 7 * P + 3})


def cuts(full):
    """output lengths: all ceil(Q*N/P) samples, and cut below that where there is anything to cut"""
    return sorted({full, min(full, max(full // 2, 1))})


@pytest.mark.parametrize("orig,new", PAIRS)
def test_apply64_is_the_yardstick(orig, new):
    P, Q, width, K, h32 = design(orig, new)
    h, habs = h32.astype(np.float64), np.abs(h32).astype(np.float64)
    for N in lengths(P):
        x = np.random.default_rng(N).standard_normal(N)
        y, _ = yardstick(x, orig, new)
        full = -((-Q * N) // P)
        assert y.shape == (full,)
        for L in cuts(full):
            bound = 2 * gamma64(K) * apply64(habs, P, width, np.abs(x), L)
            assert_within(apply64(h, P, width, x, L), y[:L], bound, f"{orig}->{new} N={N} L={L}")


@pytest.mark.parametrize("orig,new", PAIRS)
def test_adjoint64_is_the_transpose_of_apply64(orig, new):
    """<A x, w> = <x, A.T w>.  Both sides sum the products h x w: on the left a product passes through at most K roundings of A @ x and L
    of the inner product, on the right through at most Q of dy @ h, K of the scatter over the periods and N of the inner product."""
    P, Q, width, K, h32 = design(orig, new)
    h, habs = h32.astype(np.float64), np.abs(h32).astype(np.float64)
    for N in lengths(P):
        rng = np.random.default_rng(1000 + N)
        x = rng.standard_normal(N)
        full = -((-Q * N) // P)
        for L in cuts(full):
            w = rng.standard_normal(L)
            lhs = float(apply64(h, P, width, x, L) @ w)
            rhs = float(x @ adjoint64(h, P, width, w, N))
            room = (gamma64(K + L) + gamma64(Q + K + N)) * float(apply64(habs, P, width, np.abs(x), L) @ np.abs(w))
            print(f"{orig}->{new} N={N} L={L}: <Ax, w> - <x, A.T w> = {lhs - rhs:.3e}, room {room:.3e}")
            assert abs(lhs - rhs) <= room
