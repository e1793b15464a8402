"""The two formulations of the resampler in tests/resample_yardstick.py held against each other, in float64 alone: yardstick() (frames of
the whole recording times the table) and apply64 / adjoint64 (A @ x and A.T @ dy over the periods).  Nothing from the package.

Bounds (derived): both sides sum the same float64 products in an order a BLAS may choose, so each is within gamma_n * sum |terms| of the
exact value, gamma_n = n v / (1 - n v), v = 2**-53, n the number of roundings a product can pass through (Higham, Accuracy and Stability,
ch. 3): K for one output sample.  No golden file: the table goes through np.sin / np.cos, whose last bit may differ between machines.

Also what every yardstick module must be, checked for tests/bn_yardstick.py and tests/lstm_yardstick.py: it imports nothing from the
package or from the GPU test support, its case tables are not empty, and its bounds are positive float64 numbers."""
import ast
import os

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


# ------------------------------------------------------------------------------------- the BatchNorm and LSTM yardsticks as modules
ALLOWED_IMPORTS = {"functools", "math", "numpy", "torch", "torch.nn.functional", "oracle", "yardstick_common", "loss_yardstick"}


@pytest.mark.parametrize("module", ["bn_yardstick", "lstm_yardstick"])
def test_a_yardstick_imports_nothing_from_the_package(module):
    tree = ast.parse(open(os.path.join(os.path.dirname(__file__), module + ".py")).read())
    names = set()
    for node in ast.walk(tree):                     # imports inside functions count too
        if isinstance(node, ast.Import):
            names.update(a.name for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            names.add(node.module)
    assert names and names <= ALLOWED_IMPORTS, f"{module} imports {sorted(names - ALLOWED_IMPORTS)}"
    assert not any(n.startswith(("awm_amd", "gpu_support")) for n in names)
    assert ast.get_docstring(tree) and "MI355X" in ast.get_docstring(tree), "the measured ratios belong in the docstring"


def test_the_bn_yardstick_tables_and_bounds():
    import bn_yardstick as Y
    for table in (Y.FIN_NPARTS, Y.FIN_CASES, Y.EVAL_RV, Y.TAIL_T, Y.TAIL_B, Y.BWD_NPARTS, Y.BWD_CASES, Y.BWD_NMAX, Y.GS_K, Y.GS_L, Y.GS_N,
                  Y.GS_CLAMP, Y.FROM_MAX_N, Y.ROWS_CASES, Y.CHAIN_SHAPES, Y.CHAIN_RATIOS, Y.CHAIN_NAMES):
        assert len(table) > 0
    assert set(Y.FIN_NPARTS) == {1, 15, 16, 17, 256, 1000} and set(Y.TAIL_T) == {4, 28, 32, 36, 4092, 4096, 4100, 8196}
    assert set(Y.BWD_NPARTS) == {1, 16, 17, 300} and set(Y.CHAIN_RATIOS) == {0, 3, 30} and Y.ZERO_SUM == 2.0 ** -45
    inp = Y.finalize_inputs(17, 64)
    ref = Y.finalize_ref(inp)
    for k in Y.FIN_NAMES:
        b = Y.finalize_bound(ref, k)
        assert b.dtype == np.float64 and np.all(b > 0) and np.all(b <= 2.0 ** -23 * np.abs(ref[k]) + 2 * Y.TINY)
    ev = Y.eval_ref(Y.eval_inputs())
    assert all(np.all(Y.eval_bound(ev, k) > 0) and Y.eval_bound(ev, k).dtype == np.float64 for k in ("scale", "shift"))
    _, _, bound = Y.tail_ref(*Y.tail_inputs(1, 36))
    assert bound.dtype == np.float64 and np.all(bound > 0)


def test_the_lstm_yardstick_tables_and_bounds():
    import lstm_yardstick as Y
    for table in (Y.ROUTE_T, Y.ROUTE_B, Y.SAVED_T, Y.SATURATED, Y.LAUNCHES, Y.GRAD_NAMES):
        assert len(table) > 0
    assert set(Y.ROUTE_T) == {4, 8, 12, 28, 32, 60, 64, 68} and set(Y.SATURATED) == {(2, 36), (1, 96)} and set(Y.SAVED_T) == {8, 36, 64}
    assert Y.FWD_FLOOR == Y.PARITY_FWD_TOL / 10 and Y.GRAD_FLOOR == Y.PARITY_GRAD_TOL / 10
    ref = Y.sweep_ref(Y.sweep_xp())
    for k in ("gates", "c", "h"):
        assert ref[k].dtype == ref[k + "_bound"].dtype == np.float64 and np.all(ref[k + "_bound"] > 0) and ref[k].shape == ref[k + "_bound"].shape
