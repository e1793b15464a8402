"""The resampling attack on the host: the adjoint table of the resampler, attacks.Resampled on CPU tensors, resample(mixdown=False), exports.

The yardstick is apply64 / adjoint64 / attack64 / attack_grad64 of tests/resample_yardstick.py, float64 numpy with nothing from the
package; the derived one-stage and two-stage tolerances stand in that module's docstring."""
import ctypes
import os

import numpy as np
import pytest
import torch

import awm_amd
from awm_amd import _lib, ops
from resample_yardstick import adjoint64, apply64, attack64, attack_grad64, design, rows_signal
from yardstick_common import assert_within

TABLE_PAIRS = [(16000, 8000), (8000, 16000), (16000, 12000), (16000, 44100), (44100, 16000)]
RATES = [8000, 12000, 44100]


def dense_matrix(orig, new, N, L):
    """the small (L, N) float32 matrix A of one row, entry by entry from design()"""
    P, Q, width, K, h32 = design(orig, new)
    A = np.zeros((L, N), dtype=np.float32)
    for o in range(L):
        m, i = divmod(o, Q)
        for j in range(K):
            n = m * P + j - width
            if 0 <= n < N:
                A[o, n] = h32[i, j]
    return A


# ------------------------------------------------------------------------------------------ 1. the adjoint table
@pytest.mark.parametrize("orig,new", TABLE_PAIRS)
def test_adjoint_table_is_the_transpose(orig, new):
    P, Q, width, K, h32 = design(orig, new)
    fwd = ops.resample_table(orig, new)
    assert np.array_equal(fwd["dense"].numpy(), h32), "the package's float64 evaluation rounds a tap differently from numpy's"
    tab = ops.resample_adjoint_table(orig, new)
    assert ops.resample_adjoint_table(orig, new) is tab                                       # cached
    Pa, Qa, wa, Wa = tab["P"], tab["Q"], tab["width"], tab["W"]
    taps, first = tab["taps"].numpy(), tab["first"].numpy()
    assert (Pa, Qa) == (Q, P) and taps.dtype == np.float32 and taps.shape == (Qa, Wa) and first.shape == (Qa,) and first.dtype == np.int32
    assert 0 < Wa <= 2 * wa + Pa
    assert first.min() >= 0 and first.max() <= 2 * wa + Pa - Wa, "the kernel's clamp would move a phase"
    assert Wa % 2 == 1 or Wa == 2 * wa + Pa
    print(f"{orig}->{new}: adjoint P'={Pa} Q'={Qa} width'={wa} W'={Wa}, {taps.nbytes + first.nbytes} bytes")
    N = 4 * P + K + 3
    full = -((-Q * N) // P)
    for L in (full, full - Q - 1):                                                            # ... and cut below ceil(Q*N/P)
        A = dense_matrix(orig, new, N, L)
        # the kernel's own indexing with this table on (dy, L -> N): dx[m*Q' + p] += taps'[p][k] * dy[m*P' + first'[p] + k - width']
        B = np.zeros((N, L), dtype=np.float32)
        for n in range(N):
            m, p = divmod(n, Qa)
            for k in range(Wa):
                o = m * Pa + int(first[p]) + k - wa
                if 0 <= o < L:                                                                # outside [0, L) the kernel reads dy as zero
                    B[n, o] = taps[p, k]
        assert np.array_equal(B, A.T), f"{orig}->{new} L={L}: the expanded adjoint table is not A.T"


def test_adjoint_table_runs_and_equal_rates():
    """the longest runs of the adjoint phases: 13 for 16 k -> 8 k / 12 k and 44.1 k -> 16 k, 25 for 8 k -> 16 k, 34 for 16 k -> 44.1 k (made odd: 35)"""
    for (orig, new), run in {(16000, 8000): 13, (16000, 12000): 13, (44100, 16000): 13, (8000, 16000): 25, (16000, 44100): 34}.items():
        P, Q, width, K, h32 = design(orig, new)
        tab = ops.resample_adjoint_table(orig, new)
        assert tab["W"] in (run, run + 1), (orig, new, tab["W"])
        assert int((tab["taps"] != 0).sum()) == int((h32 != 0).sum())
    same = ops.resample_adjoint_table(16000, 16000)
    assert (same["P"], same["Q"], same["W"]) == (1, 1, 1)
    with pytest.raises(ValueError):
        ops.resample_adjoint_table(16000, 0)


# ------------------------------------------------------------------------------------------ 2. Resampled on CPU tensors
@pytest.mark.parametrize("rate", RATES)
def test_resampled_cpu_vs_float64(rate):
    for T in (1, 37, 4001):
        x = rows_signal(3, T, seed=rate % 97)
        y = awm_amd.Resampled(rate)(x.view(3, 1, T))
        assert tuple(y.shape) == (3, 1, T) and y.dtype == torch.float32
        for r in range(3):
            ref, bound = attack64(x[r].double().numpy(), rate)
            assert_within(y[r, 0].numpy(), ref, bound, f"Resampled({rate}) T={T} row {r}")
            alone = awm_amd.Resampled(rate)(x[r])
            assert tuple(alone.shape) == (T,)
            assert torch.equal(alone, y[r, 0]), f"row {r} of a batch differs from the row by itself"


def test_resampled_shapes_and_arguments():
    att = awm_amd.Resampled(8000)
    for shape in ((3, 1, 501), (2, 777), (333,)):
        x = torch.randn(*shape)
        y = att(x)
        assert tuple(y.shape) == shape and y.dtype == torch.float32
    x = torch.randn(2, 1, 100)
    assert awm_amd.Resampled(16000)(x) is x
    assert awm_amd.Resampled(44100, sample_rate=44100)(x) is x
    for bad in (0, -8000, 8000.5, "8000", None):
        with pytest.raises(ValueError):
            awm_amd.Resampled(bad)
    with pytest.raises(ValueError):
        awm_amd.Resampled(8000, sample_rate=0)
    with pytest.raises(ValueError):
        att(torch.zeros(2, 1, 0))
    with pytest.raises(TypeError):
        att([0.0, 1.0])
    assert "rate=8000" in repr(att) and "sample_rate=16000" in repr(att)
    assert awm_amd.attacks.Resampled is awm_amd.Resampled and "Resampled" in awm_amd.__all__


@pytest.mark.parametrize("rate", RATES)
def test_resampled_cpu_gradient_vs_float64(rate):
    for T in (37, 4001):
        x = rows_signal(2, T, seed=7).view(2, 1, T).requires_grad_()
        g = rows_signal(2, T, seed=8)
        y = awm_amd.Resampled(rate)(x)
        (y * g.view(2, 1, T)).sum().backward()
        assert tuple(x.grad.shape) == (2, 1, T)
        for r in range(2):
            ref, bound = attack_grad64(g[r].double().numpy(), rate)
            assert_within(x.grad[r, 0].numpy(), ref, bound, f"Resampled({rate}) gradient T={T} row {r}")


def test_yardstick_adjoint_is_the_transpose():
    """the test's own apply64 / adjoint64 against the entry-by-entry matrix, so a mistake in them does not pass for a mistake in the package"""
    for orig, new in ((16000, 12000), (8000, 16000)):
        P, Q, width, K, h32 = design(orig, new)
        N = 3 * P + 5
        L = -((-Q * N) // P) - 1
        A = dense_matrix(orig, new, N, L).astype(np.float64)
        rng = np.random.default_rng(3)
        x, dy = rng.standard_normal(N), rng.standard_normal(L)
        assert np.allclose(apply64(h32.astype(np.float64), P, width, x, L), A @ x, rtol=0, atol=1e-13)
        assert np.allclose(adjoint64(h32.astype(np.float64), P, width, dy, N), A.T @ dy, rtol=0, atol=1e-13)


# ------------------------------------------------------------------------------------------ 3. resample(mixdown=False)
def test_resample_without_mixdown_cpu():
    x = rows_signal(3, 2001, seed=5)
    for orig, new in ((48000, 16000), (16000, 44100)):
        y = awm_amd.resample(x, orig, new, mixdown=False)
        assert tuple(y.shape) == (3, ops.resample_length(2001, orig, new)) and y.dtype == torch.float32
        assert torch.equal(y, torch.cat([awm_amd.resample(x[c:c + 1], orig, new) for c in range(3)], dim=0))
        assert torch.equal(awm_amd.resample(x, orig, new, mixdown=True), awm_amd.resample(x, orig, new))
        assert tuple(awm_amd.resample(x, orig, new).shape) == (1, y.shape[1])
    assert awm_amd.resample(x, 16000, 16000, mixdown=False) is x
    assert tuple(awm_amd.resample(x[0], 48000, 16000, mixdown=False).shape) == (1, 667)


# ------------------------------------------------------------------------------------------ 4. exports
def test_rows_entry_point_is_declared_and_exported():
    protos = _lib.parse_header()
    assert "wm_resample_rows" in protos
    assert [name for _, name in protos["wm_resample_rows"]] == ["x", "taps", "first", "y", "rows", "N", "L", "P", "Q", "width", "W", "stream"]
    assert os.path.exists(_lib.LIB_PATH), "build with __graft_entry__.build()"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "wm_resample_rows"), "wm_resample_rows declared in include/wm_hip.h but not exported"
    assert hasattr(ops, "resample_rows") and hasattr(ops, "ResampleRowsFn")
