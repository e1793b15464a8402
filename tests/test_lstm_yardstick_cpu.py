"""tests/lstm_yardstick.py without a GPU: the float32 restatement of the kernels' gate functions meets the sweep's bounds; the trace that
supplies the saved tensors is the oracle's loop bit for bit; every case of the recurrence tables is well conditioned (its bar stays
below test_gpu_parity.py's tolerances) and the saturated cases are saturated; and a planted defect -- tanh_s with a 1e-6 error, the i and
f gates exchanged -- misses the bounds."""
import numpy as np
import pytest
import torch

import lstm_yardstick as Y
from loss_yardstick import bar
from oracle import wm_oracle as O
from yardstick_common import assert_within, ulp32

ROUTE = [("route", B, T) for T in Y.ROUTE_T for B in Y.ROUTE_B]
SAVED = [("route", 2, T) for T in Y.SAVED_T]
SATURATED = [("saturated", B, T) for B, T in Y.SATURATED]
ALL = ROUTE + SAVED + SATURATED + [("zero_x",) + Y.ZERO_X, ("all_zero",) + Y.ALL_ZERO]


def within(a, ref, bound):
    return bool(np.all(np.abs(np.asarray(a, dtype=np.float64) - ref) <= bound))


# ------------------------------------------------------------------------------------------------------------ the activation sweep
@pytest.mark.parametrize("neg_zero", [False, True])
def test_sweep_restatement_meets_the_bounds(neg_zero):
    z = Y.sweep_z(neg_zero)
    assert z.dtype == np.float32 and (z == 0).sum() == 2 and np.signbit(z[z == 0]).all() == neg_zero
    assert {2.0 ** -126, 1e4, 88.8, 44.0}.issubset({float(np.float32(v)) for v in np.abs(z)} | {88.8, 1e4})
    xp = Y.sweep_xp(neg_zero)
    assert xp.shape == (Y.SWEEP_B, Y.SWEEP_T, 256) and xp.dtype == np.float32
    cols = xp[:, 0, :].reshape(-1, 4)
    for q in range(4):                                  # every z stands four times in every gate's columns
        vals, counts = np.unique(cols[:, q].view(np.int32), return_counts=True)
        assert vals.size == np.unique(z.view(np.int32)).size and counts.min() >= 4
    ref, got = Y.sweep_ref(xp), Y.sweep_restated(xp)
    for k in ("gates", "c", "h"):
        assert ref[k].dtype == np.float64 and np.all(np.isfinite(got[k]))
        assert_within(got[k], ref[k], ref[k + "_bound"], f"sweep {k}")
    # what csrc/lstm.hpp used to claim, 3e-8 (+ half an ulp of the value), is missed by correctly rounded float32 arithmetic alone
    sig = (np.arange(256) % 4 != 2)[None, :] & np.ones((Y.SWEEP_B, 1), dtype=bool)
    err = np.abs(got["gates"].astype(np.float64) - ref["gates"])
    claimed = Y.SIGM_ABS_CLAIMED + ulp32(ref["gates"]) / 2
    worst = np.unravel_index(np.argmax(np.where(sig, err - claimed, -1.0)), err.shape)
    print(f"float32 sigm: {err[worst]:.2e} at z = {ref['z'][worst]:.3f}, the header's claim allows {claimed[worst]:.2e}")
    assert err[worst] > claimed[worst]
    assert float(np.max(Y.d_sigm(np.linspace(-100, 100, 20001)))) <= 1.9e-7 and float(np.max(Y.d_tanh(np.linspace(-50, 50, 20001)))) <= 4.3e-7
    # exact values the degenerate tests rely on
    zero = xp[:, 0, :] == 0
    assert np.all(got["gates"][zero & (np.arange(256) % 4 != 2)[None, :]] == 0.5) and np.all(got["gates"][zero & (np.arange(256) % 4 == 2)[None, :]] == 0.0)


@pytest.mark.parametrize("defect", ["tanh_1e-6", "swap_if"])
def test_sweep_defects_miss_the_bounds(defect):
    xp = Y.sweep_xp()
    ref, got = Y.sweep_ref(xp), Y.sweep_restated(xp, defect)
    assert not within(got["gates"], ref["gates"], ref["gates_bound"])
    assert not within(got["c"], ref["c"], ref["c_bound"]) and not within(got["h"], ref["h"], ref["h_bound"])


# ------------------------------------------------------------------------------------------------------------------ the recurrence
def test_route_table_covers_every_launch_choice():
    assert {T < 8 for T in Y.ROUTE_T} == {True, False} and 4 in Y.ROUTE_T and 8 in Y.ROUTE_T
    ws = {T for T in Y.ROUTE_T if T % 32 == 0 and T >= 64}
    assert ws == {64} and {32, 60, 68}.issubset(Y.ROUTE_T) and {12, 28}.issubset(Y.ROUTE_T)
    assert Y.expected_launches(4) == {"wm_lstm_xproj": 1, "wm_lstm_fwd": 1, "wm_lstm_bwd": 1, "wm_lstm_dx": 1, "wm_lstm_wgrad": 1}
    assert Y.expected_launches(64) == {"wm_lstm_fwd_fused": 1, "wm_lstm_bwd_wgrad": 1, "wm_lstm_dx": 1}
    assert set(Y.expected_launches(32)) == set(Y.expected_launches(60)) == {"wm_lstm_fwd_fused", "wm_lstm_bwd", "wm_lstm_dx", "wm_lstm_wgrad"}
    assert all(set(Y.expected_launches(T)) <= set(Y.LAUNCHES) for T in Y.ROUTE_T)


@pytest.mark.parametrize("kind,B,T", ALL)
def test_cases_are_well_conditioned(kind, B, T):
    r64, r32 = Y.lstm_ref(kind, B, T)
    x, wi, wh, bi, bh, gg = Y.lstm_inputs(kind, B, T)
    assert x.shape == gg.shape == (B, 64, T) and wi.shape == wh.shape == (256, 64)
    for name in ("h", "gates", "cst") + Y.GRAD_NAMES:
        assert r64[name].dtype == torch.float64 and r32[name].dtype == torch.float32 and bool(torch.isfinite(r64[name]).all())
        if not ((kind == "zero_x" and name == "dW_ih") or (kind == "all_zero" and name in ("h", "cst", "dx", "dW_ih", "dW_hh"))):
            assert float(r64[name].abs().max()) > 0.0, f"{name} is identically zero"
        b = bar(r32[name], r64[name], Y.floor_of(name))
        cap = Y.PARITY_FWD_TOL if name in ("h", "gates", "cst") else Y.PARITY_GRAD_TOL
        print(f"{kind} ({B}, {T}) {name}: e32 {Y.rel_err(r32[name], r64[name]):.2e}, bar {b:.2e}")
        assert b <= cap, f"{name}: the case needs a bar of {b:.2e}: badly conditioned"
    assert r64["gates"].shape == (B, T, 256) and r64["cst"].shape == (B, T, 64)
    # the trace is the oracle's loop
    h_trace, _, _ = Y.lstm_trace(x.permute(0, 2, 1), wi, wh, bi, bh)
    assert torch.equal(h_trace, O.lstm_forward(x.permute(0, 2, 1), wi, wh, bi, bh))
    assert Y.rel_err(h_trace.permute(0, 2, 1), r32["h"]) <= 1e-6          # (under autograd torch may batch the projection differently)
    if kind == "all_zero":
        for dt in (0, 1):
            r = (r64, r32)[dt]
            assert all(float(r[n].abs().max()) == 0.0 for n in ("h", "cst", "dx", "dW_ih", "dW_hh")) and float(r["db_ih"].abs().max()) > 0.0
            g = r["gates"].reshape(-1, 64, 4)
            assert bool((g[..., [0, 1, 3]] == 0.5).all()) and bool((g[..., 2] == 0.0).all())
    if kind == "zero_x":
        assert float(x.abs().max()) == 0.0 and float(r64["dW_ih"].abs().max()) == 0.0 and float(r64["db_ih"].abs().max()) > 0.0


@pytest.mark.parametrize("kind,B,T", SATURATED)
def test_saturated_cases_are_saturated(kind, B, T):
    r64, _ = Y.lstm_ref(kind, B, T)
    share = Y.saturation_share(r64["gates"])
    x, wi, wh, bi, bh, _ = Y.lstm_inputs(kind, B, T)
    pre = (x.double().permute(0, 2, 1) @ wi.double().t() + (bi + bh).double()).abs()
    print(f"saturated ({B}, {T}): {share:.3f} of the gate activations outside [0.01, 0.99], largest input pre-activation {float(pre.max()):.1f}")
    assert share >= 0.25 and float(pre.max()) >= 20.0
    # cells keep their state: some |c| grows past what one step can add
    assert float(r64["cst"].abs().max()) > 2.0


@pytest.mark.parametrize("kind,B,T", [("route", 3, 4), ("route", 1, 64), ("saturated", 2, 36)])
def test_exchanged_gates_miss_the_bar(kind, B, T):
    """(a tanh_s that is 1e-6 off stays below the recurrence's floors: the sweep is the test that sees it)"""
    r64, r32 = Y.lstm_ref(kind, B, T)
    bad = Y.lstm_defect(kind, B, T, "swap_if")
    missed = [n for n in ("h", "gates", "cst") + Y.GRAD_NAMES if Y.rel_err(bad[n], r64[n]) > bar(r32[n], r64[n], Y.floor_of(n))]
    print(f"{kind} ({B}, {T}) i and f exchanged: misses {missed}")
    assert {"h", "gates", "cst", "dx", "dW_ih", "db_ih"}.issubset(missed)
