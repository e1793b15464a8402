"""The main16 LSTM kernels against the float64 yardsticks of tests/lstm_yardstick.py, where test_gpu_parity.py does not look: the gate
functions themselves over the whole range of z (csrc/lstm.hpp's accuracy statement, tested directly through step 0 of wm_lstm_fwd), every
length at which ops._lstm_fwd / _lstm_bwd change the launch (with a spy that holds each length to its launch), the saved gate
activations and cell states of every forward entry point, gates driven deep into saturation, and the degenerate inputs.  The bounds
and the rule max(8 * e32, floor) are lstm_yardstick.py's; tests/test_lstm_yardstick_cpu.py holds the float32 restatements to them and
shows the planted defects missing them.  Every comparison prints its measured distance / bound."""
import numpy as np
import pytest
import torch

import lstm_yardstick as Y
from gpu_support import _spy, awm, bits, dev, p, st, to_dev  # noqa: F401
from yardstick_common import assert_within, ulp32

pytestmark = pytest.mark.gpu


def nan_like(*shape, dev):
    return torch.full(shape, float("nan"), device=dev)


# ------------------------------------------------------------------------------------------------------------ 1. activation sweep
@pytest.mark.parametrize("neg_zero", [False, True])
def test_activation_sweep(awm, dev, neg_zero):
    xp = Y.sweep_xp(neg_zero)
    ref = Y.sweep_ref(xp)
    B, T = Y.SWEEP_B, Y.SWEEP_T
    w_hh = Y.uniform(256, 64, seed=3, scale=0.125).to(dev)
    h, gates, cst = nan_like(B, 64, T, dev=dev), nan_like(B, T, 256, dev=dev), nan_like(B, T, 64, dev=dev)
    xpd = to_dev(xp, dev)
    awm.lib.wm_lstm_fwd(p(xpd), p(w_hh), p(h), p(gates), p(cst), B, T, st())
    torch.cuda.synchronize()
    for t in (h, gates, cst):
        assert bool(torch.isfinite(t).all()), "a gate function gave inf or NaN"
    g0 = gates[:, 0].cpu().numpy()
    # the measured worst case of either function, with the z where it occurs, next to what csrc/lstm.hpp used to state
    err = np.abs(g0.astype(np.float64) - ref["gates"])
    is_g = (np.arange(256) % 4 == 2)[None, :] & np.ones((B, 1), dtype=bool)
    for name, sel in (("sigm", ~is_g), ("tanh_s", is_g)):
        w = np.unravel_index(np.argmax(np.where(sel, err, -1.0)), err.shape)
        print(f"{name}: largest |error| {err[w]:.3e} at z = {ref['z'][w]!r} (value {ref['gates'][w]:.6f}, its ulp32 / 2 {ulp32(ref['gates'][w]) / 2:.2e}; "
              f"the header's earlier figure {Y.SIGM_ABS_CLAIMED * (2 if name == 'tanh_s' else 1):.0e})")
    assert_within(g0, ref["gates"], ref["gates_bound"], "wm_lstm_fwd step 0: sigm / tanh_s")
    assert_within(cst[:, 0].cpu().numpy(), ref["c"], ref["c_bound"], "wm_lstm_fwd step 0: c_0 = i g")
    assert_within(h[:, :, 0].cpu().numpy(), ref["h"], ref["h_bound"], "wm_lstm_fwd step 0: h_0 = o tanh_s(c_0)")
    zero = xp[:, 0, :] == 0
    assert np.all(g0[zero & ~is_g] == 0.5) and not g0[zero & is_g].view(np.int32).any(), "sigm(+-0) = 0.5 and tanh_s(+-0) = +0.0 exactly"


# ------------------------------------------------------------------------------------------------------------ 2. route edges
def _lstm_fn(awm, dev, inputs, monkeypatch=None):
    """ops.LSTMFn forward and backward at the default switches -> ({h, dx, dW_ih, dW_hh, db_ih, db_hh}, {entry point: calls})"""
    from awm_amd import ops
    x, wi, wh, bi, bh, gg = inputs
    leaves = [t.to(dev).requires_grad_() for t in (x, wi, wh, bi, bh)]
    counts = _spy(monkeypatch, awm.lib, Y.LAUNCHES) if monkeypatch is not None else {}
    h = ops.LSTMFn.apply(*leaves)
    h.backward(gg.to(dev))
    ops.join_side_stream()
    torch.cuda.synchronize()
    out = dict(h=h.detach())
    out.update({n: t.grad for n, t in zip(Y.GRAD_NAMES, leaves)})
    return out, counts


def _held(got, kind, B, T, names, what):
    r64, r32 = Y.lstm_ref(kind, B, T)
    for n in names:
        assert bool(torch.isfinite(got[n]).all()), f"{what} {n}: not finite"
        Y.held(got[n], r64[n], r32[n], Y.floor_of(n), f"{what} {n}")


@pytest.mark.parametrize("B", Y.ROUTE_B)
@pytest.mark.parametrize("T", Y.ROUTE_T)
def test_route_edges(awm, dev, monkeypatch, B, T):
    got, counts = _lstm_fn(awm, dev, Y.lstm_inputs("route", B, T), monkeypatch)
    assert counts == Y.expected_launches(T), f"T = {T} took {counts}, the table expects {Y.expected_launches(T)}"
    _held(got, "route", B, T, ("h",) + Y.GRAD_NAMES, f"LSTMFn ({B}, {T})")


@pytest.mark.parametrize("T", Y.SAVED_T)
def test_saved_gates_and_cell_states(awm, dev, T):
    """what every backward reads: the saved activations and cell states of wm_lstm_fwd_fused (both builds) and wm_lstm_xproj + wm_lstm_fwd"""
    from awm_amd import ops
    B = 2
    x, wi, wh, bi, bh, _ = (t.to(dev) for t in Y.lstm_inputs("route", B, T))
    for entry in ("fused, wave-specialised", "fused, one set of waves", "xproj + fwd"):
        h, gates, cst = nan_like(B, 64, T, dev=dev), nan_like(B, T, 256, dev=dev), nan_like(B, T, 64, dev=dev)
        if entry == "xproj + fwd":
            xp = nan_like(B, T, 256, dev=dev)
            awm.lib.wm_lstm_xproj(p(x), p(wi), p(bi), p(bh), p(xp), B, T, st())
            awm.lib.wm_lstm_fwd(p(xp), p(wh), p(h), p(gates), p(cst), B, T, st())
        else:
            with ops.switches(lstm_fwd_ws=entry.endswith("specialised")):
                awm.lib.wm_lstm_fwd_fused(p(x), p(wi), p(bi), p(bh), p(wh), p(h), p(gates), p(cst), B, T, st())
        torch.cuda.synchronize()
        _held(dict(h=h, gates=gates, cst=cst), "route", B, T, ("h", "gates", "cst"), f"{entry} ({B}, {T})")


# ------------------------------------------------------------------------------------------------------------ 3. saturated gates
@pytest.mark.parametrize("B,T", Y.SATURATED)
def test_saturated_gates(awm, dev, B, T):
    got, _ = _lstm_fn(awm, dev, Y.lstm_inputs("saturated", B, T))
    _held(got, "saturated", B, T, ("h",) + Y.GRAD_NAMES, f"saturated LSTMFn ({B}, {T})")


# ------------------------------------------------------------------------------------------------------------ 4. degenerate inputs
def test_all_zero_inputs_and_weights(awm, dev):
    """sigm(0) = 0.5 and tanh_s(0) = 0 exactly: h = +0.0 bit for bit and dx = dW_ih = dW_hh = 0; the biases' gradient is no zero (the g
    gate's da = dc / 2) and is held to float64"""
    B, T = Y.ALL_ZERO
    got, _ = _lstm_fn(awm, dev, Y.lstm_inputs("all_zero", B, T))
    assert not bits(got["h"]).any(), "h must be +0.0 everywhere"
    for n in ("dx", "dW_ih", "dW_hh"):
        assert not (got[n] != 0).any(), f"{n} must be zero"
    _held(got, "all_zero", B, T, ("db_ih", "db_hh"), f"all-zero LSTMFn ({B}, {T})")


@pytest.mark.parametrize("B,T", [(2, 36), (1, 64)])
def test_zero_upstream_gradient(awm, dev, B, T):
    x, wi, wh, bi, bh, gg = Y.lstm_inputs("route", B, T)
    got, _ = _lstm_fn(awm, dev, (x, wi, wh, bi, bh, torch.zeros_like(gg)))
    for n in Y.GRAD_NAMES:
        assert bool(torch.isfinite(got[n]).all()) and not (got[n] != 0).any(), f"{n}: a zero dh must give a zero gradient"


def test_zero_input_with_biases(awm, dev):
    B, T = Y.ZERO_X
    got, _ = _lstm_fn(awm, dev, Y.lstm_inputs("zero_x", B, T))
    assert not (got["dW_ih"] != 0).any(), "dW_ih = da^T x must be zero for x = 0"
    _held(got, "zero_x", B, T, ("h", "dx", "dW_hh", "db_ih", "db_hh"), f"zero-x LSTMFn ({B}, {T})")
