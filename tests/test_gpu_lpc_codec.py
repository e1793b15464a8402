"""wm_lpc_codec / ops.lpc_codec / ops.LpcCodecFn / attacks.LpcCodec on the GPU against the float64 yardstick of tests/lpc_yardstick.py
(numpy from the definition in include/wm_hip.h; nothing from the package).  The checks are staged so that one stage's rounding never
excuses the next; no tolerance is tuned to the kernel.

  A  coefficients.  signal_plain: per coefficient against float64 within the first-order perturbation bound of the normal equations under
     a float32 autocorrelation in any summation order (Y.coeff_bound; 2e-4 .. 5e-3 here, of which the yardstick's float32 mode uses under
     1 % in four orders -- tests/test_lpc_codec_cpu.py).  Loose for rounding, tight for a wrong window origin, lag table or expansion
     exponent.  signal_speech: condition numbers up to 7e4 make that bound say nothing, so the float64 prediction gain with the kernel's
     coefficients must sit within 0.05 dB of the float64 coefficients' (the error is second order in the coefficients).
  B  codes.  The yardstick teacher-forced with the KERNEL's coefficients in both modes: r = e / step, h = 8 max|r32 - r64|; outside the
     near-tie set (r64 within h of a half-integer, at most 1 % of the samples) the kernel's codes equal the float64 codes, inside they
     differ by at most 1.
  C  output.  The float64 yardstick with the kernel's coefficients AND codes; tolerance 4 * E32y + spacing(max|x|), E32y the float32
     mode against float64 on the same coefficients and codes, computed at run time; the 4 as in tests/test_gpu_mdct_codec.py.
  D  adjoint.  The same E32 rule against Y.adjoint, and <A u, v> = <u, A^T v> within the room formula of the MDCT test.
Every reference is computed once per case (lru_cache) and never written to."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import wm_oracle as O

import lpc_yardstick as Y
from gpu_support import awm, dev  # noqa: F401
from gpu_support import p as ptr
from gpu_support import reference_models, st

pytestmark = pytest.mark.gpu

SIGNALS = {"plain": Y.signal_plain, "speech": Y.signal_speech}
ADJ_CASES = [(3, 160, 10, 4 * 160 + 3), (3, 320, 16, 4 * 320 + 3), (1, 320, 16, 16000), (2, 640, 16, 3 * 640 + 5)]


def spacing32(v):
    return float(np.spacing(np.float32(np.abs(v).max())))


def launch(dev, x, L, p, snr=None, quantise=True, coeffs=None, coeffs_out=False, codes_out=False, mask=None, adjoint=False):
    """numpy in, numpy out: y, or the tuple ops.lpc_codec returns"""
    from awm_amd import ops
    xt = torch.from_numpy(np.array(x, dtype=np.float32)).to(dev)                  # a copy: the references are read-only
    s = None if snr is None else torch.from_numpy(np.asarray(snr, dtype=np.float32)).to(dev)
    c = None if coeffs is None else torch.from_numpy(np.ascontiguousarray(coeffs, dtype=np.float32)).to(dev)
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, dtype=np.int16)).to(dev)
    out = ops.lpc_codec(xt, s, frame=L, order=p, quantise=quantise, coeffs=c, coeffs_out=coeffs_out, codes_out=codes_out, mask_in=m,
                        adjoint=adjoint)
    return tuple(t.cpu().numpy() for t in out) if isinstance(out, tuple) else out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def bound_ref(rows, L, p, n):
    return Y.coeff_bound(Y.signal_plain(rows, n), L, p)


def check_codes_and_output(dev, x, L, p, snr, what):
    """stages B and C on one launch; returns (y, coeffs, codes)"""
    y, c, q = launch(dev, x, L, p, snr, coeffs_out=True, codes_out=True)
    assert q.dtype == np.int16 and q.shape == x.shape and c.shape == (x.shape[0], Y.frames(x.shape[1], L), p) and np.isfinite(c).all()
    tie, share, codes64, h = Y.near_tie(x, c, L, snr)
    got = q.astype(np.int64)
    differ = got != codes64
    print(f"{what}: near-tie share {share:.2e} (h {h:.2e}), codes differ in {int(differ.sum())} of {differ.size}")
    assert share <= 0.01
    assert not (differ & ~tie).any(), f"{what}: {int((differ & ~tie).sum())} codes differ from float64 outside the near-tie set"
    assert np.abs(got - codes64).max() <= 1
    e, y64 = Y.e32_output(x, c, L, snr, got)
    tol = 4 * e + spacing32(x)
    err = np.abs(y.astype(np.float64) - y64).max()
    print(f"{what}: output max err {err:.3e}, tolerance {tol:.3e} (E32y {e:.3e})")
    assert err <= tol
    return y, c, q


# ------------------------------------------------------------------------------------------ A. coefficients
@pytest.mark.parametrize("rows,L,p,n", Y.GPU_CASES)
def test_coefficients_inside_the_perturbation_bound(dev, rows, L, p, n):
    c64, bound = bound_ref(rows, L, p, n)
    _, c = launch(dev, Y.signal_plain(rows, n), L, p, Y.snr_rows(rows), coeffs_out=True)
    err = np.abs(c.astype(np.float64) - c64)
    print(f"rows {rows} L {L} p {p} n {n}: max err {err.max():.3e}, max err / bound {(err / np.maximum(bound, 1e-300)).max():.4f}, "
          f"bound {bound.min():.1e} .. {bound.max():.1e}")
    assert c.shape == c64.shape and (err <= bound).all()


@pytest.mark.parametrize("rows,L,p,n", Y.LONG_CASES)
def test_prediction_gain_of_the_kernels_coefficients(dev, rows, L, p, n):
    x = Y.signal_speech(rows, n)
    _, c = launch(dev, x, L, p, Y.snr_rows(rows), coeffs_out=True)
    g64, g = Y.prediction_gain_db(x, Y.analyse(x, L, p)["coeffs"], L), Y.prediction_gain_db(x, c, L)
    print(f"rows {rows} L {L} p {p} n {n}: gain {g64.round(3)} dB, the kernel's off by {np.abs(g - g64).max():.2e} dB")
    assert np.abs(g - g64).max() <= 0.05


# ------------------------------------------------------------------------------------------ B, C. codes and output
@pytest.mark.parametrize("rows,L,p,n", Y.GPU_CASES)
def test_codes_and_output_plain(dev, rows, L, p, n):
    x, snr = Y.signal_plain(rows, n), Y.snr_rows(rows)
    y, c, q = check_codes_and_output(dev, x, L, p, snr, f"plain rows {rows} L {L} p {p} n {n}")
    # the quantiser off, at these coefficients: y = x within the same rule
    e, _ = Y.e32_output(x, c, L, None, None, quantise=False)
    back = launch(dev, x, L, p, quantise=False, coeffs=c)
    err = np.abs(back.astype(np.float64) - x).max()
    print(f"quantiser off: max |y - x| {err:.3e}, tolerance {4 * e + spacing32(x):.3e}")
    assert err <= 4 * e + spacing32(x)
    # coeffs_in equal to this launch's coeffs_out: the same bits
    again = launch(dev, x, L, p, snr, coeffs=c, coeffs_out=True, codes_out=True)
    assert np.array_equal(again[0], y) and np.array_equal(again[1], c) and np.array_equal(again[2], q)


@pytest.mark.parametrize("rows,L,p,n", Y.LONG_CASES)
def test_codes_and_output_speech(dev, rows, L, p, n):
    x, snr = Y.signal_speech(rows, n), Y.snr_rows(rows)
    y, c, q = check_codes_and_output(dev, x, L, p, snr, f"speech rows {rows} L {L} p {p} n {n}")
    assert 0.02 < (q == 0).mean() < 0.98, "the dead zone is neither empty nor everything"
    e, _ = Y.e32_output(x, c, L, None, None, quantise=False)
    back = launch(dev, x, L, p, quantise=False, coeffs=c)
    assert np.abs(back.astype(np.float64) - x).max() <= 4 * e + spacing32(x)
    assert np.array_equal(launch(dev, x, L, p, snr, coeffs=c), y)


# ------------------------------------------------------------------------------------------ D. adjoint
@pytest.mark.parametrize("rows,L,p,n", ADJ_CASES)
def test_adjoint_and_the_tape(dev, rows, L, p, n):
    from awm_amd import ops
    x, snr = Y.signal_speech(rows, n), Y.snr_rows(rows)
    g = np.random.default_rng(L + n).standard_normal((rows, n)).astype(np.float32)
    y, c, q = launch(dev, x, L, p, snr, coeffs_out=True, codes_out=True)
    assert 0.02 < (q == 0).mean() < 0.98 and n > L, "a dead zone, and a frame boundary inside the support"
    results = {}
    for name, mask in (("dead_zone", q), ("all_ones", np.ones_like(q))):
        e, ref = Y.e32_adjoint(g, c, L, mask)
        tol = 4 * e + spacing32(g)
        direct = launch(dev, g, L, p, quantise=False, coeffs=c, mask=mask, adjoint=True)
        err = np.abs(direct.astype(np.float64) - ref).max()
        print(f"L {L} p {p} n {n} {name}: max err of A^T g {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol
        # <A x, g> = <x, A^T g>: each side is off by at most its per-sample tolerance times the other vector's l1 norm
        ev, _ = Y.e32_output(x, c, L, None, None, mask=mask, quantise=False)
        Ax = launch(dev, x, L, p, quantise=False, coeffs=c, mask=mask)
        lhs, rhs = float((Ax.astype(np.float64) * g).sum()), float((x.astype(np.float64) * direct).sum())
        room = tol * float(np.abs(x).sum()) + (4 * ev + spacing32(x)) * float(np.abs(g).sum())
        print(f"L {L} p {p} n {n} {name}: <Ax, g> - <x, A^T g> = {lhs - rhs:.3e}, room {room:.3e}")
        assert abs(lhs - rhs) <= room
        results[name] = (direct, tol)
    assert np.abs(results["all_ones"][0].astype(np.float64) - g).max() <= results["all_ones"][1], "without a dead zone dx = g"
    assert np.array_equal(launch(dev, g, L, p, quantise=False, coeffs=c, adjoint=True), results["all_ones"][0]), "no mask is the all-ones mask"
    assert not np.array_equal(results["dead_zone"][0], results["all_ones"][0]), "the dead zone changes the gradient"
    # the tape
    xt, stt, gt = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(snr).to(dev), torch.from_numpy(g).to(dev)
    xr = xt.clone().requires_grad_()
    out = ops.LpcCodecFn.apply(xr, stt, L, p, 16000, Y.FLOOR_STEP, "dead_zone")
    assert np.array_equal(out.detach().cpu().numpy(), y)
    out.backward(gt)
    assert np.array_equal(xr.grad.cpu().numpy(), results["dead_zone"][0]), "dead_zone: autograd does not return the launch's result"
    xr = xt.clone().requires_grad_()
    out = ops.LpcCodecFn.apply(xr, stt, L, p, 16000, Y.FLOOR_STEP, "straight_through")
    assert len(out.grad_fn.saved_tensors) == 0 and np.array_equal(out.detach().cpu().numpy(), y)
    out.backward(gt)
    assert torch.equal(xr.grad, gt), "straight_through: the gradient is dy itself"
    assert not ops.LpcCodecFn.apply(xt, stt, L, p, 16000, Y.FLOOR_STEP, "dead_zone").requires_grad


# ------------------------------------------------------------------------------------------ E. degenerate rows
def test_degenerate_rows(dev):
    """an all-zero row and a row under the floor step give y == 0 and codes 0; a pure tone and a constant row, whose reflection
    coefficients sit near -1 and +1, stay finite and pass stages B and C"""
    L, p, n = 320, 16, 4 * 320 + 3
    x, snr = Y.degenerate(n), Y.snr_rows(4)
    y, c, q = check_codes_and_output(dev, x, L, p, snr, "degenerate rows")
    assert not c[0].any() and not q[:2].any() and not y[:2].any()
    assert np.isfinite(y).all() and np.isfinite(c).all() and np.abs(y[2]).max() > 0.1 and np.abs(y[3]).max() > 0.4
    assert np.abs(c[2:]).max() > 1.0, "the tone's and the constant's predictors are not trivial"


# ------------------------------------------------------------------------------------------ F. plumbing
@pytest.mark.parametrize("L,p,n", [(160, 10, 16000), (320, 16, 16000), (320, 16, 321), (640, 16, 3 * 640 + 5)])
def test_two_calls_and_row_cuts_are_bit_identical(dev, L, p, n):
    from awm_amd import ops
    x, snr = Y.signal_speech(3, n), Y.snr_rows(3)
    y, c, q = launch(dev, x, L, p, snr, coeffs_out=True, codes_out=True)
    y2, c2, q2 = launch(dev, x, L, p, snr, coeffs_out=True, codes_out=True)
    assert np.array_equal(y, y2) and np.array_equal(c, c2) and np.array_equal(q, q2), "two calls"
    assert np.array_equal(launch(dev, x, L, p, snr), y), "with and without the coefficients and codes"
    for lo, hi in ((0, 1), (1, 3)):
        yp, cp, qp = launch(dev, x[lo:hi], L, p, snr[lo:hi], coeffs_out=True, codes_out=True)
        assert np.array_equal(yp, y[lo:hi]) and np.array_equal(cp, c[lo:hi]) and np.array_equal(qp, q[lo:hi]), f"rows {lo}:{hi} alone"
    # a row that does not start on a 16-byte boundary: the same bits
    pad = torch.zeros(3 * n + 1, device=dev)
    pad[1:] = torch.from_numpy(np.array(x)).to(dev).reshape(-1)
    yo = ops.lpc_codec(pad[1:].view(3, n), torch.from_numpy(snr).to(dev), frame=L, order=p)
    assert np.array_equal(yo.cpu().numpy(), y)


def test_module_on_the_gpu_draws_and_numbers_rows(awm, dev):
    x = torch.from_numpy(np.array(Y.signal_speech(3, 1027))).view(3, 1, 1027)
    att = awm.LpcCodec(snr_db=(10, 30), seed=5)
    y = att(x.to(dev))
    assert y.shape == x.shape and y.is_cuda and att.draw == 1
    want = launch(dev, x.view(3, -1).numpy(), 320, 16, att.last_snr_db.numpy())
    assert np.array_equal(y.cpu().numpy().reshape(3, -1), want)
    pieces = torch.cat([att.reset()(x[r:r + 1].to(dev), row0=r) for r in range(3)])
    assert torch.equal(pieces, y), "a batch of 3 equals its rows launched one by one with row0"
    cpu = att.reset()(x)
    assert np.array_equal(att.last_snr_db.numpy(), awm.attacks.row_lpc_snr_db(5, 0, np.arange(3), (10, 30)))
    snr_of = lambda z: 10 * torch.log10(x.pow(2).sum(-1) / (z - x).pow(2).sum(-1)).view(-1)
    print(f"SNR per row: GPU {snr_of(y.cpu()).tolist()}, CPU path {snr_of(cpu).tolist()}, drawn {att.last_snr_db.tolist()}")
    assert bool(((snr_of(cpu) - snr_of(y.cpu())).abs() < 1.0).all()), "the CPU path is the same codec: within 1 dB per row"


def test_refusals_on_the_device(awm, dev):
    """bad L and p, null pointers and in-place use: hipErrorInvalidValue, and nothing is launched (the output keeps its bits)"""
    from awm_amd import ops
    n = 1000
    x = torch.from_numpy(np.array(Y.signal_plain(2, n))).to(dev)
    y = torch.full_like(x, 7.0)
    snr = torch.tensor([20.0, 20.0], device=dev)
    lag, ex = (t.to(dev) for t in ops.lpc_tables(16))
    good = (ptr(x), ptr(y), None, None, None, None, ptr(snr), ptr(lag), ptr(ex), 2, n, 320, 16, Y.FLOOR_STEP, 1, 0, st())
    for i, v in ((11, 256), (11, 100), (12, 1), (12, 17), (0, None), (1, None), (6, None), (7, None), (8, None), (1, ptr(x)), (1, ptr(x) + 4)):
        args = list(good)
        args[i] = v
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm.lib.wm_lpc_codec(*args)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    awm.lib.wm_lpc_codec(*good)
    torch.cuda.synchronize()
    assert bool((y != 7.0).any())
    for kw in (dict(frame=256), dict(order=1), dict(order=17), dict(adjoint=True), dict(quantise=False, codes_out=True),
               dict(coeffs=torch.zeros(2, 4, 15, device=dev)), dict(mask_in=torch.ones(2, n, device=dev)), dict(floor_step=0.0)):
        with pytest.raises(ValueError):
            ops.lpc_codec(x, snr, **kw)


# ------------------------------------------------------------------------------------------ the step and the evaluation loop
@pytest.mark.parametrize("grad", ["straight_through", "dead_zone"])
def test_train_step_through_the_codec(awm, dev, grad):
    """T = 2048: the shortest clip the step's loudness loss accepts"""
    G, D = reference_models(awm, dev)
    s = O.synthetic_clips(2, seed=41, T=2048).to(dev)
    msg = torch.tensor([3, 60001], device=dev)
    codec = awm.LpcCodec(20, grad=grad)
    G.train(); D.train()
    opt = torch.optim.Adam(list(G.parameters()) + list(D.parameters()), lr=1e-3)
    out = awm.train_step(G, D, opt, s, msg, codec=codec)
    assert codec.draw == 1 and tuple(codec.last_snr_db.shape) == (2,)
    for k, v in out.items():
        if torch.is_tensor(v) and v.dim() == 0:
            assert bool(torch.isfinite(v)), f"loss {k}"
    assert bool(torch.isfinite(out["total"]))
    assert not torch.equal(out["s_w"], s + out["delta"].detach())
    for k, prm in G.named_parameters():
        assert bool(torch.isfinite(prm.grad).all()) and bool((prm.grad != 0).any()), f"Generator {k}"


def test_evaluate_robustness_with_the_codec(awm, dev):
    ck = np.load(os.path.join(os.path.dirname(__file__), "golden", "detector_best_unprefixed.npz"))
    D = awm.Detector(16)
    D.load_state_dict({k: torch.from_numpy(ck[k]) for k in ck.files})
    torch.manual_seed(17)
    G = awm.Generator(16)
    G.to(dev); D.to(dev)
    batches = [O.synthetic_clips(2, seed=51, T=2048), O.synthetic_clips(2, seed=52, T=2048)]
    messages = [torch.tensor([3, 60001]), torch.tensor([77, 12345])]
    atk = {"lpc": awm.LpcCodec(snr_db=(10, 30), seed=9), "chain": torch.nn.Sequential(awm.LpcCodec(20), awm.PcmCodec())}
    res = awm.evaluate_robustness(G, D, batches, atk, device=dev, messages=messages)
    print(res)
    assert list(res) == ["none", "lpc", "chain"]
    keys = ["bit_accuracy", "clean_prob", "delta_rms", "watermarked_prob"]
    for name in ("lpc", "chain"):
        assert sorted(res[name]) == keys and all(np.isfinite(res[name][k]) for k in keys)
    assert atk["lpc"].draw == 2, "one call per batch, on the concatenation of s + delta and s"
