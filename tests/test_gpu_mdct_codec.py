"""wm_mdct_codec / ops.mdct_codec / ops.MdctCodecFn / attacks.TransformCodec on the GPU against the float64 yardstick of
tests/mdct_yardstick.py (numpy from the definition in include/wm_hip.h; nothing from the package).

Tolerances (none tuned to the kernel):
  E32   the largest error of the yardstick's own float32 mode against float64 on the SAME input and operator, computed at run time.
  tol   4 * E32 + spacing(max|input|): the factor 4 covers the different summation order of a GPU transform (the fold to DCT-IV adds M terms
        where the dense text adds 2M).  Identity, backward and symmetry use it as it stands; the quantised output uses it scaled by
        max|Xq| / max|X|, against the yardstick run with the KERNEL's codes.
  codes outside the near-tie set (r64 within h = 8 max|r32 - r64| of a half-integer; its share is capped at 1 % for every input here by
        tests/test_mdct_codec_cpu.py) the kernel's codes equal the float64 codes exactly; inside it they differ by at most 1.
Every reference is computed once per case (lru_cache) and never written to."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import wm_oracle as O

import mdct_yardstick as Y
from gpu_support import awm, dev  # noqa: F401
from gpu_support import reference_models

pytestmark = pytest.mark.gpu


def spacing32(v):
    return float(np.spacing(np.float32(np.abs(v).max())))


@functools.lru_cache(maxsize=None)
def identity_ref(rows, M, n):
    x = Y.signal(rows, n)
    e, _ = Y.e32(x, M, Y.BAND, M)
    return x, 4 * e + spacing32(x)


@functools.lru_cache(maxsize=None)
def tie_ref(rows, M, n):
    x = Y.signal(rows, n)
    tie, share, a, _, h = Y.near_tie(x, M, Y.BAND, Y.KCUT[M], Y.snr_rows(rows), Y.default_floor_step(M))
    return tie, share, a["codes"]


def launch(awm, dev, x, M, snr=None, kcut=None, quantise=True, codes_out=False, mask=None, floor_step=None):
    from awm_amd import ops
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    st = None if snr is None else torch.from_numpy(np.asarray(snr, dtype=np.float32)).to(dev)
    mt = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, dtype=np.int16)).to(dev)
    out = ops.mdct_codec(xt, st, hop=M, band=Y.BAND, kcut=M if kcut is None else kcut, floor_step=floor_step, quantise=quantise,
                         codes_out=codes_out, mask_in=mt)
    if codes_out:
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy()


def check_codes_and_output(awm, dev, x, M, snr, tie, share, codes64, tol, what):
    y, codes = launch(awm, dev, x, M, snr, kcut=Y.KCUT[M], codes_out=True)
    assert codes.dtype == np.int16 and codes.shape == codes64.shape
    got = codes.astype(np.int64)
    differ = got != codes64
    print(f"{what}: near-tie share {share:.2e}, codes differ in {int(differ.sum())} of {differ.size}")
    assert share <= 0.01
    assert not (differ & ~tie).any(), f"{what}: {int((differ & ~tie).sum())} codes differ from float64 outside the near-tie set"
    assert np.abs(got - codes64).max() <= 1
    ref = Y.codec(x, M, Y.BAND, Y.KCUT[M], snr, Y.default_floor_step(M), codes=got)
    xmax = np.abs(ref["X"]).max()
    scale = np.abs(ref["Xq"]).max() / xmax if xmax > 0 else 1.0
    err = np.abs(y.astype(np.float64) - ref["y"]).max()
    print(f"{what}: output max err {err:.3e}, tolerance {tol * scale:.3e} (scale {scale:.3f})")
    assert err <= tol * scale
    return y, codes


# ------------------------------------------------------------------------------------------ 1. identity, codes, output
@pytest.mark.parametrize("rows,M,n", Y.GPU_CASES)
def test_identity_without_the_quantiser(awm, dev, rows, M, n):
    x, tol = identity_ref(rows, M, n)
    y = launch(awm, dev, x, M, quantise=False)
    err = np.abs(y.astype(np.float64) - x).max()
    print(f"rows {rows} M {M} n {n}: max |y - x| {err:.3e}, tolerance {tol:.3e}")
    assert y.shape == x.shape and err <= tol


@pytest.mark.parametrize("rows,M,n", Y.GPU_CASES)
def test_codes_and_output_against_float64(awm, dev, rows, M, n):
    x, tol = identity_ref(rows, M, n)
    tie, share, codes64 = tie_ref(rows, M, n)
    check_codes_and_output(awm, dev, x, M, Y.snr_rows(rows), tie, share, codes64, tol, f"rows {rows} M {M} n {n}")


def test_degenerate_rows(awm, dev):
    """an all-zero row and a row under the floor step give y == 0 and codes 0; a pure tone matches the yardstick"""
    M, n = 256, 4 * 256 + 3
    x = Y.degenerate(n)
    snr = Y.snr_rows(3)
    tie, share, a, _, _ = Y.near_tie(x, M, Y.BAND, Y.KCUT[M], snr, Y.default_floor_step(M))
    assert (a["codes"][:2] == 0).all() and (a["step"][2] == Y.default_floor_step(M)).mean() > 0.5, "the yardstick agrees on what is degenerate"
    e, _ = Y.e32(x, M, Y.BAND, M)
    y, codes = check_codes_and_output(awm, dev, x, M, snr, tie, share, a["codes"], 4 * e + spacing32(x), "degenerate rows")
    assert not y[:2].any() and not codes[:2].any()
    assert np.abs(y[2]).max() > 0.1


# ------------------------------------------------------------------------------------------ 2. backward
@pytest.mark.parametrize("rows,M,n", [(3, 128, 4 * 128 + 3), (3, 256, 4 * 256 + 3), (1, 256, 16000), (2, 512, 4 * 512 + 3)])
def test_backward_both_modes_and_symmetry(awm, dev, rows, M, n):
    from awm_amd import ops
    x = Y.signal(rows, n)
    rng = np.random.default_rng(M + n)
    dy = rng.standard_normal((rows, n)).astype(np.float32)
    snr, kcut, fs = Y.snr_rows(rows), Y.KCUT[M], Y.default_floor_step(M)
    xt, st, gt = torch.from_numpy(x).to(dev), torch.from_numpy(snr).to(dev), torch.from_numpy(dy).to(dev)
    _, codes = launch(awm, dev, x, M, snr, kcut=kcut, codes_out=True)
    assert 0.02 < (codes[:, :, :kcut] == 0).mean() < 0.98, "the dead zone is neither empty nor everything"
    for grad, mask in (("straight_through", None), ("dead_zone", codes)):
        e, ref = Y.e32(dy, M, Y.BAND, kcut, mask=mask)
        tol = 4 * e + spacing32(dy)
        direct = launch(awm, dev, dy, M, kcut=kcut, quantise=False, mask=mask)
        err = np.abs(direct.astype(np.float64) - ref["y"]).max()
        print(f"M {M} n {n} {grad}: max err of A dy {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol
        # the tape returns the same launch
        xr = xt.clone().requires_grad_()
        y = ops.MdctCodecFn.apply(xr, st, M, Y.BAND, kcut, fs, grad)
        y.backward(gt)
        assert np.array_equal(xr.grad.cpu().numpy(), direct), f"{grad}: autograd does not return the launch's result"
        # <A u, v> = <u, A v>, u = dy, v = x: each side is off by at most its per-sample tolerance times the other vector's l1 norm
        ev, _ = Y.e32(x, M, Y.BAND, kcut, mask=mask)
        Av = launch(awm, dev, x, M, kcut=kcut, quantise=False, mask=mask)
        lhs, rhs = float((direct.astype(np.float64) * x).sum()), float((dy.astype(np.float64) * Av).sum())
        room = tol * float(np.abs(x).sum()) + (4 * ev + spacing32(x)) * float(np.abs(dy).sum())
        print(f"M {M} n {n} {grad}: <Au, v> - <u, Av> = {lhs - rhs:.3e}, room {room:.3e}")
        assert abs(lhs - rhs) <= room
    # the dead zone changes the gradient
    assert not np.array_equal(launch(awm, dev, dy, M, kcut=kcut, quantise=False, mask=codes), launch(awm, dev, dy, M, kcut=kcut, quantise=False))
    # without a gradient to compute nothing is saved
    y = ops.MdctCodecFn.apply(xt, st, M, Y.BAND, kcut, fs, "dead_zone")
    assert not y.requires_grad


# ------------------------------------------------------------------------------------------ 3. determinism
@pytest.mark.parametrize("M,n", [(128, 16000), (256, 16000), (256, 257), (512, 16000)])
def test_two_calls_and_row_cuts_are_bit_identical(awm, dev, M, n):
    x, snr = Y.signal(3, n), Y.snr_rows(3)
    y, c = launch(awm, dev, x, M, snr, kcut=Y.KCUT[M], codes_out=True)
    y2, c2 = launch(awm, dev, x, M, snr, kcut=Y.KCUT[M], codes_out=True)
    assert np.array_equal(y, y2) and np.array_equal(c, c2), "two calls"
    assert np.array_equal(launch(awm, dev, x, M, snr, kcut=Y.KCUT[M]), y), "with and without the codes"
    for lo, hi in ((0, 1), (1, 3)):
        yp, cp = launch(awm, dev, x[lo:hi], M, snr[lo:hi], kcut=Y.KCUT[M], codes_out=True)
        assert np.array_equal(yp, y[lo:hi]) and np.array_equal(cp, c[lo:hi]), f"rows {lo}:{hi} alone"
    # a row that does not start on a 16-byte boundary: the same bits
    pad = torch.zeros(3 * n + 1, device=dev)
    pad[1:] = torch.from_numpy(x).to(dev).reshape(-1)
    from awm_amd import ops
    yo = ops.mdct_codec(pad[1:].view(3, n), torch.from_numpy(snr).to(dev), hop=M, band=Y.BAND, kcut=Y.KCUT[M])
    assert np.array_equal(yo.cpu().numpy(), y)


def test_module_on_the_gpu_matches_its_cpu_path_in_shape_and_draw(awm, dev):
    x = torch.from_numpy(Y.signal(4, 1027)).view(4, 1, 1027)
    att = awm.TransformCodec(snr_db=(10, 30), bandwidth_hz=7000, seed=5)
    y = att(x.to(dev))
    assert y.shape == x.shape and y.is_cuda and att.draw == 1
    snr = att.last_snr_db.numpy()
    want = launch(awm, dev, x.view(4, -1).numpy(), 256, snr, kcut=224)
    assert np.array_equal(y.cpu().numpy().reshape(4, -1), want)
    from awm_amd import ops
    by_hz = ops.mdct_codec(x.to(dev), att.last_snr_db.to(dev), bandwidth_hz=7100)            # 227 coefficients -> 224
    assert torch.equal(by_hz, y)
    with pytest.raises(ValueError):
        ops.mdct_codec(x.to(dev), att.last_snr_db.to(dev), kcut=224, bandwidth_hz=7000)
    pieces = torch.cat([att.reset()(x[:1].to(dev)), att.reset()(x[1:].to(dev), row0=1)])
    assert torch.equal(pieces, y), "a batch cut into pieces, numbered by row0, is the whole batch"
    k = att.reset().estimate_kbps(x.to(dev))
    assert att.draw == 0 and 0 < k < 16 * 16.0, "fewer bits than 16-bit PCM at 16 kHz"
    assert abs(k - att.estimate_kbps(x)) < 0.05 * k, "the CPU path's codes give nearly the same estimate"


# ------------------------------------------------------------------------------------------ 4. the step and the evaluation loop
@pytest.mark.parametrize("grad", ["straight_through", "dead_zone"])
def test_train_step_through_the_codec(awm, dev, grad):
    """T = 2048: the shortest clip the step's loudness loss accepts"""
    G, D = reference_models(awm, dev)
    s = O.synthetic_clips(2, seed=41, T=2048).to(dev)
    msg = torch.tensor([3, 60001], device=dev)
    codec = torch.nn.Sequential(awm.Distortion(seed=3), awm.TransformCodec(seed=3, grad=grad), awm.PcmCodec(grad="straight_through"))
    G.train(); D.train()
    opt = torch.optim.Adam(list(G.parameters()) + list(D.parameters()), lr=1e-3)
    out = awm.train_step(G, D, opt, s, msg, codec=codec)
    assert codec[1].draw == 1 and tuple(codec[1].last_snr_db.shape) == (2,)
    for k, v in out.items():
        if torch.is_tensor(v) and v.dim() == 0:
            assert bool(torch.isfinite(v)), f"loss {k}"
    assert bool(torch.isfinite(out["total"]))
    assert not torch.equal(out["s_w"], s + out["delta"].detach())
    for k, p in G.named_parameters():
        assert bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), f"Generator {k}"


def test_evaluate_robustness_with_the_codec(awm, dev):
    ck = np.load(os.path.join(os.path.dirname(__file__), "golden", "detector_best_unprefixed.npz"))
    D = awm.Detector(16)
    D.load_state_dict({k: torch.from_numpy(ck[k]) for k in ck.files})
    torch.manual_seed(17)
    G = awm.Generator(16)
    G.to(dev); D.to(dev)
    batches = [O.synthetic_clips(2, seed=51, T=2048), O.synthetic_clips(2, seed=52, T=2048)]
    messages = [torch.tensor([3, 60001]), torch.tensor([77, 12345])]
    atk = {"codec": awm.TransformCodec(snr_db=(10, 30), bandwidth_hz=7000, seed=9),
           "transparent": awm.TransformCodec(snr_db=60, bandwidth_hz=None)}
    res = awm.evaluate_robustness(G, D, batches, atk, device=dev, messages=messages)
    print(res)
    assert list(res) == ["none", "codec", "transparent"]
    keys = ["bit_accuracy", "clean_prob", "delta_rms", "watermarked_prob"]
    assert sorted(res["codec"]) == keys and all(np.isfinite(res["codec"][k]) for k in keys)
    assert atk["codec"].draw == 2, "one call per batch, on the concatenation of s + delta and s"
    for k in keys:
        assert abs(res["transparent"][k] - res["none"][k]) <= 1e-3, (k, res["transparent"][k], res["none"][k])
