"""Channel distortions on the GPU: wm_distort / wm_distort_bwd (csrc/distort.hip) through ops.DistortFn, the modules of attacks.py on top
of them, a train step through a chain of them, and evaluate_robustness.

The yardstick is float64 and uses nothing from the package: the Philox4x32-10 of tests/draw_yardstick.py, u = ((o >> 9) + 0.5) 2^-23 (exact in
both precisions), Box-Muller on exactly those u, the row parameters from their own counter, and y = g x + s z.  Tolerances (derived, not tuned):

  noise   NOISE_TOL = 4 * NOISE_MEASURED, where NOISE_MEASURED is the largest |y - 1 - z64| this file's noise test has shown on an MI355X
          (a row of ones at 0 dB gain and 0 dB SNR, so s = 1 and y = fl(1 + z)); math-library versions differ in the last units, hence the
          factor; never above the sanity ceiling 2e-5 (the float32 numpy evaluation of the same formula is 1.7e-6 off).
  g, snr  relative 1e-5: the argument's rounding, at most an ulp of 40 dB times ln10 / 20, plus a few ulps of exp10 is about 1e-6.
  ms      relative gamma_(n+2) = (n+2) u / (1 - (n+2) u), u = 2^-24: any summation order of n non-negative terms, each rounded once, and
          the division.   s: half of that (the square root) plus 1e-5.
  y       |y - (g x + s z64)| <= 2 spacing(float32(|g x| + |s z|)) + |s| NOISE_TOL, with the kernel's own g and s.
  dx      the same construction: 2 spacing(float32(|g dy| + |k x|)) for the two roundings, and for k = s / (n ms) * sum dy z the relative
          errors of s and ms above plus (gamma_(n+2) sum |dy z| + NOISE_TOL sum |dy|) on the sum."""
import copy
import functools
import math
import os

import numpy as np
import pytest
import torch

import biquad_yardstick
import draw_yardstick as Y
from gpu_support import awm, dev  # noqa: F401
from gpu_support import reference_models
from oracle import wm_oracle as O
from yardstick_common import U, gamma

pytestmark = pytest.mark.gpu

NOISE_MEASURED = 6.679e-7            # on an MI355X, in the (64, 4096) case of test_noise_vs_float64_box_muller
NOISE_TOL = min(4 * NOISE_MEASURED, 2e-5)
LENGTHS = [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 4099, 16000,
           16384, 16385, 40000]      # the last three: one full segment of the row sums, one sample more (the second kernel), three segments
BOUNDS = (-6.0, 6.0, 20.0, 40.0, 1.0)
SEED, DRAW, ROW0 = (7 << 32) + 11, 2, 5


# ------------------------------------------------------------------------------------------ yardstick (nothing from the package)
@functools.lru_cache(maxsize=None)
def noise64(seed, draw, row, n):
    z = Y.normals(seed, draw, row, n, None)
    z.setflags(write=False)
    return z


def params64(seed, draw, rows, bounds):
    """(gain_db, snr_db, noisy) of the rows `rows`: fmaf(hi - lo, u, lo) in float32 (the product of two float32 is exact in float64, so the one
    rounding of the sum is the fmaf's up to a double rounding no tolerance here can see)"""
    o = Y.philox4x32_10((*Y.PARAM, np.asarray(rows, dtype=np.uint64), draw), Y.key_of(seed))
    gain_db, snr_db = Y.affine32(bounds[0:2], Y.unit(o[0])), Y.affine32(bounds[2:4], Y.unit(o[1]))
    return gain_db.astype(np.float64), snr_db.astype(np.float64), Y.unit(o[2]) < np.float64(np.float32(bounds[4]))


def signal(rows, n, seed=0):
    return 0.3 * torch.randn(rows, n, generator=torch.Generator().manual_seed(1000 * seed + n))


def distort(awm, x, bounds=BOUNDS, seed=SEED, draw=DRAW, row0=ROW0, through=True):
    from awm_amd import ops
    return ops.DistortFn.apply(x, bounds, seed, draw, row0, through)


def check_forward(x_cpu, y, stat, bounds, seed, draw, row0, what):
    """stat against float64, then y against g x + s z64 with the kernel's own g and s"""
    x64 = x_cpu.double().numpy()
    rows, n = x64.shape
    st = stat.double().cpu().numpy()
    y = y.double().cpu().numpy()
    gain_db, snr_db, noisy = params64(seed, draw, row0 + np.arange(rows), bounds)
    g64 = 10.0 ** (gain_db / 20.0)
    ms64 = (x64 ** 2).mean(axis=1)
    s64 = np.where(noisy, np.abs(g64) * np.sqrt(ms64) * 10.0 ** (-snr_db / 20.0), 0.0)
    assert np.all(np.abs(st[:, 0] - g64) <= 1e-5 * g64), f"{what}: g {st[:, 0]} vs {g64}"
    assert np.all(np.abs(st[:, 2] - ms64) <= gamma(n + 2) * ms64), f"{what}: ms {st[:, 2]} vs {ms64}"
    assert np.all(np.abs(st[:, 1] - s64) <= (gamma(n + 2) / 2 + 1e-5) * s64), f"{what}: s {st[:, 1]} vs {s64}"
    assert np.all(np.isinf(st[~noisy, 3])) and np.all(np.abs(st[noisy, 3] - snr_db[noisy]) <= 1e-5 * np.abs(snr_db[noisy])), f"{what}: snr"
    z = np.stack([noise64(seed, draw, row0 + r, n) for r in range(rows)])
    gx, sz = st[:, 0:1] * x64, st[:, 1:2] * z
    bound = 2 * np.spacing((np.abs(gx) + np.abs(sz)).astype(np.float32)).astype(np.float64) + np.abs(st[:, 1:2]) * NOISE_TOL
    err = np.abs(y - (gx + sz))
    print(f"{what}: max err {err.max():.3e}, max err/bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"{what}: worst sample {np.unravel_index(int(np.argmax(err - bound)), err.shape)}"


# ------------------------------------------------------------------------------------------ 1. the noise itself
def test_noise_vs_float64_box_muller(awm, dev):
    """a row of ones at 0 dB gain and 0 dB SNR: ms = 1, s = 1, y = fl(1 + z).  Prints the figure NOISE_MEASURED records."""
    worst = 0.0
    for rows, n in ((3, 16000), (1, 40000), (3, 1025), (1, 7), (64, 4096)):
        y, stat = distort(awm, torch.ones(rows, n, device=dev), bounds=(0.0, 0.0, 0.0, 0.0, 1.0))
        assert torch.equal(stat.cpu(), torch.tensor([1.0, 1.0, 1.0, 0.0]).repeat(rows, 1)), stat
        z = np.stack([noise64(SEED, DRAW, ROW0 + r, n) for r in range(rows)])
        err = np.abs(y.double().cpu().numpy() - 1.0 - z)
        worst = max(worst, float(err.max()))
        print(f"noise ({rows}, {n}): max |y - 1 - z64| = {err.max():.3e}, max |z| = {np.abs(z).max():.3f}")
    print(f"noise: largest error {worst:.3e}; asserted at {NOISE_TOL:.3e}")
    assert worst <= NOISE_TOL


# ------------------------------------------------------------------------------------------ 2. forward against the yardstick
@pytest.mark.parametrize("rows", [1, 3])
def test_forward_vs_yardstick(awm, dev, rows):
    for n in LENGTHS:
        x = signal(rows, n)
        y, stat = distort(awm, x.to(dev))
        assert y.shape == (rows, n) and y.dtype == torch.float32 and stat.shape == (rows, 4)
        check_forward(x, y, stat, BOUNDS, SEED, DRAW, ROW0, f"rows={rows} n={n}")


@pytest.mark.parametrize("off", [1, 2, 3])
def test_forward_from_an_unaligned_start(awm, dev, off):
    """x starts `off` floats past a 256-byte boundary; with n = 1025 the rows of y (aligned itself) start at every offset as well"""
    for rows, n in ((3, 1025), (1, 16000), (2, 16386)):
        x = signal(rows, n, seed=off)
        base = torch.zeros(rows * n + 8, device=dev)
        xd = base[off:off + rows * n].view(rows, n)
        xd.copy_(x)
        assert xd.data_ptr() % 16 == 4 * off
        y, stat = distort(awm, xd)
        check_forward(x, y, stat, BOUNDS, SEED, DRAW, ROW0, f"offset {off} rows={rows} n={n}")
        y0, stat0 = distort(awm, x.to(dev))
        assert torch.equal(y, y0) and torch.equal(stat, stat0), "the bits do not depend on where x lies"
        assert bool((base[:off] == 0).all()) and bool((base[off + rows * n:] == 0).all())


def test_identity_and_gain_only(awm, dev):
    for rows, n in ((1, 1), (3, 7), (3, 1025), (2, 16000), (1, 40000)):
        x = signal(rows, n).to(dev)
        x[0, 0] = -0.0
        y, stat = distort(awm, x, bounds=(0.0, 0.0, 10.0, 20.0, 0.0))
        assert torch.equal(y.view(torch.int32), x.view(torch.int32)), f"identity ({rows}, {n})"
        assert bool((stat[:, 0] == 1).all()) and bool((stat[:, 1] == 0).all()) and bool(torch.isinf(stat[:, 3]).all())
        y, stat = distort(awm, x, bounds=(-6.0, 6.0, 10.0, 20.0, 0.0))
        assert torch.equal(y, stat[:, 0:1] * x), f"gain only ({rows}, {n})"
        assert bool((stat[:, 0] != 1).all()) and bool((stat[:, 1] == 0).all())
    # a silent row: s = 0 although the row is a noisy one, y = g x = 0
    y, stat = distort(awm, torch.zeros(2, 100, device=dev))
    assert bool((y == 0).all()) and bool((stat[:, 1] == 0).all()) and bool(torch.isfinite(stat[:, 3]).all())


def test_determinism_rows_and_draws(awm, dev):
    for n in (5, 1025, 16000, 40000):
        x = signal(3, n).to(dev)
        y, stat = distort(awm, x)
        y2, stat2 = distort(awm, x)
        assert torch.equal(y, y2) and torch.equal(stat, stat2), "two launches"
        for r in range(3):
            yr, sr = distort(awm, x[r:r + 1], row0=ROW0 + r)
            assert torch.equal(yr, y[r:r + 1]) and torch.equal(sr, stat[r:r + 1]), f"n={n}: row {r} alone"
        y3, _ = distort(awm, x, draw=DRAW + 1)
        assert bool(((y3 != y).float().mean(dim=1) > 0.99).all()), "the next draw changes every noisy row"
        y4, _ = distort(awm, x, seed=SEED + (1 << 32))
        assert not torch.equal(y4, y), "the seed's high word is part of the key"


def test_rows_are_uncorrelated(awm, dev):
    n = 16000
    y, stat = distort(awm, torch.ones(3, n, device=dev), bounds=(0.0, 0.0, 0.0, 0.0, 1.0))
    z = (y - 1).double().cpu().numpy()
    c = np.corrcoef(z)
    print("correlations", c[0, 1], c[0, 2], c[1, 2])
    assert abs(c[0, 1]) < 5 / math.sqrt(n) and abs(c[0, 2]) < 5 / math.sqrt(n) and abs(c[1, 2]) < 5 / math.sqrt(n)


def test_noise_coin(awm, dev):
    x = signal(64, 50).to(dev)
    bounds = (0.0, 0.0, 10.0, 10.0, 0.5)
    y, stat = distort(awm, x, bounds=bounds, seed=0, draw=0, row0=0)
    _, _, noisy = params64(0, 0, np.arange(64), bounds)
    assert 16 < noisy.sum() < 48
    assert np.array_equal(torch.isfinite(stat[:, 3]).cpu().numpy(), noisy)
    assert np.array_equal((stat[:, 1] != 0).cpu().numpy(), noisy)
    assert np.array_equal(((y != x).any(dim=1)).cpu().numpy(), noisy)
    assert torch.equal(y[torch.from_numpy(~noisy)], x[torch.from_numpy(~noisy)]), "rows without noise at 0 dB are x"


# ------------------------------------------------------------------------------------------ 3. backward
@pytest.mark.parametrize("n", [5, 1025, 16000, 40000])
def test_backward_vs_float64_autograd(awm, dev, n):
    rows = 3
    x = signal(rows, n, seed=2)
    dy = torch.randn(rows, n, generator=torch.Generator().manual_seed(n + 1))
    xd = x.to(dev).requires_grad_()
    y, stat = distort(awm, xd, through=True)
    y.backward(dy.to(dev))
    dx = xd.grad.double().cpu().numpy()
    xt = x.to(dev).requires_grad_()
    yt, stat_t = distort(awm, xt, through=False)
    yt.backward(dy.to(dev))
    assert torch.equal(yt, y) and torch.equal(stat_t, stat)
    assert torch.equal(xt.grad, stat[:, 0:1] * dy.to(dev)), '"detached" is g * dy bit for bit'
    # float64 autograd of the definition, z held constant, with the g and snr_db the kernel drew
    st = stat.double().cpu()
    z = torch.from_numpy(np.stack([noise64(SEED, DRAW, ROW0 + r, n) for r in range(rows)]))
    x64 = x.double().requires_grad_()
    g, c = st[:, 0:1], 10.0 ** (-st[:, 3:4] / 20.0)
    s64 = g.abs() * x64.pow(2).mean(dim=1, keepdim=True).sqrt() * c
    (g * x64 + s64 * z).backward(dy.double())
    ref = x64.grad.numpy()
    ms64 = x.double().pow(2).mean(dim=1, keepdim=True).numpy()
    dyn, xn, zn, gn = dy.double().numpy(), x.double().numpy(), z.numpy(), g.numpy()
    k64 = s64.detach().numpy() / (n * ms64) * (dyn * zn).sum(axis=1, keepdims=True)
    k_err = np.abs(k64) * (1.5 * gamma(n + 2) + 1e-5 + 4 * U) + s64.detach().numpy() / (n * ms64) * (
        gamma(n + 2) * np.abs(dyn * zn).sum(axis=1, keepdims=True) + NOISE_TOL * np.abs(dyn).sum(axis=1, keepdims=True))
    bound = 2 * np.spacing((np.abs(gn * dyn) + np.abs(k64 * xn)).astype(np.float32)).astype(np.float64) + np.abs(xn) * k_err
    err = np.abs(dx - ref)
    print(f"backward n={n}: max err {err.max():.3e}, max err/bound {np.max(err / bound):.3f}, "
          f"share of the noise term {np.abs(k64 * xn).max() / np.abs(ref).max():.3e}")
    assert np.all(err <= bound)
    assert not np.array_equal(dx, xt.grad.double().cpu().numpy()), "the noise level takes part in the gradient"


def test_backward_of_a_silent_row_is_finite(awm, dev):
    x = signal(3, 1025)
    x[1] = 0
    xd = x.to(dev).requires_grad_()
    dy = torch.randn(3, 1025, generator=torch.Generator().manual_seed(9)).to(dev)
    y, stat = distort(awm, xd)
    y.backward(dy)
    assert bool(torch.isfinite(xd.grad).all())
    assert torch.equal(xd.grad[1], stat[1, 0] * dy[1])


# ------------------------------------------------------------------------------------------ 4. the modules
def test_distortion_module(awm, dev):
    x = signal(4, 2000).view(4, 1, 2000).to(dev)
    d = awm.Distortion(seed=5)
    a, b = d(x), d(x)
    assert a.shape == x.shape and d.draw == 2 and d.last_stat.shape == (4, 4) and not torch.equal(a, b)
    check_forward(x.view(4, 2000).cpu(), b.view(4, 2000), d.last_stat, (-6.0, 6.0, 20.0, 40.0, 1.0), 5, 1, 0, "module, second draw")
    assert torch.equal(d.reset()(x), a) and torch.equal(d(x), b)
    assert torch.equal(d.reset()(x[2:], row0=2), a[2:])
    assert torch.equal(awm.Distortion(gain_db=0, snr_db=None)(x), x)
    flat = x[0, 0]
    assert torch.equal(d.reset()(flat), a[0, 0]) and d(x.view(4, 2000)).shape == (4, 2000)
    # the CPU restatement draws the same parameters and, to the noise tolerance, the same samples
    h = awm.Distortion(seed=5)
    ah = h(x.cpu())
    assert torch.equal(d.reset()(x), a)
    assert torch.allclose(h.last_stat, d.last_stat.cpu(), rtol=1e-5, atol=0)
    # g and s of the two agree to 1e-5 (relative, above), z to NOISE_TOL: |difference| <= 1e-5 (|g x| + |s z|) + s NOISE_TOL + roundings
    st = d.last_stat.cpu()
    room = 1e-5 * (st[:, 0].view(4, 1, 1) * x.cpu().abs() + st[:, 1].view(4, 1, 1) * 5.77) + st[:, 1].view(4, 1, 1) * NOISE_TOL + 5e-7
    assert bool(((ah - a.cpu()).abs() <= room).all())
    # gradient modes through the module
    for mode in ("through", "detached"):
        xg = x.clone().requires_grad_()
        m = awm.Distortion(seed=5, noise_grad=mode)
        m(xg).sum().backward()
        assert bool(torch.isfinite(xg.grad).all())
        assert torch.equal(xg.grad, m.last_stat[:, 0].view(4, 1, 1).expand_as(xg)) == (mode == "detached")


def test_lowpass_forward_and_adjoint(awm, dev):
    from awm_amd import ops
    rate, cutoff = 16000, 4000
    W = ops.biquad_warm(ops.biquad_lowpass_coeffs(rate, cutoff))
    low = awm.Lowpass(cutoff, rate)
    for n in (1, 65, 1000, 4097):
        x = 3.0 * signal(3, n, seed=4)                                            # loud: a clamp would show
        w = signal(3, n, seed=5)
        y64, bound = biquad_yardstick.yardstick(x.numpy(), rate, cutoff, W)
        xd = x.view(3, 1, n).to(dev).requires_grad_()
        y = low(xd)
        assert y.shape == (3, 1, n)
        err = np.abs(y.detach().double().cpu().numpy().reshape(3, n) - y64)
        print(f"lowpass n={n}: max err/bound {np.max(err / bound):.3f}")
        assert np.all(err <= bound)
        if n >= 1000:
            assert float(np.abs(y64).max()) > 1.0, "this input is meant to show a clamp"
        # <L x, w> = <x, L^T w>: L^T w is the filter of the flipped w, flipped; its bound is the forward bound of that run
        y.backward(w.view(3, 1, n).to(dev))
        lt = xd.grad.double().cpu().numpy().reshape(3, n)
        r64, rbound = biquad_yardstick.yardstick(w.numpy()[:, ::-1], rate, cutoff, W)
        assert np.all(np.abs(lt - r64[:, ::-1]) <= rbound[:, ::-1])
        lhs = float((y.detach().double().cpu().numpy().reshape(3, n) * w.double().numpy()).sum())
        rhs = float((x.double().numpy() * lt).sum())
        room = float((bound * np.abs(w.double().numpy())).sum() + (np.abs(x.double().numpy()) * rbound[:, ::-1]).sum())
        print(f"lowpass n={n}: <Lx, w> - <x, L^T w> = {lhs - rhs:.3e}, room {room:.3e}")
        assert abs(lhs - rhs) <= room


# ------------------------------------------------------------------------------------------ 5. the step and the evaluation loop
def test_train_step_through_a_chain(awm, dev):
    """T = 2048, not 1024: the loudness loss pads its 2048-point frames by reflection, which needs T > 1024 (wm_loud_loss returns
    hipErrorInvalidValue below that, as torch.stft does), so 2048 is the shortest clip of the other step tests that the step accepts"""
    G, D = reference_models(awm, dev)
    G2, D2 = copy.deepcopy(G), copy.deepcopy(D)
    B, T = 2, 2048
    s = O.synthetic_clips(B, seed=41, T=T).to(dev)
    msg = torch.tensor([3, 60001], device=dev)
    codec = torch.nn.Sequential(awm.Distortion(seed=3), awm.PcmCodec(grad="straight_through"))
    grads = []
    for g, d in ((G, D), (G2, D2)):
        g.train(); d.train()
        codec[0].reset()
        opt = torch.optim.Adam(list(g.parameters()) + list(d.parameters()), lr=1e-3)
        out = awm.train_step(g, d, opt, s, msg, codec=codec)
        assert codec[0].draw == 1 and bool(torch.isfinite(out["total"]))
        assert not torch.equal(out["s_w"], s + out["delta"].detach())
        grads.append({k: p.grad.clone() for k, p in g.named_parameters()})
    for k, v in grads[0].items():
        assert bool(torch.isfinite(v).all()) and bool((v != 0).any()), f"Generator {k}"
        assert torch.equal(v, grads[1][k]), f"Generator {k}: the same step from the same weights after reset()"


def test_evaluate_robustness(awm, dev):
    ck = np.load(os.path.join(os.path.dirname(__file__), "golden", "detector_best_unprefixed.npz"))
    D = awm.Detector(16)
    D.load_state_dict({k: torch.from_numpy(ck[k]) for k in ck.files})
    torch.manual_seed(17)
    G = awm.Generator(16)
    G.to(dev); D.to(dev)
    batches = [O.synthetic_clips(2, seed=51, T=2048), O.synthetic_clips(2, seed=52, T=2048)]
    messages = [torch.tensor([3, 60001]), torch.tensor([77, 12345])]
    atk = {"noise": awm.Distortion(gain_db=(-6, 6), snr_db=(5, 10), seed=9),
           "chain": torch.nn.Sequential(awm.Lowpass(3000), awm.Distortion(gain_db=-12, snr_db=None), awm.PcmCodec())}
    res = awm.evaluate_robustness(G, D, batches, atk, device=dev, messages=messages)
    assert list(res) == ["none", "noise", "chain"]
    assert not G.training and not D.training
    base = awm.evaluate_batches(G, D, batches, device=dev, messages=messages)
    print(res, base)
    assert res["none"] == base
    # by hand, from eval-mode module calls
    twin = {"noise": awm.Distortion(gain_db=(-6, 6), snr_db=(5, 10), seed=9), "chain": atk["chain"]}
    for name, attack in twin.items():
        acc = {"watermarked_prob": [], "clean_prob": [], "bit_accuracy": [], "delta_rms": []}
        with torch.no_grad():
            for s, m in zip(batches, messages):
                s, m = s.to(dev), m.to(dev)
                delta = awm.postprocess(G(s, m))
                lg = D(attack(torch.cat([s + delta, s], dim=0)))
                p = torch.sigmoid(lg[:, :, 0]).mean(dim=1)
                decoded = (torch.sigmoid(lg[:2, :, 1:]) > 0.5).float().mean(dim=1) > 0.5
                bits = (m.unsqueeze(1) & (1 << torch.arange(16, device=dev))) > 0
                acc["watermarked_prob"].append(p[:2]); acc["clean_prob"].append(p[2:])
                acc["bit_accuracy"].append((decoded == bits).float().mean(dim=1))
                acc["delta_rms"].append(torch.sqrt((delta ** 2).mean(dim=[1, 2])))
        for k, v in acc.items():
            assert res[name][k] == pytest.approx(float(torch.cat(v).double().mean()), rel=1e-6, abs=1e-9), (name, k)
    assert res["noise"]["delta_rms"] == res["none"]["delta_rms"]
    assert res["noise"]["clean_prob"] != res["none"]["clean_prob"], "the attack reaches the clean half"
    assert res["noise"]["watermarked_prob"] != res["none"]["watermarked_prob"]
