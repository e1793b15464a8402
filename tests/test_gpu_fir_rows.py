"""wm_fir_rows / wm_rir_synth / ops.fir_rows / ops.FirRowsFn / ops.rir_synth / attacks.Convolved / attacks.Reverb on the GPU against the
float64 yardstick of tests/fir_yardstick.py (numpy from the definitions in include/wm_hip.h; nothing from the package).

Tolerances (none tuned to the kernel):
  integers   x in [-8, 8], h in [-4, 4]: every partial sum stays below 2^24 (at most 4096 * 32 = 131072), so fp32 is exact in any order and the
             kernel must equal int64 np.convolve EXACTLY.
  floats     |y - y64| <= gamma(K + 2) sum_k |h_k x_{t-k}|, gamma(m) = m u / (1 - m u), u = 2^-24: the bound of ANY order of K rounded products.
  adjoint    |<H u, v> - <u, H^T v>| <= sum |v| bound(u) + sum |u| bound^T(v), the two bounds above carried through the inner products.
  responses  |h - h64| <= a64 exp(-k c) NOISE_TOL + (gamma(K + 2) + 2e-5) |h64| + 1e-37, NOISE_TOL the project's measured bound on the device
             normal (tests/test_gpu_attacks.py, restated in the yardstick).
Every reference is computed once per case (lru_cache in the yardstick) and never written to.

Measured on an MI355X (largest err / bound per test, printed by every case): see DESIGN.md section 4h."""
import os

import numpy as np
import pytest
import torch

from oracle import wm_oracle as O

import fir_yardstick as Y
from gpu_support import awm, dev  # noqa: F401
from gpu_support import bits, reference_models, to_dev

pytestmark = pytest.mark.gpu


def launch(dev, x, h, reverse=False):
    from awm_amd import ops
    return ops.fir_rows(to_dev(x, dev), to_dev(h, dev), reverse=reverse).cpu().numpy()


# ------------------------------------------------------------------------------------------ 1. exact on integers
@pytest.mark.parametrize("rows,n,K", Y.CASES)
def test_exact_on_integers(awm, dev, rows, n, K):
    x, h = Y.int_case(rows, n, K)
    for shared in (False, True):
        hh = h[0] if shared else h
        for reverse, ref in ((False, Y.fir(x, hh)), (True, Y.fir_adjoint(x, hh))):
            y = launch(dev, x, hh, reverse)
            assert y.shape == x.shape and y.dtype == np.float32
            wrong = y.astype(np.int64) != ref
            assert not wrong.any() and (y == np.rint(y)).all(), \
                f"rows {rows} n {n} K {K} shared {shared} reverse {reverse}: {int(wrong.sum())} samples differ, first at {np.argwhere(wrong)[:3].tolist()}"


# ------------------------------------------------------------------------------------------ 2. floats against float64
@pytest.mark.parametrize("rows,n,K", Y.CASES)
def test_floats_against_float64(awm, dev, rows, n, K):
    x, h = Y.float_case(rows, n, K)
    worst = 0.0
    for shared in (False, True):
        for reverse in (False, True):
            ref, bnd = Y.float_ref(rows, n, K, shared, reverse)
            y = launch(dev, x, h[0] if shared else h, reverse).astype(np.float64)
            err = np.abs(y - ref)
            ratio = float((err / np.maximum(bnd, 1e-300)).max()) if (bnd > 0).any() else 0.0
            worst = max(worst, ratio)
            assert (err <= bnd).all(), f"rows {rows} n {n} K {K} shared {shared} reverse {reverse}: err / bound {ratio:.3f}"
    print(f"rows {rows} n {n} K {K}: worst err / bound {worst:.4f}")


# ------------------------------------------------------------------------------------------ 3. independent rows, reproducible launches
@pytest.mark.parametrize("n,K", [(33, 33), (1025, 64), (4099, 1000), (16000, 2048)])
def test_rows_are_independent_and_launches_reproducible(awm, dev, n, K):
    from awm_amd import ops
    x64, h64 = Y.float_case(3, n, K)
    x, h = to_dev(x64, dev), to_dev(h64, dev)
    for reverse in (False, True):
        y = ops.fir_rows(x, h, reverse=reverse)
        assert torch.equal(bits(ops.fir_rows(x, h, reverse=reverse)), bits(y)), "two launches give identical bits"
        for r in range(3):
            one = ops.fir_rows(x[r:r + 1].clone(), h[r:r + 1].clone(), reverse=reverse)
            assert torch.equal(bits(one[0]), bits(y[r])), f"row {r} alone equals row {r} of the batch"
        ys = ops.fir_rows(x, h[0].clone(), reverse=reverse)
        yc = ops.fir_rows(x, h[0:1].repeat(3, 1), reverse=reverse)
        assert torch.equal(bits(ys), bits(yc)), "a shared response equals the same response copied per row"
        xn = x.clone()
        xn[1] = float("nan")
        yn = ops.fir_rows(xn, h, reverse=reverse)
        assert bool(torch.isnan(yn[1]).all()) and torch.equal(bits(yn[0]), bits(y[0])) and torch.equal(bits(yn[2]), bits(y[2])), \
            "a row of NaN leaves its neighbours as they were"
    assert (x != 0).all()
    one = torch.ones(1, device=dev)
    assert torch.equal(bits(ops.fir_rows(x, one)), bits(x)) and torch.equal(bits(ops.fir_rows(x, one, reverse=True)), bits(x))
    assert torch.equal(bits(ops.fir_rows(x, torch.ones(3, 1, device=dev))), bits(x)), "h = {1} hands x on bit for bit"


# ------------------------------------------------------------------------------------------ 4. adjoint
@pytest.mark.parametrize("rows,n,K", [(3, 40, 100), (3, 1000, 257), (3, 4099, 1000), (3, 16000, 2048)])
def test_adjoint(awm, dev, rows, n, K):
    from awm_amd import ops
    u, h = Y.float_case(rows, n, K)
    v = np.random.default_rng(3000 * n + K).standard_normal((rows, n)).astype(np.float32).astype(np.float64)
    Hu = launch(dev, u, h).astype(np.float64)
    Htv = launch(dev, v, h, reverse=True).astype(np.float64)
    lhs, rhs = (Hu * v).sum(axis=1), (u * Htv).sum(axis=1)
    room = (np.abs(v) * Y.float_ref(rows, n, K, False, False)[1]).sum(axis=1) + (np.abs(u) * Y.bound_adjoint(v, h)).sum(axis=1)
    print(f"rows {rows} n {n} K {K}: |<Hu, v> - <u, H^T v>| / room {(np.abs(lhs - rhs) / room).max():.4f}")
    assert (np.abs(lhs - rhs) <= room).all()
    # the tape node: backward is H^T g, and the CPU conv1d path's autograd agrees on the same data
    xt, ht, gt = to_dev(u, dev).requires_grad_(True), to_dev(h, dev).requires_grad_(True), to_dev(v, dev)
    y = ops.FirRowsFn.apply(xt, ht)
    y.backward(gt)
    assert ht.grad is None, "the response is a constant of the graph"
    ref, bnd = Y.fir_adjoint(v, h), Y.bound_adjoint(v, h)
    err = np.abs(xt.grad.cpu().numpy().astype(np.float64) - ref)
    print(f"rows {rows} n {n} K {K}: backward worst err / bound {(err / np.maximum(bnd, 1e-300)).max():.4f}")
    assert (err <= bnd).all()
    xc = torch.from_numpy(u.astype(np.float32)).requires_grad_(True)
    att = awm.Convolved(torch.from_numpy(h[0].astype(np.float32)))
    att(xc).backward(torch.from_numpy(v.astype(np.float32)))
    xg = to_dev(u, dev).requires_grad_(True)
    att.to(dev)(xg).backward(gt)
    bnd0 = Y.bound_adjoint(v, h[0])
    assert (np.abs(xg.grad.cpu().numpy().astype(np.float64) - xc.grad.numpy().astype(np.float64)) <= 2 * bnd0).all(), \
        "both are fp32 evaluations of the same sums: each within the bound of float64"


# ------------------------------------------------------------------------------------------ 5. synthetic responses
@pytest.mark.parametrize("K", [1, 2, 33, 2048, 8192])
def test_rir_synth_against_the_yardstick(awm, dev, K):
    from awm_amd import ops
    seed, draw, row0, sr = (7 << 32) + 5, 3, 11, 16000
    cases = ((0.05, 0.0), (0.3, 10.0), (0.6, 20.0))
    params = torch.tensor(cases, dtype=torch.float32, device=dev)
    h = ops.rir_synth(params, K, sr, seed, draw, row0)
    assert tuple(h.shape) == (3, K) and h.dtype == torch.float32
    assert torch.equal(bits(ops.rir_synth(params, K, sr, seed, draw, row0)), bits(h)), "two launches give identical bits"
    hn = h.cpu().numpy().astype(np.float64)
    rel = Y.gamma(K + 2) + Y.RIR_REL
    for r, (rt60, drr) in enumerate(cases):
        one = ops.rir_synth(params[r:r + 1].clone(), K, sr, seed, draw, row0 + r)
        assert torch.equal(bits(one[0]), bits(h[r])), f"row {r} alone (row0 = {row0 + r}) equals row {r} of the batch"
        ref, env = Y.rir(seed, draw, row0 + r, rt60, drr, K, float(sr))
        bnd = Y.rir_bound(ref, env)
        err = np.abs(hn[r] - ref)
        print(f"K {K} rt60 {rt60} drr {drr}: worst err / bound {(err / bnd).max():.4f}")
        assert (err <= bnd).all()
        energy = (hn[r] ** 2).sum()
        assert abs(energy - 1.0) <= rel, f"energy {energy}"
        if K > 1:
            w = 10.0 ** (-drr / 10.0)
            got = (hn[r, 1:] ** 2).sum() / hn[r, 0] ** 2
            print(f"K {K} rt60 {rt60} drr {drr}: energy - 1 {energy - 1.0:.2e}, DRR ratio - 1 {got / w - 1.0:.2e}")
            assert abs(got / w - 1.0) <= rel, f"direct-to-reverberant ratio {-10 * np.log10(got):.4f} dB, asked {drr}"
        else:
            assert hn[r, 0] == 1.0
    flat = ops.rir_synth(torch.tensor([[0.0, 6.0], [0.3, float("nan")], [1e-7, 6.0]], device=dev), max(K, 2), sr, seed, draw, 0).cpu()
    assert (flat[:, 0] == 1).all() and not flat[:, 1:].any(), "rt60 <= 0, a non-finite ratio, no energy: the response is {1, 0, ...}"


# ------------------------------------------------------------------------------------------ 6. modules
@pytest.mark.parametrize("shape", [(3, 1, 2500), (2, 1300), (700,)])
def test_reverb_gpu_agrees_with_its_cpu_path(awm, dev, shape):
    rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
    x = np.random.default_rng(61).standard_normal(shape).astype(np.float32)
    K = 513
    g, c = awm.Reverb(taps=K, seed=8), awm.Reverb(taps=K, seed=8)
    yg, yc = g(torch.from_numpy(x).to(dev), row0=4), c(torch.from_numpy(x), row0=4)
    assert yg.shape == yc.shape == x.shape and yg.is_cuda and g.draw == c.draw == 1
    assert torch.equal(g.last_params, c.last_params) and not g.last_params.is_cuda and g.last_ir.is_cuda
    rt60, drr = Y.reverb_params(8, 0, 4 + np.arange(rows), (0.1, 0.4), (0, 12))
    assert np.array_equal(g.last_params.numpy(), np.stack([rt60, drr], axis=1))
    hg, hc = g.last_ir.cpu().numpy().astype(np.float64), c.last_ir.numpy().astype(np.float64)
    for r in range(rows):
        ref, env = Y.rir(8, 0, 4 + r, rt60[r], drr[r], K, 16000.0)
        assert (np.abs(hg[r] - ref) <= Y.rir_bound(ref, env)).all() and (np.abs(hc[r] - ref) <= Y.rir_bound(ref, env)).all()
    x2 = x.reshape(rows, -1).astype(np.float64)
    room = Y.bound(x2, hg) + Y.bound(x2, hc) + Y.fir(np.abs(x2), np.abs(hg - hc))
    diff = np.abs(yg.cpu().numpy().reshape(rows, -1).astype(np.float64) - yc.numpy().reshape(rows, -1))
    print(f"{shape}: GPU against CPU worst / room {(diff / room).max():.4f}")
    assert (diff <= room).all()


def test_reverb_draw_reset_and_split_batches(awm, dev):
    x = torch.from_numpy(np.random.default_rng(62).standard_normal((5, 1, 3000)).astype(np.float32)).to(dev)
    att = awm.Reverb(taps=300, seed=2)
    a, b = att(x), att(x)
    assert att.draw == 2 and not torch.equal(a, b)
    assert torch.equal(bits(att.reset()(x)), bits(a)) and torch.equal(bits(att.reset(1)(x)), bits(b))
    att.reset()(x)
    whole_ir = att.last_ir.clone()
    parts = torch.cat([att.reset()(x[:2]), att.reset()(x[2:], row0=2)])
    assert torch.equal(bits(parts), bits(a)) and torch.equal(bits(att.last_ir), bits(whole_ir[2:])), \
        "a batch cut into pieces draws what the whole batch does"


@pytest.mark.parametrize("shape", [(6, 1, 2100), (2, 900), (500,)])
def test_convolved_gpu_agrees_with_its_cpu_path(awm, dev, shape):
    rows = int(np.prod(shape[:-1])) if len(shape) > 1 else 1
    rng = np.random.default_rng(63)
    x = rng.standard_normal(shape).astype(np.float32)
    bank = np.stack([Y.rir(9, 0, r, 0.2, 3.0, 200, 16000.0)[0] for r in range(4)]).astype(np.float32) * np.float32(1.7)
    g, c = awm.Convolved(torch.from_numpy(bank), normalize=True, seed=21).to(dev), awm.Convolved(torch.from_numpy(bank), normalize=True, seed=21)
    assert g.h.is_cuda and torch.equal(g.h.cpu(), c.h)
    yg, yc = g(torch.from_numpy(x).to(dev), row0=3), c(torch.from_numpy(x), row0=3)
    idx = Y.bank_index(21, 0, 3 + np.arange(rows), 4)
    assert np.array_equal(g.last_index.numpy(), idx) and np.array_equal(c.last_index.numpy(), idx), "the bank entry is the yardstick's"
    h = c.h.numpy().astype(np.float64)[idx]
    x2 = x.reshape(rows, -1).astype(np.float64)
    ref, bnd = Y.fir(x2, h), Y.bound(x2, h)
    assert yg.shape == x.shape and (np.abs(yg.cpu().numpy().reshape(rows, -1) - ref) <= bnd).all()
    assert (np.abs(yc.numpy().reshape(rows, -1) - ref) <= bnd).all()
    if rows > 2:
        whole = g.reset()(torch.from_numpy(x).to(dev))
        parts = torch.cat([g.reset()(torch.from_numpy(x[:2]).to(dev)), g.reset()(torch.from_numpy(x[2:]).to(dev), row0=2)])
        assert torch.equal(bits(whole), bits(parts))
    echo = awm.Convolved(awm.echo_ir(0.05, -6.0)).to(dev)
    ye = echo(torch.from_numpy(x).to(dev))
    he = awm.echo_ir(0.05, -6.0).numpy().astype(np.float64)
    assert (np.abs(ye.cpu().numpy().reshape(rows, -1) - Y.fir(x2, he)) <= Y.bound(x2, he)).all()


def test_train_step_through_the_reverb(awm, dev):
    """T = 2048: the shortest clip the step's loudness loss accepts"""
    G, D = reference_models(awm, dev)
    s = O.synthetic_clips(2, seed=41, T=2048).to(dev)
    msg = torch.tensor([3, 60001], device=dev)
    codec = torch.nn.Sequential(awm.Reverb(taps=512, seed=3), awm.PcmCodec(grad="straight_through"))
    G.train(); D.train()
    before = [p.detach().clone() for p in G.parameters()]
    opt = torch.optim.Adam(list(G.parameters()) + list(D.parameters()), lr=1e-3)
    out = awm.train_step(G, D, opt, s, msg, codec=codec)
    assert codec[0].draw == 1 and tuple(codec[0].last_params.shape) == (2, 2) and tuple(codec[0].last_ir.shape) == (2, 512)
    for k, v in out.items():
        if torch.is_tensor(v) and v.dim() == 0:
            assert bool(torch.isfinite(v)), f"loss {k}"
    assert bool(torch.isfinite(out["total"]))
    assert not torch.equal(out["s_w"], s + out["delta"].detach())
    for k, p in G.named_parameters():
        assert bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()), f"Generator {k}"
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, G.parameters())), "the step moves the parameters"


def test_evaluate_robustness_with_the_reverb(awm, dev):
    ck = np.load(os.path.join(os.path.dirname(__file__), "golden", "detector_best_unprefixed.npz"))
    D = awm.Detector(16)
    D.load_state_dict({k: torch.from_numpy(ck[k]) for k in ck.files})
    torch.manual_seed(17)
    G = awm.Generator(16)
    G.to(dev); D.to(dev)
    batches = [O.synthetic_clips(2, seed=51, T=2048), O.synthetic_clips(2, seed=52, T=2048)]
    messages = [torch.tensor([3, 60001]), torch.tensor([77, 12345])]
    atk = {"reverb": awm.Reverb(taps=1024, seed=9), "echo": awm.Convolved(awm.echo_ir(0.03, -6.0)),
           "dry": awm.Convolved(torch.tensor([1.0]))}
    res = awm.evaluate_robustness(G, D, batches, atk, device=dev, messages=messages)
    print(res)
    assert list(res) == ["none", "reverb", "echo", "dry"]
    keys = ["bit_accuracy", "clean_prob", "delta_rms", "watermarked_prob"]
    for name in ("reverb", "echo"):
        assert sorted(res[name]) == keys and all(np.isfinite(res[name][k]) for k in keys)
    assert atk["reverb"].draw == 2, "one call per batch, on the concatenation of s + delta and s"
    for k in keys:
        assert res["dry"][k] == res["none"][k], "h = {1} is the identity"


# ------------------------------------------------------------------------------------------ 7. bad arguments
def test_bad_arguments(awm, dev):
    from awm_amd import ops
    for args in Y.BAD_FIR_ARGS:
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm.lib.wm_fir_rows(*args)
    for args in Y.BAD_RIR_ARGS:
        with pytest.raises(RuntimeError, match="hipError 1$"):
            awm.lib.wm_rir_synth(*args)
    x, h = torch.zeros(3, 100, device=dev), torch.ones(8, device=dev)
    for bad_x, bad_h in ((x, torch.ones(2, 8, device=dev)), (x, torch.ones(1, 3, 8, device=dev)), (x, torch.ones(0, device=dev)),
                         (x, torch.ones(16385, device=dev)), (x, h.double()), (x.double(), h), (torch.zeros(3, 0, device=dev), h),
                         (torch.zeros((), device=dev), h)):
        with pytest.raises(ValueError):
            ops.fir_rows(bad_x, bad_h)
    with pytest.raises(RuntimeError):
        ops.fir_rows(x, h.cpu())
    with pytest.raises(RuntimeError):
        ops.fir_rows(x.cpu(), h)
    with pytest.raises(TypeError):
        ops.fir_rows(x, [1.0])
    p = torch.tensor([[0.3, 6.0]], device=dev)
    for kw in (dict(taps=0), dict(taps=16385), dict(taps=True), dict(taps=8.0), dict(sample_rate=0), dict(sample_rate=float("nan")),
               dict(draw=-1), dict(draw=2 ** 32), dict(row0=-1), dict(row0=2 ** 32), dict(draw=True)):
        a = dict(taps=8)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.rir_synth(p, **a)
    for bad in (torch.zeros(2, 3, device=dev), torch.zeros(2, device=dev), torch.zeros(0, 2, device=dev), p.double()):
        with pytest.raises(ValueError):
            ops.rir_synth(bad, 8)
    torch.cuda.synchronize()
