"""The resampling attack on the GPU: wm_resample_rows (csrc/resample.hip) on batches of rows, the same launch with the transposed table as
its adjoint, attacks.Resampled through autograd, and the attack inside evaluate_robustness / train_step.

The yardstick is apply64 / adjoint64 / attack64 / attack_grad64 of tests/resample_yardstick.py, float64 numpy with nothing from the
package; the derived one-stage and two-stage tolerances stand in that module's docstring."""
import copy
import math

import numpy as np
import pytest
import torch

from gpu_support import awm, dev  # noqa: F401
from gpu_support import reference_models
from oracle import wm_oracle as O
from resample_yardstick import adjoint64, adjoint_gamma, apply64, attack64, attack_grad64, design, forward_gamma, rows_signal
from yardstick_common import assert_within, ulp32

pytestmark = pytest.mark.gpu

PAIRS = [(16000, 8000), (8000, 16000), (16000, 12000), (12000, 16000), (16000, 44100), (44100, 16000), (16000, 12345), (12345, 16000)]
RATES = [8000, 12000, 44100]


def lengths(ops, orig, new):
    """input lengths around every path of the kernel: below one period, whole periods, the ends of a tile, several tiles"""
    P = orig // math.gcd(orig, new)
    tile = ops.resample_tile_periods(orig, new)
    if orig in (12345,) or new in (12345,):
        assert tile == 0, "the one-thread-per-sample kernel is what this pair is here for"
        return [1, P, 6 * P + 11]
    assert tile > 0 and tile % 4 == 0
    return [n for n in (1, 2, P - 1, P, 7 * P + 3, tile * P - 1, tile * P + 1, 3 * tile * P + 5) if n > 0]


def tile_periods(awm, tab):
    """wm_resample_plan for a table dict: output periods of one LDS tile, 0 when the one-thread-per-sample kernel runs"""
    import ctypes
    out = (ctypes.c_longlong * 1)()
    awm.lib.wm_resample_plan(tab["P"], tab["Q"], tab["width"], tab["W"], ctypes.addressof(out), None)
    return int(out[0])


_DEV_TABLES = {}


def launch_rows(awm, x, tab, L):
    """wm_resample_rows itself on the contiguous (rows, N) CUDA tensor x with the table dict `tab`, into a NaN-filled buffer with one guard
    row behind it: every sample is written, nothing past rows * L is touched"""
    rows, N = x.shape
    key = (id(tab), x.device)
    if key not in _DEV_TABLES:
        _DEV_TABLES[key] = (tab, tab["taps"].to(x.device), tab["first"].to(x.device))
    _, taps, first = _DEV_TABLES[key]
    buf = torch.full((rows + 1, L), float("nan"), device=x.device)
    awm.lib.wm_resample_rows(x.data_ptr(), taps.data_ptr(), first.data_ptr(), buf.data_ptr(), rows, N, L, tab["P"], tab["Q"], tab["width"],
                             tab["W"], torch.cuda.current_stream().cuda_stream)
    out = buf.cpu()
    assert not torch.isnan(out[:rows]).any(), "the kernel left samples unwritten"
    assert bool(torch.isnan(out[rows]).all()), "the kernel wrote past rows * L"
    return out[:rows]


# ------------------------------------------------------------------------------------------ 1. rows against float64
@pytest.mark.parametrize("rows", [1, 3, 5])
@pytest.mark.parametrize("orig,new", PAIRS)
def test_rows_vs_float64(awm, dev, orig, new, rows):
    from awm_amd import ops
    assert ops.resample_tile_periods(16000, 12345) == 0 and ops.resample_tile_periods(12345, 16000) == 0
    P, Q, width, K, h32 = design(orig, new)
    h, habs = h32.astype(np.float64), np.abs(h32).astype(np.float64)
    tab = ops.resample_table(orig, new)
    for k, N in enumerate(lengths(ops, orig, new)):
        x = rows_signal(rows, N, seed=10 * rows + k)
        L = ops.resample_length(N, orig, new)
        y = launch_rows(awm, x.to(dev), tab, L)
        got = ops.resample_rows(x.to(dev), orig, new)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (rows, L) and torch.equal(got.cpu(), y)
        for r in range(rows):
            x64 = x[r].double().numpy()
            ref = apply64(h, P, width, x64, L)
            bound = forward_gamma(h32, L) * apply64(habs, P, width, np.abs(x64), L) + ulp32(ref)
            assert_within(y[r].numpy(), ref, bound, f"{orig}->{new} rows={rows} N={N} row {r}")


def test_rows_arguments(awm, dev):
    from awm_amd import ops
    x = torch.randn(3, 100, device=dev)
    assert ops.resample_rows(x, 16000, 16000) is x
    assert torch.equal(ops.resample_rows(x, 16000, 16000, length=40), x[:, :40])
    assert tuple(ops.resample_rows(x, 16000, 8000, length=0).shape) == (3, 0)
    assert tuple(ops.resample_rows(torch.zeros(0, 100, device=dev), 16000, 8000).shape) == (0, 50)
    with pytest.raises(ValueError):
        ops.resample_rows(x, 16000, 8000, length=51)
    with pytest.raises(ValueError):
        ops.resample_rows(x[0], 16000, 8000)
    with pytest.raises(RuntimeError):
        ops.resample_rows(x.cpu(), 16000, 8000)                                              # a CPU tensor has no business in ops
    with pytest.raises(ValueError):
        ops.resample_rows(x, 16000, 0)
    tab = ops.resample_table(16000, 8000)
    taps, first = tab["taps"].to(dev), tab["first"].to(dev)
    y = torch.empty(3, 50, device=dev)
    for bad in ({"rows": -1}, {"N": -1}, {"L": -1}, {"P": 0}, {"Q": 0}, {"width": -1}, {"W": 0}, {"W": 2 * tab["width"] + tab["P"] + 1}):
        a = dict(rows=3, N=100, L=50, P=tab["P"], Q=tab["Q"], width=tab["width"], W=tab["W"])
        a.update(bad)
        with pytest.raises(RuntimeError):
            awm.lib.wm_resample_rows(x.data_ptr(), taps.data_ptr(), first.data_ptr(), y.data_ptr(), a["rows"], a["N"], a["L"], a["P"], a["Q"],
                                     a["width"], a["W"], None)
    with pytest.raises(RuntimeError):
        awm.lib.wm_resample_rows(x.data_ptr(), None, first.data_ptr(), y.data_ptr(), 3, 100, 50, tab["P"], tab["Q"], tab["width"], tab["W"], None)
    awm.lib.wm_resample_rows(None, None, None, None, 0, 100, 50, tab["P"], tab["Q"], tab["width"], tab["W"], None)     # nothing to do: no launch
    awm.lib.wm_resample_rows(None, None, None, None, 3, 100, 0, tab["P"], tab["Q"], tab["width"], tab["W"], None)


# ------------------------------------------------------------------------------------------ 2. bit identity with the one-recording kernel
@pytest.mark.parametrize("orig,new", PAIRS)
def test_rows_are_the_single_recording_kernel(awm, dev, orig, new):
    from awm_amd import ops
    P, Q = orig // math.gcd(orig, new), new // math.gcd(orig, new)
    ns = lengths(ops, orig, new)[-4:]
    assert any(n % 4 for n in ns), "rows off the 16-byte grid"
    for k, N in enumerate(ns):
        x = rows_signal(3, N, seed=40 + k).to(dev)
        y = ops.resample_rows(x, orig, new)
        for r in range(3):
            assert torch.equal(y[r], ops.resample(x[r:r + 1], orig, new)[0]), f"{orig}->{new} N={N} row {r}"
        for cut in sorted({0, 1, y.shape[1] // 2, max(y.shape[1] - Q - 1, 0), y.shape[1]}):
            assert torch.equal(ops.resample_rows(x, orig, new, length=cut), y[:, :cut]), f"{orig}->{new} N={N} length={cut}"


# ------------------------------------------------------------------------------------------ 3. the adjoint launch against float64
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("orig,new", PAIRS)
def test_adjoint_vs_float64(awm, dev, orig, new, rows):
    from awm_amd import ops
    P, Q, width, K, h32 = design(orig, new)
    h, habs = h32.astype(np.float64), np.abs(h32).astype(np.float64)
    adj = ops.resample_adjoint_table(orig, new)
    assert (adj["P"], adj["Q"]) == (Q, P)
    assert (tile_periods(awm, adj) == 0) == (12345 in (orig, new)), "12345: the adjoint runs from the one-thread-per-sample kernel too"
    saw_unreached = False
    for k, N in enumerate(lengths(ops, orig, new)):
        full = ops.resample_length(N, orig, new)
        for L in sorted({full, max(full // 2, 1)}):                                           # ... and cut below ceil(Q*N/P)
            dy = rows_signal(rows, L, seed=70 + 10 * rows + k)
            dx = launch_rows(awm, dy.to(dev), adj, N)
            reach = adjoint64(habs, P, width, np.ones(L), N)                                 # 0.0 where no kept output reads the sample
            for r in range(rows):
                d64 = dy[r].double().numpy()
                ref = adjoint64(h, P, width, d64, N)
                bound = adjoint_gamma(h32, P, width, N) * adjoint64(habs, P, width, np.abs(d64), N) + ulp32(ref)
                assert_within(dx[r].numpy(), ref, bound, f"adjoint of {orig}->{new} rows={rows} N={N} L={L} row {r}")
                assert bool((dx[r].numpy()[reach == 0.0] == 0.0).all()), "a sample no kept output reads has a gradient"
            saw_unreached |= L < full and bool((reach[-1:] == 0.0).all())
    assert saw_unreached, "no case where the cut leaves trailing samples without a gradient"


# ------------------------------------------------------------------------------------------ 4. autograd through the module
@pytest.mark.parametrize("T", [1, 37, 4001, 16000])
@pytest.mark.parametrize("rate", RATES)
def test_resampled_forward_and_backward(awm, dev, rate, T):
    att = awm.Resampled(rate)
    x_cpu, g_cpu = rows_signal(3, T, seed=rate % 89), rows_signal(3, T, seed=rate % 89 + 1)
    x = x_cpu.view(3, 1, T).to(dev).requires_grad_()
    y = att(x)
    assert y.is_cuda and tuple(y.shape) == (3, 1, T) and y.dtype == torch.float32
    (y * g_cpu.view(3, 1, T).to(dev)).sum().backward()
    assert tuple(x.grad.shape) == (3, 1, T)
    for r in range(3):
        ref, bound = attack64(x_cpu[r].double().numpy(), rate)
        assert_within(y[r, 0].detach().cpu().numpy(), ref, bound, f"Resampled({rate}) T={T} row {r}")
        ref, bound = attack_grad64(g_cpu[r].double().numpy(), rate)
        assert_within(x.grad[r, 0].cpu().numpy(), ref, bound, f"Resampled({rate}) gradient T={T} row {r}")
    # twice the same, bit for bit
    x2 = x_cpu.view(3, 1, T).to(dev).requires_grad_()
    y2 = att(x2)
    (y2 * g_cpu.view(3, 1, T).to(dev)).sum().backward()
    assert torch.equal(y2, y) and torch.equal(x2.grad, x.grad)
    # a view that is not contiguous
    wide = torch.stack([x_cpu, -x_cpu], dim=-1).to(dev)                                       # (3, T, 2)
    view = wide[..., 0].unsqueeze(1)
    assert T == 1 or not view.is_contiguous()
    assert torch.equal(att(view), y.detach())
    assert torch.equal(att(x_cpu[1].to(dev)), y[1, 0].detach())                               # (N,): a row by itself
    assert torch.equal(att(x_cpu.to(dev)), y[:, 0].detach())                                  # (C, N)


def test_equal_rates_and_repr(awm, dev):
    x = torch.randn(2, 1, 64, device=dev)
    assert awm.Resampled(16000)(x) is x
    with pytest.raises(ValueError):
        awm.Resampled(0)
    assert repr(awm.Resampled(8000)) == "Resampled(rate=8000, sample_rate=16000)"


# ------------------------------------------------------------------------------------------ 5. what the attack means
def test_tones_through_8k(awm, dev):
    """properties of the published design (measured in float64: the 7 kHz tone comes back at 3.3e-5 of its RMS on samples 200 .. T-200, the
    1 kHz tone within 1.5e-4; the zero extension rings at the clip ends, up to 4e-2, which is the design and why the ends are left out)"""
    T = 16000
    t = np.arange(T) / 16000.0
    att = awm.Resampled(8000)
    inner = slice(200, T - 200)
    hi = 0.5 * np.sin(2 * np.pi * 7000.0 * t)
    y = att(torch.from_numpy(hi).float().view(1, 1, T).to(dev))[0, 0].double().cpu().numpy()
    ratio = np.sqrt(np.mean(y[inner] ** 2)) / np.sqrt(np.mean(hi[inner] ** 2))
    y64, _ = attack64(hi.astype(np.float32).astype(np.float64), 8000)
    print(f"7 kHz through 8 kHz: interior RMS ratio {ratio:.3e} (float64 design {np.sqrt(np.mean(y64[inner] ** 2) / np.mean(hi[inner] ** 2)):.3e})")
    assert ratio < 1e-3
    lo = 0.5 * np.sin(2 * np.pi * 1000.0 * t)
    y = att(torch.from_numpy(lo).float().view(1, 1, T).to(dev))[0, 0].double().cpu().numpy()
    worst = np.abs(y - lo)[inner].max()
    print(f"1 kHz through 8 kHz: interior max deviation {worst:.3e}, at the ends {np.abs(y - lo).max():.3e}")
    assert worst < 1e-3


# ------------------------------------------------------------------------------------------ 6. in the loops
def test_evaluate_robustness_with_resampling(awm, dev):
    from awm_amd.step import _eval_reductions
    G, D = reference_models(awm, dev, perturb_bn=False)
    s, m = O.synthetic_clips(2, seed=61, T=16000), torch.tensor([3, 60001])
    res = awm.evaluate_robustness(G, D, [s], {"resample_8k": awm.Resampled(8000)}, device=dev, messages=[m])
    assert list(res) == ["none", "resample_8k"]
    keys = {"watermarked_prob": "prob_watermarked", "clean_prob": "prob_clean", "bit_accuracy": "bit_accuracy", "delta_rms": "delta_rms"}
    with torch.no_grad():
        s, m = s.to(dev), m.to(dev)
        delta = awm.postprocess(G(s, m))
        hand = _eval_reductions(D(awm.Resampled(8000)(torch.cat([s + delta, s], dim=0))), m, delta)
    print(res)
    for k, src in keys.items():
        assert math.isfinite(res["resample_8k"][k])
        assert abs(res["resample_8k"][k] - float(hand[src].double().mean())) <= 1e-6, k
    assert res["resample_8k"]["delta_rms"] == res["none"]["delta_rms"]
    assert res["resample_8k"]["clean_prob"] != res["none"]["clean_prob"], "the attack reaches the clean half"


def test_train_step_through_resampling(awm, dev):
    G, D = reference_models(awm, dev, perturb_bn=False)
    G2, D2 = copy.deepcopy(G), copy.deepcopy(D)
    s, msg = O.synthetic_clips(2, seed=62, T=16000).to(dev), torch.tensor([3, 60001], device=dev)
    codec = torch.nn.Sequential(awm.Resampled(8000), awm.PcmCodec(grad="straight_through"))
    grads = []
    for g, d, c in ((G, D, codec), (G2, D2, None)):
        g.train(); d.train()
        opt = torch.optim.Adam(list(g.parameters()) + list(d.parameters()), lr=1e-3)
        out = awm.train_step(g, d, opt, s, msg, codec=c)
        for k in ("l1", "mel", "loud", "loc", "bce", "hf", "raw_total", "total"):
            assert bool(torch.isfinite(out[k]).all()), k
        grads.append({k: p.grad.clone() for k, p in g.named_parameters()})
    for k, v in grads[0].items():
        assert bool(torch.isfinite(v).all()), f"Generator {k}"
    assert any(not torch.equal(v, grads[1][k]) for k, v in grads[0].items()), "the attack is not in the Generator's graph"
    assert all(bool((v != 0).any()) for v in grads[0].values()), "a Generator parameter the attacked step does not reach"


def test_resample_without_mixdown(awm, dev):
    from awm_amd import ops
    x = rows_signal(2, 48000 + 77, seed=9).to(dev)
    y = awm.resample(x, 48000, 16000, mixdown=False)
    assert y.is_cuda and tuple(y.shape) == (2, ops.resample_length(48077, 48000, 16000))
    for c in range(2):
        assert torch.equal(y[c], ops.resample(x[c:c + 1], 48000, 16000)[0])
    assert torch.equal(awm.resample(x, 48000, 16000, mixdown=True), awm.resample(x, 48000, 16000))
