"""csrc/stft_loss.hip, csrc/postproc.hip and the BCE / L1 / Adam kernels of csrc/losses.hip against the float64 yardsticks of
tests/loss_yardstick.py, at the shapes where they can go wrong: the shortest clips (both reflections on the same samples), lengths
that are and are not multiples of the hop, an odd frame count for the two-frames-per-FFT HF kernel, a LOUD mask that is half on,
asymmetric FIR taps, every stage mask, T from 1 to the 36000 limit, 1 to 64 logit channels with bit 62 set, and Adam element by
element.  The rule for every bar is max(8 * e32, floor) (loss_yardstick.py); the input conditions that keep every reference value clear
of a threshold are asserted in tests/test_loss_yardstick_cpu.py.

Measured on 1 x MI355X: the largest distance from float64 per group, the bar there at its smallest, the largest e32, and the largest
distance / bar of any compared tensor.

    group                cases   distance   smallest bar   e32       distance / bar
    MEL value              6     5.6e-08    1.2e-06        5.7e-08   0.05
    MEL gradient           6     2.0e-07    2.4e-06        1.9e-07   0.08
    LOUD value             6     1.4e-07    1.3e-06        1.3e-07   0.11
    LOUD gradient          6     6.8e-07    3.1e-06        6.3e-07   0.15
    HF value               7     3.5e-08    1.1e-06        1.2e-07   0.03
    HF gradient            7     6.5e-07    2.1e-06        4.6e-07   0.27
    postproc out         722     1.4e-06    1.8e-07        1.5e-06   0.36
    postproc f_out       722     4.2e-07    1.8e-07        4.4e-07   0.13
    postproc stats       722     1.6e-07    9.5e-07        1.7e-07   0.14
    postproc gradient    722     5.9e-07    1.8e-07        5.0e-07   0.28
    BCE values            99     8.8e-08    6.2e-06        7.9e-08   0.01
    BCE gradient          54     2.0e-07    1.0e-07        1.5e-07   0.20
    L1 value               4     6.5e-08    6.0e-07        4.8e-08   0.11
    Adam (a) p / m / v    64 steps, per element                      0.39 / 0.80 / 0.43
    Adam (b) p / m / v    64 steps, per element                      0.97 / 0.71 / 0.44

Adam (b) p at 0.97 is one float32 ulp of p between the kernel and torch.optim.Adam, which is what 2 U |p| allows.  Adam's floors hold
the bound of one operation of the kernel beside the roundings the step is made of: it is handed (float)beta and forms 1.f - beta, each
up to U / 2 off, and v sits 1.3e-5 from Adam's at beta2 = 0.999 (24 times 3 U |v|; loss_yardstick.py, section D).
One defect came out and is fixed with this file: MEL and LOUD gave a clip with watermarked == clean a gradient (MEL 2.1e-2, LOUD
7.8e-11) where it is exactly 0.
"""
import numpy as np
import pytest
import torch

import loss_yardstick as Y
from gpu_support import awm, bits, dev, p, st  # noqa: F401
from yardstick_common import assert_within

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ A. spectral losses
def _hip_loss(awm, kind, clean, sig):
    if kind == "mel":
        return awm.MultiScaleMelLoss()(clean, sig)
    if kind == "loud":
        return awm.TFLoudnessLoss()(clean, sig)
    return awm.high_freq_penalty(sig)


def _hip_spectral(awm, dev, kind, clean, sig):
    """(value (1,), gradient of 3 * loss) of the HIP path; the no_grad run (gframes == NULL) and a second launch must give the same bits"""
    c = None if clean is None else clean.to(dev)
    s = sig.to(dev).requires_grad_()
    loss = _hip_loss(awm, kind, c, s)
    (3.0 * loss).backward()
    with torch.no_grad():
        plain = _hip_loss(awm, kind, c, s.detach())
    assert torch.equal(bits(plain.reshape(1)), bits(loss.detach().reshape(1))), f"{kind}: the no_grad value differs from the grad run's"
    s2 = sig.to(dev).requires_grad_()
    loss2 = _hip_loss(awm, kind, c, s2)
    (3.0 * loss2).backward()
    assert torch.equal(bits(loss2.detach().reshape(1)), bits(loss.detach().reshape(1))), f"{kind}: a second launch gives another value"
    assert torch.equal(bits(s2.grad), bits(s.grad)), f"{kind}: a second launch gives another gradient"
    return loss.detach().reshape(1).cpu(), s.grad.cpu()


@pytest.mark.parametrize("kind,B,T,seed", Y.SPECTRAL_CASES)
def test_spectral_loss_against_float64(awm, dev, kind, B, T, seed):
    clean, sig = Y.spectral_inputs(kind, B, T, seed)
    v64, g64 = Y.spectral_ref(kind, clean, sig)
    v32, g32 = Y.spectral_ref(kind, clean, sig, torch.float32)
    v, g = _hip_spectral(awm, dev, kind, clean, sig)
    Y.held(v, v64, v32, Y.value_floor(kind), f"{kind} ({B}, {T}) value")
    Y.held(g, g64, g32, Y.grad_floor(kind), f"{kind} ({B}, {T}) grad")


@pytest.mark.parametrize("kind,T,seed", Y.DEGENERATE_CASES)
def test_spectral_loss_zero_and_identical_clips(awm, dev, kind, T, seed):
    """an all-zero clip and one with watermarked == clean (HF: two all-zero deltas) beside an ordinary one: finite values, those rows
    of the gradient exactly 0.0 (the `> 0` guards, sg = 0), as float64 torch gives; the ordinary row under the rule"""
    clean, sig = Y.degenerate_inputs(kind, T, seed)
    v64, g64 = Y.spectral_ref(kind, clean, sig)
    v32, g32 = Y.spectral_ref(kind, clean, sig, torch.float32)
    v, g = _hip_spectral(awm, dev, kind, clean, sig)
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(g).all())
    print(f"{kind} degenerate: largest |gradient| of the zero row {float(g[0].abs().max()):.3e}, of the second row {float(g[1].abs().max()):.3e}")
    assert float(g[0].abs().max()) == 0.0, f"{kind}: the all-zero clip has a gradient"
    assert float(g[1].abs().max()) == 0.0, f"{kind}: the clip with nothing to tell apart has a gradient"
    Y.held(v, v64, v32, Y.value_floor(kind), f"{kind} degenerate value")
    Y.held(g, g64, g32, Y.grad_floor(kind), f"{kind} degenerate grad")


@pytest.mark.parametrize("kind", sorted(Y.STFT))
def test_spectral_loss_refuses_half_a_window(awm, dev, kind):
    x = torch.zeros(1, 1, Y.STFT[kind][0] // 2, device=dev)
    with pytest.raises(RuntimeError):
        _hip_loss(awm, kind, x, x)


# ------------------------------------------------------------------------------------------------------------ B. post-processing
def _pp_launch(awm, dev, x, taps, stages, g):
    """wm_postproc_fwd / _bwd through the C ABI, any T: (out, f, stats, grad) on the CPU"""
    lib = awm.lib
    B, _, T = x.shape
    xd, td, gd = x.to(dev).contiguous(), taps.to(dev).contiguous(), g.to(dev).contiguous()
    out, f, grad = torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan"))
    stats = torch.full((B, 2), float("nan"), device=dev)
    lib.wm_postproc_fwd(p(xd), p(td), taps.numel(), Y.THR, Y.MAX_RMS, Y.EPS, stages, p(f), p(out), p(stats), B, T, st())
    lib.wm_postproc_bwd(p(gd), p(f), p(stats), p(td), taps.numel(), Y.THR, Y.MAX_RMS, stages, p(grad), B, T, st())
    return out.cpu(), f.cpu(), stats.cpu(), grad.cpu()


def _pp_compare(awm, dev, T, tapset, rows, stages, B=Y.PP_B):
    taps = Y.pp_taps(tapset)
    x, g = Y.pp_input(T, tapset, rows, B), Y.pp_upstream(T, B)
    r64 = Y.pp_ref(x, taps, stages, g, tapset)
    r32 = Y.pp_ref(x, taps, stages, g, tapset, torch.float32)
    got = _pp_launch(awm, dev, x, taps, stages, g)
    what = f"postproc T {T} {tapset} {rows} stages {stages}"
    fl = Y.pp_floor(taps.numel())
    Y.held(got[0], r64[0], r32[0], fl, what + " out")
    Y.held(got[1], r64[1], r32[1], fl, what + " f_out")
    Y.held(got[2], r64[2], r32[2], Y.pp_stats_floor(taps.numel(), T), what + " stats")
    Y.held(got[3], r64[3], r32[3], fl, what + " grad")
    for b, scale in enumerate(Y.PP_ROWS[rows][:B]):
        if scale == 0.0:
            assert float(got[2][b, 1]) == 1.0, what + ": the all-zero row's gain"
            assert float(got[0][b].abs().max()) == 0.0
    return x, g, got


@pytest.mark.parametrize("tapset", Y.PP_TAPSETS)
@pytest.mark.parametrize("T", Y.PP_T)
def test_postproc_against_float64(awm, dev, T, tapset):
    for rows in Y.PP_ROWS:
        for stages in Y.PP_STAGES:
            _pp_compare(awm, dev, T, tapset, rows, stages)


@pytest.mark.parametrize("tapset", Y.PP_TAPSETS)
def test_postproc_at_the_length_limit(awm, dev, tapset):
    for stages in Y.PP_BIG_STAGES:
        _pp_compare(awm, dev, Y.PP_BIG_T, tapset, "loud", stages, B=1)


@pytest.mark.parametrize("T", [t for t in Y.PP_T + (Y.PP_BIG_T,) if t % 4 == 0])
def test_postproc_wrappers_are_the_c_abi(awm, dev, T):
    """awm.postprocess / fir_lowpass / clamp_peak / limit_rms (T % 4 == 0, the package's taps): the bits of the direct launch, forward
    and backward, so the comparison with float64 above is theirs too"""
    B = 1 if T == Y.PP_BIG_T else Y.PP_B
    stage_list = Y.PP_BIG_STAGES[:2] if T == Y.PP_BIG_T else (1, 2, 4, 7)
    fns = {1: awm.fir_lowpass, 2: awm.clamp_peak, 4: awm.limit_rms, 7: awm.postprocess}
    for rows in (("loud",) if T == Y.PP_BIG_T else tuple(Y.PP_ROWS)):
        for stages in stage_list:
            x, g, got = _pp_compare(awm, dev, T, "package", rows, stages, B)
            xd = x.to(dev).requires_grad_()
            y = fns[stages](xd)
            y.backward(g.to(dev))
            assert torch.equal(bits(y.detach().cpu()), bits(got[0])), f"T {T} {rows} stages {stages}: forward"
            assert torch.equal(bits(xd.grad.cpu()), bits(got[3])), f"T {T} {rows} stages {stages}: backward"


def test_postproc_refuses_bad_shapes(awm, dev):
    lib = awm.lib
    buf = torch.zeros(1, 1, 36004, device=dev)
    out, f, stats = torch.zeros_like(buf), torch.zeros_like(buf), torch.zeros(1, 2, device=dev)
    taps = torch.zeros(130, device=dev)

    def fwd(ntaps, T):
        lib.wm_postproc_fwd(p(buf), p(taps), ntaps, Y.THR, Y.MAX_RMS, Y.EPS, 7, p(f), p(out), p(stats), 1, T, st())

    def bwd(ntaps, T):
        lib.wm_postproc_bwd(p(buf), p(f), p(stats), p(taps), ntaps, Y.THR, Y.MAX_RMS, 7, p(out), 1, T, st())

    for call in (fwd, bwd):
        for ntaps, T in ((101, 36004), (100, 1000), (2, 1000), (129, 1000), (0, 1000)):
            with pytest.raises(RuntimeError):
                call(ntaps, T)
    with pytest.raises(RuntimeError):
        awm.postprocess(buf)
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ C. BCE and L1
@pytest.mark.parametrize("B,T", Y.BCE_BT)
@pytest.mark.parametrize("NO", Y.BCE_NO)
def test_bce_against_float64(awm, dev, NO, B, T):
    msg, x = Y.bce_messages(NO, B), Y.bce_logits(NO, B, T)
    for w in Y.BCE_WEIGHTS:
        loc64, bce64, g64 = Y.bce_ref(x, msg, w)
        loc32, bce32, g32 = Y.bce_ref(x, msg, w, torch.float32)
        xd = x.to(dev).requires_grad_()
        loc, bce = awm.detection_losses(xd, msg.to(dev))
        total = 0.0
        if w[0] is not None:
            total = total + w[0] * loc
        if w[1] is not None:
            total = total + w[1] * bce
        total.backward()
        what = f"bce NO {NO} ({B}, {T}) weights {w}"
        Y.held(loc.detach().reshape(1).cpu(), loc64, loc32, Y.BCE_VALUE_FLOOR, what + " loc")
        if NO > 1:
            Y.held(bce.detach().reshape(1).cpu(), bce64, bce32, Y.BCE_VALUE_FLOOR, what + " bce")
        else:
            assert float(bce.detach()) == 0.0
        Y.held(xd.grad.cpu(), g64, g32, Y.BCE_GRAD_FLOOR, what + " grad")
        if w[0] is None:
            assert float(xd.grad[:, :, 0].abs().max()) == 0.0 and float(xd.grad[B:].abs().max()) == 0.0
        if w[1] is None and NO > 1:
            assert float(xd.grad[:, :, 1:].abs().max()) == 0.0


@pytest.mark.parametrize("n", Y.L1_N)
def test_l1_against_float64(awm, dev, n):
    x = Y.l1_input(n)
    xd = x.to(dev).requires_grad_()
    l1 = awm.l1_to_zero(xd)
    (3.0 * l1).backward()
    Y.held(l1.detach().reshape(1).cpu(), x.double().abs().mean().reshape(1), x.abs().mean().reshape(1), Y.l1_floor(n), f"l1 n {n}")
    k = np.float32(3.0) / np.float32(n)
    want = torch.from_numpy(np.where(x.numpy() > 0, k, np.where(x.numpy() < 0, -k, np.float32(0.0))).astype(np.float32))
    assert torch.equal(bits(xd.grad.cpu()), bits(want)), f"l1 n {n}: the gradient is not +-float32(g) / float32(n)"


def test_l1_zeros(awm, dev):
    xd = Y.l1_zero_input().to(dev).requires_grad_()
    l1 = awm.l1_to_zero(xd)
    l1.backward()
    assert float(l1.detach()) == 0.0 and torch.equal(bits(xd.grad.cpu()), torch.zeros(2, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------ D. Adam
def _f64(t):
    return t.detach().cpu().double().numpy()


@pytest.mark.parametrize("fresh,step0,steps", [(True, 1, 5), (False, 1000, 3)])
@pytest.mark.parametrize("lr,betas,eps", Y.ADAM_HYPER)
@pytest.mark.parametrize("n", Y.ADAM_N)
def test_adam_step_against_float64(awm, dev, n, lr, betas, eps, fresh, step0, steps):
    lib = awm.lib
    p0, m0, v0 = Y.adam_state(n, 800 + n, fresh)
    pd, md, vd = p0.to(dev), m0.to(dev), v0.to(dev)
    P = torch.nn.Parameter(p0.clone())                                   # (b): torch.optim.Adam in float32 over the same sequence
    opt = torch.optim.Adam([P], lr=lr, betas=betas, eps=eps)
    opt.state[P] = {"step": torch.tensor(float(step0 - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    seq = None
    for k in range(steps):
        step = step0 + k
        g = Y.adam_grad(n, 810 + n + k)
        before = (pd.cpu(), md.cpu(), vd.cpu())
        r64 = Y.adam_ref(before[0], g, before[1], before[2], lr, betas, eps, step)
        t32 = Y.adam_torch_step(before[0], g, before[1], before[2], lr, betas, eps, step)
        floors = Y.adam_floors(r64, g, before[1], before[2], lr, betas, eps, step)
        gd = g.to(dev)
        lib.wm_adam_step(p(pd), p(gd), p(md), p(vd), n, lr, betas[0], betas[1], eps, step, st())
        what = f"adam n {n} lr {lr} step {step}"
        for name, got, ref, t, ops, beta in zip("pmv", (pd, md, vd), r64[:3], t32, *floors):
            assert_within(_f64(got), ref, Y.adam_bound(t, ref, ops + beta), f"{what} {name} (a)")
        if fresh and n >= 255:
            for i in (5, n - 3):                                          # g = 0, m = v = 0: nothing moves
                assert torch.equal(bits(pd[i:i + 1].cpu()), bits(p0[i:i + 1])) and float(md[i]) == 0.0 and float(vd[i]) == 0.0
        P.grad = g.clone()
        opt.step()
        s = opt.state[P]
        seq = Y.adam_seq_bounds(seq, floors, r64, g, before[1], lr, betas, eps, step)
        for name, got, ref, bound in zip("pmv", (pd, md, vd), (P.detach(), s["exp_avg"], s["exp_avg_sq"]), seq):
            assert_within(_f64(got), _f64(ref), bound, f"{what} {name} (b)")


def test_adam_error_returns(awm, dev):
    lib = awm.lib
    t = [torch.ones(4, device=dev) for _ in range(4)]
    lib.wm_adam_step(p(t[0]), p(t[1]), p(t[2]), p(t[3]), 0, 1e-3, 0.9, 0.999, 1e-8, 1, st())
    torch.cuda.synchronize()
    assert all(torch.equal(a.cpu(), torch.ones(4)) for a in t)
    for step, n in ((0, 4), (-1, 4), (1, -1)):
        with pytest.raises(RuntimeError):
            lib.wm_adam_step(p(t[0]), p(t[1]), p(t[2]), p(t[3]), n, 1e-3, 0.9, 0.999, 1e-8, step, st())
    torch.cuda.synchronize()
    assert all(torch.equal(a.cpu(), torch.ones(4)) for a in t)
