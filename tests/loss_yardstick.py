"""The float64 yardsticks of the oldest kernels on the training step -- csrc/stft_loss.hip, csrc/postproc.hip and the BCE / L1 / Adam
kernels of csrc/losses.hip -- with the case tables, the input builders and the tolerance rule, for tests/test_gpu_loss_stack.py (GPU)
and tests/test_loss_yardstick_cpu.py (the input conditions, without a GPU).  `import loss_yardstick as Y`.

References.  The spectral losses and the post-processing are the oracle's own functions (oracle.wm_oracle.mel_loss, loudness_loss,
high_freq_penalty, fir_lowpass, clamp_peak, limit_rms) called with float64 tensors and differentiated by autograd: they follow their
input's dtype, and the float32 filterbank and FIR taps are cast up, so they keep the values the kernel is given.  FIR cases with other
taps take F.conv1d in float64.  BCE, L1 and Adam are a few lines of float64 torch / numpy each.

The tolerance rule (`bar`, `held`).  For every compared tensor e32 is the distance -- max |a - ref| / max |ref|, gpu_support.rel_err's
measure -- of the float32 reference (the same functions run in float32 on the CPU; torch.optim.Adam for Adam) to the float64 one, and
the kernel is held to max(8 * e32, floor).  8: the kernels sum in another order than the CPU and use a plain radix-2 FFT with float32
twiddles where torch uses pocketfft; a real defect (a dropped reflection term, a wrong frame, a shifted tap, a wrong bias correction)
is three or more orders of magnitude larger.  The floors are derived, each next to its case table, from U = 2^-24 and gamma().

Threshold flips.  An input that puts a reference value within float32 round-off of a threshold (the LOUD mask at 0.01, sign(d) of the
log-mel difference, the clamp at +-thr, the RMS cap at gain 1) moves a gradient by percent, not by 1e-6.  Every table here is chosen so
that no such value exists, and tests/test_loss_yardstick_cpu.py asserts the margins on the float64 reference alone: a changed seed or
torch version fails there, loudly, instead of flaking on the GPU."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import wm_oracle as O
from yardstick_common import U, gamma

TINY = 2.0 ** -149          # the spacing of float32's denormals


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def rel_err(a, ref):
    """gpu_support.rel_err, restated so that the CPU file needs nothing from gpu_support"""
    a, ref = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-30))


def bar(ref32, ref64, floor):
    """max(8 * e32, floor): the rule above"""
    return max(8.0 * rel_err(ref32, ref64), floor)


def held(a, ref64, ref32, floor, what):
    """the kernel's `a` against the float64 reference under the rule; prints the measured distance as gpu_support.check does"""
    assert tuple(a.shape) == tuple(ref64.shape), f"{what}: shape {tuple(a.shape)} vs {tuple(ref64.shape)}"
    assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32, what
    e, b = rel_err(a, ref64), bar(ref32, ref64, floor)
    print(f"{what}: rel err {e:.3e}, bar {b:.3e} (e32 {rel_err(ref32, ref64):.3e}, floor {floor:.3e}), ratio {e / b:.3f}")
    assert math.isfinite(e) and e <= b, f"{what}: rel err {e:.3e} > {b:.3e}"


# ------------------------------------------------------------------------------------------------------------ A. spectral losses
# kind -> (n_fft, hop).  Floors: a radix-2 transform of n_fft points is log2(n_fft) stages of one complex multiply-add each, so a
# spectrum value carries about log2(n_fft) U of its largest neighbour; the loss value passes through one transform and the reduction
# (floor 2 log2(n_fft) U relative), a gradient through two transforms (floor 4 log2(n_fft) U of its largest element).
STFT = {"mel": (1024, 256), "loud": (2048, 512), "hf": (512, 128)}
LOUD_THRESH = 0.01
LOUD_MARGIN = 2e-6           # every | |S_clean| - 0.01 | at least this: about 300 times the float32 round-off of the spectrum (7e-9)
MEL_MARGIN = 1e-4            # every |log-mel(clean) - log-mel(wm)| at least this, so that sign(d) cannot flip

# (B, T, seed).  MEL: clean = synthetic_clips(B, seed, T), wm = clean + randn(seed + 1) * 0.1 (at the workload's 0.004 the margin does
# not hold).  T: 513 = n_fft/2 + 1, both reflections overlap; 768 a multiple of the hop; 1279, 2048, 4100.  Seeds start at 50 + T and
# are the first that meet MEL_MARGIN.
MEL_CASES = [(1, 513, 563), (3, 768, 818), (2, 1279, 1329), (2, 2048, 2098), (1, 4100, 4151)]
# LOUD: clean = synthetic_clips(B, seed, T) * 0.005, wm = clean + randn(seed + 1000) * 1e-4: the share of bins above the mask
# threshold lies in [0.2, 0.8] (0.51 to 0.57 here) and no bin is within LOUD_MARGIN of it.
LOUD_CASES = [(1, 1025, 0), (3, 1536, 8), (2, 2047, 2), (2, 2048, 0), (1, 4099, 0)]
# HF: delta = randn(70 + T) * 0.004, the workload's scale; no threshold but |S| > 0.  F = 1 + T // 128 frames, two to an FFT: F odd
# (257 -> 3, 1024 and 1100 -> 9) runs the lone last frame; 640 is a multiple of the hop.
HF_CASES = [(1, 257, 327), (3, 384, 454), (2, 640, 710), (2, 700, 770), (1, 1024, 1094), (3, 1100, 1170)]
SPECTRAL_CASES = [("mel",) + c for c in MEL_CASES] + [("loud",) + c for c in LOUD_CASES] + [("hf",) + c for c in HF_CASES]


def value_floor(kind):
    return 2.0 * math.log2(STFT[kind][0]) * U


def grad_floor(kind):
    return 4.0 * math.log2(STFT[kind][0]) * U


def spectral_inputs(kind, B, T, seed):
    """(clean, signal) float32 (B, 1, T); for HF clean is None and signal is the delta"""
    if kind == "mel":
        clean = O.synthetic_clips(B, seed=seed, T=T)
        return clean, clean + rnd(B, 1, T, seed=seed + 1, scale=0.1)
    if kind == "loud":
        clean = O.synthetic_clips(B, seed=seed, T=T) * 0.005
        return clean, clean + rnd(B, 1, T, seed=seed + 1000, scale=1e-4)
    return None, rnd(B, 1, T, seed=seed, scale=0.004)


def degenerate_inputs(kind, T, seed):
    """three clips: all zeros; watermarked == clean exactly; an ordinary one.  The first two rows' gradient is exactly 0.
    HF: an all-zero delta, a second all-zero row, an ordinary one."""
    clean, sig = spectral_inputs(kind, 3, T, seed)
    sig = sig.clone()
    if kind == "hf":
        sig[:2] = 0.0
        return None, sig
    clean = clean.clone()
    clean[0] = 0.0
    sig[0] = 0.0
    sig[1] = clean[1]
    return clean, sig


DEGENERATE_CASES = [("mel", 1279, 1329), ("loud", 2047, 1), ("hf", 700, 770)]


def spectral_loss(kind, clean, sig):
    if kind == "mel":
        return O.mel_loss(clean, sig)
    if kind == "loud":
        return O.loudness_loss(clean, sig)
    return O.high_freq_penalty(sig)


def spectral_ref(kind, clean, sig, dtype=torch.float64):
    """(loss, gradient of 3 * loss w.r.t. the signal) in `dtype`"""
    c = None if clean is None else clean.to(dtype)
    s = sig.to(dtype).clone().requires_grad_()
    loss = spectral_loss(kind, c, s)
    (3.0 * loss).backward()
    return loss.detach().reshape(1), s.grad


def loud_margins(clean):
    """(share of bins with |S_clean| > 0.01, smallest | |S_clean| - 0.01 |) on the float64 spectrum"""
    mag = O._stft(clean.double().squeeze(1), 2048, 512).abs()
    return float((mag > LOUD_THRESH).double().mean()), float((mag - LOUD_THRESH).abs().min())


def mel_margin(clean, sig):
    """smallest |log-mel(clean) - log-mel(wm)| in float64"""
    d = torch.log(O.mel_spectrogram(clean.double()) + 1e-5) - torch.log(O.mel_spectrogram(sig.double()) + 1e-5)
    return float(d.abs().min())


# ------------------------------------------------------------------------------------------------------------ B. post-processing
# Floor: one FIR output is ntaps fused multiply-adds, gamma(ntaps + 2) of sum |k||x| with the two roundings after it (clamp is
# exact, the gain one multiply), stated of the tensor's largest element as the rule measures.  The statistics (rms, gain) add the sum
# of T squares -- T / 256 serial terms per thread, 8 levels of the block sum, the division, the root and the quotient:
# gamma(ceil(T / 256) + 12) -- to the error the summed values carry.
THR, MAX_RMS, EPS = 0.02, 0.005, 1e-8
CLAMP_MARGIN = 1e-4          # every float64 FIR output at least CLAMP_MARGIN * thr from +-thr
GAIN_MARGIN = 1e-3           # every row |max_rms / cur - 1| at least this
PP_B = 3
PP_T = (1, 37, 100, 255, 256, 257, 1000, 4099)
PP_STAGES = (1, 2, 4, 3, 5, 6, 7)
PP_TAPSETS = ("package", "lowpass101", "random127", "single")
PP_ROWS = {"loud": (0.03, 0.03, 0.03), "quiet": (0.001, 0.001, 0.001), "mixed": (0.03, 0.001, 0.0)}
PP_BIG_T, PP_BIG_STAGES = 36000, (1, 4, 5)      # the documented limit (145 KB of LDS), B = 1, the stages that have no per-sample threshold
# (T, tap set) -> seed of the input noise where 40 + T does not meet the margins for all stages and rows (first that does)
PP_SEEDS = {(1000, "package"): 1042, (1000, "lowpass101"): 1043, (1000, "random127"): 1042, (1000, "single"): 1043,
            (4099, "single"): 4153}


def pp_floor(ntaps):
    return gamma(ntaps + 2)


def pp_stats_floor(ntaps, T):
    return gamma(ntaps + 2) + gamma((T + 255) // 256 + 12)


@functools.lru_cache(maxsize=None)
def pp_taps(name):
    """float32 taps: the package's 101-tap all-pass; a real 101-tap low-pass at 4 kHz (Hamming-windowed sinc designed in float64,
    rounded once); 127 random asymmetric taps normalised to sum 1 (a flipped or shifted tap index shows); one tap"""
    if name == "package":
        return O.fir_kernel()
    if name == "lowpass101":
        n = np.arange(101, dtype=np.float64) - 50.0
        fc = 4000.0 / O.SAMPLE_RATE                                   # cycles per sample
        k = 2.0 * fc * np.sinc(2.0 * fc * n) * (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(101) / 100.0))
        return torch.from_numpy((k / k.sum()).astype(np.float32))
    if name == "random127":
        k = torch.randn(127, generator=torch.Generator().manual_seed(127), dtype=torch.float64)
        assert abs(float(k.sum())) >= 1.0                             # the normalisation must not blow the taps up
        return (k / k.sum()).float()
    assert name == "single"
    return torch.tensor([0.75])


def pp_seed(T, tapset):
    return PP_SEEDS.get((T, tapset), 40 + T)


def pp_input(T, tapset, rows, B=PP_B):
    """(B, 1, T) float32: one draw of unit noise per (T, tap set), scaled per row"""
    scale = torch.tensor(PP_ROWS[rows][:B]).view(B, 1, 1)
    return rnd(B, 1, T, seed=pp_seed(T, tapset)) * scale


def pp_upstream(T, B=PP_B):
    return rnd(B, 1, T, seed=9000 + T)


def pp_ref(x, taps, stages, g=None, tapset=None, dtype=torch.float64):
    """(out, f, stats (B, 2) = (rms, gain), gradient w.r.t. x for the upstream g or None) in `dtype`.  f is the FIR output (the input
    where the FIR stage is off), what the kernel saves for its backward pass."""
    x = x.to(dtype).clone().requires_grad_(g is not None)
    f = x
    if stages & 1:
        if tapset == "package":
            f = O.fir_lowpass(x)
        else:
            f = F.conv1d(x, taps.to(dtype).view(1, 1, -1), padding=(taps.numel() - 1) // 2)
    y = O.clamp_peak(f, THR) if stages & 2 else f
    B = x.shape[0]
    stats = torch.stack([torch.zeros(B, dtype=dtype), torch.ones(B, dtype=dtype)], dim=1)
    if stages & 4:
        cur = torch.sqrt((y.detach() ** 2).mean(dim=[1, 2]) + EPS)
        stats = torch.stack([cur, torch.clamp(MAX_RMS / cur, max=1.0)], dim=1)
        y = O.limit_rms(y, MAX_RMS, EPS)
    grad = None
    if g is not None:
        y.backward(g.to(dtype))
        grad = x.grad
    return y.detach(), f.detach(), stats, grad


def pp_margins(x, taps, stages, tapset=None):
    """(smallest | |f| - thr | / thr where the clamp runs else inf, smallest |max_rms / cur - 1| where the cap runs else inf)"""
    _, f, stats, _ = pp_ref(x, taps, stages, None, tapset)
    cm = float(((f.abs() - THR).abs() / THR).min()) if stages & 2 else math.inf
    gm = float((MAX_RMS / stats[:, 0] - 1.0).abs().min()) if stages & 4 else math.inf
    return cm, gm


def pp_margins_ok(T, tapset, stages_list=PP_STAGES, B=PP_B, rows_list=tuple(PP_ROWS)):
    for rows in rows_list:
        for stages in stages_list:
            cm, gm = pp_margins(pp_input(T, tapset, rows, B), pp_taps(tapset), stages, tapset)
            if cm < CLAMP_MARGIN or gm < GAIN_MARGIN:
                return False
    return True


# ------------------------------------------------------------------------------------------------------------ C. BCE and L1
# BCE value floor: wm_common.hpp documents softplus_neg_abs as log(1 + u) with the rounding of 1 + u costing up to 6e-6 of the term;
# the loss is at least the mean of those terms, so 6e-6 + 4 U relative (the sums are float64).  BCE gradient floor: 1e-7 of the
# largest element, from the 3e-8 absolute error that wm_common.hpp documents for the reciprocal sigmoid, plus the roundings of
# k * (sg - y).  L1 value floor: at most ceil(n / 65536) serial float32 adds per thread, 8 levels of the block sum and the final
# rounding, gamma(ceil(n / 65536) + 9); the L1 gradient is exact.
BCE_NO = (1, 2, 3, 17, 33, 64)
BCE_BT = ((1, 5), (2, 241), (3, 1000))
BCE_WEIGHTS = ((10.0, 1.0), (1.0, None), (None, 1.0))        # None: that loss is not used, the backward's `None` upstream path
BCE_VALUE_FLOOR = 6e-6 + 4 * U
BCE_GRAD_FLOOR = 1e-7
PLANTED = (30.0, -30.0, 100.0, -100.0, 0.0)
L1_N = (1, 255, 257, 65539)


def l1_floor(n):
    return gamma((n + 65535) // 65536 + 9)


def bce_messages(NO, B):
    """B int64 messages of NO - 1 bits: all ones first, then (NO = 64) only bit 62 / (else) zero, then the other of the two"""
    bits = NO - 1
    ones = (1 << bits) - 1
    pool = [ones, 1 << 62, 0] if NO == 64 else [ones, 0, ones & 0x5A5A5A5A5A5A5A5A]
    return torch.tensor(pool[:B], dtype=torch.int64)


def bce_logits(NO, B, T):
    """(2B, T, NO) float32: randn * 3 with +-30, +-100 and 0.0 planted at t = 0 ... 4 of the first clip of both halves, in the
    detection channel and in the first and last bit channel"""
    x = rnd(2 * B, T, NO, seed=600 + 7 * NO + T, scale=3.0)
    for r in (0, B):
        for o in {0, min(1, NO - 1), NO - 1}:
            x[r, :5, o] = torch.tensor(PLANTED)
    return x


def bce_targets(msg, NO, B, T, dtype):
    tgt = torch.cat([torch.ones(B, T, dtype=dtype), torch.zeros(B, T, dtype=dtype)])
    bits = torch.tensor([[(int(m) >> i) & 1 for i in range(NO - 1)] for m in msg], dtype=dtype).reshape(B, 1, NO - 1).expand(-1, T, -1)
    return tgt, bits


def _stable_bce(x, y):
    return (x.clamp(min=0) - x * y + torch.log1p(torch.exp(-x.abs()))).mean()


def bce_ref(logits, msg, weights, dtype=torch.float64):
    """(loc (1,), bce (1,) or None at NO = 1, gradient of w_loc * loc + w_bce * bce w.r.t. the logits) in `dtype`: the stable form in
    float64, F.binary_cross_entropy_with_logits as the oracle calls it in float32"""
    B, (_, T, NO) = msg.shape[0], logits.shape
    x = logits.to(dtype).clone().requires_grad_()
    tgt, bits = bce_targets(msg, NO, B, T, dtype)
    if dtype == torch.float64:
        # autograd of the stable form takes a subgradient of max and |.| at the planted x = 0.0: the derivative is written out
        with torch.no_grad():
            loc = _stable_bce(x[:, :, 0], tgt)
            bce = _stable_bce(x[:B, :, 1:], bits) if NO > 1 else None
            grad = torch.zeros_like(x)
            if weights[0] is not None:
                grad[:, :, 0] = weights[0] * (torch.sigmoid(x[:, :, 0]) - tgt) / (2 * B * T)
            if weights[1] is not None and NO > 1:
                grad[:B, :, 1:] = weights[1] * (torch.sigmoid(x[:B, :, 1:]) - bits) / (B * T * (NO - 1))
        return loc.reshape(1), None if bce is None else bce.reshape(1), grad
    fn = F.binary_cross_entropy_with_logits
    loc = fn(x[:, :, 0], tgt)
    bce = fn(x[:B, :, 1:], bits) if NO > 1 else None
    total = x.sum() * 0.0
    if weights[0] is not None:
        total = total + weights[0] * loc
    if weights[1] is not None and bce is not None:
        total = total + weights[1] * bce
    total.backward()
    return loc.detach().reshape(1), None if bce is None else bce.detach().reshape(1), x.grad


def l1_input(n):
    x = rnd(n, seed=610 + n, scale=0.01)
    if n >= 255:
        x[3], x[n - 2] = 0.0, -0.0
    return x


def l1_zero_input():
    return torch.tensor([0.0, -0.0])


# ------------------------------------------------------------------------------------------------------------ D. Adam
# Comparison (a), one step from the kernel's own float32 state, per element: p' = p - update is one rounding of |p'| <= U |p| after
# an update that carries the roundings of m (2), v (3, halved by the root), the quotient by sqrt(bc2), the sum with eps, m / denom
# and the product with the step size -- 8 U |update| --; m is one product and one fused multiply-add, 2 U |m|; v two products and
# one, 3 U |v|; plus the spacing of float32's denormals.
# With these alone the kernel misses v by up to 24 times (m: within, p: within), by the round-off of one operation: wm_adam_step hands
# beta over as (float)beta and the kernel forms 1.f - beta.  For beta in [0.5, 1) |(float)beta - beta| <= U / 2 and the subtraction is
# exact, so the kernel's beta and its 1 - beta are each up to U / 2 off -- of 1 - beta2 = 0.001 that is 3e-5 (measured: 1.3e-5 at
# 0.999, 1.f - 0.999f = 0.00099998713).  That operation's bound is stated as part of the floor (adam_floors' second triple):
# (U / 2) (|g| + |m|) for m, (U / 2) (g^2 + v) for v, and what those move the update by for p, to first order (the root of v by
# min(D_v / (2 sqrt v), sqrt D_v), which holds for any v >= 0; adam_update_shift).  Rounding 1 - beta once from the doubles, as the
# bias corrections are, brings v to 0.3 of 3 U |v|, but it moves every v by that 1.3e-5 and with it the trained weights of every run
# beyond rounding; it is not made here.
# Comparison (b), against torch.optim.Adam in float32 over the same sequence: twice (a)'s roundings, the beta term once (torch
# rounds 1 - beta from the double), plus two terms that are round-off of the comparison itself and not of the kernel (measured:
# without them (b) is missed in m by up to 36 times, from step 2 on, and then in p by 1.07 times).
# (1) torch forms m as lerp(m, g, 1 - beta1) = m + (1 - beta1) (g - m): the difference and the product are rounded before the sum, an
# error of 2 U (1 - beta1) |g - m| that |m'| does not bound where g and m cancel.  (2) From the second step on the two float32
# sequences start from states that already differ, and a step carries that difference on: beta1 D_m, beta2 D_v, and through the update
# into p (adam_update_shift again).  adam_seq_bounds states both.
ADAM_N = (1, 255, 257, 100003)
ADAM_HYPER = ((1e-3, (0.9, 0.999), 1e-8), (3e-4, (0.8, 0.99), 1e-6))
ADAM_SCALES = (1e-12, 1e-9, 1e-6, 1e-3, 1.0, 1e3)


def adam_grad(n, seed):
    """randn times per-element scales from 1e-12 to 1e3; where n allows, exact zeros at 5 and n - 3 and 1e-25 (g^2 underflows, the
    denominator is eps) at 7 and n - 5 in every step's gradient"""
    g = rnd(n, seed=seed) * torch.tensor(ADAM_SCALES)[torch.arange(n) % len(ADAM_SCALES)]
    if n >= 255:
        g[5] = g[n - 3] = 0.0
        g[7], g[n - 5] = 1e-25, -1e-25
    return g


def adam_state(n, seed, fresh):
    """(p, m, v): zero moments, or random m and positive v"""
    p = rnd(n, seed=seed)
    if fresh:
        return p, torch.zeros(n), torch.zeros(n)
    return p, rnd(n, seed=seed + 1, scale=0.1), rnd(n, seed=seed + 2, scale=0.1) ** 2 + 1e-12


def adam_ref(p, g, m, v, lr, betas, eps, step):
    """one float64 Adam step from float32 (or any) state: (p, m, v, update) as float64 numpy"""
    p, g, m, v = (np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64) for t in (p, g, m, v))
    b1, b2 = betas
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    upd = (lr / (1.0 - b1 ** step)) * m / (np.sqrt(v) / math.sqrt(1.0 - b2 ** step) + eps)
    return p - upd, m, v, upd


def adam_update_shift(Dm, Dv, ref, lr, betas, eps, step):
    """how far errors D_m, D_v in the moments move the update, to first order; ref = adam_ref's (p, m, v, update)"""
    bc2s = math.sqrt(1.0 - betas[1] ** step)
    root = np.sqrt(ref[2])
    denom = root / bc2s + eps
    d_root = np.minimum(Dv / (2.0 * np.maximum(root, 1e-300)), np.sqrt(Dv))
    return (lr / (1.0 - betas[0] ** step)) / denom * Dm + np.abs(ref[3]) / denom * d_root / bc2s


def adam_floors(ref, g, m_before, v_before, lr, betas, eps, step):
    """per-element floors of comparison (a) for ref = adam_ref's (p, m, v, update), as two triples (p, m, v): the roundings of the
    step's operations, and the bound of (float)beta and 1.f - (float)beta.  The floor is their sum."""
    assert all(0.5 <= b < 1.0 for b in betas)                  # where the spacing of float32 is 2 U
    g, m0, v0 = (np.asarray(t.detach().cpu().numpy(), dtype=np.float64) for t in (g, m_before, v_before))
    p, m, v, upd = ref
    ops = (U * np.abs(p) + 8 * U * np.abs(upd) + TINY, 2 * U * np.abs(m) + TINY, 3 * U * np.abs(v) + TINY)
    bm, bv = 0.5 * U * (np.abs(g) + np.abs(m0)), 0.5 * U * (g * g + v0)
    return ops, (adam_update_shift(bm, bv, ref, lr, betas, eps, step), bm, bv)


def adam_torch_step(p, g, m, v, lr, betas, eps, step):
    """torch.optim.Adam's own float32 step number `step` from the given state: (p, m, v)"""
    P = torch.nn.Parameter(p.detach().cpu().clone())
    opt = torch.optim.Adam([P], lr=lr, betas=betas, eps=eps)
    opt.state[P] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.detach().cpu().clone(), "exp_avg_sq": v.detach().cpu().clone()}
    P.grad = g.detach().cpu().clone()
    opt.step()
    return P.detach(), opt.state[P]["exp_avg"], opt.state[P]["exp_avg_sq"]


def adam_bound(ref32, ref64, floor):
    """per element max(8 * e32 * max |ref|, floor): the rule, with the floor per element"""
    ref32 = np.asarray(ref32.detach().cpu().numpy(), dtype=np.float64)
    return np.maximum(8.0 * np.abs(ref32 - ref64).max(), floor)


def adam_seq_bounds(prev, floors, ref, g, m_before, lr, betas, eps, step):
    """per-element bounds (D_p, D_m, D_v) of comparison (b) after step `step`: `prev` the bounds before it (None at the first step, where
    both sequences hold the same state), `floors` = adam_floors' two triples and `ref` = adam_ref's (p, m, v, update) for this step"""
    b1, b2 = betas
    ops, beta = floors
    Dp, Dm, Dv = prev if prev is not None else (0.0, 0.0, 0.0)
    g, m_before = (np.asarray(t.detach().cpu().numpy(), dtype=np.float64) for t in (g, m_before))
    Dm = b1 * Dm + 2.0 * ops[1] + beta[1] + 2.0 * U * (1.0 - b1) * np.abs(g - m_before)
    Dv = b2 * Dv + 2.0 * ops[2] + beta[2]
    return Dp + 2.0 * ops[0] + adam_update_shift(Dm, Dv, ref, lr, betas, eps, step), Dm, Dv
