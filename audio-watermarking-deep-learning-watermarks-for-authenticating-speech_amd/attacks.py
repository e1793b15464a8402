"""Channel distortions between s + delta and the Detector, and the loop that tells how detection moves under them.

The reference README's "Robustness Testing" section promises a watermark that survives compression, resampling, volume changes and
additive noise; it ships no code for the last two.  Here they are modules on (B, 1, T), (C, N) or (N,) that go wherever codec.PcmCodec
goes -- the `codec=` argument of forward_losses / train_step / eval_forward / evaluate_batches takes any of them, and chains are plain
torch.nn.Sequential(Distortion(...), PcmCodec(...)), which therefore already works as `codec=`:

  Distortion   per-clip gain and white Gaussian noise at a set SNR: one wm_distort call (ops.DistortFn), differentiable
  Lowpass      the biquad low-pass alone (no clamp, no 16-bit grid): ops.biquad, its backward the same launch with reverse=True
  Resampled    down to another rate and back (8 kHz telephony, say), every row by itself: two wm_resample_rows launches
               (ops.ResampleRowsFn), the backward of each the same launch with the transposed table
  evaluate_robustness   watermarked / clean probability, bit accuracy and delta RMS per attack, pooled as evaluate_batches pools them

The noise is counter-based (Philox4x32-10 -> Box-Muller), so nothing is stored for the backward pass, a run is reproducible from `seed`,
and philox4x32_10 / normal_noise below restate on the host exactly the numbers the kernel draws."""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch

from . import ops
from .codec import SAMPLE_RATE, _time_rows
from .losses import postprocess

NOISE_GRAD_MODES = ("through", "detached")
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_PARAM_Q = 0xFFFFFFFFFFFFFFFF        # the counter words (q low, q high) of a row's parameters: no sample has them (n <= 2^34)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11).  counter: four uint32 values or arrays that
    broadcast together, key: two uint32 values.  Returns a uint32 array of shape (4, ...): the four output words."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for v in counter]
    if len(c) != 4 or len(key) != 2:
        raise ValueError("philox4x32_10: a counter of four words and a key of two")
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(k) & 0xFFFFFFFF for k in key)
    lo = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]                     # 32 x 32 bits: exact in 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c).astype(np.uint32)


def _unit(o):
    """u = ((o >> 9) + 0.5) * 2^-23: 24 bits, exact in float32 (and float64), never 0 or 1"""
    return ((o >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def _key(seed):
    seed = int(seed) & (2 ** 64 - 1)
    return seed & 0xFFFFFFFF, seed >> 32


def normal_noise(seed, draw, row, n):
    """z(seed, draw, row, t) for t < n as a float64 array: counter (q low, q high, row, draw) with q = t >> 2, key (seed low, seed high);
    words (o0, o1) give sqrt(-2 ln u(o0)) * (cos, sin)(2 pi u(o1)) for samples 4q and 4q+1, (o2, o3) the same for 4q+2 and 4q+3."""
    n = int(n)
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    o = philox4x32_10((q, q >> np.uint64(32), int(row), int(draw)), _key(seed))
    z = np.empty((len(q), 4), dtype=np.float64)
    for p in (0, 1):
        rad, th = np.sqrt(-2.0 * np.log(_unit(o[2 * p]))), 2.0 * math.pi * _unit(o[2 * p + 1])
        z[:, 2 * p], z[:, 2 * p + 1] = rad * np.cos(th), rad * np.sin(th)
    return z.reshape(-1)[:n]


def row_parameters(seed, draw, rows, bounds):
    """(gain_db, snr_db, noisy) of rows `rows` (an int array of row0 + r), as the kernel draws them: float32 arrays and a bool array"""
    gain_lo, gain_hi, snr_lo, snr_hi, p_noise = (np.float32(v) for v in bounds)
    o = philox4x32_10((_PARAM_Q & 0xFFFFFFFF, _PARAM_Q >> 32, np.asarray(rows, dtype=np.uint64), int(draw)), _key(seed))

    def affine(lo, hi, u):                                                        # fmaf(hi - lo, u, lo): the product is exact in float64
        return (np.float64(hi - lo) * u + np.float64(lo)).astype(np.float32)
    return affine(gain_lo, gain_hi, _unit(o[0])), affine(snr_lo, snr_hi, _unit(o[1])), _unit(o[2]) < np.float64(p_noise)


def _pair(v, name):
    pair = tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    if len(pair) != 2 or not all(isinstance(b, (int, float)) and not isinstance(b, bool) and math.isfinite(b) for b in pair):
        raise ValueError(f"{name}: expected a finite number or a (low, high) pair of them, got {v!r}")
    lo, hi = pair
    if lo > hi:
        raise ValueError(f"{name}: low {lo} is above high {hi}")
    return float(lo), float(hi)


class Distortion(torch.nn.Module):
    """y = g x + s z for every row (clip or channel) of x, (B, 1, T), (C, N) or (N,):  g = 10^(gain_db / 20) with gain_db drawn uniformly
    from the pair `gain_db` per row, z white Gaussian noise at an SNR of snr_db (drawn from the pair `snr_db`) against g x, added to a row with
    probability p_noise.  A number in place of a pair fixes the value; snr_db=None: no noise.  No clamping: chain a PcmCodec for saturation.
    Every forward uses the next `draw` (fresh noise and parameters; a run is reproducible from `seed`); reset(draw) rewinds.  `row0`
    (forward's argument) numbers the first row, so that a batch cut into pieces draws what the whole batch would.  `last_stat`: the
    (rows, 4) tensor {g, s, mean square of x, snr_db or inf} of the last call.
    noise_grad "through": the noise level s, which follows the row's own RMS, takes part in the gradient | "detached": s is a constant, the
    gradient is g * dy.  CUDA tensors run the kernel; CPU tensors a numpy restatement of the same definition (forward only)."""

    def __init__(self, gain_db=(-6, 6), snr_db=(20, 40), p_noise=1.0, seed=0, noise_grad="through"):
        super().__init__()
        if noise_grad not in NOISE_GRAD_MODES:
            raise ValueError(f"noise_grad must be one of {NOISE_GRAD_MODES}, got {noise_grad!r}")
        if isinstance(p_noise, bool) or not isinstance(p_noise, (int, float)) or not 0.0 <= p_noise <= 1.0:
            raise ValueError(f"p_noise: expected a probability in [0, 1], got {p_noise!r}")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed: expected an int, got {seed!r}")
        self.gain_db = _pair(gain_db, "gain_db")
        self.snr_db = None if snr_db is None else _pair(snr_db, "snr_db")
        self.p_noise = float(p_noise) if snr_db is not None else 0.0
        self.seed, self.noise_grad = seed, noise_grad
        self.last_stat = None
        self.reset()

    def reset(self, draw=0):
        if isinstance(draw, bool) or not isinstance(draw, int) or not 0 <= draw < 2 ** 32:
            raise ValueError(f"draw: expected an int in [0, 2^32), got {draw!r}")
        self.draw = draw
        return self

    @property
    def bounds(self):
        return (*self.gain_db, *(self.snr_db or (0.0, 0.0)), self.p_noise)

    def forward(self, x, row0=0):
        x = _time_rows(x, "x")
        rows = x.numel() // x.shape[-1]
        if isinstance(row0, bool) or not isinstance(row0, int) or not 0 <= row0 <= 2 ** 32 - rows:
            raise ValueError(f"row0: expected an int with 0 <= row0 and row0 + rows <= 2^32, got {row0!r}")
        draw, self.draw = self.draw, (self.draw + 1) % 2 ** 32
        if x.is_cuda:
            y, stat = ops.DistortFn.apply(x.to(torch.float32), self.bounds, self.seed, draw, row0, self.noise_grad == "through")
        else:
            y, stat = self._host(x.detach().to(torch.float32), draw, row0)
        self.last_stat = stat
        return y

    def _host(self, x, draw, row0):
        n = x.shape[-1]
        x2 = x.reshape(-1, n)
        gain_db, snr_db, noisy = row_parameters(self.seed, draw, row0 + np.arange(x2.shape[0]), self.bounds)
        ms = x2.double().pow(2).mean(dim=1).numpy()
        g = np.float32(10.0) ** (gain_db.astype(np.float64) / 20.0)
        s = np.where(noisy, np.abs(g) * np.sqrt(ms) * 10.0 ** (-snr_db.astype(np.float64) / 20.0), 0.0)
        g32, s32 = g.astype(np.float32), s.astype(np.float32)
        y = x2 * torch.from_numpy(g32)[:, None]                                   # g = 1 hands x on bit for bit
        for r in np.nonzero(s32)[0]:
            z = torch.from_numpy(normal_noise(self.seed, draw, row0 + int(r), n))
            y[r] = (float(g32[r]) * x2[r].double() + float(s32[r]) * z).float()
        stat = np.stack([g32, s32, ms.astype(np.float32), np.where(noisy, snr_db, np.float32(np.inf))], axis=1)
        return y.reshape(x.shape), torch.from_numpy(stat.astype(np.float32))

    def extra_repr(self):
        return (f"gain_db={self.gain_db}, snr_db={self.snr_db}, p_noise={self.p_noise}, seed={self.seed}, "
                f"noise_grad={self.noise_grad!r}")


class _LowpassFn(torch.autograd.Function):
    """y = F x, the zero-state biquad section; dx = F^T dy = flip(F(flip(dy))), the kernel's reverse launch"""

    @staticmethod
    def forward(ctx, x, coeffs):
        ctx.coeffs = coeffs
        return ops.biquad(x, coeffs, clamp=False, mode="float")

    @staticmethod
    def backward(ctx, g):
        return ops.biquad(g.contiguous(), ctx.coeffs, clamp=False, mode="float", reverse=True), None


class Lowpass(torch.nn.Module):
    """The RBJ biquad low-pass at `cutoff` Hz along the last axis of (B, 1, T), (C, N) or (N,), every row from a zero state; no clamp and
    no 16-bit grid (PcmCodec is the one with both).  CUDA: one launch of wm_biquad, differentiable through its adjoint; CPU: scipy's
    lfilter with the same float32 coefficients (forward only)."""

    def __init__(self, cutoff, sample_rate=SAMPLE_RATE):
        super().__init__()
        self.coeffs = ops.biquad_lowpass_coeffs(sample_rate, cutoff)              # bad rates fail here
        self.cutoff, self.sample_rate = cutoff, sample_rate

    def forward(self, x):
        x = _time_rows(x, "x")
        if x.is_cuda:
            return _LowpassFn.apply(x.to(torch.float32), self.coeffs)
        from scipy.signal import lfilter
        b, a = np.array(self.coeffs[:3], dtype=np.float32), np.array((1.0,) + self.coeffs[3:], dtype=np.float32)
        y = lfilter(b, a, x.detach().to(torch.float32).numpy(), axis=-1)
        return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))

    def extra_repr(self):
        return f"cutoff={self.cutoff}, sample_rate={self.sample_rate}"


class Resampled(torch.nn.Module):
    """y = up(down(x))[..., :T] along the last axis of (B, 1, T), (C, N) or (N,), every row by itself: down is sample_rate -> rate, up is
    rate -> sample_rate, both the sinc resampler of ops.resample_table (torchaudio's default design) without mixdown.  The output has the
    input's shape (ceil(sample_rate * ceil(rate * T / sample_rate) / rate) >= T: the cut is always possible); rate == sample_rate returns
    x.  CUDA: two launches of wm_resample_rows, differentiable through the same two launches with the transposed tables
    (ops.ResampleRowsFn); CPU: the same float32 tables through F.conv1d, differentiable by autograd."""

    def __init__(self, rate, sample_rate=SAMPLE_RATE):
        super().__init__()
        ops.resample_table(sample_rate, rate)                                     # bad rates fail here
        ops.resample_table(rate, sample_rate)
        self.rate, self.sample_rate = int(rate), int(sample_rate)

    def forward(self, x):
        x = _time_rows(x, "x")
        if self.rate == self.sample_rate:
            return x
        T = x.shape[-1]
        rows = x.to(torch.float32).reshape(-1, T)
        if x.is_cuda:
            y = ops.ResampleRowsFn.apply(ops.ResampleRowsFn.apply(rows, self.sample_rate, self.rate), self.rate, self.sample_rate, T)
        else:
            from .inference import _resample_rows_host
            y = _resample_rows_host(_resample_rows_host(rows, self.sample_rate, self.rate), self.rate, self.sample_rate, T)
        return y.reshape(x.shape)

    def extra_repr(self):
        return f"rate={self.rate}, sample_rate={self.sample_rate}"


@torch.no_grad()
def evaluate_robustness(generator, detector, batches, attacks, device="cuda", message_bits=16, messages=None):
    """How detection moves under distortions: {name: {"watermarked_prob", "clean_prob", "bit_accuracy", "delta_rms"}} for every entry of
    `attacks` (name -> module on (B, 1, T)) and for "none", the undistorted signal.  Eval mode, no_grad; the Generator runs once per batch,
    every attack is applied to BOTH s + delta and s (the false-positive side: what an attack does to clean audio is half of the answer),
    as one call on their concatenation, and the Detector runs once per attack on the result.  The per-batch reductions are eval_forward's
    and the per-clip values of all batches are pooled and averaged once, as evaluate_batches does (a ragged last batch weighs by its
    clips).  `messages` (optional list, one tensor per batch) replaces the random draw."""
    from .step import _eval_reductions
    if "none" in attacks:
        raise ValueError('attacks: the name "none" is taken by the undistorted row')
    generator.eval(); detector.eval()
    keys = {"watermarked_prob": "prob_watermarked", "clean_prob": "prob_clean", "bit_accuracy": "bit_accuracy",
            "delta_rms": "delta_rms"}
    named = [("none", None)] + list(attacks.items())
    acc = OrderedDict((name, {k: [] for k in keys}) for name, _ in named)
    for bi, s in enumerate(batches):
        s = s.to(device)
        message = (messages[bi].to(device) if messages is not None else
                   torch.randint(0, 2 ** message_bits, (s.shape[0],), device=device))
        delta = postprocess(generator(s, message))
        both = torch.cat([s + delta, s], dim=0)
        for name, attack in named:
            out = _eval_reductions(detector(both if attack is None else attack(both)), message, delta)
            for k, src in keys.items():
                acc[name][k].append(out[src])
    return OrderedDict((name, {k: float(torch.cat(v).double().mean()) if v else math.nan for k, v in a.items()})
                       for name, a in acc.items())
