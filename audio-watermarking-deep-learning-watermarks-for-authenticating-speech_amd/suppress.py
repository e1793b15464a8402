"""Noise suppression as an attack: a short-time spectral Wiener gate with a decision-directed a-priori SNR, the signal path that
Ephraim-Malah / Scalart-Filho suppressors and WebRTC-style noise suppression share.  The watermark is by construction a low-level
noise-like signal, and a suppressor is the one common processing step whose purpose is to remove exactly that.  The definition is the
comment of wm_noise_suppress in include/wm_hip.h; CUDA tensors run wm_noise_suppress (csrc/noise_suppress.hip), CPU tensors the float64
numpy restatement below.

What this is, and is not: a STAND-IN.  It uses one stationary noise estimate per row (the geometric mean of the row's own frame powers, or a
profile the caller gives).  It has no voice-activity detector, no minimum-statistics tracking and no neural denoiser.  A stationary tone
counts as noise and is attenuated.  The gradient holds the gains constant: the backward is the same launch with the saved input's gains
applied to dy.  Parity with WebRTC NS, RNNoise, `noisereduce` or any product's suppressor is unmeasured.  Defined at 16 kHz.  The output
stays time-aligned with the input, so STOI and NMR apply."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import dsp
from ._host import _chk_int, _f32, _p, _stream
from ._lib import lib

SUPPRESS_RATE = 16000
SUPPRESS_FRAME, SUPPRESS_HOP, SUPPRESS_BINS = 512, 256, 257
SUPPRESS_EPS = 1e-10
EULER_GAMMA = 0.5772156649015329
SUPPRESS_MAX_REDUCE_DB = 60.0


def suppress_frames(n):
    """M = ceil(n / 256) + 1: the frames of a row of n samples"""
    return -(-int(n) // SUPPRESS_HOP) + 1


def suppress_plan(rows, n):
    """(frames, scratch_bytes) of one wm_noise_suppress launch on (rows, n): the frames a row has and the bytes of scratch"""
    for v, name in ((rows, "rows"), (n, "n")):
        _chk_int(v, name, 1, math.inf, "a positive int")
    if n > 2 ** 34 or rows * n > 2 ** 46:
        raise ValueError(f"rows = {rows}, n = {n}: a row may have 2^34 samples and a launch 2^46")
    out = (ctypes.c_longlong * 2)()
    base = ctypes.addressof(out)
    lib.wm_noise_suppress_plan(rows, n, base, base + 8, None)
    return int(out[0]), int(out[1])


def _chk_scalars(alpha, over):
    for v, name in ((alpha, "alpha"), (over, "over")):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name}: expected a finite number, got {v!r}")
    if not 0.0 <= alpha < 1.0 or not float(np.float32(alpha)) < 1.0:
        raise ValueError(f"alpha: expected a value in [0, 1), got {alpha!r}")
    if not over > 0.0 or not 0.0 < float(np.float32(over)) < math.inf:
        raise ValueError(f"over: expected a positive finite number, got {over!r}")
    return float(alpha), float(over)


def _reduce_rows(reduce_db, rows, device):
    """reduce_db, a number or a per-row tensor, as a (rows,) float32 tensor on `device`"""
    if isinstance(reduce_db, torch.Tensor):
        if reduce_db.numel() != rows or reduce_db.dim() > 1:
            raise ValueError(f"reduce_db: expected a number or a tensor of {rows} values, one per row, got shape {tuple(reduce_db.shape)}")
        return reduce_db.detach().to(device=device, dtype=torch.float32).reshape(rows).contiguous()
    if isinstance(reduce_db, bool) or not isinstance(reduce_db, (int, float)):
        raise ValueError(f"reduce_db: expected a number or a per-row tensor, got {reduce_db!r}")
    return torch.full((rows,), float(reduce_db), dtype=torch.float32, device=device)


def _profile_rows(noise_psd, rows, device):
    """noise_psd, None or a (257,) or (rows, 257) tensor of finite values >= 0, as a (rows, 257) float32 tensor on `device` (or None)"""
    if noise_psd is None:
        return None
    if not isinstance(noise_psd, torch.Tensor) or noise_psd.shape not in ((SUPPRESS_BINS,), (rows, SUPPRESS_BINS)):
        raise ValueError(f"noise_psd: expected None or a ({SUPPRESS_BINS},) or ({rows}, {SUPPRESS_BINS}) tensor, got "
                         f"{tuple(noise_psd.shape) if isinstance(noise_psd, torch.Tensor) else type(noise_psd).__name__}")
    prof = noise_psd.detach().to(device=device, dtype=torch.float32)
    if not bool((torch.isfinite(prof) & (prof >= 0)).all()):
        raise ValueError("noise_psd: expected finite values >= 0")
    return prof.expand(rows, SUPPRESS_BINS).contiguous()


def _window64():
    return np.sin(np.pi * (np.arange(SUPPRESS_FRAME) + 0.5) / SUPPRESS_FRAME)


def _frames64(v, M):
    """(M, 512) windowed frames of the float64 row v: 256 zeros in front, zeros behind up to (M + 1) 256 samples"""
    vp = np.zeros((M + 1) * SUPPRESS_HOP)
    vp[SUPPRESS_HOP:SUPPRESS_HOP + v.shape[0]] = v
    return _window64() * vp[SUPPRESS_HOP * np.arange(M)[:, None] + np.arange(SUPPRESS_FRAME)[None, :]]


def _row_host(x, src, reduce_db, noise, alpha, over):
    """(y (n,), G (M, 257), N (257,)) of one row in float64 numpy: the definition, step by step; src None: x itself"""
    n = x.shape[0]
    M = suppress_frames(n)
    if not np.isfinite(x).all():
        return np.full(n, np.nan), np.full((M, SUPPRESS_BINS), np.nan), np.full(SUPPRESS_BINS, np.nan)
    X = np.fft.rfft(_frames64(x, M), axis=1)
    P = X.real ** 2 + X.imag ** 2
    N = noise if noise is not None else math.exp(EULER_GAMMA) * np.exp(np.log(P + SUPPRESS_EPS).mean(axis=0))
    rd = 0.0 if math.isnan(reduce_db) else min(max(reduce_db, 0.0), SUPPRESS_MAX_REDUCE_DB)
    gmin = 10.0 ** (-rd / 20.0)
    g = P / (over * N + SUPPRESS_EPS)
    G = np.empty_like(P)
    q = np.ones(SUPPRESS_BINS)
    for m in range(M):
        xi = alpha * q + (1.0 - alpha) * np.maximum(g[m] - 1.0, 0.0)
        G[m] = np.maximum(xi / (1.0 + xi), gmin)
        q = G[m] ** 2 * g[m]
    S = X if src is None else np.fft.rfft(_frames64(src, M), axis=1)
    yf = _window64() * np.fft.irfft(G * S, SUPPRESS_FRAME, axis=1)
    out = np.zeros((M + 1) * SUPPRESS_HOP)
    out[:M * SUPPRESS_HOP].reshape(M, SUPPRESS_HOP)[...] += yf[:, :SUPPRESS_HOP]
    out[SUPPRESS_HOP:].reshape(M, SUPPRESS_HOP)[...] += yf[:, SUPPRESS_HOP:]
    return out[SUPPRESS_HOP:SUPPRESS_HOP + n], G, N


def suppress_rows_host(x, reduce_db, src=None, noise_psd=None, alpha=0.98, over=1.0, gains_out=False):
    """The float64 numpy restatement that CPU tensors take, rounded once, forward only: x (rows, n) a CPU tensor at 16 kHz, reduce_db a
    (rows,) tensor, src None or like x, noise_psd None or (rows, 257).  Returns y (rows, n) float32, with gains_out=True
    (y, G (rows, M, 257), N (rows, 257))."""
    x64 = x.detach().double().numpy()
    s64 = None if src is None else src.detach().double().numpy()
    prof = None if noise_psd is None else noise_psd.detach().double().numpy()
    rd = reduce_db.detach().to(torch.float32).double().numpy()
    res = [_row_host(x64[r], None if s64 is None else s64[r], float(rd[r]), None if prof is None else prof[r], float(alpha), float(over)) for r in range(x64.shape[0])]
    y = torch.from_numpy(np.stack([r[0] for r in res])).to(torch.float32)
    if not gains_out:
        return y
    return (y, torch.from_numpy(np.stack([r[1] for r in res])).to(torch.float32),
            torch.from_numpy(np.stack([r[2] for r in res])).to(torch.float32))


def _launch(xr, src, reduce_db, noise, alpha, over, gains_out):
    """wm_noise_suppress on contiguous CUDA rows at 16 kHz: (y, G or None, N or None)"""
    rows, n = xr.shape
    frames, need = suppress_plan(rows, n)
    dev = xr.device
    y = torch.empty_like(xr)
    G = _f32(rows, frames, SUPPRESS_BINS, device=dev) if gains_out else None
    N = _f32(rows, SUPPRESS_BINS, device=dev) if gains_out else None
    scratch = torch.empty(need // 4, dtype=torch.int32, device=dev)
    lib.wm_noise_suppress(_p(xr), _p(src), _p(noise), _p(reduce_db), _p(y), _p(G), _p(N), _p(scratch), rows, n, alpha, over, _stream())
    return y, G, N


def _rows_of(x, reduce_db, src, noise_psd, alpha, over):
    xr = dsp._stoi_rows(x, "x")
    rows = xr.shape[0]
    alpha, over = _chk_scalars(alpha, over)
    sr = None
    if src is not None:
        sr = dsp._stoi_rows(src, "src")
        if src.shape != x.shape or sr.device != xr.device:
            raise ValueError(f"src: expected x's shape {tuple(x.shape)} and device, got {tuple(src.shape)} on {sr.device}")
    return xr, _reduce_rows(reduce_db, rows, xr.device), sr, _profile_rows(noise_psd, rows, xr.device), alpha, over


def noise_suppress(x, reduce_db, src=None, noise_psd=None, alpha=0.98, over=1.0, gains_out=False):
    """The Wiener gate of every row of x, a float32 tensor (B, 1, T), (C, N) or (N,) at 16 kHz: gains from x, at most reduce_db dB of
    attenuation per bin (a number, or a tensor with one value per row; NaN counts as 0, values are clipped to [0, 60]), applied to src
    (None: x itself; else a tensor like x -- the backward passes dy).  noise_psd: None, the row judges itself, or a (257,) / (rows, 257)
    profile of |X|^2 of the 512-point sine-windowed transform that is taken as the noise.  alpha: the decision-directed weight; over: the
    over-subtraction factor.  Returns y in x's shape, with gains_out=True (y, G (rows, M, 257), N (rows, 257)), M = ceil(n / 256) + 1.
    A row with a non-finite sample comes back all NaN.  CUDA tensors: one wm_noise_suppress call; CPU tensors: suppress_rows_host.  A
    stand-in (one stationary estimate per row, no voice-activity detector, no minimum statistics, no neural denoiser; parity with any
    product's suppressor unmeasured).  Not differentiable: NoiseSuppressFn is."""
    xr, rd, sr, prof, alpha, over = _rows_of(x, reduce_db, src, noise_psd, alpha, over)
    if xr.is_cuda:
        y, G, N = _launch(xr.detach(), None if sr is None else sr.detach(), rd, prof, alpha, over, gains_out)
    else:
        res = suppress_rows_host(xr, rd, sr, prof, alpha, over, gains_out)
        y, G, N = res if gains_out else (res, None, None)
    y = y.reshape(x.shape)
    return (y, G, N) if gains_out else y


class NoiseSuppressFn(torch.autograd.Function):
    """y (rows, n) of the (rows, n) CUDA rows x at 16 kHz: x, reduce_db (rows,), noise (rows, 257) or None, alpha, over.  It saves x and
    reduce_db; with the gains held the map is self-adjoint, so the backward is the same call with src = dy.  The dependence of the gains
    on x is not differentiated."""

    @staticmethod
    def forward(ctx, x, reduce_db, noise, alpha, over):
        x = x.detach().contiguous()
        ctx.save_for_backward(x, reduce_db)
        ctx.noise, ctx.alpha, ctx.over = noise, alpha, over
        return _launch(x, None, reduce_db, noise, alpha, over, False)[0]

    @staticmethod
    def backward(ctx, dy):
        x, reduce_db = ctx.saved_tensors
        dx = _launch(x, dy.to(torch.float32).contiguous(), reduce_db, ctx.noise, ctx.alpha, ctx.over, False)[0]
        return dx, None, None, None, None
