"""Spectral masking: is the difference between two signals audible NEXT TO the signal that carries it?  Noise-to-mask ratio per clip (as
PEAQ's "Total NMR"), the share of time-frequency cells where the difference pokes out of the mask, and the masking loss -- the mean number
of dB by which it does -- with its gradient.  The definition is the comment of wm_masking_fwd in include/wm_hip.h; CUDA tensors run
wm_masking_fwd / wm_masking_bwd (csrc/masking.hip), CPU tensors the float64 numpy restatement below.

What this is, and is not: ONE simultaneous-masking model of the 1988 kind (Bark bands, the Schroeder spreading function, Johnston's
tonality offset, Terhardt's threshold in quiet) at an ASSUMED playback level, a full-scale sine = 96 dB SPL.  No temporal (pre / post)
masking.  Defined at 16 kHz only: other rates are resampled to 16 kHz first (dsp.resample_rows), so nothing above 8 kHz is judged.  Frames
of 512 at hop 256 without padding: a tail shorter than a hop is not judged and gets zero gradient.  The mask is a function of the
reference alone and is not differentiated: the reference gets no gradient.  Parity with PEAQ, with an MPEG encoder's model and with
listeners is unmeasured.  Like STOI it assumes time-aligned signals: under TimeWarp, TimeStretch and PitchShift the number is meaningless."""
from __future__ import annotations

import collections
import ctypes
import math

import numpy as np
import torch

from . import dsp
from ._host import _chk_int, _f32, _p, _stream
from ._lib import lib

MASKING_RATE = 16000
MASKING_FRAME, MASKING_HOP, MASKING_BANDS = 512, 256, 22
_BINS = MASKING_FRAME // 2 + 1
_LEVEL_DB = 96.0                                 # the sound pressure level a full-scale sine is taken to have

Masking = collections.namedtuple("Masking", "nmr_db over_db audible cells")
_HOST = {}


def _bark(f):
    return 13.0 * np.arctan(0.00076 * f) + 3.5 * np.arctan((f / 7500.0) ** 2)


def _tables64():
    """the six tables in float64 numpy (cached): w, c, band (int64), S, G, A"""
    if "t64" not in _HOST:
        n = MASKING_FRAME
        w = 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(n) / n))
        c = np.full(_BINS, 2.0 * (8.0 / 3.0) / n ** 2)
        c[0] = c[n // 2] = (8.0 / 3.0) / n ** 2
        freq = np.arange(_BINS) * (MASKING_RATE / n)
        Z = int(math.floor(_bark(MASKING_RATE / 2.0))) + 1
        assert Z == MASKING_BANDS
        band = np.minimum(np.floor(_bark(freq)).astype(np.int64), Z - 1)
        delta = (np.arange(Z)[:, None] - np.arange(Z)[None, :]) + 0.474
        S = 10.0 ** ((15.81 + 7.5 * delta - 17.5 * np.sqrt(1.0 + delta ** 2)) / 10.0)
        G = S.sum(axis=1)
        khz = freq / 1000.0
        khz[0] = khz[1]
        ath = 3.64 * khz ** -0.8 - 6.5 * np.exp(-0.6 * (khz - 3.3) ** 2) + 1e-3 * khz ** 4
        A = np.array([0.5 * 10.0 ** ((ath[band == b].min() - _LEVEL_DB) / 10.0) for b in range(Z)])
        _HOST["t64"] = (w, c, band, S, G, A)
    return _HOST["t64"]


def masking_tables():
    """The tables of the model as CPU tensors, formed in float64 and rounded once (cached): {"w" (512,), "c" (257,), "band" (257,) int32,
    "S" (22, 22), "G" (22,), "A" (22,), "packed" (1042,)}; "packed" is the one buffer wm_masking_fwd reads, c | band's bits | S | G | A (the
    kernels form the window themselves: "w" is here for the host)."""
    if "tab" not in _HOST:
        w, c, band, S, G, A = _tables64()
        tab = {k: torch.from_numpy(np.ascontiguousarray(v)).to(torch.float32) for k, v in (("w", w), ("c", c), ("S", S), ("G", G), ("A", A))}
        tab["band"] = torch.from_numpy(band).to(torch.int32)
        tab["packed"] = torch.cat([tab["c"], tab["band"].view(torch.float32), tab["S"].reshape(-1), tab["G"], tab["A"]]).contiguous()
        _HOST["tab"] = tab
    return _HOST["tab"]


def masking_plan(rows, n):
    """(frames, chunk, scratch_bytes) of one wm_masking_fwd launch on (rows, n): the frames a row has, the frames one workgroup handles,
    the bytes of scratch"""
    for v, name in ((rows, "rows"), (n, "n")):
        _chk_int(v, name, 1, math.inf, "a positive int")
    if n > 2 ** 34 or rows * n > 2 ** 46:
        raise ValueError(f"rows = {rows}, n = {n}: a row may have 2^34 samples and a launch 2^46")
    out = (ctypes.c_longlong * 3)()
    base = ctypes.addressof(out)
    lib.wm_masking_plan(rows, n, base, base + 8, base + 16, None)
    return int(out[0]), int(out[1]), int(out[2])


def _row_host(x, y, grad):
    """(nmr_db, over_db, audible, cells, d over_db / d y or None) of one row pair in float64 numpy: the definition, step by step"""
    n = x.shape[0]
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        return math.nan, math.nan, 0, 0, (np.full(n, np.nan) if grad else None)
    F = 1 + (n - MASKING_FRAME) // MASKING_HOP if n >= MASKING_FRAME else 0
    if F == 0:
        return math.nan, 0.0, 0, 0, (np.zeros(n) if grad else None)
    w, c, band, S, G, A = _tables64()
    edges = np.flatnonzero(np.diff(band, prepend=-1))
    idx = MASKING_HOP * np.arange(F)[:, None] + np.arange(MASKING_FRAME)[None, :]
    X = np.fft.rfft(w * x[idx], axis=1)
    D = np.fft.rfft(w * (y - x)[idx], axis=1)
    Px, Pd = c * (X.real ** 2 + X.imag ** 2), c * (D.real ** 2 + D.imag ** 2)
    Ex, Ed = np.add.reduceat(Px, edges, axis=1), np.add.reduceat(Pd, edges, axis=1)
    inner = Px[:, 1:MASKING_FRAME // 2]
    sfm = 10.0 * np.log10(np.exp(np.log(inner + 1e-30).mean(axis=1)) / (inner.mean(axis=1) + 1e-30))
    alpha = np.clip(sfm / -60.0, 0.0, 1.0)[:, None]
    O = alpha * (14.5 + np.arange(MASKING_BANDS)[None, :]) + (1.0 - alpha) * 5.5
    T = np.maximum((Ex @ S.T) * 10.0 ** (-O / 10.0) / G, A)
    r = Ed / T
    cells = r.size
    with np.errstate(divide="ignore"):
        nmr_db = float(10.0 * np.log10(r.mean()))
        over_db = float(np.maximum(0.0, 10.0 * np.log10(r)).mean())
    hot = r > 1.0
    gy = None
    if grad:
        g = np.zeros_like(r)
        g[hot] = (10.0 / math.log(10.0)) / (cells * Ed[hot])
        # Re sum_{k <= 256} 2 g c_k D_k e^(+i..) = the inverse real transform of 512 * 2 g c_0 D_k: c_k's factor 2 is irfft's own
        u = w * np.fft.irfft(MASKING_FRAME * 2.0 * c[0] * g[:, band] * D, MASKING_FRAME, axis=1)
        gy = np.zeros(n)
        gy[:MASKING_HOP * F].reshape(F, MASKING_HOP)[...] += u[:, :MASKING_HOP]
        gy[MASKING_HOP:MASKING_HOP * (F + 1)].reshape(F, MASKING_HOP)[...] += u[:, MASKING_HOP:]
    return nmr_db, over_db, int(hot.sum()), int(cells), gy


def masking_rows_host(x, y, grad=False):
    """The float64 numpy restatement that CPU tensors take: x, y (rows, n) CPU tensors at 16 kHz.  Returns Masking(nmr_db, over_db float32,
    audible, cells int32), and with grad=True a second value, d over_db[row] / d y (rows, n) float32."""
    rows = [_row_host(a, b, grad) for a, b in zip(x.detach().double().numpy(), y.detach().double().numpy())]
    res = Masking(torch.tensor([r[0] for r in rows], dtype=torch.float64).to(torch.float32),
                  torch.tensor([r[1] for r in rows], dtype=torch.float64).to(torch.float32),
                  torch.tensor([r[2] for r in rows], dtype=torch.int32), torch.tensor([r[3] for r in rows], dtype=torch.int32))
    if not grad:
        return res
    return res, torch.from_numpy(np.stack([r[4] for r in rows])).to(torch.float32)


def _pair(x, y):
    xr, yr = dsp._stoi_rows(x, "x"), dsp._stoi_rows(y, "y")
    if x.shape != y.shape:
        raise ValueError(f"x and y: expected equal shapes, got {tuple(x.shape)} and {tuple(y.shape)}")
    if xr.device != yr.device:
        raise ValueError(f"x and y: expected one device, got {xr.device} and {yr.device}")
    return xr, yr


def _tables_on(device):
    return dsp._on_device("masking", device, lambda: masking_tables()["packed"])


def _launch_fwd(xr, yr, want_coef):
    """wm_masking_fwd on contiguous CUDA rows at 16 kHz: (nmr_db, over_db, counts (rows, 2) int32, coef or None)"""
    rows, n = xr.shape
    frames, _, need = masking_plan(rows, n)
    dev = xr.device
    nmr, over = _f32(rows, device=dev), _f32(rows, device=dev)
    counts = torch.empty(rows, 2, dtype=torch.int32, device=dev)
    coef = _f32(rows, frames, MASKING_BANDS, device=dev) if want_coef else None
    scratch = torch.empty(need // 4, dtype=torch.int32, device=dev)
    lib.wm_masking_fwd(_p(xr), _p(yr), _p(_tables_on(dev)), _p(nmr), _p(over), _p(counts), _p(coef), _p(scratch), rows, n, _stream())
    return nmr, over, counts, coef


def masking(x, y, sample_rate=16000):
    """The masking model of every row of y (the processed signal) against the same row of x (the reference): float32 tensors of equal shape
    (B, 1, T), (C, N) or (N,) at `sample_rate`.  Returns Masking(nmr_db, over_db, audible, cells), one entry per row on the inputs' device:
    the noise-to-mask ratio in dB, the mean excess over the mask in dB (the loss), the number of cells where the difference is above the mask
    and the number of cells (22 per frame) as int32.  A row under 512 samples has no frame: NaN, 0, 0, 0.  y == x: -inf, 0.  A non-finite sample:
    NaN, NaN, 0, 0 for that row.  CUDA tensors: one wm_masking_fwd call, preceded by ONE resample_rows launch on x and y stacked unless
    sample_rate == 16000 (nothing above 8 kHz is judged).  CPU tensors: masking_rows_host (after the host resampler).  Not differentiable:
    MaskingLoss is."""
    rate = dsp._rate(sample_rate, "sample_rate")
    xr, yr = _pair(x, y)
    rows = xr.shape[0]
    if rate != MASKING_RATE:
        if xr.is_cuda:
            both = dsp.resample_rows(torch.cat([xr, yr], dim=0), rate, MASKING_RATE)
        else:
            from .inference import _resample_rows_host
            both = _resample_rows_host(torch.cat([xr, yr], dim=0), rate, MASKING_RATE)
        xr, yr = both[:rows].contiguous(), both[rows:].contiguous()
    if not xr.is_cuda:
        return masking_rows_host(xr, yr)
    nmr, over, counts, _ = _launch_fwd(xr.detach(), yr.detach(), False)
    return Masking(nmr, over, counts[:, 0].contiguous(), counts[:, 1].contiguous())


class MaskingFn(torch.autograd.Function):
    """over_db (rows,) of the (rows, n) rows y against x at 16 kHz.  Forward: wm_masking_fwd with the per-cell coefficients kept; backward:
    ONE wm_masking_bwd.  x gets no gradient: the mask is a constant of the backward pass.  CPU tensors go through masking_rows_host."""

    @staticmethod
    def forward(ctx, x, y):
        x, y = x.detach().contiguous(), y.detach().contiguous()
        if not x.is_cuda:
            res, gy = masking_rows_host(x, y, grad=True)
            ctx.save_for_backward(gy)
            ctx.host = True
            return res.over_db
        _, over, _, coef = _launch_fwd(x, y, True)
        ctx.save_for_backward(x, y, coef)
        ctx.host = False
        return over

    @staticmethod
    def backward(ctx, gout):
        if ctx.host:
            gy, = ctx.saved_tensors
            return None, gy * gout.to(torch.float32)[:, None]
        x, y, coef = ctx.saved_tensors
        rows, n = x.shape
        gout = gout.to(torch.float32).contiguous()
        gy = torch.empty_like(y)
        lib.wm_masking_bwd(_p(x), _p(y), _p(coef), _p(gout), _p(gy), rows, n, _stream())
        return None, gy


class MaskingLoss(torch.nn.Module):
    """The mean over the rows of over_db: by how many dB, on average over the time-frequency cells, the difference watermarked - clean is
    above the masking threshold of the clean signal.  0 when it is below the mask everywhere (and then the gradient is 0 too: the term
    switches itself off).  clean, watermarked: (B, 1, T), (C, N) or (N,) float32 at 16 kHz; the gradient goes to `watermarked` alone."""

    def forward(self, clean, watermarked):
        xr, yr = _pair(clean, watermarked)
        return MaskingFn.apply(xr, yr).mean()
