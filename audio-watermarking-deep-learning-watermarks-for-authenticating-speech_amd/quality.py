"""Signal-quality measures of the evaluation side.  STOI (short-time objective intelligibility, Taal, Hendriks, Heusdens and Jensen 2011):
what an attack, or the watermark, does to the speech itself, as a number in (about) [0, 1] per clip.  The reference's baseline variant
calls pystoi.stoi(clean, wm, 16000, extended=False) once per one-second segment in a Python loop on the CPU (py/main14.py:1099-1203,
py/main16.py:2012-2153); here all rows go through one wm_stoi call (csrc/stoi.hip) and nothing but the scores crosses to the host.

The definition is the comment of wm_stoi in include/wm_hip.h; at 10 kHz it is pystoi's.  Rows at another rate are first taken to 10 kHz
by the project's own resampler (ops.resample_rows, torchaudio's default sinc design); pystoi uses a different, Octave-style polyphase
filter there, so parity with pystoi at 16 kHz is unmeasured.  Extended STOI (extended=True) is not built.  STOI assumes time-aligned
signals: under attacks.TimeWarp it is low by construction and says nothing."""
from __future__ import annotations

import numpy as np
import torch

STOI_RATE = 10000
STOI_SENTINEL = 1e-5                             # fewer than 30 spectral frames: the published value
_EPS = 2.0 ** -52
_FRAME, _HOP, _NFFT, _SEG = 256, 128, 512, 30
STOI_BANDS = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
              (109, 138), (138, 174), (174, 219))
METRICS = ("stoi", "nmr")


def _cut(v, count):
    return v[_HOP * np.arange(count)[:, None] + np.arange(_FRAME)[None, :]]


def stoi_row_host(x, y):
    """(d, K) of one row pair at 10 kHz in float64 numpy: the definition, step by step"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        return float("nan"), 0
    n = x.shape[0]
    F = max(0, -(-(n - _FRAME) // _HOP))
    if F == 0:
        return STOI_SENTINEL, 0
    w = np.hanning(_FRAME + 2)[1:-1]
    xf, yf = w * _cut(x, F), w * _cut(y, F)
    norms = np.sqrt(np.einsum("ft,ft->f", xf, xf))
    keep = norms + _EPS > 0.01 * (norms.max() + _EPS)
    K = int(keep.sum())
    S = K - 1
    if S < _SEG:
        return STOI_SENTINEL, K
    xs, ys = np.zeros(_HOP * (K + 1)), np.zeros(_HOP * (K + 1))
    for sig, frames in ((xs, xf[keep]), (ys, yf[keep])):
        sig[:_HOP * K] += frames[:, :_HOP].reshape(-1)
        sig[_HOP:] += frames[:, _HOP:].reshape(-1)
    X = np.abs(np.fft.rfft(w * _cut(xs, S), _NFFT, axis=1)) ** 2
    Y = np.abs(np.fft.rfft(w * _cut(ys, S), _NFFT, axis=1)) ** 2
    Xb = np.sqrt(np.stack([X[:, lo:hi].sum(axis=1) for lo, hi in STOI_BANDS]))       # (15, S)
    Yb = np.sqrt(np.stack([Y[:, lo:hi].sum(axis=1) for lo, hi in STOI_BANDS]))
    xi = np.lib.stride_tricks.sliding_window_view(Xb, _SEG, axis=1)
    eta = np.lib.stride_tricks.sliding_window_view(Yb, _SEG, axis=1)
    alpha = np.linalg.norm(xi, axis=2, keepdims=True) / (np.linalg.norm(eta, axis=2, keepdims=True) + _EPS)
    eta = np.minimum(alpha * eta, (1.0 + 10.0 ** (15.0 / 20.0)) * xi)
    xi = xi - xi.mean(axis=2, keepdims=True)
    eta = eta - eta.mean(axis=2, keepdims=True)
    xi = xi / (np.linalg.norm(xi, axis=2, keepdims=True) + _EPS)
    eta = eta / (np.linalg.norm(eta, axis=2, keepdims=True) + _EPS)
    return float((xi * eta).sum(axis=2).mean()), K


def stoi_rows_host(x, y):
    """(d (rows,) float32, kept (rows,) int32) CPU tensors of the (rows, n) CPU tensors x, y at 10 kHz"""
    scores = [stoi_row_host(a, b) for a, b in zip(x.double().numpy(), y.double().numpy())]
    return (torch.tensor([s[0] for s in scores], dtype=torch.float64).to(torch.float32),
            torch.tensor([s[1] for s in scores], dtype=torch.int32))


def stoi(reference, processed, sample_rate=16000):
    """STOI of `processed` against `reference`: tensors of equal shape (B, 1, T), (C, N) or (N,) at `sample_rate`; returns d with the input's
    leading shape ((B,), (C,) or a 0-d tensor), float32 on the inputs' device.  CUDA tensors run wm_stoi (one resampling launch first unless
    the rate is 10 kHz); CPU tensors run the float64 host restatement.  A row with fewer than 30 spectral frames (under 4097 samples at
    10 kHz, or mostly silence) scores the published sentinel 1e-5; a row with a non-finite sample scores NaN."""
    from . import dsp
    d, _ = dsp.stoi(reference, processed, sample_rate)
    lead = tuple(reference.shape[:-2]) if reference.dim() == 3 else tuple(reference.shape[:-1])
    return d.reshape(lead)


def nmr(reference, processed, sample_rate=16000):
    """Noise-to-mask ratio in dB of `processed` against `reference` (masking.masking: one simultaneous-masking model at an assumed playback
    level, see that module for what it is not): tensors of equal shape (B, 1, T), (C, N) or (N,) at `sample_rate`; returns nmr_db with the
    input's leading shape, float32 on the inputs' device.  Below 0 dB the difference is, on average, under the mask.  A row under 512 samples
    at 16 kHz or with a non-finite sample scores NaN; processed == reference scores -inf."""
    from .masking import masking
    res = masking(reference, processed, sample_rate)
    lead = tuple(reference.shape[:-2]) if reference.dim() == 3 else tuple(reference.shape[:-1])
    return res.nmr_db.reshape(lead)


def check_metrics(quality):
    """the `quality=` argument of the evaluation entry points as a tuple of known names"""
    if isinstance(quality, str):
        quality = (quality,)
    quality = tuple(quality)
    for q in quality:
        if q not in METRICS:
            raise ValueError(f"quality: unknown metric {q!r}; known: {', '.join(METRICS)}")
    return quality
