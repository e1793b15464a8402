"""Argument checks and launch plumbing shared by the two wrapper modules over the C ABI: ops.py (the models' tape) and dsp.py
(the waveform ops).  No state, and nothing of the package is imported here: _host <- dsp <- ops is the only direction.
"""
from __future__ import annotations

import math

import torch


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, name: str, ndim: int | None = None, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: the watermark hot path runs on the GPU only (got a {t.device} tensor); "
                           "there is no CPU fallback")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name}: expected {ndim} dims, got shape {tuple(t.shape)}")
    return t.contiguous()


def _chk_int(v, name, lo=None, hi=None, what=None):
    """v where it is an int (bools refused), in [lo, hi] where a range is given; `what` replaces "an int in [lo, hi]" in the message"""
    if isinstance(v, bool) or not isinstance(v, int) or not (lo is None or lo <= v <= hi):
        raise ValueError(f"{name}: expected {what or f'an int in [{lo}, {hi}]'}, got {v!r}")
    return v


def _chk_positive(v, name):
    """v where it is a positive finite number (bools refused)"""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v <= 0:
        raise ValueError(f"{name} must be a positive finite number, got {v!r}")
    return v


def _seed64(seed):
    """the seed's low 64 bits as the signed value the launchers take (they split it into the key's two halves)"""
    seed = int(seed) & (2 ** 64 - 1)
    return seed - 2 ** 64 if seed >= 2 ** 63 else seed


def _f32(*shape, device):
    return torch.empty(shape, dtype=torch.float32, device=device)
