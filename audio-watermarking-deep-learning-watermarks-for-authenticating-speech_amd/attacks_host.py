"""What a CPU tensor runs in place of the attack kernels: every wm_* definition of include/wm_hip.h that attacks.py's modules launch,
restated in numpy or torch ops with the host-side draws of draws.py.  Nothing of the modules is here -- they hand over what they read
from themselves -- and suppress.suppress_rows_host, NoiseSuppress's, lives with its op in suppress.py.

  distort_rows_host, mdct_codec_rows_host, _lpc_rows_host, splice_rows_host      numpy, forward only
  _conv_rows_host, _warp_rows_host, _wsola_rows_host                              torch ops, which autograd differentiates
  pack_labels, unpack_labels                                                      Splice's bit-mask layout"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from . import dsp
from .draws import normal_noise, row_parameters, row_splice_spans


def distort_rows_host(x, draw, row0, seed, bounds):
    """(y, stat (rows, 4)) of a CPU tensor: wm_distort's definition, Distortion's `bounds` and `seed`"""
    n = x.shape[-1]
    x2 = x.reshape(-1, n)
    gain_db, snr_db, noisy = row_parameters(seed, draw, row0 + np.arange(x2.shape[0]), bounds)
    ms = x2.double().pow(2).mean(dim=1).numpy()
    g = np.float32(10.0) ** (gain_db.astype(np.float64) / 20.0)
    s = np.where(noisy, np.abs(g) * np.sqrt(ms) * 10.0 ** (-snr_db.astype(np.float64) / 20.0), 0.0)
    g32, s32 = g.astype(np.float32), s.astype(np.float32)
    y = x2 * torch.from_numpy(g32)[:, None]                                   # g = 1 hands x on bit for bit
    for r in np.nonzero(s32)[0]:
        z = torch.from_numpy(normal_noise(seed, draw, row0 + int(r), n))
        y[r] = (float(g32[r]) * x2[r].double() + float(s32[r]) * z).float()
    stat = np.stack([g32, s32, ms.astype(np.float32), np.where(noisy, snr_db, np.float32(np.inf))], axis=1)
    return y.reshape(x.shape), torch.from_numpy(stat.astype(np.float32))


def mdct_codec_rows_host(x, snr, hop, band, kcut, floor_step):
    """(y, int16 codes (rows, F, hop)) of a CPU tensor: the definition in float32 numpy, dense matrices"""
    M, n, f32 = hop, x.shape[-1], np.float32
    x2 = x.reshape(-1, n).numpy()
    rows, F = x2.shape[0], dsp.mdct_frames(n, M)
    j, k = np.arange(2 * M, dtype=np.float64), np.arange(M, dtype=np.float64)
    w = np.sin(np.pi * (j + 0.5) / (2 * M)).astype(f32)
    C = np.cos(np.pi / M * np.outer(k + 0.5, j + 0.5 + M / 2)).astype(f32)
    xp = np.zeros((rows, (F + 1) * M), dtype=f32)
    xp[:, M:M + n] = x2
    X = (np.stack([xp[:, f * M:(f + 2) * M] for f in range(F)], axis=1) * w) @ C.T
    X[:, :, kcut:] = 0
    P = (X.reshape(rows, F, M // band, band) ** 2).mean(axis=3, dtype=f32)
    scale = (f32(10) ** (-snr.numpy() / f32(20))).astype(f32).reshape(rows, 1, 1)
    step = np.repeat(np.maximum(np.sqrt(f32(12) * P) * scale, f32(floor_step)), band, axis=2)
    q = np.rint(X / step)
    yf = f32(2.0 / M) * w * ((q * step) @ C)
    out = np.zeros_like(xp)
    for f in range(F):
        out[:, f * M:(f + 2) * M] += yf[:, f]
    return torch.from_numpy(np.ascontiguousarray(out[:, M:M + n])).reshape(x.shape), torch.from_numpy(q.astype(np.int16))


def _lpc_rows_host(x2, snr, L, p, sample_rate, floor_step):
    """wm_lpc_codec's forward on a (rows, n) float32 array in float32 numpy: (y, coefficients (rows, F, p), int16 codes (rows, n)).  The
    definition of include/wm_hip.h with numpy's own summation order inside the autocorrelation and the frame energy."""
    f32 = np.float32
    rows, n = x2.shape
    F = dsp.lpc_frames(n, L)
    lag, expand = (t.numpy() for t in dsp.lpc_tables(p, sample_rate))
    j = np.arange(2 * L, dtype=np.float64)
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * (j + 0.5) / (2 * L))).astype(f32)
    xp = np.zeros((rows, L // 2 + F * L + L), dtype=f32)
    xp[:, L // 2:L // 2 + n] = x2
    s = np.stack([xp[:, f * L:f * L + 2 * L] for f in range(F)], axis=1) * w                       # (rows, F, 2L)
    Rc = np.stack([(s[..., :2 * L - k] * s[..., k:]).sum(axis=-1, dtype=f32) for k in range(p + 1)], axis=-1) * lag
    a = np.zeros((rows, F, p + 1), dtype=f32)                                                      # a[..., k] is tap k; entry 0 unused
    E = Rc[..., 0].copy()
    go = E > 0
    E = np.where(go, E, f32(1))
    for i in range(1, p + 1):
        acc = Rc[..., i].copy()
        for m in range(1, i):
            acc = acc + a[..., m] * Rc[..., i - m]
        k = -acc / E
        go = go & (np.abs(k) < 1)
        k = np.where(go, k, f32(0)).astype(f32)
        a[..., 1:i] = a[..., 1:i] + k[..., None] * a[..., i - 1:0:-1]
        a[..., i] = k
        E = (E * (f32(1) - k * k)).astype(f32)
    a = (a[..., 1:] * expand).astype(f32)
    at = np.repeat(a, L, axis=1)[:, :n]                                                            # (rows, n, p): the set of sample t
    hist = np.zeros((rows, n + p), dtype=f32)
    hist[:, p:] = x2
    e = x2.copy()
    for k in range(1, p + 1):
        e = e + at[:, :, k - 1] * hist[:, p - k:p - k + n]
    ep = np.zeros((rows, F * L), dtype=f32)
    ep[:, :n] = e
    cnt = np.minimum(L, n - L * np.arange(F)).astype(f32)
    P = (ep.reshape(rows, F, L) ** 2).sum(axis=2, dtype=f32) / cnt
    snr = np.nan_to_num(np.asarray(snr, dtype=f32), nan=0.0).clip(0, 60)
    g = (10.0 ** (-snr.astype(np.float64) / 20.0)).astype(f32).reshape(rows, 1)
    step = np.repeat(np.maximum(np.sqrt(f32(12) * P) * g, f32(floor_step)), L, axis=1)[:, :n]
    q = np.rint(e / step)
    eq = (q * step).astype(f32)
    y = np.zeros((rows, n + p), dtype=f32)                                                         # y[:, p + t]; the first p are the silence before
    ar = at[:, :, ::-1]
    for t in range(n):
        y[:, p + t] = eq[:, t] - (ar[:, t] * y[:, t:t + p]).sum(axis=1, dtype=f32)
    return np.ascontiguousarray(y[:, p:]), a, q.astype(np.int16)


def _conv_rows_host(rows2d, h):
    """H x per row of a (rows, n) float32 CPU tensor, h (K,) or (rows, K): F.conv1d with one group per row, which autograd differentiates"""
    rows, K = rows2d.shape[0], h.shape[-1]
    w = (h.expand(rows, K) if h.dim() == 1 else h).flip(-1).reshape(rows, 1, K)
    return F.conv1d(F.pad(rows2d.unsqueeze(0), (K - 1, 0)), w, groups=rows)[0]


def _sinpi(v):
    """sin(pi v) of a float64 tensor, reduced to [-1/2, 1/2] first so that the argument of sin carries no rounding of pi v at large v"""
    k = torch.round(v)
    return torch.sin(math.pi * (v - k)) * (1.0 - 2.0 * torch.remainder(k, 2.0))


def _warp_rows_host(x2, params, table, zeros, res):
    """wm_time_warp's forward map on a (rows, n) float32 CPU tensor in torch ops, which autograd differentiates: positions and weights from
    the definition (fp64 positions, float32 table, float32 weights), the taps gathered per output sample and summed in float32.  Row by
    row, so that a row's bits do not depend on the rest of the batch."""
    n = x2.shape[1]
    t = torch.arange(n, dtype=torch.float64)
    out = []
    for xr, prm in zip(x2, params):
        a, off, d, w, phi = (float(v) for v in prm[:5])
        c32 = torch.tensor(1.0 if math.isnan(float(prm[5])) else min(max(float(prm[5]), 0.25), 1.0), dtype=torch.float32)
        c = float(c32)
        q = w * t + phi
        p = a * t + off + d * _sinpi(2.0 * (q - torch.floor(q)))
        H = int(math.ceil(zeros / c))
        k = (torch.floor(p) - H)[:, None] + torch.arange(2 * H + 2, dtype=torch.float64)      # covers (p - H - 1, p + H + 1]
        v = c * (p[:, None] - k).abs()
        inside = (v < zeros) & (k >= 0) & (k < n)
        s = v * res
        i = torch.floor(s).clamp(0, zeros * res - 1)
        f = (s - i).to(torch.float32)
        i = i.to(torch.int64)
        t0 = table[i]
        W = torch.where(inside, c32 * (f * (table[i + 1] - t0) + t0), torch.zeros((), dtype=torch.float32))
        out.append((W * xr[k.clamp(0, n - 1).to(torch.int64)]).sum(dim=-1))
    return torch.stack(out)


def _wsola_rows_host(x2, rates, n_out, L, S):
    """wm_wsola's modes 0 and 1 on a (rows, n) float32 CPU tensor in torch ops: (y, delta).  The search runs on the values alone (the
    float32 scores summed in torch's order, the tie order of the definition); the synthesis is a gather at the chosen positions --
    constants -- and w u + (1 - w) v in float64 rounded to float32 once (u where u = v, bit for bit), which autograd differentiates
    with the weights w and 1 - w of the adjoint's definition.  Row by row."""
    rows, n = x2.shape
    hs = L // 2
    K = dsp.wsola_frames(n_out, L)
    win = dsp.wsola_window(L)
    cand = torch.arange(-S, S + 1)
    order = torch.argsort(torch.where(cand == 0, 0, torch.where(cand < 0, -2 * cand - 1, 2 * cand)))     # 0, -1, +1, -2, +2, ...
    j = torch.arange(hs)
    delta = torch.zeros((rows, K), dtype=torch.int32)
    out = []
    for r in range(rows):
        rate = float(np.float32(rates[r]))
        if not (0.25 <= rate <= 4.0):
            out.append(torch.zeros(n_out, dtype=torch.float32))
            continue
        xd = x2[r].detach()
        a = np.floor(rate * ((np.arange(K, dtype=np.float64) - 1.0) * hs) + 0.5).astype(np.int64)
        p = np.zeros(K, dtype=np.int64)
        p[0] = a[0]
        for k in range(1, K):
            q, c0 = int(p[k - 1]) + hs, int(a[k]) - S
            T, C = _gather_ext(xd, q + torch.arange(L), n), _gather_ext(xd, c0 + torch.arange(L + 2 * S), n)
            d = T[None, :] - C.unfold(0, L, 1)
            score = (d * d).sum(dim=1)[order]
            score = torch.where(torch.isnan(score), torch.full_like(score, float("inf")), score)
            dk = int(cand[order[int(torch.argmin(score))]])                      # the first of the smallest; all NaN: candidate 0
            delta[r, k] = dk
            p[k] = a[k] + dk
        pt = torch.from_numpy(p)
        u = _gather_ext(x2[r], (pt[1:, None] + j[None, :]).reshape(-1), n)
        v = _gather_ext(x2[r], (pt[:-1, None] + hs + j[None, :]).reshape(-1), n)
        w = win.double().repeat(K - 1)                                             # 1 - w is exact in float64
        out.append((w * u.double() + (1.0 - w) * v.double()).to(torch.float32)[:n_out])
    return torch.stack(out), delta


def _gather_ext(xr, idx, n):
    """xr[idx] with zeros where idx leaves [0, n)"""
    inside = (idx >= 0) & (idx < n)
    return torch.where(inside, xr[idx.clamp(0, n - 1)], torch.zeros((), dtype=xr.dtype))


def splice_rows_host(a, b, seed, draw, row0=0, **cut):
    """wm_splice restated in numpy: a (watermarked) and b (clean) float32 arrays (rows, n); `cut`: row_splice_spans's keywords.  Returns
    (y float32 (rows, n), labels bool (rows, n)): spans applied in rising j, so the largest active j that holds a sample decides it;
    y = b (original), +0 (silence) or b[(t + shift) mod n] (moved) there, and a elsewhere; samples are copied, never computed with."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.ndim != 2 or a.shape != b.shape or a.size == 0:
        raise ValueError(f"a and b: expected two (rows, n) arrays of one shape, got {a.shape} and {b.shape}")
    rows, n = a.shape
    y, labels = a.copy(), np.ones((rows, n), dtype=bool)
    for r, spans in enumerate(row_splice_spans(seed, draw, int(row0) + np.arange(rows), n, **cut)):
        for start, L, kind, shift, active in spans:
            if not active:
                continue
            t = np.arange(start, start + L)
            labels[r, t] = False
            y[r, t] = b[r, t] if kind == 0 else (np.float32(0.0) if kind == 1 else b[r, (t + shift) % n])
    return y, labels


def pack_labels(labels):
    """bool (rows, n) -> the mask layout, a uint32 array (rows, ceil(n / 32)): bit j of word w is sample 32 w + j, tail bits zero"""
    labels = np.asarray(labels, dtype=bool)
    if labels.ndim != 2:
        raise ValueError(f"labels: expected a (rows, n) array, got shape {labels.shape}")
    rows, n = labels.shape
    W = dsp.label_words(n)
    padded = np.zeros((rows, W * 32), dtype=np.uint64)
    padded[:, :n] = labels
    return (padded.reshape(rows, W, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def unpack_labels(lab, n):
    """the mask layout ((rows, ceil(n / 32)) uint32 / int32 array or tensor) -> bool array (rows, n)"""
    if isinstance(lab, torch.Tensor):
        lab = lab.detach().cpu().numpy()
    lab = np.ascontiguousarray(lab)
    if lab.ndim != 2 or lab.dtype not in (np.uint32, np.int32) or lab.shape[1] != dsp.label_words(n):
        raise ValueError(f"lab: expected a (rows, {dsp.label_words(n)}) uint32 or int32 mask for n = {n}, got {lab.dtype} {lab.shape}")
    words = lab.view(np.uint32)
    return (((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)) != 0).reshape(lab.shape[0], -1)[:, :int(n)]
