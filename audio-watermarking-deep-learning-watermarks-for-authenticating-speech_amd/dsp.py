"""The waveform ops: launch wrappers over the C ABI (include/wm_hip.h) that work on waveforms, rows and logits OUTSIDE the two models --
resampling and its adjoint, the biquad / 16-bit PCM codec, the channel distortions, the MDCT codec, FIR rows and RIR synthesis, time
warp, WSOLA, the LPC codec, STOI, splice / masked BCE / localisation counts, clip scores and clip features.

What is NOT here: the models' tape (ResBlock, stem, head, LSTM, embedding, ConvT7, PostprocFn, the spectral / BCE / L1 losses) and all of
its mutable host state live in ops.py.  This module imports nothing from ops; ops re-exports every name below, and `ops.<name>` stays
the public spelling.  The only state here is the caches of host and device tables.
"""
from __future__ import annotations

import collections
import math

import torch

from ._host import _chk, _chk_int, _chk_positive, _f32, _p, _seed64, _stream
from ._lib import lib

__all__ = [
    "RESAMPLE_LOWPASS_WIDTH", "RESAMPLE_ROLLOFF", "resample_length", "resample_table", "resample_tile_periods", "resample", "resample_add",
    "resample_adjoint_table", "resample_rows", "ResampleRowsFn",
    "BIQUAD_MODES", "BIQUAD_IDENTITY", "biquad_lowpass_coeffs", "biquad_warm", "biquad_plan", "biquad", "PcmCodecFn",
    "DistortFn",
    "MDCT_HOPS", "MDCT_BANDS", "MDCT_GRAD_MODES", "mdct_default_floor_step", "mdct_frames", "mdct_plan", "mdct_kcut", "mdct_codec", "MdctCodecFn",
    "FIR_MAX_TAPS", "fir_rows", "FirRowsFn", "rir_synth",
    "TIME_WARP_MAX_TABLE", "time_warp_table", "time_warp", "TimeWarpFn",
    "WSOLA_MAX_N", "wsola_window", "wsola_frames", "wsola", "WsolaFn",
    "LPC_FRAMES", "LPC_MAX_ORDER", "LPC_GRAD_MODES", "LPC_FLOOR_STEP", "lpc_tables", "lpc_frames", "lpc_codec", "LpcCodecFn",
    "stoi_plan", "stoi",
    "SPLICE_MAX_SPANS", "SPLICE_MAX_N", "label_words", "SpliceFn", "splice", "MaskedBCEFn", "loc_threshold_logit", "loc_counts",
    "CLIP_SCORES_MAX_T", "ClipScores", "clip_scores_plan", "clip_scores", "ClipFeaturesPlan", "clip_features_plan", "clip_features",
]

_ON_DEVICE = {}          # (key, str(device)) -> a family's host table(s) on that device: the one cache of device copies


def _on_device(key, device, make):
    """make()'s CPU tensor, or tuple of CPU tensors, on `device`; make runs for the first call alone.  `key` starts with the family's name"""
    k = (key, str(device))
    if k not in _ON_DEVICE:
        t = make()
        _ON_DEVICE[k] = t.to(device) if isinstance(t, torch.Tensor) else tuple(v.to(device) for v in t)
    return _ON_DEVICE[k]


# ---------------------------------------------------------------------------------------------- sample-rate conversion
# torchaudio.functional.resample with its documented defaults (resampling_method="sinc_interp_hann", lowpass_filter_width=6,
# rolloff=0.99), restated from the published description.  The reference resamples every file that is not at 16 kHz before a
# model sees it (py/main16.py:717-720).  The table is formed in float64 and rounded once to float32; the clamp of the filter
# argument makes every tap beyond +-6 zero crossings exactly 0.0, so only each phase's run of non-zero taps goes to the device.
RESAMPLE_LOWPASS_WIDTH = 6
RESAMPLE_ROLLOFF = 0.99
_RESAMPLE_HOST = {}      # (orig, new) -> table dict (CPU tensors)


def _resample_on(tab, key, device):
    """(taps, first) of the host table `tab` on the device; key: (orig, new), with "adjoint" behind them for the adjoint's table"""
    return _on_device(("resample",) + key, device, lambda: (tab["taps"], tab["first"]))


def _rate(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != int(v) or int(v) <= 0:
        raise ValueError(f"{name} must be a positive integer number of Hz, got {v!r}")
    return int(v)


def resample_length(n, orig_freq, new_freq):
    """ceil(new * n / orig): the number of samples torchaudio keeps for an input of n"""
    g = math.gcd(int(orig_freq), int(new_freq))
    P, Q = int(orig_freq) // g, int(new_freq) // g
    return -((-Q * int(n)) // P)


def resample_table(orig_freq, new_freq):
    """Host tables of one rate pair (cached): P, Q, width, K = 2*width + P, the dense float32 table `dense` (Q, K), and the compact
    one the kernel reads: `taps` (Q, W) with `first` (Q,) int32 such that dense[i, first[i]:first[i]+W] == taps[i] and every other
    entry of dense is 0.0.  W is the longest run of non-zero taps over the phases, made odd where K allows (LDS banks)."""
    orig_freq, new_freq = _rate(orig_freq, "orig_freq"), _rate(new_freq, "new_freq")
    key = (orig_freq, new_freq)
    if key in _RESAMPLE_HOST:
        return _RESAMPLE_HOST[key]
    g = math.gcd(orig_freq, new_freq)
    P, Q = orig_freq // g, new_freq // g
    if P == Q:       # equal rates: the identity as a one-tap table (only the segment padding of the kernel is used)
        tab = {"P": 1, "Q": 1, "width": 0, "K": 1, "W": 1, "dense": torch.ones(1, 1), "taps": torch.ones(1, 1),
               "first": torch.zeros(1, dtype=torch.int32)}
        _RESAMPLE_HOST[key] = tab
        return tab
    lpw = RESAMPLE_LOWPASS_WIDTH
    base = min(P, Q) * RESAMPLE_ROLLOFF
    width = int(math.ceil(lpw * P / base))
    K = 2 * width + P
    j = torch.arange(-width, width + P, dtype=torch.float64)[None, :] / P
    i = torch.arange(0, -Q, -1, dtype=torch.float64)[:, None] / Q
    t = ((i + j) * base).clamp_(-lpw, lpw)
    window = torch.cos(t * math.pi / lpw / 2) ** 2
    t = t * math.pi
    sinc = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t)
    dense = (sinc * (window * (base / P))).to(torch.float32)                   # (Q, K), the one rounding
    nz = dense != 0
    assert bool(nz.any(dim=1).all())
    idx = torch.arange(K)
    lo = torch.where(nz, idx, K).min(dim=1).values
    hi = torch.where(nz, idx, -1).max(dim=1).values
    W = int((hi - lo + 1).max())
    if W % 2 == 0 and W < K:
        W += 1
    first = torch.minimum(lo, torch.tensor(K - W)).to(torch.int32)
    taps = torch.stack([dense[q, int(first[q]):int(first[q]) + W] for q in range(Q)]).contiguous()
    tab = {"P": P, "Q": Q, "width": width, "K": K, "W": W, "dense": dense, "taps": taps, "first": first}
    _RESAMPLE_HOST[key] = tab
    return tab


def resample_tile_periods(orig_freq, new_freq):
    """output periods (Q samples each) one workgroup of the LDS kernel handles at a time; 0: the table does not fit LDS and the
    one-thread-per-sample kernel runs"""
    import ctypes
    tab = resample_table(orig_freq, new_freq)
    out = (ctypes.c_longlong * 1)()
    lib.wm_resample_plan(tab["P"], tab["Q"], tab["width"], tab["W"], ctypes.addressof(out), None)
    return int(out[0])


def resample(x, orig_freq, new_freq, seg_len=0, out=None):
    """Channel mean + sinc resampling of a CUDA waveform (C, N) or (N,) in one launch.  seg_len = 0: (1, L) with
    L = ceil(new * N / orig).  seg_len > 0: (S, 1, seg_len), S = ceil(L / seg_len), the tail of the last segment zero -- the
    Generator / Detector batch of the recording.  Equal rates with seg_len = 0 return x unchanged.  `out` (optional): a
    contiguous fp32 CUDA buffer of exactly the result's size to write into."""
    tab = resample_table(orig_freq, new_freq)
    seg_len = int(seg_len)
    if seg_len < 0:
        raise ValueError(f"seg_len must be >= 0, got {seg_len}")
    if isinstance(x, torch.Tensor) and x.dim() == 1:
        x = x.unsqueeze(0)
    x = _chk(x, "waveform", 2)
    if tab["K"] == 1 and seg_len == 0 and out is None:
        return x
    C, N = x.shape
    if C < 1:
        raise ValueError("waveform: needs at least one channel")
    L = -((-tab["Q"] * N) // tab["P"])
    S = -(-L // seg_len) if seg_len else 1
    total = S * seg_len if seg_len else L
    taps, first = _resample_on(tab, (int(orig_freq), int(new_freq)), x.device)
    if out is None:
        out = _f32(total, device=x.device)
    else:
        if not out.is_contiguous() or _chk(out, "out").numel() != total or out.device != x.device:
            raise ValueError(f"out: expected {total} floats on {x.device}, got {out.numel()} on {out.device}")
    lib.wm_resample(_p(x), _p(taps), _p(first), _p(out), C, N, tab["P"], tab["Q"], tab["width"], tab["W"], L, total, _stream())
    return out.view(S, 1, seg_len) if seg_len else out.view(1, L)


def resample_add(x, delta, orig_freq, delta_freq=16000, out=None, want_up=True):
    """The way back of the embed path in one launch: `delta` (at delta_freq) resampled to the recording's rate `orig_freq` and added to
    every channel of the recording `x` ((C, N) or (N,), fp32, CUDA).  `delta`: any contiguous fp32 CUDA tensor, read flat; its first
    n_d = resample_length(N, orig_freq, delta_freq) samples count, the rest is never read.  Returns (out (C, N), up (1, N) or None):
    up is ops.resample(delta[:n_d], delta_freq, orig_freq)[:, :N] bit for bit, out[c] = x[c] + up[0].  `out` (optional): a contiguous
    (C, N) fp32 buffer to write into; it may be x itself.  want_up=False: up is neither formed in memory nor returned."""
    tab = resample_table(delta_freq, orig_freq)
    inplace = out is x
    if isinstance(x, torch.Tensor) and x.dim() == 1:
        x = x.unsqueeze(0)                      # a view: an in-place sum still lands in the caller's (N,) tensor
    if isinstance(x, torch.Tensor) and x.dim() != 2:
        raise ValueError(f"waveform: expected (channels, samples) or (samples,), got shape {tuple(x.shape)}")
    if inplace and not x.is_contiguous():
        raise ValueError("out: an in-place sum needs a contiguous waveform")
    x = _chk(x, "waveform", 2)
    delta = _chk(delta, "delta")
    C, N = x.shape
    if C < 1:
        raise ValueError("waveform: needs at least one channel")
    n_d = resample_length(N, orig_freq, delta_freq)
    if delta.numel() < n_d:
        raise ValueError(f"delta: {N} samples at {orig_freq} Hz need {n_d} at {delta_freq} Hz, got {delta.numel()}")
    if delta.device != x.device:
        raise ValueError(f"delta: on {delta.device}, the waveform is on {x.device}")
    if out is None:
        out = _f32(C, N, device=x.device)
    elif inplace:
        out = x                                 # the (C, N) view of the caller's tensor
    elif (not out.is_contiguous() or tuple(_chk(out, "out").shape) != (C, N) or out.device != x.device):
        raise ValueError(f"out: expected a contiguous ({C}, {N}) buffer on {x.device}, got {tuple(out.shape)} on {out.device}")
    up = _f32(1, N, device=x.device) if want_up else None
    taps, first = _resample_on(tab, (int(delta_freq), int(orig_freq)), x.device)
    lib.wm_resample_add(_p(delta), _p(taps), _p(first), _p(x), _p(out), _p(up), C, N, n_d, tab["P"], tab["Q"], tab["width"], tab["W"],
                        _stream())
    return out, up


def resample_adjoint_table(orig_freq, new_freq):
    """Host table (cached) with which wm_resample_rows is the ADJOINT of the orig -> new resampler.  Write A for the (L, N) matrix of one
    row, A[m*Q + i][m*P + j - width] = dense[i][j].  Shifting the input index by P shifts the output index by Q with the same coefficients,
    so dx[n] = sum_o A[o][n] * dy[o] is itself a polyphase filter: P phases (n = m*P + p), stride Q through dy,
        dx[m*P + p] = sum_s c[p][s] * dy[m*Q + s],   c[p][s] = dense[s mod Q][-(s div Q)*P + p + width]   (0 outside dense),
    the float32 values of `dense` rearranged, nothing rounded again.  Returned in resample_table's layout with P' = Q, Q' = P:
    taps' (P, W') and first' (P,) int32 with taps'[p][k] = c[p][first'[p] + k - width'], every c outside that run exactly 0.0.
    width' is the smallest that keeps every run inside the K' = 2*width' + P' taps of a phase, so the kernels' clamp of first' to
    [0, 2*width' + P' - W'] moves no phase (asserted); W' is made odd where K' allows, as resample_table does."""
    orig_freq, new_freq = _rate(orig_freq, "orig_freq"), _rate(new_freq, "new_freq")
    key = (orig_freq, new_freq, "adjoint")
    if key in _RESAMPLE_HOST:
        return _RESAMPLE_HOST[key]
    tab = resample_table(orig_freq, new_freq)
    if tab["K"] == 1:                # equal rates: the identity is its own adjoint
        _RESAMPLE_HOST[key] = tab
        return tab
    P, Q, width, K, dense = tab["P"], tab["Q"], tab["width"], tab["K"], tab["dense"]
    # column j of dense belongs to the adjoint phase p = (j - width) mod P at the period offset d = (j - width - p) / P; its row i is s = i - d*Q
    nz = dense != 0
    rows = torch.arange(Q)[:, None]
    j = torch.arange(K)
    p_of = (j - width) % P
    d_of = (j - width - p_of) // P
    far = 1 << 40                                                             # beyond every s: a column without a non-zero tap never wins
    col_lo = torch.where(nz, rows, far).min(dim=0).values - d_of * Q          # (K,): lowest / highest s with a non-zero tap, per column
    col_hi = torch.where(nz, rows, -far).max(dim=0).values - d_of * Q
    lo = torch.full((P,), far, dtype=torch.int64).scatter_reduce(0, p_of, col_lo, "amin")
    hi = torch.full((P,), -far, dtype=torch.int64).scatter_reduce(0, p_of, col_hi, "amax")
    assert bool((lo <= hi).all()), "an input phase no output reads"
    Pa, Qa = Q, P
    wa = max(int(-lo.min()), int(hi.max()) - Pa + 1, 0)
    Ka = 2 * wa + Pa
    W = int((hi - lo + 1).max())
    if W % 2 == 0 and W < Ka:
        W += 1
    first = torch.minimum(lo + wa, torch.tensor(Ka - W))
    assert W <= Ka and int(first.min()) >= 0 and int(first.max()) <= 2 * wa + Pa - W, "the kernel would clamp a phase of the adjoint table"
    s = first[:, None] + torch.arange(W)[None, :] - wa                        # (P, W)
    i = s % Q
    jj = -((s - i) // Q) * P + torch.arange(P)[:, None] + width
    inside = (jj >= 0) & (jj < K)
    taps = torch.where(inside, dense[i, jj.clamp(0, K - 1)], torch.zeros(())).contiguous()
    assert int((taps != 0).sum()) == int(nz.sum()), "the adjoint table lost a tap"
    out = {"P": Pa, "Q": Qa, "width": wa, "K": Ka, "W": W, "taps": taps, "first": first.to(torch.int32)}
    _RESAMPLE_HOST[key] = out
    return out


def _resample_rows_launch(x, tab, dkey, L):
    rows, N = x.shape
    taps, first = _resample_on(tab, dkey, x.device)
    y = _f32(rows, L, device=x.device)
    lib.wm_resample_rows(_p(x), _p(taps), _p(first), _p(y), rows, N, L, tab["P"], tab["Q"], tab["width"], tab["W"], _stream())
    return y


def _rows_length(N, orig_freq, new_freq, length):
    full = resample_length(N, orig_freq, new_freq)
    if length is None:
        return full
    _chk_int(length, "length", 0, full, f"an int in [0, {full}] (what {N} samples give)")
    return length


def resample_rows(x, orig_freq, new_freq, length=None):
    """Sinc resampling of every row of a CUDA fp32 (rows, N) tensor by itself, one launch of wm_resample_rows: (rows, L) with
    L = resample_length(N, orig, new), or its first `length` samples.  No mixdown: row r is ops.resample(x[r:r+1], orig, new)[0] bit for
    bit.  Equal rates return x (x[:, :length] when cut)."""
    tab = resample_table(orig_freq, new_freq)
    x = _chk(x, "x", 2)
    L = _rows_length(x.shape[1], orig_freq, new_freq, length)
    if tab["K"] == 1:
        return x if L == x.shape[1] else x[:, :L]
    return _resample_rows_launch(x, tab, (int(orig_freq), int(new_freq)), L)


class ResampleRowsFn(torch.autograd.Function):
    """y = A x per row (resample_rows); dx = A^T dy, the same launch with resample_adjoint_table on (dy, rows, L -> N).  Nothing is saved
    but the rates and the lengths."""

    @staticmethod
    def forward(ctx, x, orig_freq, new_freq, length=None):
        ctx.rates, ctx.n = (int(orig_freq), int(new_freq)), x.shape[1]
        return resample_rows(x, orig_freq, new_freq, length)

    @staticmethod
    def backward(ctx, dy):
        orig, new = ctx.rates
        dy = _chk(dy, "dy", 2)
        tab = resample_adjoint_table(orig, new)
        if tab["K"] == 1:
            dx = torch.nn.functional.pad(dy, (0, ctx.n - dy.shape[1]))
        else:
            dx = _resample_rows_launch(dy, tab, (orig, new, "adjoint"), ctx.n)
        return dx, None, None, None


# ---------------------------------------------------------------------------------------------- biquad + 16-bit PCM codec
# The reference's 16-bit save path (py/main15.py:850-867: 7 kHz biquad low-pass -> clamp -> x32767 -> int16) and main15c's
# perceptual_postprocess (round(lowpass_biquad(x, 16000, 7000) * 32767) / 32767 on s_w inside the train / validation step) as one
# launch of wm_biquad.  The section is the RBJ cookbook low-pass torchaudio.functional.lowpass_biquad is published as.
BIQUAD_MODES = {"float": 0, "round": 1, "pcm16": 2}
BIQUAD_IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0)       # the quantiser alone
_BIQUAD_COEFFS = {}
_BIQUAD_PLAN = {}


def biquad_lowpass_coeffs(sample_rate, cutoff_freq, Q=0.707):
    """(b0, b1, b2, a1, a2) of the low-pass section exactly as inference.lowpass_biquad forms it: float64, divided by a0, each value
    rounded once to float32 (returned as Python floats that hold those float32 values).  Host-only, cached."""
    key = (sample_rate, cutoff_freq, Q)
    try:
        return _BIQUAD_COEFFS[key]
    except (KeyError, TypeError):
        pass
    for v, name in ((sample_rate, "sample_rate"), (cutoff_freq, "cutoff_freq"), (Q, "Q")):
        _chk_positive(v, name)
    if 2.0 * float(cutoff_freq) >= float(sample_rate):
        raise ValueError(f"cutoff_freq must lie below half the sample rate, got {cutoff_freq} Hz at {sample_rate} Hz")
    import numpy as np
    w0 = 2.0 * math.pi * float(cutoff_freq) / float(sample_rate)
    alpha = math.sin(w0) / (2.0 * float(Q))
    cw = math.cos(w0)
    b = np.array([(1.0 - cw) / 2.0, 1.0 - cw, (1.0 - cw) / 2.0], dtype=np.float64)
    a = np.array([1.0 + alpha, -2.0 * cw, 1.0 - alpha], dtype=np.float64)
    b32, a32 = (b / a[0]).astype(np.float32), (a / a[0]).astype(np.float32)
    out = (float(b32[0]), float(b32[1]), float(b32[2]), float(a32[1]), float(a32[2]))
    _BIQUAD_COEFFS[key] = out
    return out


def _biquad_coeffs(coeffs):
    import numpy as np
    try:
        c = tuple(float(v) for v in coeffs)
    except TypeError:
        raise ValueError(f"coeffs: expected (b0, b1, b2, a1, a2), got {coeffs!r}") from None
    if len(c) != 5 or not all(math.isfinite(v) and float(np.float32(v)) == v for v in c):
        raise ValueError(f"coeffs: expected five finite float32 values (b0, b1, b2, a1, a2), got {coeffs!r}")
    return c


def biquad_warm(coeffs):
    """the smallest W with r^W <= 2^-40, r the pole radius of 1 / (1 + a1 z^-1 + a2 z^-2): the warm-up after which a recursion started
    from a zero state has forgotten that (0 for a section without poles).  An unstable section (r >= 1) raises ValueError."""
    _, _, _, a1, a2 = _biquad_coeffs(coeffs)
    disc = a1 * a1 - 4.0 * a2
    r = math.sqrt(a2) if disc < 0 else (abs(a1) + math.sqrt(disc)) / 2.0
    if r >= 1.0:
        raise ValueError(f"coeffs: the section is not stable (pole radius {r})")
    if r == 0.0:
        return 0
    W = max(0, int(math.ceil(-40.0 * math.log(2.0) / math.log(r))) - 1)
    while r ** W > 2.0 ** -40:
        W += 1
    return W


def biquad_plan(coeffs):
    """(warm, chunk) wm_biquad runs this section with: the time-parallel kernel with chunks of `chunk` samples and biquad_warm(coeffs)
    samples of warm-up, or (-1, 0), one lane per row, where the library finds that warm-up too long.  A function of the coefficients alone."""
    import ctypes
    c = _biquad_coeffs(coeffs)
    if c not in _BIQUAD_PLAN:
        W = biquad_warm(c)
        out = (ctypes.c_int * 1)()
        lib.wm_biquad_plan(W, ctypes.addressof(out), None)
        _BIQUAD_PLAN[c] = (W, int(out[0])) if out[0] else (-1, 0)
    return _BIQUAD_PLAN[c]


def biquad(x, coeffs, *, clamp=True, mode="float", reverse=False, mask_out=False, mask_in=None, out=None):
    """Second-order section along the last axis of a contiguous fp32 CUDA tensor (all leading axes are rows, each from a zero state),
    one launch (wm_biquad).  mode "float": clamp(y, -1, 1) (clamp=False: y) | "round": round(clamp(y) * 32767) / 32767 | "pcm16": int16
    codes (clamp(y) * 32767).to(int16).  reverse: flip(filter(flip(x))), the adjoint.  mask_out: also returns the int32 bit mask of
    |y| <= 1 ((rows, ceil(n / 32)), bit t % 32 of word t / 32) as (out, mask).  mask_in: such a mask, applied to x on load.  `out`: a
    contiguous buffer of x's shape (int16 for "pcm16") that does not overlap x."""
    if mode not in BIQUAD_MODES:
        raise ValueError(f"mode must be one of {sorted(BIQUAD_MODES)}, got {mode!r}")
    if isinstance(x, torch.Tensor) and not x.is_cuda:
        raise ValueError(f"x: ops.biquad runs on the GPU only (got a {x.device} tensor); perceptual_postprocess / encode_pcm16 take CPU tensors")
    c = _biquad_coeffs(coeffs)
    x = _chk(x, "x")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"x: needs at least one row of at least one sample, got shape {tuple(x.shape)}")
    n = x.shape[-1]
    rows = x.numel() // n
    if mode == "pcm16" and not clamp:
        raise ValueError('mode "pcm16" needs clamp=True (the int16 cast is defined on [-1, 1] only)')
    if mask_out and reverse:
        raise ValueError("mask_out is not available with reverse=True")
    warm, _ = biquad_plan(c)
    odt = torch.int16 if mode == "pcm16" else torch.float32
    if out is None:
        out = torch.empty(x.shape, dtype=odt, device=x.device)
    else:
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != x.device or out.dtype != odt or \
                not out.is_contiguous() or out.shape != x.shape:
            raise ValueError(f"out: expected a contiguous {odt} buffer of shape {tuple(x.shape)} on {x.device}")
        xa, oa = x.data_ptr(), out.data_ptr()
        if xa < oa + out.numel() * out.element_size() and oa < xa + x.numel() * 4:
            raise ValueError("out: overlaps x (the filter reads x behind the samples it writes; in place is not supported)")
    nw = (n + 31) // 32
    if mask_in is not None:
        mask_in = _chk(mask_in, "mask_in", None, torch.int32)
        if mask_in.numel() != rows * nw or mask_in.device != x.device:
            raise ValueError(f"mask_in: expected {rows} x {nw} int32 words on {x.device}, got {mask_in.numel()} on {mask_in.device}")
    mask = torch.empty(rows, nw, dtype=torch.int32, device=x.device) if mask_out else None
    lib.wm_biquad(_p(x), _p(out), _p(mask), _p(mask_in), *c, rows, n, warm, BIQUAD_MODES[mode], int(bool(clamp)), int(bool(reverse)),
                  _stream())
    return (out, mask) if mask_out else out


class PcmCodecFn(torch.autograd.Function):
    """main15c's perceptual_postprocess, round(clamp(biquad(x)) * 32767) / 32767, on the tape.  grad "reference": the output is
    non-differentiable, as in torch (torch.round has a zero gradient, so nothing downstream of the codec reaches the Generator; marking
    it also spares the Detector an input gradient that would be multiplied by zero).  grad "straight_through" (no counterpart in the
    reference): the rounding passes the gradient unchanged, the clamp where its saved bit is set, the filter through its adjoint --
    one reverse launch with mask_in."""

    @staticmethod
    def forward(ctx, x, coeffs, grad):
        if grad not in ("reference", "straight_through"):
            raise ValueError(f'grad must be "reference" or "straight_through", got {grad!r}')
        ctx.coeffs = coeffs
        if grad == "reference" or not ctx.needs_input_grad[0]:
            out = biquad(x, coeffs, mode="round")
            ctx.mark_non_differentiable(out)
            ctx.st = False
            return out
        out, mask = biquad(x, coeffs, mode="round", mask_out=True)
        ctx.save_for_backward(mask)
        ctx.st = True
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.st:
            return None, None, None
        (mask,) = ctx.saved_tensors
        return biquad(g.contiguous(), ctx.coeffs, clamp=False, reverse=True, mask_in=mask), None, None


# ---------------------------------------------------------------------------------------------- channel distortions
class DistortFn(torch.autograd.Function):
    """wm_distort on the tape: y = g_r x + s_r z per row of a contiguous fp32 CUDA tensor (all leading axes are rows), with the row's gain,
    SNR and noise coin drawn in the kernel from (seed, draw, row0 + r).  bounds = (gain_lo, gain_hi, snr_lo, snr_hi, p_noise).  Returns
    (y, stat), stat (rows, 4) = {g_r, s_r, ms_r, snr_db_r or inf}, not differentiable.  Saved for the backward: x and stat -- never the
    noise, which wm_distort_bwd regenerates from the same counters.  through: the noise level s_r takes part in the gradient."""

    @staticmethod
    def _scratch(rows, n, device):
        import ctypes
        need = ctypes.c_longlong(0)
        lib.wm_distort_plan(rows, n, ctypes.addressof(need), None)
        return _f32(need.value, device=device)

    @staticmethod
    def forward(ctx, x, bounds, seed, draw, row0, through):
        x = _chk(x, "x")
        if x.dim() < 1 or x.numel() == 0:
            raise ValueError(f"x: needs at least one row of at least one sample, got shape {tuple(x.shape)}")
        n = x.shape[-1]
        rows = x.numel() // n
        ctx.key = (rows, n, int(row0), _seed64(seed), int(draw))
        ctx.through = bool(through)
        y, stat = torch.empty_like(x), _f32(rows, 4, device=x.device)
        lib.wm_distort(_p(x), _p(y), _p(stat), _p(DistortFn._scratch(rows, n, x.device)), *ctx.key, *map(float, bounds), _stream())
        ctx.save_for_backward(x, stat)
        ctx.mark_non_differentiable(stat)
        return y, stat

    @staticmethod
    def backward(ctx, g, _gstat):
        x, stat = ctx.saved_tensors
        g = _chk(g, "grad")
        dx = torch.empty_like(x)
        lib.wm_distort_bwd(_p(g), _p(x), _p(stat), _p(dx), _p(DistortFn._scratch(*ctx.key[:2], x.device)), *ctx.key, int(ctx.through),
                           _stream())
        return dx, None, None, None, None, None


# ---------------------------------------------------------------------------------------------- transform-codec stand-in
# Lapped MDCT -> per-band quantiser -> bandwidth cut -> synthesis (wm_mdct_codec, csrc/mdct_codec.hip): the signal path lossy codecs share,
# as a step of the graph.  A stand-in for compression, not an MP3 / AAC encoder: parity with a real encoder is unmeasured.
MDCT_HOPS = (128, 256, 512)
MDCT_BANDS = (4, 8, 16, 32)
MDCT_GRAD_MODES = ("straight_through", "dead_zone")


def mdct_default_floor_step(hop):
    """2^-15 * sqrt(hop / 2): the coefficient step whose time-domain noise equals the 16-bit grid's (synthesis scales coefficient variance
    by 2 / hop)"""
    return 2.0 ** -15 * math.sqrt(hop / 2.0)


def mdct_frames(n, hop):
    """F = ceil(n / hop) + 1: the frames of a row of n samples"""
    return -(-int(n) // int(hop)) + 1


def mdct_plan(n, hop):
    """(frames a workgroup transforms, workgroups per row) wm_mdct_codec runs a row of n samples with: a function of (n, hop) alone"""
    import ctypes
    frames, wgs = ctypes.c_int(0), ctypes.c_longlong(0)
    lib.wm_mdct_codec_plan(int(n), int(hop), ctypes.addressof(frames), ctypes.addressof(wgs), None)
    return frames.value, wgs.value


def mdct_kcut(hop, band, bandwidth_hz=None, sample_rate=16000):
    """The first coefficient the bandwidth cut zeroes: floor(bandwidth_hz * 2 hop / sample_rate) rounded down to a multiple of `band`
    (coefficient k sits at (k + 1/2) sample_rate / (2 hop) Hz); None: hop, no cut.  A cut below one band, or above Nyquist, is refused."""
    if hop not in MDCT_HOPS:
        raise ValueError(f"hop must be one of {MDCT_HOPS}, got {hop!r}")
    if band not in MDCT_BANDS:
        raise ValueError(f"band must be one of {MDCT_BANDS}, got {band!r}")
    if bandwidth_hz is None:
        return hop
    for v, name in ((bandwidth_hz, "bandwidth_hz"), (sample_rate, "sample_rate")):
        _chk_positive(v, name)
    if 2.0 * bandwidth_hz > sample_rate:
        raise ValueError(f"bandwidth_hz must not lie above half the sample rate, got {bandwidth_hz} Hz at {sample_rate} Hz")
    kcut = int(math.floor(bandwidth_hz * 2 * hop / sample_rate)) // band * band
    if kcut < band:
        raise ValueError(f"bandwidth_hz {bandwidth_hz} Hz keeps less than one band of {band} coefficients at hop {hop}")
    return kcut


def mdct_codec(x, snr_db, *, hop=256, band=8, kcut=None, bandwidth_hz=None, sample_rate=16000, floor_step=None, quantise=True,
               codes_out=False, mask_in=None):
    """One launch of wm_mdct_codec along the last axis of a contiguous fp32 CUDA tensor (all leading axes are rows): MDCT analysis at hop
    `hop`, coefficients k >= kcut (given, or mdct_kcut(hop, band, bandwidth_hz, sample_rate); neither: hop, no cut) and those where mask_in
    holds 0 set to zero, the per-band quantiser at the per-row SNR snr_db
    (a (rows,) fp32 CUDA tensor, values in [0, 60]; ignored with quantise=False, where None is allowed) with floor_step (None:
    mdct_default_floor_step(hop)), synthesis with overlap-add.  codes_out: also returns the int16 codes, (rows, mdct_frames(n, hop), hop),
    as (y, codes).  mask_in: an int16 tensor of that shape.  A stand-in for lossy compression; parity with MP3 / AAC is unmeasured."""
    x = _chk(x, "x")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"x: needs at least one row of at least one sample, got shape {tuple(x.shape)}")
    if kcut is not None and bandwidth_hz is not None:
        raise ValueError("give kcut or bandwidth_hz, not both")
    derived = mdct_kcut(hop, band, bandwidth_hz, sample_rate)                    # hop and band from their sets
    if kcut is None:
        kcut = derived
    if isinstance(kcut, bool) or not isinstance(kcut, int) or kcut % band or not band <= kcut <= hop:
        raise ValueError(f"kcut: expected a multiple of band = {band} in [{band}, {hop}], got {kcut!r}")
    if floor_step is None:
        floor_step = mdct_default_floor_step(hop)
    _chk_positive(floor_step, "floor_step")
    if codes_out and not quantise:
        raise ValueError("codes_out needs quantise=True: the linear map has no codes")
    n = x.shape[-1]
    rows = x.numel() // n
    F = mdct_frames(n, hop)
    if snr_db is None and not quantise:
        snr_db = torch.zeros(rows, dtype=torch.float32, device=x.device)
    snr_db = _chk(snr_db, "snr_db", 1)
    if snr_db.shape[0] != rows or snr_db.device != x.device:
        raise ValueError(f"snr_db: expected {rows} values on {x.device}, got shape {tuple(snr_db.shape)} on {snr_db.device}")
    if mask_in is not None:
        mask_in = _chk(mask_in, "mask_in", None, torch.int16)
        if mask_in.numel() != rows * F * hop or mask_in.device != x.device:
            raise ValueError(f"mask_in: expected {rows} x {F} x {hop} int16 values on {x.device}, got shape {tuple(mask_in.shape)}")
    y = torch.empty_like(x)
    codes = torch.empty(rows, F, hop, dtype=torch.int16, device=x.device) if codes_out else None
    lib.wm_mdct_codec(_p(x), _p(y), _p(codes), _p(mask_in), _p(snr_db), rows, n, hop, band, kcut, float(floor_step), int(bool(quantise)),
                      _stream())
    return (y, codes) if codes_out else y


class MdctCodecFn(torch.autograd.Function):
    """y = synthesis(Q(cut(analysis(x)))) per row (mdct_codec) on the tape.  With the quantiser off the map A = synthesis . cut . analysis is
    symmetric, so the backward is the same launch with quantise=False on dy:
      grad "straight_through": dx = A dy -- the quantiser is taken for the identity, the bandwidth cut is kept, nothing is saved;
      grad "dead_zone":        dx = A_mask dy -- coefficients whose forward code was 0 pass no gradient; the forward's int16 codes are saved
                               and handed to the backward launch as mask_in.
    The step follows the band's own energy and so depends on x; that dependence is NOT differentiated (the step is a constant of the
    backward pass, as the rounding is)."""

    @staticmethod
    def forward(ctx, x, snr_db, hop, band, kcut, floor_step, grad):
        if grad not in MDCT_GRAD_MODES:
            raise ValueError(f"grad must be one of {MDCT_GRAD_MODES}, got {grad!r}")
        ctx.cfg = (hop, band, kcut, floor_step)
        ctx.dead = grad == "dead_zone" and ctx.needs_input_grad[0]
        if ctx.dead:
            y, codes = mdct_codec(x, snr_db, hop=hop, band=band, kcut=kcut, floor_step=floor_step, codes_out=True)
            ctx.save_for_backward(codes)
            return y
        return mdct_codec(x, snr_db, hop=hop, band=band, kcut=kcut, floor_step=floor_step)

    @staticmethod
    def backward(ctx, g):
        hop, band, kcut, floor_step = ctx.cfg
        mask = ctx.saved_tensors[0] if ctx.dead else None
        dx = mdct_codec(g.contiguous(), None, hop=hop, band=band, kcut=kcut, floor_step=floor_step, quantise=False, mask_in=mask)
        return dx, None, None, None, None, None, None


# ---------------------------------------------------------------------------------------------- reverb / echo
# Per-row causal FIR convolution (wm_fir_rows, csrc/fir_rows.hip) and synthetic room responses (wm_rir_synth, csrc/distort.hip): the long
# convolutive channel as a step of the graph.
FIR_MAX_TAPS = 16384


def _fir_taps(h, rows, device):
    h = _chk(h, "h")
    if h.dim() not in (1, 2) or h.shape[-1] < 1 or h.shape[-1] > FIR_MAX_TAPS:
        raise ValueError(f"h: expected (K,) or (rows, K) with 1 <= K <= {FIR_MAX_TAPS}, got shape {tuple(h.shape)}")
    if h.dim() == 2 and h.shape[0] != rows:
        raise ValueError(f"h: expected one response, or one per row ({rows}), got shape {tuple(h.shape)}")
    if h.device != device:
        raise ValueError(f"h: expected a tensor on {device}, got one on {h.device}")
    return h


def fir_rows(x, h, reverse=False):
    """One launch of wm_fir_rows along the last axis of a contiguous fp32 CUDA tensor (all leading axes are rows):
    y[r][t] = sum_k h_r[k] x[r][t - k], the first n samples of the full convolution, every row from silence; h is (K,), one response for
    all rows, or (rows, K), one per row.  reverse=True: y[r][t] = sum_k h_r[k] x[r][t + k], the transposed map (the backward pass)."""
    x = _chk(x, "x")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"x: needs at least one row of at least one sample, got shape {tuple(x.shape)}")
    n = x.shape[-1]
    rows = x.numel() // n
    h = _fir_taps(h, rows, x.device)
    K = h.shape[-1]
    y = torch.empty_like(x)
    lib.wm_fir_rows(_p(x), _p(h), _p(y), rows, n, K, K if h.dim() == 2 else 0, int(bool(reverse)), _stream())
    return y


class FirRowsFn(torch.autograd.Function):
    """y = H x per row (fir_rows) on the tape.  Saved for the backward: h alone; dx = H^T dy is the same launch with reverse=True.  h is a
    CONSTANT of the graph: no gradient flows to it (a response is measured or drawn, not trained)."""

    @staticmethod
    def forward(ctx, x, h):
        y = fir_rows(x, h)
        ctx.save_for_backward(h)
        return y

    @staticmethod
    def backward(ctx, g):
        return fir_rows(g.contiguous(), ctx.saved_tensors[0], reverse=True), None


def rir_synth(params, taps, sample_rate=16000, seed=0, draw=0, row0=0):
    """One launch of wm_rir_synth: (rows, taps) fp32 synthetic room responses from params, a (rows, 2) fp32 CUDA tensor of {rt60 in seconds,
    direct-to-reverberant ratio in dB} per row -- exponentially decaying Gaussian noise behind a direct tap, unit energy, NOT a room
    simulation.  Row r is a function of (seed, draw, row0 + r, params[r], taps, sample_rate) alone."""
    params = _chk(params, "params", 2)
    if params.shape[0] < 1 or params.shape[1] != 2:
        raise ValueError(f"params: expected (rows, 2) with at least one row, got shape {tuple(params.shape)}")
    _chk_int(taps, "taps", 1, FIR_MAX_TAPS)
    _chk_positive(sample_rate, "sample_rate")
    rows = params.shape[0]
    _chk_int(draw, "draw", 0, 2 ** 32 - 1)
    _chk_int(row0, "row0", 0, 2 ** 32 - rows)
    h = _f32(rows, taps, device=params.device)
    lib.wm_rir_synth(_p(params), _p(h), rows, taps, float(sample_rate), row0, _seed64(seed), draw, _stream())
    return h


# ---------------------------------------------------------------------------------------------- speed change / wow and flutter
# Time warp through a windowed-sinc interpolator (wm_time_warp, csrc/time_warp.hip): the output reads the input at a position that
# advances `speed` samples per sample, wobbles sinusoidally and starts a cut in.  The desynchronising channel as a step of the graph.
TIME_WARP_MAX_TABLE = 128 * 1024 // 4           # floats


def _time_warp_dims(zeros, res):
    _chk_int(zeros, "zeros", 4, 32)
    _chk_int(res, "res", 64, 1024)
    if res & (res - 1):
        raise ValueError(f"res: expected a power of two, got {res}")
    if zeros * res + 2 > TIME_WARP_MAX_TABLE:
        raise ValueError(f"zeros * res + 2 = {zeros * res + 2} floats is above the {TIME_WARP_MAX_TABLE} (128 KiB) a table may take")


_TIME_WARP_HOST = {}     # (zeros, res) -> the table (a CPU tensor)


def time_warp_table(zeros=16, res=512):
    """The interpolator's half response, a (zeros * res + 2,) fp32 CPU tensor (cached; do not write to it): sinc(v) * 0.5 (1 + cos(pi v /
    zeros)) at v = i / res, a Hann-windowed sinc with `zeros` zero crossings at `res` points each, computed in float64.  Entry 0 is exactly
    1, the entries at the other multiples of res and the last two exactly 0, so that a whole-sample shift is the identity."""
    _time_warp_dims(zeros, res)
    if (zeros, res) not in _TIME_WARP_HOST:
        import numpy as np
        v = np.arange(zeros * res + 2, dtype=np.float64) / res
        tab = np.sinc(v) * 0.5 * (1.0 + np.cos(np.pi * v / zeros))
        tab[res::res] = 0.0                      # the zero crossings, exactly
        tab[0] = 1.0
        tab[-2:] = 0.0
        _TIME_WARP_HOST[(zeros, res)] = torch.from_numpy(tab.astype(np.float32))
    return _TIME_WARP_HOST[(zeros, res)]


def _time_warp_table_on(zeros, res, device):
    return _on_device(("time_warp", zeros, res), device, lambda: time_warp_table(zeros, res))


def time_warp(x, params, table=None, adjoint=False, zeros=16, res=512):
    """One launch of wm_time_warp along the last axis of a contiguous fp32 CUDA tensor (all leading axes are rows):
    y[r][t] = sum_k W(p_r(t) - k) x[r][k] with p_r(t) = a t + off + d sinpi(2 frac(w t + phi)) from params, a (rows, 6) fp32 CUDA tensor of
    {a, off, d, w, phi, c} per row, and W the table's interpolated value at cutoff c (include/wm_hip.h has the definition).  table: the
    (zeros * res + 2,) fp32 half response, None for time_warp_table(zeros, res).  adjoint=True: the transposed map (the backward pass),
    defined for increasing p."""
    x = _chk(x, "x")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"x: needs at least one row of at least one sample, got shape {tuple(x.shape)}")
    n = x.shape[-1]
    rows = x.numel() // n
    _time_warp_dims(zeros, res)
    params = _chk(params, "params", 2)
    if tuple(params.shape) != (rows, 6):
        raise ValueError(f"params: expected ({rows}, 6), one {{a, off, d, w, phi, c}} per row, got shape {tuple(params.shape)}")
    table = _time_warp_table_on(zeros, res, x.device) if table is None else _chk(table, "table", 1)
    if table.shape[0] != zeros * res + 2:
        raise ValueError(f"table: expected zeros * res + 2 = {zeros * res + 2} values, got shape {tuple(table.shape)}")
    for t, name in ((params, "params"), (table, "table")):
        if t.device != x.device:
            raise ValueError(f"{name}: expected a tensor on {x.device}, got one on {t.device}")
    y = torch.empty_like(x)
    lib.wm_time_warp(_p(x), _p(params), _p(table), _p(y), rows, n, zeros, res, int(bool(adjoint)), _stream())
    return y


class TimeWarpFn(torch.autograd.Function):
    """y = W x per row (time_warp) on the tape.  Saved for the backward: params and the table alone; dx = W^T dy is the same launch with
    adjoint=True.  params and the table are CONSTANTS of the graph: no gradient flows to them (a speed is drawn, not trained)."""

    @staticmethod
    def forward(ctx, x, params, table, zeros, res):
        y = time_warp(x, params, table, zeros=zeros, res=res)
        ctx.save_for_backward(params, table)
        ctx.dims = (zeros, res)
        return y

    @staticmethod
    def backward(ctx, g):
        params, table = ctx.saved_tensors
        return time_warp(g.contiguous(), params, table, adjoint=True, zeros=ctx.dims[0], res=ctx.dims[1]), None, None, None, None


# ---------------------------------------------------------------------------------------------- pitch-preserving time stretch
# Waveform-similarity overlap-add (wm_wsola, csrc/wsola.hip): frames of the input copied to evenly spaced places of the output, each
# taken near its nominal place where it continues the one before best.  Given the chosen positions the map is a linear gather, so the
# backward pass is exact with the positions held constant.
WSOLA_MAX_N = 2 ** 30


def _wsola_dims(L, S):
    _chk_int(L, "L", 64, 1024)
    if L & (L - 1):
        raise ValueError(f"L: expected a power of two, got {L}")
    _chk_int(S, "S", 1, L // 2)


_WSOLA_HOST = {}         # L -> the rising half window (a CPU tensor)


def wsola_window(L=512):
    """The rising half of the frame's Hann window, an (L / 2,) fp32 CPU tensor (cached; do not write to it): 0.5 - 0.5 cos(pi j / Hs),
    Hs = L / 2, computed in float64.  Entry 0 is exactly 0, so a frame that continues its predecessor hands the samples on bit for bit."""
    _wsola_dims(L, 1)
    if L not in _WSOLA_HOST:
        import numpy as np
        hs = L // 2
        w = 0.5 - 0.5 * np.cos(np.pi * np.arange(hs, dtype=np.float64) / hs)
        w[0] = 0.0
        _WSOLA_HOST[L] = torch.from_numpy(w.astype(np.float32))
    return _WSOLA_HOST[L]


def _wsola_window_on(L, device):
    return _on_device(("wsola", L), device, lambda: wsola_window(L))


def wsola_frames(n_out, L=512):
    """K, the frames of a row of n_out output samples: ceil(n_out / Hs) + 1"""
    return -(-n_out // (L // 2)) + 1


def wsola(x, rate, n_out=None, delta=None, adjoint=False, L=512, S=128):
    """One launch of wm_wsola along the last axis of a contiguous fp32 CUDA tensor (all leading axes are rows; include/wm_hip.h has the
    definition).  rate: (rows,) fp32 CUDA tensor, input samples consumed per output sample; a row whose rate is outside [1/4, 4] comes
    back as zeros.  n_out: the length of the result's last axis, None for that of x.
    delta=None: the search (mode 0); returns (y, delta), delta the (rows, K) int32 offsets of the chosen positions, K = wsola_frames(n_out, L).
    delta given: synthesis from these offsets (mode 1), clamped to [-S, S]; returns (y, delta).
    adjoint=True (delta is needed): x is the gradient of a result of x's length, and the transposed map of mode 1 comes back, dx with
    n_out samples a row -- here n_out is the FORWARD call's input length."""
    x = _chk(x, "x")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"x: needs at least one row of at least one sample, got shape {tuple(x.shape)}")
    n = x.shape[-1]
    rows = x.numel() // n
    _wsola_dims(L, S)
    n_res = _chk_int(n if n_out is None else n_out, "n_out", 1, WSOLA_MAX_N)
    if n > WSOLA_MAX_N or rows * max(n, n_res) > 2 ** 46:
        raise ValueError(f"rows = {rows}, n = {n}, n_out = {n_res}: a row may have 2^30 samples and a launch 2^46")
    rate = _chk(rate, "rate", 1)
    if rate.shape[0] != rows:
        raise ValueError(f"rate: expected ({rows},), one per row, got shape {tuple(rate.shape)}")
    if adjoint and delta is None:
        raise ValueError("delta: the adjoint needs the positions of the forward call")
    K = wsola_frames(n if adjoint else n_res, L)
    if delta is not None:
        delta = _chk(delta, "delta", 2, torch.int32)
        if tuple(delta.shape) != (rows, K):
            raise ValueError(f"delta: expected ({rows}, {K}), one offset per frame, got shape {tuple(delta.shape)}")
    for t, name in ((rate, "rate"), (delta, "delta")):
        if t is not None and t.device != x.device:
            raise ValueError(f"{name}: expected a tensor on {x.device}, got one on {t.device}")
    mode = 2 if adjoint else (0 if delta is None else 1)
    if delta is None:
        delta = torch.empty((rows, K), dtype=torch.int32, device=x.device)
    y = _f32(*x.shape[:-1], n_res, device=x.device)
    n_in, n_o = (n_res, n) if adjoint else (n, n_res)
    lib.wm_wsola(_p(x), _p(rate), _p(_wsola_window_on(L, x.device)), _p(y), _p(delta), rows, n_in, n_o, L, S, mode, _stream())
    return y if adjoint else (y, delta)


class WsolaFn(torch.autograd.Function):
    """y, delta = wsola(x, rate, n_out) on the tape.  Saved for the backward: delta and rate alone; dx is the mode-2 launch on them.  The
    positions are CONSTANTS of the graph: the map is differentiated as the linear gather it is once they are chosen, and no gradient
    flows to the rate (it is drawn, not trained)."""

    @staticmethod
    def forward(ctx, x, rate, n_out, L, S):
        y, delta = wsola(x, rate, n_out, L=L, S=S)
        ctx.save_for_backward(delta, rate)
        ctx.dims = (x.shape, L, S)
        ctx.mark_non_differentiable(delta)
        return y, delta

    @staticmethod
    def backward(ctx, g, _):
        delta, rate = ctx.saved_tensors
        shape, L, S = ctx.dims
        dx = wsola(g.contiguous(), rate, shape[-1], delta, adjoint=True, L=L, S=S)
        return dx.reshape(shape), None, None, None, None


# ---------------------------------------------------------------------------------------------- predictive speech-codec stand-in
# Per-frame linear prediction -> open-loop quantiser on the residual -> all-pole synthesis (wm_lpc_codec, csrc/lpc_codec.hip): the signal
# path ADPCM / CELP / AMR-WB / SILK share, as a step of the graph.  A stand-in, not a speech codec: no LSP interpolation, no pitch
# predictor, no noise feedback, no entropy coder; parity with a real one is unmeasured.
LPC_FRAMES = (160, 320, 640)
LPC_MAX_ORDER = 16
LPC_GRAD_MODES = ("straight_through", "dead_zone")
LPC_FLOOR_STEP = 2.0 ** -15

_LPC_HOST = {}           # (order, sample_rate) -> (lag, expand), CPU tensors


def _lpc_dims(frame, order):
    if isinstance(frame, bool) or not isinstance(frame, int) or frame not in LPC_FRAMES:
        raise ValueError(f"frame must be one of {LPC_FRAMES}, got {frame!r}")
    _chk_int(order, "order", 2, LPC_MAX_ORDER)


def lpc_tables(order=16, sample_rate=16000):
    """(lag, expand), fp32 CPU tensors (cached; do not write to them), evaluated in float64 and rounded once.  lag (order + 1,): the lag
    window the autocorrelation is multiplied by, exp(-0.5 (2 pi 60 k / sample_rate)^2) -- a 60 Hz Gaussian -- with lag[0] = 1 + 1e-4, the
    white-noise correction.  expand (order,): 0.994^k for k = 1 .. order, the bandwidth expansion of the coefficients."""
    _chk_int(order, "order", 2, LPC_MAX_ORDER)
    _chk_positive(sample_rate, "sample_rate")
    key = (order, float(sample_rate))
    if key not in _LPC_HOST:
        import numpy as np
        k = np.arange(order + 1, dtype=np.float64)
        lag = np.exp(-0.5 * (2.0 * np.pi * 60.0 * k / float(sample_rate)) ** 2)
        lag[0] = 1.0 + 1e-4
        expand = 0.994 ** k[1:]
        _LPC_HOST[key] = (torch.from_numpy(lag.astype(np.float32)), torch.from_numpy(expand.astype(np.float32)))
    return _LPC_HOST[key]


def _lpc_tables_on(order, sample_rate, device):
    return _on_device(("lpc", order, float(sample_rate)), device, lambda: lpc_tables(order, sample_rate))


def lpc_frames(n, frame=320):
    """F = ceil(n / frame): the frames of a row of n samples"""
    return -(-int(n) // int(frame))


def lpc_codec(x, snr_db, *, frame=320, order=16, sample_rate=16000, floor_step=None, quantise=True, coeffs=None, coeffs_out=False,
              codes_out=False, mask_in=None, adjoint=False):
    """One launch of wm_lpc_codec along the last axis of a contiguous fp32 CUDA tensor (all leading axes are rows; include/wm_hip.h has the
    definition): per frame of `frame` samples an order-`order` predictor from the windowed autocorrelation (lpc_tables(order,
    sample_rate) are its lag window and bandwidth expansion), the residual quantised at the per-row SNR snr_db (a (rows,) fp32 CUDA
    tensor, values in [0, 60]; ignored with quantise=False, where None is allowed) but never finer than floor_step (None: 2^-15), and
    all-pole synthesis.  coeffs: a (rows, lpc_frames(n, frame), order) fp32 tensor that replaces the analysis.  mask_in: a (rows, n) int16
    tensor; the residual is set to 0 where it holds 0.  coeffs_out / codes_out: also return the coefficients the launch used / the int16
    codes (rows, n); the result is then the tuple (y[, coeffs][, codes]).  adjoint=True (needs coeffs, quantise=False): x is a gradient
    and the transpose of the linear map synthesis . mask . residual filter at these coefficients comes back.  A stand-in for a speech
    codec; parity with a real one is unmeasured."""
    x = _chk(x, "x")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"x: needs at least one row of at least one sample, got shape {tuple(x.shape)}")
    _lpc_dims(frame, order)
    if floor_step is None:
        floor_step = LPC_FLOOR_STEP
    _chk_positive(floor_step, "floor_step")
    if codes_out and not quantise:
        raise ValueError("codes_out needs quantise=True: the linear map has no codes")
    if adjoint and (coeffs is None or quantise or coeffs_out or codes_out):
        raise ValueError("adjoint: needs coeffs and quantise=False, and has neither coeffs_out nor codes_out")
    n = x.shape[-1]
    rows = x.numel() // n
    if n > 2 ** 34 or rows * n > 2 ** 46:
        raise ValueError(f"rows = {rows}, n = {n}: a row may have 2^34 samples and a launch 2^46")
    F = lpc_frames(n, frame)
    if snr_db is None and not quantise:
        snr_db = torch.zeros(rows, dtype=torch.float32, device=x.device)
    snr_db = _chk(snr_db, "snr_db", 1)
    if snr_db.shape[0] != rows:
        raise ValueError(f"snr_db: expected ({rows},), one per row, got shape {tuple(snr_db.shape)}")
    if coeffs is not None:
        coeffs = _chk(coeffs, "coeffs")
        if coeffs.numel() != rows * F * order or coeffs.shape[-1] != order:
            raise ValueError(f"coeffs: expected {rows} x {F} x {order} fp32 values, got shape {tuple(coeffs.shape)}")
    if mask_in is not None:
        mask_in = _chk(mask_in, "mask_in", None, torch.int16)
        if mask_in.numel() != rows * n:
            raise ValueError(f"mask_in: expected {rows} x {n} int16 values, got shape {tuple(mask_in.shape)}")
    for t, name in ((snr_db, "snr_db"), (coeffs, "coeffs"), (mask_in, "mask_in")):
        if t is not None and t.device != x.device:
            raise ValueError(f"{name}: expected a tensor on {x.device}, got one on {t.device}")
    lag, expand = _lpc_tables_on(order, sample_rate, x.device)
    y = torch.empty_like(x)
    used = torch.empty(rows, F, order, dtype=torch.float32, device=x.device) if coeffs_out else None
    codes = torch.empty(rows, n, dtype=torch.int16, device=x.device) if codes_out else None
    lib.wm_lpc_codec(_p(x), _p(y), _p(coeffs), _p(used), _p(codes), _p(mask_in), _p(snr_db), _p(lag), _p(expand), rows, n, frame, order,
                     float(floor_step), int(bool(quantise)), int(bool(adjoint)), _stream())
    out = (y,) + ((used,) if coeffs_out else ()) + ((codes,) if codes_out else ())
    return out if len(out) > 1 else y


class LpcCodecFn(torch.autograd.Function):
    """y = synthesis(Q(residual(x))) per row (lpc_codec) on the tape.  The coefficients and the steps follow x, and that dependence is
    NOT differentiated: they are constants of the backward pass, as the MDCT codec's steps and WSOLA's positions are.
      grad "straight_through": with the quantiser taken for the identity, synthesis inverts the residual filter exactly, so the map is the
                               identity and the gradient IS dy: no launch, nothing saved;
      grad "dead_zone":        residual samples whose forward code was 0 pass no gradient: the forward's coefficients and int16 codes
                               are saved, and dx is the adjoint launch at those coefficients with the codes as mask_in."""

    @staticmethod
    def forward(ctx, x, snr_db, frame, order, sample_rate, floor_step, grad):
        if grad not in LPC_GRAD_MODES:
            raise ValueError(f"grad must be one of {LPC_GRAD_MODES}, got {grad!r}")
        ctx.cfg = (frame, order, sample_rate, floor_step)
        ctx.dead = grad == "dead_zone" and ctx.needs_input_grad[0]
        if ctx.dead:
            y, coeffs, codes = lpc_codec(x, snr_db, frame=frame, order=order, sample_rate=sample_rate, floor_step=floor_step,
                                         coeffs_out=True, codes_out=True)
            ctx.save_for_backward(coeffs, codes)
            return y
        return lpc_codec(x, snr_db, frame=frame, order=order, sample_rate=sample_rate, floor_step=floor_step)

    @staticmethod
    def backward(ctx, g):
        if not ctx.dead:
            return g, None, None, None, None, None, None
        frame, order, sample_rate, floor_step = ctx.cfg
        coeffs, codes = ctx.saved_tensors
        dx = lpc_codec(g.contiguous(), None, frame=frame, order=order, sample_rate=sample_rate, floor_step=floor_step, quantise=False,
                       coeffs=coeffs, mask_in=codes, adjoint=True)
        return dx.reshape(g.shape), None, None, None, None, None, None


# ---------------------------------------------------------------------------------------------- STOI
# Short-time objective intelligibility of rows at 10 kHz (wm_stoi, csrc/stoi.hip; the definition is in include/wm_hip.h): the quality
# column of the evaluation side.  Nothing is differentiated: a measure, not a loss.
def stoi_plan(rows, n):
    """bytes of scratch one wm_stoi launch on (rows, n) needs"""
    import ctypes
    for v, name in ((rows, "rows"), (n, "n")):
        _chk_int(v, name, 1, math.inf, "a positive int")
    if n > 2 ** 34 or rows * n > 2 ** 46:
        raise ValueError(f"rows = {rows}, n = {n}: a row may have 2^34 samples and a launch 2^46")
    need = ctypes.c_longlong(0)
    lib.wm_stoi_plan(rows, n, ctypes.addressof(need), None)
    return need.value


def _stoi_rows(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: expected dtype torch.float32, got {t.dtype}")
    if t.dim() == 3 and t.shape[1] == 1:
        rows = t.reshape(t.shape[0], t.shape[2])
    elif t.dim() == 2:
        rows = t
    elif t.dim() == 1:
        rows = t[None]
    else:
        raise ValueError(f"{name}: expected (B, 1, T), (C, N) or (N,), got shape {tuple(t.shape)}")
    if rows.shape[0] < 1 or rows.shape[1] < 1:
        raise ValueError(f"{name}: needs at least one row of at least one sample, got shape {tuple(t.shape)}")
    return rows.contiguous()


def stoi(x, y, sample_rate=16000):
    """STOI of every row of y (the processed signal) against the same row of x (the reference): float32 tensors of equal shape (B, 1, T),
    (C, N) or (N,) at `sample_rate`.  Returns (d (rows,) float32, kept (rows,) int32) on the inputs' device: the score and the number of
    frames that survived silent-frame removal.  CUDA tensors: one wm_stoi call, preceded by ONE resample_rows launch on x and y stacked
    unless sample_rate == 10000.  CPU tensors: the float64 restatement of quality.stoi_rows_host (after the host resampler)."""
    from .quality import STOI_RATE, stoi_rows_host
    rate = _rate(sample_rate, "sample_rate")
    xr, yr = _stoi_rows(x, "x"), _stoi_rows(y, "y")
    if x.shape != y.shape:
        raise ValueError(f"x and y: expected equal shapes, got {tuple(x.shape)} and {tuple(y.shape)}")
    if xr.device != yr.device:
        raise ValueError(f"x and y: expected one device, got {xr.device} and {yr.device}")
    rows = xr.shape[0]
    if not xr.is_cuda:
        if rate != STOI_RATE:
            from .inference import _resample_rows_host
            both = _resample_rows_host(torch.cat([xr, yr], dim=0), rate, STOI_RATE)
            xr, yr = both[:rows], both[rows:]
        return stoi_rows_host(xr, yr)
    if rate != STOI_RATE:
        both = resample_rows(torch.cat([xr, yr], dim=0), rate, STOI_RATE)
        xr, yr = both[:rows], both[rows:]
    n = xr.shape[1]
    d = _f32(rows, device=xr.device)
    kept = torch.empty(rows, dtype=torch.int32, device=xr.device)
    scratch = torch.empty(stoi_plan(rows, n) // 4, dtype=torch.float32, device=xr.device)
    lib.wm_stoi(_p(xr), _p(yr), _p(d), _p(kept), _p(scratch), rows, n, _stream())
    return d, kept


# ---------------------------------------------------------------------------------------------- splice attack and localisation
# wm_splice / wm_splice_bwd, wm_bce_masked_fwd / _bwd and wm_loc_score (csrc/splice.hip; the definitions are in include/wm_hip.h).  Labels
# travel as bit masks: (rows, ceil(n / 32)) int32 tensors, bit j of word w = sample 32 w + j, 1 = "still watermarked", tail bits zero.
SPLICE_MAX_SPANS = 8
SPLICE_MAX_N = 2 ** 24


def label_words(n):
    """words per row of a label mask over n samples"""
    return (int(n) + 31) // 32


def _lab(lab, rows, n, name="lab"):
    lab = _chk(lab, name, 2, torch.int32)
    if tuple(lab.shape) != (rows, label_words(n)):
        raise ValueError(f"{name}: expected a ({rows}, {label_words(n)}) int32 mask for {rows} rows of {n} samples, got shape {tuple(lab.shape)}")
    return lab


class SpliceFn(torch.autograd.Function):
    """wm_splice on the tape: spans of the watermarked rows `a` replaced by the clean rows `b` (as they are, silenced, or moved within the
    row), with the spans drawn in the kernel from (seed, draw, row0 + r).  cut = (max_spans, p_span, len_lo, len_hi, p_original,
    p_silence), the lengths in samples.  Returns (y, lab): y like a, lab the (rows, ceil(n / 32)) int32 label mask, not differentiable.
    Saved for the backward: lab alone.  da = wm_splice_bwd(dy, lab); b is data and gets no gradient."""

    @staticmethod
    def forward(ctx, a, b, cut, seed, draw, row0):
        a, b = _chk(a, "a"), _chk(b, "b")
        if a.shape != b.shape or a.device != b.device:
            raise ValueError(f"a and b: expected equal shapes on one device, got {tuple(a.shape)} on {a.device} and {tuple(b.shape)} on {b.device}")
        if a.dim() < 1 or a.numel() == 0:
            raise ValueError(f"a: needs at least one row of at least one sample, got shape {tuple(a.shape)}")
        n = a.shape[-1]
        rows = a.numel() // n
        max_spans, p_span, len_lo, len_hi, p_original, p_silence = cut
        y = torch.empty_like(a)
        lab = torch.empty(rows, label_words(n), dtype=torch.int32, device=a.device)
        lib.wm_splice(_p(a), _p(b), _p(y), _p(lab), rows, n, int(row0), _seed64(seed), int(draw), int(max_spans),
                      float(p_span), int(len_lo), int(len_hi), float(p_original), float(p_silence), _stream())
        ctx.save_for_backward(lab)
        ctx.mark_non_differentiable(lab)
        return y, lab

    @staticmethod
    def backward(ctx, g, _glab):
        (lab,) = ctx.saved_tensors
        g = _chk(g, "grad")
        n = g.shape[-1]
        da = torch.empty_like(g)
        lib.wm_splice_bwd(_p(g), _p(lab), _p(da), g.numel() // n, n, _stream())
        return da, None, None, None, None, None


def splice(a, b, *, max_spans=2, p_span=0.5, len_lo=800, len_hi=6400, p_original=1 / 3, p_silence=1 / 3, seed=0, draw=0, row0=0):
    """(y, lab) of one wm_splice call on contiguous fp32 CUDA tensors a (watermarked) and b (clean) of one shape, all leading axes rows;
    the lengths in samples.  Differentiable in a (ops.SpliceFn)."""
    return SpliceFn.apply(a, b, (max_spans, p_span, len_lo, len_hi, p_original, p_silence), seed, draw, row0)


class MaskedBCEFn(torch.autograd.Function):
    """(loc, bce) of wm_bce_masked_fwd: BCEFn against per-sample labels.  logits (2B, T, 1 + bits), message (B,) int64, lab the (B,
    ceil(T / 32)) int32 label mask of the watermarked half; the clean half has target 0 throughout.  The bit term averages over the
    samples whose label is 1 -- their number N1 is counted on the device and stays there for the backward (`count`, a device int64
    saved with logits, message and lab): no host sync."""

    @staticmethod
    def forward(ctx, logits, message, lab):
        logits = _chk(logits, "logits", 3)
        message = _chk(message, "message", 1, torch.int64)
        R, T, NO = logits.shape
        B = message.shape[0]
        if R != 2 * B:
            raise ValueError(f"logits must hold [watermarked; clean] = 2*B clips, got {R} for B={B}")
        lab = _lab(lab, B, T)
        dev = logits.device
        part = _f32(3 * R * ((T * NO + 4095) // 4096), device=dev)
        out = torch.zeros(2, dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        lib.wm_bce_masked_fwd(_p(logits), _p(message), _p(lab), _p(part), _p(count), _p(out[0]), _p(out[1]), B, R, T, NO, _stream())
        ctx.save_for_backward(logits, message, lab, count)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_loc, g_bce):
        logits, message, lab, count = ctx.saved_tensors
        R, T, NO = logits.shape
        gl = g_loc.contiguous().float().reshape(1) if g_loc is not None else torch.zeros(1, device=logits.device)
        gb = g_bce.contiguous().float().reshape(1) if g_bce is not None else torch.zeros(1, device=logits.device)
        d = torch.empty_like(logits)
        lib.wm_bce_masked_bwd(_p(logits), _p(message), _p(lab), _p(count), _p(gl), _p(gb), _p(d), message.shape[0], R, T, NO, _stream())
        return d, None, None


def loc_threshold_logit(threshold):
    """log(p / (1 - p)) in float64 on the host: the logit the probability threshold p stands for; exactly 0.0 at p = 0.5"""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0.0 <= threshold <= 1.0:
        raise ValueError(f"threshold: expected a probability in [0, 1], got {threshold!r}")
    p = float(threshold)
    if p == 0.5:
        return 0.0
    if p == 0.0:
        return -math.inf
    if p == 1.0:
        return math.inf
    return math.log(p / (1.0 - p))


def loc_counts(logits, lab, threshold=0.5, want_pred=False):
    """The per-sample prediction sigmoid(logits[r, t, 0]) > threshold, taken as logits[r, t, 0] > log(p / (1 - p)), against the label mask
    `lab` ((lab_rows, ceil(T / 32)) int32 with lab_rows <= R: rows behind it have label 0; None: every label is 1).  One wm_loc_score
    launch.  Returns counts (R, 4) int32 = {tp, fp, fn, tn} on the device, exact; with want_pred also pred (R, ceil(T / 32)) int32, the
    prediction in the mask layout.  NaN logits predict 0."""
    logits = _chk(logits, "logits", 3)
    R, T, NO = logits.shape
    if R < 1 or T < 1 or NO < 1:
        raise ValueError(f"logits: needs at least one row, one sample and one channel, got shape {tuple(logits.shape)}")
    thr = loc_threshold_logit(threshold)
    lab_rows = 0
    if lab is not None:
        lab = _chk(lab, "lab", 2, torch.int32)
        lab_rows = lab.shape[0]
        if lab_rows < 1 or lab_rows > R or lab.shape[1] != label_words(T):
            raise ValueError(f"lab: expected (at most {R}, {label_words(T)}) int32, got shape {tuple(lab.shape)}")
    counts = torch.empty(R, 4, dtype=torch.int32, device=logits.device)
    pred = torch.empty(R, label_words(T), dtype=torch.int32, device=logits.device) if want_pred else None
    lib.wm_loc_score(_p(logits), _p(lab), thr, _p(counts), _p(pred), R, T, NO, lab_rows, _stream())
    return (counts, pred) if want_pred else counts


# ---------------------------------------------------------------------------------------------- per-clip detection scores
# wm_clip_scores (csrc/clip_scores.hip; the definition is in include/wm_hip.h): everything an operating-point report needs of the
# Detector's logits, in one pass.  Nothing is differentiated: a measure, not a loss.
CLIP_SCORES_MAX_T = 2 ** 24
ClipScores = collections.namedtuple("ClipScores", "prob llr votes words biterr")


def clip_scores_plan(R, T, NO):
    """bytes of scratch one wm_clip_scores launch on (R, T, NO) logits needs"""
    import ctypes
    for v, name in ((R, "R"), (T, "T"), (NO, "NO")):
        _chk_int(v, name, 1, math.inf, "a positive int")
    if T > CLIP_SCORES_MAX_T or NO > 64 or R * T * NO > 2 ** 46:
        raise ValueError(f"R = {R}, T = {T}, NO = {NO}: a clip may have 2^24 samples and 64 channels, a launch 2^46 elements")
    need = ctypes.c_longlong(0)
    lib.wm_clip_scores_plan(R, T, NO, ctypes.addressof(need), None)
    return need.value


def clip_scores(logits, message=None, threshold=0.5):
    """Per-clip scores of the Detector's logits (R, T, NO) float32, channel 0 the detection logit and channels 1.. the message bits:
    ClipScores(prob, llr, votes, words, biterr) on the logits' device --
      prob (R,) float32         the mean over t of sigmoid(logits[:, t, 0]): the reference's per-clip score
      llr (R, NO) float32       the mean logit of every channel
      votes (R, NO) int32       exact: the samples with sigmoid(channel 0) > threshold (taken as logit > log(p / (1 - p)), as
                                loc_counts does), and for o >= 1 the samples with logit > 0; a NaN casts no vote
      words (R, 2) int64        the decoded message: [:, 0] the majority of the hard decisions (a tie is 0), [:, 1] the sign of the summed logits
      biterr (B, 2) int32       the wrong bits of words[:B] against `message` ((B,) int64, B <= R: the watermarked rows come first);
                                (0, 2) without a message
    CUDA tensors: one wm_clip_scores call, no host sync.  CPU tensors: the float64 restatement detection.clip_scores_host rounded to
    float32, the integers exact -- so that what is built on top runs without a GPU."""
    if not isinstance(logits, torch.Tensor):
        raise TypeError(f"logits: expected a tensor, got {type(logits).__name__}")
    if logits.dtype != torch.float32 or logits.dim() != 3:
        raise ValueError(f"logits: expected a float32 (R, T, NO) tensor, got {logits.dtype} with shape {tuple(logits.shape)}")
    R, T, NO = logits.shape
    if R < 1 or T < 1 or NO < 1 or NO > 64 or T > CLIP_SCORES_MAX_T or R * T * NO > 2 ** 46:
        raise ValueError(f"logits: needs at least one row, 1 .. 2^24 samples, 1 .. 64 channels and at most 2^46 elements, got shape {tuple(logits.shape)}")
    thr = loc_threshold_logit(threshold)
    B = 0
    if message is not None:
        if not isinstance(message, torch.Tensor) or message.dtype != torch.int64 or message.dim() != 1:
            raise ValueError("message: expected a (B,) int64 tensor")
        if message.device != logits.device:
            raise ValueError(f"logits and message: expected one device, got {logits.device} and {message.device}")
        B = message.shape[0]
        if B > R:
            raise ValueError(f"message: at most one per row of logits ({R}), got {B}")
    dev = logits.device
    if not logits.is_cuda:
        from .detection import clip_scores_host
        prob, llr, votes, words, biterr = clip_scores_host(logits.detach().numpy(), None if message is None else message.numpy(), thr)
        return ClipScores(torch.from_numpy(prob.astype("float32")), torch.from_numpy(llr.astype("float32")), torch.from_numpy(votes),
                          torch.from_numpy(words), torch.from_numpy(biterr))
    logits = logits.contiguous()
    message = None if message is None else message.contiguous()
    prob, llr = _f32(R, device=dev), _f32(R, NO, device=dev)
    votes = torch.empty(R, NO, dtype=torch.int32, device=dev)
    words = torch.empty(R, 2, dtype=torch.int64, device=dev)
    biterr = torch.empty(B, 2, dtype=torch.int32, device=dev)
    scratch = torch.empty(clip_scores_plan(R, T, NO) // 4, dtype=torch.int32, device=dev)
    lib.wm_clip_scores(_p(logits), _p(message) if B else None, thr, _p(prob), _p(llr), _p(votes), _p(words), _p(biterr) if B else None,
                       _p(scratch), B, R, T, NO, _stream())
    return ClipScores(prob, llr, votes, words, biterr)


# ---------------------------------------------------------------------------------------------- clip curation features
# wm_clip_features (csrc/clip_features.hip; the definition is in include/wm_hip.h): the speech / noise feature table and the silence
# measure of the reference's dataset scripts, one launch for all rows.  Nothing is differentiated: a measure, not a loss.
ClipFeaturesPlan = collections.namedtuple("ClipFeaturesPlan", "frames energy_frames lds_bytes")


def clip_features_plan(rows, n, sample_rate=16000):
    """ClipFeaturesPlan(frames, energy_frames, lds_bytes) of one wm_clip_features launch on (rows, n) at sample_rate: F = 1 + n // 512
    spectral frames per row, the 25-ms frames of energy_std, the LDS one workgroup takes.  ValueError where the launch would be refused."""
    import ctypes
    from .curate import check_shape
    _chk_int(rows, "rows", 1, 2 ** 40)
    _chk_int(n, "n", 1, math.inf, "a positive int")
    sr = check_shape(n, sample_rate)
    out = (ctypes.c_int * 3)()
    base = ctypes.addressof(out)
    lib.wm_clip_features_plan(rows, n, sr, base, base + 4, base + 8, None)
    return ClipFeaturesPlan(out[0], out[1], out[2])


def clip_features(x, sample_rate=16000, frames=False):
    """The curation features of every row of x: a float32 tensor (B, 1, T), (C, N) or (N,) at `sample_rate`, 400 .. 32768 samples a row.
    Returns (feat (rows, 16) float32, counts (rows, 4) int32) on x's device, and with frames=True also frames (rows, F, 4) float32 -- per
    spectral frame the centroid, the bandwidth, the roll-off bin and the zero-crossing count.  The columns of feat are curate.FEATURES
    (then three reserved zeros); counts holds the zero-crossing total, the speech score, the non-finite flag and the label (1 speech,
    0 noise, -1 non-finite).  CUDA tensors: ONE wm_clip_features launch, no host sync.  CPU tensors: the float64 restatement
    curate.clip_features_host rounded to float32, the integers exact."""
    from . import curate
    rows_t = _stoi_rows(x, "x")
    rows, n = rows_t.shape
    sr = curate.check_shape(n, sample_rate)
    if not rows_t.is_cuda:
        out = curate.clip_features_host(rows_t.detach().numpy(), sr, frames)
        res = (torch.from_numpy(out[0].astype("float32")), torch.from_numpy(out[1]))
        return res + (torch.from_numpy(out[2].astype("float32")),) if frames else res
    dev = rows_t.device
    F = clip_features_plan(rows, n, sr).frames
    tab = curate.tables_on(sr, dev)
    feat = _f32(rows, 16, device=dev)
    counts = torch.empty(rows, 4, dtype=torch.int32, device=dev)
    per = _f32(rows, F, 4, device=dev) if frames else None
    lib.wm_clip_features(_p(rows_t), _p(tab["sos"]), _p(tab["fb"]), _p(tab["klo"]), _p(tab["khi"]), _p(tab["dct"]), _p(feat), _p(counts),
                         _p(per), rows, n, sr, tab["warm"], _stream())
    return (feat, counts, per) if frames else (feat, counts)
