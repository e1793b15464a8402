"""The float64 yardstick of the resampler, for its CPU and GPU tests (`import resample_yardstick as Y`, or its names): torchaudio's
documented default design (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) evaluated in float64 numpy over ALL K = 2*width + P
taps of every phase -- no compact table, no conv1d, nothing from the package -- so a mistake the package's CPU twin and its kernel share
(say in the compact table's first index) shows against it.  Nothing from the package serves as a yardstick except in the bit-identity
checks of the tests.

One row of the resampler is the (L, N) matrix
    A[m*Q + i][m*P + j - width] = h[i][j]
Two formulations of it live here, and tests/test_yardsticks_cpu.py holds one against the other:
  yardstick(xmono, orig, new, C)   A @ xmono with its bound, for the whole-recording paths (resample, resample_add, load_audio);
  apply64 / adjoint64              A @ x and A.T @ dy as dense products over the periods, for the rows kernel, its adjoint launch and
                                   the two-stage attack (attack64 / attack_grad64).

Tolerances (derived, nothing tuned, no rtol).  The yardstick applies the same float32-rounded taps in float64, so the package differs
from it only by the roundings of its float32 sums.

  One stage.  Output sample m*Q + i (or input sample of adjoint phase p) is off by at most
      gamma_n * sum_j |h[i][j]| * |x[m*P + j]|,   gamma_n = n u / (1 - n u),   u = 2**-24
  plus one float32 ulp of the result for its final rounding.  In yardstick() n = (non-zero taps of phase i) + C: n - C products and
  additions of the filter, C roundings of the mean over C channels.  In forward_gamma / adjoint_gamma n = (non-zero taps of the
  phase) + 1.

  Two stages (y = B (A x)).  The first stage's bound b_A goes through |B|, the second adds its own:
      |B| b_A + gamma_B * |B| |A x| + ulp(y);        for the gradient A.T (B.T g):   |A|.T b_B + gamma * |A|.T |B.T g| + ulp.

  resample_add.  With (u64, bound) = yardstick(delta[:n_d], 16000, R, C=1) cut to N samples,
      |up - u64| <= bound                                                      (the one-stage bound above)
      |out[c] - (x[c] + u64)| <= bound + spacing(float32(|x[c] + u64|))        (the same error carried through ONE more float32 add).

`design` hands out read-only tables, computed once.  The dense table of 16000 -> 16001 has 16001 x 16014 entries, about 1 GB in float32,
so of the tables above BIG_TABLE bytes only the last one is kept; the small ones all stay."""
import math

import numpy as np
import torch

from yardstick_common import gamma, ulp32

LPW, ROLLOFF = 6, 0.99
BIG_TABLE = 64 << 20
_SMALL, _BIG = {}, {}


def design(orig, new):
    """(P, Q, width, K, dense float32 table (Q, K)) from the published formula, float64 rounded once to float32"""
    g = math.gcd(orig, new)
    P, Q = orig // g, new // g
    base = min(P, Q) * ROLLOFF
    width = int(math.ceil(LPW * P / base))
    K = 2 * width + P
    big = 4 * Q * K > BIG_TABLE
    cache = _BIG if big else _SMALL
    if (orig, new) not in cache:
        if big:
            _BIG.clear()                                                                     # before the next one is built, not after
        j = np.arange(K, dtype=np.float64)[None, :]
        i = np.arange(Q, dtype=np.float64)[:, None]
        t = np.clip(((j - width) / P - i / Q) * base, -LPW, LPW)
        pt = np.pi * t
        sinc = np.where(pt == 0, 1.0, np.sin(pt) / np.where(pt == 0, 1.0, pt))
        h = (base / P) * sinc * np.cos(pt / (2 * LPW)) ** 2
        h32 = h.astype(np.float32)
        h32.setflags(write=False)                                                            # computed once, shared, left unchanged
        cache[(orig, new)] = (P, Q, width, K, h32)
    return cache[(orig, new)]


def yardstick(xmono, orig, new, C=1):
    """float64 resampling of the float64 mono signal `xmono` (N,) -> (y (L,), bound (L,))"""
    P, Q, width, K, h32 = design(orig, new)
    h = h32.astype(np.float64)
    N = xmono.shape[0]
    L = -((-Q * N) // P)
    periods = N // P + 1
    xpad = np.concatenate([np.zeros(width), np.asarray(xmono, dtype=np.float64), np.zeros(width + P)])
    frames = np.lib.stride_tricks.sliding_window_view(xpad, K)[::P][:periods]            # (periods, K): xpad[m*P + j]
    gam = gamma((h32 != 0).sum(axis=1) + C)                                                  # (Q,)
    y, bound = np.empty((periods, Q)), np.empty((periods, Q))
    step = max(1, 4_000_000 // K)
    for a in range(0, periods, step):
        f = np.ascontiguousarray(frames[a:a + step])
        y[a:a + step] = f @ h.T
        bound[a:a + step] = (np.abs(f) @ np.abs(h).T) * gam[None, :]
    y, bound = y.reshape(-1)[:L], bound.reshape(-1)[:L]
    return y, bound + ulp32(y)


def apply64(h, P, width, x, L):
    """A @ x in float64 for the (Q, K) table h (or |h|): y[m*Q + i] = sum_j h[i][j] * xpad[m*P + j], the first L samples"""
    Q, K = h.shape
    N = x.shape[0]
    periods = -(-L // Q)
    xpad = np.zeros(max(N + 2 * width + P, (periods - 1) * P + K))
    xpad[width:width + N] = x
    frames = np.lib.stride_tricks.sliding_window_view(xpad, K)[::P][:periods]               # (periods, K): xpad[m*P + j]
    return (frames @ h.T).reshape(-1)[:L]


def adjoint64(h, P, width, dy, N):
    """A.T @ dy in float64, A the (L, N) matrix of the table h (or |h|), L = len(dy): period m hands dy[m*Q + i] * h[i][j] to xpad[m*P + j]"""
    Q, K = h.shape
    L = dy.shape[0]
    periods = -(-L // Q)
    d = np.zeros(periods * Q)
    d[:L] = dy
    F = d.reshape(periods, Q) @ h                                                            # (periods, K)
    buf = np.zeros(max((periods - 1) * P + K, width + N))
    for j in range(K):
        buf[j:j + (periods - 1) * P + 1:P] += F[:, j]
    return buf[width:width + N]


def forward_gamma(h32, L):
    """gamma_n of output sample o < L: n = non-zero taps of its phase o % Q, + 1"""
    return gamma((h32 != 0).sum(axis=1) + 1.0)[np.arange(L) % h32.shape[0]]


def adjoint_gamma(h32, P, width, N):
    """gamma_n of input sample n < N: the taps of adjoint phase p = n % P are the columns j = p + width (mod P) of the table"""
    col = (h32 != 0).sum(axis=0)
    nnz = np.array([col[(p + width) % P::P].sum() for p in range(P)], dtype=np.float64)
    return gamma(nnz + 1.0)[np.arange(N) % P]


def attack64(x, rate, sr=16000):
    """float64 up(down(x))[:T] of one row and its composed bound"""
    T = x.shape[0]
    Pd, Qd, wd, _, hd32 = design(sr, rate)
    Pu, Qu, wu, _, hu32 = design(rate, sr)
    hd, hu = hd32.astype(np.float64), hu32.astype(np.float64)
    L1 = -((-Qd * T) // Pd)
    v = apply64(hd, Pd, wd, x, L1)
    b1 = forward_gamma(hd32, L1) * apply64(np.abs(hd), Pd, wd, np.abs(x), L1) + ulp32(v)
    y = apply64(hu, Pu, wu, v, T)
    bound = apply64(np.abs(hu), Pu, wu, b1, T) + forward_gamma(hu32, T) * apply64(np.abs(hu), Pu, wu, np.abs(v), T) + ulp32(y)
    return y, bound


def attack_grad64(g, rate, sr=16000):
    """float64 A_down.T @ (A_up[:T].T @ g) of one row and its composed bound"""
    T = g.shape[0]
    Pd, Qd, wd, _, hd32 = design(sr, rate)
    Pu, Qu, wu, _, hu32 = design(rate, sr)
    hd, hu = hd32.astype(np.float64), hu32.astype(np.float64)
    L1 = -((-Qd * T) // Pd)
    v = adjoint64(hu, Pu, wu, g, L1)
    b_up = adjoint_gamma(hu32, Pu, wu, L1) * adjoint64(np.abs(hu), Pu, wu, np.abs(g), L1) + ulp32(v)
    dx = adjoint64(hd, Pd, wd, v, T)
    bound = adjoint64(np.abs(hd), Pd, wd, b_up, T) + adjoint_gamma(hd32, Pd, wd, T) * adjoint64(np.abs(hd), Pd, wd, np.abs(v), T) + ulp32(dx)
    return dx, bound


def signal(kind, C, N, rate, seed):
    """(C, N) float32: noise, or recording-like partials with a noise floor"""
    g = torch.Generator().manual_seed(seed)
    if kind == "noise":
        return 0.5 * torch.randn(C, N, generator=g)
    t = torch.arange(N, dtype=torch.float64) / rate                                          # recording-like: partials + a noise floor
    x = sum(a * torch.sin(2 * math.pi * f * t + p) for a, f, p in ((0.4, 220.0, 0.1), (0.2, 1730.0, 1.0), (0.1, 5200.0, 2.0)))
    return (x[None, :].repeat(C, 1) * torch.linspace(1.0, 0.6, C, dtype=torch.float64)[:, None]).float() + 0.01 * torch.randn(C, N, generator=g)


def rows_signal(rows, n, seed):
    """every row its own noise"""
    return 0.5 * torch.randn(rows, n, generator=torch.Generator().manual_seed(1000 * seed + n))
