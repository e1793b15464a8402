"""STOI (Taal et al. 2011) in float64 numpy from the definition in include/wm_hip.h (the comment of wm_stoi); nothing from the package.

stoi(x, y) scores one row pair at 10 kHz and returns a Score: d, K (the kept frames), margin_db (the smallest distance of any frame of x
from the silence threshold, in dB: how far the kept-frame mask is from flipping) and kappa (the largest ||xi||^2 / ||xi - mean||^2 over
the row's band segments: what mean removal multiplies a rounding error by).  stoi(x, y, twin=True) is the float32 twin: the same code with
every array in float32 and the transform as a dense float32 DFT product; |d_twin - d64| is what float32 arithmetic costs in SOME order.

The signal recipe: speech_like(n, seed) is 29 harmonics of a 110-150 Hz tone plus noise under a piecewise-constant on / off envelope with
pauses (the pauses are 80 dB down: their frames are dropped); stationary(n, seed) is white noise, every frame kept; noisy(x, snr_db, seed)
adds white noise at that SNR.  case(n, kind) / case_ref(...) are cached: a reference is computed once and never written to."""
import functools
from collections import namedtuple

import numpy as np

EPS = 2.0 ** -52
FS = 10000
FRAME, HOP, NFFT, J, SEG = 256, 128, 512, 15, 30
SENTINEL = 1e-5
EDGES = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109), (109, 138),
         (138, 174), (174, 219))
SNRS = (30, 10, 0)

Score = namedtuple("Score", "d K margin_db kappa")


def band_edges():
    """[(lo_b, hi_b)]: the bins nearest to 150 * 2^((2b -+ 1) / 6) Hz on the grid k * 10000 / 512"""
    grid = np.arange(NFFT // 2 + 1) * (FS / NFFT)
    out = []
    for b in range(J):
        lo, hi = 150.0 * 2.0 ** ((2 * b - 1) / 6.0), 150.0 * 2.0 ** ((2 * b + 1) / 6.0)
        out.append((int(np.argmin((grid - lo) ** 2)), int(np.argmin((grid - hi) ** 2))))
    return tuple(out)


def frame_count(n):
    return max(0, -(-(n - FRAME) // HOP))


def window():
    return np.hanning(FRAME + 2)[1:-1]


def _frames(v, count):
    return v[HOP * np.arange(count)[:, None] + np.arange(FRAME)[None, :]]


@functools.lru_cache(maxsize=None)
def _dft32():
    ang = 2.0 * np.pi * np.outer(np.arange(FRAME), np.arange(7, 219)) / NFFT
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def _overlap_add(g, dt):
    K = g.shape[0]
    out = np.zeros(HOP * (K - 1) + FRAME, dtype=dt)
    out[:HOP * K].reshape(K, HOP)[...] += g[:, :HOP]
    out[HOP:].reshape(K, HOP)[...] += g[:, HOP:]
    return out


def stoi(x, y, twin=False):
    dt = np.float32 if twin else np.float64
    x64, y64 = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    assert x64.ndim == 1 and x64.shape == y64.shape
    if not (np.isfinite(x64).all() and np.isfinite(y64).all()):
        return Score(float("nan"), 0, float("nan"), float("nan"))
    x, y = x64.astype(dt), y64.astype(dt)
    eps = dt(EPS)
    n = x.shape[0]
    F = frame_count(n)
    if F == 0:
        return Score(SENTINEL, 0, float("inf"), 1.0)
    w = window().astype(dt)
    xf, yf = w * _frames(x, F), w * _frames(y, F)
    norms = np.sqrt((xf * xf).sum(axis=1))
    thr = dt(0.01) * (norms.max() + eps)
    keep = norms + eps > thr
    K = int(keep.sum())
    with np.errstate(divide="ignore"):
        margin = float(np.abs(20.0 * np.log10((norms.astype(np.float64) + EPS) / np.float64(thr))).min()) if norms.max() > 0 else float("inf")
    S = K - 1
    if S < SEG:
        return Score(SENTINEL, K, margin, 1.0)
    xs, ys = _overlap_add(xf[keep], dt), _overlap_add(yf[keep], dt)
    fx, fy = w * _frames(xs, S), w * _frames(ys, S)
    if twin:
        C, Sn = _dft32()
        px = (fx @ C) ** 2 + (fx @ Sn) ** 2
        py = (fy @ C) ** 2 + (fy @ Sn) ** 2
    else:
        px = np.abs(np.fft.rfft(fx, NFFT, axis=1)[:, 7:219]) ** 2
        py = np.abs(np.fft.rfft(fy, NFFT, axis=1)[:, 7:219]) ** 2
    assert px.dtype == dt
    X = np.stack([np.sqrt(px[:, lo - 7:hi - 7].sum(axis=1)) for lo, hi in EDGES])          # (J, S)
    Y = np.stack([np.sqrt(py[:, lo - 7:hi - 7].sum(axis=1)) for lo, hi in EDGES])
    xi = np.lib.stride_tricks.sliding_window_view(X, SEG, axis=1)                          # (J, S - 29, 30)
    eta = np.lib.stride_tricks.sliding_window_view(Y, SEG, axis=1)
    nx = np.sqrt((xi * xi).sum(axis=2, keepdims=True))
    ny = np.sqrt((eta * eta).sum(axis=2, keepdims=True))
    alpha = nx / (ny + eps)
    etap = np.minimum(alpha * eta, dt(1.0 + 10.0 ** (15.0 / 20.0)) * xi)
    xc = xi - xi.mean(axis=2, keepdims=True)
    yc = etap - etap.mean(axis=2, keepdims=True)
    nxc = np.sqrt((xc * xc).sum(axis=2, keepdims=True))
    xc = xc / (nxc + eps)
    yc = yc / (np.sqrt((yc * yc).sum(axis=2, keepdims=True)) + eps)
    rho = (xc * yc).sum(axis=2)
    assert rho.dtype == dt and rho.shape == (J, S - SEG + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        kap = (nx.astype(np.float64) / nxc.astype(np.float64)) ** 2
    kappa = float(np.nanmax(np.where(np.isfinite(kap), kap, 1.0)))
    return Score(float(rho.mean(dtype=dt)), K, margin, kappa)


# ---------------------------------------------------------------------------------------------- the signal recipe
def speech_like(n, seed):
    """29 harmonics of a 110-150 Hz tone (the top one below 4.4 kHz) with 1 / sqrt(h) amplitudes and a slow vibrato-free pitch, plus noise 26
    dB down, under an on / off envelope: stretches of 60-400 ms at a level in [0.3, 1], pauses of 40-200 ms at 1e-4 (80 dB down)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    f0 = rng.uniform(110.0, 150.0)
    sig = np.zeros(n)
    for h in range(1, 30):
        sig += np.sin(2.0 * np.pi * (h * f0 * t + rng.uniform())) / np.sqrt(h)
    sig = sig / np.abs(sig).max() + 0.05 * rng.standard_normal(n)
    env = np.empty(n)
    pos, on = 0, True
    while pos < n:
        length = int(rng.uniform(0.06, 0.4) * FS) if on else int(rng.uniform(0.04, 0.2) * FS)
        env[pos:pos + length] = rng.uniform(0.3, 1.0) if on else 1e-4
        pos, on = pos + length, not on
    return (0.5 * env * sig).astype(np.float32)


def stationary(n, seed):
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def noisy(x, snr_db, seed):
    """x + white noise at snr_db against the row's mean square"""
    z = np.random.default_rng(seed).standard_normal(x.shape[0])
    ms = float(np.mean(x.astype(np.float64) ** 2))
    return (x + np.sqrt(ms / 10.0 ** (snr_db / 10.0)) * z).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(n, kind):
    """(x (3, n), y (3, n)) float32, read-only: the three rows are y = x + noise at 30, 10 and 0 dB.  kind: "speech" or "noise" """
    xs, ys = [], []
    for i, snr in enumerate(SNRS):
        x = (speech_like if kind == "speech" else stationary)(n, 1000 * n + i)
        xs.append(x)
        ys.append(noisy(x, snr, 7000 * n + i))
    x, y = np.stack(xs), np.stack(ys)
    x.setflags(write=False); y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def case_ref(n, kind):
    """([Score per row] in float64, [Score per row] of the twin)"""
    x, y = case(n, kind)
    return tuple(stoi(a, b) for a, b in zip(x, y)), tuple(stoi(a, b, twin=True) for a, b in zip(x, y))


# the accuracy cases of tests/test_gpu_stoi.py: (n, kind, what must come out)
SENTINEL_CASES = ((255, "speech"), (256, "speech"), (257, "speech"), (3969, "speech"), (4096, "noise"))
FLOAT_CASES = ((4097, "noise"), (6250, "speech"), (10000, "speech"), (20000, "speech"), (100000, "speech"))
