"""The yardstick of the noise-suppression attack: numpy only, nothing from the package, written from the comment of wm_noise_suppress in
include/wm_hip.h.  model() states the definition step by step in float64; with twin=True the same steps run in float32 (the window, the
transform as a matrix product, the logarithms, the recursion, the overlap-add), and the twin's distance from float64 is the floor the GPU
tests scale their bars from.  case(n) are the seeded inputs, computed once and read-only."""
import functools

import numpy as np

FS = 16000
L, H, K = 512, 256, 257
EPS = 1e-10
GAMMA_E = 0.5772156649015329
ALPHA, OVER = 0.98, 1.0
REDUCE_DB = (12.0, 18.0, 24.0)        # the rows' depths in the accuracy cases


def frame_count(n):
    return -(-n // H) + 1


@functools.lru_cache(maxsize=None)
def window(twin=False):
    w = np.sin(np.pi * (np.arange(L) + 0.5) / L)
    return w.astype(np.float32) if twin else w


@functools.lru_cache(maxsize=None)
def dft(twin=False):
    """(cos, sin) of 2 pi k t / 512 as (512, 257) matrices in the mode's precision, the angle reduced in integers first"""
    kt = np.outer(np.arange(L), np.arange(K)) % L
    ang = 2.0 * np.pi * kt / L
    dt = np.float32 if twin else np.float64
    return np.cos(ang).astype(dt), np.sin(ang).astype(dt)


def frames(v, twin=False):
    """(M, 512): H zeros, the row, zeros up to (M + 1) H samples; frame m = xp[m H : m H + L] w"""
    M = frame_count(v.shape[0])
    vp = np.zeros((M + 1) * H, dtype=v.dtype)
    vp[H:H + v.shape[0]] = v
    return window(twin) * vp[H * np.arange(M)[:, None] + np.arange(L)[None, :]]


def spectrum(v, twin=False):
    """(Re, Im) (M, 257) of the windowed frames' 512-point real transform"""
    Cm, Sm = dft(twin)
    f = frames(v, twin)
    return f @ Cm, -(f @ Sm)


def inverse(re, im, twin=False):
    """the 512-point inverse real transform of (M, 257) spectra: (M, 512)"""
    dt = np.float32 if twin else np.float64
    Cm, Sm = dft(twin)
    c = np.full(K, 2.0, dtype=dt)
    c[0] = c[K - 1] = 1.0
    return ((c * re) @ Cm.T - (c * im) @ Sm.T) / dt(L)


def clip_db(reduce_db):
    r = float(reduce_db)
    return 0.0 if r != r else min(max(r, 0.0), 60.0)


def model(x, reduce_db, src=None, noise=None, twin=False, alpha=ALPHA, over=OVER):
    """(y (n,), G (M, 257), N (257,)) of one row: gains from x, applied to src (None: x); noise: a (257,) profile or None"""
    dt = np.float32 if twin else np.float64
    x64 = np.asarray(x, dtype=np.float64)
    assert x64.ndim == 1 and x64.shape[0] >= 1
    n, M = x64.shape[0], frame_count(x64.shape[0])
    if not np.isfinite(x64).all():
        return np.full(n, np.nan, dtype=dt), np.full((M, K), np.nan, dtype=dt), np.full(K, np.nan, dtype=dt)
    xr, xi_ = spectrum(x64.astype(dt), twin)
    P = xr * xr + xi_ * xi_
    if noise is None:
        N = dt(np.exp(GAMMA_E)) * np.exp(np.log(P + dt(EPS)).mean(axis=0, dtype=dt))
    else:
        N = np.asarray(noise, dtype=np.float64).astype(dt)
    gmin = dt(10.0) ** (dt(-clip_db(dt(reduce_db))) / dt(20.0))
    g = P / (dt(over) * N + dt(EPS))
    a = dt(alpha)
    G = np.empty((M, K), dtype=dt)
    q = np.ones(K, dtype=dt)
    for m in range(M):
        xi = a * q + (dt(1.0) - a) * np.maximum(g[m] - dt(1.0), dt(0.0))
        G[m] = np.maximum(xi / (dt(1.0) + xi), gmin)
        q = G[m] * G[m] * g[m]
    if src is None:
        sr, si = xr, xi_
    else:
        s64 = np.asarray(src, dtype=np.float64)
        assert s64.shape == x64.shape
        sr, si = spectrum(s64.astype(dt), twin)
    yf = window(twin) * inverse(G * sr, G * si, twin)
    out = np.zeros((M + 1) * H, dtype=dt)
    out[:M * H].reshape(M, H)[...] += yf[:, :H]
    out[H:].reshape(M, H)[...] += yf[:, H:]
    y = out[H:H + n]
    assert y.dtype == dt and G.dtype == dt and N.dtype == dt
    return y, G, N


# ---------------------------------------------------------------------------------------------- the signal recipe
def voiced(n, seed):
    """harmonics (1 / h amplitudes, the top one below 7 kHz) of an f0 gliding between two draws from 90..220 Hz, under a 3 Hz envelope;
    peak 0.5.  float64."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    fa, fb = rng.uniform(90.0, 220.0, size=2)
    f0 = fa + (fb - fa) * np.arange(n) / max(n - 1, 1)
    phase = 2.0 * np.pi * np.cumsum(f0) / FS
    sig = np.zeros(n)
    for h in range(1, int(7000.0 / max(fa, fb)) + 1):
        sig += np.sin(h * phase + 2.0 * np.pi * rng.uniform()) / h
    sig = (0.55 + 0.45 * np.sin(2.0 * np.pi * 3.0 * t + 2.0 * np.pi * rng.uniform())) * sig
    return 0.5 * sig / max(np.abs(sig).max(), 1e-30)


@functools.lru_cache(maxsize=None)
def case(n):
    """x (3, n) float32, read-only: a speech-like harmonic row plus white noise at RMS 0.005 | loud white noise (RMS 0.3) | a row whose
    first half is digital silence and whose second half is the first kind"""
    rng = np.random.default_rng(31 * n + 5)
    a = voiced(n, 1000 * n + 1) + 0.005 * rng.standard_normal(n)
    b = 0.3 * rng.standard_normal(n)
    c = voiced(n, 1000 * n + 3) + 0.005 * rng.standard_normal(n)
    c[:n // 2] = 0.0
    x = np.stack([a, b, c]).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def cotangent(n):
    """dy (3, n) float32, read-only: seeded Gaussian"""
    dy = np.random.default_rng(77 * n + 1).standard_normal((3, n)).astype(np.float32)
    dy.setflags(write=False)
    return dy


@functools.lru_cache(maxsize=None)
def profile(n):
    """a (3, 257) float32 noise profile, read-only: the PSD of white noise at RMS 0.005 under the sine window (sum w^2 = 256), tilted by
    up to +-6 dB over the bins, another tilt per row"""
    k = np.arange(K) / (K - 1)
    p = np.stack([0.005 ** 2 * 256.0 * 10.0 ** (s * (k - 0.5) * 1.2) for s in (-1.0, 0.0, 1.0)]).astype(np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def ref(n, kind="forward", twin=False):
    """the three rows of case(n) through model() at REDUCE_DB: kind "forward" | "backward" (src = cotangent(n)) | "profile" (noise =
    profile(n)); a tuple of (y, G, N) per row, computed once"""
    x = case(n)
    out = []
    for i in range(3):
        kw = {"backward": dict(src=cotangent(n)[i]), "profile": dict(noise=profile(n)[i])}.get(kind, {})
        out.append(model(x[i], REDUCE_DB[i], twin=twin, **kw))
    return tuple(out)


def errors(got, want):
    """(relative L2 of y, max |G - G'|, max |N - N'| / max N) of one row's (y, G, N) against the float64 (y, G, N); a zero y: the absolute L2"""
    y, G, N = (np.asarray(v, dtype=np.float64) for v in got)
    yw, Gw, Nw = want
    ny = np.linalg.norm(yw)
    return (float(np.linalg.norm(y - yw) / ny) if ny > 0 else float(np.linalg.norm(y)), float(np.abs(G - Gw).max()),
            float(np.abs(N - Nw).max() / Nw.max()))


def floors_of(r64, r32):
    """the largest errors() of the float32 twin's rows against the float64 rows: (y, G, N)"""
    e = [errors(b, a) for a, b in zip(r64, r32)]
    return tuple(max(v[j] for v in e) for j in range(3))


def floors(n, kind="forward", rows=(0, 1, 2)):
    r64, r32 = ref(n, kind), ref(n, kind, True)
    return floors_of([r64[i] for i in rows], [r32[i] for i in rows])
