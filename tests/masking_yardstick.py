"""The spectral masking model in numpy from the definition in include/wm_hip.h (the comment of wm_masking_fwd); nothing from the package.

model(x, y) scores one row pair at 16 kHz in float64 and returns a Result: nmr_db, over_db, audible, cells, r (F, 22) and grad, the
analytic d over_db / d y (n,).  model(x, y, twin=True) is the float32 mode: the same steps with every array in float32 and the transform
as an explicit 257 x 512 DFT matrix product (both modes use the matrices, in their own precision), so nothing is silently promoted;
|twin - float64| is what float32 arithmetic costs in SOME order, the floor the GPU bars are multiples of.

The signal recipe: voiced(n, seed) is the harmonics of a gliding f0 under a 3 Hz envelope plus a noise floor; case(n) is three rows of it
with delta = white noise at 1e-4, 1e-3 and 1e-2 of full scale.  case(n) / case_ref(n) are cached: a reference is computed once and never
written to."""
import functools
from collections import namedtuple

import numpy as np

FS = 16000
N, HOP, BINS = 512, 256, 257
BIN_COUNTS = (4, 3, 3, 4, 3, 4, 4, 5, 5, 6, 6, 8, 8, 11, 13, 16, 20, 23, 28, 32, 38, 13)
LEVELS = (1e-4, 1e-3, 1e-2)
HINGE_MARGIN = 1e-4              # no cell of a test input may have |r - 1| below this: about 100 x the float32 floor of r

Result = namedtuple("Result", "nmr_db over_db audible cells r grad")
Tables = namedtuple("Tables", "w c band S G A")


def bark(f):
    f = np.asarray(f, dtype=np.float64)
    return 13.0 * np.arctan(0.00076 * f) + 3.5 * np.arctan((f / 7500.0) ** 2)


def frame_count(n):
    return 1 + (n - N) // HOP if n >= N else 0


@functools.lru_cache(maxsize=None)
def tables64():
    """the six tables of the definition in float64"""
    t = np.arange(N, dtype=np.float64)
    w = 0.5 * (1.0 - np.cos(2.0 * np.pi * t / N))
    c = np.full(BINS, 2.0 * (8.0 / 3.0) / N ** 2)
    c[0] = c[N // 2] = (8.0 / 3.0) / N ** 2
    Z = int(np.floor(bark(FS / 2.0))) + 1
    band = np.minimum(np.floor(bark(np.arange(BINS) * FS / N)).astype(np.int64), Z - 1)
    delta = np.arange(Z)[:, None] - np.arange(Z)[None, :] + 0.474
    S = 10.0 ** ((15.81 + 7.5 * delta - 17.5 * np.sqrt(1.0 + delta ** 2)) / 10.0)
    G = S.sum(axis=1)
    khz = np.arange(BINS) * FS / N / 1000.0
    khz[0] = khz[1]
    ath = 3.64 * khz ** -0.8 - 6.5 * np.exp(-0.6 * (khz - 3.3) ** 2) + 1e-3 * khz ** 4
    A = np.array([0.5 * 10.0 ** ((ath[band == b].min() - 96.0) / 10.0) for b in range(Z)])
    for v in (w, c, band, S, G, A):
        v.setflags(write=False)
    return Tables(w, c, band, S, G, A)


@functools.lru_cache(maxsize=None)
def tables(twin=False):
    """the tables in the mode's precision: float64, or rounded once to float32"""
    t = tables64()
    if not twin:
        return t
    return Tables(*(v if v.dtype.kind == "i" else v.astype(np.float32) for v in t))


@functools.lru_cache(maxsize=None)
def dft(twin=False):
    """(cos, sin) of 2 pi k t / 512 as (512, 257) matrices in the mode's precision, the angle reduced in integers first"""
    kt = np.outer(np.arange(N), np.arange(BINS)) % N
    ang = 2.0 * np.pi * kt / N
    dt = np.float32 if twin else np.float64
    return np.cos(ang).astype(dt), np.sin(ang).astype(dt)


def _frames(v, count):
    return v[HOP * np.arange(count)[:, None] + np.arange(N)[None, :]]


def _band_sums(p, band):
    edges = np.flatnonzero(np.diff(band, prepend=-1))
    return np.add.reduceat(p, edges, axis=1)


def spectra(v, twin=False):
    """(P (F, 257), Dr, Di): the power per bin of the row v and the windowed spectrum's two parts, in the mode's precision"""
    dt = np.float32 if twin else np.float64
    t = tables(twin)
    F = frame_count(v.shape[0])
    vf = t.w * _frames(v.astype(dt), F)
    Cm, Sm = dft(twin)
    re, im = vf @ Cm, -(vf @ Sm)
    P = t.c * (re * re + im * im)
    assert P.dtype == dt
    return P, re, im


def mask(x, twin=False):
    """T (F, 22) of the reference row x"""
    dt = np.float32 if twin else np.float64
    t = tables(twin)
    Px, _, _ = spectra(x, twin)
    Ex = _band_sums(Px, t.band)
    C = Ex @ t.S.T
    inner = Px[:, 1:N // 2]
    tiny = dt(1e-30)
    sfm = dt(10.0) * np.log10(np.exp(np.log(inner + tiny).mean(axis=1, dtype=dt)) / (inner.mean(axis=1, dtype=dt) + tiny))
    alpha = np.clip(sfm / dt(-60.0), dt(0.0), dt(1.0))[:, None]
    b = np.arange(len(BIN_COUNTS)).astype(dt)[None, :]
    O = alpha * (dt(14.5) + b) + (dt(1.0) - alpha) * dt(5.5)
    T = np.maximum(C * dt(10.0) ** (-O / dt(10.0)) / t.G, t.A)
    assert T.dtype == dt
    return T


def model(x, y, twin=False):
    dt = np.float32 if twin else np.float64
    x64, y64 = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    assert x64.ndim == 1 and x64.shape == y64.shape and x64.shape[0] >= 1
    n = x64.shape[0]
    if not (np.isfinite(x64).all() and np.isfinite(y64).all()):
        return Result(float("nan"), float("nan"), 0, 0, None, None)
    F = frame_count(n)
    if F == 0:
        return Result(float("nan"), 0.0, 0, 0, np.zeros((0, len(BIN_COUNTS)), dtype=dt), np.zeros(n, dtype=dt))
    t = tables(twin)
    x, y = x64.astype(dt), y64.astype(dt)
    d = y - x
    T = mask(x, twin)
    Pd, Dr, Di = spectra(d, twin)
    Ed = _band_sums(Pd, t.band)
    r = Ed / T
    cells = r.size
    with np.errstate(divide="ignore"):
        nmr_db = float(dt(10.0) * np.log10(r.mean(dtype=dt)))
        over_db = float(np.maximum(dt(0.0), dt(10.0) * np.log10(r)).mean(dtype=dt))
    hot = r > 1
    g = np.zeros_like(r)
    g[hot] = dt(10.0 / np.log(10.0)) / (dt(cells) * Ed[hot])
    s = dt(2.0) * g[:, t.band] * t.c                                            # (F, 257)
    Cm, Sm = dft(twin)
    u = (s * Dr) @ Cm.T - (s * Di) @ Sm.T                                       # Re sum_k s_k D_k e^(+2 pi i k t / 512)
    gw = t.w * u
    grad = np.zeros(n, dtype=dt)
    grad[:HOP * F].reshape(F, HOP)[...] += gw[:, :HOP]
    grad[HOP:HOP * (F + 1)].reshape(F, HOP)[...] += gw[:, HOP:]
    assert r.dtype == dt and grad.dtype == dt
    return Result(nmr_db, over_db, int(hot.sum()), int(cells), r, grad)


def hinge_distance(res):
    """the smallest |r - 1| over the cells of a float64 Result (inf when it has none)"""
    return float(np.abs(res.r - 1.0).min()) if res.r is not None and res.r.size else float("inf")


# ---------------------------------------------------------------------------------------------- the signal recipe
def voiced(n, seed):
    """harmonics (1 / h amplitudes, the top one below 7 kHz) of an f0 gliding between two draws from 90..220 Hz, under a 3 Hz envelope,
    plus a white noise floor 60 dB below the peak; peak 0.5"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    fa, fb = rng.uniform(90.0, 220.0, size=2)
    f0 = fa + (fb - fa) * np.arange(n) / max(n - 1, 1)
    phase = 2.0 * np.pi * np.cumsum(f0) / FS
    sig = np.zeros(n)
    for h in range(1, int(7000.0 / max(fa, fb)) + 1):
        sig += np.sin(h * phase + 2.0 * np.pi * rng.uniform()) / h
    env = 0.55 + 0.45 * np.sin(2.0 * np.pi * 3.0 * t + 2.0 * np.pi * rng.uniform())
    sig = env * sig
    sig = 0.5 * sig / np.abs(sig).max() + 5e-4 * rng.standard_normal(n)
    return sig.astype(np.float32)


SALT = {}                        # n -> a seed offset, where the plain seeds put a cell within HINGE_MARGIN of the hinge


@functools.lru_cache(maxsize=None)
def case(n):
    """(x (3, n), y (3, n)) float32, read-only: row i is y = x + white noise at LEVELS[i] of full scale"""
    salt = SALT.get(n, 0)
    xs, ys = [], []
    for i, level in enumerate(LEVELS):
        x = voiced(n, 1000 * n + i + salt)
        z = np.random.default_rng(7000 * n + i + salt).standard_normal(n)
        xs.append(x)
        ys.append((x + level * z).astype(np.float32))
    x, y = np.stack(xs), np.stack(ys)
    x.setflags(write=False); y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def case_ref(n):
    """([Result per row] in float64, [Result per row] of the float32 mode)"""
    x, y = case(n)
    return tuple(model(a, b) for a, b in zip(x, y)), tuple(model(a, b, twin=True) for a, b in zip(x, y))


def floors_of(r64, r32):
    """(nmr_db, over_db, gradient) floors of rows scored in both modes: the float32 mode against float64, absolute for the two dB numbers
    (over rows with a finite score), relative L2 for a row's gradient (over rows whose gradient is not zero)"""
    fn = max([abs(a.nmr_db - b.nmr_db) for a, b in zip(r64, r32) if np.isfinite(a.nmr_db)], default=0.0)
    fo = max([abs(a.over_db - b.over_db) for a, b in zip(r64, r32) if np.isfinite(a.over_db)], default=0.0)
    fg = max([float(np.linalg.norm(b.grad - a.grad) / np.linalg.norm(a.grad)) for a, b in zip(r64, r32) if a.grad is not None and np.any(a.grad)],
             default=0.0)
    return fn, fo, fg


def floors(n, rows=(0, 1, 2)):
    """floors_of the given rows of case(n)"""
    r64, r32 = case_ref(n)
    return floors_of([r64[i] for i in rows], [r32[i] for i in rows])
