"""The float64 yardstick of the predictive speech-codec stand-in (wm_lpc_codec, attacks.LpcCodec), written from the definition in
include/wm_hip.h.  Numpy alone; nothing from the package.  Every function takes `dtype`: float64 is the reference, float32 the yardstick's
own restatement in the kernel's number format, whose distance from float64 sizes the tolerances of tests/test_gpu_lpc_codec.py.  The
tables (window, lag window, bandwidth expansion) are part of the definition as float32 numbers, so both modes use the rounded values."""
import functools

import numpy as np

from mdct_yardstick import signal as _mdct_signal
from yardstick_common import U, gamma

SNR_DB = (10.0, 20.0, 30.0)                       # row r gets SNR_DB[r % 3]
FLOOR_STEP = 2.0 ** -15
ORDERS = ("lanes", "numpy", "seq", "rev")         # float32 summation orders of the autocorrelation: the header's 64-lane tree and three others
# the issue's shapes: (L, p, n)
SHAPES = ([(160, p, n) for p in (2, 10) for n in (1, 159, 160, 161, 4 * 160 + 3, 16000)] + [(320, 16, n) for n in (4 * 320 + 3, 16000)]
          + [(640, 16, 3 * 640 + 5)])
GPU_CASES = [(rows, L, p, n) for rows in (1, 3) for (L, p, n) in SHAPES]
LONG_CASES = [c for c in GPU_CASES if c[3] >= 3 * c[1]]           # rows of several frames: where a prediction gain means something


def snr_rows(rows):
    return np.array([SNR_DB[r % 3] for r in range(rows)], dtype=np.float32)


def frames(n, L):
    return -(-n // L)


# ------------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def signal_plain(rows, n):
    """mdct_yardstick.signal: white noise plus a 440 Hz tone.  Well conditioned, about 4 dB of prediction gain."""
    x = _mdct_signal(rows, n)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def signal_speech(rows, n):
    """Speech-like rows from default_rng(1): row r is 0.3 * normal plus a pulse train of height 8 and period 100 + 17 r, through three
    two-pole resonators at (500 + 100 r, 80), (1500, 120), (2500, 160) Hz (centre, bandwidth), 200 warm-up samples dropped, times the
    envelope 0.5 + 0.5 sin(2 pi 3 t / 16000 + r), peak set to 0.3; float32.  25-30 dB of prediction gain."""
    m = n + 200
    ex = 0.3 * np.random.default_rng(1).standard_normal((rows, m))
    r = np.arange(rows)
    for i in range(rows):
        ex[i, ::100 + 17 * i] += 8.0
    for fc, bw in ((500.0 + 100.0 * r, 80.0), (1500.0, 120.0), (2500.0, 160.0)):
        rad = np.exp(-np.pi * bw / 16000.0)
        c1, c2 = 2.0 * rad * np.cos(2.0 * np.pi * (fc + 0.0 * r) / 16000.0), -rad * rad
        y = np.zeros((rows, m + 2))
        for t in range(m):
            y[:, t + 2] = ex[:, t] + c1 * y[:, t + 1] + c2 * y[:, t]
        ex = y[:, 2:]
    x = ex[:, 200:] * (0.5 + 0.5 * np.sin(2.0 * np.pi * 3.0 * np.arange(n) / 16000.0 + r[:, None]))
    x = (0.3 * x / np.abs(x).max(axis=1, keepdims=True)).astype(np.float32)
    x.setflags(write=False)
    return x


def degenerate(n):
    """(4, n): an all-zero row, a row at amplitude 1e-7 (everything under the floor step), a pure 440 Hz tone and a constant 0.5 row (the
    last two with reflection coefficients near -1 and +1)"""
    x = np.array(signal_plain(4, n))
    x[0] = 0
    x[1] *= np.float32(1e-7) / np.abs(x[1]).max()
    x[2] = (0.2 * np.sin(2 * np.pi * 440 * np.arange(n) / 16000)).astype(np.float32)
    x[3] = 0.5
    return x


# ------------------------------------------------------------------------------------------------------------------------ tables
def window(L):
    j = np.arange(2 * L, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * (j + 0.5) / (2 * L))).astype(np.float32)


def tables(p, sample_rate=16000):
    """(lag (p + 1,), expand (p,)) as float32: evaluated in float64, rounded once"""
    k = np.arange(p + 1, dtype=np.float64)
    lag = np.exp(-0.5 * (2.0 * np.pi * 60.0 * k / sample_rate) ** 2)
    lag[0] = 1.0 + 1e-4
    return lag.astype(np.float32), (0.994 ** k[1:]).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------ sums
def _sum(v, dtype, order):
    """the sum of v over its last axis in dtype, in one of ORDERS; "lanes" is the header's: 64 chains over j = l, l + 64, ..., then the xor
    butterfly 32 .. 1"""
    v = np.asarray(v, dtype=dtype)
    if order == "numpy":
        return v.sum(axis=-1, dtype=dtype)
    if order == "seq":
        return np.cumsum(v, axis=-1, dtype=dtype)[..., -1]
    if order == "rev":
        return np.cumsum(v[..., ::-1], axis=-1, dtype=dtype)[..., -1]
    m = v.shape[-1]
    per = -(-m // 64)
    pad = np.zeros(v.shape[:-1] + (per * 64,), dtype=dtype)
    pad[..., :m] = v
    pad = pad.reshape(v.shape[:-1] + (per, 64))
    acc = np.zeros(v.shape[:-1] + (64,), dtype=dtype)
    for i in range(per):
        acc = acc + pad[..., i, :]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lanes ^ o]
    return acc[..., 0]


def segments(x, L, dtype):
    """s (rows, F, 2L): the windowed segments, one product each"""
    x = np.asarray(x, dtype=dtype)
    rows, n = x.shape
    F = frames(n, L)
    xp = np.zeros((rows, L // 2 + F * L + L), dtype=dtype)
    xp[:, L // 2:L // 2 + n] = x
    return np.stack([xp[:, f * L:f * L + 2 * L] for f in range(F)], axis=1) * window(L).astype(dtype)


def levinson(Rc, p, dtype):
    """Levinson-Durbin as the header words it, over all leading axes of Rc (..., p + 1): a (..., p) before the expansion"""
    one, zero = dtype(1), dtype(0)
    a = np.zeros(Rc.shape[:-1] + (p + 1,), dtype=dtype)
    E = Rc[..., 0].copy()
    go = E > 0
    E = np.where(go, E, one)
    for i in range(1, p + 1):
        acc = Rc[..., i].copy()
        for j in range(1, i):
            acc = acc + a[..., j] * Rc[..., i - j]
        k = -acc / E
        go = go & (np.abs(k) < 1)
        k = np.where(go, k, zero).astype(dtype)
        a[..., 1:i] = a[..., 1:i] + k[..., None] * a[..., i - 1:0:-1]
        a[..., i] = k
        E = (E * (one - k * k)).astype(dtype)
    return a[..., 1:]


def analyse(x, L, p, dtype=np.float64, order="lanes", sample_rate=16000):
    """dict(coeffs (rows, F, p) after the expansion, Rc (rows, F, p + 1)) in dtype"""
    lag, expand = (t.astype(dtype) for t in tables(p, sample_rate))
    s = segments(x, L, dtype)
    R = np.stack([_sum(s[..., :2 * L - k] * s[..., k:], dtype, order) for k in range(p + 1)], axis=-1)
    Rc = (R * lag).astype(dtype)
    return {"coeffs": (levinson(Rc, p, dtype) * expand).astype(dtype), "Rc": Rc}


def coeff_bound(x, L, p, sample_rate=16000):
    """(coeffs64, bound), both (rows, F, p): the first-order perturbation bound of the normal equations T a = -r under a float32
    autocorrelation in ANY summation order,  2 expand[k] (|T^-1| (|dT| |a| + |dr|))[k]  with  dR[k] = (gamma(2L) + 6U) lag[k] sum_j |s[j]| |s[j+k]|;
    the factor 2 covers the recursion's own roundings and the second-order terms.  A frame with Rc[0] = 0 has bound 0 (its
    coefficients are exactly 0 in any arithmetic)."""
    lag, expand = (t.astype(np.float64) for t in tables(p, sample_rate))
    ref = analyse(x, L, p)
    s = np.abs(segments(x, L, np.float64))
    dR = (gamma(2 * L) + 6 * U) * lag * np.stack([(s[..., :2 * L - k] * s[..., k:]).sum(axis=-1) for k in range(p + 1)], axis=-1)
    rows, F = dR.shape[:2]
    idx = np.abs(np.arange(p)[:, None] - np.arange(p)[None, :])
    bound = np.zeros((rows, F, p))
    for r in range(rows):
        for f in range(F):
            Rc = ref["Rc"][r, f]
            if not Rc[0] > 0:
                continue
            a = ref["coeffs"][r, f] / expand
            Tinv = np.abs(np.linalg.inv(Rc[idx]))
            bound[r, f] = 2 * expand * (Tinv @ (dR[r, f][idx] @ np.abs(a) + dR[r, f][1:]))
    return ref["coeffs"], bound


# ------------------------------------------------------------------------------------------------------------------------ the codec
def _per_sample(coeffs, L, n, dtype):
    return np.repeat(np.asarray(coeffs, dtype=dtype), L, axis=1)[:, :n]                            # (rows, n, p): the set of f(t)


def residual(x, coeffs, L, dtype=np.float64):
    x = np.asarray(x, dtype=dtype)
    rows, n = x.shape
    p = coeffs.shape[-1]
    at = _per_sample(coeffs, L, n, dtype)
    hist = np.zeros((rows, n + p), dtype=dtype)
    hist[:, p:] = x
    e = x.copy()
    for k in range(1, p + 1):
        e = e + at[:, :, k - 1] * hist[:, p - k:p - k + n]
    return e


def synthesis(eq, coeffs, L, dtype=np.float64):
    eq = np.asarray(eq, dtype=dtype)
    rows, n = eq.shape
    p = coeffs.shape[-1]
    ar = np.ascontiguousarray(_per_sample(coeffs, L, n, dtype)[:, :, ::-1])
    y = np.zeros((rows, n + p), dtype=dtype)
    for t in range(n):
        y[:, p + t] = eq[:, t] - (ar[:, t] * y[:, t:t + p]).sum(axis=1, dtype=dtype)
    return y[:, p:]


def codec(x, coeffs, L, snr_db, floor_step=FLOOR_STEP, quantise=True, codes=None, mask=None, dtype=np.float64, synth=True):
    """x (rows, n), coeffs (rows, F, p) -> dict(e, step (rows, n), r = e / step, codes int64, eq, y), all in dtype.  codes given: they
    replace rint(r) (teacher forcing).  synth=False leaves y out."""
    rows, n = np.shape(x)
    F = frames(n, L)
    e = residual(x, coeffs, L, dtype)
    out = {"e": e}
    if quantise:
        ep = np.zeros((rows, F * L), dtype=dtype)
        ep[:, :n] = e
        cnt = np.minimum(L, n - L * np.arange(F)).astype(dtype)
        P = (_sum(ep.reshape(rows, F, L) ** 2, dtype, "lanes") / cnt).astype(dtype)
        snr = np.nan_to_num(np.asarray(snr_db, dtype=np.float64), nan=0.0).clip(0, 60)
        g = (10.0 ** (-snr / 20.0)).astype(np.float32).astype(dtype).reshape(rows, 1)
        step = np.repeat(np.maximum(np.sqrt(dtype(12) * P) * g, dtype(floor_step)), L, axis=1)[:, :n].astype(dtype)
        r = e / step
        q = np.rint(r).astype(np.int64) if codes is None else np.asarray(codes, dtype=np.int64)
        eq = (q.astype(dtype) * step).astype(dtype)
        out.update(step=step, r=r, codes=q)
    else:
        eq = e.copy()
    if mask is not None:
        eq = np.where(np.asarray(mask) != 0, eq, dtype(0))
    out["eq"] = eq
    if synth:
        out["y"] = synthesis(eq, coeffs, L, dtype)
    return out


def adjoint(g, coeffs, L, mask=None, dtype=np.float64):
    """dx of the header's adjoint mode: the coefficient of a term is that of the frame of the sample it comes FROM"""
    g = np.asarray(g, dtype=dtype)
    rows, n = g.shape
    p = coeffs.shape[-1]
    at = _per_sample(coeffs, L, n, dtype)
    B = np.zeros((rows, n, p), dtype=dtype)                                                        # B[:, t, k - 1] = a_f(t + k)[k], 0 past the row
    for k in range(1, min(p, n - 1) + 1):
        B[:, :n - k, k - 1] = at[:, k:, k - 1]
    u = np.zeros((rows, n + p), dtype=dtype)
    for t in range(n - 1, -1, -1):
        u[:, t] = g[:, t] - (B[:, t] * u[:, t + 1:t + p + 1]).sum(axis=1, dtype=dtype)
    v = u.copy()
    if mask is not None:
        v[:, :n] = np.where(np.asarray(mask) != 0, v[:, :n], dtype(0))
    dx = v[:, :n].copy()
    for k in range(1, p + 1):
        dx = dx + B[:, :, k - 1] * v[:, k:k + n]
    return dx


def prediction_gain_db(x, coeffs, L):
    """per row, in float64: 10 log10(sum x^2 / sum e^2) with these coefficients"""
    x = np.asarray(x, dtype=np.float64)
    e = residual(x, np.asarray(coeffs, dtype=np.float64), L)
    return 10.0 * np.log10((x ** 2).sum(axis=1) / (e ** 2).sum(axis=1))


def near_tie(x, coeffs, L, snr_db, floor_step=FLOOR_STEP):
    """(tie, share, codes64, h) with the given coefficients in both modes: tie marks the samples whose r64 = e / step lies within
    h = 8 max|r32 - r64| of a half-integer"""
    a = codec(x, coeffs, L, snr_db, floor_step, synth=False)
    b = codec(x, coeffs, L, snr_db, floor_step, dtype=np.float32, synth=False)
    h = 8.0 * float(np.abs(b["r"].astype(np.float64) - a["r"]).max())
    tie = np.abs(a["r"] - np.floor(a["r"]) - 0.5) <= h
    return tie, float(tie.mean()), a["codes"], h


def e32_output(x, coeffs, L, snr_db, codes, mask=None, quantise=True, floor_step=FLOOR_STEP):
    """(E32y, y64): the float32 mode against float64 on the same coefficients and codes"""
    a = codec(x, coeffs, L, snr_db, floor_step, quantise, codes=codes, mask=mask)
    b = codec(x, coeffs, L, snr_db, floor_step, quantise, codes=codes, mask=mask, dtype=np.float32)
    return float(np.abs(b["y"].astype(np.float64) - a["y"]).max()), a["y"]


def e32_adjoint(g, coeffs, L, mask=None):
    a = adjoint(g, coeffs, L, mask)
    b = adjoint(g, coeffs, L, mask, dtype=np.float32)
    return float(np.abs(b.astype(np.float64) - a).max()), a


# ------------------------------------------------------------------------------------------------------------------------ refusals
# wm_lpc_codec(x, y, coeffs_in, coeffs_out, codes_out, mask_in, snr_db, lag, expand, rows, n, L, p, floor_step, quantise, adjoint, stream).
# Addresses that are never dereferenced: every tuple is refused before anything is launched.  At (2, 1000), L = 320, p = 16: x and y 8000
# bytes, coefficients 2 x 4 x 16 floats = 512 bytes, codes and mask 4000 bytes.
_X, _Y, _CI, _CO, _Q, _M, _S, _LG, _EX = (0x10000 * (i + 1) for i in range(9))
_FS = FLOOR_STEP
BAD_ARGS = ((_X, _Y, None, None, None, None, _S, _LG, _EX, 0, 1000, 320, 16, _FS, 1, 0, None),            # rows, n out of range
            (_X, _Y, None, None, None, None, _S, _LG, _EX, 2, 0, 320, 16, _FS, 1, 0, None),
            (_X, _Y, None, None, None, None, _S, _LG, _EX, 1, (1 << 34) + 1, 320, 16, _FS, 1, 0, None),
            (_X, _Y, None, None, None, None, _S, _LG, _EX, (1 << 12) + 1, 1 << 34, 320, 16, _FS, 1, 0, None),
            (_X, _Y, None, None, None, None, _S, _LG, _EX, 2, 1000, 256, 16, _FS, 1, 0, None),             # L outside {160, 320, 640}
            (_X, _Y, None, None, None, None, _S, _LG, _EX, 2, 1000, 0, 16, _FS, 1, 0, None),
            (_X, _Y, None, None, None, None, _S, _LG, _EX, 2, 1000, 1280, 16, _FS, 1, 0, None),
            (_X, _Y, None, None, None, None, _S, _LG, _EX, 2, 1000, 320, 1, _FS, 1, 0, None),              # p outside 2 .. 16
            (_X, _Y, None, None, None, None, _S, _LG, _EX, 2, 1000, 320, 17, _FS, 1, 0, None),
            (None, _Y, None, None, None, None, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 1, 0, None),           # null pointers
            (_X, None, None, None, None, None, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 1, 0, None),
            (_X, _Y, None, None, None, None, None, _LG, _EX, 2, 1000, 320, 16, _FS, 1, 0, None),
            (_X, _Y, None, None, None, None, _S, None, _EX, 2, 1000, 320, 16, _FS, 1, 0, None),
            (_X, _Y, None, None, None, None, _S, _LG, None, 2, 1000, 320, 16, _FS, 1, 0, None),
            (_X + 2, _Y, None, None, None, None, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 1, 0, None),         # misaligned
            (_X, _Y + 1, None, None, None, None, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 1, 0, None),
            (_X, _Y, _CI + 2, None, None, None, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 1, 0, None),
            (_X, _Y, None, _CO + 2, None, None, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 1, 0, None),
            (_X, _Y, None, None, _Q + 1, None, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 1, 0, None),
            (_X, _Y, None, None, None, _M + 1, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 1, 0, None),
            (_X, _Y, None, None, None, None, _S + 2, _LG, _EX, 2, 1000, 320, 16, _FS, 1, 0, None),
            (_X, _Y, None, None, None, None, _S, _LG + 1, _EX, 2, 1000, 320, 16, _FS, 1, 0, None),
            (_X, _Y, None, None, None, None, _S, _LG, _EX + 3, 2, 1000, 320, 16, _FS, 1, 0, None),
            (_X, _Y, None, None, None, None, _S, _LG, _EX, 2, 1000, 320, 16, 0.0, 1, 0, None),             # floor_step
            (_X, _Y, None, None, None, None, _S, _LG, _EX, 2, 1000, 320, 16, -1.0, 1, 0, None),
            (_X, _Y, None, None, None, None, _S, _LG, _EX, 2, 1000, 320, 16, float("nan"), 1, 0, None),
            (_X, _Y, None, None, None, None, _S, _LG, _EX, 2, 1000, 320, 16, float("inf"), 1, 0, None),
            (_X, _Y, None, None, _Q, None, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 0, 0, None),               # codes without the quantiser
            (_X, _Y, None, None, None, None, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 0, 1, None),             # the adjoint: no coefficients,
            (_X, _Y, _CI, None, None, None, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 1, 1, None),              # the quantiser on,
            (_X, _Y, _CI, _CO, None, None, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 0, 1, None),               # coefficients or codes out
            (_X, _X, None, None, None, None, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 1, 0, None),             # in place and overlaps
            (_X, _X + 7996, None, None, None, None, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 1, 0, None),
            (_X, _CI + 508, _CI, None, None, None, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 0, 0, None),
            (_X, _Y, None, _X + 7996, None, None, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 1, 0, None),
            (_X, _Y, None, None, _Y + 7998, None, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 1, 0, None),
            (_X, _Y, None, None, _M + 3998, _M, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 1, 0, None),
            (_X, _M + 3996, _CI, None, None, _M, _S, _LG, _EX, 2, 1000, 320, 16, _FS, 0, 1, None))         # the adjoint's dx over its mask
