"""The clip-curation features (the comment of wm_clip_features in include/wm_hip.h) stated in numpy, with a dtype argument, and the test
inputs.  Nothing here comes from the package.  float64: scipy.signal.butter + lfilter in transfer-function form, as the reference's
noise.py runs them.  float32: the same definition with every array and every intermediate in float32 and the band-pass as sosfilt on
float32 sections -- the arithmetic class of the kernel; its distance from the float64 run is the measure the GPU tests scale their
tolerance by."""
import math
from collections import namedtuple

import numpy as np
from scipy import signal

N_FFT, HOP, N_MELS, N_MFCC = 2048, 512, 128, 13
FEATURES = ("duration", "energy", "speech_band_energy", "zero_crossing_rate", "spectral_centroid", "spectral_bandwidth", "rolloff",
            "mfcc_mean", "mfcc_var", "kurtosis", "energy_std", "speech_to_noise_ratio", "rms")
# (column, threshold, the comparison that scores, points)
RULES = (("speech_band_energy", 0.001, ">", 1), ("zero_crossing_rate", 0.1, "<", 1), ("spectral_centroid", 3000.0, "<", 1),
         ("kurtosis", 5.0, ">", 1), ("energy_std", 0.01, ">", 1), ("speech_to_noise_ratio", 0.6, ">", 2))
KINDS = ("voiced", "noise", "quiet", "hum", "clicks", "brown")
QUIET_LEVELS = (2e-5, 5e-5, 1.5e-4, 2e-4)       # straddling silent.py's 1e-4, none within a third of it

Result = namedtuple("Result", "feat zc score finite frames")


def mel_corners(sr, n_mels=N_MELS):
    def to_mel(f):
        return f / (200.0 / 3.0) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)

    def to_hz(m):
        return (200.0 / 3.0) * m if m < 15.0 else 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0))
    top = to_mel(0.5 * sr)
    return np.array([to_hz(top * i / (n_mels + 1)) for i in range(n_mels + 2)])


def mel_table(sr, n_fft=N_FFT, n_mels=N_MELS):
    """(n_mels, n_fft / 2 + 1) float64, triangle by triangle"""
    f = mel_corners(sr, n_mels)
    bins = np.arange(n_fft // 2 + 1) * (sr / n_fft)
    fb = np.zeros((n_mels, bins.size))
    for m in range(n_mels):
        up = (bins - f[m]) / (f[m + 1] - f[m])
        down = (f[m + 2] - bins) / (f[m + 2] - f[m + 1])
        fb[m] = np.maximum(0.0, np.minimum(up, down)) * 2.0 / (f[m + 2] - f[m])
    return fb


def dct_table(n_out=N_MFCC, n_in=N_MELS):
    d = np.zeros((n_out, n_in))
    for k in range(n_out):
        for m in range(n_in):
            d[k, m] = math.sqrt((1.0 if k == 0 else 2.0) / n_in) * math.cos(math.pi * k * (2 * m + 1) / (2.0 * n_in))
    return d


def frame_count(n):
    return 1 + n // HOP


def features(x, sr=16000, dtype=np.float64):
    """Result of the rows x (rows, n): feat (rows, 13) in FEATURES' order, zc (rows,) the zero-crossing totals, score (rows,), finite
    (rows,) and frames (rows, F, 4) = centroid, bandwidth, roll-off bin, zero-crossing count, all in `dtype` arithmetic"""
    dt = np.dtype(dtype).type
    x = np.asarray(x)
    rows, n = x.shape
    finite = np.isfinite(x).all(axis=1)
    y = np.where(finite[:, None], x, 0).astype(dt)
    F = frame_count(n)
    col = {name: i for i, name in enumerate(FEATURES)}
    feat = np.zeros((rows, len(FEATURES)), dtype=dt)
    feat[:, col["duration"]] = dt(n) / dt(sr)
    energy = (y * y).mean(axis=1, dtype=dt)
    feat[:, col["energy"]] = energy
    feat[:, col["rms"]] = np.sqrt(energy)
    wn = [300.0 / (0.5 * sr), 3000.0 / (0.5 * sr)]
    if dt is np.float64:
        b, a = signal.butter(5, wn, btype="band")
        z = signal.lfilter(b, a, y, axis=1)
    else:
        z = signal.sosfilt(signal.butter(5, wn, btype="band", output="sos").astype(dt), y, axis=1)
        assert z.dtype == dt
    sbe = (z * z).mean(axis=1, dtype=dt)
    feat[:, col["speech_band_energy"]] = sbe
    feat[:, col["speech_to_noise_ratio"]] = sbe / (energy + dt(1e-10))
    idx = HOP * np.arange(F)[:, None] + np.arange(N_FFT)[None, :]
    edge = np.pad(y, ((0, 0), (N_FFT // 2, N_FFT // 2)), mode="edge")[:, idx]
    edge = np.where(np.abs(edge) <= dt(1e-10), dt(0), edge)
    sign = np.signbit(edge)
    zc = (sign[:, :, 1:] != sign[:, :, :-1]).sum(axis=2)
    feat[:, col["zero_crossing_rate"]] = (zc.sum(axis=1) / dt(F * N_FFT)).astype(dt)
    window = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)).astype(dt)
    padded = np.pad(y, ((0, 0), (N_FFT // 2, N_FFT // 2)))[:, idx]
    S = np.abs(np.fft.rfft(padded * window, axis=2)).astype(dt)
    assert S.dtype == dt
    freq = (np.arange(N_FFT // 2 + 1) * (sr / N_FFT)).astype(dt)
    tot = S.sum(axis=2, dtype=dt)
    ok = tot >= np.finfo(np.float32).tiny
    safe = np.where(ok, tot, dt(1))
    cen = np.where(ok, (S * freq).sum(axis=2, dtype=dt) / safe, dt(0))
    bw = np.where(ok, np.sqrt(((S / safe[:, :, None]) * (freq[None, None, :] - cen[:, :, None]) ** 2).sum(axis=2, dtype=dt)), dt(0))
    ro = np.where(ok, (np.cumsum(S, axis=2, dtype=dt) >= dt(0.85) * tot[:, :, None]).argmax(axis=2), 0)
    feat[:, col["spectral_centroid"]] = cen.mean(axis=1, dtype=dt)
    feat[:, col["spectral_bandwidth"]] = bw.mean(axis=1, dtype=dt)
    feat[:, col["rolloff"]] = (ro.astype(dt) * dt(sr / N_FFT)).mean(axis=1, dtype=dt)
    fb = mel_table(sr).astype(np.float32).astype(dt)                       # built in float64, rounded to float32: the table the kernel reads
    mel = (S * S) @ fb.T
    dB = dt(10) * np.log10(np.maximum(dt(1e-10), mel))
    dB = np.maximum(dB, dB.max(axis=(1, 2), keepdims=True) - dt(80))
    mfcc = dB @ dct_table().astype(np.float32).astype(dt).T
    assert mfcc.dtype == dt
    feat[:, col["mfcc_mean"]] = mfcc.mean(axis=1, dtype=dt).mean(axis=1, dtype=dt)
    feat[:, col["mfcc_var"]] = mfcc.var(axis=1, dtype=dt).mean(axis=1, dtype=dt)
    d = y - y.mean(axis=1, keepdims=True, dtype=dt)
    m2, m4 = (d ** 2).mean(axis=1, dtype=dt), (d ** 4).mean(axis=1, dtype=dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        feat[:, col["kurtosis"]] = m4 / (m2 * m2) - dt(3)
    length, hop = int(sr * 0.025), int(sr * 0.010)
    count = 1 + (n - length) // hop
    fr = y[:, hop * np.arange(count)[:, None] + np.arange(length)[None, :]]
    feat[:, col["energy_std"]] = (fr * fr).mean(axis=2, dtype=dt).std(axis=1, dtype=dt)
    feat[~finite] = np.nan
    score = np.where(finite, score_of(feat), 0)
    frames = np.stack([cen, bw, ro.astype(dt), zc.astype(dt)], axis=2)
    frames[~finite] = np.nan
    return Result(feat, np.where(finite, zc.sum(axis=1), 0), score, finite, frames)


def score_of(feat):
    """noise.py's classify_speech_noise, rule by rule; a comparison with NaN is false"""
    col = {name: i for i, name in enumerate(FEATURES)}
    total = np.zeros(feat.shape[0], dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for name, thr, op, points in RULES:
            v = feat[:, col[name]].astype(np.float64)
            total += points * ((v > thr) if op == ">" else (v < thr))
    return total


def threshold_margin(feat):
    """per row, the smallest relative distance of a scored feature from its threshold"""
    col = {name: i for i, name in enumerate(FEATURES)}
    with np.errstate(invalid="ignore"):
        return np.min(np.stack([np.abs(feat[:, col[name]].astype(np.float64) - thr) / thr for name, thr, _, _ in RULES]), axis=0)


def rel_error(got, ref):
    """per feature (13,), the worst over rows of |got - ref| / |ref| -- for the kurtosis |got - ref| / (|ref| + 3)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    den = np.abs(ref)
    den[:, FEATURES.index("kurtosis")] += 3.0
    den = np.maximum(den, np.finfo(np.float64).tiny)
    return (np.abs(got - ref) / den).max(axis=0)


def make_rows(rows, n, sr=16000, seed=0):
    """(rows, n) float32: six kinds of clip cycled over the rows, every row from its own generator"""
    t = np.arange(n) / sr
    out = np.zeros((rows, n), dtype=np.float32)
    for r in range(rows):
        rng = np.random.default_rng([seed, r, n, sr])
        kind = KINDS[r % len(KINDS)]
        if kind == "voiced":                     # harmonics of f0 under three formants, syllable bursts at 2-5 Hz
            f0 = rng.uniform(90.0, 220.0)
            formants = ((rng.uniform(500, 800), 90.0), (rng.uniform(1200, 1800), 120.0), (rng.uniform(2500, 3000), 160.0))
            v = np.zeros(n)
            for h in range(1, int(3800.0 / f0) + 1):
                amp = sum(1.0 / (1.0 + ((h * f0 - fc) / bw) ** 2) for fc, bw in formants)
                v += amp * np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 2 * np.pi))
            env = 0.05 + 0.95 * np.maximum(0.0, np.sin(2 * np.pi * rng.uniform(2.0, 5.0) * t + rng.uniform(0, np.pi))) ** 2
            v = v * env
            v *= 0.6 / np.abs(v).max()
        elif kind == "noise":
            v = rng.uniform(0.01, 0.3) * rng.standard_normal(n)
        elif kind == "quiet":
            v = QUIET_LEVELS[(r // len(KINDS)) % len(QUIET_LEVELS)] * rng.standard_normal(n)
        elif kind == "hum":
            v = 0.3 * np.sin(2 * np.pi * rng.uniform(40.0, 70.0) * t + rng.uniform(0, 2 * np.pi)) + 0.01 * rng.standard_normal(n)
        elif kind == "clicks":
            v = np.zeros(n)
            v[rng.choice(n, size=5, replace=False)] = rng.uniform(0.5, 0.95, size=5) * rng.choice([-1.0, 1.0], size=5)
        else:
            v = np.cumsum(rng.standard_normal(n))
            v -= v.mean()
            v *= 0.5 / np.abs(v).max()
        out[r] = v.astype(np.float32)
    return out


_CACHE = {}


def case(rows, n, sr=16000):
    """(x, float64 Result, float32 Result) of make_rows(rows, n, sr), computed once and shared; do not write to them"""
    key = (rows, n, sr)
    if key not in _CACHE:
        x = make_rows(rows, n, sr)
        _CACHE[key] = (x, features(x, sr, np.float64), features(x, sr, np.float32))
    return _CACHE[key]
