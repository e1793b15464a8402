"""Clip curation: from recordings to the one-second clips the train and evaluation paths assume.  The reference does this on the CPU in
three scripts -- dataset_creation/1_sec_files.py (resample, normalise to a peak of 0.99, cut into one-second files), silent.py (rms below
1e-4) and noise.py (a feature table per file through librosa and scipy, then classify_speech_noise's fixed thresholds) -- with a process
pool over hours.  Here every clip's features come from ONE wm_clip_features launch (csrc/clip_features.hip; the definition is the comment
of wm_clip_features in include/wm_hip.h), and a recording is resampled, normalised and cut on the device by launches the package already
has.

CPU tensors take clip_features_host, the definition restated in float64 numpy.  What is unmeasured: librosa is not a dependency and was
never run beside this; parity with librosa 0.10 rests on the restated definition (librosa before 0.10 pads the STFT by reflection, not with
zeros).  The thresholds are the reference's heuristics; nothing here says they classify well."""
from __future__ import annotations

import csv
import math
import os
from collections import OrderedDict

import numpy as np
import torch

N_FFT, HOP, N_MELS, N_MFCC = 2048, 512, 128, 13
MIN_SAMPLES, MAX_SAMPLES = 400, 32768
BAND = (300.0, 3000.0)
SILENCE_RMS = 1e-4
FEATURES = ("duration", "energy", "speech_band_energy", "zero_crossing_rate", "spectral_centroid", "spectral_bandwidth", "rolloff",
            "mfcc_mean", "mfcc_var", "kurtosis", "energy_std", "speech_to_noise_ratio", "rms")
FEAT_COLUMNS = 16                                # wm_clip_features writes rows of 16: FEATURES, then three reserved zeros
SPEECH, NOISE, ERROR = 1, 0, -1
LABEL_NAMES = {SPEECH: "speech", NOISE: "noise", ERROR: "error"}
CLASSES = ("speech", "noise", "silent")          # what by_class reports: a silent clip is "silent" whatever its score
_TINY = float(np.finfo(np.float32).tiny)
_HOST_CHUNK = 32


# ---------------------------------------------------------------------------------------------- tables
def butter_bandpass_sos(low, high, sr, order=5):
    """The Butterworth band-pass scipy.signal.butter(order, [low, high] / (sr / 2), 'band') as second-order sections, (order, 6) float64
    rows b0 b1 b2 1 a1 a2, in plain numpy: the analogue prototype's poles, the low-pass to band-pass transform around the pre-warped
    edges, the bilinear transform, each pole paired with its conjugate (real poles with one another, in rising order), one zero at +1
    and one at -1 per section.  The gain is spread evenly over the sections (fp32 cascades keep their intermediate signals near the
    input's scale) and the sections are ordered by rising pole radius; the product of the sections is scipy's transfer function."""
    if isinstance(order, bool) or not isinstance(order, int) or order < 1:
        raise ValueError(f"order: expected a positive int, got {order!r}")
    low, high, sr = float(low), float(high), float(sr)
    if not (0.0 < low < high < 0.5 * sr):
        raise ValueError(f"band: expected 0 < low < high < sr / 2, got low = {low}, high = {high}, sr = {sr}")
    fs = 2.0
    w0, w1 = (2.0 * fs * math.tan(math.pi * f / (0.5 * sr) / fs) for f in (low, high))
    bw, wo = w1 - w0, math.sqrt(w0 * w1)
    proto = -np.exp(1j * np.pi * np.arange(-order + 1, order, 2) / (2.0 * order))
    lp = proto * bw / 2.0
    root = np.sqrt(lp * lp - wo * wo + 0j)
    ps = np.concatenate([lp + root, lp - root])
    gain = bw ** order
    pz = (2.0 * fs + ps) / (2.0 * fs - ps)
    gain *= float(np.real((2.0 * fs) ** order / np.prod(2.0 * fs - ps)))
    tol = 1e-12
    cplx = sorted((p for p in pz if p.imag > tol), key=abs)
    real = sorted(p.real for p in pz if abs(p.imag) <= tol)
    if 2 * len(cplx) + len(real) != 2 * order or len(real) % 2:
        raise ValueError("the poles do not pair: the band is too close to 0 or to sr / 2")
    dens = [(1.0, -2.0 * p.real, abs(p) ** 2, abs(p)) for p in cplx]
    dens += [(1.0, -(real[i] + real[i + 1]), real[i] * real[i + 1], max(abs(real[i]), abs(real[i + 1]))) for i in range(0, len(real), 2)]
    dens.sort(key=lambda d: d[3])
    g = abs(gain) ** (1.0 / order)
    sos = np.array([[g, 0.0, -g, d[0], d[1], d[2]] for d in dens], dtype=np.float64)
    if gain < 0:
        sos[0, :3] *= -1.0
    return sos


def bandpass_warmup(sos, floor=1e-7):
    """samples after which the cascade's impulse response stays below `floor`: a multiple of 64 and at least 512 (at most MAX_SAMPLES).
    A chunk of wm_clip_features's band-pass starts that many samples early from zero state."""
    n = 1 << 16
    w = np.exp(-2j * np.pi * np.arange(n // 2 + 1) / n)
    h = np.ones(n // 2 + 1, dtype=np.complex128)
    for b0, b1, b2, _, a1, a2 in np.asarray(sos, dtype=np.float64):
        h *= (b0 + b1 * w + b2 * w * w) / (1.0 + a1 * w + a2 * w * w)
    imp = np.fft.irfft(h, n)
    above = np.nonzero(np.abs(imp) >= floor)[0]
    last = int(above[-1]) + 1 if above.size else 0
    return int(min(MAX_SAMPLES, max(512, 64 * -(-last // 64))))


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    lin = f / (200.0 / 3.0)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) / (math.log(6.4) / 27.0), lin)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((math.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_frequencies(sr, n_mels):
    """the n_mels + 2 corner frequencies of the Slaney mel scale from 0 to sr / 2"""
    return _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(0.5 * float(sr)), int(n_mels) + 2))


def slaney_mel(sr, n_fft=N_FFT, n_mels=N_MELS):
    """librosa.filters.mel's default: (n_mels, n_fft / 2 + 1) float64 triangles on the Slaney mel scale (linear below 1 kHz, logarithmic
    above) from 0 to sr / 2, each scaled by 2 / (f[m + 2] - f[m]) (Slaney's area normalisation)"""
    f = mel_frequencies(sr, n_mels)
    bins = np.linspace(0.0, 0.5 * float(sr), n_fft // 2 + 1)
    fdiff = np.diff(f)
    ramps = f[:, None] - bins[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    return np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (f[2:] - f[:-2]))[:, None]


def dct_ortho(n_out, n_in):
    """the first n_out rows of the orthonormal DCT-II of length n_in, (n_out, n_in) float64: scipy.fft.dct(x, norm="ortho")[:n_out] = D x"""
    k, m = np.arange(int(n_out))[:, None], np.arange(int(n_in))[None, :]
    d = math.sqrt(2.0 / n_in) * np.cos(np.pi * k * (2 * m + 1) / (2.0 * n_in))
    d[0] *= math.sqrt(0.5)
    return d


def hann_periodic(n=N_FFT):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


_TABLES, _TABLES_DEV = {}, {}


def tables(sample_rate):
    """what wm_clip_features takes besides the clips, as a dict of CPU arrays (cached; do not write to them), evaluated in float64 and
    rounded once: sos (5, 6) float32, warm int, fb (1025, 128) float32 with klo / khi (128,) int32 (the first and last bin of each mel's
    triangle; an empty one has khi < klo), dct (13, 128) float32"""
    sr = int(sample_rate)
    if sr not in _TABLES:
        sos = butter_bandpass_sos(BAND[0], BAND[1], sr, 5)
        fb = slaney_mel(sr, N_FFT, N_MELS).astype(np.float32)
        klo, khi = np.zeros(N_MELS, dtype=np.int32), np.full(N_MELS, -1, dtype=np.int32)
        for m in range(N_MELS):
            nz = np.nonzero(fb[m])[0]
            if nz.size:
                klo[m], khi[m] = nz[0], nz[-1]
        _TABLES[sr] = dict(sos=sos.astype(np.float32), warm=bandpass_warmup(sos.astype(np.float32)), fb=np.ascontiguousarray(fb.T),
                           klo=klo, khi=khi, dct=dct_ortho(N_MFCC, N_MELS).astype(np.float32))
    return _TABLES[sr]


def tables_on(sample_rate, device):
    key = (int(sample_rate), str(device))
    if key not in _TABLES_DEV:
        t = tables(sample_rate)
        _TABLES_DEV[key] = {k: (v if k == "warm" else torch.from_numpy(v).to(device)) for k, v in t.items()}
    return _TABLES_DEV[key]


# ---------------------------------------------------------------------------------------------- the host restatement
def frame_count(n):
    return 1 + int(n) // HOP


def energy_frames(n, sample_rate):
    """(length, hop, count) of the 25-ms frames of energy_std"""
    length, hop = int(sample_rate * 0.025), int(sample_rate * 0.010)
    return length, hop, 1 + (int(n) - length) // hop


def check_shape(n, sample_rate):
    """n and the sample rate as wm_clip_features takes them, or ValueError"""
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, float)) or sample_rate != int(sample_rate):
        raise ValueError(f"sample_rate must be an integer number of Hz, got {sample_rate!r}")
    sr = int(sample_rate)
    if not 6000 < sr <= 2 ** 20:
        raise ValueError(f"sample_rate: expected more than 6000 Hz (the band-pass ends at 3000 Hz) and at most 2^20, got {sr}")
    if not MIN_SAMPLES <= n <= MAX_SAMPLES:
        raise ValueError(f"clips of {n} samples: expected {MIN_SAMPLES} to {MAX_SAMPLES}")
    if int(sr * 0.025) > n:
        raise ValueError(f"clips of {n} samples are shorter than one 25-ms frame at {sr} Hz")
    return sr


def _sosfilt_rows(sos, x):
    """the cascade in transposed direct form II from zero state, along the last axis of x (rows, n), all rows at once"""
    y = np.array(x, dtype=np.float64)
    for b0, b1, b2, _, a1, a2 in np.asarray(sos, dtype=np.float64):
        s1, s2 = np.zeros(y.shape[0]), np.zeros(y.shape[0])
        for i in range(y.shape[1]):
            v = y[:, i]
            o = b0 * v + s1
            s1 = b1 * v - a1 * o + s2
            s2 = b2 * v - a2 * o
            y[:, i] = o
    return y


def speech_score(feat):
    """classify_speech_noise's score of rows of FEATURES (any float array, the columns last): int32, a comparison with NaN false"""
    f = np.asarray(feat)
    col = {name: f[..., i] for i, name in enumerate(FEATURES)}
    with np.errstate(invalid="ignore"):
        return ((col["speech_band_energy"] > 0.001).astype(np.int32) + (col["zero_crossing_rate"] < 0.1) + (col["spectral_centroid"] < 3000)
                + (col["kurtosis"] > 5) + (col["energy_std"] > 0.01) + 2 * (col["speech_to_noise_ratio"] > 0.6)).astype(np.int32)


def clip_features_host(x, sample_rate=16000, frames=False):
    """wm_clip_features restated in float64 numpy: (feat (rows, 16) float64, counts (rows, 4) int32[, frames (rows, F, 4) float64]) of
    x (rows, n); the tables are the float32 ones the kernel takes"""
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError(f"x: expected (rows, n), got shape {x.shape}")
    rows, n = x.shape
    sr = check_shape(n, sample_rate)
    if rows > _HOST_CHUNK:                                                                   # the framed copies take rows x F x 2048 doubles
        parts = [clip_features_host(x[i:i + _HOST_CHUNK], sr, frames) for i in range(0, rows, _HOST_CHUNK)]
        return tuple(np.concatenate(p, axis=0) for p in zip(*parts))
    tab = tables(sr)
    y = x.astype(np.float64)
    finite = np.isfinite(y).all(axis=1)
    y = np.where(finite[:, None], y, 0.0)
    F = frame_count(n)
    feat = np.zeros((rows, FEAT_COLUMNS))
    col = {name: i for i, name in enumerate(FEATURES)}
    feat[:, col["duration"]] = n / sr
    energy = (y * y).mean(axis=1)
    feat[:, col["energy"]] = energy
    feat[:, col["rms"]] = np.sqrt(energy)
    z = _sosfilt_rows(butter_bandpass_sos(BAND[0], BAND[1], sr, 5), y)
    sbe = (z * z).mean(axis=1)
    feat[:, col["speech_band_energy"]] = sbe
    feat[:, col["speech_to_noise_ratio"]] = sbe / (energy + 1e-10)
    idx = HOP * np.arange(F)[:, None] + np.arange(N_FFT)[None, :]
    edge = np.pad(y, ((0, 0), (N_FFT // 2, N_FFT // 2)), mode="edge")[:, idx]               # (rows, F, 2048)
    edge = np.where(np.abs(edge) <= 1e-10, 0.0, edge)
    sign = np.signbit(edge)
    zc = (sign[:, :, 1:] != sign[:, :, :-1]).sum(axis=2)
    feat[:, col["zero_crossing_rate"]] = zc.sum(axis=1) / (F * N_FFT)
    padded = np.pad(y, ((0, 0), (N_FFT // 2, N_FFT // 2)))[:, idx]
    S = np.abs(np.fft.rfft(padded * hann_periodic(), axis=2))                                # (rows, F, 1025)
    tot = S.sum(axis=2)
    ok = tot >= _TINY
    safe = np.where(ok, tot, 1.0)
    freq = np.arange(N_FFT // 2 + 1) * (sr / N_FFT)
    cen = np.where(ok, (S * freq).sum(axis=2) / safe, 0.0)
    bw = np.where(ok, np.sqrt(((S / safe[:, :, None]) * (freq[None, None, :] - cen[:, :, None]) ** 2).sum(axis=2)), 0.0)
    ro = np.where(ok, (np.cumsum(S, axis=2) >= 0.85 * tot[:, :, None]).argmax(axis=2), 0)
    feat[:, col["spectral_centroid"]] = cen.mean(axis=1)
    feat[:, col["spectral_bandwidth"]] = bw.mean(axis=1)
    feat[:, col["rolloff"]] = (ro * (sr / N_FFT)).mean(axis=1)
    mel = (S * S) @ tab["fb"].astype(np.float64)                                             # (rows, F, 128)
    dB = 10.0 * np.log10(np.maximum(1e-10, mel))
    dB = np.maximum(dB, dB.max(axis=(1, 2), keepdims=True) - 80.0)
    mfcc = dB @ tab["dct"].astype(np.float64).T                                              # (rows, F, 13)
    feat[:, col["mfcc_mean"]] = mfcc.mean(axis=1).mean(axis=1)
    feat[:, col["mfcc_var"]] = (mfcc - mfcc[:, :1]).var(axis=1).mean(axis=1)                # a clip whose frames are all alike: exactly 0
    d = y - y.mean(axis=1, keepdims=True)
    m2, m4 = (d ** 2).mean(axis=1), (d ** 4).mean(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        feat[:, col["kurtosis"]] = m4 / (m2 * m2) - 3.0
    length, hop, count = energy_frames(n, sr)
    fr = y[:, hop * np.arange(count)[:, None] + np.arange(length)[None, :]]
    feat[:, col["energy_std"]] = (fr * fr).mean(axis=2).std(axis=1)
    feat[~finite, :len(FEATURES)] = np.nan
    score = np.where(finite, speech_score(feat[:, :len(FEATURES)]), 0).astype(np.int32)
    counts = np.stack([np.where(finite, zc.sum(axis=1), 0), score, (~finite).astype(np.int64),
                       np.where(finite, (score >= 4).astype(np.int64), ERROR)], axis=1).astype(np.int32)
    if not frames:
        return feat, counts
    per = np.stack([cen, bw, ro.astype(np.float64), zc.astype(np.float64)], axis=2)
    per[~finite] = np.nan
    return feat, counts, per


# ---------------------------------------------------------------------------------------------- the public calls
def clip_features(clips, sample_rate=16000):
    """The feature table of clips (B, 1, T), (C, N) or (N,) float32 at `sample_rate`: an OrderedDict of name -> (rows,) tensor on the clips'
    device for every name of FEATURES (float32), then "speech_score" (int32) and "finite" (bool).  CUDA tensors: one wm_clip_features
    launch; CPU tensors: clip_features_host rounded to float32."""
    from . import dsp
    feat, counts = dsp.clip_features(clips, sample_rate)
    out = OrderedDict((name, feat[:, i]) for i, name in enumerate(FEATURES))
    out["speech_score"] = counts[:, 1]
    out["finite"] = counts[:, 2] == 0
    return out


def classify_speech_noise(features):
    """noise.py's classifier on a table of clip_features (or any mapping of the six columns it reads to (rows,) tensors or arrays): int8
    labels, 1 speech (score >= 4), 0 noise, -1 error (a row whose "finite" is false, or, without that column, one holding a NaN)"""
    cols = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in features.items()}
    need = ("speech_band_energy", "zero_crossing_rate", "spectral_centroid", "kurtosis", "energy_std", "speech_to_noise_ratio")
    rows = np.stack([np.atleast_1d(cols[k]).astype(np.float64) for k in need], axis=1)
    table = np.zeros((rows.shape[0], len(FEATURES)))
    for i, k in enumerate(need):
        table[:, FEATURES.index(k)] = rows[:, i]
    score = speech_score(table)
    if "finite" in cols:
        bad = ~np.atleast_1d(cols["finite"]).astype(bool)
    else:
        bad = np.isnan(rows[:, [0, 1, 2, 4, 5]]).any(axis=1)                                 # the kurtosis of a constant row is NaN by definition
    labels = np.where(bad, ERROR, (score >= 4).astype(np.int64)).astype(np.int8)
    dev = next((v.device for v in features.values() if isinstance(v, torch.Tensor)), torch.device("cpu"))
    return torch.from_numpy(labels).to(dev)


def is_silent(waveform, threshold=SILENCE_RMS):
    """silent.py's test on one waveform (channels, samples): sqrt(mean(waveform^2)) < threshold, a 0-d bool tensor"""
    return torch.sqrt(torch.mean(waveform ** 2)) < threshold


def clip_classes(clips, sample_rate=16000, threshold=SILENCE_RMS):
    """the class of every clip as an index into CLASSES, (rows,) int64 on the clips' device, -1 for a clip with a non-finite sample:
    "silent" where rms < threshold, else noise.py's label.  One wm_clip_features launch on CUDA tensors."""
    from . import dsp
    feat, counts = dsp.clip_features(clips, sample_rate)
    label = counts[:, 3].to(torch.int64)
    cls = torch.where(label == SPEECH, 0, 1)
    cls = torch.where(feat[:, FEATURES.index("rms")] < threshold, 2, cls)
    return torch.where(label == ERROR, -1, cls)


def class_report(values, classes):
    """{class name: {"clips": count, key: mean over the class's clips (NaN for none)}} of per-clip tensors `values` (key -> (rows,)) and
    clip_classes' indices: what the evaluators add under "by_class" """
    classes = classes.cpu()
    out = OrderedDict()
    for i, name in enumerate(CLASSES):
        pick = classes == i
        row = OrderedDict(clips=int(pick.sum()))
        for k, v in values.items():
            v = v.detach().cpu().double()[pick]
            row[k] = float(v.mean()) if v.numel() else math.nan
        out[name] = row
    return out


def _channels(waveform):
    if not isinstance(waveform, torch.Tensor):
        raise TypeError(f"waveform: expected a tensor or a path, got {type(waveform).__name__}")
    if waveform.dtype != torch.float32:
        raise ValueError(f"waveform: expected dtype torch.float32, got {waveform.dtype}")
    if waveform.dim() == 1:
        return waveform[None]
    if waveform.dim() == 2 and waveform.shape[0] >= 1:
        return waveform
    raise ValueError(f"waveform: expected (samples,) or (channels, samples), got shape {tuple(waveform.shape)}")


def _table(clips, sample_rate, threshold=SILENCE_RMS):
    table = clip_features(clips, sample_rate)
    label = torch.where(table["finite"], (table["speech_score"] >= 4).to(torch.int8), torch.full_like(table["speech_score"], ERROR, dtype=torch.int8))
    table["classification"] = label
    table["silent"] = table["rms"] < threshold
    return table


def _empty_table(device):
    table = OrderedDict((name, torch.empty(0, device=device)) for name in FEATURES)
    table["speech_score"] = torch.empty(0, dtype=torch.int32, device=device)
    table["finite"] = torch.empty(0, dtype=torch.bool, device=device)
    table["classification"] = torch.empty(0, dtype=torch.int8, device=device)
    table["silent"] = torch.empty(0, dtype=torch.bool, device=device)
    return table


def segment_recording(waveform, orig_freq=None, device="cuda", segment_s=1.0):
    """1_sec_files.py without the features: clips (S, 1, round(segment_s * 16000)) float32 on `device`.  `waveform` is a float32 tensor
    (samples,) or (channels, samples) at `orig_freq`, or a path (read by inference.read_audio, which gives the rate).  Mixed down to mono,
    resampled to 16 kHz by the package's resampler (ops.resample on the device, its host restatement on the CPU), scaled by 0.99 / max|x|
    over the whole recording (wm_absmax_rows on the device; an all-zero recording stays zero, where the reference divides by zero), cut
    into whole segments; the remainder is dropped."""
    from . import dsp, inference
    from ._lib import lib
    from .inference import SAMPLE_RATE
    if isinstance(waveform, (str, os.PathLike)):
        waveform, rate = inference.read_audio(os.fspath(waveform))
        orig_freq = rate if orig_freq is None else orig_freq
    if orig_freq is None:
        raise ValueError("orig_freq: the rate of a tensor has to be given")
    rate = dsp._rate(orig_freq, "orig_freq")
    seg = int(round(float(segment_s) * SAMPLE_RATE))
    if seg < 1:
        raise ValueError(f"segment_s: expected a positive duration, got {segment_s!r}")
    dev = torch.device(device)
    x = _channels(waveform).to(dev).contiguous()
    if x.shape[1] < 1:
        return torch.empty(0, 1, seg, device=dev)
    if dev.type == "cuda":
        if rate != SAMPLE_RATE:
            mono = dsp.resample(x, rate, SAMPLE_RATE)                                        # the channel mean and the filter, one launch
        else:
            mono = x.mean(dim=0, keepdim=True) if x.shape[0] > 1 else x
        head = mono.shape[1] & ~3                                                            # wm_absmax_rows takes rows of whole quads
        peak = torch.zeros(1, device=dev)
        if head:
            lib.wm_absmax_rows(mono.data_ptr(), 1, head, peak.data_ptr(), torch.cuda.current_stream().cuda_stream)
        if head < mono.shape[1]:
            peak = torch.maximum(peak, mono[0, head:].abs().max())
    else:
        mono = x.mean(dim=0, keepdim=True) if x.shape[0] > 1 else x
        if rate != SAMPLE_RATE:
            mono = inference._resample_rows_host(mono, rate, SAMPLE_RATE)
        peak = mono.abs().max().reshape(1)
    scale = torch.where(peak > 0, 0.99 / peak, torch.ones_like(peak))
    mono = mono * scale
    S = mono.shape[1] // seg
    return mono[:, :S * seg].reshape(S, 1, seg).contiguous()


def prepare_recording(waveform, orig_freq=None, device="cuda", segment_s=1.0, threshold=SILENCE_RMS):
    """1_sec_files.py, silent.py and noise.py on one recording: (clips (S, 1, T), table) with segment_recording's clips and, per clip, the
    FEATURES columns, "speech_score", "finite", "classification" (int8: 1 speech, 0 noise, -1 error) and "silent" (rms < threshold) as
    (S,) tensors on `device`.  On the device: one launch for the table."""
    clips = segment_recording(waveform, orig_freq, device, segment_s)
    if clips.shape[0] == 0:
        return clips, _empty_table(clips.device)
    return clips, _table(clips, 16000, threshold)


CSV_COLUMNS = ("file", "segment") + FEATURES + ("classification", "silent")


def curate_files(paths, out_csv=None, device="cuda", segment_s=1.0, threshold=SILENCE_RMS, max_batch=4096):
    """prepare_recording over many files with the segments of several files batched into launches of up to max_batch rows.  Returns the
    rows as dicts with the keys CSV_COLUMNS ("file", "segment" counted from 1 as the reference names its files, the features,
    "classification" as speech / noise / error, "silent" as a bool); with out_csv they are appended to that file through the csv module
    (the header is written where the file is new or empty)."""
    max_batch = int(max_batch)
    if max_batch < 1:
        raise ValueError(f"max_batch: expected a positive int, got {max_batch!r}")
    rows, pending, held = [], [], 0

    def flush():
        nonlocal pending, held
        if not pending:
            return
        clips = torch.cat([c for _, c in pending], dim=0)
        for i0 in range(0, clips.shape[0], max_batch):
            table = _table(clips[i0:i0 + max_batch], 16000, threshold)
            cols = {k: v.cpu().tolist() for k, v in table.items()}
            names = [(p, s + 1) for p, c in pending for s in range(c.shape[0])][i0:i0 + max_batch]
            for j, (p, s) in enumerate(names):
                row = OrderedDict(file=p, segment=s)
                for name in FEATURES:
                    row[name] = cols[name][j]
                row["classification"] = LABEL_NAMES[int(cols["classification"][j])]
                row["silent"] = bool(cols["silent"][j])
                rows.append(row)
        pending, held = [], 0

    for p in paths:
        clips = segment_recording(os.fspath(p), None, device, segment_s)
        if clips.shape[0]:
            pending.append((os.fspath(p), clips))
            held += clips.shape[0]
        if held >= max_batch:
            flush()
    flush()
    if out_csv is not None:
        new = not os.path.exists(out_csv) or os.path.getsize(out_csv) == 0
        with open(out_csv, "a", newline="") as fh:
            w = csv.DictWriter(fh, fieldnames=list(CSV_COLUMNS))
            if new:
                w.writeheader()
            w.writerows(rows)
    return rows
