"""Clip curation without a GPU: the tables of awm_amd.curate against scipy and against hand values, the package's float64 host path
against the numpy yardstick of tests/curate_yardstick.py, the fixed points of the definition (zero row, NaN row, every scoring rule),
prepare_recording and curate_files on the CPU, the evaluators' per-class reports, and the plumbing that needs no launch."""
import csv
import inspect
import math
import os
import wave

import numpy as np
import pytest
import torch
from scipy import fft as sfft
from scipy import signal

import curate_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "audio-watermarking-deep-learning-watermarks-for-authenticating-speech_amd")
SHAPES = ((400, 16000), (2049, 16000), (16000, 16000), (32000, 16000), (8000, 8000))


@pytest.mark.parametrize("sr", [8000, 16000, 44100])
def test_butter_bandpass_sos_is_scipys_filter(sr):
    from awm_amd import curate
    sos = curate.butter_bandpass_sos(300, 3000, sr)
    wn = [300 / (sr / 2), 3000 / (sr / 2)]
    ref = signal.butter(5, wn, btype="band", output="sos")
    assert sos.shape == (5, 6) and np.all(sos[:, 3] == 1.0) and np.all(sos[:, 1] == 0.0) and np.all(sos[:, 0] == -sos[:, 2])
    _, h = signal.sosfreqz(sos, 4096)
    _, href = signal.sosfreqz(ref, 4096)
    err = np.abs(h - href).max() / np.abs(href).max()
    print(f"sr {sr}: frequency response {err:.2e} of the peak")
    assert err <= 1e-12
    b, a = signal.butter(5, wn, btype="band")
    pb, pa = np.ones(1), np.ones(1)
    for s in sos:
        pb, pa = np.convolve(pb, s[:3]), np.convolve(pa, s[3:])
    assert np.abs(pb - b).max() <= 1e-10 * np.abs(b).max() and np.abs(pa - a).max() <= 1e-10 * np.abs(a).max()
    radii = [np.abs(np.roots(s[3:])).max() for s in sos]
    assert radii == sorted(radii) and radii[-1] < 1.0


def test_butter_refusals_and_warmup():
    from awm_amd import curate
    for low, high, sr in ((0, 3000, 16000), (300, 8000, 16000), (3000, 300, 16000), (300, 3000, 6000)):
        with pytest.raises(ValueError):
            curate.butter_bandpass_sos(low, high, sr)
    sos = curate.butter_bandpass_sos(300, 3000, 16000)
    assert abs(np.abs(np.roots(sos[-1, 3:])).max() - 0.969) < 5e-4, "the largest pole radius at 16 kHz"
    imp = signal.sosfilt(sos, np.r_[1.0, np.zeros(4095)])
    last = int(np.nonzero(np.abs(imp) >= 1e-7)[0][-1]) + 1
    warm = curate.bandpass_warmup(sos)
    print(f"impulse response below 1e-7 after {last} samples; warm-up {warm}")
    assert 400 <= last <= 512 and warm == 512 == curate.tables(16000)["warm"]
    assert curate.bandpass_warmup(curate.butter_bandpass_sos(300, 3000, 44100)) > 512


def test_slaney_mel_hand_values():
    from awm_amd import curate
    for sr in (16000, 8000):
        f = curate.mel_frequencies(sr, 128)
        assert f.shape == (130,) and f[0] == 0.0 and abs(f[-1] - sr / 2) < 1e-9 and np.all(np.diff(f) > 0)
        step = f[1] - f[0]
        linear = f < 1000.0
        assert np.abs(np.diff(f[linear]) - step).max() < 1e-9, "equal steps below 1 kHz"
        ratio = f[~linear][1:] / f[~linear][:-1]
        assert np.abs(ratio - ratio[0]).max() < 1e-12, "equal ratios above"
        fb = curate.slaney_mel(sr, 2048, 128)
        assert fb.shape == (128, 1025) and fb.min() >= 0.0
        # float64 rounding through (bin - corner) / width: a corner up to 8 kHz over a width down to 18 Hz amplifies 2^-53 by under 500
        assert np.abs(fb - Y.mel_table(sr)).max() <= 1e-12 * fb.max()
        bins = np.arange(1025) * sr / 2048
        for m in (0, 1, 40, 90, 127):
            height = 2.0 / (f[m + 2] - f[m])                               # the peak of triangle m, at its centre f[m + 1]
            k = int(np.argmin(np.abs(bins - f[m + 1])))
            side = (bins[k] - f[m]) / (f[m + 1] - f[m]) if bins[k] <= f[m + 1] else (f[m + 2] - bins[k]) / (f[m + 2] - f[m + 1])
            assert abs(fb[m, k] - height * side) <= 1e-12 * height and fb[m].max() <= height
            assert not fb[m, bins <= f[m]].any() and not fb[m, bins >= f[m + 2]].any()
        wide = fb[100:] .sum(axis=1) * (sr / 2048)
        assert np.abs(wide - 1.0).max() < 0.02, "Slaney's normalisation: unit area, up to the bin grid"
    tab = curate.tables(16000)
    assert tab["fb"].shape == (1025, 128) and tab["fb"].dtype == np.float32 and tab["dct"].shape == (13, 128)
    for m in range(128):
        nz = np.nonzero(tab["fb"][:, m])[0]
        assert tab["klo"][m] == nz[0] and tab["khi"][m] == nz[-1] and 0 <= nz[0] <= nz[-1] <= 1024


def test_dct_ortho_is_scipys():
    from awm_amd import curate
    d = curate.dct_ortho(13, 128)
    ref = sfft.dct(np.eye(128), type=2, norm="ortho", axis=0)[:13]
    assert np.abs(d - ref).max() <= 1e-13 and np.abs(d - Y.dct_table()).max() <= 1e-13
    assert np.abs(d @ d.T - np.eye(13)).max() <= 1e-13
    assert np.abs(d[0] - 1.0 / math.sqrt(128.0)).max() <= 1e-15


@pytest.mark.parametrize("n,sr", SHAPES)
def test_host_path_against_the_yardstick(n, sr):
    from awm_amd import curate, ops
    x, r64, r32 = Y.case(24, n, sr)
    feat, counts, frames = curate.clip_features_host(x, sr, frames=True)
    err = Y.rel_error(feat[:, :13], r64.feat)
    print(f"n {n} sr {sr}: host against the yardstick {err.max():.2e}; float32 yardstick {Y.rel_error(r32.feat, r64.feat).max():.2e}; "
          f"smallest threshold margin {Y.threshold_margin(r64.feat).min():.2e}; speech rows {int((r64.score >= 4).sum())}")
    assert err.max() <= 1e-9
    assert np.array_equal(counts[:, 0], r64.zc) and np.array_equal(counts[:, 1], r64.score) and not counts[:, 2].any()
    assert np.array_equal(counts[:, 3], (r64.score >= 4).astype(np.int32)) and not feat[:, 13:].any()
    assert np.array_equal(frames[:, :, 2:], r64.frames[:, :, 2:])
    assert np.abs(frames[:, :, :2] - r64.frames[:, :, :2]).max() <= 1e-9 * np.abs(r64.frames[:, :, :2]).max()
    assert 0 < (r64.score >= 4).sum() < 24, "both labels occur"
    assert Y.threshold_margin(r64.feat).min() > 1e-3 and np.abs(r64.feat[:, 12] / 1e-4 - 1.0).min() > 0.19
    f32, c32 = ops.clip_features(torch.from_numpy(x), sr)
    assert f32.dtype == torch.float32 and c32.dtype == torch.int32 and tuple(f32.shape) == (24, 16) and tuple(c32.shape) == (24, 4)
    assert np.array_equal(f32.numpy(), feat.astype(np.float32)) and np.array_equal(c32.numpy(), counts)


def test_yardstick_twin_is_close():
    x, r64, r32 = Y.case(24, 16000, 16000)
    e = Y.rel_error(r32.feat, r64.feat)
    print("float32 against float64: " + ", ".join(f"{n} {v:.1e}" for n, v in zip(Y.FEATURES, e)))
    assert e.max() < 1e-4 and np.array_equal(r32.zc, r64.zc) and np.array_equal(r32.score, r64.score)
    assert (r32.frames[:, :, 2] == r64.frames[:, :, 2]).mean() >= 0.98 and np.abs(r32.frames[:, :, 2] - r64.frames[:, :, 2]).max() <= 1


def test_zero_row_and_nan_row():
    import awm_amd
    from awm_amd import curate
    x = Y.case(24, 16000)[0][:3].copy()
    x[1] = 0.0
    x[2, 123] = np.nan
    feat, counts, frames = curate.clip_features_host(x, 16000, frames=True)
    col = {name: i for i, name in enumerate(curate.FEATURES)}
    z = feat[1]
    for name in ("energy", "speech_band_energy", "zero_crossing_rate", "spectral_centroid", "spectral_bandwidth", "rolloff", "rms", "mfcc_var",
                 "energy_std", "speech_to_noise_ratio"):
        assert z[col[name]] == 0.0, name
    assert math.isnan(z[col["kurtosis"]]) and z[col["duration"]] == 1.0
    assert abs(z[col["mfcc_mean"]] + 100.0 * math.sqrt(128.0) / 13.0) <= 1e-4          # the float32 DCT row's rounding
    assert counts[1].tolist() == [0, 2, 0, 0], "one point each for the zero-crossing rate and the centroid, nothing else: noise"
    assert not frames[1].any()
    assert np.isnan(feat[2, :13]).all() and counts[2].tolist() == [0, 0, 1, -1] and np.isnan(frames[2]).all()
    table = awm_amd.clip_features(torch.from_numpy(x))
    assert list(table)[:13] == list(curate.FEATURES) and list(table)[13:] == ["speech_score", "finite"]
    assert table["finite"].tolist() == [True, True, False]
    assert awm_amd.classify_speech_noise(table).tolist() == [1, 0, -1]
    assert awm_amd.classify_speech_noise(table).dtype == torch.int8


def test_classifier_reproduces_every_rule():
    import awm_amd
    base = dict(speech_band_energy=0.0, zero_crossing_rate=0.5, spectral_centroid=5000.0, kurtosis=0.0, energy_std=0.0, speech_to_noise_ratio=0.0)
    steps = (("speech_band_energy", 0.0011, 0.001, 1), ("zero_crossing_rate", 0.0999, 0.1, 1), ("spectral_centroid", 2999.0, 3000.0, 1),
             ("kurtosis", 5.01, 5.0, 1), ("energy_std", 0.011, 0.01, 1), ("speech_to_noise_ratio", 0.61, 0.6, 2))
    from awm_amd import curate
    for name, inside, edge, points in steps:
        for value, want in ((inside, points), (edge, 0), (float("nan"), 0)):
            row = dict(base, **{name: value})
            table = np.zeros((1, len(curate.FEATURES)))
            for k, v in row.items():
                table[0, curate.FEATURES.index(k)] = v
            assert curate.speech_score(table).tolist() == [want], (name, value)
    rows = {k: [] for k in base}
    for on in ((), ("speech_to_noise_ratio",), ("speech_to_noise_ratio", "kurtosis"), ("speech_to_noise_ratio", "kurtosis", "energy_std"),
               ("speech_band_energy", "zero_crossing_rate", "spectral_centroid"), ("speech_band_energy", "zero_crossing_rate", "spectral_centroid", "kurtosis"),
               tuple(base)):
        for name, inside, _, _ in steps:
            rows[name].append(inside if name in on else base[name])
    labels = awm_amd.classify_speech_noise({k: torch.tensor(v, dtype=torch.float64) for k, v in rows.items()})
    assert labels.tolist() == [0, 0, 0, 1, 0, 1, 1], "scores 0 2 3 4 3 4 7: speech from 4 on"
    rows["speech_band_energy"][0] = float("nan")
    assert awm_amd.classify_speech_noise(rows).tolist()[0] == -1


def test_is_silent_is_the_references_expression():
    import awm_amd
    g = torch.Generator().manual_seed(1)
    for level in (2e-5, 9.9e-5, 1.01e-4, 0.1):
        w = level * torch.randn(2, 16000, generator=g)
        want = torch.sqrt(torch.mean(w ** 2)) < 1e-4
        got = awm_amd.is_silent(w)
        assert got.dtype == torch.bool and bool(got) == bool(want)
    assert bool(awm_amd.is_silent(torch.zeros(1, 100))) and not bool(awm_amd.is_silent(torch.ones(1, 100), threshold=0.5))


def _stereo(seconds=2.5, rate=22050):
    t = torch.arange(int(seconds * rate)) / rate
    g = torch.Generator().manual_seed(5)
    return torch.stack([0.3 * torch.sin(2 * math.pi * 180.0 * t) * (0.1 + torch.sin(2 * math.pi * 3.0 * t) ** 2),
                        0.05 * torch.randn(t.numel(), generator=g)])


def test_prepare_recording_on_the_cpu():
    import awm_amd
    from awm_amd import curate, inference
    wave_ = _stereo()
    clips, table = awm_amd.prepare_recording(wave_, 22050, device="cpu")
    assert tuple(clips.shape) == (2, 1, 16000) and clips.dtype == torch.float32
    whole = inference._resample_rows_host(wave_.mean(dim=0, keepdim=True), 22050, 16000)
    assert whole.shape[1] == 40000
    scaled = whole * (0.99 / whole.abs().max())
    assert abs(float(scaled.abs().max()) - 0.99) <= 1e-6, "peak 0.99 before cutting"
    assert torch.equal(clips.reshape(-1), scaled[0, :32000]), "whole segments, the remainder dropped"
    assert list(table) == list(curate.FEATURES) + ["speech_score", "finite", "classification", "silent"]
    assert all(tuple(v.shape) == (2,) for v in table.values()) and table["silent"].tolist() == [False, False]
    assert table["classification"].dtype == torch.int8
    zero, ztab = awm_amd.prepare_recording(torch.zeros(40000), 16000, device="cpu")
    assert tuple(zero.shape) == (2, 1, 16000) and not zero.any() and ztab["silent"].tolist() == [True, True], "an all-zero recording stays zero"
    short, stab = awm_amd.prepare_recording(torch.zeros(100), 16000, device="cpu")
    assert tuple(short.shape) == (0, 1, 16000) and all(v.numel() == 0 for v in stab.values())
    half, _ = awm_amd.prepare_recording(wave_, 22050, device="cpu", segment_s=0.5)
    assert tuple(half.shape) == (5, 1, 8000)
    with pytest.raises(ValueError):
        awm_amd.prepare_recording(wave_, None, device="cpu")
    with pytest.raises(ValueError):
        awm_amd.prepare_recording(wave_.double(), 22050, device="cpu")


def _write_wav(path, samples, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes((np.clip(samples, -1, 1) * 32767).astype("<i2").tobytes())


def test_curate_files_writes_one_line_per_segment(tmp_path):
    import awm_amd
    from awm_amd import curate
    rng = np.random.default_rng(0)
    a, b, c = tmp_path / "a.wav", tmp_path / "b.wav", tmp_path / "c.wav"
    _write_wav(a, Y.make_rows(1, 32000)[0].repeat(1), 16000)
    _write_wav(b, 0.1 * rng.standard_normal(int(3.2 * 8000)), 8000)
    _write_wav(c, np.zeros(100), 16000)                                    # shorter than a segment: no row
    out = tmp_path / "table.csv"
    rows = awm_amd.curate_files([a, b, c], out_csv=out, device="cpu", max_batch=2)
    assert [(os.path.basename(r["file"]), r["segment"]) for r in rows] == [("a.wav", 1), ("a.wav", 2), ("b.wav", 1), ("b.wav", 2), ("b.wav", 3)]
    assert rows[0]["classification"] == "speech" and not any(r["silent"] for r in rows)
    _, table_b = awm_amd.prepare_recording(b, device="cpu")
    assert [r["classification"] for r in rows[2:]] == [curate.LABEL_NAMES[v] for v in table_b["classification"].tolist()]
    assert [r["energy"] for r in rows[2:]] == table_b["energy"].tolist()
    with open(out, newline="") as fh:
        lines = list(csv.reader(fh))
    assert lines[0] == list(curate.CSV_COLUMNS) == ["file", "segment"] + list(curate.FEATURES) + ["classification", "silent"]
    assert len(lines) == 1 + 5 and lines[3][0].endswith("b.wav") and lines[3][1] == "1"
    assert float(lines[1][2]) == rows[0]["duration"] == 1.0
    same = awm_amd.curate_files([a, b, c], device="cpu", max_batch=4096)
    assert [r["energy"] for r in same] == [r["energy"] for r in rows], "the batching changes nothing"
    awm_amd.curate_files([a], out_csv=out, device="cpu")
    with open(out, newline="") as fh:
        assert len(list(csv.reader(fh))) == 1 + 5 + 2, "appended, one header"


def test_by_class_default_leaves_the_evaluators_as_they_were():
    import awm_amd
    ident = torch.nn.Identity()
    four = ["bit_accuracy", "clean_prob", "delta_rms", "watermarked_prob"]
    assert sorted(awm_amd.evaluate_batches(ident, ident, [], device="cpu")) == four
    assert sorted(awm_amd.evaluate_batches(ident, ident, [], device="cpu", by_class=False)) == four
    res = awm_amd.evaluate_batches(ident, ident, [], device="cpu", by_class=True)
    assert sorted(res) == four[:1] + ["by_class"] + four[1:]
    assert list(res["by_class"]) == ["speech", "noise", "silent"]
    assert all(sorted(v) == four[:2] + ["clips"] + four[2:] and v["clips"] == 0 for v in res["by_class"].values())
    plain = awm_amd.evaluate_robustness(ident, ident, [], {"a": ident}, device="cpu")
    assert list(plain) == ["none", "a"] and all(sorted(r) == four for r in plain.values())
    per = awm_amd.evaluate_robustness_by_class(ident, ident, [], {"a": ident}, device="cpu", quality=("stoi",))
    for row in per.values():
        assert sorted(row) == ["bit_accuracy", "by_class", "clean_prob", "delta_rms", "stoi", "stoi_attack_only", "stoi_rows", "watermarked_prob"]
        assert all(v["clips"] == 0 and v["stoi_rows"] == 0 for v in row["by_class"].values())
    assert list(inspect.signature(awm_amd.evaluate_robustness_by_class).parameters) == list(inspect.signature(awm_amd.evaluate_robustness).parameters)
    det = awm_amd.evaluate_detection(ident, ident, [], device="cpu")
    det_f = awm_amd.evaluate_detection(ident, ident, [], device="cpu", by_class=False)
    assert list(det) == list(det_f) == ["none"] and list(det["none"]) == list(det_f["none"]) and "by_class" not in det["none"]
    det_c = awm_amd.evaluate_detection(ident, ident, [], device="cpu", by_class=True)
    assert list(det_c["none"]) == list(det["none"]) + ["by_class"]
    assert all(list(v) == list(det["none"]) and v["clips"] == 0 for v in det_c["none"]["by_class"].values())
    for fn in (awm_amd.evaluate_batches, awm_amd.evaluate_detection):
        assert inspect.signature(fn).parameters["by_class"].default is False


def test_clip_classes_and_class_report_on_the_cpu():
    from awm_amd import curate
    x = Y.case(24, 16000)[0]
    clips = torch.from_numpy(x[[0, 6, 1, 2, 8, 3, 4, 5]].copy())[:, None]
    bad = clips.clone()
    bad[3, 0, 5] = float("inf")
    assert curate.clip_classes(clips).tolist() == [0, 0, 1, 2, 2, 1, 1, 1]
    assert curate.clip_classes(bad).tolist() == [0, 0, 1, -1, 2, 1, 1, 1]
    rep = curate.class_report({"v": torch.arange(8.0)}, curate.clip_classes(bad))
    assert list(rep) == ["speech", "noise", "silent"] and [rep[c]["clips"] for c in rep] == [2, 4, 1]
    assert rep["speech"]["v"] == 0.5 and rep["noise"]["v"] == (2 + 5 + 6 + 7) / 4 and rep["silent"]["v"] == 4.0


def test_refusals():
    from awm_amd import ops
    for shape, sr in (((2, 399), 16000), ((2, 32769), 16000), ((2, 16000), 6000), ((2, 16000), 2 ** 21), ((2, 400), 22050), ((0, 16000), 16000),
                      ((2, 2, 16000), 16000), ((2, 16000), 16000.5), ((2, 16000), True), ((2, 16000), "16000")):
        with pytest.raises(ValueError):
            ops.clip_features(torch.zeros(*shape), sr)
    with pytest.raises(ValueError):
        ops.clip_features(torch.zeros(2, 16000, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.clip_features(torch.zeros(()))
    with pytest.raises(TypeError):
        ops.clip_features(np.zeros((2, 16000), dtype=np.float32))
    for rows, n, sr in ((0, 16000, 16000), (1, 399, 16000), (1, 32769, 16000), (1, 16000, 6000), (1.5, 16000, 16000), (True, 16000, 16000)):
        with pytest.raises(ValueError):
            ops.clip_features_plan(rows, n, sr)


def test_entry_points_are_exported_and_built():
    import awm_amd
    from awm_amd import _lib
    protos = _lib.parse_header()
    assert [c for c, _ in protos["wm_clip_features_plan"]] == ["long long", "long long", "int", "int*", "int*", "int*", "wm_stream_t"]
    assert [a for _, a in protos["wm_clip_features"]] == ["x", "sos", "fb", "klo", "khi", "dct", "feat", "counts", "frames_out", "rows", "n",
                                                           "sample_rate", "warm", "stream"]
    assert [c for c, _ in protos["wm_clip_features"]][:9] == ["const float*", "const float*", "const float*", "const int*", "const int*",
                                                               "const float*", "float*", "int*", "float*"]
    build = open(os.path.join(PKG, "csrc", "build.sh")).read()
    assert " clip_features;" in build or " clip_features " in build
    text = open(os.path.join(PKG, "csrc", "clip_features.hip")).read()
    assert "wm_clip_features_plan" in text and "atomic" not in text.replace("no atomics", "") and '#include "fft_lds.hpp"' in text
    stft = open(os.path.join(PKG, "csrc", "stft_loss.hip")).read()
    assert '#include "fft_lds.hpp"' in stft and "void fft_dif" not in stft, "one copy of the transform"
    for name in ("curate", "clip_features", "classify_speech_noise", "is_silent", "prepare_recording", "curate_files", "butter_bandpass_sos",
                 "slaney_mel", "dct_ortho", "evaluate_robustness_by_class"):
        assert name in awm_amd.__all__ and hasattr(awm_amd, name), name
    assert len(awm_amd.curate.FEATURES) == 13 and awm_amd.curate.FEATURES == Y.FEATURES


def test_plan_matches_the_layout():
    """wm_clip_features_plan is a host-only query: it needs the library, not a GPU"""
    from awm_amd import ops
    for rows, n, sr in ((1, 400, 16000), (24, 2049, 16000), (512, 16000, 16000), (3, 16384, 16000), (3, 16385, 16000), (1, 32768, 16000),
                        (7, 8000, 8000), (2, 22050, 22050)):
        plan = ops.clip_features_plan(rows, n, sr)
        F = 1 + n // 512
        length, hop = int(sr * 0.025), int(sr * 0.010)
        assert plan.frames == F == Y.frame_count(n) and plan.energy_frames == 1 + (n - length) // hop
        stage = (n + 3) // 4 * 4 if n <= 16384 else 0
        assert plan.lds_bytes == 4 * (stage + (F * 129 + 3) // 4 * 4 + 2 * 2 * 2048 + 2048 + 448 + 2304 + 3 * 128) <= 160 * 1024
