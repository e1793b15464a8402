"""wm_clip_features on the GPU against the numpy yardstick of tests/curate_yardstick.py: the integers against the float64 run, every
float feature within 8 x the float32 run's own distance from the float64 run (floored at 1e-6; the factor is the margin for another
FFT factorisation and another order of the sums than pocketfft's and numpy's), the roll-off bins frame by frame, row independence as bit
patterns, the zero row and the NaN row, the refusals, curate.prepare_recording against the host path, and the per-class report."""
import math

import numpy as np
import pytest
import torch

import curate_yardstick as Y
from gpu_support import awm, bits, dev, reference_models  # noqa: F401

pytestmark = pytest.mark.gpu

BASE = 24
SHAPES = ((400, 16000), (2049, 16000), (16000, 16000), (32000, 16000), (8000, 8000))
FACTOR, FLOOR, NEAR = 8.0, 1e-6, 1e-4


def _rows(count, n, sr):
    """(x (count, n), float64 Result, float32 Result): the 24 base rows cycled, the yardstick computed once per (n, sr)"""
    x, r64, r32 = Y.case(BASE, n, sr)
    pick = np.arange(count) % BASE
    take = lambda r: Y.Result(r.feat[pick], r.zc[pick], r.score[pick], r.finite[pick], r.frames[pick])       # noqa: E731
    return x[pick], take(r64), take(r32)


def _check(awm, dev, count, n, sr):
    x, r64, r32 = _rows(count, n, sr)
    feat, counts, frames = awm.ops.clip_features(torch.from_numpy(x).to(dev), sr, frames=True)
    feat, counts, frames = feat.cpu().numpy(), counts.cpu().numpy(), frames.cpu().numpy()
    F = Y.frame_count(n)
    assert feat.shape == (count, 16) and counts.shape == (count, 4) and frames.shape == (count, F, 4)
    assert np.array_equal(counts[:, 0], r64.zc), "zero-crossing totals"
    assert np.array_equal(frames[:, :, 3], r64.frames[:, :, 3]), "zero-crossing counts per frame"
    assert not counts[:, 2].any() and not feat[:, 13:].any()
    far = Y.threshold_margin(r64.feat) >= NEAR
    print(f"n {n} sr {sr} rows {count}: {int((~far).sum())} rows within {NEAR} of a threshold")
    assert (~far).sum() <= 0.05 * count
    assert np.array_equal(counts[far, 1], r64.score[far]), "speech scores"
    assert np.array_equal(counts[far, 3], (r64.score[far] >= 4).astype(np.int32)), "labels"
    bar = FACTOR * np.maximum(Y.rel_error(r32.feat, r64.feat), FLOOR)
    err = Y.rel_error(feat[:, :13], r64.feat)
    for name, e, b in zip(Y.FEATURES, err, bar):
        print(f"  {name:22s} err {e:.2e}  bar {b:.2e}")
    ro, ro64 = frames[:, :, 2], r64.frames[:, :, 2]
    share = float((ro == ro64).mean())
    print(f"  roll-off bins equal in {share:.4f} of {ro.size} frames, largest distance {np.abs(ro - ro64).max():.0f}")
    assert share >= 0.98 and np.abs(ro - ro64).max() <= 1
    fe = np.abs(frames[:, :, :2] - r64.frames[:, :, :2]).max() / np.abs(r64.frames[:, :, :2]).max()
    print(f"  per-frame centroid and bandwidth: {fe:.2e} of the largest")
    assert fe <= 1e-4
    worst = [f"{name}: {e:.2e} > {b:.2e}" for name, e, b in zip(Y.FEATURES, err, bar) if not e <= b]
    assert not worst, "; ".join(worst)
    return feat, counts, frames


@pytest.mark.parametrize("n,sr", SHAPES)
def test_kernel_against_the_yardstick(awm, dev, n, sr):
    _check(awm, dev, BASE, n, sr)


@pytest.mark.parametrize("n", [400, 2049, 16000, 32000])
def test_one_row_and_257_rows(awm, dev, n):
    """more rows than the grid has workgroups per pass of its loop, and a single one: the same bars, and the same bits for the same row"""
    one = _check(awm, dev, 1, n, 16000)
    many = _check(awm, dev, 257, n, 16000)
    base = awm.ops.clip_features(torch.from_numpy(_rows(BASE, n, 16000)[0]).to(dev), 16000, frames=True)
    for a, b, c in zip(one, many, base):
        c = c.cpu().numpy()
        assert a[0].tobytes() == c[0].tobytes() == b[0].tobytes(), "row 0 alone, of 24, of 257"
        assert b[256].tobytes() == c[256 % BASE].tobytes(), "row 256 of 257 is row 16 of 24"


def test_row_bits_alone_first_and_last(awm, dev):
    x = torch.from_numpy(Y.case(BASE, 16000)[0]).to(dev)
    row = x[5:6].clone()
    alone = awm.ops.clip_features(row, frames=True)
    first = awm.ops.clip_features(torch.cat([row, x[1:]]), frames=True)
    last = awm.ops.clip_features(torch.cat([x.repeat(11, 1)[:256], row]), frames=True)
    again = awm.ops.clip_features(row, frames=True)
    for a, f, l, g in zip(alone, first, last, again):
        assert torch.equal(bits(a[0].float()), bits(f[0].float())) and torch.equal(bits(a[0].float()), bits(l[256].float()))
        assert torch.equal(bits(a[0].float()), bits(g[0].float()))


def test_zero_row_and_nan_row(awm, dev):
    x = torch.from_numpy(Y.case(BASE, 16000)[0][:4].copy())
    x[1] = 0.0
    x[2, 777] = float("nan")
    feat, counts, frames = awm.ops.clip_features(x.to(dev), frames=True)
    clean, _ = awm.ops.clip_features(x[[0, 3]].to(dev))
    assert torch.equal(bits(feat[[0, 3]]), bits(clean)), "a bad neighbour changes no bit"
    col = {name: i for i, name in enumerate(Y.FEATURES)}
    z = feat[1].cpu()
    for name in ("energy", "speech_band_energy", "zero_crossing_rate", "spectral_centroid", "spectral_bandwidth", "rolloff", "rms", "mfcc_var",
                 "energy_std", "speech_to_noise_ratio"):
        assert float(z[col[name]]) == 0.0, name
    assert math.isnan(float(z[col["kurtosis"]])) and float(z[col["duration"]]) == 1.0
    assert abs(float(z[col["mfcc_mean"]]) + 100.0 * math.sqrt(128.0) / 13.0) <= 1e-4
    assert counts[1].tolist() == [0, 2, 0, 0], "one point each for the zero-crossing rate and the centroid, nothing else: noise"
    assert not frames[1].any()
    assert bool(torch.isnan(feat[2, :13]).all()) and counts[2].tolist() == [0, 0, 1, -1] and bool(torch.isnan(frames[2]).all())
    table = awm.clip_features(x.to(dev))
    assert awm.classify_speech_noise(table).tolist() == [1, 0, -1, counts[3, 3].item()]


def test_refusals_before_any_launch(awm, dev, monkeypatch):
    calls = []
    monkeypatch.setattr(awm.lib, "wm_clip_features", lambda *a: calls.append(a))
    for shape, sr in (((2, 399), 16000), ((2, 32769), 16000), ((2, 16000), 6000), ((2, 400), 22050), ((0, 16000), 16000), ((2, 2, 16000), 16000),
                      ((2, 16000), 16000.5)):
        with pytest.raises(ValueError):
            awm.ops.clip_features(torch.zeros(*shape, device=dev), sr)
    with pytest.raises(ValueError):
        awm.ops.clip_features(torch.zeros(2, 16000, device=dev, dtype=torch.float64))
    assert not calls
    monkeypatch.undo()
    import ctypes
    dll = awm.lib.load()
    x = torch.zeros(2, 16000, device=dev)
    tab = awm.curate.tables_on(16000, dev)
    feat, counts = torch.zeros(2, 16, device=dev), torch.zeros(2, 4, dtype=torch.int32, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())                                            # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = [P(x), P(tab["sos"]), P(tab["fb"]), P(tab["klo"]), P(tab["khi"]), P(tab["dct"]), P(feat), P(counts), None, 2, 16000, 16000, 512, st]
    for i, v in ((0, None), (6, None), (7, None), (6, P(x)), (9, 0), (10, 399), (10, 32769), (11, 6000), (12, -1), (12, 32769),
                 (0, ctypes.c_void_p(x.data_ptr() + 2))):
        args = list(good)
        args[i] = v
        assert dll.wm_clip_features(*args) == 1, f"argument {i} = {v}"
    torch.cuda.synchronize()
    assert not feat.any() and not counts.any(), "a refused call launches nothing"


def test_prepare_recording_device_equals_host(awm, dev):
    g = torch.Generator().manual_seed(5)
    t = torch.arange(int(2.5 * 22050)) / 22050.0
    wave = torch.stack([0.3 * torch.sin(2 * math.pi * 180.0 * t) * (0.1 + torch.sin(2 * math.pi * 3.0 * t) ** 2),
                        0.05 * torch.randn(t.numel(), generator=g)])
    clips_d, table_d = awm.prepare_recording(wave, 22050, device=dev)
    clips_h, table_h = awm.prepare_recording(wave, 22050, device="cpu")
    assert clips_d.shape == clips_h.shape == (2, 1, 16000) and clips_d.is_cuda
    assert float((clips_d.cpu() - clips_h).abs().max()) <= 1e-6
    assert table_d["classification"].tolist() == table_h["classification"].tolist()
    assert table_d["silent"].tolist() == table_h["silent"].tolist() == [False, False]
    for name in Y.FEATURES:
        a, b = table_d[name].cpu().double(), table_h[name].double()
        assert float(((a - b).abs() / (b.abs() + 3.0 * (name == "kurtosis") + 1e-30)).max()) <= 1e-4, name


def test_evaluate_robustness_by_class(awm, dev):
    G, D = reference_models(awm, dev)
    x = Y.case(BASE, 16000)[0]
    clips = torch.from_numpy(x[[0, 6, 1, 2, 8, 3, 4, 5]].copy())[:, None]                  # two voiced, one loud noise, two quiet, hum, clicks, brown
    msg = [torch.arange(8) * 7919 % 65536]
    atk = {"lowpass": awm.Lowpass(4000)}
    plain = awm.evaluate_robustness(G, D, [clips], atk, device=dev, messages=msg)
    res = awm.attacks.evaluate_robustness_by_class(G, D, [clips], atk, device=dev, messages=msg)
    classes = awm.curate.clip_classes(clips.to(dev)).cpu().tolist()
    assert classes == [0, 0, 1, 2, 2, 1, 1, 1]
    for name, row in res.items():
        per = row.pop("by_class")
        assert row == plain[name], "the pooled numbers are the call's without by_class"
        assert list(per) == ["speech", "noise", "silent"] and [per[c]["clips"] for c in per] == [2, 4, 2]
        assert sum(per[c]["clips"] for c in per) == 8
        for k, v in row.items():
            mix = sum(per[c]["clips"] * per[c][k] for c in per) / 8
            assert abs(mix - v) <= 1e-6 * max(1.0, abs(v)), f"{name} {k}: the classes' means weigh to the pooled mean"
    one = awm.evaluate_batches(G, D, [clips], device=dev, messages=msg, by_class=True)
    assert [one["by_class"][c]["clips"] for c in one["by_class"]] == [2, 4, 2]
    det = awm.evaluate_detection(G, D, [clips], device=dev, messages=msg, by_class=True)
    assert [det["none"]["by_class"][c]["clips"] for c in ("speech", "noise", "silent")] == [2, 4, 2]
    assert det["none"]["clips"] == 8
