"""STOI without a GPU: the float64 yardstick of tests/stoi_yardstick.py against the definition's fixed points, the package's host path
(ops.stoi on CPU tensors, quality.stoi_rows_host) against the yardstick, and the plumbing that needs no launch."""
import inspect
import os

import numpy as np
import pytest
import torch

import stoi_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_band_edges_follow_from_the_rule():
    assert Y.band_edges() == Y.EDGES
    from awm_amd import quality
    assert quality.STOI_BANDS == Y.EDGES
    assert Y.EDGES[0][0] == 7 and Y.EDGES[-1][1] == 219 and all(a[1] == b[0] for a, b in zip(Y.EDGES, Y.EDGES[1:]))


def test_window_and_frame_count():
    t = np.arange(256)
    assert np.abs(Y.window() - 0.5 * (1 - np.cos(2 * np.pi * (t + 1) / 257))).max() < 1e-15
    assert [Y.frame_count(n) for n in (1, 255, 256, 257, 384, 385, 3969, 4096, 4097)] == [0, 0, 0, 1, 1, 2, 30, 30, 31]


def test_yardstick_sentinels_and_fixed_points():
    for n, kind in Y.SENTINEL_CASES:
        x, y = Y.case(n, kind)
        for a, b in zip(x, y):
            s = Y.stoi(a, b)
            assert s.d == Y.SENTINEL and s.K <= 30 and s.K <= Y.frame_count(n)
    for n in (3968, 3969, 4097):                       # speech-like rows this short have pauses: fewer than 31 kept frames
        s = Y.stoi(Y.speech_like(n, 5), Y.speech_like(n, 5))
        assert s.d == Y.SENTINEL and 0 < s.K < 31
    x, _ = Y.case(4096, "noise")
    assert Y.stoi(x[0], x[0]).K == 30, "stationary noise keeps every frame"
    x, y = Y.case(4097, "noise")
    s = Y.stoi(x[0], y[0])
    assert s.K == 31 and 0.9 < s.d < 1.0, "31 kept frames: exactly one segment"
    x, y = Y.case(10000, "speech")
    assert abs(1.0 - Y.stoi(x[0], x[0]).d) < 1e-14, "a signal against itself"
    z = np.zeros(10000, dtype=np.float32)
    assert Y.stoi(z, x[0]).d == 0.0 and Y.stoi(x[0], z).d == 0.0 and Y.stoi(z, z).d == 0.0, "all-zero rows score exactly 0"
    assert Y.stoi(z, x[0]).K == Y.frame_count(10000), "an all-zero row keeps every frame"
    bad = x[0].copy()
    bad[5000] = np.nan
    assert np.isnan(Y.stoi(bad, y[0]).d) and np.isnan(Y.stoi(x[0], bad).d) and Y.stoi(bad, y[0]).K == 0
    d = [Y.stoi(a, b).d for a, b in zip(x, y)]
    assert d[0] > d[1] > d[2] > 0.3, "more noise, lower score"


def test_twin_is_close_and_masks_are_far_from_flipping():
    worst = 0.0
    for n, kind in Y.FLOAT_CASES[:4]:
        r64, r32 = Y.case_ref(n, kind)
        for a, b in zip(r64, r32):
            assert a.K == b.K and a.margin_db > 0.01
            worst = max(worst, abs(a.d - b.d))
    print(f"largest |d_twin - d64| {worst:.3e}")
    assert worst < 1e-6


def test_host_path_equals_the_yardstick():
    from awm_amd import ops, quality
    import awm_amd
    for n, kind in ((257, "speech"), (3969, "speech"), (4096, "noise"), (4097, "noise"), (6250, "speech"), (20000, "speech")):
        x, y = Y.case(n, kind)
        d, kept = ops.stoi(torch.from_numpy(x.copy()), torch.from_numpy(y.copy()), 10000)
        assert d.dtype == torch.float32 and kept.dtype == torch.int32 and tuple(d.shape) == (3,) and tuple(kept.shape) == (3,)
        for r in range(3):
            ref = Y.stoi(x[r], y[r])
            d64, K = quality.stoi_row_host(x[r], y[r])
            assert abs(d64 - ref.d) <= 1e-12 and K == ref.K == int(kept[r])
            assert float(d[r]) == float(np.float32(d64))
    x, y = Y.case(6250, "speech")
    xt, yt = torch.from_numpy(x.copy()), torch.from_numpy(y.copy())
    want = ops.stoi(xt, yt, 10000)[0]
    assert torch.equal(awm_amd.stoi(xt, yt, 10000), want)
    assert torch.equal(awm_amd.stoi(xt[:, None], yt[:, None], 10000), want)
    one = awm_amd.stoi(xt[1], yt[1], 10000)
    assert one.dim() == 0 and float(one) == float(want[1])
    bad = xt.clone()
    bad[1, 77] = float("inf")
    got = ops.stoi(bad, yt, 10000)
    assert bool(torch.isnan(got[0][1])) and int(got[1][1]) == 0 and got[0][0] == want[0] and got[0][2] == want[2]


def test_host_path_at_16k_is_the_host_resampler_then_10k():
    from awm_amd import inference, ops
    rng = np.random.default_rng(3)
    x = torch.from_numpy(Y.speech_like(12000, 9))
    y = x + 0.05 * torch.from_numpy(rng.standard_normal(12000).astype(np.float32))
    both = inference._resample_rows_host(torch.stack([x, y]), 16000, 10000)
    assert both.shape[1] == 7500
    want = ops.stoi(both[:1], both[1:], 10000)
    got = ops.stoi(x, y)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and 0.5 < float(got[0][0]) < 1.0


def test_refusals():
    from awm_amd import ops
    x = torch.zeros(2, 5000)
    for bx, by, rate in ((x, torch.zeros(2, 4999), 10000), (x, torch.zeros(3, 5000), 10000), (x.double(), x.double(), 10000),
                         (torch.zeros(2, 2, 5000), torch.zeros(2, 2, 5000), 10000), (torch.zeros(2, 0), torch.zeros(2, 0), 10000),
                         (torch.zeros(0, 50), torch.zeros(0, 50), 10000), (torch.zeros(()), torch.zeros(()), 10000),
                         (x, x, 0), (x, x, -16000), (x, x, 16000.5), (x, x, True), (x, x, "16000")):
        with pytest.raises(ValueError):
            ops.stoi(bx, by, rate)
    with pytest.raises(TypeError):
        ops.stoi(x.numpy(), x, 10000)
    for rows, n in ((0, 100), (1, 0), (-1, 5), (1, 2 ** 34 + 1), (2 ** 20, 2 ** 30), (1.5, 10), (True, 10)):
        with pytest.raises(ValueError):
            ops.stoi_plan(rows, n)


def test_entry_points_are_exported_and_built():
    from awm_amd import _lib
    protos = _lib.parse_header()
    assert [c for c, _ in protos["wm_stoi_plan"]] == ["long long", "long long", "long long*", "wm_stream_t"]
    assert [a for _, a in protos["wm_stoi"]] == ["x", "y", "d", "kept", "scratch", "rows", "n", "stream"]
    build = open(os.path.join(ROOT, "audio-watermarking-deep-learning-watermarks-for-authenticating-speech_amd", "csrc", "build.sh")).read()
    assert " stoi;" in build or " stoi " in build
    src = os.path.join(ROOT, "audio-watermarking-deep-learning-watermarks-for-authenticating-speech_amd", "csrc", "stoi.hip")
    text = open(src).read()
    assert "wm_stoi_plan" in text and "atomic" not in text.replace("No atomics", "")
    import awm_amd
    assert "stoi" in awm_amd.__all__ and callable(awm_amd.stoi)


def test_plan_matches_the_layout():
    """wm_stoi_plan is a host-only query: it needs the library, not a GPU"""
    from awm_amd import ops
    for rows, n in ((1, 1), (3, 256), (3, 257), (3, 4097), (512, 10000), (1, 6000000)):
        F = max(Y.frame_count(n), 1)
        C = max(-(-(Y.frame_count(n) - 30) // 256), 1) if Y.frame_count(n) > 30 else 1
        assert ops.stoi_plan(rows, n) == 4 * rows * (32 * F + C + 1)


def test_evaluate_robustness_signature_and_metric_names():
    import awm_amd
    from awm_amd import quality
    sig = inspect.signature(awm_amd.evaluate_robustness)
    assert list(sig.parameters) == ["generator", "detector", "batches", "attacks", "device", "message_bits", "messages", "quality"]
    assert sig.parameters["quality"].default == ()
    assert quality.check_metrics(()) == () and quality.check_metrics("stoi") == ("stoi",) and quality.check_metrics(["stoi"]) == ("stoi",)
    for bad in (("pesq",), ("stoi", "estoi"), "STOI"):
        with pytest.raises(ValueError, match="unknown metric"):
            quality.check_metrics(bad)
        with pytest.raises(ValueError, match="unknown metric"):
            awm_amd.evaluate_robustness(torch.nn.Identity(), torch.nn.Identity(), [], {}, device="cpu", quality=bad)
    for fn in (awm_amd.generate_watermarked_audio, awm_amd.evaluate_unseen_file):
        assert inspect.signature(fn).parameters["stoi"].default is False


def test_evaluate_robustness_default_keys_unchanged():
    """no batches: the rows and their key sets as they were, NaN everywhere; with the metric, three more keys"""
    import awm_amd
    ident = torch.nn.Identity()
    res = awm_amd.evaluate_robustness(ident, ident, [], {"a": ident}, device="cpu")
    assert list(res) == ["none", "a"]
    for row in res.values():
        assert sorted(row) == ["bit_accuracy", "clean_prob", "delta_rms", "watermarked_prob"]
    res = awm_amd.evaluate_robustness(ident, ident, [], {"a": ident}, device="cpu", quality=("stoi",))
    for row in res.values():
        assert sorted(row) == ["bit_accuracy", "clean_prob", "delta_rms", "stoi", "stoi_attack_only", "stoi_rows", "watermarked_prob"]
        assert row["stoi_rows"] == 0 and np.isnan(row["stoi"]) and np.isnan(row["stoi_attack_only"])


def test_parity_with_pystoi_at_10k():
    """pystoi's own rate, where no resampling happens and the definition is pystoi's.  The bar is float64 rounding of about 1e3 operations
    through the worst mean removal the yardstick sees on these rows: 1e3 * kappa * 2^-52."""
    pystoi = pytest.importorskip("pystoi")
    from awm_amd import quality
    for n, kind in Y.FLOAT_CASES[:4]:
        x, y = Y.case(n, kind)
        for r in range(3):
            ref = Y.stoi(x[r], y[r])
            want = pystoi.stoi(x[r].astype(np.float64), y[r].astype(np.float64), 10000, extended=False)
            got, _ = quality.stoi_row_host(x[r], y[r])
            bar = 1e3 * ref.kappa * 2.0 ** -52
            print(f"n {n} row {r}: |host - pystoi| {abs(got - want):.3e}, bar {bar:.3e}")
            assert abs(got - want) <= bar
