"""The splice attack without a GPU: the C boundary as declared, the host restatements of attacks.py against tests/splice_yardstick.py (bit
for bit), the label layout, the span conventions, argument validation, the `tamper=` plumbing of forward_losses and the arithmetic of
evaluate_localization's ratios."""
import math
import os

import numpy as np
import pytest
import torch

import splice_yardstick as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, DRAW, ROW0 = (7 << 32) + 1, 1, 5
CUT = dict(max_spans=2, p_span=0.5, len_lo=800, len_hi=6400, p_original=1 / 3, p_silence=1 / 3)
LENGTHS = [1, 2, 31, 32, 33, 257, 16000]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def signals(rows, n, seed=0):
    rng = np.random.default_rng(100 * seed + n)
    a, b = rng.standard_normal((rows, n)).astype(np.float32), rng.standard_normal((rows, n)).astype(np.float32)
    a[0, 0], b[0, 0] = -0.0, -0.0                                      # a copy keeps the sign of zero
    return a, b


def cut_for(n, **over):
    c = dict(CUT, **over)
    c["len_hi"] = min(c["len_hi"], n)
    c["len_lo"] = min(c["len_lo"], c["len_hi"])
    return c


# ------------------------------------------------------------------------------------------ 1. the boundary
def test_header_prototypes_and_build_list():
    from awm_amd._lib import parse_header
    protos = parse_header()
    want = {
        "wm_splice": "a b y lab rows n row0 seed draw max_spans p_span len_lo len_hi p_original p_silence stream",
        "wm_splice_bwd": "dy lab da rows n stream",
        "wm_bce_masked_fwd": "logits message lab partial count_out loc_out bce_out B R T NO stream",
        "wm_bce_masked_bwd": "logits message lab count g_loc g_bce dlogits B R T NO stream",
        "wm_loc_score": "logits lab thr_logit counts pred R T NO lab_rows stream",
    }
    for name, args in want.items():
        assert name in protos, f"{name} is not declared in include/wm_hip.h"
        assert [a for _, a in protos[name]] == args.split(), name
        assert protos[name][-1][0] == "wm_stream_t"
    types = dict((a, c) for c, a in protos["wm_splice"])
    assert types["lab"] == "int*" and types["p_span"] == "float" and types["len_lo"] == "long long" and types["max_spans"] == "int"
    assert dict((a, c) for c, a in protos["wm_bce_masked_fwd"])["count_out"] == "long long*"
    csrc = os.path.join(os.path.dirname(__import__("awm_amd").LIB_PATH), "csrc")
    build = open(os.path.join(csrc, "build.sh")).read()
    assert " splice" in build.split("for f in")[1].split(";")[0], "csrc/build.sh does not compile splice.hip"
    assert "atomic" not in open(os.path.join(csrc, "splice.hip")).read().lower()


# ------------------------------------------------------------------------------------------ 2. host restatement == yardstick
def fixture_input_condition():
    """the 8-row fixture has a row without an active span, a row whose two active spans overlap, and all three kinds: asserted, so that a
    change of the draw cannot silently hollow the tests on it out"""
    rows = [Y.spans(SEED, DRAW, ROW0 + r, 16000, **CUT) for r in range(8)]
    assert any(not any(s[4] for s in row) for row in rows), "no row without an active span"
    assert any(all(s[4] for s in row) and row[0][0] < row[1][0] + row[1][1] and row[1][0] < row[0][0] + row[0][1] for row in rows), \
        "no row with two overlapping spans"
    assert {s[2] for row in rows for s in row if s[4]} == {Y.ORIGINAL, Y.SILENCE, Y.MOVED}, "not all three kinds"


@pytest.mark.parametrize("n", LENGTHS)
def test_host_restatement_equals_the_yardstick(n):
    from awm_amd import attacks as A
    for over in ({}, dict(max_spans=8, p_span=1.0, len_lo=1, len_hi=max(1, n // 3)), dict(p_original=0.0, p_silence=0.0, p_span=1.0)):
        cut = cut_for(n, **over)
        got = A.row_splice_spans(SEED, DRAW, ROW0 + np.arange(8), n, **cut)
        want = [Y.spans(SEED, DRAW, ROW0 + r, n, **cut) for r in range(8)]
        assert [[tuple(s) for s in row] for row in got] == want, f"n={n} {over}"
        for start, L, kind, shift, _ in (s for row in want for s in row):
            assert cut["len_lo"] <= L <= cut["len_hi"] and 0 <= start and start + L <= n and kind in (0, 1, 2)
            assert 1 <= shift <= max(1, n - 1) and (n > 1 or kind != Y.MOVED)
        a, b = signals(8, n)
        y, lab = A.splice_rows_host(a, b, SEED, DRAW, ROW0, **cut)
        y0, lab0 = Y.splice(a, b, SEED, DRAW, ROW0, **cut)
        assert y.dtype == np.float32 and lab.dtype == bool
        assert np.array_equal(bits(y), bits(y0)) and np.array_equal(lab, lab0), f"n={n} {over}"


# ------------------------------------------------------------------------------------------ 3. the label layout
@pytest.mark.parametrize("n", LENGTHS)
def test_pack_unpack_round_trip(n):
    from awm_amd import attacks as A
    lab = np.random.default_rng(n).random((3, n)) < 0.5
    lab[0], lab[1] = True, False
    words = A.pack_labels(lab)
    assert words.dtype == np.uint32 and words.shape == (3, (n + 31) // 32)
    assert np.array_equal(words, Y.pack(lab))
    if n % 32:
        assert not (words[:, -1] >> np.uint32(n % 32)).any(), "bits at t >= n must be zero"
    assert words[0, 0] & 1 and np.array_equal(A.unpack_labels(words, n), lab)
    assert np.array_equal(A.unpack_labels(torch.from_numpy(words.view(np.int32)), n), lab), "an int32 tensor is the module's form"
    assert np.array_equal(Y.unpack(words, n), lab)
    with pytest.raises(ValueError):
        A.unpack_labels(words, n + 32)


# ------------------------------------------------------------------------------------------ 4. the module on CPU tensors, row0
def test_module_equals_host_and_a_batch_cut_in_two():
    from awm_amd import attacks as A
    fixture_input_condition()
    n = 16000
    a, b = signals(8, n)
    ta, tb = torch.from_numpy(a).view(8, 1, n), torch.from_numpy(b).view(8, 1, n)
    sp = A.Splice(seed=SEED).reset(DRAW)
    y, lab = sp(ta, tb, row0=ROW0)
    assert sp.draw == DRAW + 1 and y.shape == ta.shape and lab.dtype == torch.int32 and tuple(lab.shape) == (8, 500)
    y0, lab0 = Y.splice(a, b, SEED, DRAW, ROW0, **CUT)                  # the defaults at 16 kHz are CUT
    assert np.array_equal(bits(y.numpy().reshape(8, n)), bits(y0)) and np.array_equal(A.unpack_labels(lab, n), lab0)
    assert 0 < lab0.mean() < 1 and (y0 != a).any()
    y1, l1 = sp.reset(DRAW)(ta[:3], tb[:3], row0=ROW0)
    y2, l2 = sp.reset(DRAW)(ta[3:], tb[3:], row0=ROW0 + 3)
    assert torch.equal(torch.cat([y1, y2]), y) and torch.equal(torch.cat([l1, l2]), lab)
    y3, _ = sp(ta, tb, row0=ROW0)                                      # the next draw
    assert not torch.equal(y3, y)
    # (C, N) and (N,) as the other modules
    y4, l4 = sp.reset(DRAW)(ta[:, 0], tb[:, 0], row0=ROW0)
    assert torch.equal(y4, y[:, 0]) and torch.equal(l4, lab)
    y5, l5 = sp.reset(DRAW)(ta[0, 0], tb[0, 0], row0=ROW0)
    assert torch.equal(y5, y[0, 0]) and torch.equal(l5, lab[:1])
    # rows shorter than the spans: the lengths are cut to the row
    ys, ls = A.Splice(p_span=1.0, seed=1)(ta[:, :, :100], tb[:, :, :100])
    assert not A.unpack_labels(ls, 100).any()


# ------------------------------------------------------------------------------------------ 5. the span conventions
def test_span_conventions():
    from awm_amd import attacks as A
    n = 4000
    a, b = signals(8, n)
    # three spans, all active, long enough to overlap somewhere: per sample the LAST span that holds it decides
    cut = dict(max_spans=3, p_span=1.0, len_lo=1500, len_hi=2500, p_original=1 / 3, p_silence=1 / 3)
    spans = A.row_splice_spans(SEED, DRAW, ROW0 + np.arange(8), n, **cut)
    y, lab = A.splice_rows_host(a, b, SEED, DRAW, ROW0, **cut)
    overlaps = 0
    for r, row in enumerate(spans):
        assert all(s[4] for s in row)
        for t in range(0, n, 7):
            holds = [j for j, (start, L, _, _, _) in enumerate(row) if start <= t < start + L]
            overlaps += len(holds) > 1
            if not holds:
                assert lab[r, t] and bits(y[r, t]) == bits(a[r, t])
                continue
            start, L, kind, shift, _ = row[holds[-1]]
            want = b[r, t] if kind == 0 else (np.float32(0) if kind == 1 else b[r, (t + shift) % n])
            assert not lab[r, t] and bits(y[r, t]) == bits(want), (r, t, holds)
    assert overlaps > 100, "the fixture must have overlapping spans"
    # p_span = 0: nothing happens
    y, lab = A.splice_rows_host(a, b, SEED, DRAW, ROW0, **dict(cut, p_span=0.0))
    assert np.array_equal(bits(y), bits(a)) and lab.all()
    # len_lo = len_hi = n: every sample of every row is replaced
    y, lab = A.splice_rows_host(a, b, SEED, DRAW, ROW0, **dict(cut, len_lo=n, len_hi=n))
    assert not lab.any() and all(s[0] == 0 and s[1] == n for row in A.row_splice_spans(SEED, DRAW, np.arange(8), n, **dict(cut, len_lo=n, len_hi=n))
                                 for s in row)
    # silence is +0, original is b
    y, lab = A.splice_rows_host(a, b, SEED, DRAW, ROW0, **dict(cut, len_lo=n, len_hi=n, p_original=0.0, p_silence=1.0))
    assert not bits(y).any()
    y, lab = A.splice_rows_host(a, b, SEED, DRAW, ROW0, **dict(cut, len_lo=n, len_hi=n, p_original=1.0, p_silence=0.0))
    assert np.array_equal(bits(y), bits(b))
    # moved: a circular shift of b by 1 .. n - 1
    row = A.row_splice_spans(SEED, DRAW, [ROW0], n, max_spans=1, p_span=1.0, len_lo=n, len_hi=n, p_original=0.0, p_silence=0.0)[0][0]
    y, lab = A.splice_rows_host(a[:1], b[:1], SEED, DRAW, ROW0, max_spans=1, p_span=1.0, len_lo=n, len_hi=n, p_original=0.0, p_silence=0.0)
    assert row[2] == 2 and 1 <= row[3] < n and np.array_equal(bits(y[0]), bits(np.roll(b[0], -row[3])))


# ------------------------------------------------------------------------------------------ 6. validation
def test_argument_validation():
    from awm_amd import attacks as A
    for kw in (dict(max_spans=0), dict(max_spans=9), dict(max_spans=2.0), dict(max_spans=True), dict(p_span=-0.1), dict(p_span=1.5),
               dict(p_span="x"), dict(length_s=(0.4, 0.05)), dict(length_s=0.0), dict(length_s=(0.1, math.inf)), dict(kinds=(0.5, 0.6, 0.0)),
               dict(kinds=(1.0, 0.0)), dict(kinds=(-0.5, 1.0, 0.5)), dict(seed=1.5), dict(seed=True), dict(sample_rate=0),
               dict(sample_rate=math.nan)):
        with pytest.raises(ValueError):
            A.Splice(**kw)
    sp = A.Splice()
    for bad in (-1, 2 ** 32, 1.0, True):
        with pytest.raises(ValueError):
            sp.reset(bad)
    x = torch.zeros(2, 1, 64)
    with pytest.raises(TypeError):
        sp("x", x)
    with pytest.raises(ValueError):
        sp(x, torch.zeros(2, 1, 65))
    with pytest.raises(ValueError):
        sp(torch.zeros(2, 2, 2, 2), torch.zeros(2, 2, 2, 2))
    for row0 in (-1, 2 ** 32 - 1, 0.0, True):
        with pytest.raises(ValueError):
            sp(x, x, row0=row0)
    assert sp.draw == 0, "a refused call does not use up a draw"
    # every kinds triple that sums to 1 gives float32 probabilities the kernel accepts
    for kinds in ((0.6, 0.4, 0.0), (0.3, 0.7, 0.0), (1 / 3, 1 / 3, 1 / 3), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)):
        s = A.Splice(kinds=kinds)
        assert float(np.float32(s.p_original)) + float(np.float32(s.p_silence)) <= 1.0
        assert abs(s.p_silence - kinds[1]) < 1e-6
    ok = dict(max_spans=2, p_span=0.5, len_lo=1, len_hi=4, p_original=0.25, p_silence=0.25)
    for kw in (dict(len_lo=0), dict(len_lo=5), dict(len_hi=65), dict(max_spans=0), dict(max_spans=9), dict(p_span=1.1),
               dict(p_original=0.75, p_silence=0.5), dict(p_silence=-0.5)):
        with pytest.raises(ValueError):
            A.row_splice_spans(0, 0, [0], 64, **dict(ok, **kw))
    for n in (0, 2 ** 24 + 1):
        with pytest.raises(ValueError):
            A.row_splice_spans(0, 0, [0], n, **ok)
    with pytest.raises(ValueError):
        A.splice_rows_host(np.zeros((2, 8), np.float32), np.zeros((2, 9), np.float32), 0, 0, **ok)
    with pytest.raises(ValueError):
        A.pack_labels(np.zeros(8, bool))
    from awm_amd import ops
    assert ops.loc_threshold_logit(0.5) == 0.0 and ops.loc_threshold_logit(0.0) == -math.inf and ops.loc_threshold_logit(1.0) == math.inf
    assert ops.loc_threshold_logit(0.9) == math.log(0.9 / (1.0 - 0.9))
    for bad in (-0.1, 1.1, "x", True, math.nan):
        with pytest.raises(ValueError):
            ops.loc_threshold_logit(bad)


# ------------------------------------------------------------------------------------------ 7. tamper=None is the call as it was
def test_forward_losses_without_tamper_does_not_touch_the_new_code(monkeypatch):
    import awm_amd
    from awm_amd import dsp, losses as L, ops, step
    calls = []

    def forbidden(name):
        def f(*a, **k):
            raise AssertionError(f"{name} was reached with tamper=None")
        return f

    def fake_detect(detector, x, message, input_grad_rows=None):
        calls.append(("detect_with_losses", tuple(x.shape), input_grad_rows))
        return x.new_zeros(x.shape[0], x.shape[-1], 3), x.sum() * 0 + 1.0, x.sum() * 0 + 2.0

    def fake_masked(logits, message, labels):
        calls.append(("detection_losses_masked", tuple(logits.shape), tuple(labels.shape)))
        return logits.sum() * 0 + 3.0, logits.sum() * 0 + 4.0

    def detector(x, input_grad_rows=None):
        calls.append(("detector", tuple(x.shape), input_grad_rows))
        return x.new_zeros(x.shape[0], x.shape[-1], 3)

    monkeypatch.setattr(L, "postprocess", lambda d: d)
    monkeypatch.setattr(L, "l1_to_zero", lambda d: d.abs().mean())
    monkeypatch.setattr(L, "high_freq_penalty", lambda d: d.sum() * 0)
    monkeypatch.setattr(step, "_mel", lambda s, sw: (s - sw).abs().mean())
    monkeypatch.setattr(step, "_loud", lambda s, sw: (s - sw).abs().mean())
    monkeypatch.setattr(L, "detect_with_losses", fake_detect)
    for name in ("SpliceFn", "MaskedBCEFn", "loc_counts", "splice"):
        assert hasattr(ops, name), f"ops.{name} is missing"
    monkeypatch.setattr(ops.SpliceFn, "apply", forbidden("ops.SpliceFn"))
    monkeypatch.setattr(ops.MaskedBCEFn, "apply", forbidden("ops.MaskedBCEFn"))
    monkeypatch.setattr(ops, "loc_counts", forbidden("ops.loc_counts"))
    monkeypatch.setattr(dsp, "loc_counts", forbidden("dsp.loc_counts"))      # the module the package reads it from
    monkeypatch.setattr(L, "detection_losses_masked", forbidden("detection_losses_masked"))
    s, msg = torch.randn(2, 1, 64), torch.tensor([1, 2])
    gen = lambda s, m: 0.01 * s
    total, out = awm_amd.forward_losses(gen, detector, s, msg)
    total2, out2 = awm_amd.forward_losses(gen, detector, s, msg, tamper=None)
    assert calls == [("detect_with_losses", (4, 1, 64), 2)] * 2 and "labels" not in out and "s_t" not in out
    assert float(total) == float(total2) and float(out["loc"]) == 1.0 and float(out["bce"]) == 2.0
    # with a tamper: the plain detector call with input_grad_rows=B, then the masked losses; the fused route is not asked
    calls.clear()
    monkeypatch.setattr(L, "detect_with_losses", forbidden("detect_with_losses"))
    monkeypatch.setattr(L, "detection_losses_masked", fake_masked)
    seen = {}

    def tamper(s_w, clean):
        seen["args"] = (s_w, clean)
        return s_w * 0.5, torch.zeros(2, 2, dtype=torch.int32)

    total3, out3 = awm_amd.forward_losses(gen, detector, s, msg, tamper=tamper)
    assert calls == [("detector", (4, 1, 64), 2), ("detection_losses_masked", (4, 64, 3), (2, 2))]
    assert seen["args"][1] is s and torch.equal(seen["args"][0], out3["s_w"]) and torch.equal(out3["s_t"], out3["s_w"] * 0.5)
    assert float(out3["loc"]) == 3.0 and float(out3["bce"]) == 4.0 and tuple(out3["labels"].shape) == (2, 2)
    for k in ("l1", "mel", "loud", "hf"):
        assert float(out3[k]) == float(out[k]), f"{k} must see the unspliced signals"


# ------------------------------------------------------------------------------------------ 8. the ratios
def test_localization_metrics_arithmetic():
    from awm_amd import attacks as A
    m = A.localization_metrics((60, 10, 20, 10), (0, 5, 0, 95))
    assert m["iou"] == 60 / 90 and m["precision"] == 60 / 70 and m["recall"] == 60 / 80 and m["sample_accuracy"] == 70 / 100
    assert m["clean_false_positive_rate"] == 5 / 100 and m["watermarked_fraction"] == 80 / 100
    z = A.localization_metrics((0, 0, 0, 0), (0, 0, 0, 0))
    assert all(math.isnan(v) for v in z.values())
    z = A.localization_metrics((0, 0, 0, 7), (0, 0, 0, 7))              # everything cut out and nothing predicted
    assert math.isnan(z["iou"]) and math.isnan(z["precision"]) and math.isnan(z["recall"]) and z["sample_accuracy"] == 1.0
    assert z["clean_false_positive_rate"] == 0.0 and z["watermarked_fraction"] == 0.0
    import awm_amd
    for name in ("Splice", "evaluate_localization", "row_splice_spans", "splice_rows_host", "pack_labels", "unpack_labels",
                 "detection_losses_masked", "locate_watermark"):
        assert name in awm_amd.__all__ and hasattr(awm_amd, name), name
    with pytest.raises(TypeError):
        A.evaluate_localization(None, None, [], tamper=torch.nn.Identity(), device="cpu")


def test_merge_short_runs():
    from awm_amd.inference import merge_short_runs
    b = np.array([1, 1, 1, 0, 1, 1, 0, 0, 0, 0, 1], dtype=bool)
    assert merge_short_runs(b, 0) == [[0, 3, True], [3, 4, False], [4, 6, True], [6, 10, False], [10, 11, True]]
    assert merge_short_runs(b, 2) == [[0, 6, True], [6, 11, False]]
    assert merge_short_runs(b, 100) == [[0, 11, True]]                  # [0,6) T, [6,11) F: the shorter one gives way
    assert merge_short_runs(np.zeros(0, bool), 3) == [] and merge_short_runs(np.ones(5, bool), 9) == [[0, 5, True]]
