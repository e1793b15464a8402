"""Sample-rate conversion of the file ingest on the GPU: the HIP resampler (csrc/resample.hip) alone, as the (S,1,16000) segment
producer, and under the file-level wrappers' `orig_freq` keyword.

The yardstick is `yardstick()` of tests/resample_yardstick.py, float64 numpy with nothing from the package; the derived tolerance
(one stage, n = non-zero taps of the phase + C) stands in that module's docstring.  Model outputs downstream of it: FWD_TOL, as
everywhere in this suite."""
import math
import os

import numpy as np
import pytest
import torch

from gpu_support import awm, dev  # noqa: F401
from gpu_support import check, reference_models, same
from resample_yardstick import design, signal, yardstick
from yardstick_common import assert_within

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4

RATES_TO_16K = [48000, 44100, 32000, 22050, 11025, 8000]
PAIRS = [(r, 16000) for r in RATES_TO_16K] + [(16000, 48000)]


def pq(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


# ------------------------------------------------------------------------------------------ 1. the kernel against float64
@pytest.mark.parametrize("C", [1, 2, 6])
@pytest.mark.parametrize("orig,new", PAIRS)
def test_kernel_vs_float64(awm, dev, orig, new, C):
    from awm_amd import ops
    P, Q = pq(orig, new)
    tile = ops.resample_tile_periods(orig, new)
    assert tile > 0 and tile % 4 == 0
    for k, N in enumerate([1, 2, P - 1, P, 7 * P + 3, tile * P - 1, 3 * tile * P + 5, orig + 4321]):
        if N == 0:
            continue
        x = signal("noise" if k % 2 else "recording", C, N, orig, seed=100 * C + k)
        y = awm.resample(x.to(dev), orig, new)
        ref, bound = yardstick(x.double().mean(dim=0).numpy(), orig, new, C)
        assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (1, ref.shape[0])
        assert_within(y.cpu().numpy(), ref, bound, f"{orig}->{new} C={C} N={N}")


@pytest.mark.parametrize("orig,C,seconds", [(48000, 2, 200), (44100, 1, 190), (48000, 1, 61)])
def test_kernel_vs_float64_minutes(awm, dev, orig, C, seconds):
    """several minutes: every workgroup walks more than one tile, channel rows are megabytes apart"""
    N = orig * seconds + 3 * (C == 1)                                  # C = 1: an odd length, rows and tiles off the 16-byte grid
    x = signal("noise", C, N, orig, seed=7 + C)
    y = awm.resample(x.to(dev), orig, 16000)
    ref, bound = yardstick(x.double().mean(dim=0).numpy(), orig, 16000, C)
    assert tuple(y.shape) == (1, ref.shape[0])
    assert_within(y.cpu().numpy(), ref, bound, f"{orig}->16000 C={C} {seconds} s")


@pytest.mark.parametrize("C", [1, 2])
def test_table_that_does_not_fit_lds(awm, dev, C):
    """16001 -> 16000 has 16 000 phases: the one-thread-per-sample kernel, table through the cache"""
    from awm_amd import ops
    assert ops.resample_tile_periods(16001, 16000) == 0
    for N in (1, 16000, 40003):
        x = signal("recording", C, N, 16001, seed=40 + C)
        y = awm.resample(x.to(dev), 16001, 16000)
        ref, bound = yardstick(x.double().mean(dim=0).numpy(), 16001, 16000, C)
        assert_within(y.cpu().numpy(), ref, bound, f"16001->16000 C={C} N={N}")


def test_empty_and_equal_rates(awm, dev):
    from awm_amd import ops
    x = torch.randn(2, 100, device=dev)
    assert awm.resample(x, 16000, 16000) is x
    assert tuple(ops.resample(torch.zeros(2, 0, device=dev), 48000, 16000).shape) == (1, 0)
    assert tuple(ops.resample(torch.zeros(2, 0, device=dev), 48000, 16000, seg_len=16000).shape) == (0, 1, 16000)
    segs = ops.resample(x, 16000, 16000, seg_len=64)                                   # equal rates: mixdown + padding only
    want = torch.nn.functional.pad(x.double().mean(dim=0).float(), (0, 28)).view(2, 1, 64)
    assert torch.equal(segs, want)
    with pytest.raises(RuntimeError):
        ops.resample(torch.zeros(1, 10), 48000, 16000)                                  # a CPU tensor has no business in ops
    with pytest.raises(ValueError):
        ops.resample(x, 0, 16000)


# ------------------------------------------------------------------------------------------ 2. shift, bit for bit
@pytest.mark.parametrize("C", [1, 2, 6])
@pytest.mark.parametrize("orig,new", PAIRS + [(16001, 16000)])
def test_shift_is_bit_exact(awm, dev, orig, new, C):
    """the additions of a sample depend on its phase only: x delayed by d periods (P samples each) gives y delayed by d*Q samples, identically,
    wherever the sample then falls in a tile or a workgroup"""
    from awm_amd import ops
    P, Q, width, K, _ = design(orig, new)
    tile = ops.resample_tile_periods(orig, new)
    N = (3 * tile + 40) * P + 11 if tile else 6 * P + 11
    x = signal("noise", C, N, orig, seed=60 + C).to(dev)
    y = awm.resample(x, orig, new)[0]
    edge = (math.ceil(width / P) + 1) * Q
    a, b = edge, y.shape[0] - edge
    assert b - a > Q
    for d in [1, 7] + ([tile, tile + 3] if tile else []):
        xs = torch.cat([torch.zeros(C, d * P, device=dev), x], dim=1)
        ys = awm.resample(xs, orig, new)[0]
        assert torch.equal(ys[a + d * Q:b + d * Q], y[a:b]), f"{orig}->{new}: delay of {d} periods changes the samples"


# ------------------------------------------------------------------------------------------ 3. segments out of the kernel
@pytest.mark.parametrize("orig,C,N", [(48000, 2, 48000 * 3 + 1234), (44100, 1, 44100 * 2 + 99), (48000, 1, 48000), (8000, 6, 8000 * 2 + 1)])
def test_segments_and_zero_tail(awm, dev, orig, C, N):
    from awm_amd import ops
    from awm_amd.inference import _segments
    x = signal("recording", C, N, orig, seed=70 + C)
    L = ops.resample_length(N, orig, 16000)
    S = -(-L // 16000)
    buf = torch.full((S * 16000,), float("nan"), device=dev)
    segs = ops.resample(x.to(dev), orig, 16000, seg_len=16000, out=buf)
    assert tuple(segs.shape) == (S, 1, 16000) and segs.data_ptr() == buf.data_ptr()
    flat = segs.reshape(-1).cpu()
    assert not torch.isnan(flat).any(), "the kernel left samples unwritten"
    assert bool((flat[L:] == 0.0).all()) and flat[L:].numel() == S * 16000 - L
    want, rem = _segments(awm.resample(x, orig, 16000))
    assert rem == L % 16000 and want.shape == segs.shape
    ref, bound = yardstick(x.double().mean(dim=0).numpy(), orig, 16000, C)
    assert_within(flat[:L].numpy(), ref, bound, "segments vs float64")
    assert_within(flat[:L].numpy(), want.reshape(-1)[:L].double().numpy(), bound, "segments vs the CPU twin")
    assert torch.equal(want.reshape(-1)[L:], flat[L:])
    assert torch.equal(ops.resample(x.to(dev), orig, 16000).reshape(-1).cpu(), flat[:L])         # same samples with and without padding


# ------------------------------------------------------------------------------------------ 4. end to end
def shipped_detector(awm, dev):
    ck = np.load(os.path.join(os.path.dirname(__file__), "golden", "detector_best_unprefixed.npz"))
    sd = {"_orig_mod." + k: torch.from_numpy(ck[k]) for k in ck.files}      # as shipped: torch.compile prefix
    D = awm.Detector(16)
    res = awm.load_state_dict_strip_prefix(D, sd)
    assert not res.missing_keys and not res.unexpected_keys
    return D.to(dev).eval()


def compare_detections(got, want):
    assert set(got) == set(want)
    assert abs(got["mean_probability"] - want["mean_probability"]) <= FWD_TOL
    assert got["temporal_probs"].shape == want["temporal_probs"].shape
    check(torch.from_numpy(got["temporal_probs"]), torch.from_numpy(want["temporal_probs"]), FWD_TOL, "temporal probs")
    check(torch.tensor(got["message_confidence"]), torch.tensor(want["message_confidence"]), FWD_TOL, "message confidence")
    conf = torch.tensor(want["message_confidence"]).double()
    logit = torch.log(conf / (1 - conf))
    for bit, (g, w, lg) in enumerate(zip(got["predicted_message"], want["predicted_message"], logit.tolist())):
        if abs(lg) > FWD_TOL:
            assert g == w, f"bit {bit} (mean logit {lg:.3e})"


def test_detect_waveform_orig_freq(awm, dev):
    D = shipped_detector(awm, dev)
    x48 = signal("recording", 2, 48000 * 2 + 14000, 48000, seed=81)
    got = awm.detect_waveform(x48, D, device=dev, orig_freq=48000)
    want = awm.detect_waveform(awm.resample(x48.cpu(), 48000, 16000), D, device=dev)
    assert want["temporal_probs"].shape == (32000 + 4667,)
    compare_detections(got, want)
    compare_detections(awm.detect_waveform(x48.to(dev), D, device=dev, orig_freq=48000), want)       # already on the device
    compare_detections(awm.detect_watermark(x48, D, device=dev, orig_freq=48000), want)
    p_got = awm.detect_prob(x48, D, device=dev, orig_freq=48000)
    p_want = awm.detect_prob(awm.resample(x48.cpu(), 48000, 16000), D, device=dev)
    assert abs(p_got - p_want) <= FWD_TOL
    x441 = signal("recording", 1, 44100 + 500, 44100, seed=82)
    compare_detections(awm.detect_waveform(x441, D, device=dev, orig_freq=44100),
                       awm.detect_waveform(awm.resample(x441, 44100, 16000), D, device=dev))


def test_embed_waveform_orig_freq(awm, dev):
    G, D = reference_models(awm, dev)
    x48 = signal("recording", 2, 48000 * 2 + 15000, 48000, seed=83)
    msgs = torch.tensor([11, 22222, 65535])
    x16 = awm.resample(x48.cpu(), 48000, 16000)
    n = x16.shape[1]
    assert n == 32000 + 5000
    wm, delta, orig = awm.embed_waveform(x48, G, device=dev, messages=msgs, orig_freq=48000)
    wm_r, delta_r, orig_r = awm.embed_waveform(x16, G, device=dev, messages=msgs)
    for t in (wm, delta, orig):
        assert tuple(t.shape) == (1, n) and not t.is_cuda
    ref, bound = yardstick(x48.double().mean(dim=0).numpy(), 48000, 16000, 2)
    assert_within(orig.numpy(), ref, bound, "original waveform at 16 kHz")
    check(delta, delta_r, FWD_TOL, "delta")
    check(wm, wm_r, FWD_TOL, "watermarked")
    torch.manual_seed(5)
    res = awm.generate_watermarked_audio(x48, G, device=dev, orig_freq=48000)
    torch.manual_seed(5)
    res_r = awm.generate_watermarked_audio(x16, G, device=dev)
    check(res["watermarked_waveform"], res_r["watermarked_waveform"], FWD_TOL, "generate_watermarked_audio")
    ev = awm.evaluate_unseen_file(x48, G, D, device=dev, messages=msgs, orig_freq=48000)
    ev_r = awm.evaluate_unseen_file(x16, G, D, device=dev, messages=msgs)
    for a, b, name in zip(ev, ev_r, ("clean", "watermarked", "si-snr", "rms")):
        assert a == b or abs(a - b) <= FWD_TOL * max(abs(b), 1e-30), (name, a, b)         # si-snr is -inf on both sides (reference quirk)


def test_load_audio_on_the_device(awm, dev, tmp_path):
    import wave
    rng = np.random.default_rng(9)
    pcm = rng.integers(-20000, 20000, size=(48000 + 321, 2)).astype("<i2")
    p = str(tmp_path / "a.wav")
    with wave.open(p, "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(48000); w.writeframes(pcm.tobytes())
    got = awm.load_audio(p, device=dev)
    ref, bound = yardstick((pcm.astype(np.float64) / 32768.0).mean(axis=1), 48000, 16000, C=2)
    assert got.is_cuda and tuple(got.shape) == (1, ref.shape[0])
    assert_within(got.cpu().numpy(), ref, bound, "load_audio(device)")


# ------------------------------------------------------------------------------------------ 5. orig_freq=None changes nothing
def test_orig_freq_none_is_the_old_call(awm, dev):
    G, D = reference_models(awm, dev)
    w = signal("recording", 1, 2 * 16000 + 5000, 16000, seed=90)
    msgs = torch.tensor([11, 22222, 65535])
    for kw in ({"orig_freq": None}, {"orig_freq": 16000}):
        assert same(awm.embed_waveform(w, G, device=dev, messages=msgs), awm.embed_waveform(w, G, device=dev, messages=msgs, **kw))
        assert same(awm.detect_waveform(w, D, device=dev), awm.detect_waveform(w, D, device=dev, **kw))
        assert same(awm.detect_watermark(w, D, device=dev), awm.detect_watermark(w, D, device=dev, **kw))
        assert same(awm.detect_prob(w, D, device=dev), awm.detect_prob(w, D, device=dev, **kw))
        assert same(awm.evaluate_unseen_file(w, G, D, device=dev, messages=msgs), awm.evaluate_unseen_file(w, G, D, device=dev, messages=msgs, **kw))
        torch.manual_seed(3)
        a = awm.generate_watermarked_audio(w, G, device=dev)
        torch.manual_seed(3)
        assert same(a, awm.generate_watermarked_audio(w, G, device=dev, **kw))
    wm, delta, orig = awm.embed_waveform(w, G, device=dev, messages=msgs)
    assert orig is w


# ------------------------------------------------------------------------------------------ 6. two streams at once
def test_two_streams(awm, dev):
    from awm_amd import ops
    xa = signal("noise", 2, 48000 * 20 + 5, 48000, seed=95).to(dev)
    xb = signal("noise", 1, 44100 * 20 + 6, 44100, seed=96).to(dev)
    ya = ops.resample(xa, 48000, 16000, seg_len=16000)
    yb = ops.resample(xb, 44100, 16000, seg_len=16000)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            a = ops.resample(xa, 48000, 16000, seg_len=16000)
        with torch.cuda.stream(s2):
            b = ops.resample(xb, 44100, 16000, seg_len=16000)
        outs.append((a, b))
    torch.cuda.synchronize()
    for a, b in outs:
        assert torch.equal(a, ya) and torch.equal(b, yb)
