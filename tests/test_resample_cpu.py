"""Sample-rate conversion of the file ingest, on the host: `resample` / `Resample` / `load_audio` without torchaudio.

The yardstick is `yardstick()` of tests/resample_yardstick.py, float64 numpy with nothing from the package; the derived tolerance
(one stage, n = non-zero taps of the phase + C) stands in that module's docstring."""
import math
import struct
import wave

import numpy as np
import pytest
import torch

import awm_amd
from awm_amd import inference, ops
from resample_yardstick import design, signal, yardstick
from yardstick_common import assert_within

RATES_TO_16K = [48000, 44100, 32000, 22050, 11025, 8000]
PAIRS = [(r, 16000) for r in RATES_TO_16K] + [(16000, 48000)]


def lengths(P):
    return [1, P - 1, 7 * P + 3, 20 * P + 5]


# ------------------------------------------------------------------------------------------ 1 / 2. against the yardstick, lengths
@pytest.mark.parametrize("kind", ["noise", "recording"])
@pytest.mark.parametrize("orig,new", PAIRS)
def test_resample_cpu_vs_float64(orig, new, kind):
    P = orig // math.gcd(orig, new)
    for k, N in enumerate(lengths(P) + [orig // 3 + 7]):
        for C in (1, 2):
            x = signal(kind, C, N, orig, seed=10 * k + C)
            y = awm_amd.resample(x, orig, new)
            ref, bound = yardstick(x.double().mean(dim=0).numpy(), orig, new, C)
            assert y.shape == (1, ref.shape[0]) and y.dtype == torch.float32
            assert_within(y.numpy(), ref, bound, f"{orig}->{new} {kind} N={N} C={C}")


@pytest.mark.parametrize("orig,new", PAIRS)
def test_output_length(orig, new):
    g = math.gcd(orig, new)
    P, Q = orig // g, new // g
    for N in lengths(P) + [P, 2 * P, 12345]:
        L = awm_amd.resample(torch.zeros(1, N), orig, new).shape[1]
        assert L == math.ceil(Q * N / P) == ops.resample_length(N, orig, new), (N, L)


def test_equal_rates_return_the_input():
    x = torch.randn(2, 100)
    assert awm_amd.resample(x, 16000, 16000) is x
    assert awm_amd.resample(x, 44100, 44100) is x
    assert awm_amd.Resample(16000, 16000)(x) is x


def test_rates_are_validated():
    x = torch.zeros(1, 10)
    for bad in (0, -16000, 44100.5, "48000", None):
        with pytest.raises(ValueError):
            awm_amd.resample(x, bad, 16000)
        with pytest.raises(ValueError):
            ops.resample_table(16000, bad)
    assert awm_amd.resample(x, 48000.0, 16000).shape == (1, 4)          # an integer-valued float is a rate


def test_resample_class_is_the_function():
    x = signal("noise", 2, 1000, 48000, seed=3)
    r = awm_amd.Resample(48000, 16000)
    assert torch.equal(r(x), awm_amd.resample(x, 48000, 16000))
    assert torch.equal(awm_amd.resample(x[0], 48000, 16000), awm_amd.resample(x[:1], 48000, 16000))     # (N,) is one channel


# ------------------------------------------------------------------------------------------ 3. properties
@pytest.mark.parametrize("orig,new", PAIRS)
def test_shift_by_one_period(orig, new):
    """x delayed by P samples -> y delayed by Q samples, away from the ends; conv1d fixes no order of additions, so within the bound"""
    P, Q, width, K, _ = design(orig, new)
    N = 40 * P + 11
    x = signal("noise", 1, N, orig, seed=21)
    xs = torch.cat([torch.zeros(1, P), x], dim=1)
    y, ysh = awm_amd.resample(x, orig, new)[0].numpy(), awm_amd.resample(xs, orig, new)[0].numpy()
    ref, bound = yardstick(x[0].double().numpy(), orig, new)
    edge = (math.ceil(width / P) + 1) * Q
    a, b = edge, y.shape[0] - edge
    assert b - a > 10 * Q
    assert_within(y[a:b], ref[a:b], bound[a:b], "unshifted")
    assert_within(ysh[a + Q:b + Q], ref[a:b], bound[a:b], "shifted")


@pytest.mark.parametrize("orig,new", PAIRS)
def test_mono_equals_two_identical_channels(orig, new):
    x = signal("recording", 1, 5000, orig, seed=4)
    assert torch.equal(awm_amd.resample(x, orig, new), awm_amd.resample(torch.cat([x, x], dim=0), orig, new))


@pytest.mark.parametrize("orig,new", PAIRS + [(16001, 16000), (44100, 48000)])
def test_compact_table_is_the_dense_one(orig, new):
    P, Q, width, K, h32 = design(orig, new)
    tab = ops.resample_table(orig, new)
    assert (tab["P"], tab["Q"], tab["width"], tab["K"]) == (P, Q, width, K)
    dense, taps, first, W = tab["dense"].numpy(), tab["taps"].numpy(), tab["first"].numpy(), tab["W"]
    assert dense.dtype == np.float32 and dense.shape == (Q, K) and taps.shape == (Q, W) and first.shape == (Q,)
    assert W <= 2 * width + 2 and first.min() >= 0 and (first + W).max() <= K
    expanded = np.zeros_like(dense)
    kept = np.zeros(dense.shape, dtype=bool)
    for i in range(Q):
        expanded[i, first[i]:first[i] + W] = taps[i]
        kept[i, first[i]:first[i] + W] = True
    assert np.array_equal(expanded, dense)
    assert np.all(dense[~kept] == 0.0)                               # every dropped tap is exactly 0.0
    nnz = (dense != 0).sum(axis=1)
    assert nnz.max() <= 2 * width + 1
    # the package's table against the formula evaluated here: two float64 evaluations of sin / cos may round a tap differently in
    # the last float32 bit, nothing more
    assert np.all(np.abs(dense.astype(np.float64) - h32) <= np.spacing(np.abs(h32))), "table differs from the published design"
    assert np.array_equal(dense != 0, h32 != 0)


def test_non_zero_taps_per_phase():
    """the counts the kernel's table is sized for: 37 for 48 k -> 16 k (K = 41), 33 or 34 for 44.1 k -> 16 k (K = 475)"""
    for (orig, K_want, counts) in ((48000, 41, {37}), (44100, 475, {33, 34})):
        P, Q, width, K, h32 = design(orig, 16000)
        assert K == K_want and set((h32 != 0).sum(axis=1).tolist()) <= counts


# ------------------------------------------------------------------------------------------ 4. a sinusoid stays that sinusoid
def test_1khz_sinusoid_48k_to_16k():
    P, Q, width, K, _ = design(48000, 16000)
    n48 = np.arange(48000)
    x = torch.from_numpy(np.sin(2 * np.pi * 1000.0 * n48 / 48000.0)).float()[None]
    y = awm_amd.resample(x, 48000, 16000)[0].double().numpy()
    ref, _ = yardstick(x[0].double().numpy(), 48000, 16000)
    ideal = np.sin(2 * np.pi * 1000.0 * np.arange(16000) / 16000.0)
    edge = math.ceil(width / P) * Q
    ripple = np.abs(ref - ideal)[edge:-edge].max()
    dev = np.abs(y - ideal)[edge:-edge].max()
    print(f"1 kHz: design deviation {ripple:.3e}, package deviation {dev:.3e}")
    # the design's own deviation at 1 kHz (gain of the 37-tap Hann-windowed sinc there), measured with the float64 yardstick: 3.99e-4
    assert 2e-4 < ripple < 8e-4
    assert dev <= 2 * ripple


# ------------------------------------------------------------------------------------------ 5. torchaudio, where it exists
@pytest.mark.parametrize("orig,new", PAIRS)
def test_parity_with_torchaudio(orig, new):
    """PARITY WITH TORCHAUDIO UNPINNED until a machine has it: skipped where torchaudio cannot be imported"""
    ta = pytest.importorskip("torchaudio")
    x = signal("recording", 1, orig // 2 + 3, orig, seed=8)
    want = ta.functional.resample(x, orig, new)
    got = awm_amd.resample(x, orig, new)
    assert got.shape == want.shape
    ref, bound = yardstick(x[0].double().numpy(), orig, new)
    assert_within(want.numpy(), ref, bound, "torchaudio vs float64")
    assert_within(got.numpy(), ref, bound, "package vs float64")


# ------------------------------------------------------------------------------------------ 6. load_audio without torchaudio
def _riff(path, fmt_body, payload):
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt_body) + 8 + len(payload)) + b"WAVE" + b"fmt " + struct.pack("<I", len(fmt_body)) +
                fmt_body + b"data" + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b""))


def _no_torchaudio():
    try:
        import torchaudio  # noqa: F401
    except ImportError:
        return True
    return False


@pytest.mark.skipif(not _no_torchaudio(), reason="load_audio uses torchaudio where it is installed")
def test_load_audio_resamples_without_torchaudio(tmp_path):
    rng = np.random.default_rng(5)
    # (a) two channels, 48 kHz, 16-bit PCM (written with the wave module)
    N = 48000 + 77
    pcm = rng.integers(-20000, 20000, size=(N, 2)).astype("<i2")
    pa = str(tmp_path / "a.wav")
    with wave.open(pa, "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(48000); w.writeframes(pcm.tobytes())
    data, rate = inference._read_wav(pa)
    assert rate == 48000 and np.array_equal(data, pcm.astype(np.float32) / 32768.0)
    ref, bound = yardstick((pcm.astype(np.float64) / 32768.0).mean(axis=1), 48000, 16000, C=2)
    got = awm_amd.load_audio(pa)
    assert got.shape == (1, ref.shape[0]) and got.dtype == torch.float32
    assert_within(got.numpy(), ref, bound, "48 kHz stereo PCM16")

    # (b) mono, 44.1 kHz, 24-bit PCM
    N = 44100 // 2 + 13
    v = rng.integers(-2 ** 23, 2 ** 23, size=N)
    v[:4] = (-2 ** 23, 2 ** 23 - 1, -1, 0)
    raw = b"".join(struct.pack("<i", int(s))[:3] for s in v)
    pb = str(tmp_path / "b.wav")
    with wave.open(pb, "wb") as w:
        w.setnchannels(1); w.setsampwidth(3); w.setframerate(44100); w.writeframes(raw)
    data, rate = inference._read_wav(pb)
    assert rate == 44100 and np.array_equal(data[:, 0], (v / 2.0 ** 23).astype(np.float32))
    ref, bound = yardstick(data[:, 0].astype(np.float64), 44100, 16000)
    assert_within(awm_amd.load_audio(pb).numpy(), ref, bound, "44.1 kHz PCM24")

    # (c) two channels, 48 kHz, WAVE_FORMAT_EXTENSIBLE with the IEEE-float sub-format
    N = 30000
    fl = (0.3 * rng.standard_normal((N, 2))).astype("<f4")
    guid_tail = bytes.fromhex("000000001000800000aa00389b71")
    fmt = struct.pack("<HHIIHH", 0xFFFE, 2, 48000, 48000 * 8, 8, 32) + struct.pack("<HHI", 22, 32, 3) + struct.pack("<H", 3) + guid_tail
    pc = str(tmp_path / "c.wav")
    _riff(pc, fmt, fl.tobytes())
    data, rate = inference._read_wav(pc)
    assert rate == 48000 and np.array_equal(data, fl)
    ref, bound = yardstick(fl.astype(np.float64).mean(axis=1), 48000, 16000, C=2)
    assert_within(awm_amd.load_audio(pc).numpy(), ref, bound, "48 kHz stereo float extensible")
    # ... and the PCM sub-format, 24 bits
    fmt = struct.pack("<HHIIHH", 0xFFFE, 1, 44100, 44100 * 3, 3, 24) + struct.pack("<HHI", 22, 24, 4) + struct.pack("<H", 1) + guid_tail
    pd = str(tmp_path / "d.wav")
    _riff(pd, fmt, raw)
    assert torch.equal(awm_amd.load_audio(pd), awm_amd.load_audio(pb))

    # (d) a 16 kHz file loads exactly as before: channel mean of the decoded samples, nothing else
    pcm16k = rng.integers(-20000, 20000, size=(20000, 2)).astype("<i2")
    pe = str(tmp_path / "e.wav")
    with wave.open(pe, "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm16k.tobytes())
    want = torch.from_numpy((pcm16k.astype(np.float32) / 32768.0).mean(axis=1).astype(np.float32)).unsqueeze(0)
    assert torch.equal(awm_amd.load_audio(pe), want)
    # another target rate: the file's rate is converted to it
    assert awm_amd.load_audio(pe, sample_rate=8000).shape == (1, 10000)


def test_orig_freq_none_needs_no_device():
    """the default of the new keyword leaves the host-side ingest as it was: the same segments, the same waveform object"""
    w = torch.randn(1, 40000)
    segs, rem, back = inference._ingest(w, None, "cpu")
    want, rem_want = inference._segments(w)
    assert torch.equal(segs, want) and rem == rem_want and back is w
    segs, rem, back = inference._ingest(w, 16000, "cpu")
    assert torch.equal(segs, want) and back is w
