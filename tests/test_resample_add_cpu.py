"""The way back of the embed path, on the host: `resample_add` (delta at the model rate -> the recording's rate, added to every channel) through
its CPU twin, and `read_audio`.

The yardstick is `yardstick()` of tests/resample_yardstick.py, float64 numpy with nothing from the package; the two derived bounds
(`up` against u64, `out[c]` through one more float32 add) stand in that module's docstring under "resample_add"."""
import math
import wave

import numpy as np
import pytest
import torch

import awm_amd
from awm_amd import ops
from resample_yardstick import signal, yardstick
from yardstick_common import assert_within

RATES = [48000, 44100, 22050, 11025, 8000, 16001]


def delta_for(n_d, seed, extra=0):
    return 0.01 * torch.randn(n_d + extra, generator=torch.Generator().manual_seed(seed))


def assert_sum_within(out, up, x, u64, bound, what):
    """the two bounds of the module docstring; out (C, N), up (1, N), x (C, N) tensors, u64 / bound (N,) float64"""
    assert tuple(up.shape) == (1, x.shape[1]) and tuple(out.shape) == tuple(x.shape)
    assert out.dtype == torch.float32 and up.dtype == torch.float32
    assert_within(up.numpy(), u64, bound, f"{what} up")
    for c in range(x.shape[0]):
        want = x[c].double().numpy() + u64
        assert_within(out[c].numpy(), want, bound + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64), f"{what} out[{c}]")


# ------------------------------------------------------------------------------------------ A1. the CPU twin against float64
@pytest.mark.parametrize("R", RATES)
def test_cpu_twin_vs_float64(R):
    for k, (C, N) in enumerate([(1, 1), (2, 2), (2, 7 * R // 100 + 3), (6, R + 4321)]):
        n_d = ops.resample_length(N, R, 16000)
        assert n_d == math.ceil(16000 * N / R)
        x = signal("recording", C, N, R, seed=10 * k + C)
        delta = delta_for(n_d, seed=R + k)
        out, up = awm_amd.resample_add(x, delta, R)
        u64, bound = yardstick(delta.double().numpy(), 16000, R, C=1)
        assert u64.shape[0] >= N
        assert_sum_within(out, up, x, u64[:N], bound[:N], f"16000->{R} C={C} N={N}")


# ------------------------------------------------------------------------------------------ A2. what lies behind n_d is not read
@pytest.mark.parametrize("R", [48000, 44100, 8000])
def test_tail_of_delta_is_ignored(R):
    C, N = 2, R // 10 + 7
    n_d = ops.resample_length(N, R, 16000)
    x = signal("recording", C, N, R, seed=5)
    delta = delta_for(n_d, seed=6, extra=500)
    delta[n_d:] = float("nan")
    out, up = awm_amd.resample_add(x, delta.view(1, 1, -1), R)                          # any shape: read flat
    assert not torch.isnan(out).any() and not torch.isnan(up).any()
    out_cut, up_cut = awm_amd.resample_add(x, delta[:n_d], R)
    assert torch.equal(up, up_cut) and torch.equal(out, out_cut)


# ------------------------------------------------------------------------------------------ A3. equal rates
@pytest.mark.parametrize("C", [1, 3])
def test_equal_rates_add_delta_itself(C):
    N = 1234
    x = signal("recording", C, N, 16000, seed=7)
    delta = delta_for(N, seed=8, extra=66)
    for rate in (16000, 44100):
        out, up = awm_amd.resample_add(x, delta, rate, rate)
        assert torch.equal(out, x + delta[:N]) and torch.equal(up, delta[:N].view(1, N))
        keep = delta.clone()
        up.add_(1.0)                                                                      # up is the caller's to write: never a view of delta
        assert torch.equal(delta, keep)
    out, up = awm_amd.resample_add(x[0], delta, 16000)                                    # (N,) is one channel
    assert torch.equal(out, x[:1] + delta[:N])


# ------------------------------------------------------------------------------------------ A4. arguments
def test_argument_errors():
    x = torch.zeros(2, 300)
    n_d = ops.resample_length(300, 48000, 16000)
    assert n_d == 100
    awm_amd.resample_add(x, torch.zeros(n_d), 48000)
    with pytest.raises(ValueError):
        awm_amd.resample_add(x, torch.zeros(n_d - 1), 48000)
    with pytest.raises(ValueError):
        awm_amd.resample_add(torch.zeros(1, 2, 300), torch.zeros(n_d), 48000)
    with pytest.raises(ValueError):
        awm_amd.resample_add(x, torch.zeros(n_d), 0)
    with pytest.raises(ValueError):
        awm_amd.resample_add(x, torch.zeros(n_d), 48000, 0)


# ------------------------------------------------------------------------------------------ A5. read_audio
def test_read_audio_keeps_channels_and_rate(tmp_path):
    rng = np.random.default_rng(3)
    N = 44100 // 5 + 9
    pcm = rng.integers(-30000, 30000, size=(N, 2)).astype("<i2")
    p = str(tmp_path / "stereo.wav")
    with wave.open(p, "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(44100); w.writeframes(pcm.tobytes())
    x, rate = awm_amd.read_audio(p)
    assert rate == 44100 and isinstance(rate, int)
    assert tuple(x.shape) == (2, N) and x.dtype == torch.float32
    assert np.array_equal(x.numpy(), pcm.T.astype(np.float32) / 32768.0)
